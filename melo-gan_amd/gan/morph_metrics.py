"""The host side of gan/morph.py's report: the arithmetic from the device words of mg_path_probs / mg_path_d2 to the numbers in
morph.json, and host_path_stats, the numpy fp64 restatement of both reductions (the tests' reference).  numpy only: nothing
here imports torch or touches a GPU.

Rows are path-major: P paths of S1 = steps + 1 consecutive rows.  PathStats holds what the device leaves after the last
chunk:
    probs   (P, S1, K)      the classifier's softmax at every step of every path (None without a classifier)
    acc     (G, S1, K + 1)  per group: the sum of probs over the group's paths, and in word K their number
    feature (P, S1)         squared step lengths in the classifier's feature space; entry S1 - 1 = the squared distance between
                            the last step and step 0 (None unless the classifier reads notes)
    roll    (P, S1)         the same over the flattened rolls
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np


@dataclass
class PathStats:
    probs: Optional[np.ndarray]
    acc: Optional[np.ndarray]
    feature: Optional[np.ndarray]
    roll: Optional[np.ndarray]


def host_path_d2(x, P: int, S1: int) -> np.ndarray:
    """mg_path_d2 on the host: x (P * S1, D) -> (P, S1) fp64, every element widened before the subtraction."""
    x = np.asarray(x, np.float64).reshape(P, S1, -1)
    nxt = np.concatenate([x[:, 1:], x[:, :1]], axis=1)          # the step after s; after the last step, step 0
    return ((nxt - x) ** 2).sum(axis=2)


def host_path_probs(logits, group, S1: int, G: int):
    """mg_path_probs on the host: logits (P * S1, K) fp32, group (P,) -> probs (P * S1, K), acc (G, S1, K + 1), both fp64.  The
    softmax takes out the row maximum (the lowest index on ties) and does not compute its term; the others are added in class
    order.  A group's paths are added in path order."""
    z = np.asarray(logits, np.float32).astype(np.float64)
    rows, K = z.shape
    P = rows // S1
    probs = np.empty((rows, K), np.float64)
    for r in range(rows):
        pred = int(np.argmax(z[r]))
        e = np.exp(z[r] - z[r, pred])
        rest = 0.0
        for k in range(K):
            if k != pred:
                rest += e[k]
        s = 1.0 + rest
        probs[r] = e / s
        probs[r, pred] = 1.0 / s
    acc = np.zeros((G, S1, K + 1), np.float64)
    p3 = probs.reshape(P, S1, K)
    for p, g in enumerate(np.asarray(group).tolist()):
        if 0 <= g < G:
            acc[g, :, :K] += p3[p]
            acc[g, :, K] += 1.0
    return probs, acc


def host_path_stats(logits, group, S1: int, G: int, features=None, rolls=None) -> PathStats:
    """Both reductions restated in numpy fp64 over the stashed logits (None: no classifier), features (None: none) and rolls."""
    probs = acc = None
    if logits is not None:
        probs, acc = host_path_probs(logits, group, S1, G)
        probs = probs.reshape(-1, S1, probs.shape[1])
    P = len(np.asarray(group))
    return PathStats(probs, acc,
                     None if features is None else host_path_d2(np.asarray(features).reshape(P * S1, -1), P, S1),
                     None if rolls is None else host_path_d2(np.asarray(rolls).reshape(P * S1, -1), P, S1))


def crossover(w: Sequence[float], p_from: Sequence[float], p_to: Sequence[float]) -> Optional[float]:
    """Where the curve p_to reaches p_from, in units of w: the first step s with p_to >= p_from, placed between s - 1 and s by
    linear interpolation of the difference; 0.0 when s = 0, None when the curves never cross."""
    d = [float(b) - float(a) for a, b in zip(p_from, p_to)]
    for s, ds in enumerate(d):
        if ds >= 0.0:
            if s == 0:
                return 0.0
            return float(w[s - 1] + (w[s] - w[s - 1]) * (-d[s - 1] / (ds - d[s - 1])))
    return None


def curve_block(probs: np.ndarray, acc: np.ndarray, w: Sequence[float], i_from: int, i_to: int) -> dict:
    """The classifier's part of a pair's report.  probs (n, S1, K): the pair's paths; acc (S1, K + 1): the pair's sums."""
    K = probs.shape[2]
    p_mean = acc[:, :K] / acc[:, K:]
    pred = np.argmax(probs, axis=2)             # the first index of the maximum
    p_to = probs[:, :, i_to]
    monotone = np.all(p_to[:, 1:] >= p_to[:, :-1], axis=1)
    switch = (pred[:, 0] == i_from) & (pred[:, -1] == i_to)
    return {"p_mean": [[float(v) for v in row] for row in p_mean],
            "crossover": crossover(w, p_mean[:, i_from], p_mean[:, i_to]),
            "monotone_fraction": float(np.mean(monotone)),
            "switch_fraction": float(np.mean(switch))}


def distance_block(d2: np.ndarray, steps: int) -> dict:
    """A pair's report in one space from its paths' squared step lengths d2 (n, steps + 1): path_length = the mean over paths of
    sum_s sqrt(d2), endpoint_distance = the mean of sqrt(d2[:, steps]), straightness = endpoint distance over path length,
    averaged over the paths of positive length (None when there is none), ppl = the mean over paths and steps of
    d2 * steps^2 -- the squared step over the squared parameter step 1 / steps."""
    d2 = np.asarray(d2, np.float64)
    step = np.sqrt(d2[:, :steps])
    length = step.sum(axis=1)
    end = np.sqrt(d2[:, steps])
    pos = length > 0.0
    return {"path_length": float(length.mean()),
            "endpoint_distance": float(end.mean()),
            "straightness": float(np.mean(end[pos] / length[pos])) if pos.any() else None,
            "ppl": float(np.mean(d2[:, :steps] * float(steps) ** 2))}


def pair_report(stats: PathStats, g: int, paths: Sequence[int], w: Sequence[float], i_from: int, i_to: int) -> dict:
    """The block of pair g in morph.json: its paths are rows `paths` of the stats; w the step weights."""
    steps = len(w) - 1
    idx = np.asarray(list(paths), np.int64)
    out = {"w": [float(v) for v in w]}
    if stats.probs is not None:
        out.update(curve_block(stats.probs[idx], stats.acc[g], w, i_from, i_to))
    else:
        out.update({"p_mean": None, "crossover": None, "monotone_fraction": None, "switch_fraction": None})
    out["feature"] = None if stats.feature is None else distance_block(stats.feature[idx], steps)
    out["roll"] = distance_block(stats.roll[idx], steps)
    return out


def blend_report(stats: PathStats) -> dict:
    """--weights: one point, no path.  The mean probabilities over its samples."""
    if stats.probs is None:
        return {"p_mean": None}
    K = stats.probs.shape[2]
    return {"p_mean": [float(v) for v in stats.acc[0, 0, :K] / stats.acc[0, 0, K]]}


def join_offsets(rolls: Sequence[np.ndarray], bpms: Sequence[float], join_notes: int) -> List[float]:
    """--join: where each step's notes begin in the joined piece, in seconds.  A step lasts the sum over its first join_notes
    rows, in row order, of max(0.1, ((step + 1) / 2) * 4) * 60 / bpm (midi.notes_from_roll's step in beats at the step's
    tempo), in Python floats; a step begins where the one before it ends."""
    out, end = [], 0.0
    for roll, bpm in zip(rolls, bpms):
        out.append(end)
        for row in np.asarray(roll)[:join_notes]:
            end += max(0.1, ((float(row[3]) + 1.0) / 2.0) * 4.0) * 60.0 / bpm
    return out
