"""Note-level musical statistics of real and generated rolls -- the host side of `evaluate --music-metrics`.

The reference's instrument for "is the GAN actually learning different emotions" is src/gan/analyze_midi.py:28-54: note count,
mean pitch, pitch range, unique pitches, mean velocity and density of .mid files, one by one, comparing nothing.  Here the same
quantities, and the statistics set the music-generation literature compares between real and generated music (pitch and
pitch-class histograms, the pitch-class transition matrix, interval, duration and inter-onset histograms, each with a
divergence), come from the normalised (T, 4) rows themselves, per side and emotion.

The step from a row to notes is the generator's output contract, midi.notes_from_roll(roll, scale="chromatic", root_key=0)
(snapping is then the identity).  decode_rolls restates it vectorised in fp32, every operation rounded on its own, with the
Python constants entering as numpy 2.x makes them enter; csrc/note_metrics.hip (mg_note_stats) computes the same on the device
and host_stats is its reference.  This module imports no GPU code.
"""
from __future__ import annotations

import math

import numpy as np

SIDES = ("real", "fake")
NOTE_DIM = 4
PITCH_LO, PITCH_HI = 36, 96
ACC_FIELDS = (("counters", (8,)), ("pitch", (128,)), ("velocity", (128,)), ("dur16", (16,)), ("step16", (16,)),
              ("interval", (64,)), ("pctm", (12, 12)))      # one block per [side][true class]; ops.note_acc_layout
COUNTERS = ("rows", "events", "notes", "rests", "invalid", "overlaps", "transitions")
ROW_I = ("notes", "rests", "invalid", "unique_pitches", "lowest_pitch", "highest_pitch", "overlaps", "transitions")
ROW_BEATS = ("step_beats", "note_beats")
FEATURES = ("pitch", "pitch_class", "velocity", "duration", "step", "interval", "transitions")
TABLES = ("real_vs_generated", "generated_vs_generated", "real_vs_real")


def decode_rolls(x) -> dict:
    """(..., T, 4) fp32 rows -> the events of every time position, as arrays of shape (..., T): valid (all four values
    finite; an invalid position is absent from everything else), sounding (valid and not a rest), pitch, vel (int32; defined
    where sounding), dur, step (float64 beats; step where valid, dur where sounding)."""
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim < 2 or x.shape[-1] != NOTE_DIM:
        raise ValueError(f"decode_rolls: (..., T, {NOTE_DIM}) float32 rows expected, got {x.dtype} {x.shape}")
    f = np.float32
    x0, x1, x2, x3 = x[..., 0], x[..., 1], x[..., 2], x[..., 3]
    with np.errstate(all="ignore"):
        valid = np.isfinite(x).all(axis=-1)
        thr = f(-0.2)
        sounding = valid & ~(x1 < thr)
        pf = (x0 + f(1.0)) * f(63.5)
        pitch = np.where(sounding, np.clip(pf, f(PITCH_LO), f(PITCH_HI)), f(PITCH_LO)).astype(np.int32)
        vf = f(60.0) + ((x1 - thr) / f(1.2)) * f(67.0)
        vel = np.where(sounding, np.clip(vf, f(0.0), f(127.0)), f(0.0)).astype(np.int32)
        d = ((x2 + f(1.0)) / f(2.0)) * f(4.0)
        s = ((x3 + f(1.0)) / f(2.0)) * f(4.0)
        # max(0.25, d) / max(0.1, s) of the scalar code: the comparison is made in fp32, the constant stays a Python double
        dur = np.where(d > f(0.25), d.astype(np.float64), 0.25)
        step = np.where(s > f(0.1), s.astype(np.float64), 0.1)
    return {"valid": valid, "sounding": sounding, "pitch": pitch, "vel": vel, "dur": dur, "step": step}


def _bin16(beats):
    return np.minimum(15.0, np.floor(beats * 4.0)).astype(np.int64)


def acc_views(acc) -> dict:
    """A (2, K, 504) accumulator as named arrays (2, K, *shape)."""
    acc = np.asarray(acc)
    out, off = {}, 0
    for name, shape in ACC_FIELDS:
        n = math.prod(shape)
        out[name] = acc[:, :, off:off + n].reshape(acc.shape[0], acc.shape[1], *shape)
        off += n
    return out


def host_stats(real, fake, labels, K: int):
    """The kernel's reference in numpy: (acc (2, K, 504) int64, row_i (2, n, 8) int32, row_beats (2, n, 2) float64) of n rows
    real / fake (n, T, 4) fp32 with true classes `labels`; rows with a label outside [0, K) are padding and stay zero."""
    real, fake, labels = np.asarray(real), np.asarray(fake), np.asarray(labels).astype(np.int64)
    if real.shape != fake.shape or real.ndim != 3 or labels.shape != (real.shape[0],):
        raise ValueError("host_stats: real and fake (n, T, 4) and labels (n,) expected")
    n, T, _ = real.shape
    words = sum(math.prod(s) for _, s in ACC_FIELDS)
    acc = np.zeros((2, K, words), dtype=np.int64)
    row_i = np.zeros((2, n, 8), dtype=np.int32)
    row_beats = np.zeros((2, n, 2), dtype=np.float64)
    last = np.arange(T) < T - 1
    for s, x in enumerate((real, fake)):
        ev = decode_rolls(x)
        views = acc_views(acc[s:s + 1])
        for r in range(n):
            y = int(labels[r])
            if not 0 <= y < K:
                continue
            valid, snd = ev["valid"][r], ev["sounding"][r]
            pitch, vel, dur, step = ev["pitch"][r][snd], ev["vel"][r][snd], ev["dur"][r][snd], ev["step"][r]
            notes, events = int(snd.sum()), int(valid.sum())
            overlaps = int((snd & last & (ev["dur"][r] > step)).sum())
            trans = max(notes - 1, 0)
            cnt = views["counters"][0, y]
            cnt[:7] += (1, events, notes, events - notes, T - events, overlaps, trans)
            np.add.at(views["pitch"][0, y], pitch, 1)
            np.add.at(views["velocity"][0, y], vel, 1)
            np.add.at(views["dur16"][0, y], _bin16(dur), 1)
            np.add.at(views["step16"][0, y], _bin16(step[valid]), 1)
            if trans:
                a, b = pitch[:-1].astype(np.int64), pitch[1:].astype(np.int64)
                np.add.at(views["interval"][0, y], np.minimum(63, np.abs(b - a)), 1)
                np.add.at(views["pctm"][0, y], (a % 12, b % 12), 1)
            row_i[s, r] = (notes, events - notes, T - events, len(np.unique(pitch)), pitch.min() if notes else 0,
                           pitch.max() if notes else 0, overlaps, trans)
            row_beats[s, r] = (math.fsum(step[valid]), math.fsum(dur))
    return acc, row_i, row_beats


def js_divergence(p, q):
    """Jensen-Shannon divergence in base 2 of two histograms (any non-negative weights of one shape): 0 for identical
    distributions, 1 for disjoint ones; None when either holds no mass."""
    p, q = np.asarray(p, dtype=np.float64).ravel(), np.asarray(q, dtype=np.float64).ravel()
    if p.shape != q.shape:
        raise ValueError(f"js_divergence: histograms of {p.size} and {q.size} bins")
    sp, sq = float(p.sum()), float(q.sum())
    if not (sp > 0 and sq > 0):
        return None
    p, q = p / sp, q / sq
    m = 0.5 * (p + q)

    def kl(a):
        live = a > 0
        return float(np.sum(a[live] * np.log2(a[live] / m[live])))

    return min(1.0, max(0.0, 0.5 * kl(p) + 0.5 * kl(q)))


def _mean_std(v):
    v = np.asarray(v, dtype=np.float64)
    return (None, None) if v.size == 0 else (float(v.mean()), float(v.std()))


def _hist_mean_std(h):
    h = np.asarray(h, dtype=np.float64)
    n = float(h.sum())
    if n == 0:
        return None, None
    k = np.arange(h.size, dtype=np.float64)
    mean = float((h * k).sum()) / n
    return mean, math.sqrt(max(float((h * (k - mean) ** 2).sum()) / n, 0.0))


def _features(raw, s, k) -> dict:
    """The seven compared histograms of side s, class k."""
    pitch = np.asarray(raw["pitch"][s][k])
    return {"pitch": pitch, "pitch_class": np.bincount(np.arange(128) % 12, weights=pitch, minlength=12),
            "velocity": raw["velocity"][s][k], "duration": raw["dur16"][s][k], "step": raw["step16"][s][k],
            "interval": raw["interval"][s][k], "transitions": np.asarray(raw["pctm"][s][k]).ravel()}


def _side_stats(raw, rows, sel, s, k) -> dict:
    cnt = [int(v) for v in raw["counters"][s][k]]
    n_rows, events, notes, rests, invalid, overlaps, trans = cnt[:7]
    ri, rb = np.asarray(rows["row_i"])[s][sel], np.asarray(rows["row_beats"])[s][sel]
    with_note = ri[:, 0] > 0
    npr, upr = _mean_std(ri[:, 0]), _mean_std(ri[:, 3])
    rng = _mean_std((ri[:, 5] - ri[:, 4])[with_note])
    pm, vm = _hist_mean_std(raw["pitch"][s][k]), _hist_mean_std(raw["velocity"][s][k])
    beats = float(rb[:, 0].sum()) if len(rb) else 0.0
    pc = _features(raw, s, k)["pitch_class"]
    return {"rows": n_rows, "events": events, "notes": notes, "rests": rests, "invalid": invalid, "overlaps": overlaps,
            "transitions": trans,
            "notes_per_roll": {"mean": npr[0], "std": npr[1]},
            "rest_fraction": rests / events if events else None,
            "pitch": {"mean": pm[0], "std": pm[1]}, "velocity": {"mean": vm[0], "std": vm[1]},
            "unique_pitches_per_roll": {"mean": upr[0], "std": upr[1]},
            "pitch_range_per_roll": {"mean": rng[0], "std": rng[1], "rolls": int(with_note.sum())},
            "notes_per_beat": notes / beats if n_rows and beats > 0 else None,
            "overlap_fraction": overlaps / notes if notes else None,
            "pitch_class": [float(v) / notes for v in pc] if notes else None}


def music_block(raw, rows, labels, emotions) -> dict:
    """The report's `music` block.  raw: the accumulator by name (acc_views / ops.note_acc_views as numpy), each (2, K, ...);
    rows: {"row_i": (2, n, 8), "row_beats": (2, n, 2)} in split row order; labels: the n true classes; emotions: the K names.
    Plain Python values only; an empty set gives None (null)."""
    K = len(emotions)
    labels = np.asarray(labels).astype(np.int64)
    if np.asarray(raw["counters"]).shape[:2] != (2, K):
        raise ValueError(f"music_block: the accumulator is not (2, {K}, ...)")
    if np.asarray(rows["row_i"]).shape != (2, len(labels), 8) or np.asarray(rows["row_beats"]).shape != (2, len(labels), 2):
        raise ValueError("music_block: row_i (2, n, 8) and row_beats (2, n, 2) expected for n labels")
    block = {"emotions": list(emotions), "features": list(FEATURES)}
    for s, side in enumerate(SIDES):
        block[side] = {name: _side_stats(raw, rows, labels == k, s, k) for k, name in enumerate(emotions)}
    feats = [[_features(raw, s, k) for k in range(K)] for s in range(2)]
    block["js_real_vs_generated"] = {name: {f: js_divergence(feats[0][k][f], feats[1][k][f]) for f in FEATURES}
                                     for k, name in enumerate(emotions)}
    tables = {}
    for f in FEATURES:
        pairs = {"real_vs_generated": (0, 1), "generated_vs_generated": (1, 1), "real_vs_real": (0, 0)}
        tables[f] = {t: [[js_divergence(feats[a][i][f], feats[b][j][f]) for j in range(K)] for i in range(K)]
                     for t, (a, b) in pairs.items()}
    block["js_tables"] = tables
    return block


def format_block(block: dict) -> str:
    """The text table of a `music` block."""
    f = lambda v, spec: "-" if v is None else format(v, spec)  # noqa: E731
    lines = ["music (notes by the output contract; real | generated):",
             f"  {'emotion':<8} {'side':<5} {'rows':>6} {'notes/roll':>10} {'rest%':>6} {'pitch':>12} {'velocity':>12} "
             f"{'unique':>7} {'range':>7} {'notes/beat':>10} {'overlap%':>8}"]
    pct = lambda v: None if v is None else 100.0 * v  # noqa: E731
    for name in block["emotions"]:
        for side in SIDES:
            s = block[side][name]
            lines.append(
                f"  {name:<8} {side:<5} {s['rows']:>6} {f(s['notes_per_roll']['mean'], '.1f'):>10} "
                f"{f(pct(s['rest_fraction']), '.1f'):>6} "
                f"{f(s['pitch']['mean'], '.1f') + '+-' + f(s['pitch']['std'], '.1f'):>12} "
                f"{f(s['velocity']['mean'], '.1f') + '+-' + f(s['velocity']['std'], '.1f'):>12} "
                f"{f(s['unique_pitches_per_roll']['mean'], '.1f'):>7} {f(s['pitch_range_per_roll']['mean'], '.1f'):>7} "
                f"{f(s['notes_per_beat'], '.3f'):>10} {f(pct(s['overlap_fraction']), '.1f'):>8}")
    lines.append("  Jensen-Shannon divergence (base 2), real vs generated of one emotion:")
    lines.append(f"  {'emotion':<8} " + " ".join(f"{ft:>11}" for ft in block["features"]))
    for name in block["emotions"]:
        js = block["js_real_vs_generated"][name]
        lines.append(f"  {name:<8} " + " ".join(f"{f(js[ft], '.4f'):>11}" for ft in block["features"]))
    for t, title in (("real_vs_generated", "real emotion (rows) x generated emotion (columns)"),
                     ("generated_vs_generated", "generated x generated"), ("real_vs_real", "real x real")):
        lines.append(f"  pitch-class JS, {title}:")
        lines.append(f"  {'':<8} " + " ".join(f"{n:>8}" for n in block["emotions"]))
        for i, name in enumerate(block["emotions"]):
            lines.append(f"  {name:<8} " + " ".join(f"{f(v, '.4f'):>8}" for v in block["js_tables"]["pitch_class"][t][i]))
    return "\n".join(lines)
