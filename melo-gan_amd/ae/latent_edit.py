"""The host side of ae/edit.py: the row descriptors of an edit, the class means of a split's latents, the numpy fp64
restatements of mg_latent_rows and mg_latent_cycle (the tests' reference) and the arithmetic from the device words to the numbers
in edit.json.  numpy only: nothing here imports torch or touches a GPU.

An output row is `kind` (0 padding, 1 prior, 2 posterior), two sources a, b and t between them, a direction dir (< 0: none) with
its coefficient alpha, a noise scale sigma and the key (piece, sample) of its normals (include/melo_gan_hip.h, mg_latent_rows):
    z = base + alpha * dirs[dir] + sigma * s * n
Sources are named by their row in the split; Rows.sources lists the rows that have to be encoded and src_a / src_b index into
that list.  A variation k of piece p has the key (p, k) whatever else a run asks for; prior sample k has the key (-1, k).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

KIND_PAD, KIND_PRIOR, KIND_POST = 0, 1, 2
INTERP = ("lerp", "slerp")
PRIOR_PIECE = -1
MAX_L = 1024
CYCLE_WORDS = ("z_src_d2", "mu2_z_d2", "mu2_src_d2", "mu2_dot_d", "z_dot_d", "d_dot_d")
MODES = ("prior", "vary", "path", "shift")


class LatentEditError(ValueError):
    """A bad request, found on the host before any GPU use."""


@dataclass
class Rows:
    """The row descriptors of one run, in output order.  group[r]: what the rows of one request share (the piece of a variation,
    the path, the source of a shift); source_label / target (shift): the classes the direction runs between."""
    mode: str
    kind: np.ndarray            # (R,) int32
    src_a: np.ndarray           # (R,) int32, into `sources`
    src_b: np.ndarray
    t: np.ndarray               # (R,) float32
    dir: np.ndarray             # (R,) int32
    alpha: np.ndarray           # (R,) float32
    sigma: np.ndarray           # (R,) float32
    key: np.ndarray             # (R, 2) int32: (piece, sample)
    sources: List[int] = field(default_factory=list)     # split rows, ascending
    interp: int = 0
    group: Optional[np.ndarray] = None
    source_label: Optional[np.ndarray] = None             # (R,) int32, -1: none
    target: Optional[np.ndarray] = None                   # (R,) int32, -1: none
    n_classes: int = 0

    @property
    def R(self) -> int:
        return len(self.kind)

    def describe(self, r: int) -> dict:
        """Row r's descriptors as plain Python values, sources as split rows."""
        k = int(self.kind[r])
        out = {"row": int(r), "kind": ("padding", "prior", "posterior")[k], "key": [int(self.key[r, 0]), int(self.key[r, 1])],
               "sigma": float(self.sigma[r])}
        if k == KIND_POST:
            out.update(source=self.sources[int(self.src_a[r])], source_b=self.sources[int(self.src_b[r])], t=float(self.t[r]))
        if int(self.dir[r]) >= 0:
            out.update(direction=int(self.dir[r]), alpha=float(self.alpha[r]))
        if self.target is not None and int(self.target[r]) >= 0:
            out.update(source_label=int(self.source_label[r]), target=int(self.target[r]))
        return out


def _new(mode: str, R: int, sources: Sequence[int], interp: int = 0) -> Rows:
    z = lambda dt: np.zeros(R, dt)  # noqa: E731
    return Rows(mode, z(np.int32), z(np.int32), z(np.int32), z(np.float32), np.full(R, -1, np.int32), z(np.float32), z(np.float32),
                np.zeros((R, 2), np.int32), list(sources), interp, z(np.int32), np.full(R, -1, np.int32), np.full(R, -1, np.int32))


def _count(v, name: str, lo: int = 1) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < lo:
        raise LatentEditError(f"{name} = {v!r}: an integer >= {lo} expected")
    return int(v)


def _finite(v, name: str, lo: Optional[float] = None) -> float:
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise LatentEditError(f"{name} = {v!r}: a number expected") from None
    if not math.isfinite(f) or (lo is not None and f < lo):
        raise LatentEditError(f"{name} = {v!r}: a finite number" + (f" >= {lo}" if lo is not None else "") + " expected")
    return f


def check_pieces(rows: Sequence[int], n_split: Optional[int], name: str) -> List[int]:
    """Row indices of a split of n_split rows (None: unknown), at least one."""
    out = []
    for r in rows:
        if isinstance(r, bool) or not isinstance(r, (int, np.integer)):
            raise LatentEditError(f"{name}: {r!r} is not a row index")
        if int(r) < 0 or (n_split is not None and int(r) >= n_split):
            raise LatentEditError(f"{name}: row {int(r)} lies outside the split" + (f" of {n_split} rows" if n_split is not None else ""))
        out.append(int(r))
    if not out:
        raise LatentEditError(f"{name}: at least one row is needed")
    return out


def prior_rows(n: int, temperature: float = 1.0) -> Rows:
    """n samples of the prior: z = temperature * N(0, I) under the keys (-1, 1) .. (-1, n)."""
    n, temp = _count(n, "prior samples"), _finite(temperature, "temperature", 0.0)
    rows = _new("prior", n, [])
    rows.kind[:] = KIND_PRIOR
    rows.sigma[:] = temp
    rows.key[:, 0], rows.key[:, 1] = PRIOR_PIECE, np.arange(1, n + 1)
    rows.group[:] = np.arange(n)
    return rows


def vary_rows(pieces: Sequence[int], samples: int, sigma: float = 1.0, n_split: Optional[int] = None) -> Rows:
    """`samples` draws of every piece's posterior, piece-major: z = mu + sigma * exp(logvar / 2) * N(0, I) under the key
    (piece, k), k = 1 .. samples."""
    pieces, samples, sg = check_pieces(pieces, n_split, "vary"), _count(samples, "samples"), _finite(sigma, "sigma", 0.0)
    sources = sorted(set(pieces))
    rows = _new("vary", len(pieces) * samples, sources)
    for i, p in enumerate(pieces):
        for k in range(samples):
            r = i * samples + k
            rows.kind[r], rows.src_a[r], rows.src_b[r] = KIND_POST, sources.index(p), sources.index(p)
            rows.sigma[r], rows.key[r], rows.group[r] = sg, (p, k + 1), i
    return rows


def path_rows(a: int, b: int, steps: int = 8, interp: str = "lerp", n_split: Optional[int] = None) -> Rows:
    """The path from piece a to piece b in `steps` equal steps (steps + 1 rows): t = s / steps, no noise, no direction.  Step 0 is
    mu[a] and the last step mu[b] bit for bit."""
    a, b = check_pieces([a, b], n_split, "path")
    steps = _count(steps, "steps")
    if interp not in INTERP:
        raise LatentEditError(f"interp = {interp!r}: expected one of {', '.join(INTERP)}")
    sources = sorted({a, b})
    rows = _new("path", steps + 1, sources, INTERP.index(interp))
    rows.kind[:] = KIND_POST
    rows.src_a[:], rows.src_b[:] = sources.index(a), sources.index(b)
    rows.t[:] = np.arange(steps + 1, dtype=np.float64) / steps
    rows.t[steps] = 1.0
    rows.key[:, 0], rows.key[:, 1] = a, np.arange(steps + 1)
    return rows


def shift_rows(pieces: Sequence[int], labels: Sequence[int], target: int, strengths: Sequence[float], n_classes: int,
               n_split: Optional[int] = None) -> Rows:
    """Every piece moved along (class mean of `target`) - (class mean of its own label) by each strength, piece-major:
    z = mu + strength * dirs[label * n_classes + target], the row of centroids()'s difference table."""
    pieces, K = check_pieces(pieces, n_split, "shift"), _count(n_classes, "n_classes", 2)
    labels = [int(v) for v in labels]
    if len(labels) != len(pieces):
        raise LatentEditError(f"shift: {len(pieces)} rows but {len(labels)} labels")
    if isinstance(target, bool) or not isinstance(target, (int, np.integer)) or not 0 <= int(target) < K:
        raise LatentEditError(f"shift: target {target!r} lies outside the {K} classes")
    if any(not 0 <= v < K for v in labels):
        raise LatentEditError(f"shift: a source label lies outside the {K} classes")
    st = [_finite(s, "strength") for s in strengths]
    if not st:
        raise LatentEditError("shift: at least one strength is needed")
    sources = sorted(set(pieces))
    rows = _new("shift", len(pieces) * len(st), sources)
    rows.n_classes = K
    for i, (p, y) in enumerate(zip(pieces, labels)):
        for j, s in enumerate(st):
            r = i * len(st) + j
            rows.kind[r], rows.src_a[r], rows.src_b[r] = KIND_POST, sources.index(p), sources.index(p)
            rows.dir[r], rows.alpha[r], rows.key[r], rows.group[r] = y * K + int(target), s, (p, j), i
            rows.source_label[r], rows.target[r] = y, int(target)
    return rows


def centroids(acc_views: dict, need: Optional[Sequence[int]] = None):
    """Class means of mu from VaeEvaluator's accumulator (acc_host: 'c' (K, 16) with the rows of a class in c[k, 0], 'lat'
    (K, 5, L) with the sum of mu in lat[k, 0]): returns (means (K, L) fp64, counts (K,) int64, diff (K, K, L) fp64 with
    diff[i, j] = means[j] - means[i]).  A class without rows has no mean: NaN in `means` and `diff`, and an error when it is among
    `need` (default: every class)."""
    c, lat = np.asarray(acc_views["c"]), np.asarray(acc_views["lat"], np.float64)
    if c.ndim != 2 or lat.ndim != 3 or lat.shape[0] != c.shape[0] or lat.shape[1] < 1:
        raise LatentEditError(f"centroids: 'c' (K, 16) and 'lat' (K, 5, L) expected, got {c.shape} and {lat.shape}")
    K = c.shape[0]
    counts = c[:, 0].astype(np.int64)
    for k in (range(K) if need is None else need):
        if not 0 <= int(k) < K or counts[int(k)] < 1:
            raise LatentEditError(f"centroids: class {int(k)} has no rows in this split: it has no mean")
    means = np.full((K, lat.shape[2]), np.nan)
    live = counts > 0
    means[live] = lat[live, 0] / counts[live, None].astype(np.float64)
    return means, counts, means[None, :, :] - means[:, None, :]


def _lane_sums(*terms):
    """Sums as a 64-lane workgroup takes them over element blocks of four: lane u adds the blocks q = u, u + 64, .. (elements
    4q .. 4q + 3) in element order, then a butterfly over the lanes.  terms: equally long fp64 vectors; returns one sum each."""
    out = []
    for v in terms:
        lanes = np.zeros(64, np.float64)
        for q in range((len(v) + 3) // 4):
            for e in v[4 * q:4 * q + 4]:
                lanes[q % 64] = lanes[q % 64] + e
        out.append(_butterfly(lanes))
    return out


def _butterfly(lanes: np.ndarray) -> float:
    idx = np.arange(64)
    m = 1
    while m < 64:
        lanes = lanes + lanes[idx ^ m]
        m <<= 1
    return float(lanes[0])


def slerp_coefficients(x, y, t: float):
    """mg_latent_rows' (ca, cb) for the fp32 vectors x, y at t, in fp64: the chord's (1 - t, t) when sin(theta) < 2^-20 or not a
    number."""
    x, y, t = np.asarray(x, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64), float(t)
    dot, na, nb = _lane_sums(x * y, x * x, y * y)
    with np.errstate(all="ignore"):
        q = np.float64(dot) / (np.sqrt(np.float64(na)) * np.sqrt(np.float64(nb)))
        theta = math.acos(float(np.fmin(np.fmax(q, -1.0), 1.0)))        # fmax / fmin drop a NaN quotient: theta = pi
    s = math.sin(theta)
    if s >= 2.0 ** -20:
        return math.sin((1.0 - t) * theta) / s, math.sin(t * theta) / s
    return 1.0 - t, t


def host_latent_rows(mu, logvar, dirs, rows: Rows, normals, parts: bool = False):
    """mg_latent_rows on the host with the normals injected: mu, logvar (n_src, L), dirs (n_dir, L) or None, normals (R, L) (row
    r's N(0,1) draws; read only where sigma != 0).  Everything in fp64 from the fp32 inputs, one rounding at the end.  Returns z
    (R, L) float32; with parts=True also the three fp64 terms (base, alpha * d, sigma * s * n), each (R, L)."""
    f64 = lambda v: None if v is None else np.asarray(v, np.float32).astype(np.float64)  # noqa: E731
    mu, logvar, dirs, normals = f64(mu), f64(logvar), f64(dirs), f64(normals)
    R = rows.R
    Ld = normals.shape[1]
    base, move, noise = (np.zeros((R, Ld), np.float64) for _ in range(3))
    z = np.zeros((R, Ld), np.float32)
    for r in range(R):
        kind = int(rows.kind[r])
        if kind == KIND_PAD:
            continue
        s = np.ones(Ld, np.float64)
        if kind == KIND_POST:
            a, b, t = int(rows.src_a[r]), int(rows.src_b[r]), np.float32(rows.t[r])
            if t == 0 or a == b:
                base[r] = mu[a]
            elif t == 1:
                base[r] = mu[b]
            else:
                ca, cb = (1.0 - float(t), float(t)) if rows.interp == 0 else slerp_coefficients(mu[a], mu[b], float(t))
                base[r] = ca * mu[a] + cb * mu[b]
            if rows.sigma[r] != 0:
                s = np.exp(0.5 * logvar[a])
        v = base[r].copy()
        if int(rows.dir[r]) >= 0 and rows.alpha[r] != 0:
            move[r] = float(rows.alpha[r]) * dirs[int(rows.dir[r])]
            v = v + move[r]
        if rows.sigma[r] != 0:
            noise[r] = (float(rows.sigma[r]) * s) * normals[r]
            v = v + noise[r]
        z[r] = v.astype(np.float32)
    return (z, base, move, noise) if parts else z


def host_latent_cycle(z, mu2, mu, dirs, kind, src_a, dir) -> np.ndarray:
    """mg_latent_cycle on the host, with the kernel's addition order: every element widened before the subtraction, lane u of 64
    adds the elements u, u + 64, .. in that order, then a butterfly over the lanes.  Returns (R, 6) fp64 (CYCLE_WORDS)."""
    f64 = lambda v: None if v is None else np.asarray(v, np.float32).astype(np.float64)  # noqa: E731
    z, mu2, mu, dirs = f64(z), f64(mu2), f64(mu), f64(dirs)
    R, Ld = z.shape
    out = np.zeros((R, 6), np.float64)
    for r in range(R):
        k = int(kind[r])
        if k == KIND_PAD:
            continue
        m = mu[int(src_a[r])] if k == KIND_POST else np.zeros(Ld, np.float64)
        e0, e1, e2 = z[r] - m, mu2[r] - z[r], mu2[r] - m
        terms = [e0 * e0, e1 * e1, e2 * e2]
        if int(dir[r]) >= 0:
            d = dirs[int(dir[r])]
            terms += [e2 * d, e0 * d, d * d]
        for w, v in enumerate(terms):
            lanes = np.zeros(64, np.float64)
            for i0 in range(0, Ld, 64):
                n = min(64, Ld - i0)
                lanes[:n] = lanes[:n] + v[i0:i0 + n]
            out[r, w] = _butterfly(lanes)
    return out


def note_change(before, after) -> List[dict]:
    """Note-level change of each roll in `after` against the roll in `before` at the same position ((R, T, 4) float32 both),
    through gan.music_metrics.decode_rolls: the share of time positions whose sounding / rest state differs, and over the
    positions that sound in both the share whose pitch differs and the mean |pitch difference| (None when there is none)."""
    from ..gan.music_metrics import decode_rolls
    b, a = decode_rolls(np.asarray(before, np.float32)), decode_rolls(np.asarray(after, np.float32))
    out = []
    for r in range(len(b["valid"])):
        both = b["sounding"][r] & a["sounding"][r]
        n = int(both.sum())
        dp = np.abs(a["pitch"][r][both].astype(np.int64) - b["pitch"][r][both].astype(np.int64))
        out.append({"onset_changed": float(np.mean(b["sounding"][r] != a["sounding"][r])),
                    "pitch_changed": float(np.mean(dp > 0)) if n else None,
                    "mean_abs_pitch_change": float(np.mean(dp)) if n else None,
                    "notes_before": int(b["sounding"][r].sum()), "notes_after": int(a["sounding"][r].sum())})
    return out


def _ratio(num: float, den: float) -> Optional[float]:
    if den == 0.0 or not math.isfinite(num) or not math.isfinite(den):
        return None
    return float(num) / float(den)


def _root(v: float) -> Optional[float]:
    return math.sqrt(v) if math.isfinite(v) and v >= 0.0 else None


def _mean(vals) -> Optional[float]:
    vals = [float(v) for v in vals if v is not None]
    return sum(vals) / len(vals) if vals else None


def report(rows: Rows, cycle, notes: Optional[Sequence[Optional[dict]]] = None, scores: Optional[dict] = None,
           names: Optional[Sequence[str]] = None) -> dict:
    """edit.json's `rows` and `summary`.  cycle (R, 6): mg_latent_cycle's words.  notes: per row note_change's block or None (a
    prior row has no source).  scores: the classifier's {"before", "after", "cycled"} -> {"pred" (R,) int, -1: not scored,
    "p_target", "p_source" (R,): mg_emotion_score's probability of the row's target and of its source label}.  Plain Python
    values throughout; None where a denominator is zero, never NaN."""
    cycle = np.asarray(cycle, np.float64)
    if cycle.shape != (rows.R, 6):
        raise LatentEditError(f"report: cycle words of shape ({rows.R}, 6) expected, got {cycle.shape}")
    name = lambda k: (names[k] if names is not None and 0 <= k < len(names) else int(k))  # noqa: E731
    out_rows = []
    for r in range(rows.R):
        c = [float(v) for v in cycle[r]]
        row = rows.describe(r)
        if "target" in row:
            row["source_label"], row["target"] = name(row["source_label"]), name(row["target"])
        row["latent_step"], row["cycle_error"] = _root(c[0]), _root(c[1])
        if int(rows.dir[r]) >= 0:
            row["requested"], row["realised"] = _ratio(c[4], c[5]), _ratio(c[3], c[5])
        if notes is not None:
            row["notes"] = notes[r]
        if scores is not None:
            tgt = int(rows.target[r]) if rows.target is not None else -1
            src = int(rows.source_label[r]) if rows.source_label is not None else -1
            for when in ("before", "after", "cycled"):
                s = scores.get(when)
                if s is None or int(s["pred"][r]) < 0:
                    continue
                blk = {"prediction": name(int(s["pred"][r]))}
                if tgt >= 0 and src >= 0:
                    pt, ps = float(s["p_target"][r]), float(s["p_source"][r])
                    blk.update(p_target=pt if math.isfinite(pt) else None, p_source=ps if math.isfinite(ps) else None)
                row[when] = blk
        out_rows.append(row)
    summary = {"rows": rows.R, "latent_step": _mean(r["latent_step"] for r in out_rows),
               "cycle_error": _mean(r["cycle_error"] for r in out_rows)}
    if notes is not None:
        for k in ("onset_changed", "pitch_changed", "mean_abs_pitch_change"):
            summary[k] = _mean(r["notes"][k] for r in out_rows if r.get("notes") is not None)
    if rows.mode == "shift":
        by_strength = []
        for s in sorted({float(a) for a in rows.alpha}):
            sel = [r for r in out_rows if r.get("alpha") == s]
            blk = {"strength": s, "rows": len(sel), "requested": _mean(r["requested"] for r in sel),
                   "realised": _mean(r["realised"] for r in sel)}
            if scores is not None:
                scored = [r for r in sel if "after" in r]
                blk["became_target"] = _mean(float(r["after"]["prediction"] == r["target"]) for r in scored)
                blk["p_target_before"] = _mean(r["before"]["p_target"] for r in scored if "before" in r)
                blk["p_target_after"] = _mean(r["after"]["p_target"] for r in scored)
            by_strength.append(blk)
        summary["requested"] = _mean(r["requested"] for r in out_rows)
        summary["realised"] = _mean(r["realised"] for r in out_rows)
        summary["per_strength"] = by_strength
    return {"mode": rows.mode, "interp": INTERP[rows.interp], "sources": [int(s) for s in rows.sources], "rows": out_rows,
            "summary": summary}
