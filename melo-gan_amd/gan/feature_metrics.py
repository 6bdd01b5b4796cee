"""Feature-space metrics of the held-out evaluation (evaluate.py --feature-metrics): the host arithmetic behind the report's
"feature_space" block.  The device hands over kernel sums, k-NN margins and nearest-neighbour distances (ops.pair_ksum /
pair_knn / pair_margin over the classifier's encoder features); everything here is plain Python over those numbers and needs
no GPU.

  KID        Binkowski et al., "Demystifying MMD GANs" (ICLR 2018): the unbiased MMD^2 under k(x, y) = (x . y / D + 1)^3.
             Unbiased: it is about 0, and may be slightly negative, when the two sets come from one distribution.
  precision  Kynkaanniemi et al., "Improved Precision and Recall Metric for Assessing Generative Models" (NeurIPS 2019): the
  / recall   share of generated rows inside the real set's k-NN manifold (the union of the balls around every real row that
             reach its k-th neighbour), and of real rows inside the generated set's.  Mode collapse shows as low recall.
  nn_train   squared distance of every generated / validation row to its nearest training row: a generator that replays its
             training set sits far closer to it than held-out real data does.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np


def kid_from_sums(kxx: float, m: int, kyy: float, n: int, kxy: float) -> Optional[float]:
    """The unbiased MMD^2 from the three kernel sums: kxx / kyy over the ordered pairs i != j of the m real / n generated rows,
    kxy over all m n pairs.  None when either set has fewer than two rows."""
    m, n = int(m), int(n)
    if m < 2 or n < 2:
        return None
    return float(kxx) / (m * (m - 1)) + float(kyy) / (n * (n - 1)) - 2.0 * float(kxy) / (m * n)


def _share_inside(margin) -> Optional[float]:
    if margin is None:
        return None
    margin = np.asarray(margin)
    if margin.size == 0:
        return None
    return float(np.count_nonzero(margin <= 0)) / margin.size


def precision_recall(margin_fake_in_real, margin_real_in_fake):
    """(precision, recall): the shares of entries <= 0 of the two margin arrays (ops.pair_margin); None for a side that has no
    manifold (None or empty)."""
    return _share_inside(margin_fake_in_real), _share_inside(margin_real_in_fake)


def _quantiles(d2) -> Optional[dict]:
    d2 = np.asarray(d2, dtype=np.float64)
    if d2.size == 0:
        return None
    return {"median": float(np.median(d2)), "p05": float(np.quantile(d2, 0.05))}


def nn_summary(fake_d2, real_d2) -> dict:
    """The nearest-training-row check from the squared distances of the generated and of the validation rows to their nearest
    training row: median and 5th percentile of each, and the share of generated rows at least as close to the training set
    as the closest 5 % of the validation rows are (about 0.05 for a generator that does not memorise, 1.0 for a replay)."""
    fake, real = _quantiles(fake_d2), _quantiles(real_d2)
    share = None
    if fake is not None and real is not None:
        share = float(np.count_nonzero(np.asarray(fake_d2, dtype=np.float64) <= real["p05"])) / np.asarray(fake_d2).size
    return {"fake": fake, "real": real, "fake_below_real_p05": share}


def feature_block(dim: int, k: int, emotions: Sequence[str], counts: Sequence[int], sums: dict, margins: dict) -> dict:
    """The report's "feature_space" block.
    counts[e]: rows of emotion e.
    sums:      {"xx", "yy", "xy"}: the whole sets' kernel sums (real-real and fake-fake without the diagonal, real-fake);
               {"xx_e"[e], "yy_e"[e], "xy_ef"[e][f]}: the same per emotion slice (entries of sets too small are ignored).
    margins:   {"fake_in_real", "real_in_fake"}: the whole sets' margins or None; {"fake_in_real_e"[e], "real_in_fake_e"[e]}.
    Entries whose sets are too small are None: fewer than 2 rows for KID, at most k rows for a manifold."""
    counts = [int(c) for c in counts]
    n = sum(counts)
    K = len(emotions)
    precision, recall = precision_recall(margins["fake_in_real"], margins["real_in_fake"]) if n > k else (None, None)
    matrix = [[kid_from_sums(sums["xx_e"][e], counts[e], sums["yy_e"][f], counts[f], sums["xy_ef"][e][f]) for f in range(K)]
              for e in range(K)]
    per = {}
    for e, name in enumerate(emotions):
        pe, re_ = (precision_recall(margins["fake_in_real_e"][e], margins["real_in_fake_e"][e]) if counts[e] > k
                   else (None, None))
        per[name] = {"n": counts[e], "kid": matrix[e][e], "precision": pe, "recall": re_}
    return {"dim": int(dim), "k": int(k), "kid": kid_from_sums(sums["xx"], n, sums["yy"], n, sums["xy"]),
            "precision": precision, "recall": recall, "per_emotion": per,
            "kid_matrix": {emotions[e]: {emotions[f]: matrix[e][f] for f in range(K)} for e in range(K)}}


# ---------------------------------------------------------------------------------------------------------------------
# Frechet distance and covariance spectra (evaluate.py --frechet; csrc/frechet.hip)
# ---------------------------------------------------------------------------------------------------------------------
EIG_MAX_SWEEPS = 30
EIG_EPS = 2.0 ** -53
SPECTRUM_KEYS = ("participation_ratio", "effective_rank", "top1_share")


def host_moments(X):
    """(mean (D), unbiased covariance (D, D)) of the rows of X in fp64, as mg_feat_moments: the mean first, then the centred
    rows' outer products over n - 1."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 2:
        raise ValueError(f"host_moments: (n >= 2, D) rows expected, got {X.shape}")
    mean = X.sum(0) / X.shape[0]
    Xc = X - mean
    return mean, (Xc.T @ Xc) / (X.shape[0] - 1)


def round_robin_pairs(m: int, step: int):
    """The m / 2 disjoint index pairs (p < q) of step `step` (0 .. m - 2) of the round-robin tournament over m (even) indices:
    (m - 1, step), then ((step + i) mod (m - 1), (step - i) mod (m - 1)) for i = 1 .. m / 2 - 1 -- mg_sym_eig's schedule."""
    i = np.arange(1, m // 2)
    a = np.concatenate(([m - 1], (step + i) % (m - 1)))
    b = np.concatenate(([step], (step - i) % (m - 1)))
    return np.minimum(a, b), np.maximum(a, b)


def host_sym_eig(A, vectors: bool = True):
    """mg_sym_eig restated in numpy for one symmetric matrix: cyclic two-sided Jacobi over the round-robin schedule (the matrix
    padded by a zero row and column to an even size), a pair left alone when |a_pq| <= 2^-53 sqrt|a_pp a_qq| or
    |a_pq| <= 2^-53 |A|_F / m, the tangent from theta without theta^2, at most EIG_MAX_SWEEPS sweeps, the first sweep that rotates
    nothing ends the solve (and is counted), the vectors' columns normalised once at the end.  Returns (w ascending, V with
    columns in w's order or None, sweeps, converged)."""
    A = np.asarray(A, dtype=np.float64)
    if A.ndim != 2 or A.shape[0] != A.shape[1] or A.shape[0] < 1:
        raise ValueError(f"host_sym_eig: a square matrix expected, got {A.shape}")
    D = A.shape[0]
    m = D + (D & 1)
    W = np.zeros((m, m))
    W[:D, :D] = 0.5 * A + 0.5 * A.T
    V = np.eye(m) if vectors else None
    big = float(np.abs(W).max())         # |A|_F scaled by the largest entry: no square overflows
    tol_abs = EIG_EPS * big * np.sqrt(((W / big) ** 2).sum()) / m if big > 0.0 else 0.0
    sweeps, converged = 0, False
    with np.errstate(all="ignore"):
        for _ in range(EIG_MAX_SWEEPS):
            rotated = False
            for step in range(m - 1):
                p, q = round_robin_pairs(m, step)
                app, aqq, apq = W[p, p], W[q, q], W[p, q]
                mag = np.abs(apq)
                on = ~(mag <= EIG_EPS * (np.sqrt(np.abs(app)) * np.sqrt(np.abs(aqq)))) & ~(mag <= tol_abs)
                if not on.any():
                    continue
                rotated = True
                p, q, app, aqq, apq = p[on], q[on], app[on], aqq[on], apq[on]
                theta = 0.5 * (aqq - app) / apq
                at = np.abs(theta)
                t = 1.0 / (at + np.hypot(1.0, at))
                t = np.where(theta < 0.0, -t, t)
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
                Cp, Cq = W[:, p].copy(), W[:, q].copy()
                W[:, p], W[:, q] = c * Cp - s * Cq, s * Cp + c * Cq
                Rp, Rq = W[p, :].copy(), W[q, :].copy()
                W[p, :], W[q, :] = c[:, None] * Rp - s[:, None] * Rq, s[:, None] * Rp + c[:, None] * Rq
                W[p, p], W[q, q] = app - t * apq, aqq + t * apq
                W[p, q] = W[q, p] = 0.0
                if vectors:
                    Vp, Vq = V[:, p].copy(), V[:, q].copy()
                    V[:, p], V[:, q] = c * Vp - s * Vq, s * Vp + c * Vq
            sweeps += 1
            if not rotated:
                converged = True
                break
    d = np.diag(W)[:D]
    order = np.argsort(d, kind="stable")
    if vectors:         # c^2 + s^2 is 1 only to rounding: the columns' norms drift over a solve and are restored once, here
        V = V[:D, :D]
        V = (V / np.sqrt((V * V).sum(0)))[:, order]
    return d[order].copy(), V, sweeps, converged


def sqrt_term_from_moments(S1, S2) -> float:
    """tr (S1 S2)^(1/2) = sum_i sqrt(max(lambda_i(B), 0)) with B = H^T S2 H, H = V diag(sqrt(max(w, 0))), S1 = V diag(w) V^T."""
    w, V = np.linalg.eigh(np.asarray(S1, dtype=np.float64))
    H = V * np.sqrt(np.maximum(w, 0.0))
    B = H.T @ np.asarray(S2, dtype=np.float64) @ H
    return float(np.sqrt(np.maximum(np.linalg.eigvalsh(0.5 * (B + B.T)), 0.0)).sum())


def frechet_terms(m1, S1, m2, S2):
    """(fd, |m1 - m2|^2, tr S1 + tr S2, tr (S1 S2)^(1/2)) by np.linalg.eigh: the entries of mg_frechet_pairs' out row."""
    m1, m2 = np.atleast_1d(np.asarray(m1, dtype=np.float64)), np.atleast_1d(np.asarray(m2, dtype=np.float64))
    S1, S2 = np.atleast_2d(np.asarray(S1, dtype=np.float64)), np.atleast_2d(np.asarray(S2, dtype=np.float64))
    mean_term = float(((m1 - m2) ** 2).sum())
    trace_term = float(np.trace(S1) + np.trace(S2))
    root = sqrt_term_from_moments(S1, S2)
    return mean_term + trace_term - 2.0 * root, mean_term, trace_term, root


def frechet_from_moments(m1, S1, m2, S2) -> float:
    """The Frechet distance between N(m1, S1) and N(m2, S2): |m1 - m2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2), the last term
    through the symmetric B (sqrt_term_from_moments): well defined for rank-deficient covariances."""
    return frechet_terms(m1, S1, m2, S2)[0]


def spectrum_stats(w) -> dict:
    """Of a covariance's eigenvalues w, clamped at 0: participation ratio (sum w)^2 / sum w^2, effective rank
    exp(-sum p ln p) with p = w / sum w, and the largest one's share.  All None when they sum to 0."""
    w = np.maximum(np.asarray(w, dtype=np.float64).ravel(), 0.0)
    total = float(w.sum())
    if not total > 0.0:
        return dict.fromkeys(SPECTRUM_KEYS)
    p = w / total
    p = p[p > 0.0]
    return {"participation_ratio": total * total / float((w * w).sum()), "effective_rank": float(np.exp(-(p * np.log(p)).sum())),
            "top1_share": float(w.max()) / total}


def _finite(v) -> Optional[float]:
    return None if v is None or not np.isfinite(v) else float(v)


def _spectrum_entry(triple) -> dict:
    if triple is None:
        return dict.fromkeys(SPECTRUM_KEYS)
    return {k: _finite(v) for k, v in zip(SPECTRUM_KEYS, triple)}


def frechet_block(dim: int, emotions: Sequence[str], counts: Sequence[int], rows: dict, spectra: dict) -> dict:
    """The --frechet entries of the feature_space block.
    counts[e]: rows of emotion e (the real and the generated side hold the same rows).
    rows:      {"whole": (fd, mean term, trace term, sqrt term) or None; "ef"[e][f]: the same for real emotion e against
               generated emotion f, or None} -- mg_frechet_pairs' out rows; None for a pair with a side of fewer than 2 rows.
    spectra:   {"real", "fake": (participation ratio, effective rank, top-1 share) or None; "real_e"[e], "fake_e"[e]}.
    NaN (a solve that did not converge; a spectrum that sums to 0) becomes None.  Returns {"frechet", "fd_e" (by emotion name),
    "fd_matrix", "spectrum"}; evaluate puts fd_e[name] into per_emotion[name]["fd"]."""
    counts = [int(c) for c in counts]
    n, K, dim = sum(counts), len(emotions), int(dim)
    fd = lambda row: None if row is None else _finite(row[0])  # noqa: E731
    whole = rows["whole"]
    frechet = {"fd": fd(whole)}
    for i, key in enumerate(("mean_term", "trace_term", "sqrt_term"), 1):
        frechet[key] = None if whole is None else _finite(whole[i])
    frechet.update(n_real=n, n_fake=n, rank_deficient=n <= dim)
    matrix = {emotions[e]: {emotions[f]: fd(rows["ef"][e][f]) for f in range(K)} for e in range(K)}
    spectrum = {"real": _spectrum_entry(spectra["real"]), "fake": _spectrum_entry(spectra["fake"]),
                "per_emotion": {emotions[e]: {"real": _spectrum_entry(spectra["real_e"][e]),
                                              "fake": _spectrum_entry(spectra["fake_e"][e])} for e in range(K)}}
    return {"frechet": frechet, "fd_e": {emotions[e]: matrix[emotions[e]][emotions[e]] for e in range(K)}, "fd_matrix": matrix,
            "spectrum": spectrum}


def frechet_inputs_host(R, F, labels, K: int):
    """frechet_block's `rows` and `spectra` from the feature rows themselves, in fp64 on the host (np.linalg.eigh): what
    Evaluator.feature_space computes on the device.  R, F: (n, D) real and generated rows; labels (n) class indices."""
    R, F, labels = np.asarray(R, dtype=np.float64), np.asarray(F, dtype=np.float64), np.asarray(labels)
    moments = lambda X: host_moments(X) if len(X) >= 2 else None  # noqa: E731
    pair = lambda a, b: None if a is None or b is None else frechet_terms(a[0], a[1], b[0], b[1])  # noqa: E731
    spec = lambda a: None if a is None else tuple(spectrum_stats(np.linalg.eigvalsh(a[1])).values())  # noqa: E731
    mr, mf = moments(R), moments(F)
    mre, mfe = [moments(R[labels == e]) for e in range(K)], [moments(F[labels == e]) for e in range(K)]
    rows = {"whole": pair(mr, mf), "ef": [[pair(mre[e], mfe[f]) for f in range(K)] for e in range(K)]}
    spectra = {"real": spec(mr), "fake": spec(mf), "real_e": [spec(a) for a in mre], "fake_e": [spec(a) for a in mfe]}
    return rows, spectra


def format_block(fs: dict, nn_train: Optional[dict] = None) -> str:
    """The table lines of the block (evaluate.format_table)."""
    f = lambda v, spec: "-" if v is None else format(v, spec)  # noqa: E731
    lines = [f"feature space (dim {fs['dim']}, k {fs['k']}): kid {f(fs['kid'], '.5f')}  precision {f(fs['precision'], '.3f')}  "
             f"recall {f(fs['recall'], '.3f')}",
             f"  {'emotion':<8} {'n':>6} {'kid':>10} {'precision':>10} {'recall':>8}"]
    for name, s in fs["per_emotion"].items():
        lines.append(f"  {name:<8} {s['n']:>6} {f(s['kid'], '.5f'):>10} {f(s['precision'], '.3f'):>10} {f(s['recall'], '.3f'):>8}")
    names = list(fs["kid_matrix"])
    lines.append("  kid, real emotion (row) against generated emotion (column):")
    lines.append(f"  {'':<8} " + " ".join(f"{c:>10}" for c in names))
    for r in names:
        lines.append(f"  {r:<8} " + " ".join(f"{f(fs['kid_matrix'][r][c], '.5f'):>10}" for c in names))
    if nn_train is not None:
        for side in ("fake", "real"):
            q = nn_train[side]
            lines.append(f"  nearest training row, {side}: d2 median {f(q and q['median'], '.5g')}  p05 {f(q and q['p05'], '.5g')}")
        lines.append(f"  generated rows within the validation rows' p05: {f(nn_train['fake_below_real_p05'], '.3f')}")
    if "frechet" in fs:
        fr, sp = fs["frechet"], fs["spectrum"]
        lines.append(f"  frechet distance {f(fr['fd'], '.5g')}  (mean {f(fr['mean_term'], '.5g')}  trace {f(fr['trace_term'], '.5g')}  "
                     f"sqrt {f(fr['sqrt_term'], '.5g')}; {fr['n_real']} real, {fr['n_fake']} generated rows"
                     f"{', rank deficient' if fr['rank_deficient'] else ''})")
        lines.append("  fd, real emotion (row) against generated emotion (column):")
        lines.append(f"  {'':<8} " + " ".join(f"{c:>10}" for c in names))
        for r in names:
            lines.append(f"  {r:<8} " + " ".join(f"{f(fs['fd_matrix'][r][c], '.5g'):>10}" for c in names))
        lines.append(f"  covariance spectrum: {'':<6} {'eff. rank':>10} {'part. ratio':>12} {'top-1 share':>12}")
        for tag, s in [("all real", sp["real"]), ("all fake", sp["fake"])] + \
                [(f"{name} {side}", sp["per_emotion"][name][side]) for name in names for side in ("real", "fake")]:
            lines.append(f"  {tag:<27} {f(s['effective_rank'], '.3f'):>10} {f(s['participation_ratio'], '.3f'):>12} "
                         f"{f(s['top1_share'], '.3f'):>12}")
    return "\n".join(lines)
