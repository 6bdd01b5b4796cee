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
    return "\n".join(lines)
