"""Held-out statistics of a trained emotion classifier -- the host side of `python -m melo_gan_amd.emotion_discriminator.evaluate`.

The classifier is the frozen judge of the project: the generator trains against its cross-entropy, gan.evaluate reports its
accuracy on generated rolls, and KID, precision / recall and t-SNE live in its feature space.  The reference meant to evaluate
it (src/emotion_discriminator/evaluate_ed.py) but that file is a copy of the model.  Here the judge gets numbers: which
emotions it confuses (confusion matrix, precision / recall / F1, one-vs-rest AUROC), whether its confidence is worth what it
says (Brier score, ECE / MCE over equal-width bins, the NLL over a grid of temperatures and the temperature that minimises
it), and which rows it finds hardest.

csrc/cls_metrics.hip computes the accumulator (mg_cls_eval_acc) and the pair counts (mg_cls_auroc_pairs) on the device;
host_cls_stats and host_auroc_pairs are their references in numpy, with the kernels' order of operations, and report turns
the two into the JSON block.  This module imports no GPU code.
"""
from __future__ import annotations

import math

import numpy as np

N_BINS = 15
GRID = 33                       # T_g = 2^((g - 16) / 4), g = 0 .. 32: 1/16 .. 16, T = 1 at g = 16
GRID_ONE = 16
HARDEST = 10
INT_FIELDS = ("rows", "correct", "flipped", "confusion", "bin_count", "bin_correct")
FIELDS = INT_FIELDS + ("ce", "brier", "conf", "margin", "bin_conf", "nll_T")
ROW_I = ("pred", "bin", "correct", "flipped")
ROW_D = ("ce", "conf", "p_true", "margin")


def temperature_grid():
    """(T_g, 1 / T_g) of the grid as Python floats: the inverse is what both the kernel and host_cls_stats multiply by."""
    T = [2.0 ** ((g - GRID_ONE) / 4.0) for g in range(GRID)]
    return T, [2.0 ** (-(g - GRID_ONE) / 4.0) for g in range(GRID)]


def acc_fields(K: int, n_bins: int, G: int):
    """One true class's block of the accumulator, in 8-byte words: (name, shape); 7 + K + 3 n_bins + G words
    (ops.cls_eval_layout)."""
    return (("rows", ()), ("correct", ()), ("flipped", ()), ("confusion", (K,)), ("bin_count", (n_bins,)),
            ("bin_correct", (n_bins,)), ("ce", ()), ("brier", ()), ("conf", ()), ("margin", ()), ("bin_conf", (n_bins,)),
            ("nll_T", (G,)))


def new_acc(K: int, n_bins: int, G: int) -> dict:
    return {name: np.zeros((K, *shape), dtype=np.int64 if name in INT_FIELDS else np.float64)
            for name, shape in acc_fields(K, n_bins, G)}


def _nll(z, pred: int, y: int, s: float):
    """log sum_k exp(z_k s) - z_y s the kernel's way: the maximum's own term is 1 and not computed, the others are added in
    class order and go through log1p.  Returns (nll, rest)."""
    m = z[pred] * s
    rest = 0.0
    for k in range(len(z)):
        if k != pred:
            rest = rest + math.exp(z[k] * s - m)
    return math.log1p(rest) + (m - z[y] * s), rest


def host_cls_stats(logits, labels, K: int, n_bins: int, inv_temps, inv_temperature: float = 1.0, clean_logits=None):
    """The kernel's reference: (acc, probs (n, K) float64, row_i (n, 4) int64, row_d (n, 4) float64) of n rows of logits
    (n, K) fp32 with true classes `labels`; acc is new_acc's dict of (K, ...) arrays indexed by the TRUE class.  Rows with a
    label outside [0, K) are padding and stay zero.  The rows are added in order, one at a time."""
    logits, labels = np.asarray(logits), np.asarray(labels).astype(np.int64)
    if logits.ndim != 2 or logits.shape[1] != K or logits.dtype != np.float32 or labels.shape != (logits.shape[0],):
        raise ValueError(f"host_cls_stats: logits (n, {K}) float32 and labels (n,) expected")
    if not 2 <= K <= 16 or not 1 <= n_bins <= 32 or not 1 <= len(inv_temps) <= 64:
        raise ValueError("host_cls_stats: 2..16 classes, 1..32 bins and 1..64 inverse temperatures")
    if clean_logits is not None:
        clean_logits = np.asarray(clean_logits)
        if clean_logits.shape != logits.shape or clean_logits.dtype != np.float32:
            raise ValueError("host_cls_stats: clean_logits must match logits")
    n, G = logits.shape[0], len(inv_temps)
    it = float(inv_temperature)
    acc = new_acc(K, n_bins, G)
    probs = np.zeros((n, K), dtype=np.float64)
    row_i, row_d = np.zeros((n, 4), dtype=np.int64), np.zeros((n, 4), dtype=np.float64)
    for r in range(n):
        y = int(labels[r])
        if not 0 <= y < K:
            continue
        z = [float(v) * it for v in logits[r]]
        pred = int(np.argmax(z))                    # the first maximum
        ce, rest = _nll(z, pred, y, 1.0)
        s, m = 1.0 + rest, z[pred]
        p = [1.0 / s if k == pred else math.exp(z[k] - m) / s for k in range(K)]
        brier = 0.0
        for k in range(K):
            d = p[k] - (1.0 if k == y else 0.0)
            brier = brier + d * d
        conf = p[pred]
        margin = conf - max([0.0] + [p[k] for k in range(K) if k != pred])
        b = min(n_bins - 1, int(math.floor(conf * float(n_bins))))
        correct, flipped = int(pred == y), 0
        if clean_logits is not None:
            flipped = int(int(np.argmax([float(v) * it for v in clean_logits[r]])) != pred)
        a = acc
        a["rows"][y] += 1
        a["correct"][y] += correct
        a["flipped"][y] += flipped
        a["confusion"][y, pred] += 1
        a["bin_count"][y, b] += 1
        a["bin_correct"][y, b] += correct
        a["ce"][y] += ce
        a["brier"][y] += brier
        a["conf"][y] += conf
        a["margin"][y] += margin
        a["bin_conf"][y, b] += conf
        for g in range(G):
            a["nll_T"][y, g] += _nll(z, pred, y, float(inv_temps[g]))[0]
        probs[r] = p
        row_i[r] = (pred, b, correct, flipped)
        row_d[r] = (ce, conf, p[y], margin)
    return acc, probs, row_i, row_d


def host_auroc_pairs(probs, labels, K: int):
    """mg_cls_auroc_pairs' reference: int64 (4, K) wins, ties, n_pos, n_neg.  wins[k] = #{(i, j): y_i = k, y_j valid and != k,
    p_ik > p_jk}; ties likewise with ==.  Counted from sorted negatives, which is the same integer."""
    probs, labels = np.asarray(probs, dtype=np.float64), np.asarray(labels).astype(np.int64)
    if probs.ndim != 2 or probs.shape[1] != K or labels.shape != (probs.shape[0],):
        raise ValueError(f"host_auroc_pairs: probs (n, {K}) and labels (n,) expected")
    valid = (labels >= 0) & (labels < K)
    out = np.zeros((4, K), dtype=np.int64)
    for k in range(K):
        pos, neg = probs[valid & (labels == k), k], np.sort(probs[valid & (labels != k), k])
        lo, hi = np.searchsorted(neg, pos, side="left"), np.searchsorted(neg, pos, side="right")
        out[:, k] = (lo.sum(), (hi - lo).sum(), len(pos), len(neg))
    return out


def _ratio(a, b):
    a, b = float(a), float(b)
    return a / b if b != 0 and math.isfinite(a) and math.isfinite(b) else None


def _block(v: dict, n_bins: int) -> dict:
    """The metrics of one set of rows from its summed accumulator words (no confusion-derived numbers: those need every
    class's block)."""
    n = int(v["rows"])
    out = {"rows": n, "accuracy": _ratio(v["correct"], n), "cross_entropy": _ratio(v["ce"], n), "brier": _ratio(v["brier"], n),
           "mean_confidence": _ratio(v["conf"], n), "mean_margin": _ratio(v["margin"], n)}
    table, ece, mce = [], 0.0, 0.0
    for b in range(n_bins):
        c = int(v["bin_count"][b])
        acc_b, conf_b = _ratio(v["bin_correct"][b], c), _ratio(v["bin_conf"][b], c)
        table.append({"lo": b / n_bins, "hi": (b + 1) / n_bins, "rows": c, "accuracy": acc_b, "confidence": conf_b})
        if c and n:
            gap = abs(acc_b - conf_b)
            ece += gap * c / n
            mce = max(mce, gap)
    out["ece"], out["mce"] = (ece, mce) if n else (None, None)
    out["reliability"] = table
    return out


def _f1(p, r):
    if p is None or r is None:
        return None
    return 2 * p * r / (p + r) if p + r > 0 else 0.0


def _mean(vals):
    known = [x for x in vals if x is not None]
    return sum(known) / len(known) if known else None


def block(acc: dict, pairs=None, names=None, n_bins=None, with_temperature: bool = True) -> dict:
    """`overall` and `per_class` of one accumulator (and, with pairs, the AUROCs): what report holds for the plain pass and
    again under `calibrated`."""
    v = {k: np.asarray(a) for k, a in acc.items()}
    K = v["rows"].shape[0]
    n_bins = v["bin_count"].shape[1] if n_bins is None else n_bins
    names = [str(k) for k in range(K)] if names is None else list(names)
    if len(names) != K:
        raise ValueError(f"report: {len(names)} names for {K} classes")
    conf = v["confusion"]
    if conf.shape != (K, K):
        raise ValueError(f"report: the accumulator is not that of {K} classes")
    overall = _block({f: v[f].sum(axis=0) for f in FIELDS}, n_bins)
    overall["flipped"] = int(v["flipped"].sum())
    overall["confusion"] = [[int(c) for c in row] for row in conf]        # [true][predicted]
    per = {}
    for k, name in enumerate(names):
        b = _block({f: v[f][k] for f in FIELDS}, n_bins)
        b["flipped"] = int(v["flipped"][k])
        b["predicted_as"] = {names[j]: int(conf[k, j]) for j in range(K)}
        b["precision"] = _ratio(conf[k, k], conf[:, k].sum())
        b["recall"] = _ratio(conf[k, k], conf[k].sum())
        b["f1"] = _f1(b["precision"], b["recall"])
        if pairs is not None:
            w, t, npos, nneg = (int(x) for x in np.asarray(pairs)[:, k])
            b["auroc"] = (w + t / 2) / (npos * nneg) if npos and nneg else None
        per[name] = b
    live = [per[nm] for nm in names if per[nm]["rows"]]
    overall["macro_f1"] = _mean([b["f1"] for b in live])
    overall["balanced_accuracy"] = _mean([b["recall"] for b in live])
    if pairs is not None:
        overall["macro_auroc"] = _mean([per[nm]["auroc"] for nm in names])
    out = {"overall": overall, "per_class": per}
    if with_temperature:
        T, _ = temperature_grid()
        nll = v["nll_T"].sum(axis=0)
        n = int(v["rows"].sum())
        if len(nll) != len(T):
            raise ValueError(f"report: {len(nll)} temperatures in the accumulator, the grid has {len(T)}")
        g = int(np.argmin(nll)) if n else None
        out["temperature"] = {"grid": T, "nll": [_ratio(x, n) for x in nll], "argmin": g, "best_T": None if g is None else T[g],
                              "best_nll": None if g is None else _ratio(nll[g], n)}
    return out


def hardest_rows(rows: dict, labels, names=None, count: int = HARDEST):
    """The `count` split positions with the lowest p[y] among the labelled rows (ties: the lower position)."""
    labels = np.asarray(labels)
    p_true, pred = np.asarray(rows["row_d"])[:, 2], np.asarray(rows["row_i"])[:, 0]
    K = None if names is None else len(names)
    valid = np.flatnonzero((labels >= 0) & ((labels < K) if K else True))
    pick = valid[np.argsort(p_true[valid], kind="stable")[:count]]
    nm = (lambda k: names[int(k)]) if names is not None else (lambda k: int(k))
    return [{"row": int(r), "label": nm(labels[r]), "predicted": nm(pred[r]), "p_true": float(p_true[r])} for r in pick]


def report(acc: dict, pairs, names=None, rows=None, labels=None, calibrated_acc=None) -> dict:
    """The JSON block of a pass: `overall`, `per_class` by name (names: the K class names; their indices otherwise),
    `temperature` (the grid, the mean NLL at each entry, the argmin), `calibrated` (the same block of calibrated_acc, the
    accumulator of a second cls_eval_acc over the stored logits at the argmin temperature) and `hardest_rows` (rows: the
    per-row records {"row_i", "row_d"}, labels: the split's).  Plain Python values only; a ratio with a zero denominator is
    None (null), never NaN."""
    out = block(acc, pairs, names)
    n_bins = np.asarray(acc["bin_count"]).shape[1]
    out["n_bins"] = int(n_bins)
    if calibrated_acc is not None:
        cal = block(calibrated_acc, pairs=None, names=names, with_temperature=False)
        cal["T"] = out["temperature"]["best_T"]
        out["calibrated"] = cal
    if rows is not None and labels is not None:
        out["hardest_rows"] = hardest_rows(rows, labels, names)
    return out
