"""emotion_discriminator.metrics (the host restatement of csrc/cls_metrics.hip and the report) against independent formulas:
torch's cross-entropy and argmax in fp64, AUROC from average ranks, F1 from the confusion matrix by hand, and scikit-learn
where it imports.  No GPU."""
import json
import math

import numpy as np
import pytest
import torch

import melo_gan_amd  # noqa: F401
from melo_gan_amd.emotion_discriminator import metrics as M

K, NB = 4, 15


def random_case(n=97, seed=0, scale=3.0):
    g = np.random.default_rng(seed)
    logits = (g.normal(0, scale, (n, K))).astype(np.float32)
    labels = g.integers(0, K, n).astype(np.int64)
    logits[np.arange(n), labels] += 1.5          # better than chance
    labels[5], labels[40] = -1, K                # two unlabelled rows
    return logits, labels


def stats(logits, labels, **kw):
    _, inv = M.temperature_grid()
    return M.host_cls_stats(logits, labels, K, NB, inv, **kw)


def rank_auroc(score, positive):
    """AUROC from average ranks: (sum of the positives' ranks - n_pos (n_pos + 1) / 2) / (n_pos n_neg)."""
    order = np.argsort(score, kind="stable")
    ranks = np.empty(len(score))
    s = score[order]
    i = 0
    while i < len(s):
        j = i
        while j + 1 < len(s) and s[j + 1] == s[i]:
            j += 1
        ranks[order[i:j + 1]] = (i + j) / 2 + 1
        i = j + 1
    n_pos, n_neg = int(positive.sum()), int((~positive).sum())
    return (ranks[positive].sum() - n_pos * (n_pos + 1) / 2) / (n_pos * n_neg)


def test_grid_is_two_to_the_quarter_steps_with_one_in_the_middle():
    T, inv = M.temperature_grid()
    assert len(T) == len(inv) == 33 and T[16] == 1.0 and inv[16] == 1.0 and T[0] == 1 / 16 and T[32] == 16.0
    assert all(abs(t * i - 1) < 1e-15 for t, i in zip(T, inv))


def test_sums_match_torch_in_fp64():
    logits, labels = random_case()
    acc, probs, row_i, row_d = stats(logits, labels)
    ok = (labels >= 0) & (labels < K)
    z, y = torch.from_numpy(logits[ok]).double(), torch.from_numpy(labels[ok])
    ce = torch.nn.functional.cross_entropy(z, y, reduction="sum").item()
    assert abs(acc["ce"].sum() - ce) <= 1e-12 * ce
    assert int(acc["rows"].sum()) == int(ok.sum()) == len(labels) - 2
    np.testing.assert_array_equal(row_i[ok, 0], torch.argmax(z, dim=1).numpy())
    assert int(acc["correct"].sum()) == int((torch.argmax(z, dim=1) == y).sum())
    p = torch.softmax(z, dim=1).numpy()
    np.testing.assert_allclose(probs[ok], p, rtol=0, atol=1e-14)
    assert not probs[~ok].any() and not row_d[~ok].any() and not row_i[~ok].any()
    onehot = np.eye(K)[labels[ok]]
    assert abs(acc["brier"].sum() - ((p - onehot) ** 2).sum()) <= 1e-12 * acc["brier"].sum()
    assert abs(acc["conf"].sum() - p.max(axis=1).sum()) <= 1e-12 * acc["conf"].sum()
    top2 = np.sort(p, axis=1)[:, -2:]
    assert abs(acc["margin"].sum() - (top2[:, 1] - top2[:, 0]).sum()) <= 1e-12 * (top2.sum())
    # T = 1 sits at grid index 16: the same computation, so the same bits
    assert np.array_equal(acc["nll_T"][:, 16].view(np.int64), acc["ce"].view(np.int64))
    T, _ = M.temperature_grid()
    for g in (0, 9, 25, 32):
        want = torch.nn.functional.cross_entropy(z / T[g], y, reduction="sum").item()
        assert abs(acc["nll_T"][:, g].sum() - want) <= 1e-12 * want, g
    # the confusion matrix and the bins
    conf = np.zeros((K, K), dtype=np.int64)
    np.add.at(conf, (labels[ok], p.argmax(axis=1)), 1)
    np.testing.assert_array_equal(acc["confusion"], conf)
    bins = np.minimum(NB - 1, np.floor(p.max(axis=1) * NB).astype(np.int64))
    np.testing.assert_array_equal(row_i[ok, 1], bins)
    assert acc["bin_count"].sum() == ok.sum() and (acc["bin_correct"] <= acc["bin_count"]).all()
    np.testing.assert_allclose(row_d[ok, 2], p[np.arange(len(y)), y.numpy()], rtol=0, atol=1e-14)


def test_inverse_temperature_is_applied_before_everything_else():
    logits, labels = random_case(seed=3)
    acc, probs, _, _ = stats(logits, labels, inv_temperature=0.5)
    ok = (labels >= 0) & (labels < K)
    z, y = torch.from_numpy(logits[ok]).double() * 0.5, torch.from_numpy(labels[ok])
    ce = torch.nn.functional.cross_entropy(z, y, reduction="sum").item()
    assert abs(acc["ce"].sum() - ce) <= 1e-12 * ce
    np.testing.assert_allclose(probs[ok], torch.softmax(z, dim=1).numpy(), rtol=0, atol=1e-14)
    plain = stats(logits, labels)[0]
    assert np.array_equal(acc["nll_T"][:, 16].view(np.int64), acc["ce"].view(np.int64))
    # T = 2 of the plain pass is grid index 20
    np.testing.assert_allclose(plain["nll_T"][:, 20], acc["ce"], rtol=1e-13)


def test_hand_made_case():
    # rows: a tie (lowest index wins), equal logits at K = 2 -> handled in the K = 2 test below, a gap of 800, +-80
    logits = np.array([[2.0, 2.0, 0.0, 0.0],            # tie of classes 0 and 1 -> pred 0; p = e^0 / (2 + 2 e^-2)
                       [800.0, 0.0, 0.0, 0.0],          # p = 1 exactly -> the last bin
                       [0.0, 800.0, 0.0, 0.0],          # the same gap, judged wrong: ce = 800, finite
                       [80.0, -80.0, 80.0, -80.0],      # tie again, p = 0.5 each
                       [0.0, 0.0, 0.0, 0.0]], dtype=np.float32)
    labels = np.array([1, 0, 0, 2, 3], dtype=np.int64)
    acc, probs, row_i, row_d = stats(logits, labels)
    assert row_i[:, 0].tolist() == [0, 0, 1, 0, 0]
    assert row_i[:, 2].tolist() == [0, 1, 0, 0, 0]
    assert probs[1, 0] == 1.0 and row_i[1, 1] == NB - 1 and row_d[1, 0] == 0.0
    assert row_d[2, 0] == 800.0 and row_d[2, 2] == 0.0
    assert probs[3, 0] == probs[3, 2] == 0.5 and 0 < probs[3, 1] == probs[3, 3] < 1e-69 and row_d[3, 3] == 0.0
    assert probs[4].tolist() == [0.25] * 4 and row_i[4, 1] == min(NB - 1, int(0.25 * NB))
    s = 2 + 2 * math.exp(-2.0)
    assert abs(probs[0, 0] - 1 / s) < 1e-16 and abs(row_d[0, 0] - math.log(s)) < 1e-15
    for v in acc.values():
        assert np.isfinite(v).all()
    assert acc["rows"].tolist() == [2, 1, 1, 1] and acc["confusion"][0].tolist() == [1, 1, 0, 0]
    # K = 2, equal logits, 10 bins: the confidence is exactly 0.5 and goes to bin 5
    _, inv = M.temperature_grid()
    a2, p2, i2, _ = M.host_cls_stats(np.zeros((1, 2), np.float32), np.array([1]), 2, 10, inv)
    assert p2[0].tolist() == [0.5, 0.5] and i2[0].tolist() == [0, 5, 0, 0] and a2["bin_count"][1, 5] == 1


def test_flips_count_rows_whose_argmax_differs_from_the_clean_one():
    logits, labels = random_case(seed=5)
    clean = logits.copy()
    g = np.random.default_rng(6)
    noisy = (logits + g.normal(0, 2.0, logits.shape)).astype(np.float32)
    acc = stats(noisy, labels, clean_logits=clean)[0]
    ok = (labels >= 0) & (labels < K)
    want = int((noisy.argmax(axis=1) != clean.argmax(axis=1))[ok].sum())
    assert want > 0 and int(acc["flipped"].sum()) == want
    assert int(stats(logits, labels, clean_logits=clean)[0]["flipped"].sum()) == 0


def test_pair_counts_give_the_rank_auroc():
    logits, labels = random_case(n=200, seed=8)
    logits[10] = logits[11] = logits[12]        # duplicated rows: exact ties
    _, probs, _, _ = stats(logits, labels)
    pairs = M.host_auroc_pairs(probs, labels, K)
    ok = (labels >= 0) & (labels < K)
    for k in range(K):
        w, t, n_pos, n_neg = pairs[:, k]
        assert n_pos == (labels == k).sum() and n_neg == ok.sum() - n_pos
        brute_w = sum(int((probs[i, k] > probs[ok & (labels != k), k]).sum()) for i in np.flatnonzero(labels == k))
        brute_t = sum(int((probs[i, k] == probs[ok & (labels != k), k]).sum()) for i in np.flatnonzero(labels == k))
        assert (w, t) == (brute_w, brute_t)
        auroc = (w + t / 2) / (n_pos * n_neg)
        assert abs(auroc - rank_auroc(probs[ok, k], labels[ok] == k)) < 1e-12
    assert pairs[1].sum() > 0                  # the duplicated rows did tie


def test_report_by_hand_and_json():
    logits, labels = random_case(n=150, seed=11)
    labels[labels == 3] = 2                     # class 3 has no rows
    acc, probs, row_i, row_d = stats(logits, labels)
    pairs = M.host_auroc_pairs(probs, labels, K)
    names = ["happy", "sad", "angry", "calm"]
    rep = M.report(acc, pairs, names, {"row_i": row_i, "row_d": row_d}, labels, calibrated_acc=acc)
    json.dumps(rep, allow_nan=False)
    o = rep["overall"]
    conf = np.array(o["confusion"])
    n = conf.sum()
    assert o["rows"] == n == 148 and abs(o["accuracy"] - np.trace(conf) / n) < 1e-15
    f1s, recalls = [], []
    for k, nm in enumerate(names):
        b = rep["per_class"][nm]
        tp, fp, fn = conf[k, k], conf[:, k].sum() - conf[k, k], conf[k].sum() - conf[k, k]
        if nm == "calm":
            assert b["rows"] == 0 and b["recall"] is None and b["accuracy"] is None and b["auroc"] is None and b["ece"] is None
            assert b["precision"] == (0.0 if fp else None)
            continue
        assert abs(b["precision"] - tp / (tp + fp)) < 1e-15 and abs(b["recall"] - tp / (tp + fn)) < 1e-15
        assert abs(b["f1"] - 2 * tp / (2 * tp + fp + fn)) < 1e-15
        f1s.append(b["f1"]), recalls.append(b["recall"])
    assert abs(o["macro_f1"] - np.mean(f1s)) < 1e-15 and abs(o["balanced_accuracy"] - np.mean(recalls)) < 1e-15
    aurocs = [rep["per_class"][nm]["auroc"] for nm in names[:3]]
    assert abs(o["macro_auroc"] - np.mean(aurocs)) < 1e-15
    # ECE / MCE from the per-row records
    ok = (labels >= 0) & (labels < K)
    conf_r, corr, bins = row_d[ok, 1], row_i[ok, 2], row_i[ok, 1]
    ece, mce = 0.0, 0.0
    for b in range(NB):
        m = bins == b
        if m.any():
            gap = abs(corr[m].mean() - conf_r[m].mean())
            ece, mce = ece + gap * m.sum() / ok.sum(), max(mce, gap)
    assert abs(o["ece"] - ece) < 1e-12 and abs(o["mce"] - mce) < 1e-12
    assert sum(r["rows"] for r in o["reliability"]) == n and len(o["reliability"]) == NB
    t = rep["temperature"]
    assert len(t["grid"]) == len(t["nll"]) == 33 and t["nll"][t["argmin"]] == min(t["nll"]) == t["best_nll"]
    assert abs(t["nll"][16] - o["cross_entropy"]) < 1e-15
    assert rep["calibrated"]["overall"]["accuracy"] == o["accuracy"]
    hard = rep["hardest_rows"]
    assert len(hard) == 10 and [h["p_true"] for h in hard] == sorted(row_d[ok, 2])[:10]
    assert all(labels[h["row"]] == names.index(h["label"]) for h in hard)
    # an empty accumulator: nulls, never a division by zero
    empty = M.report(M.new_acc(K, NB, 33), np.zeros((4, K), np.int64), names)
    json.dumps(empty, allow_nan=False)
    assert empty["overall"]["accuracy"] is None and empty["overall"]["macro_f1"] is None and empty["temperature"]["argmin"] is None


def test_against_scikit_learn():
    skm = pytest.importorskip("sklearn.metrics")
    logits, labels = random_case(n=150, seed=13)
    acc, probs, row_i, row_d = stats(logits, labels)
    ok = (labels >= 0) & (labels < K)
    rep = M.report(acc, M.host_auroc_pairs(probs, labels, K))
    y, p = labels[ok], probs[ok]
    for k in range(K):
        assert abs(rep["per_class"][str(k)]["auroc"] - skm.roc_auc_score(y == k, p[:, k])) < 1e-12
    pr, rc, f1, _ = skm.precision_recall_fscore_support(y, row_i[ok, 0], labels=list(range(K)), zero_division=0)
    for k in range(K):
        b = rep["per_class"][str(k)]
        assert abs(b["precision"] - pr[k]) < 1e-12 and abs(b["recall"] - rc[k]) < 1e-12 and abs(b["f1"] - f1[k]) < 1e-12
    assert abs(rep["overall"]["cross_entropy"] - skm.log_loss(y, p, labels=list(range(K)))) < 1e-12


def test_kernel_argument_errors_return_minus_one_before_any_launch():
    """Validation runs without a device (as tests/test_abi.py's): non-null dummy addresses, nothing here launches."""
    import ctypes as C
    from melo_gan_amd import _lib
    lib = _lib.load()
    q, B, G = 4096, 8, 33
    temps = (C.c_double * G)(*M.temperature_grid()[1])
    need = lib.mg_cls_eval_acc_workspace_bytes(B, G)
    assert need == B * (6 + G) * 8 and lib.mg_cls_eval_acc_words(K, NB, G) == K * (7 + K + 3 * NB + G)

    def call(**kw):
        a = dict(logits=q, clean=None, B=B, K=K, labels=q, nb=NB, temps=temps, G=G, it=1.0, acc=q, probs=q, row_i=q, row_d=q,
                 dst_rows=8, counter=q, base=q, work=q, work_bytes=need, tick=None)
        a.update(kw)
        return lib.mg_cls_eval_acc(a["logits"], a["clean"], a["B"], a["K"], a["labels"], a["nb"], a["temps"], a["G"], a["it"], a["acc"],
                                   a["probs"], a["row_i"], a["row_d"], a["dst_rows"], a["counter"], a["base"], a["work"],
                                   a["work_bytes"], a["tick"], None)

    for bad_k in (1, 17):
        assert call(K=bad_k) == -1 and b"classes" in lib.mg_last_error()
        assert lib.mg_cls_eval_acc_words(bad_k, NB, G) == 0
    for bad_nb in (0, 33):
        assert call(nb=bad_nb) == -1 and b"n_bins" in lib.mg_last_error()
    for bad_g in (0, 65):
        assert call(G=bad_g) == -1 and b"temperatures" in lib.mg_last_error()
    assert call(it=0.0) == -1 and call(it=float("inf")) == -1 and b"inv_temperature" in lib.mg_last_error()
    bad = (C.c_double * G)(*([1.0] * 5 + [-1.0] + [1.0] * (G - 6)))
    assert call(temps=bad) == -1 and b"inv_temps[5]" in lib.mg_last_error()
    assert call(work_bytes=need - 1) == -1 and b"workspace" in lib.mg_last_error()
    for name in ("logits", "labels", "temps", "acc", "probs", "row_i", "row_d", "counter", "base", "work"):
        assert call(**{name: None}) == -1 and b"null" in lib.mg_last_error(), name
    assert call(B=0) == -1 and call(B=32768) == -1 and call(dst_rows=0) == -1
    assert call(probs=q + 4) == -1 and b"8-byte" in lib.mg_last_error()
    assert lib.mg_cls_auroc_pairs(q, q, 131073, K, q, None) == -1 and b"131072" in lib.mg_last_error()
    assert lib.mg_cls_auroc_pairs(q, q, 0, K, q, None) == -1 and lib.mg_cls_auroc_pairs(q, q, 10, 17, q, None) == -1
    assert lib.mg_cls_auroc_pairs(None, q, 10, K, q, None) == -1 and b"null" in lib.mg_last_error()
