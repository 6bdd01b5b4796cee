"""mg_cls_eval_acc and mg_cls_auroc_pairs (csrc/cls_metrics.hip) against their host restatement
emotion_discriminator.metrics: integer words exactly, fp64 words to 1e-12 of the sum of |terms| (the convention of
tests/test_vae_metrics_gpu.py: the kernel and the host add in the same order, but exp / log1p in fp64 may differ in the last
place), probabilities to 1e-14 absolute, bit identity between runs and under a graph replay.

Sum of |terms| of each fp64 word: ce, brier, conf, the bin confidences and the NLLs are sums of non-negative terms (ce =
log1p(rest) + (m - z_y), both >= 0), so the scale is the value itself; the margin is conf - second, its scale conf + second."""
import numpy as np
import pytest
import torch

import melo_gan_amd  # noqa: F401
from melo_gan_amd.emotion_discriminator import metrics as M

pytestmark = pytest.mark.gpu
BOUND = 1e-12
_, INV = M.temperature_grid()
INT = M.INT_FIELDS
DBL = tuple(f for f in M.FIELDS if f not in INT)


def crafted(B, K, seed):
    """Whole batches of B rows, the last one padded: (logits, clean_logits, labels, n) with n the split's rows (the padding
    rows behind carry label -1).  Class K - 1 has no rows.  The first rows are the crafted ones."""
    g = np.random.default_rng(seed)
    special = []

    def row(vals, label):
        z = np.full(K, -1.0, dtype=np.float32)
        z[:len(vals)] = vals
        special.append((z, label))

    wrong = 1 if K > 2 else 0
    row([3.0, 3.0], wrong)                                  # two equal maxima: the lowest index wins
    special.append((np.zeros(K, dtype=np.float32), 0))      # all equal: confidence exactly 1 / K (0.5 at K = 2 -> bin n_bins / 2)
    row([800.0, 0.0], 0)                                    # p = 1.0 exactly: the last bin
    special.append((np.concatenate([[0.0, 800.0], np.zeros(K - 2)]).astype(np.float32), 0))     # the same gap judged wrong
    special.append((np.where(np.arange(K) % 2 == 0, 80.0, -80.0).astype(np.float32), 0))        # +-80
    special.append((g.normal(0, 2, K).astype(np.float32), -1))                                   # skipped
    special.append((g.normal(0, 2, K).astype(np.float32), K))                                    # skipped
    nb = max(2, -(-(len(special) + 1) // B))
    rows = nb * B
    n = rows - max(1, B // 3)                               # the last batch's tail is padding
    logits = g.normal(0, 3, (rows, K)).astype(np.float32)
    labels = g.integers(0, K - 1, rows).astype(np.int64)    # class K - 1 never
    for i, (z, y) in enumerate(special[:n]):
        logits[i], labels[i] = z, y
    labels[n:] = -1
    clean = logits.copy()
    noisy = g.random(rows) < 0.4
    clean[noisy] += g.normal(0, 3, (int(noisy.sum()), K)).astype(np.float32)
    clean[2] = -logits[2]                                   # at least one flip at every size
    return logits, clean, labels, n, nb


def device_run(logits, labels, B, nb, n, n_bins, clean=None, inv_temperature=1.0):
    from melo_gan_amd import ops
    K = logits.shape[1]
    acc = ops.cls_eval_acc_new(K, n_bins, len(INV), "cuda")
    probs = torch.zeros(n, K, dtype=torch.float64, device="cuda")
    row_i = torch.zeros(n, 4, dtype=torch.int32, device="cuda")
    row_d = torch.zeros(n, 4, dtype=torch.float64, device="cuda")
    ctr, base = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
    for b in range(nb):
        s = slice(b * B, (b + 1) * B)
        t = [torch.from_numpy(np.ascontiguousarray(a[s])).cuda() for a in (logits, labels)]
        c = None if clean is None else torch.from_numpy(np.ascontiguousarray(clean[s])).cuda()
        ops.cls_eval_acc(t[0], t[1], acc, probs, row_i, row_d, ctr, base, n_bins, INV, inv_temperature, clean_logits=c, tick=ctr)
    torch.cuda.synchronize()
    assert int(ctr.item()) == nb
    views = {k: v.cpu().numpy() for k, v in ops.cls_eval_views(acc, K, n_bins, len(INV)).items()}
    return views, probs.cpu().numpy(), row_i.cpu().numpy(), row_d.cpu().numpy(), acc


def check(got, ref, what):
    g_acc, g_p, g_i, g_d = got
    r_acc, r_p, r_i, r_d = ref
    for f in INT:
        np.testing.assert_array_equal(g_acc[f], r_acc[f], err_msg=f"{what} {f}")
    np.testing.assert_array_equal(g_i, r_i.astype(np.int32), err_msg=what)
    scale = {f: r_acc[f] for f in DBL}
    scale["margin"] = 2 * r_acc["conf"] - r_acc["margin"]
    for f in DBL:
        err, bound = np.abs(g_acc[f] - r_acc[f]), BOUND * np.maximum(scale[f], 1e-30)
        print(f"{what} {f}: max |err| / (1e-12 sum|terms|) = {float((err / bound).max()):.3g}")
        assert np.isfinite(g_acc[f]).all() and (err <= bound).all(), (what, f, float((err / bound).max()))
    err = np.abs(g_p - r_p)
    print(f"{what} probs: max |err| = {float(err.max()):.3g}")
    assert np.isfinite(g_p).all() and (err <= 1e-14).all(), (what, float(err.max()))
    sc_d = r_d.copy()
    sc_d[:, 3] = 2 * r_d[:, 1] - r_d[:, 3]
    err, bound = np.abs(g_d - r_d), BOUND * np.maximum(sc_d, 1e-30)
    bound[:, 2] = 1e-14                                     # p[y]: a probability, held like probs
    print(f"{what} row_d: max |err| / bound = {float((err / bound).max()):.3g}")
    assert np.isfinite(g_d).all() and (err <= bound).all(), (what, float((err / bound).max()))


@pytest.mark.parametrize("K", [2, 4, 7, 16])
@pytest.mark.parametrize("B", [1, 7, 64, 130])
def test_kernel_matches_the_host_restatement(B, K):
    n_bins = 10 if (K == 2 or B in (7, 130)) else 15
    logits, clean, labels, n, nb = crafted(B, K, 1000 * B + K)
    ref = M.host_cls_stats(logits[:n], labels[:n], K, n_bins, INV, clean_logits=clean[:n])
    r_acc, r_p, r_i, r_d = ref
    # the crafted rows are what they claim to be
    assert r_i[0, 0] == 0 and r_p[0, 0] == r_p[0, 1]                        # the tie goes to the lowest index
    assert r_p[1, 0] == 1.0 / K and (K != 2 or (n_bins == 10 and r_i[1, 1] == 5))
    assert r_p[2, 0] == 1.0 and r_i[2, 1] == n_bins - 1 and r_d[3, 0] == 800.0
    assert r_acc["rows"][K - 1] == 0 and r_acc["rows"].sum() == n - 2 and r_acc["flipped"].sum() > 0
    got = device_run(logits, labels, B, nb, n, n_bins, clean)
    check(got[:4], ref, f"B{B} K{K}")
    g_acc, g_p, g_i, g_d, raw = got
    assert g_p[2, 0] == 1.0 and g_i[2, 1] == n_bins - 1 and g_p[1, 0] == 1.0 / K
    for r in (5, 6):                                                        # labels -1 and K wrote nothing
        assert not g_p[r].any() and not g_i[r].any() and not g_d[r].any()
    assert not g_acc["rows"][K - 1] and not g_acc["nll_T"][K - 1].any()
    # T = 1 sits at grid index 16: the same bits as the cross-entropy
    assert np.array_equal(g_acc["nll_T"][:, 16].view(np.int64), g_acc["ce"].view(np.int64))
    # a second run leaves identical bits
    again = device_run(logits, labels, B, nb, n, n_bins, clean)
    assert torch.equal(raw, again[4])
    for a, b in zip(got[1:4], again[1:4]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_inverse_temperature_and_no_clean_logits():
    B, K, n_bins = 7, 4, 15
    logits, _, labels, n, nb = crafted(B, K, 5)
    ref = M.host_cls_stats(logits[:n], labels[:n], K, n_bins, INV, inv_temperature=INV[11])
    got = device_run(logits, labels, B, nb, n, n_bins, None, INV[11])
    check(got[:4], ref, "invT")
    assert not got[0]["flipped"].any()


def test_graph_replay_leaves_the_eager_bits():
    from melo_gan_amd import ops
    B, K, n_bins = 64, 4, 15
    logits, clean, labels, n, nb = crafted(B, K, 9)
    _, p1, i1, d1, acc1 = device_run(logits, labels, B, nb, n, n_bins, clean)
    lg, cl = torch.from_numpy(logits).cuda(), torch.from_numpy(clean).cuda()
    lb = torch.from_numpy(labels).cuda()
    t = [torch.zeros(B, K, device="cuda"), torch.zeros(B, K, device="cuda"), torch.zeros(B, dtype=torch.int64, device="cuda")]
    acc = ops.cls_eval_acc_new(K, n_bins, len(INV), "cuda")
    probs = torch.zeros(n, K, dtype=torch.float64, device="cuda")
    row_i = torch.zeros(n, 4, dtype=torch.int32, device="cuda")
    row_d = torch.zeros(n, 4, dtype=torch.float64, device="cuda")
    ctr, base = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def batch():
        ops.stage_rows_cursor([(lg, t[0]), (cl, t[1]), (lb, t[2])], B, None, nb * B, ctr, base)
        ops.cls_eval_acc(t[0], t[2], acc, probs, row_i, row_d, ctr, base, n_bins, INV, clean_logits=t[1], tick=ctr)

    with torch.cuda.stream(s):
        graphs = {}
        for _ in range(nb + 1):                                 # eager (thrown away), then captured and replayed
            if graphs.get("b") == "warm":
                acc.zero_(), probs.zero_(), row_i.zero_(), row_d.zero_(), ctr.zero_()
            ops.run_graphed(graphs, "b", batch)
        torch.cuda.synchronize()
    assert int(ctr.item()) == nb and torch.equal(acc, acc1)
    assert np.array_equal(probs.cpu().numpy().view(np.int64), p1.view(np.int64))
    assert np.array_equal(row_d.cpu().numpy().view(np.int64), d1.view(np.int64)) and np.array_equal(row_i.cpu().numpy(), i1)


def pair_case(n, K, kind, seed):
    g = np.random.default_rng(seed)
    logits = g.normal(0, 2, (n, K)).astype(np.float32)
    if kind == "all_one_class":
        labels = np.zeros(n, dtype=np.int64)
    else:
        labels = g.integers(0, K - 1, n).astype(np.int64)       # class K - 1 has no positives
        if n >= 8:
            labels[g.choice(n, max(1, n // 10), replace=False)] = np.where(g.random(max(1, n // 10)) < 0.5, -1, K)
    if n >= 4:
        src = g.integers(0, n, n // 3)
        logits[g.integers(0, n, n // 3)] = logits[src]          # duplicated rows: bit-identical scores, so exact ties
    return logits, labels


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1000])
@pytest.mark.parametrize("kind", ["mixed", "all_one_class"])
def test_pair_counts_match_the_host(n, kind):
    from melo_gan_amd import ops
    K = 4
    logits, labels = pair_case(n, K, kind, 31 * n + len(kind))
    valid = np.where((labels >= 0) & (labels < K), labels, 0)
    _, probs_h, _, _, _ = device_run(logits, valid, n, 1, n, 15)      # the device's own stored probabilities, every row
    probs, lab = torch.from_numpy(probs_h).cuda(), torch.from_numpy(labels).cuda()
    want = M.host_auroc_pairs(probs_h, labels, K)
    out = ops.cls_auroc_pairs(probs, lab)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    ok = (labels >= 0) & (labels < K)
    assert want[2].sum() == ok.sum() and want[2, K - 1] == 0 and want[0, K - 1] == 0
    if kind == "all_one_class":
        assert want[2, 0] == n and not want[3, 0] and not want[0].any() and not want[1].any()
    elif n >= 63:
        assert want[1].sum() > 0 and want[0].sum() > 0          # ties and wins both occur
    out2 = ops.cls_auroc_pairs(probs, lab, out)                  # the call zeroes its output itself
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out2.cpu().numpy(), want)


def test_more_rows_than_the_pair_kernel_takes_raise_on_the_host():
    from melo_gan_amd import ops
    probs = torch.zeros(131073, 2, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="131072"):
        ops.cls_auroc_pairs(probs, torch.zeros(131073, dtype=torch.int64, device="cuda"))
