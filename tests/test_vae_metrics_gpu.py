"""mg_vae_eval_acc (csrc/vae_metrics.hip) against its host reference ae.metrics.host_vae_stats: integer words exactly, fp64
words to 1e-12 of the sum of |terms| (the bound tests/test_evaluate_gpu.py holds mg_eval_acc to: the kernel and numpy add in
the same order, but exp in fp64 may differ in the last place); bit identity between runs, between an eager run and a graph
replay, and between two ways of cutting the same rows into batches; the cursor; argument errors without a device."""
import numpy as np
import pytest
import torch

import melo_gan_amd  # noqa: F401
from melo_gan_amd.ae import metrics as M

gpu = pytest.mark.gpu
BOUND = 1e-12


def make_inputs(n, T, L, K, seed, pad_rows=(), empty_class=None):
    """x / recon uniform in [-1, 1], about a third of channel 1 of either below the rest threshold -0.2; mu / logvar of order
    one; labels cycling over the classes without `empty_class`, -1 on pad_rows."""
    g = np.random.default_rng(seed)
    x = g.uniform(-1, 1, (n, T, 4)).astype(np.float32)
    recon = g.uniform(-1, 1, (n, T, 4)).astype(np.float32)
    for a in (x, recon):
        rest = g.random((n, T)) < 1 / 3
        a[..., 1] = np.where(rest, g.uniform(-1, -0.25, (n, T)), g.uniform(-0.15, 1, (n, T))).astype(np.float32)
    mu = g.normal(0, 1, (n, L)).astype(np.float32)
    logvar = g.normal(-1, 1, (n, L)).astype(np.float32)
    classes = [k for k in range(K) if k != empty_class]
    labels = np.array([classes[r % len(classes)] for r in range(n)], dtype=np.int64)
    for r in pad_rows:
        labels[r] = -1
    return x, recon, mu, logvar, labels


def scales(acc, row_d, mu, logvar, labels, K):
    """Sum of |terms| of every fp64 word.  The squared, absolute and beat sums have non-negative terms: their own value.  The
    latent sums: |mu|, mu^2, |logvar|, exp(logvar), and for the KL the terms of the expression itself,
    (1 + |logvar| + mu^2 + exp(logvar)) / 2."""
    m, lv = mu.astype(np.float64), logvar.astype(np.float64)
    rows = np.stack([np.abs(m), m * m, np.abs(lv), np.exp(lv), 0.5 * (1 + np.abs(lv) + m * m + np.exp(lv))])      # (5, n, L)
    lat = np.stack([rows[:, labels == k].sum(axis=1) for k in range(K)])
    sc = {"se": acc["se"], "ae": acc["ae"], "beats_abs": acc["beats_abs"], "lat": lat}
    rd = row_d.copy()
    rd[:, 1] = np.where((labels >= 0) & (labels < K), rows[4].sum(axis=1), 0.0)[:len(rd)]      # row_d may stop short of the rows
    return sc, rd


def device_run(x, recon, mu, logvar, labels, K, cuts=None, dst_rows=None, acc=None):
    """The kernel over the rows cut into equal batches of `cuts` rows (default: one batch); returns (acc views as numpy, row_d,
    row_i, raw accumulator tensor, counter)."""
    from melo_gan_amd import ops
    n, L = mu.shape
    cuts = cuts or [n]
    dst_rows = dst_rows or n
    acc = ops.vae_eval_acc_new(K, L, "cuda") if acc is None else acc
    row_i = torch.zeros(dst_rows, 8, dtype=torch.int32, device="cuda")
    row_d = torch.zeros(dst_rows, 4, dtype=torch.float64, device="cuda")
    ctr, base = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
    at = 0
    for b in cuts:
        s = slice(at, at + b)
        t = [torch.from_numpy(np.ascontiguousarray(a[s])).cuda() for a in (x, recon, mu, logvar, labels)]
        before = int(ctr.item())
        ops.vae_eval_acc(t[0], t[1], t[2], t[3], t[4], acc, row_i, row_d, ctr, base, K, tick=ctr)
        assert int(ctr.item()) == before + 1        # tick advanced by exactly 1
        at += b
    torch.cuda.synchronize()
    views = {k: v.cpu().numpy() for k, v in ops.vae_eval_acc_views(acc, K, L).items()}
    return views, row_d.cpu().numpy(), row_i.cpu().numpy(), acc, ctr


def check(got, got_d, got_i, ref, ref_d, ref_i, mu, logvar, labels, K, what):
    np.testing.assert_array_equal(got["c"], ref["c"], err_msg=what)
    np.testing.assert_array_equal(got_i, ref_i.astype(np.int32), err_msg=what)
    sc, sc_d = scales(ref, ref_d, mu, logvar, labels, K)
    for k in ("se", "ae", "beats_abs", "lat"):
        err, bound = np.abs(got[k] - ref[k]), BOUND * np.maximum(sc[k], 1e-30)
        print(f"{what} {k}: max |err| / (1e-12 sum|terms|) = {float((err / bound).max()):.3g}")
        assert np.isfinite(got[k]).all() and (err <= bound).all(), (what, k, float((err / bound).max()))
    err, bound = np.abs(got_d - ref_d), BOUND * np.maximum(sc_d, 1e-30)
    print(f"{what} row_d: max |err| / (1e-12 sum|terms|) = {float((err / bound).max()):.3g}")
    assert (err <= bound).all(), (what, float((err / bound).max()))


@gpu
@pytest.mark.parametrize("B,T,L,K,pad,empty", [
    (3, 20, 5, 4, (1,), 2),         # one partial chunk, odd L, a padding row, a class with no rows
    (5, 300, 8, 4, (), None),       # two chunks, the second partial
    (2, 512, 300, 2, (), None),     # lanes stride over L
])
def test_kernel_matches_the_host_reference(B, T, L, K, pad, empty):
    x, recon, mu, logvar, labels = make_inputs(B, T, L, K, 100 + T, pad, empty)
    ref, ref_d, ref_i = M.host_vae_stats(x, recon, mu, logvar, labels, K)
    tot = ref["c"].sum(axis=0)
    assert tot[3] > 0 and tot[4] > 0 and tot[5] > 0 and tot[6] > 0        # all four rest / sounding combinations occur
    assert tot[0] == B - len(pad)
    if empty is not None:
        assert ref["c"][empty, 0] == 0
    got, got_d, got_i, _, _ = device_run(x, recon, mu, logvar, labels, K)
    check(got, got_d, got_i, ref, ref_d, ref_i, mu, logvar, labels, K, f"B{B} T{T} L{L}")
    for r in pad:
        assert not got_i[r].any() and not got_d[r].any()


@gpu
def test_non_finite_positions_land_in_invalid_and_nowhere_else():
    B, T, L, K = 4, 32, 8, 4
    x, recon, mu, logvar, labels = make_inputs(B, T, L, K, 7)
    clean = M.host_vae_stats(x, recon, mu, logvar, labels, K)[0]
    bad = [(0, 3), (1, 0), (1, 31), (2, 17)]                    # three positions of x, one of recon
    x[0, 3, 0], x[1, 0, 3], x[1, 31, 1], recon[2, 17, 2] = np.nan, np.inf, -np.inf, np.nan
    masked_x, masked_r = x.copy(), recon.copy()
    ref, ref_d, ref_i = M.host_vae_stats(x, recon, mu, logvar, labels, K)
    assert ref["c"][:, 2].sum() == 4 and ref["c"][:, 1].sum() == B * T - 4
    got, got_d, got_i, _, _ = device_run(x, recon, mu, logvar, labels, K)
    check(got, got_d, got_i, ref, ref_d, ref_i, mu, logvar, labels, K, "non-finite")
    assert got["c"][:, 2].tolist() == [1, 2, 1, 0] and np.isfinite(got_d).all()
    # nowhere else: everything but `valid` / `invalid` equals the statistics of the rows with those positions cut out
    for r, t in bad:
        masked_x[r, t] = masked_r[r, t] = 0.0
    hole = M.host_vae_stats(masked_x, masked_r, mu, logvar, labels, K)[0]
    zero = M.host_vae_stats(np.zeros((1, 1, 4), np.float32), np.zeros((1, 1, 4), np.float32), mu[:1], logvar[:1], labels[:1], K)[0]
    per_pos = zero["c"][labels[0]]                              # what one all-zero position adds on both sides
    for k in range(K):
        n_bad = sum(1 for r, _ in bad if labels[r] == k)
        np.testing.assert_array_equal(got["c"][k, 3:], hole["c"][k, 3:] - n_bad * per_pos[3:])
    assert (clean["c"][:, 1] - got["c"][:, 1]).tolist() == [1, 2, 1, 0]


@gpu
def test_two_runs_and_a_graph_replay_leave_identical_bits():
    from melo_gan_amd import ops
    B, T, L, K = 5, 300, 8, 4
    x, recon, mu, logvar, labels = make_inputs(B, T, L, K, 21)
    _, d1, i1, acc1, _ = device_run(x, recon, mu, logvar, labels, K)
    _, d2, i2, acc2, _ = device_run(x, recon, mu, logvar, labels, K)
    assert torch.equal(acc1, acc2) and np.array_equal(d1.view(np.int64), d2.view(np.int64)) and np.array_equal(i1, i2)
    t = [torch.from_numpy(a).cuda() for a in (x, recon, mu, logvar, labels)]
    acc3 = ops.vae_eval_acc_new(K, L, "cuda")
    row_i, row_d = torch.zeros(B, 8, dtype=torch.int32, device="cuda"), torch.zeros(B, 4, dtype=torch.float64, device="cuda")
    ctr, base = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        warm = ops.vae_eval_acc_new(K, L, "cuda")               # this stream's workspace exists before the capture
        ops.vae_eval_acc(*t, warm, row_i.clone(), row_d.clone(), ctr.clone(), base, K)
        g = ops.Graph.capture(lambda: ops.vae_eval_acc(*t, acc3, row_i, row_d, ctr, base, K, tick=ctr))
        g.launch()
        torch.cuda.synchronize()
    assert torch.equal(acc1, acc3) and int(ctr.item()) == 1
    assert np.array_equal(d1.view(np.int64), row_d.cpu().numpy().view(np.int64)) and np.array_equal(i1, row_i.cpu().numpy())


@gpu
def test_the_accumulator_does_not_depend_on_how_rows_are_cut_into_batches():
    B, T, L, K = 8, 40, 8, 3
    x, recon, mu, logvar, labels = make_inputs(B, T, L, K, 33)
    _, d1, i1, acc1, _ = device_run(x, recon, mu, logvar, labels, K)
    # 3 + 5: no cursor value puts a batch of 5 at split position 3, so the second call's per-row outputs go to a base of their own
    from melo_gan_amd import ops
    acc2 = ops.vae_eval_acc_new(K, L, "cuda")
    ctr, base = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
    rows = []
    for lo, hi in ((0, 3), (3, 8)):
        t = [torch.from_numpy(np.ascontiguousarray(a[lo:hi])).cuda() for a in (x, recon, mu, logvar, labels)]
        ri = torch.zeros(hi - lo, 8, dtype=torch.int32, device="cuda")
        rd = torch.zeros(hi - lo, 4, dtype=torch.float64, device="cuda")
        base.copy_(ctr)                                         # the cursor advanced between the two calls; position 0 of this call
        ops.vae_eval_acc(*t, acc2, ri, rd, ctr, base, K, tick=ctr)
        rows.append((rd.cpu().numpy(), ri.cpu().numpy()))
    assert int(ctr.item()) == 2
    assert torch.equal(acc1, acc2)
    assert np.array_equal(np.concatenate([r[0] for r in rows]).view(np.int64), d1.view(np.int64))
    assert np.array_equal(np.concatenate([r[1] for r in rows]), i1)


@gpu
def test_rows_past_the_split_end_are_dropped_but_still_counted():
    B, T, L, K = 8, 20, 5, 4
    x, recon, mu, logvar, labels = make_inputs(B, T, L, K, 44)
    ref, ref_d, ref_i = M.host_vae_stats(x, recon, mu, logvar, labels, K)
    got, got_d, got_i, _, ctr = device_run(x, recon, mu, logvar, labels, K, cuts=[4, 4], dst_rows=6)
    assert int(ctr.item()) == 2 and got_d.shape == (6, 4) and got_i.shape == (6, 8)
    assert got["c"][:, 0].sum() == 8                           # rows 6 and 7 have valid labels: counted
    check(got, got_d, got_i, ref, ref_d[:6], ref_i[:6], mu, logvar, labels, K, "cursor")


def test_argument_errors_return_minus_one_before_any_launch():
    """Validation runs without a device (as tests/test_abi.py's): non-null dummy addresses, nothing here launches."""
    from melo_gan_amd import _lib
    lib = _lib.load()
    q = 4096
    B, T, L, K = 4, 32, 8, 4
    need = lib.mg_vae_eval_acc_workspace_bytes(B, L)
    assert need == B * 26 * 8 and lib.mg_vae_eval_acc_words(K, L) == K * (26 + 5 * L)

    def call(**kw):
        a = dict(x=q, recon=q, B=B, T=T, C=4, mu=q, logvar=q, L=L, labels=q, K=K, acc=q, row_i=q, row_d=q, dst_rows=8, counter=q,
                 base=q, work=q, work_bytes=need, tick=None)
        a.update(kw)
        return lib.mg_vae_eval_acc(a["x"], a["recon"], a["B"], a["T"], a["C"], a["mu"], a["logvar"], a["L"], a["labels"], a["K"],
                                   a["acc"], a["row_i"], a["row_d"], a["dst_rows"], a["counter"], a["base"], a["work"],
                                   a["work_bytes"], a["tick"], None)

    assert call(C=8) == -1 and b"C = 8" in lib.mg_last_error()
    for bad_l in (0, 1025):
        assert call(L=bad_l) == -1 and b"latent width" in lib.mg_last_error()
        assert lib.mg_vae_eval_acc_words(K, bad_l) == 0 and lib.mg_vae_eval_acc_workspace_bytes(B, bad_l) == 0
    assert call(K=33) == -1 and b"classes" in lib.mg_last_error()
    assert lib.mg_vae_eval_acc_words(33, L) == 0
    assert call(work_bytes=need - 1) == -1 and b"workspace" in lib.mg_last_error()
    for name in ("x", "recon", "mu", "logvar", "labels", "acc", "row_i", "row_d", "counter", "base", "work"):
        assert call(**{name: None}) == -1 and b"null" in lib.mg_last_error(), name
    assert call(x=q + 4) == -1 and b"16-byte" in lib.mg_last_error()
    assert call(B=0) == -1 and call(T=0) == -1 and call(dst_rows=0) == -1
    assert lib.mg_vae_eval_acc_reset(None, K, L, None) == -1 and lib.mg_vae_eval_acc_reset(q, K, 0, None) == -1
