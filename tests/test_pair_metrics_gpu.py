"""GPU: the pairwise feature-space kernels (csrc/pair_metrics.hip: mg_pair_ksum, mg_pair_knn, mg_pair_margin) against numpy in
fp64 on the host, and mg_scatter_rows_cursor against torch indexing.

Tolerances are derived, not tuned.  With u = 2^-24, first-order rounding of the three dot products (|a|^2, |b|^2, a . b, D terms
each, any accumulation order) and of the combining operations gives
    |delta d2_ij| <= (2 D + 8) u (|a_i|^2 + |b_j|^2 + r2_j)
and sorted order statistics and row minima are 1-Lipschitz in the sup norm, so the k sorted values of mg_pair_knn and the
values of mg_pair_margin are held to that bound taken at the row-norm maxima.  The sum of mg_pair_ksum (fp64 arithmetic on
the fp32 g_ij: the derivative of the cube times g's error) is held to 2 * 3 u sum_ij (|g_ij| / D + 1)^2 |a_i| |b_j|."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import ops  # noqa: E402

U = 2.0 ** -24
SHAPES = [(4, 5, 9, 1), (32, 65, 130, 3), (32, 193, 70, 3), (16, 70, 193, 3), (256, 193, 70, 3), (256, 64, 64, 8), (4, 1, 1, 1)]


def draw_sets(D, nA, nB):
    rng = np.random.default_rng(1234)
    centres = rng.standard_normal((4, D))
    A = (centres[rng.integers(0, 4, nA)] + 0.7 * rng.standard_normal((nA, D))).astype(np.float32)
    B = (centres[rng.integers(0, 4, nB)] + 0.7 * rng.standard_normal((nB, D))).astype(np.float32)
    return A, B


def d2_ref(A, B, exclude_self=False):
    A, B = A.astype(np.float64), B.astype(np.float64)
    d2 = np.maximum((A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * (A @ B.T), 0.0)
    if exclude_self:
        np.fill_diagonal(d2, np.inf)
    return d2


def d2_bound(A, B, r2=0.0):
    D = A.shape[1]
    na, nb = (A.astype(np.float64) ** 2).sum(1).max(), (B.astype(np.float64) ** 2).sum(1).max()
    return (2 * D + 8) * U * (na + nb + float(np.max(r2)))


def ksum_ref(A, B, exclude_diag=False):
    A, B = A.astype(np.float64), B.astype(np.float64)
    g = A @ B.T
    D = A.shape[1]
    w = np.ones_like(g)
    if exclude_diag:
        np.fill_diagonal(w, 0.0)
    ref = float((w * (g / D + 1.0) ** 3).sum())
    norms = np.sqrt((A * A).sum(1))[:, None] * np.sqrt((B * B).sum(1))[None, :]
    return ref, 2 * 3 * U * float((w * (np.abs(g) / D + 1.0) ** 2 * norms).sum())


def run_ksum(A, B, exclude_diag=False):
    out = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    ops.pair_ksum(A, A if B is None else B, out, exclude_diag=exclude_diag)
    return out


def run_knn(A, B, k, exclude_self=False):
    out = torch.full((A.shape[0], k), float("nan"), device="cuda")
    ops.pair_knn(A, A if B is None else B, out, exclude_self=exclude_self)
    return out


def run_margin(A, B, r2):
    out = torch.full((A.shape[0],), float("nan"), device="cuda")
    ops.pair_margin(A, B, r2, out)
    return out


@pytest.mark.parametrize("D,nA,nB,k", SHAPES)
def test_pair_kernels_match_fp64(D, nA, nB, k):
    A, B = draw_sets(D, nA, nB)
    Ad, Bd = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    # kernel sum
    ref, bound = ksum_ref(A, B)
    got = float(run_ksum(Ad, Bd).cpu())
    print(f"ksum: {got:.12g} (fp64 {ref:.12g}), |err| {abs(got - ref):.3g}, bound {bound:.3g}")
    assert abs(got - ref) <= bound
    # k nearest
    d2 = d2_ref(A, B)
    if k <= nB:
        want = np.sort(d2, axis=1)[:, :k]
        got = run_knn(Ad, Bd, k).cpu().numpy().astype(np.float64)
        bound = d2_bound(A, B)
        print(f"knn: max |err| {np.abs(got - want).max():.3g}, bound {bound:.3g}")
        assert np.isfinite(got).all() and (got >= 0).all() and (np.diff(got, axis=1) >= 0).all()
        assert np.abs(got - want).max() <= bound
    # margin against B's own k-NN radii (fp64 reference radii, handed to the kernel in fp32)
    if nB > k:
        r2 = np.sort(d2_ref(B, B, exclude_self=True), axis=1)[:, k - 1].astype(np.float32)
    else:
        r2 = np.full(nB, 0.5, dtype=np.float32)
    want = (d2 - r2.astype(np.float64)[None, :]).min(1)
    got = run_margin(Ad, Bd, torch.from_numpy(r2).cuda()).cpu().numpy().astype(np.float64)
    bound = d2_bound(A, B, r2)
    print(f"margin: max |err| {np.abs(got - want).max():.3g}, bound {bound:.3g}")
    assert np.abs(got - want).max() <= bound
    clear = np.abs(want) > 2 * bound
    print(f"membership: {int((~clear).sum())} of {nA} rows ambiguous, {int((want <= 0).sum())} inside")
    assert (~clear).sum() <= 0.02 * nA
    assert np.array_equal((got <= 0)[clear], (want <= 0)[clear])


@pytest.mark.parametrize("n", [9, 65, 130])
def test_self_sets_duplicates_and_the_excluded_column(n):
    D = 32
    X, _ = draw_sets(D, n, 1)
    X[2::3] = X[1::3][:len(X[2::3])]                     # every third row is a copy of the row before it
    dup = np.zeros(n, dtype=bool)
    dup[2::3] = True
    dup[1::3][:len(X[2::3])] = True
    Xd = torch.from_numpy(X).cuda()
    d2 = d2_ref(X, X, exclude_self=True)
    bound = d2_bound(X, X)
    for k in sorted({1, 3, min(n - 1, 8)}):
        want = np.sort(d2, axis=1)[:, :k]
        got = run_knn(Xd, None, k, exclude_self=True).cpu().numpy().astype(np.float64)
        print(f"n {n} k {k}: max |err| {np.abs(got - want).max():.3g}, bound {bound:.3g}")
        assert np.abs(got - want).max() <= bound
        assert (got >= 0).all()                          # clamped, never negative
        assert (got[dup, 0] == 0).all()                  # a copy's distance: the norms follow the Gram chain, exactly 0
        assert (got[~dup, 0] > 2 * bound).all()          # a row's own zero does not appear
    ref, kb = ksum_ref(X, X, exclude_diag=True)
    got = float(run_ksum(Xd, None, exclude_diag=True).cpu())
    assert abs(got - ref) <= kb
    full, _ = ksum_ref(X, X)
    assert abs(float(run_ksum(Xd, None).cpu()) - full) <= kb and abs(full - ref) > 10 * kb     # the diagonal is worth seeing
    # without the exclusion every row finds itself
    assert (run_knn(Xd, None, 1).cpu().numpy() == 0).all()


def test_k_up_to_the_candidate_count():
    X, Y = draw_sets(8, 5, 4)
    Xd, Yd = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    got = run_knn(Xd, None, 4, exclude_self=True).cpu().numpy().astype(np.float64)          # k = n - 1
    assert np.abs(got - np.sort(d2_ref(X, X, exclude_self=True), axis=1)[:, :4]).max() <= d2_bound(X, X)
    got = run_knn(Xd, Yd, 4).cpu().numpy().astype(np.float64)                                # k = nB
    assert np.abs(got - np.sort(d2_ref(X, Y), axis=1)).max() <= d2_bound(X, Y)
    with pytest.raises(ValueError, match="candidates"):
        run_knn(Xd, None, 5, exclude_self=True)                                              # k = n
    with pytest.raises(ValueError, match="candidates"):
        run_knn(Xd, Yd, 5)
    with pytest.raises(ValueError, match="same array"):
        run_knn(Xd, Xd.clone(), 2, exclude_self=True)
    with pytest.raises(ValueError):
        run_knn(Xd, None, 9)
    with pytest.raises(ValueError):
        run_knn(Xd[:, :6].contiguous(), None, 1)                                             # D = 6


def test_many_tiles_one_per_workgroup():
    """5 row tiles x 17 column tiles at D = 64 (two LDS chunks): every workgroup takes one column tile (17 runs of 1), and the
    fold merges 17 lists per row."""
    A, B = draw_sets(64, 300, 1030)
    Ad, Bd = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    d2 = d2_ref(A, B)
    got = run_knn(Ad, Bd, 8).cpu().numpy().astype(np.float64)
    assert np.abs(got - np.sort(d2, axis=1)[:, :8]).max() <= d2_bound(A, B)
    got = run_knn(Ad, Bd, 1).cpu().numpy().astype(np.float64)
    assert np.abs(got[:, 0] - d2.min(1)).max() <= d2_bound(A, B)
    ref, kb = ksum_ref(A, B)
    assert abs(float(run_ksum(Ad, Bd).cpu()) - ref) <= kb


def smallest(d2, k):
    return np.sort(np.partition(d2, k - 1, axis=1)[:, :k], axis=1)


def test_workgroups_that_walk_several_column_tiles():
    """The layouts at which a workgroup carries its lists and its sum over a RUN of column tiles -- what the primitive is for
    (4096 rows: runs of 4; 16384: runs of 64).  The planner deals a row tile's ntB column tiles in runs of
    per = cdiv(ntB, min(cdiv(1024, ntA), ntB)):
      nA = 1088, nB = 71 * 64 - 5:  ntA = 17, ntB = 71 -> 36 runs of 2, the last run one tile, the last tile 59 columns
      n = 2100 against itself:       ntA = ntB = 33   -> 17 runs of 2, the last run one tile; the self column sits in every
                                     row tile's own run, first or second tile
    D = 8 keeps the fp64 reference cheap."""
    D, nA, nB = 8, 1088, 71 * 64 - 5
    A, B = draw_sets(D, nA, nB)
    Ad, Bd = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    d2, bound = d2_ref(A, B), d2_bound(A, B)
    for k in (8, 1):
        got = run_knn(Ad, Bd, k).cpu().numpy().astype(np.float64)
        print(f"knn k {k}: max |err| {np.abs(got - smallest(d2, k)).max():.3g}, bound {bound:.3g}")
        assert np.abs(got - smallest(d2, k)).max() <= bound
    r2 = smallest(d2_ref(B, B, exclude_self=True), 3)[:, 2].astype(np.float32)
    want = (d2 - r2.astype(np.float64)[None, :]).min(1)
    got = run_margin(Ad, Bd, torch.from_numpy(r2).cuda()).cpu().numpy().astype(np.float64)
    mb = d2_bound(A, B, r2)
    print(f"margin: max |err| {np.abs(got - want).max():.3g}, bound {mb:.3g}")
    assert np.abs(got - want).max() <= mb
    clear = np.abs(want) > 2 * mb
    assert (~clear).sum() <= 0.02 * nA and np.array_equal((got <= 0)[clear], (want <= 0)[clear])
    ref, kb = ksum_ref(A, B)
    got = float(run_ksum(Ad, Bd).cpu())
    print(f"ksum: |err| {abs(got - ref):.3g}, bound {kb:.3g}")
    assert abs(got - ref) <= kb
    # a set against itself, a row's own column left out
    n = 2100
    X, _ = draw_sets(D, n, 1)
    X[2::3] = X[1::3][:len(X[2::3])]
    dup = np.zeros(n, dtype=bool)
    dup[2::3] = True
    dup[1::3][:len(X[2::3])] = True
    Xd = torch.from_numpy(X).cuda()
    d2, bound = d2_ref(X, X, exclude_self=True), d2_bound(X, X)
    for k in (8, 1):
        got = run_knn(Xd, None, k, exclude_self=True).cpu().numpy().astype(np.float64)
        print(f"self-set k {k}: max |err| {np.abs(got - smallest(d2, k)).max():.3g}, bound {bound:.3g}")
        assert np.abs(got - smallest(d2, k)).max() <= bound
        assert (got >= 0).all() and (got[dup, 0] == 0).all() and (got[~dup, 0] > 0).all()
    ref, kb = ksum_ref(X, X, exclude_diag=True)
    assert abs(float(run_ksum(Xd, None, exclude_diag=True).cpu()) - ref) <= kb
    full, _ = ksum_ref(X, X)
    assert abs(full - ref) > 10 * kb


def test_runs_and_replay_leave_identical_bits():
    D, nA, nB, k = 32, 193, 70, 3
    A, B = draw_sets(D, nA, nB)
    Ad, Bd = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    r2 = torch.rand(nB, device="cuda") * 20

    def run():
        return run_ksum(Ad, Bd), run_knn(Ad, Bd, k), run_margin(Ad, Bd, r2), run_knn(Bd, None, k, exclude_self=True)

    first = [t.cpu() for t in run()]
    second = [t.cpu() for t in run()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        run()                                            # this stream's workspace exists before the capture
        torch.cuda.synchronize()
        outs = (torch.full((1,), float("nan"), dtype=torch.float64, device="cuda"), torch.full((nA, k), float("nan"), device="cuda"),
                torch.full((nA,), float("nan"), device="cuda"), torch.full((nB, k), float("nan"), device="cuda"))
        gr = ops.Graph()
        gr.begin()
        try:
            ops.pair_ksum(Ad, Bd, outs[0])
            ops.pair_knn(Ad, Bd, outs[1])
            ops.pair_margin(Ad, Bd, r2, outs[2])
            ops.pair_knn(Bd, Bd, outs[3], exclude_self=True)
        finally:
            gr.end()
        gr.launch()
    torch.cuda.synchronize()
    for a, b, c in zip(first, second, outs):
        assert torch.equal(a, b) and torch.equal(a, c.cpu())


def test_scatter_rows_cursor_matches_torch_indexing():
    rows, width, dst_rows = 8, 12, 22
    src = torch.randn(rows, width, device="cuda")
    i64 = lambda v: torch.full((1,), v, dtype=torch.int64, device="cuda")  # noqa: E731
    for batch in (1, 2):                                 # a cursor in the middle; the last batch hangs over the end by 2 rows
        dst = torch.full((dst_rows, width), -7.0, device="cuda")
        ops.scatter_rows_cursor(src, dst, i64(batch + 5), i64(5))
        want = torch.full((dst_rows, width), -7.0)
        m = min(rows, dst_rows - batch * rows)
        want[batch * rows:batch * rows + m] = src[:m].cpu()
        assert torch.equal(dst.cpu(), want), batch
    dst = torch.full((dst_rows, width), -7.0, device="cuda")
    ops.scatter_rows_cursor(src, dst, i64(3), i64(0))   # wholly past the end: nothing is written
    assert (dst == -7.0).all()
    with pytest.raises(ValueError):
        ops.scatter_rows_cursor(src, torch.zeros(dst_rows, width + 1, device="cuda"), i64(0), i64(0))
