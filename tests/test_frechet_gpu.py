"""GPU: csrc/frechet.hip (mg_feat_moments, mg_sym_eig, mg_frechet_pairs) against numpy on the host.

Bounds are derived, not tuned; every test prints its figures before it asserts.
  moments      any summation order of n fp64 terms carries at most (n - 1) 2^-53 of the sum of magnitudes; one division follows:
                   |d mean_j| <= n 2^-53 sum_r |x_rj| / n.
               A centred value carries one rounding, a product of two centred values another, so
                   |d cov_ij| <= (n + 4) 2^-53 sum_r |xc_ri| |xc_rj| / (n - 1)
               plus what the mean's own error moves, (|d mean_i| sum_r |xc_rj| + |d mean_j| sum_r |xc_ri|) / (n - 1).  The reference
               is numpy in extended precision, whose own error is 2^-11 of these.
  eigenvalues  |d w| <= EIG_C D 2^-52 |A|_2 with EIG_C from tests/test_frechet_cpu.py (4 x the measured error of the numpy
               restatement); |A V - V diag(w)|_max and |A|_2 |V^T V - I|_max are held to the same figure.
  sqrt term    an eigenvalue mu of B moved by at most tau = EIG_C D 2^-52 |B|_2 moves its square root by at most sqrt(tau), and by
               tau / (2 sqrt(mu - tau)) away from zero:  sum_i min(sqrt(tau), tau / (2 sqrt(max(mu_i - tau, tiny)))).
  fd           twice that, plus the moment bounds of both sets carried into the mean and the trace term, plus four roundings of
               the final sum.
The reference of the distance is the nuclear-norm route (test_frechet_cpu.nuclear_fd): an SVD of the centred data's product, no
covariance, no eigensolver."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import ops  # noqa: E402
from melo_gan_amd.gan import feature_metrics as FM  # noqa: E402
from test_frechet_cpu import EIG_C, PSD_DIMS, eig_unit, nuclear_fd, random_psd, special_cases  # noqa: E402

U53, U52 = 2.0 ** -53, 2.0 ** -52
F64 = torch.float64
MOMENT_SHAPES = [(4, 2), (8, 40), (64, 257), (256, 70), (256, 600)]
PAIR_SHAPES = [(8, 40, 33), (64, 300, 257), (64, 40, 33), (256, 600, 520), (256, 100, 90), (16, 3, 2)]


def draw_sets(D, nA, nB):
    """As test_pair_metrics_gpu.draw_sets, with other centres and a wider spread on the second side."""
    rng = np.random.default_rng(1234)
    ca, cb = rng.standard_normal((4, D)), 0.5 + 1.5 * rng.standard_normal((4, D))
    A = (ca[rng.integers(0, 4, nA)] + 0.7 * rng.standard_normal((nA, D))).astype(np.float32)
    B = (cb[rng.integers(0, 4, nB)] + 1.3 * rng.standard_normal((nB, D))).astype(np.float32)
    return A, B


def bits(t):
    return t.cpu().contiguous().view(torch.int64) if t.dtype == F64 else t.cpu()


# ---------------------------------------------------------------------------------------------------------------------
# moments
# ---------------------------------------------------------------------------------------------------------------------
def device_moments(X):
    Xd = X if isinstance(X, torch.Tensor) else torch.from_numpy(X).cuda()
    D = Xd.shape[1]
    mean, cov = torch.full((D,), float("nan"), dtype=F64, device="cuda"), torch.full((D, D), float("nan"), dtype=F64, device="cuda")
    ops.feat_moments(Xd, mean, cov)
    return mean, cov


def moment_bounds(X):
    """(mean bound (D), cov bound (D, D)) of the module docstring, from fp64 magnitudes."""
    X = X.astype(np.float64)
    n = X.shape[0]
    mb = n * U53 * np.abs(X).sum(0) / n
    Xa = np.abs(X - X.mean(0))
    col = Xa.sum(0)
    cb = (n + 4) * U53 * (Xa.T @ Xa) / (n - 1) + (np.outer(mb, col) + np.outer(col, mb)) / (n - 1)
    return mb, cb


def moments_ref(X):
    X = X.astype(np.longdouble)
    mean = X.sum(0) / X.shape[0]
    Xc = X - mean
    return mean, (Xc.T @ Xc) / (X.shape[0] - 1)


@pytest.mark.parametrize("D,n", MOMENT_SHAPES)
def test_moments_against_numpy(D, n):
    X = draw_sets(D, n, 2)[0]
    mean, cov = (t.cpu().numpy() for t in device_moments(X))
    rm, rc = moments_ref(X)
    mb, cb = moment_bounds(X)
    em, ec = np.abs(mean - rm).astype(np.float64), np.abs(cov - rc).astype(np.float64)
    print(f"D {D}, n {n}: mean max err / bound {np.max(em / mb):.3g}; cov max err / bound {np.max(ec / cb):.3g} "
          f"(max |cov| {np.abs(cov).max():.3g}, max err {ec.max():.3g})")
    assert np.isfinite(mean).all() and np.isfinite(cov).all()
    assert (em <= mb).all() and (ec <= cb).all()
    assert np.array_equal(cov, cov.T)


def test_moments_of_equal_rows_are_exact():
    X = np.tile(np.random.default_rng(3).standard_normal((1, 12)).astype(np.float32), (37, 1))
    mean, cov = (t.cpu().numpy() for t in device_moments(X))
    assert np.array_equal(mean, X[0].astype(np.float64)) and not cov.any()


def test_moments_runs_and_replay_leave_identical_bits():
    D, n = 64, 257
    Xd = torch.from_numpy(draw_sets(D, n, 2)[0]).cuda()
    first, second = [bits(t) for t in device_moments(Xd)], [bits(t) for t in device_moments(Xd)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        device_moments(Xd)                               # this stream's workspace exists before the capture
        torch.cuda.synchronize()
        outs = (torch.full((D,), float("nan"), dtype=F64, device="cuda"), torch.full((D, D), float("nan"), dtype=F64, device="cuda"))
        gr = ops.Graph()
        gr.begin()
        try:
            ops.feat_moments(Xd, *outs)
        finally:
            gr.end()
        gr.launch()
    torch.cuda.synchronize()
    for a, b, c in zip(first, second, outs):
        assert torch.equal(a, b) and torch.equal(a, bits(c))


# ---------------------------------------------------------------------------------------------------------------------
# the eigensolver
# ---------------------------------------------------------------------------------------------------------------------
def device_eig(mats, vectors=True):
    A = torch.from_numpy(np.stack(mats)).cuda()
    batch, D = A.shape[0], A.shape[1]
    w = torch.full((batch, D), float("nan"), dtype=F64, device="cuda")
    V = torch.full((batch, D, D), float("nan"), dtype=F64, device="cuda") if vectors else None
    info = torch.full((batch, 2), -1, dtype=torch.int32, device="cuda")
    ops.sym_eig(A, w, V, info)
    return w.cpu().numpy(), (V.cpu().numpy() if vectors else None), info.cpu().numpy()


def check_eig(name, A, w, V, info):
    D, unit = A.shape[0], eig_unit(A)
    ref = np.linalg.eigvalsh(A)
    norm2 = float(np.abs(ref).max())
    ratio = float(np.abs(w - ref).max()) / unit if unit > 0 else float(np.abs(w - ref).max())
    resid = float(np.abs(A @ V - V * w).max()) / unit if unit > 0 else 0.0
    orth = float(np.abs(V.T @ V - np.eye(D)).max()) / (D * U52)
    print(f"{name}: D {D}, sweeps {info[0]}, converged {info[1]}, |dw| {ratio:.3f}, |AV - Vw| {resid:.3f}, |V^T V - I| {orth:.3f} "
          f"of D 2^-52 |A|_2 (|A|_2 {norm2:.3g}); bound {EIG_C}")
    assert info[1] == 1 and 1 <= info[0] <= FM.EIG_MAX_SWEEPS
    assert np.all(np.diff(w) >= 0)
    assert ratio <= EIG_C and resid <= EIG_C and orth <= EIG_C


def test_sym_eig_special_matrices_in_one_batch():
    cases = special_cases()
    w, V, info = device_eig([A for _, A in cases])
    for i, (name, A) in enumerate(cases):
        check_eig(name, A, w[i], V[i], info[i])
    assert len(set(info[:, 0].tolist())) >= 3            # the members end after different numbers of sweeps
    by = {name: i for i, (name, _) in enumerate(cases)}
    D = cases[0][1].shape[0]
    assert np.array_equal(w[by["diagonal"]], np.linspace(-2.0, 9.0, D)) and info[by["diagonal"], 0] == 1
    assert np.array_equal(w[by["c * I"]], np.full(D, 3.5))
    assert np.array_equal(w[by["offdiag 1e-300"]], np.arange(1.0, D + 1.0))
    # values only: the same eigenvalues, bit for bit
    w0, _, info0 = device_eig([A for _, A in cases], vectors=False)
    assert np.array_equal(w0, w) and np.array_equal(info0, info)


@pytest.mark.parametrize("D", PSD_DIMS)
def test_sym_eig_random_psd(D):
    A, A2 = random_psd(D, 100 + D), 3.0 * random_psd(D, 900 + D)
    w, V, info = device_eig([A, A2])
    check_eig(f"psd {D}", A, w[0], V[0], info[0])
    check_eig(f"psd {D} (second member)", A2, w[1], V[1], info[1])
    if D == 1:                                           # exact: the entry itself
        assert w[0, 0] == A[0, 0] and V[0, 0, 0] == 1.0 and w[1, 0] == A2[0, 0]
    if D == 2:                                           # the closed form, to the rounding of its own square root
        tr, det = A[0, 0] + A[1, 1], A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
        closed = tr / 2 + np.array([-1.0, 1.0]) * np.sqrt(((A[0, 0] - A[1, 1]) / 2) ** 2 + A[0, 1] ** 2)
        print(f"D 2: device {w[0]}, closed form {closed}, det {det}")
        assert np.abs(w[0] - closed).max() <= 4 * U52 * np.abs(closed).max()
        wd = device_eig([np.diag([2.0, -3.0])])[0][0]
        assert np.array_equal(wd, [-3.0, 2.0])


def test_sym_eig_runs_and_replay_leave_identical_bits():
    A = torch.from_numpy(np.stack([random_psd(64, 5), random_psd(64, 6)])).cuda()

    def run(w, V, info):
        ops.sym_eig(A, w, V, info)
        return w, V, info

    new = lambda: (torch.full((2, 64), float("nan"), dtype=F64, device="cuda"),  # noqa: E731
                   torch.full((2, 64, 64), float("nan"), dtype=F64, device="cuda"),
                   torch.full((2, 2), -1, dtype=torch.int32, device="cuda"))
    first, second = [bits(t) for t in run(*new())], [bits(t) for t in run(*new())]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        run(*new())
        torch.cuda.synchronize()
        outs = new()
        gr = ops.Graph()
        gr.begin()
        try:
            run(*outs)
        finally:
            gr.end()
        gr.launch()
    torch.cuda.synchronize()
    for a, b, c in zip(first, second, outs):
        assert torch.equal(a, b) and torch.equal(a, bits(c))


# ---------------------------------------------------------------------------------------------------------------------
# the pairs
# ---------------------------------------------------------------------------------------------------------------------
def device_pairs(sets, pairs):
    """Moments of every set on the device, then one mg_frechet_pairs; returns (out, spectrum, info, means, covs) on the host."""
    S, D, P = len(sets), sets[0].shape[1], len(pairs)
    means, covs = torch.empty(S, D, dtype=F64, device="cuda"), torch.empty(S, D, D, dtype=F64, device="cuda")
    for i, X in enumerate(sets):
        ops.feat_moments(torch.from_numpy(X).cuda(), means[i], covs[i])
    out = torch.full((P, 4), float("inf"), dtype=F64, device="cuda")
    spectrum = torch.full((S, 3), float("inf"), dtype=F64, device="cuda")
    info = torch.full((S + P, 2), -1, dtype=torch.int32, device="cuda")
    ops.frechet_pairs(means, covs, torch.tensor(pairs, dtype=torch.int32).cuda(), out, spectrum, info)
    return tuple(t.cpu().numpy() for t in (out, spectrum, info, means, covs))


def sqrt_tolerance(X, Y):
    """The sqrt-term tolerance of the module docstring from B's true eigenvalues: the squared singular values of the centred
    product, padded with zeros to D."""
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    D = X.shape[1]
    s = np.linalg.svd((X - X.mean(0)) @ (Y - Y.mean(0)).T, compute_uv=False) / np.sqrt((len(X) - 1.0) * (len(Y) - 1.0))
    mu = np.zeros(D)
    mu[:min(D, len(s))] = (s * s)[:D]
    tau = EIG_C * D * U52 * mu.max()
    return float(np.minimum(np.sqrt(tau), tau / (2.0 * np.sqrt(np.maximum(mu - tau, np.finfo(np.float64).tiny)))).sum())


def fd_tolerance(X, Y, ref):
    (mbx, cbx), (mby, cby) = moment_bounds(X), moment_bounds(Y)
    dm = np.abs(X.astype(np.float64).mean(0) - Y.astype(np.float64).mean(0))
    moment = float(np.trace(cbx) + np.trace(cby) + (2.0 * dm * (mbx + mby)).sum())
    return 2.0 * sqrt_tolerance(X, Y) + moment + 4 * U53 * (ref[1] + ref[2] + 2.0 * ref[3])


def spectrum_tolerance(cov):
    """What eigenvalues within tau = EIG_C D 2^-52 |S|_2 of the true ones can move the three statistics by, to first order and
    doubled: the total moves by at most D tau, the sum of squares by 2 tau sum w, a share p by pt = 2 D tau / sum w, and a share's
    -p ln p by pt (|ln max(p, pt)| + 1)."""
    w = np.maximum(np.linalg.eigvalsh(cov), 0.0)
    D, total = len(w), w.sum()
    want = FM.spectrum_stats(w)
    tau = EIG_C * D * U52 * w.max()
    pt = 2.0 * D * tau / total
    dH = float((pt * (np.abs(np.log(np.maximum(w / total, pt))) + 1.0)).sum())
    return {"participation_ratio": 2.0 * want["participation_ratio"] * (2.0 * D * tau / total + 2.0 * tau * total / (w * w).sum()),
            "effective_rank": 2.0 * want["effective_rank"] * dH, "top1_share": 2.0 * (tau + want["top1_share"] * D * tau) / total}


@pytest.mark.parametrize("D,m,n", PAIR_SHAPES)
def test_frechet_pairs_against_the_nuclear_norm_route(D, m, n):
    X, Y = draw_sets(D, m, n)
    out, spectrum, info, means, covs = device_pairs([X, Y], [(0, 1), (1, 0), (0, 0), (1, 1)])
    print(f"D {D}, m {m}, n {n}: sweeps {info[:, 0].tolist()}, converged {info[:, 1].tolist()}")
    assert (info[:, 1] == 1).all() and (info[:, 0] <= FM.EIG_MAX_SWEEPS).all()
    refs = {(0, 1): (X, Y), (1, 0): (Y, X), (0, 0): (X, X), (1, 1): (Y, Y)}
    for row, (pair, (P_, Q_)) in zip(out, refs.items()):
        ref = nuclear_fd(P_, Q_)
        st, ft = sqrt_tolerance(P_, Q_), fd_tolerance(P_, Q_, ref)
        print(f"  pair {pair}: fd {row[0]:.12g} (ref {ref[0]:.12g}, |err| {abs(row[0] - ref[0]):.3g}, tol {ft:.3g}); sqrt term "
              f"{row[3]:.12g} (ref {ref[3]:.12g}, |err| {abs(row[3] - ref[3]):.3g}, tol {st:.3g}); mean {row[1]:.6g} trace {row[2]:.6g}")
    for row, (pair, (P_, Q_)) in zip(out, refs.items()):
        ref = nuclear_fd(P_, Q_)
        st, ft = sqrt_tolerance(P_, Q_), fd_tolerance(P_, Q_, ref)
        assert abs(row[3] - ref[3]) <= st, pair
        assert abs(row[0] - ref[0]) <= ft, pair
        assert abs(row[1] - ref[1]) <= ft and abs(row[2] - ref[2]) <= ft, pair
        assert row[0] == row[1] + row[2] - 2.0 * row[3], pair
    # fd(X, X) is 0 within its tolerance; the distance is symmetric within the two tolerances
    assert abs(out[2][0]) <= fd_tolerance(X, X, nuclear_fd(X, X)) and abs(out[3][0]) <= fd_tolerance(Y, Y, nuclear_fd(Y, Y))
    assert abs(out[0][0] - out[1][0]) <= fd_tolerance(X, Y, nuclear_fd(X, Y)) + fd_tolerance(Y, X, nuclear_fd(Y, X))
    # the spectrum of each covariance against eigvalsh of that covariance
    for i in range(2):
        want, tol = FM.spectrum_stats(np.linalg.eigvalsh(covs[i])), spectrum_tolerance(covs[i])
        for j, key in enumerate(FM.SPECTRUM_KEYS):
            print(f"  set {i} {key}: {spectrum[i][j]:.12g} (ref {want[key]:.12g}, |err| {abs(spectrum[i][j] - want[key]):.3g}, "
                  f"tol {tol[key]:.3g})")
            assert abs(spectrum[i][j] - want[key]) <= tol[key], (i, key)


def test_frechet_pairs_of_constant_sets():
    D = 8
    X, Y = draw_sets(D, 20, 20)
    c1, c2 = np.tile(X[:1], (5, 1)), np.tile(Y[:1], (9, 1))
    out, spectrum, info, means, covs = device_pairs([c1, c2, Y], [(0, 1), (0, 2), (2, 0), (9, 0)])
    assert not covs[0].any() and not covs[1].any()
    assert np.isnan(spectrum[0]).all() and np.isnan(spectrum[1]).all() and np.isfinite(spectrum[2]).all()
    mean_term = float(((X[0].astype(np.float64) - Y[0].astype(np.float64)) ** 2).sum())
    assert out[0][3] == 0.0 and out[0][2] == 0.0 and out[0][0] == out[0][1] and abs(out[0][1] - mean_term) <= 4 * D * U53 * mean_term
    # against a general set: the mean term plus that set's trace, from either side
    for row in out[1:3]:
        assert row[3] == 0.0 and row[0] == row[1] + row[2] and abs(row[2] - np.trace(covs[2])) <= D * U53 * np.trace(covs[2])
    assert np.isnan(out[3]).all()                        # a pair that names no set
    block = FM.frechet_block(D, ["a"], [5], {"whole": tuple(out[0]), "ef": [[tuple(out[3])]]},
                             {"real": tuple(spectrum[0]), "fake": tuple(spectrum[1]), "real_e": [None], "fake_e": [None]})
    assert block["frechet"]["fd"] == out[0][1] and block["spectrum"]["real"] == dict.fromkeys(FM.SPECTRUM_KEYS)
    assert block["fd_matrix"] == {"a": {"a": None}}


def test_frechet_pairs_runs_and_replay_leave_identical_bits():
    D = 16
    X, Y = draw_sets(D, 40, 33)
    means, covs = torch.empty(2, D, dtype=F64, device="cuda"), torch.empty(2, D, D, dtype=F64, device="cuda")
    for i, Z in enumerate((X, Y)):
        ops.feat_moments(torch.from_numpy(Z).cuda(), means[i], covs[i])
    pairs = torch.tensor([(0, 1), (1, 0)], dtype=torch.int32).cuda()
    new = lambda: (torch.full((2, 4), float("nan"), dtype=F64, device="cuda"),  # noqa: E731
                   torch.full((2, 3), float("nan"), dtype=F64, device="cuda"), torch.full((4, 2), -1, dtype=torch.int32, device="cuda"))
    run = lambda o: ops.frechet_pairs(means, covs, pairs, *o)  # noqa: E731
    first, second = [bits(t) for t in run(new())], [bits(t) for t in run(new())]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        run(new())
        torch.cuda.synchronize()
        outs = new()
        gr = ops.Graph()
        gr.begin()
        try:
            run(outs)
        finally:
            gr.end()
        gr.launch()
    torch.cuda.synchronize()
    for a, b, c in zip(first, second, outs):
        assert torch.equal(a, b) and torch.equal(a, bits(c))


def test_ops_refuse_bad_shapes():
    z = lambda *s, dt=F64: torch.zeros(*s, dtype=dt, device="cuda")  # noqa: E731
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.feat_moments(z(8, 6, dt=torch.float32), z(6), z(6, 6))
    with pytest.raises(ValueError, match="rows"):
        ops.feat_moments(z(1, 8, dt=torch.float32), z(8), z(8, 8))
    with pytest.raises(ValueError, match="aligned"):
        ops.feat_moments(z(9, 8, dt=torch.float32).flatten()[1:65].view(8, 8), z(8), z(8, 8))
    with pytest.raises(ValueError, match="cov"):
        ops.feat_moments(z(8, 8, dt=torch.float32), z(8), z(8, 7))
    with pytest.raises(ValueError, match="batch, D, D"):
        ops.sym_eig(z(2, 4, 5), z(2, 4))
    with pytest.raises(ValueError, match="1..256"):
        ops.sym_eig(z(1, 257, 257), z(1, 257))
    with pytest.raises(ValueError, match="pairs"):
        ops.frechet_pairs(z(2, 4), z(2, 4, 4), z(1, 3, dt=torch.int32), z(1, 4), z(2, 3), z(3, 2, dt=torch.int32))
    with pytest.raises(ValueError, match="info"):
        ops.frechet_pairs(z(2, 4), z(2, 4, 4), z(1, 2, dt=torch.int32), z(1, 4), z(2, 3), z(2, 2, dt=torch.int32))
    with pytest.raises(ValueError, match="work"):
        ops.sym_eig(z(1, 8, 8), z(1, 8), work=torch.zeros(64, dtype=torch.uint8, device="cuda"))
    assert ops.frechet_workspace(2048, 256, 10, 17, "cuda").numel() >= 17 * 2 * 256 * 256 * 8
