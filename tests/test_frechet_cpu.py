"""CPU-only: the host arithmetic of evaluate --frechet (melo_gan_amd/gan/feature_metrics.py): the Frechet distance from
moments against closed forms and against the independent nuclear-norm route, the numpy restatement of the device's Jacobi
eigensolver against np.linalg.eigvalsh, the spectrum statistics and the report block by hand, the opt-in, and the argument
checks that need no launch.

The eigenvalue bound used here and in tests/test_frechet_gpu.py is
    |delta w| <= EIG_C * D * 2^-52 * |A|_2.
EIG_C is set here: the worst ratio  max |w_host - w_eigvalsh| / (D 2^-52 |A|_2)  of host_sym_eig over eig_cases() was measured
as 0.288 (the random PSD matrix at D = 3; the 12 x 12 special matrices give up to 0.247, D = 64 gives 0.125, D = 255 0.086 and
D = 256 0.058), and a factor 4 is given for the device's different but equally valid summation order: 4 * 0.288 = 1.15,
rounded up to EIG_C = 1.2.  |A V - V diag(w)|_max and |A|_2 |V^T V - I|_max are held to the same figure, here and on the device."""
import json
import os

import numpy as np
import pytest

import melo_gan_amd  # noqa: F401
from melo_gan_amd.gan import feature_metrics as FM

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EIG_C = 1.2
EIG_MEASURED_RATIO = 0.288
U52 = 2.0 ** -52
PSD_DIMS = (1, 2, 3, 5, 64, 255, 256)
SPECIAL_D = 12


def random_psd(D, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((2 * D + 3, D))
    return X.T @ X / (2 * D + 2)


def special_cases():
    """Six symmetric 12 x 12 matrices that end after different numbers of sweeps."""
    D = SPECIAL_D
    rng = np.random.default_rng(77)
    Q = np.linalg.qr(rng.standard_normal((D, D)))[0]
    v = rng.standard_normal(D)
    G = rng.standard_normal((D, D))
    tiny = np.diag(np.arange(1.0, D + 1.0)) + 1e-300 * (1.0 - np.eye(D))
    cluster = (Q * np.array([1.0] * 5 + [2.0] + [5.0] * 4 + [7.0, 9.0])) @ Q.T
    return [("diagonal", np.diag(np.linspace(-2.0, 9.0, D))), ("c * I", 3.5 * np.eye(D)), ("rank 1", np.outer(v, v)),
            ("indefinite", 0.5 * (G + G.T)), ("cluster", 0.5 * (cluster + cluster.T)), ("offdiag 1e-300", tiny)]


def eig_cases():
    return special_cases() + [(f"psd {D}", random_psd(D, 100 + D)) for D in PSD_DIMS]


def eig_unit(A):
    """D 2^-52 |A|_2: the bound is EIG_C of these."""
    return A.shape[0] * U52 * float(np.abs(np.linalg.eigvalsh(A)).max())


@pytest.fixture(scope="module")
def solved():
    return [(name, A) + FM.host_sym_eig(A) for name, A in eig_cases()]


# ---------------------------------------------------------------------------------------------------------------------
# frechet_from_moments
# ---------------------------------------------------------------------------------------------------------------------
def draw(D, m, n, seed=5):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((m, D)) * rng.uniform(0.3, 2.0, D) + rng.standard_normal(D)).astype(np.float32)
    Y = (rng.standard_normal((n, D)) @ rng.standard_normal((D, D)) * 0.4 + 0.5).astype(np.float32)
    return X, Y


def nuclear_sqrt_term(X, Y):
    """tr (Sx Sy)^(1/2) = |Xc Yc^T|_* / sqrt((m - 1)(n - 1)), by np.linalg.svd of the centred data: no covariance is formed."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    Xc, Yc = X - X.mean(0), Y - Y.mean(0)
    return float(np.linalg.svd(Xc @ Yc.T, compute_uv=False).sum()) / np.sqrt((len(X) - 1.0) * (len(Y) - 1.0))


def nuclear_fd(X, Y):
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    Xc, Yc = X - X.mean(0), Y - Y.mean(0)
    mean_term = float(((X.mean(0) - Y.mean(0)) ** 2).sum())
    trace_term = float((Xc * Xc).sum() / (len(X) - 1) + (Yc * Yc).sum() / (len(Y) - 1))
    root = nuclear_sqrt_term(X, Y)
    return mean_term + trace_term - 2.0 * root, mean_term, trace_term, root


def test_frechet_closed_forms():
    X, Y = draw(6, 40, 30)
    m1, S1 = FM.host_moments(X)
    m2, S2 = FM.host_moments(Y)
    scale = np.trace(S1) + np.trace(S2)
    assert abs(FM.frechet_from_moments(m1, S1, m1, S1)) <= 1e-13 * scale
    # D = 1: (m1 - m2)^2 + (s1 - s2)^2 in standard deviations
    assert FM.frechet_from_moments([1.5], [[4.0]], [-0.5], [[9.0]]) == pytest.approx(2.0 ** 2 + (2.0 - 3.0) ** 2, abs=1e-13)
    # commuting diagonal covariances
    a, b = np.array([4.0, 1.0, 0.25, 0.0]), np.array([1.0, 9.0, 0.25, 2.0])
    d = np.array([0.5, -1.0, 0.0, 2.0])
    want = float((d * d).sum() + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum())
    assert FM.frechet_from_moments(d, np.diag(a), np.zeros(4), np.diag(b)) == pytest.approx(want, abs=1e-12)
    # symmetry
    assert FM.frechet_from_moments(m1, S1, m2, S2) == pytest.approx(FM.frechet_from_moments(m2, S2, m1, S1), abs=1e-11 * scale)


@pytest.mark.parametrize("D,m,n", [(8, 40, 33), (16, 3, 2), (24, 10, 60)])
def test_frechet_agrees_with_the_nuclear_norm_route(D, m, n):
    X, Y = draw(D, m, n)
    got = FM.frechet_terms(*FM.host_moments(X), *FM.host_moments(Y))
    want = nuclear_fd(X, Y)
    print(f"D {D}, m {m}, n {n}: terms {got}, nuclear route {want}")
    # a rank-deficient product has eigenvalues of rounding size whose square roots are 1e-8 of the scale
    tol = (1e-10 if min(m, n) > D else 1e-5) * want[2]
    for g, w in zip(got, want):
        assert abs(g - w) <= tol


# ---------------------------------------------------------------------------------------------------------------------
# host_sym_eig
# ---------------------------------------------------------------------------------------------------------------------
def test_host_sym_eig_against_eigvalsh(solved):
    """Sets EIG_C (the module docstring): measured worst ratio EIG_MEASURED_RATIO = 0.288, EIG_C = 1.2 >= 4 x 0.288."""
    worst = 0.0
    for name, A, w, V, sweeps, converged in solved:
        ref = np.linalg.eigvalsh(A)
        D, unit = A.shape[0], eig_unit(A)
        ratio = float(np.abs(w - ref).max()) / unit if unit > 0 else 0.0
        resid = float(np.abs(A @ V - V * w).max()) / unit
        orth = float(np.abs(V.T @ V - np.eye(D)).max()) / (D * U52)
        print(f"{name}: D {D}, sweeps {sweeps}, converged {converged}, |dw| {ratio:.3f}, |AV - Vw| {resid:.3f}, "
              f"|V^T V - I| {orth:.3f} (units of D 2^-52 |A|_2)")
        worst = max(worst, ratio)
        assert converged and 1 <= sweeps <= FM.EIG_MAX_SWEEPS
        assert np.all(np.diff(w) >= 0)
        assert ratio <= EIG_C and resid <= EIG_C and orth <= EIG_C
    print(f"worst eigenvalue ratio {worst:.3f}; EIG_C {EIG_C}")
    assert 4 * worst <= EIG_C, "the constant no longer covers four times the measured ratio"
    assert 4 * EIG_MEASURED_RATIO <= EIG_C


def test_host_sym_eig_small_and_degenerate(solved):
    by = {name: (w, V, sweeps) for name, _, w, V, sweeps, _ in solved}
    assert by["psd 1"][0][0] == random_psd(1, 101)[0, 0] and by["psd 1"][1][0, 0] == 1.0
    w, _, sweeps = by["diagonal"]
    assert np.array_equal(w, np.linspace(-2.0, 9.0, SPECIAL_D)) and sweeps == 1           # nothing to rotate
    assert np.array_equal(by["c * I"][0], np.full(SPECIAL_D, 3.5)) and by["c * I"][2] == 1
    assert np.array_equal(by["offdiag 1e-300"][0], np.arange(1.0, SPECIAL_D + 1.0))       # no overflow in the angle
    assert len({s for _, _, s in by.values()}) >= 3                                        # members end after different sweeps
    # a 2 x 2 matrix against its closed form
    w2 = FM.host_sym_eig(np.array([[2.0, 1.0], [1.0, -1.0]]))[0]
    assert np.abs(w2 - (0.5 + np.array([-1.0, 1.0]) * np.sqrt(2.25 + 1.0))).max() <= 4 * U52 * 3.0
    # huge and zero
    w, V, _, ok = FM.host_sym_eig(np.array([[1e300, 1e-300], [1e-300, -1e300]]))
    assert ok and np.array_equal(w, [-1e300, 1e300]) and np.isfinite(V).all()
    assert np.array_equal(FM.host_sym_eig(np.zeros((4, 4)))[0], np.zeros(4))
    # values only
    assert FM.host_sym_eig(random_psd(5, 1), vectors=False)[1] is None


def test_round_robin_meets_every_pair_once():
    for m in (2, 4, 6, 256):
        seen = set()
        for step in range(m - 1):
            p, q = FM.round_robin_pairs(m, step)
            assert len(p) == m // 2 and np.all(p < q) and len(set(p) | set(q)) == m
            seen |= set(zip(p.tolist(), q.tolist()))
        assert len(seen) == m * (m - 1) // 2


def test_host_moments():
    X, _ = draw(8, 40, 2)
    mean, cov = FM.host_moments(X)
    assert np.allclose(mean, X.astype(np.float64).mean(0), rtol=0, atol=1e-15)
    assert np.allclose(cov, np.cov(X.astype(np.float64), rowvar=False), rtol=1e-13, atol=1e-15)
    with pytest.raises(ValueError):
        FM.host_moments(X[:1])


# ---------------------------------------------------------------------------------------------------------------------
# spectrum and block
# ---------------------------------------------------------------------------------------------------------------------
def test_spectrum_stats_by_hand():
    s = FM.spectrum_stats(np.full(7, 0.3))
    assert s["effective_rank"] == pytest.approx(7.0, rel=1e-14) and s["participation_ratio"] == pytest.approx(7.0, rel=1e-14)
    assert s["top1_share"] == pytest.approx(1 / 7, rel=1e-14)
    s = FM.spectrum_stats([0.0, 2.5, 0.0, -1e-17])
    assert s == {"participation_ratio": 1.0, "effective_rank": 1.0, "top1_share": 1.0}
    assert FM.spectrum_stats(np.zeros(5)) == dict.fromkeys(FM.SPECTRUM_KEYS)
    s = FM.spectrum_stats([3.0, 1.0])
    assert s["participation_ratio"] == pytest.approx(16 / 10) and s["top1_share"] == 0.75
    assert s["effective_rank"] == pytest.approx(np.exp(-(0.75 * np.log(0.75) + 0.25 * np.log(0.25))))


def test_frechet_block_by_hand_and_json_round_trip():
    names = ["Q1", "Q2"]
    rows = {"whole": (5.0, 1.0, 6.0, 1.0), "ef": [[(2.0, 0.5, 2.5, 0.5), None], [(float("nan"), 1.0, 2.0, float("nan")), None]]}
    spectra = {"real": (3.0, 3.5, 0.4), "fake": (1.0, 1.0, 1.0), "real_e": [(2.0, 2.0, 0.5), (float("nan"),) * 3],
               "fake_e": [(1.5, 1.6, 0.7), None]}
    b = FM.frechet_block(4, names, [3, 1], rows, spectra)
    assert b["frechet"] == {"fd": 5.0, "mean_term": 1.0, "trace_term": 6.0, "sqrt_term": 1.0, "n_real": 4, "n_fake": 4,
                            "rank_deficient": True}
    assert FM.frechet_block(3, names, [3, 1], rows, spectra)["frechet"]["rank_deficient"] is False
    assert b["fd_matrix"] == {"Q1": {"Q1": 2.0, "Q2": None}, "Q2": {"Q1": None, "Q2": None}}      # NaN: not converged -> None
    assert b["fd_e"] == {"Q1": 2.0, "Q2": None}
    none = dict.fromkeys(FM.SPECTRUM_KEYS)
    assert b["spectrum"]["real"] == {"participation_ratio": 3.0, "effective_rank": 3.5, "top1_share": 0.4}
    assert b["spectrum"]["per_emotion"]["Q2"] == {"real": none, "fake": none}
    assert b["spectrum"]["per_emotion"]["Q1"]["fake"]["top1_share"] == 0.7
    assert json.loads(json.dumps(b, allow_nan=False)) == b


def small_block(with_frechet):
    sums = {"xx": 10.0, "yy": 11.0, "xy": 12.0, "xx_e": [1.0, 2.0], "yy_e": [1.5, 2.5], "xy_ef": [[1.0, 2.0], [3.0, 4.0]]}
    marg = {"fake_in_real": np.array([-1.0, 1.0, -1.0, 0.5]), "real_in_fake": np.array([-1.0] * 4), "fake_in_real_e": [None, None],
            "real_in_fake_e": [None, None]}
    block = FM.feature_block(8, 3, ["Q1", "Q2"], [2, 2], sums, marg)
    if with_frechet:
        X, Y = draw(8, 4, 4)
        rows, spectra = FM.frechet_inputs_host(X, Y, np.array([0, 0, 1, 1]), 2)
        fb = FM.frechet_block(8, ["Q1", "Q2"], [2, 2], rows, spectra)
        for name, v in fb.pop("fd_e").items():
            block["per_emotion"][name]["fd"] = v
        block.update(fb)
    return block


def test_block_and_table_unchanged_without_the_flag():
    plain, with_ = small_block(False), small_block(True)
    assert set(plain) == {"dim", "k", "kid", "precision", "recall", "per_emotion", "kid_matrix"}
    assert all(set(v) == {"n", "kid", "precision", "recall"} for v in plain["per_emotion"].values())
    table = FM.format_block(plain)
    assert "frechet" not in table and "spectrum" not in table
    # with the entries the earlier lines stand and the new ones follow
    assert set(with_) - set(plain) == {"frechet", "fd_matrix", "spectrum"}
    assert with_["frechet"]["rank_deficient"] and with_["frechet"]["fd"] > 0 and with_["fd_matrix"]["Q1"]["Q2"] is not None
    longer = FM.format_block(with_)
    assert longer.startswith(table + "\n") and "frechet distance" in longer and "covariance spectrum" in longer
    assert "rank deficient" in longer
    for k in plain:
        if k != "per_emotion":
            assert plain[k] == with_[k]
    json.loads(json.dumps(with_, allow_nan=False))


def test_frechet_inputs_host_leaves_small_sets_out():
    X, Y = draw(4, 7, 7)
    rows, spectra = FM.frechet_inputs_host(X, Y, np.array([0, 0, 0, 1, 2, 2, 2]), 4)
    assert rows["whole"] is not None and rows["ef"][0][2] is not None and rows["ef"][2][0] is not None
    assert rows["ef"][1][1] is None and rows["ef"][0][1] is None and rows["ef"][3][3] is None
    assert spectra["real_e"][1] is None and spectra["fake_e"][3] is None and spectra["real_e"][0] is not None


# ---------------------------------------------------------------------------------------------------------------------
# the flag and the entry points, on the host
# ---------------------------------------------------------------------------------------------------------------------
def test_evaluate_refuses_frechet_without_feature_metrics_on_the_host(capsys):
    from melo_gan_amd.gan import evaluate as EV
    with pytest.raises(EV.EvaluateError, match="--feature-metrics"):
        EV.check_frechet_options(True, False)
    with pytest.raises(EV.EvaluateError, match="notes_hidden"):
        EV.check_frechet_options(True, True, {"notes_hidden": 258})
    EV.check_frechet_options(True, True, {"notes_hidden": 256})
    EV.check_frechet_options(False, False)
    args = EV.parse_args(["--frechet"])
    assert args.frechet and not EV.parse_args([]).frechet
    with pytest.raises(EV.EvaluateError, match="--feature-metrics"):
        EV.plan(args)
    assert EV.main(["--frechet"]) == 2
    assert "evaluate: error:" in capsys.readouterr().err


def test_entry_points_refuse_bad_arguments_before_any_launch():
    import torch
    from melo_gan_amd import _lib, ops
    lib = _lib.load()
    x, m, c, w, q = 256, 512, 1024, 4096, 8192           # non-null dummy addresses: nothing here launches
    big = 1 << 30
    assert lib.mg_feat_moments(None, 8, 8, m, c, w, big, None) == -1 and b"null" in lib.mg_last_error()
    for n, D in ((1, 8), ((1 << 20) + 1, 8), (8, 6), (8, 0), (8, 260)):
        assert lib.mg_feat_moments(x, n, D, m, c, w, big, None) == -1 and b"mg_feat_moments" in lib.mg_last_error(), (n, D)
    assert lib.mg_feat_moments(x + 4, 8, 8, m, c, w, big, None) == -1 and b"aligned" in lib.mg_last_error()
    assert lib.mg_feat_moments(x, 8, 8, m, c, w, 8, None) == -3 and b"workspace" in lib.mg_last_error()
    assert lib.mg_sym_eig(None, 1, 4, m, None, c, w, big, None) == -1
    for batch, D in ((0, 4), (4097, 4), (1, 0), (1, 257)):
        assert lib.mg_sym_eig(x, batch, D, m, None, c, w, big, None) == -1 and b"mg_sym_eig" in lib.mg_last_error(), (batch, D)
    assert lib.mg_sym_eig(x, 1, 4, m, None, c, w, 8, None) == -3
    assert lib.mg_frechet_pairs(x, m, 2, 4, None, 1, c, w, q, w, big, None) == -1 and b"null" in lib.mg_last_error()
    for S, D, P in ((0, 4, 1), (4097, 4, 1), (2, 0, 1), (2, 257, 1), (2, 4, 0), (2, 4, 65536)):
        assert lib.mg_frechet_pairs(x, m, S, D, c, P, w, q, q + 4096, w, big, None) == -1, (S, D, P)
        assert b"mg_frechet_pairs" in lib.mg_last_error()
    assert lib.mg_frechet_pairs(x, m, 2, 4, c, 1, w, q, q + 4096, w, 8, None) == -3
    # the workspace: grows with every argument, 0 outside the limits
    wb = lib.mg_frechet_workspace_bytes
    assert wb(0, 256, 10, 17) > wb(0, 256, 10, 0) > wb(0, 256, 1, 0) >= 2 * 256 * 256 * 8
    assert wb(2048, 256, 0, 0) > 0 and wb(1 << 20, 256, 0, 0) >= wb(2048, 256, 0, 0)
    assert wb(0, 255, 1, 0) == wb(0, 256, 1, 0)          # an odd size is padded to the next even one
    for bad in ((1, 8, 0, 0), (8, 6, 0, 0), (0, 8, 0, 0), (0, 8, 0, 3), (0, 257, 1, 0), (0, 8, 4097, 0), (0, 8, 1, 65536)):
        assert wb(*bad) == 0, bad
    # ops: CPU tensors are refused
    f64 = torch.float64
    with pytest.raises(ValueError, match="CUDA/HIP"):
        ops.feat_moments(torch.zeros(8, 8), torch.zeros(8, dtype=f64), torch.zeros(8, 8, dtype=f64))
    with pytest.raises(ValueError, match="CUDA/HIP"):
        ops.sym_eig(torch.zeros(1, 4, 4, dtype=f64), torch.zeros(1, 4, dtype=f64))
    with pytest.raises(ValueError, match="CUDA/HIP"):
        ops.frechet_pairs(torch.zeros(2, 4, dtype=f64), torch.zeros(2, 4, 4, dtype=f64), torch.zeros(1, 2, dtype=torch.int32),
                          torch.zeros(1, 4, dtype=f64), torch.zeros(2, 3, dtype=f64), torch.zeros(3, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="frechet_workspace"):
        ops.frechet_workspace(1, 8, 0, 0, "cpu")
