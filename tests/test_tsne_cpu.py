"""CPU-only: the host half of the t-SNE feature (melo_gan_amd/gan/tsne.py: the reference's alignment rules, the SVG writer,
the PCA initialisation), the argument checks of the new C-ABI entry points (before any launch), and the numpy restatement's
own sanity (tests/tsne_ref.py: the entropy of every conditional row, the analytic gradient against a finite difference)."""
import csv
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import tsne_ref as R

import melo_gan_amd  # noqa: F401
from melo_gan_amd.gan import tsne as T


def write_csv(path, rows):
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=["npz_path", "emotion"])
        w.writeheader()
        for r in rows:
            w.writerow({"npz_path": r[0], "emotion": r[1]})


# ---- load_latents ----
def test_row_aligned_array_truncates_the_longer_side(tmp_path):
    rows = [(f"data/npz/f{i}.npz", e) for i, e in enumerate(["happy", "sad", "angry", "calm", "Happy ", "bored"])]
    write_csv(tmp_path / "s.csv", rows)
    feats = np.arange(8 * 3, dtype=np.float64).reshape(8, 3)
    np.save(tmp_path / "long.npy", feats)                   # array longer than the CSV: the array is truncated
    X, labels = T.load_latents(str(tmp_path / "s.csv"), str(tmp_path / "long.npy"))
    assert X.dtype == np.float32 and X.shape == (6, 3) and np.array_equal(X, feats[:6].astype(np.float32))
    assert labels == ["happy", "sad", "angry", "calm", "happy", "other"]      # case / blanks ignored, unknown -> other
    np.save(tmp_path / "short.npy", feats[:4])              # array shorter than the CSV: the CSV is truncated
    X, labels = T.load_latents(str(tmp_path / "s.csv"), str(tmp_path / "short.npy"))
    assert X.shape == (4, 3) and labels == ["happy", "sad", "angry", "calm"]
    np.save(tmp_path / "n1d.npy", feats[:4].reshape(4, 1, 3))       # (N, 1, D) is flattened per row, as the reference does
    assert T.load_latents(str(tmp_path / "s.csv"), str(tmp_path / "n1d.npy"))[0].shape == (4, 3)


def test_keyed_map_drops_rows_without_a_key(tmp_path):
    rows = [("data/npz/a.npz", "happy"), ("data/npz/b.npz", "sad"), ("data/npz/c.npz", "calm"), ("", "angry"),
            ("data/npz/d.npz", "weird")]
    write_csv(tmp_path / "s.csv", rows)
    table = {"data/npz/a.npz": np.array([1.0, 2.0]), "c.npz": np.array([5.0, 6.0]), "d.npz": np.array([7.0, 8.0]),
             "unused.npz": np.array([0.0, 0.0])}             # full path, basename, basename; b and the blank have no key
    arr = np.empty(len(table), dtype=object)
    for i, kv in enumerate(table.items()):
        arr[i] = kv
    np.save(tmp_path / "map.npy", arr, allow_pickle=True)
    X, labels = T.load_latents(str(tmp_path / "s.csv"), str(tmp_path / "map.npy"))
    assert labels == ["happy", "calm", "other"]
    assert np.array_equal(X, np.array([[1, 2], [5, 6], [7, 8]], dtype=np.float32))
    with pytest.raises(T.TsneError):
        T.load_latents(str(tmp_path / "nope.csv"), str(tmp_path / "map.npy"))
    with pytest.raises(T.TsneError):
        T.load_latents(str(tmp_path / "s.csv"), str(tmp_path / "nope.npy"))


# ---- SVG ----
def test_svg_is_well_formed_with_n_points_and_a_legend_of_the_classes_present(tmp_path):
    rng = np.random.default_rng(0)
    Y = rng.standard_normal((30, 2))
    labels = ["happy"] * 10 + ["calm"] * 15 + ["other"] * 5
    T.write_svg(str(tmp_path / "a.svg"), Y, labels, title="a <b> & c")
    root = ET.parse(tmp_path / "a.svg").getroot()
    ns = "{http://www.w3.org/2000/svg}"
    assert root.tag == ns + "svg"
    points = next(g for g in root.iter(ns + "g") if g.get("id") == "points")
    assert len(list(points)) == 30 and all(e.get("class") == "pt" for e in points)
    names = [g.find(ns + "text").text for g in root.iter(ns + "g") if g.get("class") == "legend-class"]
    assert names == ["happy", "calm", "other"]
    assert not [g for g in root.iter(ns + "g") if g.get("class") == "legend-group"]
    # marker shape by group: circles and crosses, both in the legend
    groups = np.array([0] * 15 + [1] * 15)
    T.write_svg(str(tmp_path / "b.svg"), Y, labels, groups=groups)
    root = ET.parse(tmp_path / "b.svg").getroot()
    points = next(g for g in root.iter(ns + "g") if g.get("id") == "points")
    assert len(points.findall(ns + "circle")) == 15 and len(points.findall(ns + "path")) == 15
    assert [g.find(ns + "text").text for g in root.iter(ns + "g") if g.get("class") == "legend-group"] == ["real", "generated"]
    with pytest.raises(T.TsneError):
        T.write_svg(str(tmp_path / "c.svg"), np.full((3, 2), np.nan), ["happy"] * 3)


# ---- PCA initialisation ----
def test_pca_init_matches_an_svd_in_fp64():
    X, _ = R.blobs(12, 9, 3)
    Y = T.pca_init(X)
    assert Y.dtype == np.float64 and Y.shape == (48, 2)
    Xc = X.astype(np.float64) - X.astype(np.float64).mean(0)
    U, S, Vt = np.linalg.svd(Xc, full_matrices=False)
    proj = Xc @ Vt[:2].T                                    # the scores, up to a sign per component
    for c in range(2):
        s = np.sign(Vt[c, np.abs(Vt[c]).argmax()])
        want = s * proj[:, c] / np.std(proj[:, 0]) * 1e-4
        assert np.abs(Y[:, c] - want).max() <= 1e-12 * np.abs(want).max()
    assert abs(np.std(Y[:, 0]) - 1e-4) <= 1e-16
    assert np.array_equal(Y, R.pca_init(X))                 # the tests' restatement is the same function


def test_tsne_checks_its_arguments_on_the_host():
    with pytest.raises(T.TsneError):
        T.Tsne(perplexity=30).check(31, 8)                  # perplexity >= N - 1
    with pytest.raises(T.TsneError):
        T.Tsne(perplexity=1).check(3, 8)
    with pytest.raises(T.TsneError):
        T.Tsne(init="umap")
    with pytest.raises(T.TsneError):
        T.Tsne(init=np.zeros((5, 2))).check(6, 3)
    t = T.Tsne(iters=120, trace_every=50)
    assert t.trace_schedule() == [49, 99, 119]
    assert T.Tsne(iters=100, trace_every=50).trace_schedule() == [49, 99]


# ---- the C-ABI ----
def test_tsne_entry_points_reject_bad_arguments_before_any_launch():
    from melo_gan_amd import _lib
    lib = _lib.load()
    x, p, w, y, u, g = 256, 512, 1024, 2048, 4096, 8192       # non-null dummy addresses; nothing here launches
    big = 1 << 30
    assert lib.mg_tsne_workspace_bytes(3) == 0 and lib.mg_tsne_workspace_bytes(16385) == 0
    need = lib.mg_tsne_workspace_bytes(192)
    assert need > 0 and lib.mg_tsne_workspace_bytes(16384) >= need
    # affinities
    assert lib.mg_tsne_affinities(None, 192, 64, 30.0, p, None, w, big, None) == -1 and b"null" in lib.mg_last_error()
    assert lib.mg_tsne_affinities(x, 192, 64, 30.0, None, None, w, big, None) == -1
    assert lib.mg_tsne_affinities(x, 192, 64, 30.0, p, None, None, big, None) == -1
    assert lib.mg_tsne_affinities(x, 3, 64, 1.0, p, None, w, big, None) == -1 and b"N = 3" in lib.mg_last_error()
    assert lib.mg_tsne_affinities(x, 16385, 64, 30.0, p, None, w, big, None) == -1
    assert lib.mg_tsne_affinities(x, 192, 0, 30.0, p, None, w, big, None) == -1 and b"D = 0" in lib.mg_last_error()
    for perp in (191.0, 250.0, 0.5, float("nan")):
        assert lib.mg_tsne_affinities(x, 192, 64, perp, p, None, w, big, None) == -1, perp
        assert b"perplexity" in lib.mg_last_error(), perp
    assert lib.mg_tsne_affinities(x, 192, 64, 30.0, p, None, w, need - 1, None) == -3 and b"workspace" in lib.mg_last_error()
    # step
    ok = (p, 192, y, u, g, 12.0, 0.5, 50.0, None, None, None, 0, w, big, None)
    for at in (0, 2, 3, 4, 12):
        bad = list(ok)
        bad[at] = None
        assert lib.mg_tsne_step(*bad) == -1 and b"null" in lib.mg_last_error(), at
    assert lib.mg_tsne_step(p, 3, *ok[2:]) == -1 and b"N = 3" in lib.mg_last_error()
    assert lib.mg_tsne_step(*ok[:13], need - 1, None) == -3 and b"workspace" in lib.mg_last_error()
    assert lib.mg_tsne_step(*ok[:5], 12.0, 1.0, 50.0, *ok[8:]) == -1 and b"momentum" in lib.mg_last_error()
    assert lib.mg_tsne_step(*ok[:9], None, x, 4, *ok[12:]) == -1 and b"cursor" in lib.mg_last_error()
    assert lib.mg_tsne_step(*ok[:9], x, None, 0, *ok[12:]) == -1 and b"records" in lib.mg_last_error()


def test_ops_wrappers_refuse_cpu_tensors_and_bad_shapes():
    import torch
    from melo_gan_amd import ops
    with pytest.raises(ValueError):
        ops.tsne_affinities(torch.zeros(8, 4), 2.0)
    with pytest.raises(ValueError):
        ops.tsne_step(torch.zeros(8, 8), torch.zeros(8, 2), torch.zeros(8, 2), torch.ones(8, 2), 12.0, 0.5, 50.0)
    with pytest.raises(ValueError):
        ops.tsne_workspace(3, "cpu")


# ---- the restatement's own sanity ----
@pytest.mark.parametrize("n_per,D,perp,scale", [(12, 8, 5, 1.0), (48, 64, 30, 1.0), (48, 64, 30, 100.0)])
def test_every_conditional_row_has_the_wanted_entropy(n_per, D, perp, scale):
    X, _ = R.blobs(n_per, D, 1)
    C, beta = R.conditional(R.sq_dists(X.astype(np.float64) * scale), perp)
    assert np.all(beta > 0) and np.all(np.diag(C) == 0)
    assert np.abs(C.sum(1) - 1).max() <= 1e-14
    assert np.abs(R.row_entropy(C) - np.log(perp)).max() <= 1e-12
    P, _ = R.affinities(X.astype(np.float64) * scale, perp)
    assert np.array_equal(P, P.T) and abs(P.sum() - 1) <= 1e-14


def test_analytic_gradient_equals_a_finite_difference_of_the_kl():
    X, _ = R.blobs(6, 5, 2)
    P, _ = R.affinities(X, 5)
    Y = np.random.default_rng(5).standard_normal((24, 2))
    grad, _, _ = R.forces(P, Y)
    h = 1e-6
    fd = np.zeros_like(Y)
    for i in range(Y.shape[0]):
        for d in range(2):
            Yp, Ym = Y.copy(), Y.copy()
            Yp[i, d] += h
            Ym[i, d] -= h
            fd[i, d] = (R.forces(P, Yp)[2] - R.forces(P, Ym)[2]) / (2 * h)
    assert np.abs(fd - grad).max() <= 1e-7 * np.abs(grad).max()


def test_float32_mode_runs_in_float32():
    X, _ = R.blobs(12, 8, 1)
    P32, b32 = R.affinities(X, 5, np.float32)
    assert P32.dtype == np.float32 and b32.dtype == np.float32
    r = R.step(P32, np.zeros((48, 2)) + 1e-4 * np.random.default_rng(0).standard_normal((48, 2)), np.zeros((48, 2)),
               np.ones((48, 2)), 12.0, 0.5, 50.0, np.float32)
    assert all(r[k].dtype == np.float32 for k in ("Y", "update", "gains", "grad"))


def test_optional_cross_check_of_p_against_scikit_learn():
    sk = pytest.importorskip("sklearn.manifold._t_sne")
    sq = pytest.importorskip("scipy.spatial.distance")
    X, _ = R.blobs(48, 64, 0)
    P, _ = R.affinities(X, 30)
    Ps = sq.squareform(sk._joint_probabilities(R.sq_dists(X).astype(np.float32), 30, 0))
    assert np.abs(Ps - P).max() <= 2e-5 * P.max()           # scikit-learn stops its search at 1e-5 and works in fp32


def test_evaluate_refuses_tsne_without_feature_metrics_on_the_host():
    from melo_gan_amd.gan import evaluate as EV
    with pytest.raises(EV.EvaluateError, match="--feature-metrics"):
        EV.check_tsne_options(True, False)
    with pytest.raises(EV.EvaluateError, match="perplexity"):
        EV.check_tsne_options(True, True, 15)               # 2 x 15 rows leave the default perplexity no root
    EV.check_tsne_options(True, True, 64)
    EV.check_tsne_options(False, False)
    args = EV.parse_args(["--tsne"])
    assert args.tsne and not EV.parse_args([]).tsne
    with pytest.raises(EV.EvaluateError, match="--feature-metrics"):
        EV.plan(args)
