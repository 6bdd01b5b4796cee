"""GPU: exact t-SNE on the device (csrc/tsne.hip: mg_tsne_affinities, mg_tsne_step; melo_gan_amd/gan/tsne.py; evaluate --tsne)
against tests/tsne_ref.py in fp64.

No tolerance is invented here.  Every compared quantity q is held to
    max |q_device - q_fp64| / max |q_fp64|   <=   4 x  max |q_float32 - q_fp64| / max |q_fp64|
where q_float32 is the SAME numpy code run with every array and operation in float32 on the same input: what fp32 rounding
alone costs, with a factor 4 for a different summation order.  Each test prints both sides before it asserts.
The end-to-end run is chaotic over 1000 iterations, so its final KL is held to a band recorded by
tests/golden/make_golden_tsne.py instead: [lo - s, hi + s] with lo / hi the fp64 reference's final KL over five 1-ulp
perturbations of Y0 and s = hi - lo, the device's fp32 rounding being one more perturbation of that size."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tsne_ref as R  # noqa: E402

import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import ops  # noqa: E402
from melo_gan_amd.gan import tsne as T  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tsne_blobs192.npz")
F32, F64 = np.float32, np.float64


def held(what, dev, ref64, ref32, factor=4.0):
    """The yardstick rule of the module docstring; returns (device deviation, yardstick)."""
    dev, ref64, ref32 = (np.asarray(a, dtype=F64) for a in (dev, ref64, ref32))
    scale = np.abs(ref64).max()
    got, yard = np.abs(dev - ref64).max() / scale, np.abs(ref32 - ref64).max() / scale
    print(f"{what}: device {got:.3e}  float32 mode {yard:.3e}  (x{factor:g} = {factor * yard:.3e})")
    assert np.isfinite(dev).all(), what
    assert got <= factor * yard, f"{what}: device deviates {got:.3e}, float32 mode {yard:.3e}"
    return got, yard


def draw(N, D, seed):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((4, D)) * 1.5
    return (centres[rng.integers(0, 4, N)] + rng.standard_normal((N, D))).astype(F32)


def cuda(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# 1. affinities
# ---------------------------------------------------------------------------------------------------------------------
def affinity_fixture(name):
    if name == "n70_d5":
        return draw(70, 5, 1), 5.0
    if name == "n193_d64":
        return draw(193, 64, 2), 30.0
    if name == "n257_d256_twins":
        X = draw(257, 256, 3)
        X[1] = X[0]
        return X, 30.0
    if name == "n193_d64_x100":
        return draw(193, 64, 2) * F32(100), 30.0
    raise KeyError(name)


@pytest.mark.parametrize("name", ["n70_d5", "n193_d64", "n257_d256_twins", "n193_d64_x100"])
def test_affinities(name):
    X, perp = affinity_fixture(name)
    N = X.shape[0]
    P64, b64 = R.affinities(X, perp, F64)
    P32, b32 = R.affinities(X, perp, F32)
    beta = torch.full((N,), float("nan"), device="cuda")
    P = torch.full((N, N), float("nan"), device="cuda")
    ops.tsne_affinities(cuda(X), perp, P=P, beta=beta)
    Pd, bd = P.cpu().numpy(), beta.cpu().numpy()
    assert np.isfinite(Pd).all() and np.isfinite(bd).all() and (bd > 0).all()
    assert np.array_equal(Pd.view(np.uint32), Pd.T.view(np.uint32)), "P_ij and P_ji differ in bits"
    assert np.all(np.diag(Pd) == 0)
    assert (Pd.sum(1) > 0).all(), "a zero row"
    held(f"{name}: P", Pd, P64, P32)
    held(f"{name}: beta", bd, b64, b32)
    # |sum P - 1|: the three sums in fp64 on the host, so that only the entries' rounding is measured
    s_dev, s_32 = abs(Pd.astype(F64).sum() - 1.0), abs(P32.astype(F64).sum() - 1.0)
    print(f"{name}: |sum P - 1| device {s_dev:.3e}  float32 mode {s_32:.3e}  fp64 mode {abs(P64.sum() - 1.0):.3e}")
    assert s_dev <= 4 * s_32
    if name == "n257_d256_twins":       # identical rows are exactly 0 apart: each is the other's nearest row, at distance 0
        assert Pd[0, 1] == Pd[1, 0] and Pd[0, 1] >= Pd[0, 2:].max()


# ---------------------------------------------------------------------------------------------------------------------
# 2. one step, teacher-forced from the fp64 run's states
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blob_run():
    g = np.load(GOLDEN)
    X, labels = R.blobs(48, 64, 0)
    P64, _ = R.affinities(X, 30.0)
    return {"X": X, "labels": labels, "P32": P64.astype(F32), "golden": g}


def device_step(P32, Y, up, gn, ee, mom, lr, trace):
    Yd, ud, gd = cuda(Y), cuda(up), cuda(gn)
    grad = torch.full_like(Yd, float("nan"))
    tr = torch.full((1, 4), float("nan"), dtype=torch.float64, device="cuda") if trace else None
    ops.tsne_step(cuda(P32), Yd, ud, gd, ee, mom, lr, grad=grad, trace=tr)
    out = {"Y": Yd.cpu().numpy(), "update": ud.cpu().numpy(), "gains": gd.cpu().numpy(), "grad": grad.cpu().numpy()}
    if trace:
        rec = tr.cpu().numpy()[0]
        out.update(kl=rec[0], grad_norm=rec[1], Z=rec[2])
    return out


@pytest.mark.parametrize("it", [0, 1, 100, 251, 600])
def test_one_step_teacher_forced(blob_run, it):
    g, P32 = blob_run["golden"], blob_run["P32"]
    k = list(g["state_its"]).index(it)
    Y, up, gn = (g[n][k].astype(F32) for n in ("state_Y", "state_update", "state_gains"))      # what the device is given
    ee, mom = R.schedule(it)
    lr = R.auto_lr(P32.shape[0])
    r64 = R.step(P32.astype(F64), Y.astype(F64), up.astype(F64), gn.astype(F64), ee, mom, lr, F64)
    r32 = R.step(P32, Y, up, gn, ee, mom, lr, F32)
    print(f"iteration {it}: max |Y| {np.abs(Y).max():.3g}, exaggeration {ee}, momentum {mom}")
    for trace in (True, False):         # both instantiations of the forces kernel
        d = device_step(P32, Y, up, gn, ee, mom, lr, trace)
        tag = f"it {it} ({'trace' if trace else 'plain'})"
        for q in ("grad", "Y", "update"):
            held(f"{tag}: {q}", d[q], r64[q], r32[q])
        if trace:
            for q in ("Z", "kl", "grad_norm"):
                held(f"{tag}: {q}", d[q], r64[q], r32[q])
        # a gain follows the sign of update * grad: compared where the gradient component is clear of 0
        clear = np.abs(r64["grad"]) >= 1e-4 * np.abs(r64["grad"]).max()
        assert (~clear).mean() <= 0.01, f"{(~clear).mean():.3%} of the gradient components are unclear"
        held(f"{tag}: gains", d["gains"][clear], r64["gains"][clear], r32["gains"][clear])


# ---------------------------------------------------------------------------------------------------------------------
# 3. free trajectory
# ---------------------------------------------------------------------------------------------------------------------
# (rows, D, perplexity, blob seed): seeds chosen by scanning 12 per shape for the margin asserted below, in fp64
TRAJ = [(48, 8, 5.0, 0), (40, 5, 5.0, 7), (68, 64, 10.0, 10)]


@pytest.mark.parametrize("N,D,perp,seed", TRAJ)
def test_free_trajectory(N, D, perp, seed):
    X, _ = R.blobs(N // 4, D, seed)
    Y0 = (np.random.default_rng(100 + seed).standard_normal((N, 2)) * 1e-4).astype(F32)
    margin = [np.inf]

    def watch(it, r):
        gm = np.abs(r["grad"])
        um = np.abs(r["update"])
        margin[0] = min(margin[0], gm.min() / gm.max(), um.min() / um.max())

    P64, _ = R.affinities(X, perp, F64)
    Y64, _, _ = R.run(P64, Y0.astype(F64), 12, exaggeration_iters=6, watch=watch)
    print(f"N {N}: smallest |component| / max |component| of grad and update over the run: {margin[0]:.3e}")
    assert margin[0] >= 1e-4, "the fixture's gains are not clear of a sign flip"
    P32, _ = R.affinities(X, perp, F32)
    Y32, _, _ = R.run(P32, Y0, 12, exaggeration_iters=6, dtype=F32)
    ts = T.Tsne(perplexity=perp, iters=12, exaggeration_iters=6, init=Y0)
    Yd = ts.fit_transform(X)
    assert ts.trace_iters == [11] and np.isfinite(ts.kl_)
    held(f"N {N}: Y after 12 iterations", Yd, Y64, Y32)


# ---------------------------------------------------------------------------------------------------------------------
# 4. end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_end_to_end_blobs(blob_run):
    g = blob_run["golden"]
    lo, hi = float(g["kl_lo"]), float(g["kl_hi"])
    s = hi - lo
    ts = T.Tsne()
    Y = ts.fit_transform(blob_run["X"])
    purity = R.knn_purity(Y, blob_run["labels"], 5)
    print(f"final KL {ts.kl_:.5f}; fp64 band [{lo:.5f}, {hi:.5f}], spread {s:.5f}; 5-NN purity {purity}")
    print("KL trace", np.round(ts.kl_trace, 4).tolist())
    assert Y.shape == (192, 2) and np.isfinite(Y).all()
    assert len(ts.kl_trace) == 20 and np.isfinite(ts.kl_trace).all() and np.isfinite(ts.grad_trace).all()
    assert ts.trace_iters == list(range(49, 1000, 50))
    assert purity == 1.0
    assert lo - s <= ts.kl_ <= hi + s


# ---------------------------------------------------------------------------------------------------------------------
# 5. determinism
# ---------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_runs_and_replay_leave_identical_bits():
    X = draw(150, 24, 9)
    kw = dict(perplexity=12.0, iters=130, exaggeration_iters=60, trace_every=20, init="random", seed=5)
    a, b, eager = T.Tsne(**kw), T.Tsne(**kw), T.Tsne(graphs=False, **kw)
    Ya, Yb, Ye = a.fit_transform(X), b.fit_transform(X), eager.fit_transform(X)
    assert np.isfinite(Ya).all() and np.abs(Ya).max() > 1e-3
    assert np.array_equal(bits(Ya), bits(Yb)) and np.array_equal(bits(a.kl_trace), bits(b.kl_trace))
    assert np.array_equal(bits(Ya), bits(Ye)), "eager stepping and graph replay differ"
    assert np.array_equal(bits(a.kl_trace), bits(eager.kl_trace)) and np.array_equal(bits(a.grad_trace), bits(eager.grad_trace))
    assert a.trace_iters == [19, 39, 59, 79, 99, 119, 129]
    other = T.Tsne(**dict(kw, seed=6)).fit_transform(X)
    assert not np.array_equal(bits(Ya), bits(other)), "the seed does not reach the random initialisation"


def test_a_step_on_a_second_stream_gives_the_same_bits():
    X = draw(333, 16, 4)
    P = ops.tsne_affinities(cuda(X), 20.0)
    P2 = ops.tsne_affinities(cuda(X), 20.0)
    assert torch.equal(P, P2)
    Y0 = cuda(np.random.default_rng(1).standard_normal((333, 2)).astype(F32))
    outs = []
    for stream in (None, torch.cuda.Stream()):
        Y, up, gn = Y0.clone(), torch.zeros_like(Y0), torch.ones_like(Y0)
        tr = torch.zeros(2, 4, dtype=torch.float64, device="cuda")
        cur = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
            for _ in range(2):
                ops.tsne_step(P, Y, up, gn, 12.0, 0.5, 50.0, trace=tr, cursor=cur)
        torch.cuda.synchronize()
        assert int(cur.item()) == 2
        outs.append((Y.cpu().numpy(), up.cpu().numpy(), gn.cpu().numpy(), tr.cpu().numpy()))
    for a, b in zip(*outs):
        assert np.isfinite(a).all() and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------------
# 6. surface: the CLI and evaluate --tsne
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_writes_embedding_plot_and_report(tmp_path):
    import csv
    import xml.etree.ElementTree as ET
    import yaml
    X, labels = R.blobs(10, 12, 4)
    names = [T.EMOTIONS[k] for k in labels]
    with open(tmp_path / "val_split.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["npz_path", "emotion"])
        for i, e in enumerate(names):
            w.writerow([f"data/npz/{i}.npz", e])
    np.save(tmp_path / "feats.npy", X)
    cfg = {"VAL_SPLIT": str(tmp_path / "val_split.csv"), "ENCODER_FEATS_VAL": str(tmp_path / "feats.npy"), "LOG_DIR": str(tmp_path / "log")}
    (tmp_path / "gan.yaml").write_text(yaml.safe_dump(cfg))
    argv = ["--config", str(tmp_path / "gan.yaml"), "--split", "val", "--perplexity", "8", "--iters", "120", "--seed", "3",
            "--out", str(tmp_path / "out")]
    assert T.main(argv) == 0
    Y = np.load(tmp_path / "out" / "val_tsne.npy")
    want = T.Tsne(perplexity=8.0, iters=120, seed=3).fit_transform(X)
    assert Y.shape == (40, 2) and np.array_equal(bits(Y), bits(want))
    rep = json.load(open(tmp_path / "out" / "val_tsne.json"))
    assert (rep["n"], rep["d"]) == (40, 12) and rep["params"]["perplexity"] == 8.0 and rep["params"]["iters"] == 120
    assert rep["kl"] == rep["kl_trace"][-1] and np.isfinite(rep["kl_trace"]).all() and rep["trace_iters"] == [49, 99, 119]
    root = ET.parse(tmp_path / "out" / "val_tsne.svg").getroot()
    ns = "{http://www.w3.org/2000/svg}"
    assert len(list(next(g for g in root.iter(ns + "g") if g.get("id") == "points"))) == 40
    assert T.main(["--config", str(tmp_path / "gan.yaml"), "--split", "val", "--perplexity", "39"]) == 2      # no root: refused on the host


def test_evaluate_tsne_block_and_unchanged_report_without_it(tmp_path):
    import yaml
    from melo_gan_amd.gan import evaluate as EV
    from test_evaluate_features_gpu import spread_state
    from test_evaluate_gpu import save_state
    S, _, ed_cfg = spread_state(32, 4)
    ck, ed = save_state(S, str(tmp_path))
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "gan_config.yaml")))
    cfg.update(MAX_NOTES=32, LOG_DIR=str(tmp_path / "log"))
    cp, ep = tmp_path / "gan.yaml", tmp_path / "ed.yaml"
    cp.write_text(yaml.safe_dump(cfg))
    ep.write_text(yaml.safe_dump(ed_cfg))
    common = ["--config", str(cp), "--ckpt", ck, "--ed_config", str(ep), "--ed_ckpt", ed, "--synthetic", "64", "--batch", "16",
              "--seed", "7"]
    assert EV.main(common + ["--tsne", "--out", str(tmp_path / "refused.json")]) == 2       # needs --feature-metrics
    assert not (tmp_path / "refused.json").exists()
    assert EV.main(common + ["--feature-metrics", "--out", str(tmp_path / "plain.json")]) == 0
    assert EV.main(common + ["--feature-metrics", "--tsne", "--out", str(tmp_path / "with.json")]) == 0
    plain, with_ = json.load(open(tmp_path / "plain.json")), json.load(open(tmp_path / "with.json"))
    block = with_.pop("tsne")
    assert "tsne" not in plain and plain == with_, "the report changed outside its tsne block"
    assert not (tmp_path / "plain_tsne.npy").exists()
    assert block["n"] == 128 and block["dim"] == ed_cfg["notes_hidden"] and block["params"]["perplexity"] == 30.0
    assert block["files"] == {"embedding": "with_tsne.npy", "plot": "with_tsne.svg"} and np.isfinite(block["kl"])
    Y = np.load(tmp_path / "with_tsne.npy")
    assert Y.shape == (128, 2) and np.isfinite(Y).all()
    svg = (tmp_path / "with_tsne.svg").read_text()
    assert svg.count("<circle class=\"pt\"") >= 64 and svg.count("<path class=\"pt\"") >= 64 and "generated" in svg
