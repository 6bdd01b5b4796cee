"""GPU: the evaluator's Frechet distance and covariance spectra (Evaluator(features=True, frechet=True), --feature-metrics
--frechet) on the tiny engines of tests/test_evaluate_features_gpu.py (helpers copied from there): every new entry of the
feature_space block against the host computation from the stashed features themselves -- the shape of the entries against
feature_metrics.frechet_block over frechet_inputs_host, every distance against the nuclear-norm route and every spectrum against
np.linalg.eigvalsh of the fp64 covariance, within the tolerances tests/test_frechet_gpu.py derives -- batch-size independence,
small emotions, the opt-in, the single device -> host read and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import eval_pass  # noqa: E402
from melo_gan_amd.gan import evaluate as EV  # noqa: E402
from melo_gan_amd.gan import feature_metrics as FM  # noqa: E402
from melo_gan_amd.gan.dataset import GANDataset  # noqa: E402
from oracle import melo_oracle as O  # noqa: E402
from test_evaluate_gpu import gen_state, save_state, make_split  # noqa: E402
from test_frechet_cpu import nuclear_fd  # noqa: E402
from test_frechet_gpu import fd_tolerance, spectrum_tolerance  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
K, N_ROWS, BATCH, KNN = 4, 22, 8, 3
ED_SCALE, PROJECT_SCALE = 8.0, 1.0 / 512.0
NEW_KEYS = ("frechet", "fd_matrix", "spectrum")


def spread_state(T, C):
    """test_evaluate_features_gpu.spread_state: gen_state with the classifier's encoder convolutions x8 and its projection
    x1/512, so that the features of different rolls lie apart."""
    S, cfg, ed_cfg = gen_state(T, C, "warm_start", "notes")
    for k in S.PED:
        if k.startswith("encoder.conv.") and k.endswith("net.0.weight"):
            S.PED[k] = S.PED[k] * ED_SCALE
        elif k.startswith("encoder.project."):
            S.PED[k] = S.PED[k] * PROJECT_SCALE
    return S, cfg, ed_cfg


def build(tmp_path, T, C, batch=BATCH, frechet=True):
    S, cfg, ed_cfg = spread_state(T, C)
    ck, ed = save_state(S, str(tmp_path))
    ev = EV.Evaluator(cfg, ed_cfg, "cuda", batch, features=True, knn_k=KNN, frechet=frechet)
    ev.load_generator(ck)
    ev.load_critic(ck)
    ev.load_ed(ed)
    return S, cfg, ed_cfg, ev


def without_frechet(block):
    out = {k: v for k, v in block.items() if k not in NEW_KEYS}
    out["per_emotion"] = {name: {k: v for k, v in pe.items() if k != "fd"} for name, pe in block["per_emotion"].items()}
    return out


def check_frechet(block, R, Fk, labels):
    """The new entries against the host, from the stashes; returns {path: tolerance} for the batch-size comparison."""
    R, Fk, labels = R.double().numpy(), Fk.double().numpy(), labels.numpy()
    D, n, names = R.shape[1], len(labels), list(EV.EMOTIONS)
    counts = [int((labels == e).sum()) for e in range(K)]
    host = FM.frechet_block(D, names, counts, *FM.frechet_inputs_host(R, Fk, labels, K))
    fr = block["frechet"]
    assert set(fr) == {"fd", "mean_term", "trace_term", "sqrt_term", "n_real", "n_fake", "rank_deficient"}
    assert (fr["n_real"], fr["n_fake"], fr["rank_deficient"]) == (n, n, n <= D) == \
        (host["frechet"]["n_real"], host["frechet"]["n_fake"], host["frechet"]["rank_deficient"])
    tols = {}

    def check_fd(got, want_host, X, Y, path):
        assert (got is None) == (want_host is None), path
        if got is None:
            assert len(X) < 2 or len(Y) < 2, path
            return
        ref = nuclear_fd(X, Y)
        tols[path] = fd_tolerance(X, Y, ref)
        print(f"{path}: fd {got:.12g} (nuclear route {ref[0]:.12g}, eigh route {want_host:.12g}), |err| {abs(got - ref[0]):.3g}, "
              f"tol {tols[path]:.3g}")
        assert abs(got - ref[0]) <= tols[path], path

    check_fd(fr["fd"], host["frechet"]["fd"], R, Fk, "fd")
    if fr["fd"] is not None:
        ref = nuclear_fd(R, Fk)
        for key, want in zip(("mean_term", "trace_term", "sqrt_term"), ref[1:]):
            assert abs(fr[key] - want) <= tols["fd"], key
    assert list(block["fd_matrix"]) == names
    for e, name in enumerate(names):
        for f, other in enumerate(names):
            check_fd(block["fd_matrix"][name][other], host["fd_matrix"][name][other], R[labels == e], Fk[labels == f],
                     f"fd.{name}.{other}")
        assert block["per_emotion"][name]["fd"] == block["fd_matrix"][name][name]

    def check_spectrum(got, want_host, X, path):
        assert set(got) == set(FM.SPECTRUM_KEYS), path
        if len(X) < 2:
            assert got == dict.fromkeys(FM.SPECTRUM_KEYS) == want_host, path
            return
        cov = FM.host_moments(X)[1]
        want, tol = FM.spectrum_stats(np.linalg.eigvalsh(cov)), spectrum_tolerance(cov)
        for key in FM.SPECTRUM_KEYS:
            # the device's covariance differs from the host's by the moment bounds, far inside the eigenvalue bound: twice it
            print(f"{path}.{key}: {got[key]:.12g} (host {want[key]:.12g}), |err| {abs(got[key] - want[key]):.3g}, tol {2 * tol[key]:.3g}")
            assert abs(got[key] - want[key]) <= 2 * tol[key], (path, key)
            tols[f"{path}.{key}"] = 2 * tol[key]

    sp = block["spectrum"]
    assert set(sp) == {"real", "fake", "per_emotion"} and list(sp["per_emotion"]) == names
    check_spectrum(sp["real"], host["spectrum"]["real"], R, "spectrum.real")
    check_spectrum(sp["fake"], host["spectrum"]["fake"], Fk, "spectrum.fake")
    for e, name in enumerate(names):
        check_spectrum(sp["per_emotion"][name]["real"], host["spectrum"]["per_emotion"][name]["real"], R[labels == e],
                       f"spectrum.{name}.real")
        check_spectrum(sp["per_emotion"][name]["fake"], host["spectrum"]["per_emotion"][name]["fake"], Fk[labels == e],
                       f"spectrum.{name}.fake")
    return tols


@pytest.mark.parametrize("T,C", [(32, 4), (64, 128)])
def test_frechet_entries_against_the_host(tmp_path, T, C, monkeypatch):
    S, cfg, ed_cfg, ev = build(tmp_path, T, C)
    ds, real, numeric, latent, labels = make_split(T, C, cfg)
    rep = ev.evaluate(ds, seed=3)
    json.loads(json.dumps(rep, allow_nan=False))
    block = rep["feature_space"]
    assert block["dim"] == ed_cfg["notes_hidden"] and block["frechet"]["rank_deficient"]
    check_frechet(block, ev.feat_real[:N_ROWS].cpu(), ev.feat_fake[:N_ROWS].cpu(), labels)
    assert block["frechet"]["fd"] > 0 and all(v["fd"] is not None for v in block["per_emotion"].values())
    table = EV.format_table(rep)
    assert "frechet distance" in table and "covariance spectrum" in table and "rank deficient" in table
    # a second pass replays the graph: the same report, to the bit
    assert ev.evaluate(ds, seed=3) == rep
    # the block is still one device -> host read
    reads, host = [], eval_pass.Packed.host
    monkeypatch.setattr(eval_pass.Packed, "host", lambda self: (reads.append(1), host(self))[1])
    again = ev.feature_space(labels, N_ROWS)
    assert len(reads) == 1 and again == block
    monkeypatch.undo()
    # opt-in: without the flag every other key of the report is what it was, to the bit
    _, _, _, plain = build(tmp_path, T, C, frechet=False)
    rep0 = plain.evaluate(ds, seed=3)
    assert not any(k in rep0["feature_space"] for k in NEW_KEYS)
    assert all("fd" not in pe for pe in rep0["feature_space"]["per_emotion"].values())
    assert "frechet" not in EV.format_table(rep0)
    assert rep0 == {**rep, "feature_space": without_frechet(block)}
    # a generator that copies the real rows: distance 0 within its tolerance
    ev.feat_fake[:N_ROWS].copy_(ev.feat_real[:N_ROWS])
    torch.cuda.synchronize()
    same = ev.feature_space(labels, N_ROWS)
    Rh = ev.feat_real[:N_ROWS].cpu().double().numpy()
    assert abs(same["frechet"]["fd"]) <= fd_tolerance(Rh, Rh, nuclear_fd(Rh, Rh))
    assert same["spectrum"]["real"] == same["spectrum"]["fake"]


def test_frechet_needs_features_and_a_width_the_kernel_reads(tmp_path):
    S, cfg, ed_cfg = spread_state(32, 4)
    with pytest.raises(EV.EvaluateError, match="--feature-metrics"):
        EV.Evaluator(cfg, ed_cfg, "cuda", BATCH, features=False, frechet=True)


def test_small_and_missing_emotions_are_none(tmp_path):
    T, C = 32, 4
    S, cfg, ed_cfg, ev = build(tmp_path, T, C)
    real, numeric, latent, _ = O.synthetic_batch(N_ROWS, T, C, cfg["LATENT_DIM"], 6, 7)
    labels = torch.tensor([0, 1] * 10 + [2, 0])          # emotion 2: one row; emotion 3: none
    ds = GANDataset(real.numpy(), labels.numpy(), numeric.numpy(), None, cfg["LATENT_DIM"], "cuda")
    rep = ev.evaluate(ds, seed=3)
    json.loads(json.dumps(rep, allow_nan=False))
    block = rep["feature_space"]
    check_frechet(block, ev.feat_real[:N_ROWS].cpu(), ev.feat_fake[:N_ROWS].cpu(), labels)
    names = EV.EMOTIONS
    none = dict.fromkeys(FM.SPECTRUM_KEYS)
    for small in (names[2], names[3]):
        assert block["per_emotion"][small]["fd"] is None
        assert block["spectrum"]["per_emotion"][small] == {"real": none, "fake": none}
        for name in names:
            assert block["fd_matrix"][name][small] is None and block["fd_matrix"][small][name] is None
    assert block["fd_matrix"][names[0]][names[1]] is not None and block["frechet"]["fd"] is not None


def test_frechet_entries_do_not_depend_on_the_batch_size(tmp_path):
    T, C = 32, 4
    blocks, tols = {}, {}
    for batch in (8, 5):
        S, cfg, ed_cfg, ev = build(tmp_path, T, C, batch=batch)
        ds, real, numeric, latent, labels = make_split(T, C, cfg)
        blocks[batch] = ev.evaluate(ds, seed=5)["feature_space"]
        tols[batch] = check_frechet(blocks[batch], ev.feat_real[:N_ROWS].cpu(), ev.feat_fake[:N_ROWS].cpu(), labels)
    a, b = blocks[8], blocks[5]

    def same(x, y, path):          # within the sum of the two runs' tolerances against the host
        assert (x is None) == (y is None), path
        if x is not None:
            assert abs(x - y) <= tols[8][path] + tols[5][path], (path, x, y)

    same(a["frechet"]["fd"], b["frechet"]["fd"], "fd")
    for name in EV.EMOTIONS:
        for other in EV.EMOTIONS:
            same(a["fd_matrix"][name][other], b["fd_matrix"][name][other], f"fd.{name}.{other}")
        for side in ("real", "fake"):
            for key in FM.SPECTRUM_KEYS:
                same(a["spectrum"]["per_emotion"][name][side][key], b["spectrum"]["per_emotion"][name][side][key],
                     f"spectrum.{name}.{side}.{key}")
    for side in ("real", "fake"):
        for key in FM.SPECTRUM_KEYS:
            same(a["spectrum"][side][key], b["spectrum"][side][key], f"spectrum.{side}.{key}")


def test_cli_frechet(tmp_path):
    S, _, ed_cfg = spread_state(32, 4)
    ck, ed = save_state(S, str(tmp_path))
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "gan_config.yaml")))
    cfg.update(MAX_NOTES=32, LOG_DIR=str(tmp_path / "log"))
    cp, ep = tmp_path / "gan.yaml", tmp_path / "ed.yaml"
    cp.write_text(yaml.safe_dump(cfg))
    ep.write_text(yaml.safe_dump(ed_cfg))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    common = ["--config", str(cp), "--ckpt", ck, "--ed_config", str(ep), "--ed_ckpt", ed, "--synthetic", "40", "--batch", "16",
              "--seed", "7"]
    assert EV.main(common + ["--frechet", "--out", str(tmp_path / "refused.json")]) == 2       # needs --feature-metrics
    assert not (tmp_path / "refused.json").exists()
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, "-m", "melo_gan_amd.gan.evaluate", *common, "--feature-metrics",
                        "--frechet"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=450)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    rep = json.load(open(tmp_path / "log" / "eval.json"))
    fs = rep["feature_space"]
    assert rep["n"] == 40 and fs["dim"] == ed_cfg["notes_hidden"]
    fr = fs["frechet"]
    assert fr["fd"] > 0 and (fr["n_real"], fr["n_fake"], fr["rank_deficient"]) == (40, 40, True)
    assert fr["fd"] == pytest.approx(fr["mean_term"] + fr["trace_term"] - 2 * fr["sqrt_term"], rel=1e-12)
    assert set(fs["fd_matrix"]) == set(EV.EMOTIONS) == set(fs["spectrum"]["per_emotion"])
    assert all(1.0 <= fs["spectrum"][side]["effective_rank"] <= 39.0 + 1e-6 for side in ("real", "fake"))
    assert all("fd" in pe for pe in fs["per_emotion"].values())
    assert "frechet distance" in r.stdout and "fd, real emotion (row)" in r.stdout and "covariance spectrum" in r.stdout
