"""Held-out classifier evaluation (melo_gan_amd/emotion_discriminator/evaluate.py) on the GPU: the pass against the oracle's eval
forward and against the host restatement of its own stored logits, in both input modes and under spectral norm; robustness
passes against the clean pass; the CLI end to end; train_ed --eval-test leaves the training untouched."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import melo_oracle as O  # noqa: E402

K, T, N = 4, 32, 10


def notes_cfg(**kw):
    return {**O.default_ed_cfg(4), **dict(dropout=0.2, max_notes=T, batch_size=4, seed=3), **kw}


def latent_cfg(D=8, **kw):
    return dict(O.default_ed_cfg(4), input_mode="latent", latent_dim=D, dropout=0.2, batch_size=4, seed=3, **kw)


def model(cfg):
    """Closed-form weights as tests/test_ed_train_gpu.py builds them, BatchNorm running statistics away from (0, 1), and unit
    u / v for every spectrally normalised layer."""
    spec, bufs = O.emotion_disc_spec(cfg)
    P = O.fill_params(spec, 9.0, O.norm_affine_names(spec))
    for v in P.values():
        if v.dim() >= 2:
            v.mul_(4.0)
    Bf = {k: (torch.rand(s, generator=torch.Generator().manual_seed(1)) + 0.5 if k.endswith("running_var")
              else torch.randn(s, generator=torch.Generator().manual_seed(2)) * 0.1) for k, s in bufs.items()}
    if cfg.get("use_spectral_norm"):
        g = torch.Generator().manual_seed(11)
        for nm in O.ed_sn_layers(cfg):
            shp = spec[nm + ".weight"]
            Bf[nm + ".weight_u"] = torch.nn.functional.normalize(torch.randn(shp[0], generator=g), dim=0)
            Bf[nm + ".weight_v"] = torch.nn.functional.normalize(torch.randn(int(np.prod(shp[1:])), generator=g), dim=0)
    return P, Bf


def random_model(cfg, gain=2.0):
    """Normal weights of standard deviation gain / sqrt(fan_in): verdicts that differ between rows and move under noise (the
    closed-form weights give every row the same verdict)."""
    spec, bufs = O.emotion_disc_spec(cfg)
    g = torch.Generator().manual_seed(5)
    P = {}
    for k, s in spec.items():
        if len(s) >= 2:
            P[k] = torch.randn(s, generator=g) * gain / float(np.sqrt(np.prod(s[1:])))
        else:
            P[k] = torch.ones(s) if k.endswith("weight") else torch.zeros(s)
    return P, {k: (torch.ones(s) if k.endswith("running_var") else torch.zeros(s)) for k, s in bufs.items()}


def split(cfg, n=N):
    g = torch.Generator().manual_seed(7)
    if cfg["input_mode"] == "notes":
        x = torch.rand(n, T, 4, generator=g) * 2 - 1
    else:
        x = torch.randn(n, cfg["latent_dim"], generator=g)
    return x, torch.arange(n, dtype=torch.int64) % K


def same(a, b, path):
    if isinstance(a, dict):
        assert set(a) == set(b), (path, set(a) ^ set(b))
        for k in a:
            same(a[k], b[k], path + "/" + str(k))
    elif isinstance(a, list):
        assert len(a) == len(b), path
        for i, (u, v) in enumerate(zip(a, b)):
            same(u, v, f"{path}[{i}]")
    elif isinstance(a, float) and isinstance(b, float):
        assert abs(a - b) <= 1e-9 * max(abs(a), abs(b), 1e-6), (path, a, b)      # ratios of sums that agree to 1e-12
    else:
        assert a == b, (path, a, b)


def check_identity(ev, rep, labels):
    """The pass's accumulator, per-row numbers, pair counts and report against the host restatement computed from the
    evaluator's OWN stored logits: integers exactly, fp64 words to 1e-12 of the sum of |terms|, the report to 1e-9."""
    from melo_gan_amd.emotion_discriminator import metrics as M
    from test_cls_metrics_gpu import check
    logits, y = ev.logits.cpu().numpy(), labels.numpy()
    ref = M.host_cls_stats(logits, y, K, ev.n_bins, ev.inv_temps)
    got = (ev.acc_host, ev.rows["probs"], ev.rows["row_i"], ev.rows["row_d"])
    check(got, ref, f"evaluator B{ev.B}")
    assert np.array_equal(ev.probs.cpu().numpy().view(np.int64), ev.rows["probs"].view(np.int64))
    pairs = M.host_auroc_pairs(ev.rows["probs"], y, K)
    np.testing.assert_array_equal(ev.pairs, pairs)
    g = rep["calibrated"]["grid_index"]
    assert rep["calibrated"]["T"] == ev.T_grid[g]
    cal = M.host_cls_stats(logits, y, K, ev.n_bins, ev.inv_temps, inv_temperature=ev.inv_temps[g])
    check((ev.calibrated_host, cal[1], cal[2], cal[3]), cal, f"calibrated B{ev.B}")
    want = M.report(ref[0], pairs, ev.names, {"row_i": ref[2], "row_d": ref[3]}, y, cal[0])
    for key in ("overall", "per_class", "temperature", "hardest_rows", "n_bins"):
        same(rep[key], want[key], key)
    for key in ("overall", "per_class"):
        same(rep["calibrated"][key], want["calibrated"][key], "calibrated/" + key)
    assert rep["rows"] == len(y) and rep["overall"]["rows"] == int(((y >= 0) & (y < K)).sum())
    json.dumps(rep, allow_nan=False)
    return logits


def bits(acc):
    return {k: v.copy().view(np.int64) for k, v in acc.items()}


def test_notes_pass_matches_the_oracle_and_its_own_host_restatement():
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.emotion_discriminator.evaluate import EdEvaluator
    cfg = notes_cfg()
    P, Bf = model(cfg)
    x, y = split(cfg)
    ev = EdEvaluator(cfg, "cuda", 4)                            # 10 rows at batch 4: a padded tail
    ev.eng.load_state(P, Bf)
    dx, dy = x.cuda(), y.cuda()
    rep = ev.evaluate(dx, dy)
    logits = check_identity(ev, rep, y)
    want = O.emotion_disc_fwd(P, Bf, x, cfg, train=False)
    np.testing.assert_allclose(logits, want.numpy(), rtol=2e-3, atol=1e-4)
    assert rep["input_mode"] == "notes" and rep["batch"] == 4
    # a second and a third pass replay the captured graph: identical bits
    first, first_pairs, first_logits = bits(ev.acc_host), ev.pairs.copy(), logits.copy()
    for _ in range(2):
        ev.evaluate(dx, dy)
        again = bits(ev.acc_host)
        assert all(np.array_equal(first[k], again[k]) for k in first) and np.array_equal(first_pairs, ev.pairs)
        assert np.array_equal(first_logits.view(np.int32), ev.logits.cpu().numpy().view(np.int32))
    # `calibrated` at the grid's T = 1 entry reproduces the plain block bit for bit
    rep1 = ev.evaluate(dx, dy, calibrate_at=16)
    cal = bits(ev.calibrated_host)
    assert all(np.array_equal(first[k], cal[k]) for k in first)
    assert rep1["calibrated"]["T"] == 1.0 and rep1["calibrated"]["overall"] == {k: v for k, v in rep1["overall"].items()
                                                                                if k in rep1["calibrated"]["overall"]}
    # unlabelled rows count nowhere
    y2 = y.clone()
    y2[3], y2[8] = -1, K
    rep2 = ev.evaluate(dx, y2.cuda())
    check_identity(ev, rep2, y2)
    assert rep2["overall"]["rows"] == N - 2 and not ev.rows["probs"][[3, 8]].any()
    # batch 10: one whole batch, compared through the same identity only (the forward may round differently per batch size)
    ev10 = EdEvaluator(cfg, "cuda", 10)
    ev10.eng.load_state(P, Bf)
    check_identity(ev10, ev10.evaluate(dx, dy), y)


def test_latent_pass_and_robustness_refused():
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.emotion_discriminator.evaluate import EdEvaluateError, EdEvaluator
    cfg = latent_cfg(8)
    P, Bf = model(cfg)
    x, y = split(cfg)
    ev = EdEvaluator(cfg, "cuda", 4)
    ev.eng.load_state(P, Bf)
    rep = ev.evaluate(x.cuda(), y.cuda())
    logits = check_identity(ev, rep, y)
    np.testing.assert_allclose(logits, O.emotion_disc_fwd(P, Bf, x, cfg, train=False).numpy(), rtol=2e-3, atol=1e-4)
    assert rep["input_mode"] == "latent"
    with pytest.raises(EdEvaluateError, match="no augmentation"):
        ev.robustness(x.cuda(), y.cuda(), None, 1)
    with pytest.raises(EdEvaluateError, match="shape"):
        ev.evaluate(torch.zeros(4, 9, device="cuda"), y[:4].cuda())
    with pytest.raises(EdEvaluateError, match="empty"):
        ev.evaluate(torch.zeros(0, 8, device="cuda"), y[:0].cuda())


def test_robustness_against_the_clean_pass():
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.emotion_discriminator.evaluate import EdEvaluateError, EdEvaluator
    cfg = notes_cfg()
    x, y = split(cfg)
    ev = EdEvaluator(cfg, "cuda", 4)
    ev.eng.load_state(*random_model(cfg))
    dx, dy = x.cuda(), y.cuda()
    clean = ev.evaluate(dx, dy)
    clean_logits = ev.logits.cpu().numpy().copy()
    # all three strengths 0: every pass is the clean pass bit for bit
    rob = ev.robustness(dx, dy, dict(noise_std=0.0, dropout_prob=0.0, pitch_shift_prob=0.0), repeats=2)
    assert set(rob["passes"]) == {"noise_std", "dropout_prob", "pitch_shift_prob", "all"}
    for name, p in rob["passes"].items():
        assert p["flipped"] == 0 and p["flip_rate"] == 0.0 and p["rows"] == 2 * N, name
        assert p["accuracy"] == clean["overall"]["accuracy"], name
        assert abs(p["cross_entropy"] - clean["overall"]["cross_entropy"]) <= 1e-12 * clean["overall"]["cross_entropy"], name
    assert np.array_equal(ev.aug_logits.cpu().numpy().view(np.int32), clean_logits.view(np.int32))
    # noise: the flip count is the host's count from the two stored logit arrays
    rob = ev.robustness(dx, dy, dict(noise_std=1.0), repeats=1)
    assert np.array_equal(ev.logits.cpu().numpy().view(np.int32), clean_logits.view(np.int32))      # the clean pass is untouched
    aug = ev.aug_logits.cpu().numpy()                           # the last pass: "all" (here: the noise under other serials)
    assert not np.array_equal(aug, clean_logits)
    want = int((aug.astype(np.float64).argmax(axis=1) != clean_logits.astype(np.float64).argmax(axis=1)).sum())
    print("flips under noise_std 1.0:", rob["passes"]["noise_std"]["flipped"], "and", rob["passes"]["all"]["flipped"], "of", N, "host:", want)
    assert rob["passes"]["all"]["flipped"] == want and rob["passes"]["all"]["rows"] == N
    assert rob["passes"]["dropout_prob"]["flipped"] == 0 and rob["passes"]["pitch_shift_prob"]["flipped"] == 0
    assert rob["strengths"] == {"noise_std": 1.0, "dropout_prob": 0.0, "pitch_shift_prob": 0.0}
    with pytest.raises(EdEvaluateError, match="unknown"):
        ev.robustness(dx, dy, dict(tempo_jitter=0.1), 1)


def test_spectral_norm_checkpoint_loads_and_matches_the_oracle(tmp_path):
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.emotion_discriminator.evaluate import EdEvaluateError, EdEvaluator
    cfg = notes_cfg(use_spectral_norm=True)
    P, Bf = model(cfg)
    names = O.ed_sn_layers(cfg)
    sd = {}
    for k, v in P.items():
        nm = k[:-len(".weight")]
        sd[nm + ".weight_orig" if k.endswith(".weight") and nm in names else k] = v.clone()
    sd.update({k: v.clone() for k, v in Bf.items()})
    assert any(k.endswith("weight_orig") for k in sd) and any(k.endswith("weight_u") for k in sd)
    path = os.path.join(str(tmp_path), "ed_sn.pth")
    torch.save(sd, path)                                        # a bare state_dict, the reference's keys
    x, y = split(cfg)
    ev = EdEvaluator(cfg, "cuda", 4)
    ev.load(path)
    rep = ev.evaluate(x.cuda(), y.cuda())
    logits = check_identity(ev, rep, y)
    np.testing.assert_allclose(logits, O.emotion_disc_fwd(P, Bf, x, cfg, train=False).numpy(), rtol=2e-3, atol=1e-4)
    # the same file is not a checkpoint of the plain model
    plain = EdEvaluator(notes_cfg(), "cuda", 4)
    with pytest.raises(EdEvaluateError, match="encoder.conv.0.net.0.weight"):
        plain.load(path)


def write_cfg(tmp_path, cfg, name="ed.yaml"):
    import yaml
    path = os.path.join(str(tmp_path), name)
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path


def test_cli_end_to_end(tmp_path, capsys):
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.emotion_discriminator import evaluate as E
    from melo_gan_amd.emotion_discriminator.engine import EdEngine
    cfg = notes_cfg(checkpoint_dir=str(tmp_path), augment_cfg=dict(noise_std=0.02))
    path = write_cfg(tmp_path, cfg)
    probs_path = os.path.join(str(tmp_path), "out", "probs.npy")
    assert E.main(["--config", path, "--synthetic", "12", "--batch", "8", "--bins", "10", "--robustness", "1", "--save-probs",
                   probs_path, "--seed", "4"]) == 0
    rep = json.load(open(os.path.join(str(tmp_path), "ed_eval.json")))
    assert rep["rows"] == 12 and rep["n_bins"] == 10 and rep["split"] == "synthetic:12" and rep["batch"] == 8
    assert set(rep["per_class"]) == {"happy", "sad", "angry", "calm"} and len(rep["hardest_rows"]) == 10
    assert rep["robustness"]["strengths"] == {"noise_std": 0.02, "dropout_prob": 0.05, "pitch_shift_prob": 0.5}
    assert rep["robustness"]["passes"]["all"]["rows"] == 12
    probs = np.load(probs_path)
    assert probs.shape == (12, 4) and probs.dtype == np.float64 and (np.abs(probs.sum(axis=1) - 1) <= 1e-12).all()
    assert "classifier evaluation of synthetic:12" in capsys.readouterr().out
    # a checkpoint of another width: the error names the key
    other = EdEngine(dict(cfg, mlp_hidden=[64, 32]), "cuda", 4, T)
    other.init_weights(0)
    ck = os.path.join(str(tmp_path), "other.pth")
    torch.save({"epoch": 1, "model": other.state_dict(), "optimizer": {}, "cfg": cfg}, ck)
    ev = E.EdEvaluator(cfg, "cuda", 4)
    with pytest.raises(E.EdEvaluateError, match="classifier.net.0.weight"):
        ev.load(ck)
    assert E.main(["--config", path, "--model", ck, "--synthetic", "12"]) == 2
    assert "classifier.net.0.weight" in capsys.readouterr().err
    assert E.main(["--config", path]) == 2 and E.main(["--config", os.path.join(str(tmp_path), "none.yaml")]) == 2


def test_train_ed_eval_test_adds_the_report_and_changes_nothing_else(tmp_path, capsys):
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.emotion_discriminator import train_ed
    runs = {}
    for flag in (False, True):
        d = os.path.join(str(tmp_path), "with" if flag else "without")
        os.makedirs(d)
        cfg = notes_cfg(checkpoint_dir=d, save_name="ed_best.pth", batch_size=8, num_epochs=2, save_freq=1,
                        optimizer=dict(name="AdamW", lr=1e-3, betas=[0.5, 0.999], weight_decay=0.0), augment=True,
                        augment_cfg=dict(noise_std=0.01))
        path = write_cfg(tmp_path, cfg, f"ed_{int(flag)}.yaml")
        train_ed.main(["--config", path, "--synthetic", "24", "--epochs", "2"] + (["--eval-test"] if flag else []))
        runs[flag] = d
    out = capsys.readouterr().out
    assert out.count("[eval-test]") == 1
    files = {flag: sorted(os.listdir(d)) for flag, d in runs.items()}
    assert files[True] == sorted(files[False] + ["ed_eval.json"]) and "ed_epoch002.pth" in files[False]
    for name in files[False]:
        a, b = (torch.load(os.path.join(runs[f], name), map_location="cpu", weights_only=False) for f in (False, True))
        assert list(a["model"]) == list(b["model"])
        for k in a["model"]:
            assert torch.equal(a["model"][k], b["model"][k]), (name, k)
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a["optimizer"]["state"][k], b["optimizer"]["state"][k]), (name, k)
        assert a["epoch"] == b["epoch"]
    rep = json.load(open(os.path.join(runs[True], "ed_eval.json")))
    assert rep["split"] == "val" and rep["rows"] == 8 and rep["model"].endswith("ed_best.pth")
