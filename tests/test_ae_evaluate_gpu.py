"""Held-out VAE evaluation (melo_gan_amd/ae/evaluate.py) on the GPU: the pass against ae.encode, the oracle's eval forward and
the host reference of its own scattered arrays; the CLI end to end; train_ae --eval-every leaves the training untouched."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import melo_oracle as O  # noqa: E402

L, K = 8, 4
N = 10


def model(T):
    """Weights and buffers as tests/test_ae_gpu.py::test_latent_export_matches_the_oracle_encoder builds them."""
    spec, bufs = O.vae_spec(T, L)
    P = O.fill_params(spec, 6.0, O.norm_affine_names(spec))
    Bf = {k: (torch.rand(s, generator=torch.Generator().manual_seed(1)) + 0.5 if k.endswith("running_var")
              else torch.randn(s, generator=torch.Generator().manual_seed(2)) * 0.1) for k, s in bufs.items()}
    return P, Bf


def cfg_of(T, B=4):
    return dict(MAX_NOTES=T, LATENT_DIM=L, BATCH_SIZE=B, LR=1e-4, WEIGHT_DECAY=1e-5)


def split(T):
    notes = torch.rand(N, T, 4, generator=torch.Generator().manual_seed(7)) * 2 - 1
    return notes, torch.arange(N, dtype=torch.int64) % K


def check_identity(ev, rep, notes, labels):
    """The pass's accumulator, per-row numbers and report against the host reference computed from the evaluator's OWN
    scattered recon / mu / logvar: integers exactly, fp64 words to 1e-12 of the sum of |terms|."""
    from melo_gan_amd.ae import metrics as M
    from test_vae_metrics_gpu import check
    mu, lv, recon = ev.mu.cpu().numpy(), ev.logvar.cpu().numpy(), ev.recon.cpu().numpy()
    y = labels.numpy()
    ref, ref_d, ref_i = M.host_vae_stats(notes.numpy(), recon, mu, lv, y, K)
    check(ev.acc_host, ev.rows["row_d"], ev.rows["row_i"], ref, ref_d, ref_i, mu, lv, y, K, f"evaluator B{ev.B}")
    want = M.report(ref, ev.eng.T, L)

    def same(a, b, path):
        if isinstance(a, dict):
            assert set(a) == set(b), path
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

    for key in ("overall", "per_class"):
        same(rep[key], want[key], key)
    assert rep["rows"] == N and rep["overall"]["rows"] == N and rep["overall"]["positions"]["valid"] == N * ev.eng.T
    return recon, mu


def test_pass_matches_encode_the_oracle_and_its_own_host_reference():
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.ae import encode as E
    from melo_gan_amd.ae.engine import VaeEngine
    from melo_gan_amd.ae.evaluate import VaeEvaluator
    T = 32
    P, Bf = model(T)
    notes, labels = split(T)
    ev = VaeEvaluator(cfg_of(T), "cuda", 4)                     # 10 rows at batch 4: a padded tail
    ev.eng.load_state(P, Bf)
    dev_notes, dev_labels = notes.cuda(), labels.cuda()
    rep = ev.evaluate(dev_notes, dev_labels, keep_recon=True)
    recon, mu = check_identity(ev, rep, notes, labels)
    enc = VaeEngine(cfg_of(T), "cuda", 4)
    enc.load_state(P, Bf)
    assert np.array_equal(mu.view(np.int32), E.encode(enc, notes.cuda()).view(np.int32))      # bit for bit
    rec_ref, _, mu_ref, _ = O.vae_fwd(P, Bf, notes, torch.zeros(N, L), T, train=False)
    np.testing.assert_allclose(mu, mu_ref.numpy(), rtol=2e-3, atol=2e-5)
    np.testing.assert_allclose(recon, rec_ref.numpy(), rtol=1e-3, atol=1e-5)
    assert "deterministic" in rep["reconstruction"]
    # a second pass replays the captured graph: identical bits
    first = {k: v.copy() for k, v in ev.acc_host.items()}
    ev.evaluate(dev_notes, dev_labels, keep_recon=True)
    for k in first:
        assert np.array_equal(first[k].view(np.int64), ev.acc_host[k].view(np.int64)), k
    # batch 10: one whole batch, compared through the same identity only (the forward may round differently per batch size)
    ev10 = VaeEvaluator(cfg_of(T), "cuda", 10)
    ev10.eng.load_state(P, Bf)
    check_identity(ev10, ev10.evaluate(notes.cuda(), labels.cuda(), keep_recon=True), notes, labels)


def test_max_notes_not_a_multiple_of_8_counts_the_zero_padded_tail():
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.ae.evaluate import VaeEvaluator
    T = 20
    P, Bf = model(T)
    notes, labels = split(T)
    ev = VaeEvaluator(cfg_of(T), "cuda", 4)
    ev.eng.load_state(P, Bf)
    rep = ev.evaluate(notes.cuda(), labels.cuda(), keep_recon=True)
    recon, mu = check_identity(ev, rep, notes, labels)
    rec_ref, _, mu_ref, _ = O.vae_fwd(P, Bf, notes, torch.zeros(N, L), T, train=False)
    np.testing.assert_allclose(mu, mu_ref.numpy(), rtol=2e-3, atol=2e-5)
    np.testing.assert_allclose(recon, rec_ref.numpy(), rtol=1e-3, atol=1e-5)
    assert not rec_ref[:, 16:].any() and not recon[:, 16:].any()           # the reference pads the reconstruction with zeros
    d = recon.astype(np.float64) - notes.numpy().astype(np.float64)
    mse = float((d * d).mean())                                             # F.mse_loss over all T positions, tail included
    assert abs(rep["overall"]["recon_mse"] - mse) <= 1e-12 * mse


def test_cli_end_to_end(tmp_path):
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import midi
    from melo_gan_amd.ae import encode as E
    from melo_gan_amd.ae import evaluate as EV
    from melo_gan_amd.ae.engine import VaeEngine
    state_dict = VaeEngine.state_dict
    T = 32
    P, Bf = model(T)
    notes, labels = split(T)
    # rows a .mid file can hold (save_recon_midi reads a row as pitch, start, duration, velocity): onsets >= 0, durations > 0
    notes[..., 1] = notes[..., 1].abs()
    notes[..., 2] = notes[..., 2].abs() * 0.95 + 0.05
    src = VaeEngine(cfg_of(T), "cuda", 4)
    src.load_state(P, Bf)
    ckpt = str(tmp_path / "ae_best.pth")
    torch.save({"epoch": 3, "model_state": state_dict(src)}, ckpt)
    os.makedirs(tmp_path / "splits" / "val")
    os.makedirs(tmp_path / "bare")
    npy = str(tmp_path / "splits" / "val" / "notes.npy")
    np.save(npy, notes.numpy())
    np.save(str(tmp_path / "bare" / "notes.npy"), notes.numpy())
    names = np.array(["happy", "sad", "angry", "calm"])
    np.save(str(tmp_path / "splits" / "val" / "emotion.npy"), names[labels.numpy()])
    cfg_path = str(tmp_path / "ae.yaml")
    with open(cfg_path, "w") as f:
        f.write(f"MAX_NOTES: {T}\nLATENT_DIM: {L}\nBATCH_SIZE: 4\nLR: 1.0e-4\nWEIGHT_DECAY: 1.0e-5\n"
                f"SPLITS_DIR: {tmp_path / 'splits'}\nLOG_DIR: {tmp_path / 'log'}\n")
    lat = str(tmp_path / "lat" / "mu.npy")
    assert EV.main(["--config", cfg_path, "--model", ckpt, "--batch", "4", "--save-latents", lat, "--recon-midi", "1"]) == 0
    rep = json.load(open(tmp_path / "log" / "ae_eval.json"))
    keys = {"recon_mse", "recon_mse_per_channel", "recon_mae_per_channel", "kld_mean", "kl_per_dim", "kl_per_sample", "mu_mean",
            "mu_var", "mean_posterior_var", "active_units", "collapsed_dims", "latent_std", "onset_precision", "onset_recall",
            "pitch_accuracy", "pitch_within_1", "pitch_class_accuracy", "mean_abs_pitch_error", "mean_abs_velocity_error",
            "mean_abs_dur_beats", "mean_abs_step_beats"}
    assert keys | {"fisher_ratio", "fisher_ratio_mean"} <= set(rep["overall"])
    assert set(rep["per_class"]) == {"happy", "sad", "angry", "calm"} and all(keys <= set(b) for b in rep["per_class"].values())
    assert [rep["per_class"][n]["rows"] for n in names] == [3, 3, 2, 2] and rep["rows"] == N
    assert len(rep["overall"]["fisher_ratio"]) == L and rep["overall"]["fisher_ratio_mean"] is not None
    # --save-latents is the array ae.encode writes
    enc_out = str(tmp_path / "feats" / "encoder_feats.npy")
    E.main(["--model", ckpt, "--notes", npy, "--out_file", enc_out, "--config", cfg_path])
    assert np.array_equal(np.load(lat).view(np.int32), np.load(enc_out).view(np.int32))
    # --recon-midi 1: the worst and the best row, input and reconstruction
    md = rep["recon_midi"]
    files = sorted(os.listdir(md["dir"]))
    assert len(files) == 4 and all(f.endswith(".mid") for f in files)
    assert sorted(f for t in ("worst", "best") for f in md[t][0]["files"]) == files
    assert md["worst"][0]["squared_error"] >= md["best"][0]["squared_error"] and md["worst"][0]["row"] != md["best"][0]["row"]
    for f in files:
        hdr, tempo, parsed = midi.read_smf_notes(os.path.join(md["dir"], f))
        assert hdr[0] == 1 and tempo > 0 and isinstance(parsed, list)
    # without emotion.npy: one overall block, no Fisher ratio
    out2 = str(tmp_path / "log" / "bare.json")
    assert EV.main(["--config", cfg_path, "--model", ckpt, "--batch", "4", "--split", str(tmp_path / "bare" / "notes.npy"),
                    "--out", out2]) == 0
    rep2 = json.load(open(out2))
    assert "per_class" not in rep2 and rep2["overall"]["fisher_ratio"] is None and rep2["overall"]["rows"] == N
    assert abs(rep2["overall"]["recon_mse"] - rep["overall"]["recon_mse"]) <= 1e-12 * rep["overall"]["recon_mse"]
    # errors come as one type: a config that does not fit the checkpoint, an empty split
    bad_cfg = str(tmp_path / "bad.yaml")
    with open(bad_cfg, "w") as f:
        f.write(f"MAX_NOTES: {T}\nLATENT_DIM: 16\nSPLITS_DIR: {tmp_path / 'splits'}\nLOG_DIR: {tmp_path / 'log'}\n")
    with pytest.raises(EV.AeEvaluateError, match="shape"):
        EV.run(EV.parse_args(["--config", bad_cfg, "--model", ckpt]))
    os.makedirs(tmp_path / "empty")
    np.save(str(tmp_path / "empty" / "notes.npy"), np.zeros((0, T, 4), np.float32))
    with pytest.raises(EV.AeEvaluateError):
        EV.run(EV.parse_args(["--config", cfg_path, "--model", ckpt, "--split", str(tmp_path / "empty" / "notes.npy")]))
    assert EV.main(["--config", cfg_path, "--model", str(tmp_path / "nope.pth")]) == 2


def test_train_ae_eval_every_leaves_the_training_untouched(tmp_path):
    import yaml
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.ae import train_ae
    base = yaml.safe_load(open(os.path.join(os.path.dirname(__file__), "..", "config", "ae_config.yaml")))
    finals = []
    for tag, extra in (("with", ["--eval-every", "1"]), ("without", [])):
        cfg = dict(base)
        cfg.update(MAX_NOTES=32, BATCH_SIZE=8, CHECKPOINT_DIR=str(tmp_path / tag / "ck"), LOG_DIR=str(tmp_path / tag / "log"),
                   RECON_DIR=str(tmp_path / tag / "recon"), SPLITS_DIR=str(tmp_path / "no_splits"))
        p = tmp_path / f"{tag}.yaml"
        p.write_text(yaml.safe_dump(cfg))
        torch.manual_seed(0)                    # the trainer draws eps from the default generator
        train_ae.main(["--config", str(p), "--synthetic", "32", "--epochs", "2"] + extra)
        finals.append(torch.load(tmp_path / tag / "ck" / "ae_final.pth", map_location="cpu"))
    a, b = finals
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    logs = {tag: b"".join(open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(tmp_path / tag / "log") for f in fs)
            for tag in ("with", "without")}
    assert b"val/active_units" in logs["with"] and b"val/pitch_accuracy" in logs["with"] and b"val/onset_recall" in logs["with"]
    assert b"val/" not in logs["without"] and b"loss/val_total" in logs["without"]
