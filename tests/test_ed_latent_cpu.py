"""Latent-mode emotion-discriminator pre-training, the parts that need no GPU: the oracle against the reference-generated
fixtures (tests/golden/make_golden_ed_latent.py), and the trainer's data rules for `input_mode: latent`
(ed_dataset.py:69-90,417-428)."""
import os

import numpy as np
import pytest
import torch

from oracle import melo_oracle as O

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = ["ed_latent_d64_b8", "ed_latent_d8_b5", "ed_latent_d32_h3_b7"]


def checksum(t):
    t = t.detach().double().flatten()
    w = torch.cos(0.11 * torch.arange(t.numel(), dtype=torch.float64))
    return np.array([t.sum().item(), (t * w).sum().item(), t.abs().sum().item()])


def latent_state(g):
    """Initial state of the fixtures (make_golden_ed_latent.py::initial_params)."""
    hidden = [int(h) for h in g["hidden"]]
    cfg = dict(O.default_ed_cfg(4), input_mode="latent", latent_dim=int(g["D"]), mlp_hidden=hidden, dropout=0.2)
    spec, _ = O.emotion_disc_spec(cfg)
    P = O.fill_params(spec, 9.0, O.norm_affine_names(spec))
    for v in P.values():
        if v.dim() >= 2:
            v.mul_(float(g["scale"]))
    return cfg, spec, P


def masks(g, it, n):
    return [torch.from_numpy(g[f"s{it}.dm{j}"]).float() / 0.8 for j in range(n)]


@pytest.mark.parametrize("name", CASES)
def test_oracle_latent_steps_match_reference(name):
    """The tolerances of tests/test_oracle_golden.py::test_ed_pretraining_steps_match_reference."""
    g = np.load(os.path.join(GOLD, name + ".npz"))
    cfg, spec, P = latent_state(g)
    n = len(cfg["mlp_hidden"])
    assert list(spec) == [f"classifier.net.{3 * j}.{p}" for j in range(n) for p in ("weight", "bias")] + ["classifier.head.weight",
                                                                                                        "classifier.head.bias"]
    opt = O.AdamState(P, 2e-4, (0.5, 0.999), 1e-8, weight_decay=0.01, decoupled=True)
    for it in range(int(g["n_steps"])):
        r = O.ed_step(P, {}, opt, torch.from_numpy(g[f"s{it}.x"]), torch.from_numpy(g[f"s{it}.y"]), cfg, masks(g, it, n))
        assert abs(r["loss"].item() - float(g[f"s{it}.loss"])) < 2e-6
        np.testing.assert_allclose(r["logits"].numpy(), g[f"s{it}.logits"], rtol=1e-4, atol=2e-6)
        if it == 0:
            np.testing.assert_allclose(r["grads"]["classifier.head.weight"].numpy(), g["s0.grad.head_w"], rtol=1e-4, atol=1e-7)
            np.testing.assert_allclose(r["grads"]["classifier.net.0.weight"].numpy(), g["s0.grad.net0_w"], rtol=2e-3,
                                       atol=1e-3 * float(np.abs(g["s0.grad.net0_w"]).max()))
    np.testing.assert_allclose(P["classifier.head.weight"].numpy(), g["end.head_w"], rtol=1e-4, atol=1e-6)
    assert set(f"end.{k}" for k in P) == set(k for k in g.files if k.startswith("end.")) - {"end.head_w", "end.eval_logits"}
    for k, v in P.items():
        ck, ref = checksum(v), g[f"end.{k}"]
        assert np.all(np.abs(ck - ref) <= 2e-4 * max(abs(ref[2]), 1e-12) + 1e-9), (k, ck, ref)
    logits = O.emotion_disc_fwd(P, {}, torch.from_numpy(g["s0.x"]), cfg)
    np.testing.assert_allclose(logits.numpy(), g["end.eval_logits"], rtol=1e-3, atol=1e-4)


def _write_split(root, stem, n, D, feats_rows=None, name="encoder_feats.npy"):
    d = os.path.join(root, stem)
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(n + len(stem))
    np.save(os.path.join(d, "emotion.npy"), np.array(["happy", "sad", "angry", "calm"] * n, dtype=object)[:n], allow_pickle=True)
    feats = rng.standard_normal((n if feats_rows is None else feats_rows, D)).astype(np.float32)
    np.save(os.path.join(d, name), feats)
    return feats


def test_latent_path_resolution_order(tmp_path):
    """ed_dataset.py:69-90: {split}_encoder_feats_path, then encoder_feats_path, then beside the split's arrays."""
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.emotion_discriminator import train_ed
    cfg = dict(splits_dir=str(tmp_path), train_split_csv="data/splits/train.csv", val_split_csv="data/splits/val.csv")
    beside = os.path.join(str(tmp_path), "train", "encoder_feats.npy")
    assert train_ed.resolve_encoder_feats(cfg, "train") == beside
    cfg["encoder_feats_path"] = "/somewhere/all.npy"
    assert train_ed.resolve_encoder_feats(cfg, "train") == "/somewhere/all.npy"
    assert train_ed.resolve_encoder_feats(cfg, "val") == "/somewhere/all.npy"
    cfg["train_encoder_feats_path"] = "/somewhere/train.npy"
    assert train_ed.resolve_encoder_feats(cfg, "train") == "/somewhere/train.npy"
    assert train_ed.resolve_encoder_feats(cfg, "val") == "/somewhere/all.npy"
    cfg["val_encoder_feats_path"] = ""                      # an empty key falls through, as in the reference
    assert train_ed.resolve_encoder_feats(cfg, "val") == "/somewhere/all.npy"
    with pytest.raises(ValueError, match="Missing split csv"):
        train_ed.resolve_encoder_feats(dict(splits_dir=str(tmp_path)), "train")


def test_latent_split_loads_rows_and_labels(tmp_path, capsys):
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.emotion_discriminator import train_ed
    from melo_gan_amd.gan.utils import emotion_to_index
    feats = _write_split(str(tmp_path), "train", 12, 8)
    cfg = dict(splits_dir=str(tmp_path), train_split_csv="x/train.csv", latent_dim=8, n_classes=4)
    x, y = train_ed.load_latent_split(cfg, "train", "cpu")
    assert x.dtype == torch.float32 and tuple(x.shape) == (12, 8) and torch.equal(x, torch.from_numpy(feats))
    assert y.dtype == torch.int64 and y.tolist() == [emotion_to_index(e) for e in ["happy", "sad", "angry", "calm"] * 3]
    assert "length OK (12) for CSV (12)" in capsys.readouterr().out
    # the explicit key wins over the file beside the arrays
    other = _write_split(str(tmp_path), "elsewhere", 12, 8)
    cfg["train_encoder_feats_path"] = os.path.join(str(tmp_path), "elsewhere", "encoder_feats.npy")
    x2, _ = train_ed.load_latent_split(cfg, "train", "cpu")
    assert torch.equal(x2, torch.from_numpy(other)) and not torch.equal(x2, x)
    cfg["train_encoder_feats_path"] = os.path.join(str(tmp_path), "missing.npy")
    with pytest.raises(FileNotFoundError):
        train_ed.load_latent_split(cfg, "train", "cpu")


def test_short_latent_array_drops_the_trailing_rows(tmp_path, capsys):
    """ed_dataset.py:422-425."""
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.emotion_discriminator import train_ed
    feats = _write_split(str(tmp_path), "train", 10, 8, feats_rows=7)
    cfg = dict(splits_dir=str(tmp_path), train_split_csv="x/train.csv", latent_dim=8)
    x, y = train_ed.load_latent_split(cfg, "train", "cpu")
    assert tuple(x.shape) == (7, 8) and tuple(y.shape) == (7,) and torch.equal(x, torch.from_numpy(feats))
    assert "[ed_dataset] encoder_feats ndarray shorter (7) than CSV (10): dropping last 3 rows." in capsys.readouterr().out
    f2, l2 = train_ed.latent_rows(np.zeros((9, 8), np.float64), list(range(4)), 8)      # longer: rows past the split are unused
    assert f2.shape == (4, 8) and f2.dtype == np.float32 and l2 == [0, 1, 2, 3]


def test_object_mapping_and_wrong_width_are_refused(tmp_path):
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.emotion_discriminator import train_ed
    _write_split(str(tmp_path), "train", 6, 8)
    d = os.path.join(str(tmp_path), "train")
    cfg = dict(splits_dir=str(tmp_path), train_split_csv="x/train.csv", latent_dim=16)
    with pytest.raises(ValueError, match=r"latent_dim = 16.*\(6, 8\)"):
        train_ed.load_latent_split(cfg, "train", "cpu")
    np.save(os.path.join(d, "encoder_feats.npy"), np.array({"a.npz": np.zeros(16, np.float32)}, dtype=object), allow_pickle=True)
    with pytest.raises(ValueError, match="per-file mapping"):
        train_ed.load_latent_split(cfg, "train", "cpu")
    with pytest.raises(ValueError, match="expected shape"):
        train_ed.latent_rows(np.zeros((6,), np.float32), [0] * 6, 16)
    with pytest.raises(ValueError, match="regular float array"):
        train_ed.latent_rows(np.array(["a", "b"]), [0, 1], 16)


def test_synthetic_latent_split_labels_the_quadrant():
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.emotion_discriminator import train_ed
    x, y = train_ed.synthetic_latent_split(4096, 8, 5, "cpu")
    ref = np.random.default_rng(5).standard_normal((4096, 8)).astype(np.float32)
    assert x.dtype == torch.float32 and torch.equal(x, torch.from_numpy(ref))
    assert torch.equal(y, 2 * (x[:, 0] > 0).long() + (x[:, 1] > 0).long())
    assert sorted(y.unique().tolist()) == [0, 1, 2, 3] and torch.bincount(y).min() > 900
    x2, _ = train_ed.synthetic_latent_split(64, 8, 6, "cpu")
    assert not torch.equal(x2, x[:64])


def test_train_accepts_a_latent_config(capsys):
    """A valid latent config gets as far as the device check (the trainer used to refuse everything but 'notes'); a bad
    input_mode is still a ValueError.  `augment: true` is accepted in latent mode and announced as a no-op."""
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.emotion_discriminator import train_ed
    cfg = dict(O.default_ed_cfg(4), input_mode="latent", latent_dim=8, batch_size=16, augment=True,
               augment_cfg=dict(not_a_notes_key=1.0))
    with pytest.raises(ValueError, match="input_mode"):
        train_ed.train(dict(cfg, input_mode="spectrogram"), synthetic=64)
    if torch.cuda.is_available():          # with a device the run itself is tests/test_ed_latent_gpu.py's
        return
    with pytest.raises(RuntimeError, match="MI355X"):
        train_ed.train(cfg, synthetic=64)
    assert "no effect with input_mode=latent" in capsys.readouterr().out


def test_engines_name_each_other():
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.emotion_discriminator.engine import EdEngine
    from melo_gan_amd.emotion_discriminator.latent_engine import EdLatentEngine, make_engine
    with pytest.raises(ValueError, match="EdLatentEngine"):
        EdEngine(dict(input_mode="latent"))
    with pytest.raises(ValueError, match="latent"):
        EdLatentEngine(dict(input_mode="notes"))
    with pytest.raises(ValueError, match="input_mode"):
        make_engine(dict(input_mode="other"))


def test_mlp_entry_points_reject_bad_arguments_before_any_launch():
    """The kernels' domain (1..4 hidden layers, widths 1..512, 2..32 classes, rows >= 1) is checked on the host: -1."""
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import _lib
    lib = _lib.load()

    def net(n_hidden=2, in_dim=64, widths=(256, 128), n_classes=4):
        c = _lib.MlpCls()
        c.n_hidden, c.in_dim, c.n_classes = n_hidden, in_dim, n_classes
        for i, h in enumerate(widths):
            c.width[i] = h
        return c

    def fwd(c, rows=8):
        return lib.mg_mlp_cls_fwd_bwd(c, rows, 256, 512, None, None, 0, None, 0, None, 0, 0, 0, 0.0, 0, None, None, 0.0, 0.0, 768, 1024,
                                      None, None)

    for bad, word in ((net(n_hidden=0), b"n_hidden"), (net(n_hidden=5), b"n_hidden"), (net(in_dim=0), b"in_dim"),
                      (net(in_dim=513), b"in_dim"), (net(widths=(256, 513)), b"width[1]"), (net(widths=(0, 8)), b"width[0]"),
                      (net(n_classes=1), b"n_classes"), (net(n_classes=33), b"n_classes")):
        assert fwd(bad) == -1 and word in lib.mg_last_error(), word
    assert fwd(net(), rows=0) == -1 and b"rows" in lib.mg_last_error()
    assert fwd(net()) == -1 and b"null weight" in lib.mg_last_error()           # in the domain, but no tensors
    assert lib.mg_mlp_cls_fwd_bwd(None, 8, 256, 512, None, None, 0, None, 0, None, 0, 0, 0, 0.0, 0, None, None, 0.0, 0.0, 768, 1024,
                                  None, None) == -1
    off = (_lib.i64 * 3)(0, 0, 0)
    assert lib.mg_mlp_cls_wgrad_update(net(n_classes=40), 8, 256, 512, off, off, 100, 768, None, None, None, 0, 0.0, 0.0, 0.0, 0.0, 0.0,
                                       None, 1024, 1280, None, None, None, None, None) == -1 and b"n_classes" in lib.mg_last_error()
