"""Host side of the generator's exponential moving average (melo_gan_amd/gan/ema.py, EMA_DECAY): the decay schedule and the
numpy restatement of mg_ema_flat held to hand-computed values, the config validation, the entry point's argument checks (no
launch happens, so no GPU is needed) and the checkpoint block's keys and dtypes."""
import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import melo_gan_amd  # noqa: F401
from melo_gan_amd.gan import ema as E


def test_decay_schedule_matches_hand_computed_values():
    # d_0 = (1 + 0) / (10 + 0) = 0.1 whatever the decay (above 0.1)
    assert E.ema_decay_at(0, 0.999, True) == 0.1 == E.ema_decay_at(0, 0.5, True)
    assert E.ema_decay_at(1, 0.999, True) == 2.0 / 11.0 and E.ema_decay_at(9, 0.999, True) == 10.0 / 19.0
    # (1 + t) / (10 + t) >= d  <=>  t >= (10 d - 1) / (1 - d): 8 for d = 0.5 (9 / 18), 890 for d = 0.99 (891 / 900)
    assert E.ema_decay_at(7, 0.5, True) == 8.0 / 17.0 < 0.5
    for t in (8, 9, 1000):
        assert E.ema_decay_at(t, 0.5, True) == 0.5
    assert E.ema_decay_at(889, 0.99, True) == 890.0 / 899.0 < 0.99
    for t in (890, 891, 10 ** 6):
        assert E.ema_decay_at(t, 0.99, True) == 0.99
    first = next(t for t in range(10 ** 5) if (1.0 + t) / (10.0 + t) >= 0.999)
    assert first == 8990 and E.ema_decay_at(first - 1, 0.999, True) < 0.999 == E.ema_decay_at(first, 0.999, True)
    # ramp off: the decay throughout; a decay below the ramp's first value is never raised
    for t in (0, 1, 5, 10 ** 4):
        assert E.ema_decay_at(t, 0.999, False) == 0.999
    assert E.ema_decay_at(0, 0.05, True) == 0.05 and E.ema_decay_at(0, 0.0, True) == 0.0


def test_ema_ref_matches_hand_computed_recurrence():
    p = [np.array([1.0, -2.0], np.float32), np.array([3.0, 0.5], np.float32)]
    s0 = np.array([0.0, 4.0])
    # ramp off, decay 0.5: s1 = s0 + 0.5 (p0 - s0) = [0.5, 1]; s2 = s1 + 0.5 (p1 - s1) = [1.75, 0.75]
    np.testing.assert_array_equal(E.ema_ref(p, 0.5, False, 0, 1, shadow0=s0), [1.75, 0.75])
    # ramp on, steps 1 and 2 from offset 0: d = 0.1 then 2/11
    s1 = s0 + (1.0 - 0.1) * (np.array([1.0, -2.0]) - s0)
    s2 = s1 + (1.0 - 2.0 / 11.0) * (np.array([3.0, 0.5]) - s1)
    np.testing.assert_array_equal(E.ema_ref(p, 0.999, True, 0, 1, shadow0=s0), s2)
    # the offset shifts the ramp: steps 8 and 9 from offset 7 are updates 0 and 1; explicit step lists are honoured
    np.testing.assert_array_equal(E.ema_ref(p, 0.999, True, 7, 8, shadow0=s0), s2)
    np.testing.assert_array_equal(E.ema_ref(p, 0.999, True, 7, [8, 9], shadow0=s0), s2)
    far = E.ema_ref(p, 0.5, True, 0, [5000, 5001], shadow0=s0)
    np.testing.assert_array_equal(far, [1.75, 0.75])
    # decay 0: the shadow is the last parameters exactly; shadow0 is not modified
    np.testing.assert_array_equal(E.ema_ref(p, 0.0, True, 0, 1, shadow0=s0), [3.0, 0.5])
    np.testing.assert_array_equal(s0, [0.0, 4.0])
    # an increment below half an ulp of an fp32 shadow still moves the fp64 one
    big = E.ema_ref([np.array([1.0 + 2.0 ** -20], np.float32)], 0.999, False, 0, 1, shadow0=np.array([1.0]))
    assert 1.0 < big[0] < 1.0 + 2.0 ** -24
    with pytest.raises(ValueError):
        E.ema_ref([np.zeros(2)], 0.5, False, 0, 1, shadow0=s0)             # fp64 parameters
    with pytest.raises(ValueError):
        E.ema_ref(p, 0.5, False, 0, [1], shadow0=s0)


@pytest.mark.parametrize("bad", [1.0, -0.1, "x", 1.5, float("nan"), None, True])
def test_config_validation_rejects_bad_decay(bad):
    with pytest.raises(ValueError, match="EMA_DECAY"):
        E.ema_config({"EMA_DECAY": bad})


def test_config_defaults_and_engine_validation():
    assert E.ema_config({}) == (0.0, True)
    assert E.ema_config({"EMA_DECAY": 0.999, "EMA_RAMP": False}) == (0.999, False)
    assert E.ema_config({"EMA_DECAY": 0}) == (0.0, True)
    with pytest.raises(ValueError, match="EMA_RAMP"):
        E.ema_config({"EMA_RAMP": "yes"})
    # the keys stay out of the pinned defaults, and the engine validates them before it touches a device
    from melo_gan_amd.gan import config as Cfg
    from melo_gan_amd.gan.engine import GanEngine
    assert "EMA_DECAY" not in Cfg.GAN_DEFAULTS and "EMA_RAMP" not in Cfg.GAN_DEFAULTS
    for bad in (1.0, -0.1, "x"):
        cfg = dict(Cfg.default_gan_cfg(8, 16, 4), EMA_DECAY=bad)
        with pytest.raises(ValueError, match="EMA_DECAY"):
            GanEngine(cfg, Cfg.default_ed_cfg(4), "cpu", 8)


def test_abi_exports_mg_ema_flat_and_rejects_bad_arguments_before_any_launch():
    import __graft_entry__ as ge
    ge.build()
    from melo_gan_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "mg_ema_flat") and "mg_ema_flat" in _lib.SIGNATURES
    src = open(os.path.join(os.path.dirname(__file__), "..", "include", "melo_gan_hip.h")).read()
    assert "int mg_ema_flat(const float* p, double* shadow, long n, double decay, int ramp" in src
    p, s, st = 256, 512, 1024          # non-null dummy addresses: nothing here launches
    assert lib.mg_ema_flat(p, s, 0, 0.5, 1, st, 0.0, None) == -1 and b"mg_ema_flat" in lib.mg_last_error()
    assert lib.mg_ema_flat(p, s, -4, 0.5, 1, st, 0.0, None) == -1
    for decay in (1.0, 1.5, -0.1, float("nan")):
        assert lib.mg_ema_flat(p, s, 8, decay, 1, st, 0.0, None) == -1 and b"decay" in lib.mg_last_error(), decay
    for args in ((None, s, st), (p, None, st), (p, s, None)):
        assert lib.mg_ema_flat(args[0], args[1], 8, 0.5, 0, args[2], 0.0, None) == -1 and b"null" in lib.mg_last_error()
    # the wrapper checks the same on the host, and refuses CPU tensors
    from melo_gan_amd import ops
    with pytest.raises(ValueError):
        ops.ema_flat(torch.zeros(4), torch.zeros(4, dtype=torch.float64), 4, 0.5, True, torch.zeros(4, dtype=torch.float64))


class _FlatStub:
    """What save_checkpoint / ema_block read of an engine, on the host."""

    def __init__(self, ema: bool):
        from melo_gan_amd.gan import config as Cfg
        from melo_gan_amd.gan.engine import FlatParams, discriminator_spec, feature_encoder_spec, generator_spec
        cfg = Cfg.default_gan_cfg(4, 16, 4)
        g = generator_spec(cfg["NOISE_DIM"], cfg["LATENT_DIM"], cfg["INTEGRATION_MODE"], 512, 16, 4, 128)
        e = feature_encoder_spec(6, (256, 128), 128)
        self.GE = FlatParams(OrderedDict([("G." + k, s) for k, s in g.items()] + [("E." + k, s) for k, s in e.items()]), "cpu")
        self.D = FlatParams(discriminator_spec(4, 256, 128), "cpu")
        gen = torch.Generator().manual_seed(3)
        self.GE.data.copy_(torch.randn(self.GE.data.shape, generator=gen))
        self.Gbuf = {f"decoder.deconv.{i}.running_{w}": torch.rand(c, generator=gen) for i, c in ((1, 128), (4, 64))
                     for w in ("mean", "var")}
        self.num_batches_tracked, self.betas, self.lr_g, self.lr_d = 5, (0.5, 0.9), 2e-4, 1e-4
        self.ema_decay, self.ema_ramp, self.ema_offset = (0.99, True, 3.0) if ema else (0.0, True, 0.0)
        self.ema = torch.randn(self.GE.n, dtype=torch.float64, generator=gen) if ema else None
        self.eng = self                 # stands in for the calibrating EvalEngine too

    def state_dicts(self):
        from melo_gan_amd.gan.engine import GanEngine
        self.ED, self.EDbuf = type("F", (), {"state_dict": lambda s: OrderedDict()})(), {}
        return GanEngine.state_dicts(self)

    def ema_state_dicts(self):
        from melo_gan_amd.gan.engine import GanEngine
        return GanEngine.ema_state_dicts(self)


def test_ema_block_keys_and_dtypes_survive_a_round_trip(tmp_path):
    from melo_gan_amd.gan import train_gan
    from melo_gan_amd.gan.eval_engine import ema_checkpoint
    from melo_gan_amd.gan.generate import GenerateError, check_generator_checkpoint
    from melo_gan_amd.gan import config as Cfg
    off, on = _FlatStub(False), _FlatStub(True)
    train_gan.save_checkpoint(off, str(tmp_path / "off.pth"), 1, full=True)
    ck = torch.load(tmp_path / "off.pth", map_location="cpu")
    assert list(ck) == ["epoch", "G", "D", "E_num", "opt_G", "opt_D"]          # exactly the keys of a run without averaging
    blk = train_gan.ema_block(on, on)
    train_gan.save_checkpoint(on, str(tmp_path / "on.pth"), 1, full=True, ema=blk)
    ck = torch.load(tmp_path / "on.pth", map_location="cpu")
    assert list(ck) == ["epoch", "G", "D", "E_num", "opt_G", "opt_D", "ema"]
    e = ck["ema"]
    assert set(e) == {"decay", "ramp", "offset", "G", "E_num"}
    assert (e["decay"], e["ramp"], e["offset"]) == (0.99, True, 3.0)
    assert list(e["G"]) == list(ck["G"]) and list(e["E_num"]) == list(ck["E_num"])
    for k, v in e["G"].items():
        want = torch.int64 if k.endswith("num_batches_tracked") else torch.float32 if "running_" in k else torch.float64
        assert v.dtype == want and v.shape == ck["G"][k].shape, k
    assert all(v.dtype == torch.float64 for v in e["E_num"].values())
    o, n = on.GE.offsets["G.decoder.pre.0.weight"]
    assert torch.equal(e["G"]["decoder.pre.0.weight"].flatten(), on.ema[o:o + n])
    assert torch.equal(e["G"]["decoder.deconv.1.running_var"], on.Gbuf["decoder.deconv.1.running_var"])
    # the final file: gan_final.pth's keys, float32
    train_gan.save_checkpoint(on, str(tmp_path / "final.pth"), full=False)
    train_gan.save_ema_final(blk, str(tmp_path / "final_ema.pth"))
    fin, fe = (torch.load(tmp_path / f, map_location="cpu") for f in ("final.pth", "final_ema.pth"))
    assert list(fe) == list(fin) == ["G", "E_num"] and list(fe["G"]) == list(fin["G"]) and list(fe["E_num"]) == list(fin["E_num"])
    for part in ("G", "E_num"):
        for k, v in fe[part].items():
            assert v.dtype == fin[part][k].dtype and torch.equal(v, e[part][k].to(v.dtype)), k
    # the loaders' view of the block; a checkpoint without one is refused by name
    cfg = Cfg.with_gan_defaults(Cfg.default_gan_cfg(4, 16, 4), require=False)
    check_generator_checkpoint(ema_checkpoint(ck, "on.pth", GenerateError), cfg, "on.pth")
    with pytest.raises(GenerateError, match="final.pth"):
        ema_checkpoint(fin, str(tmp_path / "final.pth"), GenerateError)
