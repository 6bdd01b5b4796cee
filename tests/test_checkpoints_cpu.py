"""CPU: what the trainers and tools read back from disk -- the three kinds of .pth file (GAN, VAE, emotion classifier), the
label files, the VAE split arrays and the YAML configs -- over host stand-ins for the engines (FlatParams on the CPU): which
files load, and the literal text every reader refuses the others with, per error class."""
import functools
import os
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import melo_gan_amd  # noqa: F401
from melo_gan_amd import checkpoints as CK
from melo_gan_amd.ae import edit as AED
from melo_gan_amd.ae import encode as AENC
from melo_gan_amd.ae import evaluate as AEV
from melo_gan_amd.ae import train_ae
from melo_gan_amd.ae.edit import AeEditError
from melo_gan_amd.ae.engine import VaeEngine, vae_spec
from melo_gan_amd.ae.evaluate import AeEvaluateError
from melo_gan_amd.emotion_discriminator import evaluate as EDV
from melo_gan_amd.emotion_discriminator import predict as PRED
from melo_gan_amd.emotion_discriminator.engine import EdEngine
from melo_gan_amd.emotion_discriminator.evaluate import EdEvaluateError
from melo_gan_amd.gan import evaluate as GEV
from melo_gan_amd.gan import train_gan
from melo_gan_amd.gan.config import read_config
from melo_gan_amd.gan.engine import GanEngine
from melo_gan_amd.gan.evaluate import EvaluateError
from melo_gan_amd.gan.generate import GenerateError
from melo_gan_amd.gan.morph import MorphError
from melo_gan_amd.params import (FlatParams, discriminator_spec, emotion_disc_spec, feature_encoder_spec, generator_spec,
                                 norm_buffers)

load_checkpoint = lambda path, err: CK.read_checkpoint(path, err, weights_only=None)  # noqa: E731
check_generator_checkpoint, ema_checkpoint = CK.check_generator_checkpoint, CK.ema_checkpoint
vae_state_dict = VaeEngine.state_dict
LOAD_LABELS = {err: functools.partial(AEV._load_labels, err=err) for err in (AeEvaluateError, AeEditError)}
LOAD_NOTES = {AeEditError: functools.partial(AEV._load_notes, err=AeEditError)}
GAN_ERRORS = (GenerateError, MorphError, EvaluateError)

GAN_CFG = dict(NOISE_DIM=8, LATENT_DIM=4, MAX_NOTES=8, NOTE_DIM=4, NUMERIC_INPUT_DIM=6, ENCODER_OUT_DIM=8, ENCODER_HIDDEN=[8, 8],
               INTEGRATION_MODE="conditioning")
ED_CFG = dict(input_mode="notes", note_dim=4, notes_hidden=8, notes_blocks=1, mlp_hidden=[8], n_classes=4)


def _fill(fp, seed):
    fp.data.copy_(torch.randn(fp.data.shape, generator=torch.Generator().manual_seed(seed)))


def _text_file(tmp_path, name="notes.txt"):
    p = tmp_path / name
    p.write_text("not a checkpoint\n")
    return str(p)


def _msg(e):
    return e.value.args[0]


# ---- host stand-ins -------------------------------------------------------------------------------------------------
class GanStub:
    """What the GAN checkpoint functions read and write of a GanEngine."""

    def __init__(self, seed=0, ema=False, sn=False):
        g = generator_spec(8, 4, "conditioning", 512, 8, 4, 8)
        e = feature_encoder_spec(6, (8, 8), 8)
        self.GE = FlatParams(OrderedDict([("G." + k, s) for k, s in g.items()] + [("E." + k, s) for k, s in e.items()]), "cpu")
        self.D = FlatParams(discriminator_spec(4, 256, 8), "cpu")
        edspec, edbufs, _ = emotion_disc_spec(ED_CFG)
        self.ED, self.EDbuf = FlatParams(edspec, "cpu", with_opt=False), norm_buffers(edbufs, "cpu")
        gen = torch.Generator().manual_seed(100 + seed)
        for i, fp in enumerate((self.GE, self.D)):
            _fill(fp, 10 * seed + i)
            fp.m.copy_(torch.randn(fp.m.shape, generator=gen))
            fp.v.copy_(torch.rand(fp.v.shape, generator=gen))
        self.Gbuf = {f"decoder.deconv.{i}.running_{w}": torch.rand(c, generator=gen) for i, c in ((1, 128), (4, 64))
                     for w in ("mean", "var")}
        self.num_batches_tracked, self.betas, self.lr_g, self.lr_d = 5 + seed, (0.5, 0.9), 2e-4, 1e-4
        self.ema_decay, self.ema_ramp, self.ema_offset = (0.99, True, 3.0) if ema else (0.0, True, 0.0)
        self.ema = torch.randn(self.GE.n, dtype=torch.float64, generator=gen) if ema else None
        self.eng = self                 # stands in for the calibrating EvalEngine too
        self.calls = []

    state_dicts, ema_state_dicts = GanEngine.state_dicts, GanEngine.ema_state_dicts

    def params_changed(self):
        self.calls.append("params_changed")

    def fold_ed(self):
        self.calls.append("fold_ed")

    def ema_reset(self, shadow=None, offset=None):
        self.calls.append("ema_reset")
        if self.ema is not None:
            self.ema.copy_(self.GE.data[:self.GE.n] if shadow is None else shadow)
            self.ema_offset = float(self.GE.state[0].item() if offset is None else offset)


class VaeStub:
    def __init__(self, seed=0):
        spec, bufs, _, _ = vae_spec(8, 4)
        self.P, self.buf = FlatParams(spec, "cpu"), norm_buffers(bufs, "cpu")
        self.T, self.latent, self.num_batches_tracked = 8, 4, 3
        _fill(self.P, seed)
        for i, v in enumerate(self.buf.values()):
            v.add_(0.25 * (i + 1) + seed)

    load_state = VaeEngine.load_state


class EdStub:
    input_mode = "notes"
    load_state, state_dict, _sn_keys = EdEngine.load_state, EdEngine.state_dict, EdEngine._sn_keys

    def __init__(self, seed=0, sn=False):
        self.cfg = dict(ED_CFG, use_spectral_norm=sn)
        spec, bufs, self.chans = emotion_disc_spec(self.cfg)
        self.P, self.buf = FlatParams(spec, "cpu"), norm_buffers(bufs, "cpu")
        self.sn_names = ["encoder.conv.0.net.0", "classifier.net.0"] if sn else []
        gen = torch.Generator().manual_seed(50 + seed)
        for nm in self.sn_names:
            shp = spec[nm + ".weight"]
            self.buf[nm + ".weight_u"] = torch.randn(shp[0], generator=gen)
            self.buf[nm + ".weight_v"] = torch.randn(int(np.prod(shp[1:])), generator=gen)
        _fill(self.P, 20 + seed)
        self.buf["encoder.conv.0.net.1.running_var"].add_(0.5 + seed)


def _loader(cls, eng):
    """cls.load bound to an object that holds nothing but the engine (and, for the classifier, load_state)."""
    ns = {"load": cls.load}
    if hasattr(cls, "load_state"):
        ns["load_state"] = cls.load_state
    obj = type("Holder", (), ns)()
    obj.eng, obj.acc_host = eng, "stale"
    return obj


# ---- GAN kind: reading ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("err", GAN_ERRORS)
def test_gan_checkpoint_missing_or_unreadable(tmp_path, err):
    p = str(tmp_path / "none.pth")
    with pytest.raises(err) as e:
        load_checkpoint(p, err)
    assert _msg(e) == f"checkpoint {p} does not exist"
    t = _text_file(tmp_path)
    with pytest.raises(err) as e:
        load_checkpoint(t, err)
    assert _msg(e).startswith(f"cannot read checkpoint {t}: ")


@pytest.fixture(scope="module")
def gan_ck(tmp_path_factory):
    d = tmp_path_factory.mktemp("gan_ck")
    src = GanStub(1, ema=True)
    for fp in (src.GE, src.D):
        fp.state[0], fp.state[1], fp.state[2] = 7.0, 0.5 ** 7, 0.9 ** 7
    train_gan.save_checkpoint(src, str(d / "full.pth"), 3, full=True, ema=train_gan.ema_block(src, src))
    train_gan.save_checkpoint(src, str(d / "final.pth"), full=False)
    return SimpleNamespace(src=src, full=str(d / "full.pth"), final=str(d / "final.pth"))


@pytest.mark.parametrize("err", GAN_ERRORS)
def test_generator_checkpoint_check_texts(gan_ck, err):
    ck = load_checkpoint(gan_ck.final, err)
    check_generator_checkpoint(ck, GAN_CFG, "f.pth", err)
    check_generator_checkpoint(ema_checkpoint(load_checkpoint(gan_ck.full, err), "f.pth", err), GAN_CFG, "f.pth", err)
    with pytest.raises(err) as e:
        check_generator_checkpoint({"D": {}}, GAN_CFG, "f.pth", err)
    assert _msg(e) == "f.pth: not a generator checkpoint (needs 'G' and 'E_num'; has ['D'])"
    with pytest.raises(err) as e:
        check_generator_checkpoint([1], GAN_CFG, "f.pth", err)
    assert _msg(e) == "f.pth: not a generator checkpoint (needs 'G' and 'E_num'; has list)"
    bad = {"G": {k: v for k, v in ck["G"].items() if k != "decoder.pre.0.bias"}, "E_num": ck["E_num"]}
    with pytest.raises(err) as e:
        check_generator_checkpoint(bad, GAN_CFG, "f.pth", err)
    assert _msg(e) == "f.pth: G lacks decoder.pre.0.bias"
    bad = {"G": {k: v for k, v in ck["G"].items() if k != "decoder.deconv.4.running_var"}, "E_num": ck["E_num"]}
    with pytest.raises(err) as e:
        check_generator_checkpoint(bad, GAN_CFG, "f.pth", err)
    assert _msg(e) == "f.pth: G lacks decoder.deconv.4.running_var"
    bad = {"G": ck["G"], "E_num": dict(ck["E_num"], **{"net.0.weight": torch.zeros(3)})}
    with pytest.raises(err) as e:
        check_generator_checkpoint(bad, GAN_CFG, "f.pth", err)
    assert _msg(e) == "f.pth: E_num.net.0.weight has shape (3,), the GAN config implies (6,)"
    with pytest.raises(err) as e:
        ema_checkpoint(ck, "f.pth", err)
    assert _msg(e) == ("f.pth: no averaged weights in this checkpoint (--ema reads the 'ema' block of a full gan_epochNNNN.pth "
                       "written with EMA_DECAY > 0; has ['E_num', 'G']).  A *_ema.pth file loads without the flag")


def test_critic_checkpoint_check_texts(gan_ck):
    cfg = dict(GAN_CFG)
    full, final = load_checkpoint(gan_ck.full, EvaluateError), load_checkpoint(gan_ck.final, EvaluateError)
    assert GEV.check_checkpoint(full, cfg, "f.pth") is True and GEV.check_checkpoint(final, cfg, "f.pth") is False
    bad = dict(full, D={k: v for k, v in full["D"].items() if k != "conv.0.bias"})
    with pytest.raises(EvaluateError) as e:
        GEV.check_checkpoint(bad, cfg, "f.pth")
    assert _msg(e) == "f.pth: D lacks conv.0.bias"
    bad = dict(full, D=dict(full["D"], **{"conv.0.bias": torch.zeros(3)}))
    with pytest.raises(EvaluateError) as e:
        GEV.check_checkpoint(bad, cfg, "f.pth")
    assert _msg(e) == "f.pth: D.conv.0.bias has shape (3,), the GAN config implies (64,)"
    with pytest.raises(EvaluateError) as e:
        GEV.check_checkpoint({"D": full["D"]}, cfg, "f.pth")
    assert _msg(e) == "f.pth: not a generator checkpoint (needs 'G' and 'E_num'; has ['D'])"


# ---- GAN kind: save, then resume ------------------------------------------------------------------------------------
def _beta_powers(step, betas):
    """The update kernels' running powers: an fp64 product, one factor per step, of the betas rounded to fp32."""
    b1, b2 = (torch.tensor(float(b), dtype=torch.float32).item() for b in betas)
    p1 = p2 = 1.0
    for _ in range(step):
        p1 *= b1
        p2 *= b2
    return p1, p2


def test_save_then_resume_restores_everything(gan_ck, capsys):
    src = gan_ck.src
    ck = load_checkpoint(gan_ck.full, GenerateError)
    assert list(ck) == ["epoch", "G", "D", "E_num", "opt_G", "opt_D", "ema"] and ck["epoch"] == 3
    sd = src.state_dicts()
    for part in ("G", "D", "E_num"):
        assert list(ck[part]) == list(sd[part])
        assert all(torch.equal(ck[part][k], sd[part][k]) and ck[part][k].dtype == sd[part][k].dtype for k in sd[part]), part
    assert list(load_checkpoint(gan_ck.final, GenerateError)) == ["G", "E_num"]
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(s)) for s in src.D.spec.values()], lr=1.0)
    opt.load_state_dict(ck["opt_D"])                                    # a real torch optimiser takes the block as it is
    assert opt.state_dict()["param_groups"][0]["lr"] == 1e-4 and opt.state_dict()["param_groups"][0]["betas"] == (0.5, 0.9)
    dst = GanStub(2, ema=True)
    assert train_gan.resume_checkpoint(dst, gan_ck.full) == 3
    for a, b in ((dst.GE, src.GE), (dst.D, src.D)):
        n = a.n                                                         # behind it: padding, which no file holds
        assert torch.equal(a.data[:n], b.data[:n]) and torch.equal(a.m[:n], b.m[:n]) and torch.equal(a.v[:n], b.v[:n])
        assert a.state[:3].tolist() == [7.0, *_beta_powers(7, (0.5, 0.9))]
    assert all(torch.equal(dst.Gbuf[k], src.Gbuf[k]) for k in src.Gbuf) and dst.num_batches_tracked == src.num_batches_tracked
    assert torch.equal(dst.ema, src.ema) and dst.ema_offset == 3.0 and dst.calls == ["params_changed", "ema_reset"]
    # no averaging in the resuming run: the block is named and ignored; averaging on, no block: it starts at the resumed weights
    off = GanStub(3)
    train_gan.resume_checkpoint(off, gan_ck.full)
    assert f"[WARN] {gan_ck.full} holds averaged weights ('ema') but EMA_DECAY is 0" in capsys.readouterr().out
    plain = str(os.path.join(os.path.dirname(gan_ck.full), "plain.pth"))
    train_gan.save_checkpoint(src, plain, 4, full=True)
    on = GanStub(4, ema=True)
    assert train_gan.resume_checkpoint(on, plain) == 4 and torch.equal(on.ema, src.GE.data[:src.GE.n].double())


def test_resume_refusals(gan_ck, tmp_path):
    with pytest.raises(KeyError) as e:
        train_gan.resume_checkpoint(GanStub(2), gan_ck.final)
    assert _msg(e) == f"{gan_ck.final}: not a full training checkpoint (no 'D')"
    ck = load_checkpoint(gan_ck.full, GenerateError)
    ck["ema"]["G"]["decoder.pre.0.bias"] = torch.zeros(3, dtype=torch.float64)
    p = str(tmp_path / "bad_ema.pth")
    torch.save(ck, p)
    with pytest.raises(ValueError) as e:
        train_gan.resume_checkpoint(GanStub(2, ema=True), p)
    assert _msg(e) == f"{p}: ema.G.decoder.pre.0.bias: shape (3,) != (512,)"
    with pytest.raises(Exception):
        train_gan.resume_checkpoint(GanStub(2), str(tmp_path / "none.pth"))
    with pytest.raises(Exception):
        train_gan.resume_checkpoint(GanStub(2), _text_file(tmp_path))


# ---- VAE kind -------------------------------------------------------------------------------------------------------
VAE_READERS = ((AEV.VaeEvaluator, AeEvaluateError), (AED.LatentEditor, AeEditError))


@pytest.fixture(scope="module")
def vae_ck(tmp_path_factory):
    d = tmp_path_factory.mktemp("vae_ck")
    src = VaeStub(1)
    sd = vae_state_dict(src)
    torch.save({"epoch": 2, "model_state": sd}, d / "ae_best.pth")
    torch.save(sd, d / "ae_final.pth")
    return SimpleNamespace(src=src, sd=sd, best=str(d / "ae_best.pth"), final=str(d / "ae_final.pth"))


def _same_vae(a, b):
    return torch.equal(a.P.data[:a.P.n], b.P.data[:b.P.n]) and all(torch.equal(a.buf[k], b.buf[k]) for k in b.buf)


def test_vae_state_dict_keys(vae_ck):
    spec, bufs, _, _ = vae_spec(8, 4)
    assert set(vae_ck.sd) == set(spec) | set(bufs) | {k.replace("running_var", "num_batches_tracked") for k in bufs if k.endswith("var")}
    assert list(vae_ck.sd)[:len(spec)] == list(spec)
    assert all(int(v) == 3 and v.dtype == torch.int64 for k, v in vae_ck.sd.items() if k.endswith("num_batches_tracked"))


@pytest.mark.parametrize("cls,err", VAE_READERS)
def test_vae_checkpoint_loads_wrapped_and_bare(vae_ck, cls, err):
    for path in (vae_ck.best, vae_ck.final):
        eng = VaeStub(5)
        _loader(cls, eng).load(path)
        assert _same_vae(eng, vae_ck.src), path
        eng = VaeStub(6)
        AENC.load_model(eng, path)
        assert _same_vae(eng, vae_ck.src), path


@pytest.mark.parametrize("cls,err", VAE_READERS)
def test_vae_checkpoint_refusals(vae_ck, tmp_path, cls, err):
    eng = VaeStub(5)
    before = eng.P.data.clone()
    ld = _loader(cls, eng)
    p = str(tmp_path / "none.pth")
    with pytest.raises(err) as e:
        ld.load(p)
    assert _msg(e) == f"checkpoint {p} does not exist"
    with pytest.raises(Exception):
        ld.load(_text_file(tmp_path))
    for wrap in (True, False):
        sd = {k: v for k, v in vae_ck.sd.items() if k != "fc_mu.bias"}
        p = str(tmp_path / f"lacks{wrap}.pth")
        torch.save({"epoch": 1, "model_state": sd} if wrap else sd, p)
        with pytest.raises(err) as e:
            ld.load(p)
        assert _msg(e) == f"{p}: no 'fc_mu.bias': not a checkpoint of this VAE"
    sd = {k: v for k, v in vae_ck.sd.items() if k != "encoder.conv.1.running_mean"}
    p = str(tmp_path / "lacks_buffer.pth")
    torch.save(sd, p)
    with pytest.raises(err) as e:
        ld.load(p)
    assert _msg(e) == f"{p}: no 'encoder.conv.1.running_mean': not a checkpoint of this VAE"
    p = str(tmp_path / "shape.pth")
    torch.save(dict(vae_ck.sd, **{"fc_mu.bias": torch.zeros(3)}), p)
    with pytest.raises(err) as e:
        ld.load(p)
    assert _msg(e) == f"{p}: 'fc_mu.bias' has shape (3,), the config (MAX_NOTES 8, LATENT_DIM 4) implies (4,)"
    assert torch.equal(eng.P.data, before)          # a refused file leaves the engine as it was


def test_vae_editor_refuses_what_is_no_state_dict(tmp_path):
    p = str(tmp_path / "list.pth")
    torch.save([1, 2], p)
    with pytest.raises(AeEditError) as e:
        _loader(AED.LatentEditor, VaeStub()).load(p)
    assert _msg(e) == f"{p}: neither a train_ae checkpoint nor a state_dict"


# ---- classifier kind: the evaluators (strict) -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def ed_ck(tmp_path_factory):
    d = tmp_path_factory.mktemp("ed_ck")
    out = SimpleNamespace(dir=d)
    for sn in (False, True):
        src = EdStub(1, sn)
        sd = src.state_dict()
        tag = "sn" if sn else "plain"
        torch.save({"epoch": 1, "model": sd, "optimizer": {}, "cfg": dict(src.cfg)}, d / f"{tag}_best.pth")
        torch.save(sd, d / f"{tag}_bare.pth")
        setattr(out, tag, SimpleNamespace(src=src, sd=sd, best=str(d / f"{tag}_best.pth"), bare=str(d / f"{tag}_bare.pth")))
    return out


def _same_ed(a, b):
    return torch.equal(a.P.data[:a.P.n], b.P.data[:b.P.n]) and set(a.buf) == set(b.buf) and all(torch.equal(a.buf[k], b.buf[k]) for k in b.buf)


@pytest.mark.parametrize("sn", [False, True])
def test_ed_evaluator_loads_wrapped_and_bare(ed_ck, sn):
    c = ed_ck.sn if sn else ed_ck.plain
    assert ("classifier.net.0.weight_orig" in c.sd) == sn and ("classifier.net.0.weight" in c.sd) != sn
    for path in (c.best, c.bare):
        eng = EdStub(5, sn)
        ld = _loader(EDV.EdEvaluator, eng)
        ld.load(path)
        assert _same_ed(eng, c.src) and ld.acc_host is None, path


def test_ed_evaluator_refusals(ed_ck, tmp_path):
    eng = EdStub(5)
    ld = _loader(EDV.EdEvaluator, eng)
    p = str(tmp_path / "none.pth")
    with pytest.raises(EdEvaluateError) as e:
        ld.load(p)
    assert _msg(e) == f"checkpoint {p} does not exist"
    with pytest.raises(Exception):
        ld.load(_text_file(tmp_path))
    p = str(tmp_path / "list.pth")
    torch.save([1, 2], p)
    with pytest.raises(EdEvaluateError) as e:
        ld.load(p)
    assert _msg(e) == f"{p}: neither a train_ed checkpoint nor a state_dict"
    sd = ed_ck.plain.sd
    for wrap in (True, False):
        p = str(tmp_path / f"lacks{wrap}.pth")
        less = {k: v for k, v in sd.items() if k != "classifier.head.bias"}
        torch.save({"model": less} if wrap else less, p)
        with pytest.raises(EdEvaluateError) as e:
            ld.load(p)
        assert _msg(e) == (f"{p}: no 'classifier.head.bias': not a checkpoint of this classifier (input_mode notes, "
                           "use_spectral_norm False)")
    p = str(tmp_path / "lacks_buffer.pth")
    torch.save({k: v for k, v in sd.items() if k != "encoder.conv.0.net.1.running_var"}, p)
    with pytest.raises(EdEvaluateError) as e:
        ld.load(p)
    assert _msg(e).startswith(f"{p}: no 'encoder.conv.0.net.1.running_var': not a checkpoint of this classifier")
    p = str(tmp_path / "shape.pth")
    torch.save(dict(sd, **{"classifier.head.bias": torch.zeros(3)}), p)
    with pytest.raises(EdEvaluateError) as e:
        ld.load(p)
    assert _msg(e) == f"{p}: 'classifier.head.bias' has shape (3,), the config implies (4,)"
    less = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}       # not a key the check asks for
    ld.load_state(less)
    assert _same_ed(eng, ed_ck.plain.src)
    with pytest.raises(EdEvaluateError) as e:
        ld.load_state({})
    assert _msg(e).startswith("state_dict: no '")


@pytest.mark.parametrize("part", ["weight_orig", "weight_u", "weight_v"])
def test_ed_evaluator_refuses_a_broken_spectral_norm_triple(ed_ck, tmp_path, part):
    sd = ed_ck.sn.sd
    p = str(tmp_path / "triple.pth")
    torch.save({k: v for k, v in sd.items() if k != "classifier.net.0." + part}, p)
    with pytest.raises(EdEvaluateError) as e:
        _loader(EDV.EdEvaluator, EdStub(5, True)).load(p)
    assert _msg(e) == (f"{p}: no 'classifier.net.0.{part}': not a checkpoint of this classifier (input_mode notes, "
                       "use_spectral_norm True)")
    # a plain checkpoint into a spectral-norm classifier, and the other way round
    with pytest.raises(EdEvaluateError) as e:
        _loader(EDV.EdEvaluator, EdStub(5, True)).load(ed_ck.plain.bare)
    assert "weight_orig" in _msg(e)
    with pytest.raises(EdEvaluateError) as e:
        _loader(EDV.EdEvaluator, EdStub(5, False)).load(ed_ck.sn.bare)
    assert "no 'encoder.conv.0.net.0.weight'" in _msg(e)
    p = str(tmp_path / "triple_shape.pth")
    torch.save(dict(sd, **{"classifier.net.0.weight_v": torch.zeros(3)}), p)
    with pytest.raises(EdEvaluateError) as e:
        _loader(EDV.EdEvaluator, EdStub(5, True)).load(p)
    assert _msg(e) == f"{p}: 'classifier.net.0.weight_v' has shape (3,), the config implies (8,)"


# ---- classifier kind: the GAN trainer's frozen copy (strict=False) ---------------------------------------------------
def test_frozen_ed_loads_wrapped_bare_and_folded(ed_ck, capsys):
    src = ed_ck.plain.src
    for path in (ed_ck.plain.best, ed_ck.plain.bare):
        eng = GanStub(2)
        assert train_gan.load_ed_checkpoint(eng, path) is True
        assert torch.equal(eng.ED.data[:eng.ED.n], src.P.data[:src.P.n]) and all(torch.equal(eng.EDbuf[k], src.buf[k]) for k in eng.EDbuf)
        assert eng.calls == ["fold_ed"]
        assert capsys.readouterr().out == f"[INFO] Loading pre-trained Emotion Discriminator from {path}\n"
    # spectral-norm keys: the eval-mode weight w_orig / (u^T W v), folded at load time
    eng = GanStub(2)
    assert train_gan.load_ed_checkpoint(eng, ed_ck.sn.best) is True
    sd = ed_ck.sn.sd
    for nm in ("encoder.conv.0.net.0", "classifier.net.0"):
        w = sd[nm + ".weight_orig"].double()
        sigma = torch.dot(sd[nm + ".weight_u"].double(), w.flatten(1).mv(sd[nm + ".weight_v"].double()))
        assert torch.equal(eng.ED.p[nm + ".weight"], (w / sigma).float())
    assert torch.equal(eng.ED.p["classifier.head.weight"], sd["classifier.head.weight"])
    assert "lacks" not in capsys.readouterr().out


def test_frozen_ed_missing_file_key_and_shape(ed_ck, tmp_path, capsys):
    eng = GanStub(2)
    p = str(tmp_path / "none.pth")
    assert train_gan.load_ed_checkpoint(eng, p) is False and eng.calls == []
    assert capsys.readouterr().out == f"[WARN] ED checkpoint not found at {p}. ED will be random!\n"
    with pytest.raises(Exception):
        train_gan.load_ed_checkpoint(eng, _text_file(tmp_path))
    capsys.readouterr()
    sd = ed_ck.plain.sd
    p = str(tmp_path / "lacks.pth")
    torch.save({"model": {k: v for k, v in sd.items() if k not in ("classifier.head.bias", "encoder.conv.0.net.1.running_mean")}}, p)
    eng.ED.p["classifier.head.bias"].fill_(9.0)
    assert train_gan.load_ed_checkpoint(eng, p) is True and eng.calls == ["fold_ed"]
    assert capsys.readouterr().out.splitlines()[1] == (f"[WARN] ED checkpoint {p} lacks 2 key(s), left at their initial values: "
                                                        "classifier.head.bias, encoder.conv.0.net.1.running_mean")
    assert (eng.ED.p["classifier.head.bias"] == 9.0).all()
    assert torch.equal(eng.ED.p["classifier.head.weight"], sd["classifier.head.weight"])
    p = str(tmp_path / "shape.pth")
    torch.save(dict(sd, **{"classifier.head.bias": torch.zeros(3), "encoder.conv.0.net.1.running_var": torch.zeros(5)}), p)
    with pytest.raises(RuntimeError) as e:
        train_gan.load_ed_checkpoint(GanStub(2), p)
    assert _msg(e) == ("Error(s) in loading state_dict for EmotionDiscriminator: size mismatch for classifier.head.bias: "
                       "checkpoint (3,) vs model (4,); encoder.conv.0.net.1.running_var: checkpoint (5,) vs model (64,)")


@pytest.mark.parametrize("part", ["weight_orig", "weight_u", "weight_v"])
def test_frozen_ed_counts_a_broken_triple_as_missing(ed_ck, tmp_path, capsys, part):
    p = str(tmp_path / "triple.pth")
    torch.save({k: v for k, v in ed_ck.sn.sd.items() if k != "classifier.net.0." + part}, p)
    eng = GanStub(2)
    eng.ED.p["classifier.net.0.weight"].fill_(9.0)
    assert train_gan.load_ed_checkpoint(eng, p) is True
    assert capsys.readouterr().out.splitlines()[1] == (f"[WARN] ED checkpoint {p} lacks 1 key(s), left at their initial values: "
                                                        "classifier.net.0.weight")
    assert (eng.ED.p["classifier.net.0.weight"] == 9.0).all()


# ---- label files ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("err", [AeEvaluateError, AeEditError])
def test_label_file_checks(tmp_path, err):
    load = LOAD_LABELS[err]
    p = str(tmp_path / "emotion.npy")
    np.save(p, np.array(["happy", "SAD", "angry", "calm"], dtype=object), allow_pickle=True)
    idx = load(p, 4, 4)
    assert idx.dtype == np.int64 and idx.tolist() == [0, 1, 2, 3]
    with pytest.raises(err) as e:
        load(p, 3, 4)
    assert _msg(e) == f"{p} holds 4 entries, the split 3 rows"
    with pytest.raises(err) as e:
        load(p, 4, 3)
    assert _msg(e) == f"{p}: labels outside [0, 3) (unknown emotion names map to -1)"
    np.save(p, np.array(["happy", "bored"], dtype=object), allow_pickle=True)
    with pytest.raises(err) as e:
        load(p, 2, 4)
    assert _msg(e) == f"{p}: labels outside [0, 4) (unknown emotion names map to -1)"
    t = _text_file(tmp_path, "emotion.txt")
    with pytest.raises(err) as e:
        load(t, 2, 4)
    assert _msg(e).startswith(f"cannot read labels {t}: ")


def test_trainer_validation_labels_keep_their_own_rules(tmp_path):
    cfg = {"SPLITS_DIR": str(tmp_path)}
    assert train_ae._val_labels(cfg, 4, "cpu") is None                  # no file: no labels
    os.makedirs(tmp_path / "val")
    p = os.path.join(str(tmp_path), "val", "emotion.npy")
    np.save(p, np.array(["calm", "bored", None, "happy"], dtype=object), allow_pickle=True)
    y = train_ae._val_labels(cfg, 4, "cpu")
    assert y.dtype == torch.int64 and y.tolist() == [3, -1, -1, 0]      # no range check here: the evaluator's own refuses them
    with pytest.raises(ValueError) as e:
        train_ae._val_labels(cfg, 3, "cpu")
    assert _msg(e) == f"{p} holds 4 entries, the validation split 3 rows"


# ---- the VAE's split arrays -----------------------------------------------------------------------------------------
def test_vae_split_array_checks(tmp_path):
    load = LOAD_NOTES[AeEditError]
    p = str(tmp_path / "notes.npy")
    with pytest.raises(AeEditError) as e:
        load(p, 8)
    assert _msg(e) == f"split array {p} does not exist"
    np.save(p, np.zeros((2, 8, 4), np.float64))
    got = load(p, 8)
    assert got.dtype == np.float32 and got.shape == (2, 8, 4) and got.flags["C_CONTIGUOUS"]
    for shape in ((2, 8, 3), (0, 8, 4), (8, 4)):
        np.save(p, np.zeros(shape, np.float32))
        with pytest.raises(AeEditError) as e:
            load(p, 8)
        assert _msg(e) == f"{p}: an (n, 8, 4) array with n >= 1 expected, got {shape}"
    t = _text_file(tmp_path, "notes.txt")
    with pytest.raises(AeEditError) as e:
        load(t, 8)
    assert _msg(e).startswith(f"cannot read {t}: ")
    assert AEV._split_path({"SPLITS_DIR": "s"}, "val") == os.path.join("s", "val", "notes.npy")
    assert AEV._split_path({}, "test") == os.path.join("data/splits", "test", "notes.npy") and AEV._split_path({}, "x/notes.npy") == "x/notes.npy"


# ---- configs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("err", GAN_ERRORS)
def test_read_config(tmp_path, err):
    p = str(tmp_path / "none.yaml")
    with pytest.raises(err) as e:
        read_config(p, "config", err)
    assert _msg(e) == f"config {p} does not exist"
    with pytest.raises(err) as e:
        read_config(p, "ED config", err)
    assert _msg(e) == f"ED config {p} does not exist"
    (tmp_path / "list.yaml").write_text("- 1\n- 2\n")
    p = str(tmp_path / "list.yaml")
    with pytest.raises(err) as e:
        read_config(p, "config", err)
    assert _msg(e) == f"config {p} is not a YAML mapping"
    (tmp_path / "ok.yaml").write_text("A: 1\n")
    assert read_config(str(tmp_path / "ok.yaml"), "config", err) == {"A": 1}


def test_predict_inputs_config_and_model_checks(tmp_path):
    (tmp_path / "ok.yaml").write_text("input_mode: notes\n")
    model = tmp_path / "m.pth"
    model.write_text("x")
    args = SimpleNamespace(config=str(tmp_path / "none.yaml"), model=str(model), batch=4)
    with pytest.raises(PRED.PredictError) as e:
        PRED.load_tool_inputs(args, PRED.PredictError, lambda cfg: None)
    assert _msg(e) == f"config {args.config} does not exist"
    args.config = str(tmp_path / "ok.yaml")
    assert PRED.load_tool_inputs(args, PRED.PredictError, lambda cfg: None) == {"input_mode": "notes"}
    args.model = str(tmp_path / "none.pth")
    with pytest.raises(PRED.PredictError) as e:
        PRED.load_tool_inputs(args, PRED.PredictError, lambda cfg: None)
    assert _msg(e) == f"checkpoint {args.model} does not exist"


# ---- what one shared reader adds --------------------------------------------------------------------------------------
def test_vae_checkpoint_is_opened_once(vae_ck, monkeypatch):
    calls, real = [], torch.load
    monkeypatch.setattr(torch, "load", lambda f, *a, **k: calls.append(str(f)) or real(f, *a, **k))
    eng = VaeStub(5)
    CK.load_vae_checkpoint(eng, vae_ck.best, AeEvaluateError)
    assert calls == [vae_ck.best] and _same_vae(eng, vae_ck.src)
    for load in (_loader(AEV.VaeEvaluator, VaeStub(6)).load, _loader(AED.LatentEditor, VaeStub(7)).load,
                 functools.partial(AENC.load_model, VaeStub(8))):
        del calls[:]
        load(vae_ck.final)
        assert calls == [vae_ck.final]


def test_an_unreadable_checkpoint_is_a_tool_error_everywhere(tmp_path):
    t = _text_file(tmp_path)
    for load, err in ((_loader(AEV.VaeEvaluator, VaeStub()).load, AeEvaluateError), (_loader(AED.LatentEditor, VaeStub()).load, AeEditError),
                      (_loader(EDV.EdEvaluator, EdStub()).load, EdEvaluateError)):
        with pytest.raises(err) as e:
            load(t)
        assert _msg(e).startswith(f"cannot read checkpoint {t}: ")
    p = str(tmp_path / "list.pth")
    torch.save([1, 2], p)
    with pytest.raises(AeEvaluateError) as e:
        _loader(AEV.VaeEvaluator, VaeStub()).load(p)
    assert _msg(e) == f"{p}: neither a train_ae checkpoint nor a state_dict"


def test_predict_refuses_a_config_that_is_no_mapping(tmp_path):
    (tmp_path / "list.yaml").write_text("- 1\n- 2\n")
    args = SimpleNamespace(config=str(tmp_path / "list.yaml"), model=None, batch=4)
    with pytest.raises(PRED.PredictError) as e:
        PRED.load_tool_inputs(args, PRED.PredictError, lambda cfg: cfg.get("input_mode"))
    assert _msg(e) == f"config {args.config} is not a YAML mapping"
