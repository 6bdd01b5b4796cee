"""GPU: the generator's exponential moving average (EMA_DECAY) -- mg_ema_flat against its numpy restatement bit for bit, the
rider behind the generator's update under graph replay and its read-only-ness, the BatchNorm recalibration of the averaged
weights against the oracle, and the trainer, sampler and evaluator end to end on synthetic data."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import ops  # noqa: E402
from melo_gan_amd.gan import ema as E  # noqa: E402
from melo_gan_amd.gan.dataset import GANDataset  # noqa: E402
from oracle import melo_oracle as O  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
B, T, C = 8, 16, 4


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel against ema_ref, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
STEPS = [(1, 2, 9), (9, 10, 5000), (2, 10, 5000)]          # adam_state[0] of the three successive calls: both arms of the min


def run_kernel(p_list, shadow0, decay, ramp, offset, steps):
    state = torch.zeros(4, dtype=torch.float64, device="cuda")
    shadow = torch.from_numpy(shadow0).cuda()
    for p, step in zip(p_list, steps):
        state[0] = float(step)
        ops.ema_flat(torch.from_numpy(p).cuda(), shadow, len(shadow0), decay, ramp, state, offset)
    torch.cuda.synchronize()
    return shadow.cpu().numpy()


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, 2 ** 20 + 3])
def test_kernel_matches_ema_ref_bit_for_bit(n):
    """decay 0: s + 1.0 * (p - s) is p exactly wherever p - s is exact -- a shadow whose values are fp32 numbers within 2^29 of
    the parameters' magnitude, as the engine's is from ema_reset on -- so that case also starts from such a shadow and, where no
    update has a negative t (which the ramp turns into a negative decay), must end at the last parameters exactly."""
    rng = np.random.default_rng(n)
    p_list = [rng.standard_normal(n).astype(np.float32) for _ in range(3)]
    shadows = {"fp64": rng.standard_normal(n), "fp32": rng.standard_normal(n).astype(np.float32).astype(np.float64)}
    for decay in (0.0, 0.999):
        for ramp in (True, False):
            for offset in (0, 7):
                for steps in STEPS[:2] if n > 5 else STEPS:
                    for kind, shadow0 in shadows.items():
                        got = run_kernel(p_list, shadow0, decay, ramp, float(offset), steps)
                        ref = E.ema_ref(p_list, decay, ramp, offset, list(steps), shadow0=shadow0)
                        assert np.array_equal(bits(got), bits(ref)), (n, decay, ramp, offset, steps, kind)
                        if decay == 0.0 and kind == "fp32" and (not ramp or min(steps) > offset):
                            assert np.array_equal(got, p_list[-1].astype(np.float64)), (n, ramp, offset, steps)


def test_kernel_special_values_and_unaligned_views():
    special = np.array([1e-45, -1e-40, 0.0, -0.0, 1e30, -1e30, 1.0, 3.4e38, 2.5, -7.0, 0.1], np.float32)      # denormals, +-0, huge
    rng = np.random.default_rng(5)
    p_list = [special, rng.permutation(special), special[::-1].copy()]
    shadow0 = rng.standard_normal(special.size)
    shadow0[2], shadow0[3] = -0.0, 0.0
    for decay, ramp in ((0.999, True), (0.999, False), (0.0, True)):
        got = run_kernel(p_list, shadow0, decay, ramp, 0.0, (1, 10, 5000))
        ref = E.ema_ref(p_list, decay, ramp, 0, [1, 10, 5000], shadow0=shadow0)
        assert np.array_equal(bits(got), bits(ref)), (decay, ramp)
    # non-finite parameters propagate; nothing guards them
    bad = np.array([np.inf, np.nan, 1.0, -np.inf, 2.0], np.float32)
    got = run_kernel([bad], np.ones(5), 0.5, False, 0.0, (1,))
    assert np.isposinf(got[0]) and np.isnan(got[1]) and got[2] == 1.0 and np.isneginf(got[3]) and got[4] == 1.5
    # views that are not 16-byte aligned take the element path: the same bits, and nothing outside [0, n) is written
    n = 1027
    p = rng.standard_normal(n + 8).astype(np.float32)
    s0 = rng.standard_normal(n + 8)
    state = torch.tensor([3.0, 0, 0, 0], dtype=torch.float64, device="cuda")
    for po, so in ((1, 0), (0, 1), (1, 1), (0, 0)):
        pd, sd = torch.from_numpy(p).cuda(), torch.from_numpy(s0).cuda()
        ops.ema_flat(pd[po:po + n], sd[so:so + n], n, 0.999, True, state, 0.0)
        got = sd.cpu().numpy()
        ref = E.ema_ref([p[po:po + n]], 0.999, True, 0, 3, shadow0=s0[so:so + n])
        assert np.array_equal(bits(got[so:so + n]), bits(ref)), (po, so)
        assert np.array_equal(bits(got[:so]), bits(s0[:so])) and np.array_equal(bits(got[so + n:]), bits(s0[so + n:])), (po, so)


def test_kernel_replays_from_a_graph_with_the_step_read_on_the_device():
    n = 1027
    rng = np.random.default_rng(11)
    p = rng.standard_normal(n).astype(np.float32)
    shadow0 = rng.standard_normal(n)
    steps = (1, 10, 5000)
    eager = run_kernel([p, p, p], shadow0, 0.999, True, 0.0, steps)
    pd, shadow = torch.from_numpy(p).cuda(), torch.from_numpy(shadow0).cuda()
    state = torch.zeros(4, dtype=torch.float64, device="cuda")
    with torch.cuda.stream(torch.cuda.Stream()):
        g = ops.Graph.capture(lambda: ops.ema_flat(pd, shadow, n, 0.999, True, state, 0.0))      # nothing runs during capture
        for step in steps:
            state[0] = float(step)          # a host write between replays; the launch's arguments are constant
            g.launch()
        torch.cuda.synchronize()
    assert np.array_equal(bits(shadow), bits(eager))
    assert np.array_equal(bits(eager), bits(E.ema_ref([p, p, p], 0.999, True, 0, list(steps), shadow0=shadow0)))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the engine's rider
# ---------------------------------------------------------------------------------------------------------------------
def make_engine(decay):
    from melo_gan_amd.gan.engine import GanEngine
    cfg, ed_cfg = O.default_gan_cfg(B, T, C), O.default_ed_cfg(C)
    if decay is not None:
        cfg["EMA_DECAY"] = decay
    eng = GanEngine(cfg, ed_cfg, "cuda", B)
    eng.init_weights(42)
    real, numeric, latent, emot = O.synthetic_batch(B, T, C, cfg["LATENT_DIM"], 6, 7)
    eng.set_batch(real.cuda(), numeric.cuda(), latent.cuda(), emot.cuda())
    eng.seed(42)
    return eng


def run_rounds(eng, use_graph, rounds=4):
    """rounds x (5 critic + 1 generator updates), as the trainer issues them at CRITIC_ITERS 5; returns GE.data after every
    generator update and the losses of every round."""
    stash, losses = [], []
    with torch.cuda.stream(eng.stream):
        for _ in range(rounds):
            for _ in range(4):
                eng.run("d_step_rng", use_graph)
            eng.run("dg_step_rng", use_graph)
            stash.append(eng.GE.data[:eng.GE.n].cpu().numpy().copy())
            losses.append(torch.cat([eng.loss_d_out, eng.gp, eng.adv, eng.emo]).cpu())
    torch.cuda.synchronize()
    return stash, torch.stack(losses)


@pytest.fixture(scope="module")
def rider_runs():
    runs = {}
    for name, decay, graph in (("graph", 0.99, True), ("eager", 0.99, False), ("off", 0.0, True)):
        eng = make_engine(decay)
        init = eng.GE.data[:eng.GE.n].cpu().numpy().copy()
        stash, losses = run_rounds(eng, graph)
        runs[name] = (eng, init, stash, losses)
    return runs


def test_rider_under_graph_replay_equals_ema_ref_over_the_stashed_weights(rider_runs):
    eng, init, _, _ = rider_runs["graph"]
    eager, init_e, stash, _ = rider_runs["eager"]
    assert eng.ema is not None and eng.ema.dtype == torch.float64 and eng.ema.numel() == eng.GE.n and eng.ema_offset == 0.0
    assert float(eng.GE.state[0]) == 4.0 and np.array_equal(init, init_e)
    assert any(isinstance(v, tuple) for v in eng._graphs.values())          # the steps were replayed, not run eagerly
    ref = E.ema_ref(stash, 0.99, True, 0, 1, shadow0=init.astype(np.float64))      # ema_reset: the shadow starts at the weights
    assert np.array_equal(bits(eager.ema), bits(ref))
    assert np.array_equal(bits(eng.ema), bits(eager.ema))
    assert not np.array_equal(ref, stash[-1].astype(np.float64))              # an average, not a copy
    sd = eng.ema_state_dicts()
    raw = eng.state_dicts()
    assert [k for k in raw["G"] if "running_" not in k and "num_batches" not in k] == list(sd["G"]) and list(sd["E_num"]) == list(raw["E_num"])
    o, n = eng.GE.offsets["E.net.7.weight"]
    assert sd["E_num"]["net.7.weight"].dtype == torch.float64 and np.array_equal(bits(sd["E_num"]["net.7.weight"].flatten()), bits(ref[o:o + n]))


def test_rider_is_read_only(rider_runs):
    on, _, _, loss_on = rider_runs["graph"]
    off, _, _, loss_off = rider_runs["off"]
    assert off.ema is None
    for name in ("data", "m", "v", "state"):
        assert torch.equal(getattr(on.GE, name), getattr(off.GE, name)), name
    assert torch.equal(on.D.data, off.D.data)
    for k in on.Gbuf:
        assert torch.equal(on.Gbuf[k], off.Gbuf[k]), k
    assert torch.equal(loss_on, loss_off) and torch.isfinite(loss_on).all()
    # off: the graphs hold the parent's launches -- one kernel node fewer than with the rider
    gon, goff = on._graphs["dg_step_rng"][0], off._graphs["dg_step_rng"][0]
    assert gon.kernel_nodes == goff.kernel_nodes + 1


def test_ema_reset_restarts_the_ramp_at_the_current_step(rider_runs):
    eng = make_engine(0.99)
    run_rounds(eng, True, rounds=2)
    eng.ema_reset()
    assert eng.ema_offset == 2.0 and not eng._graphs          # the captured update held the old offset
    assert np.array_equal(bits(eng.ema), bits(eng.GE.data[:eng.GE.n].double()))
    init = eng.GE.data[:eng.GE.n].cpu().numpy().copy()
    stash, _ = run_rounds(eng, True, rounds=3)
    assert np.array_equal(bits(eng.ema), bits(E.ema_ref(stash, 0.99, True, 2, 3, shadow0=init.astype(np.float64))))


# ---------------------------------------------------------------------------------------------------------------------
# 3. BatchNorm statistics of the averaged weights
# ---------------------------------------------------------------------------------------------------------------------
def rel_err(a, b):
    a, b = a.detach().cpu().double().flatten(), b.detach().cpu().double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def test_recalibrate_bn_matches_the_oracle(monkeypatch, capsys):
    from melo_gan_amd.gan.eval_engine import recalibrate_bn
    from melo_gan_amd.gan.evaluate import Evaluator
    cfg, ed_cfg = O.default_gan_cfg(B, T, C), O.default_ed_cfg(C)
    n, seed = 20, 5
    ds = GANDataset.synthetic(n, T, C, cfg["LATENT_DIM"], 3, "cuda")
    train_eng = make_engine(None)
    S = O.build_gan_state(cfg, ed_cfg, "weights_init", seed=9)
    ev = Evaluator(cfg, ed_cfg, "cuda", B)
    ev.eng.load_state(S.PE, S.PG, S.BG, S.PD, S.PED, S.BED)
    before = {k: v.clone() for k, v in train_eng.Gbuf.items()}
    assert recalibrate_bn(ev, ds, seed) is True
    torch.cuda.synchronize()
    # the oracle over the same weights, numeric rows and noise (read back from the device: the (seed, row) key is all it has):
    # per batch the mean and the unbiased variance (momentum 1 leaves exactly them in fresh buffers), then their plain mean
    k = n // B
    noise = torch.zeros(k * B, cfg["NOISE_DIM"], device="cuda")
    zero = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.eval_noise(noise, zero, zero, n, seed)
    noise, numeric = noise.cpu().double(), ds.numeric.cpu().double()
    dbl = lambda P: type(P)((kk, v.double().clone()) for kk, v in P.items())  # noqa: E731
    PE, PG = dbl(S.PE), dbl(S.PG)
    monkeypatch.setattr(O, "BN_MOMENTUM", 1.0)
    acc = {kk: torch.zeros_like(v, dtype=torch.float64) for kk, v in S.BG.items()}
    for j in range(k):
        rows = slice(j * B, (j + 1) * B)
        Bf = dbl(S.BG)
        with torch.no_grad():
            emb = O.feature_encoder_fwd(PE, numeric[rows], None)
            O.generator_fwd(PG, Bf, noise[rows], None, emb, cfg["INTEGRATION_MODE"], T, train=True)
        for kk in acc:
            acc[kk] += Bf[kk] / k
    for kk, want in acc.items():
        tol = 1e-5 if kk.endswith("running_var") else 1e-3
        err = rel_err(ev.eng.Gbuf[kk], want)
        print(f"recalibrate_bn {kk}: rel err {err:.3g} (bound {tol})")
        assert err < tol, (kk, err)
        assert rel_err(S.BG[kk], want) > 0.05, kk          # the statistics did move away from the loaded ones
    assert ev.eng.num_batches_tracked == k and ev.eng.bn_mom == 0.1
    # a second call gives identical bits; the training engine was never touched
    first = {kk: v.clone() for kk, v in ev.eng.Gbuf.items()}
    assert recalibrate_bn(ev, ds, seed) is True
    for kk in first:
        assert torch.equal(first[kk], ev.eng.Gbuf[kk]), kk
        assert torch.equal(before[kk], train_eng.Gbuf[kk]), kk
    # fewer rows than one batch: the buffers stay, with a warning
    capsys.readouterr()
    small = GANDataset.synthetic(5, T, C, cfg["LATENT_DIM"], 4, "cuda")
    assert recalibrate_bn(ev, small, seed) is False
    assert "[WARN]" in capsys.readouterr().out
    for kk in first:
        assert torch.equal(first[kk], ev.eng.Gbuf[kk]), kk


# ---------------------------------------------------------------------------------------------------------------------
# 4. trainer, sampler, evaluator end to end
# ---------------------------------------------------------------------------------------------------------------------
class _Scalars:
    def __init__(self, log_dir):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, int(step), float(value)))

    def close(self):
        pass


def same(a, b, path):
    assert type(a) is type(b), path
    if isinstance(a, dict):
        assert list(a) == list(b), path
        for k in a:
            same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{path}[{i}]")
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and a.contiguous().numpy().tobytes() == b.contiguous().numpy().tobytes(), path
    else:
        assert a == b, path


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """Four short runs at the small shape (synthetic 64 rows, 2 epochs, a checkpoint per epoch): without the keys, with
    EMA_DECAY 0, with 0.99, and 0.99 resumed from the uninterrupted run's first epoch."""
    from melo_gan_amd.gan import train_gan
    tmp = tmp_path_factory.mktemp("ema")
    base = yaml.safe_load(open(os.path.join(ROOT, "config", "gan_config.yaml")))
    ed = O.default_ed_cfg(C)
    for k in ("EMA_DECAY", "EMA_RAMP"):
        base.pop(k, None)
    mp = pytest.MonkeyPatch()
    writers = []
    mp.setattr(train_gan, "_scalar_writer", lambda d: writers.append(_Scalars(d)) or writers[-1])
    out = {"tmp": tmp, "ed": ed}
    try:
        for name, extra, resume in (("nokeys", {}, None), ("zero", {"EMA_DECAY": 0.0, "EMA_RAMP": True}, None),
                                    ("ema", {"EMA_DECAY": 0.99}, None), ("resumed", {"EMA_DECAY": 0.99}, "ema")):
            d = tmp / name
            cfg = dict(base, EPOCHS=2, BATCH_SIZE=B, MAX_NOTES=T, NOTE_DIM=C, SAVE_FREQ=1, CRITIC_ITERS=2, CHECKPOINT_DIR=str(d / "ck"),
                       LOG_DIR=str(d / "log"), SAMPLE_DIR=str(d / "s"), **extra)
            eng = train_gan.train(dict(cfg), dict(ed), str(tmp / "none.pth"), synthetic=64, eval_every=1,
                                  resume=str(tmp / resume / "ck" / "gan_epoch0001.pth") if resume else None)
            out[name] = {"dir": d / "ck", "cfg": cfg, "eng": eng, "scalars": writers[-1].rows}
    finally:
        mp.undo()
    return out


def test_trainer_with_decay_zero_is_byte_identical_to_a_config_without_the_keys(trained):
    """The guard: passes before the feature too."""
    a, b = trained["nokeys"]["dir"], trained["zero"]["dir"]
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == ["gan_epoch0001.pth", "gan_epoch0002.pth", "gan_final.pth"]
    for name in ("gan_epoch0001.pth", "gan_epoch0002.pth", "gan_final.pth"):
        same(torch.load(a / name, map_location="cpu"), torch.load(b / name, map_location="cpu"), name)
        assert open(a / name, "rb").read() == open(b / name, "rb").read(), name
    assert list(torch.load(a / "gan_epoch0002.pth", map_location="cpu")) == ["epoch", "G", "D", "E_num", "opt_G", "opt_D"]
    assert trained["nokeys"]["scalars"] == trained["zero"]["scalars"]
    assert trained["zero"]["eng"].ema is None


def test_trainer_writes_the_ema_block_and_the_final_ema_file(trained):
    run = trained["ema"]
    eng, d = run["eng"], run["dir"]
    assert sorted(os.listdir(d)) == ["gan_epoch0001.pth", "gan_epoch0002.pth", "gan_final.pth", "gan_final_ema.pth"]
    full = torch.load(d / "gan_epoch0002.pth", map_location="cpu")
    assert list(full) == ["epoch", "G", "D", "E_num", "opt_G", "opt_D", "ema"]
    blk, sd = full["ema"], eng.ema_state_dicts()
    assert (blk["decay"], blk["ramp"], blk["offset"]) == (0.99, True, 0.0)
    assert float(eng.GE.state[0]) == 8.0          # 64 rows / 8 = 8 batches an epoch, a generator update every second one
    assert list(blk["G"]) == list(full["G"]) and list(blk["E_num"]) == list(full["E_num"])
    for part in ("G", "E_num"):
        for k, v in sd[part].items():
            assert blk[part][k].dtype == torch.float64 and np.array_equal(bits(blk[part][k]), bits(v)), (part, k)
    for k, v in blk["G"].items():
        if "running_" in k:          # recalibrated on the training split: not the raw weights' running statistics
            assert v.dtype == torch.float32 and torch.isfinite(v).all() and not torch.equal(v, full["G"][k]), k
        if k.endswith("num_batches_tracked"):
            assert v.dtype == torch.int64 and int(v) == 64 // B
    # every other key is what the run without averaging wrote: the rider and the recalibration touch nothing of the training
    plain = torch.load(trained["nokeys"]["dir"] / "gan_epoch0002.pth", map_location="cpu")
    same({k: v for k, v in full.items() if k != "ema"}, plain, "gan_epoch0002.pth")
    assert open(d / "gan_final.pth", "rb").read() == open(trained["nokeys"]["dir"] / "gan_final.pth", "rb").read()
    # gan_final_ema.pth: gan_final.pth's keys, the shadow rounded to float32, the recalibrated buffers
    fin, fe = torch.load(d / "gan_final.pth", map_location="cpu"), torch.load(d / "gan_final_ema.pth", map_location="cpu")
    assert list(fe) == list(fin) and list(fe["G"]) == list(fin["G"]) and list(fe["E_num"]) == list(fin["E_num"])
    for part in ("G", "E_num"):
        for k, v in fe[part].items():
            assert v.dtype == fin[part][k].dtype, (part, k)
            want = sd[part][k].float() if k in sd[part] else blk["G"][k]
            assert np.array_equal(bits(v) if v.dtype == torch.float32 else v.numpy(), bits(want) if want.dtype == torch.float32 else want.numpy()), (part, k)
    # the reference-shaped modules load it strictly, as they load gan_final.pth
    from melo_gan_amd.gan.models import Generator
    from melo_gan_amd.gan.feature_encoder import FeatureEncoder
    cfg = run["cfg"]
    Generator(cfg["NOISE_DIM"], cfg["LATENT_DIM"], cfg.get("INTEGRATION_MODE", "conditioning"), max_notes=T, note_dim=C,
              numeric_embed_dim=128).load_state_dict(fe["G"], strict=True)
    FeatureEncoder(6, [256, 128], 128).load_state_dict(fe["E_num"], strict=True)


def test_resume_continues_the_average_as_the_uninterrupted_run(trained):
    a = torch.load(trained["ema"]["dir"] / "gan_epoch0002.pth", map_location="cpu")
    b = torch.load(trained["resumed"]["dir"] / "gan_epoch0002.pth", map_location="cpu")
    same(a, b, "gan_epoch0002.pth")
    same(torch.load(trained["ema"]["dir"] / "gan_final_ema.pth", map_location="cpu"),
         torch.load(trained["resumed"]["dir"] / "gan_final_ema.pth", map_location="cpu"), "gan_final_ema.pth")
    assert np.array_equal(bits(trained["ema"]["eng"].ema), bits(trained["resumed"]["eng"].ema))


def test_resume_without_a_block_starts_averaging_there_and_a_block_without_decay_is_ignored(trained, capsys):
    from melo_gan_amd.gan import train_gan
    from melo_gan_amd.gan.engine import GanEngine
    from melo_gan_amd.gan import config as Cfg
    cfg = Cfg.with_gan_defaults(dict(trained["ema"]["cfg"]), require=False)
    eng = GanEngine(cfg, dict(trained["ed"]), "cuda", B)
    eng.init_weights(1)
    assert train_gan.resume_checkpoint(eng, str(trained["nokeys"]["dir"] / "gan_epoch0001.pth")) == 1
    assert eng.ema_offset == 4.0 == float(eng.GE.state[0])
    assert np.array_equal(bits(eng.ema), bits(eng.GE.data[:eng.GE.n].double()))
    blk = torch.load(trained["ema"]["dir"] / "gan_epoch0001.pth", map_location="cpu")["ema"]
    assert train_gan.resume_checkpoint(eng, str(trained["ema"]["dir"] / "gan_epoch0001.pth")) == 1
    assert eng.ema_offset == 0.0
    o, n = eng.GE.offsets["G.decoder.pre.2.weight"]
    assert np.array_equal(bits(eng.ema[o:o + n]), bits(blk["G"]["decoder.pre.2.weight"].flatten()))
    off = GanEngine(dict(cfg, EMA_DECAY=0.0), dict(trained["ed"]), "cuda", B)
    off.init_weights(1)
    capsys.readouterr()
    train_gan.resume_checkpoint(off, str(trained["ema"]["dir"] / "gan_epoch0001.pth"))
    assert "[WARN]" in capsys.readouterr().out and off.ema is None


def test_eval_every_logs_the_averaged_weights_next_to_the_raw_ones(trained):
    tags = ("W_dist", "ED_Acc_Fake", "ED_CE_Fake", "ED_Acc_Real")
    ema, plain = trained["ema"]["scalars"], trained["nokeys"]["scalars"]
    for t in tags:
        raw = [(s, v) for tag, s, v in ema if tag == "Val/" + t]
        assert [s for s, _ in raw] == [1, 2] and raw == [(s, v) for tag, s, v in plain if tag == "Val/" + t], t
        avg = [(s, v) for tag, s, v in ema if tag == "ValEMA/" + t]
        assert [s for s, _ in avg] == [1, 2] and all(np.isfinite(v) for _, v in avg), t
    assert not any(tag.startswith("ValEMA/") for tag, _, _ in plain)
    assert [r for r in ema if not r[0].startswith("ValEMA/")] == plain
    assert [v for tag, _, v in ema if tag == "ValEMA/W_dist"] != [v for tag, _, v in ema if tag == "Val/W_dist"]


def test_sampler_and_evaluator_read_the_block_as_they_read_the_final_ema_file(trained, tmp_path):
    from melo_gan_amd.gan import evaluate as EV
    from melo_gan_amd.gan import generate as GN
    run = trained["ema"]
    cfg, ed, d = run["cfg"], trained["ed"], run["dir"]
    full, final, final_ema = str(d / "gan_epoch0002.pth"), str(d / "gan_final.pth"), str(d / "gan_final_ema.pth")
    # sampler: the rolls bit for bit
    rolls = {}
    for name, ck, flag in (("block", full, True), ("file", final_ema, False), ("raw", full, False)):
        s = GN.Sampler(cfg, None, "cuda", B)
        assert s.load_generator(ck, ema=flag) == ("ema" if flag else "raw")
        rolls[name] = s.sample(["all"], 3, 11).notes
    assert np.array_equal(bits(rolls["block"]), bits(rolls["file"])) and not np.array_equal(rolls["block"], rolls["raw"])
    with pytest.raises(GN.GenerateError, match="gan_final.pth"):
        GN.Sampler(cfg, None, "cuda", B).load_generator(final, ema=True)
    # evaluator: the critic of the full checkpoint under both; the reports are equal
    val = GANDataset.synthetic(20, T, C, cfg["LATENT_DIM"], 8, "cuda")
    reps = {}
    for name, ck, flag in (("block", full, True), ("file", final_ema, False), ("raw", full, False)):
        ev = EV.Evaluator(cfg, None, "cuda", B)
        ev.load_generator(ck, ema=flag)
        assert ev.load_critic(full)
        reps[name] = ev.evaluate(val, 11)
    assert reps["block"] == reps["file"] and reps["block"]["critic"] is not None
    assert reps["block"]["critic"]["mean_fake"] != reps["raw"]["critic"]["mean_fake"]
    with pytest.raises(EV.EvaluateError, match="gan_final.pth"):
        EV.Evaluator(cfg, None, "cuda", B).load_generator(final, ema=True)
    # the command lines: "weights" is the only new key of the outputs; --ema on a file without the block is refused by name
    cp = tmp_path / "gan.yaml"
    cp.write_text(yaml.safe_dump(dict(cfg, LOG_DIR=str(tmp_path / "log"), SAMPLE_DIR=str(tmp_path / "s"))))
    common = ["--config", str(cp), "--ckpt", full, "--synthetic", "20", "--batch", str(B), "--seed", "11"]
    out = {}
    for flag in ((), ("--ema",)):
        assert EV.main(common + ["--out", str(tmp_path / "eval.json"), *flag]) == 0
        out[flag] = json.load(open(tmp_path / "eval.json"))
    assert out[()]["weights"] == "raw" and out[("--ema",)]["weights"] == "ema"
    strip = lambda r: {k: v for k, v in r.items() if k not in ("weights", "checkpoint", "ed_checkpoint")}  # noqa: E731
    ev = EV.Evaluator(cfg, None, "cuda", B)
    ev.load_generator(full)
    ev.load_critic(full)
    cli_val = GANDataset.synthetic(20, T, C, cfg["LATENT_DIM"], int(cfg.get("SEED", 42)) + 1, "cuda")
    assert strip(out[()]) == json.loads(json.dumps(ev.evaluate(cli_val, 11)))
    assert set(out[()]) == set(strip(out[()])) | {"weights", "checkpoint", "ed_checkpoint"}
    assert strip(out[("--ema",)]) != strip(out[()])
    assert EV.main(["--config", str(cp), "--ckpt", final, "--synthetic", "20", "--ema"]) == 2
    gen = ["--config", str(cp), "--ckpt", full, "--emotion", "happy", "--samples", "2", "--batch", str(B), "--seed", "11"]
    for flag, want in (((), "raw"), (("--ema",), "ema")):
        assert GN.main(gen + ["--out", str(tmp_path / ("g" + want)), *flag]) == 0
        assert json.load(open(tmp_path / ("g" + want) / "summary.json"))["weights"] == want
    assert GN.main(["--config", str(cp), "--ckpt", final, "--ema"]) == 2
