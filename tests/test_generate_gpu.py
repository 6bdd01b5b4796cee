"""GPU: emotion-conditioned sampling (melo_gan_amd.gan.generate) -- the input kernel mg_gen_inputs (app.py's table + jitter,
Philox keyed per (emotion, sample)), the scoring kernel mg_emotion_score against torch.softmax / torch.argmax, the Sampler
against the oracle, and the CLI end to end through the MIDI contract.  Fixtures are built in tmp_path."""
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
from melo_gan_amd import midi, ops  # noqa: E402
from melo_gan_amd.gan import generate as G  # noqa: E402
from oracle import melo_oracle as O  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NOISE, NUM, LAT = 128, 6, 64


def draw(keys, seed, jitter=G.JITTER, graph=False):
    """mg_gen_inputs for a list of (emotion, sample) keys into NaN-filled buffers; returns host copies."""
    n = len(keys)
    kt = torch.tensor(keys, dtype=torch.int32).t().contiguous().cuda()
    noise, numeric, latent = (torch.full((n, w), float("nan"), device="cuda") for w in (NOISE, NUM, LAT))
    table = torch.tensor(G.EMOTION_TABLE, dtype=torch.float32, device="cuda")
    launch = lambda: ops.gen_inputs(kt[0], kt[1], noise, numeric, table, jitter, latent, seed)  # noqa: E731
    if graph:
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            g = ops.Graph()
            g.begin()
            launch()
            g.end()
            g.launch()
            torch.cuda.synchronize()
    else:
        launch()
    torch.cuda.synchronize()
    return noise.cpu(), numeric.cpu(), latent.cpu()


def test_gen_inputs_table_rows_and_zero_latent():
    keys = [(e, k) for k in (1, 2, 3) for e in range(4)] + [(-1, 0), (-1, 5)]
    noise, numeric, latent = draw(keys, 11, jitter=0.0)
    table = torch.tensor(G.EMOTION_TABLE, dtype=torch.float32)
    for r, (e, _) in enumerate(keys):
        if e >= 0:
            assert torch.equal(numeric[r], table[e]), (r, numeric[r], table[e])
            assert torch.isfinite(noise[r]).all() and noise[r].abs().sum() > 0
        else:       # padding rows are written too
            assert torch.equal(numeric[r], torch.zeros(NUM)) and torch.equal(noise[r], torch.zeros(NOISE))
    assert torch.equal(latent, torch.zeros_like(latent))


def test_gen_inputs_depend_on_the_key_alone():
    keys = [(e, k) for e in range(4) for k in range(1, 17)]           # 64 keys
    ref = dict(zip(keys, zip(*draw(keys, 5)[:2])))
    rng = np.random.default_rng(0)
    for chunk in (1, 3, 64):
        for order in (keys, [keys[i] for i in rng.permutation(len(keys))]):
            for c0 in range(0, len(order), chunk):
                part = order[c0:c0 + chunk]
                nz, nm, _ = draw(part, 5)
                for r, key in enumerate(part):
                    assert torch.equal(nz[r], ref[key][0]) and torch.equal(nm[r], ref[key][1]), (chunk, key)
    nz, nm, lt = draw(keys, 5, graph=True)                            # replayed graph == eager launch
    for r, key in enumerate(keys):
        assert torch.equal(nz[r], ref[key][0]) and torch.equal(nm[r], ref[key][1])
    assert torch.equal(lt, torch.zeros_like(lt))


def test_gen_inputs_statistics_and_distinct_draws():
    keys = [(e, k) for e in range(4) for k in range(1, 5001)]         # 20000 rows: 120000 numeric, 2.56 M noise draws
    noise, numeric, _ = draw(keys, 1234)
    table = torch.tensor(G.EMOTION_TABLE, dtype=torch.float64)[torch.tensor([e for e, _ in keys])]
    z = (numeric.double() - table) / 0.15
    for name, x in (("noise", noise.double().flatten()), ("numeric jitter", z.flatten())):
        n = x.numel()
        assert n >= 100000
        assert abs(float(x.mean())) <= 5.0 / n ** 0.5, (name, float(x.mean()))
        assert abs(float(x.std()) - 1.0) <= 5.0 / (2.0 * n) ** 0.5, (name, float(x.std()))
    assert torch.unique(noise, dim=0).shape[0] == len(keys)          # no two keys share a noise row
    other = draw(keys[:64], 1235)[0]
    assert not torch.equal(other, noise[:64]) and (other != noise[:64]).float().mean() > 0.99


@pytest.mark.parametrize("n_classes", [4, 7])
def test_emotion_score_matches_torch(n_classes):
    g = torch.Generator().manual_seed(n_classes)
    rows = 300                                                          # > one 256-row tile
    logits = torch.randn(rows, n_classes, generator=g) * 3
    for r in range(0, rows, 7):                                         # planted ties: first index wins
        j0, j1 = sorted(torch.randperm(n_classes, generator=g)[:2].tolist())
        logits[r, j0] = logits[r, j1] = logits[r].max() + 1.0
    target = torch.randint(0, n_classes, (rows,), generator=g, dtype=torch.int32)
    target[::11] = -1                                                   # padding rows
    lg, tg = logits.cuda(), target.cuda()
    p = torch.full((rows,), float("nan"), device="cuda")
    pred = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
    acc = torch.zeros(n_classes, 3, dtype=torch.float64, device="cuda")
    ops.emotion_score(lg, tg, p, pred, acc)
    ops.emotion_score(lg, tg, p, pred, acc)                             # accumulates
    torch.cuda.synchronize()
    ref_pred = torch.argmax(lg, dim=1).cpu()
    assert torch.equal(pred.cpu().long(), ref_pred)
    sm = torch.softmax(lg, dim=1).cpu()
    ok = target >= 0
    ref_p = torch.where(ok, sm[torch.arange(rows), target.clamp(min=0).long()], torch.zeros(rows))
    assert float((p.cpu() - ref_p).abs().max()) <= 1e-6
    a, pc = acc.cpu(), p.cpu().double()
    for c in range(n_classes):
        m = target == c
        assert a[c, 0].item() == 2 * int(m.sum()) and a[c, 1].item() == 2 * int((m & (ref_pred == c)).sum())
        host = 2 * float(pc[m].sum())
        assert abs(a[c, 2].item() - host) <= 1e-12 * max(abs(host), 1e-30), (c, a[c, 2].item(), host)


def gen_state(T, C, mode, ed_mode):
    """Closed-form weights as tests/golden/make_golden.py::gen1_case builds them (generator x4, last deconvolution x400 with
    the fixture's centring bias where one exists for the shape, non-trivial BatchNorm running statistics): outputs that
    span the MIDI writer's branches."""
    cfg, ed_cfg = O.default_gan_cfg(8, T, C), O.default_ed_cfg(C)
    cfg["INTEGRATION_MODE"], ed_cfg["input_mode"] = mode, ed_mode
    S = O.build_gan_state(cfg, ed_cfg, "closed_form")
    for k in S.PG:
        if k.endswith("weight") and S.PG[k].dim() > 1:
            S.PG[k].mul_(4.0 * (400.0 if k == "decoder.deconv.6.weight" else 1.0))
    gen1 = os.path.join(ROOT, "tests", "golden", f"gen1_c{C}_t{T}.npz")
    if os.path.exists(gen1):
        S.PG["decoder.deconv.6.bias"].copy_(torch.from_numpy(np.load(gen1)["bias6"]))
    S.BG.update(O.fill_buffers(O.generator_buffers(), 70.0))
    return S, cfg, ed_cfg


def save_state(S, d):
    ck, ed = os.path.join(d, "gan_final.pth"), os.path.join(d, "ed_best.pth")
    torch.save({"G": {**S.PG, **S.BG}, "E_num": S.PE}, ck)
    torch.save({"model": {**S.PED, **S.BED}}, ed)
    return ck, ed


@pytest.mark.parametrize("T,C,mode,ed_mode", [(512, 4, "warm_start", "notes"), (256, 128, "warm_start", "notes"),
                                              (16, 4, "conditioning", "latent")])
def test_sampler_matches_the_oracle(tmp_path, T, C, mode, ed_mode):
    S, cfg, ed_cfg = gen_state(T, C, mode, ed_mode)
    ck, ed = save_state(S, str(tmp_path))
    smp = G.Sampler(cfg, ed_cfg, "cuda", 8)
    smp.load_generator(ck)
    smp.load_ed(ed)
    res = smp.sample(["all"], 2, seed=3)                                # 8 rows = one chunk: the engine keeps its buffers
    eng = smp.eng
    assert res.emotion == [e for e in G.EMOTIONS for _ in range(2)] and res.k == [1, 2] * 4
    noise, numeric = eng.noise.cpu(), eng.numeric.cpu()
    nz, nm, _ = draw(list(zip([G.EMOTIONS.index(e) for e in res.emotion], res.k)), 3)
    assert torch.equal(noise, nz) and torch.equal(numeric, nm)          # graph replay == eager draw
    latent_in = torch.zeros(8, cfg["LATENT_DIM"])
    with torch.no_grad():
        emb = O.feature_encoder_fwd(S.PE, numeric, None)
        gen, lat = O.generator_fwd(S.PG, S.BG, noise, latent_in, emb, mode, T, train=False)
    np.testing.assert_allclose(eng.emb.cpu().numpy(), emb.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(eng.lat.cpu().numpy(), lat.numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(res.notes, gen.numpy(), rtol=1e-3, atol=1e-4)
    # the classifier on the Sampler's own notes (or latent)
    x = torch.from_numpy(res.notes) if ed_mode == "notes" else eng.lat.cpu()
    with torch.no_grad():
        ref = O.emotion_disc_fwd(S.PED, S.BED, x, ed_cfg, train=False)
    logits = eng.logits.cpu()
    np.testing.assert_allclose(logits.numpy(), ref.numpy(), rtol=1e-4, atol=2e-6)
    top2 = torch.topk(ref, 2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4
    assert clear.any()
    assert np.array_equal(res.pred[clear.numpy()], torch.argmax(ref, 1)[clear].numpy())
    tgt = torch.tensor([G.EMOTIONS.index(e) for e in res.emotion])
    np.testing.assert_allclose(res.p_target, torch.softmax(ref, 1)[torch.arange(8), tgt].numpy(), rtol=0, atol=1e-5)
    for e in G.EMOTIONS:
        m = np.array([x == e for x in res.emotion])
        s = res.summary[e]
        assert s["n"] == 2 and s["ed_accuracy"] == float((res.pred[m] == G.EMOTIONS.index(e)).mean())
        assert abs(s["ed_mean_p_target"] - float(res.p_target[m].astype(np.float64).mean())) <= 1e-7


def test_cli_end_to_end(tmp_path):
    S, _, ed_cfg = gen_state(512, 4, "warm_start", "notes")
    ck, ed = save_state(S, str(tmp_path))
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "gan_config.yaml")))
    assert (cfg["MAX_NOTES"], cfg["NOTE_DIM"], cfg["INTEGRATION_MODE"]) == (512, 4, "warm_start")
    ed_yaml = tmp_path / "ed.yaml"
    ed_yaml.write_text(yaml.safe_dump(ed_cfg))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def cli(out, emotion):
        r = subprocess.run([sys.executable, "-m", "melo_gan_amd.gan.generate", "--config", os.path.join(ROOT, "config", "gan_config.yaml"),
                            "--ckpt", ck, "--emotion", emotion, "--samples", "2", "--seed", "7", "--out", str(out),
                            "--ed_config", str(ed_yaml), "--ed_ckpt", ed], cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=400)
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
        return r

    r = cli(tmp_path / "all", "all")
    names = sorted(f for f in os.listdir(tmp_path / "all") if f.endswith(".mid"))
    assert names == sorted(f"test_{e}_{k}.mid" for e in G.EMOTIONS for k in (1, 2))
    assert all(e in r.stdout for e in G.EMOTIONS)
    # the same seed and batch in process: the files are save_piano_roll_to_midi of these notes, byte for byte
    smp = G.Sampler(cfg, ed_cfg, "cuda", 64)
    smp.load_generator(ck)
    smp.load_ed(ed)
    res = smp.sample(["all"], 2, seed=7)
    summary = json.load(open(tmp_path / "all" / "summary.json"))
    assert summary["seed"] == 7 and summary["samples"] == 2 and summary["emotions"] == list(G.EMOTIONS)
    by_file = {f["file"]: f for f in summary["files"]}
    assert sorted(by_file) == names
    for i, (e, k) in enumerate(zip(res.emotion, res.k)):
        path = tmp_path / "all" / f"test_{e}_{k}.mid"
        (fmt, div), tempo, notes = midi.read_smf_notes(str(path))
        scale, bpm = G.STYLE[e]
        assert (fmt, div) == (1, 220) and tempo == round(6e7 / bpm) and len(notes) > 0
        allowed = set(midi.SCALES[scale])
        assert {n[2] % 12 for n in notes} <= allowed, (e, sorted({n[2] % 12 for n in notes}))
        ref = str(tmp_path / "ref.mid")
        midi.save_piano_roll_to_midi(res.notes[i], ref, bpm=bpm, scale=scale, root_key=0)
        assert path.read_bytes() == open(ref, "rb").read(), path
        f = by_file[path.name]
        assert (f["emotion"], f["k"], f["ed_pred"]) == (e, k, G.EMOTIONS[int(res.pred[i])])
        assert abs(f["ed_p_target"] - float(res.p_target[i])) <= 1e-7
    for e in G.EMOTIONS:
        files = [f for f in summary["files"] if f["emotion"] == e]
        s = summary["per_emotion"][e]
        assert s["n"] == len(files) == 2
        assert s["ed_accuracy"] == sum(f["ed_pred"] == e for f in files) / len(files)
        assert abs(s["ed_mean_p_target"] - sum(f["ed_p_target"] for f in files) / len(files)) <= 1e-7
    # --emotion happy alone, same --batch: happy fills rows 0-1 of a 64-row chunk again -> identical bytes
    cli(tmp_path / "happy", "happy")
    assert sorted(f for f in os.listdir(tmp_path / "happy") if f.endswith(".mid")) == ["test_happy_1.mid", "test_happy_2.mid"]
    for k in (1, 2):
        assert (tmp_path / "happy" / f"test_happy_{k}.mid").read_bytes() == (tmp_path / "all" / f"test_happy_{k}.mid").read_bytes()
