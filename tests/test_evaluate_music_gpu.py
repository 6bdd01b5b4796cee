"""GPU: the evaluator's note-level musical statistics (Evaluator(music=True), --music-metrics): every number of the report's
`music` block against music_metrics.host_stats of the split's rolls and the engine's own generated rolls, its independence
of the batch size, the flag leaving the rest of the report untouched, and the CLI.  Fixtures are built in tmp_path."""
import json
import os
import subprocess
import sys

import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd.gan import evaluate as EV  # noqa: E402
from melo_gan_amd.gan import music_metrics as MM  # noqa: E402
from melo_gan_amd.gan.dataset import GANDataset  # noqa: E402
from oracle import melo_oracle as O  # noqa: E402
from test_evaluate_gpu import gen_state, save_state  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
K, N_ROWS, T, C = 4, 150, 32, 4


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("music"))
    S, cfg, ed_cfg = gen_state(T, C, "warm_start", "notes")
    ck, ed = save_state(S, d)
    real, numeric, _, _ = O.synthetic_batch(N_ROWS, T, C, cfg["LATENT_DIM"], 6, 7)
    real = real.clone()
    real[9, :, 1] = -1.0            # a row of rests (non-finite positions are tests/test_note_stats_gpu.py's: here they would
    #                                 turn the critic's and the classifier's means into NaN)
    labels = (torch.arange(N_ROWS) * 7 // 3) % K
    return {"cfg": cfg, "ed_cfg": ed_cfg, "ck": ck, "ed": ed, "real": real, "numeric": numeric, "labels": labels}


def dataset(s, n=N_ROWS):
    return GANDataset(s["real"][:n].numpy(), s["labels"][:n].numpy(), s["numeric"][:n].numpy(), None, s["cfg"]["LATENT_DIM"], "cuda")


def evaluator(s, batch, music=True):
    ev = EV.Evaluator(s["cfg"], s["ed_cfg"], "cuda", batch, music=music)
    ev.load_generator(s["ck"])
    ev.load_critic(s["ck"])
    ev.load_ed(s["ed"])
    return ev


def same(a, b, path="music"):
    """Integers, nulls and names equal; floats to 1e-12 relative."""
    assert type(a) is type(b), (path, a, b)
    if isinstance(a, dict):
        assert list(a) == list(b), path
        for k in a:
            same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, list):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{path}[{i}]")
    elif isinstance(a, float):
        assert abs(a - b) <= 1e-12 * abs(b), (path, a, b)
    else:
        assert a == b, (path, a, b)


def test_music_block_matches_the_host(setup):
    s, B = setup, 64
    ev = evaluator(s, B)
    # The engine's own generated rolls of every split row, from further passes under the same seed: a row's noise depends on
    # (seed, row) alone and a batch's launches on nothing outside the batch, so the last batch of a pass over the first 64,
    # the first 128 and all 150 rows is batch 0, 1 and 2 of the full pass (tests/test_evaluate_features_gpu.py's own_rolls).
    rolls = []
    for n, m in ((B, B), (2 * B, B), (N_ROWS, N_ROWS - 2 * B)):
        ev.evaluate(dataset(s, n), seed=3)
        rolls.append(ev.eng.fake_d[:m].cpu())
    rolls = torch.cat(rolls)
    ds = dataset(s)
    rep = ev.evaluate(ds, seed=3)                                          # 150 rows in batches of 64: a padded tail of 42
    assert torch.equal(ev.eng.fake_d[:N_ROWS - 2 * B].cpu(), rolls[2 * B:])
    json.loads(json.dumps(rep, allow_nan=False))
    acc, row_i, row_beats = MM.host_stats(s["real"].numpy(), rolls.numpy(), s["labels"].numpy(), K)
    want = MM.music_block(MM.acc_views(acc), {"row_i": row_i, "row_beats": row_beats}, s["labels"].numpy(), EV.EMOTIONS)
    same(rep["music"], want)
    counts = torch.bincount(s["labels"], minlength=K).tolist()
    for side in MM.SIDES:
        assert [rep["music"][side][nm]["rows"] for nm in EV.EMOTIONS] == counts
        assert sum(rep["music"][side][nm]["events"] + rep["music"][side][nm]["invalid"] for nm in EV.EMOTIONS) == N_ROWS * T
    assert sum(rep["music"]["real"][nm]["invalid"] for nm in EV.EMOTIONS) == 0
    # gen_state's closed-form generator keeps the velocity channel below the rest threshold at this size: its side is rests
    # only (sounding generated rows are tests/test_note_stats_gpu.py's), the split's side is music
    for q in ("notes", "rests", "transitions"):
        print(q, {side: [rep["music"][side][nm][q] for nm in EV.EMOTIONS] for side in MM.SIDES})
        assert all(rep["music"]["real"][nm][q] > 0 for nm in EV.EMOTIONS), q
    assert sum(rep["music"]["fake"][nm]["events"] for nm in EV.EMOTIONS) == N_ROWS * T
    assert rep["music"]["js_real_vs_generated"][EV.EMOTIONS[0]]["step"] is not None
    assert "Jensen-Shannon" in EV.format_table(rep)
    # a second pass replays the cached graph from zeroed accumulators: the same report, to the bit
    assert ev.evaluate(ds, seed=3) == rep


def test_music_block_does_not_depend_on_the_batch_size(setup):
    ds = dataset(setup)
    blocks = {B: evaluator(setup, B).evaluate(ds, seed=5)["music"] for B in (64, 37)}
    assert blocks[64] == blocks[37]


def test_the_flag_disturbs_nothing(setup):
    ds = dataset(setup)
    plain, music = evaluator(setup, 64, music=False), evaluator(setup, 64, music=True)
    rep0, rep1 = plain.evaluate(ds, seed=3), music.evaluate(ds, seed=3)
    assert "music" not in rep0 and "music" in rep1 and plain.music_buf is None
    assert "Jensen-Shannon" not in EV.format_table(rep0)
    assert rep0 == {k: v for k, v in rep1.items() if k != "music"}         # every other key, to the bit
    assert torch.equal(plain.acc.cpu(), music.acc.cpu())


def test_cli_music_metrics(tmp_path, setup):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "gan_config.yaml")))
    cfg.update(MAX_NOTES=T, LOG_DIR=str(tmp_path / "log"))
    cp, ep = tmp_path / "gan.yaml", tmp_path / "ed.yaml"
    cp.write_text(yaml.safe_dump(cfg))
    ep.write_text(yaml.safe_dump(setup["ed_cfg"]))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = ["timeout", "-k", "10", "400", sys.executable, "-m", "melo_gan_amd.gan.evaluate", "--ckpt", setup["ck"], "--ed_config", str(ep),
           "--ed_ckpt", setup["ed"], "--synthetic", "96", "--batch", "40", "--seed", "7", "--music-metrics"]
    r = subprocess.run(cmd + ["--config", str(cp)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=450)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    rep = json.load(open(tmp_path / "log" / "eval.json"))
    m = rep["music"]
    assert rep["n"] == 96 and m["emotions"] == list(EV.EMOTIONS) and m["features"] == list(MM.FEATURES)
    for side in MM.SIDES:
        assert sum(m[side][nm]["rows"] for nm in EV.EMOTIONS) == 96
        assert sum(m[side][nm]["events"] + m[side][nm]["invalid"] for nm in EV.EMOTIONS) == 96 * T
    assert set(m["js_tables"]) == set(MM.FEATURES) and len(m["js_tables"]["pitch"]["real_vs_generated"]) == K
    assert "music (notes by the output contract" in r.stdout and "Jensen-Shannon" in r.stdout
    # the piano-roll configuration: refused on the host, exit status 2
    cfg128 = tmp_path / "gan128.yaml"
    cfg128.write_text(yaml.safe_dump(dict(cfg, NOTE_DIM=128)))
    r = subprocess.run(cmd + ["--config", str(cfg128)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=450)
    assert r.returncode == 2 and "--music-metrics: NOTE_DIM = 128" in r.stderr, (r.returncode, r.stderr[-2000:])
