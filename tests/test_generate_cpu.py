"""CPU: the sampling CLI (melo_gan_amd.gan.generate) -- app.py's emotion table, jitter and scale / tempo map restated as
data, and every bad input rejected on the host with its message before any GPU use."""
import os
import subprocess
import sys

import pytest
import torch
import yaml

import melo_gan_amd  # noqa: F401
from melo_gan_amd.gan import generate as G
from oracle import melo_oracle as O

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# app.py:53-65 (get_gan_features) and :109-110 (scale, bpm), as data
APP_TABLE = {"happy": [1.0, 1.0, 0.8, 0.8, 0.5, 0.5], "sad": [-1.0, -1.0, -0.5, -0.5, -0.5, -0.5],
             "angry": [1.0, -1.0, 1.0, 1.0, -0.8, 0.8], "calm": [-1.0, 1.0, -0.8, -0.8, 0.5, -0.5]}
APP_STYLE = {"happy": ("major", 140), "sad": ("minor", 70), "angry": ("minor", 160), "calm": ("major", 90)}


def test_emotion_table_jitter_and_style_are_app_py_s():
    from melo_gan_amd.gan.utils import emotion_to_index
    assert G.EMOTIONS == ("happy", "sad", "angry", "calm")
    for e, row in APP_TABLE.items():
        assert emotion_to_index(e) == G.EMOTIONS.index(e)            # the classifier's class order
        assert list(G.EMOTION_TABLE[G.EMOTIONS.index(e)]) == row
    assert G.JITTER == 0.15
    assert G.STYLE == APP_STYLE
    assert G.emotion_names("all") == list(G.EMOTIONS) and G.emotion_names("Sad") == ["sad"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """A small GAN config (T = 16), a generator checkpoint of it, a notes-mode ED config and checkpoint."""
    d = tmp_path_factory.mktemp("gen_cpu")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "gan_config.yaml")))
    cfg.update(MAX_NOTES=16, CHECKPOINT_DIR=str(d / "ck"), SAMPLE_DIR=str(d / "samples"))
    ed_cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ed_config.yaml")))
    S = O.build_gan_state(O.default_gan_cfg(2, 16, 4), O.default_ed_cfg(4))
    paths = {}

    def dump(name, obj):
        paths[name] = str(d / name)
        with open(paths[name], "w") as f:
            yaml.safe_dump(obj, f)

    dump("gan.yaml", cfg)
    dump("ed.yaml", ed_cfg)
    dump("gan_num7.yaml", dict(cfg, NUMERIC_INPUT_DIM=7))
    dump("gan_c8.yaml", dict(cfg, NOTE_DIM=8))
    dump("ed_5cls.yaml", dict(ed_cfg, n_classes=5))
    dump("ed_note8.yaml", dict(ed_cfg, note_dim=8))
    dump("ed_lat32.yaml", dict(ed_cfg, input_mode="latent", latent_dim=32))
    os.makedirs(d / "ck")
    paths["ckpt"] = str(d / "ck" / "gan_final.pth")
    torch.save({"G": {**S.PG, **S.BG}, "E_num": S.PE}, paths["ckpt"])
    paths["no_enum"] = str(d / "no_enum.pth")
    torch.save({"G": {**S.PG, **S.BG}}, paths["no_enum"])
    paths["no_g"] = str(d / "no_g.pth")
    torch.save({"E_num": S.PE, "D": S.PD}, paths["no_g"])
    paths["ed_ckpt"] = str(d / "ed_best.pth")
    torch.save({"model": {**S.PED, **S.BED}}, paths["ed_ckpt"])
    return paths


def run(capsys, *argv):
    rc = G.main(list(argv))
    return rc, capsys.readouterr().err


@pytest.mark.parametrize("case", ["emotion", "samples", "batch", "numeric_dim", "note_dim", "ckpt_missing", "no_g", "no_enum",
                                  "ed_ckpt_alone", "ed_config_alone", "ed_ckpt_missing", "ed_classes", "ed_note_dim",
                                  "ed_latent_dim"])
def test_bad_inputs_fail_on_the_host(files, capsys, case):
    f = files
    base = ["--config", f["gan.yaml"], "--ckpt", f["ckpt"]]
    argv, msg = {
        "emotion": (base + ["--emotion", "joyful"], "unknown emotion 'joyful'"),
        "samples": (base + ["--samples", "0"], "--samples 0: must be >= 1"),
        "batch": (base + ["--batch", "0"], "--batch 0: must be >= 1"),
        "numeric_dim": (["--config", f["gan_num7.yaml"], "--ckpt", f["ckpt"]], "NUMERIC_INPUT_DIM = 7"),
        "note_dim": (["--config", f["gan_c8.yaml"], "--ckpt", f["ckpt"]], "NOTE_DIM = 8"),
        "ckpt_missing": (["--config", f["gan.yaml"], "--ckpt", f["ckpt"] + ".gone"], "does not exist"),
        "no_g": (["--config", f["gan.yaml"], "--ckpt", f["no_g"]], "needs 'G' and 'E_num'"),
        "no_enum": (["--config", f["gan.yaml"], "--ckpt", f["no_enum"]], "needs 'G' and 'E_num'"),
        "ed_ckpt_alone": (base + ["--ed_ckpt", f["ed_ckpt"]], "--ed_ckpt needs --ed_config"),
        "ed_config_alone": (base + ["--ed_config", f["ed.yaml"]], "--ed_config needs --ed_ckpt"),
        "ed_ckpt_missing": (base + ["--ed_config", f["ed.yaml"], "--ed_ckpt", f["ed_ckpt"] + ".gone"],
                            "ED checkpoint " + f["ed_ckpt"] + ".gone does not exist"),
        "ed_classes": (base + ["--ed_config", f["ed_5cls.yaml"], "--ed_ckpt", f["ed_ckpt"]], "n_classes = 5"),
        "ed_note_dim": (base + ["--ed_config", f["ed_note8.yaml"], "--ed_ckpt", f["ed_ckpt"]], "note_dim = 8"),
        "ed_latent_dim": (base + ["--ed_config", f["ed_lat32.yaml"], "--ed_ckpt", f["ed_ckpt"]], "latent_dim = 32"),
    }[case]
    rc, err = run(capsys, *argv)
    assert rc != 0 and msg in err, (rc, err)


def test_valid_inputs_pass_the_host_checks(files):
    """The checks accept a valid request (defaults from the config: gan_final.pth under CHECKPOINT_DIR, SAMPLE_DIR,
    N_SAMPLES_PER_EMOTION, SEED); only the GPU work remains."""
    p = G.plan(G.parse_args(["--config", files["gan.yaml"], "--ed_config", files["ed.yaml"], "--ed_ckpt", files["ed_ckpt"]]))
    assert p.ckpt_path == files["ckpt"] and p.emotions == list(G.EMOTIONS) and p.samples == 2 and p.seed == 42
    assert p.out.endswith("samples") and p.batch == 64 and p.ed_cfg["input_mode"] == "notes"
    p = G.plan(G.parse_args(["--config", files["gan.yaml"], "--emotion", "calm", "--samples", "3", "--seed", "9",
                             "--batch", "5", "--out", "x"]))
    assert (p.emotions, p.samples, p.seed, p.batch, p.out, p.ed_cfg) == (["calm"], 3, 9, 5, "x", None)


def test_cli_process_exits_nonzero_with_the_message(files):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "melo_gan_amd.gan.generate", "--config", files["gan.yaml"], "--ckpt",
                        files["no_enum"]], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "needs 'G' and 'E_num'" in r.stderr, (r.returncode, r.stderr[-2000:])


def test_ops_refuse_cpu_tensors():
    from melo_gan_amd import ops
    keys = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.gen_inputs(keys, keys, torch.zeros(4, 128), torch.zeros(4, 6), torch.zeros(4, 6), 0.15, None, 1)
    with pytest.raises(ValueError):
        ops.emotion_score(torch.zeros(4, 4), keys, torch.zeros(4), keys, torch.zeros(4, 3, dtype=torch.float64))
