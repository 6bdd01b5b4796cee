"""CPU: the evaluation CLI (melo_gan_amd.gan.evaluate) -- every bad input rejected on the host with the offending path or
key in the message, a checkpoint without a critic accepted (critic metrics null), and the report assembled from a hand-made
raw accumulator."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import melo_gan_amd  # noqa: F401
from melo_gan_amd.gan import evaluate as EV
from oracle import melo_oracle as O

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
T, C, N = 16, 4, 10


def write_split(root, name, notes=None, emotion=None, numeric=None):
    d = root / "splits" / name
    os.makedirs(d)
    g = np.random.default_rng(1)
    np.save(d / "notes.npy", g.uniform(-1, 1, (N, T, C)).astype(np.float32) if notes is None else notes)
    np.save(d / "emotion.npy", (np.arange(N) % 4) if emotion is None else emotion)
    np.save(d / "numeric_features.npy", g.standard_normal((N, 6)).astype(np.float32) if numeric is None else numeric)
    return str(root / "splits" / (name + ".csv"))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("eval_cpu")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "gan_config.yaml")))
    cfg.update(MAX_NOTES=T, CHECKPOINT_DIR=str(d / "ck"), LOG_DIR=str(d / "logs"), SPLITS_DIR=str(d / "splits"))
    cfg["VAL_SPLIT"] = write_split(d, "val")
    cfg["ENCODER_FEATS_VAL"] = str(d / "splits" / "val" / "encoder_feats.npy")      # absent: zeros, as the trainer
    ed_cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ed_config.yaml")))
    S = O.build_gan_state(O.default_gan_cfg(2, T, C), O.default_ed_cfg(C))
    paths = {"dir": d}

    def dump(name, obj):
        paths[name] = str(d / name)
        with open(paths[name], "w") as f:
            yaml.safe_dump(obj, f)

    dump("gan.yaml", cfg)
    dump("gan_noval.yaml", {k: v for k, v in cfg.items() if k != "VAL_SPLIT"})
    dump("gan_c6.yaml", dict(cfg, NOTE_DIM=6))
    dump("ed.yaml", ed_cfg)
    dump("ed_note8.yaml", dict(ed_cfg, note_dim=8))
    dump("ed_lat32.yaml", dict(ed_cfg, input_mode="latent", latent_dim=32))
    paths["split_t8"] = write_split(d, "t8", notes=np.zeros((N, 8, C), np.float32))
    paths["split_num5"] = write_split(d, "num5", numeric=np.zeros((N, 5), np.float32))
    paths["split_len"] = write_split(d, "len", emotion=np.arange(N - 1) % 4)
    paths["split_label"] = write_split(d, "label", emotion=np.array([0, 1, 2, 3, 4, 0, 1, 2, 3, 0]))
    paths["split_name"] = write_split(d, "name", emotion=np.array(["happy", "sad", "angry", "calm", "bored"] * 2, dtype=object))
    paths["split_gone"] = str(d / "splits" / "gone.csv")
    paths["feats_bad"] = str(d / "feats_bad.npy")
    np.save(paths["feats_bad"], np.zeros((N, 7), np.float32))
    os.makedirs(d / "ck")
    paths["final"] = str(d / "ck" / "gan_final.pth")
    torch.save({"G": {**S.PG, **S.BG}, "E_num": S.PE}, paths["final"])
    paths["full"] = str(d / "ck" / "gan_epoch0005.pth")
    torch.save({"epoch": 5, "G": {**S.PG, **S.BG}, "E_num": S.PE, "D": S.PD}, paths["full"])
    paths["bad_d"] = str(d / "bad_d.pth")
    torch.save({"G": {**S.PG, **S.BG}, "E_num": S.PE, "D": {**S.PD, "fc.1.weight": torch.zeros(3, 3)}}, paths["bad_d"])
    paths["no_enum"] = str(d / "no_enum.pth")
    torch.save({"G": {**S.PG, **S.BG}}, paths["no_enum"])
    paths["ed_ckpt"] = str(d / "ed_best.pth")
    torch.save({"model": {**S.PED, **S.BED}}, paths["ed_ckpt"])
    return paths


def run(capsys, *argv):
    rc = EV.main(list(argv))
    return rc, capsys.readouterr().err


@pytest.mark.parametrize("case", ["batch", "ckpt_missing", "no_enum", "bad_d", "note_dim_quad", "split_missing", "no_val_split",
                                  "notes_shape", "numeric_shape", "label_count", "label_range", "label_name", "feats_missing",
                                  "feats_shape", "ed_ckpt_alone", "ed_config_alone", "ed_ckpt_missing", "ed_note_dim",
                                  "ed_latent_dim"])
def test_bad_inputs_fail_on_the_host(files, capsys, case):
    f = files
    base = ["--config", f["gan.yaml"], "--ckpt", f["final"]]
    argv, msgs = {
        "batch": (base + ["--batch", "0"], ["--batch 0: must be >= 1"]),
        "ckpt_missing": (["--config", f["gan.yaml"], "--ckpt", f["final"] + ".gone"], [f["final"] + ".gone", "does not exist"]),
        "no_enum": (["--config", f["gan.yaml"], "--ckpt", f["no_enum"]], [f["no_enum"], "needs 'G' and 'E_num'"]),
        "bad_d": (["--config", f["gan.yaml"], "--ckpt", f["bad_d"]], [f["bad_d"], "D.fc.1.weight has shape (3, 3)"]),
        "note_dim_quad": (["--config", f["gan_c6.yaml"], "--ckpt", f["final"]], ["NOTE_DIM = 6"]),
        "split_missing": (base + ["--split", f["split_gone"]], [os.path.join("gone", "notes.npy"), "does not exist"]),
        "no_val_split": (["--config", f["gan_noval.yaml"], "--ckpt", f["final"]], ["lacks VAL_SPLIT"]),
        "notes_shape": (base + ["--split", f["split_t8"]], ["t8", "notes has shape (10, 8, 4)", "(n, 16, 4)"]),
        "numeric_shape": (base + ["--split", f["split_num5"]], ["num5", "numeric_features has shape (10, 5)"]),
        "label_count": (base + ["--split", f["split_len"]], ["len", "emotion holds 9 entries"]),
        "label_range": (base + ["--split", f["split_label"]], ["label", "1 of 10 outside [0, 4)", "first rows [4]"]),
        "label_name": (base + ["--split", f["split_name"]], ["name", "2 of 10 outside [0, 4)", "values [-1, -1]"]),
        "feats_missing": (base + ["--feats", f["feats_bad"] + ".gone"], [f["feats_bad"] + ".gone", "do not exist"]),
        "feats_shape": (base + ["--feats", f["feats_bad"]], ["encoder features have shape (10, 7)", "(10, 64)"]),
        "ed_ckpt_alone": (base + ["--ed_ckpt", f["ed_ckpt"]], ["--ed_ckpt needs --ed_config"]),
        "ed_config_alone": (base + ["--ed_config", f["ed.yaml"]], ["--ed_config needs --ed_ckpt"]),
        "ed_ckpt_missing": (base + ["--ed_config", f["ed.yaml"], "--ed_ckpt", f["ed_ckpt"] + ".gone"],
                            ["ED checkpoint " + f["ed_ckpt"] + ".gone does not exist"]),
        "ed_note_dim": (base + ["--ed_config", f["ed_note8.yaml"], "--ed_ckpt", f["ed_ckpt"]], [f["ed_note8.yaml"], "note_dim = 8"]),
        "ed_latent_dim": (base + ["--ed_config", f["ed_lat32.yaml"], "--ed_ckpt", f["ed_ckpt"]], [f["ed_lat32.yaml"], "latent_dim = 32"]),
    }[case]
    rc, err = run(capsys, *argv)
    assert rc != 0 and all(m in err for m in msgs), (rc, err)


def test_errors_are_value_errors(files):
    assert issubclass(EV.EvaluateError, ValueError)
    with pytest.raises(EV.EvaluateError, match="notes has shape"):
        EV.plan(EV.parse_args(["--config", files["gan.yaml"], "--ckpt", files["final"], "--split", files["split_t8"]]))


def test_valid_inputs_pass_the_host_checks(files):
    """Defaults from the config (gan_final.pth under CHECKPOINT_DIR, VAL_SPLIT, SEED, <LOG_DIR>/eval.json).  gan_final.pth holds
    no critic: not an error, the critic metrics will be null; a full checkpoint has one."""
    p = EV.plan(EV.parse_args(["--config", files["gan.yaml"], "--ed_config", files["ed.yaml"], "--ed_ckpt", files["ed_ckpt"]]))
    assert p.ckpt_path == files["final"] and p.has_critic is False and p.seed == 42 and p.batch == 64
    assert p.out == os.path.join(str(files["dir"] / "logs"), "eval.json") and p.ed_cfg["input_mode"] == "notes"
    notes, emotion, numeric, latent = p.arrays
    assert notes.shape == (N, T, C) and len(emotion) == N and numeric.shape == (N, 6) and latent is None
    p = EV.plan(EV.parse_args(["--config", files["gan.yaml"], "--ckpt", files["full"], "--synthetic", "40", "--seed", "9",
                               "--batch", "5", "--out", "x.json"]))
    assert (p.has_critic, p.synthetic, p.arrays, p.seed, p.batch, p.out, p.ed_cfg) == (True, 40, None, 9, 5, "x.json", None)


def test_cli_process_exits_nonzero_with_the_message(files):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "melo_gan_amd.gan.evaluate", "--config", files["gan.yaml"], "--ckpt",
                        files["final"], "--split", files["split_label"]], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "outside [0, 4)" in r.stderr, (r.returncode, r.stderr[-2000:])


def hand_made_raw(Tn=8, Cn=4):
    """A raw accumulator as a pass over 5 rows would leave it: classes 0 (3 rows), 1 (2 rows); classes 2 and 3 empty.
    Channel 0 of class 0 is the constant 0.1 (an fp32 value, squared in fp64)."""
    K = 4
    raw = {"n": np.array([3, 2, 0, 0], np.int64),
           "conf_fake": np.array([[2, 1, 0, 0], [0, 1, 0, 1], [0, 0, 0, 0], [0, 0, 0, 0]], np.int64),
           "conf_real": np.array([[3, 0, 0, 0], [0, 2, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], np.int64),
           "d_sum": np.array([2.5, -1.5]), "cls": np.zeros((2, 2, K)), "nsum": np.zeros((2, K, Cn)), "nsq": np.zeros((2, K, Cn)),
           "nmin": np.full((2, K, Cn), np.inf, np.float32), "nmax": np.full((2, K, Cn), -np.inf, np.float32)}
    raw["cls"][0, 0, :2], raw["cls"][0, 1, :2] = [3.0, 1.0], [1.5, 0.5]          # fake: CE sums, p sums
    raw["cls"][1, 0, :2], raw["cls"][1, 1, :2] = [0.3, 0.2], [2.7, 1.8]          # real
    raw["nmin"][:, :2], raw["nmax"][:, :2] = 0.0, 0.0                             # the live classes' other channels: all zeros
    c = float(np.float32(0.1))
    for side in range(2):
        raw["nsum"][side, 0, 0], raw["nsq"][side, 0, 0] = 3 * Tn * c, 3 * Tn * c * c
        raw["nmin"][side, 0, 0] = raw["nmax"][side, 0, 0] = np.float32(0.1)
        # class 1, channel 1: half the elements -1, half +3  ->  mean 1, std 2
        raw["nsum"][side, 1, 1], raw["nsq"][side, 1, 1] = Tn * (-1 + 3), Tn * (1 + 9)
        raw["nmin"][side, 1, 1], raw["nmax"][side, 1, 1] = -1.0, 3.0
    return raw


def test_report_from_a_hand_made_accumulator():
    raw = hand_made_raw()
    rep = EV.build_report(raw, 8, seed=7, batch=3, has_critic=True, has_ed_fake=True, has_ed_real=True)
    json.loads(json.dumps(rep, allow_nan=False))                 # plain values, no NaN / inf anywhere
    assert (rep["n"], rep["seed"], rep["batch"]) == (5, 7, 3)
    assert rep["critic"] == {"mean_real": 0.5, "mean_fake": -0.3, "w_dist": 0.8}
    f = rep["ed_fake"]
    assert f["confusion"] == raw["conf_fake"].tolist()
    assert f["accuracy"] == 3 / 5 and f["ce"] == 4.0 / 5 and f["mean_p_target"] == 2.0 / 5
    assert f["per_emotion"]["happy"] == {"n": 3, "accuracy": 2 / 3, "ce": 1.0, "mean_p_target": 0.5}
    assert f["per_emotion"]["sad"] == {"n": 2, "accuracy": 0.5, "ce": 0.5, "mean_p_target": 0.25}
    for name in ("angry", "calm"):                                # empty classes: n 0 and null, not NaN
        assert f["per_emotion"][name] == {"n": 0, "accuracy": None, "ce": None, "mean_p_target": None}
        for side in ("real", "fake"):
            e = rep["notes"][side][name]
            assert e["n_rows"] == 0 and len(e["channels"]) == 4
            assert all(ch == {"mean": None, "std": None, "min": None, "max": None} for ch in e["channels"])
    assert rep["ed_real"]["accuracy"] == 1.0 and rep["ed_real"]["per_emotion"]["sad"]["mean_p_target"] == 0.9
    for side in ("real", "fake"):
        ch = rep["notes"][side]["happy"]["channels"][0]          # a constant channel: std exactly 0, not NaN
        assert ch["std"] == 0.0 and ch["min"] == ch["max"] == float(np.float32(0.1))
        assert abs(ch["mean"] - float(np.float32(0.1))) <= 1e-15
        ch = rep["notes"][side]["sad"]["channels"][1]
        assert rep["notes"][side]["sad"]["n_rows"] == 2
        assert (ch["mean"], ch["std"], ch["min"], ch["max"]) == (1.0, 2.0, -1.0, 3.0)
    # no critic / no classifier / a classifier without a real side: null, not an error
    rep = EV.build_report(raw, 8, 7, 3, has_critic=False, has_ed_fake=True, has_ed_real=False)
    assert rep["critic"] is None and rep["ed_real"] is None and rep["ed_fake"] is not None
    assert EV.build_report(raw, 8, 7, 3, False, False, False)["ed_fake"] is None
    assert isinstance(EV.format_table(rep), str) and "w_dist" not in EV.format_table(rep)
    with pytest.raises(ValueError, match="lacks"):
        EV.build_report({k: v for k, v in raw.items() if k != "nsq"}, 8, 7, 3, True, True, True)


def test_std_of_a_constant_channel_survives_rounding():
    """sum x^2 - (sum x)^2 / N of a constant can come out a few ulps negative: the report clamps, never sqrt(negative)."""
    raw = hand_made_raw()
    raw["nsq"][0, 0, 0] = np.nextafter(raw["nsq"][0, 0, 0], 0.0)
    rep = EV.build_report(raw, 8, 7, 3, True, True, True)
    std = rep["notes"]["real"]["happy"]["channels"][0]["std"]
    assert std == 0.0 and not math.isnan(std)


def test_accumulator_layout_round_trip():
    """ops.eval_acc_layout is the header's layout: the views of a host accumulator address disjoint words that cover it."""
    from melo_gan_amd import ops
    lay = ops.eval_acc_layout(4, 8)
    acc = torch.zeros(lay["words"], dtype=torch.int64)
    views = ops.eval_acc_views(acc, 4, 8)
    assert set(views) == set(EV.RAW_KEYS)
    for i, k in enumerate(EV.RAW_KEYS):
        views[k].fill_(i + 1)
    assert (acc != 0).all()                                       # every word belongs to a view
    for i, k in enumerate(EV.RAW_KEYS):                           # and to one view only
        assert (views[k] == i + 1).all(), k
    assert views["nsum"].shape == (2, 4, 8) and views["nmin"].dtype == torch.float32 and views["cls"].dtype == torch.float64
    with pytest.raises(ValueError):
        ops.eval_acc_layout(4, 6)
    with pytest.raises(ValueError):
        ops.eval_acc_views(acc[:-1], 4, 8)


def test_ops_refuse_bad_arguments_before_any_launch():
    from melo_gan_amd import _lib, ops
    x, lab = torch.zeros(2, 8, 4), torch.zeros(2, dtype=torch.int64)
    acc = torch.zeros(ops.eval_acc_layout(4, 4)["words"], dtype=torch.int64)
    with pytest.raises(ValueError):
        ops.eval_acc(x, x, lab, None, None, torch.zeros(2, 4), None, acc)          # host tensors
    with pytest.raises(ValueError):
        ops.eval_noise(torch.zeros(2, 8), lab[:1], lab[:1], 2, 1)
    lib = _lib.load()
    a = 4096            # dummy aligned addresses: argument checks answer before any launch
    assert lib.mg_eval_acc(None, a, 2, 8, 4, a, None, None, None, None, 4, a, a, 1 << 20, None, None) == -1
    assert b"null" in lib.mg_last_error()
    assert lib.mg_eval_acc(a, a, 2, 8, 6, a, None, None, None, None, 4, a, a, 1 << 20, None, None) == -1
    assert b"multiple of 4" in lib.mg_last_error()
    assert lib.mg_eval_acc(a, a + 4, 2, 8, 4, a, None, None, None, None, 4, a, a, 1 << 20, None, None) == -1
    assert b"16-byte" in lib.mg_last_error()
    assert lib.mg_eval_acc(a, a, 2, 8, 4, a, a, None, None, None, 4, a, a, 1 << 20, None, None) == -1
    assert b"go together" in lib.mg_last_error()
    assert lib.mg_eval_acc(a, a, 2, 8, 4, a, None, None, None, None, 33, a, a, 1 << 20, None, None) == -1
    assert lib.mg_eval_acc(a, a, 0, 8, 4, a, None, None, None, None, 4, a, a, 1 << 20, None, None) == -1
    need = lib.mg_eval_acc_workspace_bytes(2, 8, 4)
    assert need > 0 and lib.mg_eval_acc(a, a, 2, 8, 4, a, None, None, None, None, 4, a, a, need - 1, None, None) == -3
    assert lib.mg_eval_acc_reset(None, 4, 4, None) == -1 and lib.mg_eval_acc_reset(a, 4, 5, None) == -1
    assert lib.mg_eval_noise(None, 2, 8, a, a, 2, 1, None) == -1 and lib.mg_eval_noise(a, 2, 8, a, a, 0, 1, None) == -1
    assert lib.mg_eval_acc_words(4, 4) == ops.eval_acc_layout(4, 4)["words"] and lib.mg_eval_acc_words(4, 6) == 0
