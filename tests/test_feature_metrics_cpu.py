"""CPU: the host side of the feature-space metrics (melo_gan_amd.gan.feature_metrics), the evaluator's host checks of
--feature-metrics / --knn-k / --memorisation, and the argument checks of the pair kernels' C-ABI (nothing here launches)."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

import melo_gan_amd  # noqa: F401
from melo_gan_amd.gan import evaluate as EV
from melo_gan_amd.gan import feature_metrics as FM
from oracle import melo_oracle as O

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
T, C, N = 16, 4, 10


# ---------------------------------------------------------------------------------------------------------------------
# host arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def test_kid_from_sums_by_hand():
    # m = 3: 6 ordered pairs summing to 12; n = 2: 2 pairs summing to 5; 6 cross pairs summing to 9
    assert FM.kid_from_sums(12.0, 3, 5.0, 2, 9.0) == pytest.approx(12 / 6 + 5 / 2 - 2 * 9 / 6, abs=1e-15)
    # one distribution: every kernel value 2  ->  exactly 0
    assert FM.kid_from_sums(2.0 * 4 * 3, 4, 2.0 * 5 * 4, 5, 2.0 * 4 * 5) == 0.0
    for m, n in ((1, 5), (5, 1), (0, 0), (1, 1)):
        assert FM.kid_from_sums(1.0, m, 1.0, n, 1.0) is None
    assert FM.kid_from_sums(1.0, 2, 1.0, 2, 1.0) == pytest.approx(0.5 + 0.5 - 0.5)


def test_precision_recall_by_hand():
    p, r = FM.precision_recall(np.array([-1.0, 0.0, 0.5, 2.0], np.float32), np.array([-3.0, 1e-9], np.float32))
    assert p == 0.5 and r == 0.5                         # a margin of exactly 0 is inside
    assert FM.precision_recall(None, np.array([-1.0])) == (None, 1.0)
    assert FM.precision_recall(np.array([1.0]), None) == (0.0, None)
    assert FM.precision_recall(np.zeros(0), None) == (None, None)


def test_nn_summary_by_hand():
    real = np.arange(1.0, 22.0)                          # 1..21: median 11, p05 = 1 + 0.05 * 20 = 2
    fake = np.array([0.0, 0.0, 2.0, 5.0])
    s = FM.nn_summary(fake, real)
    assert s["real"] == {"median": 11.0, "p05": 2.0}
    assert s["fake"] == {"median": 1.0, "p05": 0.0}
    assert s["fake_below_real_p05"] == 0.75             # 0, 0 and 2 are at least as close as the real rows' p05
    assert FM.nn_summary(np.zeros(3), real)["fake_below_real_p05"] == 1.0
    e = FM.nn_summary(np.zeros(0), real)
    assert e["fake"] is None and e["fake_below_real_p05"] is None and e["real"]["median"] == 11.0
    assert FM.nn_summary(fake, np.zeros(0)) == {"fake": {"median": 1.0, "p05": 0.0}, "real": None, "fake_below_real_p05": None}


def hand_block(k=2):
    """Counts 3 / 2 / 0 / 1 at k = 2: a manifold for the first emotion only, KID for the first two."""
    K = 4
    counts = [3, 2, 0, 1]
    sums = {"xx": 60.0, "yy": 30.0, "xy": 36.0, "xx_e": [12.0, 4.0, 0.0, 0.0], "yy_e": [6.0, 2.0, 0.0, 0.0],
            "xy_ef": [[9.0 if e == f else 4.5 for f in range(K)] for e in range(K)]}
    margins = {"fake_in_real": np.array([-1, -1, 1, 1, -1, 1], np.float32), "real_in_fake": np.array([-1] * 6, np.float32),
               "fake_in_real_e": [np.array([-1, 0, 1], np.float32), None, None, None],
               "real_in_fake_e": [np.array([1, 1, 1], np.float32), None, None, None]}
    return FM.feature_block(256, k, EV.EMOTIONS, counts, sums, margins)


def test_feature_block_by_hand_and_json():
    b = hand_block()
    assert (b["dim"], b["k"]) == (256, 2)
    assert b["kid"] == pytest.approx(60 / 30 + 30 / 30 - 2 * 36 / 36)
    assert (b["precision"], b["recall"]) == (0.5, 1.0)
    names = list(EV.EMOTIONS)
    pe = b["per_emotion"]
    assert pe[names[0]] == {"n": 3, "kid": pytest.approx(12 / 6 + 6 / 6 - 2 * 9 / 9), "precision": pytest.approx(2 / 3), "recall": 0.0}
    assert pe[names[1]] == {"n": 2, "kid": pytest.approx(4 / 2 + 2 / 2 - 2 * 9 / 4), "precision": None, "recall": None}
    assert pe[names[2]] == {"n": 0, "kid": None, "precision": None, "recall": None}
    assert pe[names[3]] == {"n": 1, "kid": None, "precision": None, "recall": None}
    m = b["kid_matrix"]
    assert list(m) == names and all(list(m[r]) == names for r in names)
    assert m[names[0]][names[1]] == pytest.approx(12 / 6 + 2 / 2 - 2 * 4.5 / 6)
    assert m[names[1]][names[0]] == pytest.approx(4 / 2 + 6 / 6 - 2 * 4.5 / 6)
    for r in names:
        assert m[r][names[2]] is None and m[names[2]][r] is None and m[r][names[3]] is None and m[names[3]][r] is None
    b["nn_train"] = FM.nn_summary(np.zeros(0), np.zeros(0))
    assert json.loads(json.dumps(b, allow_nan=False)) == b
    # the whole sets at most k rows: no manifold at all
    small = FM.feature_block(8, 6, EV.EMOTIONS, [3, 2, 0, 1], *hand_block_inputs())
    assert small["precision"] is None and small["recall"] is None and small["kid"] is not None
    text = FM.format_block(b, b["nn_train"])
    assert "kid" in text and all(nm in text for nm in names) and "nearest training row" in text


def hand_block_inputs():
    K = 4
    sums = {"xx": 1.0, "yy": 1.0, "xy": 1.0, "xx_e": [0.0] * K, "yy_e": [0.0] * K, "xy_ef": [[0.0] * K for _ in range(K)]}
    margins = {"fake_in_real": None, "real_in_fake": None, "fake_in_real_e": [None] * K, "real_in_fake_e": [None] * K}
    return sums, margins


def test_format_table_prints_the_block_only_when_present():
    from test_evaluate_cpu import hand_made_raw
    rep = EV.build_report(hand_made_raw(), 8, 1, 4, True, True, True)
    assert "feature_space" not in rep and "feature space" not in EV.format_table(rep)
    rep["feature_space"] = hand_block()
    assert "feature space (dim 256, k 2)" in EV.format_table(rep)


# ---------------------------------------------------------------------------------------------------------------------
# plan(): every new flag is checked on the host
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("feat_cpu")
    g = np.random.default_rng(1)
    for name in ("val", "train"):
        os.makedirs(d / "splits" / name)
        np.save(d / "splits" / name / "notes.npy", g.uniform(-1, 1, (N, T, C)).astype(np.float32))
        np.save(d / "splits" / name / "emotion.npy", np.arange(N) % 4)
        np.save(d / "splits" / name / "numeric_features.npy", g.standard_normal((N, 6)).astype(np.float32))
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "gan_config.yaml")))
    cfg.update(MAX_NOTES=T, CHECKPOINT_DIR=str(d / "ck"), LOG_DIR=str(d / "logs"), SPLITS_DIR=str(d / "splits"),
               VAL_SPLIT=str(d / "splits" / "val.csv"), TRAIN_SPLIT=str(d / "splits" / "train.csv"),
               ENCODER_FEATS_VAL=str(d / "none.npy"), ENCODER_FEATS_TRAIN=str(d / "none.npy"))
    ed_cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "ed_config.yaml")))
    S = O.build_gan_state(O.default_gan_cfg(2, T, C), O.default_ed_cfg(C))
    paths = {"dir": d}
    for name, obj in (("gan.yaml", cfg), ("gan_notrain.yaml", {k: v for k, v in cfg.items() if k != "TRAIN_SPLIT"}),
                      ("gan_train_gone.yaml", dict(cfg, TRAIN_SPLIT=str(d / "splits" / "gone.csv"))), ("ed.yaml", ed_cfg),
                      ("ed_latent.yaml", dict(ed_cfg, input_mode="latent", latent_dim=int(cfg["LATENT_DIM"])))):
        paths[name] = str(d / name)
        with open(paths[name], "w") as f:
            yaml.safe_dump(obj, f)
    os.makedirs(d / "ck")
    paths["final"] = str(d / "ck" / "gan_final.pth")
    torch.save({"G": {**S.PG, **S.BG}, "E_num": S.PE}, paths["final"])
    paths["ed_ckpt"] = str(d / "ed_best.pth")
    torch.save({"model": {**S.PED, **S.BED}}, paths["ed_ckpt"])
    return paths


def ed_args(f, ed="ed.yaml"):
    return ["--config", f["gan.yaml"], "--ckpt", f["final"], "--ed_config", f[ed], "--ed_ckpt", f["ed_ckpt"]]


@pytest.mark.parametrize("case", ["knn_k_0", "knn_k_9", "knn_k_0_plain", "memorisation_no_train_split", "memorisation_split_gone",
                                  "features_latent_ed", "features_no_ed", "memorisation_no_ed"])
def test_new_flags_fail_on_the_host(files, capsys, case):
    f = files
    argv, msg = {
        "knn_k_0": (ed_args(f) + ["--feature-metrics", "--knn-k", "0"], "--knn-k 0: must be in 1..8"),
        "knn_k_9": (ed_args(f) + ["--feature-metrics", "--knn-k", "9"], "--knn-k 9: must be in 1..8"),
        "knn_k_0_plain": (ed_args(f) + ["--knn-k", "0"], "--knn-k 0: must be in 1..8"),
        "memorisation_no_train_split": (["--config", f["gan_notrain.yaml"]] + ed_args(f)[2:] + ["--memorisation"], "lacks TRAIN_SPLIT"),
        "memorisation_split_gone": (["--config", f["gan_train_gone.yaml"]] + ed_args(f)[2:] + ["--memorisation"], "does not exist"),
        "features_latent_ed": (ed_args(f, "ed_latent.yaml") + ["--feature-metrics"], "notes-mode classifier"),
        "features_no_ed": (["--config", f["gan.yaml"], "--ckpt", f["final"], "--feature-metrics"], "needs the classifier"),
        "memorisation_no_ed": (["--config", f["gan.yaml"], "--ckpt", f["final"], "--memorisation"], "needs the classifier"),
    }[case]
    with pytest.raises(EV.EvaluateError, match=msg.replace(".", r"\.")):
        EV.plan(EV.parse_args(argv))
    rc = EV.main(argv)                                   # and the CLI: a message and a non-zero exit, before any GPU use
    assert rc != 0 and msg in capsys.readouterr().err


def test_valid_flags_pass_the_host_checks(files):
    p = EV.plan(EV.parse_args(ed_args(files)))
    assert (p.features, p.knn_k, p.memorisation, p.train_arrays) == (False, 3, False, None)
    p = EV.plan(EV.parse_args(ed_args(files) + ["--feature-metrics", "--knn-k", "8"]))
    assert (p.features, p.knn_k, p.memorisation, p.train_arrays) == (True, 8, False, None)
    p = EV.plan(EV.parse_args(ed_args(files) + ["--memorisation"]))
    assert p.features and p.memorisation and p.train_arrays[0].shape == (N, T, C)
    p = EV.plan(EV.parse_args(ed_args(files) + ["--memorisation", "--synthetic", "40"]))     # the training side is synthetic too
    assert p.features and p.memorisation and p.train_arrays is None and p.arrays is None


def test_evaluator_refuses_bad_feature_options_before_building_an_engine():
    cfg, ed_cfg = O.default_gan_cfg(2, T, C), O.default_ed_cfg(C)
    with pytest.raises(EV.EvaluateError, match="notes-mode"):
        EV.Evaluator(cfg, dict(ed_cfg, input_mode="latent"), "cuda", 2, features=True)
    with pytest.raises(EV.EvaluateError, match="needs the classifier"):
        EV.Evaluator(cfg, None, "cuda", 2, features=True)
    for k in (0, 9):
        with pytest.raises(EV.EvaluateError, match="knn-k"):
            EV.Evaluator(cfg, ed_cfg, "cuda", 2, features=True, knn_k=k)


# ---------------------------------------------------------------------------------------------------------------------
# the C-ABI's argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_pair_entry_points_refuse_bad_arguments_before_any_launch():
    from melo_gan_amd import _lib, ops
    lib = _lib.load()
    a, b, big = 4096, 8192, 1 << 20       # plausible, aligned addresses: no check dereferences them and nothing launches
    calls = {
        "ksum": lambda A=a, nA=5, B=b, nB=9, D=8, ex=0, out=a, work=a, wb=big: lib.mg_pair_ksum(A, nA, B, nB, D, ex, out, work, wb, None),
        "knn": lambda A=a, nA=5, B=b, nB=9, D=8, ex=0, k=3, out=a, work=a, wb=big: lib.mg_pair_knn(A, nA, B, nB, D, ex, k, out, work, wb, None),
        "margin": lambda A=a, nA=5, B=b, nB=9, D=8, r2=a, out=a, work=a, wb=big: lib.mg_pair_margin(A, nA, B, nB, D, r2, out, work, wb, None),
    }
    for name, f in calls.items():
        for kw in ({"A": None}, {"B": None}, {"out": None}, {"work": None}, {"A": a + 4}, {"B": b + 8}, {"work": a + 4}, {"D": 6},
                   {"D": 0}, {"D": 1028}, {"nA": 0}, {"nB": 0}, {"nA": (1 << 20) + 1}):
            assert f(**kw) == -1, (name, kw)
            assert name.encode() in lib.mg_last_error()
        need = lib.mg_pair_workspace_bytes(5, 9, 8, 3 if name == "knn" else 1)
        assert need > 0 and f(wb=need - 1) == -3 and b"mg_pair_workspace_bytes" in lib.mg_last_error(), name
    assert calls["margin"](r2=None) == -1
    for k in (0, 9):
        assert calls["knn"](k=k) == -1 and b"1..8" in lib.mg_last_error()
    assert calls["knn"](nB=2, k=3) == -1 and b"candidates" in lib.mg_last_error()
    assert calls["knn"](ex=1) == -1 and b"A == B" in lib.mg_last_error()                      # exclude_self with A != B
    assert calls["knn"](B=a, ex=1) == -1                                                      # ... and with nA != nB
    assert calls["knn"](B=a, nB=3, nA=3, ex=1, k=3) == -1 and b"candidates" in lib.mg_last_error()      # k = n with the self column out
    assert calls["ksum"](ex=1) == -1 and b"A == B" in lib.mg_last_error()
    assert calls["ksum"](out=a + 4) == -1
    for bad in ((0, 9, 8, 3), (5, 0, 8, 3), (5, 9, 6, 3), (5, 9, 8, 0), (5, 9, 8, 9)):
        assert lib.mg_pair_workspace_bytes(*bad) == 0, bad
    # the list slab grows with k > 1, and the workspace holds both norm vectors
    assert lib.mg_pair_workspace_bytes(64, 64, 8, 8) > lib.mg_pair_workspace_bytes(64, 64, 8, 1) >= 4 * 128
    sc = lambda src=a, rows=8, width=12, dst=b, dst_rows=22, ctr=a, base=a: lib.mg_scatter_rows_cursor(  # noqa: E731
        src, rows, width, dst, dst_rows, ctr, base, None)
    for kw in ({"src": None}, {"dst": None}, {"ctr": None}, {"base": None}, {"src": a + 2}, {"dst": b + 1}, {"rows": 0},
               {"rows": 65536}, {"width": 0}, {"dst_rows": 0}):
        assert sc(**kw) == -1 and b"mg_scatter_rows_cursor" in lib.mg_last_error(), kw
    # the wrappers refuse host tensors and mismatched shapes before the library is asked
    x = torch.zeros(5, 8)
    with pytest.raises(ValueError):
        ops.pair_ksum(x, x, torch.zeros(1, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.scatter_rows_cursor(x, x, torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64))
