"""CPU: emotion_discriminator.explain's host side -- host_explain on the fp64 oracle (the midpoint rule's convergence, exact
zeros for the silent tail), the host restatements of the ranking and of the deletion rows, and the tool's checks, which all
answer before any GPU use."""
import os

import numpy as np
import pytest
import torch
import yaml

import melo_gan_amd  # noqa: F401
from melo_gan_amd.emotion_discriminator import explain as E
from oracle import melo_oracle as O
from test_ed_evaluate_gpu import random_model

T, K = 32, 4
CFG = {**O.default_ed_cfg(4), **dict(max_notes=T, batch_size=8, seed=3, dropout=0.2)}


def rolls():
    """Five rolls, uniform in (-1, 1); roll 2 is silent from note 20 on."""
    x = (torch.rand(5, T, 4, generator=torch.Generator().manual_seed(31)) * 2 - 1).numpy().astype(np.float32)
    x[2, 20:] = -1.0
    return x, np.array([T, T, 20, T, T], np.int32)


@pytest.fixture(scope="module")
def oracle64():
    P, Bf = random_model(CFG)
    P = {k: v.double() for k, v in P.items()}
    Bf = {k: v.double() for k, v in Bf.items()}
    return lambda x: O.emotion_disc_fwd(P, Bf, x, CFG, train=False)


@pytest.fixture(scope="module")
def explained(oracle64):
    x, wl = rolls()
    return x, wl, {S: E.host_explain(oracle64, x, wl, S) for S in (32, 64)}


def test_the_residual_falls_by_the_midpoint_rules_order(explained):
    """Second order: doubling S divides the residual by 4; half of that ratio is the margin.  Measured with this model and
    these rolls: max |residual| 1.270e-3 at S = 32 and 3.182e-4 at S = 64; relative to |F(x) - F(b)| at most 4.07e-3 at 32."""
    _, _, res = explained
    r32, r64 = np.abs(res[32]["residual"]).max(), np.abs(res[64]["residual"]).max()
    delta = np.abs(res[32]["log_p"] - res[32]["log_p_silence"])
    rel = (np.abs(res[32]["residual"]) / delta).max()
    print(f"max |residual|: S=32 {r32:.3e}, S=64 {r64:.3e}; relative at 32 {rel:.3e}; |F(x) - F(b)| {delta}")
    assert r32 > 0 and r64 <= 0.5 * r32
    assert rel < 1e-2
    for S in (32, 64):
        assert (res[S]["target"] == np.argmax(res[S]["logits"], axis=1)).all()
        assert np.abs(res[S]["total"] - res[S]["attr"].sum(axis=(1, 2))).max() <= 1e-12 * np.abs(res[S]["attr"]).sum(axis=(1, 2)).max()


def test_the_silent_tail_gets_exact_zeros_and_rank_minus_one(explained):
    x, wl, res = explained
    r = res[32]
    assert (r["attr"][2, 20:] == 0.0).all() and (r["note"][2, 20:] == 0.0).all()
    assert np.abs(r["attr"][2, :20]).min() > 0
    assert (r["rank"][2, 20:] == -1).all() and sorted(r["rank"][2, :20].tolist()) == list(range(20))
    for w in (0, 1, 3, 4):
        assert sorted(r["rank"][w].tolist()) == list(range(T))
        order = np.argsort(r["rank"][w])
        assert (np.diff(r["note"][w][order]) <= 0).all()            # descending


def test_host_ig_rank_breaks_ties_to_the_lower_event_and_handles_padding_and_nan():
    note = np.array([[0.5, -1.0, 0.5, 2.0, 0.0, -0.0, 9.0, 9.0],
                     [1.0, np.nan, 3.0, 2.0, 0.0, 0.0, 0.0, 0.0],
                     [1.0, 2.0, 3.0, np.nan, 0.0, 0.0, 0.0, 0.0],
                     [1.0, 2.0, 3.0, 4.0, 0.0, 0.0, 0.0, 0.0]])
    rank = E.host_ig_rank(note, np.array([6, 4, 3, 9], np.int32))
    assert rank[0].tolist() == [1, 5, 2, 0, 3, 4, -1, -1]             # 0.5 twice and 0.0 / -0.0: the lower event first
    assert (rank[1] == -1).all()                                      # a NaN among the real events
    assert rank[2].tolist() == [2, 1, 0, -1, -1, -1, -1, -1]          # a NaN in the padding does not count
    assert (rank[3] == -1).all()                                      # a length outside [0, T]


def test_deletion_rows_run_from_the_window_itself_to_the_silent_roll(explained):
    x, wl, res = explained
    rank = res[32]["rank"]
    n_del = np.array([0, 3, 20, T], np.int32)
    D = len(n_del)
    for w in range(5):
        rows = E.host_ig_rows(x, 2 * D, 2 * D, w, E.DELETE, wl, rank, n_del)       # G = 1: the cursor is the window
        n = int(wl[w])
        for half in (0, D):
            assert rows[half + 0].tobytes() == x[w].tobytes()                        # n = 0 gives x
            assert (rows[half + 3] == -1.0).all()                                    # n = T >= win_len gives the silent roll
            if n == 20:
                assert (rows[half + 2] == -1.0).all()                                # n = win_len too
        gone = np.nonzero((rows[1] != x[w]).any(axis=1))[0]
        assert sorted(rank[w][gone].tolist()) == [0, 1, 2]                           # the three strongest supporters
        gone = np.nonzero((rows[D + 1] != x[w]).any(axis=1))[0]
        assert sorted(rank[w][gone].tolist()) == [n - 3, n - 2, n - 1]               # the three strongest opponents
    past = E.host_ig_rows(x, 2 * D, 2 * D, 5, E.DELETE, wl, rank, n_del)
    assert (past == -1.0).all()                                                      # a cursor past the last window


def test_path_rows_are_the_midpoints_and_keep_the_baseline_bit_for_bit():
    x, wl = rolls()
    rows = E.host_ig_rows(x, 8, 3, 1)                   # G = 2: windows 2 and 3, two padding rows
    assert (rows[6:] == -1.0).all() and (rows[:3, 20:] == -1.0).all()
    for j in range(3):
        want = -1.0 + (j + 0.5) / 3.0 * (x[3].astype(np.float64) + 1.0)
        assert np.abs(rows[3 + j] - want).max() <= 2.0 ** -24
    assert (E.host_ig_rows(x, 8, 3, 2)[3:] == -1.0).all() and (E.host_ig_rows(x, 8, 3, 3) == -1.0).all()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("explain_cpu")
    paths = {"dir": str(d)}
    for name, cfg in (("ed.yaml", CFG), ("ed_latent.yaml", dict(CFG, input_mode="latent", latent_dim=8))):
        paths[name] = str(d / name)
        with open(paths[name], "w") as f:
            yaml.safe_dump(cfg, f)
    P, Bf = random_model(CFG)
    paths["model"] = str(d / "ed_best.pth")
    torch.save({"model": {**P, **Bf}}, paths["model"])
    paths["notes"] = str(d / "notes.npy")
    np.save(paths["notes"], rolls()[0])
    paths["mid"] = str(d / "piece.mid")
    from melo_gan_amd import midi
    midi.write_smf_ticks(paths["mid"], [(0, 60, 90), (110, 60, 0), (220, 64, 90), (330, 64, 0)])
    return paths


@pytest.mark.parametrize("case", ["steps", "latent", "model_missing", "target", "rows", "both", "neither", "rows_alone", "shape"])
def test_bad_inputs_are_status_2_before_any_gpu_use(files, capsys, case):
    f = files
    out, save = os.path.join(f["dir"], f"{case}.json"), os.path.join(f["dir"], f"{case}.npy")
    src = ["--notes", f["notes"]]
    ok = ["--config", f["ed.yaml"], "--model", f["model"]]
    argv, msg = {
        "steps": (src + ok + ["--steps", "9", "--batch", "8"], "--steps = 9"),
        "latent": (src + ["--config", f["ed_latent.yaml"], "--model", f["model"]], "input_mode = latent"),
        "model_missing": (src + ["--config", f["ed.yaml"], "--model", f["model"] + ".gone"], "does not exist"),
        "target": (src + ok + ["--target", "joyful"], "--target joyful"),
        "rows": (src + ok + ["--rows", "0,5"], "--rows 0,5"),
        "both": ([f["mid"]] + src + ok, "not both"),
        "neither": (ok, "either MIDI files or --notes"),
        "rows_alone": ([f["mid"]] + ok + ["--rows", "0"], "--rows selects rows of --notes"),
        "shape": (["--notes", f["model"]] + ok, "not a .npy array"),
    }[case]
    rc = E.main(argv + ["--out", out, "--save", save])
    err = capsys.readouterr().err
    assert rc == 2 and err.startswith("explain: error: ") and msg in err, (rc, err)
    assert not os.path.exists(out) and not os.path.exists(save)
