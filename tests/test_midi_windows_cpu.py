"""What the tools that read MIDI as windows share on the host (midi_rolls, emotion_discriminator.predict): the one bounds check
of a Plan, the window arguments, the plan of an argument list under the caller's error class, the classifier tools' config
check, and the host side of the encode choice.  No GPU."""
import argparse
import copy
import os

import numpy as np
import pytest

import melo_gan_amd  # noqa: F401
from melo_gan_amd import midi
from melo_gan_amd import midi_rolls as MR
from melo_gan_amd.emotion_discriminator import explain, predict
from melo_gan_amd.midi_in import MidiImportError

T = 8


class ToolError(RuntimeError):
    pass


def hand_plan() -> MR.Plan:
    """Three windows of T = 8 over 20 events in two files; the last window is short."""
    g = np.random.default_rng(1)
    ev = np.stack([g.integers(30, 100, 20), g.integers(50, 128, 20), g.integers(8, 64, 20), g.integers(0, 64, 20)], axis=1)
    files = [dict(file=f"{n}.mid", notes=k, events=k, rests=0, beats=1.0, lead_q=0, dropped_drums=0, unpaired=0, dropped_events=0,
                  tempo_us=500000, division=480) for n, k in (("a", 16), ("b", 4))]
    return MR.Plan(ev.astype(np.int32), np.array([0, 8, 16], np.int64), np.array([8, 8, 4], np.int32), np.array([0, 8, 0], np.int64),
                   np.zeros(3), np.array([0, 2, 3], np.int64), files, T)


@pytest.fixture(scope="module")
def piece(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("windows") / "piece.mid")
    ev = []
    for i in range(21):
        ev += [(110 * i, 50 + i, 90), (110 * i + 100, 50 + i, 0)]
    midi.write_smf_ticks(path, ev)
    return path


def test_check_plan_accepts_what_plan_files_makes_and_the_hand_built_plan(piece):
    p = MR.plan_files([piece, piece], T, 5, 3)
    assert p.win_start.shape[0] > 2 and p.file_off[-1] == p.win_start.shape[0]
    MR.check_plan(p)
    MR.check_plan(p, T)
    MR.check_plan(hand_plan(), T)


def broken(**change) -> MR.Plan:
    p = copy.deepcopy(hand_plan())
    for k, v in change.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("case", ["start_before", "end_past", "too_long", "off_first", "off_last", "off_falls", "no_window", "other_T"])
def test_check_plan_rejects_every_broken_plan(case):
    ok = hand_plan()
    E, W = ok.events.shape[0], ok.win_start.shape[0]
    none = dict(win_start=np.zeros(0, np.int64), win_len=np.zeros(0, np.int32), file_off=np.array([0, 0], np.int64))
    p, t = {"start_before": (broken(win_start=np.array([-1, 8, 16], np.int64)), T),
            "end_past": (broken(win_len=np.array([8, 8, E - 16 + 1], np.int32)), T),
            "too_long": (broken(win_start=np.array([0, 8, 11], np.int64), win_len=np.array([8, 8, T + 1], np.int32)), T),
            "off_first": (broken(file_off=np.array([1, 2, 3], np.int64)), T),
            "off_last": (broken(file_off=np.array([0, 2, W - 1], np.int64)), T),
            "off_falls": (broken(file_off=np.array([0, 3, 2, 3], np.int64)), T),
            "no_window": (broken(**none), T),
            "other_T": (ok, T + 1)}[case]
    if case == "too_long":
        assert int(p.win_start[2] + p.win_len[2]) <= E          # inside the event list: only its length is wrong
    with pytest.raises(ValueError):
        MR.check_plan(p, t)
    if case != "other_T":
        with pytest.raises(ValueError):
            MR.check_plan(p)


def test_host_roll_encode_and_check_plan_share_the_window_condition():
    p = hand_plan()
    assert not MR.windows_outside(p.win_start, p.win_len, 20, T)
    for ws, wl in (([-1, 8], [8, 8]), ([0, 13], [8, 8]), ([0, 8], [9, 8]), ([0, 8], [-1, 8])):
        assert MR.windows_outside(ws, wl, 20, T)
        with pytest.raises(ValueError):
            MR.host_roll_encode(p.events, np.array(ws, np.int64), np.array(wl, np.int32), T)


def test_window_arguments_and_their_defaults():
    ap = argparse.ArgumentParser()
    MR.add_window_arguments(ap, max_notes=False)
    a = ap.parse_args([])
    assert (a.hop, a.min_events, a.drums) == (None, 8, False) and not hasattr(a, "max_notes")
    assert MR.DEFAULT_MIN_EVENTS == predict.DEFAULT_MIN_EVENTS == 8
    with pytest.raises(SystemExit):
        ap.parse_args(["--max-notes", "16"])
    ap = argparse.ArgumentParser()
    MR.add_window_arguments(ap, max_notes=True)
    a = ap.parse_args([])
    assert (a.hop, a.min_events, a.drums, a.max_notes) == (None, 8, False, 512)
    a = ap.parse_args(["--max-notes", "16", "--hop", "4", "--min-events", "2", "--drums"])
    assert (a.hop, a.min_events, a.drums, a.max_notes) == (4, 2, True, 16)


def test_plan_from_args_plans_and_raises_the_callers_error(piece, tmp_path):
    args = argparse.Namespace(hop=None, min_events=3, drums=False)
    want = MR.plan_files([piece], T, T, 3)
    for search, paths in ((False, [piece]), (True, [os.path.dirname(piece)])):
        p = MR.plan_from_args(paths, T, args, ToolError, search=search)
        assert p.win_start.tolist() == want.win_start.tolist() and p.win_len.tolist() == want.win_len.tolist()
        assert (p.events == want.events).all() and p.files[0]["file"] == piece
    bad = str(tmp_path / "bad.mid")
    open(bad, "wb").write(b"MThd")
    with pytest.raises(MidiImportError) as reader:
        MR.plan_files([bad], T, T, 3)
    for paths, a, inside in (([piece + "x"], args, f"{piece}x: no such file"),
                             ([piece], argparse.Namespace(hop=0, min_events=3, drums=False), "hop = 0"),
                             ([bad], args, str(reader.value))):
        with pytest.raises(ToolError) as e:
            MR.plan_from_args(paths, T, a, ToolError)
        assert inside in str(e.value) and isinstance(e.value.__cause__, MidiImportError)
    with pytest.raises(ToolError, match="no such file or directory"):
        MR.plan_from_args([piece + "x"], T, args, ToolError, search=True)
    with pytest.raises(ToolError, match="^QUERY: .*no such file"):      # motifs' prefix
        MR.plan_from_args([piece + "x"], T, args, lambda m: ToolError(f"QUERY: {m}"))


CFG = dict(input_mode="notes", note_dim=4, n_classes=4, max_notes=32)
READS = {predict: ("predict reads note rolls; the latent classifier reads the VAE's latents, whose width is not the classifier's "
                   "note input (encode the rolls with ae.encode and evaluate those)", predict.PredictError, 1, 1 << 20),
         explain: ("explain attributes the verdict to the notes of a roll; the latent classifier never sees them",
                   explain.ExplainError, 8, explain.MAX_T)}


@pytest.mark.parametrize("tool", [predict, explain])
def test_check_notes_config_raises_the_callers_class_with_the_tools_sentence(tool):
    reads, err, lo, hi = READS[tool]
    tool.check_config(CFG)
    predict.check_notes_config(CFG, ToolError, reads, lo, hi)
    for change, inside in ((dict(input_mode="latent"), "input_mode = latent: " + reads), (dict(note_dim=5), "note_dim = 5"),
                           (dict(n_classes=1), "n_classes = 1"), (dict(n_classes=33), "n_classes = 33"),
                           (dict(max_notes=lo - 1), f"max_notes = {lo - 1}"), (dict(max_notes=hi + 1), f"max_notes = {hi + 1}")):
        with pytest.raises(err) as e:
            tool.check_config(dict(CFG, **change))
        assert inside in str(e.value), change
        with pytest.raises(ToolError) as e:
            predict.check_notes_config(dict(CFG, **change), ToolError, reads, lo, hi)
        assert inside in str(e.value), change
    for T_ok in (lo, hi):
        tool.check_config(dict(CFG, max_notes=T_ok))


def test_encode_plan_on_the_host_is_host_roll_encode(piece):
    for p in (hand_plan(), MR.plan_files([piece], T, 5, 3)):
        x, loss = MR.encode_plan(p, False)
        hx, hl = MR.host_roll_encode(p.events, p.win_start, p.win_len, p.T)
        assert x.dtype == np.float32 and x.shape == (p.win_start.shape[0], T, 4)
        assert x.tobytes() == hx.tobytes() and loss.tobytes() == hl.tobytes()


def test_write_report_leaves_no_file_behind_a_value_that_is_not_finite(tmp_path):
    out = str(tmp_path / "sub" / "rep.json")
    with pytest.raises(ToolError, match="what was wrong"):
        MR.write_report(out, {"a": float("nan")}, ToolError, "what was wrong")
    with pytest.raises(ValueError):
        MR.write_report(out, {"a": float("inf")})
    assert not os.path.exists(out)
    MR.write_report(out, {"a": [1, 2.5]})
    assert open(out).read() == '{\n "a": [\n  1,\n  2.5\n ]\n}'
