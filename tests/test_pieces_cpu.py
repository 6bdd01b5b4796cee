"""CPU: what generate, morph, ae.edit and render share (melo_gan_amd.pieces) -- the writer's .mid files against the direct midi
calls, the --wav plan step, the names the sampler modules still hand on, and the error line and status of the four main()s."""
import argparse
import os
import types

import numpy as np
import pytest

import melo_gan_amd  # noqa: F401
from melo_gan_amd import midi, pieces, render
from melo_gan_amd.ae import edit as ED
from melo_gan_amd.gan import generate as G
from melo_gan_amd.gan import morph as M

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
READY = [(100, 60, 0.0, 0.5), (80, 64, 0.5, 1.25), (90, 67, 1.0, 2.0)]
STYLES = (("major", 140), ("minor", 70))


def three_pieces():
    """Two rolls of shape (16, 4) with different (scale, bpm) and one ready note list; each entry has keys of its own."""
    rng = np.random.default_rng(11)
    rolls = [rng.uniform(-1.0, 1.0, (16, 4)).astype(np.float32) for _ in STYLES]
    return [({"file": "a_1.mid", "emotion": "happy", "k": 1}, (rolls[0],) + STYLES[0]),
            ({"file": "b_s00.mid", "k": 2, "bpm": 70, "scale": "minor"}, (rolls[1],) + STYLES[1]),
            ({"file": "joined.mid", "joined": True, "join_notes": 3}, list(READY))]


def note_lists(todo):
    """The note list of every piece, as the direct midi call gives it."""
    return [p if isinstance(p, list) else midi.notes_from_roll(p[0], bpm=p[2], scale=p[1], root_key=0)[0] for _, p in todo]


def test_write_pieces_writes_what_the_direct_calls_write(tmp_path):
    todo = three_pieces()
    keys = [list(f) for f, _ in todo]
    out, ref = tmp_path / "deep" / "out", tmp_path / "ref"
    os.makedirs(ref)
    files = pieces.write_pieces(str(out), todo, None)                   # creates the missing directory
    for (f, payload), got, k in zip(todo, files, keys):
        assert got is f and list(got) == k and "wav" not in got         # the caller's entries, in order, untouched
        if isinstance(payload, list):
            midi.write_smf(str(ref / f["file"]), payload, 120.0, 0)
        else:
            roll, scale, bpm = payload
            midi.save_piano_roll_to_midi(roll, str(ref / f["file"]), bpm=bpm, scale=scale, root_key=0,
                                         instrument_name="Acoustic Grand Piano")
        assert (out / f["file"]).read_bytes() == (ref / f["file"]).read_bytes()
    assert sorted(os.listdir(out)) == sorted(f["file"] for f, _ in todo)
    assert all(len(n) > 0 for n in note_lists(todo))                    # no piece is silent: the files differ from an empty one


class PlanError(ValueError):
    pass


def wav_args(*argv):
    ap = argparse.ArgumentParser()
    pieces.add_wav_arguments(ap, help_wav="render")
    return ap.parse_args(list(argv))


def test_plan_wav():
    assert pieces.plan_wav(wav_args(), PlanError) is None
    assert pieces.plan_wav(wav_args("--wav-fs", "5", "--voice", "kazoo"), PlanError) is None           # ignored without --wav
    assert pieces.plan_wav(types.SimpleNamespace(), PlanError) is None                                  # a hand-made namespace
    assert pieces.plan_wav(wav_args("--wav"), PlanError) == {"fs": 44100, "voice": "piano", "peak_db": pieces.WAV_PEAK_DB}
    assert pieces.plan_wav(wav_args("--wav", "--wav-fs", "8000", "--voice", "sine"), PlanError, files=True, join=True) == \
        {"fs": 8000, "voice": "sine", "peak_db": pieces.WAV_PEAK_DB}
    for argv, msg in ((("--wav", "--voice", "kazoo"), "--wav: unknown voice 'kazoo'"), (("--wav", "--wav-fs", "12"), "--wav: fs = 12")):
        with pytest.raises(PlanError) as e:
            pieces.plan_wav(wav_args(*argv), PlanError)
        assert str(e.value).startswith(msg), e.value
    for argv, join in ((("--wav",), False), ((), True)):
        with pytest.raises(PlanError) as e:
            pieces.plan_wav(wav_args(*argv), PlanError, files=False, join=join, report="morph.json")
        assert str(e.value) == "--no-files writes morph.json only: it cannot go with --join or --wav"
    assert pieces.plan_wav(wav_args(), PlanError, files=False, join=False, report="edit.json") is None  # --no-files alone


def test_the_sampler_modules_hand_on_the_moved_names():
    assert M.joined_notes is pieces.joined_notes
    assert G.EMOTIONS is pieces.EMOTIONS and G.STYLE is pieces.STYLE
    assert M.EMOTIONS is pieces.EMOTIONS and ED.EMOTIONS is pieces.EMOTIONS and ED.STYLE is pieces.STYLE


def test_require_device_raises_the_class_it_is_given(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for err in (RuntimeError, PlanError):
        with pytest.raises(err, match="no CPU path: a MI355X"):
            pieces.require_device(*(() if err is RuntimeError else (err,)))


def test_run_tool_status_and_error_line(capsys):
    ran = []

    def bad(_):
        raise PlanError("no good")

    assert pieces.run_tool("tool", PlanError, lambda a: a + 1, ran.append, 1) == 0 and ran == [2]
    assert pieces.run_tool("tool", PlanError, bad, ran.append, 1) == 2 and ran == [2]
    assert capsys.readouterr().err == "tool: error: no good\n"
    with pytest.raises(PlanError):                                      # run's errors are the caller's ...
        pieces.run_tool("tool", PlanError, lambda a: a, bad, 1)
    assert pieces.run_tool("tool", PlanError, lambda a: a, bad, 1, catch_run=True) == 2                 # ... unless it asks
    assert capsys.readouterr().err == "tool: error: no good\n"


@pytest.mark.parametrize("tool", ["generate", "morph", "ae.edit", "render"])
def test_each_main_returns_2_with_its_error_line(tool, tmp_path, capsys):
    gan = ["--config", os.path.join(ROOT, "config", "gan_config.yaml")]
    main, argv, word = {
        "generate": (G.main, gan + ["--emotion", "joyful"], "unknown emotion 'joyful'"),
        "morph": (M.main, gan + ["--from", "happy", "--to", "happy"], "two emotions"),
        "ae.edit": (ED.main, ["--config", os.path.join(ROOT, "config", "ae_config.yaml"), "--synthetic", "12"], "exactly one of"),
        "render": (render.main, [str(tmp_path / "gone.mid")], "gone.mid does not exist"),
    }[tool]
    assert main(argv) == 2
    err = capsys.readouterr().err
    assert err.startswith(f"{tool}: error: ") and err.count("\n") == 1 and word in err, err
