"""CPU: python -m melo_gan_amd.gan.analyze_midi -- the reference tool's per-file report on midi.read_smf_notes, against
host_stats' per-row numbers of the rolls the files were written from, on the reference's own .mid files, and on a missing
file."""
import os

import numpy as np
import pytest

import melo_gan_amd  # noqa: F401
from melo_gan_amd import midi
from melo_gan_amd.gan import analyze_midi as AM
from melo_gan_amd.gan import music_metrics as MM

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
REF_MID = os.path.join(ROOT, "tests", "golden", "ref_mid")


@pytest.mark.parametrize("T,seed", [(1, 0), (20, 1), (64, 2), (300, 3)])
def test_analyze_agrees_with_host_stats_on_written_rolls(tmp_path, capsys, T, seed):
    g = np.random.default_rng(seed)
    roll = g.uniform(-1.3, 1.3, (T, 4)).astype(np.float32)
    roll[0, 1] = 0.5                                                            # at least one note
    path = str(tmp_path / "roll.mid")
    midi.save_piano_roll_to_midi(roll, path, scale="chromatic")
    a = AM.analyze(path)
    acc, row_i, row_beats = MM.host_stats(roll[None], roll[None], np.array([0]), 1)
    ri = dict(zip(MM.ROW_I, row_i[0, 0].tolist()))
    v = MM.acc_views(acc)
    assert a["note_count"] == ri["notes"] and a["unique_pitches"] == ri["unique_pitches"]
    assert (a["lowest_pitch"], a["highest_pitch"]) == (ri["lowest_pitch"], ri["highest_pitch"])
    pitch, vel = v["pitch"][0, 0], v["velocity"][0, 0]
    assert a["mean_pitch"] == pytest.approx(float((pitch * np.arange(128)).sum()) / ri["notes"], rel=1e-12)
    assert a["mean_velocity"] == pytest.approx(float((vel * np.arange(128)).sum()) / ri["notes"], rel=1e-12)
    # the end of the last-ending note, in seconds at 120 bpm, to the file's tick (1 / 440 s)
    ev = MM.decode_rolls(roll)
    start = np.concatenate([[0.0], np.cumsum(ev["step"])[:-1]])
    end = float(((start + ev["dur"])[ev["sounding"]]).max()) * 0.5
    assert abs(a["duration"] - end) <= 0.5 / 220 + 1e-9
    assert a["density"] == pytest.approx(a["note_count"] / a["duration"], rel=1e-12)
    capsys.readouterr()
    assert AM.main([path]) == 0
    out = capsys.readouterr().out
    assert f"Note Count:   {ri['notes']}" in out and f"Pitch Range:  {ri['lowest_pitch']} - {ri['highest_pitch']}" in out
    assert "MIDI ANALYSIS REPORT" in out and "analysis for: roll.mid" in out


@pytest.mark.parametrize("name", ["test_calm_2.mid", "test_happy_1.mid", "test_sad_2.mid"])
def test_analyze_reads_the_reference_files(name, capsys):
    path = os.path.join(REF_MID, name)
    a = AM.analyze(path)
    _, tempo, notes = midi.read_smf_notes(path)
    assert a["note_count"] == len(notes) > 0 and a["file"] == name
    assert 36 <= a["lowest_pitch"] <= a["mean_pitch"] <= a["highest_pitch"] <= 96
    assert 1 <= a["unique_pitches"] <= a["highest_pitch"] - a["lowest_pitch"] + 1
    assert 0 < a["mean_velocity"] <= 127 and a["duration"] > 0
    assert a["duration"] == pytest.approx(max(n[1] for n in notes) * tempo / 1e6 / 220, rel=1e-12)
    assert AM.main([path]) == 0
    out = capsys.readouterr().out
    for label in ("Duration:", "Note Count:", "Avg Pitch:", "Pitch Range:", "Unique Notes:", "Avg Velocity:", "Density:"):
        assert label in out
    assert f"{a['density']:.2f} notes/sec" in out


def test_missing_and_unreadable_files_give_a_line_not_a_traceback(tmp_path, capsys):
    bad = tmp_path / "bad.mid"
    bad.write_bytes(b"not a midi file")
    assert AM.main([str(tmp_path / "absent.mid"), str(bad), os.path.join(REF_MID, "test_sad_2.mid")]) == 0
    out = capsys.readouterr().out
    assert f"[WARN] File not found: {tmp_path / 'absent.mid'}" in out
    assert f"[ERROR] Could not analyze {bad}" in out
    assert "analysis for: test_sad_2.mid" in out
