"""CPU: the general MIDI reader (melo_gan_amd.midi_in.read_midi) on byte strings built here -- formats 0 and 1, running status,
both note-off forms, every skipped message kind, merged tracks, tempo changes, the drum channel, unpaired note-ons and every
error -- its agreement with midi.read_smf_notes on the files this project reads already, and events_from_notes: the grid, the
steps, and the rests a step above 4 beats turns into."""
import glob
import os
import struct

import numpy as np
import pytest

import melo_gan_amd  # noqa: F401
from melo_gan_amd import midi
from melo_gan_amd import midi_in as MI

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def vlq(n):
    out = [n & 0x7F]
    n >>= 7
    while n:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    return bytes(reversed(out))


def track(*events, end=True):
    """events: (delta, bytes)."""
    body = b"".join(vlq(d) + b for d, b in events) + (vlq(0) + b"\xff\x2f\x00" if end else b"")
    return b"MTrk" + struct.pack(">I", len(body)) + body


def smf(fmt, division, *tracks):
    return b"MThd" + struct.pack(">IHHH", 6, fmt, len(tracks), division) + b"".join(tracks)


def write(tmp_path, data, name="t.mid"):
    p = os.path.join(str(tmp_path), name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def rows(m):
    return [tuple(int(v) for v in r) for r in m.notes]


def test_format_0_with_running_status_and_both_note_off_forms(tmp_path):
    data = smf(0, 96, track((0, b"\xff\x51\x03\x07\xa1\x20"),
                            (0, b"\x90\x3c\x64"),           # C4 on
                            (48, b"\x40\x50"),              # running status: E4 on
                            (48, b"\x3c\x00"),              # running status: C4 off as a note-on of velocity 0
                            (0, b"\x80\x40\x40"),           # E4 off as 0x80
                            (0, b"\x43\x40"),               # running status under 0x80: a stray G4 off, ignored
                            (0, b"\x91\x45\x7f"), (96, b"\x81\x45\x00")))
    m = MI.read_midi(write(tmp_path, data))
    assert (m.format, m.division, m.tempo_us, m.dropped_drums, m.unpaired) == (0, 96, 500000, 0, 0)
    assert rows(m) == [(0, 96, 60, 100, 0), (48, 96, 64, 80, 0), (96, 192, 69, 127, 1)]
    assert m.notes.dtype == np.int64


@pytest.mark.parametrize("skipped", [b"\xa0\x3c\x10", b"\xb0\x07\x64", b"\xe0\x00\x40", b"\xc0\x05", b"\xd0\x33",
                                     b"\xf0\x03\x7e\x7f\xf7", b"\xf7\x02\x01\x02", b"\xff\x03\x04name", b"\xff\x7f\x00",
                                     b"\xff\x01\x81\x00" + b"x" * 128])
def test_every_other_message_is_skipped_by_its_length(tmp_path, skipped):
    data = smf(0, 480, track((5, skipped), (5, b"\x90\x3c\x64"), (10, skipped), (10, b"\x90\x3c\x00")))
    assert rows(MI.read_midi(write(tmp_path, data))) == [(10, 30, 60, 100, 0)]


def test_running_status_carries_over_skipped_channel_messages_but_not_over_meta(tmp_path):
    ok = smf(0, 480, track((0, b"\xb0\x07\x64"), (0, b"\x0a\x40"), (0, b"\x90\x3c\x64"), (10, b"\x3c\x00")))
    assert rows(MI.read_midi(write(tmp_path, ok))) == [(0, 10, 60, 100, 0)]
    bad = smf(0, 480, track((0, b"\x90\x3c\x64"), (0, b"\xff\x01\x00"), (10, b"\x3c\x00")))
    with pytest.raises(MI.MidiImportError, match="running status"):
        MI.read_midi(write(tmp_path, bad))


def test_two_tracks_merge_in_onset_pitch_track_order_and_tempo_changes_leave_beats_alone(tmp_path):
    t0 = track((0, b"\xff\x51\x03\x09\x27\xc0"), (240, b"\xff\x51\x03\x03\x0d\x40"))      # 100 bpm, then 300 bpm
    t1 = track((0, b"\x90\x40\x50"), (480, b"\x80\x40\x00"), (0, b"\x90\x3c\x51"), (480, b"\x80\x3c\x00"))
    t2 = track((0, b"\x91\x3c\x52"), (480, b"\x81\x3c\x00"), (0, b"\x91\x3c\x53"), (240, b"\x81\x3c\x00"))
    m = MI.read_midi(write(tmp_path, smf(1, 480, t0, t1, t2)))
    assert (m.format, m.tempo_us) == (1, 600000)        # the first tempo
    assert rows(m) == [(0, 480, 60, 82, 1), (0, 480, 64, 80, 0), (480, 960, 60, 81, 0), (480, 720, 60, 83, 1)]
    plain = MI.read_midi(write(tmp_path, smf(1, 480, track(), t1, t2), "plain.mid"))
    assert plain.tempo_us == MI.DEFAULT_TEMPO_US and rows(plain) == rows(m)
    ev, info = MI.events_from_notes(m.notes, m.division)
    assert ev.tolist() == [[60, 82, 64, 0], [64, 80, 64, 64], [60, 81, 64, 0], [60, 83, 32, 32]] and info["lead_q"] == 0


def test_drum_channel_is_dropped_and_counted(tmp_path):
    data = smf(0, 480, track((0, b"\x99\x24\x64"), (0, b"\x90\x3c\x64"), (10, b"\x89\x24\x00"), (0, b"\x99\x26\x64"),
                            (10, b"\x80\x3c\x00"), (0, b"\x89\x26\x00")))
    m = MI.read_midi(write(tmp_path, data))
    assert rows(m) == [(0, 20, 60, 100, 0)] and m.dropped_drums == 2
    m = MI.read_midi(write(tmp_path, data), drums=True)
    assert rows(m) == [(0, 10, 36, 100, 9), (0, 20, 60, 100, 0), (10, 20, 38, 100, 9)] and m.dropped_drums == 0
    only = smf(0, 480, track((0, b"\x99\x24\x64"), (10, b"\x89\x24\x00")))
    with pytest.raises(MI.MidiImportError, match="no notes.*drum"):
        MI.read_midi(write(tmp_path, only, "only.mid"))


def test_unpaired_note_on_is_closed_at_its_tracks_end_and_fifo_pairs_repeats(tmp_path):
    data = smf(1, 480, track((0, b"\x90\x3c\x64"), (100, b"\x90\x3c\x50"), (100, b"\x80\x3c\x00"), (300, b"\xb0\x07\x64")),
               track((0, b"\x90\x43\x64"), (50, b"\x80\x43\x00")))
    m = MI.read_midi(write(tmp_path, data))
    assert rows(m) == [(0, 200, 60, 100, 0), (0, 50, 67, 100, 0), (100, 500, 60, 80, 0)] and m.unpaired == 1


def test_errors_carry_the_path_and_the_offset(tmp_path):
    good = smf(0, 480, track((0, b"\x90\x3c\x64"), (10, b"\x80\x3c\x00")))
    trk = track((0, b"\x90\x3c\x64"), (10, b"\x80\x3c\x00"))
    cases = {
        "smpte": (b"MThd" + struct.pack(">IHhH", 6, 0, 1, 0xE728) + trk, "SMPTE"),
        "tag": (b"RIFF" + good[4:], "byte 0: no MThd"),
        "chunk": (smf(0, 480, b"MTxx" + trk[4:]), "byte 14: chunk tag"),
        "short": (good[:-3], "byte 18: truncated chunk"),
        "missing": (smf(1, 480, trk)[:10] + b"\x00\x02" + smf(1, 480, trk)[12:], "track 1 of 2 is missing"),
        "event": (smf(0, 480, track((0, b"\x90\x3c\x64"), (10, b"\x80\x3c"), end=False)), "truncated event"),
        "vlq": (smf(0, 480, b"MTrk" + struct.pack(">I", 1) + b"\x81"), "truncated variable-length"),
        "vlq5": (smf(0, 480, b"MTrk" + struct.pack(">I", 6) + b"\x81\x81\x81\x81\x01\x00"), "longer than 4 bytes"),
        "delta": (smf(0, 480, b"MTrk" + struct.pack(">I", 1) + b"\x00"), "a delta time without an event"),
        "data": (smf(0, 480, track((0, b"\x3c\x64"))), "data byte without a running status"),
        "meta": (smf(0, 480, b"MTrk" + struct.pack(">I", 4) + b"\x00\xff\x01\x09"), "truncated meta"),
        "sysex": (smf(0, 480, b"MTrk" + struct.pack(">I", 3) + b"\x00\xf0\x05"), "truncated sysex"),
        "nonotes": (smf(0, 480, track((0, b"\xc0\x05"))), "no notes"),
        "format2": (smf(2, 480, trk), "format 2"),
        "realtime": (smf(0, 480, track((0, b"\xf8"))), "status byte 0xf8"),
    }
    for name, (data, what) in cases.items():
        path = write(tmp_path, data, name + ".mid")
        with pytest.raises(MI.MidiImportError, match=what) as e:
            MI.read_midi(path)
        assert str(e.value).startswith(path + ": byte "), (name, str(e.value))


def sorted_notes(m):
    return sorted((int(a), int(b), int(p), int(v)) for a, b, p, v, _ in m.notes)


def test_agrees_with_read_smf_notes_on_the_reference_files_and_on_a_written_one(tmp_path):
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ref_mid", "*.mid")))
    assert len(paths) == 3
    own = os.path.join(str(tmp_path), "own.mid")
    midi.write_smf(own, [(100, 60, 0.0, 0.5), (64, 72, 0.25, 1.0), (90, 60, 0.5, 0.75), (127, 96, 2.0, 6.5)], 97.0, 4)
    for p in paths + [own]:
        (fmt, div), tempo, notes = midi.read_smf_notes(p)
        m = MI.read_midi(p)
        assert (m.format, m.division, m.tempo_us) == (fmt, div, tempo), p
        assert sorted_notes(m) == sorted(notes), p
        assert (m.dropped_drums, m.unpaired) == (0, 0)
        on = m.notes[:, 0]
        assert (np.diff(on) >= 0).all()


def chain(gaps, division=64, dur=16):
    """Notes whose onsets are `gaps` grid units apart (division 64: a tick is a grid unit), each `dur` long."""
    t, out = 0, []
    for i, g in enumerate(list(gaps) + [0]):
        out.append((t, t + dur, 60 + i, 100, 0))
        t += g
    return np.array(out, np.int64)


def test_steps_and_the_rests_of_long_gaps():
    gaps = [0, 6, 7, 256, 257, 262, 263, 600, 513]
    ev, info = MI.events_from_notes(chain(gaps), 64)
    R = lambda s: [0, -1, 0, s]  # noqa: E731
    N = lambda i, s: [60 + i, 100, 16, s]  # noqa: E731
    assert ev.tolist() == [N(0, 0), N(1, 6), N(2, 7), N(3, 256), N(4, 250), R(7), N(5, 255), R(7), N(6, 256), R(7),
                           N(7, 256), R(256), R(88), N(8, 256), R(250), R(7), N(9, 16)]
    assert ev.dtype == np.int32 and info["notes"] == 10 and info["rests"] == 7 and info["events"] == 17
    assert info["length_q"] == sum(gaps) + 16 and info["lead_q"] == 0
    # every event's onset; the notes' onsets are the quantised ones: no gap here lies in 1..6 but the one of 6
    onsets = info["onset_q"][ev[:, 1] >= 0]
    assert onsets.tolist() == np.concatenate([[0], np.cumsum(gaps)]).tolist()
    # what the contract's decode makes of the steps: max(0.1 beat, s / 64)
    decoded = np.where(ev[:, 3] >= 7, ev[:, 3] / 64.0, 0.1)
    want = np.concatenate([[0], np.cumsum(gaps)]) / 64.0
    got = np.concatenate([[0], np.cumsum(decoded)])[:-1][ev[:, 1] >= 0]
    far = np.arange(len(gaps) + 1) >= 3         # behind the gaps of 0 and 6, which decode as 0.1 beat each
    np.testing.assert_allclose(got[far] - got[3], want[far] - want[3], rtol=0, atol=1e-12)
    assert all(0 < s <= 256 for s in ev[ev[:, 1] < 0, 3])


def test_lead_is_dropped_and_reported_and_the_last_step_is_the_duration():
    ev, info = MI.events_from_notes(np.array([(128, 160, 60, 90, 0), (192, 1000, 62, 91, 0)]), 64)
    assert ev.tolist() == [[60, 90, 32, 64], [62, 91, 808, 256], [0, -1, 0, 256], [0, -1, 0, 256], [0, -1, 0, 40]]
    assert info["lead_q"] == 128 and info["length_q"] == 64 + 808
    with pytest.raises(ValueError):
        MI.events_from_notes(np.array([(10, 20, 60, 90, 0), (5, 20, 60, 90, 0)]), 64)


def test_grid_rounding_at_division_220_and_half_to_even():
    # 55 ticks of 220 are a quarter beat, 16 grid units, exactly; the grid unit is 3.4375 ticks
    assert MI.quantise([0, 55, 110, 220, 1, 2, 5, 6, 27, 28, 219], 220).tolist() == [0, 16, 32, 64, 0, 1, 1, 2, 8, 8, 64]
    # t * 64 / 220 is never k + 1/2 (55 (2k + 1) / 32 is no integer): halves need another division
    assert not any((t * 128) % 220 == 110 for t in range(220))
    assert MI.quantise([2, 6, 10, 14, 1, 3], 256).tolist() == [0, 2, 2, 4, 0, 1]       # 0.5, 1.5, 2.5, 3.5 to even; 0.25, 0.75
    assert MI.quantise([15, 45, 75], 1920).tolist() == [0, 2, 2]                      # 0.5, 1.5, 2.5
    ev, _ = MI.events_from_notes(np.array([(0, 55, 60, 90, 0), (55, 165, 62, 91, 0), (220, 275, 64, 92, 0)]), 220)
    assert ev.tolist() == [[60, 90, 16, 16], [62, 91, 32, 48], [64, 92, 16, 16]]
