"""CPU: the roll encode on the host (melo_gan_amd.midi_rolls) -- the exact inverse of the generator's output contract on its
image, exhaustively; the loss counts outside it; the round trip through a written file; the window plan; the votes; the two
tools' host-side errors; midi_import without a device."""
import json
import os

import numpy as np
import pytest
import yaml

import melo_gan_amd  # noqa: F401
from melo_gan_amd import midi, midi_import, midi_in
from melo_gan_amd import midi_rolls as MR
from melo_gan_amd.emotion_discriminator import predict
from melo_gan_amd.gan.music_metrics import decode_rolls

BASE = (60, 100, 64, 64)


def one_window(ev, T=None):
    ev = np.asarray(ev, np.int32).reshape(-1, 4)
    return MR.host_roll_encode(ev, [0], [ev.shape[0]], T or ev.shape[0])


def sweep(col, values):
    ev = np.tile(np.array(BASE, np.int32), (len(values), 1))
    ev[:, col] = values
    return ev


@pytest.mark.parametrize("col,lo,hi,key,scale", [(0, 36, 96, "pitch", 1), (1, 60, 127, "vel", 1), (2, 16, 256, "dur", 64),
                                                 (3, 7, 256, "step", 64)])
def test_decode_of_encode_is_the_identity_on_the_contracts_image(col, lo, hi, key, scale):
    values = np.arange(lo, hi + 1)
    ev = sweep(col, values)
    x, loss = one_window(ev)
    assert x.dtype == np.float32 and loss.sum() == 0
    d = decode_rolls(x)
    assert d["valid"].all() and d["sounding"].all()
    assert (d[key][0] * scale == values).all()
    for other, k2, s2 in ((0, "pitch", 1), (1, "vel", 1), (2, "dur", 64), (3, "step", 64)):
        if other != col:
            assert (d[k2][0] * s2 == BASE[other]).all()
    # the scalar contract itself: notes_from_roll at 60 bpm counts seconds in beats
    notes, _ = midi.notes_from_roll(x[0], bpm=60.0, scale="chromatic")
    assert len(notes) == len(values)
    t = 0.0
    for (vel, pitch, start, end), e in zip(notes, ev.tolist()):
        assert (pitch, vel) == (e[0], e[1])
        assert start == pytest.approx(t, abs=1e-9) and end - start == pytest.approx(e[2] / 64.0, abs=1e-9)
        t += e[3] / 64.0


def test_every_pitch_velocity_pair_and_every_duration_step_pair():
    p, v = np.meshgrid(np.arange(36, 97), np.arange(60, 128), indexing="ij")
    ev = np.tile(np.array(BASE, np.int32), (p.size, 1))
    ev[:, 0], ev[:, 1] = p.ravel(), v.ravel()
    d = decode_rolls(one_window(ev)[0])
    assert (d["pitch"][0] == ev[:, 0]).all() and (d["vel"][0] == ev[:, 1]).all() and d["sounding"].all()
    du, st = np.meshgrid(np.arange(16, 257), np.arange(7, 257), indexing="ij")
    ev = np.tile(np.array(BASE, np.int32), (du.size, 1))
    ev[:, 2], ev[:, 3] = du.ravel(), st.ravel()
    d = decode_rolls(one_window(ev)[0])
    assert (d["dur"][0] * 64 == ev[:, 2]).all() and (d["step"][0] * 64 == ev[:, 3]).all()


def test_rests_and_padding():
    x, loss = one_window([(0, -1, 0, 256), (0, -1, 0, 7), BASE], T=5)
    assert x[0, :2, :3].tolist() == [[-1.0] * 3] * 2 and x[0, :2, 3].tolist() == [1.0, 7 / 128 - 1]
    assert (x[0, 3:] == -1.0).all()
    d = decode_rolls(x)
    assert d["sounding"][0].tolist() == [False, False, True, False, False]
    assert d["step"][0, :3].tolist() == [4.0, 7 / 64, 1.0]
    assert loss[0].tolist() == [0, 0, 0, 0, 0, 0, 0, 2]


def test_loss_counts_outside_each_range():
    ev = [(35, 100, 64, 64), (20, 100, 64, 64), (97, 100, 64, 64), (127, 100, 64, 64),      # 2 raised, 2 lowered
          (60, 59, 64, 64), (60, 1, 64, 64), (60, 60, 64, 64),                            # 2 velocities raised
          (60, 100, 15, 64), (60, 100, 0, 64), (60, 100, 257, 64), (60, 100, 16, 64),     # 2 lengthened, 1 shortened
          (60, 100, 64, 6), (60, 100, 64, 1), (60, 100, 64, 0), (0, -1, 0, 3), (0, -1, 0, 99)]
    x, loss = one_window(ev, T=20)
    assert dict(zip(MR.LOSS, loss[0].tolist())) == {
        "pitch_raised": 2, "pitch_lowered": 2, "velocity_raised": 2, "duration_lengthened": 2, "duration_shortened": 1,
        "steps_short": 3, "steps_zero": 1, "rests": 2}
    d = decode_rolls(x)
    assert d["pitch"][0, :4].tolist() == [36, 36, 96, 96] and d["vel"][0, 4:7].tolist() == [60, 60, 60]
    assert (d["dur"][0, 7:11] * 64).tolist() == [16, 16, 256, 16]
    assert d["step"][0, 11:15].tolist() == [0.1] * 4
    info = dict(dropped_drums=0, unpaired=0, lead_q=0, dropped_events=0)
    assert not MR.faithful(loss, info)
    clean = one_window([BASE, (0, -1, 0, 100)])[1]
    assert MR.faithful(clean, info)
    for k in info:
        assert not MR.faithful(clean, dict(info, **{k: 1})), k


def grid_roll(n, seed):
    """A roll on the quarter-beat grid inside the contract's image, built by the encode itself."""
    g = np.random.default_rng(seed)
    assert n <= 61          # distinct pitches: the reader pairs note-offs per pitch first-in-first-out, a roll's notes may nest
    ev = np.stack([g.permutation(np.arange(36, 97))[:n], g.integers(60, 128, n), 16 * g.integers(1, 17, n),
                   16 * g.integers(1, 17, n)], axis=1)
    return ev.astype(np.int32), one_window(ev)[0][0]


def test_round_trip_through_a_written_file(tmp_path, capsys):
    ev, roll = grid_roll(40, 1)
    path = os.path.join(str(tmp_path), "piece.mid")
    midi.save_piano_roll_to_midi(roll, path, bpm=120, scale="chromatic")
    capsys.readouterr()
    m = midi_in.read_midi(path)
    assert m.division == 220 and m.tempo_us == 500000 and len(m.notes) == 40
    p = MR.plan_files([path], 64, 64, 8)
    x, loss = MR.host_roll_encode(p.events, p.win_start, p.win_len, p.T)
    assert x.shape == (1, 64, 4) and MR.faithful(loss, p.files[0]) and loss.sum() == 0
    want, _ = midi.notes_from_roll(roll, bpm=120, scale="chromatic")
    got, _ = midi.notes_from_roll(x[0], bpm=120, scale="chromatic")
    assert len(got) == 40
    by_onset = lambda notes: sorted((round(s * 1e9), p_, v, round(e * 1e9)) for v, p_, s, e in notes)  # noqa: E731
    assert by_onset(got) == by_onset(want)
    # the encoded rows themselves, wherever no two notes share an onset (the reader orders those by pitch)
    assert p.files[0]["beats"] == ev[:, 3].sum() / 64 - ev[-1, 3] / 64 + ev[-1, 2] / 64


def test_plan_windows():
    P = lambda *a: tuple(v.tolist() for v in MR.plan_windows(*a))  # noqa: E731
    assert P(10, 8, 8, 1) == ([0, 8], [8, 2])
    assert P(10, 8, 8, 3) == ([0], [8])                     # the short tail is dropped
    assert P(3, 8, 8, 8) == ([0], [3])                      # unless it is the file's only window
    assert P(16, 8, 8, 8) == ([0, 8], [8, 8])               # no empty window behind an exact fit
    assert P(10, 8, 4, 1) == ([0, 4], [8, 6])               # overlapping: the window that reaches the end is the last
    assert P(20, 8, 16, 1) == ([0, 16], [8, 4])             # a hop above T skips events
    assert P(1, 1, 1, 1) == ([0], [1])
    s, n = MR.plan_windows(10, 8, 8, 1)
    assert s.dtype == np.int64 and n.dtype == np.int32
    for bad in ((0, 8, 8, 1), (8, 0, 8, 1), (8, 8, 0, 1), (8, 8, 8, 0)):
        with pytest.raises(ValueError):
            MR.plan_windows(*bad)


def test_host_roll_encode_refuses_windows_outside_the_events():
    ev = np.tile(np.array(BASE, np.int32), (5, 1))
    for ws, wl in (([3], [3]), ([-1], [2]), ([0], [9]), ([0], [-1])):
        with pytest.raises(ValueError):
            MR.host_roll_encode(ev, ws, wl, 8)
    x, loss = MR.host_roll_encode(ev, [0, 4], [5, 1], 8, rows=4)
    assert x.shape == (4, 8, 4) and (x[2:] == -1).all() and (loss[2:] == 0).all() and (x[1, 1:] == -1).all()


def test_host_window_votes_ties_nan_and_an_empty_file():
    nan = float("nan")
    z = np.array([[1.0, 1.0, 0.0, 0.0],         # a tie: the lowest index
                  [0.0, 2.0, 2.0, 1.0],
                  [0.0, nan, 5.0, nan],         # NaN counts as the maximum, the first NaN
                  [3.0, 0.0, 0.0, 0.0],
                  [0.0, 0.0, 0.0, 0.0]], np.float32)
    v = MR.host_window_votes(z, [0, 2, 2, 5])
    assert v["win_pred"].tolist() == [0, 1, 1, 0, 0] and v["win_pred"].dtype == np.int32
    np.testing.assert_allclose(v["probs"][[0, 1, 3, 4]].sum(axis=1), 1.0, rtol=0, atol=1e-15)
    e = np.exp(-1.0)
    np.testing.assert_allclose(v["probs"][0], np.array([1, 1, e, e]) / (2 + 2 * e), rtol=1e-15)
    assert np.isnan(v["probs"][2]).all()
    np.testing.assert_array_equal(v["file_mean"][0], (v["probs"][0] + v["probs"][1]) / 2.0)
    assert v["file_mean"][1].tolist() == [0.0] * 4 and v["file_pred"].tolist() == [1, -1, 0] and np.isnan(v["file_mean"][2]).all()
    assert v["switches"].tolist() == [1, 0, 1]
    with pytest.raises(ValueError):
        MR.host_window_votes(z, [0, 6])
    with pytest.raises(ValueError):
        MR.host_window_votes(z, [2, 1])


def write_piece(tmp_path, name, n, seed):
    _, roll = grid_roll(n, seed)
    path = os.path.join(str(tmp_path), name)
    midi.save_piano_roll_to_midi(roll, path, bpm=120, scale="chromatic")
    return path


def test_midi_import_host_errors_return_status_2(tmp_path, capsys):
    a = write_piece(tmp_path, "a.mid", 20, 2)
    out = os.path.join(str(tmp_path), "split")
    bad = os.path.join(str(tmp_path), "bad.mid")
    open(bad, "wb").write(b"not a midi file at all")
    csv = os.path.join(str(tmp_path), "labels.csv")
    open(csv, "w").write("file,emotion\nother.mid,happy\n")
    empty = os.path.join(str(tmp_path), "empty")
    os.makedirs(empty)
    for argv in ([os.path.join(str(tmp_path), "none.mid"), "--out", out], [bad, "--out", out], [empty, "--out", out],
                 [a, "--out", out, "--emotion", "bored"], [a, "--out", out, "--emotion", "sad", "--labels", csv],
                 [a, "--out", out, "--labels", csv], [a, "--out", out, "--labels", csv + "x"], [a, "--out", out, "--max-notes", "0"],
                 [a, "--out", out, "--hop", "0"], [a, "--out", out, "--min-events", "0"]):
        assert midi_import.main(argv + ["--cpu"]) == 2, argv
        assert capsys.readouterr().err.startswith("midi_import: error: "), argv
    assert not os.path.exists(out)


def test_predict_host_errors_return_status_2(tmp_path, capsys):
    a = write_piece(tmp_path, "a.mid", 20, 2)
    model = os.path.join(str(tmp_path), "ed.pth")
    open(model, "wb").write(b"")
    def cfg(name, **kw):  # noqa: E306
        path = os.path.join(str(tmp_path), name)
        yaml.safe_dump(dict(dict(input_mode="notes", note_dim=4, n_classes=4, max_notes=32), **kw), open(path, "w"))
        return path
    ok = cfg("ok.yaml")
    bad = os.path.join(str(tmp_path), "bad.mid")
    open(bad, "wb").write(b"MThd")
    cases = [([a, "--config", os.path.join(str(tmp_path), "none.yaml"), "--model", model], "does not exist"),
             ([a, "--config", cfg("latent.yaml", input_mode="latent"), "--model", model], "latent"),
             ([a, "--config", cfg("dim.yaml", note_dim=5), "--model", model], "note_dim"),
             ([a, "--config", cfg("k.yaml", n_classes=40), "--model", model], "n_classes"),
             ([a, "--config", ok], "--model"),
             ([a, "--config", ok, "--model", model + "x"], "does not exist"),
             ([a, "--config", ok, "--model", model, "--batch", "0"], "--batch"),
             ([a, "--config", ok, "--model", model, "--hop", "0"], "hop"),
             ([bad, "--config", ok, "--model", model], "byte 0"),
             ([a + "x", "--config", ok, "--model", model], "no such file")]
    for argv, what in cases:
        assert predict.main(argv + ["--out", os.path.join(str(tmp_path), "p.json")]) == 2, argv
        err = capsys.readouterr().err
        assert err.startswith("predict: error: ") and what in err, (argv, err)
    assert not os.path.exists(os.path.join(str(tmp_path), "p.json"))


def test_midi_import_without_a_device_writes_host_roll_encode(tmp_path, capsys):
    from melo_gan_amd.gan.generate import EMOTION_TABLE
    d = os.path.join(str(tmp_path), "in")
    os.makedirs(os.path.join(d, "sub"))
    write_piece(os.path.join(d, "sub"), "b.midi", 21, 4)
    write_piece(d, "a.mid", 40, 3)
    write_piece(d, "c.MID", 5, 5)
    open(os.path.join(d, "readme.txt"), "w").write("not music")
    csv = os.path.join(str(tmp_path), "labels.csv")
    open(csv, "w").write("a.mid,sad\nb.midi,Happy\nc.MID, calm\n")
    out = os.path.join(str(tmp_path), "split")
    capsys.readouterr()
    assert midi_import.main([d, "--out", out, "--max-notes", "16", "--hop", "12", "--min-events", "6", "--labels", csv, "--cpu"]) == 0
    files = [os.path.join(d, "a.mid"), os.path.join(d, "c.MID"), os.path.join(d, "sub", "b.midi")]
    p = MR.plan_files(files, 16, 12, 6)
    x, loss = MR.host_roll_encode(p.events, p.win_start, p.win_len, 16)
    notes = np.load(os.path.join(out, "notes.npy"))
    assert notes.dtype == np.float32 and notes.tobytes() == x.tobytes() and notes.shape == (x.shape[0], 16, 4)
    # a.mid: 40 events -> windows at 0, 12, 24 (the last reaches the end); c.MID: one short window; b.midi: 0 and 12 (9 events)
    assert p.file_off.tolist() == [0, 3, 4, 6] and p.win_len.tolist() == [16, 16, 16, 5, 16, 9]
    emo = np.load(os.path.join(out, "emotion.npy"))
    assert emo.dtype == np.int64 and emo.tolist() == [1, 1, 1, 3, 0, 0]
    num = np.load(os.path.join(out, "numeric_features.npy"))
    assert num.dtype == np.float32 and num.shape == (6, 6)
    assert (num == np.asarray(EMOTION_TABLE, np.float32)[emo]).all()
    idx = json.load(open(os.path.join(out, "index.json")))
    assert [r["file"] for r in idx["rows"]] == [files[0]] * 3 + [files[1]] + [files[2]] * 2
    assert [r["window_start"] for r in idx["rows"]] == [0, 12, 24, 0, 0, 12]
    assert idx["rows"][1]["start_beat"] == float(p.start_beat[1]) > 0
    assert [f["faithful"] for f in idx["files"]] == [True, True, True] and idx["encode"] == "host"
    assert all(sum(r["loss"].values()) == 0 for r in idx["rows"])
    # without labels: zeros and no emotion.npy; a hop above max-notes leaves events outside every window
    out2 = os.path.join(str(tmp_path), "split2")
    assert midi_import.main([files[0], "--out", out2, "--max-notes", "16", "--hop", "20", "--cpu"]) == 0
    assert not os.path.exists(os.path.join(out2, "emotion.npy"))
    assert (np.load(os.path.join(out2, "numeric_features.npy")) == 0).all()
    idx2 = json.load(open(os.path.join(out2, "index.json")))
    assert idx2["files"][0]["loss"]["dropped_events"] == 8 and idx2["files"][0]["faithful"] is False
    assert np.load(os.path.join(out2, "notes.npy")).shape == (2, 16, 4)
