"""CPU: gan/music_metrics.py -- the vectorised decode against midi.notes_from_roll event for event, host_stats on hand-made
rows with known answers, the Jensen-Shannon divergence and the tables, and plan()'s refusal of the piano-roll configuration."""
import json

import numpy as np
import pytest
import yaml

import melo_gan_amd  # noqa: F401
from melo_gan_amd import midi
from melo_gan_amd.gan import evaluate as EV
from melo_gan_amd.gan import music_metrics as MM

f32 = np.float32
THR = f32(-0.2)


def boundary_values():
    """The planted boundaries: x1 at float32(-0.2), x0 at every integer pitch boundary and x1 at every integer velocity
    boundary, each with its two fp32 neighbours and with the values 1 and 4 ulps of 1.0 away on either side (x0 + 1 and
    x1 + 0.2 lie in [0, 2.4): a neighbour of x itself may round back to the same sum)."""
    def around(v):
        v = np.asarray(v, dtype=f32)
        d = f32(2.0 ** -23)
        return np.concatenate([v - f32(4) * d, v - d, np.nextafter(v, f32(-4)), v, np.nextafter(v, f32(4)), v + d, v + f32(4) * d])
    x1_thr = around([THR])
    x0 = around((np.arange(30, 101) / 63.5 - 1.0).astype(f32))
    x1_vel = around((np.arange(0, 131) / 67.0 * 1.2 - 0.2).astype(f32))
    return x1_thr, x0, x1_vel


def planted_roll(g):
    """One roll whose rows carry every planted boundary in turn, the other channels random in [-1.3, 1.3]."""
    x1_thr, x0, x1_vel = boundary_values()
    n = len(x1_thr) + len(x0) + len(x1_vel)
    r = g.uniform(-1.3, 1.3, (n, 4)).astype(f32)
    r[:, 1] = np.abs(r[:, 1])                                  # sounding unless planted otherwise
    r[:len(x1_thr), 1] = x1_thr
    r[len(x1_thr):len(x1_thr) + len(x0), 0] = x0
    r[len(x1_thr) + len(x0):, 1] = x1_vel
    return r


def check_against_notes_from_roll(roll):
    notes, bpm = midi.notes_from_roll(roll, 120.0, "chromatic", 0)
    ev = MM.decode_rolls(roll)
    assert ev["valid"].all()
    snd = ev["sounding"]
    # the sounding set: the yardstick's rests are the rows with x1 < float32(-0.2), as numpy compares the scalars
    assert int(snd.sum()) == len(notes)
    spb = 60.0 / bpm
    assert [n[1] for n in notes] == ev["pitch"][snd].tolist()
    assert [n[0] for n in notes] == ev["vel"][snd].tolist()
    # Times: the yardstick's beat clock turns fp32 with the first fp32 step added to it (numpy 2.x: Python float + np.float32
    # is np.float32), so a start carries at most one fp32 rounding per position before it, and end - start the one rounding
    # of t + dur (the factor 60 / 120 is exact): half an ulp of the end, bounded here by 2^-23 of it.
    start = np.concatenate([[0.0], np.cumsum(ev["step"])[:-1]])[snd] * spb
    got_start, got_end = np.array([n[2] for n in notes], dtype=np.float64), np.array([n[3] for n in notes], dtype=np.float64)
    np.testing.assert_allclose(got_start, start, rtol=len(roll) * 2.0 ** -23, atol=0)
    assert (np.abs((got_end - got_start) - ev["dur"][snd] * spb) <= 2.0 ** -23 * got_end).all()
    return len(notes)


def test_decode_matches_notes_from_roll_event_for_event():
    g = np.random.default_rng(0)
    total = check_against_notes_from_roll(planted_roll(g))
    for T in [1, 2, 3, 300] + g.integers(1, 301, 60).tolist():
        total += check_against_notes_from_roll(g.uniform(-1.3, 1.3, (T, 4)).astype(f32))
    assert total > 5000


def test_decode_boundaries_land_on_both_sides():
    """The planted values do straddle their boundaries: the check above is not vacuous."""
    x1_thr, x0, x1_vel = boundary_values()
    r = np.zeros((7, 4), dtype=f32)
    r[:, 1] = x1_thr
    assert MM.decode_rolls(r)["sounding"].tolist() == [False, False, False, True, True, True, True]
    r = np.zeros((len(x0), 4), dtype=f32)
    r[:, 0] = x0
    p = MM.decode_rolls(r)["pitch"].reshape(7, -1)
    # 4 ulps of 1.0 move (x0 + 1) * 63.5 by 3e-5, four ulps of a pitch: boundaries 37..96 separate the outer columns
    assert (np.diff(p, axis=0) >= 0).all() and (p[0] + 1 == p[6]).sum() == 60 and p.min() == 36 and p.max() == 96
    assert 0 < (p[2] < p[4]).sum()                              # and some separate the value's two fp32 neighbours
    r = np.zeros((len(x1_vel), 4), dtype=f32)
    r[:, 1] = x1_vel
    ev = MM.decode_rolls(r)
    v = np.where(ev["sounding"], ev["vel"], -1).reshape(7, -1)
    assert (np.diff(v, axis=0) >= 0).all() and (v[0] + 1 == v[6]).sum() >= 67 and v.max() == 127      # 61..127, and rest | 60
    assert 0 < (v[2] < v[4]).sum()


def test_decode_marks_non_finite_positions_invalid():
    r = np.zeros((4, 4), dtype=f32)
    r[1, 2], r[2, 0], r[3, 3] = np.nan, np.inf, -np.inf
    ev = MM.decode_rolls(r)
    assert ev["valid"].tolist() == [True, False, False, False] and ev["sounding"].tolist() == [True, False, False, False]
    with pytest.raises(ValueError):
        MM.decode_rolls(np.zeros((4, 4)))                      # fp64 rows would decode differently: refused


# ---- host_stats on hand-made rows ----
REST = (0.0, -1.0, 0.0, 0.0)


def x0_of(pitch):
    return (pitch + 0.5) / 63.5 - 1.0


def row(*positions):
    return np.array(positions, dtype=f32)


def stats_of(r, label=1, K=3):
    """host_stats of one row on the real side (the fake side is all rests); returns the real block's views and row numbers."""
    r = r[None]
    acc, row_i, row_beats = MM.host_stats(r, np.tile(row(REST), (1, r.shape[1], 1)), np.array([label]), K)
    v = MM.acc_views(acc)
    assert acc.shape == (2, K, 504) and acc.sum() == acc[:, label].sum()
    assert v["counters"][1, label].tolist() == [1, r.shape[1], 0, r.shape[1], 0, 0, 0, 0]        # the fake side: rests only
    return {k: a[0, label] for k, a in v.items()}, row_i[0, 0], row_beats[0, 0]


def test_host_stats_all_rests():
    v, ri, rb = stats_of(np.tile(row(REST), (5, 1)))
    assert v["counters"].tolist() == [1, 5, 0, 5, 0, 0, 0, 0]
    assert v["pitch"].sum() == v["velocity"].sum() == v["dur16"].sum() == v["interval"].sum() == v["pctm"].sum() == 0
    assert v["step16"].tolist() == [0] * 8 + [5] + [0] * 7                      # step = 2 beats
    assert ri.tolist() == [0, 5, 0, 0, 0, 0, 0, 0] and rb.tolist() == [10.0, 0.0]


def test_host_stats_one_note():
    # pitch 60; velocity 60 + (1.0 / 1.2) * 67 = 115; dur = 3 beats > step = 1 beat, but the note is the last position
    v, ri, rb = stats_of(row((x0_of(60), 0.8, 0.5, -0.5)))
    assert v["counters"].tolist() == [1, 1, 1, 0, 0, 0, 0, 0]
    assert v["pitch"][60] == 1 and v["pitch"].sum() == 1 and v["velocity"][115] == 1 and v["velocity"].sum() == 1
    assert v["dur16"][12] == 1 and v["step16"][4] == 1 and v["interval"].sum() == 0
    assert ri.tolist() == [1, 0, 0, 1, 60, 60, 0, 0] and rb.tolist() == [1.0, 3.0]


def test_host_stats_two_notes_with_rests_between():
    a, b = (x0_of(60), 0.8, 0.5, -0.5), (x0_of(67), 0.0, -1.0, -1.0)
    v, ri, rb = stats_of(row(a, REST, REST, b))
    assert v["counters"].tolist() == [1, 4, 2, 2, 0, 1, 1, 0]                    # the first note overlaps (3 > 1), one transition
    assert v["interval"][7] == 1 and v["interval"].sum() == 1
    assert v["pctm"][0, 7] == 1 and v["pctm"].sum() == 1
    assert v["dur16"][12] == 1 and v["dur16"][1] == 1                          # 3 beats; max(0.25, 0) = 0.25 -> bin 1
    assert v["step16"][4] == 1 and v["step16"][8] == 2 and v["step16"][0] == 1  # max(0.1, 0) = 0.1 -> bin 0
    assert ri.tolist() == [2, 2, 0, 2, 60, 67, 1, 1]
    assert rb[0] == 1.0 + 2.0 + 2.0 + 0.1 and rb[1] == 3.0 + 0.25
    assert v["velocity"][71] == 1                                              # 60 + (0.2 / 1.2) * 67 = 71.17


def test_host_stats_nan_position_between_two_notes():
    a, b = (x0_of(72), 0.8, -0.5, 0.0), (x0_of(60), 0.8, -0.5, 0.0)
    v, ri, rb = stats_of(row(a, (0.0, np.nan, 0.0, 0.0), b))
    assert v["counters"].tolist() == [1, 2, 2, 0, 1, 0, 1, 0]                    # the transition still counts; one invalid position
    assert v["interval"][12] == 1 and v["pctm"][0, 0] == 1
    assert ri.tolist() == [2, 0, 1, 2, 60, 72, 0, 1] and rb.tolist() == [4.0, 2.0]


def test_host_stats_durations_and_steps_beyond_one_land_in_bin_15():
    v, ri, rb = stats_of(row((x0_of(50), 0.0, 1.2, 1.3), (x0_of(50), 0.0, 0.875, 0.875)))
    assert v["dur16"][15] == 2 and v["step16"][15] == 2 and v["dur16"].sum() == 2      # 4.4 and 3.75 beats: both bin 15
    assert v["counters"][5] == 0                                               # dur < step at position 0
    assert ri[3] == 1 and ri[7] == 1 and v["interval"][0] == 1


def test_host_stats_padding_rows_and_classes():
    g = np.random.default_rng(3)
    real, fake = g.uniform(-1.3, 1.3, (6, 9, 4)).astype(f32), g.uniform(-1.3, 1.3, (6, 9, 4)).astype(f32)
    labels = np.array([0, -1, 2, 2, 5, 1])
    acc, ri, rb = MM.host_stats(real, fake, labels, 3)
    c = MM.acc_views(acc)["counters"]
    assert c[:, :, 0].tolist() == [[1, 1, 2], [1, 1, 2]]
    assert (ri[:, [1, 4]] == 0).all() and (rb[:, [1, 4]] == 0).all() and (ri[:, [0, 2, 3, 5], :3].sum(-1) == 9).all()
    # a row's numbers do not depend on its neighbours
    one = MM.host_stats(real[3:4], fake[3:4], labels[3:4], 3)
    assert (one[1][:, 0] == ri[:, 3]).all() and (one[2][:, 0] == rb[:, 3]).all()


# ---- the divergence and the tables ----
def test_js_divergence_values():
    assert MM.js_divergence([3, 1, 0, 4], [3, 1, 0, 4]) == 0.0
    assert MM.js_divergence([3, 1, 0, 4], [6, 2, 0, 8]) == 0.0                  # weights, not probabilities
    assert MM.js_divergence([1, 3, 0, 0], [0, 0, 2, 2]) == 1.0
    assert MM.js_divergence([0, 0, 0], [1, 2, 3]) is None and MM.js_divergence([1, 2, 3], [0, 0, 0]) is None
    a, b = [5, 1, 2, 0, 7], [1, 1, 4, 3, 0]
    assert MM.js_divergence(a, b) == MM.js_divergence(b, a) and 0.0 < MM.js_divergence(a, b) < 1.0
    # against the definition: H(m) - (H(p) + H(q)) / 2
    p, q = np.array(a) / 15.0, np.array(b) / 9.0
    H = lambda v: -sum(x * np.log2(x) for x in v if x > 0)  # noqa: E731
    assert abs(MM.js_divergence(a, b) - (H((p + q) / 2) - (H(p) + H(q)) / 2)) < 1e-14


def make_block(K=3, empty=2):
    g = np.random.default_rng(5)
    n, T = 12, 40
    real, fake = g.uniform(-1.3, 1.3, (n, T, 4)).astype(f32), g.uniform(-1.0, 0.4, (n, T, 4)).astype(f32)
    labels = np.arange(n) % K
    labels[labels == empty] = 0                                                 # class `empty` holds no rows
    acc, ri, rb = MM.host_stats(real, fake, labels, K)
    names = ["happy", "sad", "calm"][:K]
    return MM.music_block(MM.acc_views(acc), {"row_i": ri, "row_beats": rb}, labels, names), (acc, ri, rb, labels, names)


def test_music_block_numbers_and_tables():
    block, (acc, ri, rb, labels, names) = make_block()
    json.loads(json.dumps(block, allow_nan=False))
    v = MM.acc_views(acc)
    for s, side in enumerate(MM.SIDES):
        st = block[side]["happy"]
        sel = labels == 0
        assert st["rows"] == int(sel.sum()) == 8 and st["notes"] == int(ri[s][sel][:, 0].sum())
        assert st["notes_per_roll"]["mean"] == pytest.approx(ri[s][sel][:, 0].mean(), rel=1e-15)
        assert st["rest_fraction"] == st["rests"] / st["events"] and st["events"] == 8 * 40
        pitches = np.repeat(np.arange(128), v["pitch"][s, 0])
        assert st["pitch"]["mean"] == pytest.approx(pitches.mean(), rel=1e-12)
        assert st["pitch"]["std"] == pytest.approx(pitches.std(), rel=1e-9)
        assert st["notes_per_beat"] == pytest.approx(st["notes"] / rb[s][sel][:, 0].sum(), rel=1e-15)
        assert st["pitch_range_per_roll"]["mean"] == pytest.approx((ri[s][sel][:, 5] - ri[s][sel][:, 4]).mean(), rel=1e-15)
        assert sum(st["pitch_class"]) == pytest.approx(1.0, abs=1e-12) and len(st["pitch_class"]) == 12
        assert st["overlap_fraction"] == st["overlaps"] / st["notes"]
    assert block["features"] == list(MM.FEATURES) and len(MM.FEATURES) == 7
    for ft in MM.FEATURES:
        t = block["js_tables"][ft]
        assert set(t) == set(MM.TABLES)
        for name in MM.TABLES:
            assert np.array(t[name], dtype=object).shape == (3, 3)
        assert t["real_vs_real"][0][0] == 0.0 and t["generated_vs_generated"][1][1] == 0.0
        assert t["real_vs_real"][0][1] == t["real_vs_real"][1][0] and t["real_vs_real"][0][1] > 0.0
        assert t["real_vs_generated"][0][0] == block["js_real_vs_generated"]["happy"][ft]
        assert 0.0 < t["real_vs_generated"][0][1] <= 1.0
    text = MM.format_block(block)
    assert all(nm in text for nm in names) and "Jensen-Shannon" in text


def test_music_block_of_a_class_without_rows_is_all_null():
    block, _ = make_block(empty=2)
    for side in MM.SIDES:
        st = block[side]["calm"]
        assert st["rows"] == st["notes"] == st["events"] == 0
        for k in ("rest_fraction", "notes_per_beat", "overlap_fraction", "pitch_class"):
            assert st[k] is None, k
        for k in ("notes_per_roll", "pitch", "velocity", "unique_pitches_per_roll", "pitch_range_per_roll"):
            assert st[k]["mean"] is None and st[k]["std"] is None, k
    assert all(v is None for v in block["js_real_vs_generated"]["calm"].values())
    for ft in MM.FEATURES:
        for name in MM.TABLES:
            t = block["js_tables"][ft][name]
            assert all(t[2][j] is None and t[j][2] is None for j in range(3))
    assert "-" in MM.format_block(block)


# ---- the host check ----
def test_plan_refuses_music_metrics_for_the_piano_roll_config(tmp_path, capsys):
    cfg = {"NOISE_DIM": 16, "LATENT_DIM": 8, "MAX_NOTES": 16, "NOTE_DIM": 128}
    p = tmp_path / "gan.yaml"
    p.write_text(yaml.safe_dump(cfg))
    args = EV.parse_args(["--config", str(p), "--ckpt", str(tmp_path / "absent.pth"), "--synthetic", "8", "--music-metrics"])
    with pytest.raises(EV.EvaluateError, match="--music-metrics: NOTE_DIM = 128"):
        EV.plan(args)
    assert EV.main(["--config", str(p), "--ckpt", str(tmp_path / "absent.pth"), "--synthetic", "8", "--music-metrics"]) == 2
    assert "--music-metrics: NOTE_DIM = 128" in capsys.readouterr().err
    # the Evaluator refuses it as well, before it builds an engine
    with pytest.raises(EV.EvaluateError, match="--music-metrics: NOTE_DIM = 128"):
        EV.Evaluator(cfg, None, "cuda", 4, music=True)
    # NOTE_DIM 4 passes this check (and then fails on the absent checkpoint, as without the flag)
    p.write_text(yaml.safe_dump(dict(cfg, NOTE_DIM=4)))
    with pytest.raises(EV.EvaluateError, match="absent.pth"):
        EV.plan(EV.parse_args(["--config", str(p), "--ckpt", str(tmp_path / "absent.pth"), "--synthetic", "8", "--music-metrics"]))
