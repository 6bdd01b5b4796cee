"""CPU: the host side of the audio renderer (melo_gan_amd.audio, melo_gan_amd.render, generate --wav) -- events from notes,
voice and settings validation, the WAV writer, the chunk plan, the fp64 reference of tests/render_ref.py against a closed
form and against its own bound, and every bad input of the two commands refused on the host with its message."""
import math
import os
import wave

import numpy as np
import pytest

import melo_gan_amd  # noqa: F401
from melo_gan_amd import audio, midi, render
from melo_gan_amd.gan import generate as G

import render_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HAPPY = os.path.join(ROOT, "tests", "golden", "ref_mid", "test_happy_1.mid")


def test_events_increment_gain_and_rounding():
    for fs in (8000, 44100, 48000):
        ev = audio.events_from_notes([(127, 69, 0.0, 1.0)], fs)
        assert ev.inc.dtype == np.uint32 and int(ev.inc[0]) == round(440 / fs * 2 ** 32)
        assert ev.gain.dtype == np.float32 and ev.gain[0] == np.float32(1.0)
    ev = audio.events_from_notes([(64, 57, 0.0, 1.0)], 8000)
    assert int(ev.inc[0]) == round(220.0 / 8000 * 2 ** 32) and ev.gain[0] == np.float32((64 / 127) ** 2)
    # floor(t fs + 0.5): 0.49 / 0.5 / 1.5 samples -> 0 / 1 / 2 (round-half-even would give 0 / 0 / 2)
    fs = 1024                                                           # k / 1024 is exact in binary
    ev = audio.events_from_notes([(1, 60, 0.49 / fs, 10.5 / fs), (1, 60, 0.5 / fs, 11.5 / fs), (1, 60, 1.5 / fs, 12.5 / fs)], fs)
    assert ev.onset.tolist() == [0, 1, 2] and ev.release.tolist() == [11, 12, 13]
    assert ev.onset.dtype == np.int32 and ev.release.dtype == np.int32


def test_events_release_floor_and_nyquist():
    ev = audio.events_from_notes([(100, 60, 0.5, 0.5), (100, 60, 0.25, 0.1), (100, 60, 0.0, 0.00001)], 8000)
    assert ev.onset.tolist() == [0, 2000, 4000] and ev.release.tolist() == [1, 2001, 4001]       # release > onset, always
    # a fundamental at or above fs / 2 is stored as 2^31, which the kernel's Nyquist test silences; 127 at 8 kHz is above fs itself
    ev = audio.events_from_notes([(100, 108, 0, 1), (100, 127, 0, 1), (100, 107, 0, 1)], 8000)
    assert ev.inc.tolist() == [2 ** 31, 2 ** 31, round(440 * 2 ** (38 / 12) / 8000 * 2 ** 32)] and ev.inc[2] < 2 ** 31


def test_events_are_stably_sorted_by_onset():
    notes = [(10, 60, 0.5, 1.0), (20, 61, 0.1, 0.2), (30, 62, 0.5, 0.6), (40, 63, 0.1, 0.9), (50, 64, 0.0, 0.1), (60, 65, 0.5, 0.7)]
    ev = audio.events_from_notes(notes, 8000)
    assert ev.onset.tolist() == [0, 800, 800, 4000, 4000, 4000]
    gains = [np.float32((v / 127) ** 2) for v in (50, 20, 40, 10, 30, 60)]            # equal onsets keep their input order
    assert ev.gain.tolist() == gains
    assert len(audio.events_from_notes([], 8000)) == 0


@pytest.mark.parametrize("notes,msg", [
    ([(100, 60, -0.001, 1.0)], "is negative"),
    ([(100, 60, 0.0, 2 ** 31 / 8000)], "2^31"),
    ([(100, 60, 0.0, float("inf"))], "not finite"),
    ([(100, 60, float("nan"), 1.0)], "not finite"),
    ([(128, 60, 0.0, 1.0)], "outside 0..127"),
    ([(100, -1, 0.0, 1.0)], "outside 0..127"),
])
def test_events_errors(notes, msg):
    with pytest.raises(audio.AudioError, match=msg.replace("^", r"\^").replace(".", r"\.")):
        audio.events_from_notes([(100, 60, 0.0, 0.5)] + notes, 8000)
    assert len(audio.events_from_notes([(100, 60, 0.0, (2 ** 31 - 1) / 8000 - 1e-3)], 8000)) == 1     # just below the limit


def test_voices_and_release_len():
    assert set(audio.VOICES) == {"sine", "organ", "piano"}
    for name, v in audio.VOICES.items():
        assert audio.check_voice(name) is v and audio.check_voice(v) is v
        assert v.release_len(44100) == math.ceil(v.release_tau * math.log(1000) * 44100)
    sine, organ, piano = (audio.VOICES[k] for k in ("sine", "organ", "piano"))
    assert sine.mult == (1,) and sine.decay == (0.0,)
    assert len(organ.mult) >= 3 and set(organ.decay) == {0.0}
    assert len(piano.mult) == 6 and piano.attack_s == 0.005 and piano.release_tau == 0.08 and piano.attack(44100) == 221
    ratios = [piano.weight[h + 1] / piano.weight[h] for h in range(5)]
    assert max(ratios) - min(ratios) < 1e-12 and ratios[0] < 1                        # geometric weights
    assert all(piano.decay[h + 1] > piano.decay[h] for h in range(5))                 # higher partials decay faster


V = audio.Voice


@pytest.mark.parametrize("voice,msg", [
    ("harpsichord", "unknown voice"),
    (17, "expected a name"),
    (V((), (), (), 0.005, 0.05), "0 partials"),
    (V(tuple(range(1, 18)), (1.0,) * 17, (0.0,) * 17, 0.005, 0.05), "17 partials"),
    (V((1, 2), (1.0,), (0.0, 0.0), 0.005, 0.05), "1 weights"),
    (V((1, 0), (1.0, 1.0), (0.0, 0.0), 0.005, 0.05), r"mult\[1\]"),
    (V((1.5,), (1.0,), (0.0,), 0.005, 0.05), r"mult\[0\]"),
    (V((1,), (float("nan"),), (0.0,), 0.005, 0.05), r"weight\[0\]"),
    (V((1,), (1.0,), (-1.0,), 0.005, 0.05), r"decay\[0\]"),
    (V((1,), (1.0,), (float("inf"),), 0.005, 0.05), r"decay\[0\]"),
    (V((1,), (1.0,), (0.0,), -0.1, 0.05), "attack_s"),
    (V((1,), (1.0,), (0.0,), 0.005, 0.0), "release_tau"),
    (V((1,), (1.0,), (0.0,), 0.005, float("nan")), "release_tau"),
])
def test_voice_validation(voice, msg):
    with pytest.raises(audio.AudioError, match=msg):
        audio.check_voice(voice)


@pytest.mark.parametrize("kw,msg", [
    (dict(fs=999), "fs = 999"), (dict(fs=44100.0), "fs = 44100.0"), (dict(fs=10 ** 6), "fs = 1000000"),
    (dict(peak_db=0.5), "peak_db"), (dict(peak_db=float("nan")), "peak_db"), (dict(peak_db=-120.0), "below one step"),
    (dict(max_seconds=0), "max_seconds"), (dict(max_seconds=float("inf")), "max_seconds"),
    (dict(max_seconds=2 ** 31 / 44100), "2\\^31"), (dict(voice="kazoo"), "unknown voice"),
])
def test_settings_validation_needs_no_gpu(kw, msg):
    """Renderer checks its settings before it looks for a device."""
    args = dict(fs=44100, voice="piano", peak_db=-1.0, max_seconds=600)
    assert audio.check_settings(**args) is audio.VOICES["piano"]
    args.update(kw)
    with pytest.raises(audio.AudioError, match=msg):
        audio.check_settings(**args)
    with pytest.raises(audio.AudioError, match=msg):
        audio.Renderer("cuda", **args)


def test_plan_chunks_respects_both_caps():
    assert audio.plan_chunks([5, 5, 5, 5], 10) == [[0, 1], [2, 3]]
    assert audio.plan_chunks([5, 50, 5], 10) == [[0], [1], [2]]              # an over-long file stands alone
    assert audio.plan_chunks([1] * 5, 100, chunk_files=2) == [[0, 1], [2, 3], [4]]
    assert audio.plan_chunks([0, 0, 7], 10) == [[0, 1, 2]] and audio.plan_chunks([], 10) == []


def test_write_wav_reads_back(tmp_path):
    pcm = np.array([0, 1, -1, 32767, -32767, 12345, -2], np.int16)
    path = str(tmp_path / "a.wav")
    audio.write_wav(path, pcm, 8000)
    with wave.open(path, "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 8000, len(pcm))
        assert np.array_equal(np.frombuffer(w.readframes(len(pcm)), "<i2"), pcm)
    audio.write_wav(path, np.zeros(0, np.int16), 44100)                      # a file without notes: an empty, valid WAV
    with wave.open(path, "rb") as w:
        assert w.getnframes() == 0 and w.getframerate() == 44100
    for bad in (pcm.astype(np.float32), pcm.reshape(1, -1)):
        with pytest.raises(audio.AudioError):
            audio.write_wav(path, bad, 8000)


def test_reference_renders_an_undamped_sine_as_the_closed_form():
    """One note, one partial, no decay, attack 1, no release tail: y[n] = gain sin(2 pi inc k / 2^32) up to the phase's
    truncation to 24 bits (< 2 pi 2^-24 in the argument)."""
    ev = R.sort_notes([(3, 803, 69, 90)])
    y, S, M, A = R.render(ev, 0, 900, mult=(1,), weight=(1.0,), decay=(0.0,), attack=1, release_len=0)
    g, inc = float(ev["gain"][0]), int(ev["inc"][0])
    k = np.arange(800)
    closed = g * np.sin(2 * np.pi * ((inc * k) % 2 ** 32) / 2.0 ** 32)
    assert np.all(y[:3] == 0) and np.all(y[803:] == 0) and np.all(M[3:803] == 1) and np.all(M[:3] == 0) and np.all(A == 0)
    assert np.array_equal(S[3:803], np.full(800, g))
    assert np.max(np.abs(y[3:803] - closed)) <= 2 * np.pi * 2.0 ** -24 * g
    assert np.max(np.abs(y)) > 0.99 * g


def test_reference_windows_and_the_bound_on_the_test_files():
    """The reference is window-invariant; fp32 arithmetic stays far inside the bound on the GPU test's files while a dropped
    partial or a 1 % wrong release envelope leaves it by orders of magnitude; the planted cases are present."""
    files = R.case_files()
    assert [len(f["onset"]) for f in files] == [36, 0, 4] and R.RELEASE_LEN == 1106
    big = files[0]
    a4 = R.pitch_inc(69)
    assert (R.MULT[4] * a4) >= 2 ** 32 and (R.MULT[4] * a4) % 2 ** 32 < 2 ** 31          # wraps to an "audible" value
    assert R.pitch_inc(108) == 2 ** 31 and R.pitch_inc(96) < 2 ** 31 <= 2 * R.pitch_inc(96)
    assert np.all(np.diff(big["onset"]) >= 0) and np.sum(big["onset"] == 500) == 2 and big["onset"][0] == 0
    y, S, M, A = R.render(big, 0, 5000)
    yw = R.render(big, 901, 4097)[0]
    assert np.array_equal(yw, y[901:4998])
    assert S.min() >= 0 and M.max() >= 8 and 3.0 < A.max() < 8.0
    worst = 0.0
    for f, n in zip(files, R.LENGTHS):
        y, S, M, A = R.render(f, 0, n)
        err, b = np.abs(R.emulate_fp32(f, 0, n).astype(np.float64) - y), R.bound(S, M, A)
        assert np.all(err[S == 0] == 0)
        worst = max(worst, float(np.max(err[S > 0] / b[S > 0], initial=0.0)))
    assert 0 < worst < 0.25, worst
    y, S, M, A = R.render(big, 0, 5000)
    for wrong in (R.render(big, 0, 5000, skip_partial=3)[0], R.render(big, 0, 5000, release_scale=1.01)[0]):
        assert np.max(np.abs(wrong - y)[S > 0] / R.bound(S, M, A)[S > 0]) > 100


# ---------------------------------------------------------------------------------------------------------------------
# the two commands' host checks
# ---------------------------------------------------------------------------------------------------------------------
def test_notes_of_file_reads_the_reference_file_in_seconds():
    (_, div), tempo, ticks = midi.read_smf_notes(HAPPY)
    notes = render.notes_of_file(HAPPY)
    assert len(notes) == len(ticks) > 0
    on, off, pitch, vel = ticks[5]
    assert notes[5][:2] == (vel, pitch) and off > on
    assert notes[5][2:] == pytest.approx((on * tempo / (div * 1e6), off * tempo / (div * 1e6)), rel=1e-14)


@pytest.mark.parametrize("case", ["missing", "garbage", "truncated", "fs", "voice", "peak", "max_seconds", "same_stem", "out_is_file"])
def test_render_bad_inputs_fail_on_the_host(tmp_path, capsys, case):
    garbage, cut, plain = tmp_path / "g.mid", tmp_path / "cut.mid", tmp_path / "plain.txt"
    garbage.write_bytes(b"not a midi file at all")
    cut.write_bytes(open(HAPPY, "rb").read()[:200])
    plain.write_text("x")
    os.makedirs(tmp_path / "d", exist_ok=True)
    other = tmp_path / "d" / "test_happy_1.mid"
    other.write_bytes(open(HAPPY, "rb").read())
    argv, msg = {
        "missing": ([str(tmp_path / "gone.mid")], "gone.mid does not exist"),
        "garbage": ([str(garbage)], "not a MIDI file this project reads"),
        "truncated": ([HAPPY, str(cut)], "cut.mid: not a MIDI file this project reads"),
        "fs": ([HAPPY, "--fs", "100"], "fs = 100"),
        "voice": ([HAPPY, "--voice", "kazoo"], "unknown voice 'kazoo'"),
        "peak": ([HAPPY, "--peak-db", "3"], "peak_db = 3.0"),
        "max_seconds": ([HAPPY, "--max-seconds", "-1"], "max_seconds = -1.0"),
        "same_stem": ([HAPPY, str(other)], "a second input that would be written to"),
        "out_is_file": ([HAPPY, "--out", str(plain)], "is not a directory"),
    }[case]
    rc = render.main(argv)
    err = capsys.readouterr().err
    assert rc == 2 and err.startswith("render: error: ") and msg in err, (rc, err)


def test_render_plan_accepts_a_valid_request(tmp_path):
    p = render.plan(render.parse_args([HAPPY, "--out", str(tmp_path / "o"), "--fs", "8000", "--voice", "organ"]))
    assert p.wavs == [str(tmp_path / "o" / "test_happy_1.wav")] and (p.fs, p.voice, p.peak_db, p.max_seconds) == (8000, "organ", -1.0, 600.0)
    assert len(p.notes[0]) == len(midi.read_smf_notes(HAPPY)[2]) and not os.path.exists(tmp_path / "o")


def _gen_files(tmp_path):
    """A generator checkpoint and config as tests/test_generate_cpu.py builds them."""
    import torch
    import yaml
    from oracle import melo_oracle as O
    cfg = yaml.safe_load(open(os.path.join(ROOT, "config", "gan_config.yaml")))
    cfg.update(MAX_NOTES=16, CHECKPOINT_DIR=str(tmp_path), SAMPLE_DIR=str(tmp_path / "samples"))
    S = O.build_gan_state(O.default_gan_cfg(2, 16, 4), O.default_ed_cfg(4))
    (tmp_path / "gan.yaml").write_text(yaml.safe_dump(cfg))
    torch.save({"G": {**S.PG, **S.BG}, "E_num": S.PE}, str(tmp_path / "gan_final.pth"))
    return ["--config", str(tmp_path / "gan.yaml")]


def test_generate_wav_planning(tmp_path, capsys):
    base = _gen_files(tmp_path)
    assert G.plan(G.parse_args(base)).wav is None
    assert G.plan(G.parse_args(base + ["--wav-fs", "5", "--voice", "kazoo"])).wav is None       # ignored without --wav
    assert G.plan(G.parse_args(base + ["--wav"])).wav == {"fs": 44100, "voice": "piano", "peak_db": -1.0}
    assert G.plan(G.parse_args(base + ["--wav", "--wav-fs", "8000", "--voice", "sine"])).wav == {"fs": 8000, "voice": "sine", "peak_db": -1.0}
    for extra, msg in ((["--wav", "--voice", "kazoo"], "--wav: unknown voice 'kazoo'"), (["--wav", "--wav-fs", "12"], "--wav: fs = 12")):
        rc = G.main(base + extra)
        err = capsys.readouterr().err
        assert rc == 2 and err.startswith("generate: error: ") and msg in err, (rc, err)
