"""GPU: the audio renderer -- mg_render_notes against the fp64 reference of tests/render_ref.py and against itself (windows,
batches, graph replay: bit for bit), mg_pcm_peak / mg_pcm_quantise against numpy fp32, the pitch of a rendered note, the entry
points' argument checks, and the two commands end to end.  fs = 8000 and at most 40 notes throughout."""
import ctypes as C
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import _lib, audio, midi, ops  # noqa: E402
from melo_gan_amd import render as render_cmd  # noqa: E402
from melo_gan_amd.gan import generate as G  # noqa: E402

import render_ref as R  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HAPPY = os.path.join(ROOT, "tests", "golden", "ref_mid", "test_happy_1.mid")


def ref_voice():
    return ops.voice_struct(R.MULT, R.WEIGHT, R.DECAY, R.ATTACK, R.RELEASE_TAU, R.RELEASE_LEN, R.FS)


def launch(files, lengths, begins, voice=None, graph=False, want_peak=True):
    """One mg_render_notes launch of `files` (render_ref's note dicts) into a NaN-filled buffer; returns (pcm, peak) on the host."""
    voice = voice or ref_voice()
    F = len(files)
    cat = lambda k, dt: torch.from_numpy(np.concatenate([f[k] for f in files]).astype(dt)).cuda()  # noqa: E731
    onset, release, gain = cat("onset", np.int32), cat("release", np.int32), cat("gain", np.float32)
    inc = torch.from_numpy(np.concatenate([f["inc"] for f in files]).astype(np.uint32).view(np.int32)).cuda()
    if onset.numel() == 0:
        onset, release, inc, gain = (torch.zeros(1, dtype=t.dtype, device="cuda") for t in (onset, release, inc, gain))
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")  # noqa: E731
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")  # noqa: E731
    note_ptr = i64([0] + np.cumsum([len(f["onset"]) for f in files]).tolist())
    pcm_ptr = i64([0] + np.cumsum(lengths).tolist())
    max_len = i32([int((f["release"].astype(np.int64) - f["onset"]).max()) + voice.release_len if len(f["onset"]) else 0 for f in files])
    pcm = torch.full((sum(lengths),), float("nan"), device="cuda")
    peak = torch.full((F,), float("nan"), device="cuda") if want_peak else None
    n_begin = i32(list(begins))
    run = lambda: ops.render_notes(onset, release, inc, gain, note_ptr, pcm_ptr, n_begin, max_len, max(lengths), voice, pcm, peak)  # noqa: E731
    if graph:
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.Stream()):
            g = ops.Graph.capture(run)
            assert torch.isnan(pcm).all()                   # the capture ran nothing
            g.launch()
            torch.cuda.synchronize()
    else:
        run()
    torch.cuda.synchronize()
    return pcm.cpu().numpy(), None if peak is None else peak.cpu().numpy()


@pytest.fixture(scope="module")
def rendered():
    """The three files of render_ref.case_files() in one launch, with the fp64 reference of each; shared, never modified."""
    files = R.case_files()
    pcm, peak = launch(files, R.LENGTHS, [0, 0, 0])
    cuts = np.cumsum(R.LENGTHS)[:-1]
    return files, np.split(pcm, cuts), peak, [R.render(f, 0, n) for f, n in zip(files, R.LENGTHS)]


def test_kernel_against_the_fp64_reference(rendered):
    """Per sample |y - ref| <= (32 + 2 A + M) 2^-24 S (render_ref.py derives it); the planted cases of case_files() are in.
    Worst measured ratio |y - ref| / bound on the MI355X: 0.055 (the 5000-sample file, up to 50 terms), 0.040 (257 samples)."""
    files, ys, _, refs = rendered
    big = files[0]
    on, rel = big["onset"].astype(np.int64), big["release"].astype(np.int64)
    assert len(big["onset"]) + len(files[2]["onset"]) == 40 and len(files[1]["onset"]) == 0
    assert np.any(rel - on < R.ATTACK) and np.sum(on == 500) == 2 and on[0] == 0 and np.any(rel + R.RELEASE_LEN > 5000)
    assert np.sum(big["inc"] == 2 ** 31) == 1 and R.pitch_inc(96) in big["inc"].tolist() and R.pitch_inc(69) in big["inc"].tolist()
    for y, (ref, S, M, A), n in zip(ys, refs, R.LENGTHS):
        assert y.shape == (n,) and np.isfinite(y).all()                           # every element written
        assert np.all(y[S == 0] == 0)
        err, b = np.abs(y.astype(np.float64) - ref), R.bound(S, M, A)
        live = S > 0
        print(f"length {n}: worst |y - ref| / bound = {float(np.max(err[live] / b[live], initial=0.0)):.4f}, "
              f"terms <= {int(M.max())}, A <= {float(A.max()):.2f}")
        assert np.all(err <= b), (n, float(np.max(err[live] / b[live])))
    assert np.all(ys[1] == 0) and np.abs(ys[0]).max() > 0.5 and np.abs(ys[2]).max() > 0.2
    # pitch 108 alone is silent; pitch 96 sounds with its fundamental only
    solo = [R.sort_notes([(0, 200, 108, 127)]), R.sort_notes([(0, 200, 96, 127)])]
    y, peak = launch(solo, [300, 300], [0, 0])
    assert np.all(y[:300] == 0) and peak[0] == 0
    ref = R.render(solo[1], 0, 300, mult=R.MULT[:1], weight=R.WEIGHT[:1], decay=R.DECAY[:1])
    assert np.all(np.abs(y[300:] - ref[0]) <= R.bound(*ref[1:])) and peak[1] > 0.5


def test_a_sample_depends_on_its_file_and_index_alone(rendered):
    files, ys, _, _ = rendered
    big, whole = files[0], ys[0]
    wins = [(1, 1), (77, 255), (333, 1024), (901, 4097)]                          # odd offsets; 1 .. 17 tiles
    y, _ = launch([big] * 4, [m for _, m in wins], [b for b, _ in wins])
    for part, (b, m) in zip(np.split(y, np.cumsum([m for _, m in wins])[:-1]), wins):
        assert part.tobytes() == whole[b:b + m].tobytes(), (b, m)
    alone, _ = launch([big], [5000], [0])
    assert alone.tobytes() == whole.tobytes()
    moved, _ = launch([files[2], files[1], big], [257, 1, 5000], [0, 0, 0])       # another position of the batch
    assert moved[258:].tobytes() == whole.tobytes() and moved[:257].tobytes() == ys[2].tobytes()
    replay, peak = launch(files, R.LENGTHS, [0, 0, 0], graph=True)
    assert replay.tobytes() == np.concatenate(ys).tobytes() and peak.tobytes() == rendered[2].tobytes()
    no_peak, _ = launch(files, R.LENGTHS, [0, 0, 0], want_peak=False)
    assert no_peak.tobytes() == replay.tobytes()


def test_peak_and_quantise_equal_numpy_fp32(rendered):
    _, ys, rider, _ = rendered
    rng = np.random.default_rng(3)
    lengths = [5000, 1, 257, 4100, 300]
    parts = ys + [rng.standard_normal(4100).astype(np.float32) * 3, np.zeros(300, np.float32)]       # the last file is silent
    parts[3][17], parts[3][4099] = -13.5, 13.5                                    # both signs at the peak, one in the last tile
    host = np.concatenate(parts)
    pcm = torch.from_numpy(host).cuda()
    ptr = torch.tensor([0] + np.cumsum(lengths).tolist(), dtype=torch.int64, device="cuda")
    peak = torch.full((5,), float("nan"), device="cuda")
    ops.pcm_peak(pcm, ptr, 5000, peak)
    want = np.array([np.abs(p).max() for p in parts], np.float32)
    assert peak.cpu().numpy().tobytes() == want.tobytes()
    assert rider.tobytes() == want[:3].tobytes() and rider[1] == 0                 # the render launch's own peaks
    for target in (1.0, 10 ** (-1 / 20), 0.001):
        q = torch.full((len(host),), -7, dtype=torch.int16, device="cuda")
        ops.pcm_quantise(pcm, ptr, peak, 5000, target, q)
        got = np.split(q.cpu().numpy(), np.cumsum(lengths)[:-1])
        full = np.float32(target) * np.float32(32767)
        for p, g, pk in zip(parts, got, want):
            s = full / pk if pk else np.float32(0)
            ref = np.clip(np.rint(p * s), -32767, 32767).astype(np.int16)
            assert np.array_equal(g, ref), target
            assert np.abs(g.astype(np.int32)).max() <= 32767
        top = int(np.rint(full))
        assert got[3][17] == -top and got[3][4099] == top and np.abs(got[3].astype(np.int32)).max() == top
        assert np.all(got[4] == 0) and got[1][0] == 0
    # a peak below the data's (another window's, say) saturates instead of wrapping
    small = torch.full((5,), 0.5, device="cuda")
    ops.pcm_quantise(pcm, ptr, small, 5000, 1.0, q)
    g = q.cpu().numpy().astype(np.int32)
    assert g.max() == 32767 and g.min() == -32767


def test_a4_lands_in_the_440_hz_bin():
    sine = ops.voice_struct((1,), (1.0,), (0.0,), 8, 0.005, 0, R.FS)
    y, _ = launch([R.sort_notes([(0, 8000, 69, 127)])], [8000], [0], voice=sine)
    spec = np.abs(np.fft.rfft(y.astype(np.float64)))                               # 1-Hz bins
    assert int(np.argmax(spec)) == 440 and spec[440] > 100 * np.delete(spec, [439, 440, 441]).max()


def test_bad_arguments_are_refused_on_the_host():
    """Dummy non-null addresses: an entry point that got past its checks would fault, so every call must return -1."""
    lib = _lib.load()
    a = [C.c_void_p(256 * (i + 1)) for i in range(12)]

    def voice(**kw):
        f = dict(mult=(1, 2), weight=(1.0, 0.5), decay=(0.0, 1.0), attack=8, release_tau=0.02, release_len=100, fs=8000.0)
        f.update(kw)
        v = ops.voice_struct(f["mult"], f["weight"], f["decay"], f["attack"], f["release_tau"], f["release_len"], f["fs"])
        v.n_partials = kw.get("n_partials", v.n_partials)
        return v

    def render(v=None, F=2, max_samples=100, null=None, peak=True):
        ptrs = list(a[:10])
        if null is not None:
            ptrs[null] = None
        return lib.mg_render_notes(*ptrs[:8], F, max_samples, C.byref(v) if v is not None else None, ptrs[8], ptrs[9] if peak else None, None)

    for i in range(9):
        assert render(voice(), null=i) == -1 and b"null" in lib.mg_last_error(), i
    assert render(None) == -1 and b"null" in lib.mg_last_error()
    nan, inf = float("nan"), float("inf")
    for v, word in [(voice(n_partials=0), b"n_partials"), (voice(n_partials=17), b"n_partials"), (voice(attack=0), b"attack"),
                    (voice(release_len=-1), b"release_len"), (voice(fs=0.0), b"fs"), (voice(fs=-8000.0), b"fs"), (voice(fs=nan), b"fs"),
                    (voice(fs=inf), b"fs"), (voice(release_tau=0.0), b"release_tau"), (voice(release_tau=nan), b"release_tau"),
                    (voice(release_tau=inf), b"release_tau"), (voice(decay=(0.0, -1.0)), b"decay[1]"),
                    (voice(decay=(nan, 0.0)), b"decay[0]"), (voice(decay=(0.0, inf)), b"decay[1]"), (voice(weight=(1.0, nan)), b"weight[1]")]:
        assert render(v) == -1 and word in lib.mg_last_error(), (word, lib.mg_last_error())
    for F in (0, -1, 65536):
        assert render(voice(), F=F) == -1 and b"F =" in lib.mg_last_error()
        assert lib.mg_pcm_peak(a[0], a[1], F, 100, a[2], None) == -1 and b"F =" in lib.mg_last_error()
        assert lib.mg_pcm_quantise(a[0], a[1], a[2], F, 100, 0.5, a[3], None) == -1 and b"F =" in lib.mg_last_error()
    for m in (0, -5):
        assert render(voice(), max_samples=m) == -1 and b"max_samples" in lib.mg_last_error()
        assert lib.mg_pcm_peak(a[0], a[1], 2, m, a[2], None) == -1 and b"max_samples" in lib.mg_last_error()
        assert lib.mg_pcm_quantise(a[0], a[1], a[2], 2, m, 0.5, a[3], None) == -1 and b"max_samples" in lib.mg_last_error()
    assert render(voice(), max_samples=2 ** 31) == -1 and b"2^31" in lib.mg_last_error()
    for i in range(3):
        p = [a[0], a[1], a[2]]
        p[i] = None
        assert lib.mg_pcm_peak(p[0], p[1], 2, 100, p[2], None) == -1 and b"null" in lib.mg_last_error()
    for i in range(4):
        p = [a[0], a[1], a[2], a[3]]
        p[i] = None
        assert lib.mg_pcm_quantise(p[0], p[1], p[2], 2, 100, 0.5, p[3], None) == -1 and b"null" in lib.mg_last_error()
    for target in (0.0, -0.5, 1.0001, nan, inf):
        assert lib.mg_pcm_quantise(a[0], a[1], a[2], 2, 100, target, a[3], None) == -1 and b"target" in lib.mg_last_error(), target
    # the wrappers refuse host tensors and mismatched shapes before the library is asked
    z = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.render_notes(z, z, z, torch.zeros(4), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), z[:1], z[:1], 4,
                         voice(), torch.zeros(4))
    with pytest.raises(ValueError):
        ops.pcm_quantise(torch.zeros(4, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(1, device="cuda"),
                         4, 0.5, torch.zeros(3, dtype=torch.int16, device="cuda"))


def test_renderer_chunks_and_windows_agree(rendered):
    """Renderer: the same files through one chunk, through chunks of one file, and with a PCM cap so small that the long file
    goes through in windows -- identical int16 output, equal to quantising the kernel's PCM on the host."""
    lists = [[(100, 60, 0.0, 0.3), (90, 64, 0.1, 0.35), (127, 67, 0.1, 0.2)], [], [(64, 72, 0.01, 0.02)]]
    one = audio.Renderer("cuda", fs=R.FS, voice="piano", peak_db=-3.0)
    a = one.render(lists)
    rel_len = audio.VOICES["piano"].release_len(R.FS)
    assert [len(x) for x in a] == [2800 + rel_len, 0, 160 + rel_len] and all(x.dtype == np.int16 for x in a)
    assert [(r.notes, r.samples, r.truncated) for r in one.report] == [(3, len(a[0]), False), (0, 0, False), (1, len(a[2]), False)]
    top = int(np.rint(np.float32(10 ** (-3 / 20)) * np.float32(32767)))
    assert abs(int(np.abs(a[0].astype(np.int32)).max()) - top) <= 1 and abs(int(np.abs(a[2].astype(np.int32)).max()) - top) <= 1
    small = audio.Renderer("cuda", fs=R.FS, voice="piano", peak_db=-3.0, cap_bytes=4 * 1000)      # windows of 1000 samples
    b = small.render(lists)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    cut = audio.Renderer("cuda", fs=R.FS, voice="piano", peak_db=-3.0, max_seconds=0.75)
    c = cut.render(lists)
    assert [len(x) for x in c] == [6000, 0, len(a[2])] and [r.truncated for r in cut.report] == [True, False, False]
    assert cut.report[0].seconds == 0.75


def test_render_command_end_to_end(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = tmp_path / "wav"
    r = subprocess.run([sys.executable, "-m", "melo_gan_amd.render", HAPPY, "--out", str(out), "--fs", "8000"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    ev = audio.events_from_notes(render_cmd.notes_of_file(HAPPY), 8000)
    frames = int(ev.release.max()) + audio.VOICES["piano"].release_len(8000)
    with wave.open(str(out / "test_happy_1.wav"), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 8000)
        assert w.getnframes() == frames
        pcm = np.frombuffer(w.readframes(frames), "<i2").astype(np.int32)
    assert abs(int(np.abs(pcm).max()) - int(np.rint(10 ** (-1 / 20) * 32767))) <= 1
    line = r.stdout.strip().splitlines()[-1]
    assert f"{frames / 8000:.3f} s" in line and f"{len(ev)} notes" in line and "truncated" not in line


TODAY_TOP = {"checkpoint", "weights", "ed_checkpoint", "seed", "samples", "batch", "emotions", "per_emotion", "files"}
TODAY_FILE = {"file", "emotion", "k", "ed_pred", "ed_p_target"}


def test_generate_wav_end_to_end(tmp_path, capsys):
    """The closed-form generator of tests/test_generate_gpu.py (gen_state: weights x4, the last deconvolution x400 with the
    fixture's centring bias, non-trivial running statistics -- rolls that span the MIDI writer's branches) under the committed
    config; --wav renders the note list of every .mid, and without it the summary keeps exactly today's keys."""
    from oracle import melo_oracle as O
    cfg, ed_cfg = O.default_gan_cfg(8, 512, 4), O.default_ed_cfg(4)
    cfg["INTEGRATION_MODE"] = "warm_start"
    S = O.build_gan_state(cfg, ed_cfg, "closed_form")
    for k in S.PG:
        if k.endswith("weight") and S.PG[k].dim() > 1:
            S.PG[k].mul_(4.0 * (400.0 if k == "decoder.deconv.6.weight" else 1.0))
    S.PG["decoder.deconv.6.bias"].copy_(torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "gen1_c4_t512.npz"))["bias6"]))
    S.BG.update(O.fill_buffers(O.generator_buffers(), 70.0))
    ck = str(tmp_path / "gan_final.pth")
    torch.save({"G": {**S.PG, **S.BG}, "E_num": S.PE}, ck)
    base = ["--config", os.path.join(ROOT, "config", "gan_config.yaml"), "--ckpt", ck, "--emotion", "angry", "--samples", "2", "--seed", "7",
            "--batch", "8"]
    assert G.main(base + ["--out", str(tmp_path / "plain")]) == 0
    assert G.main(base + ["--out", str(tmp_path / "wav"), "--wav", "--wav-fs", "8000", "--voice", "organ"]) == 0
    capsys.readouterr()
    plain = json.load(open(tmp_path / "plain" / "summary.json"))
    assert set(plain) == TODAY_TOP and all(set(f) == TODAY_FILE for f in plain["files"])
    assert not [f for f in os.listdir(tmp_path / "plain") if f.endswith(".wav")]
    s = json.load(open(tmp_path / "wav" / "summary.json"))
    assert set(s) == TODAY_TOP | {"wav"} and s["wav"] == {"fs": 8000, "voice": "organ", "peak_db": -1.0}
    names = sorted(os.listdir(tmp_path / "wav"))
    mids = [n for n in names if n.endswith(".mid")]
    assert len(mids) == 2 and [n for n in names if n.endswith(".wav")] == [m[:-4] + ".wav" for m in mids]
    rel_len = audio.VOICES["organ"].release_len(8000)
    sounding = 0
    for f in s["files"]:
        assert set(f) == TODAY_FILE | {"wav", "seconds", "truncated"} and f["wav"] == f["file"][:-4] + ".wav" and f["truncated"] is False
        assert (tmp_path / "wav" / f["file"]).read_bytes() == (tmp_path / "plain" / f["file"]).read_bytes()
        with wave.open(str(tmp_path / "wav" / f["wav"]), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 8000)
            frames = w.getnframes()
            pcm = np.frombuffer(w.readframes(frames), "<i2").astype(np.int32)
        assert f["seconds"] == frames / 8000
        # the .mid holds the same notes, on a tick grid: its last note-off lies within a tick of the rendered release
        (_, div), tempo, notes = midi.read_smf_notes(str(tmp_path / "wav" / f["file"]))
        if notes:
            last = max(n[1] for n in notes) * tempo / (div * 1e6)
            assert abs((frames - rel_len) / 8000 - last) <= tempo / (div * 1e6) + 1 / 8000
            assert abs(int(np.abs(pcm).max()) - int(np.rint(10 ** (-1 / 20) * 32767))) <= 1
            sounding += 1
        else:
            assert frames == 0
    assert sounding == 2
