"""Note lists -> 16-bit mono PCM on the device, with no synthesiser from outside: what lets one LISTEN to test_sad_2.mid.

An additive synthesiser with an integer phase accumulator (csrc/render.hip: mg_render_notes; include/melo_gan_hip.h states the
formula).  A note (velocity, pitch, start, end) becomes an event -- onset and release in samples, the fundamental's phase
increment in units of 2^-32 turns, a gain -- and a voice says which partials sound, how fast each decays, how long the attack
ramp and the release tail are.  A sample depends on its file's events and its own index only, so files are rendered in
chunks (and a file longer than the PCM cap in windows) without the result depending on the cut.

    Renderer("cuda", fs=44100, voice="piano").render([notes_a, notes_b]) -> [int16 array, int16 array]
    write_wav("a.wav", pcm, 44100)

Host code validates everything that comes from outside (AudioError) before the device is touched.
"""
from __future__ import annotations

import math
import wave
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

MAX_PARTIALS = 16
PCM_CAP_BYTES = 256 << 20           # the float PCM buffer of one chunk stays below this
CHUNK_FILES = 64                    # and a chunk holds at most this many files
MIN_FS, MAX_FS = 1000, 768000


class AudioError(ValueError):
    """A bad input of the renderer, found on the host before any GPU use."""


@dataclass(frozen=True)
class Voice:
    """Partial h sounds at mult[h] times the fundamental with weight[h] and decays at decay[h] 1/s from the onset; the note
    ramps up linearly over attack_s seconds and dies away with time constant release_tau (s) after its release."""
    mult: Tuple[int, ...]
    weight: Tuple[float, ...]
    decay: Tuple[float, ...]
    attack_s: float
    release_tau: float

    def attack(self, fs: float) -> int:
        return max(1, int(math.floor(self.attack_s * fs + 0.5)))

    def release_len(self, fs: float) -> int:
        """Samples until the release envelope has fallen to 1/1000 (-60 dB)."""
        return int(math.ceil(self.release_tau * math.log(1000.0) * fs))


VOICES: Dict[str, Voice] = {
    "sine": Voice((1,), (1.0,), (0.0,), 0.005, 0.03),
    "organ": Voice((1, 2, 3, 4, 6, 8), (1.0, 0.6, 0.35, 0.25, 0.12, 0.08), (0.0,) * 6, 0.01, 0.05),
    # six harmonics, weights 0.55^h; partial h decays at 1.2 (h + 1) 1/s: the upper ones fade first, as a struck string's do
    "piano": Voice(tuple(range(1, 7)), tuple(0.55 ** h for h in range(6)), tuple(1.2 * (h + 1) for h in range(6)), 0.005, 0.08),
}


def check_voice(voice: Union[str, Voice]) -> Voice:
    """A name in VOICES or a Voice whose table the kernel accepts; raises AudioError."""
    if isinstance(voice, str):
        if voice not in VOICES:
            raise AudioError(f"unknown voice {voice!r}: expected one of {', '.join(VOICES)}")
        return VOICES[voice]
    if not isinstance(voice, Voice):
        raise AudioError(f"voice: expected a name or an audio.Voice, got {type(voice).__name__}")
    n = len(voice.mult)
    if not 1 <= n <= MAX_PARTIALS:
        raise AudioError(f"voice: {n} partials, expected 1..{MAX_PARTIALS}")
    if len(voice.weight) != n or len(voice.decay) != n:
        raise AudioError(f"voice: {n} multipliers, {len(voice.weight)} weights, {len(voice.decay)} decay rates")
    for h in range(n):
        m = voice.mult[h]
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= int(m) < 2 ** 32:
            raise AudioError(f"voice: mult[{h}] = {m!r}: an integer in 1..2^32-1")
        if not math.isfinite(voice.weight[h]):
            raise AudioError(f"voice: weight[{h}] = {voice.weight[h]!r} is not finite")
        if not (math.isfinite(voice.decay[h]) and voice.decay[h] >= 0):
            raise AudioError(f"voice: decay[{h}] = {voice.decay[h]!r}: finite and >= 0")
    if not (math.isfinite(voice.attack_s) and voice.attack_s >= 0):
        raise AudioError(f"voice: attack_s = {voice.attack_s!r}: finite and >= 0")
    if not (math.isfinite(voice.release_tau) and voice.release_tau > 0):
        raise AudioError(f"voice: release_tau = {voice.release_tau!r}: finite and > 0")
    return voice


def check_settings(fs, voice, peak_db, max_seconds) -> Voice:
    """What Renderer, `render` and `generate --wav` accept; raises AudioError.  Returns the Voice."""
    if isinstance(fs, bool) or not isinstance(fs, (int, np.integer)) or not MIN_FS <= fs <= MAX_FS:
        raise AudioError(f"fs = {fs!r}: an integer sample rate in {MIN_FS}..{MAX_FS} Hz")
    v = check_voice(voice)
    if not (isinstance(peak_db, (int, float)) and math.isfinite(peak_db) and peak_db <= 0):
        raise AudioError(f"peak_db = {peak_db!r}: the peak level in dB full scale, finite and <= 0")
    if 10.0 ** (peak_db / 20.0) * 32767 < 1:
        raise AudioError(f"peak_db = {peak_db!r}: below one step of 16-bit PCM")
    if not (isinstance(max_seconds, (int, float)) and math.isfinite(max_seconds) and max_seconds > 0):
        raise AudioError(f"max_seconds = {max_seconds!r}: finite and > 0")
    if max_seconds * fs >= 2 ** 31:
        raise AudioError(f"max_seconds = {max_seconds!r} at {fs} Hz: a file holds fewer than 2^31 samples")
    return v


@dataclass
class Events:
    """One file's notes as the kernel reads them, stably sorted by onset."""
    onset: np.ndarray       # int32 samples
    release: np.ndarray     # int32 samples, > onset
    inc: np.ndarray         # uint32, 2^-32 turns per sample (2^31: at or above fs / 2, silent)
    gain: np.ndarray        # float32

    def __len__(self):
        return len(self.onset)


def events_from_notes(notes: Sequence[Tuple[int, int, float, float]], fs) -> Events:
    """midi.Note tuples (velocity, pitch, start_s, end_s) -> Events at the sample rate fs:
        onset = floor(start fs + 0.5)      release = max(onset + 1, floor(end fs + 0.5))
        inc = round(440 2^((pitch - 69) / 12) / fs 2^32) in doubles      gain = (velocity / 127)^2
    A fundamental at or above fs / 2 (inc >= 2^31) is stored as 2^31: the kernel's Nyquist test silences every partial of it.
    Raises AudioError on a negative or non-finite time, end fs >= 2^31, or a velocity / pitch outside 0..127."""
    n = len(notes)
    onset, release = np.empty(n, np.int64), np.empty(n, np.int64)
    inc, gain = np.empty(n, np.int64), np.empty(n, np.float32)
    for i, (vel, pitch, start, end) in enumerate(notes):
        start, end = float(start), float(end)
        if not (math.isfinite(start) and math.isfinite(end)):
            raise AudioError(f"note {i}: start = {start!r}, end = {end!r}: not finite")
        if start < 0:
            raise AudioError(f"note {i}: start = {start!r} s is negative")
        if end * fs >= 2 ** 31 or max(math.floor(start * fs + 0.5) + 1, math.floor(end * fs + 0.5)) >= 2 ** 31:
            raise AudioError(f"note {i}: end = {end!r} s at {fs} Hz lies at or past sample 2^31")
        if not (0 <= vel <= 127 and 0 <= pitch <= 127):
            raise AudioError(f"note {i}: velocity {vel!r} / pitch {pitch!r} outside 0..127")
        onset[i] = math.floor(start * fs + 0.5)
        release[i] = max(onset[i] + 1, math.floor(end * fs + 0.5))
        inc[i] = min(2 ** 31, round(440.0 * 2.0 ** ((pitch - 69) / 12.0) / fs * 2.0 ** 32))
        gain[i] = (vel / 127.0) ** 2
    order = np.argsort(onset, kind="stable")
    return Events(onset[order].astype(np.int32), release[order].astype(np.int32), inc[order].astype(np.uint32), gain[order])


def write_wav(path: str, pcm: np.ndarray, fs: int) -> None:
    """Mono 16-bit PCM."""
    pcm = np.asarray(pcm)
    if pcm.dtype != np.int16 or pcm.ndim != 1:
        raise AudioError(f"write_wav: expected a 1-D int16 array, got {pcm.dtype} {pcm.shape}")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(fs))
        w.writeframes(pcm.astype("<i2", copy=False).tobytes())


@dataclass
class FileReport:
    notes: int
    samples: int
    seconds: float
    truncated: bool         # the file would have run past max_seconds and was cut there


def plan_chunks(lengths: Sequence[int], cap_samples: int, chunk_files: int = CHUNK_FILES) -> List[List[int]]:
    """File indices in order, cut into chunks of at most chunk_files files and cap_samples samples.  A file longer than
    cap_samples stands alone (Renderer renders it in windows)."""
    chunks, cur, tot = [], [], 0
    for i, n in enumerate(lengths):
        if cur and (tot + n > cap_samples or len(cur) >= chunk_files):
            chunks.append(cur)
            cur, tot = [], 0
        cur.append(i)
        tot += n
    if cur:
        chunks.append(cur)
    return chunks


class Renderer:
    """render(list of note lists) -> list of int16 arrays, one per file: file length = min(last release + release_len,
    max_seconds fs), peak-normalised to peak_db dB full scale per file (a silent file stays silent).  self.report holds a
    FileReport per file of the last render: a truncated file is reported there, never cut silently.

    Files go through in chunks whose float PCM stays under cap_bytes: per chunk one packed upload, mg_render_notes (with the
    peak in the same launch), mg_pcm_quantise, one download.  The launches are eager, not replayed graphs: a chunk's launch
    arguments are its own (file count, longest file, the note arrays' sizes), chunk shapes rarely repeat, and GraphCache's
    first use of a shape runs the launches once before capturing them -- it would render every new shape twice to save two
    launches.  The kernels are capturable all the same (tests/test_render_gpu.py, tools/render_bench.py)."""

    def __init__(self, device="cuda", fs: int = 44100, voice: Union[str, Voice] = "piano", peak_db: float = -1.0,
                 max_seconds: float = 600, cap_bytes: int = PCM_CAP_BYTES):
        self.voice = check_settings(fs, voice, peak_db, max_seconds)
        if int(cap_bytes) < 4:
            raise AudioError(f"cap_bytes = {cap_bytes}: room for at least one sample")
        self.fs, self.peak_db, self.max_seconds = int(fs), float(peak_db), max_seconds
        self.target = 10.0 ** (self.peak_db / 20.0)
        self.max_samples = int(math.floor(max_seconds * self.fs))
        self.release_len = self.voice.release_len(self.fs)
        self.cap_samples = int(cap_bytes) // 4
        self.device = device
        self.report: List[FileReport] = []
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("melo_gan_amd has no CPU path: a MI355X (ROCm) device is required")
        from . import ops
        v = self.voice
        self._struct = ops.voice_struct(v.mult, v.weight, v.decay, v.attack(self.fs), v.release_tau, self.release_len, self.fs)

    # -- host side ----------------------------------------------------------------------------------------------------
    def plan(self, note_lists) -> Tuple[List[Events], List[int]]:
        """Events and sample count of every file, self.report filled; host only."""
        events = [n if isinstance(n, Events) else events_from_notes(n, self.fs) for n in note_lists]
        lengths, self.report = [], []
        for ev in events:
            full = int(ev.release.max()) + self.release_len if len(ev) else 0
            n = min(full, self.max_samples)
            lengths.append(n)
            self.report.append(FileReport(len(ev), n, n / self.fs, full > n))
        return events, lengths

    # -- device side --------------------------------------------------------------------------------------------------
    def _upload(self, events: Sequence[Events], lengths: Sequence[int], begins: Sequence[int]):
        """One packed int64 buffer with the chunk's per-file and per-note arrays; returns its typed device views."""
        import torch
        from .eval_pass import Packed
        F, N = len(events), max(1, sum(len(e) for e in events))
        i32, i64, f32 = torch.int32, torch.int64, torch.float32
        pk = Packed([("note_ptr", (F + 1,), i64), ("pcm_ptr", (F + 1,), i64), ("n_begin", (F,), i32), ("max_len", (F,), i32),
                     ("onset", (N,), i32), ("release", (N,), i32), ("inc", (N,), i32), ("gain", (N,), f32)], self.device)
        host = torch.zeros(pk.words, dtype=i64)
        hv = {k: v.numpy() for k, v in pk.views(host).items()}
        hv["note_ptr"][1:] = np.cumsum([len(e) for e in events])
        hv["pcm_ptr"][1:] = np.cumsum(lengths)
        hv["n_begin"][:] = begins
        a = 0
        for f, e in enumerate(events):
            b = a + len(e)
            hv["onset"][a:b], hv["release"][a:b], hv["gain"][a:b] = e.onset, e.release, e.gain
            hv["inc"][a:b] = e.inc.view(np.int32)
            hv["max_len"][f] = int((e.release.astype(np.int64) - e.onset).max()) + self.release_len if len(e) else 0
            a = b
        pk.buf.copy_(host)
        return pk.dev

    def _render_chunk(self, events, lengths, begins, peak=None):
        """Render and quantise one chunk; peak: the files' peaks when they are not this launch's own (a window of a file).
        Returns (int16 host array of the chunk, the launch's own peaks on the device)."""
        import torch
        from . import ops
        total, longest = sum(lengths), max(lengths)
        d = self._upload(events, lengths, begins)
        pcm = torch.empty(total, dtype=torch.float32, device=self.device)
        own = torch.empty(len(events), dtype=torch.float32, device=self.device)
        ops.render_notes(d["onset"], d["release"], d["inc"], d["gain"], d["note_ptr"], d["pcm_ptr"], d["n_begin"], d["max_len"],
                         longest, self._struct, pcm, own)
        if peak is False:            # the first pass over a windowed file wants the peak alone
            return None, own
        q = torch.empty(total, dtype=torch.int16, device=self.device)
        ops.pcm_quantise(pcm, d["pcm_ptr"], own if peak is None else peak, longest, self.target, q)
        return q.cpu().numpy(), own

    def _render_windowed(self, ev: Events, n: int) -> np.ndarray:
        """A file longer than the PCM cap: a first pass over its windows for the peak (the integer maximum of the windows'
        peaks' bits), a second that renders each window again and quantises it with that peak."""
        import torch
        wins = [(b, min(self.cap_samples, n - b)) for b in range(0, n, self.cap_samples)]
        peak = torch.zeros(1, dtype=torch.int32, device=self.device)
        for b, m in wins:
            peak = torch.maximum(peak, self._render_chunk([ev], [m], [b], peak=False)[1].view(torch.int32))
        peak = peak.view(torch.float32)
        return np.concatenate([self._render_chunk([ev], [m], [b], peak=peak)[0] for b, m in wins])

    def render(self, note_lists) -> List[np.ndarray]:
        events, lengths = self.plan(note_lists)
        out: List[Optional[np.ndarray]] = [None] * len(events)
        for chunk in plan_chunks(lengths, self.cap_samples):
            ev, ln = [events[i] for i in chunk], [lengths[i] for i in chunk]
            if sum(ln) == 0:
                q = np.zeros(0, np.int16)
            elif len(chunk) == 1 and ln[0] > self.cap_samples:
                q = self._render_windowed(ev[0], ln[0])
            else:
                q = self._render_chunk(ev, ln, [0] * len(chunk))[0]
            for i, a in zip(chunk, np.split(q, np.cumsum(ln)[:-1])):
                out[i] = a
        return out
