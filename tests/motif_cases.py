"""What the motif tests and tools/motif_bench.py share: seeded random-walk melodies as events and as tokens, the brute-force
scan that host_lcs answers to, and the MIDI files of the command-line tests.  numpy only."""
import os

import numpy as np

from melo_gan_amd import midi
from melo_gan_amd import midi_rolls as MR

# one representative step in ticks of 1/64 beat per rhythm class, and how often a melody takes it
CLASS_STEPS = (8, 16, 32, 64, 128, 256)
CLASS_WEIGHTS = (0.10, 0.40, 0.25, 0.15, 0.07, 0.03)


def walk_tokens(rng, rows: int, m: int) -> np.ndarray:
    """Tokens of random-walk melodies, uint16 (rows, m): intervals N(0, 3) rounded and clipped to +-12, six unevenly weighted
    rhythm classes."""
    interval = np.clip(np.rint(rng.normal(0.0, 3.0, (rows, m))), -12, 12).astype(np.int64)
    rhythm = rng.choice(6, size=(rows, m), p=CLASS_WEIGHTS)
    return ((interval + 64) | (rhythm << 7)).astype(np.uint16)


def walk_events(rng, n: int, rests: float = 0.0) -> np.ndarray:
    """A random-walk melody as (pitch, velocity, dur_q, step_q) events, int64 (n, 4), inside the roll contract's image, the
    pitches kept in 48..84 so that a transposed copy stays inside it; `rests`: the share of rest events."""
    pitch, p = np.empty(n, np.int64), 66
    for k in range(n):
        p = int(np.clip(p + int(np.clip(np.rint(rng.normal(0.0, 3.0)), -12, 12)), 48, 84))
        pitch[k] = p
    step = np.asarray(CLASS_STEPS)[rng.choice(6, size=n, p=CLASS_WEIGHTS)]
    ev = np.stack([pitch, rng.integers(60, 128, n), np.full(n, 32), step], axis=1).astype(np.int64)
    rest = rng.random(n) < rests
    ev[rest, :3] = (0, -1, 0)
    return ev


def rolls_of(event_lists, T: int) -> np.ndarray:
    """(N, T, 4) float32 rolls of N event lists, each at most T long, filled up with the padding row."""
    x = np.full((len(event_lists), T, 4), -1.0, np.float32)
    for n, ev in enumerate(event_lists):
        ev = np.asarray(ev).reshape(-1, 4)
        x[n, :ev.shape[0]] = MR.encode_events(ev)[0]
    return x


def brute_lcs(a, b):
    """(L, i_end, j_end, reach) of two token sequences by the definition: every cell's run counted backwards on its own."""
    a, b = list(a), list(b)
    best, reach = (0, -1, -1), np.zeros(len(a), np.int64)
    for i in range(len(a)):
        for j in range(len(b)):
            r = 0
            while i - r >= 0 and j - r >= 0 and a[i - r] == b[j - r]:
                r += 1
            reach[i] = max(reach[i], r)
            if r > best[0]:         # i, then j, ascending: the first cell that attains it
                best = (r, i, j)
    return best[0], best[1], best[2], reach


def token_rows(seqs, T: int):
    """(tokens uint16 (N, T) padded with 0xFFFF, lengths int32 (N,)) of N token sequences."""
    t = np.full((len(seqs), T), 0xFFFF, np.uint16)
    for n, s in enumerate(seqs):
        t[n, :len(s)] = np.asarray(s, np.uint16)
    return t, np.array([len(s) for s in seqs], np.int32)


PHRASE_SHIFT = 5        # b.mid plays a.mid's phrase this many semitones higher


def _notes(pitches, steps_beats, bpm=120.0, start_beats=0.0):
    out, t, spb = [], start_beats, 60.0 / bpm
    for p, s in zip(pitches, steps_beats):
        out.append((90, int(p), t * spb, (t + min(s, 0.5)) * spb))
        t += s
    return out, t


def write_midi_cases(folder: str) -> dict:
    """a.mid and b.mid share a 20-note phrase, PHRASE_SHIFT semitones apart and at different places; c.mid shares nothing
    with either.  Returns {"a", "b", "c": the paths; "phrase_notes": 20}."""
    g = np.random.default_rng(11)
    beats = np.array([0.25, 0.5, 1.0, 1.5])
    phrase_p = 60 + np.array([0, 4, 7, 5, 9, 2, 11, 7, 12, 3, 8, 1, 10, 6, 13, 4, 9, 0, 7, 5])
    phrase_s = beats[np.array([1, 0, 2, 1, 1, 3, 0, 0, 2, 1, 3, 1, 0, 2, 1, 1, 0, 3, 2, 1])]

    def filler(n, lo):     # a stepwise line: intervals of +-1 only, which the phrase never has twice in a row
        return lo + np.cumsum(g.choice([-1, 1], n)), np.full(n, 0.75)

    os.makedirs(folder, exist_ok=True)
    paths = {}
    # b's fillers start one semitone off a's: the intervals into and out of the phrase differ in parity or size between the
    # two files, so the shared run is the phrase's 19 tokens exactly
    for name, lead, tail, shift in (("a", 6, 4, 0), ("b", 11, 9, PHRASE_SHIFT)):
        lp, ls = filler(lead, 50 + (shift > 0))
        tp, ts = filler(tail, 80 + (shift > 0))
        notes, _ = _notes(np.concatenate([lp, phrase_p + shift, tp]), np.concatenate([ls, phrase_s, ts]))
        paths[name] = os.path.join(folder, name + ".mid")
        midi.write_smf(paths[name], notes, 120.0, 0)
    cp = 70 + np.cumsum(np.tile([2, -2, 2, 2, -2, -2], 6))       # a whole-tone zigzag, steps of 1.25 beats
    notes, _ = _notes(cp, np.full(cp.size, 1.25))
    paths["c"] = os.path.join(folder, "c.mid")
    midi.write_smf(paths["c"], notes, 120.0, 0)
    paths["phrase_notes"] = int(phrase_p.size)
    return paths
