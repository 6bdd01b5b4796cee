"""The fp64 restatement of mg_render_notes (include/melo_gan_hip.h), the bound tests/test_render_gpu.py holds the kernel to, and
the note set both test files use.  A plain helper module beside support_ref / rowstep_ref: nothing here is collected.

For the file-local sample n, with k = n - onset and kr = max(n - release, 0), a note is live while onset <= n < release +
release_len, and

    y[n] = sum over live notes i in array order, over partials h ascending, skipped when mult[h] * inc[i] >= 2^31
             gain[i] * min((k + 1) / attack, 1) * exp(-kr / (fs * release_tau)) * weight[h] * exp(-decay[h] * k / fs) * sin(2 pi x)
    x    = ((((mult[h] * inc[i]) mod 2^32) * k mod 2^32) >> 8) * 2^-24

The phase is the kernel's integer phase; k / fs, the envelopes and the sine are evaluated in doubles from the fp32 table values
the kernel is given.  Besides y, render() returns per sample S = the sum of |amplitude| over its terms (the term without its
sine), M = the number of terms and A = the largest magnitude of an exponent among them.

THE BOUND  |y_kernel - y| <= (32 + 2 A + M) 2^-24 S  per sample: 4 ulp for the sine and 3 for the exponential, the roundings of
the products that build the amplitude, the fp32 roundings of the two exponents (each relative, so worth A ulp of the
exponential) and M fp32 additions of terms no larger than S.  It is derived from the formats, not from any kernel's output.
emulate_fp32() is the formula in numpy fp32 (tests/test_render_cpu.py shows it stays far inside the bound while a dropped
partial or a wrong envelope does not).
"""
import numpy as np

FS = 8000
# the tests' own voice: (mult, weight, decay 1/s), attack and release_len in samples, release_tau in s.  40003 x an audible
# increment wraps past 2^32 (test below): that partial must be silent, not aliased.
MULT = (1, 2, 3, 5, 40003)
WEIGHT = (1.0, 0.5, 0.33, 0.2, 0.25)
DECAY = (0.0, 1.5, 3.0, 6.0, 0.5)
ATTACK, RELEASE_TAU = 40, 0.02
RELEASE_LEN = int(np.ceil(RELEASE_TAU * np.log(1000.0) * FS))           # 1106
LENGTHS = (5000, 1, 257)                                                 # the three files of the kernel test, in batch order


def pitch_inc(pitch, fs=FS):
    """events_from_notes' increment: round(f / fs 2^32) in doubles, 2^31 at or above fs / 2."""
    return min(2 ** 31, round(440.0 * 2.0 ** ((pitch - 69) / 12.0) / fs * 2.0 ** 32))


def sort_notes(rows):
    """rows of (onset, release, pitch, velocity) -> the kernel's arrays, stably sorted by onset."""
    rows = sorted(rows, key=lambda r: r[0])
    return {"onset": np.array([r[0] for r in rows], np.int32), "release": np.array([r[1] for r in rows], np.int32),
            "inc": np.array([pitch_inc(r[2]) for r in rows], np.uint32),
            "gain": np.array([(r[3] / 127.0) ** 2 for r in rows], np.float32)}


def case_files():
    """The kernel test's three files (LENGTHS): 36 notes in the long one, none in the one-sample one, 4 in the 257-sample one."""
    rng = np.random.default_rng(20)
    big = [(100, 110, 60, 100),                  # released inside its own attack (40 samples)
           (500, 900, 64, 90), (500, 700, 67, 80),       # one onset, two notes
           (0, 300, 57, 110),                    # sounds from sample 0
           (4800, 4990, 62, 100),                # the tail runs past the end of the file
           (4500, 5600, 55, 70),                 # so does the note itself
           (1200, 2400, 108, 127),               # 4186 Hz > fs / 2: silent
           (1300, 2600, 96, 120),                # 2093 Hz: only the first partial is below fs / 2
           (2000, 2800, 69, 100)]                # A4: 40003 x its increment wraps past 2^32 to a value below 2^31
    for _ in range(36 - len(big)):
        on = int(rng.integers(0, 4900))
        big.append((on, on + int(rng.integers(20, 1500)), int(rng.integers(36, 97)), int(rng.integers(30, 128))))
    small = [(0, 50, 72, 100), (0, 400, 48, 64), (200, 256, 81, 127), (255, 300, 60, 90)]
    return [sort_notes(big), sort_notes([]), sort_notes(small)]


def render(ev, n_begin, length, mult=MULT, weight=WEIGHT, decay=DECAY, attack=ATTACK, release_tau=RELEASE_TAU,
           release_len=RELEASE_LEN, fs=FS, skip_partial=None, release_scale=1.0):
    """fp64: (y, S, M, A) over the file-local samples n_begin .. n_begin + length - 1.  skip_partial / release_scale plant the
    structural mistakes the bound has to catch (a dropped partial, a wrong release envelope)."""
    w = np.asarray(weight, np.float32).astype(np.float64)
    d = np.asarray(decay, np.float32).astype(np.float64)
    tau, fs64 = float(np.float32(release_tau)), float(np.float32(fs))
    y, S, A = np.zeros(length), np.zeros(length), np.zeros(length)
    M = np.zeros(length, np.int64)
    for on, rel, inc, g in zip(ev["onset"].astype(np.int64), ev["release"].astype(np.int64), ev["inc"].astype(np.uint64),
                               ev["gain"].astype(np.float64)):
        a, b = max(on, n_begin), min(rel + release_len, n_begin + length)
        if a >= b:
            continue
        n = np.arange(a, b, dtype=np.int64)
        k, kr = n - on, np.maximum(n - rel, 0)
        sl = slice(a - n_begin, b - n_begin)
        env = g * np.minimum((k + 1) / attack, 1.0)
        xr = kr / (fs64 * tau) * release_scale
        for h in range(len(mult)):
            step = int(mult[h]) * int(inc)
            if step >= 2 ** 31 or h == skip_partial:
                continue
            phase = (np.uint64(step & 0xFFFFFFFF) * k.astype(np.uint64)) & np.uint64(0xFFFFFFFF)
            x = (phase >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
            xd = d[h] * k / fs64
            amp = env * np.exp(-xr) * w[h] * np.exp(-xd)
            y[sl] += amp * np.sin(2.0 * np.pi * x)
            S[sl] += np.abs(amp)
            M[sl] += 1
            A[sl] = np.maximum(A[sl], np.maximum(xr, xd))
    return y, S, M, A


def bound(S, M, A):
    return (32.0 + 2.0 * A + M) * 2.0 ** -24 * S


def emulate_fp32(ev, n_begin, length, mult=MULT, weight=WEIGHT, decay=DECAY, attack=ATTACK, release_tau=RELEASE_TAU,
                 release_len=RELEASE_LEN, fs=FS):
    """The formula with every operation in numpy fp32 (phase in integers), added in array order."""
    f32 = np.float32
    w, d = np.asarray(weight, f32), np.asarray(decay, f32)
    y = np.zeros(length, f32)
    for on, rel, inc, g in zip(ev["onset"].astype(np.int64), ev["release"].astype(np.int64), ev["inc"].astype(np.uint64), ev["gain"]):
        a, b = max(on, n_begin), min(rel + release_len, n_begin + length)
        if a >= b:
            continue
        n = np.arange(a, b, dtype=np.int64)
        k, kr = n - on, np.maximum(n - rel, 0)
        sl = slice(a - n_begin, b - n_begin)
        env = f32(g) * np.minimum((k + 1).astype(f32) / f32(attack), f32(1))
        er = np.exp(-(kr.astype(f32) / (f32(fs) * f32(release_tau))))
        for h in range(len(mult)):
            step = int(mult[h]) * int(inc)
            if step >= 2 ** 31:
                continue
            phase = (np.uint64(step & 0xFFFFFFFF) * k.astype(np.uint64)) & np.uint64(0xFFFFFFFF)
            x = (phase >> np.uint64(8)).astype(f32) * f32(2.0 ** -24)
            ed = np.exp(-(d[h] * k.astype(f32) / f32(fs)))
            y[sl] = y[sl] + env * er * w[h] * ed * np.sin(f32(2 * np.pi) * x)
    return y
