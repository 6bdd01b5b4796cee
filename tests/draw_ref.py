"""Host restatement of every device random draw (numpy, uint64 arithmetic, no torch): Philox4x32-10, u01, Box-Muller, the
counter layout of each kernel that draws (include/melo_gan_hip.h: mg_rng_fill, mg_gen_inputs, mg_stage_augment,
mg_weighted_order, mg_eval_noise, mg_latent_rows) and the two augmentation programs of mg_stage_augment element by element.
A plain helper module beside support_ref; nothing here is collected.  tests/test_draw_ref.py holds this file to the
Random123 known answers and to its own statistics; tests/test_draw_contract_gpu.py holds the kernels to this file.

What is exact and what is bounded.  A Philox word is an integer: exact.  u01 is one conversion of a 24-bit integer (exact),
one fp32 add and one scale by 2^-24 (exact), then the clamp: the float32 arithmetic below gives the device's bits.  So do
uniforms, masks, gates, shifts, dropped rows and sampler orders.  A normal is r cos(t) / r sin(t) with r = sqrt(-2 log u):
u and t = 6.2831855f * u' (one fp32 product) are restated bit for bit, the rest is evaluated in fp64 here and by logf, sqrtf,
cosf / sinf and one fp32 product on the device.  All of the device's error is therefore relative:

    |dev - ref| <= (L/2 + S + C + 1/2) 2^-23 |ref| + 2^-23 r        r = sqrt(-2 log u) <= 5.89

L, S, C the ulp limits of logf, sqrtf and cosf / sinf (L enters halved: it sits under the square root), 1/2 the final
product; the floor term covers the library's argument reduction near the zeros of cos and sin (below 7e-7).  The ROCm
toolchain installs no document or header that states ulp limits for these four functions (its OpenCL header states them
only for the half_ / native_ forms), so the limits are OpenCL's full-profile ones (OpenCL C specification, "Relative error as
ULPs", single precision): log 3, sqrt 3, sin / cos 4.  These are worst-case limits, not measurements; nothing is added.
"""
from fractions import Fraction

import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85

GEN_TAG, AUG_TAG, EVAL_TAG, LAT_TAG = 0x47454E00, 0x41554700, 0x4556414C, 0x4C415400
AUG_GATES, AUG_GATES2, AUG_DROP, AUG_NOISE, AUG_ORDER = 0, 1, 2, 3, 4

U01_MIN, U01_MAX = np.float32(2.0 ** -25), np.float32(1.0 - 2.0 ** -24)
TWO_PI_F = np.float32(6.28318530717958647692)       # the device's literal 6.28318530717958647692f = 6.2831855f

ULP_LOG, ULP_SQRT, ULP_SINCOS = 3.0, 3.0, 4.0       # OpenCL full profile (see the module docstring)
NORMAL_REL = (ULP_LOG / 2 + ULP_SQRT + ULP_SINCOS + 0.5) * 2.0 ** -23
NORMAL_FLOOR = 2.0 ** -23
HALF_ULP = 2.0 ** -24                               # one fp32 rounding, relative


def w32(x):
    """The low 32 bits of integers (Python ints of any size and sign, or integer arrays) as uint64: a C cast to unsigned."""
    if isinstance(x, (int, np.integer)):
        return np.uint64(int(x) & M32)
    a = np.asarray(x)
    if a.dtype.kind == "i":
        a = a.astype(np.int64).view(np.uint64)
    return a.astype(np.uint64) & np.uint64(M32)


def lo_hi(x):
    """(low word, high word) of a 64-bit value given as a Python int or an integer array, modulo 2^64."""
    if isinstance(x, (int, np.integer)):
        x = int(x) & M64
        return np.uint64(x & M32), np.uint64(x >> 32)
    a = np.asarray(x)
    if a.dtype.kind == "i":
        a = a.astype(np.int64).view(np.uint64)
    a = a.astype(np.uint64)
    return a & np.uint64(M32), a >> np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11), vectorised: counter words and key words broadcast against each other; the result
    has a last axis of 4 (uint32), in the order philox_round writes the words."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(w32(v) for v in (c0, c1, c2, c3, k0, k1)))
    m32, s32 = np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c0
        p1 = np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0 = (k0 + np.uint64(PHILOX_W0)) & m32
        k1 = (k1 + np.uint64(PHILOX_W1)) & m32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def keyed(c0, c1, c2, c3, seed):
    """philox4x32_10 under key = (seed lo, seed hi), as every kernel here keys it."""
    k0, k1 = lo_hi(seed)
    return philox4x32_10(c0, c1, c2, c3, k0, k1)


def u01(word):
    """csrc/common.h u01 in float32, bit for bit: ((float)(x >> 8) + 0.5f) * 2^-24, clamped to 1 - 2^-24 (the sum
    16777215.5 is a tie and rounds to 2^24).  Range [2^-25, 1 - 2^-24]."""
    x = (np.asarray(word).astype(np.uint64) >> np.uint64(8)).astype(np.float32)
    return np.minimum((x + np.float32(0.5)) * np.float32(2.0 ** -24), U01_MAX)


def box_muller_r(words):
    """r = sqrt(-2 log u) of each of the four normals of a block (fp64; the pairs share theirs)."""
    u = u01(words).astype(np.float64)
    r0, r1 = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    return np.stack([r0, r0, r1, r1], axis=-1)


def box_muller4(words):
    """csrc/common.h box_muller4 in fp64 from the device's own u and t: words (..., 4) -> normals (..., 4), Box-Muller on the
    pairs (c0, c1) and (c2, c3): (r0 cos t0, r0 sin t0, r1 cos t1, r1 sin t1)."""
    u = u01(words)
    t32 = TWO_PI_F * u                                  # one float32 product ...
    assert t32.dtype == np.float32
    t = t32.astype(np.float64)                          # ... then widened
    r = box_muller_r(words)
    return np.stack([r[..., 0] * np.cos(t[..., 1]), r[..., 1] * np.sin(t[..., 1]),
                     r[..., 2] * np.cos(t[..., 3]), r[..., 3] * np.sin(t[..., 3])], axis=-1)


def normal_bound(v, r):
    """The bound of the module docstring for device normals whose fp64 references are v, with their r."""
    return NORMAL_REL * np.abs(v) + NORMAL_FLOOR * r


def normals(words):
    """(fp64 normals, bounds) of Philox blocks (..., 4)."""
    v = box_muller4(words)
    return v, normal_bound(v, box_muller_r(words))


# ---- counter builders: one per site (X_counter: the four counter words; X_words: the Philox block under key = seed) --------
def rng_fill_counter(q, jid, step):
    """rng_fill_kernel: (q, (q >> 32) ^ (jid << 28), step lo, step hi); jid = the tensor's place among the non-NULL ones."""
    qlo, qhi = lo_hi(q)
    slo, shi = lo_hi(step)
    return qlo, qhi ^ np.uint64((jid << 28) & M32), slo, shi


def gen_counter(qb, which, emotion, sample):
    """gen_inputs_kernel / gen_draw: (qb, GEN_TAG | which, emotion, sample); which 0 noise, 1 jitter."""
    return w32(qb), w32(GEN_TAG | which), w32(emotion), w32(sample)


def aug_counter(t, need, serial):
    """aug_draw: (t, AUG_TAG | need, serial lo, serial hi); need 4 is weighted_order_kernel's (t = i, serial = epoch)."""
    slo, shi = lo_hi(serial)
    return w32(t), w32(AUG_TAG | need), slo, shi


def eval_counter(qb, i):
    """eval_noise_kernel: (qb, EVAL_TAG, i lo, i hi), i the split row."""
    ilo, ihi = lo_hi(i)
    return w32(qb), w32(EVAL_TAG), ilo, ihi


def lat_counter(q, piece, sample):
    """latent_rows_kernel: (q, LAT_TAG, piece, sample)."""
    return w32(q), w32(LAT_TAG), w32(piece), w32(sample)


def rng_fill_words(q, jid, seed, step):
    return keyed(*rng_fill_counter(q, jid, step), seed)


def gen_words(qb, which, emotion, sample, seed):
    return keyed(*gen_counter(qb, which, emotion, sample), seed)


def aug_words(t, need, serial, seed):
    return keyed(*aug_counter(t, need, serial), seed)


def eval_words(qb, i, seed):
    return keyed(*eval_counter(qb, i), seed)


def lat_words(q, piece, sample, seed):
    return keyed(*lat_counter(q, piece, sample), seed)


def word1_ranges():
    """Counter word 1 of each layout as an inclusive (lowest, highest) range over jid < 4, q < 2^32, which < 2, need < 5, read
    off the counter builders themselves (word 1 depends on nothing else)."""
    def span(words):
        words = [int(w) for w in words]
        return min(words), max(words)
    return {"rng_fill": span(rng_fill_counter(q, jid, 0)[1] for jid in range(4) for q in (0, M32)),
            "gen": span(gen_counter(0, which, 0, 0)[1] for which in range(2)),
            "aug": span(aug_counter(0, need, 0)[1] for need in range(5)),
            "eval": span([eval_counter(0, 0)[1]]),
            "lat": span([lat_counter(0, 0, 0)[1]])}


# ---- mg_rng_fill ------------------------------------------------------------------------------------------------------------
def _blocks(n):
    return np.arange((n + 3) // 4, dtype=np.uint64)


def rng_fill(n_normal, n_uniform, n_mask0, n_mask1, p_drop, seed, step):
    """One mg_rng_fill call at step counter `step`; a length of None or 0 is an absent tensor.  Returns a dict with
    'normal': (fp64 reference, bound), 'uniform', 'mask0', 'mask1': float32 arrays (bit-exact); absent ones are missing."""
    out, jid = {}, 0
    p = np.float32(p_drop)
    sc = np.float32(1.0) / (np.float32(1.0) - p)
    for name, n in (("normal", n_normal), ("uniform", n_uniform), ("mask0", n_mask0), ("mask1", n_mask1)):
        if not n:
            continue
        w = rng_fill_words(_blocks(n), jid, seed, step)
        jid += 1
        if name == "normal":
            v, b = normals(w)
            out[name] = (v.reshape(-1)[:n], b.reshape(-1)[:n])
        elif name == "uniform":
            out[name] = u01(w).reshape(-1)[:n]
        else:
            out[name] = np.where(u01(w) >= p, sc, np.float32(0.0)).astype(np.float32).reshape(-1)[:n]
    return out


def find_unit_uniform(seed, steps, n_blocks, jid=1):
    """The (step, element, word) of every rng_fill draw of stream jid whose top 24 bits are all ones (the words the
    unclamped u01 took to 1.0), over the given steps and the first n_blocks blocks."""
    steps = np.asarray(list(steps), dtype=np.uint64)
    w = rng_fill_words(np.arange(n_blocks, dtype=np.uint64)[None, :], jid, seed, steps[:, None])
    s, q, e = np.nonzero(w >= np.uint32(0xFFFFFF00))
    return [(int(steps[a]), int(4 * b + c), int(w[a, b, c])) for a, b, c in zip(s, q, e)]


# ---- mg_gen_inputs, mg_eval_noise, mg_latent_rows ---------------------------------------------------------------------------
def _rows_of_normals(words_of_row, rows, dim):
    """(rows, dim) fp64 normals and bounds from a function row -> Philox blocks ((dim + 3) / 4, 4)."""
    v = np.zeros((rows, dim))
    b = np.zeros((rows, dim))
    for r in range(rows):
        w = words_of_row(r)
        if w is None:
            continue
        vr, br = normals(w)
        v[r], b[r] = vr.reshape(-1)[:dim], br.reshape(-1)[:dim]
    return v, b


def gen_inputs(emotion, sample, noise_dim, num_dim, table, jitter, seed):
    """mg_gen_inputs: returns a dict of fp64 (value, bound) pairs: 'noise', 'jitter' (the normals v under the numeric input)
    and 'numeric'.  table (n_emotions, num_dim) float32.  A row whose emotion lies outside the table is zeros (bound 0).
    numeric = base + jitter * v: the device rounds the product and the sum (once, if fused: no more than twice), so its
    bound is |jitter| * the normal's + one ulp of the result; with a zero table and jitter 1 it is v itself."""
    table = np.asarray(table, dtype=np.float32)
    rows, n_em = len(emotion), table.shape[0]
    live = [0 <= int(e) < n_em for e in emotion]
    z, zb = _rows_of_normals(lambda r: gen_words(_blocks(noise_dim), 0, int(emotion[r]), int(sample[r]), seed) if live[r] else None,
                             rows, noise_dim)
    v, vb = _rows_of_normals(lambda r: gen_words(_blocks(num_dim), 1, int(emotion[r]), int(sample[r]), seed) if live[r] else None,
                             rows, num_dim)
    j = float(np.float32(jitter))
    num, numb = np.zeros((rows, num_dim)), np.zeros((rows, num_dim))
    for r in range(rows):
        if live[r]:
            num[r] = table[int(emotion[r])].astype(np.float64) + j * v[r]
            numb[r] = abs(j) * vb[r] + 2.0 ** -23 * np.abs(num[r])
    return {"noise": (z, zb), "jitter": (v, vb), "numeric": (num, numb)}


def eval_noise(rows, noise_dim, k, n, seed):
    """mg_eval_noise for batch k = counter - base of `rows` rows over a split of n rows: row r has i = k * rows + r and is
    zeros (bound 0) when i >= n."""
    return _rows_of_normals(lambda r: eval_words(_blocks(noise_dim), k * rows + r, seed) if k * rows + r < n else None,
                            rows, noise_dim)


def latent_prior(keys, L, seed):
    """mg_latent_rows for prior rows (kind 1, no direction, sigma 1): z is the normal itself.  keys: (piece, sample) pairs."""
    return _rows_of_normals(lambda r: lat_words(_blocks(L), int(keys[r][0]), int(keys[r][1]), seed), len(keys), L)


# ---- mg_stage_augment -------------------------------------------------------------------------------------------------------
AE_GATE_ODDS = {"tempo": 0.3, "pitch": 0.3, "drop": 0.2, "velocity": 0.3, "timing": 0.2}


def _f32(v):
    return np.float32(v)


def ae_gates(serial, seed):
    """The five gate decisions of the AE program for one sample (each before its parameter's `> 0` switch), and the two
    Philox blocks they come from."""
    c, g = aug_words(0, AUG_GATES, serial, seed), aug_words(0, AUG_GATES2, serial, seed)
    return {"tempo": bool(u01(c[0]) < _f32(0.3)), "pitch": bool(u01(c[1]) < _f32(0.3)), "drop": bool(u01(c[2]) < _f32(0.2)),
            "velocity": bool(u01(c[3]) < _f32(0.3)), "timing": bool(u01(g[0]) < _f32(0.2))}, c, g


def ae_tempo_factor(word, tempo_jitter):
    """(factor, fused_differs): 1 + (2 u01(word) - 1) * tempo_jitter in float32 with the product and the sum each rounded on
    its own (2u - 1 is exact), and whether a single rounding of the exact value -- what one fused multiply-add gives -- is
    another float32, decided in exact rational arithmetic."""
    d = _f32(2.0) * u01(word) - _f32(1.0)
    f = _f32(1.0) + d * _f32(tempo_jitter)
    exact = 1 + Fraction(float(d)) * Fraction(float(_f32(tempo_jitter)))
    err = abs(Fraction(float(f)) - exact)
    beside = min(abs(Fraction(float(np.nextafter(f, _f32(to)))) - exact) for to in (0.0, 2.0))
    return f, beside < err


def stage_position(r, n_rows, order, order_len, k, last):
    pos = order_len - n_rows + r if last else ((k * n_rows + r) & M64) % order_len
    return pos, (pos if order is None else int(order[pos]))


def stage_augment(x, program, seed, params, n_rows, order=None, order_len=None, k=0, serial_base=0, last=False):
    """mg_stage_augment on the host.  x (src_rows, T, C) float32; params: the program's parameters by name (missing: 0).
    Returns (exact, ref, bound, info): exact float32 (n_rows, T, C) -- the device's bits wherever bound == 0; ref fp64 and
    bound fp64 -- where an element received a normal (bound > 0) the device is held to |dev - ref| <= bound = sigma * the
    normal's bound + the fp32 rounding of the product and that of the sum.  info[r]: the sample's serial and what its gates
    decided.  Everything else is float32 arithmetic with every product and sum rounded on its own, as the kernel's
    __fmul_rn / __fadd_rn."""
    x = np.asarray(x, dtype=np.float32)
    src_rows, T, C = x.shape
    order_len = (src_rows if order is None else len(order)) if order_len is None else order_len
    P = {key: params.get(key, 0) for key in ("noise_std", "dropout_prob", "pitch_shift_prob", "tempo_jitter", "pitch_shift",
                                             "note_dropout", "velocity_jitter", "timing_jitter")}
    exact = np.empty((n_rows, T, C), np.float32)
    ref = np.empty((n_rows, T, C), np.float64)
    bound = np.zeros((n_rows, T, C), np.float64)
    info = []
    t = np.arange(T, dtype=np.uint64)

    def add_normal(base32, sigma, nv, nb):
        """fadd(base, fmul(sigma, n)): the fp64 value and its bound."""
        s = float(sigma)
        prod, e_prod = s * nv, s * nb
        e_prod = e_prod + HALF_ULP * (np.abs(prod) + e_prod)
        val = base32.astype(np.float64) + prod
        return val, e_prod + HALF_ULP * (np.abs(val) + e_prod)

    for r in range(n_rows):
        pos, sr = stage_position(r, n_rows, order, order_len, k, last)
        sr = min(max(sr, 0), src_rows - 1)
        serial = (serial_base + pos) & M64
        v = x[sr].copy()
        nval = {}                                   # column -> (fp64 value, bound) of the elements that received a normal
        row = {"serial": serial, "pos": pos, "src": sr}
        if program == "ed":
            shift = 0.0
            if _f32(P["pitch_shift_prob"]) > 0:
                c = aug_words(0, AUG_GATES, serial, seed)
                if u01(c[0]) < _f32(P["pitch_shift_prob"]):
                    shift = 1.0 if int(c[1]) & 1 else -1.0
            row["shift"] = shift
            if _f32(P["noise_std"]) > 0:
                nv, nb = normals(aug_words(t, AUG_NOISE, serial, seed))
                for col in (1, 2, 3):
                    nval[col] = add_normal(v[:, col], _f32(P["noise_std"]), nv[:, col - 1], nb[:, col - 1])
            dropped = np.zeros(T, bool)
            if _f32(P["dropout_prob"]) > 0:
                u = u01(aug_words(t, AUG_DROP, serial, seed)[:, 0])
                dropped = ~(u >= _f32(P["dropout_prob"]))
                v[dropped] = 0.0
            row["dropped"] = dropped
            if shift != 0.0:
                v[:, 0] = v[:, 0] + _f32(shift)
            exact[r], ref[r] = v, v.astype(np.float64)
            for col, (val, b) in nval.items():
                ref[r, :, col] = np.where(dropped, 0.0, val)
                bound[r, :, col] = np.where(dropped, 0.0, b)
        else:
            gates, c, g = ae_gates(serial, seed)
            row["gates"] = gates
            tj = _f32(P["tempo_jitter"])
            factor = _f32(1.0)
            if tj > 0 and gates["tempo"]:
                factor, row["fused_differs"] = ae_tempo_factor(g[1], tj)
                v[:, 1] = v[:, 1] * factor
                v[:, 2] = v[:, 2] * factor
            row["factor"] = float(factor)
            shift, ps = 0.0, int(P["pitch_shift"])
            if ps > 0 and gates["pitch"]:
                shift = float(((int(g[2]) * (2 * ps + 1)) >> 32) - ps)
                if shift != 0.0:
                    v[:, 0] = v[:, 0] + _f32(shift)
            row["shift"] = shift
            dropped = np.zeros(T, bool)
            if _f32(P["note_dropout"]) > 0 and gates["drop"]:
                u = u01(aug_words(t, AUG_DROP, serial, seed)[:, 0])
                dropped = ~(u > _f32(P["note_dropout"]))
                v[dropped] = 0.0
            row["dropped"] = dropped
            jit_v = _f32(P["velocity_jitter"]) > 0 and gates["velocity"]
            jit_t = _f32(P["timing_jitter"]) > 0 and gates["timing"]
            exact[r], ref[r] = v, v.astype(np.float64)
            if jit_v or jit_t:
                nv, nb = normals(aug_words(t, AUG_NOISE, serial, seed))
                if jit_v:
                    ref[r, :, 3], bound[r, :, 3] = add_normal(v[:, 3], _f32(P["velocity_jitter"]), nv[:, 0], nb[:, 0])
                if jit_t:
                    val, b = add_normal(v[:, 1], _f32(P["timing_jitter"]), nv[:, 1], nb[:, 1])
                    ref[r, :, 1], bound[r, :, 1] = np.maximum(val, 0.0), b          # fmaxf(., 0): 1-Lipschitz
        info.append(row)
    return exact, ref, bound, info


def randint_shift(word, p):
    """The AE program's randint(-p, p), both ends included, from one Philox word: (word * (2p + 1)) >> 32, minus p."""
    return ((np.asarray(word).astype(np.uint64) * np.uint64(2 * p + 1)) >> np.uint64(32)).astype(np.int64) - p


# ---- mg_weighted_order ------------------------------------------------------------------------------------------------------
def weighted_order(cdf, m, seed, epoch):
    """weighted_order_kernel, exactly: draw i has the 53 bits (c0 >> 5) << 26 | (c1 >> 6) of the block (i, AUG_TAG | 4, epoch),
    x = bits * 2^-53 * cdf[-1] in fp64, and the kernel's binary search for the first row with cdf[row] > x, clamped to n - 1."""
    cdf = np.asarray(cdf, dtype=np.float64)
    n = len(cdf)
    w = aug_words(np.arange(m, dtype=np.uint64), AUG_ORDER, epoch, seed).astype(np.uint64)
    bits = ((w[:, 0] >> np.uint64(5)) << np.uint64(26)) | (w[:, 1] >> np.uint64(6))
    xs = bits.astype(np.float64) * 2.0 ** -53 * cdf[n - 1]
    lo, hi = np.zeros(m, np.int64), np.full(m, n - 1, np.int64)
    while np.any(lo < hi):
        act = lo < hi
        mid = (lo + hi) >> 1
        up = cdf[mid] > xs
        hi = np.where(act & up, mid, hi)
        lo = np.where(act & ~up, mid + 1, lo)
    return np.minimum(lo, n - 1)
