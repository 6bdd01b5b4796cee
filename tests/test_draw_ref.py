"""The host restatement of the device random draws (tests/draw_ref.py) held to things that do not depend on this project:
the Random123 known answers of Philox4x32-10, the range of u01, the disjointness of the counter layouts, and the statistics
of its own Box-Muller, randint and sampler.  No GPU.

Statistical bounds are 5 standard errors from the sample size, as tests/test_augment_gpu.py writes them: 5/sqrt(N) for the
mean of unit draws, 5/sqrt(2N) for their standard deviation, 5 sqrt(96/N) for their fourth moment (Var z^4 = 105 - 9)."""
import math

import numpy as np

import draw_ref as D


def hexwords(w):
    return " ".join(f"{int(x):08x}" for x in np.asarray(w).reshape(-1))


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    assert hexwords(D.philox4x32_10(0, 0, 0, 0, 0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    f = 0xFFFFFFFF
    assert hexwords(D.philox4x32_10(f, f, f, f, f, f)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    got = D.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)
    assert hexwords(got) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # vectorised: the three at once, and the key taken from a 64-bit seed as the kernels take it
    c = np.array([[0, 0, 0, 0], [f, f, f, f], [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]], dtype=np.uint64)
    k = np.array([[0, 0], [f, f], [0xA4093822, 0x299F31D0]], dtype=np.uint64)
    got = D.philox4x32_10(c[:, 0], c[:, 1], c[:, 2], c[:, 3], k[:, 0], k[:, 1])
    assert hexwords(got[2]) == "d16cfe09 94fdcceb 5001e420 24126ea1" and hexwords(got[0]) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert hexwords(D.keyed(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0x299F31D0A4093822)) == hexwords(got[2])


def test_philox_is_not_one_of_its_neighbours():
    """What a wrong generator would give for the third known answer differs from it: nine rounds, swapped multipliers, the
    second key word bumped by the first one's constant."""
    right = D.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)
    saved = D.PHILOX_M0, D.PHILOX_M1, D.PHILOX_W1
    try:
        D.PHILOX_M0, D.PHILOX_M1 = saved[1], saved[0]
        assert hexwords(D.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)) != hexwords(right)
        D.PHILOX_M0, D.PHILOX_M1, D.PHILOX_W1 = saved[0], saved[1], D.PHILOX_W0
        assert hexwords(D.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)) != hexwords(right)
    finally:
        D.PHILOX_M0, D.PHILOX_M1, D.PHILOX_W1 = saved


def test_u01_range_and_bits():
    words = np.array([0, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000, 0xFFFFFEFF, 0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint64)
    u = D.u01(words)
    assert u.dtype == np.float32
    assert float(u.min()) >= 2.0 ** -25 and float(u.max()) <= 1.0 - 2.0 ** -24
    # from k = 2^23 on, k + 0.5 is a tie between two fp32 numbers and rounds to the even one: k itself when k is even
    want = [2.0 ** -25, 2.0 ** -25, 1.5 * 2.0 ** -24, 0.5 - 2.0 ** -25, 0.5, 1.0 - 2.0 ** -23,
            1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24]
    assert u.astype(np.float64).tolist() == want
    # the tie the clamp is there for: without it the last two words give 1.0
    raw = (np.float32(0xFFFFFF) + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert float(raw) == 1.0
    assert float(D.U01_MIN) == 2.0 ** -25 and float(D.U01_MAX) == 1.0 - 2.0 ** -24


def test_unit_uniform_coordinates():
    """The draws tests/test_draw_contract_gpu.py replays: under seed 1234 with the uniform as the second tensor (jid 1), the
    words of step 8939 / element 662 and step 13926 / element 1074 have their top 24 bits all ones."""
    hits = D.find_unit_uniform(1234, range(8900, 8960), 256) + D.find_unit_uniform(1234, range(13900, 13960), 512)
    assert (8939, 662, 0xFFFFFF37) in hits and (13926, 1074, 0xFFFFFF21) in hits
    ref = D.rng_fill(8, 1001, None, None, 0.0, 1234, 8939)["uniform"]
    assert float(ref[662]) == 1.0 - 2.0 ** -24 and float(ref.max()) < 1.0 and float(ref.min()) > 0.0


def test_counter_layouts_are_pairwise_disjoint():
    """Counter word 1 tells the five layouts apart (the claim in the comments of small_kernels.hip, eval_metrics.hip and
    latent_edit.hip): for jid < 4, q < 2^32, which < 2, need < 5 the word-1 ranges do not meet."""
    rg = D.word1_ranges()
    assert set(rg) == {"rng_fill", "gen", "aug", "eval", "lat"}
    assert rg["rng_fill"] == (0, 0x30000000) and rg["rng_fill"][1] < 0x40000000
    assert rg["gen"] == (0x47454E00, 0x47454E01) and rg["aug"] == (0x41554700, 0x41554704)
    assert rg["eval"] == (0x4556414C, 0x4556414C) and rg["lat"] == (0x4C415400, 0x4C415400)
    names = sorted(rg)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert rg[a][1] < rg[b][0] or rg[b][1] < rg[a][0], (a, b)
    # and the builders place what they are given where the header says
    c = D.rng_fill_counter((5 << 32) | 9, 3, (7 << 32) | 11)
    assert [int(x) for x in c] == [9, 5 ^ (3 << 28), 11, 7]
    assert [int(x) for x in D.gen_counter(2, 1, 3, -5)] == [2, 0x47454E01, 3, 0xFFFFFFFB]
    assert [int(x) for x in D.aug_counter(6, 2, (1 << 32) | 4)] == [6, 0x41554702, 4, 1]
    assert [int(x) for x in D.eval_counter(1, (3 << 32) | 2)] == [1, 0x4556414C, 2, 3]
    assert [int(x) for x in D.lat_counter(1, -2, 8)] == [1, 0x4C415400, 0xFFFFFFFE, 8]


def test_box_muller_statistics():
    nb = 1 << 18                                    # 2^20 words, 2^20 normals
    w = D.rng_fill_words(np.arange(nb, dtype=np.uint64), 0, 99, 3)
    z, b = D.normals(w)
    assert z.shape == (nb, 4) and np.isfinite(z).all()
    N = z.size
    m, s, k = z.mean(), z.std(), (z ** 4).mean()
    print(f"mean {m:+.6f} (bound {5 / math.sqrt(N):.6f}) std {s:.6f} (1 +- {5 / math.sqrt(2 * N):.6f}) "
          f"m4 {k:.5f} (3 +- {5 * math.sqrt(96 / N):.5f})")
    assert abs(m) <= 5 / math.sqrt(N) and abs(s - 1) <= 5 / math.sqrt(2 * N) and abs(k - 3) <= 5 * math.sqrt(96 / N)
    for e in range(4):                              # each of the four positions on its own, and no pair correlated
        assert abs(z[:, e].mean()) <= 5 / math.sqrt(nb) and abs(z[:, e].std() - 1) <= 5 / math.sqrt(2 * nb)
    cc = np.corrcoef(z.T)
    assert np.abs(cc - np.eye(4)).max() <= 5 / math.sqrt(nb)
    # the bound is what the docstring says: below 9.5 ulp of 6 at the very worst
    assert float(b.max()) <= (D.NORMAL_REL + D.NORMAL_FLOOR) * 5.89 and D.NORMAL_REL == 9 * 2.0 ** -23
    # (r cos t)^2 + (r sin t)^2 = -2 log u: the pairs are (c0, c1) and (c2, c3)
    u = D.u01(w).astype(np.float64)
    assert np.allclose(z[:, 0] ** 2 + z[:, 1] ** 2, -2 * np.log(u[:, 0]), rtol=1e-12)
    assert np.allclose(z[:, 2] ** 2 + z[:, 3] ** 2, -2 * np.log(u[:, 2]), rtol=1e-12)
    t = 2 * math.pi * u[:, 1]
    assert np.allclose(np.arctan2(z[:, 1], z[:, 0]) % (2 * math.pi), t % (2 * math.pi), atol=1e-6)


def test_randint_covers_both_ends():
    for p in (1, 2, 12):
        assert int(D.randint_shift(0, p)) == -p and int(D.randint_shift(0xFFFFFFFF, p)) == p
        w = D.aug_words(0, D.AUG_GATES2, np.arange(20000, dtype=np.uint64), 5)[:, 2]
        d = D.randint_shift(w, p)
        vals, counts = np.unique(d, return_counts=True)
        assert vals.tolist() == list(range(-p, p + 1))
        q = 1.0 / (2 * p + 1)
        assert np.abs(counts / d.size - q).max() <= 5 * math.sqrt(q * (1 - q) / d.size)


def test_tempo_factor_and_its_fused_neighbour():
    tj = np.float32(0.07)
    words = D.aug_words(0, D.AUG_GATES2, np.arange(2000, dtype=np.uint64), 9)[:, 1]
    got = [D.ae_tempo_factor(w, tj) for w in words]
    f = np.array([g[0] for g in got], dtype=np.float64)
    assert f.min() >= 1 - float(tj) - 2.0 ** -24 and f.max() <= 1 + float(tj) + 2.0 ** -23 and f.min() < 0.94 and f.max() > 1.06
    share = np.mean([g[1] for g in got])
    assert 0.01 < share < 0.25                                  # a fused multiply-add gives another float now and then
    # where the two agree, the float64 evaluation (exact product, sum rounded at 2^-53) rounds to the same float32
    d = 2.0 * D.u01(words).astype(np.float64) - 1.0
    f64 = (1.0 + d * float(tj)).astype(np.float32)
    agree = np.array([not g[1] for g in got])
    assert np.array_equal(f64[agree], f[agree].astype(np.float32))


def test_weighted_order_reference():
    w = np.array([0.0, 1.0, 0.0, 0.0, 2.0, 1.0, 0.0], dtype=np.float64)
    cdf = np.cumsum(w)
    o = D.weighted_order(cdf, 40000, 3, 1)
    assert set(np.unique(o).tolist()) == {1, 4, 5}          # zero-weight rows, the first one included, are never chosen
    for row, q in ((1, 0.25), (4, 0.5), (5, 0.25)):
        assert abs((o == row).mean() - q) <= 5 * math.sqrt(q * (1 - q) / o.size)
    # the kernel's binary search is "first row whose prefix sum exceeds x", clamped
    wd = D.aug_words(np.arange(o.size, dtype=np.uint64), D.AUG_ORDER, 1, 3).astype(np.uint64)
    bits = ((wd[:, 0] >> np.uint64(5)) << np.uint64(26)) | (wd[:, 1] >> np.uint64(6))
    assert int(bits.max()) < 1 << 53
    x = bits.astype(np.float64) * 2.0 ** -53 * cdf[-1]
    assert np.array_equal(o, np.minimum(np.searchsorted(cdf, x, side="right"), len(cdf) - 1))
    assert np.array_equal(D.weighted_order(np.array([0.5]), 9, 3, 1), np.zeros(9, np.int64))
    assert not np.array_equal(D.weighted_order(cdf, 64, 3, 1), D.weighted_order(cdf, 64, 3, (1 << 32) + 1))


def test_stage_augment_reference_switches():
    """With every parameter 0 the reference is a plain gather; each program's dropped rows are whole rows of zeros; only the
    columns that receive a normal carry a bound."""
    rng = np.random.default_rng(0)
    x = (rng.random((7, 9, 8), dtype=np.float32) * 2 - 1).astype(np.float32)
    order = np.array([3, 1, 6, 0, 5, 2, 4])
    for prog in ("ed", "ae"):
        ex, ref, b, info = D.stage_augment(x, prog, 5, {}, 4, order, 7, k=1)
        assert np.array_equal(ex.view(np.int32), x[order[[4, 5, 6, 0]]].view(np.int32)) and not b.any()
        assert [row["pos"] for row in info] == [4, 5, 6, 0]
    ex, ref, b, info = D.stage_augment(x, "ed", 5, dict(noise_std=0.1, dropout_prob=0.5, pitch_shift_prob=1.0), 5, order, 7, last=True)
    assert [row["pos"] for row in info] == [2, 3, 4, 5, 6]
    for r, row in enumerate(info):
        d = row["dropped"]
        assert 0 < d.sum() < d.size or d.size < 4
        assert (ex[r][d][:, 1:] == 0).all() and (np.abs(ex[r][d][:, 0]) == 1).all() and not b[r][d].any()
        assert (b[r][~d][:, 1:4] > 0).all() and not b[r][:, 4:].any() and not b[r][:, 0].any()
    ex, ref, b, info = D.stage_augment(x, "ae", 5, dict(velocity_jitter=0.1, timing_jitter=0.1, note_dropout=0.5), 7)
    for r, row in enumerate(info):
        g = row["gates"]
        assert bool(b[r][:, 3].all()) == g["velocity"] and bool(b[r][:, 1].all()) == g["timing"]
        assert not b[r][:, [0, 2, 4, 5, 6, 7]].any()
        if g["timing"]:
            assert (ref[r][:, 1] >= 0).all()                    # max(., 0)
        d = row["dropped"]
        assert d.any() == g["drop"] and (ex[r][d][:, [0, 2, 4, 5, 6, 7]] == 0).all()
    assert any(row["gates"]["velocity"] for row in info) and not all(row["gates"]["velocity"] for row in info)
