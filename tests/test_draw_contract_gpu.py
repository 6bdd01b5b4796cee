"""Every device random draw on the MI355X against the host restatement tests/draw_ref.py, word by word: mg_rng_fill (plain,
ticked, ticked with a staged batch), mg_gen_inputs, mg_eval_noise, mg_latent_rows, mg_stage_augment (both programs) and
mg_weighted_order.  (mg_mlp_cls_fwd_bwd's drawn masks are tied to mg_rng_fill's by tests/test_ed_latent_gpu.py,
test_drawn_masks_are_rng_fills_..., and through it to this file.)

Every destination lies between sentinel rows and starts as NaN (-1 for an order).  Uniforms, masks, gates, shifts, dropped
rows, sampler orders and step counters are compared bit for bit.  A normal v is compared with its fp64 reference under

    |dev - ref| <= (L/2 + S + C + 1/2) 2^-23 |ref| + 2^-23 r,   r = sqrt(-2 log u) <= 5.89

with L = 3, S = 3, C = 4: the ulp limits of log, sqrt and sin / cos of OpenCL's full profile (OpenCL C specification,
"Relative error as ULPs").  The ROCm toolchain installs no document or header that states limits for logf, sqrtf, cosf and
sinf, so the issue's fallback applies; draw_ref's docstring has the derivation.  These are worst-case limits: nothing is
added.  Where a kernel adds sigma * v to an exact fp32 value, the bound is |sigma| times the above plus the fp32 roundings of
the product and of the sum (draw_ref.stage_augment, draw_ref.gen_inputs).

Measured worst error / bound on the MI355X (printed by every test; a ratio above 1 fails):
    rng_fill normals      0.18       gen_inputs noise      0.14       gen_inputs numeric    0.33
    eval_noise            0.13       latent_rows           0.13       stage_augment ed      0.83
    stage_augment ae      0.79
The bare normals sit at a fifth of the bound or less (the library is better than its worst-case limits).  The two
stage_augment sections are near 1 by construction: there sigma * v (sigma <= 0.1) is added to a value of order 1, the bound
is dominated by the half ulp of that sum's rounding, and a correctly rounded sum uses all of it.

Against a library with one of these mistakes compiled in (a one-off check on a scratch copy, not kept), tests of this file
fail: 9 Philox rounds (41 of 55), the second key word bumped by the first one's constant (41), the high word of the step
counter dropped (4: the seeds-and-high-word cases and the ticked forms), sin and cos swapped (32), jid << 27 (21), the ED
row dropout's >= as > (3: the tie of test_stage_augment_ed), c0 >> 6 in the sampler (2).  Against the parent of the commit
that added this file 3 fail: the two open-interval cases (the device returned 1.0) and the tempo-factor test (the
compiler had contracted 1 + (2u - 1) * tempo_jitter into one fused multiply-add).

The open-interval test replays a draw whose Philox word has its top 24 bits all ones: seed 1234, step 8939, the uniform as the
second tensor, element 662 (word 0xffffff37), and step 13926, element 1074 (word 0xffffff21).  They were found by
draw_ref.find_unit_uniform(1234, range(16384), 512), a search over the host restatement of rng_fill_kernel's counters;
tests/test_draw_ref.py repeats the search around both.  Before u01 was clamped the device returned exactly 1.0 there.
"""
import numpy as np
import pytest
import torch

import draw_ref as D

pytestmark = pytest.mark.gpu

PAD = 64                        # sentinel elements on each side of a destination
SENT_F, SENT_I = -1.2345678e33, -0x5EA7135
WORST = {}


@pytest.fixture(scope="module")
def ops():
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import ops as _ops
    return _ops


class Dest:
    """A destination of `shape` inside a flat canvas with PAD sentinel elements on both sides, prefilled with NaN (-1)."""

    def __init__(self, shape, dtype=torch.float32):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = int(np.prod(shape))
        self.sent, fill = (SENT_F, float("nan")) if dtype == torch.float32 else (SENT_I, -1)
        self.canvas = torch.full((n + 2 * PAD,), self.sent, dtype=dtype, device="cuda")
        self.t = self.canvas[PAD:PAD + n].view(*shape)
        self.t.fill_(fill)

    def get(self, what):
        """The destination on the host, after the sentinels were found intact."""
        c = self.canvas.cpu()
        want = torch.tensor(self.sent, dtype=c.dtype)
        assert bool((c[:PAD] == want).all()) and bool((c[-PAD:] == want).all()), f"{what}: a sentinel was overwritten"
        return c[PAD:c.numel() - PAD].view(*self.t.shape).numpy()


def i64(v):
    """A device uint64 scalar in an int64 tensor (values from 2^63 on wrap)."""
    v &= D.M64
    return torch.tensor([v - (1 << 64) if v >> 63 else v], dtype=torch.int64, device="cuda")


def same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    view = np.int32 if got.dtype == np.float32 else got.dtype
    bad = np.flatnonzero(got.view(view).reshape(-1) != ref.view(view).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} elements differ, first at {bad[0]}: " \
                          f"{got.reshape(-1)[bad[0]]!r} != {ref.reshape(-1)[bad[0]]!r}"


def within(got, ref, bound, what, section):
    """|got - ref| <= bound element by element; where bound == 0 that is equality.  Records the worst ratio of the section."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), f"{what}: shape {got.shape} vs {ref.shape}, or a NaN left"
    err = np.abs(got - ref)
    live = bound > 0
    ratio = float((err[live] / bound[live]).max()) if live.any() else 0.0
    WORST[section] = max(WORST.get(section, 0.0), ratio)
    bad = np.flatnonzero((err > bound).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} elements out of bound, worst ratio {ratio:.3g}, first at {bad[0]}: " \
                          f"{got.reshape(-1)[bad[0]]!r} vs {ref.reshape(-1)[bad[0]]!r}"
    return ratio


def report(section):
    print(f"{section}: worst error / bound = {WORST.get(section, 0.0):.3f}")


# ---- mg_rng_fill ------------------------------------------------------------------------------------------------------------
RNG_LENGTHS = [1, 2, 3, 5, 1023, 1024, 1025, 262144, 262149]    # 262149: a second grid-stride pass with a ragged tail
NAMES = ("normal", "uniform", "mask0", "mask1")


def rng_call(ops, lengths, p_drop, seed, ctr, **riders):
    """One mg_rng_fill into guarded destinations; lengths: (normal, uniform, mask0, mask1), None = absent.  Returns the
    host copies by name."""
    dests = [None if not n else Dest(n) for n in lengths]
    ops.rng_fill(*[None if d is None else d.t for d in dests], p_drop, seed, ctr, **riders)
    torch.cuda.synchronize()
    return {nm: d.get(f"rng_fill {nm}") for nm, d in zip(NAMES, dests) if d is not None}


def rng_check(got, lengths, p_drop, seed, step, what):
    ref = D.rng_fill(*lengths, p_drop, seed, step)
    assert set(got) == set(ref)
    for nm in got:
        if nm == "normal":
            within(got[nm], ref[nm][0], ref[nm][1], f"{what} normal", "rng_fill normals")
        else:
            same_bits(got[nm], ref[nm], f"{what} {nm}")
    return ref


@pytest.mark.parametrize("i", range(len(RNG_LENGTHS)), ids=[f"n{n}" for n in RNG_LENGTHS])
def test_rng_fill_lengths(ops, i):
    """All four tensors, each of another length: the normal has RNG_LENGTHS[i], the uniform the next of the list, and so on
    round the list -- every length meets every kind, and in most cases the longest tensor (which sizes the grid) is not the
    first."""
    lengths = tuple(RNG_LENGTHS[(i + j) % len(RNG_LENGTHS)] for j in range(4))
    ctr = i64(41)
    got = rng_call(ops, lengths, 0.2, 7, ctr)
    assert int(ctr.item()) == 42
    rng_check(got, lengths, 0.2, 7, 41, f"lengths {lengths}")
    report("rng_fill normals")


@pytest.mark.parametrize("lengths", [(None, 1025, None, None), (None, None, 1025, 37), (1025, None, None, 37), (37, 1025, None, 5)],
                         ids=["uniform", "masks", "normal+mask1", "no-mask0"])
def test_rng_fill_stream_id_is_the_place_among_the_present(ops, lengths):
    ctr = i64(3)
    got = rng_call(ops, lengths, 0.2, 7, ctr)
    rng_check(got, lengths, 0.2, 7, 3, f"subset {lengths}")
    report("rng_fill normals")


@pytest.mark.parametrize("seed", [7, 0x100000007, (1 << 64) - 1], ids=["7", "hi-word", "all-ones"])
def test_rng_fill_seeds_and_the_step_high_word(ops, seed):
    lengths = (261, 130, 67, 1030)
    ctr = i64(0)
    got = rng_call(ops, lengths, 0.2, seed, ctr)
    assert int(ctr.item()) == 1
    first = rng_check(got, lengths, 0.2, seed, 0, f"seed {seed:#x} step 0")
    ctr = i64((1 << 32) - 1)
    got = rng_call(ops, lengths, 0.2, seed, ctr)
    assert int(ctr.item()) == 1 << 32                      # advanced by exactly 1, with the carry
    rng_check(got, lengths, 0.2, seed, (1 << 32) - 1, f"seed {seed:#x} step 2^32 - 1")
    got = rng_call(ops, lengths, 0.2, seed, ctr)
    assert int(ctr.item()) == (1 << 32) + 1
    at_carry = rng_check(got, lengths, 0.2, seed, 1 << 32, f"seed {seed:#x} step 2^32")
    assert not np.array_equal(first["uniform"], at_carry["uniform"])        # a dropped high word would repeat step 0
    report("rng_fill normals")


@pytest.mark.parametrize("p", [0.0, 0.2, 0.5])
def test_rng_fill_masks(ops, p):
    lengths = (None, 5, 4099, 1025)
    got = rng_call(ops, lengths, p, 11, i64(2))
    rng_check(got, lengths, p, 11, 2, f"p_drop {p}")
    sc = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    for nm in ("mask0", "mask1"):
        vals = np.unique(got[nm])
        assert vals.tolist() == ([float(sc)] if p == 0 else [0.0, float(sc)]), (nm, vals)


def test_rng_fill_mask_keeps_the_tie(ops):
    """An element is kept when its uniform >= p_drop: with p_drop set to the uniform of one element, that element is kept."""
    lengths, seed, step, e = (None, 5, 4099, 1025), 11, 2, 41
    p = float(D.u01(D.rng_fill_words(e // 4, 1, seed, step)[e % 4]))      # mask0 is the second tensor present
    assert 0.0 < p < 1.0 and float(np.float32(p)) == p
    got = rng_call(ops, lengths, p, seed, i64(step))
    ref = rng_check(got, lengths, p, seed, step, "the tie")
    assert got["mask0"][e] == ref["mask0"][e] != 0.0


def test_rng_fill_ticked_forms_draw_the_plain_bits(ops):
    lengths = (1025, 262, 67, 1030)
    betas = (0.5, 0.9)
    step = (1 << 32) + 5
    plain = rng_call(ops, lengths, 0.2, 7, i64(step))
    rng_check(plain, lengths, 0.2, 7, step, "plain")
    ctr, state = i64(step), torch.zeros(4, dtype=torch.float64, device="cuda")
    ticked = rng_call(ops, lengths, 0.2, 7, ctr, tick_state=state, betas=betas)
    assert int(ctr.item()) == step and state.tolist() == [1.0, float(np.float32(0.5)), float(np.float32(0.9)), 0.0]
    # ... and with a second state and a staged batch riding in the launch
    src = torch.arange(16 * 4, dtype=torch.float32, device="cuda").reshape(16, 4)
    staged = Dest((8, 4))
    state2, base = torch.zeros(4, dtype=torch.float64, device="cuda"), i64(step - 1)
    both = rng_call(ops, lengths, 0.2, 7, ctr, tick_state=state, betas=betas, tick_state2=state2,
                    stage=([(src, staged.t)], 8, None, 16, base))
    assert int(ctr.item()) == step and state[0].item() == 2.0 and state2[0].item() == 1.0
    same_bits(staged.get("staged rows"), src[8:16].cpu().numpy(), "staged rows")      # batch 1 of 8 rows
    for nm in NAMES:
        same_bits(ticked[nm], plain[nm], f"ticked {nm}")
        same_bits(both[nm], plain[nm], f"ticked + staged {nm}")


@pytest.mark.parametrize("step,element,word", [(8939, 662, 0xFFFFFF37), (13926, 1074, 0xFFFFFF21)])
def test_uniform_stays_inside_the_open_interval(ops, step, element, word):
    """The draw whose 24 bits are all ones (see the module docstring for where the coordinates come from)."""
    assert int(D.rng_fill_words(element // 4, 1, 1234, step)[element % 4]) == word
    lengths = (8, 2048, None, None)
    got = rng_call(ops, lengths, 0.2, 1234, i64(step))
    u = got["uniform"]
    print(f"uniform[{element}] = {float(u[element])!r}, max {float(u.max())!r}, min {float(u.min())!r}")
    assert float(u[element]) < 1.0 and float(u.max()) < 1.0 and float(u.min()) > 0.0
    assert u[element] == D.U01_MAX == D.u01(word)
    rng_check(got, lengths, 0.2, 1234, step, f"step {step}")


# ---- mg_gen_inputs ----------------------------------------------------------------------------------------------------------
EMOTIONS = [0, 2, -1, 1, 2]             # row 2 is padding
SAMPLES = [0, (1 << 31) - 1, 9, -7, 0]  # a negative sample is the word sample & 0xffffffff


def gen_call(ops, noise_dim, num_dim, table, jitter, seed, latent_dim=5):
    rows = len(EMOTIONS)
    noise, numeric, latent = Dest((rows, noise_dim)), Dest((rows, num_dim)), Dest((rows, latent_dim))
    em = torch.tensor(EMOTIONS, dtype=torch.int32, device="cuda")
    sa = torch.tensor(SAMPLES, dtype=torch.int32, device="cuda")
    ops.gen_inputs(em, sa, noise.t, numeric.t, torch.from_numpy(table).cuda(), jitter, latent.t, seed)
    torch.cuda.synchronize()
    lat = latent.get("latent")
    same_bits(lat, np.zeros_like(lat), "latent")
    return noise.get("noise"), numeric.get("numeric")


@pytest.mark.parametrize("num_dim", [3, 8])
@pytest.mark.parametrize("noise_dim", [1, 6, 100, 260])        # 260: more than 64 lanes x 4 elements
def test_gen_inputs_normals(ops, noise_dim, num_dim):
    seed = 0x2000000AB
    table = np.zeros((3, num_dim), np.float32)
    noise, numeric = gen_call(ops, noise_dim, num_dim, table, 1.0, seed)
    ref = D.gen_inputs(EMOTIONS, SAMPLES, noise_dim, num_dim, table, 1.0, seed)
    within(noise, *ref["noise"], "noise", "gen_inputs noise")
    within(numeric, *ref["jitter"], "numeric (zero table, jitter 1)", "gen_inputs numeric")
    assert not noise[2].any() and not numeric[2].any() and noise[[0, 1, 3, 4]].all()
    assert not np.array_equal(noise[1], noise[4]) and not np.array_equal(numeric[1], numeric[4])      # same emotion, other sample
    report("gen_inputs noise")
    report("gen_inputs numeric")


def test_gen_inputs_table_and_jitter(ops):
    seed, num_dim = 5, 8
    table = (np.arange(3 * num_dim, dtype=np.float32).reshape(3, num_dim) - 7.25) / np.float32(3.0)
    noise, numeric = gen_call(ops, 100, num_dim, table, 0.15, seed)
    ref = D.gen_inputs(EMOTIONS, SAMPLES, 100, num_dim, table, 0.15, seed)
    within(noise, *ref["noise"], "noise", "gen_inputs noise")
    within(numeric, *ref["numeric"], "numeric", "gen_inputs numeric")
    report("gen_inputs numeric")


# ---- mg_eval_noise ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 3, 1 << 30], ids=["k0", "k3", "k2^30"])      # 2^30 batches of 4 rows: i >= 2^32
@pytest.mark.parametrize("noise_dim", [6, 100, 260])
def test_eval_noise(ops, noise_dim, k):
    rows, base, seed = 4, 11, 0x300000011
    n = k * rows + 2                                    # the last two rows are padding
    noise = Dest((rows, noise_dim))
    ops.eval_noise(noise.t, i64(base + k), i64(base), n, seed)
    torch.cuda.synchronize()
    got = noise.get("eval noise")
    within(got, *D.eval_noise(rows, noise_dim, k, n, seed), f"eval_noise k {k}", "eval_noise")
    assert got[:2].all() and not got[2:].any()
    report("eval_noise")


# ---- mg_latent_rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [6, 64, 260])
def test_latent_rows_prior_normals(ops, L):
    keys = [(0, 0), (5, 3), (-2, 7), (3, -1), (5, 4)]
    rows, seed = len(keys) + 1, 0x40000000D
    dev = lambda v, dt: torch.tensor(v, dtype=dt, device="cuda")       # noqa: E731
    kind = dev([1] * len(keys) + [0], torch.int32)                      # the last row is padding
    zero_i, zero_f = dev([0] * rows, torch.int32), dev([0.0] * rows, torch.float32)
    z = Dest((rows, L))
    ops.latent_rows(None, None, None, kind, zero_i, zero_i, zero_f, dev([-1] * rows, torch.int32), zero_f,
                    dev([1.0] * rows, torch.float32), dev(keys + [(9, 9)], torch.int32), z.t, interp=0, seed=seed)
    torch.cuda.synchronize()
    got = z.get("latent rows")
    ref, bound = D.latent_prior(keys, L, seed)
    within(got[:-1], ref, bound, "latent_rows", "latent_rows")
    assert not got[-1].any() and got[:-1].all()
    report("latent_rows")


# ---- mg_stage_augment -------------------------------------------------------------------------------------------------------
STAGE_SHAPES = [(4, 37, 5), (128, 37, 3), (4, 1100, 2)]         # (C, T, batch rows); T * C / 4 = 1100 crosses the 1024-piece block
SRC_ROWS = 7
ORDER = [3, 6, 1, 0, 5, 2, 4]
WRAP_BATCH = {5: 1, 3: 2, 2: 3}                                  # batch number whose rows wrap round the end of the order
SERIAL_BASE = (1 << 32) - 2                                      # the rows straddle the carry into the serial's high word
ED_ALL = dict(noise_std=0.05, dropout_prob=0.3, pitch_shift_prob=0.5)
AE_ALL = dict(tempo_jitter=0.07, pitch_shift=2, note_dropout=0.25, velocity_jitter=0.1, timing_jitter=0.02)


def stage_source(C, T):
    rng = np.random.default_rng(C * 10007 + T)
    x = (rng.random((SRC_ROWS, T, C), dtype=np.float32) * np.float32(2) - np.float32(1)).astype(np.float32)
    x[:, :, 1] = np.abs(x[:, :, 1]) * np.float32(0.05)         # onsets near 0: the timing jitter's max(., 0) clips some
    return x


def stage_positions(n, last):
    return [D.stage_position(r, n, ORDER, SRC_ROWS, WRAP_BATCH[n], last)[0] for r in range(n)]


def ae_seed(n):
    """The first seed under which, by the host reference, each of the five AE gates fires in at least one row of the wrapped
    batch and fails in at least one, and a fired pitch gate draws a shift other than 0."""
    serials = [SERIAL_BASE + p for p in stage_positions(n, False)]
    for seed in range(1, 100000):
        got = [D.ae_gates(s, seed) for s in serials]
        g = [r[0] for r in got]
        if all(any(r[k] for r in g) and not all(r[k] for r in g) for k in D.AE_GATE_ODDS) and \
                any(r[0]["pitch"] and int(D.randint_shift(r[2][2], AE_ALL["pitch_shift"])) != 0 for r in got):
            return seed
    raise AssertionError("no such seed")


def stage_check(ops, x, program, seed, params, n, last, section, order=ORDER, k=None):
    C, src_rows = x.shape[2], x.shape[0]
    labels = torch.arange(100, 100 + src_rows, dtype=torch.int64, device="cuda")
    out, lab = Dest((n,) + x.shape[1:]), Dest(n, torch.int64)
    k = WRAP_BATCH[n] if k is None else k
    order_dev = None if order is None else torch.tensor(order, dtype=torch.int64, device="cuda")
    ops.stage_augment(torch.from_numpy(x).cuda(), labels, out.t, lab.t, n, order_dev, src_rows, i64(20 + k), i64(20),
                      i64(SERIAL_BASE), ops.augment_spec(program, seed, **params), last=last)
    torch.cuda.synchronize()
    got, got_lab = out.get("staged notes"), lab.get("staged labels")
    exact, ref, bound, info = D.stage_augment(x, program, seed, params, n, order, src_rows, k=k, serial_base=SERIAL_BASE, last=last)
    what = f"{program} C {C} {'last' if last else 'batch'} {sorted(params)}"
    assert got_lab.tolist() == [100 + row["src"] for row in info], what
    assert got.dtype == np.float32
    loose = bound > 0
    same_bits(np.where(loose, np.float32(0), got), np.where(loose, np.float32(0), exact), what)      # every element without a normal
    within(got, ref, bound, what, section)
    assert not loose[:, :, 4:].any() and not loose[:, :, 0].any()
    return info, loose


@pytest.mark.parametrize("C,T,n", STAGE_SHAPES)
def test_stage_augment_ed(ops, C, T, n):
    x = stage_source(C, T)
    pos = stage_positions(n, False)
    assert pos != sorted(pos) and min(SERIAL_BASE + p for p in pos) < 1 << 32 <= max(SERIAL_BASE + p for p in pos)
    seed = 0x500000000 + 17
    for params in [dict(noise_std=0.05), dict(dropout_prob=0.3), dict(pitch_shift_prob=0.5), ED_ALL]:
        for last in (False, True):
            info, loose = stage_check(ops, x, "ed", seed, params, n, last, "stage_augment ed")
            if "noise_std" in params and "dropout_prob" not in params:
                assert loose[:, :, 1:4].all()
            if "dropout_prob" in params and not last:
                d = np.stack([row["dropped"] for row in info])
                assert d.any() and not d.all()
    # the tie: a time row is dropped when !(u >= p), so with p set to the uniform of one time row that row is kept
    t0 = T // 2
    p = float(D.u01(D.aug_words(t0, D.AUG_DROP, SERIAL_BASE + pos[0], seed)[0]))
    info, _ = stage_check(ops, x, "ed", seed, dict(dropout_prob=p), n, False, "stage_augment ed")
    assert not info[0]["dropped"][t0] and float(np.float32(p)) == p
    shifts = {row["shift"] for row in D.stage_augment(x, "ed", seed, ED_ALL, SRC_ROWS)[3]}
    assert shifts == {0.0, 1.0, -1.0}               # under this seed the reference itself takes all three branches
    report("stage_augment ed")


@pytest.mark.parametrize("C,T,n", STAGE_SHAPES)
def test_stage_augment_ae(ops, C, T, n):
    x = stage_source(C, T)
    seed = ae_seed(n)
    gates = [D.ae_gates(SERIAL_BASE + p, seed)[0] for p in stage_positions(n, False)]
    for name in D.AE_GATE_ODDS:                     # asserted on the reference: every gate fires in a row and fails in a row
        assert any(g[name] for g in gates) and not all(g[name] for g in gates), (name, seed)
    for params in [dict(tempo_jitter=0.07), dict(pitch_shift=2), dict(note_dropout=0.25), dict(velocity_jitter=0.1),
                   dict(timing_jitter=0.02), AE_ALL]:
        for last in (False, True):
            info, loose = stage_check(ops, x, "ae", seed, params, n, last, "stage_augment ae")
            if not last:
                assert [row["gates"] for row in info] == gates
                if "tempo_jitter" in params:
                    assert any(row["factor"] != 1.0 for row in info)
                if "pitch_shift" in params:
                    assert any(row["shift"] != 0.0 for row in info)
                if "note_dropout" in params:
                    assert any(0 < row["dropped"].sum() < T for row in info)
                if "velocity_jitter" in params:
                    assert [bool(m[:, 3].all()) for m in loose] == [g["velocity"] for g in gates]
                if "timing_jitter" in params:
                    assert [bool(m[:, 1].all()) for m in loose] == [g["timing"] for g in gates]
    # the tie: this program drops a time row when !(u > p), so with p set to the uniform of one time row that row is dropped
    r0, t0 = [g["drop"] for g in gates].index(True), T // 2
    p = float(D.u01(D.aug_words(t0, D.AUG_DROP, SERIAL_BASE + stage_positions(n, False)[r0], seed)[0]))
    info, _ = stage_check(ops, x, "ae", seed, dict(note_dropout=p), n, False, "stage_augment ae")
    assert info[r0]["dropped"][t0] and float(np.float32(p)) == p
    report("stage_augment ae")


def test_stage_augment_ae_tempo_factor_rounds_its_product_and_its_sum(ops):
    """The tempo factor 1 + (2u - 1) * tempo_jitter is two fp32 roundings, not one fused multiply-add.  The two differ for
    about one factor in fifty, so 1024 small samples are staged and the reference is asked that some of them tell the two
    apart (a compiler contracted the expression once; the kernel now forbids it)."""
    rng = np.random.default_rng(3)
    x = (rng.random((1024, 3, 4), dtype=np.float32) + np.float32(0.5)).astype(np.float32)
    info, _ = stage_check(ops, x, "ae", 71, dict(tempo_jitter=0.07), 1024, False, "stage_augment ae", order=None, k=0)
    fired = [row for row in info if row["gates"]["tempo"]]
    telling = [row for row in fired if row["fused_differs"]]
    print(f"{len(fired)} of 1024 samples scaled; a fused multiply-add would give another factor for {len(telling)} of them")
    assert len(fired) > 200 and len(telling) >= 5


# ---- mg_weighted_order ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 7, 1000])
def test_weighted_order(ops, n):
    rng = np.random.default_rng(n)
    w = rng.integers(0, 4, n).astype(np.float64)        # zeros among the weights: flat segments of the cdf, never chosen
    w[0], w[-1] = 0.0, 1.0                              # a zero first weight (n = 1: the single row has weight 1)
    if n >= 7:
        w[3:6] = 0.0
    cdf = np.cumsum(w)
    for m in (1, 255, 257, 1000):
        for epoch in (0, 5, (1 << 32) + 1):
            order = Dest(m, torch.int64)
            ops.weighted_order(torch.from_numpy(cdf).cuda(), order.t, 0x600000000 + 29, epoch)
            torch.cuda.synchronize()
            got = order.get("order")
            ref = D.weighted_order(cdf, m, 0x600000000 + 29, epoch)
            same_bits(got, ref, f"weighted_order n {n} m {m} epoch {epoch}")
            assert (w[got] > 0).all()
