"""The stride-2 five-tap family pinned to fp64, element by element (tests/stride2_ref.py: the reference and its bound).

conv16 (csrc/conv16_mfma.hip) has eight instantiations conv16_kernel<TR2, RT, RID>; pick_rt chooses RT per shape, so
every case here forces it (MG_CONV16_RT) and asserts, through ops.set_launch_hook, which symbol ran.  Each instantiation
meets the edge shapes (smallest Tm, partial last time tiles with n_ttiles >= 3, ragged batch groups, an odd number of
16-channel chunks, B = 193 through the batch / tile decode), the fused epilogue and the riders, with NaN-prefilled
outputs inside sentinel rows.  The window-GEMM fallback the engine would otherwise take must pass the same bound; the
domain boundary of conv16_supported is swept; every conv16 signature the cfg2 engine launches in its production flows
is recorded and replayed under both tile sizes; and the stride-2 weight gradient (wgrad_multi_kernel<2,5>) is held to
fp64 under single-slice through maximum-slice plans, with and without a second segment."""
import contextlib
import random

import pytest
import torch

import stride2_ref as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import ops as o
    return o


class _Symbols:
    def __init__(self):
        self.seen = []

    def __call__(self, sym, flops, launch=None):
        self.seen.append(sym)
        return contextlib.nullcontext()


@pytest.fixture
def hook(ops):
    rec = _Symbols()
    ops.set_launch_hook(rec)
    try:
        yield rec
    finally:
        ops.set_launch_hook(None)


def sym(tr2, rt, rid):
    b = lambda v: "true" if v else "false"  # noqa: E731
    return f"conv16_kernel<{b(tr2)},{rt},{b(rid)}>"


INSTANCES = [(tr2, rt, rid) for tr2 in (False, True) for rt in (1, 2) for rid in (False, True)]
INSTANCE_IDS = [sym(*i) for i in INSTANCES]


def rnd(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def tout_of(transposed, Tin, odd):
    return (2 * Tin - (1 if odd else 0)) if transposed else S.tm_gather(Tin)


class Problem:
    """Random x, w of one conv16 shape, the WQ image of w, and the fp64 reference of the window sum."""

    def __init__(self, ops, transposed, B, Tin, Cin, N, odd=False, seed=0):
        self.transposed, self.B, self.Tin, self.Cin, self.N, self.odd = transposed, B, Tin, Cin, N, odd
        self.Tout = tout_of(transposed, Tin, odd)
        self.x = rnd(B, Tin, Cin, seed=seed)
        self.wq = torch.empty(N * Cin * 5, device="cuda")
        if transposed:      # (Cin, N, 5): ConvTranspose1d forward / Conv1d data gradient
            self.w = rnd(Cin, N, 5, seed=seed + 1, scale=0.05)
            ops.wq_relayout(self.w, self.wq, N, Cin, 5, 5, N * 5)
            self.acc = S.scatter(self.x, self.w, self.Tout)
        else:               # (N, Cin, 5): Conv1d forward / ConvTranspose1d data gradient
            self.w = rnd(N, Cin, 5, seed=seed + 1, scale=0.05)
            ops.wq_relayout(self.w, self.wq, N, Cin, 5, Cin * 5, 5)
            self.acc = S.gather(self.x, self.w)

    def ref(self):
        return S.Ref(self.acc[0].clone(), self.acc[1].clone(), 5 * self.Cin)

    def shape(self):
        return (self.B, self.Tout, self.N)

    def name(self):
        return f"B={self.B} Tin={self.Tin} Cin={self.Cin} N={self.N} {'T' if self.transposed else 'G'}{' odd' if self.odd else ''}"


def tail_buffer(n, dtype=torch.float32, tail=4096):
    """A 1-D buffer of n NaN elements followed by `tail` sentinels."""
    t = torch.full((n + tail,), float("nan"), device="cuda", dtype=dtype)
    t[n:] = S.Guarded.SENTINEL
    return t


def assert_tail(t, n, what):
    bad = (t[n:] != S.Guarded.SENTINEL).nonzero()
    assert bad.numel() == 0, f"{what}: wrote {bad.numel()} element(s) past the {n} the plan allows"
    assert bool(torch.isfinite(t[:n]).all()), f"{what}: plan rows left unwritten"


# ---------------------------------------------------------------------------------------------------------------------
# edge shapes, every instantiation
# ---------------------------------------------------------------------------------------------------------------------
# (Tin, odd, Cin, N, B): B = "tb-1" / "tb+1" are relative to the batch rows one tile spans under the forced RT
EDGE_G = [(7, False, 16, 32, "tb+1"), (8, False, 48, 96, "tb-1"), (9, False, 80, 32, 1), (33, False, 16, 256, "tb+1"),
          (66, False, 128, 96, 3), (125, False, 48, 32, "tb-1"), (130, False, 256, 32, 2), (299, False, 80, 32, 3),
          (300, False, 16, 96, 1), (420, False, 48, 32, 2), (150, False, 16, 32, 193), (65, False, 16, 32, 193),
          (10, False, 256, 256, "tb+1")]
EDGE_T = [(4, False, 16, 32, "tb+1"), (4, True, 48, 96, "tb-1"), (5, True, 80, 32, 1), (17, False, 48, 32, "tb+1"),
          (33, True, 16, 256, "tb+1"), (63, False, 128, 96, 3), (65, True, 48, 32, "tb-1"), (150, False, 80, 32, 3),
          (150, True, 16, 96, 2), (210, False, 48, 32, 1), (210, True, 256, 32, 2), (75, True, 16, 32, 193),
          (33, False, 16, 32, 193)]


def edge_cases(ops, transposed):
    for Tin, odd, Cin, N, bsel in (EDGE_T if transposed else EDGE_G):
        tb = ops.conv16_plan(1, Tin, N, transposed)[0]
        B = {"tb-1": max(tb - 1, 1), "tb+1": tb + 1}.get(bsel, bsel)
        yield B, Tin, Cin, N, odd


@pytest.mark.parametrize("tr2,rt,rid", INSTANCES, ids=INSTANCE_IDS)
def test_edge_shapes(ops, hook, monkeypatch, tr2, rt, rid):
    monkeypatch.setenv("MG_CONV16_RT", str(rt))
    n_tt = []
    for i, (B, Tin, Cin, N, odd) in enumerate(edge_cases(ops, tr2)):
        p = Problem(ops, tr2, B, Tin, Cin, N, odd, seed=i)
        assert ops.conv16_supported(B, Tin, Cin, N, tr2, p.Tout), p.name()
        tb, rows, bm = ops._conv16_plan(B, Tin, N, tr2)
        assert bm == 32 * rt
        n_tt.append(rows // 2 // -(-B // tb))
        y = S.Guarded(p.shape())
        kw = {}
        if rid:
            part = tail_buffer(3 * rows * N)
            kw["stats"] = part
        hook.seen.clear()
        ops.conv16(p.x, p.wq, y.t, N, tr2, odd=odd, **kw)
        assert hook.seen == [sym(tr2, rt, rid)], (p.name(), hook.seen)
        S.check(y.t, p.ref(), p.name())
        y.check(p.name())
        if rid:
            assert_tail(part, 3 * rows * N, "stats " + p.name())
            pv = part[:3 * rows * N].view(rows, 3, N).double()
            assert bool((pv[:, 2].sum(0) == B * p.Tout).all()), p.name()
            yd = y.t.double()
            S.check(pv[:, 0].sum(0), S.Ref(yd.sum((0, 1)), yd.abs().sum((0, 1)), B * p.Tout), "stats sum " + p.name())
    assert max(n_tt) >= 3     # a time axis of at least three tiles, the last one partial, went through the tile decode


def test_fallback_agrees_at_edge_shapes(ops, hook):
    """The window-GEMM kernels the engine takes where conv16 does not apply pass the same bound at the same shapes:
    conv1d_fwd / convT1d_dgrad (gather form) and convT1d_fwd / conv1d_dgrad (scatter form)."""
    for tr2 in (False, True):
        for i, (B, Tin, Cin, N, odd) in enumerate(edge_cases(ops, tr2)):
            p = Problem(ops, tr2, B, Tin, Cin, N, odd, seed=i)
            y = S.Guarded(p.shape())
            hook.seen.clear()
            if not tr2:
                (ops.conv1d_fwd if i % 2 == 0 else ops.convT1d_dgrad)(p.x, p.w, y.t, *((2,) if i % 2 == 0 else ()))
            elif odd or i % 2:
                ops.conv1d_dgrad(p.x, p.w, y.t, 2)
            else:
                ops.convT1d_fwd(p.x, p.w, y.t)
            assert len(hook.seen) == 1 and not hook.seen[0].startswith("conv16"), hook.seen
            S.check(y.t, p.ref(), "fallback " + hook.seen[0] + " " + p.name())
            y.check(p.name())


# ---------------------------------------------------------------------------------------------------------------------
# the fused epilogue, every instantiation (RID: with the interpolate rider attached, checked bit for bit)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr2,rt,rid", INSTANCES, ids=INSTANCE_IDS)
def test_epilogues(ops, hook, monkeypatch, tr2, rt, rid):
    monkeypatch.setenv("MG_CONV16_RT", str(rt))
    odd_list = (False, True) if tr2 else (False,)
    for odd in odd_list:
        B, Tin, Cin, N = (3, 34, 48, 96) if tr2 else (3, 67, 48, 96)
        p = Problem(ops, tr2, B, Tin, Cin, N, odd, seed=7)
        shp = p.shape()
        bias, scale, shift, gscale = rnd(N, seed=20), rnd(N, seed=21), rnd(N, seed=22), rnd(N, seed=23)
        gref, base = rnd(*shp, seed=24), rnd(*shp, seed=25)
        gref_t = torch.tanh(gref)
        cases = [
            ("bias", dict(bias=bias), dict(bias=bias)),
            ("scale/shift", dict(bias=bias, scale=scale, shift=shift), dict(bias=bias, scale=scale, shift=shift)),
            ("zout+lrelu", dict(bias=bias, act=ops.ACT_LRELU, zout=True), dict(bias=bias, act=S.ACT_LRELU, zout=True)),
            ("zout+relu", dict(scale=scale, shift=shift, act=ops.ACT_RELU, zout=True), dict(scale=scale, shift=shift, act=S.ACT_RELU, zout=True)),
            ("gref lrelu+gscale", dict(gref=gref, gact=ops.ACT_LRELU, gscale=gscale), dict(gref=gref, gact=S.ACT_LRELU, gscale=gscale)),
            ("gref relu", dict(bias=bias, gref=gref, gact=ops.ACT_RELU), dict(bias=bias, gref=gref, gact=S.ACT_RELU)),
            ("gref tanh+gscale", dict(gref=gref_t, gact=ops.ACT_TANH, gscale=gscale), dict(gref=gref_t, gact=S.ACT_TANH, gscale=gscale)),
            ("accumulate", dict(bias=bias, accumulate=True), dict(bias=bias, base=base)),
        ]
        for what, epi, repi in cases:
            y = S.Guarded(shp)
            if "accumulate" in epi:
                y.t.copy_(base)
            kw = dict(epi)
            z = None
            if kw.pop("zout", False):
                z = S.Guarded(shp)
                kw["zout"] = z.t
            mix = _mix(shp, rows=B - 1) if rid else None
            if mix is not None:
                kw["mix"] = mix[0]
            hook.seen.clear()
            ops.conv16(p.x, p.wq, y.t, N, tr2, odd=odd, **kw)
            assert hook.seen == [sym(tr2, rt, rid)], hook.seen
            ref = p.ref().epilogue(**repi)
            S.check(y.t, ref, f"{what} {p.name()}")
            y.check(what)
            if z is not None:
                S.check(z.t, ref.z, f"{what} zout {p.name()}")
                z.check(what + " zout")
            if mix is not None:
                _check_mix(ops, mix, y.t, p.Tout)
        # the transposed form's zero-padded output (the generator's T % 8 != 0 branch): rows beyond Tout untouched
        Ty = p.Tout + 3
        y = S.Guarded((B, Ty, N), fill=7.0)
        kw = {}
        mix = _mix((B, Ty, N), rows=B) if rid else None
        if mix is not None:
            kw["mix"] = mix[0]
        ops.conv16(p.x, p.wq, y.t, N, tr2, odd=odd, bias=bias, **kw)
        S.check(y.t[:, :p.Tout], p.ref().epilogue(bias=bias), "padded " + p.name())
        assert bool((y.t[:, p.Tout:] == 7.0).all()), "padded rows written"
        y.check("padded")
        if mix is not None:
            _check_mix(ops, mix, y.t, p.Tout)


def _mix(shape, rows):
    """(conv16 mix rider argument, guard of mix_out, rows): mix_out prefilled with 7.0 inside sentinels."""
    B = shape[0]
    real, alpha = rnd(*shape, seed=30), torch.rand(B, generator=torch.Generator().manual_seed(31)).cuda()
    out = S.Guarded(shape, fill=7.0)
    return (real, alpha, out.t, rows), out, rows


def _check_mix(ops, mix, y, Tout):
    (real, alpha, out, rows), guard, _ = mix
    want = torch.empty_like(real[:rows])
    ops.gp_interp(real[:rows].contiguous(), y[:rows].contiguous(), alpha[:rows].contiguous(), want)
    assert torch.equal(out[:rows, :Tout], want[:, :Tout]), "mix != gp_interp of the stored output"
    assert bool((out[rows:] == 7.0).all()) and bool((out[:, Tout:] == 7.0).all()), "mix wrote rows it does not own"
    guard.check("mix_out")


# ---------------------------------------------------------------------------------------------------------------------
# riders under both tile sizes
# ---------------------------------------------------------------------------------------------------------------------
def _plain(ops, p, **epi):
    y = torch.full(p.shape(), float("nan"), device="cuda")
    ops.conv16(p.x, p.wq, y, p.N, p.transposed, odd=p.odd, **epi)
    return y


@pytest.mark.parametrize("rt", [1, 2])
@pytest.mark.parametrize("tr2", [False, True], ids=["gather", "transposed"])
def test_stats_rider_finishes_to_fp64_statistics(ops, hook, monkeypatch, rt, tr2):
    monkeypatch.setenv("MG_CONV16_RT", str(rt))
    p = Problem(ops, tr2, 6, 21 if tr2 else 41, 48, 64, seed=3)
    N, bias = p.N, rnd(p.N, seed=4, scale=3.0)
    tb, rows = ops.conv16_plan(p.B, p.Tin, N, tr2)
    part = tail_buffer(3 * rows * N)
    z = S.Guarded(p.shape())
    hook.seen.clear()
    ops.conv16(p.x, p.wq, z.t, N, tr2, odd=p.odd, bias=bias, stats=part)
    assert hook.seen == [sym(tr2, rt, True)]
    assert_tail(part, 3 * rows * N, "stats")
    z.check("stats")
    assert torch.equal(z.t, _plain(ops, p, bias=bias))
    S.check(z.t, p.ref().epilogue(bias=bias), "stats output")
    gamma, beta = rnd(N, seed=5).abs() + 0.5, rnd(N, seed=6)
    a = torch.empty_like(z.t)
    rm, rv = torch.zeros(N, device="cuda"), torch.ones(N, device="cuda")
    m, i = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    ops.bn_train_fwd_parts(part, rows, 1, z.t, a, gamma, beta, rm, rv, m, i, ops.ACT_RELU)
    z64 = z.t.double().view(-1, N)
    mean, var = z64.mean(0), z64.var(0, unbiased=False)
    cnt = z64.shape[0]
    S.check(m, S.Ref(mean, z64.abs().mean(0), cnt), "mean")
    torch.testing.assert_close(i.double(), 1.0 / torch.sqrt(var + 1e-5), rtol=2e-5, atol=0)
    torch.testing.assert_close(rm.double(), 0.1 * mean, rtol=2e-6, atol=1e-7)
    torch.testing.assert_close(rv.double(), 0.9 + 0.1 * z64.var(0, unbiased=True), rtol=2e-5, atol=0)


@pytest.mark.parametrize("rt", [1, 2])
def test_pool_rider(ops, hook, monkeypatch, rt):
    monkeypatch.setenv("MG_CONV16_RT", str(rt))
    Tout = 16 * rt
    B, Tin, Cin, N = 5, 2 * Tout, 48, 96
    assert ops.conv16_poolable(B, Tin, Cin, N)
    assert not ops.conv16_poolable(B, 2 * (16 * (3 - rt)), Cin, N)       # the other tile size's pooling length
    p = Problem(ops, False, B, Tin, Cin, N, seed=8)
    bias = rnd(N, seed=9)
    y, pool = S.Guarded(p.shape()), S.Guarded((B, N), rows=8)
    hook.seen.clear()
    ops.conv16_pool(p.x, p.wq, y.t, N, pool.t, 1.0 / Tout, bias=bias, act=ops.ACT_LRELU)
    assert hook.seen == [sym(False, rt, True)]
    y.check("pool y")
    pool.check("pool")
    assert torch.equal(y.t, _plain(ops, p, bias=bias, act=ops.ACT_LRELU))
    S.check(y.t, p.ref().epilogue(bias=bias, act=S.ACT_LRELU), "pool output")
    yd = y.t.double()
    S.check(pool.t, S.Ref(yd.mean(1), yd.abs().mean(1), Tout), "pool")


@pytest.mark.parametrize("rt", [1, 2])
@pytest.mark.parametrize("tr2", [False, True], ids=["gather", "transposed"])
def test_perm_rider(ops, hook, monkeypatch, rt, tr2):
    monkeypatch.setenv("MG_CONV16_RT", str(rt))
    p = Problem(ops, tr2, 5, 13 if tr2 else 37, 48, 64, odd=tr2, seed=10)
    gref = rnd(*p.shape(), seed=11)
    dense = _plain(ops, p, gref=gref, gact=ops.ACT_RELU)
    perm = S.Guarded((p.B, p.N, p.Tout))
    hook.seen.clear()
    ops.conv16(p.x, p.wq, perm.t, p.N, tr2, odd=p.odd, perm=True, gref=gref, gact=ops.ACT_RELU)
    assert hook.seen == [sym(tr2, rt, True)]
    perm.check("perm")
    assert torch.equal(perm.t, dense.permute(0, 2, 1).contiguous())
    S.check(dense, p.ref().epilogue(gref=gref, gact=S.ACT_RELU), "perm dense")


@pytest.mark.parametrize("rt", [1, 2])
@pytest.mark.parametrize("tr2", [False, True], ids=["gather", "transposed"])
def test_mix_rider(ops, hook, monkeypatch, rt, tr2):
    monkeypatch.setenv("MG_CONV16_RT", str(rt))
    p = Problem(ops, tr2, 7, 16 if tr2 else 33, 48, 64, seed=12)
    bias = rnd(p.N, seed=13)
    y = S.Guarded(p.shape())
    mix = _mix(p.shape(), rows=4)
    hook.seen.clear()
    ops.conv16(p.x, p.wq, y.t, p.N, tr2, bias=bias, mix=mix[0])
    assert hook.seen == [sym(tr2, rt, True)]
    y.check("mix y")
    assert torch.equal(y.t, _plain(ops, p, bias=bias))
    _check_mix(ops, mix, y.t, p.Tout)


@pytest.mark.parametrize("act", ["relu", "lrelu"])
@pytest.mark.parametrize("rt", [1, 2])
@pytest.mark.parametrize("tr2", [False, True], ids=["gather", "transposed"])
def test_bnb_rider_column_sums(ops, hook, monkeypatch, rt, tr2, act):
    """bnb: sum g and sum g * x_hat per column, g = dy * act'(a), x_hat = (z - mean) * invstd -- against fp64 sums of the
    stored dy; the bnb-only launch runs (and is labelled) conv16_kernel<.., true>."""
    monkeypatch.setenv("MG_CONV16_RT", str(rt))
    p = Problem(ops, tr2, 6, 19 if tr2 else 45, 48, 96, seed=14)
    N, shp = p.N, p.shape()
    code = ops.ACT_RELU if act == "relu" else ops.ACT_LRELU
    z = rnd(*shp, seed=15)
    a = torch.where(z > 0, z, z * (0.0 if act == "relu" else 0.2))
    mean, invstd = rnd(N, seed=16, scale=0.1), rnd(N, seed=17).abs() + 0.5
    rows = ops.conv16_plan(p.B, p.Tin, N, tr2)[1]
    part = tail_buffer(2 * rows * N, dtype=torch.float64)
    dy = S.Guarded(shp)
    hook.seen.clear()
    ops.conv16(p.x, p.wq, dy.t, N, tr2, odd=p.odd, bnb=(a, z, mean, invstd, part, code))
    assert hook.seen == [sym(tr2, rt, True)]
    assert_tail(part, 2 * rows * N, "bnb part")
    dy.check("bnb dy")
    assert torch.equal(dy.t, _plain(ops, p))
    S.check(dy.t, p.ref(), "bnb dy")
    f = torch.where(a > 0, 1.0, 0.0 if act == "relu" else 0.2).double()
    g = (dy.t.double() * f).view(-1, N)
    xhat = ((z.double() - mean.double()) * invstd.double()).view(-1, N)
    pv = part[:2 * rows * N].view(rows, 2, N)
    S.check(pv[:, 0].sum(0), S.Ref(g.sum(0), g.abs().sum(0), 2), "bnb sum g")
    S.check(pv[:, 1].sum(0), S.Ref((g * xhat).sum(0), (g * xhat).abs().sum(0), 4), "bnb sum g*xhat")


# ---------------------------------------------------------------------------------------------------------------------
# the domain boundary: supported => runs and passes; unsupported => ValueError before any launch
# ---------------------------------------------------------------------------------------------------------------------
def test_domain_boundary_sweep(ops, hook, monkeypatch):
    """Seeded shapes on both sides of each limit: Cin % 16, N % 32, Tm < 4, under both tile sizes.  The staging limit
    (TB * R * 4 <= 256 * MAXX window slots) is tightest at the smallest Tm of each tile height -- Tm = 4, 5, 9, 17, 33
    (gather, RT = 2: 704 / 608 / 560 / 536 / 524 of 768) -- which the sweep covers with many batch groups."""
    rng = random.Random(1234)
    seen = {True: 0, False: 0}
    for i in range(60):
        tr2, odd, rt = rng.random() < 0.5, rng.random() < 0.5, rng.choice((1, 2))
        monkeypatch.setenv("MG_CONV16_RT", str(rt))
        B = rng.choice((1, 2, 3, 15, 16, 17, 31, 33, 65, 193))
        Cin = rng.choice((16, 32, 48, 80, 16 * rng.randint(1, 4) + rng.choice((4, 8, 12))))
        N = rng.choice((32, 64, 96, 256, 32 * rng.randint(1, 3) + rng.choice((8, 16, 24))))
        Tm = rng.choice((1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33))
        Tin = Tm if tr2 else 2 * Tm - rng.choice((0, 1))
        odd = odd and tr2
        Tout = tout_of(tr2, Tin, odd)
        ok = ops.conv16_supported(B, Tin, Cin, N, tr2, Tout)
        assert ok == (Cin % 16 == 0 and N % 32 == 0 and Tm >= 4), (B, Tin, Cin, N, tr2)
        seen[ok] += 1
        p = Problem(ops, tr2, B, Tin, Cin, N, odd, seed=100 + i)
        y = S.Guarded(p.shape())
        hook.seen.clear()
        if ok:
            ops.conv16(p.x, p.wq, y.t, N, tr2, odd=odd)
            assert hook.seen == [sym(tr2, rt, False)]
            S.check(y.t, p.ref(), "sweep " + p.name())
        else:
            with pytest.raises(ValueError):
                ops.conv16(p.x, p.wq, y.t, N, tr2, odd=odd)
            torch.cuda.synchronize()
            assert hook.seen == [] and bool(torch.isnan(y.t).all()), p.name()
        y.check(p.name())
    assert seen[True] >= 10 and seen[False] >= 10, seen


# ---------------------------------------------------------------------------------------------------------------------
# production coverage: every conv16 launch of the cfg2 engine's flows, replayed in isolation under both tile sizes
# ---------------------------------------------------------------------------------------------------------------------
_EPI_FLAGS = ("bias", "scale", "shift", "zout", "gref", "emul", "gscale")


def _signature(x, y, N, transposed, odd, stats, pool, perm, mix, bnb, epi):
    B, Tin, Cin = x.shape
    riders = tuple(sorted(k for k, v in (("stats", stats), ("pool", pool), ("perm", perm or None), ("mix", mix),
                                          ("bnb", bnb)) if v is not None))
    kinds = tuple(k for k in _EPI_FLAGS if epi.get(k) is not None)
    kinds += tuple(f"{k}={int(epi[k])}" for k in ("act", "gact") if epi.get(k, 0))
    if epi.get("accumulate"):
        kinds += ("accumulate",)
    Ty = y.shape[2] if perm else y.shape[1]
    extra = (("mix_rows", mix[3]),) if mix is not None else ()
    extra += (("bnb_act", int(bnb[5])),) if bnb is not None else ()
    return (B, Tin, Cin, N, bool(transposed), bool(odd), riders, kinds, Ty) + extra


def _replay(ops, sig, rt, seed):
    B, Tin, Cin, N, tr2, odd, riders, kinds, Ty = sig[:9]
    extra = dict(sig[9:])
    p = Problem(ops, tr2, B, Tin, Cin, N, odd, seed=seed)
    shp = p.shape()
    epi, repi = {}, {}
    for k in kinds:
        if k in ("bias", "gscale"):
            epi[k] = repi[k] = rnd(N, seed=seed + 2)
        elif k == "scale":
            epi["scale"] = repi["scale"] = rnd(N, seed=seed + 3)
            epi["shift"] = repi["shift"] = rnd(N, seed=seed + 4)
        elif k in ("gref", "emul"):
            epi[k] = repi[k] = rnd(*shp, seed=seed + 5)
        elif k == "zout":
            repi["zout"] = True
        elif k.startswith("act="):
            epi["act"] = repi["act"] = int(k[4:])
        elif k.startswith("gact="):
            epi["gact"] = repi["gact"] = int(k[5:])
        elif k == "accumulate":
            epi["accumulate"] = True
            repi["base"] = rnd(*shp, seed=seed + 6)
    if "gref" in epi and epi.get("gact") == S.ACT_TANH:
        epi["gref"] = repi["gref"] = torch.tanh(epi["gref"])
    perm = "perm" in riders
    y = S.Guarded((B, N, p.Tout) if perm else (B, Ty, N))
    if "base" in repi:
        y.t[:, :p.Tout].copy_(repi["base"])
    z = S.Guarded(shp) if "zout" in repi else None
    if z is not None:
        epi["zout"] = z.t
    kw = {}
    if "stats" in riders:
        kw["stats"] = tail_buffer(3 * ops.conv16_plan(B, Tin, N, tr2)[1] * N)
    if "pool" in riders and ops.conv16_poolable(B, Tin, Cin, N):
        kw["pool"] = (torch.empty(B, N, device="cuda"), 1.0 / p.Tout)
    if "mix" in riders:
        kw["mix"] = _mix((B, Ty, N), rows=extra["mix_rows"])[0]
    if "bnb" in riders:
        zz = rnd(*shp, seed=seed + 7)
        kw["bnb"] = (torch.relu(zz), zz, rnd(N, seed=seed + 8), rnd(N, seed=seed + 9).abs(),
                     torch.empty(2 * ops.conv16_plan(B, Tin, N, tr2)[1] * N, device="cuda", dtype=torch.float64),
                     extra["bnb_act"])
    ops.conv16(p.x, p.wq, y.t, N, tr2, odd=odd, perm=perm, **kw, **epi)
    ref = p.ref().epilogue(**repi)
    got = y.t.permute(0, 2, 1) if perm else y.t[:, :p.Tout]
    S.check(got, ref, f"replay RT={rt} {sig}")
    y.check(f"replay {sig}")
    if Ty != p.Tout:
        assert bool(torch.isnan(y.t[:, p.Tout:]).all()), f"replay {sig}: padded rows written"
    if z is not None:
        S.check(z.t, ref.z, f"replay zout {sig}")
        z.check(f"replay zout {sig}")


def test_engine_conv16_launches_cfg2_replayed(ops, monkeypatch, capsys):
    """The engine at cfg2 (B=64, T=256, C=128) through the flows a training step takes -- teacher-forced d_backward /
    g_backward, the fused dg_step_rng, the forked dg_fork_step_rng that DataParallel(eng, 1) takes -- eagerly; every
    ops.conv16 launch is recorded (the call goes through) and each distinct signature is replayed under RT = 1 and 2."""
    from oracle import melo_oracle as O
    from melo_gan_amd.gan.engine import GanEngine
    B, T, C = 64, 256, 128
    cfg, ed_cfg = O.default_gan_cfg(B, T, C), O.default_ed_cfg(C)
    St = O.build_gan_state(cfg, ed_cfg, "weights_init", seed=3)
    sigs = []
    real_conv16 = ops.conv16

    def recorder(x, wq, y, N, transposed, odd=False, stats=None, pool=None, perm=False, mix=None, bnb=None, **epi):
        sigs.append(_signature(x, y, N, transposed, odd, stats, pool, perm, mix, bnb, epi))
        return real_conv16(x, wq, y, N, transposed, odd=odd, stats=stats, pool=pool, perm=perm, mix=mix, bnb=bnb, **epi)

    monkeypatch.setattr(ops, "conv16", recorder)
    eng = GanEngine(cfg, ed_cfg, "cuda", B)
    eng.load_state(St.PE, St.PG, St.BG, St.PD, St.PED, St.BED)
    eng.set_batch(*(t.cuda() for t in O.synthetic_batch(B, T, C, cfg["LATENT_DIM"], 6, 42)))
    R = O.step_randoms(B, cfg["NOISE_DIM"], seed=9)
    with torch.cuda.stream(eng.stream):
        eng.set_randoms(R["noise_d"].cuda(), [m.cuda() for m in R["dm_d"]], R["alpha"].cuda())
        eng.d_backward()
        eng.set_randoms(R["noise_g"].cuda(), [m.cuda() for m in R["dm_g"]])
        eng.g_backward()
        n_teacher = len(sigs)
        eng.seed(77)
        eng.dg_step_rng()
        n_fused = len(sigs) - n_teacher
        assert eng.ed_side is not None                       # the default: the forked flow has its side stream
        eng.dg_fork_step_rng()
        torch.cuda.synchronize()
    monkeypatch.setattr(ops, "conv16", real_conv16)
    assert n_teacher > 0 and n_fused > 0 and len(sigs) > n_teacher + n_fused
    assert {s[4] for s in sigs} == {False, True}            # both forms
    # the riders these flows pass (engine.py: deconv.0 / .3 statistics, deconv.6 interpolate, conv.4 temporal mean,
    # deconv.6 / .3 BatchNorm-backward sums, deconv.0's permuted data gradient)
    assert {r for s in sigs for r in s[6]} == {"stats", "pool", "perm", "mix", "bnb"}
    distinct = sorted(set(sigs), key=repr)
    with capsys.disabled():
        print(f"\ncfg2: {len(sigs)} conv16 launches, {len(distinct)} distinct signatures, replayed at RT=1 and RT=2:")
        for s in distinct:
            print("  ", s)
    for rt in (1, 2):
        monkeypatch.setenv("MG_CONV16_RT", str(rt))
        for j, s in enumerate(distinct):
            _replay(ops, s, rt, seed=1000 + 10 * j)


# ---------------------------------------------------------------------------------------------------------------------
# stride-2 weight gradients: wgrad_multi_kernel<2,5>, every slice plan
# ---------------------------------------------------------------------------------------------------------------------
TARGETS = ["1", "64", None, "100000"]          # one slice ... MAX_SPLITS slices (None: the default plan)


def _set_target(monkeypatch, t):
    if t is None:
        monkeypatch.delenv("MG_WGRAD_TARGET", raising=False)
    else:
        monkeypatch.setenv("MG_WGRAD_TARGET", t)


def _wgrad_twice(launch):
    """Runs launch() twice into fresh NaN outputs; asserts identical bits; returns the first result."""
    outs = [launch() for _ in range(2)]
    for a, b in zip(*outs):
        assert torch.equal(a, b), "wgrad: run-to-run bits differ"
    return outs[0]


# (Cin, Cout, T) of the critic's stride-2 Conv1d layers; (Cin, Cout, L) of the generator's ConvTranspose1d layers
CRITIC = [(128, 64, 256), (64, 128, 128), (128, 256, 64)]
GENERATOR = [(256, 128, 32), (128, 64, 64), (64, 128, 128)]


@pytest.mark.parametrize("target", TARGETS, ids=lambda t: f"target={t or 'default'}")
def test_conv1d_wgrad_stride2(ops, monkeypatch, hook, target):
    _set_target(monkeypatch, target)
    shapes = [(Cin, Cout, T, rows, seg2) for (Cin, Cout, T) in CRITIC for rows in (64, 128, 192) for seg2 in (False, True)]
    shapes += [(20, 32, 63, 5, False), (20, 32, 63, 5, True), (16, 32, 9, 1, False)]
    for i, (Cin, Cout, T, rows, seg2) in enumerate(shapes):
        nb0 = min(rows, 64) if seg2 and rows > 64 else (rows - 2 if seg2 else rows)
        nb0 = max(nb0, 1)
        Ts = S.tm_gather(T)
        x, dy = rnd(rows, T, Cin, seed=i), rnd(rows, Ts, Cout, seed=i + 50)
        seg = dict(x2=x[nb0:].contiguous(), dy2=dy[nb0:].contiguous()) if seg2 and nb0 < rows else {}
        x0, dy0 = x[:nb0].contiguous(), dy[:nb0].contiguous()

        def launch():
            dw, db = torch.full((Cout, Cin, 5), float("nan"), device="cuda"), torch.full((Cout,), float("nan"), device="cuda")
            ops.conv1d_wgrad(x0, dy0, dw, 2, db=db, **seg)
            return dw, db
        hook.seen.clear()
        dw, db = _wgrad_twice(launch)
        assert hook.seen[0] == "wgrad_multi_kernel<2,5>"
        (rdw, mdw, n), (rdb, mdb, nbias) = S.conv_wgrad(x0, dy0, seg.get("x2"), seg.get("dy2"))
        what = f"conv dw Cin={Cin} Cout={Cout} T={T} rows={rows} nb0={nb0} target={target}"
        S.check(dw, S.Ref(rdw, mdw, n), what)
        S.check(db, S.Ref(rdb, mdb, nbias), what + " db")


@pytest.mark.parametrize("target", TARGETS, ids=lambda t: f"target={t or 'default'}")
def test_convT1d_wgrad(ops, monkeypatch, hook, target):
    _set_target(monkeypatch, target)
    shapes = [(Cin, Cout, L, rows) for (Cin, Cout, L) in GENERATOR for rows in (64, 128, 192)]
    shapes += [(20, 24, 31, 5), (16, 32, 4, 1)]
    for i, (Cin, Cout, L, rows) in enumerate(shapes):
        x, dy = rnd(rows, L, Cin, seed=i), rnd(rows, 2 * L, Cout, seed=i + 50)

        def launch():
            dw, db = torch.full((Cin, Cout, 5), float("nan"), device="cuda"), torch.full((Cout,), float("nan"), device="cuda")
            ops.convT1d_wgrad(x, dy, dw, db=db)
            return dw, db
        hook.seen.clear()
        dw, db = _wgrad_twice(launch)
        assert hook.seen[0] == "wgrad_multi_kernel<2,5>"
        (rdw, mdw, n), (rdb, mdb, nbias) = S.convT_wgrad(x, dy)
        what = f"convT dw Cin={Cin} Cout={Cout} L={L} rows={rows} target={target}"
        S.check(dw, S.Ref(rdw, mdw, n), what)
        S.check(db, S.Ref(rdb, mdb, nbias), what + " db")


@pytest.mark.parametrize("target", TARGETS, ids=lambda t: f"target={t or 'default'}")
def test_wgrad_multi_several_stride2_jobs(ops, monkeypatch, hook, target):
    """The critic's three gradients (penalty segment included) and the generator's three deconvolutions in one launch
    (+ a ragged job), as the engine batches them."""
    _set_target(monkeypatch, target)
    specs = [("conv", 128, 64, 256, 64, 128), ("conv", 64, 128, 128, 64, 128), ("conv", 128, 256, 64, 64, 128),
             ("convT", 256, 128, 32, 128, 0), ("convT", 128, 64, 64, 128, 0), ("convT", 64, 128, 128, 128, 0),
             ("conv", 20, 32, 63, 5, 3)]
    data = []
    for i, (kind, Cin, Cout, T, nb0, nb1) in enumerate(specs):
        if kind == "conv":
            x, dy = rnd(nb0 + nb1, T, Cin, seed=i), rnd(nb0 + nb1, S.tm_gather(T), Cout, seed=i + 50)
            data.append((kind, x[:nb0].contiguous(), dy[:nb0].contiguous(), x[nb0:].contiguous() if nb1 else None,
                         dy[nb0:].contiguous() if nb1 else None, (Cout, Cin, 5), Cout))
        else:
            x, dy = rnd(nb0, T, Cin, seed=i), rnd(nb0, 2 * T, Cout, seed=i + 50)
            data.append((kind, x, dy, None, None, (Cin, Cout, 5), Cout))

    def launch():
        outs, jobs = [], []
        for kind, x, dy, x2, dy2, wshape, nb in data:
            dw, db = torch.full(wshape, float("nan"), device="cuda"), torch.full((nb,), float("nan"), device="cuda")
            if kind == "conv":
                jobs.append(ops.conv1d_wgrad(x, dy, dw, 2, x2=x2, dy2=dy2, db=db, defer=True))
            else:
                jobs.append(ops.convT1d_wgrad(x, dy, dw, db=db, defer=True))
            outs += [dw, db]
        ops.wgrad_multi(jobs)
        return outs
    hook.seen.clear()
    outs = _wgrad_twice(launch)
    assert hook.seen[0] == "wgrad_multi_kernel<2,5>" and len(hook.seen) == 2      # one launch per run
    for j, (kind, x, dy, x2, dy2, _, _) in enumerate(data):
        (rdw, mdw, n), (rdb, mdb, nbias) = S.conv_wgrad(x, dy, x2, dy2) if kind == "conv" else S.convT_wgrad(x, dy)
        S.check(outs[2 * j], S.Ref(rdw, mdw, n), f"multi job {j} {specs[j]} target={target}")
        S.check(outs[2 * j + 1], S.Ref(rdb, mdb, nbias), f"multi job {j} {specs[j]} db target={target}")
