"""The stride-1 window GEMMs, their split-K path, wino3, the skinny Linear kernel, the stride-1 weight gradients and the row
chain's Linear ops pinned to fp64, element by element (tests/window_ref.py: the references and the bound).

Every case forces the instantiation or plan it is about through the library's own switches (MG_FORCE_TILE, MG_SPLITK_TARGET,
MG_LINEAR_SKINNY_ONLY, MG_WGRAD_TARGET, read per call), asserts through ops.set_launch_hook which symbol ran and through the
host queries ops.conv_plan / ops.linear_route which split it ran with, writes into NaN-prefilled outputs inside sentinel
rows, and checks every element.  The shape tables below are plain data: tests/test_window_ref.py sweeps them on the host
and asserts that they reach what this file claims (18 window-GEMM instantiations, ksplit 2 / 4 / 8 with an uneven last
slab, both finish variants, four skinny instantiations, the split skinny plans with and without a column permutation, the
window-GEMM route of a permuted Linear).  The fp64 references are evaluated on the device.

Each test prints the worst error / bound ratio of its section (pytest -s shows it).  Measured on an MI355X: a. 0.20 (n = 16),
b. 0.13, c. 0.17 with a GELU' epilogue and 0.02 without, d. 0.20 (n = 1), e. 0.26 (n = 2), f. 0.39 (n = 1); the file takes
about 7 s.  Which conv_finish_kernel<VEC> follows a split launch is not announced through the hook: it is
read from mg_conv_finish_vec, the predicate the launch itself evaluates, with the tensors the case used."""
import contextlib
import ctypes as C

import pytest
import torch

import stride2_ref as S
import window_ref as W

pytestmark = pytest.mark.gpu

ACTS = (S.ACT_RELU, S.ACT_LRELU, S.ACT_GELU, S.ACT_TANH)


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


class Worst:
    """Keeps the worst error / bound ratio of a section and prints it when the test is over."""

    def __init__(self, section):
        self.section, self.r, self.what, self.n = section, 0.0, "", 0

    def check(self, got, ref, what):
        r = W.check(got, ref, what)
        self.n += 1
        if r >= self.r:
            self.r, self.what = r, what
        return r

    def report(self, capsys):
        with capsys.disabled():
            print(f"\n[window contract] {self.section}: {self.n} checks, worst error / bound = {self.r:.4f} ({self.what})")


def rnd(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def off4(t):
    """A contiguous copy of t that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def wsym(S_, K, tr2, nck, tile):
    b = lambda v: "true" if v else "false"  # noqa: E731
    return f"conv_wgemm_kernel<{S_},{K},{b(tr2)},{b(nck)},{tile // 10},{tile % 10}>"


# ---------------------------------------------------------------------------------------------------------------------
# a. stride-1 window GEMM: conv_wgemm_kernel<1, K, false, NCK, TM, TN>
# ---------------------------------------------------------------------------------------------------------------------
TILES = (11, 12, 22)
S1_INSTANCES = [(K, nck, tile) for K in (1, 3, 5) for nck in (True, False) for tile in TILES]


def batch_rows_per_tile(T, tile):
    """Batch rows one tile of conv_wgemm_kernel spans (launch_cfg: TB = BM >> min(ceil log2 T, log2 BM))."""
    bm = 64 * (tile // 10)
    lg = min((T - 1).bit_length(), bm.bit_length() - 1)
    return bm >> lg, -(-T // (1 << lg))


def s1_edge_cases(K, tile):
    """(B, T, Cin, N, padded y) of one instantiation.  T: 1, 2, 3, K-1, K, 63, 64, 65, 130, 300 (several tt_log2; a partial
    last time tile with n_ttiles >= 3); B one below / one above the batch rows of a tile, and 193; Cin incl. 24 (not a chunk
    multiple) and, for K = 1, 100 (not a multiple of 64); N incl. 130 (N % 4 != 0); N > 64 wherever the tile is forced (N <=
    64 runs the 64x64 tile whatever MG_FORCE_TILE says); Cin, N > 8 (below, K > 1 goes to the thin kernels).  The 128x128
    tile of K = 5 cannot stage a T = 1 problem (128 batch rows x 5 window rows exceed the LDS): that one starts at T = 2."""
    Ts = sorted({t for t in (1, 2, 3, K - 1, K, 63, 64, 65, 130, 300) if t > 0})
    if K == 5 and tile == 22:
        Ts.remove(1)
    cins = [16, 24, 48, 80, 256] + ([100] if K == 1 else [])
    ns = [32, 96, 130, 256] if tile == 11 else [96, 130, 256]
    bsel = ["tb+1", "tb-1", 1, 2, "tb+1", 3]
    out = []
    for i, T in enumerate(Ts):
        tb, _ = batch_rows_per_tile(T, tile)
        B = {"tb+1": tb + 1, "tb-1": max(tb - 1, 1)}.get(bsel[i % len(bsel)], bsel[i % len(bsel)])
        out.append((B, T, cins[i % len(cins)], ns[i % len(ns)], i % 3 == 1))
    out.append((193, 5, cins[-1], ns[-1], False))
    out.append((193, 65, 16, 96, True))
    return out


def _s1_problem(K, nck, B, T, Cin, N, seed):
    """x, w and the fp64 (value, M) of one stride-1 case: NCK = the forward of a Conv1d whose weight is (N, Cin, K); CNK = the
    data gradient over a Conv1d weight (Cout = Cin of this GEMM, N, K), flipped."""
    x = rnd(B, T, Cin, seed=seed)
    if nck:
        w = rnd(N, Cin, K, seed=seed + 1, scale=0.05)
        return x, w, W.gather_s1(x, w, K)
    w = rnd(Cin, N, K, seed=seed + 1, scale=0.05)
    return x, w, W.gather_s1(x, w, K, flip=True)


def _s1_run(ops, nck, x, w, y, **kw):
    return (ops.conv1d_fwd if nck else ops.conv1d_dgrad)(x, w, y, 1, **kw)


@pytest.mark.parametrize("K,nck,tile", S1_INSTANCES, ids=[wsym(1, i[0], False, i[1], i[2]) for i in S1_INSTANCES])
def test_stride1_edge_shapes(ops, hook, monkeypatch, capsys, K, nck, tile):
    monkeypatch.setenv("MG_FORCE_TILE", str(tile))
    monkeypatch.delenv("MG_SPLITK_TARGET", raising=False)
    worst, n_tt, lgs = Worst(f"a. {wsym(1, K, False, nck, tile)}"), [], set()
    for i, (B, T, Cin, N, padded) in enumerate(s1_edge_cases(K, tile)):
        x, w, acc = _s1_problem(K, nck, B, T, Cin, N, seed=10 * i)
        what = f"K={K} nck={nck} tile={tile} B={B} T={T} Cin={Cin} N={N}"
        n_tt.append(batch_rows_per_tile(T, tile)[1])
        lgs.add(min((T - 1).bit_length(), 6 + tile // 20))
        bias = rnd(N, seed=3)
        Ty = T + 2 if padded else T
        y = S.Guarded((B, Ty, N), fill=7.0 if padded else float("nan"))
        hook.seen.clear()
        _s1_run(ops, nck, x, w, y.t, bias=bias)
        assert hook.seen == [wsym(1, K, False, nck, tile)], (what, hook.seen)
        worst.check(y.t[:, :T], W.Ref(acc[0], acc[1], K * Cin).epilogue(bias=bias), what)
        y.check(what)
        if padded:
            assert bool((y.t[:, T:] == 7.0).all()), what + ": rows beyond Tout written"
        if i % 4 == 0:                      # the occupancy pad changes the LDS request, not a bit of the result
            y2 = S.Guarded((B, Ty, N), fill=7.0 if padded else float("nan"))
            if nck:
                ops.conv_gather(x, w, y2.t, N, K, 1, Cin * K, K, lds_pad=42000, bias=bias)
            else:
                ops.conv1d_dgrad(x, w, y2.t, 1, lds_pad=42000, bias=bias)
            assert torch.equal(y2.t, y.t), what + ": lds_pad changed the result"
            y2.check(what + " lds_pad")
    assert max(n_tt) >= 3 and len(lgs) >= 4
    worst.report(capsys)


@pytest.mark.parametrize("K,nck,tile", S1_INSTANCES, ids=[wsym(1, i[0], False, i[1], i[2]) for i in S1_INSTANCES])
def test_stride1_every_epilogue_piece_in_the_gemm_kernel(ops, hook, monkeypatch, capsys, K, nck, tile):
    """Unsplit (Cin < 64: no workspace is offered), so the epilogue runs in conv_wgemm_kernel itself; N = 130 takes its
    scalar stores, N = 96 the vector ones; a partial last time tile and a ragged batch group."""
    monkeypatch.setenv("MG_FORCE_TILE", str(tile))
    monkeypatch.delenv("MG_SPLITK_TARGET", raising=False)
    worst = Worst(f"a. epilogues in {wsym(1, K, False, nck, tile)}")
    for B, T, Cin, N in ((3, 70, 48, 130), (5, 9, 24, 96)):
        assert ops.conv_plan(B, T, Cin, N, K, 1)[0] == 1
        x, w, acc = _s1_problem(K, nck, B, T, Cin, N, seed=3)
        for misalign in (False, True):
            for name, epi, repi in _epilogue_cases(ops, (B, T, N), N, misalign=misalign):
                if misalign and name in ("bias", "scale/shift", "accumulate"):
                    continue
                hook.seen.clear()
                _run_epilogue_case(lambda y, **e: _s1_run(ops, nck, x, w, y, **e), (B, T, N), epi, repi, acc, K * Cin, worst,
                                   f"{name} misalign={misalign} K={K} nck={nck} tile={tile} N={N}", misalign)
                assert hook.seen == [wsym(1, K, False, nck, tile)], hook.seen
    worst.report(capsys)


# channel counts that are not multiples of 4 (rows off the 16-byte grid) and operands that start off it: (B, T, Cin, N)
ODD_S1 = [(3, 37, 18, 17), (2, 65, 50, 33), (1, 9, 9, 9), (4, 5, 67, 131)]


@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("nck", [True, False], ids=["nck", "cnk"])
def test_stride1_odd_channel_counts_and_misaligned_operands(ops, hook, monkeypatch, capsys, K, nck):
    monkeypatch.delenv("MG_FORCE_TILE", raising=False)
    monkeypatch.delenv("MG_SPLITK_TARGET", raising=False)
    worst = Worst(f"a. odd channels / misaligned, K={K} nck={nck}")
    for i, (B, T, Cin, N) in enumerate(ODD_S1):
        x, w, acc = _s1_problem(K, nck, B, T, Cin, N, seed=i)
        for mis in (False, True):
            y = S.Guarded((B, T, N))
            hook.seen.clear()
            _s1_run(ops, nck, off4(x) if mis else x, off4(w) if mis else w, y.t)
            assert hook.seen == [wsym(1, K, False, nck, 11)], hook.seen
            what = f"K={K} nck={nck} B={B} T={T} Cin={Cin} N={N} misaligned={mis}"
            worst.check(y.t, W.Ref(acc[0], acc[1], K * Cin), what)
            y.check(what)
    worst.report(capsys)


def test_k5_t1_on_the_128_tile_is_refused_on_the_host(ops, hook, monkeypatch):
    """The one (instantiation, edge) pair of section a that cannot run: 128 batch rows x 5 window rows x 2 buffers exceed the
    160 KiB of LDS.  The library says so before any launch; nothing is written."""
    monkeypatch.setenv("MG_FORCE_TILE", "22")
    x, w, _ = _s1_problem(5, True, 3, 1, 16, 96, seed=1)
    y = S.Guarded((3, 1, 96))
    with pytest.raises(RuntimeError, match="LDS"):
        ops.conv1d_fwd(x, w, y.t, 1)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.t).all())
    y.check("refused")


# K = 1 above 512 rows through the Linear entry points (rows, in, out)
LINEAR_BIG = [(513, 100, 130), (777, 256, 96), (600, 24, 256)]


@pytest.mark.parametrize("tile", TILES)
def test_k1_through_the_linear_entry_points_above_512_rows(ops, hook, monkeypatch, capsys, tile):
    monkeypatch.setenv("MG_FORCE_TILE", str(tile))
    monkeypatch.delenv("MG_SPLITK_TARGET", raising=False)
    worst = Worst(f"a. Linear > 512 rows, tile {tile}")
    for i, (M, Kin, N) in enumerate(LINEAR_BIG):
        x, w, bias = rnd(M, Kin, seed=i), rnd(N, Kin, seed=i + 1, scale=0.05), rnd(N, seed=i + 2)
        y = S.Guarded((M, N))
        hook.seen.clear()
        ops.linear_fwd(x, w, y.t, bias=bias, act=ops.ACT_LRELU)
        assert hook.seen == [wsym(1, 1, False, True, tile)], hook.seen
        worst.check(y.t, W.Ref(*W.linear(x, w), Kin).epilogue(bias=bias, act=S.ACT_LRELU), f"linear_fwd {M}x{Kin}->{N}")
        y.check("linear_fwd")
        dy = rnd(M, N, seed=i + 3)
        dx = S.Guarded((M, Kin))
        hook.seen.clear()
        ops.linear_dgrad(dy, w, dx.t)
        assert hook.seen == [wsym(1, 1, False, False, tile if Kin > 64 else 11)], hook.seen
        worst.check(dx.t, W.Ref(*W.linear_dgrad(dy, w), N), f"linear_dgrad {M}x{N}->{Kin}")
        dx.check("linear_dgrad")
    worst.report(capsys)


# ---------------------------------------------------------------------------------------------------------------------
# b. split-K: blockIdx.z slabs + conv_finish_kernel<VEC>
# ---------------------------------------------------------------------------------------------------------------------
SPLIT_TARGET = "100000"
# (K, NCK, B, T, Cin, N, ksplit, cps): chunks are 16 channels (64 for K = 1); an uneven last slab where nchunks % cps != 0
SPLIT_CASES = [
    (3, True, 3, 33, 80, 96, 2, 3),          # 5 chunks -> 3 + 2
    (3, False, 2, 16, 176, 96, 4, 3),        # 11 chunks -> 3 + 3 + 3 + 2
    (3, True, 2, 64, 256, 130, 8, 2),        # N % 4 != 0: the scalar finish
    (5, False, 3, 7, 80, 32, 2, 3),
    (5, True, 1, 130, 128, 96, 4, 2),
    (5, False, 2, 20, 272, 64, 6, 3),        # 17 chunks: planned 8 slabs of 3 chunks = six slabs, 3 x 5 + 2
    (5, True, 2, 20, 256, 64, 8, 2),
    (1, True, 5, 9, 320, 96, 2, 3),          # 5 chunks of 64
    (1, False, 3, 16, 512, 130, 4, 2),
    (1, True, 2, 5, 1024, 64, 8, 2),
    (1, False, 1, 3, 1100, 96, 6, 3),        # 18 chunks (the last one partial) -> six slabs of 3
]


def _epilogue_cases(ops, shape, N, seed=40, misalign=False):
    """(name, ops keywords, reference keywords) covering every epilogue piece; the keyword 'zout' / 'base' are filled by the
    caller.  misalign: the elementwise tensors start 4 bytes past a 16-byte boundary."""
    bias, scale, shift, gscale = rnd(N, seed=seed), rnd(N, seed=seed + 1), rnd(N, seed=seed + 2), rnd(N, seed=seed + 3)
    gref, emul = rnd(*shape, seed=seed + 4), rnd(*shape, seed=seed + 5)
    if misalign:
        gref, emul = off4(gref), off4(emul)
    gref_t = torch.tanh(gref)
    if misalign:
        gref_t = off4(gref_t)
    cases = [("bias", dict(bias=bias), dict(bias=bias)),
             ("scale/shift", dict(bias=bias, scale=scale, shift=shift), dict(bias=bias, scale=scale, shift=shift)),
             ("emul+gscale", dict(emul=emul, gscale=gscale), dict(emul=emul, gscale=gscale)),
             ("accumulate", dict(bias=bias, accumulate=True), dict(bias=bias, base=True))]
    for a in ACTS:
        cases.append((f"zout+act{a}", dict(bias=bias, act=a, zout=True), dict(bias=bias, act=a, zout=True)))
        g = gref_t if a == S.ACT_TANH else gref
        cases.append((f"gref gact{a}", dict(gref=g, gact=a, gscale=gscale), dict(gref=g, gact=a, gscale=gscale)))
    return cases


def _run_epilogue_case(launch, shape, epi, repi, acc, n, worst, what, misalign=False, extra_n=0):
    """launch(y, **epi) into guarded outputs; checks y (and zout) against the reference epilogue."""
    epi, repi = dict(epi), dict(repi)
    y = S.Guarded(shape)
    if repi.get("base") is True:
        repi["base"] = rnd(*shape, seed=77)
        y.t.copy_(repi["base"])
    z = None
    if epi.pop("zout", False):
        z = S.Guarded(shape)
        epi["zout"] = off4(z.t) if misalign else z.t
    launch(y.t, **epi)
    epi["y"] = y.t
    ref = W.Ref(acc[0].reshape(shape).clone(), acc[1].reshape(shape).clone(), n + extra_n).epilogue(**repi)
    worst.check(y.t, ref, what)
    y.check(what)
    if z is not None:
        worst.check(epi["zout"], ref.z, what + " zout")
        z.check(what + " zout")
    return epi


@pytest.mark.parametrize("case", SPLIT_CASES, ids=[f"K{c[0]}-{'nck' if c[1] else 'cnk'}-Cin{c[4]}-N{c[5]}-ks{c[6]}" for c in SPLIT_CASES])
def test_split_k_every_epilogue_piece(ops, hook, monkeypatch, capsys, case):
    K, nck, B, T, Cin, N, ksplit, cps = case
    monkeypatch.setenv("MG_SPLITK_TARGET", SPLIT_TARGET)
    monkeypatch.delenv("MG_FORCE_TILE", raising=False)
    assert ops.conv_plan(B, T, Cin, N, K, 1) == (ksplit, cps)
    nchunks = -(-Cin // (64 if K == 1 else 16))
    assert -(-nchunks // cps) == ksplit
    x, w, acc = _s1_problem(K, nck, B, T, Cin, N, seed=5)
    worst = Worst(f"b. split-K {wsym(1, K, False, nck, 11)} ksplit={ksplit}")
    variants = set()
    for misalign in (False, True):
        for name, epi, repi in _epilogue_cases(ops, (B, T, N), N, misalign=misalign):
            if misalign and name in ("bias", "scale/shift", "accumulate"):
                continue                                  # nothing elementwise to misalign
            hook.seen.clear()
            used = _run_epilogue_case(lambda y, **e: _s1_run(ops, nck, x, w, y, **e), (B, T, N), epi, repi, acc, K * Cin, worst,
                                      f"{name} misalign={misalign} {case}", misalign)
            assert hook.seen == [wsym(1, K, False, nck, 11)], hook.seen
            # which conv_finish_kernel<VEC> followed: the launch's own predicate (mg_conv_finish_vec), fed with the tensors used
            variants.add(ops.conv_finish_vec(used["y"], N, used.get("zout"), used.get("gref"), used.get("emul")))
    assert variants == ({False} if N % 4 else {True, False})
    worst.report(capsys)


@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("tile", [12, 22])
def test_split_k_on_the_wide_tiles(ops, hook, monkeypatch, capsys, tile, K):
    """The blockIdx.z slab path of conv_wgemm_kernel<1,K,false,NCK,1,2> and <..,2,2>: tile and split both forced, the plan
    read back (mg_conv_plan sees MG_FORCE_TILE as the launch does)."""
    monkeypatch.setenv("MG_SPLITK_TARGET", SPLIT_TARGET)
    monkeypatch.setenv("MG_FORCE_TILE", str(tile))
    worst = Worst(f"b. split-K on tile {tile}, K={K}")
    for B, T, Cin, N in ((2, 70, 1024 if K == 1 else 256, 96), (3, 9, 320 if K == 1 else 80, 130)):
        ks, cps = ops.conv_plan(B, T, Cin, N, K, 1)
        assert ks > 1 and ks == (8 if Cin in (256, 1024) else 2), (ks, cps)
        for nck in (True, False):
            x, w, acc = _s1_problem(K, nck, B, T, Cin, N, seed=K)
            bias, gref = rnd(N, seed=1), rnd(B, T, N, seed=2)
            for name, epi, repi in (("bias+lrelu+zout", dict(bias=bias, act=ops.ACT_LRELU, zout=True), dict(bias=bias, act=S.ACT_LRELU, zout=True)),
                                    ("gref relu", dict(gref=gref, gact=ops.ACT_RELU), dict(gref=gref, gact=S.ACT_RELU)),
                                    ("accumulate", dict(accumulate=True), dict(base=True))):
                hook.seen.clear()
                _run_epilogue_case(lambda y, **e: _s1_run(ops, nck, x, w, y, **e), (B, T, N), epi, repi, acc, K * Cin, worst,
                                   f"{name} tile={tile} K={K} nck={nck} Cin={Cin} N={N} ksplit={ks}")
                assert hook.seen == [wsym(1, K, False, nck, tile)], hook.seen
    worst.report(capsys)


def test_split_k_workspace_too_small_falls_back_to_one_slab(ops, monkeypatch, capsys):
    """mg_conv1d_gather with a workspace one byte short of the planned split: the plan query says ksplit = 1, the launch
    runs unsplit (the workspace, prefilled with NaN, stays NaN) and the result passes."""
    from melo_gan_amd import _lib as L
    monkeypatch.setenv("MG_SPLITK_TARGET", SPLIT_TARGET)
    lib = L.load()
    B, T, Cin, N, K = 2, 64, 256, 96, 3
    x, w, acc = _s1_problem(K, True, B, T, Cin, N, seed=9)
    total = B * T * N
    ks, cps = C.c_int(), C.c_int()
    for nbytes, want in ((8 * total * 4, 8), (8 * total * 4 - 1, 1)):
        assert lib.mg_conv_plan(B, T, T, N, Cin, K, 1, 0, nbytes, C.byref(ks), C.byref(cps)) == 0
        assert ks.value == want, (nbytes, ks.value)
        work = torch.full((8 * total,), float("nan"), device="cuda")
        y = S.Guarded((B, T, N))
        e = ops.epilogue((B, T, N), N)
        rc = lib.mg_conv1d_gather(x.data_ptr(), w.data_ptr(), y.t.data_ptr(), B, T, Cin, N, K, 1, 0, Cin * K, K, T * Cin, T * N,
                                  C.byref(e), work.data_ptr(), nbytes, 0, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        L.check(rc, "mg_conv1d_gather")
        W.check(y.t, W.Ref(acc[0], acc[1], K * Cin), f"workspace {nbytes} bytes")
        y.check("workspace")
        assert bool(torch.isnan(work).all()) == (want == 1)


# the stride-2 window GEMMs (what the engine takes where conv16 does not apply) under a forced split: (transposed, B, Tin,
# Cin, N, odd, ksplit)
SPLIT_S2 = [(False, 3, 67, 80, 96, False, 2), (False, 2, 33, 256, 130, False, 8), (True, 3, 34, 128, 96, False, 4),
            (True, 2, 17, 80, 130, True, 2)]


@pytest.mark.parametrize("case", SPLIT_S2, ids=[f"{'scatter' if c[0] else 'gather'}-Cin{c[3]}-N{c[4]}-ks{c[6]}" for c in SPLIT_S2])
def test_split_k_stride2_fallback(ops, hook, monkeypatch, capsys, case):
    tr2, B, Tin, Cin, N, odd, ksplit = case
    monkeypatch.setenv("MG_SPLITK_TARGET", SPLIT_TARGET)
    monkeypatch.delenv("MG_FORCE_TILE", raising=False)
    assert ops.conv_plan(B, Tin, Cin, N, 5, 2, scatter2=tr2, odd=odd)[0] == ksplit
    x = rnd(B, Tin, Cin, seed=1)
    worst = Worst(f"b. split-K stride 2 {'scatter' if tr2 else 'gather'} ksplit={ksplit}")
    bias, gref = rnd(N, seed=3), None
    if tr2:
        w = rnd(Cin, N, 5, seed=2, scale=0.05)
        Tout = 2 * Tin - (1 if odd else 0)
        acc = S.scatter(x, w, Tout)
        run = (lambda y, **e: ops.conv1d_dgrad(x, w, y, 2, **e)) if odd else (lambda y, **e: ops.convT1d_fwd(x, w, y, **e))
    else:
        w = rnd(N, Cin, 5, seed=2, scale=0.05)
        Tout = S.tm_gather(Tin)
        acc = S.gather(x, w)
        run = lambda y, **e: ops.conv1d_fwd(x, w, y, 2, **e)  # noqa: E731
    gref = rnd(B, Tout, N, seed=4)
    for name, epi, repi in (("bias+lrelu+zout", dict(bias=bias, act=ops.ACT_LRELU, zout=True), dict(bias=bias, act=S.ACT_LRELU, zout=True)),
                            ("gref relu", dict(gref=gref, gact=ops.ACT_RELU), dict(gref=gref, gact=S.ACT_RELU)),
                            ("accumulate", dict(accumulate=True), dict(base=True))):
        hook.seen.clear()
        _run_epilogue_case(run, (B, Tout, N), epi, repi, acc, 5 * Cin, worst, f"{name} {case}")
        assert hook.seen == [wsym(2, 5, tr2, not tr2, 11)], hook.seen
    worst.report(capsys)


# ---------------------------------------------------------------------------------------------------------------------
# c. wino3_kernel
# ---------------------------------------------------------------------------------------------------------------------
# (B, T, Cin, N): a workgroup owns 128 rows of one sequence -- a lone partial tile, an exact one, a second tile holding one
# output pair, the halo across the row 127 / 128 seam
WINO_CASES = [(1, 2, 16, 64), (2, 4, 48, 192), (5, 6, 16, 256), (2, 126, 48, 64), (5, 128, 16, 64), (1, 130, 256, 64),
              (2, 254, 16, 192), (1, 256, 48, 256), (5, 258, 16, 64), (2, 384, 256, 192)]


def _in_canvas(t, fill=1.0e3, rows=8):
    """A copy of t (B, T, C) inside a buffer of non-zero values: what lies before sample 0 and after the last sample must
    never be read as a halo row."""
    pad = rows * t.shape[-1]
    canvas = torch.full((t.numel() + 2 * pad,), fill, device=t.device)
    v = canvas[pad:pad + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 0
    return v, canvas


@pytest.mark.parametrize("flip", [False, True], ids=["forward", "flipped"])
def test_wino3_edge_shapes(ops, hook, capsys, flip):
    ww, wd = Worst(f"c. wino3_kernel flip={flip}"), Worst(f"c. direct kernel at wino3's shapes flip={flip}")
    for i, (B, T, Cin, N) in enumerate(WINO_CASES):
        assert ops.wino3_supported(B, T, Cin, N)
        x, canvas = _in_canvas(rnd(B, T, Cin, seed=i))
        what = f"wino B={B} T={T} Cin={Cin} N={N} flip={flip}"
        if flip:           # the data gradient of a Conv1d whose weight is (Cout = Cin here, N, 3)
            w = rnd(Cin, N, 3, seed=i + 50, scale=0.05)
            wt = ops.wino3_weights(w, N, Cin, 3, 3 * N, flip=True)
        else:
            w = rnd(N, Cin, 3, seed=i + 50, scale=0.05)
            wt = ops.wino3_weights(w, N, Cin, 3 * Cin, 3)
        bias = rnd(N, seed=i + 60)
        y = S.Guarded((B, T, N))
        hook.seen.clear()
        ops.conv_wino3(x, wt, y.t, bias=bias)
        assert hook.seen == ["wino3_kernel"]
        val, mag, n = W.wino3(x, w, flip)
        ww.check(y.t, W.Ref(val, mag, n).epilogue(bias=bias), what)
        y.check(what)
        assert bool((canvas[:8 * Cin] == 1.0e3).all()) and bool((canvas[-8 * Cin:] == 1.0e3).all())
        yd = S.Guarded((B, T, N))
        hook.seen.clear()
        _s1_run(ops, not flip, x, w, yd.t, bias=bias)
        assert hook.seen == [wsym(1, 3, False, not flip, 11)]
        wd.check(yd.t, W.Ref(*W.gather_s1(x, w, 3, flip), 3 * Cin).epilogue(bias=bias), "direct " + what)
        yd.check("direct " + what)
    ww.report(capsys)
    wd.report(capsys)


def test_wino3_refuses_a_misaligned_input(ops, hook):
    x, w = off4(rnd(2, 130, 16, seed=1)), rnd(64, 16, 3, seed=2)
    y = S.Guarded((2, 130, 64))
    with pytest.raises(RuntimeError, match="aligned"):
        ops.conv_wino3(x, ops.wino3_weights(w, 64, 16, 48, 3), y.t)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.t).all())


@pytest.mark.parametrize("flip", [False, True], ids=["forward", "flipped"])
@pytest.mark.parametrize("B,T,Cin,N", [(2, 130, 48, 64), (1, 256, 16, 192)])
def test_wino3_every_epilogue_piece(ops, hook, capsys, B, T, Cin, N, flip):
    x = rnd(B, T, Cin, seed=1)
    if flip:
        w = rnd(Cin, N, 3, seed=2, scale=0.05)
        wt = ops.wino3_weights(w, N, Cin, 3, 3 * N, flip=True)
    else:
        w = rnd(N, Cin, 3, seed=2, scale=0.05)
        wt = ops.wino3_weights(w, N, Cin, 3 * Cin, 3)
    val, mag, n = W.wino3(x, w, flip)
    worst = Worst(f"c. wino3_kernel epilogues T={T} flip={flip}")
    for name, epi, repi in _epilogue_cases(ops, (B, T, N), N):
        hook.seen.clear()
        _run_epilogue_case(lambda y, **e: ops.conv_wino3(x, wt, y, **e), (B, T, N), epi, repi, (val, mag), n, worst, f"wino {name}")
        assert hook.seen == ["wino3_kernel"]
    worst.report(capsys)


# ---------------------------------------------------------------------------------------------------------------------
# d. linear_skinny_kernel<W_KCONTIG, VEC> (+ linear_finish_kernel)
# ---------------------------------------------------------------------------------------------------------------------
# (M, K, N, forward?, misaligned operand or None, expected <W_KCONTIG, VEC>, expected ksplit).  forward: x (M, K) @ w (N, K)^T,
# K contiguous in w; otherwise the data gradient dy (M, K) @ w (K, N): N contiguous.  VEC needs K % (64 * ksplit) == 0 and
# aligned operands.
SKINNY_CASES = [
    (1, 6, 1, True, None, (True, False), 1),
    (31, 8, 31, True, None, (True, False), 1),
    (32, 64, 33, True, None, (True, True), 1),
    (33, 100, 130, True, None, (True, False), 1),
    (512, 192, 33, True, None, (True, True), 1),          # span 24: none of the unrolled cases
    (33, 1000, 31, True, None, (True, False), 1),
    (31, 2048, 33, True, None, (True, True), 2),
    (33, 8192, 31, True, None, (True, True), 8),
    (1, 8192, 1, True, None, (True, True), 8),
    (32, 64, 8192, True, None, (True, True), 1),
    (32, 64, 33, True, "x", (True, False), 1),            # would vectorise, but x starts off a 16-byte boundary
    (32, 64, 33, True, "w", (True, False), 1),
    (31, 2000, 33, True, None, (True, False), 2),         # split and not vectorised: 2000 % 128 != 0
    (1, 6, 1, False, None, (True, False), 1),             # N = 1: both weight strides are 1, which reads as K-contiguous
    (1, 6, 33, False, None, (False, False), 1),
    (31, 8, 31, False, None, (False, False), 1),
    (32, 64, 33, False, None, (False, True), 1),
    (33, 100, 130, False, None, (False, False), 1),
    (512, 192, 130, False, None, (False, True), 1),
    (33, 1000, 31, False, None, (False, False), 1),
    (31, 2048, 33, False, None, (False, True), 2),
    (33, 8192, 31, False, None, (False, True), 8),
    (32, 64, 8192, False, None, (False, True), 1),
    (32, 64, 33, False, "x", (False, False), 1),
    (32, 64, 33, False, "w", (False, True), 1),           # N-contiguous weights are read with scalar loads either way
]
# (M, K, N, perm_L, expected ksplit) on the skinny kernel; the last one takes the window-GEMM route unless MG_LINEAR_SKINNY_ONLY
PERM_CASES = [(5, 40, 96, 8, 1), (33, 512, 130 * 4, 4, 1), (4, 2048, 64, 8, 2), (31, 4096, 96, 32, 4)]
PRE2 = (128, 512, 8192, 32)


def skinny_sym(kcontig, vec):
    b = lambda v: "true" if v else "false"  # noqa: E731
    return f"linear_skinny_kernel<{b(kcontig)},{b(vec)}>"


def test_skinny_every_instantiation(ops, hook, capsys):
    worst, seen = Worst("d. linear_skinny_kernel"), set()
    for i, (M, K, N, fwd, mis, inst, ksplit) in enumerate(SKINNY_CASES):
        what = f"skinny M={M} K={K} N={N} fwd={fwd} misaligned={mis}"
        x = rnd(M, K, seed=i)
        w = rnd(N, K, seed=i + 1, scale=0.05) if fwd else rnd(K, N, seed=i + 1, scale=0.05)
        x, w = (off4(x) if mis == "x" else x), (off4(w) if mis == "w" else w)
        bias = rnd(N, seed=i + 2)
        route = ops.linear_route(M, K, N, K if fwd else 1, 1 if fwd else N, 0, x.data_ptr() % 16 == 0, w.data_ptr() % 16 == 0)
        assert route == (skinny_sym(*inst), ksplit), (what, route)
        y = S.Guarded((M, N))
        hook.seen.clear()
        if fwd:
            ops.linear_fwd(x, w, y.t, bias=bias, act=ops.ACT_RELU)
            acc = W.linear(x, w)
        else:
            ops.linear_dgrad(x, w, y.t, bias=bias, act=ops.ACT_RELU)
            acc = W.linear_dgrad(x, w)
        assert hook.seen == [skinny_sym(*inst)], (what, hook.seen)
        seen.add((inst, ksplit > 1))
        worst.check(y.t, W.Ref(*acc, K).epilogue(bias=bias, act=S.ACT_RELU), what)
        y.check(what)
    assert {s[0] for s in seen} == {(a, b) for a in (True, False) for b in (True, False)}
    assert {(True, True), (True, False), (False, True)} <= {(s[0][1], s[1]) for s in seen}      # split with and without VEC
    worst.report(capsys)


# odd lengths, K below a wave's 8-deep step, operands off the 16-byte grid: (M, K, N)
ODD_SKINNY = [(3, 7, 3), (33, 13, 65), (512, 1, 1), (2, 1030, 5), (7, 4100, 9)]


def test_skinny_odd_lengths_and_misaligned_operands(ops, hook, capsys):
    worst = Worst("d. linear_skinny_kernel, odd lengths")
    for i, (M, K, N) in enumerate(ODD_SKINNY):
        for fwd in (True, False):
            x = rnd(M, K, seed=i)
            w = rnd(N, K, seed=i + 1, scale=0.05) if fwd else rnd(K, N, seed=i + 1, scale=0.05)
            acc = W.linear(x, w) if fwd else W.linear_dgrad(x, w)
            for mis in (None, "x", "w"):
                y = S.Guarded((M, N))
                hook.seen.clear()
                (ops.linear_fwd if fwd else ops.linear_dgrad)(off4(x) if mis == "x" else x, off4(w) if mis == "w" else w, y.t)
                assert len(hook.seen) == 1 and hook.seen[0].startswith("linear_skinny_kernel<"), hook.seen
                what = f"skinny M={M} K={K} N={N} fwd={fwd} misaligned={mis}"
                worst.check(y.t, W.Ref(*acc, K), what)
                y.check(what)
    worst.report(capsys)


@pytest.mark.parametrize("M,K,N,ksplit", [(33, 8192, 31, 8), (33, 100, 130, 1), (32, 64, 33, 1)])
def test_skinny_every_epilogue_piece_in_the_kernel_and_in_the_finish_kernel(ops, hook, capsys, M, K, N, ksplit):
    """ksplit = 1: the epilogue runs in linear_skinny_kernel (scalar and vector loads of the operands); ksplit = 8: in
    linear_finish_kernel.  Forward and data-gradient layout."""
    worst = Worst(f"d. skinny epilogues K={K} ksplit={ksplit}")
    for fwd in (True, False):
        x = rnd(M, K, seed=1)
        w = rnd(N, K, seed=2, scale=0.05) if fwd else rnd(K, N, seed=2, scale=0.05)
        sym, ks = ops.linear_route(M, K, N, K if fwd else 1, 1 if fwd else N)
        assert ks == ksplit
        acc = W.linear(x, w) if fwd else W.linear_dgrad(x, w)
        run = ops.linear_fwd if fwd else ops.linear_dgrad
        for name, epi, repi in _epilogue_cases(ops, (M, N), N):
            hook.seen.clear()
            _run_epilogue_case(lambda y, **e: run(x, w, y, **e), (M, N), epi, repi, acc, K, worst, f"{name} fwd={fwd} ksplit={ks}")
            assert hook.seen == [sym]
    worst.report(capsys)


def _perm_case(ops, hook, worst, M, K, N, L, want_sym, want_ks):
    x, w, bias = rnd(M, K, seed=M), rnd(N, K, seed=M + 1, scale=0.05), rnd(N, seed=M + 2)
    assert ops.linear_route(M, K, N, K, 1, L) == (want_sym, want_ks)
    y, z = S.Guarded((M, L, N // L)), S.Guarded((M, L, N // L))
    hook.seen.clear()
    ops.linear_fwd(x, w, y.t, perm_L=L, bias=bias, act=ops.ACT_RELU, zout=z.t)
    assert hook.seen == [want_sym], hook.seen
    idx = W.perm_index(N, L, "cuda")
    ref = W.Ref(*W.linear(x, w, L), K).epilogue(bias=bias[idx], act=S.ACT_RELU, zout=True)
    what = f"perm M={M} K={K} N={N} L={L} {want_sym} ksplit={want_ks}"
    worst.check(y.t.view(M, N), ref, what)
    worst.check(z.t.view(M, N), ref.z, what + " zout")
    y.check(what)
    z.check(what + " zout")
    # the same numbers as the unpermuted Linear, moved: column n' holds weight row idx[n']
    plain = torch.empty(M, N, device="cuda")
    ops.linear_fwd(x, w, plain, bias=bias, act=ops.ACT_RELU)
    W.check(plain[:, idx], ref, what + " (plain, gathered)")


def test_permuted_linear_on_the_skinny_kernel(ops, hook, monkeypatch, capsys):
    monkeypatch.delenv("MG_LINEAR_SKINNY_ONLY", raising=False)
    worst = Worst("d. permuted Linear, skinny kernel")
    for M, K, N, L, ks in PERM_CASES:
        _perm_case(ops, hook, worst, M, K, N, L, skinny_sym(True, K % (64 * ks) == 0), ks)
    worst.report(capsys)


def test_permuted_linear_window_gemm_route_and_skinny_only(ops, hook, monkeypatch, capsys):
    """decoder.pre.2 at the fused step's 128 rows: routed to the 64x64-tile window GEMM; MG_LINEAR_SKINNY_ONLY=1 keeps it on
    the skinny kernel.  Both within the bound."""
    M, K, N, L = PRE2
    worst = Worst("d. permuted Linear 128 x 512 -> 8192, both routes")
    monkeypatch.delenv("MG_LINEAR_SKINNY_ONLY", raising=False)
    monkeypatch.delenv("MG_FORCE_TILE", raising=False)
    _perm_case(ops, hook, worst, M, K, N, L, wsym(1, 1, False, True, 11), 1)
    monkeypatch.setenv("MG_LINEAR_SKINNY_ONLY", "1")
    _perm_case(ops, hook, worst, M, K, N, L, skinny_sym(True, True), 1)
    worst.report(capsys)


# ---------------------------------------------------------------------------------------------------------------------
# e. stride-1 weight gradients: wgrad_multi_kernel<1, K>
# ---------------------------------------------------------------------------------------------------------------------
TARGETS = ["1", "64", None, "100000"]
# (K, rows, T, Cin, Cout): the classifier's four convolutions (gan/engine.py emotion_disc_spec: note_dim 4 -> 64 with five taps
# -- the only production caller of wgrad_multi_kernel<1,5>, and its narrowest L operand -- then 64 -> 128 -> 256 -> 256 with three;
# 512 notes in config/ed_config.yaml, 256 at cfg2) at a small and a large batch -- a dropped sample is 48x the bound at 64 x 64
# rows but 190000x at 5 x 7, see test_window_ref.py -- and other five-tap and ragged shapes
CONV_WGRAD = [(5, 5, 512, 4, 64), (5, 64, 256, 4, 64), (3, 5, 512, 64, 128), (3, 64, 256, 64, 128), (3, 5, 256, 128, 256),
              (3, 64, 256, 128, 256), (3, 5, 512, 256, 256), (3, 64, 256, 256, 256), (3, 5, 7, 20, 12), (3, 1, 2, 16, 32),
              (5, 5, 7, 20, 12), (5, 16, 64, 64, 64), (5, 1, 2, 16, 32), (3, 193, 3, 24, 130)]
# (rows, in, out): every Linear weight of the cfg2 models that takes this kernel (numeric encoder 6 -> 256 -> 128 -> 128,
# noise_to_latent 256 -> 512 -> 64, decoder.pre 64 -> 512 -> 8192, critic fc 256 -> 256, classifier project 256 -> 256 and MLP 256
# -> 256 -> 128 -> 4) at B = 64 and at the fused step's 2B = 128 rows, and ragged ones
LINEAR_WGRAD = [(64, 6, 256), (64, 256, 128), (128, 128, 128), (64, 256, 512), (128, 512, 64), (64, 64, 512), (128, 512, 8192),
                (64, 256, 256), (64, 128, 4), (30, 100, 36), (777, 100, 130), (5, 20, 12)]


# channel counts off the 16-byte grid and misaligned operands: (rows, T, Cin, Cout)
ODD_WGRAD = [(3, 5, 7, 9), (65, 3, 18, 33), (2, 130, 130, 6)]


@pytest.mark.parametrize("K", [1, 3, 5])
def test_wgrad_stride1_odd_channel_counts_and_misaligned_operands(ops, hook, monkeypatch, capsys, K):
    monkeypatch.delenv("MG_WGRAD_TARGET", raising=False)
    worst = Worst(f"e. wgrad_multi_kernel<1,{K}>, odd channels / misaligned")
    for i, (rows, T, Cin, Cout) in enumerate(ODD_WGRAD):
        x, dy = rnd(rows, T, Cin, seed=i), rnd(rows, T, Cout, seed=i + 50)
        (rdw, mdw, n), (rdb, mdb, nb) = W.wgrad_s1(x, dy, K)
        for mis in (False, True):
            dw, db, guards = _wgrad_outputs((Cout, Cin, K), Cout)
            hook.seen.clear()
            ops.conv1d_wgrad(off4(x) if mis else x, off4(dy) if mis else dy, dw, 1, db=db)
            assert hook.seen == [f"wgrad_multi_kernel<1,{K}>"]
            what = f"dw K={K} rows={rows} T={T} Cin={Cin} Cout={Cout} misaligned={mis}"
            _check_guards(guards, what)
            worst.check(dw, W.Ref(rdw, mdw, n), what)
            worst.check(db, W.Ref(rdb, mdb, nb), what + " db")
    worst.report(capsys)


def _wgrad_outputs(wshape, nbias):
    """(dw, db) as NaN-prefilled tensors inside sentinel rows, and the two guards."""
    gw, gb = S.Guarded(wshape), S.Guarded((nbias,))
    return gw.t, gb.t, (gw, gb)


def _check_guards(guards, what):
    for g in guards:
        g.check(what)


def _set_target(monkeypatch, t):
    if t is None:
        monkeypatch.delenv("MG_WGRAD_TARGET", raising=False)
    else:
        monkeypatch.setenv("MG_WGRAD_TARGET", t)


def _twice(launch):
    outs = [launch() for _ in range(2)]
    for a, b in zip(*outs):
        assert torch.equal(a, b), "wgrad: run-to-run bits differ"
    return outs[0]


def _segments(x, dy, seg2):
    rows = x.shape[0]
    if not seg2 or rows < 2:
        return x, dy, {}
    nb0 = rows - max(rows // 3, 1)
    return x[:nb0].contiguous(), dy[:nb0].contiguous(), dict(x2=x[nb0:].contiguous(), dy2=dy[nb0:].contiguous())


@pytest.mark.parametrize("target", TARGETS, ids=lambda t: f"target={t or 'default'}")
def test_conv1d_wgrad_stride1(ops, hook, monkeypatch, capsys, target):
    _set_target(monkeypatch, target)
    worst = Worst(f"e. wgrad_multi_kernel<1,3|5> target={target}")
    for i, (K, rows, T, Cin, Cout) in enumerate(CONV_WGRAD):
        for seg2 in (False, True):
            x, dy = rnd(rows, T, Cin, seed=i), rnd(rows, T, Cout, seed=i + 50)
            x0, dy0, seg = _segments(x, dy, seg2)

            def launch():
                dw, db, guards = _wgrad_outputs((Cout, Cin, K), Cout)
                ops.conv1d_wgrad(x0, dy0, dw, 1, db=db, **seg)
                _check_guards(guards, f"K={K} rows={rows} T={T} Cin={Cin} Cout={Cout}")
                return dw, db
            hook.seen.clear()
            dw, db = _twice(launch)
            assert hook.seen == [f"wgrad_multi_kernel<1,{K}>"] * 2, hook.seen
            (rdw, mdw, n), (rdb, mdb, nb) = W.wgrad_s1(x0, dy0, K, seg.get("x2"), seg.get("dy2"))
            what = f"dw K={K} rows={rows} T={T} Cin={Cin} Cout={Cout} seg2={bool(seg)} target={target}"
            worst.check(dw, W.Ref(rdw, mdw, n), what)
            worst.check(db, W.Ref(rdb, mdb, nb), what + " db")
    worst.report(capsys)


@pytest.mark.parametrize("target", TARGETS, ids=lambda t: f"target={t or 'default'}")
def test_linear_wgrad(ops, hook, monkeypatch, capsys, target):
    _set_target(monkeypatch, target)
    worst = Worst(f"e. wgrad_multi_kernel<1,1> target={target}")
    for i, (rows, fin, fout) in enumerate(LINEAR_WGRAD):
        for seg2 in (False, True):
            x, dy = rnd(rows, fin, seed=i), rnd(rows, fout, seed=i + 50)
            x0, dy0, seg = _segments(x, dy, seg2)

            def launch():
                dw, db, guards = _wgrad_outputs((fout, fin), fout)
                ops.linear_wgrad(x0, dy0, dw, db=db, **seg)
                _check_guards(guards, f"linear rows={rows} {fin}->{fout}")
                return dw, db
            hook.seen.clear()
            dw, db = _twice(launch)
            assert hook.seen == ["wgrad_multi_kernel<1,1>"] * 2, hook.seen
            u = lambda t: None if t is None else t.unsqueeze(1)  # noqa: E731
            (rdw, mdw, n), (rdb, mdb, nb) = W.wgrad_s1(u(x0), u(dy0), 1, u(seg.get("x2")), u(seg.get("dy2")))
            what = f"linear dw rows={rows} {fin}->{fout} seg2={bool(seg)} target={target}"
            worst.check(dw, W.Ref(rdw.squeeze(2), mdw.squeeze(2), n), what)
            worst.check(db, W.Ref(rdb, mdb, nb), what + " db")
    worst.report(capsys)


@pytest.mark.parametrize("target", TARGETS, ids=lambda t: f"target={t or 'default'}")
def test_wgrad_multi_jobs_of_all_three_k(ops, hook, monkeypatch, capsys, target):
    """One wgrad_multi call holding Linear, three-tap and five-tap jobs goes out as one launch per K."""
    _set_target(monkeypatch, target)
    worst = Worst(f"e. wgrad_multi, jobs of K = 1, 3, 5 target={target}")
    specs = [(1, 64, 1, 256, 128, 0), (3, 64, 32, 64, 64, 21), (5, 5, 7, 20, 12, 2), (1, 30, 1, 100, 36, 7), (3, 5, 7, 20, 12, 0),
             (5, 16, 64, 64, 64, 0), (1, 128, 1, 512, 64, 64), (5, 64, 256, 4, 64, 0)]       # the last: the classifier's first layer
    data = []
    for i, (K, rows, T, Cin, Cout, nb1) in enumerate(specs):
        x, dy = rnd(rows, T, Cin, seed=i), rnd(rows, T, Cout, seed=i + 50)
        nb0 = rows - nb1
        data.append((K, x[:nb0].contiguous(), dy[:nb0].contiguous(), x[nb0:].contiguous() if nb1 else None,
                     dy[nb0:].contiguous() if nb1 else None, Cin, Cout))

    def launch():
        outs, jobs, guards = [], [], []
        for K, x, dy, x2, dy2, Cin, Cout in data:
            dw, db, g = _wgrad_outputs((Cout, Cin) if K == 1 else (Cout, Cin, K), Cout)
            guards += g
            if K == 1:
                f = lambda t: None if t is None else t.view(t.shape[0], -1)  # noqa: E731
                jobs.append(ops.linear_wgrad(f(x), f(dy), dw, x2=f(x2), dy2=f(dy2), db=db, defer=True))
            else:
                jobs.append(ops.conv1d_wgrad(x, dy, dw, 1, x2=x2, dy2=dy2, db=db, defer=True))
            outs += [dw, db]
        ops.wgrad_multi(jobs)
        _check_guards(guards, "wgrad_multi")
        return outs
    hook.seen.clear()
    outs = _twice(launch)
    assert hook.seen == ["wgrad_multi_kernel<1,1>", "wgrad_multi_kernel<1,3>", "wgrad_multi_kernel<1,5>"] * 2, hook.seen
    for j, (K, x, dy, x2, dy2, Cin, Cout) in enumerate(data):
        (rdw, mdw, n), (rdb, mdb, nb) = W.wgrad_s1(x, dy, K, x2, dy2)
        worst.check(outs[2 * j].view(Cout, Cin, K), W.Ref(rdw, mdw, n), f"multi job {j} {specs[j]} target={target}")
        worst.check(outs[2 * j + 1], W.Ref(rdb, mdb, nb), f"multi job {j} {specs[j]} db target={target}")
    worst.report(capsys)


# ---------------------------------------------------------------------------------------------------------------------
# f. row chain: LIN_FWD / LIN_DGRAD
# ---------------------------------------------------------------------------------------------------------------------
CHAIN_LENGTHS = [(1, 512), (5, 511), (18, 100), (33, 33), (100, 18), (511, 5), (512, 1), (512, 512), (511, 511), (1, 1)]
CHAIN_ROWS = (1, 9, 192)


def test_row_chain_linear_forward(ops, hook, capsys):
    worst = Worst("f. row chain LIN_FWD")
    for i, (K, N) in enumerate(CHAIN_LENGTHS):
        for j, rows in enumerate(CHAIN_ROWS):
            act = (0,) + ACTS
            act = act[(i + j) % 5]
            x, w, b = rnd(rows, K, seed=i), rnd(N, K, seed=i + 1, scale=0.1), rnd(N, seed=i + 2)
            mask = (torch.rand(rows, N, generator=torch.Generator().manual_seed(i + 3)) > 0.2).float().cuda() / 0.8
            assert ops.Chain.supported(K, N) and ops.Chain.weights_ok(w)
            z, wide = S.Guarded((rows, N)), S.Guarded((rows, N + 3))
            hook.seen.clear()
            ops.Chain(rows).load(0, x).linear_fwd(0, 1, w, b, act, mask, zout=z.t, out=wide.t[:, 3:]).launch()
            assert hook.seen == ["row_chain_kernel"]
            ref = W.Ref(*W.linear(x, w), K).epilogue(bias=b, zout=True, act=act, emul=mask)
            what = f"chain fwd rows={rows} K={K} N={N} act={act}"
            worst.check(wide.t[:, 3:], ref, what)
            worst.check(z.t, ref.z, what + " zout")
            assert bool(torch.isnan(wide.t[:, :3]).all()), what + ": wrote outside its column block"
            z.check(what)
            wide.check(what)
    worst.report(capsys)


def test_row_chain_linear_data_gradient(ops, hook, capsys):
    worst = Worst("f. row chain LIN_DGRAD")
    for i, (OUT, IN) in enumerate(CHAIN_LENGTHS):
        for j, rows in enumerate(CHAIN_ROWS):
            gact = ((0,) + ACTS)[(i + j) % 5]
            dy, w, gref = rnd(rows, OUT, seed=i), rnd(OUT, IN, seed=i + 1, scale=0.1), rnd(rows, IN, seed=i + 2)
            if gact == S.ACT_TANH:
                gref = torch.tanh(gref)
            mask = (torch.rand(rows, IN, generator=torch.Generator().manual_seed(i + 3)) > 0.2).float().cuda() / 0.8
            wide = S.Guarded((rows, IN + 3))
            hook.seen.clear()
            ops.Chain(rows).load(0, dy).linear_dgrad(0, 1, w, gref=gref if gact else None, gact=gact, mask=mask,
                                                     out=wide.t[:, 3:]).launch()
            assert hook.seen == ["row_chain_kernel"]
            repi = dict(gref=gref, gact=gact, emul=mask) if gact else dict(emul=mask)
            what = f"chain dgrad rows={rows} OUT={OUT} IN={IN} gact={gact}"
            worst.check(wide.t[:, 3:], W.Ref(*W.linear_dgrad(dy, w), OUT).epilogue(**repi), what)
            assert bool(torch.isnan(wide.t[:, :3]).all()), what + ": wrote outside its column block"
            wide.check(what)
    worst.report(capsys)
