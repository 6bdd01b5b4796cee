"""CPU self-test of what tests/test_thin_contract_gpu.py and tests/test_bf16_contract_gpu.py hold csrc/conv_thin.hip and
csrc/conv_bf16.hip to: (a) the references (W.thin over window_ref / stride2_ref, bf16_ref) equal torch's fp64 conv1d /
conv_transpose1d / autograd at every table shape; (b) the tables of tests/thin_bf16_tables.py reach the paths they claim --
the route rule, rpt = 1 / 2 / 4 / 8, both NMAX, the second channel pass, the 16-byte and the scalar loads and stores, odd and
even chunk counts -- recomputed on the host and compared with mg_conv_thin_route; (c) an fp32 host computation of every
operation at every table shape stays within its bound (bf16: fp32 arithmetic on bf16-rounded operands, rounded once to bf16
where the output is bf16); (d) each of twelve plausible kernel mistakes, built from the reference at table shapes, leaves
it -- the measured ratios are in test_mistakes_are_flagged's docstring.  No GPU needed."""
import pytest
import torch
import torch.nn.functional as F

import bf16_ref as R
import stride2_ref as S
import thin_bf16_tables as T
import window_ref as W

BF = torch.bfloat16
ALL_THIN = T.THIN_IN + T.THIN_OUT + T.RPT + T.EPILOGUE


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-300))


def thin_problem(case, seed=1):
    e, B, Tin, C, N, K, stride, flags = case
    x, w = rnd(B, Tin, C, seed=seed), rnd(*T.ENTRIES[e][2](C, N, K), seed=seed + 1, scale=0.3)
    return x, w, T.tout(e, Tin, K, stride, flags)


def torch_thin(case, x, w, Tout):
    """The entry point's operation by torch's own convolutions / autograd, in the dtype of x and w."""
    e, B, Tin, C, N, K, stride, flags = case
    xt = x.transpose(1, 2)
    if e == "fwd":
        return F.conv1d(xt, w, None, stride, K // 2).transpose(1, 2)
    if e == "convT_fwd":
        return F.conv_transpose1d(xt, w, None, 2, 2, 1).transpose(1, 2)
    if e == "convT_dgrad":          # x = dy (B, T, Cout of the transposed convolution), w (N, Cout, 5)
        z = torch.zeros(B, N, Tout, dtype=x.dtype, requires_grad=True)
        F.conv_transpose1d(z, w, None, 2, 2, Tin - (2 * Tout - 1)).backward(xt)
    elif e == "dgrad1":             # x = dy (B, T, Cout), w (Cout, N, K)
        z = torch.zeros(B, N, Tout, dtype=x.dtype, requires_grad=True)
        F.conv1d(z, w, None, 1, K // 2).backward(xt)
    else:                           # dgrad2
        z = torch.zeros(B, N, Tout, dtype=x.dtype, requires_grad=True)
        F.conv1d(z, w, None, 2, 2).backward(xt)
    return z.grad.transpose(1, 2)


# ---------------------------------------------------------------------------------------------------------------------
# (a) the references are the operations they claim to be
# ---------------------------------------------------------------------------------------------------------------------
def test_thin_references_are_torchs_convolutions_at_every_table_shape():
    for case in ALL_THIN:
        x, w, Tout = thin_problem(case)
        ref, mag = W.thin(case[0], x, w, case[5], case[6], Tout)
        want = torch_thin(case, x.double(), w.double(), Tout)
        assert ref.shape == (case[1], Tout, case[4]) and rel(ref, want) < 1e-12, T.case_id(case)
        assert bool((mag >= ref.abs() * (1 - 1e-12)).all())


def test_gather3_is_conv1d_k3_s2():
    for Tn in (1, 2, 7, 8):
        x, w = rnd(2, Tn, 3, seed=1).double(), rnd(5, 3, 3, seed=2).double()
        ref, mag = S.gather3(x, w)
        assert rel(ref, F.conv1d(x.transpose(1, 2), w, None, 2, 1).transpose(1, 2)) < 1e-12
        assert rel(mag, F.conv1d(x.abs().transpose(1, 2), w.abs(), None, 2, 1).transpose(1, 2)) < 1e-12


@pytest.mark.parametrize("K", [3, 5])
def test_bf16_references_are_torchs_convolutions_on_rounded_operands(K):
    for i, (B, Tn, Cin, N) in enumerate(T.BF16_SHAPES):
        x = rnd(B, Tn, Cin, seed=i)
        w = rnd(N, Cin, K, seed=i + 1, scale=0.05)
        xq, wq = x.to(BF).double(), w.to(BF).double()
        assert rel(R.conv(x, w, K).val, F.conv1d(xq.transpose(1, 2), wq, None, 1, K // 2).transpose(1, 2)) < 1e-12
        assert rel(R.conv(x.to(BF), w, K).val, R.conv(x, w, K).val) == 0.0          # rounding is idempotent
        wd = rnd(Cin, N, K, seed=i + 2, scale=0.05)                                    # data gradient over a (Cout = Cin, N, K) weight
        z = torch.zeros(B, N, Tn, dtype=torch.float64, requires_grad=True)
        F.conv1d(z, wd.to(BF).double(), None, 1, K // 2).backward(xq.transpose(1, 2))
        assert rel(R.conv(x, wd, K, flip=True).val, z.grad.transpose(1, 2)) < 1e-12
        assert rel(R.conv_fp32_host(x, wd, K, True).double(), z.grad.transpose(1, 2)) < 1e-5
    t = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8 - 2.0 ** -20])
    assert R.q(t).float().tolist() == [1.0 + 2.0 ** -7, 1.0, 1.0 + 2.0 ** -6, -1.0 - 2.0 ** -7]     # to nearest, ties to even
    assert R.truncated(t).float().tolist() == [1.0, 1.0, 1.0 + 2.0 ** -7, -1.0]


def test_relayout_is_the_permuted_rounded_weight():
    for N, Cc, K, layout in T.RELAYOUT:
        for flip in (False, True):
            w = rnd(N, Cc, K, seed=3) if layout == "nck" else rnd(Cc, N, K, seed=3)
            sn, sc = (Cc * K, K) if layout == "nck" else (K, N * K)
            wd = w if layout == "nck" else w.permute(1, 0, 2)
            assert torch.equal(R.relayout(w, N, Cc, K, sn, sc, flip), (wd.flip(2) if flip else wd).to(BF).permute(2, 0, 1))
    assert {(r[3], r[2]) for r in T.RELAYOUT} == {(lay, K) for lay in ("nck", "cnk") for K in (3, 5)}


# ---------------------------------------------------------------------------------------------------------------------
# (b) the tables reach what they claim
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from melo_gan_amd import _lib
    return _lib.load()


def test_route_rule_is_the_librarys(lib, monkeypatch):
    monkeypatch.delenv("MG_CONV_THIN", raising=False)
    for case in ALL_THIN:
        e, B, Tin, C, N, K, stride, flags = case
        tr = T.ENTRIES[e][0]
        for aligned in (True, False):
            got = lib.mg_conv_thin_route(4096 if aligned else 4100, Tin * C, C, N, K, stride, 1 if tr else 0)
            assert got == T.route(C, N, K, stride, tr, aligned), (T.case_id(case), aligned)
    for C, N, K, stride, tr in ((16, 4, 3, 2, False), (16, 4, 3, 2, True), (4, 64, 1, 1, False), (9, 9, 5, 1, False), (6, 4, 5, 1, False)):
        assert lib.mg_conv_thin_route(4096, 7 * C, C, N, K, stride, int(tr)) == T.route(C, N, K, stride, tr)
    assert T.route(16, 4, 3, 2, False) == 0 and T.route(4, 64, 3, 2, False) == 1          # K = 3 at stride 2: thin_in only


def test_thin_in_table_coverage():
    rows = lambda c: c[1] * T.tout(c[0], c[2], c[5], c[6], c[7])  # noqa: E731
    tab = T.THIN_IN
    assert all(T.route(c[3], c[4], c[5], c[6], False, "xoff" not in c[7]) == 1 for c in tab)
    assert {c[3] for c in tab} == {1, 3, 4, 8} and {c[4] for c in tab} >= {4, 6, 64, 68, 100}
    assert {rows(c) for c in tab} >= {1, 15, 16, 17}
    assert any(T.tout(*c[:3:2], c[5], c[6], c[7]) == 5 and c[1] == 7 for c in tab)
    x4s = {(T.x4(c[3], c[2], "xoff" not in c[7]), c[3] == 4) for c in tab}
    assert x4s >= {(True, True), (False, True), (False, False)}            # 16-byte loads; Cin = 4 off the grid; other Cin
    assert any(c[3] == 4 and "xoff" in c[7] for c in tab)
    vo = {(T.vec_out(c[4], T.tout(c[0], c[2], c[5], c[6], c[7]) + (3 if "ypad" in c[7] else 0), "yoff" not in c[7]), c[4] % 4 == 0) for c in tab}
    assert vo >= {(True, True), (False, True), (False, False)}
    s1 = {(c[5], c[0]) for c in tab if c[6] == 1}
    assert s1 >= {(3, "fwd"), (5, "fwd"), (3, "dgrad1"), (5, "dgrad1")}      # flip = 1 at both K
    s2 = [c for c in tab if c[6] == 2 and c[5] == 5]
    assert {c[2] for c in s2} >= {1, 2} and {c[2] % 2 for c in s2 if c[2] > 2} == {0, 1}
    assert {c[2] % 2 for c in tab if c[6] == 2 and c[5] == 3} == {0, 1}
    assert any("ypad" in c[7] for c in tab) and any("yoff" in c[7] for c in tab)
    # N = 68, 100: a partial column quad on the second blockIdx.y needs N % 4 != 0 there -- 6 is the partial quad, 68 / 100 the
    # second block
    assert any(c[4] > 64 for c in tab) and any(c[4] % 4 for c in tab) and any(c[4] > 64 and c[4] % 4 for c in tab)
    for c in T.EPILOGUE:
        assert T.route(c[3], c[4], c[5], c[6], T.ENTRIES[c[0]][0]) in (1, 2, 3)
    assert {T.route(c[3], c[4], c[5], c[6], T.ENTRIES[c[0]][0]) for c in T.EPILOGUE} == {1, 2, 3}
    assert {(T.ENTRIES[c[0]][0], T.route(c[3], c[4], c[5], c[6], T.ENTRIES[c[0]][0]) == 1) for c in T.EPILOGUE} == {(False, True), (True, False), (False, False)}


def test_thin_out_table_coverage():
    tab = T.THIN_OUT
    routes = {c: T.route(c[3], c[4], c[5], c[6], T.ENTRIES[c[0]][0]) for c in map(tuple, [c[:7] for c in tab])}
    assert all((r == 0) == (c[3] > T.THIN_OUT_CMAX) for c, r in routes.items())
    for tr in (True, False):
        sub = [c for c in tab if T.ENTRIES[c[0]][0] == tr]
        assert {T.route(c[3], c[4], c[5], c[6], tr) for c in sub} == {0, 2, 3}
        assert {c[3] for c in sub} >= ({4, 16, 64, 68, 128, 256, 260} if tr else {16, 64, 68, 128, 256, 260})
    assert {c[4] for c in tab} == {1, 3, 4, 5, 8}
    pos = {c[1] * c[2] for c in tab}
    assert pos >= {1, 15, 16, 17} and any(c[1] == 7 and c[2] == 5 for c in tab)
    assert any("odd" in c[7] for c in tab) and any("ypad" in c[7] for c in tab)
    g = {(c[5], T.ENTRIES[c[0]][1]) for c in tab if not T.ENTRIES[c[0]][0]}
    assert g == {(3, True), (5, True), (3, False), (5, False)}
    assert any(c[3] > 64 and c[3] % 64 == 4 for c in tab)                    # the second channel pass with lane 0 only
    assert all(T.rpt(c[1] * c[2]) == 1 for c in tab)
    assert [T.rpt(c[1] * c[2]) for c in T.RPT] == [2, 2, 4, 4, 8, 8, 2]
    assert [c[1] * c[2] for c in T.RPT] == [32768 + 21] * 2 + [65536 + 37] * 2 + [131072 + 53] * 2 + [32768 + 37]
    assert all(c[3] <= 16 and c[4] == 4 and T.route(c[3], c[4], c[5], c[6], T.ENTRIES[c[0]][0]) == 2 for c in T.RPT)
    assert {T.ENTRIES[c[0]][0] for c in T.RPT[0:6:2]} == {True} and {T.ENTRIES[c[0]][0] for c in T.RPT[1:6:2]} == {False}
    dead = {}
    for c in T.RPT:                           # the last workgroup: a partly live block, then (2050 blocks at rpt = 2 apart) wholly
        rows, r = c[1] * c[2], T.rpt(c[1] * c[2])           # dead iterations
        assert rows % 16, rows
        dead.setdefault(r, set()).add((r - -(-rows // 16) % r) % r)
    assert dead == {2: {0, 1}, 4: {1}, 8: {4}}
    assert [T.rpt(v) for v in (16 * 2047, 16 * 2047 + 1, 16 * 4096, 16 * 8192, 1 << 24)] == [1, 2, 4, 8, 8]


def test_bf16_table_coverage(lib):
    assert [T.nchunks(s[2]) for s in T.BF16_SHAPES] == [1, 2, 3, 5, 8]              # odd counts above 1: the break mid-ring
    assert len(T.BF16_INSTANCES) == 8 == len({T.bf16_sym(*i) for i in T.BF16_INSTANCES})
    for B, Tn, Cin, N in T.BF16_SHAPES + T.BF16_EPI_SHAPES:
        assert lib.mg_conv1d_s1_bf16_supported(B, Tn, Cin, N, 3) and lib.mg_conv1d_s1_bf16_supported(B, Tn, Cin, N, 5)
    assert any(s[1] == 128 and s[0] > 1 for s in T.BF16_SHAPES) and any(s[1] > 128 for s in T.BF16_SHAPES)
    assert any(s[3] > 64 for s in T.BF16_SHAPES) and {T.nchunks(s[2]) % 2 for s in T.BF16_EPI_SHAPES} == {0, 1}
    for bad in ((1, 100, 32, 64), (1, 128, 48, 64), (1, 128, 32, 96)):
        assert not lib.mg_conv1d_s1_bf16_supported(*bad, 3)
    assert {s[1] for s in T.MEANT_FWD} == {1, 5, 13, 17, 29, 256} and {s[2] for s in T.MEANT_FWD} == {8, 64, 72}
    # meanT_fwd_bf16: the unrolled loop runs while t + 12 < T from t = row lane 0..3: T < 13 never enters it, T % 16 leaves a tail
    assert {s[1] < 13 for s in T.MEANT_FWD} == {True, False} and any(s[1] % 16 for s in T.MEANT_FWD if s[1] > 13)
    assert all((B * Tn * C) % 2048 for B, Tn, C in T.MEANT_BWD) and {s[2] for s in T.MEANT_BWD} == {8, 72}
    assert any(B * Tn * C > 2048 for B, Tn, C in T.MEANT_BWD)


# ---------------------------------------------------------------------------------------------------------------------
# (c) a correct fp32 computation passes the bound
# ---------------------------------------------------------------------------------------------------------------------
def test_fp32_host_thin_convolutions_pass_the_bound():
    """Measured here: worst 0.23 of the bound (at n = 3 one rounding is a visible share of (3 + 4 + 1) U M)."""
    top = 0.0
    for case in ALL_THIN:
        x, w, Tout = thin_problem(case)
        bias = rnd(case[4], seed=9)
        got = torch_thin(case, x, w, Tout) + bias
        ref = W.Ref(*W.thin(case[0], x, w, case[5], case[6], Tout), case[5] * case[3]).epilogue(bias=bias)
        top = max(top, W.check(got, ref, T.case_id(case)))
    print(f"thin fp32 host: worst {top:.4f} of the bound")
    assert top <= 1.0


@pytest.mark.parametrize("K", [3, 5])
def test_fp32_host_bf16_convolutions_pass_both_bounds(K):
    """Measured here: 0.0003-0.02 of the fp32 bound; rounded once to bf16, 0.83-1.0 of bound16 (by construction)."""
    for i, (B, Tn, Cin, N) in enumerate(T.BF16_SHAPES):
        for flip in (False, True):
            x = rnd(B, Tn, Cin, seed=i)
            w = rnd(Cin, N, K, seed=i + 1, scale=0.05) if flip else rnd(N, Cin, K, seed=i + 1, scale=0.05)
            ref, got = R.conv(x, w, K, flip), R.conv_fp32_host(x, w, K, flip)
            r32 = W.check(got, ref, "fp32")
            r16 = W.check(got.to(BF), R.Out16(ref), "bf16")
            print(f"bf16 conv K={K} B={B} T={Tn} Cin={Cin} N={N} flip={flip}: {r32:.4f} of bound32, rounded to bf16 {r16:.4f} of bound16")
            assert r32 <= 1.0 and r16 <= 1.0
            # with the epilogue of a forward layer, and of a data gradient
            sc, sh, gs = rnd(N, seed=5), rnd(N, seed=6), rnd(N, seed=7)
            gref = rnd(B, Tn, N, seed=8).to(BF)
            z = got * sc + sh
            e = W.Ref(ref.val.clone(), ref.mag.clone(), ref.n).epilogue(scale=sc, shift=sh, zout=True, act=S.ACT_GELU)
            assert W.check(F.gelu(z), e, "layer") <= 1.0 and W.check(z.to(BF), R.Out16(e.z), "zout") <= 1.0
            assert W.check(F.gelu(z).to(BF), R.Out16(e), "layer bf16") <= 1.0
            base = rnd(B, Tn, N, seed=9)
            gf = S.act_grad_ref(S.ACT_GELU, gref.float())
            e = W.Ref(ref.val.clone(), ref.mag.clone(), ref.n).epilogue(gref=gref, gact=S.ACT_GELU, gscale=gs, base=base)
            assert W.check(got * gf * gs + base, e, "dgrad") <= 1.0


def test_fp32_host_meanT_passes_the_bounds():
    top = 0.0
    for i, (B, Tn, C) in enumerate(T.MEANT_FWD):
        a = (rnd(B, Tn, C, seed=i) + 0.5).to(BF)
        top = max(top, W.check(a.float().sum(1) / Tn, R.meanT_fwd(a), "meanT_fwd"))
    print(f"meanT_fwd fp32 host: worst {top:.4f}")
    top = 0.0
    for i, (B, Tn, C) in enumerate(T.MEANT_BWD):
        dh, gref, gs = rnd(B, C, seed=i), rnd(B, Tn, C, seed=i + 1).to(BF), rnd(C, seed=i + 2)
        for gact in (S.ACT_NONE, S.ACT_RELU, S.ACT_LRELU, S.ACT_GELU, S.ACT_TANH):
            g = torch.tanh(gref.float()).to(BF) if gact == S.ACT_TANH else gref
            got = (dh * (1.0 / Tn))[:, None, :] * S.act_grad_ref(gact, g.float()) * gs
            top = max(top, W.check(got.to(BF), R.meanT_bwd(dh, Tn, g, gact, gs), "meanT_bwd"))
    print(f"meanT_bwd fp32 host, rounded to bf16: worst {top:.4f} of bound16")
    assert top <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# (d) plausible mistakes leave the bound
# ---------------------------------------------------------------------------------------------------------------------
def _thin(case, seed=1):
    x, w, Tout = thin_problem(case, seed)
    val, mag = W.thin(case[0], x, w, case[5], case[6], Tout)
    return x.double(), w.double(), Tout, W.Ref(val, mag, case[5] * case[3])


CROSS = ("fwd", 7, 5, 4, 100, 5, 1, set())            # thin_in: blocks cross sample boundaries
BSAMPLE = (2, 128, 64, 64)                            # bf16: tile edge = sample edge


def _bf(shape, K, seed=1):
    B, Tn, Cin, N = shape
    x, w = rnd(B, Tn, Cin, seed=seed), rnd(N, Cin, K, seed=seed + 1, scale=0.05)
    return R.q(x).double(), R.q(w).double(), R.conv(x, w, K)


def m01_outer_tap_of_the_first_row_dropped_thin():
    x, w, Tout, ref = _thin(CROSS)
    got = ref.val.clone()
    got[1, 0] -= torch.einsum("c,nc->n", x[1, 2], w[:, :, 4])            # tap 4 of row 0 reads x[2]
    return got, ref


def m01_outer_tap_of_the_last_row_dropped_thin():
    x, w, Tout, ref = _thin(CROSS)
    got = ref.val.clone()
    got[0, -1] -= torch.einsum("c,nc->n", x[0, -3], w[:, :, 0])
    return got, ref


def _m01_bf16(out16):
    x, w, ref = _bf(BSAMPLE, 3)
    got = ref.val.clone()
    got[1, 0] -= torch.einsum("c,nc->n", x[1, 1], w[:, :, 2])
    return got, (R.Out16(ref) if out16 else ref)


def m01_outer_tap_of_the_first_row_dropped_bf16_fp32out():
    return _m01_bf16(False)


def m01_outer_tap_of_the_first_row_dropped_bf16_bf16out():
    return _m01_bf16(True)


def m02_halo_from_the_neighbouring_sample_thin():
    x, w, Tout, ref = _thin(CROSS)
    got = ref.val.clone()
    got[3, 0] += torch.einsum("kc,nck->n", x[2, -2:], w[:, :, 0:2])       # x[-2], x[-1] of sample 3 := sample 2's last rows
    return got, ref


def _m02_bf16(out16):
    x, w, ref = _bf(BSAMPLE, 3)
    got = ref.val.clone()
    got[0, -1] += torch.einsum("c,nc->n", x[1, 0], w[:, :, 2])           # x[T] of sample 0 := sample 1's first row
    return got, (R.Out16(ref) if out16 else ref)


def m02_halo_from_the_neighbouring_sample_bf16_fp32out():
    return _m02_bf16(False)


def m02_halo_from_the_neighbouring_sample_bf16_bf16out():
    return _m02_bf16(True)


def m03_flip_forgotten_in_thin_in():
    case = ("dgrad1", 2, 17, 4, 64, 3, 1, set())
    x, w, Tout, ref = _thin(case)
    return W.gather_s1(x, w.flip(2), 3, flip=True)[0], ref


def m04_transposed_phase1_taps_swapped():
    case = ("convT_fwd", 3, 5, 16, 3, 5, 2, set())
    x, w, Tout, ref = _thin(case)
    return S.scatter(x, w[:, :, [0, 3, 2, 1, 4]], Tout)[0], ref


def m05_channels_64_67_of_68_skipped():
    case = ("convT_fwd", 1, 17, 68, 5, 5, 2, set())
    x, w, Tout, ref = _thin(case)
    xl = x.clone()
    xl[..., 64:] = 0
    return S.scatter(xl, w, Tout)[0], ref


def m06_one_shuffle_step_missing():
    case = ("convT_fwd", 1, 16, 64, 4, 5, 2, set())          # without the xor-8 step lane 0 holds lanes 0..7: channels 0..31
    x, w, Tout, ref = _thin(case)
    xl = x.clone()
    xl[..., 32:] = 0
    return S.scatter(xl, w, Tout)[0], ref


def m06_one_shuffle_step_missing_xor1():
    case = ("fwd", 1, 16, 16, 3, 5, 1, set())                # without the xor-1 step: lanes 0, 2 -> channels 0..3 and 8..11
    x, w, Tout, ref = _thin(case)
    xl = x.clone()
    xl[..., 4:8] = 0
    xl[..., 12:16] = 0
    return W.gather_s1(xl, w, 5)[0], ref


def m07_last_row_of_an_odd_length_dropped():
    case = ("dgrad2", 3, 9, 68, 4, 5, 2, {"odd"})
    x, w, Tout, ref = _thin(case)
    got = ref.val.clone()
    got[:, -1] = float("nan")                                # the NaN prefill stays
    return got, ref


def m07_row_written_one_past_an_odd_length():
    case = ("dgrad2", 3, 9, 68, 4, 5, 2, {"odd"})
    x, w, Tout, ref = _thin(case)
    even = S.scatter(x, w, Tout + 1)[0]
    got = ref.val.clone()
    got[1:, 0] = even[:-1, -1]                               # row 2 Tin - 1 of sample b lands on row 0 of sample b + 1
    return got, ref


def _m08(fill):
    case = T.RPT[0]
    x, w, Tout, ref = _thin(case)
    r = T.rpt(case[1] * case[2])
    u = torch.arange(case[2])
    dead = ((u // 16) % r == r - 1).repeat_interleave(2)     # the positions of every workgroup's last iteration, both phases
    got = ref.val.clone()
    got[:, dead] = fill
    return got, ref


def m08_last_rpt_iteration_unwritten_nan_prefill():
    return _m08(float("nan"))


def m08_last_rpt_iteration_left_zero():
    return _m08(0.0)


def _m09(out16, K=3):
    B, Tn, Cin, N = T.BF16_SHAPES[2]
    x, w = rnd(B, Tn, Cin, seed=1), rnd(N, Cin, K, seed=2, scale=0.05)
    ref = R.conv(x, w, K)
    xl = x.clone()
    xl[..., 64:] = 0
    return R.conv(xl, w, K).val, (R.Out16(ref) if out16 else ref)


def m09_last_chunk_of_cin96_dropped_fp32out():
    return _m09(False)


def m09_last_chunk_of_cin96_dropped_bf16out():
    return _m09(True)


def _m10(shape, K):
    B, Tn, Cin, N = shape
    x, w = rnd(B, Tn, Cin, seed=1), rnd(N, Cin, K, seed=2, scale=0.05)
    return R.conv(R.truncated(x), w, K).val, R.conv(x, w, K)


def m10_fp32_x_truncated_cin32_k3():
    return _m10(T.BF16_SHAPES[0], 3)


def m10_fp32_x_truncated_cin256_k5():
    return _m10(T.BF16_SHAPES[4], 5)


def _m11(thin):
    if thin:
        x, w, Tout, acc = _thin(T.EPILOGUE[0])
        N = T.EPILOGUE[0][4]
    else:
        x, w, acc = _bf(BSAMPLE, 3)
        N = BSAMPLE[3]
    sc, sh = rnd(N, seed=5), rnd(N, seed=6)
    ref = acc.epilogue(scale=sc, shift=sh, zout=True, act=S.ACT_GELU)
    return ref.val.clone(), (ref.z if thin else R.Out16(ref.z))


def m11_zout_taken_after_the_activation_thin():
    return _m11(True)


def m11_zout_taken_after_the_activation_bf16():
    return _m11(False)


def _m12(thin):
    if thin:
        x, w, Tout, acc = _thin(T.EPILOGUE[2])
    else:
        x, w, acc = _bf(BSAMPLE, 5)
    got = acc.val.clone()
    return got, acc.epilogue(base=rnd(*acc.val.shape, seed=7))


def m12_accumulate_overwrites_thin():
    return _m12(True)


def m12_accumulate_overwrites_bf16_fp32out():
    return _m12(False)


MISTAKES = [v for k, v in sorted(globals().items()) if k.startswith("m") and k[1:3].isdigit() and callable(v)]


@pytest.mark.parametrize("mistake", MISTAKES, ids=[m.__name__ for m in MISTAKES])
def test_mistakes_are_flagged(mistake):
    """Measured worst error / bound (this file, seeds as committed; DESIGN.md section 2 has the same table):
      01 outer tap of the first / last row dropped     thin_in 244059 / 322298     bf16, fp32 / bf16 output: 17376 / 6210
      02 halo row from the neighbouring sample         thin 1156711                bf16, fp32 / bf16 output: 21444 / 8707
      03 flip forgotten in thin_in                     2857755
      04 transposed phase-1 taps k = 1, 3 swapped      178811
      05 channels 64-67 of Cin = 68 skipped            4354
      06 one shuffle step missing                      xor 8 at Cin = 64: 11755    xor 1 at Cin = 16: 82561
      07 last row of an odd Tout                       dropped: inf (NaN prefill)  written one past: 10456
      08 last rpt iteration                            unwritten: inf (NaN prefill)  left zero: 381300
      09 last chunk of Cin = 96 dropped                fp32 / bf16 output: 12999 / 6260
      10 fp32 x truncated, not rounded (fp32 output)   Cin = 32, K = 3: 458        Cin = 256, K = 5: 10.5
      11 zout taken after the activation               thin 619561                 bf16 254
      12 accumulate overwriting                        thin 8498                   bf16, fp32 output: 17421
    Every one exceeds 1.  Truncation has the smallest margin (its error grows like sqrt(n), the bound like n): the GPU file
    runs the XF32 instantiations at the one-chunk shape as well."""
    got, ref = mistake()
    r, idx, err, bnd = W.worst(got, ref)
    print(f"{mistake.__name__}: worst element {idx}: error {err:.3e} = {r:.1f} x bound {bnd:.3e}")
    assert r > 1.0
    with pytest.raises(AssertionError, match=r"worst element"):
        W.check(got, ref, mistake.__name__)
    out16 = isinstance(ref, R.Out16)
    assert W.check(ref.val.to(BF) if out16 else ref.val.float(), ref) <= 1.0          # the unmutated result, rounded, passes


def test_guarded_canvas_in_bf16_and_fp32():
    """The sentinel check compares in the canvas's dtype: an intact bf16 canvas passes, a stray write on either side fails;
    fp32 as before."""
    for dt in (torch.float32, BF):
        g = S.Guarded((2, 3, 8), device="cpu", dtype=dt, rows=2)
        assert bool(torch.isnan(g.t).all())
        g.t.fill_(1.0)
        g.check("intact")
        for pos in (g.pad - 1, g.canvas.numel() - g.pad):
            keep = g.canvas[pos].clone()
            g.canvas[pos] = 0.0
            with pytest.raises(AssertionError, match="sentinel"):
                g.check("stray")
            g.canvas[pos] = keep
        g.check("restored")
