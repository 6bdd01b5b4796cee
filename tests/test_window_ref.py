"""CPU self-test of tests/window_ref.py, the fp64 references and per-element bounds tests/test_window_contract_gpu.py holds
the stride-1 window GEMMs, wino3, the Linear kernels and the stride-1 weight gradients to: (a) the references equal
torch's fp64 conv1d / linear / autograd; (b) fp32 torch results, and an fp32 emulation of F(2,3), pass the bound; (c) each
of a list of plausible kernel mistakes, built from the fp64 reference at the contract's shapes, is flagged -- the measured
worst error / bound ratios are in test_subtle_errors_are_flagged's docstring; (d) the host plan queries (mg_conv_plan,
mg_linear_route) say that the GPU file's shape tables reach every instantiation and plan they claim to.  No GPU needed."""
import pytest
import torch
import torch.nn.functional as F

import window_ref as W


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-300))


# ---------------------------------------------------------------------------------------------------------------------
# (a) the references are the operations they claim to be
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("B,T,Cin,N", [(1, 1, 3, 2), (2, 2, 4, 5), (3, 9, 16, 8), (2, 33, 5, 3), (1, 4, 2, 2)])
def test_gather_s1_is_conv1d_and_its_data_gradient(K, B, T, Cin, N):
    x, w = rnd(B, T, Cin, seed=1), rnd(N, Cin, K, seed=2)
    ref, mag = W.gather_s1(x, w, K)
    want = F.conv1d(x.transpose(1, 2), w, None, stride=1, padding=K // 2).transpose(1, 2)
    assert ref.shape == (B, T, N) and rel(ref, want) < 1e-12
    assert rel(mag, F.conv1d(x.abs().transpose(1, 2), w.abs(), None, padding=K // 2).transpose(1, 2)) < 1e-12
    xr = x.clone().requires_grad_(True)
    dy = rnd(B, T, N, seed=3)
    F.conv1d(xr.transpose(1, 2), w, None, padding=K // 2).transpose(1, 2).backward(dy)
    dx, dmag = W.gather_s1(dy, w, K, flip=True)
    assert dx.shape == (B, T, Cin) and rel(dx, xr.grad) < 1e-12
    assert bool((dmag >= dx.abs() - 1e-12).all())
    with pytest.raises(ValueError):
        W.gather_s1(x, w, K + 2)


@pytest.mark.parametrize("M,K,N,L", [(3, 7, 12, 0), (2, 5, 12, 3), (4, 16, 8, 4), (1, 1, 6, 6)])
def test_linear_and_its_permuted_columns(M, K, N, L):
    x, w, b = rnd(M, K, seed=1), rnd(N, K, seed=2), rnd(N, seed=3)
    ref, mag = W.linear(x, w, L)
    want = F.linear(x, w, b)
    if L > 1:                                           # the reference model: view(B, C, L) + permute(0, 2, 1)
        want = want.view(M, N // L, L).permute(0, 2, 1).reshape(M, N)
    assert rel(ref + b[W.perm_index(N, L)], want) < 1e-12
    assert bool((mag >= ref.abs() - 1e-12).all())
    dy = rnd(M, N, seed=4)
    xr = x.clone().requires_grad_(True)
    F.linear(xr, w).backward(dy)
    assert rel(W.linear_dgrad(dy, w)[0], xr.grad) < 1e-12


@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("B,B2,T,Cin,N", [(2, 0, 9, 3, 4), (3, 2, 8, 5, 2), (1, 1, 2, 4, 3), (4, 3, 1, 6, 5)])
def test_wgrad_s1_is_autograd(K, B, B2, T, Cin, N):
    x = rnd(B + B2, T, Cin, seed=1)
    wr, br = rnd(N, Cin, K, seed=2).requires_grad_(True), rnd(N, seed=3).requires_grad_(True)
    y = F.conv1d(x.transpose(1, 2), wr, br, padding=K // 2).transpose(1, 2)
    dy = rnd(*y.shape, seed=4)
    y.backward(dy)
    seg = (x[:B], dy[:B], K, x[B:], dy[B:]) if B2 else (x, dy, K)
    (dw, mdw, ndw), (db, mdb, ndb) = W.wgrad_s1(*seg)
    assert rel(dw, wr.grad) < 1e-12 and ndw == (B + B2) * T
    assert rel(db, dy[:B].sum(dim=(0, 1))) < 1e-12 and ndb == B * T              # the bias: segment 0 only
    assert bool((mdw >= dw.abs() - 1e-12).all()) and bool((mdb >= db.abs() - 1e-12).all())


@pytest.mark.parametrize("flip", [False, True])
def test_wino3_value_is_the_direct_convolution_and_its_magnitude_covers_it(flip):
    B, T, Cin, N = 2, 10, 6, 5
    x = rnd(B, T, Cin, seed=1)
    w = rnd(Cin, N, 3, seed=2) if flip else rnd(N, Cin, 3, seed=2)
    val, mag, n = W.wino3(x, w, flip)
    direct, mdirect = W.gather_s1(x, w, 3, flip)
    assert torch.equal(val, direct) and n == 3 * Cin + 4
    assert bool((mag >= mdirect * (1 - 1e-12)).all())          # |m0| + |m1| + |m2| >= |their sum|, term by term
    assert rel(W.wino3_fp32_emulation(x, w, flip).double(), val) < 1e-5      # the emulation is the same convolution
    with pytest.raises(ValueError):
        W.wino3(x[:, :9], w, flip)


# ---------------------------------------------------------------------------------------------------------------------
# (b) a correct fp32 computation passes the bound
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("B,T,Cin,N", [(3, 300, 48, 32), (5, 3, 24, 130), (2, 130, 256, 96)])
def test_fp32_cpu_convolutions_pass_the_bound(K, B, T, Cin, N):
    x, w = rnd(B, T, Cin, seed=1).float(), rnd(N, Cin, K, seed=2, scale=0.05).float()
    bias = rnd(N, seed=3).float()
    got = F.conv1d(x.transpose(1, 2), w, bias, padding=K // 2).transpose(1, 2)
    ref = W.Ref(*W.gather_s1(x, w, K), K * Cin).epilogue(bias=bias, act=2)
    assert W.check(F.leaky_relu(got, 0.2), ref, "conv1d fp32") <= 1.0
    dy = rnd(B, T, N, seed=4).float()
    xr = x.clone().requires_grad_(True)
    F.conv1d(xr.transpose(1, 2), w, None, padding=K // 2).transpose(1, 2).backward(dy)
    assert W.check(xr.grad, W.Ref(*W.gather_s1(dy, w, K, flip=True), K * N), "conv1d dgrad fp32") <= 1.0


@pytest.mark.parametrize("M,K,N,L", [(33, 100, 130, 0), (128, 512, 8192, 32), (1, 8192, 31, 0), (512, 6, 33, 0)])
def test_fp32_cpu_linear_passes_the_bound(M, K, N, L):
    x, w, b = rnd(M, K, seed=1).float(), rnd(N, K, seed=2, scale=0.05).float(), rnd(N, seed=3).float()
    got = F.linear(x, w, b)
    if L > 1:
        got = got.view(M, N // L, L).permute(0, 2, 1).reshape(M, N)
    assert W.check(got, W.Ref(*W.linear(x, w, L), K).epilogue(bias=b[W.perm_index(N, L)]), "linear fp32") <= 1.0
    dy = rnd(M, N, seed=4).float()
    assert W.check(dy @ w, W.Ref(*W.linear_dgrad(dy, w), N), "linear dgrad fp32") <= 1.0


@pytest.mark.parametrize("K,B,T,Cin,N", [(1, 30, 1, 100, 36), (3, 5, 7, 20, 12), (5, 16, 64, 64, 64), (1, 777, 1, 100, 130),
                                         (5, 5, 512, 4, 64), (5, 64, 256, 4, 64)])        # the last two: the classifier's first layer
def test_fp32_cpu_weight_gradients_pass_the_bound(K, B, T, Cin, N):
    x = rnd(B, T, Cin, seed=1).float()
    w, b = rnd(N, Cin, K, seed=2, scale=0.05).float().requires_grad_(True), torch.zeros(N, requires_grad=True)
    y = F.conv1d(x.transpose(1, 2), w, b, padding=K // 2).transpose(1, 2)
    dy = rnd(*y.shape, seed=3).float()
    y.backward(dy)
    (dw, mdw, n), (db, mdb, nb) = W.wgrad_s1(x, dy, K)
    assert W.check(w.grad, W.Ref(dw, mdw, n), "dw fp32") <= 1.0
    assert W.check(b.grad, W.Ref(db, mdb, nb), "db fp32") <= 1.0


# the shapes of tests/test_conv_wino_gpu.py's comparison (B, T, Cin, N) that fit a host run, forward and flipped
WINO_SHAPES = [(2, 128, 16, 64), (1, 130, 48, 64), (3, 64, 64, 128), (2, 256, 128, 64), (5, 6, 16, 192), (1, 384, 256, 64)]


@pytest.mark.parametrize("B,T,Cin,N", WINO_SHAPES)
def test_fp32_emulation_of_f23_passes_the_wino_bound(B, T, Cin, N):
    """Measured here (worst error / bound over the six shapes, forward and flipped): 0.0011 - 0.017; M_wino / M_direct
    averages 2.67 - 2.98.  wino3_kernel's input transform is one subtraction / addition per operand, so the constant 8 of the
    bound stands as derived."""
    for flip in (False, True):
        x = rnd(B, T, Cin, seed=1).float()
        w = (rnd(Cin, N, 3, seed=2, scale=0.05) if flip else rnd(N, Cin, 3, seed=2, scale=0.05)).float()
        val, mag, n = W.wino3(x, w, flip)
        r = W.check(W.wino3_fp32_emulation(x, w, flip), W.Ref(val, mag, n), "F(2,3) fp32 emulation")
        ratio = float((mag / W.gather_s1(x, w, 3, flip)[1]).mean())
        print(f"wino emulation B={B} T={T} Cin={Cin} N={N} flip={flip}: worst {r:.4f} of the bound; M_wino/M_direct {ratio:.2f}")
        assert r <= 1.0 and 1.0 <= ratio < 4.0


# ---------------------------------------------------------------------------------------------------------------------
# (c) subtle kernel errors are flagged
# ---------------------------------------------------------------------------------------------------------------------
def _s1_case(K, B=3, T=300, Cin=48, N=96, seed=11):
    x, w = rnd(B, T, Cin, seed=seed).float(), rnd(N, Cin, K, seed=seed + 1, scale=0.05).float()
    return x, w, W.Ref(*W.gather_s1(x, w, K), K * Cin)


def _outer_tap(K, last):
    x, w, ref = _s1_case(K)
    got, p = ref.val.clone(), K // 2
    if last:        # tap 0 of the last row reads x[T - 1 - p]
        got[0, -1] -= torch.einsum("c,nc->n", x[0, -1 - p].double(), w[:, :, 0].double())
    else:           # tap K - 1 of row 0 reads x[p]
        got[1, 0] -= torch.einsum("c,nc->n", x[1, p].double(), w[:, :, K - 1].double())
    return got, ref


def mut_a_first_row_outer_tap_dropped_k3():
    return _outer_tap(3, False)


def mut_a_last_row_outer_tap_dropped_k3():
    return _outer_tap(3, True)


def mut_a_first_row_outer_tap_dropped_k5():
    return _outer_tap(5, False)


def mut_a_last_row_outer_tap_dropped_k5():
    return _outer_tap(5, True)


def mut_b_halo_from_neighbouring_sample_k3():
    x, w, ref = _s1_case(3, B=5, T=65, Cin=16, N=32)
    got = ref.val.clone()
    got[2, 0] += torch.einsum("c,nc->n", x[1, -1].double(), w[:, :, 0].double())    # x[-1] of sample 2 := sample 1's last row
    return got, ref


def mut_b_halo_from_neighbouring_sample_k5():
    x, w, ref = _s1_case(5, B=5, T=65, Cin=16, N=32)
    got = ref.val.clone()
    got[2, -1] += torch.einsum("kc,nck->n", x[3, :2].double(), w[:, :, 3:5].double())   # x[T], x[T+1] := sample 3's first rows
    return got, ref


def _chunk_dropped(K, Cin, chunk):
    x, w, ref = _s1_case(K, B=2, T=130, Cin=Cin, N=130)
    xl = torch.zeros_like(x)
    xl[..., chunk:2 * chunk] = x[..., chunk:2 * chunk]
    part = W.gather_s1(xl, w, K)[0]
    got = ref.val.clone()
    got[1, 64:128, 64:128] -= part[1, 64:128, 64:128]       # one 64 x 64 tile misses one channel chunk
    return got, ref


def mut_c_chunk16_dropped_in_one_tile_k3():
    return _chunk_dropped(3, 80, 16)


def mut_c_chunk16_dropped_in_one_tile_k5():
    return _chunk_dropped(5, 256, 16)


def mut_c_chunk64_dropped_in_one_tile_k1():
    return _chunk_dropped(1, 256, 64)


def mut_d_linear_wave_tail_dropped():
    M, K, N = 33, 100, 130          # 8 waves x 16: the last wave's range is k = 96 .. 99, the K % 8 tail
    x, w = rnd(M, K, seed=21).float(), rnd(N, K, seed=22, scale=0.05).float()
    ref = W.Ref(*W.linear(x, w), K)
    got = ref.val.clone()
    got[32:33, 96:128] -= (x[32:33, 96:].double() @ w[96:128, 96:].double().t())    # in one 32 x 32 tile
    return got, ref


def mut_e_flip_forgotten_in_data_gradient():
    B, T, Cout, Cin = 2, 64, 48, 32
    dy, w = rnd(B, T, Cout, seed=23).float(), rnd(Cout, Cin, 3, seed=24, scale=0.05).float()
    ref = W.Ref(*W.gather_s1(dy, w, 3, flip=True), 3 * Cout)
    return W.gather_s1(dy, w.flip(2), 3, flip=True)[0], ref


def _slab(K, sign):
    Cin = 1024 if K == 1 else 256       # ksplit = 8: slabs of two chunks
    x, w, ref = _s1_case(K, B=2, T=16, Cin=Cin, N=96)
    per = Cin // 8
    xl = torch.zeros_like(x)
    xl[..., 3 * per:4 * per] = x[..., 3 * per:4 * per]
    return ref.val + sign * W.gather_s1(xl, w, K)[0], ref


def mut_f_splitk_slab_dropped_k3():
    return _slab(3, -1.0)


def mut_f_splitk_slab_dropped_k1():
    return _slab(1, -1.0)


def mut_g_splitk_slab_added_twice_k5():
    return _slab(5, 1.0)


def mut_h_permuted_bias_by_output_column():
    M, K, N, L = 128, 512, 8192, 32
    x, w, b = rnd(M, K, seed=25).float(), rnd(N, K, seed=26, scale=0.05).float(), rnd(N, seed=27, scale=0.1).float()
    acc = W.linear(x, w, L)
    ref = W.Ref(acc[0].clone(), acc[1].clone(), K).epilogue(bias=b[W.perm_index(N, L)])
    return acc[0] + b.double(), ref


def mut_i_wino_m2_sign_on_odd_row():
    B, T, Cin, N = 2, 128, 48, 64
    x, w = rnd(B, T, Cin, seed=28).float(), rnd(N, Cin, 3, seed=29, scale=0.05).float()
    ref = W.Ref(*W.wino3(x, w))
    xd, g = x.double(), w.double()
    m2 = torch.einsum("bpc,nc->bpn", xd[:, 1::2] - xd[:, 0::2], 0.5 * (g[:, :, 0] - g[:, :, 1] + g[:, :, 2]))
    got = ref.val.clone()
    got[:, 1::2] += 2.0 * m2            # y[2p+1] = m1 + m2 - m3 instead of m1 - m2 - m3
    return got, ref


def _wgrad_dropped(K, B, T, Cin, N):
    x, dy = rnd(B, T, Cin, seed=31).float(), rnd(B, T, N, seed=32).float()
    (dw, m, n), _ = W.wgrad_s1(x, dy, K)
    keep = [i for i in range(B) if i != B // 2]
    return W.wgrad_s1(x[keep], dy[keep], K)[0][0], W.Ref(dw, m, n)


def mut_j_wgrad_sample_dropped_linear_b5():
    return _wgrad_dropped(1, 5, 1, 100, 36)


def mut_j_wgrad_sample_dropped_linear_b64():
    return _wgrad_dropped(1, 64, 1, 512, 128)


def mut_j_wgrad_sample_dropped_conv3_b5():
    return _wgrad_dropped(3, 5, 7, 20, 12)


def mut_j_wgrad_sample_dropped_conv3_b64_t64():
    return _wgrad_dropped(3, 64, 64, 32, 32)


def mut_j_wgrad_sample_dropped_conv5_b64_t16():
    return _wgrad_dropped(5, 64, 16, 32, 32)


MUTATIONS = [mut_a_first_row_outer_tap_dropped_k3, mut_a_last_row_outer_tap_dropped_k3, mut_a_first_row_outer_tap_dropped_k5,
             mut_a_last_row_outer_tap_dropped_k5, mut_b_halo_from_neighbouring_sample_k3, mut_b_halo_from_neighbouring_sample_k5,
             mut_c_chunk16_dropped_in_one_tile_k3, mut_c_chunk16_dropped_in_one_tile_k5, mut_c_chunk64_dropped_in_one_tile_k1,
             mut_d_linear_wave_tail_dropped, mut_e_flip_forgotten_in_data_gradient, mut_f_splitk_slab_dropped_k3,
             mut_f_splitk_slab_dropped_k1, mut_g_splitk_slab_added_twice_k5, mut_h_permuted_bias_by_output_column,
             mut_i_wino_m2_sign_on_odd_row, mut_j_wgrad_sample_dropped_linear_b5, mut_j_wgrad_sample_dropped_linear_b64,
             mut_j_wgrad_sample_dropped_conv3_b5, mut_j_wgrad_sample_dropped_conv3_b64_t64,
             mut_j_wgrad_sample_dropped_conv5_b64_t16]


@pytest.mark.parametrize("mutation", MUTATIONS, ids=[m.__name__[4:] for m in MUTATIONS])
def test_subtle_errors_are_flagged(mutation):
    """Measured worst error / bound (this file, seeds as committed):
      first / last row's outer tap dropped           K = 3: 30573 / 34060     K = 5: 14008 / 17647
      halo from the neighbouring sample              K = 3: 133642            K = 5: 49097
      one channel chunk dropped in one 64x64 tile    K = 3 (16 of 80): 13575  K = 5 (16 of 256): 541   K = 1 (64 of 256): 11474
      K % 8 tail of one wave dropped, Linear K=100   9468
      flip forgotten in the data gradient            62705
      one of eight split-K slabs dropped             K = 3: 1686   K = 1: 943;   added twice, K = 5: 1041
      permuted bias indexed by output column         1140
      wino3: m2 with the wrong sign on the odd row   28877
      one sample dropped from a weight gradient      Linear B = 5: 1677090   Linear B = 64: 45217   K = 3, 5 x 7 rows: 194601
                                                     K = 3, 64 x 64 rows: 48   K = 5, 64 x 16 rows: 433
    Every one is flagged.  The smallest margins are the dropped sample at many rows (n = 4096: 48x) -- the GPU file runs the
    weight gradients at 5 rows as well as at 64 -- and the dropped chunk at Cin = 256, K = 5 (n = 1280: 541x)."""
    got, ref = mutation()
    r, idx, err, bnd = W.worst(got, ref)
    print(f"{mutation.__name__}: worst element {idx}: error {err:.3e} = {r:.1f} x bound {bnd:.3e}")
    assert r > 1.0
    with pytest.raises(AssertionError, match=r"worst element"):
        W.check(got, ref, mutation.__name__)
    assert W.check(ref.val.float(), ref) <= 1.0          # the unmutated result, rounded to fp32, passes


# ---------------------------------------------------------------------------------------------------------------------
# (d) the GPU file's shape tables reach what they claim: the host plan queries, swept without a GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge
    ge.build()
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import ops as o
    return o


def test_tables_reach_every_stride1_instantiation(ops, monkeypatch):
    import test_window_contract_gpu as G
    from melo_gan_amd import _lib
    lib = _lib.load()
    assert len(G.S1_INSTANCES) == 18
    for K, nck, tile in G.S1_INSTANCES:
        monkeypatch.setenv("MG_FORCE_TILE", str(tile))
        cases = G.s1_edge_cases(K, tile)
        for B, T, Cin, N, padded in cases:
            assert lib.mg_conv_tile_config(B * T, N, 0) == tile, (K, tile, B, T, Cin, N)
            assert Cin > 8 and N > 8 and lib.mg_conv_thin_route(None, T * Cin, Cin, N, K, 1, 0) == 0
        Ts = {c[1] for c in cases}
        assert {2, 3, K, 63, 64, 65, 130, 300} <= Ts and (1 in Ts or (K, tile) == (5, 22)) and (K == 1 or K - 1 in Ts)
        assert {16, 24, 48, 80, 256} <= {c[2] for c in cases} and (K != 1 or 100 in {c[2] for c in cases})
        assert {96, 130, 256} <= {c[3] for c in cases} and (tile != 11 or 32 in {c[3] for c in cases})
        assert 193 in {c[0] for c in cases} and any(c[4] for c in cases)
        tbs = [(c[0], G.batch_rows_per_tile(c[1], tile)[0]) for c in cases]
        assert any(b == tb + 1 for b, tb in tbs) and any(b == tb - 1 for b, tb in tbs)
        assert max(G.batch_rows_per_tile(c[1], tile)[1] for c in cases) >= 3
    for tile in G.TILES:                          # the Linear entry points above 512 rows
        monkeypatch.setenv("MG_FORCE_TILE", str(tile))
        for M, Kin, N in G.LINEAR_BIG:
            assert M > ops.SKINNY_MAX_ROWS and lib.mg_conv_tile_config(M, N, 0) == tile


def test_tables_reach_the_split_k_plans_and_both_finish_variants(ops, monkeypatch):
    import test_window_contract_gpu as G
    monkeypatch.setenv("MG_SPLITK_TARGET", G.SPLIT_TARGET)
    monkeypatch.delenv("MG_FORCE_TILE", raising=False)
    seen, uneven = set(), 0
    for K, nck, B, T, Cin, N, ksplit, cps in G.SPLIT_CASES:
        assert ops.conv_plan(B, T, Cin, N, K, 1) == (ksplit, cps), (K, B, T, Cin, N)
        nchunks = -(-Cin // (64 if K == 1 else 16))
        uneven += nchunks % cps != 0
        seen.add((K, ksplit))
    assert {k for _, k in seen} >= {2, 4, 8} and uneven >= 3
    for K in (1, 3, 5):
        assert {k for kk, k in seen if kk == K} >= {2, 4, 8}, K
    assert {c[1] for c in G.SPLIT_CASES} == {True, False}
    # the vector finish needs N % 4 == 0: both kinds of N occur, and the misaligned views give the scalar one at N % 4 == 0
    assert {c[5] % 4 == 0 for c in G.SPLIT_CASES} == {True, False}
    lib = __import__("melo_gan_amd")._lib.load()
    assert [lib.mg_conv_finish_vec(*a) for a in ((96, 96 * 33, 1), (96, 96 * 33, 0), (130, 130 * 64, 1), (96, 96 * 33 + 2, 1))] == [1, 0, 0, 0]
    for tile in (12, 22):                         # the wide tiles under a forced split (test_split_k_on_the_wide_tiles)
        monkeypatch.setenv("MG_FORCE_TILE", str(tile))
        for K in (1, 3, 5):
            assert ops.conv_plan(2, 70, 1024 if K == 1 else 256, 96, K, 1)[0] == 8
            assert ops.conv_plan(3, 9, 320 if K == 1 else 80, 130, K, 1)[0] == 2
    monkeypatch.delenv("MG_FORCE_TILE")
    for tr2, B, Tin, Cin, N, odd, ksplit in G.SPLIT_S2:
        assert ops.conv_plan(B, Tin, Cin, N, 5, 2, scatter2=tr2, odd=odd)[0] == ksplit
    assert {c[0] for c in G.SPLIT_S2} == {True, False}
    # without the switch the same shapes plan fewer slabs or none; without a workspace there is no split at all
    monkeypatch.delenv("MG_SPLITK_TARGET")
    from melo_gan_amd import _lib
    import ctypes as C
    ks, cps = C.c_int(), C.c_int()
    assert _lib.load().mg_conv_plan(2, 64, 64, 96, 256, 3, 1, 0, 0, C.byref(ks), C.byref(cps)) == 0 and (ks.value, cps.value) == (1, 16)
    assert _lib.load().mg_conv_plan(2, 64, 64, 96, 256, 7, 1, 0, 0, C.byref(ks), C.byref(cps)) == -1


def test_tables_reach_every_skinny_instantiation_and_route(ops, monkeypatch):
    import test_window_contract_gpu as G
    monkeypatch.delenv("MG_LINEAR_SKINNY_ONLY", raising=False)
    monkeypatch.delenv("MG_FORCE_TILE", raising=False)
    seen = set()
    for M, K, N, fwd, mis, inst, ksplit in G.SKINNY_CASES:
        got = ops.linear_route(M, K, N, K if fwd else 1, 1 if fwd else N, 0, mis != "x", mis != "w")
        assert got == (G.skinny_sym(*inst), ksplit), (M, K, N, fwd, mis, got)
        seen.add((inst, ksplit > 1))
    assert {s[0] for s in seen} == {(a, b) for a in (True, False) for b in (True, False)}
    assert {s for s in seen if s[1]} >= {((True, True), True), ((True, False), True), ((False, True), True)}
    assert {c[0] for c in G.SKINNY_CASES} >= {1, 31, 32, 33, 512} and {c[2] for c in G.SKINNY_CASES} >= {1, 31, 33, 130, 8192}
    assert {c[1] for c in G.SKINNY_CASES} >= {6, 8, 64, 100, 192, 1000, 2048, 8192}
    perm_split = set()
    for M, K, N, L, ks in G.PERM_CASES:
        assert ops.linear_route(M, K, N, K, 1, L) == (G.skinny_sym(True, K % (64 * ks) == 0), ks)
        perm_split.add(ks > 1)
    assert perm_split == {True, False}
    M, K, N, L = G.PRE2
    assert ops.linear_route(M, K, N, K, 1, L) == ("conv_wgemm_kernel<1,1,false,true,1,1>", 1)
    assert ops.linear_route(M, K, N, K, 1, L, x_aligned=False)[0] == "linear_skinny_kernel<true,false>"
    assert ops.linear_route(M, K, N, K, 1, 0)[0] == "linear_skinny_kernel<true,true>"          # unpermuted: never the window GEMM
    monkeypatch.setenv("MG_LINEAR_SKINNY_ONLY", "1")
    assert ops.linear_route(M, K, N, K, 1, L) == ("linear_skinny_kernel<true,true>", 1)
    with pytest.raises(RuntimeError):
        ops.linear_route(4, 8, 12, 8, 1, 5)                                                    # perm_L must divide N
