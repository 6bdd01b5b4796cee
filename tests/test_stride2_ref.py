"""CPU self-test of tests/stride2_ref.py, the fp64 references and the per-element bound that
tests/test_stride2_contract_gpu.py holds the stride-2 kernels to: the references equal torch's fp64 convolutions and
autograd; an fp32 computation of the same op passes the bound; and each of a list of subtle kernel errors -- built from
the fp64 reference at the contract's edge shapes -- is flagged.  The last part is the evidence that the GPU contract
catches subtle errors; it needs no GPU."""
import pytest
import torch
import torch.nn.functional as F

import stride2_ref as S


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-300))


# ---------------------------------------------------------------------------------------------------------------------
# the references are the operations they claim to be
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Tin,Cin,N", [(1, 7, 3, 2), (2, 8, 4, 5), (3, 9, 16, 8), (2, 33, 5, 3), (1, 4, 2, 2)])
def test_gather_is_conv1d_stride2(B, Tin, Cin, N):
    x, w = rnd(B, Tin, Cin, seed=1), rnd(N, Cin, 5, seed=2)
    ref, mag = S.gather(x, w)
    want = F.conv1d(x.transpose(1, 2), w, None, stride=2, padding=2).transpose(1, 2)
    assert ref.shape == (B, S.tm_gather(Tin), N)
    assert rel(ref, want) < 1e-13
    assert rel(mag, F.conv1d(x.abs().transpose(1, 2), w.abs(), None, stride=2, padding=2).transpose(1, 2)) < 1e-13
    # ... and the ConvTranspose1d data gradient (w = its (Cin, Cout, 5) weight, x = the gradient of its output)
    dy = rnd(B, 2 * Tin, Cin, seed=3)
    xt = rnd(B, Tin, N, seed=4, scale=0.0).requires_grad_(True)
    F.conv_transpose1d(xt.transpose(1, 2), w, None, stride=2, padding=2, output_padding=1).transpose(1, 2).backward(dy)
    assert rel(S.gather(dy, w)[0], xt.grad) < 1e-13


@pytest.mark.parametrize("B,Tin,Cin,N,odd", [(1, 4, 3, 2, False), (2, 5, 4, 5, True), (3, 9, 16, 8, False),
                                            (2, 9, 16, 8, True), (1, 1, 2, 3, True), (2, 2, 2, 3, False)])
def test_scatter_is_conv_transpose1d_stride2(B, Tin, Cin, N, odd):
    x, w = rnd(B, Tin, Cin, seed=1), rnd(Cin, N, 5, seed=2)
    Tout = 2 * Tin - (1 if odd else 0)
    ref, mag = S.scatter(x, w, Tout)
    want = F.conv_transpose1d(x.transpose(1, 2), w, None, stride=2, padding=2, output_padding=0 if odd else 1).transpose(1, 2)
    assert ref.shape == want.shape == (B, Tout, N)
    assert rel(ref, want) < 1e-13
    assert rel(mag, F.conv_transpose1d(x.abs().transpose(1, 2), w.abs(), None, stride=2, padding=2,
                                       output_padding=0 if odd else 1).transpose(1, 2)) < 1e-13
    # ... and the Conv1d data gradient over an input of length Tout (w = the Conv1d's (Cout, Cin, 5) weight)
    xc = rnd(B, Tout, N, seed=3).requires_grad_(True)
    yc = F.conv1d(xc.transpose(1, 2), w, None, stride=2, padding=2).transpose(1, 2)
    assert yc.shape[1] == Tin
    yc.backward(x)
    assert rel(ref, xc.grad) < 1e-13
    with pytest.raises(ValueError):
        S.scatter(x, w, 2 * Tin + 1)


@pytest.mark.parametrize("B,B2,T,Cin,N", [(2, 0, 9, 3, 4), (3, 2, 8, 5, 2), (1, 1, 33, 4, 3)])
def test_weight_gradients_are_autograd(B, B2, T, Cin, N):
    x, w, b = rnd(B + B2, T, Cin, seed=1), rnd(N, Cin, 5, seed=2), rnd(N, seed=3)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.conv1d(xr.transpose(1, 2), wr, br, stride=2, padding=2).transpose(1, 2)
    dy = rnd(*y.shape, seed=4)
    y.backward(dy)
    seg = (x[:B], dy[:B], x[B:], dy[B:]) if B2 else (x, dy, None, None)
    (dw, mdw, ndw), (db, mdb, ndb) = S.conv_wgrad(*seg)
    assert rel(dw, wr.grad) < 1e-13 and ndw == (B + B2) * S.tm_gather(T)
    assert rel(db, dy[:B].sum(dim=(0, 1))) < 1e-13 and ndb == B * S.tm_gather(T)     # the bias: segment 0 only
    assert bool((mdw >= dw.abs()).all()) and bool((mdb >= db.abs()).all())
    # ConvTranspose1d
    wt, bt = rnd(Cin, N, 5, seed=5), rnd(N, seed=6)
    xr, wr, br = x.clone().requires_grad_(True), wt.clone().requires_grad_(True), bt.clone().requires_grad_(True)
    y = F.conv_transpose1d(xr.transpose(1, 2), wr, br, stride=2, padding=2, output_padding=1).transpose(1, 2)
    dy = rnd(*y.shape, seed=7)
    y.backward(dy)
    (dw, _, ndw), (db, _, ndb) = S.convT_wgrad(x, dy)
    assert rel(dw, wr.grad) < 1e-13 and rel(db, br.grad) < 1e-13
    assert ndw == (B + B2) * T and ndb == (B + B2) * 2 * T


def test_epilogue_reference_order():
    """(acc + bias) * scale + shift -> zout; act; * act'(gref); * emul; * gscale; + base."""
    acc = rnd(2, 3, 4, seed=1)
    bias, scale, shift, gscale = rnd(4, seed=2), rnd(4, seed=3), rnd(4, seed=4), rnd(4, seed=5)
    gref, emul, base = rnd(2, 3, 4, seed=6), rnd(2, 3, 4, seed=7), rnd(2, 3, 4, seed=8)
    r = S.Ref(acc.clone(), acc.abs(), 10).epilogue(bias=bias, scale=scale, shift=shift, zout=True, act=S.ACT_LRELU,
                                                   gref=gref, gact=S.ACT_RELU, emul=emul, gscale=gscale, base=base)
    z = (acc + bias) * scale + shift
    assert torch.equal(r.z.val, z)
    want = torch.where(z > 0, z, 0.2 * z) * (gref > 0) * emul * gscale + base
    assert rel(r.val, want) < 1e-15
    assert bool((r.mag >= r.val.abs() - 1e-12).all()) and r.k_epi == 8


# ---------------------------------------------------------------------------------------------------------------------
# a correct fp32 computation passes the bound
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Tin,Cin,N", [(3, 299, 48, 32), (1, 7, 16, 96), (5, 130, 256, 32)])
def test_fp32_cpu_convolutions_pass_the_bound(B, Tin, Cin, N):
    x, w = rnd(B, Tin, Cin, seed=1).float(), rnd(N, Cin, 5, seed=2, scale=0.05).float()
    bias = rnd(N, seed=3).float()
    got = F.conv1d(x.transpose(1, 2), w, bias, stride=2, padding=2).transpose(1, 2)
    ref = S.Ref(*S.gather(x, w), 5 * Cin).epilogue(bias=bias, act=S.ACT_LRELU)
    assert S.check(F.leaky_relu(got, 0.2), ref, "conv1d fp32") < 0.1
    for odd in (False, True):
        wt = rnd(Cin, N, 5, seed=4, scale=0.05).float()
        Tout = 2 * Tin - (1 if odd else 0)
        got = F.conv_transpose1d(x.transpose(1, 2), wt, None, stride=2, padding=2,
                                 output_padding=0 if odd else 1).transpose(1, 2)
        assert S.check(got, S.Ref(*S.scatter(x, wt, Tout), 5 * Cin), "conv_transpose1d fp32") < 0.1


@pytest.mark.parametrize("B,T,Cin,N", [(5, 63, 20, 32), (16, 128, 64, 64)])
def test_fp32_cpu_weight_gradients_pass_the_bound(B, T, Cin, N):
    x = rnd(B, T, Cin, seed=1).float().requires_grad_(False)
    w = rnd(N, Cin, 5, seed=2, scale=0.05).float().requires_grad_(True)
    b = torch.zeros(N, requires_grad=True)
    y = F.conv1d(x.transpose(1, 2), w, b, stride=2, padding=2).transpose(1, 2)
    dy = rnd(*y.shape, seed=3).float()
    y.backward(dy)
    (dw, mdw, n), (db, mdb, nb) = S.conv_wgrad(x, dy)
    assert S.check(w.grad, S.Ref(dw, mdw, n), "conv dw fp32") < 0.1
    assert S.check(b.grad, S.Ref(db, mdb, nb), "conv db fp32") < 0.1


# ---------------------------------------------------------------------------------------------------------------------
# subtle kernel errors are flagged
# ---------------------------------------------------------------------------------------------------------------------
def _gather_case(B=3, Tin=299, Cin=48, N=96):
    x, w = rnd(B, Tin, Cin, seed=11).float(), rnd(N, Cin, 5, seed=12, scale=0.05).float()
    return x, w, S.Ref(*S.gather(x, w), 5 * Cin)


def mut_a_dropped_tap_first_row():
    x, w, ref = _gather_case()
    got = ref.val.clone()
    got[1, 0] -= torch.einsum("c,nc->n", x[1, 2].double(), w[:, :, 4].double())     # tap 4 of output row 0 (reads x[2])
    return got, ref


def mut_a_dropped_tap_last_row():
    x, w, ref = _gather_case(Tin=300)
    got = ref.val.clone()
    t = ref.val.shape[1] - 1
    got[0, t] -= torch.einsum("c,nc->n", x[0, 2 * t - 2].double(), w[:, :, 0].double())   # tap 0 of the last row
    return got, ref


def mut_b_halo_from_neighbouring_sample():
    x, w, ref = _gather_case(B=5, Tin=65, Cin=16, N=32)
    got = ref.val.clone()
    # output row 0 of sample 2: taps 0, 1 read x[-2], x[-1] -- zero padding -- taken instead from sample 1's last rows
    got[2, 0] += torch.einsum("kc,nck->n", x[1, -2:].double(), w[:, :, 0:2].double())
    return got, ref


def mut_c_last_chunk_dropped_in_one_tile():
    x, w, ref = _gather_case(B=2, Tin=130, Cin=80, N=96)
    xl = torch.zeros_like(x)
    xl[..., -16:] = x[..., -16:]
    part = S.gather(xl, w)[0]
    got = ref.val.clone()
    got[1, 32:64, 32:64] -= part[1, 32:64, 32:64]           # one 32 x 32 tile misses channels Cin-16 .. Cin-1
    return got, ref


def mut_d_odd_scatter_last_row_missing():
    B, Tin, Cin, N = 3, 75, 48, 32
    x, w = rnd(B, Tin, Cin, seed=13).float(), rnd(Cin, N, 5, seed=14, scale=0.05).float()
    ref = S.Ref(*S.scatter(x, w, 2 * Tin - 1), 5 * Cin)
    got = ref.val.clone()
    got[:, -1] = 0.0
    return got, ref


def mut_e_scatter_phases_swapped():
    B, Tin, Cin, N = 2, 33, 16, 32
    x, w = rnd(B, Tin, Cin, seed=15).float(), rnd(Cin, N, 5, seed=16, scale=0.05).float()
    ref = S.Ref(*S.scatter(x, w, 2 * Tin), 5 * Cin)
    got = ref.val.clone()
    got[:, 0::2], got[:, 1::2] = ref.val[:, 1::2], ref.val[:, 0::2]
    return got, ref


def _wgrad_case(B=64, T=128, Cin=64, N=128):
    x, dy = rnd(B, T, Cin, seed=17).float(), rnd(B, S.tm_gather(T), N, seed=18).float()
    (dw, m, n), _ = S.conv_wgrad(x, dy)
    return x, dy, S.Ref(dw, m, n)


def mut_f_wgrad_sample_dropped():
    x, dy, ref = _wgrad_case()
    return S.conv_wgrad(x[1:], dy[1:])[0][0], ref


def mut_f_wgrad_sample_dropped_ragged():
    x, dy, ref = _wgrad_case(B=5, T=63, Cin=20, N=32)
    return S.conv_wgrad(torch.cat([x[:3], x[4:]]), torch.cat([dy[:3], dy[4:]]))[0][0], ref


def mut_g_wgrad_time_tile_twice():
    x, dy, ref = _wgrad_case()
    # rows t = 32 .. 63 of sample 7 summed twice: the window of x they read is x[62 .. 129]
    xs = torch.zeros_like(x[7:8])
    xs[:, 62:130] = x[7:8, 62:130]
    dys = torch.zeros_like(dy[7:8])
    dys[:, 32:64] = dy[7:8, 32:64]
    return ref.val + S.conv_wgrad(xs, dys)[0][0], ref


MUTATIONS = [mut_a_dropped_tap_first_row, mut_a_dropped_tap_last_row, mut_b_halo_from_neighbouring_sample,
             mut_c_last_chunk_dropped_in_one_tile, mut_d_odd_scatter_last_row_missing, mut_e_scatter_phases_swapped,
             mut_f_wgrad_sample_dropped, mut_f_wgrad_sample_dropped_ragged, mut_g_wgrad_time_tile_twice]


@pytest.mark.parametrize("mutation", MUTATIONS, ids=[m.__name__[4:] for m in MUTATIONS])
def test_subtle_errors_are_flagged(mutation):
    got, ref = mutation()
    r, idx, err, bnd = S.worst(got, ref)
    print(f"{mutation.__name__}: worst element {idx}: error {err:.3e} = {r:.1f} x bound {bnd:.3e}")
    assert r > 1.0
    with pytest.raises(AssertionError, match=r"worst element"):
        S.check(got, ref, mutation.__name__)
    assert S.check(ref.val.float(), ref) <= 1.0          # the unmutated result, rounded to fp32, passes


def test_non_finite_results_are_flagged():
    x, w, ref = _gather_case(B=1, Tin=9, Cin=16, N=32)
    got = ref.val.clone()
    got[0, 4, 31] = float("nan")
    assert S.worst(got, ref)[1] == (0, 4, 31)
    with pytest.raises(AssertionError):
        S.check(got, ref)


def test_guard_sees_writes_outside_the_output():
    g = S.Guarded((2, 3, 4), device="cpu", rows=2)
    assert bool(torch.isnan(g.t).all())
    g.t.fill_(1.0)
    g.check()
    g.canvas[g.pad - 1] = 0.0                        # one element before the output
    with pytest.raises(AssertionError, match="before"):
        g.check()
    g = S.Guarded((2, 3, 4), device="cpu", rows=2)
    g.canvas[g.pad + 24] = 0.0                       # one element after it
    with pytest.raises(AssertionError, match="after"):
        g.check()
