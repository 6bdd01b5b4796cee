"""fp64 references of the stride-1 window GEMMs (conv_wgemm_kernel<1,K,...>, K = 1 / 3 / 5), the F(2,3) minimal-filtering
kernel (wino3_kernel), the Linear kernels (linear_skinny_kernel, the row chain's LIN_FWD / LIN_DGRAD) and the stride-1
weight gradients (wgrad_multi_kernel<1,K>), with the per-element bound their fp32 results are held to.  A plain helper
module beside stride2_ref (whose Ref / check / worst / Guarded it uses); nothing here is collected.

Same construction as stride2_ref: zero padding, `unfold`, one fp64 einsum; every function returns, beside the value, the
magnitude M of each output element -- the same expression on |x| and |w| -- and works on whatever device its inputs are
on, so large shapes can be evaluated in fp64 on the GPU.  The bound is stride2_ref's

    |got - ref| <= (n + 4 + k_epi) * 2^-24 * M

with n = the products of the element's sum.  Split-K (blockIdx.z slabs + a finish kernel), the skinny kernel's split of K
over eight waves and over blockIdx.z, and the weight gradients' batch slabs need NO extra budget: whatever the summation
tree over the same n products, a product passes through at most n - 1 additions, which is what n * 2^-24 * M already pays
for.  Do not add slack for them.

wino3 is the exception in M, not in form.  F(2,3) multiplies TRANSFORMED operands, which round before the product:

    d0..d3 = x[2p-1 .. 2p+2]          m0 = (d0 - d2) g0                 m1 = (d1 + d2) (g0 + g1 + g2)/2
    y[2p]   = m0 + m1 + m2            m2 = (d2 - d1) (g0 - g1 + g2)/2   m3 = (d1 - d3) g2
    y[2p+1] = m1 - m2 - m3

so the magnitude an error is relative to is that of the transformed products, without cancellation: with d, g the
absolute values and gs = (g0 + g1 + g2) / 2, summed over channels,

    M[2p] = (d0 + d2) g0 + 2 (d1 + d2) gs            M[2p+1] = (d1 + d3) g2 + 2 (d1 + d2) gs

and bound = (3 Cin + 8 + k_epi) * 2^-24 * M: 3 Cin products per output; one rounding on a data operand (one subtraction /
addition: wino3_kernel's input transform), two on a filter operand (wino3_weights_kernel computes 0.5f * (g0 +- g1 + g2): two
additions, the halving is exact), two additions in the output transform, and the 4 of the direct bound minus the one
already counted.  M_wino / M_direct averages about 2.7."""
import torch

from stride2_ref import Ref, check, worst, Guarded, act_ref, act_grad_ref, U  # noqa: F401  (re-exported for the tests)
from stride2_ref import _both, _cat


def _windows_s1(x, K):
    """(B, T, C) -> (B, T, C, K): window k of output t is x[t + k - K // 2] (zeros outside)."""
    B, T, C = x.shape
    p = K // 2
    xp = torch.cat([x.new_zeros(B, p, C), x, x.new_zeros(B, p, C)], dim=1) if p else x
    return xp.unfold(1, K, 1)


def gather_s1(x, w, K, flip=False):
    """Conv1d(k=K, s=1, p=K//2) forward, y[b,t,n] = sum_{c,k} x[b,t+k-p,c] w[n,c,k] with w (N, Cin, K); flip=True: the data
    gradient dx[b,t,n] = sum_{c,k} x[b,t+p-k,c] w[c,n,k] with w the Conv1d's (Cout = C of x, Cin = N, K) weight -- what
    ops.conv1d_dgrad(x, w, dx, 1) computes.  Returns (ref, M) in fp64, (B, T, N); n = K * C."""
    if w.shape[2] != K or x.shape[2] != (w.shape[0] if flip else w.shape[1]):
        raise ValueError(f"gather_s1: x {tuple(x.shape)} / w {tuple(w.shape)} / K={K} flip={flip}")
    if flip:
        return _both(lambda a, b: torch.einsum("btck,cnk->btn", _windows_s1(a, K), b.flip(2)), x, w)
    return _both(lambda a, b: torch.einsum("btck,nck->btn", _windows_s1(a, K), b), x, w)


def thin(entry, x, w, K, stride, Tout):
    """(ref, M) of the ops.py entry points csrc/conv_thin.hip serves (tests/thin_bf16_tables.py: ENTRIES), from the
    references above and stride2_ref's -- no arithmetic of its own.  n = K * x.shape[2]."""
    import stride2_ref as S
    if entry == "fwd":
        return gather_s1(x, w, K) if stride == 1 else (S.gather(x, w) if K == 5 else S.gather3(x, w))
    if entry == "convT_dgrad":
        return S.gather(x, w)
    if entry == "dgrad1":
        return gather_s1(x, w, K, flip=True)
    if entry in ("convT_fwd", "dgrad2"):
        return S.scatter(x, w, Tout)
    raise ValueError(entry)


def perm_index(N, perm_L, device="cpu"):
    """Weight row behind output column n' of mg_linear with perm_L: (n' % C) * L + n' // C, C = N / L (identity for perm_L <= 1)."""
    n = torch.arange(N, device=device)
    if perm_L <= 1:
        return n
    Cc = N // perm_L
    return (n % Cc) * perm_L + n // Cc


def linear(x, w, perm_L=0):
    """nn.Linear forward without bias: x (M, K) @ w (N, K)^T, columns in mg_linear's perm_L order when perm_L > 1 (a bias /
    scale / gscale vector follows the weight row: index it with perm_index).  Returns (ref, M), (M, N); n = K."""
    idx = perm_index(w.shape[0], perm_L, w.device)
    return _both(lambda a, b: (a @ b.t())[:, idx], x, w)


def linear_dgrad(dy, w):
    """dx = dy (M, N) @ w (N, K).  Returns (ref, M), (M, K); n = N."""
    return _both(lambda a, b: a @ b, dy, w)


def wgrad_s1(x, dy, K, x2=None, dy2=None):
    """Weight gradient of Conv1d(k=K, s=1, p=K//2): dw[n,c,k] = sum_{b,t} dy[b,t,n] x[b,t+k-p,c] over both segments;
    db[n] = sum_{b,t} dy[b,t,n] over segment 0 only.  K = 1 with T = 1 is linear_wgrad.  x (B, T, Cin), dy (B, T, Cout).
    Returns ((dw, M_dw, n_dw), (db, M_db, n_db)); n = rows * T."""
    xs, ds = _cat(x, x2), _cat(dy, dy2)
    dw = _both(lambda a, b: torch.einsum("btn,btck->nck", b, _windows_s1(a, K)), xs, ds)
    db = _both(lambda b: b.sum(dim=(0, 1)), dy)
    return (dw[0], dw[1], ds.shape[0] * ds.shape[1]), (db[0], db[1], dy.shape[0] * dy.shape[1])


def wino3_mag(x, w, flip=False):
    """The F(2,3) magnitude M (module docstring) of every output element, fp64 (B, T, N); T even."""
    B, T, C = x.shape
    if T % 2:
        raise ValueError("wino3: T must be even")
    d = x.double().abs()
    g = w.double().abs()
    g = g.flip(2).permute(1, 0, 2) if flip else g                # (N, C, 3), taps in the order the pair sees them
    dp = torch.cat([d.new_zeros(B, 1, C), d, d.new_zeros(B, 1, C)], dim=1)      # dp[i] = |x[i - 1]|
    d0, d1, d2, d3 = dp[:, 0:T:2], dp[:, 1:T + 1:2], dp[:, 2:T + 2:2], dp[:, 3:T + 2:2]      # (B, T/2, C) each
    g0, g2 = g[:, :, 0], g[:, :, 2]
    gs = 0.5 * (g[:, :, 0] + g[:, :, 1] + g[:, :, 2])
    mid = 2.0 * torch.einsum("bpc,nc->bpn", d1 + d2, gs)
    even = torch.einsum("bpc,nc->bpn", d0 + d2, g0) + mid
    odd = torch.einsum("bpc,nc->bpn", d1 + d3, g2) + mid
    return torch.stack([even, odd], dim=2).reshape(B, T, g.shape[0])


WINO_EXTRA = 4          # (3 Cin + 8) = (n + 4) with n = 3 Cin + WINO_EXTRA


def wino3(x, w, flip=False):
    """(ref, M_wino, n) of the three-tap stride-1 convolution computed by minimal filtering: the value is gather_s1's, the
    magnitude and product count are F(2,3)'s.  Ref(ref, M, n).bound() = (3 Cin + 8 + k_epi) * 2^-24 * M."""
    val = gather_s1(x, w, 3, flip)[0]
    return val, wino3_mag(x, w, flip), 3 * x.shape[2] + WINO_EXTRA


def wino3_fp32_emulation(x, w, flip=False):
    """F(2,3) carried out in fp32 with torch on the host, operand transforms rounded as the kernels round them: what a
    correct wino3_kernel computes up to the order of its channel sum.  x (B, T, C), T even."""
    B, T, C = x.shape
    g, xf = w.float(), x.float()
    g = g.flip(2).permute(1, 0, 2) if flip else g
    xp = torch.cat([xf.new_zeros(B, 1, C), xf, xf.new_zeros(B, 1, C)], dim=1)
    d0, d1, d2, d3 = xp[:, 0:T:2], xp[:, 1:T + 1:2], xp[:, 2:T + 2:2], xp[:, 3:T + 2:2]
    g0, g1, g2 = g[:, :, 0], g[:, :, 1], g[:, :, 2]
    m0 = torch.einsum("bpc,nc->bpn", d0 - d2, g0)
    m1 = torch.einsum("bpc,nc->bpn", d1 + d2, 0.5 * (g0 + g1 + g2))
    m2 = torch.einsum("bpc,nc->bpn", d2 - d1, 0.5 * (g0 - g1 + g2))
    m3 = torch.einsum("bpc,nc->bpn", d1 - d3, g2)
    return torch.stack([m0 + m1 + m2, m1 - m2 - m3], dim=2).reshape(B, T, g.shape[0])
