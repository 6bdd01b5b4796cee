"""fp64 references of csrc/conv_bf16.hip (conv_bf16_kernel<K, XF32, YF32>, wb_relayout, meanT_fwd_bf16, meanT_bwd_bf16)
with the per-element bound their results are held to.  A plain helper module beside window_ref / support_ref (whose
gather_s1, Ref, meanT_fwd, meanT_bwd it uses unchanged); nothing here is collected.

Operands.  The reference takes every operand as the kernel multiplies it: rounded to bf16 to nearest-even (q() below:
torch's .to(torch.bfloat16)), then fp64 -- x (the kernel's XF32 conversion of an fp32 input is this rounding; a truncating
one fails, tests/test_thin_bf16_ref.py), the weight image (wb_relayout rounds the fp32 weight), gref, meanT's input.

fp32 output.  A product of two bf16 values has 16 significant bits: it is exact in fp32.  Only the accumulation rounds,
so the project's bound holds unchanged, |got - ref| <= (n + 4 + k_epi) 2^-24 M + eps_abs with n = K Cin, M the same
expression on the absolute values of the rounded operands, the epilogue steps counted by Ref.epilogue.

bf16 output (y, zout, dz of meanT_bwd_bf16).  The fp32 value v the kernel holds satisfies |v - ref| <= bound32, and the
store rounds it once to 8 significant bits: |bf16(v) - v| <= 2^-8 |v| <= 2^-8 (|ref| + bound32).  Together

    bound16 = bound32 + 2^-8 (|ref| + bound32)

-- a theorem about one round-to-nearest, not a tolerance; an exact result rounded once sits at up to 1.0 of it by
construction, and the term hides whatever is below 2^-8 relative, which is why every bf16-output case also runs in its
fp32-output instantiation."""
import torch

import support_ref as SR
import window_ref as W
from stride2_ref import Ref, U  # noqa: F401

BF = torch.bfloat16
U16 = 2.0 ** -8                 # unit roundoff of bf16 (8 significant bits)


def q(t):
    """t as a bf16 kernel operand: rounded to nearest-even."""
    return t.to(BF)


def truncated(t):
    """An fp32 tensor cut to bf16 by dropping the low 16 bits (the conversion a kernel must NOT use)."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)


def conv(x, w, K, flip=False):
    """Ref of the stride-1 K-tap convolution on bf16-rounded operands; x (B, T, Cin) bf16 or fp32, w the fp32 weight handed
    to wb_relayout: (N, Cin, K), or with flip the Conv1d weight (Cout = C of x, N, K) of the data gradient."""
    val, mag = W.gather_s1(q(x).double(), q(w).double(), K, flip)
    return Ref(val, mag, K * x.shape[2])


class Out16:
    """A Ref seen through one rounding to bf16: .val, .n and .bound() as check / worst use them."""

    def __init__(self, ref):
        self.val, self.n, self._b32 = ref.val, ref.n, ref.bound()

    def bound(self):
        return self._b32 + U16 * (self.val.abs() + self._b32)


def relayout(w, N, Cc, K, w_sn, w_sc, flip=False):
    """wb[k][n][c] = bf16(w[n w_sn + c w_sc + (flip ? K-1-k : k)]) by index arithmetic on the host: (K, N, Cc) bf16."""
    flat = w.detach().cpu().flatten()
    n, c, k = torch.arange(N)[None, :, None], torch.arange(Cc)[None, None, :], torch.arange(K)[:, None, None]
    return q(flat[n * w_sn + c * w_sc + ((K - 1 - k) if flip else k)])


def meanT_fwd(a):
    """h[b, c] = mean_t a[b, t, c], a bf16: conversions exact, an fp32 sum of T terms, one division: (T + 4 + 1) U M."""
    return SR.meanT_fwd(q(a))


def meanT_bwd(dh, T, gref, gact, gscale=None):
    """dz = dh / T * act'(gref) * gscale elementwise in fp32 (support_ref.meanT_bwd with its transcendental terms), gref
    bf16, then one rounding to bf16."""
    return Out16(SR.meanT_bwd(dh, T, q(gref), gact, gscale))


def conv_fp32_host(x, w, K, flip=False):
    """fp32 arithmetic on the bf16-rounded operands with torch on the host: what a correct kernel computes up to the order
    of its sum."""
    import torch.nn.functional as F
    xq, wq = q(x).float(), q(w).float()
    if flip:
        wq = wq.flip(2).permute(1, 0, 2).contiguous()
    return F.conv1d(xq.transpose(1, 2), wq, None, padding=K // 2).transpose(1, 2).contiguous()
