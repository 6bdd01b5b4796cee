"""fp64 references of the stride-2 five-tap family (conv16 / conv_gather / conv_scatter2 / wgrad_multi<2,5>) and the
per-element error bound their fp32 results are held to.  A plain helper module, imported by the test files as
`import stride2_ref` (tests/ is on sys.path under pytest's default import mode); nothing here is collected.

Every reference is built from zero padding, zero-stuffing and `unfold` plus one fp64 einsum -- no fp64 convolution
kernels, whose backend support is not something to rely on -- and every one returns, beside the value, the magnitude M
of each output element: the same expression evaluated on |x| and |w|.  The check is the deterministic fp32 bound

    |got - ref| <= (n + 4) * 2^-24 * M + eps_epi

n = the products in the element's sum (5 * Cin for the window forms, the rows summed for weight gradients) and eps_epi
= one rounding per elementwise epilogue step, each at most 2^-24 times the magnitude carried to that step.  A correct
fp32 kernel cannot exceed it (fp32 MFMA measures 0.75-1.5e-7 * sum|a b|, far below n * 2^-24 * M); one dropped tap
(Cin products) or one dropped sample exceeds it by orders of magnitude, which tests/test_stride2_ref.py shows."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24                  # unit roundoff of fp32
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_GELU, ACT_TANH = 0, 1, 2, 3, 4
GELU_DMAX = 1.13                # max |d/dv gelu(v)| = 1.1289 (at v = 1.4142...)


def tm_gather(Tin):
    """Output positions of Conv1d(k=5, s=2, p=2)."""
    return (Tin - 1) // 2 + 1


def _windows_s2(x):
    """(B, T, C) -> (B, (T - 1) // 2 + 1, C, 5): window k of output t is x[2t + k - 2] (zeros outside)."""
    B, T, C = x.shape
    xp = torch.cat([x.new_zeros(B, 2, C), x, x.new_zeros(B, 2, C)], dim=1)
    return xp.unfold(1, 5, 2)


def _windows_scatter(x, Tout):
    """(B, Tin, C) -> (B, Tout, C, 5): zero-stuffed input xs[2u] = x[u]; window i of output t is xs[t + i - 2], which
    ConvTranspose1d(k=5, s=2, p=2) multiplies with tap 4 - i."""
    B, Tin, C = x.shape
    xs = x.new_zeros(B, 2 * Tin - 1, C)
    xs[:, 0::2] = x
    xp = torch.cat([x.new_zeros(B, 2, C), xs, x.new_zeros(B, Tout + 2 - (2 * Tin - 1), C)], dim=1)
    return xp.unfold(1, 5, 1)


def _both(fn, *ts):
    d = [t.double() for t in ts]
    return fn(*d), fn(*(t.abs() for t in d))


def gather(x, w):
    """y[b,t,n] = sum_{c,k} x[b, 2t+k-2, c] w[n,c,k]: Conv1d(k=5, s=2, p=2) forward with w (N, Cin, 5); also the
    ConvTranspose1d data gradient (w = the transposed convolution's (Cin, Cout, 5) weight, N = its Cin).
    Returns (ref, M) in fp64, (B, Tm, N)."""
    return _both(lambda a, b: torch.einsum("btck,nck->btn", _windows_s2(a), b), x, w)


def _windows_s2k3(x):
    """(B, T, C) -> (B, (T - 1) // 2 + 1, C, 3): window k of output t is x[2t + k - 1] (zeros outside)."""
    B, T, C = x.shape
    xp = torch.cat([x.new_zeros(B, 1, C), x, x.new_zeros(B, 1, C)], dim=1)
    return xp.unfold(1, 3, 2)


def gather3(x, w):
    """y[b,t,n] = sum_{c,k} x[b, 2t+k-1, c] w[n,c,k]: Conv1d(k=3, s=2, p=1) forward with w (N, Cin, 3) -- no layer of the
    models, but thin_in_kernel admits it (Cin <= 8).  Returns (ref, M) in fp64, (B, (T - 1) // 2 + 1, N)."""
    return _both(lambda a, b: torch.einsum("btck,nck->btn", _windows_s2k3(a), b), x, w)


def scatter(x, w, Tout):
    """ConvTranspose1d(k=5, s=2, p=2) forward with w (Cin, N, 5) and Tout = 2 Tin (output_padding 1) or 2 Tin - 1; also
    the Conv1d data gradient (w = the Conv1d's (Cout, Cin, 5) weight).  Returns (ref, M) in fp64, (B, Tout, N)."""
    Tin = x.shape[1]
    if Tout not in (2 * Tin, 2 * Tin - 1):
        raise ValueError(f"scatter: Tout={Tout} must be 2*Tin or 2*Tin-1 (Tin={Tin})")
    return _both(lambda a, b: torch.einsum("btci,cni->btn", _windows_scatter(a, Tout), b.flip(2)), x, w)


def _cat(seg0, seg1):
    return seg0 if seg1 is None else torch.cat([seg0, seg1], dim=0)


def conv_wgrad(x, dy, x2=None, dy2=None):
    """Weight gradient of Conv1d(k=5, s=2, p=2) in the Conv1d layout: dw[n,c,k] = sum_{b,t} dy[b,t,n] x[b,2t+k-2,c] over
    both segments, db[n] = sum_{b,t} dy[b,t,n] over segment 0 only (the second segment carries no bias).
    Returns ((dw, M_dw, n_dw), (db, M_db, n_db))."""
    xs, ds = _cat(x, x2), _cat(dy, dy2)
    dw = _both(lambda a, b: torch.einsum("btn,btck->nck", b, _windows_s2(a)), xs, ds)
    db = _both(lambda b: b.sum(dim=(0, 1)), dy)
    return (dw[0], dw[1], ds.shape[0] * ds.shape[1]), (db[0], db[1], dy.shape[0] * dy.shape[1])


def convT_wgrad(x, dy):
    """Weight gradient of ConvTranspose1d(k=5, s=2, p=2, output_padding=1) in its (Cin, Cout, 5) layout:
    dw[c,n,k] = sum_{b,u} x[b,u,c] dy[b,2u+k-2,n], db[n] = sum_{b,t} dy[b,t,n].  Returns ((dw, M, n), (db, M, n))."""
    dw = _both(lambda a, b: torch.einsum("buc,bunk->cnk", a, _windows_s2(b)), x, dy)
    db = _both(lambda b: b.sum(dim=(0, 1)), dy)
    return (dw[0], dw[1], x.shape[0] * x.shape[1]), (db[0], db[1], dy.shape[0] * dy.shape[1])


def act_ref(act, v):
    if act == ACT_NONE:
        return v
    if act == ACT_RELU:
        return torch.relu(v)
    if act == ACT_LRELU:
        return torch.where(v > 0, v, 0.2 * v)
    if act == ACT_GELU:
        return F.gelu(v)
    if act == ACT_TANH:
        return torch.tanh(v)
    raise ValueError(f"act {act}")


def act_grad_ref(gact, r):
    """The epilogue's derivative factor from a saved reference value r (mg_act_grad)."""
    if gact == ACT_NONE:
        return torch.ones_like(r)
    if gact == ACT_RELU:
        return (r > 0).to(r.dtype)
    if gact == ACT_LRELU:
        return torch.where(r > 0, 1.0, 0.2).to(r.dtype)
    if gact == ACT_TANH:
        return 1.0 - r * r
    if gact == ACT_GELU:
        c = torch.exp(-0.5 * r * r) * 0.3989422804014327
        return 0.5 * (1.0 + torch.erf(r * 0.7071067811865476)) + r * c
    raise ValueError(f"gact {gact}")


class Ref:
    """An fp64 reference with its error budget: value, magnitude M (sum |terms| carried through the epilogue), the
    product count n of the dot product, and the extra epilogue rounding budget (eps_epi in units of 2^-24 * M, plus an
    absolute part for transcendental activations)."""

    def __init__(self, val, mag, n):
        self.val, self.mag, self.n = val, mag, n
        self.k_epi = 0
        self.eps_abs = torch.zeros_like(val)
        self.z = None

    def epilogue(self, bias=None, scale=None, shift=None, zout=False, act=ACT_NONE, gref=None, gact=ACT_NONE,
                 emul=None, gscale=None, base=None):
        """Apply the fused epilogue of the kernels (mg_apply_epilogue order) in fp64: v = (acc + bias) * scale + shift
        [-> zout]; v = act(v); v *= act'(gref); v *= emul; v *= gscale; v += base (accumulate).  Each step that rounds in
        fp32 adds one 2^-24 * M to the budget; a transcendental step adds its derivative bound on top."""
        d = lambda t: t.double().to(self.val.device)  # noqa: E731
        v, m = self.val, self.mag
        if bias is not None:
            v, m = v + d(bias), m + d(bias).abs()
            self.k_epi += 1
        if scale is not None:
            v, m = v * d(scale) + d(shift), m * d(scale).abs() + d(shift).abs()
            self.k_epi += 2
        if zout:
            self.z = Ref(v, m, self.n)
            self.z.k_epi = self.k_epi
            self.z.eps_abs = self.eps_abs.clone()
        if act != ACT_NONE:
            v = act_ref(act, v)
            if act in (ACT_GELU, ACT_TANH):
                m = m * (GELU_DMAX if act == ACT_GELU else 1.0)
                self.eps_abs = self.eps_abs * (GELU_DMAX if act == ACT_GELU else 1.0) + 8 * U * (v.abs() + 1e-30)
            self.k_epi += 1
        if gref is not None:
            r = d(gref)
            f = act_grad_ref(gact, r)
            if gact in (ACT_GELU, ACT_TANH):      # the factor itself is computed in fp32: a few roundings of 1 + r^2
                self.eps_abs = self.eps_abs * f.abs() + 8 * U * (1.0 + r * r) * v.abs()
            else:
                self.eps_abs = self.eps_abs * f.abs()
            v, m = v * f, m * f.abs()
            self.k_epi += 1
        if emul is not None:
            e = d(emul)
            v, m, self.eps_abs = v * e, m * e.abs(), self.eps_abs * e.abs()
            self.k_epi += 1
        if gscale is not None:
            g = d(gscale)
            v, m, self.eps_abs = v * g, m * g.abs(), self.eps_abs * g.abs()
            self.k_epi += 1
        if base is not None:
            v, m = v + d(base), m + d(base).abs()
            self.k_epi += 1
        self.val, self.mag = v, m
        return self

    def bound(self):
        return (self.n + 4 + self.k_epi) * U * self.mag + self.eps_abs


def worst(got, ref: Ref):
    """(ratio of the worst element's error to its bound, its index, error, bound).  Non-finite got -> ratio inf."""
    g = got.detach().to(ref.val.device).double()
    err = (g - ref.val).abs()
    bnd = ref.bound()
    ratio = err / (bnd + 1e-300)
    ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, float("inf")))
    i = int(torch.argmax(ratio))
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
    return float(ratio.flatten()[i]), idx, float(err.flatten()[i]), float(bnd.flatten()[i])


def check(got, ref: Ref, what=""):
    """Assert |got - ref| <= bound element by element; the message names the worst element (b, t, n) and its ratio."""
    if tuple(got.shape) != tuple(ref.val.shape):
        raise AssertionError(f"{what}: shape {tuple(got.shape)} != reference {tuple(ref.val.shape)}")
    r, idx, e, b = worst(got, ref)
    assert r <= 1.0, f"{what}: worst element {idx}: |err| {e:.3e} = {r:.3g} x bound {b:.3e} (n={ref.n})"
    return r


class Guarded:
    """An output tensor placed inside a flat canvas with `rows` sentinel rows (of the last dimension) on both sides.
    .t is the (contiguous) output, prefilled with `fill`; .check() asserts that every sentinel is bit-for-bit intact."""

    SENTINEL = -1.2345678e33

    def __init__(self, shape, device="cuda", dtype=torch.float32, fill=float("nan"), rows=64):
        n = 1
        for s in shape:
            n *= s
        self.pad = rows * shape[-1]
        self.canvas = torch.full((n + 2 * self.pad,), self.SENTINEL, device=device, dtype=dtype)
        self.t = self.canvas[self.pad:self.pad + n].view(*shape)
        self.t.fill_(fill)

    def check(self, what=""):
        head, tail = self.canvas[:self.pad], self.canvas[self.canvas.numel() - self.pad:]
        # a bf16 (or any narrower) canvas holds the sentinel rounded to its dtype: compare with that value
        sent = self.SENTINEL if self.canvas.dtype == torch.float32 else torch.tensor(self.SENTINEL, dtype=self.canvas.dtype,
                                                                                     device=self.canvas.device)
        for nm, s in (("before", head), ("after", tail)):
            bad = (s != sent).nonzero()
            assert bad.numel() == 0, f"{what}: {bad.numel()} sentinel element(s) {nm} the output overwritten (first {int(bad[0])})"
