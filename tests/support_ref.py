"""fp64 references of the streaming kernels of csrc/small_kernels.hip (column sums, BatchNorm forward / backward / eval,
the mean over time, LayerNorm(6), the critic head, the WGAN-GP pieces, the losses, the elementwise helpers, flat Adam, the
gradient-norm clip and the VAE pieces) with the per-element bound their fp32 results are held to.  A plain helper module
beside stride2_ref / window_ref (whose U / Ref / check / worst / Guarded / act_ref / act_grad_ref it uses unchanged);
nothing here is collected.  Every function works on whatever device its inputs are on and returns Ref objects, so that
check(got, ref, what) applies.

Every reference is written from the mathematical definition (torch.nn semantics restated by hand in fp64: tests/
test_support_ref.py compares them with torch's fp64 modules and autograd wherever torch defines the operation), never from
a kernel.  Scalars a kernel receives as fp32 (momentum, eps, lr, the betas, ...) enter as the fp32 value, f32(): the
reference computes from the same inputs.  The bounds count roundings; none is tuned.  k is the number of fp32 roundings
on the element's path in a correct implementation, 4 the project's constant (stride2_ref):

  fp32-accumulated sums of n terms    (n + 4 + k) U M, M the same expression on absolute values.  No extra budget for a
                                      wave / block / partial split: a term passes through at most n - 1 additions whatever
                                      the tree.
  fp64-accumulated reductions         (4 + k) U M + n 2^-53 M: n does not enter at fp32 scale (the fp64 term is 2^-29 of an
  rounded once to fp32                fp32 rounding per term).  A kernel that falls back to fp32 accumulation fails here.
  BatchNorm statistics                mean: the line above with M = sum|z| / R.  invstd = (var + eps)^-1/2: one rounding
                                      (k = 1, M = invstd) plus the conditioning of the variance in fp64,
                                      (R + 4) 2^-53 (E[z^2] + mean^2) / (var + eps) / 2 relative -- what one-pass fp64 sums
                                      of squares (or any fp64 formulation) are good for; on z = 100 + 0.01 randn, R = 1000
                                      that is 1e-5, while fp32 E[z^2] - mean^2 is wrong by O(1).
  BatchNorm apply                     M = (|z| + |mean|) invstd |gamma| + |beta|, budget 4 U M: the rounding of save_mean,
                                      that of save_invstd, the final rounding and one spare.  An activation on top adds
                                      stride2_ref's epilogue terms (Ref.epilogue) unchanged.
  BatchNorm backward                  dz = gamma invstd (dy - S1 / R - xhat S2 / R): the magnitude of each of the three
                                      terms carried through gamma invstd, |xhat| <= (|z| + |mean|) invstd; k = 2 (the fp32
                                      product dy = da act'(.), the final rounding).
  transcendental steps                an absolute term 8 U |value| per expf / logf / sqrtf / rcp step, scaled through what
                                      follows.  GELU and GELU' are the Abramowitz-Stegun 7.1.26 forms of csrc/common.h:
                                      |GELU error| <= 4.2e-7, |GELU' error| <= 3.2e-7, absolute, a property of the
                                      approximation.  tanh' = 1 - r^2 in fp32: 4 U (1 + r^2).  LeakyReLU's 0.2f: U 0.2.
  Adam                                one step from a given state; the roundings of m, v, sqrt, the division and the final
                                      subtraction are counted in adam_step's docstring.

tests/test_support_ref.py shows that fp32 host computations stay inside every bound and that each of a list of plausible
mistakes leaves it."""
import math

import torch
import torch.nn.functional as F

from stride2_ref import Ref, check, worst, Guarded, act_ref, act_grad_ref, U  # noqa: F401  (re-exported for the tests)
from stride2_ref import ACT_NONE, ACT_RELU, ACT_LRELU, ACT_GELU, ACT_TANH, GELU_DMAX  # noqa: F401

U64 = 2.0 ** -53                # unit roundoff of fp64
GELU_ERR = 4.2e-7               # csrc/common.h: |GELU error| of the A-S 7.1.26 form, measured in fp32 over [-8, 8]
GELU_GRAD_ERR = 3.2e-7          # csrc/common.h: |GELU' error|
GELU_D2MAX = 0.8                # max |GELU''| = 2 phi(0) = 0.7979
TRANS = 8                       # an expf / logf / sqrtf / rcp step: 8 U |value| (stride2_ref's eps_abs)
TINY = 2.0 ** -126              # the smallest normal fp32: what an expf result below it may be flushed to zero by


def f32(v):
    """The fp32 value of a Python scalar, as a Python float: what a kernel receives for a `float` argument."""
    return float(torch.tensor(v, dtype=torch.float32))


def d(t):
    return t.double()


def mk(val, mag, n=0, k=0, eps_abs=None):
    """Ref(val, mag, n) with k epilogue roundings and an absolute term: bound = (n + 4 + k) U mag + eps_abs."""
    r = Ref(val, mag, n)
    r.k_epi = k
    if eps_abs is not None:
        r.eps_abs = eps_abs + torch.zeros_like(val)
    return r


def grad_factor(gact, r, r_err=None):
    """(act'(r), the absolute error of the fp32 factor) for a saved value r (fp64).  r_err: the error of r itself where
    the kernel recomputes it (BatchNorm backward under GELU), carried through |act''| <= GELU_D2MAX."""
    f = act_grad_ref(gact, r)
    if gact == ACT_GELU:
        e = torch.full_like(r, GELU_GRAD_ERR)
        if r_err is not None:
            e = e + GELU_D2MAX * r_err
    elif gact == ACT_TANH:
        e = 4 * U * (1.0 + r * r)
    elif gact == ACT_LRELU:
        e = U * f.abs()
    else:
        e = torch.zeros_like(r)
    return f, e


def act_on(ref: Ref, act):
    """stride2_ref's activation step on a Ref, plus the absolute A-S figure for GELU."""
    ref.epilogue(act=act)
    if act == ACT_GELU:
        ref.eps_abs = ref.eps_abs + GELU_ERR
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# column sums and BatchNorm
# ---------------------------------------------------------------------------------------------------------------------
def rows(x):
    return x.reshape(-1, x.shape[-1])


def colsum(x):
    """(sum_r x[r, c], sum_r x[r, c]^2) over all leading dimensions; fp64 accumulation, one rounding each."""
    x = d(rows(x))
    R = x.shape[0]
    s, m = x.sum(0), x.abs().sum(0)
    q = (x * x).sum(0)
    return mk(s, m, 0, 1, R * U64 * m), mk(q, q, 0, 1, R * U64 * q)


def bn_stats(z, groups=1, eps=1e-5):
    """Per-group batch statistics of z (groups * R rows, C): dict of fp64 (groups, C) tensors mean, var (biased), unb
    (unbiased; R = 1: the biased value, 0 -- torch raises there, the project keeps the running variance moving towards 0),
    invstd = (var + eps)^-1/2, and Refs `save_mean`, `save_invstd`."""
    eps = f32(eps)
    x = d(rows(z))
    C = x.shape[1]
    x = x.view(groups, -1, C)
    R = x.shape[1]
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    unb = var * R / (R - 1) if R > 1 else var
    invstd = (var + eps) ** -0.5
    mabs = x.abs().mean(1)
    ex2 = (x * x).mean(1)
    cond = 0.5 * (R + 4) * U64 * (ex2 + mean * mean) / (var + eps)
    return dict(R=R, mean=mean, var=var, unb=unb, invstd=invstd, mabs=mabs, e_mean=R * U64 * mabs,
                e_unb=2.0 * cond * (var + eps) * (R / (R - 1.0) if R > 1 else 1.0),
                save_mean=mk(mean, mabs, 0, 1, R * U64 * mabs), save_invstd=mk(invstd, invstd, 0, 1, cond * invstd))


def bn_running(st, running_mean, running_var, momentum=0.1):
    """Running statistics after one training forward per group, group after group (`groups` consecutive calls of
    nn.BatchNorm1d): r <- (1 - momentum) r + momentum stat, rounded to fp32 after every call.  Refs (rm, rv)."""
    mom = f32(momentum)
    out = []
    for r0, stat, sabs, serr in ((running_mean, st["mean"], st["mabs"], st["e_mean"]), (running_var, st["unb"], st["unb"], st["e_unb"])):
        v = d(r0)
        m = v.abs()
        e = torch.zeros_like(v)
        G = stat.shape[0]
        for g in range(G):
            v = (1.0 - mom) * v + mom * stat[g]
            m = (1.0 - mom) * m + mom * sabs[g]
            e = (1.0 - mom) * e + mom * serr[g]       # the statistic's own fp64 conditioning (bn_stats)
        out.append(mk(v, m, 0, G, e))          # one fp32 rounding per call
    return out


def bn_apply(z, mean, invstd, gamma, beta, act=ACT_NONE):
    """a = act((z - mean) invstd gamma + beta) with per-group statistics mean / invstd (groups, C) (fp64: the exact ones
    in training, whatever is passed otherwise); z (groups * R rows, C).  Budget 4 U M before the activation."""
    x = d(rows(z))
    C = x.shape[1]
    G = mean.shape[0]
    x = x.view(G, -1, C)
    g, b = d(gamma), d(beta)
    mu, is_ = d(mean)[:, None], d(invstd)[:, None]
    v = (x - mu) * is_ * g + b
    m = (x.abs() + mu.abs()) * is_ * g.abs() + b.abs()
    return act_on(mk(v.reshape(z.shape), m.reshape(z.shape), 0, 0), act)


def bn_eval(z, gamma, beta, rm, rv, eps=1e-5, act=ACT_NONE):
    """Eval-mode BatchNorm in fp32 arithmetic: (z - rm) / sqrt(rv + eps) gamma + beta -- the subtraction, rv + eps, the
    square root, the division, the product and the sum round: k = 6."""
    eps = f32(eps)
    x, g, b, m_, v_ = d(z), d(gamma), d(beta), d(rm), d(rv)
    s = (v_ + eps) ** -0.5
    v = (x - m_) * s * g + b
    m = (x.abs() + m_.abs()) * s * g.abs() + b.abs()
    return act_on(mk(v, m, 0, 6), act)


def bn_fold(gamma, beta, rm, rv, conv_bias=None, eps=1e-5):
    """scale = gamma / sqrt(rv + eps) (k = 3), shift = beta + (conv_bias - rm) scale (k = 3 more, + 1 with a bias)."""
    eps = f32(eps)
    g, b, m_, v_ = d(gamma), d(beta), d(rm), d(rv)
    cb = d(conv_bias) if conv_bias is not None else torch.zeros_like(g)
    s = g * (v_ + eps) ** -0.5
    sh = b + (cb - m_) * s
    return mk(s, s.abs(), 0, 3), mk(sh, b.abs() + (cb.abs() + m_.abs()) * s.abs(), 0, 6 + (conv_bias is not None))


def bn_bwd(da, a, z, gamma, beta, save_mean, save_invstd, act):
    """Training-mode BatchNorm backward behind an activation, from the SAVED fp32 statistics (inputs of the operation):
    dy = da act'(.), act' taken at the saved activation a (ReLU / LeakyReLU / tanh) or at the BN output recomputed from z
    (GELU); dbeta = sum dy, dgamma = sum dy xhat, dz = gamma invstd (dy - dbeta / R - xhat dgamma / R).
    Returns Refs (dz, dgamma, dbeta)."""
    x, g = d(rows(z)), d(gamma)
    R = x.shape[0]
    mu, is_ = d(save_mean), d(save_invstd)
    xh = (x - mu) * is_
    mxh = (x.abs() + mu.abs()) * is_
    if act == ACT_GELU:
        b = d(beta)
        y = xh * g + b
        fac, fe = grad_factor(act, y, 4 * U * (mxh * g.abs() + b.abs()))
    else:
        fac, fe = grad_factor(act, d(rows(a)))
    dd = d(rows(da))
    dy, ady, edy = dd * fac, (dd * fac).abs(), dd.abs() * fe
    S1, M1, E1 = dy.sum(0), ady.sum(0), edy.sum(0)
    S2, M2, E2 = (dy * xh).sum(0), (ady * mxh).sum(0), (edy * mxh).sum(0)
    dbeta = mk(S1, M1, 0, 2, E1 + R * U64 * M1)
    dgamma = mk(S2, M2, 0, 2, E2 + R * U64 * M2)
    gi = g.abs() * is_
    dz = g * is_ * (dy - S1 / R - xh * S2 / R)
    mz = gi * (ady + M1 / R + mxh * M2 / R)
    ez = gi * (edy + E1 / R + mxh * E2 / R)
    return mk(dz.reshape(z.shape), mz.reshape(z.shape), 0, 2, ez.reshape(z.shape)), dgamma, dbeta


def split_rows(R, np_, empty_rows=(), seed=0):
    """np_ chunk sizes summing to R, the chunks in empty_rows of size 0, the others very unequal (at least one row each
    while rows last; a few large chunks take the rest)."""
    live = [i for i in range(np_) if i not in set(empty_rows)]
    if not live or R < 1:
        raise ValueError("split_rows: no live chunk")
    gen = torch.Generator().manual_seed(seed)
    sizes = [0] * np_
    left = R
    for i in live:
        if left == 0:
            break
        sizes[i] = 1
        left -= 1
    w = torch.rand(len(live), generator=gen) ** 6 + 1e-9
    share = torch.floor(w / w.sum() * left).long().tolist()
    for i, s in zip(live, share):
        if sizes[i]:
            sizes[i] += s
            left -= s
    sizes[live[0]] += left
    assert sum(sizes) == R
    return sizes


def conv16_parts(z, np_, empty_rows=(), seed=0):
    """The (np_, 3, C) fp32 partial statistics bn_train_fwd_parts consumes, for an arbitrary split of z's rows into np_
    chunks: per chunk the column sum, M2 = sum (z - chunk mean)^2 about the chunk's OWN mean, and the row count (0 for the
    chunks in empty_rows, whose other planes then hold garbage a correct combine must not read into the result).  The
    planes are the fp64 values rounded to fp32: what the producer hands over."""
    x = d(rows(z))
    R, C = x.shape
    sizes = split_rows(R, np_, empty_rows, seed)
    out = torch.empty(np_, 3, C, dtype=torch.float64, device=x.device)
    r = 0
    for p, s in enumerate(sizes):
        if s == 0:
            out[p, 0], out[p, 1], out[p, 2] = 1e30, 1e30, 0.0
            continue
        c = x[r:r + s]
        out[p, 0] = c.sum(0)
        out[p, 1] = ((c - c.mean(0)) ** 2).sum(0)
        out[p, 2] = float(s)
        r += s
    return out.float(), sizes


def parts_stats(part, eps=1e-5):
    """Statistics of the whole from conv16_parts-style fp32 partials (np, 3, C) of ONE group, by the parallel-variance
    rule in fp64: n = sum n_p, mean = sum S_p / n, M2 = sum M2_p + sum n_p (S_p / n_p - mean)^2.  The inputs of the
    operation are the ROUNDED partials, so the result differs from the statistics of the raw rows by their rounding;
    the combine itself is exact up to fp64.  Returns the same dict as bn_stats (one group)."""
    eps = f32(eps)
    p = d(part)
    live = p[:, 2, 0] > 0
    S, Q, n = p[live, 0], p[live, 1], p[live, 2]
    N = n.sum(0)
    mean = S.sum(0) / N
    cm = S / n
    m2 = Q.sum(0) + (n * (cm - mean) ** 2).sum(0)
    var = m2 / N
    R = int(N[0].item())
    unb = var * R / (R - 1) if R > 1 else var
    invstd = (var + eps) ** -0.5
    mabs = S.abs().sum(0) / N
    npl = S.shape[0]
    # fp64 conditioning of the between-chunk term: sum n_p cm_p^2 against N mean^2
    cond = 0.5 * (npl + 4) * U64 * ((n * cm * cm).sum(0) / N + mean * mean) / (var + eps)
    one = lambda t: t[None]  # noqa: E731
    return dict(R=R, mean=one(mean), var=one(var), unb=one(unb), invstd=one(invstd), mabs=one(mabs), e_mean=one(npl * U64 * mabs),
                e_unb=one(2.0 * cond * (var + eps) * (R / (R - 1.0) if R > 1 else 1.0)),
                save_mean=mk(one(mean), one(mabs), 0, 1, one(npl * U64 * mabs)),
                save_invstd=mk(one(invstd), one(invstd), 0, 1, one(cond * invstd)))


def cat_stats(sts):
    """Stack per-group dicts of parts_stats into one of bn_stats' form."""
    out = dict(R=sts[0]["R"])
    for k in ("mean", "var", "unb", "invstd", "mabs", "e_mean", "e_unb"):
        out[k] = torch.cat([s[k] for s in sts])
    for k in ("save_mean", "save_invstd"):
        out[k] = mk(torch.cat([s[k].val for s in sts]), torch.cat([s[k].mag for s in sts]), 0, 1,
                    torch.cat([s[k].eps_abs for s in sts]))
    return out


def bwd_parts(da, a, z, save_mean, save_invstd, act, np_, seed=0):
    """The (np_, 2, C) fp64 partial sums bn_train_bwd_parts consumes -- per chunk sum dy and sum dy xhat, dy the fp32
    product da act'(a) the producer forms (ReLU / LeakyReLU: the mask is exact) -- for a very unequal split of the rows
    (no chunk is left out: an empty one holds zeros)."""
    x = d(rows(z))
    R = x.shape[0]
    fac = act_grad_ref(act, rows(a).float())
    dy = d(rows(da).float() * fac)
    xh = (x - d(save_mean)) * d(save_invstd)
    sizes = split_rows(R, np_, (), seed) if np_ <= R else [1] * R + [0] * (np_ - R)
    out = torch.zeros(np_, 2, x.shape[1], dtype=torch.float64, device=x.device)
    r = 0
    for p, s in enumerate(sizes):
        out[p, 0] = dy[r:r + s].sum(0)
        out[p, 1] = (dy[r:r + s] * xh[r:r + s]).sum(0)
        r += s
    return out


# ---------------------------------------------------------------------------------------------------------------------
# mean over time, LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def meanT_fwd(a):
    """h[b, c] = mean_t a[b, t, c]: n = T fp32 terms, k = 1 (the division)."""
    x = d(a)
    T = x.shape[1]
    return mk(x.mean(1), x.abs().mean(1), T, 1)


def meanT_bwd(dh, T, gref=None, gact=ACT_NONE, gscale=None):
    """dz[b, t, c] = dh[b, c] / T * act'(gref[b, t, c]) * gscale[c].  k = 2 (1 / T and the product) + one per factor."""
    v = (d(dh) / T)[:, None, :].expand(-1, T, -1)
    m, k = v.abs(), 2
    e = torch.zeros_like(v)
    if gref is not None:
        f, fe = grad_factor(gact, d(gref))
        e = v.abs() * fe
        v, m, k = v * f, m * f.abs(), k + 1
    if gscale is not None:
        g = d(gscale)
        v, m, e, k = v * g, m * g.abs(), e * g.abs(), k + 1
    return mk(v.contiguous(), m.contiguous(), 0, k, e.contiguous())


def mean_scaled(src, scale=1.0):
    """out[0] = scale * mean(src): n terms, k = 2 (the product and the division)."""
    s = d(src).flatten()
    sc = f32(scale)
    return mk((sc * s.mean()).reshape(1), (abs(sc) * s.abs().mean()).reshape(1), s.numel(), 2)


def layernorm_fwd(x, gamma, beta, eps=1e-5):
    """LayerNorm over the last dimension (biased variance), Refs (y, xhat).  The bound follows a two-pass fp32
    computation: the mean is a D-term sum (e_mean = (D + 5) U mean|x|); c = x - mean carries e_c = e_mean + U (|x| +
    |mean|); the variance a D-term sum of c^2 (e_var = (D + 5) U var + 2 mean(|c| e_c)); invstd = 1 / sqrt(var + eps)
    three roundings (the sum, the root, the reciprocal) on top of e_var / (2 (var + eps)); xhat = c invstd one more; y =
    xhat gamma + beta two more."""
    eps = f32(eps)
    v, g, b = d(x), d(gamma), d(beta)
    D = v.shape[-1]
    mean = v.mean(-1, keepdim=True)
    e_mean = (D + 5) * U * v.abs().mean(-1, keepdim=True)
    c = v - mean
    e_c = e_mean + U * (v.abs() + mean.abs())
    var = (c * c).mean(-1, keepdim=True)
    e_var = (D + 5) * U * var + 2.0 * (c.abs() * e_c).mean(-1, keepdim=True) + (e_c * e_c).mean(-1, keepdim=True)
    is_ = (var + eps) ** -0.5
    rel_is = 0.5 * e_var / (var + eps) + (3 + TRANS) * U
    xh = c * is_
    e_xh = e_c * is_ + c.abs() * is_ * rel_is
    y = xh * g + b
    e_y = e_xh * g.abs()
    return mk(y, xh.abs() * g.abs() + b.abs(), 0, 2, e_y), mk(xh, xh.abs(), 0, 1, e_xh)


def layernorm_bwd_params(dy, xhat):
    """dgamma = sum_b dy xhat (n = B products), dbeta = sum_b dy (n = B)."""
    a, h = d(dy), d(xhat)
    B = a.shape[0]
    return mk((a * h).sum(0), (a * h).abs().sum(0), B, 0), mk(a.sum(0), a.abs().sum(0), B, 0)


# ---------------------------------------------------------------------------------------------------------------------
# critic head
# ---------------------------------------------------------------------------------------------------------------------
def _emb_rows(emb, B):
    Be = emb.shape[0]
    return d(emb)[torch.arange(B, device=emb.device) % Be]


def dhead_fwd(f, emb, w, bias):
    """s[b] = f[b] . w[:F] + emb[b % Be] . w[F:] + bias: n = F + E products, k = 1."""
    ff, ww = d(f), d(w).flatten()
    B, Fd = ff.shape
    s, m, n = ff @ ww[:Fd], ff.abs() @ ww[:Fd].abs(), Fd
    if emb is not None:
        e = _emb_rows(emb, B)
        s, m, n = s + e @ ww[Fd:], m + e.abs() @ ww[Fd:].abs(), n + emb.shape[1]
    b = d(bias).flatten()[0]
    return mk(s + b, m + b.abs(), n, 1)


def dhead_bwd(ds, f, w, Be=0, E=0, nb_emb=0):
    """dU[b, j] = ds[b] w[j] lrelu'(f[b, j]) (k = 3: two products and the constant 0.2f);
    demb[be, j] = (sum over rows b = be, be + Be, ... < nb_emb of ds[b]) w[F + j] (n = nb_emb / Be, k = 1)."""
    s, ff, ww = d(ds), d(f), d(w).flatten()
    Fd = ff.shape[1]
    slope = torch.where(ff > 0, torch.ones_like(ff), torch.full_like(ff, 0.2))
    dU = s[:, None] * ww[None, :Fd] * slope
    out = [mk(dU, dU.abs(), 0, 3)]
    if E:
        grp = s[:nb_emb].view(-1, Be)
        sm, sa = grp.sum(0), grp.abs().sum(0)
        out.append(mk(sm[:, None] * ww[None, Fd:], sa[:, None] * ww[None, Fd:].abs(), nb_emb // Be, 1))
    return out


def dhead_wgrad(ds, f, emb, gf, nb, ng):
    """dw[j < F] = sum_{b < nb} ds[b] f[b, j] + sum_{b < ng} gf[b, j]; dw[F + j] = sum_{b < nb} ds[b] emb[b % Be, j];
    dbias = sum_{b < nb} ds[b].  Refs (dw[:F] (n = nb + ng), dw[F:] (n = nb; None without emb), dbias (n = nb))."""
    s, ff = d(ds)[:nb], d(f)[:nb]
    v, m, n = s @ ff, s.abs() @ ff.abs(), nb
    if gf is not None:
        g = d(gf)[:ng]
        v, m, n = v + g.sum(0), m + g.abs().sum(0), n + ng
    dwe = None
    if emb is not None:
        e = _emb_rows(emb, nb)
        dwe = mk(s @ e, s.abs() @ e.abs(), nb, 0)
    return mk(v, m, n, 0), dwe, mk(s.sum().reshape(1), s.abs().sum().reshape(1), nb, 0)


def wgan_d_loss(s, norms, lambda_gp, nb):
    """The critic's loss scalars from s = [D(real) (nb), D(fake) (nb)] and the gradient norms: mean_real, mean_fake (n = nb,
    k = 1), gp = mean((norms - 1)^2) (n = nb; the difference rounds relative to |norms| + 1: k = 3 on M = mean((|norms| +
    1)^2)) and loss_d = mean_fake - mean_real + lambda gp (the three bounds added, three more roundings).
    Refs (loss_d, mean_real, mean_fake, gp), (1,) each."""
    lam = f32(lambda_gp)
    sv, nv = d(s).flatten(), d(norms).flatten()
    r, fk = sv[:nb], sv[nb:2 * nb]
    mr, mf = mk(r.mean().reshape(1), r.abs().mean().reshape(1), nb, 1), mk(fk.mean().reshape(1), fk.abs().mean().reshape(1), nb, 1)
    gp = mk(((nv - 1) ** 2).mean().reshape(1), ((nv.abs() + 1) ** 2).mean().reshape(1), nb, 3)
    val = mf.val - mr.val + lam * gp.val
    mag = mf.val.abs() + mr.val.abs() + abs(lam) * gp.val.abs()
    loss = mk(val, mag, 0, 3, mf.bound() + mr.bound() + abs(lam) * gp.bound())
    return loss, mr, mf, gp


# ---------------------------------------------------------------------------------------------------------------------
# WGAN-GP and losses
# ---------------------------------------------------------------------------------------------------------------------
def gp_interp(real, fake, alpha):
    """xhat = alpha real + (1 - alpha) fake per sample: 1 - alpha, one product and the fused multiply-add round: k = 3."""
    r, fk = d(real), d(fake)
    a = d(alpha).view(-1, *([1] * (r.dim() - 1)))
    return mk(a * r + (1 - a) * fk, a.abs() * r.abs() + (1 + a.abs()) * fk.abs(), 0, 3)


def gp_penalty(g, coef):
    """Per sample b: norms[b] = |g_b|_2, gbar_b = coef (2 / B) (norms - 1) / norms g_b (0 for a zero gradient): the
    gradient of coef mean((norms - 1)^2); gp = mean((norms - 1)^2).
    norms: n fp32 products and additions under a square root: ((n + 5) / 2 + TRANS) U norms.  The factor: 2 / B, the
    product with coef, norms - 1 (relative to norms + 1), one product and the division (k = 5, M = c (norms + 1) / norms),
    plus the error of norms through d fac / d norms = c / norms^2.  gbar: one more product.  gp: B terms."""
    c = f32(coef)
    x = d(g).reshape(g.shape[0], -1)
    B, n = x.shape
    s = (x * x).sum(1)
    nrm = s.sqrt()
    e_n = ((n + 5) / 2.0 + TRANS) * U * nrm
    norms = mk(nrm, nrm, 0, 0, e_n)
    safe = torch.where(nrm > 0, nrm, torch.ones_like(nrm))
    c2 = abs(c) * 2.0 / B
    fac = torch.where(nrm > 0, c * (2.0 / B) * (nrm - 1) / safe, torch.zeros_like(nrm))
    e_f = torch.where(nrm > 0, c2 * e_n / (safe * safe) + (5 + TRANS) * U * c2 * (nrm + 1) / safe, torch.zeros_like(nrm))
    gbar = mk((fac[:, None] * x).reshape(g.shape), (fac.abs()[:, None] * x.abs()).reshape(g.shape), 0, 1,
              (e_f[:, None] * x.abs()).reshape(g.shape))
    dd = nrm - 1
    e_d = e_n + U * (nrm + 1)
    gp = mk((dd * dd).mean().reshape(1), (dd * dd).mean().reshape(1), B, 2, ((2 * dd.abs() * e_d + e_d * e_d).mean()).reshape(1))
    return norms, gbar, gp


def softmax_ce(logits, target, coef=1.0):
    """loss = mean_b (logsumexp(z_b) - z_b[y_b]); dlogits = coef (softmax(z_b) - onehot(y_b)) / B.  A target outside
    [0, C) makes the loss NaN and that row's dlogits NaN (torch raises; the project poisons -- csrc/small_kernels.hip,
    softmax_ce_kernel).  Per row in fp32: t_j = z_j - max rounds (U (|z_j| + |max|) absolute in the exponent, i.e.
    relative in exp), expf (TRANS U), a C-term sum, logf (TRANS U |log| + the sum's relative error), max + log rounds;
    the row loss rounds once more; B rows are summed in fp32 (n = B, k = 1).  dlogits: the exponent z_j - lse carries the
    error of lse and its own rounding; expf; the subtraction, the product and the division round; a probability below
    the smallest normal fp32 may come out as 0 (TINY, once for expf and once for the result)."""
    cf = f32(coef)
    z = d(logits)
    B, Cn = z.shape
    y = target.to(z.device)
    bad = (y < 0) | (y >= Cn)
    ys = torch.where(bad, torch.zeros_like(y), y)
    mx = z.max(1, keepdim=True).values
    ex = torch.exp(z - mx)
    se = ex.sum(1, keepdim=True)
    lse = mx + se.log()
    rel_se = U * (z.abs() + mx.abs()).max(1, keepdim=True).values + (TRANS + Cn + 4) * U
    e_lse = rel_se + TRANS * U * se.log().abs() + U * (mx.abs() + se.log().abs())
    zy = z.gather(1, ys[:, None])
    row = lse - zy
    e_row = e_lse + U * (lse.abs() + zy.abs())
    row = torch.where(bad[:, None], torch.full_like(row, float("nan")), row)
    loss = mk(row.mean().reshape(1), (lse.abs() + zy.abs()).mean().reshape(1), B, 1, e_row.mean().reshape(1))
    p = torch.exp(z - lse)
    oh = F.one_hot(ys, Cn).double()
    e_p = p * (e_lse + U * (z.abs() + lse.abs()) + TRANS * U)
    dl = cf * (p - oh) / B
    dl = torch.where(bad[:, None], torch.full_like(dl, float("nan")), dl)
    dlog = mk(dl, abs(cf) * (p + oh) / B, 0, 3, abs(cf) * (e_p + TINY) / B + TINY)
    return loss, dlog, bad


# ---------------------------------------------------------------------------------------------------------------------
# elementwise
# ---------------------------------------------------------------------------------------------------------------------
def axpby(x, y, a, b):
    """y <- a x + b y (b = 0: y is not read).  Two products and a sum: k = 3."""
    a, b = f32(a), f32(b)
    xv = d(x)
    if b == 0.0:
        return mk(a * xv, (a * xv).abs(), 0, 1)
    yv = d(y)
    return mk(a * xv + b * yv, (a * xv).abs() + (b * yv).abs(), 0, 3)


def act_bwd(dy, gref=None, gact=ACT_NONE, emul=None):
    """dx = dy act'(gref) emul: one rounding per factor."""
    v = d(dy)
    m, e, k = v.abs(), torch.zeros_like(v), 0
    if gref is not None:
        f, fe = grad_factor(gact, d(gref))
        e = v.abs() * fe
        v, m, k = v * f, m * f.abs(), k + 1
    if emul is not None:
        q = d(emul)
        v, m, e, k = v * q, m * q.abs(), e * q.abs(), k + 1
    return mk(v, m, 0, k, e)


# ---------------------------------------------------------------------------------------------------------------------
# optimiser and VAE
# ---------------------------------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, step, lr, beta1, beta2, eps=1e-8, weight_decay=0.0, grad_scale=1.0, gs_dev=None,
              decoupled=True):
    """One Adam / AdamW step number `step` (>= 1) in fp64 from fp32 inputs: g' = g grad_scale gs_dev; p <- p (1 - lr wd)
    (decoupled); m <- m + (g' - m)(1 - b1); v <- b2 v + (1 - b2) g'^2; p <- p - lr / (1 - b1^step) m / (sqrt(v) /
    sqrt(1 - b2^step) + eps).  decoupled=False is torch.optim.Adam's coupled decay g' += wd p (for the self-test).
    Roundings of a correct fp32 implementation: g' two (the scale product, the gradient product); m: 1 - b1, the
    difference, the product, the sum on top of g' -> k = 6 on M_m = |m| + (|g'| + |m|)(1 - b1); v: g' squared (4), 1 - b2,
    three products, the sum -> k = 9 on M_v = v (all terms positive); sqrt(v): half of that plus its own rounding;
    sqrt(1 - b2^step) rounded, the division, + eps -> 10.5 U denom in all; the update: lr / bc1 rounded, m / denom, the
    product -> step e_m / denom + 13.5 U |update|; the decay: lr wd, 1 - ., the product (3 U |p|); the final subtraction.
    Returns Refs (p, m, v)."""
    lr, b1, b2, eps, wd, gs = (f32(t) for t in (lr, beta1, beta2, eps, weight_decay, grad_scale))
    P, G, M_, V = d(p), d(g), d(m), d(v)
    if gs_dev is not None:
        gs = gs * float(d(gs_dev).flatten()[0])
    G = G * gs
    if wd != 0.0 and not decoupled:
        G = G + wd * P
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    Pd = P * (1.0 - lr * wd) if (wd != 0.0 and decoupled) else P
    mn = M_ + (G - M_) * (1.0 - b1)
    Mm = M_.abs() + (G.abs() + M_.abs()) * (1.0 - b1)
    vn = V * b2 + (1.0 - b2) * G * G
    rm, rv = mk(mn, Mm, 0, 6), mk(vn, vn, 0, 9)
    den = vn.sqrt() / math.sqrt(bc2) + eps
    ss = lr / bc1
    upd = ss * mn / den
    e_upd = ss * rm.bound() / den + 13.5 * U * upd.abs()
    e_p = (3 * U * P.abs() if wd != 0.0 else 0.0) + e_upd
    return mk(Pd - upd, Pd.abs() + upd.abs(), 0, 1, e_p), rm, rv


def wq_layout(w, N, Cc, K, cnk):
    """The WQ copy of a dense weight W(n, c, k): dst[((c // 4) K + k) N + n][c % 4] = W(n, c, k); w is the flat slice,
    laid out w[n][c][k] (cnk False) or w[c][n][k] (cnk True).  A pure re-layout: compared exactly."""
    Wn = w.view(Cc, N, K).permute(1, 0, 2) if cnk else w.view(N, Cc, K)          # (N, Cc, K)
    return Wn.view(N, Cc // 4, 4, K).permute(1, 3, 0, 2).contiguous().view(-1)    # (c / 4, k, n, c % 4)


def grad_norm_clip(g, max_norm):
    """out = (|g|_2, min(1, max_norm / (|g|_2 + 1e-6))): clip_grad_norm_'s total norm and coefficient.  The norm: n fp32
    products and additions under a square root; the coefficient: the sum with 1e-6 and the division round (the clamp is
    1-Lipschitz)."""
    mx, tiny = f32(max_norm), f32(1e-6)
    x = d(g).flatten()
    n = x.numel()
    nrm = (x * x).sum().sqrt()
    e_n = ((n + 5) / 2.0 + TRANS) * U * nrm
    c = mx / (nrm + tiny)
    e_c = c * e_n / (nrm + tiny) + 2 * U * c
    cc = torch.clamp(c, max=1.0)
    return mk(torch.stack([nrm, cc]), torch.stack([nrm, cc]), 0, 0, torch.stack([e_n, e_c]))


def reparam_fwd(mu, logvar, eps):
    """z = mu + eps exp(logvar / 2): expf, one product, one sum."""
    m_, l_, e_ = d(mu), d(logvar), d(eps)
    t = e_ * torch.exp(0.5 * l_)
    return mk(m_ + t, m_.abs() + t.abs(), 0, 2, TRANS * U * t.abs())


def reparam_bwd(dz, logvar, eps, dmu_kld=None, dlv_kld=None):
    """dmu = dz + dmu_kld; dlv = dz eps exp(logvar / 2) / 2 + dlv_kld.  Refs (dmu, dlv)."""
    z_, l_, e_ = d(dz), d(logvar), d(eps)
    a = d(dmu_kld) if dmu_kld is not None else torch.zeros_like(z_)
    b = d(dlv_kld) if dlv_kld is not None else torch.zeros_like(z_)
    t = z_ * e_ * 0.5 * torch.exp(0.5 * l_)
    return mk(z_ + a, z_.abs() + a.abs(), 0, 1), mk(t + b, t.abs() + b.abs(), 0, 4, TRANS * U * t.abs())


def vae_loss(recon, x, mu, logvar, beta):
    """out = (mse + beta kld, mse, kld) with mse = mean((recon - x)^2), kld = -mean(1 + logvar - mu^2 - exp(logvar)) / 2,
    and the gradients drecon = 2 (recon - x) / n_x, dmu = beta mu / n_z, dlv = -beta (1 - exp(logvar)) / (2 n_z).
    mse: the difference rounds relative to |recon| + |x|, so the squared term is relative to (|recon| + |x|)^2: n_x terms,
    k = 4 (two for the squared difference, the product, the final division).  kld: n_z terms of magnitude 1 + |logvar| +
    mu^2 + exp(logvar), k = 5 (mu^2, three sums, the final scaling), + expf.  The sum: the two bounds added, two
    more roundings.  Returns ((total, mse, kld) Refs of shape (1,), drecon, dmu, dlv)."""
    bt = f32(beta)
    r, t, m_, l_ = d(recon).flatten(), d(x).flatten(), d(mu).flatten(), d(logvar).flatten()
    nx, nz = r.numel(), m_.numel()
    df = r - t
    ma = r.abs() + t.abs()
    mse = mk((df * df).mean().reshape(1), (ma * ma).mean().reshape(1), nx, 4)
    ex = torch.exp(l_)
    term = 1 + l_ - m_ * m_ - ex
    tm = 1 + l_.abs() + m_ * m_ + ex
    kld = mk((-0.5 * term.mean()).reshape(1), (0.5 * tm.mean()).reshape(1), nz, 5, (0.5 * TRANS * U * ex.mean()).reshape(1))
    tot = mk(mse.val + bt * kld.val, mse.val.abs() + abs(bt) * kld.val.abs(), 0, 2, mse.bound() + abs(bt) * kld.bound())
    drecon = mk((2.0 / nx * df).reshape(recon.shape), (2.0 / nx * ma).reshape(recon.shape), 0, 3)
    dmu = mk((bt * m_ / nz).reshape(mu.shape), (abs(bt) * m_.abs() / nz).reshape(mu.shape), 0, 2)
    dlv = mk((bt * -0.5 * (1 - ex) / nz).reshape(mu.shape), (abs(bt) * 0.5 * (1 + ex) / nz).reshape(mu.shape), 0, 4,
             (abs(bt) * 0.5 * TRANS * U * ex / nz).reshape(mu.shape))
    return (tot, mse, kld), drecon, dmu, dlv
