"""fp64 references, per-element bounds and shape tables of the three pieces of the training path that the earlier contract
files left to norm-wise checks: the row chain's non-Linear ops (csrc/row_chain.hip: MEAN_T, LAYERNORM, SOFTMAX_CE, DHEAD,
LOAD / COPY / STORE), the fused MLP step (csrc/mlp_train.hip: mlp_rows_kernel, mlp_params_kernel) and spectral normalisation
(spectral_norm_fwd_kernel / spectral_norm_bwd_kernel of csrc/small_kernels.hip).  A plain helper module beside support_ref /
window_ref, whose Ref / mk / check / worst / Guarded and references it uses wherever they already state the operation;
nothing here is collected.  tests/test_rowstep_ref.py is the host self-test, tests/test_rowstep_contract_gpu.py the GPU file.

The bound is the project's, |got - ref| <= (n + 4 + k) U M + eps_abs, U = 2^-24, M the same expression on absolute values, n
the terms of the element's fp32 sum, k the other roundings on its path.  No extra budget for a split of a sum: the chain's
wave / LDS-partial splits, the MFMA's four-product step, `acc0 + acc1` of the two MFMA chains, block_sum.

Row chain
  MEAN_T        support_ref.meanT_fwd (n = T, k = 1) for both paths.
  LAYERNORM     support_ref.layernorm_fwd.  The chain's arithmetic is a sequential fp32 sum of D terms per thread, a division,
                the variance as the sequential sum of (x - fp32 mean)^2, a division, 1.f / sqrtf(var + eps), one product for
                xhat and a product and a sum for y.  That is the two-pass computation whose roundings layernorm_fwd counts
                (it carries the error of the fp32 mean into the centred values and from there into the variance), so the
                count covers it unchanged; the self-test's sequential fp32 emulation confirms it at D = 64.
  SOFTMAX_CE    ce_rows below: support_ref.softmax_ce's per-row terms without its mean over the batch (the chain stores the
                row losses and scales the gradient by `coef`, launch A of the MLP step divides by `rows` instead).
  DHEAD         support_ref.dhead_fwd (n = F + E, k = 1) and dhead_bwd (dU: k = 3; demb: one term, k = 1).
  LOAD / COPY / STORE   exact.
  LIN_FWD / LIN_DGRAD in the composed chain: window_ref.linear / linear_dgrad with stride2_ref's epilogue, as in
                tests/test_window_contract_gpu.py, each stage from the kernel's own stored input.

MLP step: every stage is referenced from the kernel's own stored upstream tensors, so each bound is a one-stage count
(mlp_stages).  GELU / GELU' carry the absolute 4.2e-7 / 3.2e-7 of the A-S forms (support_ref.act_on / grad_factor).

Spectral norm: sn_fwd / sn_bwd.  A normalised vector y = x / max(|x|, eps) computed from a raw fp32 product x with per-element
bound e: the computed norm differs from |x| by at most |e| (triangle inequality) plus its own roundings -- the sum of `len`
squares ((len + 1) U relative, halved by the root), the root, the reciprocal, the product: below (len + 4 + 3) U relative --
so |got_i - y_i| <= e_i / |x| + |x_i| / |x| (|e| / |x| + (len + 4 + 3) U)."""
import torch
import torch.nn.functional as F

import support_ref as S
import window_ref as W
from support_ref import U, mk, d, f32, TRANS, TINY, ACT_GELU

Ref, check, worst, Guarded = S.Ref, S.check, S.worst, S.Guarded

CH_THREADS, CH_MAXV = 1024, 512
MLP_ROWS, MLP_WAVES, UPD_WAVES, MLP_MAX_HIDDEN = 16, 8, 4, 4
MAX_SN_JOBS = 8

# ---------------------------------------------------------------------------------------------------------------------
# tables (plain data; shared by the host self-test and the GPU file)
# ---------------------------------------------------------------------------------------------------------------------
CHAIN_ROWS = (1, 3)
# (T, C, off): off = floats by which the base view is shifted off a 16-byte boundary
MEANT_VEC = [(1, 16, 0), (37, 100, 0), (33, 128, 0), (130, 512, 0)]
MEANT_SCALAR = [(5, 6, 0), (7, 18, 0), (9, 16, 1)]
LN_D = (1, 6, 63, 64)
LN_KINDS = ("randn", "const", "offset", "small")      # small: 0.01 randn, where eps is a tenth of the variance
CE_C = (1, 2, 4, 32)
CE_KINDS = ("randn", "big")
CE_BAD = (-1, None, 1 << 40)            # None: the class count itself
# (F, E, emb rows: 0 = none, 2 = fewer than the chain's rows (taken modulo), -1 = one per row)
DHEAD = [(1, 0, 0), (100, 3, 2), (256, 128, -1), (512, 128, 2), (100, 0, 0), (512, 3, -1)]
# (in_dim, hidden widths, classes)
MLP_SHAPES = {"one": (1, [1], 2), "edge16": (16, [130], 17), "two32": (32, [512], 32), "deep": (33, [48, 33, 16, 130], 2),
              "k48": (48, [32], 17), "wide": (512, [16], 32)}
MLP_ROWS_ALL = (1, 7, 8, 9, 15, 16, 17, 33, 100)
# every shape at three row counts, the small one at all of them; each case runs aligned and at odd offsets
MLP_CASES = ([("edge16", r) for r in MLP_ROWS_ALL] + [("one", 1), ("one", 17), ("two32", 9), ("two32", 33), ("deep", 7), ("deep", 15),
             ("deep", 100), ("k48", 8), ("k48", 16), ("wide", 1), ("wide", 17), ("wide", 100)])
SN_SHAPES = [(1, 1), (7, 3), (17, 65), (3, 1029), (1030, 5), (256, 768)]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def meant_input(rows, T, C, seed=0):
    return torch.randn(rows, T, C, generator=gen(100 + seed)) + 0.25


def ln_input(rows, D, kind, seed=0):
    g = gen(200 + seed)
    x = torch.randn(rows, D, generator=g)
    if kind == "const":
        x = torch.full((rows, D), 1.75) * torch.arange(1, rows + 1)[:, None]
    elif kind == "offset":
        x = 100.0 + 0.01 * x
    elif kind == "small":
        x = 0.01 * x
    return x, torch.randn(D, generator=g).abs() + 0.5, torch.randn(D, generator=g)


def ce_input(rows, C, kind, seed=0):
    g = gen(300 + seed)
    z = torch.randn(rows, C, generator=g)
    if kind == "big":
        z = torch.where(torch.rand(rows, C, generator=g) > 0.5, 80.0, -80.0) + 0.01 * z
    return z, torch.randint(0, C, (rows,), generator=g)


def dhead_input(rows, Fd, E, Be, seed=0):
    g = gen(400 + seed)
    f = torch.randn(rows, Fd, generator=g)
    f[:, ::3] = 0.0                       # exact zeros take the 0.2 side of `f > 0`
    Be = rows if Be < 0 else Be
    emb = torch.randn(Be, E, generator=g) if E else None
    return f, emb, torch.randn(Fd + E, generator=g), torch.randn(1, generator=g), torch.randn(rows, generator=g)


def mlp_problem(name, rows, seed=0):
    """Host tensors of an MLP case: weights, biases, x, y, masks."""
    in_dim, hidden, C = MLP_SHAPES[name]
    g = gen(1000 * rows + seed + sum(hidden))
    dims = [in_dim] + hidden + [C]
    ws = [torch.randn(o, i, generator=g) * (1.5 / i ** 0.5) for i, o in zip(dims, dims[1:])]
    bs = [torch.randn(o, generator=g) * 0.1 for o in dims[1:]]
    x = torch.randn(rows, in_dim, generator=g)
    y = torch.randint(0, C, (rows,), generator=g)
    masks = [(torch.rand(rows, h, generator=g) >= 0.2).float() / 0.8 for h in hidden]
    return dict(ws=ws, bs=bs, x=x, y=y, masks=masks, hidden=hidden, C=C, in_dim=in_dim, rows=rows)


def flat_layout(ws, bs, aligned):
    """Element offsets of w0, b0, w1, b1, ... in one flat buffer: every tensor on a multiple of four floats (aligned) or on
    an odd element.  Returns (w_off, b_off, n_flat)."""
    offs, o = [], 4 if aligned else 3
    for t in [t for pair in zip(ws, bs) for t in pair]:
        offs.append(o)
        o += t.numel() + 1
        o = (o + 3) // 4 * 4 if aligned else o + (1 - o % 2)
    return offs[0::2], offs[1::2], o + 2


def sn_input(R, C, seed=0):
    g = gen(500 + 7 * R + C + seed)
    w = torch.randn(R, C, generator=g) * 0.3
    return (w, F.normalize(torch.randn(R, generator=g), dim=0), F.normalize(torch.randn(C, generator=g), dim=0),
            torch.randn(R, C, generator=g))


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' predicates, restated for the self-test and for the GPU file's assertions
# ---------------------------------------------------------------------------------------------------------------------
def meant_plan(T, C, off=0, ld=None):
    ld = C if ld is None else ld
    vec = C % 4 == 0 and C >= 16 and ld % 4 == 0 and off % 4 == 0
    if not vec:
        return dict(vec=False)
    L4 = C // 4
    RL = CH_THREADS // L4
    return dict(vec=True, L4=L4, RL=RL, live=RL * L4, outer=-(-T // (16 * RL)), in_flight=min(16, -(-T // RL)),
                clamped=T % (16 * RL) != 0)


def dgrad_branch(IN):
    return "vec" if IN % 4 == 0 and IN >= 16 else ("rows" if IN <= 64 else "scalar")


def mlp_plan(in_dim, hidden, C, rows, w_off, b_off):
    """Launch A: per layer (in, out, vec, kpad, two-chunk trips, single-chunk trips, tiles, rounds over the 8 waves).
    Launch B: tiles_i, tile_end, blocks, and the (layer, to, ti) of every tile."""
    dims = [in_dim] + list(hidden) + [C]
    layers, tiles, tmap = [], 0, []
    for l, (i, o) in enumerate(zip(dims, dims[1:])):
        kpad = (i + 15) // 16 * 16
        trips = [k0 + 16 < kpad for k0 in range(0, kpad, 32)]
        nt = (o + 15) // 16
        ti_n = (i + 15) // 16
        layers.append(dict(l=l, inn=i, out=o, vec=i % 4 == 0 and w_off[l] % 4 == 0, kpad=kpad, two=sum(trips), single=len(trips) - sum(trips),
                           tiles=nt, rounds=-(-nt // MLP_WAVES), tiles_i=ti_n))
        for to in range(nt):
            for ti in range(ti_n):
                tmap.append((l, to, ti))
        tiles += nt * ti_n
        layers[-1]["tile_end"] = tiles
    return dict(layers=layers, tiles=tiles, blocks=-(-tiles // UPD_WAVES), tile_map=tmap, row_blocks=-(-rows // MLP_ROWS),
                b_trips=-(-rows // 8))


# ---------------------------------------------------------------------------------------------------------------------
# row chain
# ---------------------------------------------------------------------------------------------------------------------
meanT = S.meanT_fwd
layernorm = S.layernorm_fwd          # Refs (y, xhat)


def ce_rows(logits, target, coef=1.0, div=1.0):
    """Per row: loss_r = logsumexp(z_r) - z_r[y_r]; g_r = coef (softmax(z_r) - onehot(y_r)) / div.  A target outside [0, C)
    makes its row NaN.  support_ref.softmax_ce's terms per row: t_j = z_j - max rounds, expf, a C-term sum, logf, max + log
    rounds, the row loss rounds once more (k = 1 on |lse| + |z_y|).  Gradient: the exponent z_j - lse carries the error of lse
    and its own rounding, expf, then the subtraction and one rounding per scaling that is not 1."""
    cf, dv = f32(coef), float(div)
    z = d(logits)
    B, Cn = z.shape
    y = target.to(z.device)
    bad = (y < 0) | (y >= Cn)
    ys = torch.where(bad, torch.zeros_like(y), y)
    mx = z.max(1, keepdim=True).values
    se = torch.exp(z - mx).sum(1, keepdim=True)
    lse = mx + se.log()
    rel_se = U * (z.abs() + mx.abs()).max(1, keepdim=True).values + (TRANS + Cn + 4) * U
    e_lse = rel_se + TRANS * U * se.log().abs() + U * (mx.abs() + se.log().abs())
    zy = z.gather(1, ys[:, None])
    nan = float("nan")
    row = torch.where(bad[:, None], torch.full_like(lse, nan), lse - zy)
    loss = mk(row[:, 0], (lse.abs() + zy.abs())[:, 0], 0, 1, e_lse[:, 0])
    p = torch.exp(z - lse)
    oh = F.one_hot(ys, Cn).double()
    e_p = p * (e_lse + U * (z.abs() + lse.abs()) + TRANS * U)
    sc = abs(cf) / dv
    g = torch.where(bad[:, None], torch.full_like(p, nan), cf * (p - oh) / dv)
    return loss, mk(g, sc * (p + oh), 0, 1 + (cf != 1.0) + (dv != 1.0), sc * (e_p + TINY) + TINY), bad


def dhead(f, emb, w, bias, ds, with_demb):
    """Refs (s, dU, demb or None) of the chain's DHEAD op (one embedding row per sample for demb)."""
    rows, Fd = f.shape
    E = emb.shape[1] if emb is not None else 0
    s = S.dhead_fwd(f, emb, w, bias)
    out = S.dhead_bwd(ds, f, w, Be=rows, E=E if with_demb else 0, nb_emb=rows)
    return s, out[0], (out[1] if with_demb else None)


def lin_fwd(x, w, b, act, mask):
    """LIN_FWD of the chain: Ref of the output with .z the pre-activation (tests/test_window_contract_gpu.py, section f)."""
    return W.Ref(*W.linear(x, w), w.shape[1]).epilogue(bias=b, zout=True, act=act, emul=mask)


# ---------------------------------------------------------------------------------------------------------------------
# MLP step
# ---------------------------------------------------------------------------------------------------------------------
def _gelu_masked(z, mask):
    r = S.act_on(mk(d(z), d(z).abs(), 0, 0), ACT_GELU)
    return r.epilogue(emul=mask) if mask is not None else r


def _dz(dn, wn, z, mask):
    """(dn @ wn) GELU'(z) mask: n = out products, the factor's own error on |dn @ wn|, two products."""
    v, m = W.linear_dgrad(dn, wn)
    fac, fe = S.grad_factor(ACT_GELU, d(z))
    mq = d(mask)
    return mk(v * fac * mq, m * fac.abs() * mq.abs(), wn.shape[0], 2, v.abs() * fe * mq.abs())


def mlp_stages(ws, bs, x, y, masks, st, train=True):
    """One-stage references of launch A from the kernel's own stored tensors st = dict(z, a, dz: lists; logits, loss_rows,
    dlogits).  Returns a dict name -> Ref.  z[l]: n = in, k = 1 (the bias).  a[l]: GELU and the mask product from the stored
    z[l].  logits: from the stored a[L - 1].  loss_rows / dlogits: ce_rows of the stored logits, divided by rows.  dz[l]: from the
    stored dz[l + 1] (dlogits for the last hidden layer), z[l] and the mask, n = out of layer l + 1.  Eval mode (train False):
    no masks, no backward; a[l] is not stored, so z[l] of the next layer cannot be staged and only the chain's end is compared
    (mlp_eval)."""
    L = len(ws) - 1
    rows = x.shape[0]
    out = {}
    prev = x
    for l in range(L):
        out[f"z{l}"] = W.Ref(*W.linear(prev, ws[l]), ws[l].shape[1]).epilogue(bias=bs[l])
        out[f"a{l}"] = _gelu_masked(st["z"][l], masks[l])
        prev = st["a"][l]
    out["logits"] = W.Ref(*W.linear(prev, ws[L]), ws[L].shape[1]).epilogue(bias=bs[L])
    out["loss_rows"], dl, _ = ce_rows(st["logits"], y, 1.0, rows if train else 1.0)
    if train:
        out["dlogits"] = dl
        dn = st["dlogits"]
        for l in range(L - 1, -1, -1):
            out[f"dz{l}"] = _dz(dn, ws[l + 1], st["z"][l], masks[l])
            dn = st["dz"][l]
    return out


def mlp_eval(ws, bs, x):
    """Eval-mode logits through the whole stack (no stored intermediates to stage from): per layer the bound of the layer's
    own roundings plus the previous layer's bound carried through |W| and |GELU'| <= GELU_DMAX.  Ref of the logits."""
    v = d(x)
    e = torch.zeros_like(v)
    for l, (w, b) in enumerate(zip(ws, bs)):
        r = W.Ref(*W.linear(v, w), w.shape[1]).epilogue(bias=b)
        e = e @ d(w).abs().t() + r.bound()
        v = r.val
        if l < len(ws) - 1:
            g = S.act_on(mk(v, v.abs(), 0, 0), ACT_GELU)
            v, e = g.val, S.GELU_DMAX * e + g.bound()
    return mk(v, torch.zeros_like(v), 0, 0, e)


def mlp_params(ws, x, st):
    """Launch B's gradients from the stored dz / a / dlogits / loss_rows: dW[l][o, i] = sum_r dz[l][r, o] a[l - 1][r, i], db[l][o]
    = sum_r dz[l][r, o] (both n = rows; the bias MFMA's products by 1.f are exact), loss = mean(loss_rows) (n = rows, k = 1)."""
    L = len(ws) - 1
    rows = x.shape[0]
    out = {}
    for l in range(L + 1):
        ap = x if l == 0 else st["a"][l - 1]
        dz = st["dlogits"] if l == L else st["dz"][l]
        (dw, mw, n), (db, mb, nb) = W.wgrad_s1(ap[:, None, :], dz[:, None, :], 1)
        out[f"dW{l}"] = W.Ref(dw[:, :, 0], mw[:, :, 0], n)
        out[f"db{l}"] = W.Ref(db, mb, nb)
    lr = d(st["loss_rows"])
    out["loss"] = mk(lr.mean().reshape(1), lr.abs().mean().reshape(1), rows, 1)
    return out


def argmax_nan_first(logits):
    """mlp_params_kernel's argmax (ed_metrics_acc's): the first maximum; a NaN beats every number and the first NaN stays."""
    z = logits.detach().cpu().double()
    key = torch.where(torch.isnan(z), torch.full_like(z, float("inf")), torch.where(torch.isinf(z) & (z > 0), torch.full_like(z, 1e308), z))
    return torch.argmax((key == key.max(1, keepdim=True).values).to(torch.uint8), dim=1)


# ---------------------------------------------------------------------------------------------------------------------
# spectral norm
# ---------------------------------------------------------------------------------------------------------------------
def _normalised(x, e, eps):
    """Ref of x / max(|x|, eps) for a raw product x (fp64) with per-element bound e (module docstring)."""
    ln = x.numel()
    nrm = max(float(x.norm()), eps)
    y = x / nrm
    err = e / nrm + y.abs() * (float(e.norm()) / nrm + (ln + 4 + 3) * U)
    return mk(y, torch.zeros_like(y), 0, 0, err)


def sn_fwd(w, u0, v0, st, power_iter=True, eps=1e-12):
    """Stage-wise references of spectral_norm_fwd_kernel; w (R, C).  v is overwritten in place, so v is referenced from the
    inputs (u0); u from the STORED v; sigma from the stored u, v: sum_i u_i sum_j W_ij v_j -- a product passes through at
    most C - 1 additions in its row, the product with u_i and R - 1 additions across rows: n = R + C, k = 1; w_eff from the
    stored sigma (one division).  st = dict(u, v, sigma) as the kernel left them.  Returns dict of Refs."""
    eps = f32(eps)
    Wd = d(w)
    R, Cc = Wd.shape
    out = {}
    if power_iter:
        x, m = Wd.t() @ d(u0), Wd.abs().t() @ d(u0).abs()
        out["v"] = _normalised(x, (R + 4) * U * m, eps)
        x, m = Wd @ d(st["v"]), Wd.abs() @ d(st["v"]).abs()
        out["u"] = _normalised(x, (Cc + 4) * U * m, eps)
    us, vs = d(st["u"]), d(st["v"])
    out["sigma"] = mk((us @ (Wd @ vs)).reshape(1), (us.abs() @ (Wd.abs() @ vs.abs())).reshape(1), R + Cc, 1)
    sg = d(st["sigma"]).reshape(())
    out["w_eff"] = mk(Wd / sg, (Wd / sg).abs(), 0, 1)
    return out


def sn_bwd(dw, st):
    """spectral_norm_bwd_kernel from the stored w_eff, u, v, sigma: d = <dw, w_eff> (n = R C), out = (dw - d u_i v_j) / sigma:
    1 / sigma, two products, the subtraction and the last product round (k = 5); d's bound carried through |u_i v_j / sigma|."""
    D, We = d(dw), d(st["w_eff"])
    dd, md = (D * We).sum(), (D * We).abs().sum()
    e_d = (D.numel() + 4) * U * md
    uv = d(st["u"])[:, None] * d(st["v"])[None, :]
    sg = d(st["sigma"]).reshape(())
    return mk((D - dd * uv) / sg, (D.abs() + dd.abs() * uv.abs()) / sg.abs(), 0, 5, e_d * uv.abs() / sg.abs())
