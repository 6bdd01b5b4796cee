"""Stage tables of the engines' training steps: every launch (or pair of launches summing into one tensor) of a flow as a
row -- output tensor(s), input tensors, the fp64 operation with its epilogue and its rounding count -- so that a step can be
held to fp64 LAUNCH BY LAUNCH: every stage is referenced from the stored upstream tensors, the bound is the one-stage count
of the kernel that carries it, and nothing compounds.  A plain helper module beside stride2_ref / window_ref / support_ref,
whose (value, M) pairs and Refs it strings together; it defines no convolution, BatchNorm, loss or optimiser reference of
its own.  Nothing here is collected.

The rows are written from the model (oracle/melo_oracle.py: vae_fwd, vae_loss, ae_step, feature_encoder_fwd, generator_fwd,
discriminator_fwd, gradient_penalty, d_step, g_step; the reference's src/ae/model.py, src/ae/train_ae.py:110-122,
src/gan/models.py, src/gan/train_gan.py:183-251), never from an engine: tests/test_engine_ref.py evaluates each table in fp64 from the batch,
the parameters and the injected randoms alone and compares it with the oracle's autograd, which is what makes the tables
independent of melo_gan_amd/ae/engine.py and melo_gan_amd/gan/engine.py.  Tensor names are the engines' attribute names, so that a GPU test can snapshot
them (tests/test_engine_contract_gpu.py).

Tables: the VAE's forward(True), backward(beta) and update() (vae_tables); of the GAN the numeric encoder's and the generator's
forward for one group of B rows (either half of the split flow) and for two (the fused flow's 2B-row pass)
(gen_forward_table), the critic step behind it (critic_table), the two optimiser updates with the re-laid weight copies
(gan_update_table; with the EMA shadow where averaging is on), the frozen emotion discriminator's fold and branch, fp32 and
bf16 storage (ed_fold_table, ed_branch_table), and the generator step from g_critic_front to the end of g_backward_b
(gen_backward_table).  Not tabulated: spectral norm inside an engine (neither engine has a configuration that enables it).

A row is a Stage:
  outs   names written.  "b.<name>" a BatchNorm buffer, "g.<name>" a parameter's gradient, "P.data" / "P.grad" / "P.m" /
         "P.v" / "P.state" the flat optimiser buffers, "a@b" the tensor `a` as captured before the call that overwrites it
         (b says which), anything else an engine attribute (a trailing digit indexes a list: "ez1" is eng.ez[1]).
  ins    names read: "p.<name>" a parameter, "pre:<name>" the value BEFORE the sub-step (running statistics, optimiser
         state), anything else the value after it -- the stage's own stored upstream.
  ref    fp64 function of the inputs (and the hyper-parameters) returning one Ref per output.
  host   the same operation written with torch in the dtype of its inputs: the fp32 host evaluation (and, in fp64, a second
         formulation through torch.nn.functional the Refs are compared with).

Bounds: a matrix stage is (n + 4 + k) U M with n the products of the element's sum (stride2_ref / window_ref); a stage that
sums two launches into one tensor (g_h) has n = n1 + n2 on M = M1 + M2 and one rounding more for the accumulate; a rider
(a bias gradient, the loss) has the bound of the kernel that carries it; the rest are support_ref's."""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

import stride2_ref as S2
import support_ref as S
import window_ref as W
from support_ref import ACT_NONE, ACT_RELU, ACT_TANH, Ref, U, U64, f32, mk

BN_EPS, BN_MOM = 1e-5, 0.1


# ---------------------------------------------------------------------------------------------------------------------
# the frame
# ---------------------------------------------------------------------------------------------------------------------
class Stage:
    def __init__(self, section, outs, ins, ref, host):
        self.section, self.outs, self.ins, self.ref, self.host = section, tuple(outs), tuple(ins), ref, host

    @property
    def name(self):
        return "+".join(self.outs)


def from_bounds(val, bound):
    """A Ref whose bound is `bound` itself (concatenations of Refs with different counts; exact stages: bound 0)."""
    r = Ref(val, torch.zeros_like(val), 0)
    r.k_epi = -4
    r.eps_abs = bound + torch.zeros_like(val)
    return r


def exact(val):
    return from_bounds(val.double(), torch.zeros_like(val, dtype=torch.float64))


def cat_refs(refs, dim=0):
    return from_bounds(torch.cat([r.val for r in refs], dim), torch.cat([r.bound() for r in refs], dim))


def fetch(name, pre, post):
    return pre[name[4:]] if name.startswith("pre:") else post[name]


def evaluate(table, pre, hp, dtype=torch.float64, mutate=None, carry="host", mags=None):
    """Run a table from `pre` (name -> tensor: the state before the sub-step plus its inputs); returns (post, ratios): post
    the state after it, ratios[output name] = the worst error / bound of stage.host's result in `dtype` against the stage's
    Ref taken from the SAME upstream tensors (the fp32 host evaluation's figure; in fp64 the agreement of the two
    formulations).  carry: what a stage hands to the next, "host" (its host result, rounded to `dtype`: what a device
    stores) or "ref" (the Ref's fp64 value: the table itself, evaluated exactly).  mutate: {stage name: host function}
    replaces a stage's host function (a wiring mistake).  mags: a dict that receives every output's largest stage magnitude
    M (at least its largest value): what a cancelling result is small against."""
    pre = {k: (v.to(dtype) if v.is_floating_point() and k != "P.state" and v.dtype != torch.bfloat16 else v) for k, v in pre.items()}
    post = dict(pre)
    ratios = OrderedDict()
    for st in table:
        ins = [fetch(n, pre, post) for n in st.ins]
        got = (mutate or {}).get(st.name, st.host)(hp, *ins)
        refs = st.ref(hp, *ins)
        assert len(got) == len(refs) == len(st.outs), st.name
        for n, g, r in zip(st.outs, got, refs):
            assert tuple(g.shape) == tuple(r.val.shape), (n, tuple(g.shape), tuple(r.val.shape))
            ratios[n] = S.worst(g, r)[0]
            if mags is not None and r.val.numel():
                mags[n] = max(float(r.mag.abs().max()), float(r.val.abs().max()))
            post[n] = g.contiguous() if carry == "host" else r.val
    return post, ratios


def judge(table, pre, post, hp, only=None):
    """Hold `post` (snapshots of a device, or anything else) to the table: {output name: worst error / bound}, every stage
    referenced from post's / pre's own upstream tensors."""
    out = OrderedDict()
    for st in table:
        if only is not None and st.name not in only:
            continue
        refs = st.ref(hp, *[fetch(n, pre, post) for n in st.ins])
        for n, r in zip(st.outs, refs):
            got = post[n]
            assert tuple(got.shape) == tuple(r.val.shape), (n, tuple(got.shape), tuple(r.val.shape))
            if st.section == "re-layout":       # exact, and a NaN upstream (a prefill nobody overwrote) is this stage's input
                same = (got.double() == r.val) | (torch.isnan(got) & torch.isnan(r.val))
                out[n] = 0.0 if bool(same.all()) else float("inf")
            else:
                out[n] = S.worst(got, r)[0]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# operations: (ref, host) pairs
# ---------------------------------------------------------------------------------------------------------------------
def _ncl(x):
    return x.permute(0, 2, 1)


def _vjp(fn, args, wrt, dy):
    a = [t.detach().clone().requires_grad_(i in wrt) for i, t in enumerate(args)]
    return torch.autograd.grad(fn(*a), [a[i] for i in wrt], dy)


def _act(act, v):
    return S2.act_ref(act, v)


def conv_s2(act=ACT_NONE):
    """Conv1d(k5, s2, p2) + bias, channels-last."""
    def ref(hp, x, w, b):
        v, m = S2.gather(x, w)
        return (Ref(v, m, 5 * x.shape[2]).epilogue(bias=b, act=act),)

    def host(hp, x, w, b):
        return (_act(act, _ncl(F.conv1d(_ncl(x), w, b, 2, 2))),)
    return ref, host


def convT_s2(act=ACT_NONE, T=None):
    """ConvTranspose1d(k5, s2, p2, op1) + bias; T: rows of the output buffer, those past 2 Tin zero (model.py's padding to
    max_notes: the activation is not applied to them)."""
    def ref(hp, x, w, b):
        Tout = 2 * x.shape[1]
        v, m = S2.scatter(x, w, Tout)
        r = Ref(v, m, 5 * x.shape[2]).epilogue(bias=b, act=act)
        if T is not None and T != Tout:
            z = torch.zeros(v.shape[0], T - Tout, v.shape[2], dtype=torch.float64, device=v.device)
            r = cat_refs([r, exact(z)], 1)
        return (r,)

    def host(hp, x, w, b):
        y = _act(act, _ncl(F.conv_transpose1d(_ncl(x), w, b, 2, 2, 1)))
        if T is not None and T != y.shape[1]:
            y = torch.cat([y, y.new_zeros(y.shape[0], T - y.shape[1], y.shape[2])], 1)
        return (y,)
    return ref, host


def bn_train(act=ACT_RELU):
    """Training BatchNorm over all rows + activation: save_mean, save_invstd, a, and the moved running statistics."""
    def ref(hp, z, gamma, beta, rm0, rv0):
        st = S.bn_stats(z, 1, BN_EPS)
        a = S.bn_apply(z, st["mean"], st["invstd"], gamma, beta, act)
        rm, rv = S.bn_running(st, rm0, rv0, BN_MOM)
        sm, si = st["save_mean"], st["save_invstd"]
        return (from_bounds(sm.val[0], sm.bound()[0]), from_bounds(si.val[0], si.bound()[0]), a, rm, rv)

    def host(hp, z, gamma, beta, rm0, rv0, moves=1):
        x = S.rows(z)
        R = x.shape[0]
        # the statistics in fp64 rounded once, as the kernels are held to (support_ref: "fp64-accumulated reductions")
        mean = x.double().mean(0)
        var = ((x.double() - mean) ** 2).mean(0)
        istd = ((var + f32(BN_EPS)) ** -0.5).to(z.dtype)
        unb = (var * R / (R - 1)).to(z.dtype)
        mean = mean.to(z.dtype)
        a = _act(act, (z - mean) * istd * gamma + beta)
        mom = f32(BN_MOM)
        rm, rv = rm0, rv0
        for _ in range(moves):
            rm, rv = (1.0 - mom) * rm + mom * mean, (1.0 - mom) * rv + mom * unb
        return (mean, istd, a, rm, rv)
    return ref, host


def bn_back(act=ACT_RELU):
    """BatchNorm backward behind the activation from the saved statistics: dz, dgamma, dbeta."""
    def ref(hp, da, a, z, gamma, beta, sm, si):
        return S.bn_bwd(da, a, z, gamma, beta, sm, si, act)

    def host(hp, da, a, z, gamma, beta, sm, si):
        R = S.rows(z).shape[0]
        dy = da * S2.act_grad_ref(act, a)
        xh = (z - sm) * si
        s1, s2 = S.rows(dy).sum(0), S.rows(dy * xh).sum(0)
        return (gamma * si * (dy - s1 / R - xh * s2 / R), s2, s1)
    return ref, host


SLOPE = f32(0.2)        # LeakyReLU's negative slope as the kernels hold it (0.2f), forward and backward (stride2_ref.act_grad_ref)


def lrelu_on(r):
    """LeakyReLU with the fp32 slope on a Ref: one rounding (stride2_ref's epilogue step with 0.2f for 0.2)."""
    r.val = torch.where(r.val > 0, r.val, SLOPE * r.val)
    r.k_epi += 1
    return r


def _lrelu(v):
    return torch.where(v > 0, v, SLOPE * v)


def linear(act=ACT_NONE):
    def ref(hp, x, w, b):
        v, m = W.linear(x, w)
        r = Ref(v, m, x.shape[1])
        return (lrelu_on(r.epilogue(bias=b)) if act == S.ACT_LRELU else r.epilogue(bias=b, act=act),)

    def host(hp, x, w, b):
        return (_lrelu(F.linear(x, w, b)) if act == S.ACT_LRELU else _act(act, F.linear(x, w, b)),)
    return ref, host


def linear_dgrad(gact=ACT_NONE):
    """dx = dy @ w (* act'(gref))."""
    def ref(hp, dy, w, *gref):
        v, m = W.linear_dgrad(dy, w)
        r = Ref(v, m, dy.shape[1])
        return (r.epilogue(gref=gref[0], gact=gact) if gref else r,)

    def host(hp, dy, w, *gref):
        v = dy @ w
        return (v * S2.act_grad_ref(gact, gref[0]) if gref else v,)
    return ref, host


def linear_dgrad_sum2():
    """One tensor summed from two Linear data gradients (the second launch accumulates onto the first): n = n1 + n2 products
    on M = M1 + M2, k = 1 for the accumulate's addition."""
    def ref(hp, dy1, w1, dy2, w2):
        (v1, m1), (v2, m2) = W.linear_dgrad(dy1, w1), W.linear_dgrad(dy2, w2)
        return (mk(v1 + v2, m1 + m2, dy1.shape[1] + dy2.shape[1], 1),)

    def host(hp, dy1, w1, dy2, w2):
        return (dy1 @ w1 + dy2 @ w2,)
    return ref, host


def act_back(gact):
    def ref(hp, dy, gref):
        return (S.act_bwd(dy, gref, gact),)

    def host(hp, dy, gref):
        return (dy * S2.act_grad_ref(gact, gref),)
    return ref, host


def linear_wgrad():
    """dw = dy^T x and its bias rider db = column sums of dy."""
    def ref(hp, x, dy):
        B = x.shape[0]
        (dw, mw, n), (db, mb, nb) = W.wgrad_s1(x.reshape(B, 1, -1), dy.reshape(B, 1, -1), 1)
        return (Ref(dw[:, :, 0], mw[:, :, 0], n), Ref(db, mb, nb))

    def host(hp, x, dy):
        return (dy.t() @ x, dy.sum(0))
    return ref, host


def conv_s2_wgrad():
    def ref(hp, x, dy):
        (dw, mw, n), (db, mb, nb) = S2.conv_wgrad(x, dy)
        return (Ref(dw, mw, n), Ref(db, mb, nb))

    def host(hp, x, dy):
        w0 = x.new_zeros(dy.shape[2], x.shape[2], 5)
        (dw,) = _vjp(lambda w: _ncl(F.conv1d(_ncl(x), w, None, 2, 2)), [w0], [0], dy)
        return (dw, dy.sum((0, 1)))
    return ref, host


def convT_s2_wgrad():
    def ref(hp, x, dy):
        (dw, mw, n), (db, mb, nb) = S2.convT_wgrad(x, dy)
        return (Ref(dw, mw, n), Ref(db, mb, nb))

    def host(hp, x, dy):
        w0 = x.new_zeros(x.shape[2], dy.shape[2], 5)
        (dw,) = _vjp(lambda w: _ncl(F.conv_transpose1d(_ncl(x), w, None, 2, 2, 1)), [w0], [0], dy)
        return (dw, dy.sum((0, 1)))
    return ref, host


def conv_s2_dgrad():
    """Data gradient of Conv1d(k5, s2, p2): dx has the input's length (even or odd), taken from hp-free shape rule
    Tin = the stored upstream activation's length, passed as the third input (read for its shape only)."""
    def ref(hp, dy, w, like):
        v, m = S2.scatter(dy, w, like.shape[1])
        return (Ref(v, m, 5 * dy.shape[2]),)

    def host(hp, dy, w, like):
        x0 = dy.new_zeros(like.shape)
        return (_vjp(lambda x: _ncl(F.conv1d(_ncl(x), w, None, 2, 2)), [x0], [0], dy)[0],)
    return ref, host


def convT_s2_dgrad():
    def ref(hp, dy, w):
        v, m = S2.gather(dy, w)
        return (Ref(v, m, 5 * dy.shape[2]),)

    def host(hp, dy, w):
        x0 = dy.new_zeros(dy.shape[0], dy.shape[1] // 2, w.shape[0])
        return (_vjp(lambda x: _ncl(F.conv_transpose1d(_ncl(x), w, None, 2, 2, 1)), [x0], [0], dy)[0],)
    return ref, host


def relayout(fn):
    """A pure re-layout: compared exactly."""
    def ref(hp, x):
        return (exact(fn(x)),)

    def host(hp, x):
        return (fn(x).contiguous(),)
    return ref, host


# ---------------------------------------------------------------------------------------------------------------------
# the VAE (oracle vae_fwd / vae_loss / ae_step; src/ae/model.py, src/ae/train_ae.py:110-122)
# ---------------------------------------------------------------------------------------------------------------------
VAE_ENC = ((0, 4, 32), (3, 32, 64), (6, 64, 128))          # (index in encoder.conv, Cin, Cout): model.py:11-19
VAE_DEC = ((0, 128, 64), (3, 64, 32), (6, 32, 4))          # (index in decoder.deconv, Cin, Cout): model.py:111-121
VAE_ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8)           # torch.optim.AdamW defaults (train_ae.py:79)
VAE_CLIP = 1.0                                              # clip_grad_norm_(1.0), train_ae.py:121

# (B, T, latent): the golden fixture's shape, and one T with T % 8 != 0 (the decoder reaches 8 (T // 8) = 16 rows, the
# rest of recon is the model's zero padding; the encoder's lengths 20 -> 10 -> 5 -> 3 make one data gradient odd)
VAE_CONFIGS = ((4, 32, 8), (4, 20, 8))


def vae_hp(B, T, latent, beta=10.0, lr=1e-4, wd=1e-5, grad_scale=1.0):
    Ts = [T]
    for _ in range(3):
        Ts.append((Ts[-1] - 1) // 2 + 1)
    red = max(1, T // 8)
    return dict(B=B, T=T, latent=latent, beta=beta, lr=lr, wd=wd, grad_scale=grad_scale, Ts=Ts, red=red,
                Ld=[red, 2 * red, 4 * red, 8 * red])


def _vae_loss_ref(hp, recon, x, mu, lv):
    (tot, mse, kld), drecon, dmu, dlv = S.vae_loss(recon, x, mu, lv, hp["beta"])
    return (cat_refs([tot, mse, kld]), drecon, dmu, dlv)


def _vae_loss_host(hp, recon, x, mu, lv):
    bt = f32(hp["beta"])
    nx, nz = recon.numel(), mu.numel()
    df = recon - x
    mse = (df * df).mean()
    ex = torch.exp(lv)
    kld = -0.5 * (1 + lv - mu * mu - ex).mean()
    return (torch.stack([mse + bt * kld, mse, kld]), 2.0 / nx * df, bt * mu / nz, bt * -0.5 * (1 - ex) / nz)


def _reparam_fwd():
    def ref(hp, mu, lv, eps):
        return (S.reparam_fwd(mu, lv, eps),)

    def host(hp, mu, lv, eps):
        return (mu + eps * torch.exp(0.5 * lv),)
    return ref, host


def _reparam_bwd(kld=True):
    def ref(hp, dz, lv, eps, k_mu, k_lv):
        return S.reparam_bwd(dz, lv, eps, k_mu, k_lv)

    def host(hp, dz, lv, eps, k_mu, k_lv):
        t = dz * eps * 0.5 * torch.exp(0.5 * lv)
        return (dz + k_mu, t + k_lv) if kld else (dz.clone(), t)
    return ref, host


def vae_grad_names(spec):
    return ["g." + k for k in spec]


def flat_of(spec, named, prefix, dtype):
    """The flat buffer (spec order, padded to a multiple of 4 with zeros: FlatParams) of named tensors."""
    v = torch.cat([named[prefix + k].reshape(-1).to(dtype) for k in spec])
    pad = (-v.numel()) % 4
    return torch.cat([v, v.new_zeros(pad)]) if pad else v


def _vae_gather_grad(spec):
    def ref(hp, *gs):
        return (exact(flat_of(spec, dict(zip(spec, gs)), "", torch.float64)),)

    def host(hp, *gs):
        return (flat_of(spec, dict(zip(spec, gs)), "", gs[0].dtype),)
    return ref, host


def _clip(n):
    def ref(hp, grad):
        return (S.grad_norm_clip(grad[:n], VAE_CLIP),)

    def host(hp, grad):
        g = grad[:n]
        nrm = (g * g).sum().sqrt()
        return (torch.stack([nrm, torch.clamp(f32(VAE_CLIP) / (nrm + f32(1e-6)), max=1.0)]),)
    return ref, host


def adam_state_ref(state, b1, b2):
    """The (4,) fp64 step state after one advance: step + 1, beta1^step, beta2^step (products in fp64: (step + 1) 2^-53
    relative), the fourth entry untouched."""
    s = state.double()
    t = float(s[0]) + 1.0
    val = torch.stack([s[0] + 1.0, s[0] * 0 + f32(b1) ** t, s[0] * 0 + f32(b2) ** t, s[3]])
    return from_bounds(val, torch.stack([val[0] * 0, (t + 1) * U64 * val[1], (t + 1) * U64 * val[2], val[3] * 0]))


def _adam(hyper, scale=1.0, advance=1, use_clip=True):
    """One flat Adam / AdamW step: p, m, v, state from the stored gradient, moments and step state (and, as a sixth input, the
    device scalars of the clip where the flow has one).  scale / advance / use_clip: the host function's mistakes (grad_scale
    wrong, the state advanced twice, the clip ignored)."""
    def ref(hp, p, g, m, v, state, *gnorm):
        if hp.get("ticked"):        # the step state was advanced by the draw in front of the sub-step: read, not written
            advanced = exact(state)
        else:
            advanced = adam_state_ref(state, hyper["beta1"], hyper["beta2"])
        step = int(advanced.val[0].item())
        rp, rm, rv = S.adam_step(p, g, m, v, step, hp["lr"], hyper["beta1"], hyper["beta2"], hyper["eps"], hp["wd"],
                                 grad_scale=hp["grad_scale"], gs_dev=gnorm[0][1:2] if gnorm else None)
        return (rp, rm, rv, advanced)

    def host(hp, p, g, m, v, state, *gnorm):
        lr, b1, b2, eps, wd = (f32(t) for t in (hp["lr"], hyper["beta1"], hyper["beta2"], hyper["eps"], hp["wd"]))
        st = state.double().clone()
        for _ in range(advance - (1 if hp.get("ticked") else 0)):
            if float(st[0]) == 0.0:
                st[1], st[2] = 1.0, 1.0
            st[0] += 1.0
            st[1] *= b1
            st[2] *= b2
        gg = g * (f32(hp["grad_scale"]) * scale) * (gnorm[0][1] if gnorm and use_clip else 1.0)
        step_size, bc2_sqrt = lr / (1.0 - float(st[1])), math.sqrt(1.0 - float(st[2]))
        if p.dtype == torch.float32:          # the two scalars a kernel forms in fp64 and rounds once
            step_size, bc2_sqrt = f32(step_size), f32(bc2_sqrt)
        pd = p * (1.0 - lr * wd)
        mn = m + (gg - m) * (1.0 - b1)
        vn = v * b2 + (1.0 - b2) * gg * gg
        return (pd - step_size * mn / (vn.sqrt() / bc2_sqrt + eps), mn, vn, st)
    return ref, host


# ---------------------------------------------------------------------------------------------------------------------
# the GAN's two optimiser updates (train_gan.py:136-145: Adam(lr, betas) without decay on D and on G + E_num) and the re-laid
# copies of the stride-2 convolution weights they keep current
# ---------------------------------------------------------------------------------------------------------------------
GAN_ADAM = dict(beta1=0.5, beta2=0.9, eps=1e-8)             # BETA1 / BETA2 of config/gan_config.yaml (oracle.default_gan_cfg)
GAN_UPDATE_CONFIGS = ((4, 32, 4), (128, 64, 4), (4, 20, 3))        # (C, T, B): the golden fixtures' settings


def wq_plan(spec, transposed_conv):
    """[(parameter, direction, N, Cc, cnk)]: the re-laid (WQ) copies of a network's stride-2 five-tap weights, one per
    direction the weight is used in, wherever the reduction channels are a multiple of 16 and the output columns of 32
    (include/melo_gan_hip.h: mg_conv16).  nn.Conv1d stores (Cout, Cin, 5): forward reduces over Cin with N = Cout (memory
    w[n][c][k]), its data gradient over Cout with N = Cin (memory w[c][n][k]); nn.ConvTranspose1d stores (Cin, Cout, 5) and
    swaps the two."""
    out = []
    for name, shape in spec.items():
        if len(shape) != 3 or shape[2] != 5:
            continue
        a, b = shape[0], shape[1]
        # (direction, N, Cc, memory is [c][n][k])
        both = (("fwd", b, a, True), ("dgrad", a, b, False)) if transposed_conv else (("fwd", a, b, False), ("dgrad", b, a, True))
        for direction, N, Cc, cnk in both:
            if Cc % 16 == 0 and N % 32 == 0:
                out.append((name, direction, N, Cc, cnk))
    return out


def _views(spec, order):
    def split(flat):
        out, off = {}, 0
        for k in order:
            n = math.prod(spec[k])
            out[k] = flat[off:off + n].view(spec[k])
            off += n
        return [out[k] for k in spec]

    def ref(hp, flat):
        return tuple(exact(t) for t in split(flat))

    def host(hp, flat):
        return tuple(t.clone() for t in split(flat))
    return ref, host


def _ema(decay, ramp, offset, n):
    """The fp64 shadow behind the generator's update: s + (1 - d)(p - s), d from the ADVANCED step state, every operation
    rounded on its own -- melo_gan_amd.gan.ema's host restatement, which the kernel is held to bit for bit (an exact stage)."""
    from melo_gan_amd.gan.ema import ema_decay_at

    def value(shadow0, data, state):
        t = float(state[0]) - 1.0 - float(offset)
        omd = 1.0 - float(ema_decay_at(t, decay, ramp))
        s0 = shadow0.double()
        return s0 + omd * (data[:n].double() - s0)

    def ref(hp, shadow0, data, state):
        return (exact(value(shadow0, data, state)),)

    def host(hp, shadow0, data, state):
        return (value(shadow0, data, state),)
    return ref, host


def gan_update_table(X, spec, transposed_conv, order=None, ema=None):
    """`X`.update (X = "D": d_update, "GE": g_update): the flat Adam step; the named parameters are views of the flat buffer
    (`order`: their sequence in it, default the spec's); then every re-laid copy from the UPDATED weights, and the EMA
    shadow where averaging is on."""
    tab = [Stage("Adam", [f"{X}.data", f"{X}.m", f"{X}.v", f"{X}.state"],
                 [f"pre:{X}.data", f"{X}.grad", f"pre:{X}.m", f"pre:{X}.v", f"pre:{X}.state"], *_adam(GAN_ADAM)),
           Stage("re-layout", ["p." + k for k in spec], [f"{X}.data"], *_views(spec, list(order or spec)))]
    for name, direction, N, Cc, cnk in wq_plan(spec, transposed_conv):
        tab.append(Stage("re-layout", [f"wq.{name}.{direction}"], ["p." + name],
                         *relayout(lambda w, N=N, Cc=Cc, cnk=cnk: S.wq_layout(w.reshape(-1), N, Cc, 5, cnk))))
    if ema is not None:         # (decay, ramp, offset): EMA_DECAY > 0, the generator's update only
        tab.append(Stage("re-layout", ["ema"], ["pre:ema", f"{X}.data", f"{X}.state"],
                         *_ema(*ema, sum(math.prod(s_) for s_ in spec.values()))))
    return tab


def gan_update_hp(lr):
    return dict(lr=lr, wd=0.0, grad_scale=1.0)


def vae_tables(spec, hp):
    """{"forward": [...], "backward": [...], "update": [...]}: VaeEngine.forward(True) / backward(beta) / update()."""
    B, T, red, Ld = hp["B"], hp["T"], hp["red"], hp["Ld"]
    Lenc = hp["Ts"][3]
    fwd, bwd, upd = [], [], []
    P = lambda k: "p." + k  # noqa: E731

    def bn_names(nm):
        return [P(nm + ".weight"), P(nm + ".bias")], ["b." + nm + ".running_mean", "b." + nm + ".running_var"]

    # ---- forward ----
    a = "x"
    for j, (i, ci, co) in enumerate(VAE_ENC):
        fwd.append(Stage("encoder conv", [f"ez{j}"], [a, P(f"encoder.conv.{i}.weight"), P(f"encoder.conv.{i}.bias")], *conv_s2()))
        aff, run = bn_names(f"encoder.conv.{i + 1}")
        fwd.append(Stage("BatchNorm forward", [f"e_mean{j}", f"e_istd{j}", f"ea{j}"] + run,
                         [f"ez{j}"] + aff + ["pre:" + r for r in run], *bn_train()))
        a = f"ea{j}"
    # h.reshape(B, -1) of the (B, 128, L) tensor: model.py:46
    fwd.append(Stage("re-layout", ["flat"], [a], *relayout(lambda t: t.transpose(1, 2).reshape(t.shape[0], -1))))
    fwd.append(Stage("Linear forward", ["h"], ["flat", P("encoder._linear.1.weight"), P("encoder._linear.1.bias")], *linear(ACT_RELU)))
    fwd.append(Stage("Linear forward", ["mu"], ["h", P("fc_mu.weight"), P("fc_mu.bias")], *linear()))
    fwd.append(Stage("Linear forward", ["lv"], ["h", P("fc_log_var.weight"), P("fc_log_var.bias")], *linear()))
    fwd.append(Stage("reparameterise", ["zl"], ["mu", "lv", "eps"], *_reparam_fwd()))
    fwd.append(Stage("Linear forward", ["p0"], ["zl", P("decoder.pre.0.weight"), P("decoder.pre.0.bias")], *linear(ACT_RELU)))
    fwd.append(Stage("Linear forward", ["p2"], ["p0", P("decoder.pre.2.weight"), P("decoder.pre.2.bias")], *linear(ACT_RELU)))
    fwd.append(Stage("re-layout", ["y0"], ["p2"], *relayout(lambda t: t.view(t.shape[0], 128, -1).transpose(1, 2))))
    a = "y0"
    for j, (i, ci, co) in enumerate(VAE_DEC):
        wb = [P(f"decoder.deconv.{i}.weight"), P(f"decoder.deconv.{i}.bias")]
        if i == 6:
            fwd.append(Stage("decoder convT", ["recon"], [a] + wb, *convT_s2(ACT_TANH, T)))
            break
        fwd.append(Stage("decoder convT", [f"dz_{j}"], [a] + wb, *convT_s2()))
        aff, run = bn_names(f"decoder.deconv.{i + 1}")
        fwd.append(Stage("BatchNorm forward", [f"d_mean{j}", f"d_istd{j}", f"da_{j}"] + run,
                         [f"dz_{j}"] + aff + ["pre:" + r for r in run], *bn_train()))
        a = f"da_{j}"

    # ---- backward ----
    G = lambda k: "g." + k  # noqa: E731
    bwd.append(Stage("loss", ["loss", "g_recon@loss", "k_mu", "k_lv"], ["recon", "x", "mu", "lv"], _vae_loss_ref, _vae_loss_host))
    bwd.append(Stage("activation backward", ["g_recon"], ["g_recon@loss", "recon"], *act_back(ACT_TANH)))
    dn = "g_recon"
    if Ld[3] != T:      # the padding rows carry no gradient into the decoder (torch.cat with zeros, vae_fwd)
        bwd.append(Stage("re-layout", ["g_rec_dense"], ["g_recon"], *relayout(lambda t: t[:, :Ld[3]])))
        dn = "g_rec_dense"
    ins = ["y0", "da_0", "da_1"]
    for j in (2, 1, 0):
        i = VAE_DEC[j][0]
        w = P(f"decoder.deconv.{i}.weight")
        bwd.append(Stage("decoder weight gradient", [G(f"decoder.deconv.{i}.weight"), G(f"decoder.deconv.{i}.bias")], [ins[j], dn], *convT_s2_wgrad()))
        if j == 0:
            bwd.append(Stage("decoder data gradient", ["g_y0"], [dn, w], *convT_s2_dgrad()))
            break
        bwd.append(Stage("decoder data gradient", [f"g_da{j - 1}"], [dn, w], *convT_s2_dgrad()))
        nm = f"decoder.deconv.{VAE_DEC[j - 1][0] + 1}"
        bwd.append(Stage("BatchNorm backward", [f"g_dz{j - 1}", G(nm + ".weight"), G(nm + ".bias")],
                         [f"g_da{j - 1}", f"da_{j - 1}", f"dz_{j - 1}", P(nm + ".weight"), P(nm + ".bias"), f"d_mean{j - 1}", f"d_istd{j - 1}"], *bn_back()))
        dn = f"g_dz{j - 1}"

    def gp2_ref(hp_, gy0, p2):
        return (S.act_bwd(gy0.transpose(1, 2).reshape(gy0.shape[0], -1), p2, ACT_RELU),)

    def gp2_host(hp_, gy0, p2):
        return (gy0.transpose(1, 2).reshape(gy0.shape[0], -1) * (p2 > 0).to(gy0.dtype),)
    bwd.append(Stage("activation backward", ["g_p2"], ["g_y0", "p2"], gp2_ref, gp2_host))
    bwd.append(Stage("Linear weight gradient", [G("decoder.pre.2.weight"), G("decoder.pre.2.bias")], ["p0", "g_p2"], *linear_wgrad()))
    bwd.append(Stage("Linear data gradient", ["g_p0"], ["g_p2", P("decoder.pre.2.weight"), "p0"], *linear_dgrad(ACT_RELU)))
    bwd.append(Stage("Linear weight gradient", [G("decoder.pre.0.weight"), G("decoder.pre.0.bias")], ["zl", "g_p0"], *linear_wgrad()))
    bwd.append(Stage("Linear data gradient", ["g_z"], ["g_p0", P("decoder.pre.0.weight")], *linear_dgrad()))
    bwd.append(Stage("reparameterise backward", ["g_mu", "g_lv"], ["g_z", "lv", "eps", "k_mu", "k_lv"], *_reparam_bwd()))
    bwd.append(Stage("Linear weight gradient", [G("fc_mu.weight"), G("fc_mu.bias")], ["h", "g_mu"], *linear_wgrad()))
    bwd.append(Stage("Linear weight gradient", [G("fc_log_var.weight"), G("fc_log_var.bias")], ["h", "g_lv"], *linear_wgrad()))
    bwd.append(Stage("Linear data gradient", ["g_h@sum"], ["g_mu", P("fc_mu.weight"), "g_lv", P("fc_log_var.weight")], *linear_dgrad_sum2()))
    bwd.append(Stage("activation backward", ["g_h"], ["g_h@sum", "h"], *act_back(ACT_RELU)))
    bwd.append(Stage("Linear weight gradient", [G("encoder._linear.1.weight"), G("encoder._linear.1.bias")], ["flat", "g_h"], *linear_wgrad()))
    bwd.append(Stage("Linear data gradient", ["g_flat"], ["g_h", P("encoder._linear.1.weight")], *linear_dgrad()))
    bwd.append(Stage("re-layout", ["g_ea2"], ["g_flat"], *relayout(lambda t: t.view(t.shape[0], 128, -1).transpose(1, 2))))
    ins = ["x", "ea0", "ea1"]
    for j in (2, 1, 0):
        i = VAE_ENC[j][0]
        nm = f"encoder.conv.{i + 1}"
        bwd.append(Stage("BatchNorm backward", [f"g_ez{j}", G(nm + ".weight"), G(nm + ".bias")],
                         [f"g_ea{j}", f"ea{j}", f"ez{j}", P(nm + ".weight"), P(nm + ".bias"), f"e_mean{j}", f"e_istd{j}"], *bn_back()))
        bwd.append(Stage("encoder weight gradient", [G(f"encoder.conv.{i}.weight"), G(f"encoder.conv.{i}.bias")], [ins[j], f"g_ez{j}"], *conv_s2_wgrad()))
        if j > 0:
            bwd.append(Stage("encoder data gradient", [f"g_ea{j - 1}"], [f"g_ez{j}", P(f"encoder.conv.{i}.weight"), ins[j]], *conv_s2_dgrad()))
    bwd.append(Stage("re-layout", ["P.grad"], vae_grad_names(spec), *_vae_gather_grad(spec)))

    # ---- update ----
    n = sum(math.prod(s) for s in spec.values())
    upd.append(Stage("gradient-norm clip", ["gnorm"], ["P.grad"], *_clip(n)))
    upd.append(Stage("AdamW", ["P.data", "P.m", "P.v", "P.state"], ["pre:P.data", "P.grad", "pre:P.m", "pre:P.v", "pre:P.state", "gnorm"],
                     *_adam(VAE_ADAM)))
    return OrderedDict(forward=fwd, backward=bwd, update=upd)


VAE_FLOWS = ("forward", "backward", "update")


def vae_initial(spec, bufs, P, Bf, x, eps):
    """The `pre` dict of a first step: parameters (named and flat), buffers, zero moments and step state, the batch."""
    pre = {"p." + k: P[k] for k in spec}
    pre.update({"b." + k: Bf[k] for k in bufs})
    pre["P.data"] = flat_of(spec, pre, "p.", P[next(iter(spec))].dtype)
    pre["P.m"], pre["P.v"] = torch.zeros_like(pre["P.data"]), torch.zeros_like(pre["P.data"])
    pre["P.state"] = torch.zeros(4, dtype=torch.float64)
    pre["x"], pre["eps"] = x, eps
    return pre


def unflatten(spec, flat, prefix):
    out, off = {}, 0
    for k, s in spec.items():
        n = math.prod(s)
        out[prefix + k] = flat[off:off + n].view(s)
        off += n
    return out


def vae_step(tables, spec, pre, hp, dtype=torch.float64, mutate=None, carry="host"):
    """forward, backward, update in one go: (post, ratios per flow).  post carries the updated named parameters, so it is
    the `pre` of the next step once x / eps are replaced."""
    ratios = OrderedDict()
    cur = pre
    for flow in VAE_FLOWS:
        cur, ratios[flow] = evaluate(tables[flow], cur, hp, dtype, mutate, carry)
    cur.update(unflatten(spec, cur["P.data"], "p."))
    return cur, ratios


# ---------------------------------------------------------------------------------------------------------------------
# the critic step's critic part (train_gan.py:183-205; oracle d_step / discriminator_fwd / gradient_penalty), from the
# real batch, the fake batch, the numeric embedding and alpha: the three critic evaluations as ONE batch of 3B rows
# [x_hat | real | fake] back-propagated with ds = [1 | -1/B | +1/B] (the penalty's autograd.grad(grad_outputs=ones) and the
# two Wasserstein means), the penalty's second-order term as a tangent pass through the critic with x_hat's LeakyReLU
# masks (D is piecewise linear), and every weight gradient = [real | fake] activations x Wasserstein dZ + tangent x
# penalty dZ in one two-segment sum.
# ---------------------------------------------------------------------------------------------------------------------
ACT_LRELU = S.ACT_LRELU
CRITIC_CONVS = (("conv.0", "A1"), ("conv.2", "A2"), ("conv.4", "A3"))
# (C, T, B): the golden fixtures' settings -- thin kernels; conv16 with its riders; an odd time axis (20 -> 10 -> 5 -> 3)
# and the smallest roll at which conv.4's launch carries the pooled mean at B = 2 (one sample's 32 output positions = one
# wave tile of two 16-row MFMA tiles: T3 = 32, T = 256; tests/test_engine_ref.py recomputes the predicate)
GAN_CRITIC_CONFIGS = ((4, 32, 4), (128, 64, 4), (4, 20, 3), (4, 256, 2))


def critic_ds(B, exact_thirds=False):
    """ds of the 3B rows: the device holds the fp32 values of -1/B and 1/B (exact_thirds: the fp64 ones, for the comparison
    with the oracle's means)."""
    v = torch.cat([torch.ones(B, dtype=torch.float64), torch.full((B,), -1.0 / B, dtype=torch.float64), torch.full((B,), 1.0 / B, dtype=torch.float64)])
    return v if exact_thirds else v.float().double()


def critic_hp(B, T, lambda_gp=10.0, pooled=False, pooled_tan=False, exact_thirds=False):
    return dict(B=B, T=T, lambda_gp=lambda_gp, pooled=pooled, pooled_tan=pooled_tan, ds=critic_ds(B, exact_thirds))


def _slope(a):
    return torch.where(a > 0, torch.ones_like(a), torch.full_like(a, SLOPE))


def _conv_raw(x, w, b=None):
    return _ncl(F.conv1d(_ncl(x), w, b, 2, 2))


def _x3():
    def ref(hp, xhat, real, fake):
        return (exact(torch.cat([xhat, real, fake], 0)),)

    def host(hp, xhat, real, fake):
        return (torch.cat([xhat, real, fake], 0),)
    return ref, host


def _interp():
    def ref(hp, real, fake, alpha):
        return (S.gp_interp(real, fake, alpha.reshape(-1)),)

    def host(hp, real, fake, alpha):
        a = alpha.reshape(-1, 1, 1)
        return (a * real + (1 - a) * fake,)
    return ref, host


def _critic_conv():
    def ref(hp, x, w, b):
        v, m = S2.gather(x, w)
        return (lrelu_on(Ref(v, m, 5 * x.shape[2]).epilogue(bias=b)),)

    def host(hp, x, w, b):
        return (_lrelu(_conv_raw(x, w, b)),)
    return ref, host


def _pool(flag):
    """AdaptiveAvgPool1d(1): its own launch (n = T, k = 1) or the rider of the convolution launch that stores the rows
    (the mean of T stored values: n = T)."""
    def ref(hp, a):
        r = S.meanT_fwd(a)
        if hp.get(flag):
            r.k_epi = 0
        return (r,)

    def host(hp, a):
        return (a.mean(1),)
    return ref, host


def _emb_rows(emb, n):
    return emb[torch.arange(n, device=emb.device) % emb.shape[0]]


def _head():
    def ref(hp, f, emb, w, b):
        return (S.dhead_fwd(f, emb, w.reshape(-1), b),)

    def host(hp, f, emb, w, b):
        Fd = f.shape[1]
        ww = w.reshape(-1)
        return (f @ ww[:Fd] + _emb_rows(emb, f.shape[0]) @ ww[Fd:] + b[0],)
    return ref, host


def _head_bwd(ds_of=lambda hp: hp["ds"]):
    """dU = ds w LeakyReLU'(f): support_ref.dhead_bwd's count (k = 3: two products and the constant), with the slope at its
    fp32 value like every other LeakyReLU' here (dhead_bwd takes the exact 0.2, which differs by a quarter of a rounding:
    inside its bound, but not equal to an oracle that holds 0.2f throughout)."""
    def ref(hp, f, w):
        v = ds_of(hp).to(f.device)[:, None] * w.double().reshape(-1)[None, :f.shape[1]] * _slope(f.double())
        return (mk(v, v.abs(), 0, 3),)

    def host(hp, f, w):
        ds = ds_of(hp).to(f.device, f.dtype)
        return (ds[:, None] * w.reshape(-1)[None, :f.shape[1]] * _slope(f),)
    return ref, host


def _pool_bwd():
    def ref(hp, dh, a):
        return (S.meanT_bwd(dh, a.shape[1], gref=a, gact=ACT_LRELU),)

    def host(hp, dh, a):
        return ((dh / a.shape[1])[:, None, :] * _slope(a),)
    return ref, host


def _critic_dgrad(rows=None, masked=True, other_rows=False):
    """Data gradient of a critic convolution (times LeakyReLU' of the layer below, taken at the stored activation of the
    SAME rows); rows: the first `rows` samples only (the penalty's x_hat third).  other_rows: the host's mistake of reading
    the mask from the next third."""
    def ref(hp, dy, w, a):
        n = rows(hp) if rows else dy.shape[0]
        v, m = S2.scatter(dy[:n], w, a.shape[1])
        r = Ref(v, m, 5 * dy.shape[2])
        return (r.epilogue(gref=a[:n], gact=ACT_LRELU) if masked else r,)

    def host(hp, dy, w, a):
        n = rows(hp) if rows else dy.shape[0]
        x0 = dy.new_zeros(n, a.shape[1], w.shape[1])
        (g,) = _vjp(lambda x: _conv_raw(x, w), [x0], [0], dy[:n])
        o = n if other_rows else 0
        return (g * _slope(a[o:o + n]) if masked else g,)
    return ref, host


def _penalty():
    def ref(hp, gx):
        norms, gbar, _ = S.gp_penalty(gx, hp["lambda_gp"])
        return (norms, gbar)

    def host(hp, gx):
        B = gx.shape[0]
        n = (gx * gx).reshape(B, -1).sum(1).sqrt()
        fac = f32(hp["lambda_gp"]) * (2.0 / B) * (n - 1) / n
        return (n, fac.view(B, 1, 1) * gx)
    return ref, host


def _tangent_conv(other_rows=False):
    """A tangent through a critic convolution: no bias, times the LeakyReLU mask of the x_hat rows (the first B)."""
    def ref(hp, t, w, a):
        v, m = S2.gather(t, w)
        return (Ref(v, m, 5 * t.shape[2]).epilogue(gref=a[:hp["B"]], gact=ACT_LRELU),)

    def host(hp, t, w, a):
        B = hp["B"]
        o = B if other_rows else 0
        return (_conv_raw(t, w) * _slope(a[o:o + B]),)
    return ref, host


def _tangent_fc():
    def ref(hp, g, w, f):
        v, m = W.linear(g, w)
        return (Ref(v, m, g.shape[1]).epilogue(gref=f[:hp["B"]], gact=ACT_LRELU),)

    def host(hp, g, w, f):
        return (F.linear(g, w) * _slope(f[:hp["B"]]),)
    return ref, host


def _critic_conv_wgrad(tangent=True):
    """[real | fake] activations x Wasserstein dZ + tangent x penalty dZ: ONE sum over 2B + B samples; the bias gradient
    sums the Wasserstein rows only (the tangent pass has no bias).  tangent=False: the host's mistake."""
    def ref(hp, x, dy, t):
        B = hp["B"]
        (dw, mw, n), (db, mb, nb) = S2.conv_wgrad(x[B:3 * B], dy[B:3 * B], t, dy[:B])
        return (Ref(dw, mw, n), Ref(db, mb, nb))

    def host(hp, x, dy, t):
        B = hp["B"]
        xs, ds = (torch.cat([x[B:3 * B], t], 0), torch.cat([dy[B:3 * B], dy[:B]], 0)) if tangent else (x[B:3 * B], dy[B:3 * B])
        w0 = x.new_zeros(dy.shape[2], x.shape[2], 5)
        (dw,) = _vjp(lambda w: _conv_raw(xs, w), [w0], [0], ds)
        return (dw, dy[B:3 * B].sum((0, 1)))
    return ref, host


def _critic_fc_wgrad():
    def ref(hp, h, du, ghb):
        B = hp["B"]
        v3 = lambda t: t.reshape(t.shape[0], 1, -1)  # noqa: E731
        (dw, mw, n), (db, mb, nb) = W.wgrad_s1(v3(h[B:3 * B]), v3(du[B:3 * B]), 1, v3(ghb), v3(du[:B]))
        return (Ref(dw[:, :, 0], mw[:, :, 0], n), Ref(db, mb, nb))

    def host(hp, h, du, ghb):
        B = hp["B"]
        return (du[B:3 * B].t() @ h[B:3 * B] + du[:B].t() @ ghb, du[B:3 * B].sum(0))
    return ref, host


def _critic_head_wgrad(swap=False):
    """The scoring head's gradient over the 2B Wasserstein rows + the penalty's sum of gfb, and the loss scalars that ride in
    its launch: (loss_d, mean_real, mean_fake) and gp.  swap: the host's mistake of ds with real and fake exchanged."""
    def ref(hp, f, emb, gfb, s, norms):
        B = hp["B"]
        ds = hp["ds"].to(f.device)[B:]
        dwf, dwe, dbias = S.dhead_wgrad(ds, f[B:3 * B], emb, gfb, 2 * B, B)
        loss, mr, mf, gp = S.wgan_d_loss(s[B:3 * B], norms, hp["lambda_gp"], B)
        return (_row(cat_refs([dwf, dwe])), dbias, cat_refs([loss, mr, mf]), gp)

    def host(hp, f, emb, gfb, s, norms):
        B = hp["B"]
        ds = hp["ds"].to(f.device, f.dtype)[B:]
        if swap:
            ds = torch.cat([ds[B:], ds[:B]])
        fw = f[B:3 * B]
        dw = torch.cat([ds @ fw + gfb.sum(0), ds @ _emb_rows(emb, 2 * B)])
        mr, mf = s[B:2 * B].mean(), s[2 * B:3 * B].mean()
        gp = ((norms - 1) ** 2).mean()
        return (dw[None], ds.sum().reshape(1), torch.stack([mf - mr + f32(hp["lambda_gp"]) * gp, mr, mf]), gp.reshape(1))
    return ref, host


def _row(r):
    """A Ref of a vector as the (1, n) tensor real_fake.weight is."""
    return from_bounds(r.val[None], r.bound()[None])


def critic_table(hp):
    """The critic part of d_backward.  Tensor names are GanEngine's; xhat / real / fake_d are its X0[:B] / [B:2B] / [2B:3B]."""
    P, G = (lambda k: "p." + k), (lambda k: "g." + k)  # noqa: E731
    first = lambda hp_: hp_["B"]  # noqa: E731
    t = [Stage("gradient penalty", ["xhat"], ["real", "fake_d", "alpha"], *_interp()),
         Stage("re-layout", ["X3"], ["xhat", "real", "fake_d"], *_x3())]
    a = "X3"
    for nm, out in CRITIC_CONVS:
        t.append(Stage("critic forward", [out], [a, P(nm + ".weight"), P(nm + ".bias")], *_critic_conv()))
        a = out
    t += [Stage("critic forward", ["H"], ["A3"], *_pool("pooled")),
          Stage("critic forward", ["Fh"], ["H", P("fc.1.weight"), P("fc.1.bias")], *linear(ACT_LRELU)),
          Stage("critic head", ["s"], ["Fh", "emb_d", P("real_fake.weight"), P("real_fake.bias")], *_head()),
          Stage("critic head", ["dU"], ["Fh", P("real_fake.weight")], *_head_bwd()),
          Stage("critic data gradient", ["dH"], ["dU", P("fc.1.weight")], *linear_dgrad()),
          Stage("critic data gradient", ["dZ3"], ["dH", "A3"], *_pool_bwd()),
          Stage("critic data gradient", ["dZ2"], ["dZ3", P("conv.4.weight"), "A2"], *_critic_dgrad()),
          Stage("critic data gradient", ["dZ1"], ["dZ2", P("conv.2.weight"), "A1"], *_critic_dgrad()),
          Stage("critic data gradient", ["gx"], ["dZ1", P("conv.0.weight"), "xhat"], *_critic_dgrad(first, masked=False)),
          Stage("gradient penalty", ["norms", "TAN0"], ["gx"], *_penalty()),
          Stage("tangent pass", ["TAN1"], ["TAN0", P("conv.0.weight"), "A1"], *_tangent_conv()),
          Stage("tangent pass", ["TAN2"], ["TAN1", P("conv.2.weight"), "A2"], *_tangent_conv()),
          Stage("tangent pass", ["TZ3"], ["TAN2", P("conv.4.weight"), "A3"], *_tangent_conv()),
          Stage("tangent pass", ["ghb"], ["TZ3"], *_pool("pooled_tan")),
          Stage("tangent pass", ["gfb"], ["ghb", P("fc.1.weight"), "Fh"], *_tangent_fc()),
          Stage("critic weight gradient", [G("conv.0.weight"), G("conv.0.bias")], ["X3", "dZ1", "TAN0"], *_critic_conv_wgrad()),
          Stage("critic weight gradient", [G("conv.2.weight"), G("conv.2.bias")], ["A1", "dZ2", "TAN1"], *_critic_conv_wgrad()),
          Stage("critic weight gradient", [G("conv.4.weight"), G("conv.4.bias")], ["A2", "dZ3", "TAN2"], *_critic_conv_wgrad()),
          Stage("critic weight gradient", [G("fc.1.weight"), G("fc.1.bias")], ["H", "dU", "ghb"], *_critic_fc_wgrad()),
          Stage("critic head weight gradient + loss", [G("real_fake.weight"), G("real_fake.bias"), "loss_d_out", "gp"],
                ["Fh", "emb_d", "gfb", "s", "norms"], *_critic_head_wgrad())]
    return t


# ---------------------------------------------------------------------------------------------------------------------
# the numeric encoder's and the generator's forward (oracle feature_encoder_fwd / generator_fwd; feature_encoder.py:16-45,
# models.py:66-130) on `groups` batches of B rows stacked along dim 0: one group is a sub-step's own pass (the critic step's
# no_grad pass or the generator step's), two are the fused step's 2B-row pass -- same weights, per-group noise, dropout
# masks and BatchNorm batch statistics, the running statistics moved once per group, first group first.
# ---------------------------------------------------------------------------------------------------------------------
ACT_GELU = S.ACT_GELU
LN_EPS = 1e-5


def _ln_fwd():
    def ref(hp, x, g, b):
        return S.layernorm_fwd(x, g, b, LN_EPS)

    def host(hp, x, g, b):
        mean = x.mean(-1, keepdim=True)
        c = x - mean
        xh = c * ((c * c).mean(-1, keepdim=True) + f32(LN_EPS)) ** -0.5
        return (xh * g + b, xh)
    return ref, host


def _gelu_linear():
    """z = x W^T + b kept, a = GELU(z) * mask (the keep-mask times 1 / (1 - p))."""
    def ref(hp, x, w, b, mask):
        v, m = W.linear(x, w)
        r = Ref(v, m, x.shape[1]).epilogue(bias=b, zout=True)
        z = r.z
        return (z, S.act_on(r, ACT_GELU).epilogue(emul=mask))

    def host(hp, x, w, b, mask):
        z = F.linear(x, w, b)
        return (z, F.gelu(z) * mask)
    return ref, host


def _gin():
    def ref(hp, *parts):
        return (exact(_gin_host(hp, *parts)),)

    def host(hp, *parts):
        return (_gin_host(hp, *parts),)
    return ref, host


def _gin_host(hp, noise, emb, *latent):
    cols = [noise, emb] + [torch.cat([l] * hp["groups"], 0) for l in latent]      # the batch's latent, once per group
    return torch.cat(cols, 1)


def _pre2():
    """decoder.pre.2 + ReLU in the channels-last order the first deconvolution reads: view(B, 256, L) + permute."""
    def ref(hp, x, w, b):
        v, m = W.linear(x, w)
        r = Ref(v, m, x.shape[1]).epilogue(bias=b, act=ACT_RELU)
        cl = lambda t: t.view(t.shape[0], 256, -1).transpose(1, 2).contiguous()  # noqa: E731
        return (from_bounds(cl(r.val), cl(r.bound())),)

    def host(hp, x, w, b):
        y = torch.relu(F.linear(x, w, b))
        return (y.view(y.shape[0], 256, -1).transpose(1, 2).contiguous(),)
    return ref, host


def bn_train_groups(act=ACT_RELU, stats_of=None):
    """bn_train over hp["groups"] stacked batches: save_mean / save_invstd are (groups, C) (one group: (C,)).
    stats_of: the host's mistake of normalising group g with the statistics of group stats_of(g)."""
    def ref(hp, z, gamma, beta, rm0, rv0):
        G = hp["groups"]
        st = S.bn_stats(z, G, BN_EPS)
        a = S.bn_apply(z, st["mean"], st["invstd"], gamma, beta, act)
        rm, rv = S.bn_running(st, rm0, rv0, BN_MOM)
        sm, si = st["save_mean"], st["save_invstd"]
        sq = (lambda r: from_bounds(r.val[0], r.bound()[0])) if G == 1 else (lambda r: r)
        return (sq(sm), sq(si), a, rm, rv)

    def host(hp, z, gamma, beta, rm0, rv0):
        G = hp["groups"]
        one = bn_train(act)[1]
        hp1 = dict(hp, groups=1)
        outs, rm, rv = [], rm0, rv0
        for zg in z.chunk(G, 0):
            m, i, a, rm, rv = one(hp1, zg, gamma, beta, rm, rv)
            outs.append((m, i, zg))
        if stats_of is not None:
            acts = [_act(act, (zg - outs[stats_of(g)][0]) * outs[stats_of(g)][1] * gamma + beta) for g, (_, _, zg) in enumerate(outs)]
        else:
            acts = [_act(act, (zg - m) * i * gamma + beta) for (m, i, zg) in outs]
        mean, istd = torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])
        if G == 1:
            mean, istd = mean[0], istd[0]
        return (mean, istd, torch.cat(acts, 0), rm, rv)
    return ref, host


def parts_totals(part, groups, C):
    """(groups, 3, C) fp64: per group the column sum, the row count and the biased variance that the (chunks, 3, C) fp32
    partial statistics (per chunk: sum, M2 about the chunk's own mean, rows; support_ref.conv16_parts) combine to."""
    p = part.reshape(-1, 3, C)
    out = []
    for pg in p.chunk(groups, 0):
        st = S.parts_stats(pg.float())
        out.append(torch.stack([st["mean"][0] * st["R"], torch.full_like(st["mean"][0], float(st["R"])), st["var"][0]]))
    return torch.stack(out)


def _parts_rider():
    """The statistics rider of the convolution launch that stores z: per group the sum of R stored rows (n = R), their
    count (exact) and the variance -- each chunk's M2 is a sum of squared differences from the chunk's fp32 mean, so k = 3
    (that mean, the difference, the square) on M = E[z^2] + mean^2 with n = R."""
    def ref(hp, part, z):
        C = z.shape[-1]
        out = []
        for zg in z.chunk(hp["groups"], 0):
            x = S.rows(zg).double()
            R = x.shape[0]
            mean = x.mean(0)
            var = ((x - mean) ** 2).mean(0)
            refs = [mk(x.sum(0), x.abs().sum(0), R, 0), exact(torch.full((C,), float(R), dtype=torch.float64, device=z.device)),
                    mk(var, (x * x).mean(0) + mean * mean, R, 3)]
            out.append(from_bounds(torch.stack([r.val for r in refs]), torch.stack([r.bound() for r in refs])))
        return (from_bounds(torch.stack([o.val for o in out]), torch.stack([o.bound() for o in out])),)

    def host(hp, part, z):
        return (parts_totals(part, hp["groups"], z.shape[-1]),)
    return ref, host


def bn_train_from_parts(act=ACT_RELU):
    """bn_train_groups where the producing launch left partial statistics: the statistics are those the ROUNDED partials
    combine to (support_ref.parts_stats: the combine is fp64), everything behind them as in bn_train_groups."""
    def stats(hp, part, C):
        return S.cat_stats([S.parts_stats(pg.float()) for pg in part.reshape(-1, 3, C).chunk(hp["groups"], 0)])

    def ref(hp, part, z, gamma, beta, rm0, rv0):
        G = hp["groups"]
        st = stats(hp, part, z.shape[-1])
        a = S.bn_apply(z, st["mean"], st["invstd"], gamma, beta, act)
        rm, rv = S.bn_running(st, rm0, rv0, BN_MOM)
        sq = (lambda r: from_bounds(r.val[0], r.bound()[0])) if G == 1 else (lambda r: r)
        return (sq(st["save_mean"]), sq(st["save_invstd"]), a, rm, rv)

    def host(hp, part, z, gamma, beta, rm0, rv0):
        G = hp["groups"]
        st = stats(hp, part, z.shape[-1])
        mean, istd, unb = (st[k].to(z.dtype) for k in ("mean", "invstd", "unb"))
        acts = [_act(act, (zg - mean[g]) * istd[g] * gamma + beta) for g, zg in enumerate(z.chunk(G, 0))]
        mom, rm, rv = f32(BN_MOM), rm0, rv0
        for g in range(G):
            rm, rv = (1.0 - mom) * rm + mom * mean[g], (1.0 - mom) * rv + mom * unb[g]
        return ((mean[0], istd[0]) if G == 1 else (mean, istd)) + (torch.cat(acts, 0), rm, rv)
    return ref, host


# which of the generator's two BatchNorm layers take the partial statistics at the critic configurations (one group; the
# same with two): where conv16 runs the deconvolution and no row tile straddles two groups.  tests/test_engine_ref.py
# recomputes this from the library's plan, the GPU file asserts it on the launches.
GAN_PARTS_ROUTES = {(4, 32, 4): (False, False), (128, 64, 4): (False, True), (4, 20, 3): (False, False), (4, 256, 2): (True, True),
                    (4, 16, 3): (False, False), (128, 128, 2): (False, True)}
# (C, T, B) of the bf16 emotion branch (ed_dtype="bf16": MAX_NOTES % 128, channels % 32 / % 64)
GAN_BF16_ED_CONFIG = (128, 128, 2)
# (C, T, B) with INTEGRATION_MODE "conditioning" and the latent-mode emotion classifier (the golden fixture gan_c4_t16_cond_lat)
GAN_COND_LATENT_CONFIG = (4, 16, 3)


def gen_forward_hp(B, T, groups=1, parts=(False, False)):
    """parts[j]: BatchNorm j takes its statistics from the partials the deconvolution's launch left (conv16's rider)."""
    return dict(B=B, T=T, groups=groups, parts=tuple(parts))


def gen_forward_table(hp, conditioning=False):
    PE, PG = (lambda k: "p.E." + k), (lambda k: "p.G." + k)  # noqa: E731
    T = hp["T"]
    t = [Stage("numeric encoder", ["e_x0", "e_xhat"], ["numeric", PE("net.0.weight"), PE("net.0.bias")], *_ln_fwd()),
         Stage("numeric encoder", ["e_z1", "e_h1"], ["e_x0", PE("net.1.weight"), PE("net.1.bias"), "dmask0"], *_gelu_linear()),
         Stage("numeric encoder", ["e_z2", "e_h2"], ["e_h1", PE("net.4.weight"), PE("net.4.bias"), "dmask1"], *_gelu_linear()),
         Stage("numeric encoder", ["emb"], ["e_h2", PE("net.7.weight"), PE("net.7.bias")], *linear()),
         Stage("re-layout", ["gin"], ["noise", "emb"] + (["latent"] if conditioning else []), *_gin()),
         Stage("generator Linear", ["a_n0"], ["gin", PG("noise_to_latent.net.0.weight"), PG("noise_to_latent.net.0.bias")], *linear(ACT_RELU)),
         Stage("generator Linear", ["lat"], ["a_n0", PG("noise_to_latent.net.2.weight"), PG("noise_to_latent.net.2.bias")], *linear()),
         Stage("generator Linear", ["a_p0"], ["lat", PG("decoder.pre.0.weight"), PG("decoder.pre.0.bias")], *linear(ACT_RELU)),
         Stage("generator Linear", ["y0"], ["a_p0", PG("decoder.pre.2.weight"), PG("decoder.pre.2.bias")], *_pre2())]
    a = "y0"
    for j, (i, z, act_) in enumerate(((0, "z_d0", "a_d0"), (3, "z_d3", "a_d3"))):
        nm = f"decoder.deconv.{i + 1}"
        run = ["b." + nm + ".running_mean", "b." + nm + ".running_var"]
        t.append(Stage("generator convT", [z], [a, PG(f"decoder.deconv.{i}.weight"), PG(f"decoder.deconv.{i}.bias")], *convT_s2()))
        if hp["parts"][j]:
            t.append(Stage("generator BatchNorm partials", [f"partsum{j}"], [f"part{j}", z], *_parts_rider()))
            t.append(Stage("generator BatchNorm", [f"bn_mean{j}", f"bn_invstd{j}", act_] + run,
                           [f"part{j}", z, PG(nm + ".weight"), PG(nm + ".bias")] + ["pre:" + r for r in run], *bn_train_from_parts()))
        else:
            t.append(Stage("generator BatchNorm", [f"bn_mean{j}", f"bn_invstd{j}", act_] + run,
                           [z, PG(nm + ".weight"), PG(nm + ".bias")] + ["pre:" + r for r in run], *bn_train_groups()))
        a = act_
    t.append(Stage("generator convT", ["notes"], [a, PG("decoder.deconv.6.weight"), PG("decoder.deconv.6.bias")], *convT_s2(ACT_NONE, T)))
    return t


# ---------------------------------------------------------------------------------------------------------------------
# the generator step behind its forward and the emotion branch (train_gan.py:211-251; oracle g_step): the UPDATED critic on
# the generated batch, adv = -mean(D(fake)), its input gradient added to the emotion branch's, the generator's and the
# numeric encoder's backward.  The emotion branch's own gradient (dnotes@ed: what it left in dnotes; latent mode: ed_dfeat)
# is an input here: its own rows are ed_branch_table's, below.
# ---------------------------------------------------------------------------------------------------------------------
def _scaled_mean(scale):
    def ref(hp, s):
        return (S.mean_scaled(s, scale),)

    def host(hp, s):
        return ((f32(scale) * s.mean()).reshape(1),)
    return ref, host


def _g_ds(hp, like):
    """ds of the generator step's B rows: -1/B, at its fp32 value on the device (critic_ds)."""
    return hp["ds"].to(like.device)


def _demb_head():
    """The embedding half of the scoring head's input gradient: demb[b, j] = ds[b] w[F + j] (one term, k = 1)."""
    def ref(hp, f, w):
        v = _g_ds(hp, f)[:, None] * w.double().reshape(-1)[None, f.shape[1]:]
        return (mk(v, v.abs(), 1, 1),)

    def host(hp, f, w):
        return (_g_ds(hp, f).to(f.dtype)[:, None] * w.reshape(-1)[None, f.shape[1]:],)
    return ref, host


def _dnotes(accumulate, overwrite=False):
    """conv.0's data gradient of the critic path, ADDED to what the emotion branch left in dnotes (notes mode).
    overwrite: the host's mistake."""
    def ref(hp, dz, w, like, *base):
        v, m = S2.scatter(dz, w, like.shape[1])
        r = Ref(v, m, 5 * dz.shape[2])
        return (r.epilogue(base=base[0]) if accumulate else r,)

    def host(hp, dz, w, like, *base):
        (g,) = _vjp(lambda x: _conv_raw(x, w), [dz.new_zeros(like.shape)], [0], dz)
        return (g + base[0] if accumulate and not overwrite else g,)
    return ref, host


def _dp2():
    """deconv.0's data gradient times decoder.pre.2's ReLU', in the (B, 256 L) order of the Linear's output."""
    def ref(hp, dy, w, y0):
        v, m = S2.gather(dy, w)
        r = Ref(v, m, 5 * dy.shape[2]).epilogue(gref=y0, gact=ACT_RELU)
        fl = lambda t: t.transpose(1, 2).reshape(t.shape[0], -1)  # noqa: E731
        return (from_bounds(fl(r.val), fl(r.bound())),)

    def host(hp, dy, w, y0):
        g = convT_s2_dgrad()[1](hp, dy, w)[0] * (y0 > 0).to(dy.dtype)
        return (g.transpose(1, 2).reshape(g.shape[0], -1),)
    return ref, host


def _sum2(drop=None):
    """One tensor summed from two: the second is added onto the first (k = 1).  drop: the host's mistake (0 or 1)."""
    def ref(hp, a, b):
        v, m = a.double() + b.double(), a.double().abs() + b.double().abs()
        return (mk(v, m, 0, 1),)

    def host(hp, a, b):
        return ((a + b) if drop is None else (b.clone() if drop == 0 else a.clone()),)
    return ref, host


def _dlat(with_ed, drop_ed=False):
    def ref(hp, dy, w, *ed):
        v, m = W.linear_dgrad(dy, w)
        r = Ref(v, m, dy.shape[1])
        return (r.epilogue(base=ed[0]) if with_ed else r,)

    def host(hp, dy, w, *ed):
        return (dy @ w + ed[0] if with_ed and not drop_ed else dy @ w,)
    return ref, host


def _demb(nd, E_, drop=None):
    """The embedding's gradient = the scoring head's path + the generator-input slice [noise | EMBEDDING (| latent)]."""
    inner_ref, inner_host = _sum2(drop)
    return (lambda hp, head, dgin: inner_ref(hp, head, dgin[:, nd:nd + E_])), (lambda hp, head, dgin: inner_host(hp, head, dgin[:, nd:nd + E_]))


def _gelu_dgrad():
    """dx = (dy @ w) GELU'(z) mask."""
    def ref(hp, dy, w, z, mask):
        v, m = W.linear_dgrad(dy, w)
        f, fe = S.grad_factor(ACT_GELU, z.double())
        q = mask.double()
        return (mk(v * f * q, m * f.abs() * q.abs(), dy.shape[1], 2, v.abs() * fe * q.abs()),)

    def host(hp, dy, w, z, mask):
        return ((dy @ w) * S2.act_grad_ref(ACT_GELU, z) * mask,)
    return ref, host


def _ln_params():
    def ref(hp, dy, xhat):
        return S.layernorm_bwd_params(dy, xhat)

    def host(hp, dy, xhat):
        return ((dy * xhat).sum(0), dy.sum(0))
    return ref, host


def gen_backward_hp(B, T, pooled=False, exact_thirds=False):
    return dict(B=B, T=T, pooled=pooled, ds=critic_ds(B, exact_thirds)[B:2 * B].clone(), groups=1)


def gen_backward_table(hp, noise_dim, E_, notes_mode=True):
    """g_critic_front + g_critic_back + g_backward_b.  Critic tensors carry a g prefix: gA1 is GanEngine's A1[:B] during the
    generator step."""
    PD, PE, PG = (lambda k: "p.D." + k), (lambda k: "p.E." + k), (lambda k: "p.G." + k)  # noqa: E731
    GE_, GG = (lambda k: "g.E." + k), (lambda k: "g.G." + k)  # noqa: E731
    T, L3 = hp["T"], 8 * max(1, hp["T"] // 8)
    t, a = [], "notes"
    for nm, out in CRITIC_CONVS:
        t.append(Stage("critic forward", ["g" + out], [a, PD(nm + ".weight"), PD(nm + ".bias")], *_critic_conv()))
        a = "g" + out
    t += [Stage("critic forward", ["gH"], ["gA3"], *_pool("pooled")),
          Stage("critic forward", ["gFh"], ["gH", PD("fc.1.weight"), PD("fc.1.bias")], *linear(ACT_LRELU)),
          Stage("critic head", ["gs"], ["gFh", "emb", PD("real_fake.weight"), PD("real_fake.bias")], *_head()),
          Stage("critic head", ["adv"], ["gs"], *_scaled_mean(-1.0)),
          Stage("critic head", ["gdU"], ["gFh", PD("real_fake.weight")], *_head_bwd()),
          Stage("critic head", ["demb@head"], ["gFh", PD("real_fake.weight")], *_demb_head()),
          Stage("critic data gradient", ["gdH"], ["gdU", PD("fc.1.weight")], *linear_dgrad()),
          Stage("critic data gradient", ["gdZ3"], ["gdH", "gA3"], *_pool_bwd()),
          Stage("critic data gradient", ["gdZ2"], ["gdZ3", PD("conv.4.weight"), "gA2"], *_critic_dgrad()),
          Stage("critic data gradient", ["gdZ1"], ["gdZ2", PD("conv.2.weight"), "gA1"], *_critic_dgrad()),
          Stage("dnotes", ["dnotes"], ["gdZ1", PD("conv.0.weight"), "notes"] + (["dnotes@ed"] if notes_mode else []), *_dnotes(notes_mode))]
    dn = "dnotes"
    if L3 != T:     # the zero-padded tail rows carry no gradient (models.py:78-81)
        t.append(Stage("re-layout", ["dn_dense"], ["dnotes"], *relayout(lambda x: x[:, :L3])))
        dn = "dn_dense"
    for (src, i, da, a_, z_, dz_, j) in ((dn, 6, "d_ad3", "a_d3", "z_d3", "d_zd3", 1), ("d_zd3", 3, "d_ad0", "a_d0", "z_d0", "d_zd0", 0)):
        bn = f"decoder.deconv.{i - 2}"
        t.append(Stage("generator data gradient", [da], [src, PG(f"decoder.deconv.{i}.weight")], *convT_s2_dgrad()))
        t.append(Stage("generator BatchNorm backward", [dz_, GG(bn + ".weight"), GG(bn + ".bias")],
                       [da, a_, z_, PG(bn + ".weight"), PG(bn + ".bias"), f"bn_mean{j}", f"bn_invstd{j}"], *bn_back()))
    t += [Stage("generator data gradient", ["d_p2"], ["d_zd0", PG("decoder.deconv.0.weight"), "y0"], *_dp2()),
          Stage("generator weight gradient", [GG("decoder.pre.2.weight"), GG("decoder.pre.2.bias")], ["a_p0", "d_p2"], *linear_wgrad()),
          Stage("generator weight gradient", [GG("decoder.deconv.6.weight"), GG("decoder.deconv.6.bias")], ["a_d3", dn], *convT_s2_wgrad()),
          Stage("generator weight gradient", [GG("decoder.deconv.3.weight"), GG("decoder.deconv.3.bias")], ["a_d0", "d_zd3"], *convT_s2_wgrad()),
          Stage("generator weight gradient", [GG("decoder.deconv.0.weight"), GG("decoder.deconv.0.bias")], ["y0", "d_zd0"], *convT_s2_wgrad()),
          Stage("generator data gradient", ["d_p0"], ["d_p2", PG("decoder.pre.2.weight"), "a_p0"], *linear_dgrad(ACT_RELU)),
          Stage("d_lat", ["d_lat"], ["d_p0", PG("decoder.pre.0.weight")] + ([] if notes_mode else ["ed_dfeat"]), *_dlat(not notes_mode)),
          Stage("generator data gradient", ["d_n0"], ["d_lat", PG("noise_to_latent.net.2.weight"), "a_n0"], *linear_dgrad(ACT_RELU)),
          Stage("generator data gradient", ["d_gin"], ["d_n0", PG("noise_to_latent.net.0.weight")], *linear_dgrad()),
          Stage("demb", ["demb"], ["demb@head", "d_gin"], *_demb(noise_dim, E_)),
          Stage("numeric encoder data gradient", ["d_ez2"], ["demb", PE("net.7.weight"), "e_z2", "dmask1"], *_gelu_dgrad()),
          Stage("numeric encoder data gradient", ["d_ez1"], ["d_ez2", PE("net.4.weight"), "e_z1", "dmask0"], *_gelu_dgrad()),
          Stage("numeric encoder data gradient", ["d_ex0"], ["d_ez1", PE("net.1.weight")], *linear_dgrad()),
          Stage("numeric encoder weight gradient", [GE_("net.0.weight"), GE_("net.0.bias")], ["d_ex0", "e_xhat"], *_ln_params())]
    for x, dy, (g_, nm) in (("lat", "d_p0", (GG, "decoder.pre.0")), ("a_n0", "d_lat", (GG, "noise_to_latent.net.2")),
                            ("gin", "d_n0", (GG, "noise_to_latent.net.0")), ("e_h2", "demb", (GE_, "net.7")),
                            ("e_h1", "d_ez2", (GE_, "net.4")), ("e_x0", "d_ez1", (GE_, "net.1"))):
        sec = "generator weight gradient" if g_ is GG else "numeric encoder weight gradient"
        t.append(Stage(sec, [g_(nm + ".weight"), g_(nm + ".bias")], [x, dy], *linear_wgrad()))
    return t


# ---------------------------------------------------------------------------------------------------------------------
# the frozen emotion discriminator's branch of the generator step (oracle emotion_disc_fwd in eval mode + F.cross_entropy,
# weighted by LAMBDA_EMOTION: ed_model.py:24-46,61-69,86-95,147-165; train_gan.py:226-236): eval-mode BatchNorm folded with the
# convolution's bias into scale / shift (a stage of its own: the fold happens where parameters are written, not in a
# sub-step), four stride-1 convolutions with GELU, the mean over time, the projection, the MLP tail, the cross-entropy and
# every data gradient back to the generated notes (notes mode) or to the generator's latent (latent mode).
# ---------------------------------------------------------------------------------------------------------------------
def ed_chans(note_dim, hidden=256, blocks=4):
    """(Cin, Cout, K) of NotesEncoder's blocks (ed_model.py:52-58): 5 taps first, then 3; channels double up to `hidden`."""
    out, ci, co = [], note_dim, 64
    for i in range(blocks):
        out.append((ci, co, 5 if i == 0 else 3))
        ci, co = co, min(co * 2, hidden)
    return out


def _ed_fold():
    def ref(hp, gamma, beta, rm, rv, cb):
        return S.bn_fold(gamma, beta, rm, rv, cb, BN_EPS)

    def host(hp, gamma, beta, rm, rv, cb):
        s = gamma * (rv + f32(BN_EPS)) ** -0.5
        return (s, beta + (cb - rm) * s)
    return ref, host


def _conv_s1(x, w, flip=False):
    K = w.shape[2]
    if flip:
        return _ncl(F.conv_transpose1d(_ncl(x), w, None, 1, K // 2))
    return _ncl(F.conv1d(_ncl(x), w, None, 1, K // 2))


def _ed_conv(wino):
    """Conv1d(K, s1) -> folded BatchNorm (z kept) -> GELU.  wino: the launch computes by F(2,3) minimal filtering, whose
    magnitude and product count window_ref.wino3 states."""
    def ref(hp, x, w, scale, shift):
        K = w.shape[2]
        v, m, n = W.wino3(x, w) if wino else W.gather_s1(x, w, K) + (K * x.shape[2],)
        r = Ref(v, m, n).epilogue(scale=scale, shift=shift, zout=True)
        return (r.z, S.act_on(r, ACT_GELU))

    def host(hp, x, w, scale, shift):
        z = _conv_s1(x, w) * scale + shift
        return (z, F.gelu(z))
    return ref, host


def _ed_dgrad(wino, masked=True):
    """A block's input gradient: times GELU'(z) and the folded scale of the block below (none below the first)."""
    def ref(hp, dz, w, *zs):
        K = w.shape[2]
        v, m, n = W.wino3(dz, w, flip=True) if wino else W.gather_s1(dz, w, K, flip=True) + (K * dz.shape[2],)
        r = Ref(v, m, n)
        return (r.epilogue(gref=zs[0], gact=ACT_GELU, gscale=zs[1]) if masked else r,)

    def host(hp, dz, w, *zs):
        g = _conv_s1(dz, w, flip=True)
        return (g * S2.act_grad_ref(ACT_GELU, zs[0]) * zs[1] if masked else g,)
    return ref, host


def _ed_pool_bwd():
    def ref(hp, dh, z, scale):
        return (S.meanT_bwd(dh, z.shape[1], gref=z, gact=ACT_GELU, gscale=scale),)

    def host(hp, dh, z, scale):
        return ((dh / z.shape[1])[:, None, :] * S2.act_grad_ref(ACT_GELU, z) * scale,)
    return ref, host


def _gelu_linear_plain():
    def ref(hp, x, w, b):
        v, m = W.linear(x, w)
        r = Ref(v, m, x.shape[1]).epilogue(bias=b, zout=True)
        return (r.z, S.act_on(r, ACT_GELU))

    def host(hp, x, w, b):
        z = F.linear(x, w, b)
        return (z, F.gelu(z))
    return ref, host


def _gelu_dgrad_plain():
    def ref(hp, dy, w, z):
        v, m = W.linear_dgrad(dy, w)
        return (Ref(v, m, dy.shape[1]).epilogue(gref=z, gact=ACT_GELU),)

    def host(hp, dy, w, z):
        return ((dy @ w) * S2.act_grad_ref(ACT_GELU, z),)
    return ref, host


def _emotion_loss(weighted=True):
    """emo = F.cross_entropy(logits, target) (mean over the batch) and dlogits = lambda_emo (softmax - onehot) / B.
    weighted=False: the host's mistake of leaving lambda_emo / B out."""
    def ref(hp, logits, target):
        loss, dlog, _ = S.softmax_ce(logits, target, hp["lambda_emo"])
        return (loss, dlog)

    def host(hp, logits, target):
        p = torch.softmax(logits, 1)
        oh = F.one_hot(target, logits.shape[1]).to(logits.dtype)
        loss = -(torch.log_softmax(logits, 1) * oh).sum(1).mean().reshape(1)
        return (loss, f32(hp["lambda_emo"]) * (p - oh) / logits.shape[0] if weighted else p - oh)
    return ref, host


# ---- the bf16 variant (ed_dtype="bf16"): activations and weight images stored in bf16, fp32 accumulation; operands enter as
# the kernel multiplies them (bf16_ref.q), a bf16 output is the fp32 bound seen through one rounding (bf16_ref.Out16) ----
def _ed_conv_bf16():
    def ref(hp, x, w, scale, shift):
        import bf16_ref as B16
        r = B16.conv(x, w, w.shape[2]).epilogue(scale=scale, shift=shift, zout=True)
        z = r.z
        return (B16.Out16(z), B16.Out16(S.act_on(r, ACT_GELU)))

    def host(hp, x, w, scale, shift):
        import bf16_ref as B16
        z = B16.conv_fp32_host(x, w, w.shape[2]) * scale.float() + shift.float()
        return (z.to(B16.BF), F.gelu(z).to(B16.BF))
    return ref, host


def _ed_dgrad_bf16(masked=True):
    def ref(hp, dz, w, *zs):
        import bf16_ref as B16
        r = B16.conv(dz, w, w.shape[2], flip=True)
        return (B16.Out16(r.epilogue(gref=B16.q(zs[0]), gact=ACT_GELU, gscale=zs[1])) if masked else r,)

    def host(hp, dz, w, *zs):
        import bf16_ref as B16
        g = B16.conv_fp32_host(dz, w, w.shape[2], flip=True)
        return ((g * S2.act_grad_ref(ACT_GELU, zs[0].float()) * zs[1].float()).to(B16.BF) if masked else g,)
    return ref, host


def _ed_pool_bf16():
    def ref(hp, a):
        import bf16_ref as B16
        return (B16.meanT_fwd(a),)

    def host(hp, a):
        return (a.float().mean(1),)
    return ref, host


def _ed_pool_bwd_bf16():
    def ref(hp, dh, z, scale):
        import bf16_ref as B16
        return (B16.meanT_bwd(dh, z.shape[1], z, ACT_GELU, scale),)

    def host(hp, dh, z, scale):
        import bf16_ref as B16
        return (((dh.float() / z.shape[1])[:, None, :] * S2.act_grad_ref(ACT_GELU, z.float()) * scale.float()).to(B16.BF),)
    return ref, host


def ed_fold_table(chans):
    t = []
    for i in range(len(chans)):
        pre = f"encoder.conv.{i}.net"
        t.append(Stage("emotion branch fold", [f"ed_scale{i}", f"ed_shift{i}"],
                       ["p.ED." + pre + ".1.weight", "p.ED." + pre + ".1.bias", "b.ED." + pre + ".1.running_mean", "b.ED." + pre + ".1.running_var",
                        "p.ED." + pre + ".0.bias"], *_ed_fold()))
    return t


def ed_hp(B, lambda_emo=5.0):
    return dict(B=B, lambda_emo=lambda_emo)


def ed_branch_table(chans, n_hidden=2, notes_mode=True, wino_f=None, wino_d=None, bf16=False):
    """g_ed_branch.  chans: ed_chans(note_dim) (notes mode).  wino_f / wino_d: per block, whether the forward / the data
    gradient launch is the F(2,3) kernel.  Output of the branch: dnotes@ed (notes mode) or ed_dfeat (latent mode)."""
    P = lambda k: "p.ED." + k  # noqa: E731
    L = len(chans) if notes_mode else 0
    wino_f, wino_d = list(wino_f or [False] * L), list(wino_d or [False] * L)
    t, feat = [], "lat"
    if notes_mode:
        a = "notes"
        for i in range(L):
            t.append(Stage("emotion branch convolution", [f"ed_z{i}", f"ed_a{i}"],
                           [a, P(f"encoder.conv.{i}.net.0.weight"), f"ed_scale{i}", f"ed_shift{i}"], *(_ed_conv_bf16() if bf16 else _ed_conv(wino_f[i]))))
            a = f"ed_a{i}"
        t.append(Stage("emotion branch tail", ["ed_pool"], [a], *(_ed_pool_bf16() if bf16 else _pool("_never"))))
        t.append(Stage("emotion branch tail", ["ed_proj"], ["ed_pool", P("encoder.project.weight"), P("encoder.project.bias")], *linear()))
        feat = "ed_proj"
    x = feat
    for j in range(n_hidden):
        t.append(Stage("emotion branch tail", [f"ed_cz{j}", f"ed_ca{j}"], [x, P(f"classifier.net.{3 * j}.weight"), P(f"classifier.net.{3 * j}.bias")],
                       *_gelu_linear_plain()))
        x = f"ed_ca{j}"
    t.append(Stage("emotion branch tail", ["logits"], [x, P("classifier.head.weight"), P("classifier.head.bias")], *linear()))
    t.append(Stage("emotion loss", ["emo", "dlogits"], ["logits", "emot_idx"], *_emotion_loss()))
    g = "dlogits"
    ws = [P(f"classifier.net.{3 * j}.weight") for j in range(n_hidden)] + [P("classifier.head.weight")]
    for j in range(n_hidden - 1, -1, -1):
        t.append(Stage("emotion branch tail gradient", [f"ed_dcz{j}"], [g, ws[j + 1], f"ed_cz{j}"], *_gelu_dgrad_plain()))
        g = f"ed_dcz{j}"
    if not notes_mode:
        t.append(Stage("emotion branch tail gradient", ["ed_dfeat"], [g, ws[0]], *linear_dgrad()))
        return t
    t.append(Stage("emotion branch tail gradient", ["ed_dproj"], [g, ws[0]], *linear_dgrad()))
    t.append(Stage("emotion branch tail gradient", ["ed_dpool"], ["ed_dproj", P("encoder.project.weight")], *linear_dgrad()))
    t.append(Stage("emotion branch data gradient", [f"ed_dz{L - 1}"], ["ed_dpool", f"ed_z{L - 1}", f"ed_scale{L - 1}"],
                   *(_ed_pool_bwd_bf16() if bf16 else _ed_pool_bwd())))
    for i in range(L - 1, 0, -1):
        t.append(Stage("emotion branch data gradient", [f"ed_dz{i - 1}"],
                       [f"ed_dz{i}", P(f"encoder.conv.{i}.net.0.weight"), f"ed_z{i - 1}", f"ed_scale{i - 1}"],
                       *(_ed_dgrad_bf16() if bf16 else _ed_dgrad(wino_d[i]))))
    t.append(Stage("emotion branch data gradient", ["dnotes@ed"], ["ed_dz0", P("encoder.conv.0.net.0.weight")],
                   *(_ed_dgrad_bf16(masked=False) if bf16 else _ed_dgrad(wino_d[0], masked=False))))
    return t
