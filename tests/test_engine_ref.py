"""Host self-test of tests/engine_ref.py (no GPU): (a) every table, evaluated in fp64 from the batch, the parameters and
the injected randoms alone, equals the oracle's autograd step; (b) an fp32 host evaluation of every table, stage by stage from
fp32-stored upstream tensors, stays inside every bound for two free-running steps; (c) plausible wiring mistakes, built from
the fp64 table, leave the bound of the stage they belong to and of no other; (d) the tables reach the branches
tests/test_engine_contract_gpu.py asserts.  The ratios of (b) and (c) are printed (pytest -s) and quoted in DESIGN.md §2."""
import math
from collections import OrderedDict

import pytest
import torch

import engine_ref as E
import support_ref as S
from oracle import melo_oracle as O

FP32, MISTAKES = OrderedDict(), OrderedDict()
U64 = S.U64
# (a): both sides start from the batch, so -- unlike the per-stage contract -- their fp64 roundings do compound.  What the
# multiple counts: a sum of up to 128 * 4 * 5 = 2560 products (encoder._linear at T = 32, the widest: 2^11.3), times the
# conditioning of a BatchNorm over 12..128 rows of nearly constant closed-form activations, 1 / sqrt(var + eps) with var down
# to 1e-5 (2^8.3 on unit-scale data), and the tolerance is relative to the COMPARED tensor's largest value, which for a
# running mean or an Adam update is up to 2^-2 of the tensors it is computed from: 2^18 in all.  The largest multiple the
# comparisons reach is 2^16.8 (a decoder running mean in step 2); 2^14 fails two of them.  2^18 x 2^-53 is 2^-11 of ONE fp32
# rounding: nothing an fp32 contract could see hides under it.
K64 = 2.0 ** 18


def note(table, key, r):
    table[key] = max(table.get(key, 0.0), r)


def teardown_module(module):
    for name, tab in (("fp32 host evaluation, worst error / bound", FP32), ("mistakes, worst error / bound of the stage", MISTAKES)):
        print(f"\n[engine ref] {name}")
        for k, v in tab.items():
            print(f"    {k}: {v:.4g}")


def close64(a, b, what, extra=0.0, mag=0.0):
    """mag: the stage magnitude M of the table's row (engine_ref.evaluate(mags=...)): a gradient that cancels (BatchNorm over
    a dozen rows) is small against it, and so is either side's rounding."""
    a, b = a.double(), b.double()
    assert tuple(a.shape) == tuple(b.shape), (what, tuple(a.shape), tuple(b.shape))
    tol = K64 * U64 * max(float(b.abs().max()), mag) + extra
    err = float((a - b).abs().max()) if a.numel() else 0.0
    assert err <= tol, f"{what}: |table - oracle| {err:.3e} > {tol:.3e}"


PRE_BN_BIAS = {"encoder.conv.0.bias": "g_ez0", "encoder.conv.3.bias": "g_ez1", "encoder.conv.6.bias": "g_ez2",
               "decoder.deconv.0.bias": "g_dz0", "decoder.deconv.3.bias": "g_dz1"}


def vae_problem(B, T, latent, dtype=torch.float32):
    spec, bufs = O.vae_spec(T, latent)
    P = O.fill_params(spec, 6.0, O.norm_affine_names(spec))
    Bf = O.fill_buffers(bufs)
    g = torch.Generator().manual_seed(5)
    xs = [torch.rand(B, T, 4, generator=g) * 2 - 1 for _ in range(2)]
    es = [torch.randn(B, latent, generator=g) for _ in range(2)]
    return spec, bufs, P, Bf, xs, es


@pytest.fixture(autouse=True)
def oracle_takes_fp32_scalars(monkeypatch):
    """The kernels receive eps, momentum and LeakyReLU's slope as fp32 values and the references compute from those (support_ref.f32): so
    does the oracle here, or the two would differ by the rounding of 1e-5 and 0.1 rather than by fp64 roundings."""
    monkeypatch.setattr(O, "BN_EPS", S.f32(1e-5))
    monkeypatch.setattr(O, "BN_MOMENTUM", S.f32(0.1))
    monkeypatch.setattr(O, "LN_EPS", S.f32(1e-5))
    real = torch.nn.functional.leaky_relu
    # ... and LeakyReLU's slope: 0.2f on the device, forward and backward
    monkeypatch.setattr(torch.nn.functional, "leaky_relu", lambda x, negative_slope=0.01, inplace=False: real(x, S.f32(negative_slope), inplace))


# ---------------------------------------------------------------------------------------------------------------------
# (a) the tables against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", E.VAE_CONFIGS, ids=str)
def test_vae_tables_equal_the_oracle(cfg):
    B, T, latent = cfg
    spec, bufs, P, Bf, xs, es = vae_problem(*cfg)
    hp = E.vae_hp(B, T, latent)
    tables = E.vae_tables(spec, hp)
    P64 = OrderedDict((k, v.double().clone()) for k, v in P.items())
    B64 = OrderedDict((k, v.double().clone()) for k, v in Bf.items())
    f = S.f32
    opt = O.AdamState(P64, f(hp["lr"]), (f(0.9), f(0.999)), f(1e-8), weight_decay=f(hp["wd"]), decoupled=True)
    pre = E.vae_initial(spec, bufs, P, Bf, xs[0], es[0])
    for it in range(2):
        pre["x"], pre["eps"] = xs[it], es[it]
        post, ratios = E.vae_step(tables, spec, pre, hp, torch.float64, carry="ref")
        # the two formulations of every stage (unfold + einsum Refs, torch.nn.functional + autograd) agree in fp64
        for flow, rs in ratios.items():
            for n, r in rs.items():
                assert r < 1e-6, (it, flow, n, r)
        _, z, mu, lv = O.vae_fwd(P64, {k: v.clone() for k, v in B64.items()}, xs[it].double(), es[it].double(), T, True)
        r = O.ae_step(P64, B64, opt, xs[it].double(), es[it].double(), hp["beta"], T)
        what = f"{cfg} step {it + 1} "
        close64(post["recon"], r["recon"], what + "recon")
        close64(post["mu"], r["mu"], what + "mu")
        close64(post["lv"], r["log_var"], what + "lv")
        close64(post["zl"], z, what + "zl")
        close64(post["loss"], torch.stack([r["loss"], r["recon_loss"], r["kld"]]), what + "loss")
        for k in spec:
            # a pre-BatchNorm bias has a zero gradient: both sides hold the rounding noise of a column sum of dz, so the
            # magnitude is that of the summands
            extra = K64 * U64 * float(post[PRE_BN_BIAS[k]].abs().sum()) if k in PRE_BN_BIAS else 0.0
            close64(post["g." + k], r["grads"][k], what + "gradient " + k, extra)
        close64(post["gnorm"][0], r["grad_norm"], what + "gradient norm")      # fp64 here: the norm of the per-tensor norms
        for k in spec:
            # Adam divides by sqrt(v) + 1e-8: where the gradient is rounding noise around zero (the pre-BatchNorm biases) the
            # two sides' noise reaches the parameter amplified by up to lr / (1 - beta1^t) / 1e-8.  (The per-stage contract
            # has no such term: it references the update from the stored gradient.)
            extra = hp["lr"] / (1.0 - 0.9 ** (it + 1)) / 1e-8 * K64 * U64 * float(post[PRE_BN_BIAS[k]].abs().sum()) if k in PRE_BN_BIAS else 0.0
            close64(post["p." + k], P64[k], what + "updated " + k, extra)
        for k in bufs:
            close64(post["b." + k], B64[k], what + "running " + k)
        assert float(post["P.state"][0]) == it + 1 == opt.t
        pre = post


# ---------------------------------------------------------------------------------------------------------------------
# (b) fp32 host evaluation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", E.VAE_CONFIGS, ids=str)
def test_vae_fp32_host_evaluation_stays_inside_the_bounds(cfg):
    B, T, latent = cfg
    spec, bufs, P, Bf, xs, es = vae_problem(*cfg)
    hp = E.vae_hp(B, T, latent)
    tables = E.vae_tables(spec, hp)
    section = {n: st.section for flow in tables.values() for st in flow for n in st.outs}
    pre = E.vae_initial(spec, bufs, P, Bf, xs[0], es[0])
    for it in range(2):
        pre["x"], pre["eps"] = xs[it], es[it]
        post, ratios = E.vae_step(tables, spec, pre, hp, torch.float32)
        for flow, rs in ratios.items():
            for n, r in rs.items():
                note(FP32, "VAE " + section[n], r)
                assert r < 1.0, (cfg, it, flow, n, r)
        pre = post


# ---------------------------------------------------------------------------------------------------------------------
# (c) plausible wiring mistakes
# ---------------------------------------------------------------------------------------------------------------------
def _flat_prefix(hp, t):
    B, L = t.shape[0], hp["Ld"][3]
    return (t.reshape(-1)[:B * L * 4].view(B, L, 4).clone(),)


VAE_MISTAKES = OrderedDict([
    # name: (configuration, step (1 or 2), stage name, replacement host function)
    ("g_h without the fc_log_var path", ((4, 32, 8), 1, "g_h@sum", lambda hp, d1, w1, d2, w2: (d1 @ w1,))),
    ("g_h: accumulate off (fc_mu path overwritten)", ((4, 32, 8), 1, "g_h@sum", lambda hp, d1, w1, d2, w2: (d2 @ w2,))),
    ("g_mu / g_lv without the KLD gradients", ((4, 32, 8), 1, "g_mu+g_lv", E._reparam_bwd(kld=False)[1])),
    ("KLD gradients without beta", ((4, 32, 8), 1, "loss+g_recon@loss+k_mu+k_lv",
                                    lambda hp, *a: E._vae_loss_host(hp, *a)[:2] + E._vae_loss_host(dict(hp, beta=1.0), *a)[2:])),
    ("tanh' taken at the target, not at recon", ((4, 32, 8), 1, "g_recon", lambda hp, dy, r: (dy,))),
    ("flat in (B, L, 128) order (no transpose)", ((4, 32, 8), 1, "flat", lambda hp, t: (t.reshape(t.shape[0], -1).clone(),))),
    ("g_rec_dense: flat prefix, not each sample's first rows (T = 20)", ((4, 20, 8), 1, "g_rec_dense", _flat_prefix)),
    ("recon: padding rows written (tanh of the bias) (T = 20)", ((4, 20, 8), 1, "recon",
                                                              lambda hp, x, w, b: (torch.cat([E.convT_s2(E.ACT_TANH)[1](hp, x, w, b)[0],
                                                                                              torch.tanh(b).expand(x.shape[0], hp["T"] - 2 * x.shape[1], 4)], 1),))),
    ("running statistics moved twice", ((4, 32, 8), 1, "e_mean1+e_istd1+ea1+b.encoder.conv.4.running_mean+b.encoder.conv.4.running_var",
                                        lambda hp, *a: E.bn_train()[1](hp, *a, moves=2))),
    ("Adam: grad_scale doubled", ((4, 32, 8), 2, "P.data+P.m+P.v+P.state", E._adam(E.VAE_ADAM, scale=2.0)[1])),
    ("Adam: step state advanced twice", ((4, 32, 8), 2, "P.data+P.m+P.v+P.state", E._adam(E.VAE_ADAM, advance=2)[1])),
    ("Adam: the clip coefficient ignored", ((4, 32, 8), 2, "P.data+P.m+P.v+P.state", E._adam(E.VAE_ADAM, use_clip=False)[1])),
])


@pytest.mark.parametrize("name", list(VAE_MISTAKES), ids=lambda s: s.replace(" ", "_"))
def test_vae_wiring_mistakes_leave_their_stage(name):
    cfg, step, stage, fn = VAE_MISTAKES[name]
    B, T, latent = cfg
    spec, bufs, P, Bf, xs, es = vae_problem(*cfg)
    hp = E.vae_hp(B, T, latent)
    tables = E.vae_tables(spec, hp)
    assert any(st.name == stage for flow in tables.values() for st in flow), stage
    pre = E.vae_initial(spec, bufs, P, Bf, xs[0], es[0])
    for it in range(step):
        pre["x"], pre["eps"] = xs[it], es[it]
        post, ratios = E.vae_step(tables, spec, pre, hp, torch.float64, mutate={stage: fn} if it == step - 1 else None)
        pre = post
    flat = {n: r for rs in ratios.values() for n, r in rs.items()}
    mine = max(flat[n] for n in stage.split("+"))
    note(MISTAKES, "VAE " + name, mine)
    assert mine > 1.0, (name, {n: flat[n] for n in stage.split("+")})
    # every other stage is referenced from its own (now wrong) upstream and stays clean: the contract names the stage
    others = {n: r for n, r in flat.items() if n not in stage.split("+")}
    assert max(others.values()) < 1e-3, (name, max(others, key=others.get), max(others.values()))


def test_vae_clip_is_active_at_the_table_configurations():
    """The clip coefficient is a stage input of AdamW; it is only visible where the norm exceeds 1."""
    for cfg in E.VAE_CONFIGS:
        spec, bufs, P, Bf, xs, es = vae_problem(*cfg)
        hp = E.vae_hp(*cfg)
        post, _ = E.vae_step(E.vae_tables(spec, hp), spec, E.vae_initial(spec, bufs, P, Bf, xs[0], es[0]), hp)
        assert float(post["gnorm"][0]) > 1.0 > float(post["gnorm"][1]), (cfg, post["gnorm"])


# ---------------------------------------------------------------------------------------------------------------------
# the GAN's two optimiser updates: (a), (b), (c) as above
# ---------------------------------------------------------------------------------------------------------------------
def gan_oracle_state(C, T, B):
    """The oracle's GAN state in fp64 with the fp32 values of the learning rates, betas and eps the kernels receive."""
    f = S.f32
    cfg, ed_cfg = O.default_gan_cfg(B, T, C), O.default_ed_cfg(C)
    cfg.update(LR_G=f(cfg["LR_G"]), LR_D=f(cfg["LR_D"]), BETA1=f(cfg["BETA1"]), BETA2=f(cfg["BETA2"]))
    S0 = O.build_gan_state(cfg, ed_cfg, "closed_form", d_scale=6.0)
    d64 = lambda dct: OrderedDict((k, v.double().clone()) for k, v in dct.items())  # noqa: E731
    S64 = O.GanState(cfg, ed_cfg, d64(S0.PE), d64(S0.PG), d64(S0.BG), d64(S0.PD), d64(S0.PED), d64(S0.BED))
    S64.opt_D.eps = S64.opt_G.eps = f(1e-8)
    return cfg, S64


def gan_update_problem(cfg, S64, X):
    spec = OrderedDict((k, tuple(v.shape)) for k, v in (S64.PD if X == "D" else S64.PGE).items())
    table = E.gan_update_table(X, spec, transposed_conv=(X == "GE"))
    hp = E.gan_update_hp(cfg["LR_D" if X == "D" else "LR_G"])
    return spec, table, hp


def gan_oracle_steps(C, T, B, n_steps=2):
    """Yields (X, spec, table, hp, named parameters before, gradients, named parameters after) for every update of n_steps
    oracle steps (critic, then generator), all fp64."""
    cfg, S64 = gan_oracle_state(C, T, B)
    real, numeric, latent, emot = O.synthetic_batch(B, T, C, cfg["LATENT_DIM"], 6, 7)
    for it in range(n_steps):
        R = O.step_randoms(B, cfg["NOISE_DIM"], seed=1 + it)
        for X in ("D", "GE"):
            P = S64.PD if X == "D" else S64.PGE
            before = OrderedDict((k, v.detach().clone()) for k, v in P.items())
            if X == "D":
                r = O.d_step(S64, real.double(), latent.double(), numeric.double(), R["noise_d"].double(), R["alpha"].double(), R["dm_d"])
            else:
                r = O.g_step(S64, latent.double(), numeric.double(), emot, R["noise_g"].double(), R["dm_g"])
            yield (X,) + gan_update_problem(cfg, S64, X) + (before, r["grads"], OrderedDict((k, v.detach().clone()) for k, v in P.items()))


@pytest.mark.parametrize("cfg", E.GAN_UPDATE_CONFIGS, ids=str)
def test_gan_update_tables_equal_the_oracle_and_fp32_stays_inside(cfg):
    state = {}
    for X, spec, table, hp, before, grads, after in gan_oracle_steps(*cfg):
        if X not in state:
            flat = E.flat_of(spec, before, "", torch.float64)
            state[X] = {f"{X}.data": flat, f"{X}.m": torch.zeros_like(flat), f"{X}.v": torch.zeros_like(flat),
                        f"{X}.state": torch.zeros(4, dtype=torch.float64)}
        pre = dict(state[X])
        pre[f"{X}.grad"] = E.flat_of(spec, grads, "", torch.float64)
        close64(pre[f"{X}.data"], E.flat_of(spec, before, "", torch.float64), f"{cfg} {X} parameters before")
        post, ratios = E.evaluate(table, pre, hp, torch.float64, carry="ref")
        assert max(ratios.values()) < 1e-6, ratios
        for k in spec:
            close64(post["p." + k], after[k], f"{cfg} {X} updated {k}")
        # (b) the same update in fp32 from the fp32-stored state
        _, r32 = E.evaluate(table, pre, hp, torch.float32)
        for n, r in r32.items():
            note(FP32, "GAN " + {st_.outs[0]: st_.section for st_ in table}.get(n, "Adam" if n.startswith(X + ".") else "re-layout"), r)
            assert r < 1.0, (cfg, X, n, r)
        state[X] = {k: post[k] for k in state[X]}
    # the copies the tables cover: the critic's three convolutions in both directions bar conv.0's thin side(s), the
    # generator's three deconvolutions likewise
    C = cfg[0]
    _, S64 = gan_oracle_state(*cfg)
    plans = {X: [(n, d) for n, d, *_ in E.wq_plan(gan_update_problem(O.default_gan_cfg(cfg[2], cfg[1], C), S64, X)[0], X == "GE")] for X in ("D", "GE")}
    assert ("conv.0.weight", "fwd") in plans["D"] if C % 16 == 0 else ("conv.0.weight", "fwd") not in plans["D"]
    assert {("conv.2.weight", "fwd"), ("conv.2.weight", "dgrad"), ("conv.4.weight", "fwd"), ("conv.4.weight", "dgrad")} <= set(plans["D"])
    assert {("G.decoder.deconv.0.weight", "fwd"), ("G.decoder.deconv.3.weight", "dgrad")} <= set(plans["GE"])
    assert (("G.decoder.deconv.6.weight", "fwd") in plans["GE"]) == (C % 32 == 0)


GAN_UPDATE_MISTAKES = OrderedDict([
    ("Adam: grad_scale doubled", ("D.data+D.m+D.v+D.state", lambda stale: E._adam(E.GAN_ADAM, scale=2.0)[1])),
    ("Adam: step state advanced twice", ("D.data+D.m+D.v+D.state", lambda stale: E._adam(E.GAN_ADAM, advance=2)[1])),
    ("step 2 with step 1's re-laid conv.2 weights", ("wq.conv.2.weight.fwd", lambda stale: (lambda hp, w: (S.wq_layout(stale.reshape(-1), 128, 64, 5, False),)))),
])


@pytest.mark.parametrize("name", list(GAN_UPDATE_MISTAKES), ids=lambda s: s.replace(" ", "_"))
def test_gan_update_mistakes_leave_their_stage(name):
    stage, make = GAN_UPDATE_MISTAKES[name]
    steps = [t for t in gan_oracle_steps(4, 32, 4) if t[0] == "D"]
    X, spec, table, hp, before, grads, _ = steps[0]
    flat = E.flat_of(spec, before, "", torch.float64)
    pre = {"D.data": flat, "D.m": torch.zeros_like(flat), "D.v": torch.zeros_like(flat), "D.state": torch.zeros(4, dtype=torch.float64),
           "D.grad": E.flat_of(spec, grads, "", torch.float64)}
    pre, _ = E.evaluate(table, pre, hp)                                  # step 1, clean
    stale = pre["p.conv.2.weight"]
    pre["D.grad"] = E.flat_of(spec, steps[1][5], "", torch.float64)
    _, ratios = E.evaluate(table, pre, hp, mutate={stage: make(stale)})  # step 2, with the mistake
    mine = max(ratios[n] for n in stage.split("+"))
    note(MISTAKES, "GAN " + name, mine)
    assert mine > 1.0, (name, mine)
    assert max(r for n, r in ratios.items() if n not in stage.split("+")) < 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# the critic step's critic part: (a), (b), (c)
# ---------------------------------------------------------------------------------------------------------------------
def critic_problem(C, T, B, exact_thirds):
    """(hp, table, pre, the oracle's d_step result) of the first critic step: the fake batch and the embedding are the
    oracle's (the generator's forward has its own table and test), everything behind them is the table's."""
    cfg, S64 = gan_oracle_state(C, T, B)
    real, numeric, latent, emot = O.synthetic_batch(B, T, C, cfg["LATENT_DIM"], 6, 7)
    R = O.step_randoms(B, cfg["NOISE_DIM"], seed=1)
    pre = {"p." + k: v.detach().clone() for k, v in S64.PD.items()}
    r = O.d_step(S64, real.double(), latent.double(), numeric.double(), R["noise_d"].double(), R["alpha"].double(), R["dm_d"])
    pre.update(real=real.double(), fake_d=r["fake"].detach(), emb_d=r["emb"].detach(), alpha=R["alpha"].double().reshape(-1))
    hp = E.critic_hp(B, T, cfg["LAMBDA_GP"], exact_thirds=exact_thirds)
    return hp, E.critic_table(hp), pre, r


@pytest.mark.parametrize("cfg", E.GAN_CRITIC_CONFIGS, ids=str)
def test_critic_table_equals_the_oracle(cfg):
    C, T, B = cfg
    hp, table, pre, r = critic_problem(C, T, B, exact_thirds=True)
    post, ratios = E.evaluate(table, pre, hp, torch.float64, carry="ref")
    assert max(ratios.values()) < 1e-6, {n: v for n, v in ratios.items() if v >= 1e-6}
    what = f"{cfg} "
    close64(post["s"][B:2 * B], r["d_real"].reshape(-1), what + "D(real)")
    close64(post["s"][2 * B:], r["d_fake"].reshape(-1), what + "D(fake)")
    close64(post["gp"], r["gp"].reshape(1), what + "gp")
    close64(post["loss_d_out"][0], r["loss_d"], what + "loss_d")
    for k, g in r["grads"].items():
        close64(post["g." + k], g, what + "gradient " + k)


@pytest.mark.parametrize("cfg", E.GAN_CRITIC_CONFIGS, ids=str)
def test_critic_fp32_host_evaluation_stays_inside_the_bounds(cfg):
    C, T, B = cfg
    hp, table, pre, _ = critic_problem(C, T, B, exact_thirds=False)
    section = {n: st.section for st in table for n in st.outs}
    for pooled in (False, True):
        hp.update(pooled=pooled, pooled_tan=pooled)
        _, ratios = E.evaluate(table, pre, hp, torch.float32)
        for n, v in ratios.items():
            note(FP32, "GAN " + section[n], v)
            assert v < 1.0, (cfg, n, v)


CRITIC_MISTAKES = OrderedDict([
    ("ds_d: real and fake swapped", ((4, 32, 4), "dU", E._head_bwd(lambda hp: torch.cat([hp["ds"][:hp["B"]], hp["ds"][2 * hp["B"]:], hp["ds"][hp["B"]:2 * hp["B"]]]))[1])),
    ("ds_d swapped in the head's weight gradient", ((4, 32, 4), "g.real_fake.weight+g.real_fake.bias+loss_d_out+gp", E._critic_head_wgrad(swap=True)[1])),
    ("conv.2 weight gradient: tangent contribution dropped", ((4, 32, 4), "g.conv.2.weight+g.conv.2.bias", E._critic_conv_wgrad(tangent=False)[1])),
    ("dZ1: gref from rows [B:2B] instead of its own", ((4, 32, 4), "dZ1", lambda hp, dy, w, a: (
        E._critic_dgrad()[1](hp, dy, w, torch.cat([a[hp["B"]:2 * hp["B"]], a[:hp["B"]], a[2 * hp["B"]:]]))[0],))),
    ("TAN1: mask of the real rows, not x_hat's", ((4, 32, 4), "TAN1", E._tangent_conv(other_rows=True)[1])),
    ("x_hat with alpha on the fake batch", ((4, 32, 4), "xhat", lambda hp, real, fake, alpha: E._interp()[1](hp, fake, real, alpha))),
    ("gx from the real rows", ((4, 20, 3), "gx", lambda hp, dy, w, a: E._critic_dgrad(lambda h: h["B"], masked=False)[1](hp, dy[hp["B"]:], w, a))),
    ("fc.1 weight gradient without the tangent segment", ((4, 32, 4), "g.fc.1.weight+g.fc.1.bias",
                                                        lambda hp, h, du, ghb: (du[hp["B"]:].t() @ h[hp["B"]:], du[hp["B"]:].sum(0)))),
])


@pytest.mark.parametrize("name", list(CRITIC_MISTAKES), ids=lambda s: s.replace(" ", "_"))
def test_critic_wiring_mistakes_leave_their_stage(name):
    cfg, stage, fn = CRITIC_MISTAKES[name]
    hp, table, pre, _ = critic_problem(*cfg, exact_thirds=False)
    assert any(st.name == stage for st in table), stage
    _, ratios = E.evaluate(table, pre, hp, torch.float64, mutate={stage: fn})
    mine = max(ratios[n] for n in stage.split("+"))
    note(MISTAKES, "GAN " + name, mine)
    assert mine > 1.0, (name, {n: ratios[n] for n in stage.split("+")})
    others = {n: v for n, v in ratios.items() if n not in stage.split("+")}
    assert max(others.values()) < 1e-3, (name, max(others, key=others.get))


# ---------------------------------------------------------------------------------------------------------------------
# the numeric encoder's and the generator's forward, one group and two: (a), (b), (c)
# ---------------------------------------------------------------------------------------------------------------------
def forward_problem(C, T, B, conditioning=False):
    cfg, S64 = gan_oracle_state(C, T, B)
    if conditioning:
        cfg = dict(cfg, INTEGRATION_MODE="conditioning")
        S0 = O.build_gan_state(cfg, O.default_ed_cfg(C), "closed_form", d_scale=6.0)
        d64 = lambda dct: OrderedDict((k, v.double().clone()) for k, v in dct.items())  # noqa: E731
        S64 = O.GanState(cfg, S0.ed_cfg, d64(S0.PE), d64(S0.PG), d64(S0.BG), d64(S0.PD), d64(S0.PED), d64(S0.BED))
    real, numeric, latent, emot = O.synthetic_batch(B, T, C, cfg["LATENT_DIM"], 6, 7)
    latent = latent + torch.randn(latent.shape, generator=torch.Generator().manual_seed(3))       # the synthetic latent is zero
    R = O.step_randoms(B, cfg["NOISE_DIM"], seed=1)
    pre = {"p.E." + k: v.clone() for k, v in S64.PE.items()}
    pre.update({"p.G." + k: v.clone() for k, v in S64.PG.items()})
    pre.update({"b." + k: v.clone() for k, v in S64.BG.items()})
    halves = {}
    for h in ("d", "g"):
        halves[h] = dict(numeric=numeric.double(), noise=R["noise_" + h].double(), dmask0=R["dm_" + h][0].double() * 1.25,
                         dmask1=R["dm_" + h][1].double() * 1.25)
    pre["latent"] = latent.double()
    return cfg, S64, pre, halves, (real, numeric, latent, emot, R)


def oracle_forward(cfg, S64, numeric, latent, noise, dm):
    emb = O.feature_encoder_fwd(S64.PE, numeric.double(), dm)
    fake, lat = O.generator_fwd(S64.PG, S64.BG, noise.double(), latent.double(), emb, cfg["INTEGRATION_MODE"], cfg["MAX_NOTES"], train=True)
    return emb, fake, lat


FORWARD_CONFIGS = ((4, 32, 4, False), (4, 20, 3, False), (4, 16, 3, True))


@pytest.mark.parametrize("cfg4", FORWARD_CONFIGS, ids=str)
def test_forward_tables_equal_the_oracle_one_group_and_two(cfg4):
    C, T, B, cond = cfg4
    cfg, S64, pre, halves, (real, numeric, latent, emot, R) = forward_problem(C, T, B, cond)
    table1 = E.gen_forward_table(E.gen_forward_hp(B, T, 1), cond)
    table2 = E.gen_forward_table(E.gen_forward_hp(B, T, 2), cond)
    both = {k: torch.cat([halves["d"][k], halves["g"][k]], 0) for k in halves["d"]}
    post2, r2 = E.evaluate(table2, dict(pre, **both), E.gen_forward_hp(B, T, 2), torch.float64, carry="ref")
    assert max(r2.values()) < 1e-6, r2
    cur = dict(pre)
    for gi, h in enumerate(("d", "g")):
        cur, r1 = E.evaluate(table1, dict(cur, **halves[h]), E.gen_forward_hp(B, T, 1), torch.float64, carry="ref")
        assert max(r1.values()) < 1e-6, r1
        emb, fake, lat = oracle_forward(cfg, S64, numeric, latent, R["noise_" + h], R["dm_" + h])     # moves S64.BG
        for name, want in (("emb", emb), ("notes", fake), ("lat", lat)):
            close64(cur[name], want, f"{cfg4} half {h} {name}")
            close64(post2[name][gi * B:(gi + 1) * B], want, f"{cfg4} 2B-row pass, group {gi} {name}")
    for k in S64.BG:
        close64(cur["b." + k], S64.BG[k], f"{cfg4} running {k} after both halves")
        close64(post2["b." + k], S64.BG[k], f"{cfg4} running {k} after the 2B-row pass")
    # (b) fp32
    for table, hp, inp in ((table1, E.gen_forward_hp(B, T, 1), halves["g"]), (table2, E.gen_forward_hp(B, T, 2), both)):
        section = {n: st.section for st in table for n in st.outs}
        _, r32 = E.evaluate(table, dict(pre, **inp), hp, torch.float32)
        for n, v in r32.items():
            note(FP32, "GAN " + section[n], v)
            assert v < 1.0, (cfg4, hp["groups"], n, v)


def test_forward_mistake_group_1_normalised_with_group_0s_statistics():
    C, T, B, cond = FORWARD_CONFIGS[0]
    cfg, S64, pre, halves, _ = forward_problem(C, T, B, cond)
    hp = E.gen_forward_hp(B, T, 2)
    table = E.gen_forward_table(hp, cond)
    both = {k: torch.cat([halves["d"][k], halves["g"][k]], 0) for k in halves["d"]}
    stage = next(st.name for st in table if "a_d0" in st.outs)
    _, ratios = E.evaluate(table, dict(pre, **both), hp, torch.float64, mutate={stage: E.bn_train_groups(stats_of=lambda g: 0)[1]})
    note(MISTAKES, "GAN 2B-row pass: group 1 normalised with group 0's statistics", ratios["a_d0"])
    assert ratios["a_d0"] > 1.0 and max(v for n, v in ratios.items() if n != "a_d0") < 1e-3
    bad_tail = lambda hp_, x, w, b: (torch.cat([E.convT_s2()[1](hp_, x, w, b)[0], b.expand(x.shape[0], 4, b.shape[0])], 1),)  # noqa: E731
    C, T, B, cond = FORWARD_CONFIGS[1]
    cfg, S64, pre, halves, _ = forward_problem(C, T, B, cond)
    hp = E.gen_forward_hp(B, T, 1)
    _, ratios = E.evaluate(E.gen_forward_table(hp, cond), dict(pre, **halves["g"]), hp, torch.float64, mutate={"notes": bad_tail})
    note(MISTAKES, "GAN notes: zero-padded tail rows written (T = 20)", ratios["notes"])
    assert ratios["notes"] > 1.0


def g_backward_problem(C, T, B, cond=False, latent_ed=False, exact_thirds=False):
    """The generator step on the host: forward by the forward table, the emotion branch's gradient by autograd on the oracle's
    frozen classifier, then the backward table.  Returns (hp, table, pre, the oracle's g_step result, notes_mode)."""
    cfg, S64, pre, halves, (real, numeric, latent, emot, R) = forward_problem(C, T, B, cond)
    if latent_ed:
        ed_cfg = dict(S64.ed_cfg, input_mode="latent", latent_dim=cfg["LATENT_DIM"])
        S0 = O.build_gan_state(cfg, ed_cfg, "closed_form", d_scale=6.0)
        d64 = lambda dct: OrderedDict((k, v.double().clone()) for k, v in dct.items())  # noqa: E731
        S64 = O.GanState(cfg, ed_cfg, d64(S64.PE), d64(S64.PG), d64(S64.BG), d64(S64.PD), d64(S0.PED), d64(S0.BED))
    fhp = E.gen_forward_hp(B, T, 1)
    post, _ = E.evaluate(E.gen_forward_table(fhp, cond), dict(pre, **halves["g"]), fhp, torch.float64, carry="ref")
    post.update({"p.D." + k: v.clone() for k, v in S64.PD.items()})
    notes_mode = not latent_ed
    # the emotion branch by its own tables (fold, then g_ed_branch), and against autograd on the oracle's frozen classifier
    chans = E.ed_chans(C) if notes_mode else []
    post.update({"p.ED." + k: v.clone() for k, v in S64.PED.items()})
    post.update({"b.ED." + k: v.clone() for k, v in S64.BED.items()})
    post["emot_idx"] = emot
    ehp = E.ed_hp(B, cfg["LAMBDA_EMOTION"])
    post, rf = E.evaluate(E.ed_fold_table(chans), post, ehp, torch.float64, carry="ref")
    etable = E.ed_branch_table(chans, 2, notes_mode)
    post, re_ = E.evaluate(etable, post, ehp, torch.float64, carry="ref")
    assert max(list(rf.values()) + list(re_.values()) + [0.0]) < 1e-6, (rf, re_)
    x = (post["notes"] if notes_mode else post["lat"]).clone().requires_grad_(True)
    logits = O.emotion_disc_fwd(S64.PED, S64.BED, x, S64.ed_cfg)
    (g,) = torch.autograd.grad(cfg["LAMBDA_EMOTION"] * torch.nn.functional.cross_entropy(logits, emot), x)
    close64(post["logits"], logits.detach(), f"{(C, T, B)} emotion logits")
    close64(post["dnotes@ed" if notes_mode else "ed_dfeat"], g, f"{(C, T, B)} emotion branch gradient")
    ED_PROBLEM[(C, T, B, cond, latent_ed)] = (chans, etable, ehp, {k: v for k, v in post.items()})
    r = O.g_step(S64, latent.double(), numeric.double(), emot, R["noise_g"].double(), R["dm_g"])
    hp = E.gen_backward_hp(B, T, exact_thirds=exact_thirds)
    return hp, E.gen_backward_table(hp, cfg["NOISE_DIM"], cfg["ENCODER_OUT_DIM"], notes_mode), post, r, notes_mode


ED_PROBLEM = {}


G_BACKWARD_CONFIGS = ((4, 32, 4, False, False), (4, 20, 3, False, False), (4, 16, 3, True, True))


@pytest.mark.parametrize("cfg5", G_BACKWARD_CONFIGS, ids=str)
def test_generator_backward_table_equals_the_oracle_and_fp32_stays_inside(cfg5):
    hp, table, pre, r, _ = g_backward_problem(*cfg5, exact_thirds=True)
    mags = {}
    post, ratios = E.evaluate(table, pre, hp, torch.float64, carry="ref", mags=mags)
    assert max(ratios.values()) < 1e-6, {n: v for n, v in ratios.items() if v >= 1e-6}
    close64(post["adv"][0], r["loss_g_adv"], f"{cfg5} adv")
    close64(post["emo"][0], r["loss_g_emo"], f"{cfg5} emo")
    for k, g in r["grads"].items():
        # a bias in front of a train-mode BatchNorm: zero up to the rounding of a column sum of dz
        extra = K64 * U64 * float(post[{"G.decoder.deconv.0.bias": "d_zd0", "G.decoder.deconv.3.bias": "d_zd3"}[k]].abs().sum()) \
            if k in ("G.decoder.deconv.0.bias", "G.decoder.deconv.3.bias") else 0.0
        close64(post["g." + k], g, f"{cfg5} gradient {k}", extra, mags["g." + k])
    section = {n: st.section for st in table for n in st.outs}
    hp["ds"] = E.gen_backward_hp(cfg5[2], cfg5[1])["ds"]          # the device's fp32 -1/B
    _, r32 = E.evaluate(table, pre, hp, torch.float32)
    for n, v in r32.items():
        note(FP32, "GAN " + section[n], v)
        assert v < 1.0, (cfg5, n, v)


G_BACKWARD_MISTAKES = OrderedDict([
    ("dnotes: emotion gradient overwritten instead of accumulated", ((4, 32, 4, False, False), "dnotes", lambda nd, E_: E._dnotes(True, overwrite=True)[1])),
    ("demb without the generator-input slice", ((4, 32, 4, False, False), "demb", lambda nd, E_: E._demb(nd, E_, drop=1)[1])),
    ("demb without the critic-head path", ((4, 32, 4, False, False), "demb", lambda nd, E_: E._demb(nd, E_, drop=0)[1])),
    ("d_lat (latent mode) without ed_dfeat", ((4, 16, 3, True, True), "d_lat", lambda nd, E_: E._dlat(True, drop_ed=True)[1])),
    ("zero-padded tail rows (T = 20) left carrying gradient", ((4, 20, 3, False, False), "dn_dense", lambda nd, E_: (
        lambda hp, x: (x.reshape(x.shape[0], -1)[:, -16 * x.shape[2]:].reshape(x.shape[0], 16, x.shape[2]).clone(),)))),
    ("d_zd3 with BatchNorm 0's statistics slice", ((4, 32, 4, False, False), "d_zd3+g.G.decoder.deconv.4.weight+g.G.decoder.deconv.4.bias",
                                                  lambda nd, E_: (lambda hp, da, a, z, g, b, sm, si: E.bn_back()[1](hp, da, a, z, g, b, sm.flip(0), si)))),
])


@pytest.mark.parametrize("name", list(G_BACKWARD_MISTAKES), ids=lambda s: s.replace(" ", "_"))
def test_generator_backward_mistakes_leave_their_stage(name):
    cfg5, stage, make = G_BACKWARD_MISTAKES[name]
    hp, table, pre, _, _ = g_backward_problem(*cfg5)
    assert any(st.name == stage for st in table), stage
    _, ratios = E.evaluate(table, pre, hp, torch.float64, mutate={stage: make(128, 128)})
    mine = max(ratios[n] for n in stage.split("+"))
    note(MISTAKES, "GAN " + name, mine)
    assert mine > 1.0, (name, mine)
    assert max(v for n, v in ratios.items() if n not in stage.split("+")) < 1e-3


@pytest.mark.parametrize("cfg5", ((128, 128, 2, False, False),) + G_BACKWARD_CONFIGS, ids=str)
def test_emotion_branch_fp32_and_mistakes(cfg5):
    """(b) and (c) for g_ed_branch: fp32 host evaluation of the fold and of the branch, with the direct and with the F(2,3)
    bounds where the engine may take either, and the mistakes of its loss and its wiring.  (128, 128, 2): the bf16 shapes."""
    g_backward_problem(*cfg5)
    chans, table, hp, pre = ED_PROBLEM[tuple(cfg5)]
    notes_mode = bool(chans)
    for wino in ((False, True) if notes_mode else (False,)):
        wf = [wino and k == 3 for _, _, k in chans]
        tab = E.ed_fold_table(chans) + E.ed_branch_table(chans, 2, notes_mode, wf, wf)
        section = {n: st.section for st in tab for n in st.outs}
        _, r32 = E.evaluate(tab, pre, hp, torch.float32)
        for n, v in r32.items():
            note(FP32, "GAN " + section[n] + (" (F(2,3) bound)" if wino and "ed_" in n and "conv" in section[n] + "data" else ""), v)
            assert v < 1.0, (cfg5, wino, n, v)
    if tuple(cfg5[:3]) == E.GAN_BF16_ED_CONFIG:
        # the bf16 variant: fp32 arithmetic on bf16-rounded operands, outputs rounded once to bf16, stays inside bf16_ref's
        # bounds; a GELU taken at a shifted pre-activation does not
        import bf16_ref as B16
        tab = E.ed_fold_table(chans) + E.ed_branch_table(chans, 2, True, bf16=True)
        _, r16 = E.evaluate(tab, pre, hp, torch.float32)
        for n, v in r16.items():
            note(FP32, "GAN emotion branch, bf16 storage", v)
            assert v < 1.0, (cfg5, n, v)
        _, rt = E.evaluate(tab, pre, hp, torch.float32, mutate={"ed_z1+ed_a1": lambda hp_, x, w, sc, sh: (
            (B16.conv_fp32_host(x, w, 3) * sc + sh).to(B16.BF), torch.nn.functional.gelu(B16.conv_fp32_host(x, w, 3) * sc + sh + 0.01).to(B16.BF))})
        note(MISTAKES, "GAN bf16 emotion branch: GELU of a shifted z", rt["ed_a1"])
        assert rt["ed_a1"] > 1.0 and rt["ed_z1"] < 1.0
    mistakes = [("emotion loss: lambda_emo / B missing", "emo+dlogits", E._emotion_loss(weighted=False)[1])]
    if notes_mode:
        mistakes += [("emotion branch: GELU' at the block's own z instead of the block below's", "ed_dz1",
                      lambda hp_, dz, w, z, sc: E._ed_dgrad(False)[1](hp_, dz, w, z.roll(1, 1), sc)),
                     ("emotion branch: the folded scale left out of the pooling backward", f"ed_dz{len(chans) - 1}",
                      lambda hp_, dh, z, sc: E._ed_pool_bwd()[1](hp_, dh, z, torch.ones_like(sc))),
                     ("emotion branch: fold without the convolution's bias", "ed_scale0+ed_shift0",
                      lambda hp_, g_, b_, rm, rv, cb: E._ed_fold()[1](hp_, g_, b_, rm, rv, torch.zeros_like(cb)))]
    tab = E.ed_fold_table(chans) + table
    for name, stage, fn in mistakes:
        _, ratios = E.evaluate(tab, pre, hp, torch.float64, mutate={stage: fn})
        mine = max(ratios[n] for n in stage.split("+"))
        note(MISTAKES, "GAN " + name, mine)
        assert mine > 1.0, (name, mine)
        assert max(v for n, v in ratios.items() if n not in stage.split("+")) < 1e-3, name


def test_batchnorm_from_partials_route():
    """The `parts` route of the generator's BatchNorm, stage by stage on the host: fp32 partials of a very unequal split (one
    chunk empty and holding garbage), the rider held against z, the BatchNorm against what the ROUNDED partials combine to."""
    for groups, Rn, C, np_ in ((1, 128, 64, 4), (2, 96, 128, 3)):
        g = torch.Generator().manual_seed(Rn)
        z = (torch.randn(groups * Rn, C, generator=g) * 0.3 + 0.5).view(groups * 4, -1, C)
        part = torch.cat([S.conv16_parts(zg, np_ + 1, empty_rows=(1,), seed=i)[0] for i, zg in enumerate(z.chunk(groups, 0))])
        gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
        rm0, rv0 = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
        hp = E.gen_forward_hp(4, 32, groups, (True, True))
        (ref,), (got,) = E._parts_rider()[0](hp, part, z), E._parts_rider()[1](hp, part, z)
        note(FP32, "GAN generator BatchNorm partials", S.worst(got, ref)[0])
        assert S.worst(got, ref)[0] < 1.0
        refs, gots = E.bn_train_from_parts()[0](hp, part, z, gamma, beta, rm0, rv0), E.bn_train_from_parts()[1](hp, part, z, gamma, beta, rm0, rv0)
        for r, v in zip(refs, gots):
            note(FP32, "GAN generator BatchNorm", S.worst(v, r)[0])
            assert S.worst(v, r)[0] < 1.0
        # a chunk left out of the combine / the statistics of the raw rows where the partials' are meant: the first is
        # far outside, the second is what the one-rounding budget of the apply cannot absorb in general
        lost = part.clone()
        lost[0, 2] = 0.0
        bad = E.bn_train_from_parts()[1](hp, lost, z, gamma, beta, rm0, rv0)
        note(MISTAKES, "GAN BatchNorm from partials: one chunk left out of the combine", S.worst(bad[2], refs[2])[0])
        assert S.worst(bad[2], refs[2])[0] > 1.0


# ---------------------------------------------------------------------------------------------------------------------
# (d) the branches the GPU file asserts
# ---------------------------------------------------------------------------------------------------------------------
def test_critic_configurations_reach_the_pooled_rider_only_where_chosen():
    """conv.4 (128 -> 256 channels) carries the mean over time where a sample's output positions are one wave tile; at
    B = 2 the smallest such roll has T3 = 32 (T = 256), for the 3B-row pass and the B-row tangent pass alike."""
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import ops
    half = lambda t: (t - 1) // 2 + 1  # noqa: E731
    for C, T, B in E.GAN_CRITIC_CONFIGS:
        T2 = half(half(T))
        for rows in (3 * B, B):
            assert bool(ops.conv16_poolable(rows, T2, 128, 256)) == (T == 256), (C, T, B, rows)
    # the generator's BatchNorm layers read conv16's partial statistics where it runs the deconvolution in front of them
    # (256 -> 128 and 128 -> 64 channels) and its row tile holds whole groups of B samples
    for (C, T, B), want in E.GAN_PARTS_ROUTES.items():
        red = max(1, T // 8)
        for groups in (1, 2):
            got = tuple(bool(ops.conv16_supported(groups * B, Tin, Cin, N, True, 2 * Tin)) and B % ops.conv16_plan(groups * B, Tin, N, True)[0] == 0
                        for Tin, Cin, N in ((red, 256, 128), (2 * red, 128, 64)))
            assert got == want, (C, T, B, groups, got)
    assert {v for v in E.GAN_PARTS_ROUTES.values()} == {(False, False), (False, True), (True, True)}
    for T in (64, 128, 192, 248):                  # shorter rolls at B = 2 are not poolable
        assert not ops.conv16_poolable(6, half(half(T)), 128, 256), T

def test_vae_tables_reach_both_decoder_tails():
    seen = set()
    for B, T, latent in E.VAE_CONFIGS:
        hp = E.vae_hp(B, T, latent)
        spec, _ = O.vae_spec(T, latent)
        names = [st.name for flow in E.vae_tables(spec, hp).values() for st in flow]
        dense = hp["Ld"][3] != T           # VaeEngine.g_rec_dense is allocated under this condition
        assert ("g_rec_dense" in names) == dense == (T % 8 != 0)
        seen.add(dense)
        # an odd time axis in the encoder: its data gradient is the 2 Tin - 1 form of the scatter kernel
        seen.add(("odd", any(t % 2 for t in hp["Ts"][1:3])))
        assert sum(math.prod(s) for s in spec.values()) % 4 == 0      # no padding element behind the flat buffers
    assert seen == {True, False, ("odd", True), ("odd", False)}
