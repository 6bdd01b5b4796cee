"""The engines' training steps against the stage tables of tests/engine_ref.py, LAUNCH BY LAUNCH and element by element: each
flow runs eagerly for two free-running steps (no re-synchronisation: step 2 sees the updated parameters, moments, step state
and running statistics), every named tensor is snapshot after every public sub-step, and every stage is held to its one-stage
bound from the engine's OWN stored upstream tensors.  Nothing is excluded: no parameter, no element, no mask; a cancelling
gradient (a bias in front of a BatchNorm) is bounded through its magnitude M.  Whatever a sub-step is supposed to write is
NaN-prefilled first.  Buffers a sub-step overwrites in place are captured in front of the overwriting call -- the VAE's g_recon
and g_h by wrapping the `ops` function here, dnotes and demb at the public sub-step boundaries, the BatchNorm partial
statistics behind their launch; the engines are not touched.  The mutation tests at the end break one
launch each at Python level (a flag, or two valid same-shaped buffers swapped) and require the contract to flag exactly the
stage named.  tests/test_engine_ref.py shows on the host that the tables equal the oracle, that fp32 arithmetic stays inside
the bounds and that plausible mistakes leave them.  The worst error / bound per section is printed (pytest -s) and quoted
in DESIGN.md §2.

Covered: VaeEngine (forward / backward / update); GanEngine's d_backward (generator forward of the critic-step half + the
critic step), d_update, the generator step through its public sub-steps (g_forward, g_ed_branch, g_critic_front,
g_critic_back, g_backward_b), g_update, the fold of the frozen emotion discriminator, with the row chains and with
MELO_CHAINS=0, fp32 and bf16 emotion branch; and the fused flow from the randoms the device draws, its constituents by hand
with every stage judged and the launch list compared with dg_step_rng's.  Every case asserts the routes it is here for; the
measured figures are in DESIGN.md section 2."""
import contextlib
from collections import OrderedDict

import pytest
import torch

import engine_ref as E
import support_ref as S
from oracle import melo_oracle as O

pytestmark = pytest.mark.gpu

SECTIONS = OrderedDict()
ROUTES = {}             # (C, T, B, groups) -> the (parts0, parts1) routes the generator's two BatchNorm layers took
IN_PLACE = ("b.", "P.data", "P.m", "P.v", "P.state")          # read as pre:, written in place: never prefilled


@pytest.fixture(scope="module")
def ops():
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import ops as o
    return o


class _Symbols:
    def __init__(self):
        self.seen = []

    def __call__(self, sym, flops, launch=None):
        self.seen.append(sym)
        return contextlib.nullcontext()


@pytest.fixture
def hook(ops):
    rec = _Symbols()
    ops.set_launch_hook(rec)
    try:
        yield rec
    finally:
        ops.set_launch_hook(None)


def teardown_module(module):
    total = 0
    for k, (n, r, what) in SECTIONS.items():
        total += n
        print(f"\n[engine contract] {k}: {n} checks, worst error / bound = {r:.4f} ({what})")
    print(f"\n[engine contract] {total} bound checks")
    print(f"\n[engine contract] BatchNorm-from-partials routes: {ROUTES}")


def record(section, r, what):
    s = SECTIONS.setdefault(section, [0, 0.0, ""])
    s[0] += 1
    if r >= s[1]:
        s[1], s[2] = r, what


# ---------------------------------------------------------------------------------------------------------------------
# the VAE
# ---------------------------------------------------------------------------------------------------------------------
def vae_engine(B, T, latent):
    from melo_gan_amd.ae.engine import VaeEngine
    spec, bufs = O.vae_spec(T, latent)
    P = O.fill_params(spec, 6.0, O.norm_affine_names(spec))
    eng = VaeEngine(dict(MAX_NOTES=T, LATENT_DIM=latent, BATCH_SIZE=B, LR=1e-4, WEIGHT_DECAY=1e-5), "cuda", B)
    assert list(eng.P.spec) == list(spec) and all(tuple(eng.P.spec[k]) == tuple(spec[k]) for k in spec)
    eng.load_state(P, O.fill_buffers(bufs))
    g = torch.Generator().manual_seed(5)
    xs = [(torch.rand(B, T, 4, generator=g) * 2 - 1).cuda() for _ in range(2)]
    es = [torch.randn(B, latent, generator=g).cuda() for _ in range(2)]
    return eng, spec, xs, es


def vae_live(eng):
    """name (engine_ref's) -> the engine's live tensor."""
    t = OrderedDict(x=eng.x, eps=eng.eps, flat=eng.flat, h=eng.h, mu=eng.mu, lv=eng.lv, zl=eng.zl, p0=eng.p0, p2=eng.p2, y0=eng.y0,
                    recon=eng.recon, loss=eng.loss, gnorm=eng.gnorm, g_recon=eng.g_recon, k_mu=eng.k_mu, k_lv=eng.k_lv, g_y0=eng.g_y0,
                    g_p2=eng.g_p2, g_p0=eng.g_p0, g_z=eng.g_z, g_mu=eng.g_mu, g_lv=eng.g_lv, g_h=eng.g_h, g_flat=eng.g_flat)
    if eng.g_rec_dense is not None:
        t["g_rec_dense"] = eng.g_rec_dense
    for nm in ("ez", "ea", "e_mean", "e_istd", "dz_", "da_", "d_mean", "d_istd", "g_da", "g_dz", "g_ea", "g_ez"):
        for j, v in enumerate(getattr(eng, nm)):
            t[f"{nm}{j}"] = v
    for k in eng.P.spec:
        t["p." + k], t["g." + k] = eng.P.p[k], eng.P.g[k]
    for k, v in eng.buf.items():
        t["b." + k] = v
    t["P.data"], t["P.grad"], t["P.m"], t["P.v"], t["P.state"] = eng.P.data, eng.P.grad, eng.P.m, eng.P.v, eng.P.state
    return t


def snapshot(live):
    return {k: v.detach().clone() for k, v in live.items()}


@contextlib.contextmanager
def vae_captures(ops, eng, monkeypatch, into):
    """g_recon after vae_loss and g_h after the accumulating launch, each as the in-place act_bwd is about to overwrite it."""
    real = ops.act_bwd

    def act_bwd(dy, dx, **kw):
        if dx is eng.g_recon:
            into["g_recon@loss"] = dy.detach().clone()
        elif dx is eng.g_h:
            into["g_h@sum"] = dy.detach().clone()
        return real(dy, dx, **kw)

    with monkeypatch.context() as m:
        m.setattr(ops, "act_bwd", act_bwd)
        yield


def vae_substep(ops, eng, monkeypatch, flow, table, hp, call):
    """Prefill, run one public sub-step, snapshot, judge: {output name: worst error / bound}."""
    live = vae_live(eng)
    n = eng.P.n
    for st in table:
        for name in st.outs:
            if "@" in name or name.startswith(IN_PLACE) or name.startswith("g.") or name == "P.grad":
                continue
            if name == "recon":          # the rows past the decoder's reach are the model's zero padding: an input, never written
                live[name][:, :hp["Ld"][3]].fill_(float("nan"))
            else:
                live[name].fill_(float("nan"))
    if flow == "backward":
        eng.P.grad[:n].fill_(float("nan"))
    pre = snapshot(live)
    extra = {}
    with vae_captures(ops, eng, monkeypatch, extra):
        call()
    torch.cuda.synchronize()
    post = snapshot(live)
    post.update(extra)
    if flow == "forward":
        assert bool((post["recon"][:, hp["Ld"][3]:] == 0).all()), "recon: the padding rows were written"
    if flow == "backward":
        assert bool((post["P.grad"][n:] == 0).all()), "the gradient buffer's padding was written"
    return E.judge(table, pre, post, hp)


def vae_run_step(ops, eng, monkeypatch, tables, hp, x, eps, flows=E.VAE_FLOWS):
    eng.x.copy_(x)
    eng.eps.copy_(eps)
    out = OrderedDict()
    for flow, call in (("forward", lambda: eng.forward(True)), ("backward", lambda: eng.backward(hp["beta"])), ("update", eng.update)):
        if flow in flows:
            out[flow] = vae_substep(ops, eng, monkeypatch, flow, tables[flow], hp, call)
    return out


def flagged(ratios, tables):
    """The stages (by name) with an output above its bound."""
    bad = {n for rs in ratios.values() for n, r in rs.items() if not r <= 1.0}
    return {st.name for flow in tables.values() for st in flow if bad & set(st.outs)}


@pytest.mark.parametrize("cfg", E.VAE_CONFIGS, ids=str)
def test_vae_two_free_running_steps(ops, hook, monkeypatch, cfg):
    B, T, latent = cfg
    eng, spec, xs, es = vae_engine(B, T, latent)
    hp = E.vae_hp(B, T, latent)
    tables = E.vae_tables(spec, hp)
    section = {n: st.section for flow in tables.values() for st in flow for n in st.outs}
    # the branch taken: the dense copy of the gradient exists exactly where the decoder stops short of T
    assert (eng.g_rec_dense is not None) == (T % 8 != 0) == any(st.name == "g_rec_dense" for st in tables["backward"])
    launches = []
    for it in range(2):
        hook.seen.clear()
        ratios = vae_run_step(ops, eng, monkeypatch, tables, hp, xs[it], es[it])
        launches.append(list(hook.seen))
        for flow, rs in ratios.items():
            for n, r in rs.items():
                record("VAE " + section[n], r, f"{cfg} step {it + 1} {n}")
        bad = {n: r for rs in ratios.values() for n, r in rs.items() if not r <= 1.0}
        assert not bad, f"{cfg} step {it + 1}: stages above their bound: {bad}"
        assert float(eng.P.state[0]) == it + 1 == eng.num_batches_tracked
    # both steps took the same routes; every matrix stage of the table is one launch of the family it belongs to (a stage
    # summed from two launches counts two), and the weight gradients went out through the two multi-job launches
    assert launches[0] == launches[1], (launches[0], launches[1])
    count = lambda *secs: sum(2 if st.name == "g_h@sum" else 1 for flow in tables.values() for st in flow if st.section in secs)  # noqa: E731
    seen = launches[0]
    assert sum(s.startswith("linear_skinny_kernel<") for s in seen) == count("Linear forward", "Linear data gradient") == 10, seen
    convs = count("encoder conv", "decoder convT", "decoder data gradient", "encoder data gradient")
    assert sum(s.startswith(("conv_wgemm_kernel<2,5,", "thin_in_kernel", "thin_out_kernel<")) for s in seen) == convs == 11, seen
    assert seen[-2:] == ["wgrad_multi_kernel<2,5>", "wgrad_multi_kernel<1,1>"] and len(seen) == 10 + convs + 2, seen


# ---------------------------------------------------------------------------------------------------------------------
# mutations on the device: one launch broken at Python level; the contract flags exactly its stage
# ---------------------------------------------------------------------------------------------------------------------
def _mut_accumulate_off(ops, eng):
    real = ops.linear_dgrad

    def f(dy, w, dx, **epi):
        if dx is eng.g_h:
            epi.pop("accumulate", None)
        return real(dy, w, dx, **epi)
    return "linear_dgrad", f


def _mut_gref_other_buffer(ops, eng):
    real = ops.linear_dgrad

    def f(dy, w, dx, **epi):
        if epi.get("gref") is eng.p0:
            epi["gref"] = eng.h              # same shape (B, 512), the other ReLU output
        return real(dy, w, dx, **epi)
    return "linear_dgrad", f


def _mut_kld_swapped(ops, eng):
    real = ops.reparam_bwd

    def f(g_z, lv, eps, k_mu, k_lv, g_mu, g_lv):
        return real(g_z, lv, eps, k_lv, k_mu, g_mu, g_lv)
    return "reparam_bwd", f


def _mut_wgrad_job_dropped(ops, eng):
    real = ops.wgrad_multi

    def f(jobs, *a, **kw):
        return real(list(jobs)[:-1], *a, **kw)      # the last job of the list: encoder.conv.0
    return "wgrad_multi", f


def _mut_grad_scale_doubled(ops, eng):
    real = ops.adam_flat

    def f(*a, **kw):
        kw["grad_scale"] = 2.0 * kw.get("grad_scale", 1.0)
        return real(*a, **kw)
    return "adam_flat", f


VAE_MUTATIONS = OrderedDict([
    ("accumulate off on the g_h launch", (_mut_accumulate_off, "g_h@sum")),
    ("gref from the other buffer in decoder.pre.2's data gradient", (_mut_gref_other_buffer, "g_p0")),
    ("the two KLD gradients swapped", (_mut_kld_swapped, "g_mu+g_lv")),
    # its gradient keeps the NaN prefill: the update behind it is not run
    ("one job dropped from the wgrad_multi list", (_mut_wgrad_job_dropped, "g.encoder.conv.0.weight+g.encoder.conv.0.bias", ("forward", "backward"))),
    ("grad_scale doubled", (_mut_grad_scale_doubled, "P.data+P.m+P.v+P.state")),
])


@pytest.mark.parametrize("name", list(VAE_MUTATIONS), ids=lambda s: s.replace(" ", "_"))
def test_vae_mutation_is_flagged_at_its_stage(ops, monkeypatch, name):
    make, stage, *flows = VAE_MUTATIONS[name]
    B, T, latent = E.VAE_CONFIGS[0]
    eng, spec, xs, es = vae_engine(B, T, latent)
    hp = E.vae_hp(B, T, latent)
    tables = E.vae_tables(spec, hp)
    attr, fn = make(ops, eng)
    with monkeypatch.context() as m:
        m.setattr(ops, attr, fn)
        ratios = vae_run_step(ops, eng, monkeypatch, tables, hp, xs[0], es[0], *flows)
    assert flagged(ratios, tables) == {stage}, (name, flagged(ratios, tables))


# ---------------------------------------------------------------------------------------------------------------------
# the GAN's optimiser updates (d_update, g_update) and the re-laid weight copies they keep current
# ---------------------------------------------------------------------------------------------------------------------
def gan_engine(C, T, B, ema_decay=0.0):
    """The golden fixtures' settings; E.GAN_COND_LATENT_CONFIG: conditioning mode with the latent-mode emotion classifier."""
    from melo_gan_amd.gan.engine import GanEngine
    cfg, ed_cfg = O.default_gan_cfg(B, T, C), O.default_ed_cfg(C)
    if (C, T, B) == E.GAN_COND_LATENT_CONFIG:
        cfg["INTEGRATION_MODE"] = "conditioning"
        ed_cfg.update(input_mode="latent", latent_dim=cfg["LATENT_DIM"])
    if ema_decay:
        cfg["EMA_DECAY"] = ema_decay
    bf16 = (C, T, B) == E.GAN_BF16_ED_CONFIG            # the secondary configuration: the frozen classifier's convolutions in bf16
    St = O.build_gan_state(cfg, ed_cfg, "closed_form", d_scale=6.0)
    eng = GanEngine(cfg, ed_cfg, "cuda", B, ed_dtype="bf16" if bf16 else "fp32")
    eng.load_state(St.PE, St.PG, St.BG, St.PD, St.PED, St.BED)
    real, numeric, latent, emot = O.synthetic_batch(B, T, C, cfg["LATENT_DIM"], 6, 7)
    latent = torch.randn(latent.shape, generator=torch.Generator().manual_seed(3))       # the synthetic latent is zero
    eng.set_batch(real.cuda(), numeric.cuda(), latent.cuda(), emot.cuda())
    return eng, cfg, St


def gan_update_live(eng, X):
    fp = eng.D if X == "D" else eng.GE
    t = OrderedDict([(f"{X}.data", fp.data), (f"{X}.grad", fp.grad), (f"{X}.m", fp.m), (f"{X}.v", fp.v), (f"{X}.state", fp.state)])
    for k in fp.spec:
        t["p." + k] = fp.p[k]
    for (name, direction), w in eng.wq.items():
        if (name in fp.spec):
            t[f"wq.{name}.{direction}"] = w
    if X == "GE" and eng.ema is not None:
        t["ema"] = eng.ema
    return t


def gan_update_table(eng, cfg, X):
    fp = eng.D if X == "D" else eng.GE
    order = sorted(fp.spec, key=lambda k: fp.offsets[k][0])
    ema = (eng.ema_decay, eng.ema_ramp, eng.ema_offset) if X == "GE" and eng.ema is not None else None
    table = E.gan_update_table(X, fp.spec, transposed_conv=(X == "GE"), order=order, ema=ema)
    # the table covers every copy the engine holds, and the engine holds every copy the table expects
    assert {n for st in table for n in st.outs if n.startswith("wq.")} == {f"wq.{n}.{d}" for (n, d) in eng.wq if n in fp.spec}
    return table, E.gan_update_hp(cfg["LR_D" if X == "D" else "LR_G"])


def gan_update_substep(eng, cfg, X, call, prefill=True):
    table, hp = gan_update_table(eng, cfg, X)
    hp["ticked"] = bool((eng.D if X == "D" else eng.GE).ticked)       # the draw in front already advanced the step state
    live = gan_update_live(eng, X)
    if prefill:
        for n, t in live.items():
            if n.startswith("wq."):
                t.fill_(float("nan"))
    pre = snapshot(live)
    call()
    torch.cuda.synchronize()
    return table, E.judge(table, pre, snapshot(live), hp)


def gan_half_step(eng, cfg, R, X):
    if X == "D":
        eng.set_randoms(R["noise_d"].cuda(), [m.cuda() for m in R["dm_d"]], R["alpha"].cuda())
        eng.d_backward()
    else:
        eng.set_randoms(R["noise_g"].cuda(), [m.cuda() for m in R["dm_g"]])
        eng.g_backward()


FWD_NAMES = ("numeric", "noise", "e_x0", "e_xhat", "e_z1", "e_h1", "e_z2", "e_h2", "emb", "gin", "a_n0", "lat", "a_p0", "y0", "z_d0", "a_d0",
             "z_d3", "a_d3")


def forward_live(eng, half):
    """engine_ref's forward names -> the engine's tensors of one half ('d': critic step, 'g': generator step) or of the
    2B-row pass ('both')."""
    B = eng.B
    sfx = {"d": "_d", "g": "", "both": "_2"}[half]
    t = OrderedDict((nm, getattr(eng, nm + sfx)) for nm in FWD_NAMES)
    masks = {"d": eng.dmask_d, "g": eng.dmask, "both": eng.dmask_2}[half]
    t["dmask0"], t["dmask1"], t["latent"] = masks[0], masks[1], eng.latent
    for j in range(2):
        for nm in ("bn_mean", "bn_invstd"):
            full = getattr(eng, nm + "_2")[j]
            t[f"{nm}{j}"] = full if half == "both" else full[0 if half == "d" else 1]
    t["notes"] = {"d": eng.fake_d, "g": eng.notes, "both": eng.X0[2 * B:]}[half]
    for k in eng.GE.spec:
        t["p." + k] = eng.GE.p[k]
    for k, v in eng.Gbuf.items():
        t["b." + k] = v
    return t


def forward_prefill(eng, half, table):
    live = forward_live(eng, half)
    for st in table:
        for n in st.outs:
            if n.startswith("b."):
                continue
            (live[n][:, :eng.L3] if n == "notes" else live[n]).fill_(float("nan"))
    return live, snapshot(live)


def forward_routes(eng, riders, groups):
    """(parts flags, {part0 / part1: the copied partials}) of the forward pass among the recorded launches."""
    flags, parts = [], {}
    for j, nm in enumerate(("G.decoder.deconv.0.weight", "G.decoder.deconv.3.weight")):
        part = next(p for kind, name, rows, r, p in riders if kind == "convT_fwd" and name == nm and rows == groups * eng.B)
        flags.append(part is not None)
        if part is not None:
            parts[f"part{j}"] = part
    return tuple(flags), parts


def forward_judge(eng, half, riders, live, pre, what):
    groups = 2 if half == "both" else 1
    flags, parts = forward_routes(eng, riders, groups)
    hp = E.gen_forward_hp(eng.B, eng.T, groups, flags)
    table = E.gen_forward_table(hp, eng.mode == "conditioning")
    post = snapshot(live)
    post.update(parts)
    for j, on in enumerate(flags):
        if on:
            post[f"partsum{j}"] = E.parts_totals(parts[f"part{j}"], groups, post[f"z_d{3 * j}"].shape[-1])
    ROUTES.setdefault((eng.C, eng.T, eng.B, groups), set()).add(flags)
    assert flags == E.GAN_PARTS_ROUTES[(eng.C, eng.T, eng.B)], (what, flags)
    assert bool((post["notes"][:, eng.L3:] == 0).all()), what + ": the zero-padded tail rows were written"
    ratios = E.judge(table, pre, post, hp)
    section = {n: st.section for st in table for n in st.outs}
    for n, r in ratios.items():
        if not what.startswith("mutation"):
            record("GAN " + section[n], r, f"{what} {n}")
    bad = {n: r for n, r in ratios.items() if not r <= 1.0}
    assert not bad, f"{what}: forward stages above their bound: {bad}"


def forward_table(eng, groups):
    hp = E.gen_forward_hp(eng.B, eng.T, groups)
    return E.gen_forward_table(hp, eng.mode == "conditioning"), hp


def g_backward_live(eng):
    B = eng.B
    t = forward_live(eng, "g")
    for k in eng.GE.spec:
        t["g." + k] = eng.GE.g[k]
    for k in eng.D.spec:
        t["p.D." + k] = eng.D.p[k]
    for nm, src in (("gA1", "A1"), ("gA2", "A2"), ("gA3", "A3"), ("gH", "H"), ("gFh", "Fh"), ("gs", "s"), ("gdU", "dU"), ("gdH", "dH"),
                    ("gdZ3", "dZ3"), ("gdZ2", "dZ2"), ("gdZ1", "dZ1")):
        t[nm] = getattr(eng, src)[:B]
    for nm in ("adv", "dnotes", "d_ad3", "d_zd3", "d_ad0", "d_zd0", "d_p2", "d_p0", "d_lat", "d_n0", "d_gin", "demb", "d_ez2", "d_ez1", "d_ex0",
               "ed_dfeat"):
        t[nm] = getattr(eng, nm)
    if eng.dn_dense is not None:
        t["dn_dense"] = eng.dn_dense
    return t


def conv16_runs(ops, eng, name, direction, rows, Tin, Cin, N):
    """Whether _conv5s2 takes conv16 for a gather-form launch: the re-laid copy exists and the library covers the shape."""
    return (name, direction) in eng.wq and bool(ops.conv16_supported(rows, Tin, Cin, N, False, 0))


def g_backward_routes(ops, eng, riders, chains):
    """The routes of the generator step's backward, asserted launch by launch: the BatchNorm backward's column sums ride in
    the two data-gradient launches in front of it (`bnb`) and decoder.pre.2's gradient is written in (B, C, L) order (`perm`)
    exactly where conv16 runs those launches; the small layer stacks are chains exactly where chains are on."""
    B, red, C = eng.B, eng.red, eng.C
    dg = {name: r for kind, name, rows, r, _ in riders if kind == "convT_dgrad"}
    want_bnb = [conv16_runs(ops, eng, "G.decoder.deconv.6.weight", "dgrad", B, 8 * red, C, 64),
                conv16_runs(ops, eng, "G.decoder.deconv.3.weight", "dgrad", B, 4 * red, 64, 128)]
    got_bnb = [dg["G.decoder.deconv.6.weight"].bnb is not None, dg["G.decoder.deconv.3.weight"].bnb is not None]
    assert got_bnb == want_bnb, (got_bnb, want_bnb)
    want_perm = conv16_runs(ops, eng, "G.decoder.deconv.0.weight", "dgrad", B, 2 * red, 128, 256)
    assert dg["G.decoder.deconv.0.weight"].perm == want_perm, (dg["G.decoder.deconv.0.weight"].perm, want_perm)
    if (eng.C, eng.T, eng.B) == (128, 64, 4):          # the configuration that is here for these riders
        assert got_bnb == [True, True] and want_perm
    assert eng._chain_gf == eng._chain_ed == chains, (eng._chain_gf, eng._chain_ed, chains)
    ROUTES.setdefault(("bnb/perm", eng.C, eng.T, eng.B), set()).add((tuple(got_bnb), want_perm))


def ed_live(eng):
    t = OrderedDict(notes=eng.notes, lat=eng.lat, emot_idx=eng.emot_idx, ed_pool=eng.ed_pool, ed_proj=eng.ed_proj, logits=eng.logits,
                    emo=eng.emo, dlogits=eng.dlogits, ed_dproj=eng.ed_dproj, ed_dpool=eng.ed_dpool, ed_dfeat=eng.ed_dfeat)
    for nm in ("ed_z", "ed_a", "ed_dz", "ed_scale", "ed_shift", "ed_cz", "ed_ca", "ed_dcz"):
        for j, v in enumerate(getattr(eng, nm)):
            t[f"{nm}{j}"] = v
    for k in eng.ED.spec:
        t["p.ED." + k] = eng.ED.p[k]
    for k, v in eng.EDbuf.items():
        t["b.ED." + k] = v
    return t


def ed_tables(eng):
    notes_mode = eng.ed_mode == "notes"
    chans = E.ed_chans(eng.C) if notes_mode else []
    assert [tuple(c) for c in eng.ed_chans] == chans
    bf16 = eng.ed_dtype == "bf16"
    assert not bf16 or all(t.dtype == torch.bfloat16 for t in eng.ed_z + eng.ed_a + eng.ed_dz)
    return chans, E.ed_branch_table(chans, len(eng.ed_cz), notes_mode, eng.ed_wino_f, eng.ed_wino_d, bf16=bf16), E.ed_hp(eng.B, eng.lambda_emo)


def ed_fold_check(eng, what):
    """The fold of the frozen classifier's eval-mode BatchNorm (params_changed -> fold_ed), NaN-prefilled and judged."""
    chans, _, hp = ed_tables(eng)
    live = ed_live(eng)
    for i in range(len(chans)):
        live[f"ed_scale{i}"].fill_(float("nan"))
        live[f"ed_shift{i}"].fill_(float("nan"))
    eng.fold_ed()
    torch.cuda.synchronize()
    snap = snapshot(live)
    for n, r in E.judge(E.ed_fold_table(chans), snap, snap, hp).items():
        record("GAN emotion branch fold", r, f"{what} {n}")
        assert r <= 1.0, (what, n, r)


def g_step_substeps(eng, cfg, riders, what, forward=True, ops=None, chains=None):
    """The generator step through its public sub-steps -- g_forward, g_ed_branch, g_critic_front, g_critic_back,
    g_backward_b (= g_backward) -- with dnotes captured behind the emotion branch and demb behind the critic's head, both
    overwritten later; judges the forward and the backward tables."""
    notes_mode = eng.ed_mode == "notes"
    if forward:
        ftable, _ = forward_table(eng, 1)
        flive, fpre = forward_prefill(eng, "g", ftable)
    live = g_backward_live(eng)
    btable = E.gen_backward_table(E.gen_backward_hp(eng.B, eng.T), eng.noise_dim, eng.E, notes_mode)
    for st in btable:
        for n in st.outs:
            if "@" not in n and not n.startswith("g."):
                live[n].fill_(float("nan"))
    eng.GE.grad[:eng.GE.n].fill_(float("nan"))
    _, etable, ehp = ed_tables(eng)
    elive = ed_live(eng)
    for st in etable:
        for n in st.outs:
            if "@" not in n:
                elive[n].fill_(float("nan"))
    pre = snapshot(live)
    del riders[:]
    if forward:
        eng.g_forward()
    eng.g_ed_branch()
    torch.cuda.synchronize()
    extra = {"dnotes@ed": eng.dnotes.clone()} if notes_mode else {}
    esnap = snapshot(elive)
    esnap.update(extra)
    eratios = E.judge(etable, esnap, esnap, ehp)
    eng.g_critic_front()
    torch.cuda.synchronize()
    extra["demb@head"] = eng.demb.clone()
    eng.g_critic_back()
    eng.g_backward_b()
    torch.cuda.synchronize()
    if forward:
        forward_judge(eng, "g", riders, flive, fpre, what + " generator-step half")
    if ops is not None:
        g_backward_routes(ops, eng, riders, chains)
    pooled = [r.pooled for kind, name, rows, r, _ in riders if kind == "conv_fwd" and name == "conv.4.weight"]
    assert pooled == [eng.T == 256], pooled
    hp = E.gen_backward_hp(eng.B, eng.T, pooled=pooled[0])
    post = snapshot(live)
    post.update(extra)
    assert bool((eng.GE.grad[eng.GE.n:] == 0).all())
    ratios = E.judge(btable, pre, post, hp)
    ratios.update(eratios)
    section = {n: st.section for st in btable + etable for n in st.outs}
    for n, r in ratios.items():
        if what != "mutation":
            record("GAN " + section[n], r, f"{what} {n}")
    return btable + etable, ratios


def critic_live(eng):
    B = eng.B
    t = OrderedDict(real=eng.real, fake_d=eng.fake_d, alpha=eng.alpha, emb_d=eng.emb_d, xhat=eng.X0[:B], X3=eng.X0[:3 * B])
    for nm in ("A1", "A2", "A3", "H", "Fh", "s", "dU", "dH", "dZ3", "dZ2", "dZ1", "gx", "norms", "TAN0", "TAN1", "TAN2", "TZ3", "ghb",
               "gfb", "loss_d_out", "gp"):
        t[nm] = getattr(eng, nm)
    for k in eng.D.spec:
        t["p." + k], t["g." + k] = eng.D.p[k], eng.D.g[k]
    return t


def spy_riders(eng):
    """Record what every _conv5s2 launch carried: [(kind, weight, rows, _Riders)]."""
    seen, real = [], eng._conv5s2

    def spy(kind, x, fp, name, y, **kw):
        r = real(kind, x, fp, name, y, **kw)
        # the partial statistics live in a workspace the next such launch reuses: copied here
        part = r.parts[0][:3 * r.parts[1] * y.shape[-1]].clone() if r.parts is not None else None
        seen.append((kind, name, x.shape[0], r, part))
        return r
    eng._conv5s2 = spy
    return seen


def critic_substep(eng, cfg, riders, call=None):
    """NaN-prefill, d_backward(), snapshot, judge the critic part: (table, {output: worst error / bound})."""
    B, live = eng.B, critic_live(eng)
    for n, t in live.items():
        if n not in ("real", "fake_d", "alpha", "emb_d", "X3") and not n.startswith(("p.", "g.")):
            t.fill_(float("nan"))
    eng.D.grad[:eng.D.n].fill_(float("nan"))
    pre = snapshot(live)
    del riders[:]
    (call or eng.d_backward)()
    torch.cuda.synchronize()
    assert bool((eng.D.grad[eng.D.n:] == 0).all())
    pooled = {rows: r.pooled for kind, name, rows, r, _ in riders if kind == "conv_fwd" and name == "conv.4.weight"}
    hp = E.critic_hp(B, eng.T, cfg["LAMBDA_GP"], pooled=pooled[3 * B], pooled_tan=pooled[B])
    table = E.critic_table(hp)
    return table, hp, E.judge(table, pre, snapshot(live), hp)


@pytest.mark.parametrize("chains", ("1", "0"), ids=("chains", "no-chains"))
@pytest.mark.parametrize("cfg3", E.GAN_CRITIC_CONFIGS + (E.GAN_COND_LATENT_CONFIG, E.GAN_BF16_ED_CONFIG), ids=str)
def test_gan_critic_step_and_updates_two_free_running_steps(ops, hook, monkeypatch, cfg3, chains):
    C, T, B = cfg3
    monkeypatch.setenv("MELO_CHAINS", chains)
    eng, cfg, _ = gan_engine(C, T, B)
    riders = spy_riders(eng)
    # the routes this configuration is here for
    assert eng._chain_d == eng._chain_e == (chains == "1")
    assert (("conv.0.weight", "fwd") in eng.wq) == (C % 16 == 0) and ("conv.4.weight", "dgrad") in eng.wq
    assert (eng.dn_dense is not None) == (T % 8 != 0)
    assert (eng.mode == "conditioning") == (eng.ed_mode == "latent") == (cfg3 == E.GAN_COND_LATENT_CONFIG)
    assert (eng.ed_dtype == "bf16") == (cfg3 == E.GAN_BF16_ED_CONFIG)
    ed_fold_check(eng, f"{cfg3}")
    # the frozen classifier's three-tap layers go through F(2,3) where the layer is wide enough and the roll even
    ROUTES.setdefault(("wino f/d", C, T, B), set()).add((tuple(eng.ed_wino_f), tuple(eng.ed_wino_d)))
    for it in range(2):
        R = O.step_randoms(B, cfg["NOISE_DIM"], seed=1 + it)
        eng.set_randoms(R["noise_d"].cuda(), [m.cuda() for m in R["dm_d"]], R["alpha"].cuda())
        hook.seen.clear()
        ftable, fhp = forward_table(eng, 1)
        flive, fpre = forward_prefill(eng, "d", ftable)
        table, hp, ratios = critic_substep(eng, cfg, riders)
        forward_judge(eng, "d", riders, flive, fpre, f"{cfg3} chains={chains} step {it + 1} critic-step half")
        assert ("row_chain_kernel" in hook.seen) == (chains == "1"), hook.seen
        # the pooled mean rides in conv.4's launch exactly at the configuration chosen for it (3B rows and B rows alike),
        # and x_hat in the last deconvolution's exactly where conv16 runs that layer over the whole time axis
        assert hp["pooled"] == hp["pooled_tan"] == (T == 256), (hp["pooled"], hp["pooled_tan"])
        mixed = [r.mixed for kind, name, rows, r, _ in riders if name == "G.decoder.deconv.6.weight"]
        assert mixed == [eng._mix_fused] and eng._mix_fused == (C % 32 == 0 and T % 8 == 0), (mixed, eng._mix_fused)
        section = {n: st.section for st in table for n in st.outs}
        for n, r in ratios.items():
            record("GAN " + section[n], r, f"{cfg3} chains={chains} step {it + 1} {n}")
        bad = {n: r for n, r in ratios.items() if not r <= 1.0}
        assert not bad, f"{cfg3} chains={chains} step {it + 1} d_backward: stages above their bound: {bad}"
        for X, upd in (("D", eng.d_update), ("GE", eng.g_update)):
            if X == "GE":
                eng.set_randoms(R["noise_g"].cuda(), [m.cuda() for m in R["dm_g"]])
                _, ratios = g_step_substeps(eng, cfg, riders, f"{cfg3} chains={chains} step {it + 1}", ops=ops, chains=chains == "1")
                bad = {n: r for n, r in ratios.items() if not r <= 1.0}
                assert not bad, f"{cfg3} chains={chains} step {it + 1} generator step: stages above their bound: {bad}"
            table, ratios = gan_update_substep(eng, cfg, X, upd)
            for n, r in ratios.items():
                record("GAN update " + ("Adam" if n.startswith(X + ".") else "re-layout"), r, f"{cfg3} step {it + 1} {X} {n}")
            bad = {n: r for n, r in ratios.items() if not r <= 1.0}
            assert not bad, f"{cfg3} step {it + 1} {X}: stages above their bound: {bad}"
            assert float((eng.D if X == "D" else eng.GE).state[0]) == it + 1


@pytest.mark.parametrize("chains", ("1", "0"), ids=("chains", "no-chains"))
@pytest.mark.parametrize("cfg3", ((128, 64, 4), (4, 20, 3)), ids=str)
def test_gan_fused_flow_constituents_by_hand(ops, hook, monkeypatch, cfg3, chains):
    """dg_step_rng's constituents called by hand in its order, two free-running steps, from the randoms the DEVICE draws
    (read back from the engine's buffers, which is where every stage takes its inputs from): the draw with its two Adam-state
    riders, the 2B-row generator pass with two BatchNorm groups, d_backward(forward=False), d_update on the already advanced
    state, the generator step's backward on rows [B:2B] of the `*_2` buffers, g_update; and the launches they issue are
    exactly the ones dg_step_rng issues."""
    C, T, B = cfg3
    monkeypatch.setenv("MELO_CHAINS", chains)
    eng, cfg, _ = gan_engine(C, T, B)
    riders = spy_riders(eng)
    ftable, fhp = forward_table(eng, 2)
    hand = []
    for it in range(2):
        what = f"{cfg3} chains={chains} fused step {it + 1}"
        hook.seen.clear()
        drawn = [eng.noise_2, eng.alpha] + list(eng.dmask_2)
        for t in drawn:
            t.fill_(float("nan"))
        states = [eng.D.state.clone(), eng.GE.state.clone()]
        step0 = int(eng.rng_step.item())
        eng.draw_randoms_both()
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(t).all()) for t in drawn), what + ": the draw left a buffer unwritten"
        assert all(bool(((m == 0) | ((m - 1.25).abs() < 1e-6)).all()) and 0.5 < float((m > 0).float().mean()) < 0.95 for m in eng.dmask_2), what
        assert bool(((eng.alpha >= 0) & (eng.alpha < 1)).all()) and not torch.equal(eng.noise_2[:B], eng.noise_2[B:])
        for fp, s0 in zip((eng.D, eng.GE), states):         # both optimisers' step states advanced by the draw, once
            assert S.worst(fp.state, E.adam_state_ref(s0, *eng.betas))[0] <= 1.0 and float(fp.state[0]) == it + 1, what
        assert eng.D.ticked is True and eng.GE.ticked == "nobump" and int(eng.rng_step.item()) == step0
        flive, fpre = forward_prefill(eng, "both", ftable)
        eng.X0[:B].fill_(float("nan"))
        del riders[:]
        eng.dg_forward()
        torch.cuda.synchronize()
        forward_judge(eng, "both", riders, flive, fpre, what + " 2B-row pass")
        assert eng.num_batches_tracked == 2 * (it + 1)
        xhat = eng.X0[:B].clone()
        table, hp, ratios = critic_substep(eng, cfg, riders, call=lambda: (eng.X0[:B].copy_(xhat), eng.d_backward(forward=False)))
        section = {n: st.section for st in table for n in st.outs}
        for n, r in ratios.items():
            record("GAN " + section[n], r, f"{what} {n}")
        bad = {n: r for n, r in ratios.items() if not r <= 1.0}
        assert not bad, f"{what} d_backward(forward=False): stages above their bound: {bad}"
        for X, upd in (("D", eng.d_update), ("GE", eng.g_update)):
            if X == "GE":       # g_backward_a2 (= g_ed_branch + g_critic_front + g_critic_back) and g_backward_b, judged
                _, ratios = g_step_substeps(eng, cfg, riders, what, forward=False, ops=ops, chains=chains == "1")
                bad = {n: r for n, r in ratios.items() if not r <= 1.0}
                assert not bad, f"{what} generator backward: stages above their bound: {bad}"
            table, ratios = gan_update_substep(eng, cfg, X, upd)
            for n, r in ratios.items():
                record("GAN update " + ("Adam" if n.startswith(X + ".") else "re-layout"), r, f"{what} {X} {n}")
            bad = {n: r for n, r in ratios.items() if not r <= 1.0}
            assert not bad, f"{what} {X}: stages above their bound: {bad}"
            assert float((eng.D if X == "D" else eng.GE).state[0]) == it + 1       # advanced by the draw, not again
        assert int(eng.rng_step.item()) == step0 + 1 and not eng.D.ticked and not eng.GE.ticked     # the critic's update bumps it
        hand.append(list(hook.seen))
    assert hand[0] == hand[1]
    hook.seen.clear()
    eng.dg_step_rng()
    torch.cuda.synchronize()
    assert list(hook.seen) == hand[0], (list(hook.seen), hand[0])       # launch for launch, the draw included


def _mut_ds_swapped(ops, eng):
    B = eng.B
    eng.ds_d.copy_(torch.cat([eng.ds_d[:B], eng.ds_d[2 * B:], eng.ds_d[B:2 * B]]))
    return None, None


def _mut_tangent_job_dropped(ops, eng):
    real = ops.conv1d_wgrad

    def f(x, dy, dw, stride, x2=None, dy2=None, **kw):
        if dw is eng.D.g["conv.2.weight"]:
            x2 = dy2 = None
        return real(x, dy, dw, stride, x2, dy2, **kw)
    return "conv1d_wgrad", f


def _mut_tangent_mask_other_rows(ops, eng):
    real = ops.conv1d_fwd

    def f(x, w, y, stride, **epi):
        if x is eng.TAN0 and epi.get("gref") is not None:
            epi["gref"] = eng.A1[eng.B:2 * eng.B]       # the real rows' mask: same shape, the other third
        return real(x, w, y, stride, **epi)
    return "conv1d_fwd", f


def test_dnotes_accumulate_forced_off_is_flagged_at_dnotes(ops, monkeypatch):
    C, T, B = E.GAN_CRITIC_CONFIGS[0]
    eng, cfg, _ = gan_engine(C, T, B)
    riders = spy_riders(eng)
    R = O.step_randoms(B, cfg["NOISE_DIM"], seed=1)
    eng.set_randoms(R["noise_g"].cuda(), [m.cuda() for m in R["dm_g"]])
    real = ops.conv1d_dgrad

    def f(dy, w, dx, stride, **epi):
        if dx is eng.dnotes and stride == 2:          # the critic path's launch (the emotion branch's has stride 1)
            assert epi.pop("accumulate") is True
        return real(dy, w, dx, stride, **epi)
    with monkeypatch.context() as m:
        m.setattr(ops, "conv1d_dgrad", f)
        table, ratios = g_step_substeps(eng, cfg, riders, "mutation")
    assert flagged({"g": ratios}, {"g": table}) == {"dnotes"}


CRITIC_MUTATIONS = OrderedDict([
    ("ds_d: real and fake swapped", (_mut_ds_swapped, {"dU", "g.real_fake.weight+g.real_fake.bias+loss_d_out+gp"})),
    ("the tangent segment dropped from conv.2's wgrad_multi job", (_mut_tangent_job_dropped, {"g.conv.2.weight+g.conv.2.bias"})),
    ("TAN1: gref from the other third of A1", (_mut_tangent_mask_other_rows, {"TAN1"})),
])


@pytest.mark.parametrize("name", list(CRITIC_MUTATIONS), ids=lambda s: s.replace(" ", "_"))
def test_critic_mutation_is_flagged_at_its_stage(ops, monkeypatch, name):
    make, stages = CRITIC_MUTATIONS[name]
    C, T, B = E.GAN_CRITIC_CONFIGS[0]
    eng, cfg, _ = gan_engine(C, T, B)
    riders = spy_riders(eng)
    R = O.step_randoms(B, cfg["NOISE_DIM"], seed=1)
    eng.set_randoms(R["noise_d"].cuda(), [m.cuda() for m in R["dm_d"]], R["alpha"].cuda())
    attr, fn = make(ops, eng)
    with monkeypatch.context() as m:
        if attr:
            m.setattr(ops, attr, fn)
        table, hp, ratios = critic_substep(eng, cfg, riders)
    assert flagged({"d": ratios}, {"d": table}) == stages, (name, flagged({"d": ratios}, {"d": table}))


def test_g_update_moves_the_ema_shadow(ops):
    """EMA_DECAY > 0: the fp64 shadow behind the generator's update, two free-running steps (the ramp's first two decays),
    exactly; a second launch of the shadow's update is flagged there and nowhere else."""
    C, T, B = E.GAN_CRITIC_CONFIGS[0]
    eng, cfg, _ = gan_engine(C, T, B, ema_decay=0.999)
    assert eng.ema is not None and eng.ema_ramp
    for it in range(2):
        R = O.step_randoms(B, cfg["NOISE_DIM"], seed=1 + it)
        gan_half_step(eng, cfg, R, "D")
        eng.d_update()
        gan_half_step(eng, cfg, R, "GE")
        table, ratios = gan_update_substep(eng, cfg, "GE", eng.g_update)
        assert "ema" in ratios and not {n: r for n, r in ratios.items() if not r <= 1.0}, ratios
    R = O.step_randoms(B, cfg["NOISE_DIM"], seed=3)
    gan_half_step(eng, cfg, R, "GE")

    def twice():
        eng.g_update()
        ops.ema_flat(eng.GE.data, eng.ema, eng.GE.n, eng.ema_decay, eng.ema_ramp, eng.GE.state, eng.ema_offset)
    table, ratios = gan_update_substep(eng, cfg, "GE", twice)
    assert flagged({"u": ratios}, {"u": table}) == {"ema"}


def test_gan_update_mutations_are_flagged_at_their_stage(ops, monkeypatch):
    C, T, B = E.GAN_UPDATE_CONFIGS[0]
    eng, cfg, St = gan_engine(C, T, B)
    R = O.step_randoms(B, cfg["NOISE_DIM"], seed=1)
    gan_half_step(eng, cfg, R, "D")
    attr, fn = _mut_grad_scale_doubled(ops, eng)
    with monkeypatch.context() as m:
        m.setattr(ops, attr, fn)
        table, ratios = gan_update_substep(eng, cfg, "D", eng.d_update)
    assert flagged({"update": ratios}, {"update": table}) == {"D.data+D.m+D.v+D.state"}
    # parameters written from outside with params_changed() skipped: every re-laid copy of the critic is stale, nothing
    # else is; with it, nothing is
    eng.D.load(OrderedDict((k, v * 1.5) for k, v in St.PD.items()))
    torch.cuda.synchronize()
    table, hp = gan_update_table(eng, cfg, "D")
    wq_stages = [st for st in table if st.outs[0].startswith("wq.")]
    live = snapshot(gan_update_live(eng, "D"))
    assert flagged({"update": E.judge(wq_stages, live, live, hp)}, {"update": table}) == {st.name for st in wq_stages}
    eng.params_changed()
    torch.cuda.synchronize()
    live = snapshot(gan_update_live(eng, "D"))
    assert not flagged({"update": E.judge(wq_stages, live, live, hp)}, {"update": table})


def test_params_changed_skipped_before_step_2_is_flagged_at_the_launches_that_read_a_copy(ops):
    """Step 1 runs clean; then the critic's parameters are written from outside and params_changed() is skipped, so step 2's
    d_backward runs with step 1's re-laid copies: exactly the convolution stages whose launch reads a copy (conv16 runs it)
    leave their bound -- every other stage, the weight gradients included, is referenced from its own stored inputs and the
    CURRENT parameters and stays inside.  With params_changed() the same step is clean."""
    C, T, B = 128, 64, 4
    eng, cfg, St = gan_engine(C, T, B)
    riders = spy_riders(eng)
    R = O.step_randoms(B, cfg["NOISE_DIM"], seed=1)
    eng.set_randoms(R["noise_d"].cuda(), [m.cuda() for m in R["dm_d"]], R["alpha"].cuda())
    table, hp, ratios = critic_substep(eng, cfg, riders)
    assert not flagged({"d": ratios}, {"d": table})
    eng.d_update()
    eng.D.load(OrderedDict((k, v * 1.25) for k, v in St.PD.items()))
    T1, T2, T3 = eng.T1, eng.T2, eng.T3
    sup = lambda name, d, *a: (name, d) in eng.wq and bool(ops.conv16_supported(*a))  # noqa: E731
    reads_copy = {"A1": sup("conv.0.weight", "fwd", 3 * B, T, C, 64, False, 0), "A2": sup("conv.2.weight", "fwd", 3 * B, T1, 64, 128, False, 0),
                  "A3": sup("conv.4.weight", "fwd", 3 * B, T2, 128, 256, False, 0),
                  "dZ2": sup("conv.4.weight", "dgrad", 3 * B, T3, 256, 128, True, T2), "dZ1": sup("conv.2.weight", "dgrad", 3 * B, T2, 128, 64, True, T1),
                  "gx": sup("conv.0.weight", "dgrad", B, T1, 64, C, True, T),
                  "TAN1": sup("conv.0.weight", "fwd", B, T, C, 64, False, 0), "TAN2": sup("conv.2.weight", "fwd", B, T1, 64, 128, False, 0),
                  "TZ3": sup("conv.4.weight", "fwd", B, T2, 128, 256, False, 0)}
    want = {n for n, on in reads_copy.items() if on}
    assert {"A2", "A3", "dZ2", "dZ1", "TAN2", "TZ3"} <= want, want
    table, hp, ratios = critic_substep(eng, cfg, riders)
    assert flagged({"d": ratios}, {"d": table}) == want, (flagged({"d": ratios}, {"d": table}), want)
    eng.params_changed()
    table, hp, ratios = critic_substep(eng, cfg, riders)
    assert not flagged({"d": ratios}, {"d": table})
