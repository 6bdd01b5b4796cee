"""The row chain's non-Linear ops (csrc/row_chain.hip), the fused MLP step (csrc/mlp_train.hip) and spectral normalisation
(csrc/small_kernels.hip) against the fp64 references of tests/rowstep_ref.py, ELEMENT BY ELEMENT, at the shapes of its tables
(tests/test_rowstep_ref.py shows on the host which kernel paths those reach, that fp32 host computations stay inside the
bounds and that plausible mistakes leave them).  Outputs go into NaN-prefilled guarded canvases; every chain launch asserts
through the launch hook that row_chain_kernel ran (the MLP and spectral-norm entry points report to no hook: they have one
kernel each).  Every stage is referenced from the kernel's own stored upstream tensors, so each bound is a one-stage count.
The worst error / bound of every section is printed (pytest -s) and quoted in DESIGN.md §2."""
import contextlib

import pytest
import torch

import rowstep_ref as R
import support_ref as S

pytestmark = pytest.mark.gpu

GELU = S.ACT_GELU
SECTIONS = {}


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


class Worst:
    """Keeps the worst error / bound ratio of a section; the module prints all sections when it is over."""

    def __init__(self, section):
        self.section = section
        SECTIONS.setdefault(section, [0, 0.0, ""])

    def check(self, got, ref, what):
        r = R.check(got, ref, what)
        s = SECTIONS[self.section]
        s[0] += 1
        if r >= s[1]:
            s[1], s[2] = r, what
        return r


def teardown_module(module):
    for k, (n, r, what) in SECTIONS.items():
        print(f"\n[rowstep contract] {k}: {n} checks, worst error / bound = {r:.4f} ({what})")


def launch(ch, hook):
    hook.seen.clear()
    ch.launch()
    assert hook.seen == ["row_chain_kernel"], hook.seen


def wide(rows, n, lead=3):
    """A guarded (rows, lead + n) canvas and its column block [:, lead:]."""
    g = S.Guarded((rows, lead + n))
    return g, g.t[:, lead:]


def block_only(g, lead, what):
    assert bool(torch.isnan(g.t[:, :lead]).all()), what + ": wrote outside its column block"
    g.check(what)


def into(shape, src):
    """A guarded canvas holding a copy of src (an in / out tensor of a kernel)."""
    g = S.Guarded(shape)
    g.t.copy_(src)
    return g


# ---------------------------------------------------------------------------------------------------------------------
# a. row chain
# ---------------------------------------------------------------------------------------------------------------------
def test_mean_t(ops, hook):
    worst = Worst("a. chain MEAN_T")
    for rows in R.CHAIN_ROWS:
        for T, C, off in R.MEANT_VEC + R.MEANT_SCALAR:
            a = R.meant_input(rows, T, C).cuda()
            if off:
                buf = torch.empty(a.numel() + off, device="cuda")
                v = buf[off:].view(a.shape)
                v.copy_(a)
                a = v
            plan = R.meant_plan(T, C, off)
            assert plan["vec"] == (C % 4 == 0 and C >= 16 and a.data_ptr() % 16 == 0)
            g, out = wide(rows, C)
            slot = S.Guarded((rows, C))
            what = f"mean_t rows={rows} T={T} C={C} off={off} vec={plan['vec']}"
            launch(ops.Chain(rows).mean_t(2, a, out=out).store(2, slot.t), hook)
            worst.check(out, R.meanT(a), what)
            assert torch.equal(slot.t, out), what + ": the slot and the stored rows differ"
            block_only(g, 3, what)
            slot.check(what)


def test_layernorm(ops, hook):
    worst = Worst("a. chain LAYERNORM")
    i = 0
    for rows in R.CHAIN_ROWS:
        for D in R.LN_D:
            for kind in R.LN_KINDS:
                x, gm, bt = (t.cuda() for t in R.ln_input(rows, D, kind))
                ry, rxh = R.layernorm(x, gm, bt)
                for variant in (i % 4, (i + 2) % 4):          # 0: xhat and y; 1: y only; 2: xhat only, in place; 3: neither, in place
                    xh, y = (wide(rows, D) if variant in (0, 2) else None), (wide(rows, D) if variant in (0, 1) else None)
                    a, b = 1, (1 if variant >= 2 else 4)
                    slot = S.Guarded((rows, D))
                    what = f"layernorm rows={rows} D={D} {kind} variant={variant}"
                    ch = ops.Chain(rows).load(a, x).layernorm(a, b, gm, bt, xhat=xh[1] if xh else None, y=y[1] if y else None)
                    launch(ch.store(b, slot.t), hook)
                    worst.check(slot.t, ry, what + " slot")
                    slot.check(what)
                    if xh:
                        worst.check(xh[1], rxh, what + " xhat")
                        block_only(xh[0], 3, what)
                    if y:
                        assert torch.equal(y[1], slot.t), what + ": y rows and the slot differ"
                        block_only(y[0], 3, what)
                i += 1


def test_softmax_ce(ops, hook):
    worst = Worst("a. chain SOFTMAX_CE")
    i = 0
    for rows in R.CHAIN_ROWS:
        for C in R.CE_C:
            for kind in R.CE_KINDS:
                z, y = (t.cuda() for t in R.ce_input(rows, C, kind))
                for coef, bad in ((1.0, "none"), (0.37, R.CE_BAD[i % 3])):
                    tgt = y.clone()
                    if bad != "none":
                        tgt[rows - 1] = C if bad is None else bad
                    lr, (g, dl) = S.Guarded((rows,)), wide(rows, C)
                    what = f"softmax_ce rows={rows} C={C} {kind} coef={coef} bad={bad}"
                    launch(ops.Chain(rows).load(0, z).softmax_ce(0, 1, tgt, lr.t, coef, C).store(1, dl), hook)
                    rl, rd, isbad = R.ce_rows(z, tgt, coef)
                    ok = ~isbad
                    assert int(isbad.sum()) == (bad != "none")
                    assert bool(torch.isnan(lr.t[isbad]).all()) and bool(torch.isnan(dl[isbad]).all()), what + ": a bad target must poison its row"
                    if ok.any():
                        worst.check(lr.t[ok], S.mk(rl.val[ok], rl.mag[ok], 0, 1, rl.eps_abs[ok]), what + " loss")
                        sub = S.mk(rd.val[ok], rd.mag[ok], 0, rd.k_epi, rd.eps_abs[ok])
                        worst.check(dl[ok], sub, what + " gradient")
                    lr.check(what)
                    block_only(g, 3, what)
                i += 1


def test_critic_head(ops, hook):
    worst = Worst("a. chain DHEAD")
    for rows in R.CHAIN_ROWS:
        for Fd, E, Be in R.DHEAD:
            f, emb, w, bias, ds = (t.cuda() if t is not None else None for t in R.dhead_input(rows, Fd, E, Be))
            for with_demb in ((False, True) if E and emb.shape[0] == rows else (False,)):
                s, (g, dU) = S.Guarded((rows,)), wide(rows, Fd)
                de = wide(rows, E) if with_demb else None
                what = f"dhead rows={rows} F={Fd} E={E} emb rows={0 if emb is None else emb.shape[0]} demb={with_demb}"
                launch(ops.Chain(rows).load(0, f).dhead(0, 1, w, bias, emb, ds, s.t, demb=de[1] if de else None).store(1, dU), hook)
                rs, rdU, rde = R.dhead(f, emb, w, bias, ds, with_demb)
                worst.check(s.t, rs, what + " s")
                worst.check(dU, rdU, what + " dU")
                s.check(what)
                block_only(g, 3, what)
                if de:
                    worst.check(de[1], rde, what + " demb")
                    block_only(de[0], 3, what)


def test_load_copy_store_are_exact(ops, hook):
    for rows in R.CHAIN_ROWS:
        g_ = R.gen(rows)
        A, Bm, Cc = (torch.randn(n, 40, generator=g_).cuda() for n in (rows, 2, rows))
        idx = torch.arange(rows, device="cuda") % 2
        # plain: a column block in, a column block out, n below both widths
        g, out = wide(rows, 30)
        launch(ops.Chain(rows).load(3, A[:, 5:], n=30).store(3, out), hook)
        assert torch.equal(out, A[:, 5:35])
        block_only(g, 3, "load / store")
        # at > 0, accumulate, mod, copy with both offsets, store of fewer elements than were loaded
        g, out = wide(rows, 32)
        ch = ops.Chain(rows).load(0, A, n=24, at=5).load(0, Bm, n=24, accumulate=True, mod=2, at=5).load(1, Cc, n=40)
        launch(ch.copy(0, 1, 20, src_at=7, dst_at=3).store(1, out, n=32), hook)
        want = Cc[:, :32].clone()
        want[:, 3:23] = (A[:, :24] + Bm[idx][:, :24])[:, 2:22]
        assert torch.equal(out, want)
        block_only(g, 3, "load(at, accumulate, mod) / copy / store")
        # accumulate twice on top of a plain load: (A + A) + Bm, in that order
        g, out = wide(rows, 40)
        launch(ops.Chain(rows).load(5, A).load(5, A, accumulate=True).load(5, Bm, accumulate=True, mod=2).store(5, out), hook)
        assert torch.equal(out, (A + A) + Bm[idx])
        block_only(g, 3, "load accumulate")


def test_composed_chain_stage_by_stage(ops, hook):
    """The numeric encoder's shape: LayerNorm(6) -> three Linears with GELU and masks -> store, then its data gradients;
    every intermediate against the reference built from the kernel's own previous stage, so a slot hand-off error shows."""
    worst = Worst("a. chain composed")
    dims = [6, 256, 128, 128]
    for rows in R.CHAIN_ROWS:
        gen = R.gen(40 + rows)
        x = torch.randn(rows, 6, generator=gen).cuda()
        gm, bt = (torch.randn(6, generator=gen).abs() + 0.5).cuda(), torch.randn(6, generator=gen).cuda()
        ws = [(torch.randn(o, i, generator=gen) / i ** 0.5).cuda() for i, o in zip(dims, dims[1:])]
        bs = [(torch.randn(o, generator=gen) * 0.1).cuda() for o in dims[1:]]
        ms = [((torch.rand(rows, o, generator=gen) > 0.2).float() / 0.8).cuda() for o in dims[1:]]
        assert ops.Chain.weights_ok(*ws)
        ln = S.Guarded((rows, 6))
        zs, outs = [S.Guarded((rows, o)) for o in dims[1:]], [S.Guarded((rows, o)) for o in dims[1:]]
        fin = S.Guarded((rows, 128))
        ch = ops.Chain(rows).load(0, x).layernorm(0, 1, gm, bt, y=ln.t)
        for l in range(3):
            ch.linear_fwd(1 + l, 2 + l, ws[l], bs[l], GELU, ms[l], zout=zs[l].t, out=outs[l].t)
        launch(ch.store(4, fin.t), hook)
        what = f"composed rows={rows}"
        worst.check(ln.t, R.layernorm(x, gm, bt)[0], what + " layernorm")
        prev = ln.t
        for l in range(3):
            ref = R.lin_fwd(prev, ws[l], bs[l], GELU, ms[l])
            worst.check(zs[l].t, ref.z, what + f" z{l}")
            # the activation from the STORED pre-activation
            worst.check(outs[l].t, S.act_on(S.mk(zs[l].t.double(), zs[l].t.double().abs(), 0, 0), GELU).epilogue(emul=ms[l]), what + f" a{l}")
            prev = outs[l].t
        assert torch.equal(fin.t, outs[2].t)
        for gd in [ln, fin] + zs + outs:
            gd.check(what)
        # data gradients back to the LayerNorm output: vec branch twice, then the few-outputs branch (IN = 6)
        assert [R.dgrad_branch(n) for n in (128, 256, 6)] == ["vec", "vec", "rows"]
        dy = torch.randn(rows, 128, generator=gen).cuda()
        ds_ = [S.Guarded((rows, n)) for n in (128, 256, 6)]
        ch = ops.Chain(rows).load(0, dy).linear_dgrad(0, 1, ws[2], gref=zs[1].t, gact=GELU, mask=ms[1], out=ds_[0].t)
        ch.linear_dgrad(1, 2, ws[1], gref=zs[0].t, gact=GELU, mask=ms[0], out=ds_[1].t).linear_dgrad(2, 3, ws[0], out=ds_[2].t)
        launch(ch, hook)
        up = dy
        for j, (w, gref, m) in enumerate(((ws[2], zs[1].t, ms[1]), (ws[1], zs[0].t, ms[0]), (ws[0], None, None))):
            ref = R.W.Ref(*R.W.linear_dgrad(up, w), w.shape[0])
            if gref is not None:
                ref.epilogue(gref=gref, gact=GELU, emul=m)
            worst.check(ds_[j].t, ref, what + f" dgrad {j}")
            ds_[j].check(what)
            up = ds_[j].t


# ---------------------------------------------------------------------------------------------------------------------
# b. the fused MLP step
# ---------------------------------------------------------------------------------------------------------------------
LR, BETAS, WD = 1e-3, (0.5, 0.999), 0.01


def mlp_device(ops, name, rows, aligned):
    h = R.mlp_problem(name, rows)
    w_off, b_off, n = R.flat_layout(h["ws"], h["bs"], aligned)
    flat = torch.zeros(n)
    for off, t in zip(w_off + b_off, h["ws"] + h["bs"]):
        flat[off:off + t.numel()] = t.flatten()
    flat = flat.cuda()
    assert flat.data_ptr() % 16 == 0
    wv = [flat[o:o + w.numel()].view(w.shape) for o, w in zip(w_off, h["ws"])]
    bv = [flat[o:o + b.numel()] for o, b in zip(b_off, h["bs"])]
    plan = R.mlp_plan(h["in_dim"], h["hidden"], h["C"], rows, w_off, b_off)
    for ly, w in zip(plan["layers"], wv):          # launch A's `vec`, recomputed on the tensor the launch gets
        assert ly["vec"] == (w.shape[1] % 4 == 0 and w.data_ptr() % 16 == 0) == (aligned and w.shape[1] % 4 == 0)
    named = torch.zeros(n, dtype=torch.bool, device="cuda")
    for off, t in zip(w_off + b_off, h["ws"] + h["bs"]):
        named[off:off + t.numel()] = True
    G = lambda *s: S.Guarded(s)  # noqa: E731
    C = h["C"]
    dev = dict(flat=flat, wv=wv, bv=bv, x=h["x"].cuda(), y=h["y"].cuda(), mask=[m.cuda() for m in h["masks"]], named=named,
               z=[G(rows, w) for w in h["hidden"]], a=[G(rows, w) for w in h["hidden"]], dz=[G(rows, w) for w in h["hidden"]],
               logits=G(rows, C), dlogits=G(rows, C), loss_rows=G(rows), loss=G(1), g=torch.full((n,), float("nan"), device="cuda"),
               w_off=w_off, b_off=b_off, plan=plan)
    t = lambda lst: [q.t for q in lst]  # noqa: E731
    net = ops.MlpNet(rows, wv, bv, t(dev["z"]), t(dev["a"]), t(dev["dz"]), dev["mask"])
    return h, dev, net


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "odd"])
@pytest.mark.parametrize("name,rows", R.MLP_CASES)
def test_mlp_step(ops, name, rows, aligned):
    h, d, net = mlp_device(ops, name, rows, aligned)
    L, C = len(h["hidden"]), h["C"]
    what = f"mlp {name} rows={rows} {'aligned' if aligned else 'odd'}"
    state = torch.zeros(4, dtype=torch.float64, device="cuda")
    ops.mlp_cls_fwd_bwd(net, d["x"], d["y"], d["logits"].t, d["loss_rows"].t, d["dlogits"].t, train=True, tick_state=state, betas=BETAS)
    assert state.tolist()[:3] == [1.0, S.f32(BETAS[0]), S.f32(BETAS[1])]
    ops.mlp_cls_wgrad_update(net, d["x"], d["dlogits"].t, d["w_off"], d["b_off"], d["g"], d["loss_rows"].t, d["loss"].t)
    st = dict(z=[q.t for q in d["z"]], a=[q.t for q in d["a"]], dz=[q.t for q in d["dz"]], logits=d["logits"].t,
              loss_rows=d["loss_rows"].t, dlogits=d["dlogits"].t)
    wa, wb = Worst("b. MLP launch A"), Worst("b. MLP launch B")
    for k, ref in R.mlp_stages(d["wv"], d["bv"], d["x"], d["y"], d["mask"], st).items():
        got = st[k] if k in st else st[k[:-1]][int(k[-1])]
        wa.check(got, ref, f"{what} {k}")
    refs_b = R.mlp_params(d["wv"], d["x"], st)
    for l in range(L + 1):
        gw = d["g"][d["w_off"][l]:d["w_off"][l] + d["wv"][l].numel()].view(d["wv"][l].shape)
        gb = d["g"][d["b_off"][l]:d["b_off"][l] + d["bv"][l].numel()]
        wb.check(gw, refs_b[f"dW{l}"], f"{what} dW{l}")
        wb.check(gb, refs_b[f"db{l}"], f"{what} db{l}")
    wb.check(d["loss"].t, refs_b["loss"], what + " loss")
    assert bool(torch.isnan(d["g"][~d["named"]]).all()), what + ": the gradient buffer was written outside the named tensors"
    for k in ("z", "a", "dz"):
        for q in d[k]:
            q.check(what + " " + k)
    for k in ("logits", "dlogits", "loss_rows", "loss"):
        d[k].check(what + " " + k)

    # eval mode: the same weights without masks; nothing but logits and loss_rows is written
    lg, lrw = S.Guarded((rows, C)), S.Guarded((rows,))
    ops.mlp_cls_fwd_bwd(ops.MlpNet(rows, d["wv"], d["bv"]), d["x"], d["y"], lg.t, lrw.t, None, train=False)
    we = Worst("b. MLP eval")
    we.check(lg.t, R.mlp_eval(d["wv"], d["bv"], d["x"]), what + " eval logits")
    we.check(lrw.t, R.ce_rows(lg.t, d["y"])[0], what + " eval loss_rows")
    lg.check(what)
    lrw.check(what)

    # apply mode with the metrics rider on logits that hold a NaN (rows > 1: one row of them)
    n = d["flat"].numel()
    gen = R.gen(7)
    m, v = (torch.randn(n, generator=gen) * 1e-3).cuda(), (torch.rand(n, generator=gen) * 1e-6).cuda()
    p0, m0, v0 = d["flat"].clone(), m.clone(), v.clone()
    mlog = d["logits"].t.clone()
    mlog[rows // 2, C - 1] = float("nan")
    if rows > 1:
        mlog[0, 0] = float("inf")
    metrics = torch.tensor([2.0, 3.0], device="cuda")
    g1 = torch.full((n,), float("nan"), device="cuda")
    ctr = torch.tensor([41], dtype=torch.int64, device="cuda")
    loss2 = S.Guarded((1,))
    ops.mlp_cls_wgrad_update(net, d["x"], d["dlogits"].t, d["w_off"], d["b_off"], g1, d["loss_rows"].t, loss2.t,
                             adam=dict(p=d["flat"], m=m, v=v, state=state, lr=LR, betas=BETAS, weight_decay=WD), metrics=metrics,
                             logits=mlog, y=d["y"], rng_step=ctr)
    nm = d["named"]
    assert torch.equal(g1[nm], d["g"][nm]) and bool(torch.isnan(g1[~nm]).all()) and int(ctr.item()) == 42, what
    assert torch.equal(loss2.t, d["loss"].t)
    for got, before in ((d["flat"], p0), (m, m0), (v, v0)):
        assert torch.equal(got[~nm], before[~nm]), what + ": the update touched elements outside the named tensors"
    wu = Worst("b. MLP fused AdamW")
    rp, rm, rv = S.adam_step(p0[nm], g1[nm], m0[nm], v0[nm], 1, LR, BETAS[0], BETAS[1], 1e-8, WD)
    wu.check(d["flat"][nm], rp, what + " p")
    wu.check(m[nm], rm, what + " m")
    wu.check(v[nm], rv, what + " v")
    hits = int((R.argmax_nan_first(mlog) == d["y"].cpu()).sum())
    assert metrics[1].item() == 3.0 + hits, (what, metrics.tolist(), hits)
    ls = d["loss"].t.double() * rows
    Worst("b. MLP metrics rider").check(metrics[:1], S.mk(2.0 + ls, 2.0 + ls.abs(), 0, 2), what + " loss sum")


# ---------------------------------------------------------------------------------------------------------------------
# c. spectral norm
# ---------------------------------------------------------------------------------------------------------------------
def sn_job(Rr, C, seed=0):
    w, u0, v0, dw = (t.cuda() for t in R.sn_input(Rr, C, seed))
    g = dict(w_eff=S.Guarded((Rr, C)), u=into((Rr,), u0), v=into((C,), v0), sigma=S.Guarded((1,)), dw=into((Rr, C), dw))
    ly = dict(w_orig=w, w_eff=g["w_eff"].t, u=g["u"].t, v=g["v"].t, sigma=g["sigma"].t, dw=g["dw"].t)
    return dict(w=w, u0=u0, v0=v0, dw0=dw, g=g, ly=ly, what=f"spectral norm ({Rr}, {C})")


def sn_check_fwd(j, train, worst):
    st = {k: j["ly"][k] for k in ("u", "v", "sigma", "w_eff")}
    refs = R.sn_fwd(j["w"], j["u0"], j["v0"], st, train)
    for k, ref in refs.items():
        worst.check(st[k], ref, f"{j['what']} train={train} {k}")
    if not train:
        assert torch.equal(st["u"], j["u0"]) and torch.equal(st["v"], j["v0"]), j["what"] + ": eval mode moved the buffers"
    for k in ("w_eff", "u", "v", "sigma"):
        j["g"][k].check(j["what"] + " " + k)


def sn_check_bwd(j, worst):
    st = {k: j["ly"][k] for k in ("u", "v", "sigma", "w_eff")}
    worst.check(j["ly"]["dw"], R.sn_bwd(j["dw0"], st), j["what"] + " backward")
    j["g"]["dw"].check(j["what"] + " dw")


@pytest.mark.parametrize("shape", R.SN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_spectral_norm_forward_then_backward(ops, shape):
    wf, wb = Worst("c. spectral norm forward"), Worst("c. spectral norm backward")
    for train in (True, False):
        j = sn_job(*shape)
        ops.spectral_norm_fwd([j["ly"]], train)
        sn_check_fwd(j, train, wf)
        ops.spectral_norm_bwd([j["ly"]])
        sn_check_bwd(j, wb)


def test_spectral_norm_job_table(ops):
    """One launch carrying MG_MAX_SN_JOBS jobs of different shapes: every job against its own reference."""
    wf, wb = Worst("c. spectral norm, 8 jobs per launch"), Worst("c. spectral norm, 8 jobs per launch")
    shapes = R.SN_SHAPES + [(7, 3), (17, 65)]
    assert len(shapes) == R.MAX_SN_JOBS
    jobs = [sn_job(Rr, C, seed=i) for i, (Rr, C) in enumerate(shapes)]
    ops.spectral_norm_fwd([j["ly"] for j in jobs], True)
    for j in jobs:
        sn_check_fwd(j, True, wf)
    ops.spectral_norm_bwd([j["ly"] for j in jobs])
    for j in jobs:
        sn_check_bwd(j, wb)


# ---------------------------------------------------------------------------------------------------------------------
# d. the host refuses what the kernels do not handle
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(ops):
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    out = S.Guarded((4, 80))
    for build in (lambda c: c.load(0, z(4, 65)).layernorm(0, 1, z(65), z(65), y=out.t[:, :65]),          # LayerNorm beyond one wave
                  lambda c: c.mean_t(0, z(4, 0, 16), out=out.t[:, :16]),                                  # no time steps
                  lambda c: c.load(0, z(4, 8)).store(0, out.t, n=0)):                                     # an empty store
        with pytest.raises((ValueError, RuntimeError)):
            build(ops.Chain(4)).launch()
    with pytest.raises((ValueError, RuntimeError)):
        ops.Chain(0).load(0, z(1, 8)).launch()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.t).all())
    out.check("refused chains")
    ly = lambda r, c: dict(w_orig=z(r, c), w_eff=z(r, c), u=z(r), v=z(c), sigma=z(1), dw=z(r, c))  # noqa: E731
    for fn in (lambda l: ops.spectral_norm_fwd(l, True), ops.spectral_norm_bwd):
        with pytest.raises(ValueError):
            fn([ly(0, 4)])                                   # an empty weight: no rows
        with pytest.raises(ValueError):
            fn([ly(4, 0)])                                   # no columns
        with pytest.raises(ValueError):
            fn([dict(ly(3, 3), w_orig=torch.zeros((), device="cuda"))])
        with pytest.raises(ValueError):
            fn([ly(2, 2)] * (R.MAX_SN_JOBS + 1))
        with pytest.raises(ValueError):
            fn([dict(ly(3, 5), v=z(4))])
