"""Host self-test of tests/rowstep_ref.py (no GPU): (a) the references equal torch's fp64 modules / autograd at every table
shape; (b) the tables reach the kernel paths the GPU file is meant to reach, shown by recomputing the kernels' predicates;
(c) an fp32 host computation of every operation at every table shape stays inside its bound; (d) plausible mistakes, built
from the reference at table shapes, leave it.  The ratios of (c) and (d) are printed (pytest -s) and quoted in DESIGN.md §2."""
import torch
import torch.nn as nn
import torch.nn.functional as F

import rowstep_ref as R
import support_ref as S

U = S.U
FP32, MISTAKES = {}, {}


def ratio(got, ref):
    return R.worst(got, ref)[0]


def same(a, b, tol=1e-12):
    a, b = a.double(), b.double()
    ok = torch.isnan(a) == torch.isnan(b)
    return bool(ok.all()) and float((torch.nan_to_num(a) - torch.nan_to_num(b)).abs().max()) <= tol * (1.0 + float(torch.nan_to_num(b).abs().max()))


def note(table, key, r):
    table[key] = max(table.get(key, 0.0), r)


def teardown_module(module):
    for name, tab in (("fp32 emulation, worst error / bound", FP32), ("mistakes, worst error / bound", MISTAKES)):
        print(f"\n[rowstep ref] {name}")
        for k, v in tab.items():
            print(f"    {k}: {v:.4g}")


# ---------------------------------------------------------------------------------------------------------------------
# helpers: exact and fp32 runs of the MLP step and of spectral norm
# ---------------------------------------------------------------------------------------------------------------------
def mlp_run(h, dtype):
    """The step in `dtype` with torch; every stage computed from the previous stage's value ROUNDED TO fp32 (what a kernel
    stores), so the stored tensors are a consistent teacher-forcing set.  Returns fp32 st and the raw `dtype` values."""
    c = lambda t: t.to(dtype)  # noqa: E731
    L, rows = len(h["hidden"]), h["rows"]
    st, raw = dict(z=[], a=[], dz=[None] * L), dict(z=[], a=[], dz=[None] * L)
    prev = h["x"]
    for l in range(L):
        z = F.linear(c(prev), c(h["ws"][l]), c(h["bs"][l]))
        a = F.gelu(c(z.float())) * c(h["masks"][l])
        raw["z"].append(z), raw["a"].append(a), st["z"].append(z.float()), st["a"].append(a.float())
        prev = a.float()
    raw["logits"] = F.linear(c(prev), c(h["ws"][L]), c(h["bs"][L]))
    st["logits"] = raw["logits"].float()
    zl = c(st["logits"])
    raw["loss_rows"] = F.cross_entropy(zl, h["y"], reduction="none")
    raw["dlogits"] = (torch.softmax(zl, 1) - F.one_hot(h["y"], h["C"]).to(dtype)) / rows
    st["loss_rows"], st["dlogits"] = raw["loss_rows"].float(), raw["dlogits"].float()
    dn = st["dlogits"]
    for l in range(L - 1, -1, -1):
        zz = c(st["z"][l]).clone().requires_grad_(True)
        gp, = torch.autograd.grad(F.gelu(zz).sum(), zz)
        raw["dz"][l] = (c(dn) @ c(h["ws"][l + 1])) * gp * c(h["masks"][l])
        st["dz"][l] = raw["dz"][l].float()
        dn = st["dz"][l]
    for l in range(L + 1):
        ap = h["x"] if l == 0 else st["a"][l - 1]
        dz = st["dlogits"] if l == L else st["dz"][l]
        raw[f"dW{l}"], raw[f"db{l}"] = c(dz).t() @ c(ap), c(dz).sum(0)
    raw["loss"] = c(st["loss_rows"]).mean().reshape(1)
    return st, raw


def mlp_refs(h, st):
    out = R.mlp_stages(h["ws"], h["bs"], h["x"], h["y"], h["masks"], st)
    out.update(R.mlp_params(h["ws"], h["x"], st))
    return out


def raw_of(raw, name):
    return raw[name[:-1]][int(name[-1])] if name[0] in "za" and name[-1].isdigit() or name.startswith("dz") else raw[name]


def sn_run(w, u0, v0, dw, dtype, power_iter=True, eps=1e-12, stored=True):
    """stored: every stage continues from the previous one ROUNDED TO fp32 (what the kernel leaves in memory)."""
    c = lambda t: t.to(dtype)  # noqa: E731
    f = (lambda t: t.float()) if stored else (lambda t: t)  # noqa: E731
    W_, u, v = c(w), c(u0), c(v0)
    raw = {}
    if power_iter:
        x = W_.t() @ u
        v = x / max(float(x.norm()), eps)
        raw["v"] = v
        v = c(f(v))
        x = W_ @ v
        u = x / max(float(x.norm()), eps)
        raw["u"] = u
        u = c(f(u))
    raw["sigma"] = (u @ (W_ @ v)).reshape(1)
    sg = c(f(raw["sigma"]))
    raw["w_eff"] = W_ / sg
    st = dict(u=f(u), v=f(v), sigma=f(sg), w_eff=f(raw["w_eff"]))
    we = c(st["w_eff"])
    raw["dw"] = (c(dw) - (c(dw) * we).sum() * u[:, None] * v[None, :]) / sg
    return st, raw


# ---------------------------------------------------------------------------------------------------------------------
# (a) the references are torch's fp64 modules / autograd
# ---------------------------------------------------------------------------------------------------------------------
def test_chain_references_equal_torch_fp64():
    for rows in R.CHAIN_ROWS:
        for T, C, _ in R.MEANT_VEC + R.MEANT_SCALAR:
            a = R.meant_input(rows, T, C)
            assert same(R.meanT(a).val, F.adaptive_avg_pool1d(a.double().transpose(1, 2), 1)[:, :, 0])
        for D in R.LN_D:
            for kind in R.LN_KINDS:
                x, g, b = R.ln_input(rows, D, kind)
                y, xh = R.layernorm(x, g, b)
                assert same(y.val, F.layer_norm(x.double(), (D,), g.double(), b.double(), S.f32(1e-5)), 1e-9)
                assert same(xh.val, F.layer_norm(x.double(), (D,), None, None, S.f32(1e-5)), 1e-9)
        for C in R.CE_C:
            for kind in R.CE_KINDS:
                z, y = R.ce_input(rows, C, kind)
                zz = z.double().requires_grad_(True)
                lr = F.cross_entropy(zz, y, reduction="none")
                g, = torch.autograd.grad(lr.sum() * S.f32(0.37), zz)
                loss, dl, bad = R.ce_rows(z, y, 0.37)
                assert same(loss.val, lr.detach()) and same(dl.val, g) and not bad.any()
                # and the batch form support_ref already pins
                l2, d2, _ = S.softmax_ce(z, y, 0.37)
                assert same(loss.val.mean().reshape(1), l2.val) and same(dl.val / rows, d2.val)
                yb = y.clone()
                yb[rows - 1] = C
                loss, dl, bad = R.ce_rows(z, yb)
                assert torch.isnan(loss.val[rows - 1]) and torch.isnan(dl.val[rows - 1]).all() and torch.isfinite(dl.val[:rows - 1]).all()
        for Fd, E, Be in R.DHEAD:
            f, emb, w, bias, ds = R.dhead_input(rows, Fd, E, Be)
            ff = f.double().requires_grad_(True)
            er = emb.double()[torch.arange(rows) % emb.shape[0]].requires_grad_(True) if E else None
            act = ff                                       # the head scores f itself; dU is the gradient behind LeakyReLU
            s = act @ w.double()[:Fd] + bias.double()
            if E:
                s = s + er @ w.double()[Fd:]
            sr, dU, demb = R.dhead(f, emb, w, bias, ds, with_demb=bool(E) and emb.shape[0] == rows)
            assert same(sr.val, s.detach())
            pre = f.double().requires_grad_(True)           # dU[b, j] = ds w_j lrelu'(f): autograd through leaky_relu at f
            (F.leaky_relu(pre, 0.2) @ w.double()[:Fd] * ds.double()).sum().backward()
            assert same(dU.val, pre.grad)
            if demb is not None:
                g, = torch.autograd.grad((s * ds.double()).sum(), er)
                assert same(demb.val, g)


def test_mlp_references_equal_autograd():
    for name, rows in R.MLP_CASES:
        h = R.mlp_problem(name, rows)
        L = len(h["hidden"])
        ws = [w.double().requires_grad_(True) for w in h["ws"]]
        bs = [b.double().requires_grad_(True) for b in h["bs"]]
        a, zs, as_ = h["x"].double(), [], []
        for l in range(L):
            z = F.linear(a, ws[l], bs[l])
            z.retain_grad()
            a = F.gelu(z) * h["masks"][l].double()
            zs.append(z), as_.append(a)
        logits = F.linear(a, ws[L], bs[L])
        logits.retain_grad()
        lr = F.cross_entropy(logits, h["y"], reduction="none")
        lr.mean().backward()
        st = dict(z=[z.detach() for z in zs], a=[a.detach() for a in as_], dz=[z.grad for z in zs], logits=logits.detach(),
                  loss_rows=lr.detach(), dlogits=logits.grad)
        refs = mlp_refs(h, st)
        for l in range(L):
            assert same(refs[f"z{l}"].val, st["z"][l]) and same(refs[f"a{l}"].val, st["a"][l]) and same(refs[f"dz{l}"].val, st["dz"][l], 1e-10)
        assert same(refs["logits"].val, st["logits"]) and same(refs["loss_rows"].val, st["loss_rows"]) and same(refs["dlogits"].val, st["dlogits"])
        for l in range(L + 1):
            assert same(refs[f"dW{l}"].val, ws[l].grad) and same(refs[f"db{l}"].val, bs[l].grad)
        assert same(refs["loss"].val, lr.mean().detach().reshape(1))
        # eval mode: the whole stack without masks
        a = h["x"].double()
        for l in range(L):
            a = F.gelu(F.linear(a, h["ws"][l].double(), h["bs"][l].double()))
        assert same(R.mlp_eval(h["ws"], h["bs"], h["x"]).val, F.linear(a, h["ws"][L].double(), h["bs"][L].double()))
    # the fused AdamW is support_ref.adam_step, which tests/test_support_ref.py compares with torch.optim.AdamW
    am = R.argmax_nan_first(torch.tensor([[1.0, 3.0, 3.0], [float("nan"), 9.0, float("nan")], [float("inf"), float("nan"), 0.0],
                                          [float("-inf"), float("-inf"), float("-inf")]]))
    assert am.tolist() == [1, 0, 1, 0]


def test_spectral_norm_references_equal_torchs_wrapper():
    for Rr, C in R.SN_SHAPES:
        w, u0, v0, dw = R.sn_input(Rr, C)
        for train in (True, False):
            m = nn.utils.spectral_norm(nn.Linear(C, Rr, bias=False).double())
            with torch.no_grad():
                m.weight_orig.copy_(w.double()), m.weight_u.copy_(u0.double()), m.weight_v.copy_(v0.double())
            m.train(train)
            m(torch.zeros(1, C, dtype=torch.float64))
            # from exact "stored" values the stage-wise references are the wrapper's
            ex, _ = sn_run(w, u0, v0, dw, torch.float64, train, stored=False)
            refs = R.sn_fwd(w, u0, v0, ex, train)
            assert same(refs["w_eff"].val, m.weight.detach(), 1e-9)
            if train:
                assert same(refs["u"].val, m.weight_u, 1e-9) and same(refs["v"].val, m.weight_v, 1e-9)
            else:
                assert "u" not in refs and torch.equal(m.weight_u, u0.double())
            wo = w.double().clone().requires_grad_(True)
            sig = ex["u"] @ (wo @ ex["v"])
            ((wo / sig) * dw.double()).sum().backward()
            assert same(R.sn_bwd(dw, ex).val, wo.grad, 1e-9), (Rr, C, train)


# ---------------------------------------------------------------------------------------------------------------------
# (b) the tables reach the paths
# ---------------------------------------------------------------------------------------------------------------------
def test_tables_reach_the_paths():
    p = {(T, C): R.meant_plan(T, C, off) for T, C, off in R.MEANT_VEC}
    assert all(q["vec"] for q in p.values())
    assert p[(1, 16)]["RL"] == 256 and p[(1, 16)]["in_flight"] == 1
    assert p[(37, 100)]["live"] == 1000 and p[(37, 100)]["outer"] == 1 and p[(37, 100)]["in_flight"] == 1
    assert p[(33, 128)]["RL"] == 32 and p[(33, 128)]["in_flight"] == 2 and p[(33, 128)]["outer"] == 1
    assert p[(130, 512)]["RL"] == 8 and p[(130, 512)]["outer"] == 2 and p[(130, 512)]["clamped"]
    assert [R.meant_plan(T, C, off)["vec"] for T, C, off in R.MEANT_SCALAR] == [False, False, False]
    assert R.MEANT_SCALAR[2][1] % 4 == 0 and R.MEANT_SCALAR[2][1] >= 16          # scalar by the alignment predicate alone
    assert set(R.LN_D) == {1, 6, 63, 64} and set(R.CE_C) == {1, 2, 4, 32}
    assert {f for f, _, _ in R.DHEAD} == {1, 100, 256, 512} and {e for _, e, _ in R.DHEAD} == {0, 3, 128}
    assert {b for _, e, b in R.DHEAD if e} == {2, -1} and 2 < max(R.CHAIN_ROWS)
    assert {R.dgrad_branch(n) for n in (256, 128, 6)} == {"vec", "rows"}          # the composed chain's data gradients
    seen = dict(vec=set(), kpad=set(), two=set(), single=set(), rounds=set(), rows=set(), hidden=set(), C=set(), inn=set(), width=set(),
                ragged_blocks=False, ti=set(), b_trips=set())
    for name, rows in R.MLP_CASES:
        in_dim, hidden, C = R.MLP_SHAPES[name]
        h = R.mlp_problem(name, rows)
        for aligned in (True, False):
            w_off, b_off, n = R.flat_layout(h["ws"], h["bs"], aligned)
            assert all(o % 4 == (0 if aligned else o % 4) for o in w_off) and (aligned or all(o % 2 == 1 for o in w_off + b_off))
            plan = R.mlp_plan(in_dim, hidden, C, rows, w_off, b_off)
            for ly in plan["layers"]:
                assert ly["vec"] == (aligned and ly["inn"] % 4 == 0)
                seen["vec"].add(ly["vec"]), seen["kpad"].add(ly["kpad"]), seen["rounds"].add(ly["rounds"]), seen["inn"].add(ly["inn"])
                seen["two"].add(ly["two"]), seen["single"].add(ly["single"]), seen["ti"].add(ly["tiles_i"])
            seen["ragged_blocks"] |= plan["tiles"] % R.UPD_WAVES != 0
            # launch B's decode of a tile index (tile_end scan, to = tl / tiles_i, ti = tl % tiles_i) names every (layer, to, ti)
            # once, and exactly one tile per output tile row carries the bias (ti == 0)
            ends = [ly["tile_end"] for ly in plan["layers"]]
            for t, want in enumerate(plan["tile_map"]):
                l = next(i for i, e in enumerate(ends) if t < e)
                tl = t - (ends[l - 1] if l else 0)
                assert (l, tl // plan["layers"][l]["tiles_i"], tl % plan["layers"][l]["tiles_i"]) == want
            for ly in plan["layers"]:
                mine = [(to, ti) for l, to, ti in plan["tile_map"] if l == ly["l"]]
                assert len(set(mine)) == len(mine) == ly["tiles"] * ly["tiles_i"] and sum(ti == 0 for _, ti in mine) == ly["tiles"]
            assert len(plan["tile_map"]) == plan["tiles"] and plan["tile_map"][plan["layers"][0]["tile_end"] - 1][0] == 0
            # spans are disjoint and inside the buffer
            spans = sorted([(o, o + w.numel()) for o, w in zip(w_off, h["ws"])] + [(o, o + b.numel()) for o, b in zip(b_off, h["bs"])])
            assert spans[0][0] > 0 and spans[-1][1] < n and all(a[1] < b[0] for a, b in zip(spans, spans[1:]))
        seen["rows"].add(rows), seen["hidden"].add(len(hidden)), seen["C"].add(C), seen["width"].update(hidden), seen["b_trips"].add(-(-rows // 8))
    assert seen["vec"] == {True, False} and {16, 32, 48, 512} <= seen["kpad"] and {1, 16, 32, 33, 48, 512} <= seen["inn"]
    assert {0, 1} <= seen["two"] and {0, 1} <= seen["single"] and 2 in seen["rounds"]         # 130 columns: nine tiles on eight waves
    assert seen["rows"] == set(R.MLP_ROWS_ALL) and seen["hidden"] == {1, R.MLP_MAX_HIDDEN} and seen["C"] == {2, 17, 32}
    assert {1, 130, 512} <= seen["width"] and seen["ragged_blocks"] and {1, 2} <= seen["b_trips"] and {1, 3} <= seen["ti"]
    assert any(C > 1024 for _, C in R.SN_SHAPES) and any(Rr > 1024 for Rr, _ in R.SN_SHAPES) and len(R.SN_SHAPES) <= R.MAX_SN_JOBS


# ---------------------------------------------------------------------------------------------------------------------
# (c) fp32 host computations stay inside the bounds
# ---------------------------------------------------------------------------------------------------------------------
def seq_sum(x):
    return torch.cumsum(x, -1)[..., -1:]          # fp32, in sequence: the chain's LayerNorm loop


def ln_fp32(x, g, b, eps=1e-5):
    D = x.shape[-1]
    mean = seq_sum(x) / D
    c = x - mean
    var = seq_sum(c * c) / D
    xh = c * (1.0 / torch.sqrt(var + eps))
    return xh * g + b, xh


def test_fp32_host_computations_stay_inside_the_bounds():
    for rows in R.CHAIN_ROWS:
        for T, C, _ in R.MEANT_VEC + R.MEANT_SCALAR:
            a = R.meant_input(rows, T, C)
            note(FP32, "MEAN_T", ratio(a.sum(1) / T, R.meanT(a)))
            note(FP32, "MEAN_T", ratio(torch.cumsum(a, 1)[:, -1] / T, R.meanT(a)))
        for D in R.LN_D:
            for kind in R.LN_KINDS:
                x, g, b = R.ln_input(rows, D, kind)
                y, xh = ln_fp32(x, g, b)
                ry, rxh = R.layernorm(x, g, b)
                note(FP32, f"LAYERNORM {kind}", max(ratio(y, ry), ratio(xh, rxh)))
        for C in R.CE_C:
            for kind in R.CE_KINDS:
                z, y = R.ce_input(rows, C, kind)
                loss, dl, _ = R.ce_rows(z, y, 0.37)
                lse = torch.logsumexp(z, 1)
                note(FP32, f"SOFTMAX_CE {kind}", max(ratio(lse - z.gather(1, y[:, None])[:, 0], loss),
                                                     ratio(torch.tensor(0.37) * (torch.exp(z - lse[:, None]) - F.one_hot(y, C)), dl)))
        for Fd, E, Be in R.DHEAD:
            f, emb, w, bias, ds = R.dhead_input(rows, Fd, E, Be)
            with_demb = bool(E) and emb.shape[0] == rows
            sr, dU, demb = R.dhead(f, emb, w, bias, ds, with_demb)
            s = f @ w[:Fd] + ((emb[torch.arange(rows) % emb.shape[0]] @ w[Fd:]) if E else 0.0) + bias
            note(FP32, "DHEAD", max(ratio(s, sr), ratio(ds[:, None] * w[None, :Fd] * torch.where(f > 0, 1.0, 0.2), dU)))
            if with_demb:
                note(FP32, "DHEAD", ratio(ds[:, None] * w[None, Fd:], demb))
    for name, rows in R.MLP_CASES:
        h = R.mlp_problem(name, rows)
        st, raw = mlp_run(h, torch.float32)
        for k, ref in mlp_refs(h, st).items():
            sect = "MLP launch B" if k[:2] in ("dW", "db", "lo") and k != "logits" else "MLP launch A"
            note(FP32, sect, ratio(raw_of(raw, k), ref))
        a = h["x"]
        for l in range(len(h["hidden"])):
            a = F.gelu(F.linear(a, h["ws"][l], h["bs"][l]))
        note(FP32, "MLP eval", ratio(F.linear(a, h["ws"][-1], h["bs"][-1]), R.mlp_eval(h["ws"], h["bs"], h["x"])))
        # the fused AdamW from the stored gradient
        g = gen_like(raw["dW0"], 1)
        p, m, v = h["ws"][0], gen_like(g, 2) * 1e-3, gen_like(g, 3).abs() * 1e-6
        refs = S.adam_step(p, g, m, v, 3, 1e-3, 0.5, 0.999, 1e-8, 0.01)
        b1, b2, lr, wd = (torch.tensor(t, dtype=torch.float32) for t in (0.5, 0.999, 1e-3, 0.01))
        mi = m + (g - m) * (1 - b1)
        vi = v * b2 + (1 - b2) * g * g
        ss = torch.tensor(float(lr) / (1 - float(b1) ** 3), dtype=torch.float32)
        bc2 = torch.tensor((1 - float(b2) ** 3) ** 0.5, dtype=torch.float32)
        pn = p * (1 - lr * wd) - ss * (mi / (torch.sqrt(vi) / bc2 + 1e-8))
        note(FP32, "MLP AdamW", max(ratio(pn, refs[0]), ratio(mi, refs[1]), ratio(vi, refs[2])))
    for Rr, C in R.SN_SHAPES:
        w, u0, v0, dw = R.sn_input(Rr, C)
        for train in (True, False):
            st, raw = sn_run(w, u0, v0, dw, torch.float32, train)
            refs = R.sn_fwd(w, u0, v0, st, train)
            for k, ref in refs.items():
                note(FP32, f"spectral norm {k}", ratio(raw[k].reshape(ref.val.shape), ref))
            note(FP32, "spectral norm bwd", ratio(raw["dw"], R.sn_bwd(dw, st)))
    assert max(FP32.values()) <= 1.0, FP32


def gen_like(t, seed):
    return torch.randn(t.shape, generator=R.gen(seed))


# ---------------------------------------------------------------------------------------------------------------------
# (d) plausible mistakes leave the bounds
# ---------------------------------------------------------------------------------------------------------------------
def test_plausible_mistakes_leave_the_bounds():
    M = MISTAKES
    rows = 3
    # MEAN_T at (130, 512): RL = 8, so the second outer iteration holds rows 128, 129 and fourteen clamped copies of row 129
    a = R.meant_input(rows, 130, 512).double()
    ref = R.meanT(a)
    # lane group rl takes t0 = rl + 128 (rl < 2) and the clamped rows u = 1..15 of it: row 129, 15 times per group
    M["MEAN_T: clamped rows of the last group added"] = ratio((a.sum(1) + 30 * a[:, 129]) / 130, ref)
    M["MEAN_T: 1/T as 1/(T+1), T = 130"] = ratio(a.sum(1) / 131, ref)
    M["MEAN_T: second outer iteration dropped, T = 130"] = ratio(a[:, :128].sum(1) / 130, ref)
    x, g, b = R.ln_input(rows, 6, "randn")
    xd, gd, bd = x.double(), g.double(), b.double()
    ry, rxh = R.layernorm(x, g, b)
    c = xd - xd.mean(-1, keepdim=True)
    M["LAYERNORM: unbiased variance, D = 6 / 64"] = ratio(c / torch.sqrt(c.pow(2).sum(-1, keepdim=True) / 5 + 1e-5), rxh)
    x64, g64, b64 = R.ln_input(rows, 64, "randn")
    c64 = x64.double() - x64.double().mean(-1, keepdim=True)
    M["LAYERNORM: unbiased variance, D = 6 / 64"] = (M["LAYERNORM: unbiased variance, D = 6 / 64"],
                                                    ratio(c64 / torch.sqrt(c64.pow(2).sum(-1, keepdim=True) / 63 + 1e-5), R.layernorm(x64, g64, b64)[1]))
    xo, go, bo = R.ln_input(rows, 64, "offset")
    co = xo.double() - xo.double().mean(-1, keepdim=True)
    xs, gs, bs_ = R.ln_input(rows, 64, "small")
    cs = xs.double() - xs.double().mean(-1, keepdim=True)
    M["LAYERNORM: eps outside the root (0.01 randn, D = 64)"] = ratio(cs / (cs.pow(2).mean(-1, keepdim=True).sqrt() + 1e-5), R.layernorm(xs, gs, bs_)[1])
    ex2 = (xo * xo).mean(-1, keepdim=True) - xo.mean(-1, keepdim=True) ** 2                        # fp32
    M["LAYERNORM: variance as fp32 E[x^2] - mean^2 (offset data)"] = ratio((xo - xo.mean(-1, keepdim=True)) / torch.sqrt(ex2.clamp_min(0) + 1e-5),
                                                                             R.layernorm(xo, go, bo)[1])
    z, y = R.ce_input(rows, 4, "randn")
    loss, dl, _ = R.ce_rows(z, y, 0.37)
    p = torch.softmax(z.double(), 1)
    M["SOFTMAX_CE: coef missing (coef = 0.37)"] = ratio(p - F.one_hot(y, 4), dl)
    M["SOFTMAX_CE: one-hot on the wrong class"] = ratio(S.f32(0.37) * (p - F.one_hot((y + 1) % 4, 4)), dl)
    f, emb, w, bias, ds = R.dhead_input(rows, 100, 3, 2)
    sr, dU, _ = R.dhead(f, emb, w, bias, ds, False)
    fd, wd_, dsd = f.double(), w.double(), ds.double()
    M["DHEAD: slope 0.2 applied at f > 0"] = ratio(dsd[:, None] * wd_[None, :100] * torch.where(fd > 0, 0.2, 1.0), dU)
    M["DHEAD: embedding row not taken modulo (clamped)"] = ratio(fd @ wd_[:100] + emb.double()[torch.arange(rows).clamp(max=1)] @ wd_[100:] + bias.double(), sr)
    M["DHEAD: bias added once per wave"] = ratio(sr.val + 15 * bias.double(), sr)
    M["LOAD accumulate overwriting"] = float((x + x != x).double().mean())          # exact comparison: share of elements that differ

    # MLP
    def stored(name, rows_):
        h_ = R.mlp_problem(name, rows_)
        st_, _ = mlp_run(h_, torch.float64)
        return h_, st_, mlp_refs(h_, st_)
    h, st, refs = stored("deep", 15)
    w0 = h["ws"][0].double().clone()
    w0[:, 32:] = 0
    M["MLP: ld_w4 tail quad dropped, in = 33"] = ratio(F.linear(h["x"].double(), w0, h["bs"][0].double()), refs["z0"])
    M["MLP: wrong layer's mask in dz"] = ratio(_dz_with_mask(h, st, 1, h["masks"][0][:, :33]), refs["dz1"])
    h, st, refs = stored("two32", 33)
    w0 = h["ws"][0].double().clone()
    w0[:, 16:] = 0
    M["MLP: second 16-chunk dropped, kpad = 32"] = ratio(F.linear(h["x"].double(), w0, h["bs"][0].double()), refs["z0"])
    bb = h["bs"][0].double().clone()
    bb[1] = bb[0]
    M["MLP: bias of tile column 1 from column 0"] = ratio(F.linear(h["x"].double(), h["ws"][0].double(), bb), refs["z0"])
    z15 = refs["z0"].val.clone()
    z15[15] = 0
    M["MLP: row 15 of a block zeroed"] = ratio(z15, refs["z0"])
    M["MLP: dlogits without / rows, rows = 33"] = ratio(refs["dlogits"].val * 33, refs["dlogits"])
    for r in (9, 100):
        name = "two32" if r == 9 else "deep"
        h, st, refs = stored(name, r)
        dz, ap = st["dz"][0].double(), h["x"].double()
        M[f"MLP: one row dropped from dW, rows = {r}"] = ratio(dz[:-1].t() @ ap[:-1], refs["dW0"])
    h, st, refs = stored("one", 17)
    M["MLP: db from the ti = 1 tile (in <= 16: never written)"] = ratio(torch.full_like(refs["db0"].val, float("nan")), refs["db0"])
    g = gen_like(h["ws"][0], 1)
    p, m, v = h["ws"][0] + 1.0, gen_like(g, 2) * 1e-3, gen_like(g, 3).abs() * 1e-6
    good = S.adam_step(p, g, m, v, 3, 1e-3, 0.5, 0.999, 1e-8, 0.01)
    M["MLP: AdamW decay coupled"] = ratio(S.adam_step(p, g, m, v, 3, 1e-3, 0.5, 0.999, 1e-8, 0.01, decoupled=False)[0].val, good[0])

    # spectral norm
    w, u0, v0, dw = R.sn_input(17, 65)
    st, raw = sn_run(w, u0, v0, dw, torch.float64)
    refs = R.sn_fwd(w, u0, v0, st)
    M["SN: sigma from the pre-iteration u"] = ratio((u0.double() @ (w.double() @ st["v"].double())).reshape(1), refs["sigma"])
    rb = R.sn_bwd(dw, st)
    sg = st["sigma"].double()
    M["SN: backward without the u v^T term"] = ratio(dw.double() / sg, rb)
    M["SN: backward dividing by sigma^2"] = ratio(rb.val / sg, rb)
    w, u0, v0, dw = R.sn_input(3, 1029)
    st, raw = sn_run(w, u0, v0, dw, torch.float64)
    x = w.double().t() @ u0.double()
    M["SN: columns >= 1024 left out of |v|, C = 1029"] = ratio(x / x[:1024].norm(), R.sn_fwd(w, u0, v0, st)["v"])

    flat = {}
    for k, v in M.items():
        for i, r in enumerate(v if isinstance(v, tuple) else (v,)):
            flat[f"{k} [{i}]"] = r
    MISTAKES.clear()
    MISTAKES.update(flat)
    low = {k: r for k, r in flat.items() if not r >= 2.0 and not k.startswith("LOAD")}
    assert not low, low
    assert flat["LOAD accumulate overwriting [0]"] > 0.99


def _dz_with_mask(h, st, l, mask):
    dn = st["dz"][l + 1].double()
    zz = st["z"][l].double().requires_grad_(True)
    gp, = torch.autograd.grad(F.gelu(zz).sum(), zz)
    return (dn @ h["ws"][l + 1].double()) * gp * mask.double()
