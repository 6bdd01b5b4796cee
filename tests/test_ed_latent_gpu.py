"""Latent-mode emotion-discriminator pre-training (SURVEY f-2 with `input_mode: latent`; ed_model.py:72-95, train_ed.py:51-82)
on the GPU: the two fused launches of csrc/mlp_train.hip alone against fp64, the engine (fused and on the per-layer
comparator launches) against the reference-generated fixtures and the oracle at the tolerances tests/test_ed_train_gpu.py
holds EdEngine to, device-drawn masks, graph replay, staging, spectral norm (bounds of tests/test_sn_gpu.py), and the trainer
end to end."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import melo_oracle as O  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = ["ed_latent_d64_b8", "ed_latent_d8_b5", "ed_latent_d32_h3_b7"]
OPT = dict(name="AdamW", lr=2e-4, betas=[0.5, 0.999], weight_decay=0.01)
TICKED_ONCE = [1.0, 0.5, float(np.float32(0.999))]      # the betas are float arguments of the launch, as mg_rng_fill's


def rel_err(a, b):
    a, b = a.detach().cpu().double().flatten(), b.detach().cpu().double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def latent_cfg(D, hidden, **kw):
    return dict(O.default_ed_cfg(4), input_mode="latent", latent_dim=D, mlp_hidden=list(hidden), dropout=0.2, **kw)


def closed_form_params(cfg, scale):
    spec, _ = O.emotion_disc_spec(cfg)
    P = O.fill_params(spec, 9.0, O.norm_affine_names(spec))
    for v in P.values():
        if v.dim() >= 2:
            v.mul_(scale)
    return spec, P


def engine(cfg, B, fused=True, seed=None):
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.emotion_discriminator.latent_engine import EdLatentEngine
    eng = EdLatentEngine(cfg, "cuda", B, fused=fused)
    if seed is not None:
        eng.init_weights(seed)
    return eng


# ---- teacher-forced steps against the fixtures ------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_latent_pretraining_steps_match_reference(name, fused):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    B, D, hidden, n_steps = int(g["B"]), int(g["D"]), [int(h) for h in g["hidden"]], int(g["n_steps"])
    ed_cfg = latent_cfg(D, hidden)
    spec, P = closed_form_params(ed_cfg, float(g["scale"]))
    eng = engine(dict(ed_cfg, batch_size=B, optimizer=OPT), B, fused)
    assert list(eng.P.spec) == list(spec) and all(tuple(eng.P.spec[k]) == tuple(spec[k]) for k in spec)
    eng.load_state(P)
    opt = O.AdamState(P, 2e-4, (0.5, 0.999), 1e-8, weight_decay=0.01, decoupled=True)
    for it in range(n_steps):
        x, y = torch.from_numpy(g[f"s{it}.x"]), torch.from_numpy(g[f"s{it}.y"])
        dm = [torch.from_numpy(g[f"s{it}.dm{j}"]).float() / 0.8 for j in range(len(hidden))]
        eng.set_batch(x.cuda(), y.cuda())
        eng.set_masks([m.cuda() for m in dm])
        eng.backward()
        # fp64 truth and the reference's own fp32 arithmetic from the same (re-synchronised) parameters
        P64 = {k: v.double().clone().requires_grad_(True) for k, v in P.items()}
        l64 = F.cross_entropy(O.emotion_disc_fwd(P64, {}, x.double(), ed_cfg, True, [m.double() for m in dm]), y)
        g64 = dict(zip(P64, torch.autograd.grad(l64, list(P64.values()))))
        old = {k: v.clone() for k, v in P.items()}
        r = O.ed_step(P, {}, opt, x, y, ed_cfg, dm)
        print(name, fused, it, "loss", eng.loss.item(), float(g[f"s{it}.loss"]))
        assert abs(eng.loss.item() - float(g[f"s{it}.loss"])) < 5e-6
        np.testing.assert_allclose(eng.logits.cpu().numpy(), g[f"s{it}.logits"], rtol=2e-3, atol=2e-5)
        if it == 0:
            np.testing.assert_allclose(eng.P.g["classifier.head.weight"].cpu().numpy(), g["s0.grad.head_w"], rtol=2e-3, atol=1e-6)
        for k in spec:
            e_mine, e_ref = rel_err(eng.P.g[k], g64[k]), rel_err(r["grads"][k], g64[k])
            print("   grad", k, e_mine, e_ref)
            assert e_mine <= 6.0 * e_ref + 3e-4, (it, k, e_mine, e_ref)
        eng.update()
        for k in spec:
            upd, upd_ref = eng.P.p[k].cpu() - old[k], P[k] - old[k]
            assert rel_err(upd, upd_ref) < 0.1, (it, "AdamW update", k, rel_err(upd, upd_ref))
        eng.load_state(P)          # teacher forcing: each step is judged from identical inputs
    np.testing.assert_allclose(eng.P.p["classifier.head.weight"].cpu().numpy(), g["end.head_w"], rtol=1e-4, atol=2e-6)
    eng.set_batch(torch.from_numpy(g["s0.x"]).cuda(), torch.from_numpy(g["s0.y"]).cuda())
    eng.forward_eval()
    np.testing.assert_allclose(eng.logits.cpu().numpy(), g["end.eval_logits"], rtol=2e-3, atol=1e-4)
    assert float(eng.P.state[0].item()) == n_steps
    sd = eng.state_dict()
    assert set(f"end.{k}" for k in sd) == set(k for k in g.files if k.startswith("end.")) - {"end.head_w", "end.eval_logits"}


# ---- the two launches alone -----------------------------------------------------------------------------------------------
# Bound on ||got - fp64|| / ||fp64|| per tensor: an fp32 dot product of K terms carries at most K * 2^-24 of relative error
# against the sum of magnitudes (K <= 512: 3.1e-5), the project's GELU is within 4.2e-7 absolute of the exact form
# (csrc/common.h), and the tensors here are sums of same-sized terms, so the norm-wise error stays below that one-layer
# worst case through the <= 5 layers.
KERNEL_TOL = 512 * 2.0 ** -24 + 5e-6
SHAPES = {"odd": (7, [33, 130], 3), "limit": (512, [512, 300], 32), "default": (64, [256, 128], 4), "tiny": (1, [1], 2),
          "four": (16, [96, 48, 24, 12], 5)}


def kernel_problem(rows, shape, seed=0):
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import ops
    in_dim, hidden, C = SHAPES[shape]
    gen = torch.Generator().manual_seed(1000 * rows + seed)
    dims = [in_dim] + hidden + [C]
    ws = [(torch.randn(o, i, generator=gen) * (1.5 / math.sqrt(i))) for i, o in zip(dims, dims[1:])]
    bs = [torch.randn(o, generator=gen) * 0.1 for o in dims[1:]]
    x = torch.randn(rows, in_dim, generator=gen)
    y = torch.randint(0, C, (rows,), generator=gen)
    masks = [(torch.rand(rows, h, generator=gen) >= 0.2).float() / 0.8 for h in hidden]
    # one flat buffer with the tensors at odd offsets (not multiples of 4 floats)
    sizes = [t.numel() for pair in zip(ws, bs) for t in pair]
    offs, o = [], 3
    for s in sizes:
        offs.append(o)
        o += s + 1
    flat = torch.zeros(o + 2)
    for (off, t) in zip(offs, [t for pair in zip(ws, bs) for t in pair]):
        flat[off:off + t.numel()] = t.flatten()
    dev = dict(flat=flat.cuda(), x=x.cuda(), y=y.cuda())
    wv = [dev["flat"][offs[2 * l]:offs[2 * l] + ws[l].numel()].view(ws[l].shape) for l in range(len(ws))]
    bv = [dev["flat"][offs[2 * l + 1]:offs[2 * l + 1] + bs[l].numel()] for l in range(len(ws))]
    f = lambda *s: torch.full(s, float("nan"), device="cuda")      # noqa: E731
    dev.update(z=[f(rows, h) for h in hidden], a=[f(rows, h) for h in hidden], dz=[f(rows, h) for h in hidden],
               mask=[m.cuda() for m in masks], logits=f(rows, C), loss_rows=f(rows), dlogits=f(rows, C), loss=f(1),
               g=torch.full_like(dev["flat"], float("nan")))
    net = ops.MlpNet(rows, wv, bv, dev["z"], dev["a"], dev["dz"], dev["mask"])
    return net, dev, dict(ws=ws, bs=bs, x=x, y=y, masks=masks, w_off=offs[0::2], b_off=offs[1::2], hidden=hidden, C=C)


def fp64_reference(h):
    ws = [w.double().requires_grad_(True) for w in h["ws"]]
    bs = [b.double().requires_grad_(True) for b in h["bs"]]
    a, zs, acts = h["x"].double(), [], []
    for l in range(len(h["hidden"])):
        z = F.linear(a, ws[l], bs[l])
        z.retain_grad()
        a = F.gelu(z) * h["masks"][l].double()
        zs.append(z)
        acts.append(a)
    logits = F.linear(a, ws[-1], bs[-1])
    rows_loss = F.cross_entropy(logits, h["y"], reduction="none")
    rows_loss.mean().backward()
    return dict(z=zs, a=acts, dz=[z.grad for z in zs], logits=logits, loss_rows=rows_loss, dW=[w.grad for w in ws], db=[b.grad for b in bs])


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("rows", [1, 5, 64, 100])
def test_the_two_launches_against_fp64(rows, shape):
    from melo_gan_amd import ops
    net, d, h = kernel_problem(rows, shape)
    ops.mlp_cls_fwd_bwd(net, d["x"], d["y"], d["logits"], d["loss_rows"], d["dlogits"], train=True)
    ops.mlp_cls_wgrad_update(net, d["x"], d["dlogits"], h["w_off"], h["b_off"], d["g"], d["loss_rows"], d["loss"])
    torch.cuda.synchronize()
    ref = fp64_reference(h)
    worst = {}
    for l in range(len(h["hidden"])):
        for nm in ("z", "a", "dz"):
            worst[f"{nm}{l}"] = rel_err(d[nm][l], ref[nm][l])
    worst["logits"] = rel_err(d["logits"], ref["logits"])
    worst["loss_rows"] = rel_err(d["loss_rows"], ref["loss_rows"])
    for l in range(len(h["ws"])):
        gw = d["g"][h["w_off"][l]:h["w_off"][l] + h["ws"][l].numel()].view(h["ws"][l].shape)
        gb = d["g"][h["b_off"][l]:h["b_off"][l] + h["bs"][l].numel()]
        worst[f"dW{l}"], worst[f"db{l}"] = rel_err(gw, ref["dW"][l]), rel_err(gb, ref["db"][l])
    print(rows, shape, {k: f"{v:.2e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= KERNEL_TOL, (k, v)
    assert abs(d["loss"].item() - ref["loss_rows"].mean().item()) <= KERNEL_TOL * max(1.0, abs(ref["loss_rows"].mean().item()))
    # nothing outside the named tensors of the flat gradient buffer was written
    named = torch.zeros_like(d["g"], dtype=torch.bool)
    for off, t in zip(h["w_off"] + h["b_off"], h["ws"] + h["bs"]):
        named[off:off + t.numel()] = True
    assert torch.isnan(d["g"][~named]).all() and torch.isfinite(d["g"][named]).all()
    # eval mode: the same logits without the masks, nothing else touched
    lg, lr_ = torch.full_like(d["logits"], float("nan")), torch.full_like(d["loss_rows"], float("nan"))
    enet = ops.MlpNet(rows, net.keep[0], net.keep[1])
    ops.mlp_cls_fwd_bwd(enet, d["x"], d["y"], lg, lr_, None, train=False)
    a = h["x"].double()
    for l in range(len(h["hidden"])):
        a = F.gelu(F.linear(a, h["ws"][l].double(), h["bs"][l].double()))
    want = F.linear(a, h["ws"][-1].double(), h["bs"][-1].double())
    assert rel_err(lg, want) <= KERNEL_TOL
    assert rel_err(lr_, F.cross_entropy(want, h["y"], reduction="none")) <= KERNEL_TOL


def test_fused_update_is_adam_flat_on_the_same_gradient():
    """Launch B in apply mode against launch B (gradients only) followed by ops.adam_flat on a copy: the same AdamW formula,
    so at most the last-bit differences of a differently contracted expression; the step counter advances, the state does not."""
    from melo_gan_amd import ops
    net, d, h = kernel_problem(64, "odd", seed=1)
    n = d["flat"].numel()
    state = torch.zeros(4, dtype=torch.float64, device="cuda")
    m, v = torch.rand(n, device="cuda") * 1e-3, torch.rand(n, device="cuda") * 1e-6
    p2, m2, v2, state2 = d["flat"].clone(), m.clone(), v.clone(), state.clone()
    ctr = torch.tensor([41], dtype=torch.int64, device="cuda")
    ops.mlp_cls_fwd_bwd(net, d["x"], d["y"], d["logits"], d["loss_rows"], d["dlogits"], train=True, tick_state=state, betas=(0.5, 0.999))
    assert state.tolist()[:3] == TICKED_ONCE
    g2 = torch.zeros(n, device="cuda")
    ops.mlp_cls_wgrad_update(net, d["x"], d["dlogits"], h["w_off"], h["b_off"], g2, d["loss_rows"], d["loss"])
    before = d["flat"].clone()
    g1 = torch.zeros(n, device="cuda")
    ops.mlp_cls_wgrad_update(net, d["x"], d["dlogits"], h["w_off"], h["b_off"], g1, d["loss_rows"], d["loss"],
                             adam=dict(p=d["flat"], m=m, v=v, state=state, lr=1e-3, betas=(0.5, 0.999), weight_decay=0.01), rng_step=ctr)
    assert torch.equal(g1, g2) and int(ctr.item()) == 42 and state.tolist()[:3] == TICKED_ONCE
    ops.adam_flat(p2, g2, m2, v2, state2, 1e-3, 0.5, 0.999, weight_decay=0.01)
    named = torch.zeros(n, dtype=torch.bool, device="cuda")
    for off, t in zip(h["w_off"] + h["b_off"], h["ws"] + h["bs"]):
        named[off:off + t.numel()] = True
    assert torch.equal(d["flat"][~named], before[~named])
    assert rel_err((d["flat"] - before)[named], (p2 - before)[named]) < 1e-5
    assert rel_err(m[named], m2[named]) < 1e-6 and rel_err(v[named], v2[named]) < 1e-6


def test_domain_violations_raise_before_a_launch():
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import ops
    w = lambda o, i: torch.zeros(o, i, device="cuda")      # noqa: E731
    b = lambda o: torch.zeros(o, device="cuda")            # noqa: E731
    for dims in ([8, 513, 4], [513, 8, 4], [8, 8, 1], [8, 8, 33], [8, 8, 8, 8, 8, 8, 4], [8, 4]):
        ws = [w(o, i) for i, o in zip(dims, dims[1:])]
        with pytest.raises(ValueError):
            ops.MlpNet(4, ws, [b(o) for o in dims[1:]])
    with pytest.raises(ValueError):
        ops.MlpNet(0, [w(8, 8), w(4, 8)], [b(8), b(4)])
    with pytest.raises(ValueError):
        ops.MlpNet(4, [w(8, 8).cpu(), w(4, 8)], [b(8), b(4)])
    with pytest.raises(ValueError):
        ops.MlpNet(4, [w(8, 8), w(4, 9)], [b(8), b(4)])             # the head does not fit the hidden layer
    net, d, h = kernel_problem(5, "odd")
    with pytest.raises(ValueError):
        ops.mlp_cls_fwd_bwd(net, d["x"].cpu(), d["y"], d["logits"], d["loss_rows"], d["dlogits"])
    with pytest.raises(ValueError):
        ops.mlp_cls_fwd_bwd(net, d["x"], d["y"].int(), d["logits"], d["loss_rows"], d["dlogits"])
    with pytest.raises(ValueError):
        ops.mlp_cls_fwd_bwd(net, d["x"], d["y"], d["logits"], d["loss_rows"], None)
    with pytest.raises(ValueError):
        ops.mlp_cls_wgrad_update(net, d["x"], d["dlogits"], h["w_off"], [0] * 3, d["g"], d["loss_rows"], d["loss"])     # overlapping
    with pytest.raises(ValueError):
        ops.mlp_cls_wgrad_update(net, d["x"], d["dlogits"], h["w_off"], h["b_off"], d["g"][:50], d["loss_rows"], d["loss"])


@pytest.mark.parametrize("bad", [-1, 3, 1 << 40])
def test_out_of_range_label_poisons_its_row_and_is_never_an_index(bad):
    from melo_gan_amd import ops
    net, d, h = kernel_problem(5, "odd")
    d["y"][3] = bad
    ops.mlp_cls_fwd_bwd(net, d["x"], d["y"], d["logits"], d["loss_rows"], d["dlogits"], train=True)
    ops.mlp_cls_wgrad_update(net, d["x"], d["dlogits"], h["w_off"], h["b_off"], d["g"], d["loss_rows"], d["loss"])
    torch.cuda.synchronize()
    ok = torch.tensor([True, True, True, False, True], device="cuda")
    assert torch.isnan(d["loss"]).all() and torch.isnan(d["loss_rows"][3]) and torch.isfinite(d["loss_rows"][ok]).all()
    assert torch.isnan(d["dlogits"][3]).all() and torch.isfinite(d["dlogits"][ok]).all()
    assert torch.isfinite(d["logits"]).all()
    for l in range(2):
        assert torch.isnan(d["dz"][l][3]).all() and torch.isfinite(d["dz"][l][ok]).all()


# ---- device-drawn masks ---------------------------------------------------------------------------------------------------
def test_drawn_masks_are_rng_fills_and_a_step_on_them_matches_the_oracle():
    from melo_gan_amd import ops
    B, D, hidden = 448, 64, [256, 128]                      # 448 * 256 = 114,688 elements in the first mask
    ed_cfg = latent_cfg(D, hidden)
    spec, P = closed_form_params(ed_cfg, 16.0)
    eng = engine(dict(ed_cfg, batch_size=B, optimizer=OPT, seed=77), B)
    eng.load_state(P)
    gen = torch.Generator().manual_seed(4)
    x, y = torch.randn(B, D, generator=gen), torch.randint(0, 4, (B,), generator=gen)
    eng.set_batch(x.cuda(), y.cuda())
    eng.rng_step.fill_(5)
    for m in eng.dmask:
        m.fill_(float("nan"))
    old = {k: v.clone() for k, v in P.items()}
    eng.step_rng()
    torch.cuda.synchronize()
    assert int(eng.rng_step.item()) == 6 and eng.P.state.tolist()[:3] == TICKED_ONCE
    want = [torch.empty(B, h, device="cuda") for h in hidden]
    ops.rng_fill(None, None, want[0], want[1], 0.2, 77, torch.tensor([5], dtype=torch.int64, device="cuda"))
    for l in range(2):
        assert torch.equal(eng.dmask[l], want[l]), l
        keep = (eng.dmask[l] != 0)
        assert torch.equal(eng.dmask[l][keep], torch.full_like(eng.dmask[l][keep], 1.0 / (1.0 - 0.2)))
        n, frac = keep.numel(), keep.float().mean().item()
        assert abs(frac - 0.8) <= 5 * math.sqrt(0.8 * 0.2 / n), (l, frac)
    # the step it took is the oracle's step on exactly these masks
    opt = O.AdamState(P, 2e-4, (0.5, 0.999), 1e-8, weight_decay=0.01, decoupled=True)
    r = O.ed_step(P, {}, opt, x, y, ed_cfg, [m.cpu() for m in eng.dmask])
    assert abs(eng.loss.item() - float(r["loss"])) < 5e-6
    np.testing.assert_allclose(eng.logits.cpu().numpy(), r["logits"].numpy(), rtol=2e-3, atol=2e-5)
    for k in spec:
        upd, upd_ref = eng.P.p[k].cpu() - old[k], P[k] - old[k]
        assert rel_err(upd, upd_ref) < 0.1, (k, rel_err(upd, upd_ref))
    # a different counter draws different masks; layers 2 and 3 have streams of their own
    first = [m.clone() for m in eng.dmask]
    eng.step_rng()
    assert not torch.equal(first[0], eng.dmask[0])
    e4 = engine(dict(latent_cfg(16, [128, 128, 128, 128]), batch_size=256, optimizer=OPT, seed=77), 256, seed=1)
    e4.set_batch(torch.randn(256, 16).cuda(), torch.zeros(256, dtype=torch.int64).cuda())
    e4.step_rng()
    torch.cuda.synchronize()
    ms = [m.flatten() for m in e4.dmask]
    for i in range(4):
        assert abs((ms[i] != 0).float().mean().item() - 0.8) <= 5 * math.sqrt(0.16 / ms[i].numel())
        for j in range(i):
            assert not torch.equal(ms[i], ms[j]), (i, j)


# ---- reproducibility and graph shape --------------------------------------------------------------------------------------
def snapshot(eng):
    torch.cuda.synchronize()
    s = {"data": eng.P.data, "m": eng.P.m, "v": eng.P.v, "state": eng.P.state, "rng_step": eng.rng_step, "metrics": eng.metrics,
         "grad": eng.P.grad, "loss": eng.loss}
    s.update({"buf." + k: v for k, v in eng.buf.items()})
    return {k: v.clone() for k, v in s.items() if v is not None}      # no split attached: no metrics


@pytest.mark.parametrize("sn", [False, True])
def test_graph_replay_equals_eager_and_reruns_are_bit_identical(sn):
    B, D, n = 16, 24, 16 * 5
    cfg = dict(latent_cfg(D, [72, 40], use_spectral_norm=sn), batch_size=B, optimizer=dict(OPT, lr=1e-3), seed=9)
    gen = torch.Generator().manual_seed(2)
    x, y = torch.randn(n, D, generator=gen).cuda(), torch.randint(0, 4, (n,), generator=gen).cuda()
    order = torch.randperm(n, generator=gen)
    snaps = []
    for use_graph in (True, False, False):
        eng = engine(cfg, B, seed=3)
        eng.attach_split(x, y)
        eng.set_epoch(order, 0)
        with torch.cuda.stream(eng.stream):
            for _ in range(5):
                eng.run("step_staged", use_graph)
        snaps.append(snapshot(eng))
        if use_graph:
            graph = eng._graphs["step_staged"]
            assert not isinstance(graph, str)
            assert graph.kernel_nodes <= (5 if sn else 2), graph.kernel_nodes
    for k in snaps[0]:
        assert torch.equal(snaps[0][k].view(torch.uint8), snaps[1][k].view(torch.uint8)), ("graph vs eager", k)
        assert torch.equal(snaps[1][k].view(torch.uint8), snaps[2][k].view(torch.uint8)), ("rerun", k)
    assert int(snaps[0]["rng_step"].item()) == 5 and snaps[0]["state"][0].item() == 5.0
    assert snaps[0]["metrics"][0].item() > 0 and torch.isfinite(snaps[0]["data"]).all()


# ---- staging --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("fused,D", [(True, 10), (True, 64), (False, 64)])
def test_staged_epochs_are_the_host_loop_bit_for_bit(use_graph, fused, D):
    """n = 2B + 3: three epochs by the staged step leave the parameters, Adam moments and counters of run_epoch's host path and
    return the same (loss, acc), the trailing partial batch included (tests/test_ed_staged_gpu.py's check, in latent mode)."""
    from melo_gan_amd.emotion_discriminator import train_ed
    B = 8
    n = 2 * B + 3
    cfg = dict(latent_cfg(D, [40, 24]), batch_size=B, optimizer=dict(OPT, lr=1e-3))
    g = torch.Generator().manual_seed(21)
    x, y = torch.randn(n, D, generator=g).cuda(), torch.randint(0, 4, (n,), generator=g).cuda()
    host, staged = engine(cfg, B, fused, seed=3), engine(cfg, B, fused, seed=3)
    staged.attach_split(x, y)
    gen_h, gen_s = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    for epoch in range(3):
        with torch.cuda.stream(host.stream):
            want = train_ed.run_epoch(host, x, y, True, use_graph, gen_h)
        with torch.cuda.stream(staged.stream):
            got = train_ed.run_epoch_staged(staged, epoch, use_graph, gen_s)
        assert got == want, (epoch, got, want)
        a, b = snapshot(host), snapshot(staged)
        for k in ("data", "m", "v", "state", "rng_step"):
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), (epoch, k)
    assert float(staged.P.state[0].item()) == 9.0 and int(staged.rng_step.item()) == 9
    if use_graph:
        assert not isinstance(staged._graphs["step_staged"], str) and not isinstance(staged.tail(3)._graphs["step_staged"], str)


def test_weighted_sampler_epoch_uses_weighted_orders_buffer():
    from melo_gan_amd import ops
    from melo_gan_amd.emotion_discriminator import train_ed
    B, D, n = 8, 12, 37
    cfg = dict(latent_cfg(D, [40, 24]), batch_size=B, optimizer=OPT, seed=13)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(n, D, generator=g).cuda()
    y = torch.tensor([0] * 30 + [1] * 4 + [2] * 2 + [3], dtype=torch.int64).cuda()
    eng = engine(cfg, B, seed=3)
    eng.attach_split(x, y)
    cdf = ops.sampler_cdf(y)
    seen = []
    orig = eng.tail(n % B)
    with torch.cuda.stream(eng.stream):
        for epoch in range(2):
            train_ed.run_epoch_staged(eng, epoch, True, None, cdf)
            torch.cuda.synchronize()
            want = ops.weighted_order(cdf, torch.empty(n, dtype=torch.int64, device="cuda"), 13, epoch)
            assert torch.equal(eng.order, want), epoch
            seen.append(eng.order.clone())
            # the trailing partial batch really came from the order's last positions
            assert torch.equal(orig.y, y[want[n - n % B:]]) and torch.equal(orig.x, x[want[n - n % B:]])
    assert not torch.equal(seen[0], seen[1])
    assert torch.bincount(y[torch.cat(seen)], minlength=4).min() >= 5          # every class ~ 1/4 of the 74 draws, the 1-row class too


# ---- spectral norm --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
def test_latent_pretraining_with_spectral_norm_matches_the_oracle(fused):
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.emotion_discriminator.ed_model import EmotionDiscriminator
    B, D, hidden = 8, 32, [256, 128]
    ed_cfg = latent_cfg(D, hidden, use_spectral_norm=True)
    spec, P = closed_form_params(ed_cfg, 4.0)
    g = torch.Generator().manual_seed(11)
    names = O.ed_sn_layers(ed_cfg)
    assert names == ["classifier.net.0", "classifier.net.3"]
    Bf = {}
    for nm in names:
        shp = spec[nm + ".weight"]
        Bf[nm + ".weight_u"] = F.normalize(torch.randn(shp[0], generator=g), dim=0)
        Bf[nm + ".weight_v"] = F.normalize(torch.randn(shp[1], generator=g), dim=0)
    eng = engine(dict(ed_cfg, batch_size=B, optimizer=OPT), B, fused)
    assert eng.sn_names == names
    eng.load_state(P, Bf)
    opt = O.AdamState(P, 2e-4, (0.5, 0.999), 1e-8, weight_decay=0.01, decoupled=True)
    for it in range(3):
        x, y = torch.randn(B, D, generator=g), torch.randint(0, 4, (B,), generator=g)
        dm = [(torch.rand(B, h, generator=g) >= 0.2).float() / 0.8 for h in hidden]
        eng.set_batch(x.cuda(), y.cuda())
        eng.set_masks([m.cuda() for m in dm])
        eng.backward()
        P64 = {k: v.double().clone().requires_grad_(True) for k, v in P.items()}
        B64 = {k: v.double().clone() for k, v in Bf.items()}
        l64 = F.cross_entropy(O.emotion_disc_fwd(P64, B64, x.double(), ed_cfg, True, [m.double() for m in dm]), y)
        g64 = dict(zip(P64, torch.autograd.grad(l64, list(P64.values()))))
        old = {k: v.clone() for k, v in P.items()}
        r = O.ed_step(P, Bf, opt, x, y, ed_cfg, dm)
        assert abs(eng.loss.item() - float(r["loss"])) < 2e-5
        assert rel_err(eng.logits, r["logits"]) < 2e-3
        for k in spec:
            e_mine, e_ref = rel_err(eng.P.g[k], g64[k]), rel_err(r["grads"][k], g64[k])
            assert e_mine <= 6.0 * e_ref + 3e-4, (it, k, e_mine, e_ref)
        for nm in names:
            assert rel_err(eng.buf[nm + ".weight_u"], Bf[nm + ".weight_u"]) < 1e-5, (it, nm)
            assert rel_err(eng.buf[nm + ".weight_v"], Bf[nm + ".weight_v"]) < 1e-5, (it, nm)
        eng.update()
        for k in spec:
            upd, upd_ref = eng.P.p[k].cpu() - old[k], P[k] - old[k]
            assert rel_err(upd, upd_ref) < 0.1, (it, "AdamW update", k, rel_err(upd, upd_ref))
        eng.load_state(P, Bf)
    x = torch.randn(B, D, generator=g)
    eng.set_batch(x.cuda(), torch.zeros(B, dtype=torch.int64).cuda())
    u_before = {nm: eng.buf[nm + ".weight_u"].clone() for nm in names}
    eng.forward_eval()
    want = O.emotion_disc_fwd(P, Bf, x, ed_cfg, train=False)
    assert rel_err(eng.logits, want) < 2e-3
    assert all(torch.equal(eng.buf[nm + ".weight_u"], u_before[nm]) for nm in names)
    sd = eng.state_dict()
    mirror = EmotionDiscriminator(dict(ed_cfg)).cuda().eval()
    assert set(sd) == set(mirror.state_dict()), set(sd) ^ set(mirror.state_dict())
    assert all(tuple(sd[k].shape) == tuple(v.shape) for k, v in mirror.state_dict().items())
    mirror.load_state_dict(sd)
    assert rel_err(mirror(x.cuda()), want) < 2e-3


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_trainer_cli_learns_the_quadrants_and_its_checkpoint_feeds_the_gan(tmp_path, capsys):
    """train_ed's CLI on the synthetic latent split (class = quadrant of (x0, x1)): validation accuracy >= 0.80 after ten
    epochs -- the reference module with the same data rule and optimiser reaches 0.906-0.945 (val loss <= 0.49) on the CPU over
    three seeds; the margin absorbs a different initialisation and mask stream.  The checkpoint then loads into the GAN
    engine's frozen latent-mode classifier and into gan.generate's sampler."""
    import yaml
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.emotion_discriminator import train_ed
    from melo_gan_amd.gan import generate as G
    from melo_gan_amd.gan import train_gan
    from melo_gan_amd.gan.engine import GanEngine
    cfg = dict(O.default_ed_cfg(4), input_mode="latent", latent_dim=8, dropout=0.2, batch_size=64, num_epochs=50, seed=42,
               optimizer=dict(name="AdamW", lr="2e-4", betas=[0.5, 0.999], weight_decay=0.0),
               scheduler=dict(name="ReduceLROnPlateau", mode="min", factor=0.5, patience=5, threshold=0.0001),
               metric_for_best="val_loss", early_stopping_patience=10, save_freq=5, augment=True,
               checkpoint_dir=str(tmp_path), save_name="ed_best.pth")
    path = os.path.join(str(tmp_path), "ed_latent.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    train_ed.main(["--config", path, "--synthetic", "1024", "--epochs", "10"])
    out = capsys.readouterr().out
    assert "Input mode: latent" in out and "no effect with input_mode=latent" in out
    last = [ln for ln in out.splitlines() if ln.startswith("[Epoch 010]")]
    assert len(last) == 1, out
    val_acc = float(last[0].split("Val-Acc=")[1].split()[0])
    print(last[0])
    assert val_acc >= 0.80, last[0]
    ck_path = os.path.join(str(tmp_path), "ed_best.pth")
    ck = torch.load(ck_path, map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "model", "optimizer", "cfg"}
    assert list(ck["model"]) == ["classifier.net.0.weight", "classifier.net.0.bias", "classifier.net.3.weight", "classifier.net.3.bias",
                                 "classifier.head.weight", "classifier.head.bias"]
    assert os.path.exists(os.path.join(str(tmp_path), "ed_epoch005.pth"))
    gcfg = dict(O.default_gan_cfg(4, 16, 4), LATENT_DIM=8, INTEGRATION_MODE="conditioning")
    ecfg = dict(O.default_ed_cfg(4), input_mode="latent", latent_dim=8)
    gan = GanEngine(gcfg, ecfg, "cuda", 4)
    gan.init_weights(0)
    assert train_gan.load_ed_checkpoint(gan, ck_path)
    for k in gan.ED.spec:
        assert torch.equal(gan.ED.p[k].cpu(), ck["model"][k]), k
    smp = G.Sampler(gcfg, ecfg, "cuda", 8)
    smp.load_ed(ck_path)
    for k in smp.eng.ED.spec:
        assert torch.equal(smp.eng.ED.p[k].cpu(), ck["model"][k]), k
    res = smp.sample(["all"], 2, seed=3)
    assert np.isfinite(smp.eng.logits.cpu().numpy()).all() and np.isfinite(res.p_target).all()
