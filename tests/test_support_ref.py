"""CPU self-test of tests/support_ref.py, the fp64 references and per-element bounds tests/test_support_contract_gpu.py holds
the streaming kernels to: (a) the references equal torch's fp64 modules and autograd wherever torch defines the operation;
(b) an fp32 host computation of every operation passes every bound at every shape of the GPU file's tables (the ratios are
printed; BatchNorm is emulated with fp64 statistics rounded to fp32, as a correct kernel computes it, the rest is plain fp32
torch), and the tables reach the branches the GPU file claims -- the launch plans are restated here with a pointer to the
source line; (c) each of a list of plausible kernel mistakes, built from the fp64 reference at a table shape, leaves its
bound -- the measured ratios are in test_subtle_errors_are_flagged's docstring.  No GPU needed."""
import math

import pytest
import torch
import torch.nn.functional as F

import support_ref as R
import test_support_contract_gpu as G

NONE, RELU, LRELU, GELU, TANH = G.NONE, G.RELU, G.LRELU, G.GELU, G.TANH
CPU = "cpu"


def rnd(*shape, seed=0, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale + shift


def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-300))


def ratio(got, ref):
    return R.worst(got, ref)[0]


def torch_act(act, v):
    return {NONE: lambda t: t, RELU: torch.relu, LRELU: lambda t: F.leaky_relu(t, 0.2), GELU: F.gelu, TANH: torch.tanh}[act](v)


# ---------------------------------------------------------------------------------------------------------------------
# (a) the references are the operations they claim to be
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [1, 2, 3])
@pytest.mark.parametrize("Rn,C", [(2, 4), (37, 6), (65, 5)])
@pytest.mark.parametrize("act", [NONE, RELU, LRELU, GELU, TANH])
def test_batchnorm_is_torch_batch_norm_and_its_autograd(groups, Rn, C, act):
    z = rnd(groups * Rn, C, seed=1, scale=2.0, shift=0.3)
    gamma, beta = rnd(C, seed=2, shift=1.0), rnd(C, seed=3)
    rm0, rv0 = rnd(C, seed=4), rnd(C, seed=5).abs() + 0.5
    mom, eps = R.f32(0.1), R.f32(1e-5)
    st = R.bn_stats(z, groups, 1e-5)
    rm, rv = rm0.clone(), rv0.clone()
    outs = []
    for g in range(groups):                                 # `groups` consecutive calls of the module
        outs.append(F.batch_norm(z[g * Rn:(g + 1) * Rn], rm, rv, gamma, beta, True, mom, eps))
    r_m, r_v = R.bn_running(st, rm0, rv0, 0.1)
    assert rel(r_m.val, rm) < 1e-13 and rel(r_v.val, rv) < 1e-13
    a = R.bn_apply(z, st["mean"], st["invstd"], gamma, beta, act)
    assert rel(a.val, torch_act(act, torch.cat(outs))) < 1e-13
    assert bool((a.mag >= torch.cat(outs).abs() * (1 - 1e-12)).all())
    # autograd of one group
    zz, gg, bb = z[:Rn].clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = torch_act(act, F.batch_norm(zz, None, None, gg, bb, True, mom, eps))
    da = rnd(Rn, C, seed=6)
    y.backward(da)
    s1 = R.bn_stats(z[:Rn], 1, 1e-5)
    dz, dg, db = R.bn_bwd(da, y.detach(), z[:Rn], gamma, beta, s1["mean"][0], s1["invstd"][0], act)
    # stride2_ref.act_grad_ref carries LeakyReLU's slope as the fp32 constant the kernels use (0.2f = 0.2 (1 + 7.5e-9))
    tol = 2e-8 if act == LRELU else 1e-12
    assert float(((dz.val - zz.grad).abs() / (dz.mag + 1e-300)).max()) < tol        # relative to the magnitude: two rows cancel almost fully
    assert rel(dg.val, gg.grad) < 10 * tol and rel(db.val, bb.grad) < 10 * tol
    assert bool((dz.mag >= dz.val.abs() * (1 - 1e-12)).all())


def test_batchnorm_of_one_row_and_eval_mode():
    z, gamma, beta = rnd(1, 4, seed=1), rnd(4, seed=2), rnd(4, seed=3)
    st = R.bn_stats(z, 1, 1e-5)                             # F.batch_norm raises for one row
    assert bool((st["var"] == 0).all()) and bool((st["unb"] == 0).all())
    assert rel(R.bn_apply(z, st["mean"], st["invstd"], gamma, beta).val, beta[None]) < 1e-15
    _, rv = R.bn_running(st, torch.zeros(4), torch.ones(4), 0.1)
    assert rel(rv.val, torch.full((4,), 1.0 - R.f32(0.1), dtype=torch.float64)) < 1e-15
    z = rnd(9, 4, seed=4)
    rm, rv = rnd(4, seed=5), rnd(4, seed=6).abs() + 0.1
    want = F.batch_norm(z, rm, rv, gamma, beta, False, 0.1, R.f32(1e-5))
    assert rel(R.bn_eval(z, gamma, beta, rm, rv, 1e-5).val, want) < 1e-13
    cb = rnd(4, seed=7)
    sc, sh = R.bn_fold(gamma, beta, rm, rv, cb, 1e-5)
    x = rnd(9, 4, seed=8)
    assert rel(x * sc.val + sh.val, F.batch_norm(x + cb, rm, rv, gamma, beta, False, 0.1, R.f32(1e-5))) < 1e-13


@pytest.mark.parametrize("np_,Rn,empties", [(1, 5, ()), (4, 37, (1,)), (17, 100, (0, 16)), (300, 1000, (0, 1, 299))])
def test_partials_combine_to_the_statistics_of_the_whole(np_, Rn, empties):
    z = rnd(Rn, 6, seed=np_, scale=2.0, shift=0.3).float()
    part, sizes = R.conv16_parts(z, np_, empties)
    assert part.shape == (np_, 3, 6) and part.dtype == torch.float32 and sum(sizes) == Rn
    assert all(sizes[e] == 0 for e in empties) and bool((part[list(empties), 2] == 0).all())
    if np_ > 1:
        assert max(sizes) > 4 * sorted(sizes)[len(sizes) // 2] or Rn < 40          # very unequal chunks
    st, want = R.parts_stats(part, 1e-5), R.bn_stats(z, 1, 1e-5)
    assert rel(st["mean"], want["mean"]) < 1e-6 and rel(st["var"], want["var"]) < 1e-5 and st["R"] == Rn
    # the fp64 partials of the backward add up to the whole
    da, a = rnd(Rn, 6, seed=3).float(), rnd(Rn, 6, seed=4).float()
    mean, invstd = want["mean"][0].float(), want["invstd"][0].float()
    bp = R.bwd_parts(da, a, z, mean, invstd, RELU, np_)
    _, dg, db = R.bn_bwd(da, a, z, torch.ones(6), torch.zeros(6), mean, invstd, RELU)
    assert bp.shape == (np_, 2, 6) and rel(bp[:, 0].sum(0), db.val) < 1e-12 and rel(bp[:, 1].sum(0), dg.val) < 1e-12


@pytest.mark.parametrize("B,D", [(1, 1), (3, 6), (65, 63)])
def test_layernorm_and_mean_over_time(B, D):
    x, gamma, beta = rnd(B, D, seed=1, shift=0.5), rnd(D, seed=2), rnd(D, seed=3)
    y, xh = R.layernorm_fwd(x, gamma, beta, 1e-5)
    assert rel(y.val, F.layer_norm(x, (D,), gamma, beta, R.f32(1e-5))) < 1e-13
    gg, bb = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    dy = rnd(B, D, seed=4)
    (xh.val * gg + bb).backward(dy)
    dg, db = R.layernorm_bwd_params(dy, xh.val)
    assert rel(dg.val, gg.grad) < 1e-13 and rel(db.val, bb.grad) < 1e-13
    a = rnd(B, 7, D, seed=5).requires_grad_(True)
    h = R.meanT_fwd(a.detach())
    assert rel(h.val, a.detach().mean(1)) < 1e-15
    gscale, dh = rnd(D, seed=6), rnd(B, D, seed=7)
    (torch.tanh(a).mean(1) * gscale).backward(dh)
    dz = R.meanT_bwd(dh, 7, torch.tanh(a.detach()), TANH, gscale)
    assert rel(dz.val, a.grad) < 1e-13
    assert rel(R.mean_scaled(dh, -1.0).val, -dh.mean().reshape(1)) < 1e-15


@pytest.mark.parametrize("B,Be,Fd,E", [(1, 1, 1, 0), (6, 3, 5, 2), (8, 8, 3, 4)])
def test_critic_head_is_a_linear_layer_behind_leaky_relu(B, Be, Fd, E):
    Uu = rnd(B, Fd, seed=1).requires_grad_(True)
    w, bias = rnd(Fd + E, seed=2).requires_grad_(True), rnd(1, seed=3).requires_grad_(True)
    emb = rnd(Be, E, seed=4).requires_grad_(True) if E else None
    f = F.leaky_relu(Uu, 0.2)
    full = torch.cat([f, emb.repeat(B // Be, 1)], dim=1) if E else f
    s = F.linear(full, w[None], bias)[:, 0]
    ds = rnd(B, seed=5)
    s.backward(ds)
    fd = f.detach()
    assert rel(R.dhead_fwd(fd, None if emb is None else emb.detach(), w.detach(), bias.detach()).val, s.detach()) < 1e-13
    refs = R.dhead_bwd(ds, fd, w.detach(), Be, E, B)
    assert rel(refs[0].val, Uu.grad) < 1e-13
    if E:
        assert rel(refs[1].val, emb.grad) < 1e-13
    dwf, dwe, dbias = R.dhead_wgrad(ds, fd, None if emb is None else emb.detach(), None, B, 0)
    assert rel(torch.cat([dwf.val, dwe.val]) if E else dwf.val, w.grad) < 1e-13 and rel(dbias.val, bias.grad) < 1e-13
    gf = rnd(3, Fd, seed=6)
    assert rel(R.dhead_wgrad(ds, fd, None, gf, B, 3)[0].val, w.grad[:Fd] + gf.sum(0)) < 1e-13
    sv, norms = rnd(2 * B, seed=7), rnd(B, seed=8).abs()
    ld, mr, mf, gp = R.wgan_d_loss(sv, norms, 10.0, B)
    assert rel(ld.val, (sv[B:].mean() - sv[:B].mean() + 10.0 * ((norms - 1) ** 2).mean()).reshape(1)) < 1e-13
    assert rel(gp.val, ((norms - 1) ** 2).mean().reshape(1)) < 1e-14 and rel(mr.val, sv[:B].mean().reshape(1)) < 1e-14


def test_gradient_penalty_and_cross_entropy_are_autograd():
    g = rnd(6, 37, seed=1, scale=0.2).requires_grad_(True)
    pen = 10.0 * ((g.norm(dim=1) - 1) ** 2).mean()
    pen.backward()
    norms, gbar, gp = R.gp_penalty(g.detach(), 10.0)
    assert rel(gbar.val, g.grad) < 1e-13 and rel(10.0 * gp.val, pen.detach().reshape(1)) < 1e-13
    assert rel(norms.val, g.detach().norm(dim=1)) < 1e-15
    zero = torch.zeros(2, 5, dtype=torch.float64)
    assert bool((R.gp_penalty(zero, 1.0)[1].val == 0).all())
    real, fake, alpha = rnd(3, 4, seed=2), rnd(3, 4, seed=3), torch.tensor([0.0, 1.0, 0.3], dtype=torch.float64)
    assert rel(R.gp_interp(real, fake, alpha).val, alpha[:, None] * real + (1 - alpha[:, None]) * fake) < 1e-15
    z = rnd(9, 5, seed=4, scale=30.0).requires_grad_(True)
    y = torch.randint(0, 5, (9,), generator=torch.Generator().manual_seed(5))
    (R.f32(0.7) * F.cross_entropy(z, y)).backward()
    loss, dl, bad = R.softmax_ce(z.detach(), y, 0.7)
    assert rel(loss.val, F.cross_entropy(z.detach(), y).reshape(1)) < 1e-13 and rel(dl.val, z.grad) < 1e-13 and not bool(bad.any())
    y[2] = 5
    loss, dl, bad = R.softmax_ce(z.detach(), y, 0.7)
    assert math.isnan(float(loss.val)) and bool(torch.isnan(dl.val[2]).all()) and int(torch.isnan(dl.val).sum()) == 5


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("decoupled", [True, False])
def test_adam_step_is_torch_optim(wd, decoupled):
    p0, g, m0 = rnd(50, seed=1), rnd(50, seed=2, scale=0.3), rnd(50, seed=3, scale=0.1)
    v0 = rnd(50, seed=4, scale=0.1) ** 2
    hp = dict(lr=R.f32(2e-4), betas=(R.f32(0.5), R.f32(0.999)), eps=R.f32(1e-8), weight_decay=R.f32(wd))
    p = p0.clone().requires_grad_(True)
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([p], **hp)
    opt.state[p] = dict(step=torch.tensor(7.0), exp_avg=m0.clone(), exp_avg_sq=v0.clone())
    p.grad = g.clone()
    opt.step()
    rp, rm, rv = R.adam_step(p0, g, m0, v0, 8, 2e-4, 0.5, 0.999, 1e-8, wd, decoupled=decoupled)
    assert rel(rp.val, p.detach()) < 1e-13
    assert rel(rm.val, opt.state[p]["exp_avg"]) < 1e-13 and rel(rv.val, opt.state[p]["exp_avg_sq"]) < 1e-13
    # the scales multiply the gradient
    rp2, _, _ = R.adam_step(p0, g * 4, m0, v0, 8, 2e-4, 0.5, 0.999, 1e-8, wd, grad_scale=0.5, gs_dev=torch.tensor([0.5]))
    assert decoupled is False or rel(rp2.val, R.adam_step(p0, g, m0, v0, 8, 2e-4, 0.5, 0.999, 1e-8, wd)[0].val) < 1e-13


def test_clip_coefficient_vae_loss_and_wq_layout():
    for scale, mx in ((1.0, 0.25), (0.01, 4.0)):
        g = rnd(100, seed=1, scale=scale)
        p = torch.zeros(100, dtype=torch.float64, requires_grad=True)
        p.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_([p], mx)
        ref = R.grad_norm_clip(g, mx)
        assert rel(ref.val[0], total) < 1e-14 and rel(ref.val[1] * g, p.grad) < 1e-9
    assert R.grad_norm_clip(torch.zeros(5), 1.0).val.tolist() == [0.0, 1.0]
    recon, x = rnd(3, 10, seed=2).requires_grad_(True), rnd(3, 10, seed=3)
    mu, lv = rnd(3, 4, seed=4).requires_grad_(True), rnd(3, 4, seed=5).requires_grad_(True)
    bt = R.f32(0.3)
    mse = F.mse_loss(recon, x)
    kld = -0.5 * torch.mean(1 + lv - mu.pow(2) - lv.exp())
    (mse + bt * kld).backward()
    (tot, rmse, rk), dr, dm, dl = R.vae_loss(recon.detach(), x, mu.detach(), lv.detach(), 0.3)
    assert rel(tot.val, (mse + bt * kld).detach().reshape(1)) < 1e-13 and rel(rmse.val, mse.detach().reshape(1)) < 1e-13
    assert rel(rk.val, kld.detach().reshape(1)) < 1e-13
    assert rel(dr.val, recon.grad) < 1e-13 and rel(dm.val, mu.grad) < 1e-13 and rel(dl.val, lv.grad) < 1e-13
    e = rnd(3, 4, seed=6)
    (mu + e * torch.exp(0.5 * lv)).backward(rnd(3, 4, seed=7))
    # reparameterisation: autograd adds to the KLD gradients already in .grad
    rm_, rl_ = R.reparam_bwd(rnd(3, 4, seed=7), lv.detach(), e, dm.val, dl.val)
    assert rel(rm_.val, mu.grad) < 1e-13 and rel(rl_.val, lv.grad) < 1e-13
    assert rel(R.reparam_fwd(mu.detach(), lv.detach(), e).val, (mu + e * torch.exp(0.5 * lv)).detach()) < 1e-15
    N, Cc, K = 3, 8, 5
    w = torch.arange(N * Cc * K, dtype=torch.float32)
    for cnk in (False, True):
        dst = R.wq_layout(w, N, Cc, K, cnk)
        for n in range(N):
            for c in range(Cc):
                for k in range(K):
                    src = (c * N + n) * K + k if cnk else (n * Cc + c) * K + k
                    assert dst[(((c // 4) * K + k) * N + n) * 4 + c % 4] == w[src]


# ---------------------------------------------------------------------------------------------------------------------
# (b) the tables reach what the GPU file claims, and fp32 host computations pass every bound
# ---------------------------------------------------------------------------------------------------------------------
RED_SPLITS, BNA_PL = 256, 16              # csrc/small_kernels.hip: RED_SPLITS, BNA_PL = BNA_THREADS / 64


def cdiv(a, b):
    return -(-a // b)


def red_plan(Rn):
    """csrc/small_kernels.hip, red_plan(): (nsplit, rows_per)."""
    ns = max(1, min(cdiv(Rn, 64), RED_SPLITS))
    rows_per = cdiv(Rn, ns)
    return cdiv(Rn, rows_per), rows_per


def bn_row_slices(Rn, C, groups):
    """csrc/small_kernels.hip, bn_row_slices(): (slices, rows_per)."""
    n = max(1, 256 // (cdiv(C, 64) * groups))
    n = min(n, cdiv(Rn, 64))
    rows_per = cdiv(Rn, n)
    return cdiv(Rn, rows_per), rows_per


def combine_rounds(np_):
    """Trips of the `for (q0 = pl; q0 < np; q0 += 8 * BNA_PL)` loop of combine_parts64 / combine_colsum64 / the bwd combine."""
    return cdiv(np_, 8 * BNA_PL)


def test_tables_reach_the_branches_they_claim():
    Rs, Cs = {r for r, _ in G.RC_PAIRS}, {c for _, c in G.RC_PAIRS}
    assert Rs == {1, 15, 16, 17, 63, 64, 65, 1000, 8193, 16385} and Cs == {1, 3, 4, 6, 60, 64, 65, 68, 130, 256}
    assert max(r * c for r, c in G.RC_PAIRS) == 16385 * 130
    assert red_plan(16385) == (253, 65) and red_plan(8193) == (129, 64) and red_plan(1) == (1, 1)        # the RED_SPLITS clamp
    assert combine_rounds(red_plan(8193)[0]) == 2 and combine_rounds(red_plan(16385)[0]) == 2 and combine_rounds(red_plan(1000)[0]) == 1
    ragged4 = [(r, c) for r, c in G.RC_PAIRS if c % 4 == 0 and c % 64]           # vector path, ragged last channel block
    assert (16385, 68) in ragged4 and (1000, 68) in ragged4
    assert any(c % 4 and red_plan(r)[0] == 253 for r, c in G.RC_PAIRS)           # scalar path x clamped R
    assert any(bn_row_slices(r, c, 1)[0] > 1 and r % bn_row_slices(r, c, 1)[1] for r, c in G.RC_PAIRS)   # a short last row slice
    # b. every act, groups 1 / 2 / 3, R = 1 and 2, with and without running statistics, offset data, clamped R
    assert {c[3] for c in G.BN_FWD} == set(G.ALL_ACTS) and {c[2] for c in G.BN_FWD} == {1, 2, 3}
    assert {1, 2} <= {c[0] for c in G.BN_FWD} and {c[4] for c in G.BN_FWD} == {True, False} and any(c[5] for c in G.BN_FWD)
    assert any(c[0] == 1 and c[2] > 1 and c[4] for c in G.BN_FWD)                # the R > 1 ? ... : var guard, group after group
    assert any(red_plan(c[0])[0] == 253 and c[1] == 68 for c in G.BN_FWD)
    assert all(c[1] % 4 or c[1] % 64 for c in G.BN_EVAL)
    # c. / d. the partial counts: one round, exactly one round, a second round, three rounds
    assert [c[0] for c in G.BN_PARTS] == [1, 16, 17, 128, 129, 300] == [c[0] for c in G.BWD_PARTS]
    assert [combine_rounds(n) for n in (1, 16, 17, 128, 129, 300)] == [1, 1, 1, 1, 2, 3]
    assert {c[1] for c in G.BN_PARTS} == {1, 2} and sum(1 for c in G.BN_PARTS if c[4]) >= 4 and any(c[5] for c in G.BN_PARTS)
    assert all(len(c[4]) < c[0] and c[0] - len(c[4]) <= c[2] for c in G.BN_PARTS)
    # e. T and C; the vector kernel needs C % 4 == 0 (and aligned tensors: off4 takes the scalar one)
    assert {t for _, t, _ in G.MEANT} == {1, 15, 16, 17, 37, 300} and {c for _, _, c in G.MEANT} == {4, 6, 64, 68, 96, 130}
    assert any(c % 4 for _, _, c in G.MEANT) and any(c % 4 == 0 and c % 64 for _, _, c in G.MEANT)
    assert G.MEAN_N == [1, 255, 256, 257, 1000]                                   # block_sum of 256 threads: below, at, above, a loop
    assert {d_ for _, d_ in G.LAYERNORM} == {1, 6, 63, 64} and {b for b, _ in G.LAYERNORM} == {1, 3, 4, 5, 64, 65, 300}
    assert {c[2] for c in G.DHEAD} == {1, 63, 64, 65, 256} and {c[3] for c in G.DHEAD} == {0, 1, 128, 130}
    assert {(c[0], c[1]) for c in G.DHEAD} == {(1, 1), (6, 3), (65, 65), (192, 64)}
    # h. gp_penalty: vec = n % 4 == 0 && n <= 32768 && aligned (gp_norm_kernel); n4 = 1025 is no multiple of 1024
    vec = lambda n, off: n % 4 == 0 and n <= 1024 * 32 and not off  # noqa: E731
    ns = {c[1] for c in G.GP_PENALTY}
    assert ns == {1, 5, 4096, 4100, 32768, 32772, 40001} and {c[0] for c in G.GP_PENALTY} == {1, 6, 257}
    assert vec(32768, False) and not vec(32772, False) and not vec(40001, False) and not vec(5, False) and (4100 // 4) % 1024
    assert any(c[2] and c[1] % 4 == 0 for c in G.GP_PENALTY) and any(not c[3] for c in G.GP_PENALTY) and any(not c[4] for c in G.GP_PENALTY)
    assert {b for b, _ in G.SOFTMAX_CE if b > 256} == {257, 1000} and {c for _, c in G.SOFTMAX_CE} >= {1, 32}
    # j. vae_loss: vec = n_x % 4 == 0 && aligned; more than VAE_LOSS_BLOCKS * 1024 elements make a block loop
    assert [nx % 4 == 0 for nx, _ in G.VAE] == [True, False, False, True, True, False] and max(nx for nx, _ in G.VAE) > 256 * 256
    assert {nz for _, nz in G.VAE} == {1, 255, 256, 257, 2048}
    assert [min(cdiv(n, 8192), 1024) for n in G.GRAD_NORM_N] == [1, 1, 1, 2, 1024]          # mg_grad_norm_clip: nparts


class Ratios:
    def __init__(self):
        self.rows = []

    def add(self, what, got, ref):
        r = ratio(got, ref)
        self.rows.append((r, what))
        return r

    def finish(self, capsys, title):
        with capsys.disabled():
            print(f"\n[support ref] {title}")
            for r, what in self.rows:
                print(f"    {r:10.4f}  {what}")
        bad = [(r, what) for r, what in self.rows if not r <= 1.0]
        assert not bad, bad


def emu_bn_apply(z, mean32, invstd32, gamma, beta, act, groups):
    """What a correct kernel computes: fp64 per-element math from the fp32-rounded statistics, one rounding, fp32 activation."""
    C = z.shape[1]
    v = (z.double().view(groups, -1, C) - mean32.double()[:, None]) * invstd32.double()[:, None] * gamma.double() + beta.double()
    return torch_act(act, v.view(z.shape).float())


def emu_running(st, r0m, r0v, mom):
    mom = R.f32(mom)
    rm, rv = r0m.clone(), r0v.clone()
    for g in range(st["mean"].shape[0]):
        rm = ((1.0 - mom) * rm.double() + mom * st["mean"][g]).float()
        rv = ((1.0 - mom) * rv.double() + mom * st["unb"][g]).float()
    return rm, rv


def one_pass_stats(z, groups, eps):
    """fp64 sums of x and x^2 (colsum partials), mean and E[x^2] - mean^2 in fp64: the formulation the bound's fp64 term allows."""
    C = z.shape[1]
    x = z.double().view(groups, -1, C)
    mean = x.sum(1) / x.shape[1]
    var = ((x * x).sum(1) / x.shape[1] - mean * mean).clamp_min(0.0)
    return mean, (var + R.f32(eps)) ** -0.5


def test_fp32_batchnorm_and_colsum_pass_the_bound(capsys):
    rt = Ratios()
    for i, (Rn, C) in enumerate(G.RC_PAIRS):
        for offset in (False, True):
            x = G.data(Rn, C, seed=i, offset=offset, device=CPU)
            rs, rq = R.colsum(x)
            rt.add(f"colsum R={Rn} C={C} offset={offset} sum", x.double().sum(0).float(), rs)
            rt.add(f"colsum R={Rn} C={C} offset={offset} sumsq", (x.double() ** 2).sum(0).float(), rq)
    for case in G.BN_FWD:
        Rn, C, groups, act, running, offset = case
        z = G.data(Rn, C, seed=Rn + C, offset=offset, groups=groups, device=CPU)
        gamma, beta = G._affine(C, seed=C, device=CPU)
        st = R.bn_stats(z, groups, 1e-5)
        mean, invstd = one_pass_stats(z, groups, 1e-5)
        rt.add(f"bn_train_fwd {case} save_mean", mean.float(), st["save_mean"])
        rt.add(f"bn_train_fwd {case} save_invstd", invstd.float(), st["save_invstd"])
        rt.add(f"bn_train_fwd {case} a", emu_bn_apply(z, mean.float(), invstd.float(), gamma, beta, act, groups),
               R.bn_apply(z, st["mean"], st["invstd"], gamma, beta, act))
        r0 = (G.rnd(C, seed=C + 5, scale=0.2, device=CPU), G.rnd(C, seed=C + 6, scale=0.1, device=CPU).abs() + 0.5)
        rm, rv = emu_running(st, r0[0], r0[1], 0.1)
        r_m, r_v = R.bn_running(st, r0[0], r0[1], 0.1)
        rt.add(f"bn_train_fwd {case} running_mean", rm, r_m)
        rt.add(f"bn_train_fwd {case} running_var", rv, r_v)
    for i, (Rn, C) in enumerate(G.BN_EVAL):
        z = G.data(Rn, C, seed=i, offset=False, device=CPU)
        gamma, beta = G._affine(C, seed=i, device=CPU)
        rm, rv = G.rnd(C, seed=i + 7, scale=0.4, device=CPU), G.rnd(C, seed=i + 8, scale=0.2, device=CPU).abs() + 0.05
        for act in G.ALL_ACTS:
            got = torch_act(act, (z - rm) / torch.sqrt(rv + 1e-5) * gamma + beta)
            rt.add(f"bn_eval_fwd R={Rn} C={C} act={act}", got, R.bn_eval(z, gamma, beta, rm, rv, 1e-5, act))
        cb = G.rnd(C, seed=i + 9, device=CPU)
        s = gamma / torch.sqrt(rv + 1e-5)
        rs, rh = R.bn_fold(gamma, beta, rm, rv, cb, 1e-5)
        rt.add(f"bn_fold C={C} scale", s, rs)
        rt.add(f"bn_fold C={C} shift", beta + (cb - rm) * s, rh)
    for case in G.BN_PARTS:
        np_, groups, Rn, C, empties, offset, act = case
        z, part, st = G.parts_problem(case, device=CPU)
        gamma, beta = G._affine(C, seed=C, device=CPU)
        # the kernel's formulation of the combine, in fp64: M2 = sum Q + (sum S^2 / n - (sum S)^2 / N)
        p = part.double().view(groups, np_, 3, C)
        live = (p[:, :, 2] > 0).double()
        S, Q, n = p[:, :, 0] * live, p[:, :, 1] * live, p[:, :, 2]
        N = n.sum(1)
        mean = S.sum(1) / N
        m2 = Q.sum(1) + ((S * S / n.clamp_min(1.0)).sum(1) - S.sum(1) * mean)
        invstd = (m2.clamp_min(0.0) / N + R.f32(1e-5)) ** -0.5
        rt.add(f"bn_train_fwd_parts {case} save_mean", mean.float(), st["save_mean"])
        rt.add(f"bn_train_fwd_parts {case} save_invstd", invstd.float(), st["save_invstd"])
        rt.add(f"bn_train_fwd_parts {case} a", emu_bn_apply(z, mean.float(), invstd.float(), gamma, beta, act, groups),
               R.bn_apply(z, st["mean"], st["invstd"], gamma, beta, act))
    rt.finish(capsys, "(b) fp32 emulation / bound: colsum and BatchNorm forward")


def emu_bn_bwd(da, a, z, gamma, beta, mean, invstd, act):
    xh = (z.double() - mean.double()) * invstd.double()
    ref = (xh * gamma.double() + beta.double()).float() if act == GELU else a
    fac = R.act_grad_ref(act, ref.float()).float()
    dy = (da * fac).double()
    s1, s2 = dy.sum(0), (dy * xh).sum(0)
    n = z.shape[0]
    dz = (gamma.double() * invstd.double() * (dy - s1 / n - xh * s2 / n)).float()
    return dz, s2.float(), s1.float()


def test_fp32_batchnorm_backward_passes_the_bound(capsys):
    rt = Ratios()
    for act in G.BWD_ACTS:
        for i, (Rn, C) in enumerate(G.RC_PAIRS):
            args = G.bwd_problem(Rn, C, act, seed=i, offset=bool(i % 2), device=CPU)
            z, da, a, gamma, beta, mean, invstd = args
            for nm, got, ref in zip(("dz", "dgamma", "dbeta"), emu_bn_bwd(da, a, z, gamma, beta, mean, invstd, act),
                                    R.bn_bwd(da, a, z, gamma, beta, mean, invstd, act)):
                rt.add(f"bn_train_bwd R={Rn} C={C} act={act} {nm}", got, ref)
    rt.finish(capsys, "(b) fp32 emulation / bound: BatchNorm backward")


def test_fp32_reductions_head_and_losses_pass_the_bound(capsys):
    rt = Ratios()
    for i, (B, T, C) in enumerate(G.MEANT):
        a = G.rnd(B, T, C, seed=i, shift=0.5, device=CPU)
        rt.add(f"meanT_fwd B={B} T={T} C={C}", a.sum(1) / T, R.meanT_fwd(a))
        dh, gref, gs = G.rnd(B, C, seed=i, device=CPU), G.rnd(B, T, C, seed=i + 1, scale=0.8, device=CPU), G.rnd(C, seed=i + 2, shift=1.0, device=CPU)
        for gact in G.ALL_ACTS:
            got = (dh * (1.0 / T))[:, None, :] * R.act_grad_ref(gact, gref) * gs
            rt.add(f"meanT_bwd B={B} T={T} C={C} gact={gact}", got, R.meanT_bwd(dh, T, gref, gact, gs))
    for n in G.MEAN_N:
        src = G.rnd(n, seed=n, shift=0.3, device=CPU)
        rt.add(f"mean_scaled n={n}", (-1.5 * src.sum() / n).reshape(1), R.mean_scaled(src, -1.5))
    for i, (B, D) in enumerate(G.LAYERNORM):
        x = G.rnd(B, D, seed=i, scale=1.5, shift=0.7, device=CPU)
        gamma, beta = G._affine(D, seed=i, device=CPU)
        ry, rx = R.layernorm_fwd(x, gamma, beta, 1e-5)
        rt.add(f"layernorm_fwd B={B} D={D} y", F.layer_norm(x, (D,), gamma, beta, 1e-5), ry)
        rt.add(f"layernorm_fwd B={B} D={D} xhat", F.layer_norm(x, (D,), None, None, 1e-5), rx)
        dy, xh = G.rnd(B, D, seed=i + 3, device=CPU), G.rnd(B, D, seed=i + 4, device=CPU)
        rg, rb = R.layernorm_bwd_params(dy, xh)
        rt.add(f"layernorm_bwd_params B={B} D={D} dgamma", (dy * xh).sum(0), rg)
        rt.add(f"layernorm_bwd_params B={B} D={D} dbeta", dy.sum(0), rb)
    for i, (B, Be, Fd, E) in enumerate(G.DHEAD):
        f, wt, bias, ds = (G.rnd(*s, seed=i + j, device=CPU) for j, s in enumerate(((B, Fd), (Fd + E,), (1,), (B,))))
        emb = G.rnd(Be, E, seed=i + 4, device=CPU) if E else None
        full = torch.cat([f, emb.repeat(B // Be, 1)], 1) if E else f
        rt.add(f"dhead_fwd {G.DHEAD[i]}", full @ wt + bias, R.dhead_fwd(f, emb, wt, bias))
        refs = R.dhead_bwd(ds, f, wt, Be, E, Be)
        rt.add(f"dhead_bwd {G.DHEAD[i]} dU", ds[:, None] * wt[None, :Fd] * torch.where(f > 0, 1.0, 0.2), refs[0])
        if E:
            rt.add(f"dhead_bwd {G.DHEAD[i]} demb", ds[:Be, None] * wt[None, Fd:], refs[1])
        nb = max(n for n in G.DHEAD_NB if n <= B)
        gf = G.rnd(3, Fd, seed=i, device=CPU)
        rf, re_, rb = R.dhead_wgrad(ds, f, emb, gf, nb, 3)
        rt.add(f"dhead_wgrad {G.DHEAD[i]} nb={nb} dw[:F]", ds[:nb] @ f[:nb] + gf.sum(0), rf)
        if E:
            rt.add(f"dhead_wgrad {G.DHEAD[i]} nb={nb} dw[F:]", ds[:nb] @ full[:nb, Fd:], re_)
        rt.add(f"dhead_wgrad {G.DHEAD[i]} nb={nb} dbias", ds[:nb].sum().reshape(1), rb)
    for nbl in G.DHEAD_NB_LOSS:
        s, norms = G.rnd(2 * nbl, seed=nbl, shift=0.2, device=CPU), G.rnd(nbl, seed=nbl + 1, scale=0.3, shift=1.0, device=CPU).abs()
        mr, mf, pen = s[:nbl].mean(), s[nbl:].mean(), ((norms - 1) ** 2).mean()
        for nm, got, ref in zip(("loss_d", "mean_real", "mean_fake", "gp"), (mf - mr + 10.0 * pen, mr, mf, pen), R.wgan_d_loss(s, norms, 10.0, nbl)):
            rt.add(f"wgan_d_loss nb_loss={nbl} {nm}", got.reshape(1), ref)
    real, fake = G.rnd(5, 37, 3, seed=1, device=CPU), G.rnd(5, 37, 3, seed=2, device=CPU)
    alpha = torch.tensor([0.0, 1.0, 0.3, 0.7, 0.5])
    rt.add("gp_interp", alpha[:, None, None] * real + (1 - alpha[:, None, None]) * fake, R.gp_interp(real, fake, alpha))
    for i, (B, n, off, _, _) in enumerate(G.GP_PENALTY):
        g = G.gp_problem(B, n, seed=i, device=CPU)
        nrm = (g * g).sum(1).sqrt()
        fac = torch.where(nrm > 0, 10.0 * (2.0 / B) * (nrm - 1) / nrm.clamp_min(1e-30), torch.zeros_like(nrm))
        rn, rg, rp = R.gp_penalty(g, 10.0)
        rt.add(f"gp_penalty B={B} n={n} norms", nrm, rn)
        rt.add(f"gp_penalty B={B} n={n} gbar", fac[:, None] * g, rg)
        rt.add(f"gp_penalty B={B} n={n} gp", ((nrm - 1) ** 2).mean().reshape(1), rp)
    for i, (B, C) in enumerate(G.SOFTMAX_CE):
        for scale in (1.0, 30.0):
            z, y = G.ce_problem(B, C, i, scale, device=CPU)
            zz = z.clone().requires_grad_(True)
            loss = F.cross_entropy(zz, y)
            (0.7 * loss).backward()
            rl, rd, _ = R.softmax_ce(z, y, 0.7)
            rt.add(f"softmax_ce B={B} C={C} scale={scale} loss", loss.detach().reshape(1), rl)
            rt.add(f"softmax_ce B={B} C={C} scale={scale} dlogits", zz.grad, rd)
    rt.finish(capsys, "(b) fp32 torch / bound: reductions, LayerNorm, the critic head, WGAN-GP, losses")


def emu_adam(p, g, m, v, step, lr, b1, b2, eps, wd, gs):
    """adam_step in fp32 arithmetic (the bias corrections in fp64, rounded once)."""
    f = torch.float32
    lr_, b1_, b2_, eps_, wd_ = (torch.tensor(t, dtype=f) for t in (lr, b1, b2, eps, wd))
    bc1, bc2 = 1.0 - R.f32(b1) ** step, 1.0 - R.f32(b2) ** step
    ss, bs = torch.tensor(R.f32(lr) / bc1, dtype=f), torch.tensor(math.sqrt(bc2), dtype=f)
    gi = g * torch.tensor(gs, dtype=f)
    pi = p * (1 - lr_ * wd_) if wd else p
    mi = m + (gi - m) * (1 - b1_)
    vi = v * b2_ + (1 - b2_) * gi * gi
    return pi - ss * (mi / (vi.sqrt() / bs + eps_)), mi, vi


def test_fp32_optimiser_and_vae_pass_the_bound(capsys):
    rt = Ratios()
    for i, n in enumerate(G.ADAM_N):
        for wd in (0.0, 0.01):
            p0, g, m0, v0, _ = G.adam_problem(n, seed=i, device=CPU)
            got = emu_adam(p0, g, m0, v0, 8, wd=wd, gs=0.5 * 0.7, b1=G.ADAM_HP["beta1"], b2=G.ADAM_HP["beta2"], lr=G.ADAM_HP["lr"], eps=G.ADAM_HP["eps"])
            refs = R.adam_step(p0, g, m0, v0, 8, weight_decay=wd, grad_scale=0.5, gs_dev=torch.tensor([0.7]), **G.ADAM_HP)
            for nm, a, b in zip("pmv", got, refs):
                rt.add(f"adam_flat n={n} wd={wd} {nm}", a, b)
    for i, n in enumerate(G.GRAD_NORM_N):
        g = G.rnd(n, seed=i, scale=1.0 / n ** 0.5, device=CPU)
        for mx in (0.25, 4.0):
            nrm = (g * g).sum().sqrt()
            got = torch.stack([nrm, torch.clamp(torch.tensor(mx) / (nrm + 1e-6), max=1.0)])
            rt.add(f"grad_norm_clip n={n} max_norm={mx}", got, R.grad_norm_clip(g, mx))
    for n in (1, 255, 257, 2048):
        mu, lv, eps, dz = (G.rnd(n, seed=n + j, scale=(0.7 if j == 1 else 1.0), device=CPU) for j in range(4))
        rt.add(f"reparam_fwd n={n}", mu + eps * torch.exp(0.5 * lv), R.reparam_fwd(mu, lv, eps))
        rm, rl = R.reparam_bwd(dz, lv, eps, mu * 0.01, lv * 0.01)
        rt.add(f"reparam_bwd n={n} dmu", dz + mu * 0.01, rm)
        rt.add(f"reparam_bwd n={n} dlv", dz * eps * 0.5 * torch.exp(0.5 * lv) + lv * 0.01, rl)
    for i, (nx, nz) in enumerate(G.VAE):
        recon, x, mu, lv = G.vae_problem(nx, nz, seed=i, device=CPU)
        (rt_, rmse, rk), rdr, rdm, rdl = R.vae_loss(recon, x, mu, lv, 0.3)
        df, e = recon - x, torch.exp(lv)
        mse, kld = (df * df).mean(), -0.5 * (1 + lv - mu * mu - e).mean()
        for nm, got, ref in (("total", mse + 0.3 * kld, rt_), ("mse", mse, rmse), ("kld", kld, rk)):
            rt.add(f"vae_loss n_x={nx} n_z={nz} {nm}", got.reshape(1), ref)
        rt.add(f"vae_loss n_x={nx} n_z={nz} drecon", (2.0 / nx) * df, rdr)
        rt.add(f"vae_loss n_x={nx} n_z={nz} dmu", 0.3 * mu / nz, rdm)
        rt.add(f"vae_loss n_x={nx} n_z={nz} dlv", 0.3 * -0.5 * (1 - e) / nz, rdl)
    rt.finish(capsys, "(b) fp32 torch / bound: Adam, the gradient-norm clip, the VAE pieces")


# ---------------------------------------------------------------------------------------------------------------------
# (c) plausible mistakes leave the bound
# ---------------------------------------------------------------------------------------------------------------------
def test_subtle_errors_are_flagged(capsys):
    """Each mistake is built from the fp64 reference at a shape of the GPU file's tables and rounded to fp32; its worst
    error / bound ratio must exceed 1.  Measured (the same figures are in DESIGN.md):
    running_var from the biased variance 2.3 (R = 65, offset data) / 193 (R = 8193); save_invstd from the unbiased variance
    9024 (R = 65) / 49 (R = 1000, offset data) / 205 (R = 8193); fp32 E[x^2] - mean^2 on offset data 2.4e5; momentum on the
    wrong operand 1.2e7; running statistics from group 0 only 4.3e4, group 1 normalised with group 0's statistics 6.5e4; the
    last row dropped 1.4e5 (R = 65) / 773 (R = 16385), the last row slice 1.0e6 / 1830; fp32 accumulation at R = 16385 5.7;
    channels 4-5 of C = 6 skipped 6.0e5; an unwritten ragged tail inf (NaN prefill); a zero-count partial row counted 6.7e31,
    M2 without the between-chunk term 3.7e4; GELU' at the activation 5.6e5 (dz) / 3.2e4 (dbeta); LeakyReLU slope 0.01 1.6e6 /
    6.0e4; 1 / (T + 1) 9290 (meanT_bwd) / 126 (meanT_fwd); gscale indexed by row 2.2e8; gp factor without 2 / B 5200; KLD sign
    4.4e4, its 0.5 lost 2.2e4, in dlv 1.6e6; Adam bias correction one step late 632, coupled weight decay 413; the clip
    coefficient applied below max_norm 3058; the WQ scatter with c and n swapped: 110 of 120 elements differ.
    The biased / unbiased mix-up in running_var is NOT visible on the offset data at R = 1000 (ratio 0.25): the batch
    variance is 1e-4 of the running value there; it is on the data whose variance is O(1)."""
    rows = []

    def flag(what, got, ref):
        r = ratio(got.float(), ref)
        rows.append((r, what))

    # --- BatchNorm forward at (R = 4096 is not in the tables: the smallest table shapes are used instead)
    case = (65, 68, 2, RELU, True, True)                    # BN_FWD: offset data, two groups
    assert case in G.BN_FWD
    Rn, C, groups = case[:3]
    z = G.data(Rn, C, seed=Rn + C, offset=True, groups=groups, device=CPU)
    gamma, beta = G._affine(C, seed=C, device=CPU)
    st = R.bn_stats(z, groups, 1e-5)
    r0 = (G.rnd(C, seed=C + 5, scale=0.2, device=CPU), G.rnd(C, seed=C + 6, scale=0.1, device=CPU).abs() + 0.5)
    r_m, r_v = R.bn_running(st, r0[0], r0[1], 0.1)
    biased = dict(st, unb=st["var"])
    flag("running_var from the biased variance (R = 65, offset data)", R.bn_running(biased, *r0, 0.1)[1].val, r_v)
    flag("save_invstd from the unbiased variance (R = 65, offset data)", (st["unb"] + 1e-5) ** -0.5, st["save_invstd"])
    big = (1000, 64, 1, GELU, True, True)
    assert big in G.BN_FWD
    zb = G.data(1000, 64, seed=1064, offset=True, device=CPU)
    stb = R.bn_stats(zb, 1, 1e-5)
    r0b = (G.rnd(64, seed=69, scale=0.2, device=CPU), G.rnd(64, seed=70, scale=0.1, device=CPU).abs() + 0.5)
    wide = (8193, 64, 1, LRELU, True, False)
    assert wide in G.BN_FWD
    stw = R.bn_stats(G.data(8193, 64, seed=8193 + 64, offset=False, device=CPU), 1, 1e-5)
    flag("running_var from the biased variance (R = 8193)", R.bn_running(dict(stw, unb=stw["var"]), *r0b, 0.1)[1].val, R.bn_running(stw, *r0b, 0.1)[1])
    flag("save_invstd from the unbiased variance (R = 8193)", (stw["unb"] + 1e-5) ** -0.5, stw["save_invstd"])
    flag("save_invstd from the unbiased variance (R = 1000, offset data)", (stb["unb"] + 1e-5) ** -0.5, stb["save_invstd"])
    x32 = zb.float()
    var32 = ((x32 * x32).mean(0) - x32.mean(0) ** 2).clamp_min(0.0)            # fp32 E[x^2] - mean^2
    flag("variance as fp32 E[x^2] - mean^2 (R = 1000, offset data): save_invstd", ((var32 + 1e-5) ** -0.5)[None], stb["save_invstd"])
    wrong = 0.1 * r0[0].double() + 0.9 * st["mean"][0]
    wrong = 0.1 * wrong + 0.9 * st["mean"][1]
    flag("momentum applied to the wrong operand: running_mean", wrong, r_m)
    g0 = dict(st, mean=st["mean"][[0, 0]], unb=st["unb"][[0, 0]])
    flag("groups' running statistics from group 0 only: running_mean", R.bn_running(g0, *r0, 0.1)[0].val, r_m)
    flag("the second group normalised with group 0's statistics: a", R.bn_apply(z, st["mean"][[0, 0]], st["invstd"][[0, 0]], gamma, beta, RELU).val,
         R.bn_apply(z, st["mean"], st["invstd"], gamma, beta, RELU))
    # --- dropped rows and channels
    for (Rn, C) in ((65, 65), (16385, 68)):
        assert (Rn, C) in G.RC_PAIRS
        x = G.data(Rn, C, seed=3, offset=False, device=CPU)
        rs, rq = R.colsum(x)
        flag(f"colsum: the last row dropped (R = {Rn})", x[:-1].double().sum(0), rs)
        last = Rn - red_plan(Rn)[1] * (red_plan(Rn)[0] - 1)
        flag(f"colsum: the last row slice ({last} rows) dropped (R = {Rn})", x[:-last].double().sum(0), rs)
        s1 = R.bn_stats(x, 1, 1e-5)
        flag(f"bn_train_fwd: save_mean without the last row (R = {Rn})", x[:-1].double().mean(0)[None], s1["save_mean"])
    x = G.data(16385, 68, seed=3, offset=True, device=CPU)
    acc = torch.zeros(68)
    for row in x:                                           # fp32 all the way: every addition rounds
        acc = acc + row
    flag("colsum: fp32 accumulation, one running sum per channel (R = 16385, offset data)", acc, R.colsum(x)[0])
    x = G.data(17, 6, seed=3, offset=False, device=CPU)
    got = x.double().sum(0)
    got[4:] = 0.0
    flag("colsum: channels 4-5 of C = 6 skipped", got, R.colsum(x)[0])
    x = G.data(1000, 68, seed=7, offset=False, device=CPU)
    gamma, beta = G._affine(68, seed=68, device=CPU)
    s1 = R.bn_stats(x, 1, 1e-5)
    ref = R.bn_apply(x, s1["mean"], s1["invstd"], gamma, beta, NONE)
    got = ref.val.clone()
    got[:, 64:] = float("nan")
    flag("bn apply: the last 4 channels of C = 68 left unwritten (NaN prefill)", got, ref)
    # --- a zero-count partial row counted in the combine
    case = G.BN_PARTS[2]
    _, part, stp = G.parts_problem(case, device=CPU)
    p = part.double()
    S, n = p[:, 0].clone(), p[:, 2]
    S[n[:, 0] == 0] = 1e30
    flag("combine: a zero-count partial row's sum counted: save_mean", (S.sum(0) / n.sum(0))[None], stp["save_mean"])
    flag("combine: M2 without the between-chunk term: save_invstd", ((p[n[:, 0] > 0, 1].sum(0) / n.sum(0) + 1e-5) ** -0.5)[None], stp["save_invstd"])
    # --- BatchNorm backward
    Rn, C = 1000, 68
    for act, what, f in ((GELU, "GELU' taken at the activation instead of the BN output", None),
                         (LRELU, "LeakyReLU slope 0.01 instead of 0.2", 0.01)):
        z, da, a, gamma, beta, mean, invstd = G.bwd_problem(Rn, C, act, seed=7, offset=False, device=CPU)
        rz, rg, rb = R.bn_bwd(da, a, z, gamma, beta, mean, invstd, act)
        xh = (z.double() - mean.double()) * invstd.double()
        fac = R.act_grad_ref(GELU, a.double()) if f is None else torch.where(a > 0, 1.0, f).double()
        dy = da.double() * fac
        s1_, s2_ = dy.sum(0), (dy * xh).sum(0)
        flag(f"bn_train_bwd: {what}: dz", gamma.double() * invstd.double() * (dy - s1_ / Rn - xh * s2_ / Rn), rz)
        flag(f"bn_train_bwd: {what}: dbeta", s1_, rb)
    # --- mean over time
    B, T, C = 2, 300, 130
    assert (B, T, C) in G.MEANT
    dh, gs = G.rnd(B, C, seed=5, device=CPU), G.rnd(C, seed=7, shift=1.0, device=CPU)
    flag("meanT_bwd: 1 / T as 1 / (T + 1) (T = 300)", (dh.double() / (T + 1))[:, None, :].expand(B, T, C), R.meanT_bwd(dh, T))
    flag("meanT_fwd: 1 / T as 1 / (T + 1) (T = 300)", G.rnd(B, T, C, seed=5, shift=0.5, device=CPU).double().sum(1) / (T + 1),
         R.meanT_fwd(G.rnd(B, T, C, seed=5, shift=0.5, device=CPU)))
    rows_idx = (torch.arange(B * T) % C).view(B, T)
    flag("meanT_bwd: gscale indexed by row", (dh.double() / T)[:, None, :] * gs.double()[rows_idx][:, :, None].expand(B, T, C), R.meanT_bwd(dh, T, gscale=gs))
    # --- WGAN-GP, VAE
    g = G.gp_problem(6, 4100, seed=4, device=CPU)
    _, rg, _ = R.gp_penalty(g, 10.0)
    flag("gp_penalty: the factor without 2 / B", rg.val * 6 / 2, rg)
    recon, x, mu, lv = G.vae_problem(6, 255, seed=1, device=CPU)
    (rt_, rmse, rk), rdr, rdm, rdl = R.vae_loss(recon, x, mu, lv, 0.3)
    got = rdr.val.clone()
    got[4:] = float("nan")
    flag("vae_loss: the n % 4 tail of drecon left unwritten (NaN prefill)", got, rdr)
    flag("vae_loss: the sign of the KLD", -rk.val, rk)
    flag("vae_loss: the 0.5 of the KLD lost", 2 * rk.val, rk)
    flag("vae_loss: the 0.5 lost in dlv", 2 * rdl.val, rdl)
    # --- Adam, the clip, the WQ scatter
    p0, gr, m0, v0, _ = G.adam_problem(257, seed=3, device=CPU)
    rp, _, _ = R.adam_step(p0, gr, m0, v0, 8, weight_decay=0.01, **G.ADAM_HP)
    flag("adam: bias correction one step late", R.adam_step(p0, gr, m0, v0, 7, weight_decay=0.01, **G.ADAM_HP)[0].val, rp)
    flag("adam: weight decay coupled instead of decoupled", R.adam_step(p0, gr, m0, v0, 8, weight_decay=0.01, decoupled=False, **G.ADAM_HP)[0].val, rp)
    gg = G.rnd(8193, seed=3, scale=1.0 / 8193 ** 0.5, device=CPU)
    ref = R.grad_norm_clip(gg, 4.0)
    flag("grad_norm_clip: the coefficient applied below max_norm", torch.stack([ref.val[0], 4.0 / (ref.val[0] + 1e-6)]), ref)
    N, Cc, K = G.WQ["N"], G.WQ["Cc"], G.WQ["K"]
    w = torch.randn(N * Cc * K, generator=torch.Generator().manual_seed(1))
    right = R.wq_layout(w, N, Cc, K, cnk=True)
    swapped = w.view(N, Cc, K).view(N, Cc // 4, 4, K).permute(1, 3, 0, 2).contiguous().view(-1)      # read as w[n][c][k]
    assert not torch.equal(right, swapped)
    rows.append((float("inf"), f"WQ scatter with c and n swapped in the w[c][n][k] layout: {int((right != swapped).sum())} of {right.numel()} elements differ (compared exactly)"))
    with capsys.disabled():
        print("\n[support ref] (c) mistake: worst error / bound")
        for r, what in rows:
            print(f"    {r:12.4g}  {what}")
    bad = [(r, what) for r, what in rows if not r > 1.0]
    assert not bad, bad
