"""The streaming kernels of csrc/small_kernels.hip -- column sums, BatchNorm, the mean over time, LayerNorm, the critic head,
the WGAN-GP pieces, the losses, the elementwise helpers, flat Adam, the gradient-norm clip and the VAE pieces -- pinned to
fp64, element by element (tests/support_ref.py: the references and the bounds).

Every output lives in a NaN-prefilled canvas between sentinel rows; every element and every sentinel is checked.  The
shape tables below are plain data: tests/test_support_ref.py sweeps them on the host with fp32 emulations, and recomputes
the launch plans (red_plan, bn_row_slices, the vector predicates) to show that they reach what this file claims: a second
round of the partial-combine loop (R = 8193, 16385; np = 129, 300), the RED_SPLITS clamp (R = 16385: 253 slices of 65
rows), a ragged last channel block with C % 4 == 0 (C = 68), the scalar paths (C % 4 != 0, n % 4 != 0, misaligned
tensors), n > 32768 in gp_penalty, the B > 256 loops and every rider.  Misaligned tensors (off4) go only to the entry
points that evaluate an alignment predicate themselves: meanT_fwd, meanT_bwd, gp_penalty, vae_loss.  The fp64 references
are evaluated on the device.

Each test prints the worst error / bound ratio of its section (pytest -s shows it).  Measured on an MI355X:
a. colsum 0.20; b. bn_train_fwd 0.34 (the apply pass under LeakyReLU, R = 8193; statistics and running statistics 0.14-0.28),
bn_eval_fwd / bn_fold 0.29; c. bn_train_fwd_parts 0.46 (the apply pass, np = 128, two groups; running_var 0.17-0.26); d.
bn_train_bwd 0.17 (ReLU), 0.14 (LeakyReLU), 0.33 (GELU), 0.16 (tanh), always dz at R = 8193; bn_train_bwd_parts 0.17; e.
meanT_fwd 0.15, meanT_bwd 0.55 (a GELU' gref, scalar kernel); f. layernorm 0.26; g. dhead_fwd / bwd / fwd_bwd 0.28, dhead_wgrad
and its loss rider 0.20; h. gp_interp 0.10, gp_penalty 0.10, softmax_ce 0.38 (dlogits, logits x 30), mean_scaled 0.002; i.
elementwise 0.50 (transpose with a GELU' gref); j. adam_flat 0.28, grad_norm_clip 0.013, reparam 0.20, vae_loss 0.28.  1032
bound checks besides the exact comparisons; the file takes about 5 s."""
import pytest
import torch

import support_ref as R

pytestmark = pytest.mark.gpu

NONE, RELU, LRELU, GELU, TANH = R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU, R.ACT_GELU, R.ACT_TANH
ALL_ACTS = (NONE, RELU, LRELU, GELU, TANH)

# ---------------------------------------------------------------------------------------------------------------------
# the tables (plain data; tests/test_support_ref.py imports them)
# ---------------------------------------------------------------------------------------------------------------------
# a./d. (rows, channels): every R of {1, 15, 16, 17, 63, 64, 65, 1000, 8193, 16385} and every C of {1, 3, 4, 6, 60, 64, 65,
# 68, 130, 256}; ragged C x clamped R twice (16385 x 130: C % 4 != 0; 16385 x 68: C % 4 == 0 with a ragged last block)
RC_PAIRS = [(1, 1), (15, 3), (16, 4), (17, 6), (63, 60), (64, 256), (65, 65), (1000, 68), (8193, 64), (16385, 130), (16385, 68)]
# b. (rows per group, C, groups, act, running statistics, offset data)
BN_FWD = [(1, 4, 1, NONE, True, False), (2, 4, 1, RELU, True, False), (1, 6, 2, LRELU, True, False),
          (37, 4, 1, GELU, False, False), (65, 6, 3, TANH, True, False), (65, 68, 2, RELU, True, True),
          (1000, 64, 1, GELU, True, True), (8193, 64, 1, LRELU, True, False), (16385, 68, 1, NONE, True, True),
          (16385, 130, 1, RELU, False, False), (64, 256, 2, TANH, True, False), (1000, 68, 3, GELU, True, True)]
BN_EVAL = [(5, 6), (37, 68), (65, 130)]                       # (R, C): ragged C
# c. (np, groups, rows per group, C, empty partial rows, offset data, act)
BN_PARTS = [(1, 1, 37, 4, (), False, RELU), (16, 2, 65, 6, (3,), True, LRELU), (17, 1, 1000, 68, (0, 16), True, RELU),
            (128, 2, 1000, 64, (5, 77), False, NONE), (129, 1, 16385, 68, (128,), True, RELU),
            (300, 2, 1000, 130, (0, 1, 299), True, LRELU)]
# d. (np, R, C) of bn_train_bwd_parts
BWD_PARTS = [(1, 37, 4), (16, 65, 6), (17, 1000, 68), (128, 1000, 64), (129, 16385, 68), (300, 1000, 130)]
BWD_ACTS = (RELU, LRELU, GELU, TANH)
# e. (B, T, C): T of {1, 15, 16, 17, 37, 300}, C of {4, 6, 64, 68, 96, 130}
MEANT = [(2, 1, 4), (3, 15, 6), (1, 16, 64), (2, 17, 68), (3, 37, 96), (2, 300, 130), (2, 300, 4), (1, 1, 130)]
MEAN_N = [1, 255, 256, 257, 1000]
# f. (B, D)
LAYERNORM = [(1, 1), (3, 6), (4, 63), (5, 64), (64, 6), (65, 63), (300, 6), (300, 64)]
# g. (B, Be, F, E)
DHEAD = [(1, 1, 1, 0), (6, 3, 63, 1), (65, 65, 64, 128), (192, 64, 65, 130), (6, 3, 256, 128), (192, 64, 256, 0)]
DHEAD_NB = [1, 63, 64, 65]
DHEAD_NB_LOSS = [1, 255, 257]
# h. (B, n, off4, gbar, gp): n of {1, 5, 4096, 4100, 32768, 32772, 40001}, B of {1, 6, 257}
GP_PENALTY = [(6, 1, False, True, True), (6, 5, False, True, False), (1, 4096, False, True, True), (6, 4096, True, True, True),
              (6, 4100, False, True, True), (6, 4100, False, False, True), (6, 32768, False, True, True),
              (6, 32772, False, True, True), (1, 40001, False, True, True), (257, 5, False, True, True),
              (257, 4096, False, True, True)]
SOFTMAX_CE = [(1, 1), (7, 4), (256, 32), (257, 5), (1000, 32)]
# i.
TRANSPOSE = [(1, 70), (31, 33), (32, 32), (33, 31), (70, 1), (70, 70)]        # (C, L)
# j.
ADAM_N = [1, 255, 256, 257, 4099]
WQ = dict(N=3, Cc=8, K=5, starts=(7, 200))          # one w[n][c][k] entry at 7, one w[c][n][k] entry at 200: 120 elements each
GRAD_NORM_N = [1, 8191, 8192, 8193, 1024 * 8 * 1024 + 5]
VAE = [(4, 1), (6, 255), (1023, 256), (1024, 257), (65536 + 4, 2048), (65536 + 6, 1)]       # (n_x, n_z)


@pytest.fixture(scope="module")
def ops():
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import ops as o
    return o


class Worst:
    """Keeps the worst error / bound ratio of a section and prints it when the test is over."""

    def __init__(self, section):
        self.section, self.r, self.what, self.n = section, 0.0, "", 0

    def check(self, got, ref, what):
        r = R.check(got, ref, what)
        self.n += 1
        if r >= self.r:
            self.r, self.what = r, what
        return r

    def report(self, capsys):
        with capsys.disabled():
            print(f"\n[support contract] {self.section}: {self.n} checks, worst error / bound = {self.r:.4f} ({self.what})")


def rnd(*shape, seed=0, scale=1.0, shift=0.0, device="cuda"):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift).to(device)


def data(Rn, C, seed, offset, groups=1, device="cuda"):
    """BatchNorm input (groups * Rn, C): offset data is 100 + 0.01 randn (where E[x^2] - mean^2 in fp32 has no digits left),
    otherwise 0.3 + 2 randn; group g is shifted by 3 g more, so that the wrong group's statistics are visible."""
    base, std = (100.0, 0.01) if offset else (0.3, 2.0)
    z = torch.randn(groups, Rn, C, generator=torch.Generator().manual_seed(seed)) * std + base
    z += 3.0 * torch.arange(groups).view(-1, 1, 1)
    return z.view(groups * Rn, C).float().to(device)


def off4(t):
    """A contiguous copy of t that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


class Out(R.Guarded):
    """stride2_ref.Guarded (NaN-prefilled output between sentinel rows), optionally 4 bytes past a 16-byte boundary, or
    prefilled with `init` for in/out tensors."""

    def __init__(self, shape, off=False, init=None, dtype=torch.float32, rows=64):
        shape = tuple(shape)
        n = 1
        for s in shape:
            n *= s
        self.pad = min(rows * shape[-1], 16384)
        buf = torch.full((n + 2 * self.pad + 4,), self.SENTINEL, device="cuda", dtype=dtype)
        self.canvas = buf[1:1 + n + 2 * self.pad] if off else buf[:n + 2 * self.pad]
        self.t = self.canvas[self.pad:self.pad + n].view(*shape)
        assert self.t.data_ptr() % 16 == (4 if off else 0)
        if init is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(init)


def exact(got, want, what):
    assert got.shape == want.shape, what
    assert torch.equal(got, want), f"{what}: {int((got != want).sum())} element(s) differ from the exact result"


# ---------------------------------------------------------------------------------------------------------------------
# a. colsum
# ---------------------------------------------------------------------------------------------------------------------
def test_colsum(ops, capsys):
    w = Worst("a. colsum")
    for i, (Rn, C) in enumerate(RC_PAIRS):
        for offset in (False, True):
            x = data(Rn, C, seed=i, offset=offset)
            rs, rq = R.colsum(x)
            what = f"colsum R={Rn} C={C} offset={offset}"
            o1, o2 = Out((C,)), Out((C,))
            ops.colsum(x, o1.t, o2.t)
            w.check(o1.t, rs, what + " sum")
            w.check(o2.t, rq, what + " sumsq")
            o3 = Out((C,))
            ops.colsum(x, o3.t)
            w.check(o3.t, rs, what + " sum (no sumsq)")
            for o in (o1, o2, o3):
                o.check(what)
    w.report(capsys)


# ---------------------------------------------------------------------------------------------------------------------
# b. bn_train_fwd, bn_eval_fwd, bn_fold
# ---------------------------------------------------------------------------------------------------------------------
def _affine(C, seed, device="cuda"):
    return rnd(C, seed=seed, scale=0.5, shift=1.0, device=device), rnd(C, seed=seed + 1, scale=0.3, device=device)


def _check_bn_fwd(w, what, st, z, gamma, beta, act, groups, run0, outs):
    a, sm, si, rm, rv = outs
    C = z.shape[1]
    w.check(sm.t.view(groups, C), st["save_mean"], what + " save_mean")
    w.check(si.t.view(groups, C), st["save_invstd"], what + " save_invstd")
    w.check(a.t, R.bn_apply(z, st["mean"], st["invstd"], gamma, beta, act), what + " a")
    if rm is not None:
        r_m, r_v = R.bn_running(st, run0[0], run0[1], 0.1)
        w.check(rm.t, r_m, what + " running_mean")
        w.check(rv.t, r_v, what + " running_var")
    for o in outs:
        if o is not None:
            o.check(what)


def _bn_outs(z, C, groups, running, seed):
    sshape = (C,) if groups == 1 else (groups, C)
    run0 = (rnd(C, seed=seed + 5, scale=0.2), rnd(C, seed=seed + 6, scale=0.1).abs() + 0.5)
    rm = Out((C,), init=run0[0]) if running else None
    rv = Out((C,), init=run0[1]) if running else None
    return run0, (Out(z.shape), Out(sshape), Out(sshape), rm, rv)


@pytest.mark.parametrize("case", BN_FWD, ids=[f"R{c[0]}-C{c[1]}-g{c[2]}-act{c[3]}" for c in BN_FWD])
def test_bn_train_fwd(ops, capsys, case):
    Rn, C, groups, act, running, offset = case
    w = Worst(f"b. bn_train_fwd {case}")
    z = data(Rn, C, seed=Rn + C, offset=offset, groups=groups)
    gamma, beta = _affine(C, seed=C)
    run0, outs = _bn_outs(z, C, groups, running, seed=C)
    a, sm, si, rm, rv = outs
    ops.bn_train_fwd(z, a.t, gamma, beta, rm.t if running else None, rv.t if running else None, sm.t, si.t, act=act,
                     momentum=0.1, eps=1e-5, groups=groups)
    _check_bn_fwd(w, f"bn_train_fwd {case}", R.bn_stats(z, groups, 1e-5), z, gamma, beta, act, groups, run0, outs)
    w.report(capsys)


def test_bn_eval_and_fold(ops, capsys):
    w = Worst("b. bn_eval_fwd / bn_fold")
    for i, (Rn, C) in enumerate(BN_EVAL):
        z = data(Rn, C, seed=i, offset=False)
        gamma, beta = _affine(C, seed=i)
        rm, rv = rnd(C, seed=i + 7, scale=0.4), rnd(C, seed=i + 8, scale=0.2).abs() + 0.05
        for act in ALL_ACTS:
            a = Out((Rn, C))
            ops.bn_eval_fwd(z, a.t, gamma, beta, rm, rv, act=act, eps=1e-5)
            w.check(a.t, R.bn_eval(z, gamma, beta, rm, rv, 1e-5, act), f"bn_eval_fwd R={Rn} C={C} act={act}")
            a.check("bn_eval_fwd")
        for cb in (None, rnd(C, seed=i + 9)):
            sc, sh = Out((C,)), Out((C,))
            ops.bn_fold(gamma, beta, rm, rv, cb, sc.t, sh.t, eps=1e-5)
            rs, rh = R.bn_fold(gamma, beta, rm, rv, cb, 1e-5)
            w.check(sc.t, rs, f"bn_fold C={C} scale")
            w.check(sh.t, rh, f"bn_fold C={C} shift bias={cb is not None}")
            sc.check("bn_fold"), sh.check("bn_fold")
    w.report(capsys)


# ---------------------------------------------------------------------------------------------------------------------
# c. bn_train_fwd_parts on host-built partials
# ---------------------------------------------------------------------------------------------------------------------
def parts_problem(case, device="cuda"):
    """z (groups * Rn, C), the (groups * np, 3, C) fp32 partials and the statistics a correct combine derives from them."""
    np_, groups, Rn, C, empties, offset, act = case
    z = data(Rn, C, seed=np_ + C, offset=offset, groups=groups, device=device)
    parts, sts = [], []
    for g in range(groups):
        p, _ = R.conv16_parts(z[g * Rn:(g + 1) * Rn], np_, empties, seed=g)
        parts.append(p)
        sts.append(R.parts_stats(p, 1e-5))
    return z, torch.cat(parts).contiguous(), R.cat_stats(sts)


@pytest.mark.parametrize("case", BN_PARTS, ids=[f"np{c[0]}-g{c[1]}-R{c[2]}-C{c[3]}" for c in BN_PARTS])
def test_bn_train_fwd_parts(ops, capsys, case):
    np_, groups, Rn, C, empties, offset, act = case
    w = Worst(f"c. bn_train_fwd_parts {case}")
    z, part, st = parts_problem(case)
    gamma, beta = _affine(C, seed=C)
    run0, outs = _bn_outs(z, C, groups, True, seed=C)
    a, sm, si, rm, rv = outs
    ops.bn_train_fwd_parts(part, groups * np_, groups, z, a.t, gamma, beta, rm.t, rv.t, sm.t, si.t, act=act, momentum=0.1, eps=1e-5)
    _check_bn_fwd(w, f"bn_train_fwd_parts {case}", st, z, gamma, beta, act, groups, run0, outs)
    w.report(capsys)


# ---------------------------------------------------------------------------------------------------------------------
# d. bn_train_bwd, bn_train_bwd_parts
# ---------------------------------------------------------------------------------------------------------------------
def bwd_problem(Rn, C, act, seed, offset, device="cuda"):
    """The inputs of a BatchNorm backward: z, da, the affine pair, the SAVED fp32 statistics and activation of a forward."""
    z = data(Rn, C, seed=seed, offset=offset, device=device)
    gamma, beta = _affine(C, seed + 11, device)
    st = R.bn_stats(z, 1, 1e-5)
    mean, invstd = st["mean"][0].float(), st["invstd"][0].float()
    a = R.bn_apply(z, mean[None], invstd[None], gamma, beta, act).val.float()
    da = (torch.randn(Rn, C, generator=torch.Generator().manual_seed(seed + 3))).to(device)
    return z, da, a, gamma, beta, mean, invstd


@pytest.mark.parametrize("act", BWD_ACTS)
def test_bn_train_bwd(ops, capsys, act):
    w = Worst(f"d. bn_train_bwd act={act}")
    for i, (Rn, C) in enumerate(RC_PAIRS):
        z, da, a, gamma, beta, mean, invstd = bwd_problem(Rn, C, act, seed=i, offset=bool(i % 2))
        dz, dg, db = Out((Rn, C)), Out((C,)), Out((C,))
        ops.bn_train_bwd(da, a, z, dz.t, gamma, mean, invstd, dg.t, db.t, act=act, beta=beta if act == GELU else None)
        rz, rg, rb = R.bn_bwd(da, a, z, gamma, beta, mean, invstd, act)
        what = f"bn_train_bwd R={Rn} C={C} act={act}"
        w.check(dz.t, rz, what + " dz")
        w.check(dg.t, rg, what + " dgamma")
        w.check(db.t, rb, what + " dbeta")
        for o in (dz, dg, db):
            o.check(what)
    w.report(capsys)


@pytest.mark.parametrize("act", (RELU, LRELU))
def test_bn_train_bwd_parts(ops, capsys, act):
    w = Worst(f"d. bn_train_bwd_parts act={act}")
    for i, (np_, Rn, C) in enumerate(BWD_PARTS):
        z, da, a, gamma, beta, mean, invstd = bwd_problem(Rn, C, act, seed=20 + i, offset=bool(i % 2))
        part = R.bwd_parts(da, a, z, mean, invstd, act, np_, seed=i).contiguous()
        dz, dg, db = Out((Rn, C)), Out((C,)), Out((C,))
        ops.bn_train_bwd_parts(part, np_, da, a, z, dz.t, gamma, mean, invstd, dg.t, db.t, act=act)
        rz, rg, rb = R.bn_bwd(da, a, z, gamma, beta, mean, invstd, act)
        what = f"bn_train_bwd_parts np={np_} R={Rn} C={C} act={act}"
        w.check(dz.t, rz, what + " dz")
        w.check(dg.t, rg, what + " dgamma")
        w.check(db.t, rb, what + " dbeta")
        for o in (dz, dg, db):
            o.check(what)
    w.report(capsys)


# ---------------------------------------------------------------------------------------------------------------------
# e. meanT_fwd / meanT_bwd
# ---------------------------------------------------------------------------------------------------------------------
def test_meanT_fwd(ops, capsys):
    w = Worst("e. meanT_fwd")
    for i, (B, T, C) in enumerate(MEANT):
        a = rnd(B, T, C, seed=i, shift=0.5)
        ref = R.meanT_fwd(a)
        for off in (False, True):
            h = Out((B, C))
            ops.meanT_fwd(off4(a) if off else a, h.t)
            w.check(h.t, ref, f"meanT_fwd B={B} T={T} C={C} off4={off}")
            h.check("meanT_fwd")
    w.report(capsys)


def test_meanT_bwd(ops, capsys):
    w = Worst("e. meanT_bwd")
    k = 0
    for i, (B, T, C) in enumerate(MEANT):
        dh, gref, gscale = rnd(B, C, seed=i), rnd(B, T, C, seed=i + 1, scale=0.8), rnd(C, seed=i + 2, shift=1.0)
        for gact in (None,) + ALL_ACTS:
            for off in (False, True):
                k += 1
                gs = gscale if k % 2 else None
                gr = None if gact is None else (off4(gref) if off else gref)
                dz = Out((B, T, C), off=off)
                rider, mref = None, None
                if k % 3 == 0:
                    mn = MEAN_N[(k // 3) % len(MEAN_N)]
                    src, mo = rnd(mn, seed=k, shift=0.25), Out((1,))
                    rider, mref = (src, mo.t, -1.5), R.mean_scaled(src, -1.5)
                ops.meanT_bwd(off4(dh) if off else dh, dz.t, gref=gr, gact=gact or NONE, gscale=gs, mean=rider)
                what = f"meanT_bwd B={B} T={T} C={C} gact={gact} gscale={gs is not None} off4={off}"
                w.check(dz.t, R.meanT_bwd(dh, T, None if gact is None else gref, gact or NONE, gs), what)
                dz.check(what)
                if rider is not None:
                    w.check(mo.t, mref, what + f" mean rider n={mn}")
                    mo.check(what)
    w.report(capsys)


# ---------------------------------------------------------------------------------------------------------------------
# f. layernorm
# ---------------------------------------------------------------------------------------------------------------------
def test_layernorm(ops, capsys):
    w = Worst("f. layernorm")
    for i, (B, D) in enumerate(LAYERNORM):
        x = rnd(B, D, seed=i, scale=1.5, shift=0.7)
        gamma, beta = _affine(D, seed=i)
        ry, rx = R.layernorm_fwd(x, gamma, beta, 1e-5)
        what = f"layernorm_fwd B={B} D={D}"
        y, xh = Out((B, D)), Out((B, D))
        ops.layernorm_fwd(x, y.t, xh.t if i % 2 == 0 else None, gamma, beta, eps=1e-5)
        w.check(y.t, ry, what + " y")
        if i % 2 == 0:
            w.check(xh.t, rx, what + " xhat")
        y.check(what), xh.check(what)
        dy, xhat = rnd(B, D, seed=i + 3), rnd(B, D, seed=i + 4)
        dg, db = Out((D,)), Out((D,))
        ops.layernorm_bwd_params(dy, xhat, dg.t, db.t)
        rg, rb = R.layernorm_bwd_params(dy, xhat)
        w.check(dg.t, rg, f"layernorm_bwd_params B={B} D={D} dgamma")
        w.check(db.t, rb, f"layernorm_bwd_params B={B} D={D} dbeta")
        dg.check(what), db.check(what)
    w.report(capsys)


# ---------------------------------------------------------------------------------------------------------------------
# g. critic head
# ---------------------------------------------------------------------------------------------------------------------
def test_dhead(ops, capsys):
    w = Worst("g. dhead_fwd / dhead_bwd / dhead_fwd_bwd")
    for i, (B, Be, Fd, E) in enumerate(DHEAD):
        f, wt, bias, ds = rnd(B, Fd, seed=i), rnd(Fd + E, seed=i + 1, scale=0.3), rnd(1, seed=i + 2), rnd(B, seed=i + 3)
        emb = rnd(Be, E, seed=i + 4) if E else None
        what = f"dhead B={B} Be={Be} F={Fd} E={E}"
        rs = R.dhead_fwd(f, emb, wt, bias)
        s = Out((B,))
        ops.dhead_fwd(f, emb, wt, bias, s.t)
        w.check(s.t, rs, what + " fwd s")
        s.check(what)
        nb_emb = Be                                  # nb_emb < B wherever B > Be
        refs = R.dhead_bwd(ds, f, wt, Be, E, nb_emb)
        dU, demb = Out((B, Fd)), (Out((Be, E)) if E else None)
        ops.dhead_bwd(ds, f, wt, dU.t, demb.t if E else None, nb_emb if E else 0)
        w.check(dU.t, refs[0], what + " bwd dU")
        dU.check(what)
        if E:
            w.check(demb.t, refs[1], what + f" bwd demb nb_emb={nb_emb}")
            demb.check(what)
            refs_full = R.dhead_bwd(ds, f, wt, Be, E, B)
            for with_demb in (True, False):
                s2, dU2, de2 = Out((B,)), Out((B, Fd)), Out((Be, E))
                ops.dhead_fwd_bwd(ds, f, emb, wt, bias, s2.t, dU2.t, de2.t if with_demb else None, B if with_demb else 0)
                w.check(s2.t, rs, what + " fwd_bwd s")
                w.check(dU2.t, refs_full[0], what + " fwd_bwd dU")
                if with_demb:
                    w.check(de2.t, refs_full[1], what + " fwd_bwd demb")
                else:
                    assert bool(torch.isnan(de2.t).all()), what + ": demb written although not asked for"
                for o in (s2, dU2, de2):
                    o.check(what)
    w.report(capsys)


def test_dhead_wgrad_and_loss_rider(ops, capsys):
    w = Worst("g. dhead_wgrad")
    k = 0
    for i, (B, Be, Fd, E) in enumerate(DHEAD):
        f, ds = rnd(B, Fd, seed=i), rnd(B, seed=i + 3, scale=0.1)
        emb = rnd(Be, E, seed=i + 4) if E else None
        for nb in [n for n in DHEAD_NB if n <= B]:
            k += 1
            ng = {1: 3, 63: 64, 64: 1, 65: 70}[nb]                 # ng != nb
            gf = rnd(ng, Fd, seed=k, scale=0.1) if k % 2 else None
            dw, dbias = Out((Fd + E,)), Out((1,))
            loss, lrefs, louts = None, None, None
            if k % 2 == 0 or nb == 1:
                nbl = DHEAD_NB_LOSS[k % len(DHEAD_NB_LOSS)]
                s, norms = rnd(2 * nbl, seed=k + 1, shift=0.2), rnd(nbl, seed=k + 2, scale=0.3, shift=1.0).abs()
                louts = (Out((3,)), Out((1,)))
                loss = (s, norms, 10.0, louts[0].t, louts[1].t, nbl)
                lrefs = R.wgan_d_loss(s, norms, 10.0, nbl)
            ops.dhead_wgrad(ds, f, emb, gf, dw.t, dbias.t, nb, ng, loss=loss)
            what = f"dhead_wgrad B={B} Be={Be} F={Fd} E={E} nb={nb} ng={ng if gf is not None else 0}"
            rf, re_, rb = R.dhead_wgrad(ds, f, emb, gf, nb, ng)
            w.check(dw.t[:Fd], rf, what + " dw[:F]")
            if E:
                w.check(dw.t[Fd:], re_, what + " dw[F:]")
            w.check(dbias.t, rb, what + " dbias")
            dw.check(what), dbias.check(what)
            if loss is not None:
                ld, mr, mf, gp = lrefs
                for j, (r_, nm) in enumerate(((ld, "loss_d"), (mr, "mean_real"), (mf, "mean_fake"))):
                    w.check(louts[0].t[j:j + 1], r_, what + f" rider {nm} nb_loss={nbl}")
                w.check(louts[1].t, gp, what + f" rider gp nb_loss={nbl}")
                louts[0].check(what), louts[1].check(what)
    w.report(capsys)


# ---------------------------------------------------------------------------------------------------------------------
# h. WGAN-GP and losses
# ---------------------------------------------------------------------------------------------------------------------
def test_gp_interp(ops, capsys):
    w = Worst("h. gp_interp")
    real, fake = rnd(5, 37, 3, seed=1), rnd(5, 37, 3, seed=2)
    alpha = torch.tensor([0.0, 1.0, 0.3, 0.7, 0.5]).cuda()
    x = Out((5, 37, 3))
    ops.gp_interp(real, fake, alpha, x.t)
    w.check(x.t, R.gp_interp(real, fake, alpha), "gp_interp")
    exact(x.t[0], fake[0], "gp_interp alpha=0")
    exact(x.t[1], real[1], "gp_interp alpha=1")
    x.check("gp_interp")
    w.report(capsys)


def gp_problem(B, n, seed, device="cuda"):
    g = torch.randn(B, n, generator=torch.Generator().manual_seed(seed)) * (1.3 / n ** 0.5)
    if B > 1:
        g[1] = 0.0                                   # one sample with a zero gradient: fac = 0
    return g.to(device)


def test_gp_penalty(ops, capsys):
    w = Worst("h. gp_penalty")
    for i, (B, n, off, want_gbar, want_gp) in enumerate(GP_PENALTY):
        g = gp_problem(B, n, seed=i)
        rn, rg, rp = R.gp_penalty(g, 10.0)
        norms, gbar, gp = Out((B,)), Out((B, n), off=off), Out((1,))
        ops.gp_penalty(off4(g) if off else g, gbar.t if want_gbar else None, norms.t, gp.t if want_gp else None, 10.0)
        what = f"gp_penalty B={B} n={n} off4={off} gbar={want_gbar} gp={want_gp}"
        w.check(norms.t, rn, what + " norms")
        if want_gbar:
            w.check(gbar.t, rg, what + " gbar")
            if B > 1:
                exact(gbar.t[1], torch.zeros_like(gbar.t[1]), what + " zero-gradient sample")
        if want_gp:
            w.check(gp.t, rp, what + " gp")
        for o in (norms, gbar, gp):
            o.check(what)
    w.report(capsys)


def ce_problem(B, C, seed, scale, device="cuda"):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, C, generator=g) * scale).to(device), torch.randint(0, C, (B,), generator=g).to(device)


def test_softmax_ce(ops, capsys):
    w = Worst("h. softmax_ce")
    for i, (B, C) in enumerate(SOFTMAX_CE):
        for scale in (1.0, 30.0):
            z, y = ce_problem(B, C, i, scale)
            rl, rd, _ = R.softmax_ce(z, y, 0.7)
            what = f"softmax_ce B={B} C={C} scale={scale}"
            loss, dl = Out((1,)), Out((B, C))
            ops.softmax_ce(z, y, loss.t, dl.t, coef=0.7)
            w.check(loss.t, rl, what + " loss")
            w.check(dl.t, rd, what + " dlogits")
            loss2 = Out((1,))
            ops.softmax_ce(z, y, loss2.t, None, coef=0.7)
            w.check(loss2.t, rl, what + " loss (no dlogits)")
            for o in (loss, dl, loss2):
                o.check(what)
    # one target outside [0, C): a NaN loss, NaN in that row of dlogits only
    for bad_value in (4, -1):
        z, y = ce_problem(7, 4, 99, 1.0)
        yb = y.clone()
        yb[3] = bad_value
        _, rd, _ = R.softmax_ce(z, y, 1.0)
        loss, dl = Out((1,)), Out((7, 4))
        ops.softmax_ce(z, yb, loss.t, dl.t, coef=1.0)
        assert bool(torch.isnan(loss.t).all()), "softmax_ce: a bad target must poison the loss"
        assert bool(torch.isnan(dl.t[3]).all()), "softmax_ce: a bad target must poison its row of dlogits"
        keep = torch.ones(7, dtype=torch.bool, device="cuda")
        keep[3] = False
        w.check(torch.where(keep[:, None], dl.t, rd.val.float()), rd, f"softmax_ce bad target {bad_value}: the other rows")
        loss.check("softmax_ce"), dl.check("softmax_ce")
    w.report(capsys)


def test_mean_scaled(ops, capsys):
    w = Worst("h. mean_scaled")
    for i, n in enumerate(MEAN_N):
        src, out = rnd(n, seed=i, shift=0.3), Out((1,))
        ops.mean_scaled(src, out.t, scale=-1.0)
        w.check(out.t, R.mean_scaled(src, -1.0), f"mean_scaled n={n}")
        out.check("mean_scaled")
    w.report(capsys)


# ---------------------------------------------------------------------------------------------------------------------
# i. elementwise
# ---------------------------------------------------------------------------------------------------------------------
def test_elementwise(ops, capsys):
    w = Worst("i. elementwise")
    x, y0 = rnd(1000, seed=1), rnd(1000, seed=2)
    y = Out((1000,))                                 # b = 0 must not read y: it is full of NaN
    ops.axpby(x, y.t, a=0.3, b=0.0)
    exact(y.t, x * torch.tensor(0.3, dtype=torch.float32), "axpby b=0")
    y.check("axpby")
    y = Out((1000,), init=y0)
    ops.axpby(x, y.t, a=0.3, b=-1.7)
    w.check(y.t, R.axpby(x, y0, 0.3, -1.7), "axpby")
    y.check("axpby")
    # copy_cols: offsets, one column, full width, accumulate
    src, d0 = rnd(7, 10, seed=3), rnd(7, 13, seed=4)
    for soff, doff, nc, acc in ((2, 5, 6, False), (9, 12, 1, False), (0, 0, 1, True), (3, 1, 7, True), (0, 3, 10, False)):
        dst = Out((7, 13), init=d0)
        ops.copy_cols(src, soff, dst.t, doff, nc, accumulate=acc)
        want = d0.clone()
        want[:, doff:doff + nc] = (d0[:, doff:doff + nc] + src[:, soff:soff + nc]) if acc else src[:, soff:soff + nc]
        exact(dst.t, want, f"copy_cols soff={soff} doff={doff} ncols={nc} accumulate={acc}")
        dst.check("copy_cols")
    full = Out((7, 10))
    ops.copy_cols(src, 0, full.t, 0, 10)
    exact(full.t, src, "copy_cols full width")
    full.check("copy_cols")
    # act_bwd: every gact x emul
    dy, gref, emul = rnd(1031, seed=5), rnd(1031, seed=6, scale=0.8), rnd(1031, seed=7)
    for gact in (None,) + ALL_ACTS:
        for em in (None, emul):
            dx = Out((1031,))
            ops.act_bwd(dy, dx.t, gref=None if gact is None else gref, gact=gact or NONE, emul=em)
            what = f"act_bwd gact={gact} emul={em is not None}"
            w.check(dx.t, R.act_bwd(dy, None if gact is None else gref, gact or NONE, em), what)
            if gact in (None, NONE, RELU):
                want = dy * (1.0 if gact != RELU else (gref > 0).float())
                exact(dx.t, want if em is None else want * em, what)
            dx.check(what)
    # transpose_bcl_blc
    for i, (C, L) in enumerate(TRANSPOSE):
        xin, gr = rnd(2, C, L, seed=i), rnd(2, L, C, seed=i + 1, scale=0.8)
        yt = Out((2, L, C))
        ops.transpose_bcl_blc(xin, yt.t)
        exact(yt.t, xin.transpose(1, 2).contiguous(), f"transpose C={C} L={L}")
        yt.check("transpose")
        gact = ALL_ACTS[i % len(ALL_ACTS)] or TANH
        yt = Out((2, L, C))
        ops.transpose_bcl_blc(xin, yt.t, gref=gr, gact=gact)
        w.check(yt.t, R.act_bwd(xin.transpose(1, 2).contiguous(), gr, gact), f"transpose C={C} L={L} gact={gact}")
        yt.check("transpose")
    w.report(capsys)


# ---------------------------------------------------------------------------------------------------------------------
# j. optimiser and VAE
# ---------------------------------------------------------------------------------------------------------------------
ADAM_HP = dict(lr=2e-4, beta1=0.5, beta2=0.999, eps=1e-8)


def adam_problem(n, seed, device="cuda"):
    """A mid-training state: step 7 done, m ~ 0.1 randn, v ~ (0.1 randn)^2."""
    g = torch.Generator().manual_seed(seed)
    p, gr, m = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.3, torch.randn(n, generator=g) * 0.1
    v = (torch.randn(n, generator=g) * 0.1) ** 2
    b1, b2 = R.f32(ADAM_HP["beta1"]), R.f32(ADAM_HP["beta2"])
    state = torch.tensor([7.0, b1 ** 7, b2 ** 7, 0.0], dtype=torch.float64)
    return tuple(t.to(device) for t in (p, gr, m, v, state))


def test_adam_flat_one_step(ops, capsys):
    w = Worst("j. adam_flat")
    for i, n in enumerate(ADAM_N):
        for wd in (0.0, 0.01):
            p0, g, m0, v0, state = adam_problem(n, seed=i)
            gs_dev = torch.tensor([0.7]).cuda() if i % 2 else None
            p, m, v = Out((n,), init=p0), Out((n,), init=m0), Out((n,), init=v0)
            ops.adam_flat(p.t, g, m.t, v.t, state, weight_decay=wd, grad_scale=0.5, gs_dev=gs_dev, **ADAM_HP)
            rp, rm, rv = R.adam_step(p0, g, m0, v0, 8, weight_decay=wd, grad_scale=0.5, gs_dev=gs_dev, **ADAM_HP)
            what = f"adam_flat n={n} wd={wd} gs_dev={gs_dev is not None}"
            w.check(p.t, rp, what + " p")
            w.check(m.t, rm, what + " m")
            w.check(v.t, rv, what + " v")
            assert float(state[0]) == 8.0, what + ": the step counter"
            for o in (p, m, v):
                o.check(what)
    w.report(capsys)


def test_adam_flat_wq_scatter(ops, capsys):
    """The WQ copies the update refreshes: one w[n][c][k] and one w[c][n][k] entry that do not cover the buffer; the copies
    equal the updated parameters re-laid out on the host, bit for bit, and nothing beside them is written."""
    N, Cc, K = WQ["N"], WQ["Cc"], WQ["K"]
    cnt = N * Cc * K
    for n in (257, 4099):
        p0, g, m0, v0, state = adam_problem(n, seed=n)
        p, m, v = Out((n,), init=p0), Out((n,), init=m0), Out((n,), init=v0)
        d_nck, d_cnk = Out((cnt,)), Out((cnt,))
        s0, s1 = WQ["starts"] if n > 400 else (3, 130)
        table = ops.wq_table([(s0, N, Cc, K, Cc * K, K, d_nck.t), (s1, N, Cc, K, K, N * K, d_cnk.t)])
        ops.adam_flat(p.t, g, m.t, v.t, state, wq=table, **ADAM_HP)
        rp, _, _ = R.adam_step(p0, g, m0, v0, 8, **ADAM_HP)
        R.check(p.t, rp, f"adam_flat wq n={n} p")
        exact(d_nck.t, R.wq_layout(p.t[s0:s0 + cnt], N, Cc, K, cnk=False), f"adam_flat wq n={n} w[n][c][k] copy")
        exact(d_cnk.t, R.wq_layout(p.t[s1:s1 + cnt], N, Cc, K, cnk=True), f"adam_flat wq n={n} w[c][n][k] copy")
        for o in (p, m, v, d_nck, d_cnk):
            o.check("adam_flat wq")


def test_grad_norm_clip(ops, capsys):
    w = Worst("j. grad_norm_clip")
    for i, n in enumerate(GRAD_NORM_N):
        g = rnd(n, seed=i, scale=1.0 / n ** 0.5)                  # |g| ~ 1
        for max_norm in (0.25, 4.0):                                # above and below the norm
            out = Out((2,))
            ops.grad_norm_clip(g, max_norm, out.t)
            w.check(out.t, R.grad_norm_clip(g, max_norm), f"grad_norm_clip n={n} max_norm={max_norm}")
            out.check("grad_norm_clip")
    for n in (1, 8193):
        out = Out((2,))
        g = torch.zeros(n).cuda()
        ops.grad_norm_clip(g, 1.0, out.t)
        exact(out.t, torch.tensor([0.0, 1.0]).cuda(), f"grad_norm_clip all-zero n={n}")
        out.check("grad_norm_clip")
    w.report(capsys)


def test_reparam(ops, capsys):
    w = Worst("j. reparam")
    for i, n in enumerate((1, 255, 257, 2048)):
        mu, lv, eps, dz = rnd(n, seed=i), rnd(n, seed=i + 1, scale=0.7), rnd(n, seed=i + 2), rnd(n, seed=i + 3)
        z = Out((n,))
        ops.reparam_fwd(mu, lv, eps, z.t)
        w.check(z.t, R.reparam_fwd(mu, lv, eps), f"reparam_fwd n={n}")
        z.check("reparam_fwd")
        km, kl = rnd(n, seed=i + 4, scale=0.01), rnd(n, seed=i + 5, scale=0.01)
        dmu, dlv = Out((n,)), Out((n,))
        ops.reparam_bwd(dz, lv, eps, km, kl, dmu.t, dlv.t)
        rm, rl = R.reparam_bwd(dz, lv, eps, km, kl)
        w.check(dmu.t, rm, f"reparam_bwd n={n} dmu")
        w.check(dlv.t, rl, f"reparam_bwd n={n} dlv")
        dmu.check("reparam_bwd"), dlv.check("reparam_bwd")
    w.report(capsys)


def test_reparam_bwd_without_kld_terms(ops, capsys):
    w = Worst("j. reparam_bwd without the KLD terms")
    n = 257
    lv, eps, dz = rnd(n, seed=1, scale=0.7), rnd(n, seed=2), rnd(n, seed=3)
    dmu, dlv = Out((n,)), Out((n,))
    ops.reparam_bwd(dz, lv, eps, None, None, dmu.t, dlv.t)
    rm, rl = R.reparam_bwd(dz, lv, eps)
    exact(dmu.t, dz, "reparam_bwd dmu without KLD")
    w.check(dlv.t, rl, "reparam_bwd dlv without KLD")
    dmu.check("reparam_bwd"), dlv.check("reparam_bwd")
    w.report(capsys)


def vae_problem(nx, nz, seed, device="cuda"):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(nx, generator=g)
    recon = x + torch.randn(nx, generator=g) * 0.2
    return tuple(t.to(device) for t in (recon, x, torch.randn(nz, generator=g), torch.randn(nz, generator=g) * 0.7))


def test_vae_loss(ops, capsys):
    w = Worst("j. vae_loss")
    k = 0
    for i, (nx, nz) in enumerate(VAE):
        recon, x, mu, lv = vae_problem(nx, nz, seed=i)
        (rt, rmse, rk), rdr, rdm, rdl = R.vae_loss(recon, x, mu, lv, 0.3)
        for off in (False, True):
            for grads in ((True, True, True), (True, False, False), (False, True, False), (False, False, True), (False, False, False)):
                k += 1
                out, dr, dm, dl = Out((3,)), Out((nx,), off=off), Out((nz,)), Out((nz,))
                ops.vae_loss(off4(recon) if off else recon, off4(x) if off else x, mu, lv, 0.3, out.t,
                             drecon=dr.t if grads[0] else None, dmu=dm.t if grads[1] else None, dlv=dl.t if grads[2] else None)
                what = f"vae_loss n_x={nx} n_z={nz} off4={off} grads={grads}"
                for j, r_ in enumerate((rt, rmse, rk)):
                    w.check(out.t[j:j + 1], r_, what + f" out[{j}]")
                for o, r_, on, nm in ((dr, rdr, grads[0], "drecon"), (dm, rdm, grads[1], "dmu"), (dl, rdl, grads[2], "dlv")):
                    if on:
                        w.check(o.t, r_, what + " " + nm)
                    else:
                        assert bool(torch.isnan(o.t).all()), what + f": {nm} written although not asked for"
                    o.check(what)
                out.check(what)
    w.report(capsys)
