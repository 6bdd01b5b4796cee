"""The forked step's generator tail (GanEngine.g_backward_b with a side stream): decoder.pre.2's data gradient heads the
critical path and is enqueued in front of the side branch's weight gradients; MELO_P2_DGRAD_FIRST=0, read when the step is
captured, keeps the earlier order.  Both orders make the same launches with the same job lists, so parameters, optimiser
state and losses are equal bit for bit -- to each other and to what test_engine_gpu holds the forked flow to.  Also the
split Linear plans linear_finish_kernel sums more than one round of eight slabs for (16 and 32 slabs), against fp64."""
import contextlib

import pytest
import torch

import stride2_ref as S
import window_ref as W
from test_engine_gpu import engine_mod, load, make  # noqa: F401  (fixture)
from test_window_contract_gpu import Worst, rnd

pytestmark = pytest.mark.gpu


class _Launches:
    def __init__(self):
        self.seen = []

    def __call__(self, sym, flops, launch=None):
        self.seen.append((sym, flops))
        return contextlib.nullcontext()


def _forked_steps(engine_mod, monkeypatch, first):
    from melo_gan_amd import ops
    from melo_gan_amd.gan.dp import DataParallel
    monkeypatch.setenv("MELO_P2_DGRAD_FIRST", first)
    g = load("gan_c128_t64_b4")
    _, eng, cfg, batch = make(engine_mod, g, use_graph=True)
    dp = DataParallel(eng, 1, None)
    eng.seed(5)
    rec = _Launches()
    ops.set_launch_hook(rec)
    try:
        with torch.cuda.stream(eng.stream):
            for _ in range(3):
                eng.set_batch(*[t.cuda() for t in batch])
                dp.step(True, g_step=True)
        torch.cuda.synchronize()
    finally:
        ops.set_launch_hook(None)
    assert "dg_fork_step_rng" in eng._graphs
    # pre.2's data gradient, by its FLOPs: (B, 256 red) x (256 red, 512); the launch enqueued next to it
    flops = 2.0 * eng.B * 512 * 256 * eng.red
    at = [i for i, (s, f) in enumerate(rec.seen) if s.startswith("linear_skinny_kernel<false,") and f == flops]
    assert at, [s for s, _ in rec.seen]
    i = at[-1]
    state = (eng.D.data.clone(), eng.GE.data.clone(), eng.GE.m.clone(), float(eng.loss_d_out[0]), float(eng.adv), float(eng.emo))
    return state, rec.seen[i - 1][0], rec.seen[i + 1][0]


def test_both_orders_of_the_forked_tail_leave_the_same_bits(engine_mod, monkeypatch):
    new, before_new, after_new = _forked_steps(engine_mod, monkeypatch, "1")
    old, before_old, after_old = _forked_steps(engine_mod, monkeypatch, "0")
    # new: the weight gradients follow the data gradient; old: they are enqueued in front of it
    assert after_new.startswith("wgrad_multi_kernel<") and not before_new.startswith("wgrad_multi_kernel<"), (before_new, after_new)
    assert before_old.startswith("wgrad_multi_kernel<") and not after_old.startswith("wgrad_multi_kernel<"), (before_old, after_old)
    for a, b in zip(new[:3], old[:3]):
        assert torch.equal(a, b)
    assert new[3:] == old[3:]


# (M, K, N, forward?, ksplit): plan_ksplit doubles the split while a wave keeps more than 128 k
DEEP_SPLITS = [(3, 16384, 33, True, 16), (3, 16384, 33, False, 16), (2, 20480, 5, True, 32), (2, 20480, 5, False, 32)]


def test_finish_kernel_sums_sixteen_and_thirty_two_slabs(capsys):
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import ops
    worst = Worst("d. linear_finish_kernel, 16 and 32 slabs")
    for i, (M, K, N, fwd, ks) in enumerate(DEEP_SPLITS):
        what = f"M={M} K={K} N={N} fwd={fwd} ksplit={ks}"
        x = rnd(M, K, seed=i)
        w = rnd(N, K, seed=i + 1, scale=0.05) if fwd else rnd(K, N, seed=i + 1, scale=0.05)
        bias = rnd(N, seed=i + 2)
        assert ops.linear_route(M, K, N, K if fwd else 1, 1 if fwd else N)[1] == ks, what
        y = S.Guarded((M, N))
        (ops.linear_fwd if fwd else ops.linear_dgrad)(x, w, y.t, bias=bias, act=ops.ACT_RELU)
        acc = W.linear(x, w) if fwd else W.linear_dgrad(x, w)
        worst.check(y.t, W.Ref(*acc, K).epilogue(bias=bias, act=S.ACT_RELU), what)
        y.check(what)
    worst.report(capsys)
