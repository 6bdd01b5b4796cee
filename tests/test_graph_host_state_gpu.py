"""Graph replay and the host state a sub-step's Python changes (ops.run_graphed): FlatParams.ticked, which selects the Adam
launch form of the next update, GanEngine.num_batches_tracked and EdEngine.updates.  A replay runs no Python and re-applies
what the capture recorded, so an engine driven through run(name, True) must hold, after every call, the host state of its twin
driven through run(name, False), and end in the same bits -- in every production order, and for a flow of any name."""
import os
import socket
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_ed_latent_gpu import OPT, engine as latent_engine, latent_cfg  # noqa: E402
from test_ed_staged_gpu import ed_cfg, fresh_engine  # noqa: E402
from test_engine_gpu import engine_mod, load, make  # noqa: E402,F401  (fixture)

GAN_CASES = ["gan_c4_t20_b3", "gan_c128_t64_b4", "gan_c4_t16_cond_lat"]      # no conv16 layer / conv16 and chains / latent fork


def traced(eng):
    """eng.run logging the host state every call leaves."""
    log, run = [], eng.run

    def logged(name, use_graph=True):
        run(name, use_graph)
        log.append(eng.host_state())
    eng.run = logged
    return log


def gan_pair(engine_mod, case, seed=5):
    """(replaying engine, eager engine) from the same state, batch and seed, with their logs."""
    pair = [make(engine_mod, load(case))[1] for _ in range(2)]
    for e in pair:
        e.seed(seed)
    return pair, [traced(e) for e in pair]


def same_bits(a, b):
    torch.cuda.synchronize()
    tensors = lambda e: dict(D=e.D.data, GE=e.GE.data, GE_m=e.GE.m, D_state=e.D.state, GE_state=e.GE.state, rng_step=e.rng_step)  # noqa: E731
    for (what, x), y in zip(tensors(a).items(), tensors(b).values()):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), what
    assert a.host_state() == b.host_state()


def same_logs(logs, least):
    assert len(logs[0]) == len(logs[1]) >= least
    for i, (x, y) in enumerate(zip(*logs)):
        assert x == y, (i, x, y)


def replayed_at_least(eng, times, calls):
    """Every key of eng._graphs is captured and was called often enough for `times` pure replays (calls: name -> count)."""
    for key, entry in eng._graphs.items():
        assert not isinstance(entry, str) and calls[key.split("#")[0]] >= 2 + times, key


# ---- GAN -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GAN_CASES)
def test_gan_single_gpu_orders_leave_the_eager_host_state_after_every_call(engine_mod, case):
    """dg_step_rng / d_step_rng mixed, then DataParallel.step on one GPU with back-to-back generator steps (the forked graph;
    eagerly the same batches take dg_step_rng, which test_forked_flow_equals_the_single_graph_flow holds bit-equal)."""
    from melo_gan_amd.gan.dp import DataParallel
    (eg, ee), logs = gan_pair(engine_mod, case)
    dps = [DataParallel(e, 1, None) for e in (eg, ee)]
    with torch.cuda.stream(eg.stream):
        for it in range(10):
            for e, graph in ((eg, True), (ee, False)):
                e.run("dg_step_rng" if it % 2 else "d_step_rng", graph)
        for g_step in [True] * 6 + [False] * 3:
            for dp, graph in zip(dps, (True, False)):
                dp.step(graph, g_step=g_step)
    same_logs(logs, 19)
    same_bits(eg, ee)
    calls = dict(dg_step_rng=6, d_step_rng=8, dg_fork_step_rng=5)
    assert set(eg._graphs) == set(calls)                   # no optimiser step is pending between whole steps: plain keys
    replayed_at_least(eg, 3, calls)
    assert eg.num_batches_tracked > 19 and not eg.D.ticked and not eg.GE.ticked


@pytest.fixture
def one_rank_group():
    """A 1-rank RCCL process group, as bench.py's MELO_FORCE_DP rehearsal makes it; gone again behind the test (its watchdog
    thread must not meet a later test's capture)."""
    import torch.distributed as dist
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    keep = {k: os.environ.get(k) for k in ("MASTER_ADDR", "MASTER_PORT")}
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", torch.cuda.current_device()))
    try:
        yield dist
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()
        for k, v in keep.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)


@pytest.mark.parametrize("mode", ["gather", "allreduce", "overlap"])
@pytest.mark.parametrize("case", GAN_CASES[:2])
def test_gan_distributed_orders_leave_the_eager_host_state_after_every_call(engine_mod, monkeypatch, one_rank_group, case, mode):
    """The three torch.distributed step orders on a 1-rank group, prepare() included: every graph is captured by the dry
    steps, before the first collective (gan/dp.py), and from then on each sub-step is a replay."""
    from melo_gan_amd.gan.dp import DataParallel
    monkeypatch.setenv("MELO_DP_MODE", mode)
    (eg, ee), logs = gan_pair(engine_mod, case)
    dps = [DataParallel(e, 1, one_rank_group, force_collectives=True) for e in (eg, ee)]
    assert all(dp.active and dp.mode == mode for dp in dps)
    with torch.cuda.stream(eg.stream):
        before = eg.host_state()
        dps[0].prepare(True)
        assert eg.capture_locked and eg.host_state() == before
        assert all(not isinstance(v, str) for v in eg._graphs.values())
        del logs[0][:]                                     # the dry steps: not the eager engine's calls
        for g_step in (True, True, False, True, False, False, True):
            for dp, graph in zip(dps, (True, False)):
                dp.step(graph, g_step=g_step)
    same_logs(logs, 4 * 5 + 3 * 2)
    same_bits(eg, ee)
    names = {k.split("#")[0] for k in eg._graphs}
    assert len(names) == len(eg._graphs)                   # each sub-step always arrives in the same state: one graph each
    assert {"d_update#True/False", "d_update_g_critic_chain#True/nobump", "g_update#False/nobump"} <= set(eg._graphs)


def test_gan_flow_of_any_name_replays_like_the_flow_it_copies(engine_mod):
    """Nothing is derived from a sub-step's name: `foo`, whose body is dg_step_rng's, `critic_then`, which is d_backward_rng
    + d_update, and `front`, which is d_backward_rng alone in front of a d_update, replayed through run() leave the parameters
    and the host state of dg_step_rng / d_step_rng / d_backward_rng replayed: the d_update behind a replayed `front` must meet
    the pending Adam state the draw left, and take the launch form that goes with it."""
    (named, plain), logs = gan_pair(engine_mod, "gan_c4_t20_b3")
    cls = type(named)
    named.foo = types.MethodType(lambda self: cls.dg_step_rng(self), named)
    named.critic_then = types.MethodType(lambda self: (self.d_backward_rng(), self.d_update()), named)
    named.front = types.MethodType(lambda self: cls.d_backward_rng(self), named)
    with torch.cuda.stream(named.stream):
        for it in range(5):
            for e, (dg, d, front) in ((named, ("foo", "critic_then", "front")), (plain, ("dg_step_rng", "d_step_rng", "d_backward_rng"))):
                e.run(dg)
                e.run(d)
                e.run(front)
                e.run("d_update")
    same_logs(logs, 20)
    same_bits(named, plain)
    same = {"foo": "dg_step_rng", "critic_then": "d_step_rng", "front": "d_backward_rng"}
    assert {same.get(k, k) for k in named._graphs} == set(plain._graphs) == {"dg_step_rng", "d_step_rng", "d_backward_rng", "d_update#True/False"}
    assert all(not isinstance(v, str) for v in named._graphs.values())


# ---- emotion classifier --------------------------------------------------------------------------------------------------------
def ed_pair(kind):
    B, n = 8, 24 * 8
    g = torch.Generator().manual_seed(5)
    if kind == "notes":
        pair = [fresh_engine(ed_cfg(4), B, 32) for _ in range(2)]
        x = (torch.rand(n, 32, 4, generator=g) * 2 - 1).cuda()
    else:
        cfg = dict(latent_cfg(24, [40, 24]), batch_size=B, optimizer=dict(OPT, lr=1e-3), seed=9)
        pair = [latent_engine(cfg, B, kind == "latent-fused", seed=3) for _ in range(2)]
        x = torch.randn(n, 24, generator=g).cuda()
    y = torch.randint(0, 4, (n,), generator=g).cuda()
    for e in pair:
        e.attach_split(x, y)
        e.set_epoch(torch.arange(n), 0)
        e.tail(3).set_batch(x[:3], y[:3])
    return pair, x, y


@pytest.mark.parametrize("kind", ["notes", "latent-fused", "latent-layers"])
def test_ed_orders_leave_the_eager_host_state_after_every_call(kind):
    """step_rng, backward_rng + update, step_staged on the full engine and on a tail(3), forward_eval: five rounds, so every
    graph sees its eager call, its capture and three replays.  Then set_lr: the graphs whose capture saw an optimiser step
    go, a captured forward_eval stays."""
    (eg, ee), x, y = ed_pair(kind)
    logs = [traced(e) for e in (eg, ee)]
    tail_logs = [traced(e.tail(3)) for e in (eg, ee)]
    with torch.cuda.stream(eg.stream):
        for it in range(5):
            for e, graph in ((eg, True), (ee, False)):
                e.set_batch(x[it * 8:it * 8 + 8], y[it * 8:it * 8 + 8])
                for name in ("step_rng", "backward_rng", "update", "step_staged"):
                    e.run(name, graph)
                e.tail(3).run("step_staged", graph)
                e.run("forward_eval", graph)
                e.tail(3).run("forward_eval", graph)
            assert eg.host_state() == ee.host_state() and eg.tail(3).host_state() == ee.tail(3).host_state(), it
    torch.cuda.synchronize()
    same_logs(logs, 25)
    same_logs(tail_logs, 10)
    assert eg.host_state() == ((False,), (15,)) and eg.tail(3).host_state() == ((False,), (5,))
    for a, b in ((eg, ee), (eg.tail(3), ee.tail(3))):
        assert torch.equal(a.logits, b.logits)
    for what in ("data", "m", "v", "state"):
        assert torch.equal(getattr(eg.P, what).view(torch.uint8), getattr(ee.P, what).view(torch.uint8)), what
    assert torch.equal(eg.rng_step, ee.rng_step) and int(eg.rng_step.item()) == 20 and float(eg.P.state[0].item()) == 20.0
    for k in eg.buf:
        assert torch.equal(eg.buf[k], ee.buf[k]), k
    assert set(eg._graphs) == {"step_rng", "backward_rng", "update#True", "step_staged", "forward_eval"}
    assert set(eg.tail(3)._graphs) == {"step_staged", "forward_eval"}
    assert all(not isinstance(v, str) for e in (eg, eg.tail(3)) for v in e._graphs.values())
    kept = eg._graphs["forward_eval"], eg._graphs["backward_rng"], eg.tail(3)._graphs["forward_eval"]
    eg.set_lr(5e-4)
    assert set(eg._graphs) == {"backward_rng", "forward_eval"} and set(eg.tail(3)._graphs) == {"forward_eval"}
    assert kept == (eg._graphs["forward_eval"], eg._graphs["backward_rng"], eg.tail(3)._graphs["forward_eval"])
