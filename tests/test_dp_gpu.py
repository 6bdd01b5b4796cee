"""Data-parallel "gather" mode on the GPU engine (melo-gan_amd/gan/dp.py): decoder.pre.2.weight's gradient computed from
the all-gathered per-sample factors equals the sum of the shards' own weight gradients -- what an all-reduce delivers.
Two engines in one process stand in for two ranks; the collectives are done by hand."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import melo_oracle as O  # noqa: E402


def rel_err(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def test_factor_gather_equals_summed_shard_gradients():
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.gan.engine import GanEngine
    B, T, C, WORLD = 4, 32, 4, 2
    cfg, ed_cfg = O.default_gan_cfg(B, T, C), O.default_ed_cfg(C)
    engs = [GanEngine(cfg, ed_cfg, "cuda", B) for _ in range(WORLD)]
    inputs = []
    for r, e in enumerate(engs):
        e.init_weights(seed=3)                       # identical replicas
        g = torch.Generator().manual_seed(50 + r)    # each rank its own shard and its own draws
        real, numeric, latent, emot = O.synthetic_batch(B, T, C, cfg["LATENT_DIM"], 6, 70 + r)
        noise = torch.randn(tuple(e.noise.shape), generator=g)
        masks = [(torch.rand(tuple(m.shape), generator=g) < 0.8).float() for m in e.dmask]
        inputs.append((real.cuda(), numeric.cuda(), latent.cuda(), emot.cuda(), noise.cuda(), [m.cuda() for m in masks]))
    assert torch.equal(engs[0].GE.data, engs[1].GE.data)

    def feed(e, x):
        e.set_batch(*x[:4])
        e.set_randoms(x[4], x[5])

    # the shards' own gradients (single-GPU path), summed = what all-reduce(SUM) hands every rank
    ref = []
    for e, x in zip(engs, inputs):
        feed(e, x)
        e.g_backward()
        ref.append(e.GE.grad.clone())
    want = ref[0] + ref[1]
    off, n = engs[0].p2_grad_slice()                    # pre.2's weight and bias: adjacent, first in the flat buffer
    assert off == 0 and n == 256 * engs[0].red * 512 + 256 * engs[0].red

    # gather mode
    for e, x in zip(engs, inputs):
        e.enable_p2_gather(WORLD)
        e.GE.grad.fill_(float("nan"))
        feed(e, x)
        e.g_backward_a()
    d_all = torch.cat([e.d_p2 for e in engs])        # all_gather_into_tensor: rank order
    a_all = torch.cat([e.a_p0 for e in engs])
    for e in engs:
        e.d_p2_all.copy_(d_all)
        e.a_p0_all.copy_(a_all)
        e.g_backward_p2b()
    assert not torch.isnan(engs[0].GE.grad).any()
    assert torch.equal(engs[0].GE.grad[:n], engs[1].GE.grad[:n])            # every rank holds the same global gradient
    assert rel_err(engs[0].GE.grad[:n], want[:n]) < 2e-6
    rest = engs[0].GE.grad[n:] + engs[1].GE.grad[n:]                         # the remaining all-reduce
    assert rel_err(rest, want[n:]) < 2e-6
    o, m = engs[0].GE.offsets["G.decoder.pre.2.bias"]
    assert o + m == n and rel_err(engs[0].GE.grad[o:o + m], want[o:o + m]) < 2e-6   # bias: column sums of the gathered d_p2


@pytest.mark.timeout(600)
def test_two_rank_trainer_gather_equals_allreduce(tmp_path):
    """The trainer CLI under torch.distributed.run with 2 ranks (sharing this GPU, gloo): one epoch in MELO_DP_MODE=gather
    and in =allreduce from the same seed ends in the same generator / encoder parameters (tools/dp_mode_equivalence.sh)."""
    import os
    import subprocess
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    r = subprocess.run(["bash", os.path.join(root, "tools", "dp_mode_equivalence.sh"), str(tmp_path)], cwd=root,
                       capture_output=True, text=True, timeout=560)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "largest relative difference gather vs allreduce" in r.stdout


@pytest.mark.timeout(600)
@pytest.mark.parametrize("mode", ["ingraph", "gather", "allreduce", "overlap"])
def test_step_orders_run_on_a_one_rank_rccl_group(mode):
    """bench.py with MELO_FORCE_DP=1: a 1-rank RCCL ("nccl") process group and the N > 1 step order on this GPU, through
    warm-up, graph capture and replay.  Guards the interplay of on-stream collectives, the process group's watchdog
    thread and hipGraph capture (an abort in the first version of this path, ops._quiesce_process_group)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    env = dict(os.environ, MELO_FORCE_DP="1", MELO_DP_MODE=mode, MASTER_ADDR="127.0.0.1", MASTER_PORT="29611")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "12", "--warmup", "4", "--no-cpu-baseline",
                        "--profile-steps", "0"], cwd=root, env=env, capture_output=True, text=True, timeout=560)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["value"] > 0 and line["config"]["dp_mode"] == mode
    for v in line["losses"].values():
        assert v == v and abs(v) < 1e6


def test_rccl_collectives_are_graph_nodes_and_the_ingraph_step_equals_the_single_gpu_step():
    """gan/rccl.py on a 1-rank communicator: all-reduce / all-gather (also grouped) enqueued on the engine's stream, eagerly
    and replayed from a captured hipGraph; and the data-parallel step with the collectives INSIDE its graphs leaves the same
    bits as the plain single-GPU step (world = 1: the collectives are identities, grad_scale is 1)."""
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import ops
    from melo_gan_amd.gan import rccl
    from melo_gan_amd.gan.dp import DataParallel
    from melo_gan_amd.gan.engine import GanEngine
    comm = rccl.RcclComm(0, 1, rccl.unique_id())
    st = torch.cuda.Stream()
    a, b = torch.arange(1000, dtype=torch.float32, device="cuda"), torch.ones(64, 8, device="cuda")
    g1, g2 = torch.zeros(64, 8, device="cuda"), torch.zeros(1000, device="cuda")
    with torch.cuda.stream(st):
        for graph in (False, True):
            if graph:
                torch.cuda.synchronize()
                g = ops.Graph()
                g.begin()
            comm.group_start()
            comm.all_reduce(a)
            comm.all_gather(b, g1)
            comm.group_end()
            comm.all_gather(a, g2)
            if graph:
                g.end()
                b.fill_(3.0)
                g.launch()
            torch.cuda.synchronize()
            assert torch.equal(a, torch.arange(1000, dtype=torch.float32, device="cuda")) and torch.equal(g1, b) and torch.equal(g2, a)
    B, T, C = 4, 64, 128
    cfg, ed_cfg = O.default_gan_cfg(B, T, C), O.default_ed_cfg(C)
    S = O.build_gan_state(cfg, ed_cfg, "closed_form", d_scale=6.0)
    batch = O.synthetic_batch(B, T, C, cfg["LATENT_DIM"], 6, 70)
    res = []
    for dp_on in (False, True):
        e = GanEngine(cfg, ed_cfg, "cuda", B)
        e.load_state(S.PE, S.PG, S.BG, S.PD, S.PED, S.BED)
        e.seed(5)
        dp = DataParallel(e, 1, None, force_collectives=dp_on, comm=comm if dp_on else None)
        assert dp.mode == ("ingraph" if dp_on else dp.mode) and (e.coll is not None) == dp_on
        with torch.cuda.stream(e.stream):
            e.set_batch(*(t.cuda() for t in batch))
            for g_step in (True, True, True, False, True, True, False, True, True, True):
                dp.step(True, g_step=g_step)
            torch.cuda.synchronize()
        res.append((e.D.data.clone(), e.GE.data.clone(), e.GE.m.clone(), float(e.loss_d_out[0]), float(e.adv), float(e.emo)))
    for x, y in zip(*res):
        assert (torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y)
    comm.destroy()


class _Work:
    def wait(self):
        return True


class _ThreadDist:
    """torch.distributed stand-in for two ranks living in one process as two threads (one engine and one stream each):
    every collective is a rendezvous at a barrier with the data exchanged through a shared slot list."""

    class ReduceOp:
        SUM = "sum"

    def __init__(self, rank, world, barrier, slots):
        self.rank, self.world, self.barrier, self.slots = rank, world, barrier, slots

    def _exchange(self, t):
        torch.cuda.current_stream().synchronize()
        self.slots[self.rank] = t
        self.barrier.wait()
        return list(self.slots)

    def get_backend(self, group=None):
        return "thread"

    def all_reduce(self, t, op=None, group=None, async_op=False):
        ts = self._exchange(t)
        total = ts[0].clone()
        for x in ts[1:]:
            total += x                      # rank order on every rank: identical bits everywhere
        torch.cuda.current_stream().synchronize()
        self.barrier.wait()                 # everyone has read before anyone overwrites
        t.copy_(total)
        return _Work()

    def all_gather_into_tensor(self, dst, src, group=None, async_op=False):
        ts = self._exchange(src)
        n = src.shape[0]
        for r, x in enumerate(ts):
            dst[r * n:(r + 1) * n].copy_(x)
        torch.cuda.current_stream().synchronize()
        self.barrier.wait()
        return _Work()

    def broadcast(self, t, src=0, group=None, async_op=False):
        ts = self._exchange(t)
        if self.rank != src:
            t.copy_(ts[src])
        torch.cuda.current_stream().synchronize()
        self.barrier.wait()
        return _Work()


class _ThreadComm:
    """gan/rccl.py's communicator interface over _ThreadDist (eager only): the ingraph step order on two threads."""

    def __init__(self, td):
        self.td, self.rank, self.world = td, td.rank, td.world

    def all_reduce(self, t):
        self.td.all_reduce(t)

    def all_gather(self, src, dst):
        self.td.all_gather_into_tensor(dst, src)

    def group_start(self):
        pass

    def group_end(self):
        pass


@pytest.mark.parametrize("mode", ["ingraph", "overlap", "gather", "allreduce"])
def test_two_engines_as_two_ranks_full_step(mode, monkeypatch):
    """DataParallel.step for the full critic + generator step with two engines as two ranks (two threads, a barrier-based
    stand-in for torch.distributed): graphs captured by prepare(), every collective of the mode's step order issued.
    Afterwards both replicas hold bit-identical parameters, the reduced gradients equal the mean of the shards' own
    gradients as the ORACLE computes them from the randoms each rank drew, and the parameters moved the way Adam moves
    them on that averaged gradient."""
    import threading
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.gan.dp import DataParallel
    from melo_gan_amd.gan.engine import GanEngine
    monkeypatch.setenv("MELO_DP_MODE", mode)
    B, T, C, WORLD = 4, 32, 4, 2
    cfg, ed_cfg = O.default_gan_cfg(B, T, C), O.default_ed_cfg(C)
    S = O.build_gan_state(cfg, ed_cfg, "closed_form", d_scale=6.0)
    barrier, slots = threading.Barrier(WORLD), [None] * WORLD
    engs, dps, shards = [], [], []
    for r in range(WORLD):
        e = GanEngine(cfg, ed_cfg, "cuda", B)
        e.load_state(S.PE, S.PG, S.BG, S.PD, S.PED, S.BED)
        e.seed(100 + r)
        shard = O.synthetic_batch(B, T, C, cfg["LATENT_DIM"], 6, 70 + r)
        with torch.cuda.stream(e.stream):
            e.set_batch(*(t.cuda() for t in shard))
            td = _ThreadDist(r, WORLD, barrier, slots)
            dp = DataParallel(e, WORLD, td, force_collectives=False, comm=_ThreadComm(td) if mode == "ingraph" else None)
            assert dp.active and dp.mode == mode
            dp.prepare(True)                 # dry steps: no rendezvous, so the ranks can be prepared one after the other
        assert (e.capture_locked or mode == "ingraph") and int(e.rng_step.item()) == 0 and float(e.D.state[0].item()) == 0.0
        engs.append(e); dps.append(dp); shards.append(shard)
    for k in S.PD:
        assert torch.equal(engs[0].D.p[k].cpu(), S.PD[k]) and torch.equal(engs[1].D.p[k].cpu(), S.PD[k])   # prepare() restored
    errors = []

    def rank_main(r):
        try:
            with torch.cuda.stream(engs[r].stream):
                dps[r].broadcast_params()
                # ingraph over the thread stand-in: eager (a Python rendezvous cannot be a graph node); RCCL's are captured
                # in test_rccl_collectives_are_graph_nodes_and_the_ingraph_step_equals_the_single_gpu_step
                dps[r].step(mode != "ingraph", g_step=True)
                torch.cuda.current_stream().synchronize()
        except Exception as ex:                  # noqa: BLE001
            errors.append(ex)
            barrier.abort()
    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(WORLD)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errors, errors
    torch.cuda.synchronize()
    e0, e1 = engs
    assert torch.equal(e0.D.data, e1.D.data) and torch.equal(e0.GE.data, e1.GE.data)          # replicas stay replicas
    assert torch.equal(e0.D.grad, e1.D.grad)
    assert not torch.equal(e0.noise_d, e1.noise_d)                                             # each rank its own draws
    # emulation: the oracle on each shard with the randoms that rank drew, gradients averaged, one Adam step each
    gd, gg = [], []
    keep = lambda m: (m > 0).float().cpu()  # noqa: E731
    Sd = O.build_gan_state(cfg, ed_cfg, "closed_form", d_scale=6.0)
    for e, (real, numeric, latent, emot) in zip(engs, shards):
        Sr = O.build_gan_state(cfg, ed_cfg, "closed_form", d_scale=6.0)
        rd = O.d_step(Sr, real, latent, numeric, e.noise_d.cpu(), e.alpha.cpu().view(-1, 1, 1), [keep(m) for m in e.dmask_d])
        gd.append(rd["grads"])
    mean_d = {k: sum(g[k] for g in gd) / WORLD for k in gd[0]}
    Sd.opt_D.step(Sd.PD, mean_d)                                   # the critic every rank holds after C1 + d_update
    for e, (real, numeric, latent, emot) in zip(engs, shards):
        Sr = O.build_gan_state(cfg, ed_cfg, "closed_form", d_scale=6.0)
        for k in Sr.PD:
            Sr.PD[k].copy_(Sd.PD[k])
        rg = O.g_step(Sr, latent, numeric, emot, e.noise.cpu(), [keep(m) for m in e.dmask])
        gg.append(rg["grads"])
    mean_g = {k: sum(g[k] for g in gg) / WORLD for k in gg[0]}
    for k, ref in mean_d.items():
        if k in ("real_fake.bias", "fc.1.bias"):
            continue
        got = e0.D.g[k].cpu() / WORLD
        if k == "real_fake.weight":
            got, ref = got[:, :256], ref[:, :256]
        assert rel_err(got, ref) < 2e-3, (mode, "D", k, rel_err(got, ref))
    for k, ref in mean_g.items():
        if k in ("G.decoder.deconv.0.bias", "G.decoder.deconv.3.bias"):
            continue
        assert rel_err(e0.GE.g[k].cpu() / WORLD, ref) < 5e-3, (mode, "GE", k, rel_err(e0.GE.g[k].cpu() / WORLD, ref))
    # first Adam step on the averaged gradient: -lr * g / (|g| + eps) wherever the gradient is well-conditioned
    for fp, mean, P0, lr in ((e0.D, mean_d, S.PD, e0.lr_d), (e0.GE, mean_g, S.PGE, e0.lr_g)):
        for k, ref in mean.items():
            if k in ("G.decoder.deconv.0.bias", "G.decoder.deconv.3.bias", "real_fake.bias", "real_fake.weight", "fc.1.bias"):
                continue                # zero-gradient parameters: rounding noise (tests/test_engine_gpu.py)
            mask = ref.abs() >= 0.1 * ref.pow(2).mean().sqrt()
            upd = fp.p[k].cpu() - P0[k]
            want = -lr * ref / (ref.abs() + 1e-8)
            assert float((upd - want)[mask].abs().max()) <= 2e-2 * lr, (mode, k)


def test_bench_runs_to_completion_on_two_ranks():
    """bench.py's N > 1 path end to end (two ranks sharing this GPU over gloo -- the control path, not the speed): every
    leg that only rank 0 runs must be free of collectives.  Round 2 had the roofline leg step through the data-parallel
    wrapper on rank 0 alone, which left rank 0 waiting in an all-reduce the other rank never joined."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MELO_SHARE_GPU="1", MELO_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29571", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2",
           "--profile-steps", "2", "--no-cpu-baseline", "--full"]
    out = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=240)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{"metric"')]
    assert out.returncode == 0 and len(lines) == 1, out.stderr[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["value"] > 0 and d["roofline"] is not None
