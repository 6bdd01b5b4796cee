"""CPU: host-side logic that needs no GPU -- label validation, the plateau scheduler, DataParallel step orders live in
test_dp_cpu.py."""
import numpy as np
import pytest
import torch

import melo_gan_amd  # noqa: F401
from melo_gan_amd.gan.utils import check_labels, emotion_to_index


def test_check_labels_rejects_what_cross_entropy_would():
    ok = check_labels(torch.tensor([0, 3, 1, 2]), 4)
    assert ok.tolist() == [0, 3, 1, 2]
    for bad in ([0, -1, 2], [4], [0, 1, 100]):
        with pytest.raises(ValueError, match="outside"):
            check_labels(torch.tensor(bad), 4, "labels")
    # emotion_to_index (src/gan/utils.py:63-73) maps unknown names / None to -1: caught when the dataset is built
    idx = [emotion_to_index(e) for e in ("happy", "SAD", None, "bored", np.array([0, 0, 1, 0]), 3)]
    assert idx == [0, 1, -1, -1, 2, 3]
    with pytest.raises(ValueError, match="2 of 6"):
        check_labels(torch.tensor(idx), 4)


def test_plateau_matches_torch_reduce_lr_on_plateau():
    from melo_gan_amd.emotion_discriminator.train_ed import Plateau
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=1.0)
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=2, threshold=1e-4)
    mine, lr = Plateau("min", 0.5, 2, 1e-4), 1.0
    g = np.random.default_rng(0)
    for m in np.concatenate([np.linspace(2, 1, 5), 1 + 0.01 * g.random(12), np.linspace(0.9, 0.5, 4), 0.5 + 0.01 * g.random(9)]):
        sch.step(float(m))
        lr = mine.step(float(m), lr)
        assert lr == opt.param_groups[0]["lr"]


def test_optimizer_checkpoint_is_a_torch_adam_state_dict():
    """opt_G / opt_D of gan_epochNNNN.pth (reference train_gan.py:267-276) are `torch.optim.Adam.state_dict()`s of the
    reference's optimisers: a torch Adam over parameters of the same shapes, in the same order, loads them as they are --
    and the flat buffers take them back (resume)."""
    import torch
    from collections import OrderedDict
    from melo_gan_amd.gan.engine import FlatParams
    from melo_gan_amd.checkpoints import adam_state_dict, load_adam_state_dict
    spec = OrderedDict([("a.weight", (3, 4)), ("a.bias", (3,)), ("b.weight", (2, 3, 5))])
    fp = FlatParams(spec, "cpu", first="b.weight")           # flat order differs from the spec's order on purpose
    g = torch.Generator().manual_seed(0)
    fp.m.copy_(torch.randn(fp.m.shape, generator=g))
    fp.v.copy_(torch.rand(fp.v.shape, generator=g))
    fp.state[0] = 7.0
    sd = adam_state_dict(fp, 2e-4, (0.5, 0.9))
    params = [torch.nn.Parameter(torch.zeros(s)) for s in spec.values()]
    opt = torch.optim.Adam(params, lr=1.0, betas=(0.1, 0.2))
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == 2e-4 and tuple(opt.param_groups[0]["betas"]) == (0.5, 0.9)
    for i, k in enumerate(spec):
        off, n = fp.offsets[k]
        assert torch.equal(opt.state[params[i]]["exp_avg"], fp.m[off:off + n].view(spec[k]))
        assert torch.equal(opt.state[params[i]]["exp_avg_sq"], fp.v[off:off + n].view(spec[k]))
        assert float(opt.state[params[i]]["step"]) == 7.0
    fp2 = FlatParams(spec, "cpu", first="b.weight")
    load_adam_state_dict(fp2, opt.state_dict())
    assert torch.equal(fp2.m[:fp.n], fp.m[:fp.n]) and torch.equal(fp2.v[:fp.n], fp.v[:fp.n])
    assert float(fp2.state[0]) == 7.0 and abs(float(fp2.state[1]) - 0.5 ** 7) < 1e-15 and abs(float(fp2.state[2]) - 0.9 ** 7) < 1e-15


def test_optimizer_state_dict_is_validated_on_load():
    """A partial or mismatched optimiser checkpoint must fail with a message, not restore a wrong step silently."""
    import pytest
    import torch
    from collections import OrderedDict
    from melo_gan_amd.gan.engine import FlatParams
    from melo_gan_amd.checkpoints import adam_state_dict, load_adam_state_dict
    spec = OrderedDict([("a.weight", (3, 4)), ("a.bias", (3,))])
    fp = FlatParams(spec, "cpu")
    fp.state[0] = 3.0
    good = adam_state_dict(fp, 1e-4, (0.5, 0.9))
    sd = {"state": {0: good["state"][0]}, "param_groups": good["param_groups"]}
    with pytest.raises(ValueError, match="parameter entries"):
        load_adam_state_dict(fp, sd)
    sd = adam_state_dict(fp, 1e-4, (0.5, 0.9))
    sd["state"][1]["exp_avg"] = torch.zeros(4)
    with pytest.raises(ValueError, match="shape"):
        load_adam_state_dict(fp, sd)
    sd = adam_state_dict(fp, 1e-4, (0.5, 0.9))
    sd["state"][1]["step"] = torch.tensor(9.0)
    with pytest.raises(ValueError, match="step counts differ"):
        load_adam_state_dict(fp, sd)
    fp.m.fill_(1.0)
    load_adam_state_dict(fp, {"state": {}, "param_groups": good["param_groups"]})       # never stepped: fresh moments
    assert float(fp.m.abs().sum()) == 0.0 and float(fp.state[0]) == 0.0


def test_spectral_norm_checkpoint_weights_fold_at_load():
    """A frozen emotion discriminator trained with use_spectral_norm (ed_model.py:29-32): the weight its eval-mode forward
    uses is weight_orig / (u^T W v); checkpoints.spectral_norm_weight reproduces what torch's wrapper computes."""
    import torch
    from melo_gan_amd.checkpoints import spectral_norm_weight
    torch.manual_seed(0)
    conv = torch.nn.utils.spectral_norm(torch.nn.Conv1d(4, 8, 5, padding=2))
    lin = torch.nn.utils.spectral_norm(torch.nn.Linear(6, 3))
    for m in (conv, lin):                     # a few training-mode forwards move u / v, as training would
        m.train()
        for _ in range(3):
            m(torch.randn(2, 4, 16) if m is conv else torch.randn(2, 6))
        m.eval()
        m(torch.randn(2, 4, 16) if m is conv else torch.randn(2, 6))        # eval forward: sets .weight from the stored u, v
        sd = {"x." + k: v for k, v in m.state_dict().items()}
        got = spectral_norm_weight(sd, "x.weight")
        torch.testing.assert_close(got, m.weight.detach(), rtol=1e-6, atol=1e-7)
    assert spectral_norm_weight({"x.weight": torch.ones(2)}, "x.weight").sum() == 2 and spectral_norm_weight({}, "x.weight") is None


def test_run_graphed_goes_eager_then_captures_then_replays():
    """ops.run_graphed, the one copy of the training engines' None -> "warm" -> captured step, with a stand-in capture: the
    dict keeps the format bench.py and the tests read ("warm", then the graph -- or, for an engine with host state, a tuple
    led by it that launches and counts kernel nodes like it)."""
    from melo_gan_amd import ops

    for host in (None, FakeHost()):
        graphs, calls, g = {}, [], FakeGraph()
        wrap = (lambda g: g) if host is None else (lambda g: (g, (False,), (0, 0)))

        def capture(fn):
            calls.append("capture")
            return g

        fn = lambda: calls.append("eager")  # noqa: E731
        assert ops.run_graphed(graphs, "k", fn, host, capture) is None and graphs == {"k": "warm"} and calls == ["eager"]
        for n in (1, 2, 3):
            assert ops.run_graphed(graphs, "k", fn, host, capture) is graphs["k"] and graphs["k"] == wrap(g) and g.launches == n
            assert graphs["k"].kernel_nodes == 7 and (host is None or isinstance(graphs["k"], tuple))
        assert calls == ["eager", "capture"]
        # a capture that raises leaves the key warm: the next call captures again
        graphs["j"] = "warm"
        with pytest.raises(RuntimeError):
            ops.run_graphed(graphs, "j", fn, host, lambda f: (_ for _ in ()).throw(RuntimeError("locked")))
        assert graphs["j"] == "warm"


class FakeGraph:
    launches, kernel_nodes = 0, 7

    def launch(self):
        self.launches += 1


class FakeHost:
    """The engines' side of ops.run_graphed: one flag and two counters."""

    def __init__(self):
        self.flag, self.n, self.updates = False, 0, 0

    def host_state(self):
        return (self.flag,), (self.n, self.updates)

    def set_host_state(self, flags, counters):
        (self.flag,), (self.n, self.updates) = flags, counters


def fake_capture(fn):
    """ops.Graph.capture as far as the host sees it: fn's Python runs once, nothing is launched."""
    fn()
    return FakeGraph()


def test_run_graphed_replays_the_host_effects_of_the_capture():
    """A captured entry carries what its sub-step's Python did to the host state during the capture and a replay re-applies
    exactly that: after an eager call, the capturing call and three replays the state is what five eager calls leave, call by
    call -- the capturing call adds nothing of its own (the counter moves by 1, never 2)."""
    from melo_gan_amd import ops
    graphs, host, eager = {}, FakeHost(), FakeHost()

    def sub_step(h):
        h.flag = not h.flag
        h.n += 1
        h.updates += 3

    def draw(h):
        h.flag = "nobump"

    for call in range(5):
        for h, run in ((eager, lambda name, fn: fn()), (host, lambda name, fn: ops.run_graphed(graphs, name, fn, host, fake_capture))):
            h.flag = False
            run("step", lambda: sub_step(h))          # arrives plain, leaves the flag set
            assert h.host_state() == ((True,), (2 * call + 1, 6 * call + 3)), (call, h is host)
            run("step", lambda: sub_step(h))          # the same name arriving with the flag pending: a graph of its own
            run("draw", lambda: draw(h))
        assert host.host_state() == eager.host_state() == (("nobump",), (2 * call + 2, 6 * call + 6)), call
    assert set(graphs) == {"step", "step#True", "draw"} and all(k.split("#")[0] in ("step", "draw") for k in graphs)
    assert all(g.launches == 4 for g, _, _ in graphs.values())
    assert graphs["step"][1:] == ((True,), (1, 3)) and graphs["step#True"][1:] == ((False,), (1, 3))
    assert graphs["draw"][1:] == (("nobump",), (0, 0))
    # a capture that raises: the key stays warm and the state is as fn left it
    host.flag = "nobump"
    ops.run_graphed(graphs, "late", lambda: sub_step(host), host, fake_capture)
    assert graphs["late#nobump"] == "warm" and host.host_state() == ((False,), (11, 33))

    def refuse(fn):
        fn()
        raise RuntimeError("locked")
    host.flag = "nobump"
    with pytest.raises(RuntimeError):
        ops.run_graphed(graphs, "late", lambda: sub_step(host), host, refuse)
    assert graphs["late#nobump"] == "warm" and host.host_state() == ((False,), (12, 36))


def test_set_lr_drops_the_graphs_whose_capture_saw_an_update():
    """EdEngine.set_lr on stand-in entries: exactly the captured graphs whose record holds an optimiser step go -- by the
    record, whatever the key -- and a tail engine follows."""
    import types
    from melo_gan_amd import ops
    from melo_gan_amd.emotion_discriminator.engine import EdEngine
    entry = lambda updates: ops.Captured(FakeGraph(), (False,), (updates,))  # noqa: E731
    tail = types.SimpleNamespace(_graphs={"step_staged": entry(1), "forward_eval": entry(0)}, _tails={})
    tail.set_lr = lambda lr: EdEngine.set_lr(tail, lr)
    eng = types.SimpleNamespace(_tails={3: tail}, _graphs={
        "step_rng": entry(1), "update#True": entry(1), "anything": entry(2), "backward_rng": entry(0), "forward_eval": entry(0),
        "update": "warm"})
    EdEngine.set_lr(eng, 0.5)
    assert eng.lr == tail.lr == 0.5
    assert set(eng._graphs) == {"backward_rng", "forward_eval", "update"} and set(tail._graphs) == {"forward_eval"}


def test_graph_cache_rules(monkeypatch):
    """eval_pass.GraphCache (under the Sampler and the three evaluators) with a stand-in for ops.Graph.capture: a key seen
    for the first time runs eagerly once in front of its capture; a key that holds is not touched, a returning one included;
    clear() forgets every graph.  A capture that raises stores nothing: the keys before it stand, the next call captures
    again."""
    from melo_gan_amd import ops
    from melo_gan_amd.eval_pass import GraphCache
    log = []
    monkeypatch.setattr(ops.Graph, "capture", staticmethod(lambda fn: (log.append("capture"), fn(), object())[-1]))
    c = GraphCache()
    launches = lambda: log.append("launch")  # noqa: E731
    g1 = c.graph(1, launches)
    assert c.graph(1, launches) is g1
    g2 = c.graph(2, launches)
    assert g2 is not g1 and c.graph(2, launches) is g2
    assert c.graph(1, launches) is g1 and 1 in c and 2 in c and 3 not in c
    assert log == ["launch", "capture", "launch", "launch", "capture", "launch"], log

    def fail():
        raise RuntimeError("capture failed")
    with pytest.raises(RuntimeError):
        c.graph(3, fail)
    assert 3 not in c and c.graph(1, launches) is g1 and c.graph(2, launches) is g2
    del log[:]
    monkeypatch.setattr(ops.Graph, "capture", staticmethod(lambda fn: (_ for _ in ()).throw(RuntimeError("locked"))))
    with pytest.raises(RuntimeError):
        c.graph(3, launches)                      # the eager run passed, the capture itself refused
    assert log == ["launch"] and 3 not in c and c.graph(1, launches) is g1
    monkeypatch.setattr(ops.Graph, "capture", staticmethod(lambda fn: (log.append("capture"), fn(), object())[-1]))
    c.clear()
    assert 1 not in c and c.graph(1, launches) not in (g1, g2)
    assert log == ["launch", "launch", "capture", "launch"], log
