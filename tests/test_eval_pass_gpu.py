"""GPU: the resident-split pass under the three evaluators (melo_gan_amd/eval_pass.py).  A pass over split A (5 rows at batch 2:
three batches, the last one padded), then over split B (3 rows), then over A again: the second pass over A leaves the bits of
the first, the pass over B the bits a fresh evaluator leaves for B -- a pass's result does not depend on whether its graph was
new, nor on what the evaluator held before.  ops.Graph.capture is wrapped to count captures: a repeated pass captures nothing,
a changed split captures once per key, and a second EdEvaluator.robustness call with the same strengths captures nothing."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import ops  # noqa: E402

B, NA, NB = 2, 5, 3


@pytest.fixture
def captures(monkeypatch):
    """The number of ops.Graph.capture calls so far, as a one-element list."""
    count, capture = [0], ops.Graph.capture

    def counting(fn, *a, **kw):
        count[0] += 1
        return capture(fn, *a, **kw)

    monkeypatch.setattr(ops.Graph, "capture", staticmethod(counting))
    return count


def bits(arrays):
    return {k: np.ascontiguousarray(v).view(np.uint8).copy() for k, v in arrays.items()}


def same_bits(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


def aba(make, run, captures, per_key=1):
    """run(ev, split) -> the pass's bits.  A, A, B, A on one evaluator and B on a fresh one."""
    ev = make()
    assert captures[0] == 0
    a1 = run(ev, "A")
    assert captures[0] == per_key
    same_bits(run(ev, "A"), a1)
    assert captures[0] == per_key                                         # a repeated pass captures nothing
    b1 = run(ev, "B")
    assert captures[0] == 2 * per_key                                     # a changed split: once per key
    a2 = run(ev, "A")
    assert captures[0] == 3 * per_key
    same_bits(a2, a1)
    same_bits(run(make(), "B"), b1)
    return ev


def test_vae_evaluator_a_b_a(captures):
    from melo_gan_amd.ae.evaluate import VaeEvaluator
    from test_ae_evaluate_gpu import K, cfg_of, model
    T = 32
    P, Bf = model(T)
    notes = (torch.rand(NA + NB, T, 4, generator=torch.Generator().manual_seed(7)) * 2 - 1)
    labels = torch.arange(NA + NB, dtype=torch.int64) % K
    splits = {"A": (notes[:NA].cuda(), labels[:NA].cuda()), "B": (notes[NA:].cuda(), labels[NA:].cuda())}

    def make():
        ev = VaeEvaluator(cfg_of(T, B), "cuda", B)
        ev.eng.load_state(P, Bf)
        return ev

    def run(ev, which):
        x, y = splits[which]
        rep = ev.evaluate(x, y)
        assert rep["rows"] == x.shape[0]
        return bits({**ev.acc_host, **ev.rows, "mu": ev.mu.cpu().numpy(), "logvar": ev.logvar.cpu().numpy()})

    ev = aba(make, run, captures)
    assert tuple(ev.mu.shape) == (NA, ev.eng.latent) and ev.rows["row_i"].shape == (NA, 8)


def test_ed_evaluator_a_b_a_and_robustness_graphs(captures):
    from melo_gan_amd.emotion_discriminator.evaluate import EdEvaluator
    from test_ed_evaluate_gpu import K, T, notes_cfg, random_model
    cfg = notes_cfg(batch_size=B)
    P, Bf = random_model(cfg)
    x = torch.rand(NA + NB, T, 4, generator=torch.Generator().manual_seed(7)) * 2 - 1
    y = torch.arange(NA + NB, dtype=torch.int64) % K
    splits = {"A": (x[:NA].cuda(), y[:NA].cuda()), "B": (x[NA:].cuda(), y[NA:].cuda())}

    def make():
        ev = EdEvaluator(cfg, "cuda", B)
        ev.eng.load_state(P, Bf)
        return ev

    def run(ev, which):
        xs, ys = splits[which]
        rep = ev.evaluate(xs, ys)
        assert rep["rows"] == xs.shape[0] and int(ev.acc_host["rows"].sum()) == xs.shape[0]
        return bits({**ev.acc_host, **ev.rows, "pairs": ev.pairs, "logits": ev.logits.cpu().numpy(),
                     **{"cal_" + k: v for k, v in ev.calibrated_host.items()}})

    ev = aba(make, run, captures)
    assert tuple(ev.logits.shape) == (NA, K)
    # robustness: one graph per augmentation setting, kept across calls; the clean pass over A is the evaluator's last one
    n0 = captures[0]
    strengths = {"noise_std": 0.05, "dropout_prob": 0.1, "pitch_shift_prob": 0.5}
    r1 = ev.robustness(*splits["A"], strengths, repeats=2)
    assert captures[0] == n0 + 4 and list(r1["passes"]) == list(ops.AUG_ED_KEYS) + ["all"]
    aug1 = ev.aug_logits.cpu()
    r2 = ev.robustness(*splits["A"], strengths, repeats=2)
    assert captures[0] == n0 + 4                                          # the same strengths: nothing is captured
    assert r2 == r1 and torch.equal(ev.aug_logits.cpu(), aug1)            # and a new graph's eager run left no trace in r1
    assert all(p["rows"] == 2 * NA for p in r1["passes"].values())
    # a fresh evaluator, whose every robustness graph is new, reports the same
    fresh = make()
    assert fresh.robustness(*splits["A"], strengths, repeats=2) == r1
    # other strengths are other keys
    ev.robustness(*splits["A"], dict(strengths, noise_std=0.2), repeats=1)
    assert captures[0] == n0 + 4 + 2 + 5                                  # fresh: clean + 4; ev: noise_std alone and "all"


def test_gan_evaluator_with_music_a_b_a(captures, tmp_path):
    from melo_gan_amd.gan import evaluate as EV
    from melo_gan_amd.gan.dataset import GANDataset
    from oracle import melo_oracle as O
    from test_evaluate_gpu import gen_state, save_state
    T, C = 32, 4
    S, cfg, ed_cfg = gen_state(T, C, "warm_start", "notes")
    ck, ed = save_state(S, str(tmp_path))
    real, numeric, _, _ = O.synthetic_batch(NA + NB, T, C, cfg["LATENT_DIM"], 6, 7)
    labels = torch.arange(NA + NB) % 4
    cut = {"A": slice(0, NA), "B": slice(NA, NA + NB)}
    splits = {k: GANDataset(real[c].numpy(), labels[c].numpy(), numeric[c].numpy(), None, cfg["LATENT_DIM"], "cuda")
              for k, c in cut.items()}

    def make():
        ev = EV.Evaluator(cfg, ed_cfg, "cuda", B, music=True)
        ev.load_generator(ck)
        ev.load_critic(ck)
        ev.load_ed(ed)
        return ev

    reports = {}

    def run(ev, which):
        rep = ev.evaluate(splits[which], seed=3)
        assert rep["n"] == len(splits[which]) and "music" in rep
        assert reports.setdefault(which, rep) == rep                      # the report itself, value for value
        return bits({"acc": ev.acc.cpu().numpy(), "music_buf": ev.music_buf.buf.cpu().numpy()})

    ev = aba(make, run, captures)
    assert tuple(ev.note_row_i.shape) == (2, 3 * B, 8) and tuple(ev.note_row_beats.shape) == (2, 3 * B, 2)


def test_a_freed_label_array_cannot_pass_for_the_next_one():
    """The same rows with two label arrays that live only for their call: the pass keeps the arrays whose addresses make up
    its key, so the second array cannot take the first one's address, compare equal and be judged against the first labels."""
    from melo_gan_amd.ae.evaluate import VaeEvaluator
    from melo_gan_amd.emotion_discriminator.evaluate import EdEvaluator
    import test_ae_evaluate_gpu as A
    import test_ed_evaluate_gpu as E
    y1 = torch.arange(NA, dtype=torch.int64) % 4
    y2 = (y1 + 1) % 4
    assert torch.bincount(y1, minlength=4).tolist() != torch.bincount(y2, minlength=4).tolist()
    cfg = E.notes_cfg(batch_size=B)
    ed = EdEvaluator(cfg, "cuda", B)
    ed.eng.load_state(*E.random_model(cfg))
    vae = VaeEvaluator(A.cfg_of(E.T, B), "cuda", B)
    vae.eng.load_state(*A.model(E.T))
    x = (torch.rand(NA, E.T, 4, generator=torch.Generator().manual_seed(7)) * 2 - 1).cuda()
    for y in (y1, y2, y1):
        want = torch.bincount(y, minlength=4).tolist()
        ed.evaluate(x, y.cuda())                                          # the device copy dies with the call
        assert ed.acc_host["rows"].tolist() == want and ed.labels_host.tolist() == y.tolist()
        assert ed.pairs[2].tolist() == want                               # n_pos of the one-vs-rest counts: the same labels
        got = vae.evaluate(x, y.cuda())["per_class"]
        assert [got[k]["rows"] for k in got] == want and vae.acc_host["c"][:, 0].tolist() == want
    assert all(t.is_cuda for t in ed.split_pass.split.held) and len(vae.split_pass.split.held) == 2


def test_sampler_keeps_one_graph_and_a_new_seed_is_a_new_key(captures, tmp_path):
    """The Sampler on the cache: a seed is a launch argument the capture froze, so a new seed captures again (after one eager
    run, as every new key) and the old graph goes; the same seed captures nothing; a returning seed gives the same samples."""
    from melo_gan_amd.gan import generate as G
    from test_generate_gpu import gen_state, save_state
    S, cfg, ed_cfg = gen_state(16, 4, "conditioning", "latent")
    ck, ed = save_state(S, str(tmp_path))
    smp = G.Sampler(cfg, ed_cfg, "cuda", 8)
    smp.load_generator(ck)
    smp.load_ed(ed)
    first = smp.sample(["all"], 2, seed=3)
    assert captures[0] == 1 and list(smp.graphs) == [3]
    again = smp.sample(["all"], 2, seed=3)
    assert captures[0] == 1 and np.array_equal(again.notes, first.notes) and again.summary == first.summary
    other = smp.sample(["all"], 2, seed=4)
    assert captures[0] == 2 and list(smp.graphs) == [4] and not np.array_equal(other.notes, first.notes)
    back = smp.sample(["all"], 2, seed=3)
    assert captures[0] == 3 and list(smp.graphs) == [3]
    assert np.array_equal(back.notes, first.notes) and back.summary == first.summary
