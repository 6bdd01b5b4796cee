"""The classifier's staged training step (EdEngine.step_staged: stage + augment -> mask draw -> forward / backward -> AdamW ->
metrics in one capturable sequence) and the trainers that use the device-side data plane."""
import math
import os

import pytest
import torch

from oracle import melo_oracle as O

pytestmark = pytest.mark.gpu

SIZES = [260, 228, 213, 196]          # the reference's training split, per class


def ed_cfg(C=4, **kw):
    return dict(O.default_ed_cfg(C), dropout=0.2, optimizer=dict(name="AdamW", lr=1e-3, betas=[0.5, 0.999], weight_decay=0.01), **kw)


def fresh_engine(cfg, B, T, seed=3):
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd.emotion_discriminator.engine import EdEngine
    eng = EdEngine(cfg, "cuda", B, T)
    eng.init_weights(seed)
    return eng


def snapshot(eng):
    torch.cuda.synchronize()
    s = {"data": eng.P.data, "m": eng.P.m, "v": eng.P.v, "state": eng.P.state, "rng_step": eng.rng_step}
    s.update({"buf." + k: v for k, v in eng.buf.items()})
    return {k: v.clone() for k, v in s.items()}


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("C", [4, 128])
def test_staged_epochs_with_everything_off_are_the_host_loop_bit_for_bit(use_graph, C):
    """n = 2B + 3, augmentation and sampler off: epochs by the staged step leave bit-identical parameters, Adam moments,
    BatchNorm buffers and step counters and return the same (loss, acc) as run_epoch's host path from the same generator
    state.  Three epochs, so that under use_graph the eager, the capturing and the replayed launch of the full and of the
    tail engine are all compared."""
    from melo_gan_amd.emotion_discriminator import train_ed
    B, T = 8, 32
    n = 2 * B + 3
    g = torch.Generator().manual_seed(21)
    x = (torch.rand(n, T, C, generator=g) * 2 - 1).cuda()
    y = torch.randint(0, 4, (n,), generator=g).cuda()
    host, staged = fresh_engine(ed_cfg(C), B, T), fresh_engine(ed_cfg(C), B, T)
    staged.attach_split(x, y)
    gen_h, gen_s = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    for epoch in range(3):
        with torch.cuda.stream(host.stream):
            want = train_ed.run_epoch(host, x, y, True, use_graph, gen_h)
        with torch.cuda.stream(staged.stream):
            got = train_ed.run_epoch_staged(staged, epoch, use_graph, gen_s)
        assert got == want, (epoch, got, want)
        a, b = snapshot(host), snapshot(staged)
        for k in a:
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), (epoch, k)
    assert float(staged.P.state[0].item()) == 9.0 and int(staged.rng_step.item()) == 9
    assert torch.equal(gen_h.get_state(), gen_s.get_state())
    if use_graph:
        assert not isinstance(staged._graphs["step_staged"], str) and not isinstance(staged.tail(3)._graphs["step_staged"], str)


def test_set_lr_reaches_the_staged_training_step():
    """The twin of test_set_lr_reaches_the_one_graph_training_step: the rate is baked into the captured 'step_staged' graph,
    so set_lr must drop it -- with lr = 0 the eager, the captured and the replayed step leave every parameter untouched while
    the cursor still advances."""
    B, T, C = 8, 32, 4
    eng = fresh_engine(ed_cfg(C), B, T)
    g = torch.Generator().manual_seed(5)
    n = 10 * B
    x = (torch.rand(n, T, C, generator=g) * 2 - 1).cuda()
    y = (torch.arange(n) % 4).cuda()
    eng.attach_split(x, y)
    staged_labels = []
    with torch.cuda.stream(eng.stream):
        eng.set_epoch(torch.arange(n), 0)
        for _ in range(3):                       # eager warm-up, capture, replay
            eng.run("step_staged")
            staged_labels.append(eng.y.clone())
        torch.cuda.synchronize()
        assert not isinstance(eng._graphs["step_staged"], str)
        before = eng.P.data.clone()
        eng.run("step_staged")
        staged_labels.append(eng.y.clone())
        torch.cuda.synchronize()
        assert not torch.equal(before, eng.P.data)
        eng.set_lr(0.0)
        assert "step_staged" not in eng._graphs
        before = eng.P.data.clone()
        for _ in range(3):                       # eager, capture, replay -- all with lr = 0
            eng.run("step_staged")
            staged_labels.append(eng.y.clone())
        torch.cuda.synchronize()
        assert torch.equal(before, eng.P.data)
        assert not isinstance(eng._graphs["step_staged"], str)
    assert float(eng.P.state[0].item()) == 7.0 and int(eng.rng_step.item()) == 7
    for k, lab in enumerate(staged_labels):      # the cursor moved on through all seven steps
        assert torch.equal(lab, y[k * B:(k + 1) * B]), k
        assert torch.equal(eng.x, x[6 * B:7 * B])
    assert eng.metrics[1].item() >= 0 and math.isfinite(eng.metrics[0].item())


def test_staged_step_needs_a_split_and_tails_share_it():
    eng = fresh_engine(ed_cfg(4), 8, 32)
    with pytest.raises(ValueError):
        eng.step_staged()
    with pytest.raises(ValueError):
        eng.set_epoch(None, 0)
    with pytest.raises(ValueError):
        eng.attach_split(torch.zeros(5, 16, 4, device="cuda"), torch.zeros(5, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        eng.tail(3).attach_split(torch.zeros(5, 32, 4, device="cuda"), torch.zeros(5, dtype=torch.int64, device="cuda"))


def unbalanced_split(T, C, seed):
    from melo_gan_amd.emotion_discriminator import train_ed
    x, _ = train_ed.synthetic_split(sum(SIZES), T, C, seed, "cuda")
    y = torch.cat([torch.full((k,), c, dtype=torch.int64) for c, k in enumerate(SIZES)])
    return x, y[torch.randperm(len(y), generator=torch.Generator().manual_seed(seed))].cuda()


def test_the_sampler_balances_the_labels_actually_trained_on(monkeypatch):
    """Class sizes in the reference's proportions (260 / 228 / 213 / 196): with use_weighted_sampler the labels the step
    trains on have shares within 5 standard errors of 1/4; without it every epoch trains on the split exactly once."""
    from melo_gan_amd import ops
    from melo_gan_amd.emotion_discriminator import train_ed
    from melo_gan_amd.emotion_discriminator.engine import EdEngine
    B, T, C = 64, 8, 4
    x, y = unbalanced_split(T, C, 2)
    n = len(y)
    seen = []
    real = EdEngine.step_staged

    def recording(self):
        real(self)
        seen.append(self.y.clone())
    monkeypatch.setattr(EdEngine, "step_staged", recording)
    eng = fresh_engine(ed_cfg(C), B, T)
    eng.attach_split(x, y, ops.augment_spec("ed", 42, noise_std=0.01, dropout_prob=0.05, pitch_shift_prob=0.1))
    gen = torch.Generator().manual_seed(0)
    with torch.cuda.stream(eng.stream):
        for epoch in range(2):
            seen.clear()
            train_ed.run_epoch_staged(eng, epoch, False, gen)
            torch.cuda.synchronize()
            assert torch.equal(torch.bincount(torch.cat(seen), minlength=4).cpu(), torch.tensor(SIZES))
        seen.clear()
        cdf = ops.sampler_cdf(y)
        epochs = 40
        for epoch in range(epochs):
            train_ed.run_epoch_staged(eng, epoch, False, gen, cdf)
        torch.cuda.synchronize()
    lab = torch.cat(seen)
    N = epochs * n
    assert lab.numel() == N
    bound = 5 * math.sqrt(0.25 * 0.75 / N)
    shares = (torch.bincount(lab, minlength=4).double() / N).tolist()
    print("shares with the sampler:", [f"{s:.4f}" for s in shares], f"bound {bound:.4f}; split:", [f"{k / n:.4f}" for k in SIZES])
    assert all(abs(s - 0.25) <= bound for s in shares), shares
    assert abs(SIZES[0] / n - 0.25) > 2 * bound          # the bound tells the balanced order from the split's own shares


def test_trainer_with_augmentation_and_sampler_on(tmp_path, capsys):
    """train_ed.train on the learnable synthetic split with all three augmentations and the weighted sampler: finishes, the
    validation loss falls well below ln 4 (the existing trainer test's criterion), the checkpoint loads into GanEngine."""
    from melo_gan_amd.emotion_discriminator import train_ed
    from melo_gan_amd.gan import train_gan
    from melo_gan_amd.gan.engine import GanEngine
    cfg = dict(O.default_ed_cfg(4), dropout=0.2, batch_size=32, max_notes=32, num_epochs=8, seed=1,
               optimizer=dict(name="AdamW", lr=2e-3, betas=[0.5, 0.999], weight_decay=0.0),
               scheduler=dict(name="ReduceLROnPlateau", mode="min", factor=0.5, patience=1, threshold=1e-4),
               metric_for_best="val_loss", early_stopping_patience=10, save_freq=4,
               checkpoint_dir=str(tmp_path), save_name="ed_best.pth",
               augment=True, augment_cfg=dict(noise_std=0.01, dropout_prob=0.05, pitch_shift_prob=0.1),
               use_weighted_sampler=True, preload=True)
    eng, best = train_ed.train(cfg, synthetic=500, use_graph=True)            # 500 = 15 * 32 + 20: a tail batch too
    out = capsys.readouterr().out
    assert "Using WeightedRandomSampler: classes={" in out and "samples=500" in out
    assert best < 1.0, best
    assert not isinstance(eng._graphs["step_staged"], str) and not isinstance(eng.tail(20)._graphs["step_staged"], str)
    ck = torch.load(os.path.join(str(tmp_path), "ed_best.pth"), map_location="cpu", weights_only=False)
    assert set(ck) == {"epoch", "model", "optimizer", "cfg"} and ck["cfg"]["augment_cfg"]["dropout_prob"] == 0.05
    gan = GanEngine(O.default_gan_cfg(4, 32, 4), O.default_ed_cfg(4), "cuda", 4)
    gan.init_weights(0)
    assert train_gan.load_ed_checkpoint(gan, os.path.join(str(tmp_path), "ed_best.pth"))
    for k in gan.ED.spec:
        assert torch.equal(gan.ED.p[k].cpu(), ck["model"][k]), k


def _ae_cfg(tmp_path, **augment):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(__file__), "..", "config", "ae_config.yaml")))
    cfg.update(MAX_NOTES=32, BATCH_SIZE=8, EPOCHS=2, CHECKPOINT_DIR=str(tmp_path / "ck"), LOG_DIR=str(tmp_path / "log"))
    cfg["AUGMENT"] = dict(cfg["AUGMENT"], **augment)
    p = tmp_path / "ae.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return cfg, str(p)


def test_ae_trainer_augments_its_training_batches_on_the_device(tmp_path, monkeypatch):
    from melo_gan_amd import ops
    from melo_gan_amd.ae import train_ae
    _, path = _ae_cfg(tmp_path, tempo_jitter=0.07, pitch_shift=1, note_dropout=0.03, velocity_jitter=0.1, timing_jitter=0.02)
    real, calls = ops.stage_augment, []

    def recording(notes, labels, notes_out, labels_out, n_rows, order, order_len, counter, base, serial_base, aug, last=False):
        real(notes, labels, notes_out, labels_out, n_rows, order, order_len, counter, base, serial_base, aug, last=last)
        k = int(counter.item()) - int(base.item())
        plain = notes.index_select(0, order[k * n_rows:(k + 1) * n_rows])
        touched = (notes_out != plain).flatten(1).any(dim=1)
        calls.append((int(serial_base.item()), k, int(touched.sum()), bool(torch.isfinite(notes_out).all())))
    monkeypatch.setattr(ops, "stage_augment", recording)
    train_ae.main(["--config", path, "--synthetic", "32"])
    assert [(s, k) for s, k, _, _ in calls] == [(0, 0), (0, 1), (0, 2), (0, 3), (32, 0), (32, 1), (32, 2), (32, 3)]
    assert all(fin for *_, fin in calls)
    assert sum(t for _, _, t, _ in calls) >= 16          # each sample passes at least one of five gates with odds 0.78
    final = torch.load(tmp_path / "ck" / "ae_final.pth", map_location="cpu")
    assert all(torch.isfinite(v.float()).all() for v in final.values())


def test_ae_trainer_with_the_committed_all_zero_block_never_launches_the_kernel(tmp_path, monkeypatch):
    from melo_gan_amd import ops
    from melo_gan_amd.ae import train_ae
    cfg, path = _ae_cfg(tmp_path)
    assert set(cfg["AUGMENT"]) == set(ops.AUG_AE_KEYS) and not any(cfg["AUGMENT"].values())

    def boom(*a, **k):
        raise AssertionError("stage_augment launched with an all-zero AUGMENT block")
    monkeypatch.setattr(ops, "stage_augment", boom)
    train_ae.main(["--config", path, "--synthetic", "32"])
    assert os.path.exists(tmp_path / "ck" / "ae_final.pth")
