"""CPU-only checks of the augmentation / weighted-sampler data plane: the three entry points reject bad arguments before any
launch (so no GPU is needed), and the trainers validate the config blocks (ed_config.yaml: augment, augment_cfg,
use_weighted_sampler; ae_config.yaml: AUGMENT) before the GPU is touched."""
import ctypes as C

import pytest
import torch


def _lib():
    import __graft_entry__ as ge
    ge.build()
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import _lib
    return _lib, _lib.load()


def _stage_args(L, **over):
    """A well-formed mg_stage_augment call on dummy (never dereferenced: every case below is rejected) addresses."""
    aug = L.Augment()
    aug.program = L.AUG_ED
    a = dict(notes=256, labels=512, src_rows=8, T=16, note_dim=4, notes_out=1024, labels_out=2048, n_rows=4, order=4096,
             order_len=8, counter=8192, base=8200, serial_base=8208, rule=L.STAGE_BATCH, aug=aug)
    for k, v in over.items():
        if hasattr(aug, k):
            setattr(aug, k, v)
        else:
            a[k] = v
    return [a["notes"], a["labels"], a["src_rows"], a["T"], a["note_dim"], a["notes_out"], a["labels_out"], a["n_rows"],
            a["order"], a["order_len"], a["counter"], a["base"], a["serial_base"], a["rule"], C.byref(a["aug"]), None]


@pytest.mark.parametrize("over,word", [
    (dict(notes=None), b"notes"),
    (dict(notes_out=None), b"notes_out"),
    (dict(labels_out=None), b"labels"),
    (dict(src_rows=0), b"src_rows"),
    (dict(n_rows=0), b"n_rows"),
    (dict(n_rows=65536), b"n_rows"),
    (dict(order_len=0), b"order_len"),
    (dict(order=None, order_len=9), b"order_len"),
    (dict(T=0), b"row bytes"),
    (dict(note_dim=6), b"row bytes"),
    (dict(notes=260), b"aligned"),
    (dict(rule=2), b"rule"),
    (dict(counter=None), b"counter"),
    (dict(rule=1, n_rows=9, order_len=8, src_rows=16), b"n_rows <= order_len"),
    (dict(program=2), b"program"),
    (dict(dropout_prob=1.5), b"dropout_prob"),
    (dict(dropout_prob=float("nan")), b"dropout_prob"),
    (dict(pitch_shift_prob=-0.1), b"pitch_shift_prob"),
    (dict(note_dropout=2.0), b"note_dropout"),
    (dict(noise_std=-1.0), b"noise_std"),
    (dict(tempo_jitter=-0.5), b"tempo_jitter"),
    (dict(velocity_jitter=float("inf")), b"velocity_jitter"),
    (dict(timing_jitter=-1e-3), b"timing_jitter"),
    (dict(pitch_shift=-1), b"pitch_shift"),
])
def test_stage_augment_rejects_bad_arguments_before_any_launch(over, word):
    L, lib = _lib()
    assert lib.mg_stage_augment(*_stage_args(L, **over)) == -1
    assert word in lib.mg_last_error(), lib.mg_last_error()


def test_stage_augment_null_aug_is_rejected():
    L, lib = _lib()
    args = _stage_args(L)
    args[14] = None
    assert lib.mg_stage_augment(*args) == -1 and b"aug" in lib.mg_last_error()


def test_weighted_order_and_metrics_reject_bad_arguments_before_any_launch():
    L, lib = _lib()
    assert lib.mg_version() >= 102
    for args, word in (((None, 4, 256, 4, 1, 0, None), b"cdf"), ((256, 4, None, 4, 1, 0, None), b"order"),
                       ((256, 0, 512, 4, 1, 0, None), b"n must"), ((256, -3, 512, 4, 1, 0, None), b"n must"),
                       ((256, 4, 512, 0, 1, 0, None), b"m must"), ((256, 4, 512, -1, 1, 0, None), b"m must")):
        assert lib.mg_weighted_order(*args) == -1 and word in lib.mg_last_error(), (args, lib.mg_last_error())
    good = [256, 512, 1024, 8, 4, 2048, None]
    for i, word in ((0, b"logits"), (1, b"labels"), (2, b"loss"), (5, b"acc")):
        a = list(good)
        a[i] = None
        assert lib.mg_ed_metrics_acc(*a) == -1 and word in lib.mg_last_error(), (i, lib.mg_last_error())
    for i, v, word in ((3, 0, b"rows"), (3, -2, b"rows"), (4, 0, b"n_classes")):
        a = list(good)
        a[i] = v
        assert lib.mg_ed_metrics_acc(*a) == -1 and word in lib.mg_last_error(), (i, v, lib.mg_last_error())


def test_ed_config_validation_happens_before_the_gpu_is_touched():
    L, _ = _lib()
    from melo_gan_amd.emotion_discriminator import train_ed
    base = dict(input_mode="notes", seed=7)
    assert train_ed.augment_from_cfg(base) is None
    assert train_ed.augment_from_cfg(dict(base, augment=False, augment_cfg=dict(bogus=1.0))) is None      # off: the block is not read
    a = train_ed.augment_from_cfg(dict(base, augment=True, augment_cfg=dict(noise_std=0.01, dropout_prob=0.05, pitch_shift_prob=0.3)))
    assert a.program == L.AUG_ED and a.seed == 7
    assert (a.noise_std, a.dropout_prob, a.pitch_shift_prob) == tuple(C.c_float(v).value for v in (0.01, 0.05, 0.3))
    a = train_ed.augment_from_cfg(dict(base, augment=True))            # switched on with no block: every step off
    assert (a.noise_std, a.dropout_prob, a.pitch_shift_prob) == (0.0, 0.0, 0.0)
    bad = [dict(bogus=0.1), dict(noise_std=-0.01), dict(dropout_prob=1.01), dict(dropout_prob=-0.2), dict(pitch_shift_prob=1.5),
           dict(noise_std=float("nan")), dict(noise_std=float("inf")), dict(noise_std="a lot"), dict(tempo_jitter=0.1)]
    for acfg in bad:
        with pytest.raises(ValueError):
            train_ed.augment_from_cfg(dict(base, augment=True, augment_cfg=acfg))
        with pytest.raises(ValueError):        # train() itself: before the device check and before any allocation
            train_ed.train(dict(base, augment=True, augment_cfg=acfg), synthetic=8)
    with pytest.raises(ValueError):
        train_ed.augment_from_cfg(dict(base, augment=True, augment_cfg=[0.1]))


def test_ae_config_validation_happens_before_the_gpu_is_touched():
    L, _ = _lib()
    from melo_gan_amd.ae import train_ae
    zero = dict(tempo_jitter=0.0, pitch_shift=0, note_dropout=0.0, velocity_jitter=0.0, timing_jitter=0.0)
    assert train_ae.augment_from_cfg({}) is None and train_ae.augment_from_cfg(dict(AUGMENT=zero)) is None
    a = train_ae.augment_from_cfg(dict(AUGMENT=dict(zero, tempo_jitter=0.07, pitch_shift=1, note_dropout=0.03, velocity_jitter=8.0,
                                                    timing_jitter=0.02)), seed=3)
    assert a.program == L.AUG_AE and a.pitch_shift == 1 and a.seed == 3 and a.velocity_jitter == 8.0
    assert train_ae.augment_from_cfg(dict(AUGMENT=dict(pitch_shift=2))).pitch_shift == 2           # missing keys are 0
    bad = [dict(zero, bogus=1), dict(zero, pitch_shift=-1), dict(zero, pitch_shift=1.5), dict(zero, note_dropout=1.2),
           dict(zero, tempo_jitter=-0.1), dict(zero, velocity_jitter=float("inf")), dict(zero, timing_jitter=float("nan")),
           dict(zero, noise_std=0.1)]
    for acfg in bad:
        with pytest.raises(ValueError):
            train_ae.augment_from_cfg(dict(AUGMENT=acfg))
        with pytest.raises(ValueError):
            train_ae.train(dict(AUGMENT=acfg, BATCH_SIZE=8, MAX_NOTES=32, EPOCHS=1), synthetic=8)


def test_sampler_weights_sum_to_the_number_of_classes():
    """ed_dataset.py:531-536: weight = 1 / class count, so every class carries total weight 1 -- the training split's class
    sizes are 260 / 228 / 213 / 196."""
    _lib()
    from melo_gan_amd import ops
    from melo_gan_amd.emotion_discriminator import train_ed
    sizes = [260, 228, 213, 196]
    labels = torch.cat([torch.full((k,), c, dtype=torch.int64) for c, k in enumerate(sizes)])[torch.randperm(897, generator=torch.Generator().manual_seed(0))]
    w = train_ed.sampler_weights(labels)
    assert w.dtype == torch.float64 and w.shape == (897,)
    assert abs(float(w.sum()) - 4.0) < 1e-12
    for c, k in enumerate(sizes):
        assert torch.equal(w[labels == c], torch.full((k,), 1.0 / k, dtype=torch.float64))
    cdf = ops.sampler_cdf(labels)
    assert cdf.dtype == torch.float64 and torch.equal(cdf, torch.cumsum(w, 0)) and bool((cdf[1:] > cdf[:-1]).all())
    with pytest.raises(ValueError):
        ops.sampler_cdf(torch.zeros(0, dtype=torch.int64))


def test_augment_spec_rejects_unknown_programs():
    _lib()
    from melo_gan_amd import ops
    with pytest.raises(ValueError):
        ops.augment_spec("gan")
