"""CPU-only: melo_gan_amd/ae/metrics.py -- host_vae_stats (the reference of mg_vae_eval_acc) against independent straight-line
computations, and report's definitions (active units, Fisher ratio, null instead of NaN)."""
import json
import math

import numpy as np
import torch
import torch.nn.functional as F

import melo_gan_amd  # noqa: F401
from melo_gan_amd import midi
from melo_gan_amd.ae import metrics as M


def make_inputs(n, T, L, K, seed, pad_rows=()):
    """x / recon uniform in [-1, 1] with about a third of channel 1 below the rest threshold on either side, mu / logvar of
    order 1, labels cycling over the classes (pad_rows: label -1)."""
    g = np.random.default_rng(seed)
    x = g.uniform(-1, 1, (n, T, 4)).astype(np.float32)
    recon = g.uniform(-1, 1, (n, T, 4)).astype(np.float32)
    for a in (x, recon):
        rest = g.random((n, T)) < 1 / 3
        a[..., 1] = np.where(rest, g.uniform(-1, -0.25, (n, T)), g.uniform(-0.15, 1, (n, T))).astype(np.float32)
    mu = g.normal(0, 1, (n, L)).astype(np.float32)
    logvar = g.normal(-1, 1, (n, L)).astype(np.float32)
    labels = np.arange(n, dtype=np.int64) % K
    for r in pad_rows:
        labels[r] = -1
    return x, recon, mu, logvar, labels


def scalar_decode(row):
    """One position by the scalar code of midi.notes_from_roll (chromatic: no snapping), in Python floats of fp32 values:
    (sounding, pitch, velocity, dur beats, step beats)."""
    f = np.float32
    p, v, d, s = (f(t) for t in row)
    step = max(0.1, float(((s + f(1.0)) / f(2.0)) * f(midi.MAX_BEAT_TIME)))
    sounding = not (v < f(midi.VELOCITY_THRESHOLD))
    pitch = int(np.clip(int((p + f(1.0)) * f(63.5)), 36, 96))
    vel = int(np.clip(int(f(60.0) + ((v - f(midi.VELOCITY_THRESHOLD)) / f(1.2)) * f(67.0)), 0, 127))
    dur = max(0.25, float(((d + f(1.0)) / f(2.0)) * f(midi.MAX_BEAT_TIME)))
    return sounding, pitch, vel, dur, step


def test_the_scalar_decode_of_this_file_is_the_output_contract():
    """scalar_decode above against midi.notes_from_roll itself on one row: same notes, same onsets."""
    x = make_inputs(1, 20, 5, 4, 3)[0][0]
    notes, _ = midi.notes_from_roll(x, bpm=120.0, scale="chromatic", root_key=0)
    t, want = 0.0, []
    for row in x:
        snd, pitch, vel, dur, step = scalar_decode(row)
        if snd:
            want.append((vel, pitch, t * 0.5, (t + dur) * 0.5))
        t += step
    assert len(notes) == len(want) > 0
    for got, w in zip(notes, want):
        assert tuple(got[:2]) == w[:2]
        assert abs(got[2] - w[2]) < 1e-5 and abs(got[3] - w[3]) < 1e-5      # the onsets there accumulate in fp32


def test_host_vae_stats_against_straight_line_computations():
    n, T, L, K = 6, 20, 5, 4
    x, recon, mu, logvar, labels = make_inputs(n, T, L, K, 11)
    acc, row_d, row_i = M.host_vae_stats(x, recon, mu, logvar, labels, K)
    rep = M.report(acc, T, L)
    o = rep["overall"]
    # KL per dimension against oracle.vae_loss's formula in torch fp64
    tm, tl = torch.from_numpy(mu).double(), torch.from_numpy(logvar).double()
    kl = -0.5 * (1 + tl - tm.pow(2) - tl.exp())
    np.testing.assert_allclose(o["kl_per_dim"], kl.mean(0).numpy(), rtol=1e-13)
    np.testing.assert_allclose(acc["lat"][:, 4].sum(0), kl.sum(0).numpy(), rtol=1e-13)
    assert abs(o["kld_mean"] - float(kl.mean())) <= 1e-13 * float(kl.abs().mean())
    assert abs(o["kld_mean"] * L - o["kl_per_sample"]) <= 1e-13 * abs(o["kl_per_sample"])
    np.testing.assert_allclose(row_d[:, 1], kl.sum(1).numpy(), rtol=1e-13)
    assert abs(o["kl_per_sample"] - float(row_d[:, 1].mean())) <= 1e-13 * float(np.abs(row_d[:, 1]).mean())
    # the trainer's reconstruction loss
    mse = float(F.mse_loss(torch.from_numpy(recon).double(), torch.from_numpy(x).double()))
    assert abs(o["recon_mse"] - mse) <= 1e-13 * mse
    per = ((recon.astype(np.float64) - x.astype(np.float64)) ** 2).mean(axis=(0, 1))
    np.testing.assert_allclose([o["recon_mse_per_channel"][c] for c in M.CHANNELS], per, rtol=1e-13)
    np.testing.assert_allclose(row_d[:, 0], ((recon.astype(np.float64) - x.astype(np.float64)) ** 2).sum(axis=(1, 2)), rtol=1e-13)
    # note counters: a per-position Python loop over the scalar decode
    want = np.zeros((K, 12), dtype=np.int64)
    dur_abs, step_abs = np.zeros(K), np.zeros(K)
    for r in range(n):
        k = labels[r]
        want[k, 0] += 1
        for t in range(T):
            sa, pa, va, da, ta = scalar_decode(x[r, t])
            sb, pb, vb, db, tb = scalar_decode(recon[r, t])
            want[k, 1] += 1
            step_abs[k] += abs(tb - ta)
            if sa and sb:
                dp = abs(pb - pa)
                want[k, 3] += 1
                want[k, 7] += dp == 0
                want[k, 8] += dp <= 1
                want[k, 9] += pa % 12 == pb % 12
                want[k, 10] += dp
                want[k, 11] += abs(vb - va)
                dur_abs[k] += abs(db - da)
            elif sa:
                want[k, 5] += 1
            elif sb:
                want[k, 6] += 1
            else:
                want[k, 4] += 1
    assert (want[:, 3:7].sum(0) > 0).all()              # all four rest / sounding combinations occur
    np.testing.assert_array_equal(acc["c"][:, :12], want)
    assert not acc["c"][:, 12:].any()
    np.testing.assert_allclose(acc["beats_abs"][:, 0], dur_abs, rtol=1e-13)
    np.testing.assert_allclose(acc["beats_abs"][:, 1], step_abs, rtol=1e-13)
    np.testing.assert_array_equal(row_i.sum(0), want[:, 1:9].sum(0))
    assert o["onset_recall"] == want[:, 3].sum() / (want[:, 3].sum() + want[:, 5].sum())
    assert o["onset_precision"] == want[:, 3].sum() / (want[:, 3].sum() + want[:, 6].sum())
    assert o["pitch_accuracy"] == want[:, 7].sum() / want[:, 3].sum()


def test_invalid_positions_are_counted_and_otherwise_absent():
    n, T, L, K = 2, 20, 5, 2
    x, recon, mu, logvar, labels = make_inputs(n, T, L, K, 5)
    clean = M.host_vae_stats(x[:, 3:], recon[:, 3:], mu, logvar, labels, K)[0]
    x[:, 0, 0], x[:, 1, 3], recon[:, 2, 2] = np.nan, np.inf, -np.inf
    acc = M.host_vae_stats(x, recon, mu, logvar, labels, K)[0]
    assert (acc["c"][:, 2] == 3).all() and (acc["c"][:, 1] == T - 3).all()
    np.testing.assert_array_equal(acc["c"][:, 3:], clean["c"][:, 3:])
    for k in ("se", "ae", "beats_abs"):
        assert np.isfinite(acc[k]).all()
        np.testing.assert_allclose(acc[k], clean[k], rtol=1e-13)


def test_active_units_counts_dimensions_above_the_collapse_threshold():
    """Var(mu) = {1.0, 0.25, 0.0101, 0.0099, 0.0} per dimension: three are above diagnose.py's 0.1 standard deviation."""
    n = 400
    base = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)           # population variance exactly 1
    mu = np.stack([base * math.sqrt(v) for v in (1.0, 0.25, 0.0101, 0.0099, 0.0)], axis=1).astype(np.float32)
    x = np.zeros((n, 8, 4), dtype=np.float32)
    acc = M.host_vae_stats(x, x, mu, np.zeros_like(mu), np.zeros(n, dtype=np.int64), 1)[0]
    o = M.report(acc, 8, 5)["overall"]
    np.testing.assert_allclose(o["mu_var"], [1.0, 0.25, 0.0101, 0.0099, 0.0], rtol=1e-6, atol=1e-12)
    assert o["active_units"] == 3 and o["collapsed_dims"] == [3, 4]
    assert o["latent_warning"] is None and o["latent_std"] > 0.1
    tiny = M.host_vae_stats(x, x, mu * 0.05, np.zeros_like(mu), np.zeros(n, dtype=np.int64), 1)[0]
    o = M.report(tiny, 8, 5)["overall"]
    assert o["latent_std"] < 0.1 and "collapse" in o["latent_warning"] and o["active_units"] == 0


def test_fisher_ratio_separates_a_separating_dimension_from_a_shared_one():
    g = np.random.default_rng(2)
    n = 200
    labels = np.arange(n, dtype=np.int64) % 2
    mu = g.normal(0, 1, (n, 2)).astype(np.float32)
    mu[:, 0] += np.where(labels == 0, -10.0, 10.0).astype(np.float32)
    x = np.zeros((n, 8, 4), dtype=np.float32)
    acc = M.host_vae_stats(x, x, mu, np.zeros_like(mu), labels, 4)[0]           # classes 2 and 3 are empty
    o = M.report(acc, 8, 2)["overall"]
    assert o["fisher_ratio"][0] > 50 and o["fisher_ratio"][1] < 0.05
    # against the definition, straight from the array
    m = mu.astype(np.float64)
    between = sum((labels == k).mean() * (m[labels == k].mean(0) - m.mean(0)) ** 2 for k in (0, 1))
    within = sum((labels == k).mean() * m[labels == k].var(0) for k in (0, 1))
    np.testing.assert_allclose(o["fisher_ratio"], between / within, rtol=1e-9)
    assert abs(o["fisher_ratio_mean"] - float((between / within).mean())) < 1e-9 * float((between / within).mean())


def test_empty_and_padding_only_classes_give_null_and_never_nan():
    n, T, L, K = 4, 20, 5, 3
    x, recon, mu, logvar, _ = make_inputs(n, T, L, K, 9)
    labels = np.array([0, -1, 0, -1], dtype=np.int64)       # class 1: nothing; class 2: nothing but would-be padding rows
    acc, row_d, row_i = M.host_vae_stats(x, recon, mu, logvar, labels, K)
    assert acc["c"][:, 0].tolist() == [2, 0, 0] and not row_i[1].any() and not row_d[3].any()
    rep = M.report(acc, T, L, names=("a", "b", "c"))
    text = json.dumps(rep, allow_nan=False)                 # raises on NaN / inf
    assert "NaN" not in text
    assert rep["overall"]["fisher_ratio"] is None and rep["overall"]["fisher_ratio_mean"] is None
    for name in ("b", "c"):
        blk = rep["per_class"][name]
        assert blk["rows"] == 0
        for key in ("recon_mse", "kld_mean", "kl_per_sample", "kl_per_dim", "active_units", "onset_precision", "onset_recall",
                    "pitch_accuracy", "mean_abs_dur_beats", "mean_abs_step_beats", "latent_std"):
            assert blk[key] is None, key
    assert rep["per_class"]["a"]["rows"] == 2 and rep["per_class"]["a"]["recon_mse"] > 0


def test_report_has_the_documented_keys():
    x, recon, mu, logvar, labels = make_inputs(5, 20, 5, 4, 1)
    rep = M.report(M.host_vae_stats(x, recon, mu, logvar, labels, 4)[0], 20, 5)
    keys = {"recon_mse", "recon_mse_per_channel", "recon_mae_per_channel", "kld_mean", "kl_per_dim", "kl_per_sample", "mu_mean",
            "mu_var", "mean_posterior_var", "active_units", "collapsed_dims", "latent_std", "onset_precision", "onset_recall",
            "pitch_accuracy", "pitch_within_1", "pitch_class_accuracy", "mean_abs_pitch_error", "mean_abs_velocity_error",
            "mean_abs_dur_beats", "mean_abs_step_beats"}
    assert keys | {"fisher_ratio", "fisher_ratio_mean"} <= set(rep["overall"])
    assert set(rep["per_class"]) == {"0", "1", "2", "3"} and all(keys <= set(b) for b in rep["per_class"].values())
    assert "deterministic" in rep["reconstruction"] and "diagnose.py" in rep["active_units_threshold"]


def test_the_layout_holds_26_plus_5L_words_per_class():
    from melo_gan_amd import ops
    for K, L in ((1, 1), (4, 8), (3, 300), (32, 1024)):
        lay = ops.vae_eval_acc_layout(K, L)
        assert lay["block"] == 26 + 5 * L and lay["words"] == K * (26 + 5 * L)
        assert sum(math.prod(s) for _, s in M.acc_fields(L)) == lay["block"]
        assert [(n, lay[n][1]) for n, _ in M.acc_fields(L)] == list(M.acc_fields(L))
