"""Held-out statistics of a trained VAE -- the host side of `python -m melo_gan_amd.ae.evaluate`.

The reference trains the VAE on one MSE over four channels of different scales plus a KL term and asks twice, without a number,
whether the latents it hands to the classifier and the generator are any good: src/gan/diagnose.py:82-91 warns of "Posterior
Collapse" when latents.std() < 0.1, src/gan/tsne.py asks whether the VAE clusters emotions.  Here both get numbers -- active
units, KL per dimension, the Fisher ratio of mu between the emotion classes -- next to the reconstruction error per channel
and the note-level agreement of the real and the reconstructed roll, decoded by the generator's output contract
(gan.music_metrics.decode_rolls).

csrc/vae_metrics.hip (mg_vae_eval_acc) computes the accumulator on the device; host_vae_stats is its reference in numpy, with
the kernel's addition order for the fp64 words, and report turns an accumulator into the JSON block.  This module imports no
GPU code.
"""
from __future__ import annotations

import math

import numpy as np

from ..gan.music_metrics import NOTE_DIM, decode_rolls

LANES = 256                     # the kernel's workgroup: lane u adds positions u, u + 256, ... in order, then a fixed tree
COUNTERS = ("rows", "valid", "invalid", "both_sounding", "both_rest", "missed", "extra", "pitch_equal", "pitch_within_1",
            "pitch_class_equal", "pitch_abs", "velocity_abs")      # c[0 .. 11]; c[12 .. 15] are zero
ROW_I = COUNTERS[1:9]
ROW_D = ("squared_error", "kl", "dur_abs_beats", "step_abs_beats")
LAT = ("mu", "mu_sq", "logvar", "var", "kl")
CHANNELS = ("pitch", "velocity", "duration", "step")
ACTIVE_VAR = 0.01               # Var(mu_j) above diagnose.py:88's 0.1 standard deviation, squared
COLLAPSE_STD = 0.1              # diagnose.py:88


def acc_fields(L: int):
    """One class's block of the accumulator, in 8-byte words: (name, shape); 26 + 5 L words (ops.vae_eval_acc_layout)."""
    return (("c", (16,)), ("se", (4,)), ("ae", (4,)), ("beats_abs", (2,)), ("lat", (5, int(L))))


def new_acc(K: int, L: int) -> dict:
    return {name: np.zeros((K, *shape), dtype=np.int64 if name == "c" else np.float64) for name, shape in acc_fields(L)}


def _lane_tree(terms):
    """The kernel's sum of a row's terms (n, q) -> (q,): lane u adds terms u, u + 256, ... in order, the 256 lanes are
    reduced by the tree v[u] += v[u + s], s = 128, 64, ..., 1."""
    terms = np.asarray(terms, dtype=np.float64)
    n = terms.shape[0]
    pad = np.zeros((-n % LANES,) + terms.shape[1:], dtype=np.float64)
    chunks = np.concatenate([terms, pad]).reshape(-1, LANES, *terms.shape[1:])
    v = np.zeros((LANES,) + terms.shape[1:], dtype=np.float64)
    for c in chunks:
        v = v + c
    s = LANES // 2
    while s:
        v = v[:s] + v[s:2 * s]
        s //= 2
    return v[0]


def kl_terms(mu, logvar):
    """-1/2 (1 + logvar - mu^2 - exp(logvar)) per element, in fp64 (train_ae.py:35-51 sums / averages these)."""
    mu, logvar = np.asarray(mu, dtype=np.float64), np.asarray(logvar, dtype=np.float64)
    return -0.5 * (((1.0 + logvar) - mu * mu) - np.exp(logvar))


def host_vae_stats(x, recon, mu, logvar, labels, K: int):
    """The kernel's reference in numpy: (acc, row_d (n, 4) float64, row_i (n, 8) int64) of n rows x / recon (n, T, 4) fp32
    with posteriors mu / logvar (n, L) fp32 and true classes `labels`; acc is new_acc's dict of (K, ...) arrays.  Rows with a
    label outside [0, K) are padding and stay zero.  The rows are added in order, one at a time."""
    x, recon = np.asarray(x), np.asarray(recon)
    mu, logvar, labels = np.asarray(mu), np.asarray(logvar), np.asarray(labels).astype(np.int64)
    if x.shape != recon.shape or x.ndim != 3 or x.shape[2] != NOTE_DIM or x.dtype != np.float32 or recon.dtype != np.float32:
        raise ValueError("host_vae_stats: x and recon (n, T, 4) float32 expected")
    n, T, _ = x.shape
    if mu.ndim != 2 or mu.shape[0] != n or mu.shape != logvar.shape or labels.shape != (n,) or mu.dtype != np.float32 \
            or logvar.dtype != np.float32:
        raise ValueError("host_vae_stats: mu and logvar (n, L) float32 and labels (n,) expected")
    L = mu.shape[1]
    acc = new_acc(K, L)
    row_d, row_i = np.zeros((n, 4), dtype=np.float64), np.zeros((n, 8), dtype=np.int64)
    a, b = decode_rolls(x), decode_rolls(recon)
    with np.errstate(all="ignore"):
        diff = recon.astype(np.float64) - x.astype(np.float64)
    for r in range(n):
        y = int(labels[r])
        if not 0 <= y < K:
            continue
        valid = a["valid"][r] & b["valid"][r]
        sa, sb = a["sounding"][r] & valid, b["sounding"][r] & valid
        both = sa & sb
        dp = np.abs(b["pitch"][r].astype(np.int64) - a["pitch"][r].astype(np.int64))
        dv = np.abs(b["vel"][r].astype(np.int64) - a["vel"][r].astype(np.int64))
        c = np.zeros(16, dtype=np.int64)
        c[:12] = (1, valid.sum(), T - valid.sum(), both.sum(), (valid & ~sa & ~sb).sum(), (sa & ~sb).sum(), (sb & ~sa).sum(),
                  (both & (dp == 0)).sum(), (both & (dp <= 1)).sum(), (both & (dp % 12 == 0)).sum(), dp[both].sum(),
                  dv[both].sum())
        d = np.where(valid[:, None], diff[r], 0.0)
        terms = np.concatenate([d * d, np.abs(d),
                                np.where(both, np.abs(b["dur"][r] - a["dur"][r]), 0.0)[:, None],
                                np.where(valid, np.abs(b["step"][r] - a["step"][r]), 0.0)[:, None]], axis=1)
        sums = _lane_tree(terms)                                # se[4], ae[4], dur_abs, step_abs
        m, lv = mu[r].astype(np.float64), logvar[r].astype(np.float64)
        with np.errstate(all="ignore"):
            elv, kl = np.exp(lv), kl_terms(m, lv)
            acc["c"][y] += c
            acc["se"][y] += sums[0:4]
            acc["ae"][y] += sums[4:8]
            acc["beats_abs"][y] += sums[8:10]
            acc["lat"][y] += np.stack([m, m * m, lv, elv, kl])
        row_i[r] = c[1:9]
        row_d[r] = (((sums[0] + sums[1]) + sums[2]) + sums[3], _lane_tree(kl[:, None])[0], sums[8], sums[9])
    return acc, row_d, row_i


def _ratio(a, b):
    a, b = float(a), float(b)
    return a / b if b != 0 and math.isfinite(a) and math.isfinite(b) else None


def _floats(v):
    return [float(t) for t in v]


def _block(c, se, ae, beats, lat, T: int, L: int) -> dict:
    """The metrics of one set of rows from its summed accumulator words."""
    n, valid, both = int(c[0]), int(c[1]), int(c[3])
    out = {"rows": n, "positions": {k: int(v) for k, v in zip(COUNTERS[1:7], c[1:7])}}
    # the trainer's number (F.mse_loss over every element) when no position is invalid: invalid ones are left out of both sides
    out["recon_mse"] = _ratio(se.sum(), 4 * valid)
    out["recon_mse_per_channel"] = {ch: _ratio(se[i], valid) for i, ch in enumerate(CHANNELS)}
    out["recon_mae_per_channel"] = {ch: _ratio(ae[i], valid) for i, ch in enumerate(CHANNELS)}
    out["kld_mean"] = _ratio(lat[4].sum(), n * L)           # train_ae.py:35-51: a mean over B L
    out["kl_per_sample"] = _ratio(lat[4].sum(), n)
    if n:
        mean = lat[0] / n
        var = np.maximum(lat[1] / n - mean * mean, 0.0)
        active = var > ACTIVE_VAR
        tot_mean = lat[0].sum() / (n * L)
        std = math.sqrt(max(lat[1].sum() / (n * L) - tot_mean * tot_mean, 0.0))
        out.update(kl_per_dim=_floats(lat[4] / n), mu_mean=_floats(mean), mu_var=_floats(var),
                   mean_posterior_var=_floats(lat[3] / n), mean_logvar=_floats(lat[2] / n),
                   active_units=int(active.sum()), collapsed_dims=[int(j) for j in np.flatnonzero(~active)], latent_std=std,
                   latent_warning=("latent vectors are very collapsed (low variance): the autoencoder might have suffered "
                                   "posterior collapse") if std < COLLAPSE_STD else None)
    else:
        out.update(kl_per_dim=None, mu_mean=None, mu_var=None, mean_posterior_var=None, mean_logvar=None, active_units=None,
                   collapsed_dims=None, latent_std=None, latent_warning=None)
    out.update(onset_precision=_ratio(both, both + int(c[6])), onset_recall=_ratio(both, both + int(c[5])),
               pitch_accuracy=_ratio(c[7], both), pitch_within_1=_ratio(c[8], both), pitch_class_accuracy=_ratio(c[9], both),
               mean_abs_pitch_error=_ratio(c[10], both), mean_abs_velocity_error=_ratio(c[11], both),
               mean_abs_dur_beats=_ratio(beats[0], both), mean_abs_step_beats=_ratio(beats[1], valid))
    return out


def fisher_ratio(c, lat):
    """Per latent dimension, the between-class over the within-class variance of mu (the numeric answer to tsne.py's "is your
    VAE clustering emotions?"): (list with None where the within-class variance is zero, mean of the defined ones), or
    (None, None) with fewer than two non-empty classes."""
    n = np.asarray(c)[:, 0].astype(np.float64)
    live = n > 0
    if int(live.sum()) < 2:
        return None, None
    s1, s2, nk = np.asarray(lat)[live, 0], np.asarray(lat)[live, 1], n[live][:, None]
    N = nk.sum()
    mk = s1 / nk
    m = s1.sum(axis=0) / N
    between = (nk * (mk - m) ** 2).sum(axis=0) / N
    within = np.maximum((s2 - nk * mk * mk).sum(axis=0) / N, 0.0)
    per = [_ratio(b, w) for b, w in zip(between, within)]
    known = [v for v in per if v is not None]
    return per, (sum(known) / len(known) if known else None)


def report(acc_views: dict, T: int, L: int, names=None) -> dict:
    """The JSON block of an accumulator (host_vae_stats' dict, or ops.vae_eval_acc_views of a host tensor): `overall`, and
    `per_class` by name (names: the K class names; their indices otherwise).  Plain Python values only; a ratio with a zero
    denominator is None (null), never NaN."""
    v = {k: np.asarray(a) for k, a in acc_views.items()}
    K = v["c"].shape[0]
    if v["lat"].shape != (K, 5, L) or v["c"].shape != (K, 16):
        raise ValueError(f"report: the accumulator is not that of {K} classes and {L} latent dimensions")
    names = [str(k) for k in range(K)] if names is None else list(names)
    if len(names) != K:
        raise ValueError(f"report: {len(names)} names for {K} classes")
    fields = ("c", "se", "ae", "beats_abs", "lat")
    overall = _block(*(v[f].sum(axis=0) for f in fields), T, L)
    overall["fisher_ratio"], overall["fisher_ratio_mean"] = fisher_ratio(v["c"], v["lat"])
    return {"max_notes": int(T), "latent_dim": int(L),
            "reconstruction": "decoded from mu (eps = 0): deterministic",
            "active_units_threshold": f"Var(mu) > {ACTIVE_VAR} (diagnose.py:88's 0.1 standard deviation, squared)",
            "overall": overall,
            "per_class": {name: _block(*(v[f][k] for f in fields), T, L) for k, name in enumerate(names)}}
