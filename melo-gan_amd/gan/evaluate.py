#!/usr/bin/env python3
"""Held-out evaluation of a trained GAN on the validation split -- is the generator producing different music for different
emotions on data it was not trained on?  The reference answers with host scripts over files (src/gan/analyze_midi.py:28-45:
pitch / velocity / density of written .mid files "to check if the GAN is actually learning different emotions";
src/gan/diagnose.py:53-80: ranges and variance of a split; src/emotion_discriminator/evaluate_ed.py, an accidental copy of
ed_model.py):

    python -m melo_gan_amd.gan.evaluate --config config/gan_config.yaml \
        [--ckpt <CHECKPOINT_DIR>/gan_final.pth | gan_epochNNNN.pth] [--split <VAL_SPLIT>] [--feats <ENCODER_FEATS_VAL>] \
        [--ed_config config/ed_config.yaml --ed_ckpt data/models/ed/ed_best.pth] [--seed <SEED>] [--batch 64] \
        [--out <LOG_DIR>/eval.json] [--synthetic N] [--feature-metrics [--knn-k 3] [--tsne] [--frechet]] [--memorisation]
        [--music-metrics] [--ema]

--ema evaluates the averaged generator in the `ema` block of a full checkpoint (EMA_DECAY, gan/ema.py) with that checkpoint's
critic -- the critic has no average; the noise is keyed by (seed, split row), so the same checkpoint and seed with and without
--ema is a paired comparison.  eval.json records "weights": "ema" | "raw".

One pass over the split in row order.  Per batch ONE replayed hipGraph: stage the batch by a device-side cursor -> noise
(mg_eval_noise: Philox keyed by (seed, split row), so the report does not depend on the batch size) -> E_num -> G (eval:
dropout off, BatchNorm on running statistics) -> critic on [real | fake] -> classifier on the real and the generated rolls
(latent mode: on the generator's internal latent, fake side only, as train_gan.py:232-237) -> mg_eval_acc, which adds the
batch to a device-resident accumulator and advances the cursor.  The host reads the accumulator once, when the pass ends.
A full checkpoint (gan_epochNNNN.pth) carries the critic; gan_final.pth does not and the critic metrics are then null.
--feature-metrics adds what means over rows cannot see -- mode collapse and memorisation -- in the classifier's feature space
(encoder.project's output): each batch's features are scattered to their split position inside the same graph, and after the
pass the pair kernels (mg_pair_ksum / mg_pair_knn / mg_pair_margin) give KID, k-NN precision / recall, both per emotion, and
the real-emotion x generated-emotion KID table (gan/feature_metrics.py).  --memorisation runs the real side over TRAIN_SPLIT
as well and reports every generated and validation row's distance to its nearest training row.
--music-metrics reports in notes what analyze_midi.py reads off written files: one more launch per batch (mg_note_stats, in
front of mg_eval_acc) decodes every real and every generated row into note events by the output contract and adds them to
device-resident integer histograms per side and true emotion; after the pass the host reads them once and
gan/music_metrics.py builds the `music` block -- note count, pitch, velocity, rests, density per emotion, and the
Jensen-Shannon divergence of seven histograms between real and generated music.  NOTE_DIM 4 only.
--tsne (needs --feature-metrics) lets one LOOK at those features: after the pass the stashed real and generated features are
embedded jointly by exact t-SNE on the device (gan/tsne.py) and written next to the report as <out stem>_tsne.npy / .svg --
colour = emotion, marker shape = real / generated -- with a `tsne` block (parameters, final KL, file names) in the report.
--frechet (needs --feature-metrics) adds the Frechet distance between the real and the generated features -- whole sets, per
emotion and the real-emotion x generated-emotion table -- and the spectrum of every feature covariance (effective rank,
participation ratio, top-1 share: a generator collapsed onto a few directions shows a rank far below the real data's).  The
moments are fp64 (mg_feat_moments), the eigenvalues come from the device's Jacobi solver (mg_frechet_pairs), and the results
ride in the buffer of the pair kernels' sums: the block is still one device -> host read (gan/feature_metrics.py).
Every input from outside is checked on the host before any GPU use.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
from dataclasses import dataclass
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import feature_metrics as FM
from . import generate as G
from . import music_metrics as MM
from ..checkpoints import check_critic_checkpoint, check_generator_checkpoint, ema_checkpoint, read_checkpoint
from ..eval_pass import Packed, ResidentPass
from ..pieces import require_device
from .config import read_config
from .eval_engine import EvalEngine
from .generate import EMOTIONS, GenerateError
from .utils import label_indices

DEFAULT_BATCH = 64
DEFAULT_KNN_K, MAX_KNN_K = 3, 8
SIDES = ("real", "fake")            # order of the accumulator's note statistics
RAW_KEYS = ("n", "conf_fake", "conf_real", "d_sum", "cls", "nsum", "nsq", "nmin", "nmax")


class EvaluateError(GenerateError):
    """A bad input of the evaluator, found on the host before any GPU use."""


# ---------------------------------------------------------------------------------------------------------------------
# host checks
# ---------------------------------------------------------------------------------------------------------------------
def check_ed_config(ed_cfg: dict, cfg: dict, path: str = "ED config"):
    G.check_ed_config(ed_cfg, cfg, err=EvaluateError, prefix=f"{path}: ")


def check_feature_options(features: bool, knn_k: int, ed_cfg: Optional[dict]):
    """What the feature-space metrics need: a neighbour count the kernel serves and a classifier that sees the real rolls."""
    if not features:
        return
    if not 1 <= int(knn_k) <= MAX_KNN_K:
        raise EvaluateError(f"--knn-k {knn_k}: must be in 1..{MAX_KNN_K}")
    if ed_cfg is None:
        raise EvaluateError("--feature-metrics needs the classifier (--ed_config / --ed_ckpt): its encoder is the feature space")
    if ed_cfg.get("input_mode", "notes") != "notes":
        raise EvaluateError("--feature-metrics needs a notes-mode classifier: a latent-mode one never sees the real rolls, so "
                            "the real side of every metric is missing")


def check_tsne_options(tsne: bool, features: bool, n: Optional[int] = None):
    """The t-SNE plot embeds the feature stashes, which only --feature-metrics fills; 2 n rows must fit the dense affinities and
    leave the default perplexity a root."""
    if not tsne:
        return
    from . import tsne as TS
    if not features:
        raise EvaluateError("--tsne needs --feature-metrics: it embeds the classifier features that pass stashes")
    if n is not None:
        try:
            TS.Tsne().check(2 * int(n), 1)
        except TS.TsneError as e:
            raise EvaluateError(f"--tsne: {e} (the real and the generated rows are embedded jointly: 2 x {n})") from e


def check_frechet_options(frechet: bool, features: bool, ed_cfg: Optional[dict] = None):
    """The Frechet distance is computed from the feature stashes, which only --feature-metrics fills; the moments kernel reads
    rows of a multiple of 4 in 4..256 features."""
    if not frechet:
        return
    if not features:
        raise EvaluateError("--frechet needs --feature-metrics: it compares the classifier features that pass stashes")
    dim = None if ed_cfg is None else ed_cfg.get("notes_hidden")
    if dim is not None and (int(dim) % 4 or not 4 <= int(dim) <= 256):
        raise EvaluateError(f"--frechet: notes_hidden = {dim}: the moments kernel reads a multiple of 4 in 4..256 features")


def check_music_options(music: bool, cfg: dict, batch: int = DEFAULT_BATCH):
    """The note-level statistics decode (T, 4) note rows; the piano-roll configuration has no such decode.  The batch and the
    row length must lie in mg_note_stats' domain."""
    if not music:
        return
    if int(cfg["NOTE_DIM"]) != MM.NOTE_DIM:
        raise EvaluateError(f"--music-metrics: NOTE_DIM = {cfg['NOTE_DIM']}: only the note-row format (NOTE_DIM "
                            f"{MM.NOTE_DIM}: pitch, velocity, duration, step) decodes into notes")
    if int(batch) > 32767 or not 1 <= int(cfg["MAX_NOTES"]) <= 1 << 20:
        raise EvaluateError(f"--music-metrics: --batch {batch} / MAX_NOTES {cfg['MAX_NOTES']}: at most 32767 rows per batch and "
                            "2^20 positions per row")


def check_checkpoint(ck, cfg: dict, path: str = "checkpoint") -> bool:
    """G and E_num as the sampler needs them; returns whether the checkpoint also holds a critic ('D') of the config's shapes."""
    check_generator_checkpoint(ck, cfg, path, EvaluateError)
    return check_critic_checkpoint(ck, cfg, path, EvaluateError)


def check_split_arrays(notes, emotions, numeric, latent, cfg: dict, where: str = "split"):
    """The row-aligned arrays of a split against the config; returns the class indices."""
    T, Cn, nd, ld = int(cfg["MAX_NOTES"]), int(cfg["NOTE_DIM"]), int(cfg.get("NUMERIC_INPUT_DIM", 6)), int(cfg["LATENT_DIM"])
    if notes.ndim != 3 or tuple(notes.shape[1:]) != (T, Cn):
        raise EvaluateError(f"{where}: notes has shape {tuple(notes.shape)}, the GAN config implies (n, {T}, {Cn})")
    n = notes.shape[0]
    if n < 1:
        raise EvaluateError(f"{where}: notes holds no rows")
    if numeric.ndim != 2 or tuple(numeric.shape) != (n, nd):
        raise EvaluateError(f"{where}: numeric_features has shape {tuple(numeric.shape)}, expected ({n}, {nd})")
    if len(emotions) != n:
        raise EvaluateError(f"{where}: emotion holds {len(emotions)} entries, notes {n} rows")
    if latent is not None and tuple(latent.shape) != (n, ld):
        raise EvaluateError(f"{where}: encoder features have shape {tuple(latent.shape)}, expected ({n}, {ld})")
    try:
        return label_indices(emotions, len(EMOTIONS), f"{where}: emotion labels")
    except ValueError as e:
        raise EvaluateError(str(e)) from e


def load_split_arrays(cfg: dict, split_csv: str, feats: Optional[str], feats_required: bool = False):
    """<SPLITS_DIR>/<split stem>/{notes,emotion,numeric_features}.npy (+ the encoder features), checked against the config."""
    d = os.path.join(cfg.get("SPLITS_DIR", "data/splits"), Path(split_csv).stem)
    arrs = {}
    for k in ("notes", "emotion", "numeric_features"):
        p = os.path.join(d, k + ".npy")
        if not os.path.isfile(p):
            raise EvaluateError(f"split array {p} does not exist")
        try:
            arrs[k] = np.load(p, mmap_mode="r" if k == "notes" else None, allow_pickle=(k == "emotion"))
        except Exception as e:      # noqa: BLE001 -- any unreadable file is the same user error
            raise EvaluateError(f"cannot read split array {p}: {e}") from e
    latent = None
    if feats and os.path.isfile(feats):
        try:
            latent = np.load(feats)
        except Exception as e:      # noqa: BLE001
            raise EvaluateError(f"cannot read encoder features {feats}: {e}") from e
    elif feats and feats_required:
        raise EvaluateError(f"encoder features {feats} do not exist")
    elif feats:         # from the config, as the trainer: tolerated, but said -- the latents are then zeros
        print(f"[WARN] encoder features {feats} not found: the split's latents are zeros (they feed a conditioning-mode "
              "generator and a latent-mode classifier)")
    check_split_arrays(arrs["notes"], arrs["emotion"], arrs["numeric_features"], latent, cfg, d)
    return arrs["notes"], arrs["emotion"], arrs["numeric_features"], latent


# ---------------------------------------------------------------------------------------------------------------------
# the report
# ---------------------------------------------------------------------------------------------------------------------
def raw_from_acc(acc_host: torch.Tensor, n_classes: int, n_channels: int) -> dict:
    """The accumulator (host copy) as named numpy arrays (ops.eval_acc_layout)."""
    from .. import ops
    return {k: v.numpy().copy() for k, v in ops.eval_acc_views(acc_host, n_classes, n_channels).items()}


def _ed_side(conf, ce, p, counts):
    n = int(counts.sum())
    conf = np.asarray(conf, dtype=np.int64)
    per = {}
    for k, name in enumerate(EMOTIONS):
        nk = int(counts[k])
        per[name] = ({"n": 0, "accuracy": None, "ce": None, "mean_p_target": None} if nk == 0 else
                     {"n": nk, "accuracy": float(conf[k, k]) / nk, "ce": float(ce[k]) / nk, "mean_p_target": float(p[k]) / nk})
    live = counts > 0
    return {"ce": float(ce[live].sum()) / n if n else None, "accuracy": float(np.trace(conf)) / n if n else None,
            "mean_p_target": float(p[live].sum()) / n if n else None, "confusion": conf.tolist(), "per_emotion": per}


def build_report(raw: dict, T: int, seed: int, batch: int, has_critic: bool, has_ed_fake: bool, has_ed_real: bool) -> dict:
    """The evaluation report from the raw accumulator (RAW_KEYS; ops.eval_acc_layout): plain Python values only."""
    missing = [k for k in RAW_KEYS if k not in raw]
    if missing:
        raise ValueError(f"build_report: the raw accumulator lacks {missing}")
    counts = np.asarray(raw["n"], dtype=np.int64)
    K = len(EMOTIONS)
    if counts.shape != (K,):
        raise ValueError(f"build_report: n has shape {counts.shape}, expected ({K},)")
    n = int(counts.sum())
    critic = None
    if has_critic and n:
        mr, mf = float(raw["d_sum"][0]) / n, float(raw["d_sum"][1]) / n
        critic = {"mean_real": mr, "mean_fake": mf, "w_dist": mr - mf}
    cls = np.asarray(raw["cls"], dtype=np.float64)
    notes = {}
    for s, side in enumerate(SIDES):
        notes[side] = {}
        for k, name in enumerate(EMOTIONS):
            nk = int(counts[k])
            cnt = float(nk) * T
            ch = []
            for c in range(np.asarray(raw["nsum"]).shape[2]):
                if nk == 0:
                    ch.append({"mean": None, "std": None, "min": None, "max": None})
                    continue
                sm, sq = float(raw["nsum"][s][k][c]), float(raw["nsq"][s][k][c])
                var = max((sq - sm * sm / cnt) / cnt, 0.0)       # population variance from the fp64 sums
                ch.append({"mean": sm / cnt, "std": math.sqrt(var), "min": float(raw["nmin"][s][k][c]),
                           "max": float(raw["nmax"][s][k][c])})
            notes[side][name] = {"n_rows": nk, "channels": ch}
    return {"n": n, "seed": int(seed), "batch": int(batch), "critic": critic,
            "ed_fake": _ed_side(raw["conf_fake"], cls[0][0], cls[0][1], counts) if has_ed_fake else None,
            "ed_real": _ed_side(raw["conf_real"], cls[1][0], cls[1][1], counts) if has_ed_real else None,
            "notes": notes}


def format_table(rep: dict) -> str:
    f = lambda v, spec: "-" if v is None else format(v, spec)  # noqa: E731
    lines = [f"rows {rep['n']}  seed {rep['seed']}  batch {rep['batch']}"]
    c = rep["critic"]
    lines.append("critic: " + ("-" if c is None else f"mean_real {c['mean_real']:.5f}  mean_fake {c['mean_fake']:.5f}  "
                                                        f"w_dist {c['w_dist']:.5f}"))
    for side in ("ed_fake", "ed_real"):
        e = rep[side]
        if e is None:
            lines.append(f"{side}: -")
            continue
        lines.append(f"{side}: ce {f(e['ce'], '.4f')}  accuracy {f(e['accuracy'], '.3f')}  mean_p_target {f(e['mean_p_target'], '.4f')}")
        lines.append(f"  {'emotion':<8} {'n':>6} {'accuracy':>9} {'ce':>9} {'p_target':>9}")
        for name, s in e["per_emotion"].items():
            lines.append(f"  {name:<8} {s['n']:>6} {f(s['accuracy'], '.3f'):>9} {f(s['ce'], '.4f'):>9} {f(s['mean_p_target'], '.4f'):>9}")
    lines.append("notes, channel 0 (mean / std / min / max):")
    for name in EMOTIONS:
        cells = []
        for side in SIDES:
            ch = rep["notes"][side][name]["channels"][0]
            cells.append(f"{side} " + " / ".join(f(ch[k], '.4f') for k in ("mean", "std", "min", "max")))
        lines.append(f"  {name:<8} " + "   ".join(cells))
    if "feature_space" in rep:
        lines.append(FM.format_block(rep["feature_space"], rep["feature_space"].get("nn_train")))
    if "music" in rep:
        lines.append(MM.format_block(rep["music"]))
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------------------------------------------------
class Evaluator(EvalEngine):
    """One GanEngine of `batch` rows in eval mode: encoder dropout off, generator BatchNorm on running statistics, no
    optimiser, no update of any buffer.  features: also keep every row's encoder features of the real and the generated roll
    and report the feature-space metrics over them (notes-mode classifier only); knn_k: the manifolds' neighbour count.
    music: also decode every real and generated row into notes and report the `music` block (NOTE_DIM 4 only).
    frechet (needs features): also report the Frechet distance and the covariance spectra of the feature sets."""
    error = EvaluateError

    def __init__(self, cfg: dict, ed_cfg: Optional[dict], device="cuda", batch: int = DEFAULT_BATCH, features: bool = False,
                 knn_k: int = DEFAULT_KNN_K, music: bool = False, frechet: bool = False):
        from .. import ops
        self.features, self.knn_k, self.music = bool(features), int(knn_k), bool(music)      # _check_config reads them
        self.frechet = bool(frechet)
        super().__init__(cfg, ed_cfg, device, batch)
        eng = self.eng
        if self.frechet:
            check_frechet_options(True, True, {"notes_hidden": eng.ed_feat_dim})
        self.has_d = False                                  # load_critic / copy_from: the critic's weights mean something
        self.ed_real = self.has_ed and eng.ed_mode == "notes"
        d = eng.dev
        self.K = len(EMOTIONS)
        self.split_pass = ResidentPass(self.B, d, self.graphs)
        self.ctr, self.base = self.split_pass.ctr, self.split_pass.base      # batch cursor, advanced by mg_eval_acc
        self.acc = ops.eval_acc_new(self.K, eng.C, d)
        self.logits_real = torch.zeros(self.B, self.K, device=d)
        self.feat_real = self.feat_fake = self.feat_train = None      # (whole batches, notes_hidden) stashes in split row order
        self.music_buf = self.note_acc = self.note_row_i = self.note_row_beats = None      # one Packed buffer, three views of it
        self._labels_host = None

    def _check_config(self, cfg: dict, ed_cfg: Optional[dict]):
        check_feature_options(self.features, self.knn_k, ed_cfg)
        check_frechet_options(self.frechet, self.features, ed_cfg)
        check_music_options(self.music, cfg, self.B)
        if ed_cfg is not None:
            check_ed_config(ed_cfg, cfg)

    # ---- weights ----
    def load_critic(self, ck) -> bool:
        """The critic from a full gan_epochNNNN.pth (key 'D').  gan_final.pth holds none: returns False and the critic metrics
        of the report are null."""
        ck, path = self._read(ck)
        if not check_checkpoint(ck, self.cfg, path):
            self.has_d = False
            return False
        self.eng.D.load(ck["D"])
        self.eng.params_changed()
        self.has_d = True
        return True

    def copy_from(self, src):
        """The current weights of a training engine (same configs), device to device: generator + encoder, critic, frozen
        classifier and the BatchNorm buffers.  Reads `src` only; the copies are ordered behind the caller's current stream."""
        e = self.eng
        for a, b in ((e.GE, src.GE), (e.D, src.D), (e.ED, src.ED)):
            if a.data.shape != b.data.shape or list(a.spec.items()) != list(b.spec.items()):
                raise EvaluateError("copy_from: the engines were built from different configs")
        e.stream.wait_stream(torch.cuda.current_stream(e.dev))
        with torch.cuda.stream(e.stream):
            for a, b in ((e.GE, src.GE), (e.D, src.D), (e.ED, src.ED)):
                a.data.copy_(b.data)
            for k in e.Gbuf:
                e.Gbuf[k].copy_(src.Gbuf[k])
            for k in e.EDbuf:
                e.EDbuf[k].copy_(src.EDbuf[k])
            e.params_changed()
        self.has_d = True

    # ---- the pass ----
    def _launches(self, jobs, order, order_len, n, seed, draw, metrics=True):
        """One batch.  metrics=False leaves the accumulation out (tools/eval_bench.py times the batch with and without it)."""
        from .. import ops
        eng, B = self.eng, self.B
        ops.stage_rows_cursor(jobs, B, order, order_len, self.ctr, self.base)
        if draw:
            ops.eval_noise(eng.noise, self.ctr, self.base, n, seed)
        eng._e_fwd(False, "g", gin=True)
        eng._g_fwd(eng.fake_d, False, "g")                  # rows [2B, 3B) of X0: [real | fake] is one 2B-row critic batch
        if self.has_d:
            eng._d_fwd(eng.X0[B:3 * B], 2 * B, eng.emb)
        lf = lr = None
        if self.has_ed:
            if self.ed_real:
                eng._ed_fwd(eng.real)
                ops.axpby(eng.logits, self.logits_real, 1.0, 0.0)
                lr = self.logits_real
                if self.features:                           # in front of eval_acc, which advances the cursor
                    ops.scatter_rows_cursor(eng.ed_proj, self.feat_real, self.ctr, self.base)
            eng._ed_fwd(eng.fake_d)                         # latent mode: reads the generator's internal latent instead
            lf = eng.logits
            if self.features:
                ops.scatter_rows_cursor(eng.ed_proj, self.feat_fake, self.ctr, self.base)
        if not metrics:
            return
        if self.music:                                      # in front of eval_acc, which advances the cursor
            ops.note_stats(eng.real, eng.fake_d, eng.emot_idx, self.note_acc, self.note_row_i, self.note_row_beats, self.ctr,
                           self.base, self.K)
        ops.eval_acc(eng.real, eng.fake_d, eng.emot_idx, eng.s[:B] if self.has_d else None,
                     eng.s[B:2 * B] if self.has_d else None, lf, lr, self.acc, tick=self.ctr, n_classes=self.K)

    def _check_split(self, dataset, who):
        eng = self.eng
        if not getattr(dataset, "resident", False):
            raise EvaluateError(f"evaluate: the {who} must be resident on the device (GANDataset(resident=True))")
        if len(dataset) < 1 or tuple(dataset.notes.shape[1:]) != (eng.T, eng.C):
            raise EvaluateError(f"evaluate: the {who}'s notes have shape {tuple(dataset.notes.shape)}, the engine reads "
                                f"(n, {eng.T}, {eng.C})")

    def _train_features(self, train_dataset):
        """The real-side-only pass over the training split: stage -> classifier -> scatter, batch b under cursor value b."""
        from .. import ops
        eng, B = self.eng, self.B
        n = len(train_dataset)
        nb = (n + B - 1) // B
        self.feat_train = torch.zeros(nb * B, eng.ed_feat_dim, device=eng.dev)
        order = torch.arange(nb * B, dtype=torch.int64, device=eng.dev)
        cursors = torch.arange(nb, dtype=torch.int64, device=eng.dev)
        for b in range(nb):
            ops.stage_rows_cursor([(train_dataset.notes, eng.real)], B, order, nb * B, cursors[b:b + 1], self.base)
            eng._ed_fwd(eng.real)
            ops.scatter_rows_cursor(eng.ed_proj, self.feat_train, cursors[b:b + 1], self.base)
        return self.feat_train[:n]

    def feature_space(self, labels_host, n, train=None):
        """The report's feature_space block from the stashes: the pair kernels over the whole sets and the per-emotion slices,
        every result in one device buffer that the host reads once.  labels_host: the split's class indices on the host (read
        from the device once, when the pass's graph is built); the per-emotion row indices go up to the device on every call."""
        from .. import ops
        dev, k, K = self.eng.dev, self.knn_k, self.K
        R, F = self.feat_real[:n], self.feat_fake[:n]
        idx = [torch.nonzero(labels_host == e).flatten().to(dev) for e in range(K)]
        counts = [int(i.numel()) for i in idx]
        Re = [R.index_select(0, i) if c else None for i, c in zip(idx, counts)]
        Fe = [F.index_select(0, i) if c else None for i, c in zip(idx, counts)]
        # the result buffer: the fp64 kernel sums, then the fp32 margins of every pair of sets that holds more than k rows
        # (fake in real, real in fake: over all rows, then per emotion), then the nearest-training-row distances
        n_sums = 3 + 2 * K + K * K
        sets = [(tag, A, Bm) for tag, A, Bm in [("", F, R)] + [(str(e), Fe[e], Re[e]) for e in range(K)]
                if A is not None and A.shape[0] > k]
        out = Packed([("sums", (n_sums,), torch.float64)] +
                     [(side + tag, (A.shape[0],), torch.float32) for tag, A, _ in sets for side in ("fr", "rf")] +
                     ([("nn_fake", (n,), torch.float32), ("nn_real", (n,), torch.float32)] if train is not None else []) +
                     (self._frechet_parts(R, F, Re, Fe) if self.frechet else []), dev)
        ks = out.dev["sums"]
        slot = iter(range(n_sums))

        def ksum(A, Bm, same):
            i = next(slot)
            if A is not None and Bm is not None and A.shape[0] >= 2 and Bm.shape[0] >= 2:
                ops.pair_ksum(A, Bm, ks[i:i + 1], exclude_diag=same)
            return i

        s_xx, s_yy, s_xy = ksum(R, R, True), ksum(F, F, True), ksum(R, F, False)
        s_xx_e = [ksum(Re[e], Re[e], True) for e in range(K)]
        s_yy_e = [ksum(Fe[e], Fe[e], True) for e in range(K)]
        s_xy_ef = [[ksum(Re[e], Fe[f], False) for f in range(K)] for e in range(K)]
        for tag, A, Bm in sets:             # A's rows in Bm's manifold ("fr"), Bm's rows in A's ("rf")
            for side, X, Y in (("fr", A, Bm), ("rf", Bm, A)):          # Y's radii, then X against Y's manifold
                nn = torch.empty(A.shape[0], k, device=dev)
                ops.pair_knn(Y, Y, nn, exclude_self=True)
                ops.pair_margin(X, Y, nn[:, k - 1].contiguous(), out.dev[side + tag])
        if train is not None:
            ops.pair_knn(F, train, out.dev["nn_fake"].view(n, 1))
            ops.pair_knn(R, train, out.dev["nn_real"].view(n, 1))
        if self.frechet:
            self._frechet_launches(out.dev)
        host = {name: v.numpy() for name, v in out.host().items()}      # every result of the pair kernels in one read
        hk = host["sums"]
        sums = {"xx": hk[s_xx], "yy": hk[s_yy], "xy": hk[s_xy], "xx_e": [hk[i] for i in s_xx_e], "yy_e": [hk[i] for i in s_yy_e],
                "xy_ef": [[hk[i] for i in row] for row in s_xy_ef]}
        marg = {"fake_in_real": host.get("fr"), "real_in_fake": host.get("rf"),
                "fake_in_real_e": [host.get(f"fr{e}") for e in range(K)], "real_in_fake_e": [host.get(f"rf{e}") for e in range(K)]}
        block = FM.feature_block(R.shape[1], k, EMOTIONS, counts, sums, marg)
        if train is not None:
            block["nn_train"] = FM.nn_summary(host["nn_fake"], host["nn_real"])
        if self.frechet:
            self._frechet_entries(block, counts, host)
        return block

    # ---- --frechet: the moments of every set of at least 2 rows, then one mg_frechet_pairs ----
    def _frechet_parts(self, R, F, Re, Fe):
        """Plans the sets (whole real, whole fake, every emotion's real and fake slice; fewer than 2 rows: left out) and the
        pairs (whole x whole, every real emotion x generated emotion); returns their parts of the result buffer."""
        K = self.K
        named = [("real", R), ("fake", F)] + [(f"real{e}", Re[e]) for e in range(K)] + [(f"fake{e}", Fe[e]) for e in range(K)]
        self._fd_sets = [(name, X) for name, X in named if X is not None and X.shape[0] >= 2]
        at = {name: i for i, (name, _) in enumerate(self._fd_sets)}
        wanted = [("whole", "real", "fake")] + [((e, f), f"real{e}", f"fake{f}") for e in range(K) for f in range(K)]
        self._fd_pairs = [(tag, at[a], at[b]) for tag, a, b in wanted if a in at and b in at]
        S, P = len(self._fd_sets), len(self._fd_pairs)
        if not P:           # no set on one of the sides: nothing to launch
            return []
        return [("fd_out", (P, 4), torch.float64), ("fd_spectrum", (S, 3), torch.float64), ("fd_info", (S + P, 2), torch.int32)]

    def _frechet_launches(self, dev_views):
        from .. import ops
        if not self._fd_pairs:
            return
        dev, D, S = self.eng.dev, self.eng.ed_feat_dim, len(self._fd_sets)
        means = torch.empty(S, D, dtype=torch.float64, device=dev)
        covs = torch.empty(S, D, D, dtype=torch.float64, device=dev)
        for i, (_, X) in enumerate(self._fd_sets):
            ops.feat_moments(X, means[i], covs[i])
        pairs = torch.tensor([[a, b] for _, a, b in self._fd_pairs], dtype=torch.int32).to(dev)
        ops.frechet_pairs(means, covs, pairs, dev_views["fd_out"], dev_views["fd_spectrum"], dev_views["fd_info"])

    def _frechet_entries(self, block, counts, host):
        """The host side: NaN (a solve that did not converge) becomes None, with a line on stderr."""
        K = self.K
        rows = {"whole": None, "ef": [[None] * K for _ in range(K)]}
        spectra = {"real": None, "fake": None, "real_e": [None] * K, "fake_e": [None] * K}
        if self._fd_pairs:
            S = len(self._fd_sets)
            out, spec, info = host["fd_out"], host["fd_spectrum"], host["fd_info"]
            for i, (name, _) in enumerate(self._fd_sets):
                if not info[i][1]:
                    print(f"[WARN] frechet: the eigensolver did not converge on the covariance of set '{name}' in "
                          f"{int(info[i][0])} sweeps: its spectrum and distances are null", file=sys.stderr)
                triple = tuple(float(v) for v in spec[i])
                if name in ("real", "fake"):
                    spectra[name] = triple
                else:
                    spectra[name[:4] + "_e"][int(name[4:])] = triple
            for j, (tag, a, b) in enumerate(self._fd_pairs):
                if not info[S + j][1]:
                    print(f"[WARN] frechet: the eigensolver did not converge on pair {tag} in {int(info[S + j][0])} sweeps: "
                          "its distance is null", file=sys.stderr)
                row = tuple(float(v) for v in out[j])
                if tag == "whole":
                    rows["whole"] = row
                else:
                    rows["ef"][tag[0]][tag[1]] = row
        fb = FM.frechet_block(block["dim"], EMOTIONS, counts, rows, spectra)
        for name, v in fb.pop("fd_e").items():
            block["per_emotion"][name]["fd"] = v
        block.update(fb)

    def evaluate(self, dataset, seed: int, noise: Optional[torch.Tensor] = None, train_dataset=None) -> dict:
        """One pass over a resident GANDataset in row order; returns the report.  noise: an (n, NOISE_DIM) resident fp32
        array staged instead of drawn (tests, externally paired runs).  train_dataset (features=True only): the resident
        training split of the nearest-training-row check."""
        from .. import ops
        eng, B = self.eng, self.B
        self._check_split(dataset, "split")
        n = len(dataset)
        if train_dataset is not None:
            if not self.features:
                raise EvaluateError("evaluate: the nearest-training-row check needs an Evaluator built with features=True")
            self._check_split(train_dataset, "training split")
        if tuple(dataset.numeric.shape) != (n, eng.num_in) or tuple(dataset.latent.shape) != (n, eng.latent_dim):
            raise EvaluateError("evaluate: the split's numeric features / latents do not match the config")
        if noise is not None and (not isinstance(noise, torch.Tensor) or not noise.is_cuda or noise.dtype != torch.float32 or
                                  not noise.is_contiguous() or tuple(noise.shape) != (n, eng.noise_dim)):
            raise EvaluateError(f"evaluate: noise must be a contiguous fp32 device array of shape ({n}, {eng.noise_dim})")
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        def build(split):
            if self.features:
                self.feat_real = torch.zeros(split.rows, eng.ed_feat_dim, device=eng.dev)
                self.feat_fake = torch.zeros(split.rows, eng.ed_feat_dim, device=eng.dev)
            if self.music:      # accumulator | per-row fp64 sums | per-row int32 numbers: one device -> host read
                self.music_buf = Packed([("acc", (ops.note_acc_layout(self.K)["words"],), torch.int64),
                                         ("row_beats", (2, split.rows, 2), torch.float64),
                                         ("row_i", (2, split.rows, 8), torch.int32)], eng.dev)
                self.note_acc, self.note_row_beats, self.note_row_i = self.music_buf.dev.values()
            split.jobs = [(dataset.notes, eng.real), (dataset.numeric, eng.numeric), (split.labels, eng.emot_idx)]
            split.dataset = dataset         # held with the keyed arrays for as long as the key stands
            if eng.latent_dim > 0:
                split.jobs.append((dataset.latent, eng.latent))
            if noise is not None:
                split.jobs.append((noise, eng.noise))
            # the grouping of the feature metrics and of the per-row note statistics
            self._labels_host = dataset.emot_idx.cpu() if self.features or self.music else None

        def reset():
            ops.eval_acc_reset(self.acc, self.K, eng.C)
            if self.music:
                self.music_buf.buf.zero_()      # the empty accumulator (mg_note_acc_reset's zeros) and the per-row stashes

        train = None
        with torch.cuda.stream(eng.stream):
            if train_dataset is not None:
                train = self._train_features(train_dataset)
            sp = self.split_pass.bind((dataset.notes, dataset.emot_idx, noise), (n, seed, self.has_d, self.music), n,
                                      dataset.emot_idx, build)
            self.split_pass.run("batch", lambda: self._launches(sp.jobs, sp.order, sp.rows, n, seed, noise is None), reset)
            acc = self.acc.cpu()                # the pass's only device -> host read (with the note statistics' buffer)
            music_host = self.music_buf.host() if self.music else None
            block = self.feature_space(self._labels_host, n, train) if self.features else None
        raw = raw_from_acc(acc, self.K, eng.C)
        rep = build_report(raw, eng.T, seed, B, self.has_d, self.has_ed, self.ed_real)
        if block is not None:
            rep["feature_space"] = block
        if music_host is not None:
            raw = {k: v.numpy() for k, v in ops.note_acc_views(music_host["acc"], self.K).items()}
            rows = {k: music_host[k].numpy()[:, :n] for k in ("row_i", "row_beats")}
            rep["music"] = MM.music_block(raw, rows, self._labels_host.numpy(), EMOTIONS)
        return rep

    def tsne(self, n: int, stem: str, **params) -> dict:
        """After evaluate() with features=True: the joint exact t-SNE of [feat_real[:n]; feat_fake[:n]] (2 n rows) written to
        <stem>_tsne.npy and <stem>_tsne.svg (colour = true emotion, marker = real / generated); returns the report's `tsne`
        block.  params: gan.tsne.Tsne's."""
        from . import tsne as TS
        if not self.features or self.feat_real is None or self._labels_host is None:
            raise EvaluateError("tsne: needs an Evaluator built with features=True, after evaluate()")
        check_tsne_options(True, True, n)
        ts = TS.Tsne(**params)
        with torch.cuda.stream(self.eng.stream):
            X = torch.cat([self.feat_real[:n], self.feat_fake[:n]])
            Y = ts.fit_transform(X)
        names = [EMOTIONS[int(k)] if 0 <= int(k) < len(EMOTIONS) else TS.OTHER for k in self._labels_host[:n].tolist()]
        files = {"embedding": stem + "_tsne.npy", "plot": stem + "_tsne.svg"}
        np.save(files["embedding"], Y)
        TS.write_svg(files["plot"], Y, names + names, title=f"t-SNE of the classifier features: {n} real, {n} generated",
                     groups=[0] * n + [1] * n)
        return {"n": 2 * n, "dim": int(X.shape[1]), "rows": "real rows 0..n-1, then generated rows 0..n-1", "params": ts.params(),
                "kl": ts.kl_, "trace_iters": ts.trace_iters, "kl_trace": ts.kl_trace.tolist(),
                "files": {k: os.path.basename(v) for k, v in files.items()}}


# ---------------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m melo_gan_amd.gan.evaluate",
                                 description="Held-out evaluation of a trained GAN on the validation split.")
    ap.add_argument("--config", type=str, default="config/gan_config.yaml", help="Path to the main GAN config")
    ap.add_argument("--ckpt", type=str, default=None, help="gan_final.pth (default, under CHECKPOINT_DIR) or a full gan_epochNNNN.pth")
    ap.add_argument("--split", type=str, default=None, help="split to evaluate (default VAL_SPLIT)")
    ap.add_argument("--feats", type=str, default=None, help="encoder features of the split (default ENCODER_FEATS_VAL)")
    ap.add_argument("--ed_config", type=str, default=None, help="ED config of the classifier")
    ap.add_argument("--ed_ckpt", type=str, default=None, help="ED checkpoint (ed_best.pth)")
    ap.add_argument("--seed", type=int, default=None, help="noise seed (default SEED)")
    ap.add_argument("--batch", type=int, default=DEFAULT_BATCH, help="rows per replayed batch")
    ap.add_argument("--out", type=str, default=None, help="report file (default <LOG_DIR>/eval.json)")
    ap.add_argument("--synthetic", type=int, default=0, help="evaluate on N synthetic rolls (drawn with SEED + 1) instead of a split")
    ap.add_argument("--feature-metrics", action="store_true",
                    help="add KID and k-NN precision / recall in the classifier's feature space (needs a notes-mode classifier)")
    ap.add_argument("--knn-k", type=int, default=DEFAULT_KNN_K, help=f"neighbours of the precision / recall manifolds (1..{MAX_KNN_K})")
    ap.add_argument("--memorisation", action="store_true",
                    help="also report every generated / validation row's distance to its nearest TRAIN_SPLIT row (implies "
                         "--feature-metrics)")
    ap.add_argument("--music-metrics", action="store_true",
                    help="add the note-level musical statistics of the real and the generated rolls, per emotion (NOTE_DIM 4)")
    ap.add_argument("--tsne", action="store_true",
                    help="also embed the real and the generated features jointly by exact t-SNE and write <out stem>_tsne.npy / "
                         ".svg (needs --feature-metrics)")
    ap.add_argument("--frechet", action="store_true",
                    help="also report the Frechet distance between the real and the generated features and the spectrum of "
                         "every feature covariance (needs --feature-metrics)")
    ap.add_argument("--ema", action="store_true", help="evaluate the averaged weights in a full checkpoint's 'ema' block")
    return ap.parse_args(argv)


@dataclass
class Plan:
    cfg: dict
    ed_cfg: Optional[dict]
    ckpt_path: str
    ckpt: dict
    has_critic: bool
    ed_ckpt: Optional[str]
    arrays: Optional[tuple]
    synthetic: int
    seed: int
    batch: int
    out: str
    features: bool = False
    knn_k: int = DEFAULT_KNN_K
    memorisation: bool = False
    train_arrays: Optional[tuple] = None
    music: bool = False
    tsne: bool = False
    ema: bool = False
    frechet: bool = False


def plan(args) -> Plan:
    """Every check of what comes from outside, on the host (no GPU needed); raises EvaluateError."""
    if args.batch < 1:
        raise EvaluateError(f"--batch {args.batch}: must be >= 1")
    if args.synthetic < 0:
        raise EvaluateError(f"--synthetic {args.synthetic}: must be >= 0")
    memorisation = bool(getattr(args, "memorisation", False))
    features = bool(getattr(args, "feature_metrics", False)) or memorisation
    knn_k = int(getattr(args, "knn_k", DEFAULT_KNN_K))
    if not 1 <= knn_k <= MAX_KNN_K:
        raise EvaluateError(f"--knn-k {knn_k}: must be in 1..{MAX_KNN_K}")
    tsne = bool(getattr(args, "tsne", False))
    check_tsne_options(tsne, features, args.synthetic or None)
    frechet = bool(getattr(args, "frechet", False))
    check_frechet_options(frechet, features)
    if features and args.ed_config is None:
        check_feature_options(True, knn_k, None)
    cfg, ckpt_path = G.plan_config(args, EvaluateError)
    if int(cfg["NOTE_DIM"]) % 4 or not 4 <= int(cfg["NOTE_DIM"]) <= 1024:
        raise EvaluateError(f"config {args.config}: NOTE_DIM = {cfg['NOTE_DIM']}: the metrics kernel reads 4 channels per lane "
                            "(a multiple of 4 in 4..1024)")
    music = bool(getattr(args, "music_metrics", False))
    check_music_options(music, cfg, args.batch)
    ckpt = read_checkpoint(ckpt_path, EvaluateError, weights_only=None)      # torch's default: a GAN file holds tensors and numbers
    has_critic = check_checkpoint(ckpt, cfg, ckpt_path)
    ema = bool(getattr(args, "ema", False))
    if ema:
        check_generator_checkpoint(ema_checkpoint(ckpt, ckpt_path, EvaluateError), cfg, ckpt_path, EvaluateError)
    ed_cfg = None
    if args.ed_config is not None:
        ed_cfg = read_config(args.ed_config, "ED config", EvaluateError)
        check_ed_config(ed_cfg, cfg, f"ED config {args.ed_config}")
        check_feature_options(features, knn_k, ed_cfg)
        check_frechet_options(frechet, features, ed_cfg)
        if not os.path.isfile(args.ed_ckpt):
            raise EvaluateError(f"ED checkpoint {args.ed_ckpt} does not exist")
    arrays = None
    if not args.synthetic:
        split = args.split or cfg.get("VAL_SPLIT")
        if not split:
            raise EvaluateError(f"config {args.config} lacks VAL_SPLIT and no --split was given")
        arrays = load_split_arrays(cfg, split, args.feats or cfg.get("ENCODER_FEATS_VAL"), feats_required=args.feats is not None)
        check_tsne_options(tsne, features, arrays[0].shape[0])
    train_arrays = None
    if memorisation and not args.synthetic:     # with --synthetic the training side is the trainer's synthetic split (SEED)
        if not cfg.get("TRAIN_SPLIT"):
            raise EvaluateError(f"--memorisation: config {args.config} lacks TRAIN_SPLIT")
        train_arrays = load_split_arrays(cfg, cfg["TRAIN_SPLIT"], None)
    out = args.out or os.path.join(cfg.get("LOG_DIR", "experiments/gan/logs"), "eval.json")
    seed = args.seed if args.seed is not None else int(cfg.get("SEED", 42))
    return Plan(cfg, ed_cfg, ckpt_path, ckpt, has_critic, args.ed_ckpt, arrays, int(args.synthetic), seed, args.batch, out,
                features, knn_k, memorisation, train_arrays, music, tsne, ema, frechet)


def main(argv=None) -> int:
    args = parse_args(argv)
    try:
        p = plan(args)
    except GenerateError as e:
        print(f"evaluate: error: {e}", file=sys.stderr)
        return 2
    require_device()
    from .dataset import GANDataset
    cfg = p.cfg
    if p.synthetic:
        ds = GANDataset.synthetic(p.synthetic, int(cfg["MAX_NOTES"]), int(cfg["NOTE_DIM"]), int(cfg["LATENT_DIM"]),
                                  int(cfg.get("SEED", 42)) + 1, "cuda")
    else:
        ds = GANDataset(*p.arrays, int(cfg["LATENT_DIM"]), "cuda", resident=True)
    train_ds = None
    if p.memorisation:
        train_ds = (GANDataset.synthetic(p.synthetic, int(cfg["MAX_NOTES"]), int(cfg["NOTE_DIM"]), int(cfg["LATENT_DIM"]),
                                         int(cfg.get("SEED", 42)), "cuda") if p.synthetic else
                    GANDataset(*p.train_arrays, int(cfg["LATENT_DIM"]), "cuda", resident=True))
    ev = Evaluator(cfg, p.ed_cfg, "cuda", p.batch, features=p.features, knn_k=p.knn_k, music=p.music,
                   frechet=p.frechet)
    weights = ev.load_generator(p.ckpt, ema=p.ema)
    if p.has_critic:
        ev.load_critic(p.ckpt)
    if p.ed_cfg is not None:
        ev.load_ed(p.ed_ckpt)
    rep = ev.evaluate(ds, p.seed, train_dataset=train_ds)
    rep["checkpoint"], rep["ed_checkpoint"], rep["weights"] = p.ckpt_path, p.ed_ckpt, weights
    os.makedirs(os.path.dirname(os.path.abspath(p.out)), exist_ok=True)
    if p.tsne:
        rep["tsne"] = ev.tsne(rep["n"], os.path.splitext(p.out)[0], seed=p.seed)
    with open(p.out, "w") as f:
        json.dump(rep, f, indent=1)
    print(format_table(rep))
    if p.tsne:
        print(f"t-SNE of {rep['tsne']['n']} feature rows: KL {rep['tsne']['kl']:.4f}; wrote {rep['tsne']['files']['embedding']}, "
              f"{rep['tsne']['files']['plot']}")
    print(f"wrote {p.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
