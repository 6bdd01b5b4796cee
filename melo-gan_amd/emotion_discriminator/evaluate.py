#!/usr/bin/env python3
"""Held-out evaluation of a trained emotion classifier on the device.

    python -m melo_gan_amd.emotion_discriminator.evaluate --config config/ed_config.yaml --model data/models/ed/ed_best.pth
        [--split test|val|train] [--batch 64] [--bins 15] [--robustness R] [--out <checkpoint_dir>/ed_eval.json]
        [--save-probs PATH.npy] [--synthetic N] [--seed S]

The classifier is the frozen judge of the project (the generator's cross-entropy, gan.generate's verdicts, gan.evaluate's
accuracy, the feature space of KID / precision-recall / t-SNE) and train_ed keeps one validation loss and one accuracy of it
per epoch.  The reference's own evaluation script (src/emotion_discriminator/evaluate_ed.py) is a copy of the model file.
This is the held-out pass the GAN has in gan/evaluate.py and the VAE in ae/evaluate.py: one pass over a resident split in row
order, eval mode, every statistic accumulated where the batch lies (ops.cls_eval_acc), the one-vs-rest pair counts from the
pass's own stored probabilities (ops.cls_auroc_pairs), and one device -> host read at the end.  The temperature that
minimises the NLL is then applied by a second run of ops.cls_eval_acc over the stored logits: no second forward pass.  The
numbers and their definitions are emotion_discriminator/metrics.py's.

--robustness R (input_mode notes only) repeats the pass R times under each of the training augmentation's three steps alone
and under all three, at the strengths of the config's augment_cfg (else the reference's fallbacks, ed_dataset.py:299-314), and
reports accuracy, cross-entropy and how often the verdict differs from the clean pass's.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Optional

import numpy as np
import torch

from ..checkpoints import ed_state_shapes, read_ed_state, state_mismatches
from ..gan.config import read_config
from ..eval_pass import Packed, ResidentPass, check_split
from ..pieces import EMOTIONS, require_device
from . import metrics as M
from .latent_engine import make_engine

DEFAULT_BATCH = 64
SPLITS = ("test", "val", "train")
AUG_FALLBACK = {"noise_std": 0.01, "dropout_prob": 0.05, "pitch_shift_prob": 0.5}      # ed_dataset.py:303,308; a coin for the shift


class EdEvaluateError(RuntimeError):
    """What every check of this module raises: no device, a config that does not fit the checkpoint or the split, an empty
    split, robustness asked of the latent classifier."""


def class_names(K: int):
    return list(EMOTIONS) if K == len(EMOTIONS) else [str(k) for k in range(K)]


def augment_strengths(cfg: dict) -> dict:
    """The three strengths --robustness uses: the config's augment_cfg where it sets a positive value, else AUG_FALLBACK."""
    acfg = cfg.get("augment_cfg") or {}
    if not isinstance(acfg, dict):
        raise EdEvaluateError(f"augment_cfg must be a mapping, got {type(acfg).__name__}")
    out = {}
    for k, fallback in AUG_FALLBACK.items():
        v = acfg.get(k, 0.0)
        out[k] = float(v) if isinstance(v, (int, float)) and not isinstance(v, bool) and v > 0 else fallback
    return out


class EdEvaluator:
    """One classifier engine (latent_engine.make_engine: either input_mode, spectral norm included) of `batch` rows that only
    ever runs forward(train=False)."""

    def __init__(self, cfg: dict, device="cuda", batch: int = DEFAULT_BATCH, n_bins: int = M.N_BINS):
        from .. import ops
        require_device(EdEvaluateError)
        if int(batch) < 1 or int(batch) > 32767:
            raise EdEvaluateError(f"batch = {batch}: must be in 1..32767")
        if not 1 <= int(n_bins) <= ops.CLS_MAX_BINS:
            raise EdEvaluateError(f"bins = {n_bins}: must be in 1..{ops.CLS_MAX_BINS}")
        K = int(cfg.get("n_classes", 4))
        if not 2 <= K <= ops.CLS_MAX_CLASSES:
            raise EdEvaluateError(f"n_classes = {K}: the evaluation reads 2..{ops.CLS_MAX_CLASSES} classes")
        try:
            self.eng = make_engine(cfg, device, int(batch), int(cfg.get("max_notes", 512)))
        except ValueError as e:
            raise EdEvaluateError(str(e)) from e
        eng = self.eng
        self.cfg, self.B, self.K, self.n_bins = cfg, eng.B, K, int(n_bins)
        self.names = class_names(K)
        self.T_grid, self.inv_temps = M.temperature_grid()
        self.G = len(self.inv_temps)
        d = eng.dev
        self.split_pass = ResidentPass(self.B, d)
        self.ctr, self.base = self.split_pass.ctr, self.split_pass.base      # batch cursor, advanced by mg_cls_eval_acc
        self.serial = torch.zeros(1, dtype=torch.int64, device=d)    # the augmentation's serial base of a robustness pass
        self.labels = torch.zeros(self.B, dtype=torch.int64, device=d)
        self.clean = torch.zeros(self.B, K, device=d)                # the clean pass's logits of the batch (robustness)
        self.words = ops.cls_eval_layout(K, self.n_bins, self.G)["words"]
        self.out = self.acc = self.probs = self.row_d = self.row_i = self.pair_out = None      # one packed buffer, five views
        self.logits = self.aug_logits = None                         # split-position arrays of the last pass
        self.acc_host = self.rows = self.pairs = self.calibrated_host = self.labels_host = None

    # ---- weights --------------------------------------------------------------------------------------------
    def load(self, path: str):
        """train_ed's ed_best.pth / ed_epochNNN.pth ({"model": state_dict, ...}), or a bare state_dict (the reference's
        EmotionDiscriminator.state_dict(), weight_orig / _u / _v under spectral norm).  Every key and shape is checked
        against the config first."""
        # weights_only=False, as this tool always read it: an ed_best.pth carries the training config, whatever its YAML held
        self.load_state(read_ed_state(path, EdEvaluateError, weights_only=False), path)

    def load_state(self, sd: dict, where: str = "state_dict"):
        eng = self.eng
        missing, bad = state_mismatches(sd, ed_state_shapes(eng.cfg, eng.sn_names))
        if missing:
            raise EdEvaluateError(f"{where}: no '{missing[0]}': not a checkpoint of this classifier (input_mode {eng.input_mode}, "
                                  f"use_spectral_norm {bool(eng.sn_names)})")
        if bad:
            raise EdEvaluateError("{}: '{}' has shape {}, the config implies {}".format(where, *bad[0]))
        eng.load_state(sd)          # in place: captured graphs keep their addresses
        self.acc_host = None

    # ---- one batch --------------------------------------------------------------------------------------------
    def _batch(self, jobs, order, order_len, metrics=True):
        """One clean batch.  metrics=False leaves the accumulation out (the pass is then timed without it; the cursor is the
        caller's to advance)."""
        from .. import ops
        eng = self.eng
        ops.stage_rows_cursor(jobs, self.B, order, order_len, self.ctr, self.base)
        eng.forward(train=False)
        ops.scatter_rows_cursor(eng.logits, self._logits_pad, self.ctr, self.base)     # in front of cls_eval_acc, which ticks
        if metrics:
            ops.cls_eval_acc(eng.logits, self.labels, self.acc, self.probs, self.row_i, self.row_d, self.ctr, self.base,
                             self.n_bins, self.inv_temps, tick=self.ctr)

    def _aug_batch(self, x, pad, order, order_len, aug):
        """One augmented batch of a robustness pass: staged through ops.stage_augment, judged against the clean logits."""
        from .. import ops
        eng = self.eng
        ops.stage_augment(x, None, eng.x, None, self.B, order, order_len, self.ctr, self.base, self.serial, aug)
        ops.stage_rows_cursor([(pad, self.labels), (self._logits_pad, self.clean)], self.B, None, order_len, self.ctr, self.base)
        eng.forward(train=False)
        ops.scatter_rows_cursor(eng.logits, self._aug_pad, self.ctr, self.base)
        ops.cls_eval_acc(eng.logits, self.labels, self._aug_acc, self._aug_probs, self._aug_row_i, self._aug_row_d, self.ctr,
                         self.base, self.n_bins, self.inv_temps, clean_logits=self.clean, tick=self.ctr)

    # ---- the pass ---------------------------------------------------------------------------------------------
    def evaluate(self, x: torch.Tensor, labels: torch.Tensor, calibrate_at: Optional[int] = None) -> dict:
        """One pass over a resident split x (n, max_notes, note_dim) or (n, latent_dim) in row order; returns
        metrics.report's block.  labels: the n true classes (int64, on the device); a label outside [0, n_classes) is an
        unlabelled row and counts nowhere.  calibrate_at: the grid index `calibrated` is computed at (default: the argmin of
        the NLL).  Afterwards self.logits (n, K) fp32 and self.probs (n, K) fp64 lie on the device in split order;
        self.acc_host (the accumulator by name), self.rows (the per-row records) and self.pairs are on the host."""
        from .. import ops
        eng, B, K = self.eng, self.B, self.K
        n = check_split(EdEvaluateError, x, tuple(eng.x.shape[1:]), labels)
        if n > ops.CLS_MAX_PAIR_ROWS:
            raise EdEvaluateError(f"evaluate: {n} rows: the exact AUROC counts pairs of at most {ops.CLS_MAX_PAIR_ROWS} rows")

        def build(split):
            self.out = Packed([("acc", (self.words,), torch.int64), ("pairs", (4, K), torch.int64), ("probs", (n, K), torch.float64),
                               ("row_d", (n, 4), torch.float64), ("row_i", (n, 4), torch.int32)], eng.dev)
            self.acc, self.pair_out, self.probs, self.row_d, self.row_i = self.out.dev.values()
            self._logits_pad = torch.zeros(split.rows, K, device=eng.dev)
            self.logits = self._logits_pad[:n]
            split.jobs = [(x, eng.x), (split.labels, self.labels)]
            self._aug_pad = None

        with torch.cuda.stream(eng.stream):
            sp = self.split_pass.bind((x, labels), (n,), n, labels, build)
            self.base.zero_()
            self.split_pass.run("batch", lambda: self._batch(sp.jobs, sp.order, sp.rows), self.out.buf.zero_)
            ops.cls_auroc_pairs(self.probs, labels, self.pair_out)
            host = self.out.host()      # the pass's only device -> host read
        self.acc_host = {k: v.numpy() for k, v in ops.cls_eval_views(host["acc"], K, self.n_bins, self.G).items()}
        self.pairs = host["pairs"].numpy()
        self.rows = {k: host[k].numpy() for k in ("probs", "row_d", "row_i")}
        self.labels_host = sp.labels[:n].cpu().numpy()
        g = calibrate_at
        if g is None:
            total = self.acc_host["nll_T"].sum(axis=0)
            g = int(np.argmin(total)) if int(self.acc_host["rows"].sum()) else M.GRID_ONE
        self.calibrated_host = self.rescored(g)
        rep = M.report(self.acc_host, self.pairs, self.names, self.rows, self.labels_host, self.calibrated_host)
        rep["calibrated"]["T"], rep["calibrated"]["grid_index"] = self.T_grid[g], int(g)
        rep["rows"], rep["batch"], rep["input_mode"] = n, B, eng.input_mode
        return rep

    def rescored(self, g: int) -> dict:
        """The accumulator of the last pass's stored logits at temperature T_g: ops.cls_eval_acc over the stored logits, batch
        by batch in the pass's own cuts, with inv_temperature = 1 / T_g.  No forward pass."""
        from .. import ops
        if self.split_pass.key is None or self.acc_host is None:
            raise EdEvaluateError("rescored: no pass has run")
        if not 0 <= int(g) < self.G:
            raise EdEvaluateError(f"rescored: grid index {g} outside 0..{self.G - 1}")
        eng, B, K = self.eng, self.B, self.K
        sp = self.split_pass.split
        n, nb, pad = sp.n, sp.nb, sp.labels
        with torch.cuda.stream(eng.stream):
            acc = ops.cls_eval_acc_new(K, self.n_bins, self.G, eng.dev)
            probs = torch.zeros(n, K, dtype=torch.float64, device=eng.dev)
            row_i = torch.zeros(n, 4, dtype=torch.int32, device=eng.dev)
            row_d = torch.zeros(n, 4, dtype=torch.float64, device=eng.dev)
            self.ctr.zero_()
            for b in range(nb):
                ops.cls_eval_acc(self._logits_pad[b * B:(b + 1) * B], pad[b * B:(b + 1) * B], acc, probs, row_i, row_d, self.ctr,
                                 self.base, self.n_bins, self.inv_temps, inv_temperature=self.inv_temps[int(g)], tick=self.ctr)
            host = acc.cpu()
        return {k: v.numpy() for k, v in ops.cls_eval_views(host, K, self.n_bins, self.G).items()}

    def robustness(self, x: torch.Tensor, labels: torch.Tensor, aug_params: Optional[dict] = None, repeats: int = 1) -> dict:
        """The verdict under the training augmentation (input_mode notes only): `repeats` passes under each of the `ed`
        program's three steps alone and under all three, staged through ops.stage_augment with distinct serial bases, judged
        against the clean pass's stored logits.  aug_params: {noise_std, dropout_prob, pitch_shift_prob} (default:
        augment_strengths(cfg)).  Afterwards self.aug_logits holds the last pass's logits in split order."""
        from .. import ops
        eng, B, K = self.eng, self.B, self.K
        if eng.input_mode != "notes":
            raise EdEvaluateError("robustness: latent mode has no augmentation (the reference augments notes only)")
        if int(repeats) < 1:
            raise EdEvaluateError(f"robustness: repeats = {repeats}: must be >= 1")
        params = dict(augment_strengths(self.cfg) if aug_params is None else aug_params)
        unknown = sorted(set(params) - set(ops.AUG_ED_KEYS))
        if unknown:
            raise EdEvaluateError(f"robustness: unknown augmentation key(s) {unknown}; known: {list(ops.AUG_ED_KEYS)}")
        n = check_split(EdEvaluateError, x, tuple(eng.x.shape[1:]), labels)
        if eng.C % 4 or x.data_ptr() % 16:
            raise EdEvaluateError("robustness: the augmentation moves 16-byte pieces: note_dim must be a multiple of 4")
        if self.split_pass.key != self.split_pass.key_of((x, labels), n) or self.acc_host is None:
            self.evaluate(x, labels)                # the clean pass these are judged against
        sp = self.split_pass.split
        settings = [(k, {k: params.get(k, 0.0)}) for k in ops.AUG_ED_KEYS] + [("all", {k: params.get(k, 0.0) for k in ops.AUG_ED_KEYS})]
        out = {"repeats": int(repeats), "strengths": {k: float(params.get(k, 0.0)) for k in ops.AUG_ED_KEYS}, "passes": {}}
        with torch.cuda.stream(eng.stream):
            if self._aug_pad is None:
                d = eng.dev
                self._aug_pad = torch.zeros(sp.rows, K, device=d)
                self._aug_acc = ops.cls_eval_acc_new(K, self.n_bins, self.G, d)
                self._aug_probs = torch.zeros(n, K, dtype=torch.float64, device=d)
                self._aug_row_i = torch.zeros(n, 4, dtype=torch.int32, device=d)
                self._aug_row_d = torch.zeros(n, 4, dtype=torch.float64, device=d)
            self.aug_logits = self._aug_pad[:n]
            for si, (name, p) in enumerate(settings):
                try:
                    aug = ops.augment_spec("ed", int(self.cfg.get("seed", 42)), **p)
                except ValueError as e:
                    raise EdEvaluateError(f"robustness: {e}") from e
                # one graph per augmentation setting, kept across calls; the accumulator is zeroed behind a new one's eager run
                gkey = "aug:" + name + ":" + ",".join(repr(float(v)) for v in p.values())
                for rep in range(int(repeats)):
                    self.serial.fill_((si * int(repeats) + rep + 1) * sp.rows)
                    self.split_pass.run(gkey, lambda: self._aug_batch(x, sp.labels, sp.order, sp.rows, aug),
                                        None if rep else self._aug_acc.zero_)
                host = self._aug_acc.cpu()
                v = {k: a.numpy() for k, a in ops.cls_eval_views(host, K, self.n_bins, self.G).items()}
                rows = int(v["rows"].sum())
                out["passes"][name] = {"rows": rows, "accuracy": M._ratio(v["correct"].sum(), rows),
                                       "cross_entropy": M._ratio(v["ce"].sum(), rows), "flipped": int(v["flipped"].sum()),
                                       "flip_rate": M._ratio(v["flipped"].sum(), rows),
                                       "flip_rate_per_class": {nm: M._ratio(v["flipped"][k], v["rows"][k])
                                                               for k, nm in enumerate(self.names)}}
        return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Held-out evaluation of a trained emotion classifier")
    ap.add_argument("--config", type=str, default="config/ed_config.yaml")
    ap.add_argument("--model", type=str, default=None, help="ed_best.pth / ed_epochNNN.pth / a state_dict (not needed with --synthetic)")
    ap.add_argument("--split", type=str, default="test", choices=SPLITS)
    ap.add_argument("--batch", type=int, default=DEFAULT_BATCH)
    ap.add_argument("--bins", type=int, default=M.N_BINS)
    ap.add_argument("--robustness", type=int, default=0, metavar="R", help="R augmented passes per augmentation step (notes mode)")
    ap.add_argument("--out", type=str, default=None, help="report (default <checkpoint_dir>/ed_eval.json)")
    ap.add_argument("--save-probs", type=str, default=None, help="write the pass's probabilities (n, n_classes) float64 here")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N synthetic rows and labels; untrained weights without --model")
    ap.add_argument("--seed", type=int, default=None, help="seed of --synthetic (default: the config's)")
    return ap.parse_args(argv)


def load_rows(cfg: dict, split: str, synthetic: int, seed: int, device):
    """The split as train_ed loads it: (x, labels, source)."""
    from . import train_ed as TR
    latent = cfg.get("input_mode", "latent") == "latent"
    if synthetic:
        if latent:
            x, y = TR.synthetic_latent_split(synthetic, int(cfg.get("latent_dim", 128)), seed, device)
        else:
            x, y = TR.synthetic_split(synthetic, int(cfg.get("max_notes", 512)), int(cfg.get("note_dim", 4)), seed, device)
        return x, y, f"synthetic:{synthetic}"
    try:
        x, y = (TR.load_latent_split if latent else TR.load_split)(cfg, split, device)
        return x, y, TR.split_dir(cfg, split)
    except (ValueError, FileNotFoundError) as e:
        raise EdEvaluateError(str(e)) from e


def run(args) -> dict:
    require_device(EdEvaluateError)
    cfg = read_config(args.config, "config", EdEvaluateError)
    if args.robustness < 0:
        raise EdEvaluateError("--robustness must be >= 0")
    if args.synthetic < 0:
        raise EdEvaluateError("--synthetic must be >= 0")
    if args.model is None and not args.synthetic:
        raise EdEvaluateError("give --model (or --synthetic N)")
    seed = int(cfg.get("seed", 42) if args.seed is None else args.seed)
    ev = EdEvaluator(cfg, "cuda", args.batch, args.bins)
    if args.model is not None:
        ev.load(args.model)
    else:
        ev.eng.init_weights(seed)
    x, y, source = load_rows(cfg, args.split, args.synthetic, seed, ev.eng.dev)
    x, y = x.contiguous(), y.contiguous()
    rep = ev.evaluate(x, y)
    if args.robustness:
        rep["robustness"] = ev.robustness(x, y, None, args.robustness)
    rep.update(model=args.model, split=source)
    out = args.out or os.path.join(cfg.get("checkpoint_dir", "data/models/ed"), "ed_eval.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    if args.save_probs:
        os.makedirs(os.path.dirname(os.path.abspath(args.save_probs)), exist_ok=True)
        np.save(args.save_probs, ev.rows["probs"])
        rep["probs"] = args.save_probs
    with open(out, "w") as f:
        json.dump(rep, f, indent=1, allow_nan=False)
    o, t = rep["overall"], rep["temperature"]
    print(f"classifier evaluation of {source}: {rep['rows']} rows, accuracy {o['accuracy']}, cross_entropy {o['cross_entropy']}, "
          f"macro_f1 {o['macro_f1']}, macro_auroc {o.get('macro_auroc')}, ece {o['ece']}, best T {t['best_T']} "
          f"(nll {t['best_nll']}), calibrated ece {rep['calibrated']['overall']['ece']}")
    print("report ->", out)
    return rep


def main(argv=None) -> int:
    try:
        run(parse_args(argv))
    except EdEvaluateError as e:
        print(f"emotion_discriminator.evaluate: error: {e}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
