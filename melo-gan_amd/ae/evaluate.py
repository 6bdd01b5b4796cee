#!/usr/bin/env python3
"""Held-out evaluation of a trained VAE on the device.

    python -m melo_gan_amd.ae.evaluate --config config/ae_config.yaml --model data/models/ae/ae_best.pth
        [--split val|train|test|PATH/notes.npy] [--labels PATH/emotion.npy] [--batch 64]
        [--out <LOG_DIR>/ae_eval.json] [--save-latents PATH.npy] [--recon-midi N] [--synthetic N]

The reference keeps three loss scalars per epoch and six reconstructed .mid files of its VAE, although the VAE's `mu` is what
the latent-mode classifier trains on and the generator is warm-started from (full_script.sh).  This is the held-out pass the
GAN has in gan/evaluate.py: one pass over a resident split in row order, eval-mode BatchNorm, the reconstruction decoded
from mu (eps = 0, so it is deterministic), every statistic accumulated where the batch lies (ops.vae_eval_acc) and read by
the host once, at the end.  The numbers and their definitions are ae/metrics.py's.

Labels default to <SPLITS_DIR>/<split>/emotion.npy; without that file every row goes to class 0 and the report holds the
`overall` block alone, with fisher_ratio null.  --save-latents writes the pass's mu: the array ae.encode writes.
--recon-midi N writes the N worst and the N best rows by squared error as <out dir>/ae_eval_midi/{worst,best}<i>_row<r>_{in,out}.mid.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Optional

import numpy as np
import torch

from ..checkpoints import load_vae_checkpoint
from ..gan.config import read_config
from ..gan.utils import label_indices
from ..pieces import EMOTIONS, require_device
from ..eval_pass import Packed, ResidentPass, check_split
from . import metrics as M
from .engine import VaeEngine

DEFAULT_BATCH = 64
SPLITS = ("val", "train", "test")


class AeEvaluateError(RuntimeError):
    """What every check of this module raises: no device, a config that does not fit the checkpoint or the split, an empty
    split."""


class VaeEvaluator:
    """One VaeEngine of `batch` rows that only ever runs forward(train=False) with eps = 0.  share: a training engine whose
    parameters, BatchNorm buffers and stream this one reads (train_ae --eval-every); nothing of it is written."""

    def __init__(self, cfg: dict, device="cuda", batch: int = DEFAULT_BATCH, share: Optional[VaeEngine] = None,
                 n_classes: int = len(EMOTIONS)):
        from .. import ops
        require_device(AeEvaluateError)
        if int(batch) < 1 or int(batch) > 32767:
            raise AeEvaluateError(f"batch = {batch}: must be in 1..32767")
        for k in ("MAX_NOTES", "LATENT_DIM"):
            if k not in cfg:
                raise AeEvaluateError(f"the AE config has no {k}")
        if not 1 <= int(cfg["LATENT_DIM"]) <= 1024:
            raise AeEvaluateError(f"LATENT_DIM = {cfg['LATENT_DIM']}: the evaluation reads 1..1024 latent dimensions")
        try:
            self.eng = VaeEngine(cfg, device, int(batch), share=share)
        except ValueError as e:
            raise AeEvaluateError(str(e)) from e
        eng = self.eng
        self.B, self.K = eng.B, int(n_classes)
        d = eng.dev
        self.split_pass = ResidentPass(self.B, d)
        self.ctr, self.base = self.split_pass.ctr, self.split_pass.base           # batch cursor, advanced by mg_vae_eval_acc
        self.labels = torch.zeros(self.B, dtype=torch.int64, device=d)
        self.words = ops.vae_eval_acc_layout(self.K, eng.latent)["words"]
        self.out = self.acc = self.row_d = self.row_i = None         # one packed buffer, three views of it
        self.mu = self.logvar = self.recon = None                    # split-position arrays of the last pass
        self.acc_host = self.rows = None

    def load(self, path: str):
        """The weights and BatchNorm buffers of train_ae's ae_best.pth / ae_final.pth, checked against the config first."""
        load_vae_checkpoint(self.eng, path, AeEvaluateError)

    def _launches(self, jobs, order, order_len, keep_recon, metrics=True):
        """One batch.  metrics=False leaves the accumulation out (the pass is then timed without it; the cursor is the
        caller's to advance)."""
        from .. import ops
        eng = self.eng
        ops.stage_rows_cursor(jobs, self.B, order, order_len, self.ctr, self.base)
        eng.forward(train=False)
        ops.scatter_rows_cursor(eng.mu, self.mu, self.ctr, self.base)       # in front of vae_eval_acc, which advances the cursor
        ops.scatter_rows_cursor(eng.lv, self.logvar, self.ctr, self.base)
        if keep_recon:
            ops.scatter_rows_cursor(eng.recon.view(self.B, -1), self.recon.view(self.recon.shape[0], -1), self.ctr, self.base)
        if metrics:
            ops.vae_eval_acc(eng.x, eng.recon, eng.mu, eng.lv, self.labels, self.acc, self.row_i, self.row_d, self.ctr, self.base,
                             self.K, tick=self.ctr)

    def evaluate(self, notes: torch.Tensor, labels: Optional[torch.Tensor] = None, keep_recon: bool = False, names=None) -> dict:
        """One pass over a resident split notes (n, MAX_NOTES, 4) in row order; returns ae.metrics.report's block.  labels: the
        n true classes (int64, on the device), or None: every row is class 0 and the block holds `overall` alone.  Afterwards
        self.mu / self.logvar (n, L), self.recon (n, T, 4; keep_recon) lie on the device in split order; self.acc_host
        (the accumulator by name) and self.rows (the per-row numbers) are on the host."""
        from .. import ops
        eng, B = self.eng, self.B
        n = check_split(AeEvaluateError, notes, (eng.T, 4), labels, "the split's notes have", labels_optional=True)
        if labels is not None and bool(((labels < 0) | (labels >= self.K)).any()):
            raise AeEvaluateError(f"evaluate: labels outside [0, {self.K})")

        def build(split):
            self.out = Packed([("acc", (self.words,), torch.int64), ("row_d", (n, 4), torch.float64), ("row_i", (n, 8), torch.int32)],
                              eng.dev)
            self.acc, self.row_d, self.row_i = self.out.dev.values()
            self.mu, self.logvar = (torch.zeros(n, eng.latent, device=eng.dev) for _ in range(2))
            self.recon = torch.zeros(n, eng.T, 4, device=eng.dev) if keep_recon else None
            split.jobs = [(notes, eng.x), (split.labels, self.labels)]

        with torch.cuda.stream(eng.stream):
            sp = self.split_pass.bind((notes, labels), (n, bool(keep_recon)), n, labels, build)
            eng.eps.zero_()             # in front of a new graph's eager run too: a shared engine's eps is the trainer's
            self.split_pass.run("batch", lambda: self._launches(sp.jobs, sp.order, sp.rows, keep_recon), self.out.buf.zero_)
            host = self.out.host()      # the pass's only device -> host read
        self.acc_host = {k: v.numpy() for k, v in ops.vae_eval_acc_views(host["acc"], self.K, eng.latent).items()}
        self.rows = {"row_d": host["row_d"].numpy(), "row_i": host["row_i"].numpy()}
        rep = M.report(self.acc_host, eng.T, eng.latent, names)
        rep["rows"], rep["batch"] = n, B
        if labels is None:
            del rep["per_class"]
        return rep


def _split_path(cfg: dict, name: str) -> str:
    return os.path.join(cfg.get("SPLITS_DIR", "data/splits"), name, "notes.npy") if name in SPLITS else name


def _load_notes(path: str, T: int, err) -> np.ndarray:
    if not os.path.isfile(path):
        raise err(f"split array {path} does not exist")
    try:
        notes = np.ascontiguousarray(np.load(path), dtype=np.float32)
    except Exception as e:      # noqa: BLE001 -- any unreadable file is the same user error
        raise err(f"cannot read {path}: {e}") from e
    if notes.ndim != 3 or notes.shape[0] < 1 or tuple(notes.shape[1:]) != (T, 4):
        raise err(f"{path}: an (n, {T}, 4) array with n >= 1 expected, got {notes.shape}")
    return notes


def _load_labels(path: str, n: int, K: int, err) -> np.ndarray:
    try:
        emo = np.load(path, allow_pickle=True)
    except Exception as e:      # noqa: BLE001
        raise err(f"cannot read labels {path}: {e}") from e
    if len(emo) != n:
        raise err(f"{path} holds {len(emo)} entries, the split {n} rows")
    idx = label_indices(emo, None).numpy()
    if ((idx < 0) | (idx >= K)).any():
        raise err(f"{path}: labels outside [0, {K}) (unknown emotion names map to -1)")
    return idx


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Held-out evaluation of a trained VAE")
    ap.add_argument("--config", type=str, default="config/ae_config.yaml")
    ap.add_argument("--model", type=str, default=None, help="ae_best.pth or ae_final.pth (not needed with --synthetic)")
    ap.add_argument("--split", type=str, default="val", help="val | train | test | PATH/notes.npy")
    ap.add_argument("--labels", type=str, default=None, help="emotion.npy (default: next to the split's notes.npy)")
    ap.add_argument("--batch", type=int, default=DEFAULT_BATCH)
    ap.add_argument("--out", type=str, default=None, help="report (default <LOG_DIR>/ae_eval.json)")
    ap.add_argument("--save-latents", type=str, default=None, help="write the pass's mu (n, LATENT_DIM) here")
    ap.add_argument("--recon-midi", type=int, default=0, metavar="N", help="write the N worst and N best reconstructions")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N random rows and labels, untrained weights")
    return ap.parse_args(argv)


def run(args) -> dict:
    from ..midi import save_recon_midi
    require_device(AeEvaluateError)
    cfg = read_config(args.config, "config", AeEvaluateError)
    if args.recon_midi < 0:
        raise AeEvaluateError("--recon-midi must be >= 0")
    ev = VaeEvaluator(cfg, "cuda", args.batch)
    K, T = ev.K, ev.eng.T
    labels_path = None
    if args.synthetic:
        g = torch.Generator().manual_seed(0)
        notes = torch.rand(args.synthetic, T, 4, generator=g) * 2 - 1
        idx = np.arange(args.synthetic, dtype=np.int64) % K
        ev.eng.init_weights(0)
        source = f"synthetic:{args.synthetic}"
    else:
        if args.model is None:
            raise AeEvaluateError("give --model (or --synthetic N)")
        path = _split_path(cfg, args.split)
        notes = torch.from_numpy(_load_notes(path, T, AeEvaluateError))
        labels_path = args.labels or os.path.join(os.path.dirname(path), "emotion.npy")
        if args.labels and not os.path.isfile(labels_path):
            raise AeEvaluateError(f"labels {labels_path} do not exist")
        idx = _load_labels(labels_path, notes.shape[0], K, AeEvaluateError) if os.path.isfile(labels_path) else None
        ev.load(args.model)
        source = path
    dev_notes = notes.cuda()
    dev_labels = None if idx is None else torch.from_numpy(idx).cuda()
    rep = ev.evaluate(dev_notes, dev_labels, keep_recon=args.recon_midi > 0, names=EMOTIONS)
    rep.update(model=args.model, split=source, labels=labels_path if idx is not None and not args.synthetic else None)
    out = args.out or os.path.join(cfg.get("LOG_DIR", "experiments/ae"), "ae_eval.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    if args.save_latents:
        os.makedirs(os.path.dirname(os.path.abspath(args.save_latents)), exist_ok=True)
        np.save(args.save_latents, ev.mu.cpu().numpy())
        rep["latents"] = args.save_latents
    if args.recon_midi:
        se = ev.rows["row_d"][:, 0]
        by_err = np.argsort(se, kind="stable")
        n_each = min(args.recon_midi, len(se))
        midi_dir = os.path.join(os.path.dirname(os.path.abspath(out)), "ae_eval_midi")
        rep["recon_midi"] = {"dir": midi_dir}
        recon = ev.recon.cpu().numpy()
        for tag, rows in (("worst", by_err[::-1][:n_each]), ("best", by_err[:n_each])):
            rep["recon_midi"][tag] = []
            for i, r in enumerate(rows):
                prefix = f"{tag}{i}_row{int(r):06d}"
                save_recon_midi(notes[int(r)].numpy(), recon[int(r)], midi_dir, prefix)
                rep["recon_midi"][tag].append({"row": int(r), "squared_error": float(se[r]), "mse": float(se[r]) / (4 * T),
                                               "files": [f"{prefix}_in.mid", f"{prefix}_out.mid"]})
    with open(out, "w") as f:
        json.dump(rep, f, indent=1, allow_nan=False)
    o = rep["overall"]
    print(f"VAE evaluation of {source}: {rep['rows']} rows, recon_mse {o['recon_mse']}, kld_mean {o['kld_mean']}, "
          f"active_units {o['active_units']}/{rep['latent_dim']}, latent_std {o['latent_std']}, "
          f"pitch_accuracy {o['pitch_accuracy']}, onset_recall {o['onset_recall']}, fisher_ratio {o['fisher_ratio_mean']}")
    if o["latent_warning"]:
        print("[WARNING]", o["latent_warning"])
    print("report ->", out)
    return rep


def main(argv=None) -> int:
    try:
        run(parse_args(argv))
    except AeEvaluateError as e:
        print(f"ae.evaluate: error: {e}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
