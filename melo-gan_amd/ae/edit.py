#!/usr/bin/env python3
"""Edit pieces in a trained VAE's latent space: variations, a morph between two pieces, a shift towards another emotion.

    python -m melo_gan_amd.ae.edit --config config/ae_config.yaml --model data/models/ae/ae_best.pth
        [--split val|train|test|PATH/notes.npy] [--labels PATH/emotion.npy]
        ( --prior N [--temperature 1.0]
        | --vary ROWS --samples N [--sigma 1.0]
        | --from ROW --to ROW [--steps 8] [--interp lerp|slerp]
        | --shift ROWS --to EMOTION [--strength 0.5,1,1.5] [--centroids train|val|PATH/notes.npy] )
        [--seed S] [--batch 64] [--out DIR] [--bpm 120] [--scale chromatic] [--join]
        [--ed_config config/ed_config.yaml --ed_ckpt data/models/ed/ed_best.pth]
        [--wav [--wav-fs 44100] [--voice piano]] [--no-files] [--synthetic N]

train_ae, ae.encode and ae.evaluate only ever run the decoder on what the encoder has just produced.  Here the decoder's input is
written by mg_latent_rows: z = base + alpha * direction + sigma * std * N(0, I) per output row (ae/latent_edit.py builds the row
descriptors).  ROWS are comma-separated row indices of the split's notes.npy; other .mid files become such rows through
melo_gan_amd.midi_import, which reports what of a file the roll contract cannot hold.  --prior samples z ~ temperature * N(0, I); --vary draws around each piece's posterior mean;
--from / --to walks between two pieces' means; --shift moves a piece along (mean latent of the target emotion) - (mean latent of
its own emotion), both taken from one VaeEvaluator pass over the --centroids split (default: train), so that strength 1 carries
the source class mean onto the target's.  --shift needs labels: <split dir>/emotion.npy or --labels.

The needed source rows are encoded once; their mu / logvar stay resident.  One hipGraph per run -- stage the chunk's descriptors
-> mg_latent_rows -> decode -> recon -> x -> encode -> mg_latent_cycle -> scatter z, recon, mu2 and the cycle words to their
output positions -- is replayed per chunk of `batch` rows (eval_pass.CursorPass; a trailing partial chunk is padded with kind-0
rows), and the run ends with one device -> host read.  After the requested rows the run holds one identity row per source: the source's own
reconstruction, which the note-level change and the classifier's `before` are measured against.

Writes (unless --no-files) prior_<k>.mid, vary_r<row>_<k>.mid, path_r<a>_r<b>_s<ss>.mid (--join: also path_r<a>_r<b>.mid, the
first 64 notes of every step one after the other) or shift_r<row>_<emotion>_<j>.mid through midi.save_piano_roll_to_midi; --shift
decodes with the target emotion's scale and tempo (pieces.STYLE), the other modes with --scale / --bpm.  <out>/edit.json holds
per output row its descriptors, latent_step = |z - mu_a|, cycle_error = |mu2 - z|, for shifts requested = (z - mu_a).d / d.d and
realised = (mu2 - mu_a).d / d.d, the note-level change against the source's own reconstruction and, with a classifier, its
verdict before and after; and one summary block of their means (per strength for --shift).  Every check raises AeEditError; the
tool prints `ae.edit: error: ...` and returns status 2.
"""
from __future__ import annotations

import argparse
import json
import os
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from .. import ops
from ..checkpoints import load_vae_checkpoint
from ..eval_pass import CursorPass, Packed
from ..gan.config import read_config
from ..pieces import EMOTIONS, STYLE, add_wav_arguments, joined_notes, plan_wav, require_device, run_tool, write_pieces
from . import latent_edit as LE
from .engine import VaeEngine
from .evaluate import AeEvaluateError, VaeEvaluator, _load_labels, _load_notes, _split_path

DEFAULT_BATCH = 64
JOIN_NOTES = 64


class AeEditError(RuntimeError):
    """What every check of this module raises."""


@dataclass
class EditResult:
    """Host arrays of one run, the requested rows first, then one identity row per source (rows.sources order)."""
    z: np.ndarray               # (R + n_src, L) float32
    recon: np.ndarray           # (R + n_src, T, 4) float32
    mu2: np.ndarray             # (R + n_src, L) float32
    cycle: np.ndarray           # (R + n_src, 6) float64
    scores: Optional[dict]
    R: int

    def source_row(self, rows: LE.Rows, r: int) -> Optional[int]:
        """Where the identity row of output row r's source lies (None for a prior row)."""
        return self.R + int(rows.src_a[r]) if int(rows.kind[r]) == LE.KIND_POST else None


DESCRIPTORS = (("kind", torch.int32, ()), ("src_a", torch.int32, ()), ("src_b", torch.int32, ()), ("t", torch.float32, ()),
               ("dir", torch.int32, ()), ("alpha", torch.float32, ()), ("sigma", torch.float32, ()), ("key", torch.int32, (2,)))


class LatentEditor:
    """One eval-mode VaeEngine of `batch` rows behind mg_latent_rows."""

    def __init__(self, cfg: dict, device="cuda", batch: int = DEFAULT_BATCH):
        require_device(AeEditError)
        if int(batch) < 1 or int(batch) > 32767:
            raise AeEditError(f"batch = {batch}: must be in 1..32767")
        check_ae_config(cfg)
        try:
            self.eng = VaeEngine(cfg, device, int(batch))
        except ValueError as e:
            raise AeEditError(str(e)) from e
        eng = self.eng
        self.B = eng.B
        d = eng.dev
        self.cur = CursorPass(d)
        self.desc = {n: torch.zeros((self.B,) + s, dtype=dt, device=d) for n, dt, s in DESCRIPTORS}    # the chunk's descriptors
        self.cyc = torch.zeros(self.B, 6, dtype=torch.float64, device=d)
        self.graphs = self.cur.graphs
        self.shape = None                   # what the resident arrays below were allocated for
        self.res = self.all = self.mu = self.logvar = self.dirs = None

    def load(self, path: str):
        """The weights and BatchNorm buffers of train_ae's ae_best.pth / ae_final.pth, checked against the config first."""
        load_vae_checkpoint(self.eng, path, AeEditError)

    # ---- one chunk --------------------------------------------------------------------------------------------
    def _launches(self, seed: int, interp: int):
        eng, B, a, c, ctr, base = self.eng, self.B, self.all, self.desc, self.cur.ctr, self.cur.base
        ops.stage_rows_cursor([(a[n], c[n]) for n, _, _ in DESCRIPTORS], B, None, a["kind"].shape[0], ctr, base)
        ops.latent_rows(self.mu, self.logvar, self.dirs, c["kind"], c["src_a"], c["src_b"], c["t"], c["dir"], c["alpha"], c["sigma"],
                        c["key"], eng.zl, interp, seed)
        eng.decode(False)
        ops.copy_cols(eng.recon.view(B, -1), 0, eng.x.view(B, -1), 0, eng.T * 4)
        eng.encode(False)
        ops.latent_cycle(eng.zl, eng.mu, self.mu, self.dirs, c["kind"], c["src_a"], c["dir"], self.cyc)
        d = self.res.dev
        ops.scatter_rows_cursor(eng.zl, d["z"], ctr, base)
        ops.scatter_rows_cursor(eng.recon.view(B, -1), d["recon"], ctr, base)
        ops.scatter_rows_cursor(eng.mu, d["mu2"], ctr, base)
        ops.scatter_rows_cursor(self.cyc.view(torch.float32), d["cycle"].view(torch.float32), ctr, base)

    def _encode_sources(self, notes: torch.Tensor, sources: List[int]):
        """mu / logvar of the source rows, in chunks of `batch` in `sources` order (a trailing chunk's free slots hold zeros)."""
        eng, B = self.eng, self.B
        idx = torch.tensor(sources, dtype=torch.int64, device=eng.dev)
        for c0 in range(0, len(sources), B):
            n = min(B, len(sources) - c0)
            eng.x.zero_()
            eng.x[:n].copy_(notes.index_select(0, idx[c0:c0 + n]))
            eng.encode(False)
            self.mu[c0:c0 + n].copy_(eng.mu[:n])
            self.logvar[c0:c0 + n].copy_(eng.lv[:n])

    def run(self, notes: Optional[torch.Tensor], rows: LE.Rows, seed: int, centroids=None, ed=None) -> EditResult:
        """The rows' latents, decodings and re-encodings.  notes: the resident split (n, MAX_NOTES, 4) the rows' sources index
        (None when there are none).  centroids: latent_edit.centroids()'s result, or its (K, K, L) difference table, whose row
        label * K + target a shift row names.  ed: emotion_discriminator.evaluate.EdEvaluator with its weights loaded."""
        eng, B = self.eng, self.B
        d, Ld, T = eng.dev, eng.latent, eng.T
        if not isinstance(rows, LE.Rows) or rows.R < 1:
            raise AeEditError("run: at least one output row is needed")
        R, n_src = rows.R, len(rows.sources)
        if n_src:
            if not isinstance(notes, torch.Tensor) or not notes.is_cuda or notes.dtype != torch.float32 or notes.dim() != 3 or \
                    tuple(notes.shape[1:]) != (T, 4):
                raise AeEditError(f"run: the split must be an fp32 device array of shape (n, {T}, 4)")
            if min(rows.sources) < 0 or max(rows.sources) >= notes.shape[0]:
                raise AeEditError(f"run: source rows {min(rows.sources)}..{max(rows.sources)} lie outside the split of {notes.shape[0]} rows")
        post = rows.kind == LE.KIND_POST
        if (~np.isin(rows.kind, (LE.KIND_PAD, LE.KIND_PRIOR, LE.KIND_POST))).any() or \
                (post & ((rows.src_a < 0) | (rows.src_a >= n_src) | (rows.src_b < 0) | (rows.src_b >= n_src))).any():
            raise AeEditError("run: a row's kind or source index lies outside its range")
        dirs_host = None
        if (rows.dir >= 0).any():
            if centroids is None:
                raise AeEditError("run: rows with a direction need the class means (centroids)")
            diff = np.asarray(centroids[2] if isinstance(centroids, tuple) else centroids, np.float64)
            if diff.ndim != 3 or diff.shape[0] != diff.shape[1] or diff.shape[2] != Ld:
                raise AeEditError(f"run: a (K, K, {Ld}) difference table expected, got {diff.shape}")
            dirs_host = diff.reshape(-1, Ld)
            used = np.unique(rows.dir[rows.dir >= 0])
            if used.max() >= dirs_host.shape[0]:
                raise AeEditError(f"run: direction {int(used.max())} lies outside the table's {dirs_host.shape[0]} rows")
            if not np.isfinite(dirs_host[used]).all():
                raise AeEditError("run: a direction runs from or to a class without rows: it has no mean")
            dirs_host = np.nan_to_num(dirs_host, nan=0.0).astype(np.float32)          # the unused rows of empty classes
        n_dir = 0 if dirs_host is None else dirs_host.shape[0]
        if ed is not None:
            check_classifier(ed.eng, T, Ld)
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        R_all = R + n_src                                       # the requested rows, then one identity row per source
        nb = (R_all + B - 1) // B
        R_pad = nb * B
        host = {n: np.zeros((R_pad,) + s, dtype=torch.zeros(0, dtype=dt).numpy().dtype) for n, dt, s in DESCRIPTORS}
        host["dir"][:] = -1
        for n, _, _ in DESCRIPTORS:
            host[n][:R] = getattr(rows, n)
        ref = slice(R, R_all)
        host["kind"][ref] = LE.KIND_POST
        host["src_a"][ref] = host["src_b"][ref] = np.arange(n_src)
        host["key"][ref, 0] = rows.sources
        with torch.cuda.stream(eng.stream):
            shape = (R_pad, n_src, n_dir)
            if self.shape != shape:                             # the captured graphs hold these addresses
                self.graphs.clear()
                self.res = Packed([("cycle", (R_pad, 6), torch.float64), ("z", (R_pad, Ld), torch.float32),
                                   ("recon", (R_pad, T * 4), torch.float32), ("mu2", (R_pad, Ld), torch.float32),
                                   ("score_f", (3, 2, R_pad), torch.float32), ("score_i", (3, R_pad), torch.int32)], d)
                self.all = {n: torch.zeros((R_pad,) + s, dtype=dt, device=d) for n, dt, s in DESCRIPTORS}
                self.mu = torch.zeros(n_src, Ld, device=d) if n_src else None
                self.logvar = torch.zeros(n_src, Ld, device=d) if n_src else None
                self.dirs = torch.zeros(n_dir, Ld, device=d) if n_dir else None
                self.shape = shape
            for n in host:
                self.all[n].copy_(torch.from_numpy(host[n]))
            if n_dir:
                self.dirs.copy_(torch.from_numpy(dirs_host))
            if n_src:
                self._encode_sources(notes, rows.sources)
            key = (seed, int(rows.interp))
            if key not in self.graphs:                          # the seed and interp are launch arguments the capture froze
                self.graphs.clear()
            self.cur.replay(key, lambda: self._launches(*key), nb, self.res.buf.zero_)
            scored = self._score(ed, rows, host, R, R_all) if ed is not None else None
            out = self.res.host()                               # the run's one device -> host read; synchronises the stream
        scores = None
        if scored:
            sf, si = out["score_f"].numpy(), out["score_i"].numpy()
            scores = {when: {"p_target": sf[i, 0, :R].copy(), "p_source": sf[i, 1, :R].copy(), "pred": si[i, :R].copy()}
                      for i, when in enumerate(("before", "after", "cycled")) if when in scored}
            prior = rows.kind != LE.KIND_POST
            scores["before"]["pred"][prior] = -1                # a prior row has no source
        return EditResult(out["z"].numpy()[:R_all].copy(), out["recon"].numpy()[:R_all].reshape(R_all, T, 4).copy(),
                          out["mu2"].numpy()[:R_all].copy(), out["cycle"].numpy()[:R_all].copy(), scores, R)

    def _score(self, ed, rows: LE.Rows, host: dict, R: int, R_all: int):
        """The classifier over the resident results, in chunks of its own batch: `after` scores the decoded rolls (input_mode
        notes) or z (latent), `cycled` mu2 (latent only), `before` the identity row of each row's source.  Per row the
        probability of its target and of its source label and the prediction (mg_emotion_score) go into the packed result."""
        e, d = ed.eng, self.res.dev
        dev, K, R_pad = e.dev, e.n_classes, d["z"].shape[0]
        latent = e.input_mode == "latent"
        inputs = {"after": d["z"] if latent else d["recon"]}
        if latent:
            inputs["cycled"] = d["mu2"]
        tgt = torch.full((R_pad,), -1, dtype=torch.int32, device=dev)
        src = torch.full((R_pad,), -1, dtype=torch.int32, device=dev)
        if rows.target is not None:
            tgt[:R].copy_(torch.from_numpy(np.ascontiguousarray(rows.target, np.int32)))
            src[:R].copy_(torch.from_numpy(np.ascontiguousarray(rows.source_label, np.int32)))
        before_of = np.arange(R_pad, dtype=np.int64)
        before_of[:R] = np.where(rows.kind == LE.KIND_POST, R + rows.src_a.astype(np.int64), np.arange(R))
        before_of = torch.from_numpy(before_of).to(dev)
        acc = torch.zeros(K, 3, dtype=torch.float64, device=dev)
        pred2 = torch.zeros(R_pad, dtype=torch.int32, device=dev)
        logits = {}
        for when, x in inputs.items():
            lg = torch.zeros(R_pad, K, device=dev)
            for c0 in range(0, R_all, e.B):
                n = min(e.B, R_all - c0)
                e.x.zero_()
                e.x[:n].copy_(x[c0:c0 + n].view((n,) + tuple(e.x.shape[1:])))
                e.forward(train=False)
                lg[c0:c0 + n].copy_(e.logits[:n])
            logits[when] = lg
        logits["before"] = logits["after"].index_select(0, before_of).contiguous()
        for i, when in enumerate(("before", "after", "cycled")):
            if when in logits:
                ops.emotion_score(logits[when], tgt, d["score_f"][i, 0], d["score_i"][i], acc)
                ops.emotion_score(logits[when], src, d["score_f"][i, 1], pred2, acc)
            else:
                d["score_i"][i].fill_(-1)
        return set(logits)


def check_ae_config(cfg: dict):
    for k in ("MAX_NOTES", "LATENT_DIM"):
        if k not in cfg:
            raise AeEditError(f"the AE config has no {k}")
    if not 1 <= int(cfg["LATENT_DIM"]) <= LE.MAX_L:
        raise AeEditError(f"LATENT_DIM = {cfg['LATENT_DIM']}: the latent kernels read 1..{LE.MAX_L} dimensions")
    if int(cfg["MAX_NOTES"]) < 8:
        raise AeEditError(f"MAX_NOTES = {cfg['MAX_NOTES']}: must be >= 8")


def check_classifier(e, T: int, Ld: int):
    """The classifier's input against what the VAE hands it: rolls of (T, 4) in notes mode, latents of Ld in latent mode."""
    if e.input_mode == "latent":
        if int(e.D) != Ld:
            raise AeEditError(f"the classifier reads latents of {e.D} dimensions, the VAE has LATENT_DIM {Ld}")
    elif (int(e.T), int(e.C)) != (T, 4):
        raise AeEditError(f"the classifier reads rolls of ({e.T}, {e.C}), the VAE decodes ({T}, 4)")
    if e.n_classes > 32:
        raise AeEditError(f"n_classes = {e.n_classes}: at most 32")


# ---------------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m melo_gan_amd.ae.edit", description="Edit pieces in a trained VAE's latent space.")
    ap.add_argument("--config", type=str, default="config/ae_config.yaml")
    ap.add_argument("--model", type=str, default=None, help="ae_best.pth or ae_final.pth (not needed with --synthetic)")
    ap.add_argument("--split", type=str, default="val", help="val | train | test | PATH/notes.npy: where ROWS point")
    ap.add_argument("--labels", type=str, default=None, help="emotion.npy (default: next to the split's notes.npy)")
    ap.add_argument("--prior", type=int, default=None, metavar="N", help="N samples of the prior")
    ap.add_argument("--temperature", type=float, default=1.0, help="--prior: the scale of the normal draws")
    ap.add_argument("--vary", type=str, default=None, metavar="ROWS", help="variations of these rows, e.g. 3,17")
    ap.add_argument("--samples", type=int, default=None, metavar="N", help="--vary: variations per row")
    ap.add_argument("--sigma", type=float, default=1.0, help="--vary: the scale of the posterior's standard deviation")
    ap.add_argument("--from", dest="from_", type=int, default=None, metavar="ROW", help="the row a path starts at")
    ap.add_argument("--to", type=str, default=None, help="the row a path ends at, or the emotion a shift moves towards")
    ap.add_argument("--steps", type=int, default=8, help="--from / --to: steps of the path (it has steps + 1 points)")
    ap.add_argument("--interp", type=str, default="lerp", help="--from / --to: lerp or slerp")
    ap.add_argument("--shift", type=str, default=None, metavar="ROWS", help="move these rows towards the emotion --to")
    ap.add_argument("--strength", type=str, default="0.5,1,1.5", help="--shift: multiples of the class-mean difference")
    ap.add_argument("--centroids", type=str, default="train", help="--shift: the split whose class means give the direction")
    ap.add_argument("--seed", type=int, default=None, help="sampling seed (default SEED, else 42)")
    ap.add_argument("--batch", type=int, default=DEFAULT_BATCH, help="rows per replayed chunk")
    ap.add_argument("--out", type=str, default=None, help="output directory (default <LOG_DIR>/ae_edit)")
    ap.add_argument("--bpm", type=float, default=120.0)
    ap.add_argument("--scale", type=str, default="chromatic")
    ap.add_argument("--join", action="store_true", help="--from / --to: also write the steps one after the other as one piece")
    ap.add_argument("--ed_config", type=str, default=None, help="ED config of the classifier that scores the rows")
    ap.add_argument("--ed_ckpt", type=str, default=None, help="ED checkpoint (ed_best.pth)")
    add_wav_arguments(ap, help_wav="also render every .mid to a .wav", help_fs=None, help_voice=None)
    ap.add_argument("--no-files", action="store_true", help="write edit.json only")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N random rows and labels, untrained weights")
    return ap.parse_args(argv)


def parse_rows(text: str, flag: str) -> List[int]:
    out = []
    for part in str(text).split(","):
        try:
            out.append(int(part.strip()))
        except ValueError:
            raise AeEditError(f"{flag}: {part!r} is not a row index") from None
    return out


def parse_strengths(text: str) -> List[float]:
    out = []
    for part in str(text).split(","):
        try:
            out.append(float(part.strip()))
        except ValueError:
            raise AeEditError(f"--strength: {part!r} is not a number") from None
        if not np.isfinite(out[-1]):
            raise AeEditError(f"--strength: {part!r} is not finite")
    return out


@dataclass
class Plan:
    cfg: dict
    ed_cfg: Optional[dict]
    model: Optional[str]
    ed_ckpt: Optional[str]
    mode: str
    rows: LE.Rows
    notes: Optional[np.ndarray]
    labels: Optional[np.ndarray]
    source: str
    centroid_notes: Optional[np.ndarray]
    centroid_labels: Optional[np.ndarray]
    centroid_source: Optional[str]
    target: Optional[int]
    out: str
    seed: int
    batch: int
    bpm: float
    scale: str
    files: bool
    join: bool
    wav: Optional[dict]
    synthetic: int


def plan(args) -> Plan:
    """Every check of what comes from outside, on the host (no GPU needed); raises AeEditError."""
    from .. import midi
    K = len(EMOTIONS)
    modes = [m for m, on in (("prior", args.prior is not None), ("vary", args.vary is not None), ("path", args.from_ is not None),
                             ("shift", args.shift is not None)) if on]
    if len(modes) != 1:
        raise AeEditError("exactly one of --prior N, --vary ROWS, --from ROW --to ROW and --shift ROWS --to EMOTION is needed")
    mode = modes[0]
    if mode in ("path", "shift") and args.to is None:
        raise AeEditError("--from ROW needs --to ROW" if mode == "path" else "--shift ROWS needs --to EMOTION")
    if mode in ("prior", "vary") and args.to is not None:
        raise AeEditError("--to goes with --from ROW or --shift ROWS")
    if args.batch < 1:
        raise AeEditError(f"--batch {args.batch}: must be >= 1")
    if args.synthetic < 0:
        raise AeEditError(f"--synthetic {args.synthetic}: must be >= 0")
    for flag, v in (("--prior", args.prior), ("--samples", args.samples), ("--steps", args.steps if mode == "path" else None)):
        if v is not None and v < 1:
            raise AeEditError(f"{flag} {v}: must be >= 1")
    for flag, v in (("--temperature", args.temperature), ("--sigma", args.sigma)):
        if not np.isfinite(v) or v < 0:
            raise AeEditError(f"{flag} {v}: must be finite and >= 0")
    if mode == "path" and args.interp not in LE.INTERP:
        raise AeEditError(f"--interp {args.interp!r}: expected one of {', '.join(LE.INTERP)}")
    files = not args.no_files
    wav = plan_wav(args, AeEditError, files, args.join, "edit.json")
    if args.join and mode != "path":
        raise AeEditError("--join joins the steps of a path: it needs --from ROW --to ROW")
    if args.scale not in midi.SCALES:
        raise AeEditError(f"--scale {args.scale!r}: expected one of {', '.join(sorted(midi.SCALES))}")
    if not np.isfinite(args.bpm) or args.bpm <= 0:
        raise AeEditError(f"--bpm {args.bpm}: must be positive")
    target = None
    if mode == "shift":
        if str(args.to).lower() not in EMOTIONS:
            raise AeEditError(f"--to {args.to!r}: expected one of {', '.join(EMOTIONS)}")
        target = EMOTIONS.index(str(args.to).lower())
        strengths = parse_strengths(args.strength)
        pieces = parse_rows(args.shift, "--shift")
    elif mode == "path":
        try:
            to_row = int(args.to)
        except ValueError:
            raise AeEditError(f"--to {args.to!r}: a row index expected after --from") from None
    elif mode == "vary":
        if args.samples is None:
            raise AeEditError("--vary ROWS needs --samples N")
        pieces = parse_rows(args.vary, "--vary")
    if (args.ed_ckpt is None) != (args.ed_config is None):
        raise AeEditError("--ed_config and --ed_ckpt go together")
    cfg = read_config(args.config, "config", AeEditError)
    check_ae_config(cfg)
    T = int(cfg["MAX_NOTES"])
    notes = labels = c_notes = c_labels = c_source = None
    if args.synthetic:
        g = torch.Generator().manual_seed(0)
        notes = (torch.rand(args.synthetic, T, 4, generator=g) * 2 - 1).numpy()
        labels = np.arange(args.synthetic, dtype=np.int64) % K
        source = f"synthetic:{args.synthetic}"
    elif mode != "prior":
        path = _split_path(cfg, args.split)
        notes = _load_notes(path, T, AeEditError)
        source = path
        lp = args.labels or os.path.join(os.path.dirname(path), "emotion.npy")
        if os.path.isfile(lp):
            labels = _load_labels(lp, notes.shape[0], K, AeEditError)
        elif args.labels:
            raise AeEditError(f"labels {lp} do not exist")
    else:
        source = "prior"
    if mode == "shift" and labels is None:
        raise AeEditError("--shift needs labels: give --labels PATH/emotion.npy or put emotion.npy next to the split's notes.npy")
    n_split = None if notes is None else notes.shape[0]
    try:
        if mode == "prior":
            rows = LE.prior_rows(args.prior, args.temperature)
        elif mode == "vary":
            rows = LE.vary_rows(pieces, args.samples, args.sigma, n_split)
        elif mode == "path":
            rows = LE.path_rows(args.from_, to_row, args.steps, args.interp, n_split)
        else:
            LE.check_pieces(pieces, n_split, "shift")                  # in front of labels[p]
            rows = LE.shift_rows(pieces, [int(labels[p]) for p in pieces], target, strengths, K, n_split)
    except LE.LatentEditError as e:
        raise AeEditError(str(e)) from e
    if mode == "shift":
        if args.synthetic:
            c_notes, c_labels, c_source = notes, labels, source
        else:
            c_source = _split_path(cfg, args.centroids)
            c_notes = _load_notes(c_source, T, AeEditError)
            clp = os.path.join(os.path.dirname(c_source), "emotion.npy")
            if not os.path.isfile(clp):
                raise AeEditError(f"--centroids: {clp} does not exist: the class means need labels")
            c_labels = _load_labels(clp, c_notes.shape[0], K, AeEditError)
        for k in sorted({target} | {int(labels[p]) for p in pieces}):
            if not (c_labels == k).any():
                raise AeEditError(f"--centroids: {c_source} has no row of class {EMOTIONS[k]}: it has no mean")
    if not args.synthetic:
        if args.model is None:
            raise AeEditError("give --model (or --synthetic N)")
        if not os.path.isfile(args.model):
            raise AeEditError(f"checkpoint {args.model} does not exist")
    ed_cfg = None
    if args.ed_config is not None:
        ed_cfg = read_config(args.ed_config, "ED config", AeEditError)
        if not os.path.isfile(args.ed_ckpt):
            raise AeEditError(f"ED checkpoint {args.ed_ckpt} does not exist")
    out = args.out or os.path.join(cfg.get("LOG_DIR", "experiments/ae"), "ae_edit")
    seed = args.seed if args.seed is not None else int(cfg.get("SEED", 42))
    return Plan(cfg, ed_cfg, args.model, args.ed_ckpt, mode, rows, notes, labels, source, c_notes, c_labels, c_source, target, out,
                seed, args.batch, float(args.bpm), args.scale, files, bool(args.join), wav, args.synthetic)


def file_name(p: Plan, r: int) -> str:
    rows = p.rows
    piece, k = int(rows.key[r, 0]), int(rows.key[r, 1])
    if p.mode == "prior":
        return f"prior_{k}.mid"
    if p.mode == "vary":
        return f"vary_r{piece}_{k}.mid"
    if p.mode == "path":
        return f"path_r{rows.sources[int(rows.src_a[r])]}_r{rows.sources[int(rows.src_b[r])]}_s{k:02d}.mid"
    return f"shift_r{piece}_{EMOTIONS[p.target]}_{k}.mid"


def write_files(p: Plan, res: EditResult) -> List[dict]:
    """The .mid (and --wav: .wav) files of a run; returns edit.json's files[] entries, one per output row first."""
    scale, bpm = (STYLE[EMOTIONS[p.target]][0], float(STYLE[EMOTIONS[p.target]][1])) if p.mode == "shift" else (p.scale, p.bpm)
    todo = [({"file": file_name(p, r), "row": r, "bpm": bpm, "scale": scale}, (res.recon[r], scale, bpm)) for r in range(res.R)]
    if p.join:
        a, b = p.rows.sources[int(p.rows.src_a[0])], p.rows.sources[int(p.rows.src_b[0])]
        n = min(JOIN_NOTES, res.recon.shape[1])
        todo.append(({"file": f"path_r{a}_r{b}.mid", "joined": True, "join_notes": n},
                     joined_notes(list(res.recon[:res.R]), [(scale, bpm)] * res.R, n)))
    return write_pieces(p.out, todo, p.wav)


def build_report(p: Plan, res: EditResult, files: List[dict], counts=None) -> dict:
    """edit.json."""
    rows = p.rows
    refs = [res.source_row(rows, r) for r in range(res.R)]
    changes = LE.note_change(res.recon[[i if i is not None else r for r, i in enumerate(refs)]], res.recon[:res.R])
    notes = [c if i is not None else None for c, i in zip(changes, refs)]
    try:
        rep = LE.report(rows, res.cycle[:res.R], notes, res.scores, EMOTIONS)
    except LE.LatentEditError as e:
        raise AeEditError(str(e)) from e
    for f in files:
        if "row" in f:
            rep["rows"][f["row"]]["file"] = f["file"]
    rep.update(model=p.model, split=p.source, seed=p.seed, batch=p.batch, files=files, ed_checkpoint=p.ed_ckpt,
               classifier_input=None if p.ed_cfg is None else p.ed_cfg.get("input_mode", "latent"))
    if p.mode == "shift":
        rep["centroids"] = {"split": p.centroid_source, "target": EMOTIONS[p.target],
                            "counts": None if counts is None else {e: int(c) for e, c in zip(EMOTIONS, counts)}}
    if p.wav is not None:
        rep["wav"] = dict(p.wav)
    return rep


def run(p: Plan) -> dict:
    require_device()
    ed =LatentEditor(p.cfg, "cuda", p.batch)
    if p.synthetic:
        ed.eng.init_weights(0)
    else:
        ed.load(p.model)
    cls = None
    if p.ed_cfg is not None:
        from ..emotion_discriminator.evaluate import EdEvaluateError, EdEvaluator
        try:
            cls = EdEvaluator(p.ed_cfg, "cuda", p.batch)
            cls.load(p.ed_ckpt)
        except EdEvaluateError as e:
            raise AeEditError(f"classifier: {e}") from e
        check_classifier(cls.eng, ed.eng.T, ed.eng.latent)
    cent = counts = None
    if p.mode == "shift":
        try:
            ev = VaeEvaluator(p.cfg, "cuda", p.batch, share=ed.eng, n_classes=len(EMOTIONS))
            ev.evaluate(torch.from_numpy(p.centroid_notes).cuda(), torch.from_numpy(p.centroid_labels).cuda())
            need = sorted({p.target} | {int(v) for v in p.rows.source_label})
            cent = LE.centroids(ev.acc_host, need)
        except (AeEvaluateError, LE.LatentEditError) as e:
            raise AeEditError(f"--centroids: {e}") from e
        counts = cent[1]
    dev_notes = None if p.notes is None or not p.rows.sources else torch.from_numpy(p.notes).cuda()
    res = ed.run(dev_notes, p.rows, p.seed, cent, cls)
    files = write_files(p, res) if p.files else []
    os.makedirs(p.out, exist_ok=True)
    rep = build_report(p, res, files, counts)
    with open(os.path.join(p.out, "edit.json"), "w") as f:
        json.dump(rep, f, indent=1, allow_nan=False)
    s = rep["summary"]
    fmt = lambda v: "-" if v is None else format(v, ".4g")  # noqa: E731
    print(f"ae.edit {p.mode}: {s['rows']} rows, latent_step {fmt(s['latent_step'])}, cycle_error {fmt(s['cycle_error'])}"
          + (f", requested {fmt(s['requested'])}, realised {fmt(s['realised'])}" if p.mode == "shift" else ""))
    print(f"wrote {len(files)} files and edit.json to {p.out}")
    return rep


def main(argv=None) -> int:
    return run_tool("ae.edit", AeEditError, plan, run, parse_args(argv), catch_run=True)


if __name__ == "__main__":
    raise SystemExit(main())
