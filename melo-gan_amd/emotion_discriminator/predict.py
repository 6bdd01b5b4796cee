#!/usr/bin/env python3
"""What emotion the trained classifier hears in MIDI files, window by window.

    python -m melo_gan_amd.emotion_discriminator.predict FILE.mid... --config config/ed_config.yaml --model data/models/ed/ed_best.pth
        [--hop <max_notes>] [--min-events 8] [--batch 64] [--drums] [--out predict.json]

Every file is read by midi_in.read_midi, turned into events on the 1/64-beat grid and cut into windows of the config's
max_notes events, --hop events apart (midi_rolls.plan_files).  All files' events go into one device array.  One hipGraph per
run -- mg_roll_encode of the chunk's windows into the engine's input -> forward(train=False) -> mg_scatter_rows_cursor of the
logits to their window positions -- is replayed once per chunk of `batch` windows, the cursor advancing behind each replay;
then one mg_window_votes turns the logits into probabilities, per-window verdicts, per-file means and the number of changes of
verdict, and the run ends with one device -> host read.  The engine is EdEvaluator's, in eval mode.

input_mode: notes with note_dim 4 only: the latent classifier reads the VAE's latents, whose width is not a roll's.

<out> holds per file: notes, events, windows, beats, the loss block (the encode's clamp counts summed over the file's windows,
dropped drum notes, unpaired note-ons, the offset in front of the first note), `faithful` (midi_rolls.faithful), the
prediction, the mean probabilities, the switches, and a timeline of {window, start_beat, prediction, probabilities}.  Stdout
holds one line per file.  Every check runs on the host before any GPU use and raises PredictError; the tool prints
`predict: error: ...` and returns status 2.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from dataclasses import dataclass

import numpy as np

from .. import midi_rolls as MR
from ..midi_in import MidiImportError
from ..pieces import require_device, run_tool

DEFAULT_BATCH = 64
DEFAULT_MIN_EVENTS = 8
MAX_CLASSES = 32


class PredictError(RuntimeError):
    """What every check of this module raises."""


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="The trained emotion classifier's verdict on MIDI files, window by window")
    ap.add_argument("files", nargs="+", metavar="FILE.mid")
    ap.add_argument("--config", type=str, default="config/ed_config.yaml")
    ap.add_argument("--model", type=str, default=None, help="ed_best.pth / ed_epochNNN.pth / a state_dict")
    ap.add_argument("--hop", type=int, default=None, help="events between window starts (default: the config's max_notes)")
    ap.add_argument("--min-events", type=int, default=DEFAULT_MIN_EVENTS)
    ap.add_argument("--batch", type=int, default=DEFAULT_BATCH)
    ap.add_argument("--drums", action="store_true", help="keep the notes of channel 10")
    ap.add_argument("--out", type=str, default="predict.json")
    return ap.parse_args(argv)


@dataclass
class PredictPlan:
    cfg: dict
    model: str
    batch: int
    out: str
    plan: MR.Plan


def check_config(cfg: dict):
    """The classifier must read rolls: input_mode notes, note_dim 4, 2..32 classes."""
    mode = cfg.get("input_mode", "latent")
    if mode != "notes":
        raise PredictError(f"input_mode = {mode}: predict reads note rolls; the latent classifier reads the VAE's latents, whose "
                           "width is not the classifier's note input (encode the rolls with ae.encode and evaluate those)")
    if int(cfg.get("note_dim", 4)) != 4:
        raise PredictError(f"note_dim = {cfg.get('note_dim')}: a roll holds 4 values per note")
    K = int(cfg.get("n_classes", 4))
    if not 2 <= K <= MAX_CLASSES:
        raise PredictError(f"n_classes = {K}: 2..{MAX_CLASSES}")
    T = int(cfg.get("max_notes", 512))
    if not 1 <= T <= (1 << 20):
        raise PredictError(f"max_notes = {T}: 1..2^20")


def plan(args) -> PredictPlan:
    from ..gan.config import load_config
    if not os.path.isfile(args.config):
        raise PredictError(f"config {args.config} does not exist")
    cfg = load_config(args.config)
    check_config(cfg)
    if args.model is None:
        raise PredictError("give --model")
    if not os.path.isfile(args.model):
        raise PredictError(f"checkpoint {args.model} does not exist")
    if not 1 <= int(args.batch) <= 32767:
        raise PredictError(f"--batch = {args.batch}: must be in 1..32767")
    T = int(cfg.get("max_notes", 512))
    try:
        files = [f for f in args.files]
        for f in files:
            if not os.path.isfile(f):
                raise MidiImportError(f"{f}: no such file")
        p = MR.plan_files(files, T, T if args.hop is None else args.hop, args.min_events, args.drums)
    except MidiImportError as e:
        raise PredictError(str(e)) from e
    require_device(PredictError)
    return PredictPlan(cfg, args.model, int(args.batch), args.out, p)


class Predictor:
    """EdEvaluator's eval-mode engine behind mg_roll_encode."""

    def __init__(self, cfg: dict, device="cuda", batch: int = DEFAULT_BATCH):
        import torch
        from ..eval_pass import GraphCache
        from .evaluate import EdEvaluateError, EdEvaluator
        require_device(PredictError)
        check_config(cfg)
        try:
            self.ev = EdEvaluator(cfg, device, batch)
        except EdEvaluateError as e:
            raise PredictError(str(e)) from e
        eng = self.ev.eng
        self.B, self.K, self.T = eng.B, self.ev.K, eng.T
        self.ctr = torch.zeros(1, dtype=torch.int64, device=eng.dev)
        self.base = torch.zeros(1, dtype=torch.int64, device=eng.dev)
        self.graphs = GraphCache()
        self.held = self.res = None
        self.replay_ms = None           # the last run's time per replayed chunk (events around the replays)

    def load(self, path: str):
        from .evaluate import EdEvaluateError
        try:
            self.ev.load(path)
        except EdEvaluateError as e:
            raise PredictError(str(e)) from e

    def _launches(self):
        from .. import ops
        eng, (events, ws, wl, _), d = self.ev.eng, self.held, self.res.dev
        ops.roll_encode(events, ws, wl, eng.x, d["loss"], self.ctr, self.base)
        eng.forward(train=False)
        ops.scatter_rows_cursor(eng.logits, d["logits"], self.ctr, self.base)

    def run(self, p: MR.Plan) -> dict:
        """The plan's windows through the classifier: {"logits" (W, K) fp32, "loss" (W, 8) int64, "probs" (W, K) fp64,
        "win_pred" (W,), "file_mean" (F, K) fp64, "file_pred" (F,), "switches" (F,)} on the host."""
        import torch
        from .. import ops
        from ..eval_pass import Packed
        eng, B, K = self.ev.eng, self.B, self.K
        if not isinstance(p, MR.Plan) or p.T != self.T:
            raise PredictError(f"run: a plan of windows of {self.T} events expected")
        W, F, E = p.win_start.shape[0], len(p.files), p.events.shape[0]
        if W < 1 or ((p.win_start < 0) | (p.win_len < 0) | (p.win_len > self.T) | (p.win_start + p.win_len > E)).any() or \
                p.file_off[0] != 0 or p.file_off[-1] != W or (np.diff(p.file_off) < 0).any():
            raise PredictError("run: a window points outside the event list, or the files' offsets do not cover the windows")
        d = eng.dev
        with torch.cuda.stream(eng.stream):
            self.graphs.clear()             # the captured graph holds the addresses of the arrays below
            self.held = (torch.from_numpy(p.events).to(d), torch.from_numpy(p.win_start).to(d), torch.from_numpy(p.win_len).to(d),
                         torch.from_numpy(p.file_off).to(d))
            self.res = Packed([("loss", (W, ops.ROLL_LOSS_WORDS), torch.int64), ("probs", (W, K), torch.float64),
                               ("file_mean", (F, K), torch.float64), ("logits", (W, K), torch.float32),
                               ("win_pred", (W,), torch.int32), ("file_pred", (F,), torch.int32), ("switches", (F,), torch.int32)], d)
            r = self.res.dev
            self.ctr.zero_()
            self.base.zero_()
            g = self.graphs.graph("chunk", self._launches)
            self.res.buf.zero_()
            self.ctr.zero_()
            nb = (W + B - 1) // B
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(nb):
                g.launch()
                self.ctr.add_(1)
            t1.record()
            ops.window_votes(r["logits"], self.held[3], r["probs"], r["win_pred"], r["file_mean"], r["file_pred"], r["switches"])
            host = self.res.host()          # the run's one device -> host read; synchronises the stream
            self.replay_ms = t0.elapsed_time(t1) / nb
        return {k: v.numpy().copy() for k, v in host.items()}


def report(p: MR.Plan, res: dict, names) -> dict:
    """predict.json from the plan and Predictor.run's arrays."""
    files = []
    for f, info in enumerate(p.files):
        lo, hi = int(p.file_off[f]), int(p.file_off[f + 1])
        loss = res["loss"][lo:hi]
        files.append({"file": info["file"], "notes": info["notes"], "events": info["events"], "windows": hi - lo,
                      "beats": info["beats"], "loss": MR.loss_block(loss, info), "faithful": MR.faithful(loss, info),
                      "prediction": names[int(res["file_pred"][f])],
                      "probabilities": {n: float(v) for n, v in zip(names, res["file_mean"][f])},
                      "switches": int(res["switches"][f]),
                      "timeline": [{"window": w - lo, "start_beat": float(p.start_beat[w]), "prediction": names[int(res["win_pred"][w])],
                                    "probabilities": {n: float(v) for n, v in zip(names, res["probs"][w])}} for w in range(lo, hi)]})
    return {"max_notes": p.T, "classes": list(names), "files": files}


def run(pp: PredictPlan) -> dict:
    from .evaluate import class_names
    pr = Predictor(pp.cfg, "cuda", pp.batch)
    pr.load(pp.model)
    res = pr.run(pp.plan)
    rep = report(pp.plan, res, class_names(pr.K))
    rep["model"] = pp.model
    os.makedirs(os.path.dirname(os.path.abspath(pp.out)), exist_ok=True)
    try:
        with open(pp.out, "w") as f:
            json.dump(rep, f, indent=1, allow_nan=False)
    except ValueError as e:
        raise PredictError(f"the classifier's probabilities are not finite ({e}): is {pp.model} a trained checkpoint?") from e
    for b in rep["files"]:
        print(f"{b['file']}: {b['prediction']} ({b['probabilities'][b['prediction']]:.3f}) over {b['windows']} windows, "
              f"{b['switches']} switches, {b['notes']} notes, {b['beats']:.1f} beats, " +
              ("faithful" if b["faithful"] else "lossy (see loss)"))
    print("report ->", pp.out)
    return rep


def main(argv=None) -> int:
    return run_tool("predict", PredictError, plan, run, parse_args(argv), catch_run=True)


if __name__ == "__main__":
    sys.exit(main())
