#!/usr/bin/env python3
"""What emotion the trained classifier hears in MIDI files, window by window.

    python -m melo_gan_amd.emotion_discriminator.predict FILE.mid... --config config/ed_config.yaml --model data/models/ed/ed_best.pth
        [--hop <max_notes>] [--min-events 8] [--batch 64] [--drums] [--out predict.json]

Every file is read by midi_in.read_midi, turned into events on the 1/64-beat grid and cut into windows of the config's
max_notes events, --hop events apart (midi_rolls.plan_from_args).  All files' events go into one device array
(eval_pass.DeviceWindows).  One hipGraph per run -- mg_roll_encode of the chunk's windows into the engine's input ->
forward(train=False) -> mg_scatter_rows_cursor of the logits to their window positions -- is replayed once per chunk of `batch`
windows, the cursor advancing behind each replay (eval_pass.CursorPass); then one mg_window_votes turns the logits into
probabilities and verdicts per window and per file, and the run ends with one device -> host read.  The engine is EdEvaluator's.

input_mode: notes with note_dim 4 only: the latent classifier reads the VAE's latents, whose width is not a roll's.

<out> holds per file: notes, events, windows, beats, the loss block (the encode's clamp counts summed over the file's windows,
dropped drum notes, unpaired note-ons, the offset in front of the first note), `faithful` (midi_rolls.faithful), the
prediction, the mean probabilities, the switches, and a timeline of {window, start_beat, prediction, probabilities}.  Stdout
holds one line per file.  Every check runs on the host before any GPU use and raises PredictError; the tool prints
`predict: error: ...` and returns status 2.
"""
from __future__ import annotations

import argparse
import os
import sys
from dataclasses import dataclass

from .. import midi_rolls as MR
from ..gan.config import read_config
from ..pieces import require_device, run_tool

DEFAULT_BATCH, MAX_CLASSES, DEFAULT_MIN_EVENTS = 64, 32, MR.DEFAULT_MIN_EVENTS


class PredictError(RuntimeError):
    """What every check of this module raises."""


# ---- what this tool and explain check in front of the device: err is the tool's error class ----
def check_notes_config(cfg: dict, err, reads: str, min_T: int, max_T: int):
    """The classifier must read rolls: input_mode notes (`reads`: what the tool does with them), note_dim 4, 2..32 classes,
    max_notes in min_T..max_T."""
    mode = cfg.get("input_mode", "latent")
    if mode != "notes":
        raise err(f"input_mode = {mode}: {reads}")
    if int(cfg.get("note_dim", 4)) != 4:
        raise err(f"note_dim = {cfg.get('note_dim')}: a roll holds 4 values per note")
    K = int(cfg.get("n_classes", 4))
    if not 2 <= K <= MAX_CLASSES:
        raise err(f"n_classes = {K}: 2..{MAX_CLASSES}")
    T = int(cfg.get("max_notes", 512))
    if not min_T <= T <= max_T:
        raise err(f"max_notes = {T}: {min_T}..{max_T}")


def check_batch(batch, err):
    if not 1 <= int(batch) <= 32767:
        raise err(f"--batch = {batch}: must be in 1..32767")


def load_tool_inputs(args, err, check) -> dict:
    """The config of --config, which must exist and pass check(cfg); --model must be given and exist, --batch be in range."""
    cfg = read_config(args.config, "config", err)
    check(cfg)
    if args.model is None:
        raise err("give --model")
    if not os.path.isfile(args.model):
        raise err(f"checkpoint {args.model} does not exist")
    check_batch(args.batch, err)
    return cfg


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="The trained emotion classifier's verdict on MIDI files, window by window")
    ap.add_argument("files", nargs="+", metavar="FILE.mid")
    ap.add_argument("--config", type=str, default="config/ed_config.yaml")
    ap.add_argument("--model", type=str, default=None, help="ed_best.pth / ed_epochNNN.pth / a state_dict")
    MR.add_window_arguments(ap, max_notes=False)
    ap.add_argument("--batch", type=int, default=DEFAULT_BATCH)
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
    check_notes_config(cfg, PredictError, "predict reads note rolls; the latent classifier reads the VAE's latents, whose width is "
                       "not the classifier's note input (encode the rolls with ae.encode and evaluate those)", 1, 1 << 20)


def plan(args) -> PredictPlan:
    cfg = load_tool_inputs(args, PredictError, check_config)
    p = MR.plan_from_args(args.files, int(cfg.get("max_notes", 512)), args, PredictError)
    require_device(PredictError)
    return PredictPlan(cfg, args.model, int(args.batch), args.out, p)


class Predictor:
    """EdEvaluator's eval-mode engine behind mg_roll_encode."""

    def __init__(self, cfg: dict, device="cuda", batch: int = DEFAULT_BATCH):
        from ..eval_pass import CursorPass
        from .evaluate import EdEvaluateError, EdEvaluator
        require_device(PredictError)
        check_config(cfg)
        try:
            self.ev = EdEvaluator(cfg, device, batch)
        except EdEvaluateError as e:
            raise PredictError(str(e)) from e
        eng = self.ev.eng
        self.B, self.K, self.T = eng.B, self.ev.K, eng.T
        self.cur = CursorPass(eng.dev)
        self.win = self.res = None      # the last run's windows and results: the captured graph holds their addresses
        self.replay_ms = None           # the last run's time per replayed chunk (events around the replays)

    def load(self, path: str):
        from .evaluate import EdEvaluateError
        try:
            self.ev.load(path)
        except EdEvaluateError as e:
            raise PredictError(str(e)) from e

    def _launches(self):
        from .. import ops
        eng, d, cur = self.ev.eng, self.res.dev, self.cur
        self.win.encode(eng.x, d["loss"], cur)
        eng.forward(train=False)
        ops.scatter_rows_cursor(eng.logits, d["logits"], cur.ctr, cur.base)

    def run(self, p: MR.Plan) -> dict:
        """The plan's windows through the classifier: {"logits" (W, K) fp32, "loss" (W, 8) int64, "probs" (W, K) fp64,
        "win_pred" (W,), "file_mean" (F, K) fp64, "file_pred" (F,), "switches" (F,)} on the host."""
        import torch
        from ..eval_pass import DeviceWindows, Packed
        eng = self.ev.eng
        MR.check_plan(p, self.T, PredictError)
        with torch.cuda.stream(eng.stream):
            self.cur.graphs.clear()         # the captured graph holds the addresses of the arrays below
            self.win = DeviceWindows(p, eng.dev)
            self.res = Packed(self.win.vote_parts(self.K), eng.dev)
            nb = (self.win.W + self.B - 1) // self.B
            t0, t1 = self.cur.replay("chunk", self._launches, nb, self.res.buf.zero_)
            self.win.votes(self.res.dev)
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
    MR.write_report(pp.out, rep, PredictError, f"the classifier's probabilities are not finite: is {pp.model} a trained checkpoint?")
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
