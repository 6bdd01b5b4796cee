#!/usr/bin/env python3
"""Emotion-conditioned sampling from a trained generator -- the generation step that ends the reference pipeline
(full_script.sh:33-36 runs `python -m src.gan.test_gan --emotion <e> --samples 1`, a module the reference tree does not
hold; its only generation code left is the Flask route, app.py:53-65,92-119):

    python -m melo_gan_amd.gan.generate --config config/gan_config.yaml \
        [--ckpt <CHECKPOINT_DIR>/gan_final.pth] [--emotion happy|sad|angry|calm|all] \
        [--samples <N_SAMPLES_PER_EMOTION>] [--out <SAMPLE_DIR>] [--seed <SEED>] [--batch 64] \
        [--ed_config config/ed_config.yaml --ed_ckpt data/models/ed/ed_best.pth] [--ema]
        [--wav [--wav-fs 44100] [--voice piano|organ|sine]]

--ema samples from the averaged generator in the `ema` block of a full gan_epochNNNN.pth (trained with EMA_DECAY > 0;
gan_final_ema.pth is an ordinary checkpoint and needs no flag); summary.json records "weights": "ema" | "raw".
writes <out>/test_<emotion>_<k>.mid for k = 1..N (the reference's file names) with app.py's scale and tempo per emotion,
and <out>/summary.json with the frozen emotion classifier's verdict on every sample when one is given.

--wav also writes test_<emotion>_<k>.wav beside every .mid: the note list that goes into the .mid (midi.notes_from_roll with the
emotion's scale and tempo), rendered on the device by melo_gan_amd.audio.Renderer at --wav-fs Hz with --voice, peak -1 dB full
scale.  Each files[] entry of summary.json then gains "wav", "seconds" and "truncated", and the top level a "wav" block {fs,
voice, peak_db}; without --wav the summary has neither.

The inputs follow app.py: noise ~ N(0,1), numeric = the emotion's base vector + 0.15 * N(0,1), latent = 0.  mg_gen_inputs
draws them on the device from a Philox counter per (emotion, sample), so a sample does not depend on what else is
requested.  One hipGraph -- inputs -> E_num -> G (eval) [-> ED (eval) -> mg_emotion_score] -- is replayed once per chunk of
`batch` rows; the last chunk is padded.  Every input from outside is checked on the host before any GPU use.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import pieces
from ..checkpoints import check_generator_checkpoint, ema_checkpoint, read_checkpoint
from ..pieces import EMOTIONS, STYLE           # also for those who read generate.EMOTIONS and generate.STYLE
from . import config as C
from .eval_engine import EvalEngine

# app.py:53-65 (get_gan_features): the base vector of each emotion and the jitter added to it
EMOTION_TABLE = ((1.0, 1.0, 0.8, 0.8, 0.5, 0.5),
                 (-1.0, -1.0, -0.5, -0.5, -0.5, -0.5),
                 (1.0, -1.0, 1.0, 1.0, -0.8, 0.8),
                 (-1.0, 1.0, -0.8, -0.8, 0.5, -0.5))
JITTER = 0.15
DEFAULT_BATCH = 64


class GenerateError(ValueError):
    """A bad input of the sampler, found on the host before any GPU use."""


def emotion_names(emotion: str) -> List[str]:
    """--emotion: one name or 'all' (the four in class order)."""
    e = str(emotion).lower()
    if e == "all":
        return list(EMOTIONS)
    if e not in EMOTIONS:
        raise GenerateError(f"unknown emotion {emotion!r}: expected one of {', '.join(EMOTIONS)} or all")
    return [e]


def check_gan_config(cfg: dict):
    n = int(cfg.get("NUMERIC_INPUT_DIM", 6))
    if n != len(EMOTION_TABLE[0]):
        raise GenerateError(f"NUMERIC_INPUT_DIM = {n}: the emotion table (app.py:53-65) holds {len(EMOTION_TABLE[0])}-wide "
                            "numeric vectors")


def check_ed_config(ed_cfg: dict, cfg: dict, err=GenerateError, prefix: str = ""):
    """The classifier must score the four emotions and read what this generator produces.  prefix: put in front of the message."""
    n = ed_cfg.get("n_classes", 4)
    if n != len(EMOTIONS):
        raise err(f"{prefix}ED config: n_classes = {n}, the sampler scores the {len(EMOTIONS)} emotions {', '.join(EMOTIONS)}")
    mode = ed_cfg.get("input_mode", "notes")
    if mode == "notes":
        if ed_cfg.get("note_dim", 4) != cfg["NOTE_DIM"]:
            raise err(f"{prefix}ED config: note_dim = {ed_cfg.get('note_dim', 4)} but the GAN config's NOTE_DIM = {cfg['NOTE_DIM']}")
    elif mode == "latent":
        if ed_cfg.get("latent_dim", 128) != cfg["LATENT_DIM"]:
            raise err(f"{prefix}ED config: latent_dim = {ed_cfg.get('latent_dim', 128)} but the GAN config's LATENT_DIM = "
                      f"{cfg['LATENT_DIM']}")
    else:
        raise err(f"{prefix}ED config: input_mode = {mode!r}, expected 'notes' or 'latent'")


@dataclass
class Samples:
    """What Sampler.sample returns, in (emotion, k) order."""
    emotion: List[str]
    k: List[int]
    notes: np.ndarray                   # (M, MAX_NOTES, NOTE_DIM)
    p_target: Optional[np.ndarray]      # (M,) softmax probability of the requested emotion (None without a classifier)
    pred: Optional[np.ndarray]          # (M,) the classifier's predicted class
    summary: Dict[str, dict]            # emotion -> {n, ed_accuracy, ed_mean_p_target}


class Sampler(EvalEngine):
    """One GanEngine of `batch` rows in eval mode: E_num -> G, and the frozen emotion classifier when ed_cfg is given."""
    error = GenerateError

    def __init__(self, cfg: dict, ed_cfg: Optional[dict], device="cuda", batch: int = DEFAULT_BATCH):
        super().__init__(cfg, ed_cfg, device, batch)
        d = self.eng.dev
        self.keys = torch.full((2, self.B), -1, dtype=torch.int32, device=d)      # (emotion, sample) of every row
        self.table = torch.tensor(EMOTION_TABLE, dtype=torch.float32, device=d)
        self.p_target = torch.zeros(self.B, device=d)
        self.pred = torch.zeros(self.B, dtype=torch.int32, device=d)
        self.acc = torch.zeros(len(EMOTIONS), 3, dtype=torch.float64, device=d)

    def _check_config(self, cfg: dict, ed_cfg: Optional[dict]):
        check_gan_config(cfg)
        if ed_cfg is not None:
            check_ed_config(ed_cfg, cfg)

    def _launches(self, seed: int):
        from .. import ops
        eng = self.eng
        ops.gen_inputs(self.keys[0], self.keys[1], eng.noise, eng.numeric, self.table, JITTER,
                       eng.latent if eng.latent_dim > 0 else None, seed)
        eng._e_fwd(False, "g", gin=True)
        eng._g_fwd(eng.notes, False, "g")
        if self.has_ed:
            eng._ed_fwd(eng.notes)
            ops.emotion_score(eng.logits, self.keys[0], self.p_target, self.pred, self.acc)

    def sample(self, emotions: Sequence[str], samples: int, seed: int) -> Samples:
        names = []
        for e in emotions:
            for n in emotion_names(e):
                if n not in names:
                    names.append(n)
        if int(samples) < 1:
            raise GenerateError(f"samples = {samples}: must be >= 1")
        keys = [(EMOTIONS.index(e), k) for e in names for k in range(1, int(samples) + 1)]
        M, B, eng = len(keys), self.B, self.eng
        notes = np.empty((M, eng.T, eng.C), np.float32)
        p = np.empty(M, np.float32) if self.has_ed else None
        pred = np.empty(M, np.int64) if self.has_ed else None
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        with torch.cuda.stream(eng.stream):
            if seed not in self.graphs:         # the seed is a launch argument the capture froze; one graph at a time
                self.graphs.clear()
            g = self.graphs.graph(seed, lambda: self._launches(seed))
            self.acc.zero_()
            for c0 in range(0, M, B):
                chunk = keys[c0:c0 + B]
                n = len(chunk)
                host = torch.full((2, B), -1, dtype=torch.int32)
                host[:, :n] = torch.tensor(chunk, dtype=torch.int32).t()
                host[1, n:] = 0
                self.keys.copy_(host)
                g.launch()
                notes[c0:c0 + n] = eng.notes[:n].cpu().numpy()         # synchronises the stream
                if self.has_ed:
                    p[c0:c0 + n] = self.p_target[:n].cpu().numpy()
                    pred[c0:c0 + n] = self.pred[:n].cpu().numpy()
            acc = self.acc.cpu().numpy()
        summary = {}
        for e in names:
            cnt, hits, sp = acc[EMOTIONS.index(e)]
            summary[e] = {"n": int(samples),
                          "ed_accuracy": float(hits / cnt) if self.has_ed else None,
                          "ed_mean_p_target": float(sp / cnt) if self.has_ed else None}
        return Samples([EMOTIONS[e] for e, _ in keys], [k for _, k in keys], notes, p, pred, summary)


# ---------------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m melo_gan_amd.gan.generate",
                                 description="Emotion-conditioned MIDI samples from a trained generator.")
    ap.add_argument("--config", type=str, default="config/gan_config.yaml", help="Path to the main GAN config")
    ap.add_argument("--ckpt", type=str, default=None, help="generator checkpoint (default <CHECKPOINT_DIR>/gan_final.pth)")
    ap.add_argument("--emotion", type=str, default="all", help="happy, sad, angry, calm or all")
    ap.add_argument("--samples", type=int, default=None, help="samples per emotion (default N_SAMPLES_PER_EMOTION)")
    ap.add_argument("--out", type=str, default=None, help="output directory (default SAMPLE_DIR)")
    ap.add_argument("--seed", type=int, default=None, help="sampling seed (default SEED)")
    ap.add_argument("--batch", type=int, default=DEFAULT_BATCH, help="rows per replayed chunk")
    ap.add_argument("--ed_config", type=str, default=None, help="ED config of the classifier that scores the samples")
    ap.add_argument("--ed_ckpt", type=str, default=None, help="ED checkpoint (ed_best.pth)")
    ap.add_argument("--ema", action="store_true", help="sample from the averaged weights in a full checkpoint's 'ema' block")
    pieces.add_wav_arguments(ap, help_wav="also render every sample to test_<emotion>_<k>.wav")
    return ap.parse_args(argv)


@dataclass
class Plan:
    cfg: dict
    ed_cfg: Optional[dict]
    ckpt_path: str
    ckpt: dict
    ed_ckpt: Optional[str]
    emotions: List[str]
    samples: int
    out: str
    seed: int
    batch: int
    ema: bool = False
    wav: Optional[dict] = None          # --wav: {"fs", "voice", "peak_db"}


def plan_config(args, err=GenerateError):
    """What generate's and evaluate's command lines share: the GAN config with its defaults and the keys every later check
    reads, the pairing of --ed_ckpt with --ed_config, and the checkpoint's path.  Returns (cfg, checkpoint path)."""
    cfg = C.with_gan_defaults(C.read_config(args.config, "config", err), require=False)
    missing = [k for k in ("NOISE_DIM", "LATENT_DIM", "MAX_NOTES", "NOTE_DIM") if k not in cfg]
    if missing:
        raise err(f"config {args.config} lacks {', '.join(missing)}")
    if args.ed_ckpt is not None and args.ed_config is None:
        raise err("--ed_ckpt needs --ed_config (the classifier's architecture)")
    if args.ed_config is not None and args.ed_ckpt is None:
        raise err("--ed_config needs --ed_ckpt (an untrained classifier's verdict means nothing)")
    return cfg, args.ckpt or os.path.join(cfg.get("CHECKPOINT_DIR", "experiments/gan/checkpoints"), "gan_final.pth")


def plan(args) -> Plan:
    """Every check of what comes from outside, on the host (no GPU needed); raises GenerateError."""
    emotions = emotion_names(args.emotion)
    if args.batch < 1:
        raise GenerateError(f"--batch {args.batch}: must be >= 1")
    cfg, ckpt_path = plan_config(args)
    samples = args.samples if args.samples is not None else int(cfg.get("N_SAMPLES_PER_EMOTION", 2))
    if samples < 1:
        raise GenerateError(f"--samples {samples}: must be >= 1")
    check_gan_config(cfg)
    if int(cfg["NOTE_DIM"]) != 4:
        raise GenerateError(f"NOTE_DIM = {cfg['NOTE_DIM']}: the MIDI writer reads (pitch, velocity, duration, step) rows")
    ckpt = read_checkpoint(ckpt_path, GenerateError, weights_only=None)      # torch's default: a GAN file holds tensors and numbers
    ema = bool(getattr(args, "ema", False))
    check_generator_checkpoint(ema_checkpoint(ckpt, ckpt_path, GenerateError) if ema else ckpt, cfg, ckpt_path, GenerateError)
    ed_cfg = None
    if args.ed_config is not None:
        ed_cfg = C.read_config(args.ed_config, "ED config", GenerateError)
        check_ed_config(ed_cfg, cfg)
        if not os.path.isfile(args.ed_ckpt):
            raise GenerateError(f"ED checkpoint {args.ed_ckpt} does not exist")
    out = args.out or cfg.get("SAMPLE_DIR", "experiments/gan/samples")
    seed = args.seed if args.seed is not None else int(cfg.get("SEED", 42))
    wav = pieces.plan_wav(args, GenerateError)
    return Plan(cfg, ed_cfg, ckpt_path, ckpt, args.ed_ckpt, emotions, samples, out, seed, args.batch, ema, wav)


def midi_name(emotion: str, k: int) -> str:
    return f"test_{emotion}_{k}.mid"


def wav_name(emotion: str, k: int) -> str:
    """The .wav beside midi_name(emotion, k): the name pieces.write_pieces derives from the .mid's, x.mid -> x.wav."""
    return f"test_{emotion}_{k}.wav"


def write_outputs(p: Plan, res: Samples) -> dict:
    """Every sample with its emotion's scale and tempo through pieces.write_pieces, then summary.json."""
    todo = []
    for i, (e, k) in enumerate(zip(res.emotion, res.k)):
        f = {"file": midi_name(e, k), "emotion": e, "k": k,
             "ed_pred": None if res.pred is None else EMOTIONS[int(res.pred[i])],
             "ed_p_target": None if res.p_target is None else float(res.p_target[i])}
        todo.append((f, (res.notes[i],) + STYLE[e]))
    files = pieces.write_pieces(p.out, todo, p.wav)
    summary = {"checkpoint": p.ckpt_path, "weights": "ema" if p.ema else "raw", "ed_checkpoint": p.ed_ckpt, "seed": p.seed, "samples": p.samples,
               "batch": p.batch, "emotions": p.emotions, "per_emotion": res.summary, "files": files}
    if p.wav is not None:
        summary["wav"] = dict(p.wav)
    with open(os.path.join(p.out, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
    return summary


def run(p: Plan) -> None:
    pieces.require_device()
    sampler = Sampler(p.cfg, p.ed_cfg, "cuda", p.batch)
    sampler.load_generator(p.ckpt, ema=p.ema)
    if p.ed_cfg is not None:
        sampler.load_ed(p.ed_ckpt)
    res = sampler.sample(p.emotions, p.samples, p.seed)
    write_outputs(p, res)
    fmt = lambda v, spec: "-" if v is None else format(v, spec)  # noqa: E731
    print(f"{'emotion':<8} {'n':>4} {'ed_accuracy':>12} {'ed_mean_p_target':>17}")
    for e, s in res.summary.items():
        print(f"{e:<8} {s['n']:>4} {fmt(s['ed_accuracy'], '.3f'):>12} {fmt(s['ed_mean_p_target'], '.4f'):>17}")
    print(f"wrote {len(res.emotion)} MIDI files{' and WAV files' if p.wav is not None else ''} and summary.json to {p.out}")


def main(argv=None) -> int:
    return pieces.run_tool("generate", GenerateError, plan, run, parse_args(argv))


if __name__ == "__main__":
    sys.exit(main())
