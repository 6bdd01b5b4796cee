#!/usr/bin/env python3
"""Blends of and transitions between emotions from a trained generator, and how the generator answers its conditioning:

    python -m melo_gan_amd.gan.morph --config config/gan_config.yaml [--ckpt <CHECKPOINT_DIR>/gan_final.pth] [--ema]
        (--from E --to E | --pairs all | --weights happy=0.7,calm=0.3)
        [--steps 8] [--samples 2] [--noise fixed|slerp] [--seed <SEED>] [--batch 64] [--out <DIR>]
        [--ed_config config/ed_config.yaml --ed_ckpt data/models/ed/ed_best.pth]
        [--join [--join-notes 64]] [--wav [--wav-fs 44100] [--voice piano]] [--no-files]

generate conditions on one of four fixed vectors; the conditioning input is continuous.  A pair mode (--from a --to b, or
--pairs all: the six unordered pairs in class order) walks `samples` paths per pair from a to b in `steps` equal steps: step s
has the weights (1 - w_s) on a and w_s = s / steps on b, and the noise keys (a, k), (b, k) of generate's samples.  --noise fixed
keeps key (a, k)'s noise and jitter at every step (one piece, only the condition moves); --noise slerp interpolates them
spherically, so that step 0 is generate's sample (a, k) and the last step its sample (b, k).  --weights is one blended point:
weights >= 0, normalised to sum 1, drawn under the key of the heaviest emotion (the lower class index on a tie).

One hipGraph -- mg_gen_inputs_mix -> E_num -> G (eval) [-> ED (eval)] -- is replayed per chunk of `batch` rows; the logits, the
classifier's ed_proj features (notes mode) and the rolls of every chunk are copied device to device into resident arrays, and
mg_path_probs / mg_path_d2 run once over them after the last chunk: nothing in the report depends on --batch.

Writes (unless --no-files) morph_<a>_<b>_<k>_s<ss>.mid per step, or blend_<k>.mid, with bpm = round(sum_e w_e bpm_e) and the
scale of the heaviest emotion (pieces.STYLE); with --join also morph_<a>_<b>_<k>.mid, the first --join-notes rows of every
step one after the other (morph_metrics.join_offsets), written at 120 bpm; with --wav the same note lists rendered by
audio.Renderer.  morph.json holds, per pair, the step weights w, p_mean[s][k], the crossover of the mean curves,
monotone_fraction, switch_fraction, and a `feature` and a `roll` block of path_length, endpoint_distance, straightness and ppl
(gan/morph_metrics.py).  Every input from outside is checked on the host before any GPU use; bad input exits with status 2.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import pieces
from ..checkpoints import check_generator_checkpoint, ema_checkpoint, read_checkpoint
from ..pieces import EMOTIONS, STYLE, joined_notes          # joined_notes also for those who read morph.joined_notes
from . import morph_metrics as MM
from .config import read_config
from .eval_engine import EvalEngine
from .generate import DEFAULT_BATCH, EMOTION_TABLE, JITTER, GenerateError, check_ed_config, check_gan_config, plan_config

NOISE_MODES = ("fixed", "slerp")


class MorphError(GenerateError):
    """A bad input of the morpher, found on the host before any GPU use."""


@dataclass
class Rows:
    """The row descriptors of one run, path-major: P paths of S1 consecutive rows; group[p] = the path's pair."""
    weights: np.ndarray         # (P * S1, n_emotions) float32
    key_a: np.ndarray           # (P * S1, 2) int32: (emotion, sample)
    key_b: np.ndarray
    t: np.ndarray               # (P * S1,) float32
    group: np.ndarray           # (P,) int32
    S1: int
    G: int
    paths: List[Tuple[int, int, int]]       # per path: (from, to, k)

    @property
    def P(self) -> int:
        return len(self.paths)


def pair_rows(pairs: Sequence[Tuple[int, int]], steps: int, samples: int, noise: str) -> Rows:
    """Paths (pair, k), k = 1..samples, in pair order: step s has (1 - s / steps) on a and s / steps on b, the keys (a, k) and
    (b, k), and t = 0 (fixed) or s / steps (slerp)."""
    if int(steps) < 1:
        raise MorphError(f"steps = {steps}: must be >= 1")
    if int(samples) < 1:
        raise MorphError(f"samples = {samples}: must be >= 1")
    if noise not in NOISE_MODES:
        raise MorphError(f"noise = {noise!r}: expected one of {', '.join(NOISE_MODES)}")
    for a, b in pairs:
        if not (0 <= a < len(EMOTIONS) and 0 <= b < len(EMOTIONS)) or a == b:
            raise MorphError(f"pair ({a}, {b}): two different emotions in 0..{len(EMOTIONS) - 1} expected")
    S1 = int(steps) + 1
    paths = [(a, b, k) for a, b in pairs for k in range(1, int(samples) + 1)]
    R = len(paths) * S1
    rows = Rows(np.zeros((R, len(EMOTIONS)), np.float32), np.zeros((R, 2), np.int32), np.zeros((R, 2), np.int32),
                np.zeros(R, np.float32), np.repeat(np.arange(len(pairs), dtype=np.int32), int(samples)), S1, len(pairs), paths)
    for p, (a, b, k) in enumerate(paths):
        for s in range(S1):
            r, w = p * S1 + s, s / int(steps)
            rows.weights[r, a], rows.weights[r, b] = 1.0 - w, w
            rows.key_a[r], rows.key_b[r] = (a, k), (b, k)
            rows.t[r] = w if noise == "slerp" else 0.0
    return rows


def blend_rows(weights: Sequence[float], samples: int) -> Rows:
    """One blended point: `samples` single-row paths with the normalised weights under the key (heaviest emotion, k), t = 0."""
    if int(samples) < 1:
        raise MorphError(f"samples = {samples}: must be >= 1")
    w = normalise(weights)
    e = heaviest(w)
    paths = [(e, e, k) for k in range(1, int(samples) + 1)]
    n = len(paths)
    key = np.array([(e, k) for _, _, k in paths], np.int32)
    return Rows(np.tile(np.asarray(w, np.float32), (n, 1)), key, key.copy(), np.zeros(n, np.float32), np.zeros(n, np.int32), 1, 1,
                paths)


def normalise(weights: Sequence[float]) -> List[float]:
    w = [float(v) for v in weights]
    if len(w) != len(EMOTIONS) or not all(math.isfinite(v) and v >= 0.0 for v in w) or sum(w) <= 0.0:
        raise MorphError(f"weights {w}: {len(EMOTIONS)} finite values >= 0 with a positive sum expected")
    total = sum(w)
    return [v / total for v in w]


def heaviest(weights: Sequence[float]) -> int:
    """The emotion with the largest weight, the lower class index on a tie."""
    return max(range(len(weights)), key=lambda e: (weights[e], -e))


def style_of(weights: Sequence[float]) -> Tuple[str, int]:
    """(scale, bpm) of a weight vector: the scale of the heaviest emotion, bpm = round(sum_e w_e bpm_e) (pieces.STYLE)."""
    return STYLE[EMOTIONS[heaviest(weights)]][0], int(round(sum(float(w) * STYLE[e][1] for w, e in zip(weights, EMOTIONS))))


@dataclass
class MorphResult:
    notes: np.ndarray                   # (P * S1, MAX_NOTES, NOTE_DIM)
    stats: MM.PathStats


class Morpher(EvalEngine):
    """One GanEngine of `batch` rows in eval mode behind mg_gen_inputs_mix: E_num -> G, and the frozen emotion classifier when
    ed_cfg is given.  After run() the device arrays self.stash = {logits, feature, rolls} hold every row of the run."""
    error = MorphError

    def __init__(self, cfg: dict, ed_cfg: Optional[dict], device="cuda", batch: int = DEFAULT_BATCH):
        super().__init__(cfg, ed_cfg, device, batch)
        d, E = self.eng.dev, len(EMOTIONS)
        self.weights = torch.zeros(self.B, E, device=d)
        self.key_a = torch.full((self.B, 2), -1, dtype=torch.int32, device=d)
        self.key_b = torch.full((self.B, 2), -1, dtype=torch.int32, device=d)
        self.t = torch.zeros(self.B, device=d)
        self.table = torch.tensor(EMOTION_TABLE, dtype=torch.float32, device=d)
        self.has_feature = self.has_ed and self.eng.ed_mode == "notes"
        self.stash = {}

    def _check_config(self, cfg: dict, ed_cfg: Optional[dict]):
        try:
            check_gan_config(cfg)
        except GenerateError as e:
            raise MorphError(str(e)) from e
        if ed_cfg is not None:
            check_ed_config(ed_cfg, cfg, err=MorphError)

    def _launches(self, seed: int):
        from .. import ops
        eng = self.eng
        ops.gen_inputs_mix(self.weights, self.key_a, self.key_b, self.t, eng.noise, eng.numeric, self.table, JITTER,
                           eng.latent if eng.latent_dim > 0 else None, seed)
        eng._e_fwd(False, "g", gin=True)
        eng._g_fwd(eng.notes, False, "g")
        if self.has_ed:
            eng._ed_fwd(eng.notes)

    def run(self, rows: Rows, seed: int) -> MorphResult:
        from .. import ops
        from ..eval_pass import Packed
        eng, B, P, S1, G = self.eng, self.B, rows.P, rows.S1, rows.G
        R, K = P * S1, eng.n_classes
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        parts = [("roll", (P, S1), torch.float64)]
        if self.has_ed:
            parts += [("probs", (R, K), torch.float64), ("acc", (G, S1, K + 1), torch.float64)]
        if self.has_feature:
            parts.append(("feature", (P, S1), torch.float64))
        with torch.cuda.stream(eng.stream):
            if seed not in self.graphs:         # the seed is a launch argument the capture froze; one graph at a time
                self.graphs.clear()
            g = self.graphs.graph(seed, lambda: self._launches(seed))
            d = eng.dev
            res = Packed(parts, d)
            st = {"rolls": torch.empty(R, eng.T * eng.C, device=d),
                  "logits": torch.empty(R, K, device=d) if self.has_ed else None,
                  "feature": torch.empty(R, eng.ed_proj.shape[1], device=d) if self.has_feature else None}
            for c0 in range(0, R, B):
                n = min(B, R - c0)
                for dev, host, fill in ((self.weights, rows.weights, 0.0), (self.key_a, rows.key_a, -1), (self.key_b, rows.key_b, -1),
                                        (self.t, rows.t, 0.0)):
                    h = torch.full(tuple(dev.shape), fill, dtype=dev.dtype)
                    h[:n] = torch.from_numpy(np.ascontiguousarray(host[c0:c0 + n]))
                    dev.copy_(h)
                g.launch()
                st["rolls"][c0:c0 + n].copy_(eng.notes[:n].reshape(n, -1))
                if self.has_ed:
                    st["logits"][c0:c0 + n].copy_(eng.logits[:n])
                if self.has_feature:
                    st["feature"][c0:c0 + n].copy_(eng.ed_proj[:n])
            ops.path_d2(st["rolls"], P, S1, res.dev["roll"])
            if self.has_ed:
                group = torch.from_numpy(np.ascontiguousarray(rows.group, np.int32)).to(d)
                ops.path_probs(st["logits"], group, S1, G, res.dev["probs"], res.dev["acc"])
            if self.has_feature:
                ops.path_d2(st["feature"], P, S1, res.dev["feature"])
            host = res.host()                   # the report's one device -> host read; synchronises the stream
            notes = st["rolls"].cpu().numpy().reshape(R, eng.T, eng.C)
        self.stash = st
        stats = MM.PathStats(host["probs"].numpy().reshape(P, S1, K) if self.has_ed else None,
                             host["acc"].numpy() if self.has_ed else None,
                             host["feature"].numpy() if self.has_feature else None, host["roll"].numpy())
        return MorphResult(notes, stats)


# ---------------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m melo_gan_amd.gan.morph",
                                 description="Blends of and transitions between emotions from a trained generator.")
    ap.add_argument("--config", type=str, default="config/gan_config.yaml", help="Path to the main GAN config")
    ap.add_argument("--ckpt", type=str, default=None, help="generator checkpoint (default <CHECKPOINT_DIR>/gan_final.pth)")
    ap.add_argument("--ema", action="store_true", help="use the averaged weights in a full checkpoint's 'ema' block")
    ap.add_argument("--from", dest="from_", type=str, default=None, help="the emotion a path starts at")
    ap.add_argument("--to", type=str, default=None, help="the emotion a path ends at")
    ap.add_argument("--pairs", type=str, default=None, help="all: the six unordered pairs in class order")
    ap.add_argument("--weights", type=str, default=None, help="one blended point, e.g. happy=0.7,calm=0.3")
    ap.add_argument("--steps", type=int, default=8, help="steps per path (a path has steps + 1 points)")
    ap.add_argument("--samples", type=int, default=2, help="paths per pair (or samples of a blend)")
    ap.add_argument("--noise", type=str, default="fixed", help="fixed: key (from, k)'s draws at every step; slerp: interpolated")
    ap.add_argument("--seed", type=int, default=None, help="sampling seed (default SEED)")
    ap.add_argument("--batch", type=int, default=DEFAULT_BATCH, help="rows per replayed chunk")
    ap.add_argument("--out", type=str, default=None, help="output directory (default SAMPLE_DIR)")
    ap.add_argument("--ed_config", type=str, default=None, help="ED config of the classifier that scores the paths")
    ap.add_argument("--ed_ckpt", type=str, default=None, help="ED checkpoint (ed_best.pth)")
    ap.add_argument("--join", action="store_true", help="also write each path as one piece, morph_<a>_<b>_<k>.mid")
    ap.add_argument("--join-notes", type=int, default=64, help="rows of each step's roll that go into the joined piece")
    pieces.add_wav_arguments(ap, help_wav="also render every .mid to a .wav")
    ap.add_argument("--no-files", action="store_true", help="write morph.json only")
    return ap.parse_args(argv)


def parse_weights(text: str) -> List[float]:
    """--weights happy=0.7,calm=0.3 -> the normalised weights in class order."""
    w = [0.0] * len(EMOTIONS)
    seen = set()
    for part in str(text).split(","):
        name, eq, val = part.partition("=")
        name = name.strip().lower()
        if not eq or name not in EMOTIONS:
            raise MorphError(f"--weights: {part!r}: expected <emotion>=<weight> with one of {', '.join(EMOTIONS)}")
        if name in seen:
            raise MorphError(f"--weights: {name} is given twice")
        seen.add(name)
        try:
            w[EMOTIONS.index(name)] = float(val)
        except ValueError:
            raise MorphError(f"--weights: {val!r} is not a number") from None
    try:
        return normalise(w)
    except MorphError as e:
        raise MorphError(f"--weights: {e}") from None


def _emotion(name: str, flag: str) -> int:
    e = str(name).lower()
    if e not in EMOTIONS:
        raise MorphError(f"{flag} {name!r}: expected one of {', '.join(EMOTIONS)}")
    return EMOTIONS.index(e)


@dataclass
class Plan:
    cfg: dict
    ed_cfg: Optional[dict]
    ckpt_path: str
    ckpt: dict
    ed_ckpt: Optional[str]
    mode: str                           # "pairs" | "blend"
    pairs: List[Tuple[int, int]]
    blend: Optional[List[float]]
    rows: Rows
    steps: int
    samples: int
    noise: str
    out: str
    seed: int
    batch: int
    ema: bool
    files: bool
    join: Optional[int]                 # --join: the rows per step
    wav: Optional[dict]


def plan(args) -> Plan:
    """Every check of what comes from outside, on the host (no GPU needed); raises MorphError."""
    n_modes = sum((args.from_ is not None or args.to is not None, args.pairs is not None, args.weights is not None))
    if n_modes != 1:
        raise MorphError("exactly one of --from E --to E, --pairs all and --weights is needed")
    blend = None
    if args.weights is not None:
        mode, pairs, blend = "blend", [], parse_weights(args.weights)
    elif args.pairs is not None:
        if str(args.pairs).lower() != "all":
            raise MorphError(f"--pairs {args.pairs!r}: expected all")
        mode, pairs = "pairs", [(a, b) for a in range(len(EMOTIONS)) for b in range(a + 1, len(EMOTIONS))]
    else:
        if args.from_ is None or args.to is None:
            raise MorphError("--from and --to go together")
        a, b = _emotion(args.from_, "--from"), _emotion(args.to, "--to")
        if a == b:
            raise MorphError(f"--from and --to are both {EMOTIONS[a]}: a path needs two emotions")
        mode, pairs = "pairs", [(a, b)]
    if args.batch < 1:
        raise MorphError(f"--batch {args.batch}: must be >= 1")
    if args.steps < 1:
        raise MorphError(f"--steps {args.steps}: must be >= 1")
    if args.samples < 1:
        raise MorphError(f"--samples {args.samples}: must be >= 1")
    if args.noise not in NOISE_MODES:
        raise MorphError(f"--noise {args.noise!r}: expected one of {', '.join(NOISE_MODES)}")
    files = not args.no_files
    wav = pieces.plan_wav(args, MorphError, files, args.join, "morph.json")
    if args.join and mode != "pairs":
        raise MorphError("--join joins the steps of a path: it needs --from / --to or --pairs")
    if args.join and args.join_notes < 1:
        raise MorphError(f"--join-notes {args.join_notes}: must be >= 1")
    rows = blend_rows(blend, args.samples) if mode == "blend" else pair_rows(pairs, args.steps, args.samples, args.noise)
    cfg, ckpt_path = plan_config(args, MorphError)
    check_gan_config(cfg)
    if files and int(cfg["NOTE_DIM"]) != 4:
        raise MorphError(f"NOTE_DIM = {cfg['NOTE_DIM']}: the MIDI writer reads (pitch, velocity, duration, step) rows (--no-files "
                         "reports without writing any)")
    ckpt = read_checkpoint(ckpt_path, MorphError, weights_only=None)         # torch's default: a GAN file holds tensors and numbers
    check_generator_checkpoint(ema_checkpoint(ckpt, ckpt_path, MorphError) if args.ema else ckpt, cfg, ckpt_path, MorphError)
    ed_cfg = None
    if args.ed_config is not None:
        ed_cfg = read_config(args.ed_config, "ED config", MorphError)
        check_ed_config(ed_cfg, cfg, MorphError)
        if not os.path.isfile(args.ed_ckpt):
            raise MorphError(f"ED checkpoint {args.ed_ckpt} does not exist")
    out = args.out or cfg.get("SAMPLE_DIR", "experiments/gan/samples")
    seed = args.seed if args.seed is not None else int(cfg.get("SEED", 42))
    return Plan(cfg, ed_cfg, ckpt_path, ckpt, args.ed_ckpt, mode, pairs, blend, rows, args.steps, args.samples, args.noise, out, seed,
                args.batch, bool(args.ema), files, args.join_notes if args.join else None, wav)


def step_name(a: int, b: int, k: int, s: int) -> str:
    return f"morph_{EMOTIONS[a]}_{EMOTIONS[b]}_{k}_s{s:02d}.mid"


def join_name(a: int, b: int, k: int) -> str:
    return f"morph_{EMOTIONS[a]}_{EMOTIONS[b]}_{k}.mid"


def blend_name(k: int) -> str:
    return f"blend_{k}.mid"


def write_files(p: Plan, res: MorphResult) -> List[dict]:
    """The .mid (and --wav: .wav) files of a run; returns morph.json's files[] entries."""
    rows, S1 = p.rows, p.rows.S1
    todo = []
    for pi, (a, b, k) in enumerate(rows.paths):
        rolls = res.notes[pi * S1:(pi + 1) * S1]
        styles = [style_of(rows.weights[pi * S1 + s]) for s in range(S1)]
        for s, (roll, (scale, bpm)) in enumerate(zip(rolls, styles)):
            f = {"file": blend_name(k) if p.mode == "blend" else step_name(a, b, k, s), "k": k, "bpm": bpm, "scale": scale}
            f.update({"weights": [float(w) for w in rows.weights[pi * S1]]} if p.mode == "blend" else
                     {"from": EMOTIONS[a], "to": EMOTIONS[b], "step": s})
            todo.append((f, (roll, scale, bpm)))
        if p.join is not None:
            f = {"file": join_name(a, b, k), "k": k, "from": EMOTIONS[a], "to": EMOTIONS[b], "joined": True, "join_notes": p.join}
            todo.append((f, joined_notes(rolls, styles, p.join)))
    return pieces.write_pieces(p.out, todo, p.wav)


def report(p: Plan, res: MorphResult, weights: str, files: List[dict]) -> dict:
    """morph.json."""
    rows, S1 = p.rows, p.rows.S1
    out = {"checkpoint": p.ckpt_path, "weights": weights, "ed_checkpoint": p.ed_ckpt, "seed": p.seed, "steps": p.steps if p.mode == "pairs" else 0,
           "samples": p.samples, "noise": p.noise if p.mode == "pairs" else "fixed", "mode": p.mode, "files": files}
    if p.wav is not None:
        out["wav"] = dict(p.wav)
    if p.mode == "blend":
        out["blend"] = {"weights": dict(zip(EMOTIONS, p.blend)), "key_emotion": EMOTIONS[heaviest(p.blend)], **MM.blend_report(res.stats)}
        return out
    w = [s / p.steps for s in range(S1)]
    out["pairs"] = []
    for g, (a, b) in enumerate(p.pairs):
        paths = [pi for pi in range(rows.P) if rows.group[pi] == g]
        out["pairs"].append({"from": EMOTIONS[a], "to": EMOTIONS[b], **MM.pair_report(res.stats, g, paths, w, a, b)})
    return out


def run(p: Plan) -> None:
    pieces.require_device()
    m = Morpher(p.cfg, p.ed_cfg, "cuda", p.batch)
    weights = m.load_generator(p.ckpt, ema=p.ema)
    if p.ed_cfg is not None:
        m.load_ed(p.ed_ckpt)
    res = m.run(p.rows, p.seed)
    files = write_files(p, res) if p.files else []
    os.makedirs(p.out, exist_ok=True)
    rep = report(p, res, weights, files)
    with open(os.path.join(p.out, "morph.json"), "w") as f:
        json.dump(rep, f, indent=1)
    fmt = lambda v, spec: "-" if v is None else format(v, spec)  # noqa: E731
    for blk in rep.get("pairs", []):
        print(f"{blk['from']:>6} -> {blk['to']:<6} crossover {fmt(blk['crossover'], '.3f'):>6}  monotone {fmt(blk['monotone_fraction'], '.2f'):>5}"
              f"  switch {fmt(blk['switch_fraction'], '.2f'):>5}  roll ppl {blk['roll']['ppl']:.4g}")
    print(f"wrote {len(files)} files and morph.json to {p.out}")


def main(argv=None) -> int:
    return pieces.run_tool("morph", GenerateError, plan, run, parse_args(argv))


if __name__ == "__main__":
    sys.exit(main())
