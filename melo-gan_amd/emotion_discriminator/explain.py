#!/usr/bin/env python3
"""Why the trained classifier hears what it hears: integrated gradients per note.

    python -m melo_gan_amd.emotion_discriminator.explain (FILE.mid... | --notes PATH.npy [--rows 0,5,9])
        --config config/ed_config.yaml --model data/models/ed/ed_best.pth [--target predicted|happy|sad|angry|calm]
        [--steps 32] [--top 8] [--deletion 1,2,4,8] [--hop <max_notes>] [--min-events 8] [--batch 64] [--drums]
        [--save attr.npy] [--out explain.json]

The method, per window x (T, 4) of a roll, against the silent roll b (every value -1, mg_roll_encode's padding row):

    k             the window's own prediction, or --target
    F(x)          log softmax(logits(x))[k]
    alpha_s       (s + 1/2) / S, s = 0 .. S-1                                       the midpoint rule, equal weights 1 / S
    attr[t, c]    (x[t,c] - b[t,c]) * (1 / S) * sum_s dF/dx[t,c] (b + alpha_s (x - b))
    note[t]       sum_c attr[t, c];   total = sum_t note[t]
    residual      total - (F(x) - F(b)), which goes to 0 as S grows: every window reports it

A note past the window's length equals b and gets exactly 0.  The notes are ranked by note[t], descending, among the window's
real events, ties to the lower t; padding has rank -1.

The classifier's forward and input gradient are the ones the generator is trained against: GanEngine._ed_fwd / _ed_bwd of an
eval-mode engine (gan.eval_engine.EvalEngine), fp32.  Pass 0 encodes the windows (eval_pass.DeviceWindows) into the resident X
chunk by chunk (mg_roll_encode), runs the forward, scatters the logits and takes the votes (mg_window_votes); one more row gives
F(b).  Pass 1 is one linear hipGraph -- mg_ig_rows -> _ed_fwd -> mg_ig_seed -> _ed_bwd -> mg_ig_accumulate -- replayed once per
G = batch // steps windows, the cursor advancing behind each replay (eval_pass.CursorPass); then one mg_ig_rank.  Pass 2
(--deletion) is a second graph -- mg_ig_rows in deletion mode -> _ed_fwd -> mg_ig_seed -- that removes the n strongest
supporters, and the n strongest opponents, and reads the log-probability again.  The run ends with one device -> host read.

host_ig_rows / host_ig_seed / host_ig_accumulate / host_ig_rank restate the four kernels in numpy; host_explain runs the whole
method over any differentiable forward under torch autograd.

Every check runs on the host before any GPU use and raises ExplainError; the tool prints `explain: error: ...` and returns
status 2.  Non-finite attributions are the same error.
"""
from __future__ import annotations

import argparse
import os
import sys
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from .. import midi_rolls as MR
from ..pieces import require_device, run_tool
from .predict import DEFAULT_BATCH, check_batch, check_notes_config, load_tool_inputs

DEFAULT_STEPS = 32
DEFAULT_TOP = 8
MAX_T = 4096
CHANNELS = ("pitch", "velocity", "duration", "step")
SILENCE = np.float32(-1.0)
PATH, DELETE = 0, 1


class ExplainError(RuntimeError):
    """What every check of this module raises."""


# ---------------------------------------------------------------------------------------------------------------------
# the four kernels on the host (numpy)
# ---------------------------------------------------------------------------------------------------------------------
def host_window_of(r: int, B: int, R: int, W: int, cursor: int) -> int:
    """The window of batch row r (include/melo_gan_hip.h), -1 for none."""
    G = B // R
    if r >= G * R:
        return -1
    w = cursor * G + r // R
    return w if 0 <= w < W else -1


def host_ig_rows(X, B: int, R: int, cursor: int = 0, mode: int = PATH, win_len=None, rank=None, n_del=None):
    """mg_ig_rows: one batch (B, T, 4) fp32 of path rows (R steps per window) or deletion rows (R = 2 len(n_del))."""
    X = np.asarray(X, np.float32)
    W, T, _ = X.shape
    out = np.full((B, T, 4), SILENCE, np.float32)
    for r in range(B):
        w = host_window_of(r, B, R, W, cursor)
        if w < 0:
            continue
        j = r % R
        if mode == PATH:
            alpha = (float(j) + 0.5) / float(R)
            out[r] = (-1.0 + alpha * (X[w].astype(np.float64) - (-1.0))).astype(np.float32)
            continue
        D, n_len = len(n_del), int(win_len[w])
        q, t = np.asarray(rank[w]), np.arange(T)
        n = int(n_del[j if j < D else j - D])
        gone = (q >= 0) & (t < n_len) & ((q < n) if j < D else (q >= n_len - n))
        out[r] = X[w]
        out[r][gone] = SILENCE
    return out


def host_softmax(z):
    """softmax64.h over one row of fp32 logits: (p fp64 (K,), max index, 1 + the other terms in class order)."""
    z = np.asarray(z, np.float32).astype(np.float64)
    pred = int(np.argmax(z))
    e = np.exp(z - z[pred])
    rest = 0.0
    for k in range(z.shape[0]):
        if k != pred:
            rest += e[k]
    s = 1.0 + rest
    p = e / s
    p[pred] = 1.0 / s
    return p, pred, s


def host_log_softmax(z, k: int) -> float:
    """mg_ig_seed's logp: (z[k] - max) - log(1 + the other terms)."""
    _, pred, s = host_softmax(z)
    z = np.asarray(z, np.float32).astype(np.float64)
    return float((z[k] - z[pred]) - np.log(s))


def host_ig_seed(logits, target, R: int, cursor: int = 0):
    """mg_ig_seed: (dlogits (B, K) fp32, logp (B,) fp64)."""
    z = np.asarray(logits, np.float32)
    B, K = z.shape
    W = len(target)
    dl, lp = np.zeros((B, K), np.float32), np.zeros(B, np.float64)
    for r in range(B):
        w = host_window_of(r, B, R, W, cursor)
        if w < 0:
            continue
        k = int(target[w])
        if not 0 <= k < K:
            dl[r], lp[r] = np.nan, np.nan
            continue
        p, _, _ = host_softmax(z[r])
        onehot = np.zeros(K)
        onehot[k] = 1.0
        dl[r] = (onehot - p).astype(np.float32)
        lp[r] = host_log_softmax(z[r], k)
    return dl, lp


def host_ig_accumulate(dnotes, X, R: int, cursor: int, attr, note, sums):
    """mg_ig_accumulate: writes the batch's windows into attr (W, T, 4), note (W, T) and sums (W, 5), all fp64, in place.  The
    device adds sums' terms in another fixed order: they agree to the rounding of fp64 sums, the rest bit for bit."""
    d, X = np.asarray(dnotes, np.float32), np.asarray(X, np.float32)
    B, W = d.shape[0], X.shape[0]
    for g in range(B // R):
        w = host_window_of(g * R, B, R, W, cursor)
        if w < 0:
            continue
        s = np.zeros(d.shape[1:], np.float64)
        for i in range(R):
            s = s + d[g * R + i].astype(np.float64)
        dx = X[w].astype(np.float64) - (-1.0)
        with np.errstate(all="ignore"):
            a = np.where(dx == 0.0, 0.0, dx * (s / float(R)))
        attr[w] = a
        note[w] = ((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]
        sums[w, 0] = note[w].sum()
        sums[w, 1:] = a.sum(axis=0)
    return attr, note, sums


def host_ig_rank(note, win_len):
    """mg_ig_rank: rank (W, T) int32, descending by note among t < win_len, ties to the lower t; -1 for padding, and for the
    whole window where a real event's note is NaN or the length lies outside [0, T]."""
    v = np.asarray(note, np.float64)
    W, T = v.shape
    rank = np.full((W, T), -1, np.int32)
    for w in range(W):
        n = int(win_len[w])
        if not 0 <= n <= T or np.isnan(v[w, :n]).any():
            continue
        order = np.argsort(-v[w, :n], kind="stable")         # descending; equal values keep their order: the lower t first
        rank[w, order] = np.arange(n, dtype=np.int32)
    return rank


# ---------------------------------------------------------------------------------------------------------------------
# the whole method over any differentiable forward
# ---------------------------------------------------------------------------------------------------------------------
def host_explain(forward_fn, X, win_len, steps: int, target=None, deletion: Sequence[int] = (), dtype=None) -> dict:
    """Integrated gradients of forward_fn (a (n, T, 4) tensor -> (n, K) logits, differentiable by torch autograd) for the
    windows X (W, T, 4) fp32.  target: None (each window's own arg-max) or one class for all.  dtype: what the rows are cast
    to in front of forward_fn (default float64).  Returns Explainer.run's arrays, computed window by window: logits,
    target, log_p, log_p_silence, attr, note, sums, total, residual, rank, and with deletion del_log_p (W, 2 D)."""
    import torch
    dtype = torch.float64 if dtype is None else dtype
    X = np.ascontiguousarray(X, np.float32)
    W, T, _ = X.shape
    S, D = int(steps), len(deletion)
    win_len = np.asarray(win_len, np.int32)

    def logp_of(rows, k, grad=False):
        x = torch.from_numpy(np.ascontiguousarray(rows)).to(dtype).requires_grad_(grad)
        lp = torch.log_softmax(forward_fn(x).double(), dim=1)[:, k]
        if not grad:
            return lp.detach().numpy(), None
        g, = torch.autograd.grad(lp.sum(), x)
        return lp.detach().numpy(), g.double().numpy()

    with torch.no_grad():
        logits = forward_fn(torch.from_numpy(X).to(dtype)).double().numpy()
        silence = np.full((1, T, 4), SILENCE, np.float32)
    tgt = np.array([int(np.argmax(z)) for z in logits], np.int32) if target is None else np.full(W, int(target), np.int32)
    out = {"logits": logits, "target": tgt, "attr": np.zeros((W, T, 4)), "note": np.zeros((W, T)), "sums": np.zeros((W, 5)),
           "log_p": np.zeros(W), "log_p_silence": np.zeros(W)}
    for w in range(W):
        k = int(tgt[w])
        with torch.no_grad():
            out["log_p"][w] = logp_of(X[w:w + 1], k)[0][0]
            out["log_p_silence"][w] = logp_of(silence, k)[0][0]
        rows = host_ig_rows(X[w:w + 1], S, S)
        _, g = logp_of(rows, k, grad=True)
        dx = X[w].astype(np.float64) - (-1.0)
        a = np.where(dx == 0.0, 0.0, dx * (g.sum(axis=0) / float(S)))
        out["attr"][w], out["note"][w] = a, a.sum(axis=1)
        out["sums"][w, 0], out["sums"][w, 1:] = a.sum(), a.sum(axis=0)
    out["total"] = out["sums"][:, 0].copy()
    out["residual"] = out["total"] - (out["log_p"] - out["log_p_silence"])
    out["rank"] = host_ig_rank(out["note"], win_len)
    if D:
        n_del = np.asarray(deletion, np.int32)
        out["del_log_p"] = np.zeros((W, 2 * D))
        for w in range(W):
            rows = host_ig_rows(X[w:w + 1], 2 * D, 2 * D, 0, DELETE, win_len[w:w + 1], out["rank"][w:w + 1], n_del)
            with torch.no_grad():
                out["del_log_p"][w] = logp_of(rows, int(tgt[w]))[0]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the plan (host only)
# ---------------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Which notes made the emotion classifier's verdict: integrated gradients per note")
    ap.add_argument("files", nargs="*", metavar="FILE.mid")
    ap.add_argument("--notes", type=str, default=None, help="a (n, max_notes, 4) float32 .npy of rolls instead of MIDI files")
    ap.add_argument("--rows", type=str, default=None, help="with --notes: the rows to explain, e.g. 0,5,9 (default: all)")
    ap.add_argument("--config", type=str, default="config/ed_config.yaml")
    ap.add_argument("--model", type=str, default=None, help="ed_best.pth / ed_epochNNN.pth / a state_dict")
    ap.add_argument("--target", type=str, default="predicted", help="predicted, or one class for every window")
    ap.add_argument("--steps", type=int, default=DEFAULT_STEPS, help="points of the midpoint rule along the path")
    ap.add_argument("--top", type=int, default=DEFAULT_TOP, help="notes listed at either end of the ranking")
    ap.add_argument("--deletion", type=str, default=None, help="counts of notes to remove, e.g. 1,2,4,8")
    MR.add_window_arguments(ap, max_notes=False)
    ap.add_argument("--batch", type=int, default=DEFAULT_BATCH)
    ap.add_argument("--save", type=str, default=None, help="write attr (W, T, 4) float64 to this .npy")
    ap.add_argument("--out", type=str, default="explain.json")
    return ap.parse_args(argv)


@dataclass
class ExplainPlan:
    cfg: dict
    model: str
    batch: int
    steps: int
    top: int
    target: Optional[int]       # None: each window's own prediction
    deletion: tuple
    out: str
    save: Optional[str]
    source: object              # MR.Plan, or the rolls (W, T, 4) float32
    plan: MR.Plan               # the files and windows the report speaks of (a --notes array is one file)


def check_config(cfg: dict):
    """predict's requirements -- input_mode notes, note_dim 4, 2..32 classes -- and the kernels' T <= 4096."""
    check_notes_config(cfg, ExplainError, "explain attributes the verdict to the notes of a roll; the latent classifier never sees "
                       "them", 8, MAX_T)


def check_sizes(batch, steps):
    check_batch(batch, ExplainError)
    if not 1 <= int(steps) <= int(batch):
        raise ExplainError(f"--steps = {steps}: must be in 1..--batch = {batch} (a window's path is one part of a batch)")


def int_list(text: str, what: str):
    try:
        return [int(v) for v in str(text).split(",") if v.strip() != ""]
    except ValueError:
        raise ExplainError(f"{what} {text!r}: a comma-separated list of integers expected") from None


def rolls_plan(path: str, x, rows) -> MR.Plan:
    """A --notes array as one file of full windows, for report()."""
    W, T = x.shape[0], x.shape[1]
    info = {"file": path, "notes": int((x[:, :, 1] >= np.float32(-0.2)).sum()), "events": W * T, "rests": 0, "beats": 0.0, "lead_q": 0,
            "dropped_drums": 0, "unpaired": 0, "dropped_events": 0, "tempo_us": 500000, "division": 0, "rows": [int(r) for r in rows]}
    return MR.Plan(np.zeros((0, 4), np.int32), np.arange(W, dtype=np.int64) * T, np.full(W, T, np.int32),
                   np.arange(W, dtype=np.int64) * T, np.zeros(W), np.array([0, W], np.int64), [info], T)


def plan(args) -> ExplainPlan:
    from .evaluate import class_names
    cfg = load_tool_inputs(args, ExplainError, check_config)
    T, K = int(cfg.get("max_notes", 512)), int(cfg.get("n_classes", 4))
    check_sizes(args.batch, args.steps)
    if int(args.top) < 1:
        raise ExplainError(f"--top = {args.top}: must be >= 1")
    names = class_names(K)
    if args.target == "predicted":
        target = None
    elif args.target in names:
        target = names.index(args.target)
    else:
        raise ExplainError(f"--target {args.target}: predicted, or one of {', '.join(names)}")
    deletion = ()
    if args.deletion is not None:
        deletion = tuple(int_list(args.deletion, "--deletion"))
        if not deletion or min(deletion) < 0 or max(deletion) > T or 2 * len(deletion) > int(args.batch):
            raise ExplainError(f"--deletion {args.deletion}: counts in 0..{T}, at most --batch / 2 = {int(args.batch) // 2} of them")
    if bool(args.files) == (args.notes is not None):
        raise ExplainError("give either MIDI files or --notes PATH.npy" + (", not both" if args.files else ""))
    if args.rows is not None and args.notes is None:
        raise ExplainError("--rows selects rows of --notes")
    if args.notes is not None:
        if not os.path.isfile(args.notes):
            raise ExplainError(f"{args.notes}: no such file")
        try:
            x = np.load(args.notes, mmap_mode="r", allow_pickle=False)
        except (ValueError, OSError) as e:
            raise ExplainError(f"{args.notes}: not a .npy array ({e})") from e
        if not isinstance(x, np.ndarray):
            raise ExplainError(f"{args.notes}: not a .npy array")
        if x.dtype != np.float32 or x.ndim != 3 or tuple(x.shape[1:]) != (T, 4) or x.shape[0] < 1:
            raise ExplainError(f"{args.notes}: float32 (n >= 1, {T}, 4) expected, got {x.dtype} {tuple(x.shape)}")
        rows = list(range(x.shape[0])) if args.rows is None else int_list(args.rows, "--rows")
        if not rows or min(rows) < 0 or max(rows) >= x.shape[0]:
            raise ExplainError(f"--rows {args.rows}: rows in 0..{x.shape[0] - 1} of {args.notes}")
        x = np.ascontiguousarray(x[rows], np.float32)
        if not np.isfinite(x).all():
            raise ExplainError(f"{args.notes}: a selected row holds a value that is not finite")
        source, p = x, rolls_plan(args.notes, x, rows)
    else:
        source = p = MR.plan_from_args(args.files, T, args, ExplainError)
    require_device(ExplainError)
    return ExplainPlan(cfg, args.model, int(args.batch), int(args.steps), int(args.top), target, deletion, args.out, args.save,
                       source, p)


# ---------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------
def gan_config(ed_cfg: dict) -> dict:
    """The GAN config of the engine that holds the classifier: the roll's shape from the ED config, defaults elsewhere (the
    keys without a default, which size the generator that is never run here, as config.default_gan_cfg sets them)."""
    from ..gan.config import default_gan_cfg, with_gan_defaults
    T = int(ed_cfg.get("max_notes", 512))
    sizes = {k: v for k, v in default_gan_cfg(1, T, 4).items() if k in ("NOISE_DIM", "LATENT_DIM")}
    return with_gan_defaults({**sizes, "MAX_NOTES": T, "NOTE_DIM": 4}, require=False)


def _engine_class():
    from ..gan.eval_engine import EvalEngine

    class _Engine(EvalEngine):
        error = ExplainError

        def _check_config(self, cfg, ed_cfg):
            check_config(ed_cfg)

    return _Engine


class Explainer:
    """An eval-mode GanEngine's frozen classifier (gan.eval_engine.EvalEngine) behind the four mg_ig_* kernels."""

    def __init__(self, ed_cfg: dict, device="cuda", batch: int = DEFAULT_BATCH, steps: int = DEFAULT_STEPS):
        import torch
        from ..eval_pass import CursorPass
        require_device(ExplainError)
        check_config(ed_cfg)
        check_sizes(batch, steps)
        try:
            self.ee = _engine_class()(gan_config(ed_cfg), dict(ed_cfg), device, int(batch))
        except (ValueError, KeyError) as e:
            raise ExplainError(str(e)) from e
        eng = self.eng = self.ee.eng
        if eng.ed_dtype != "fp32" or eng.ed_mode != "notes":
            raise ExplainError("explain: the fp32 notes-mode classifier only")
        self.B, self.S, self.T, self.K = eng.B, int(steps), eng.T, int(eng.n_classes)
        self.G = self.B // self.S
        self.cur = CursorPass(eng.dev, self.ee.graphs)
        self.logp_rows = torch.zeros(self.B, dtype=torch.float64, device=eng.dev)
        self.X = self.win = self.res = self.n_del = None    # the last run's arrays: the captured graphs hold their addresses
        self.replay_ms = None           # the last run's time per replay of the pass-1 graph (events around the replays)

    def load(self, path: str):
        try:
            self.ee.load_ed(path)
        except RuntimeError as e:           # ExplainError included: a checkpoint of another classifier
            raise ExplainError(str(e)) from e

    # ---- what the two graphs hold ----
    def _path_launches(self):
        from .. import ops
        eng, r, ctr, base = self.eng, self.res.dev, self.cur.ctr, self.cur.base
        ops.ig_rows(self.X, eng.notes, self.S, ctr, base)
        eng._ed_fwd(eng.notes)
        ops.ig_seed(eng.logits, r["target"], self.S, eng.dlogits, self.logp_rows, ctr, base)
        eng._ed_bwd(eng.dnotes)
        ops.ig_accumulate(eng.dnotes, self.X, self.S, r["attr"], r["note"], r["sums"], ctr, base)

    def _deletion_launches(self):
        from .. import ops
        import torch
        eng, r, R, ctr, base = self.eng, self.res.dev, 2 * self.n_del.numel(), self.cur.ctr, self.cur.base
        G = self.B // R
        ops.ig_rows(self.X, eng.notes, R, ctr, base, ops.IG_DELETE, self.win.win_len, r["rank"], self.n_del)
        eng._ed_fwd(eng.notes)
        ops.ig_seed(eng.logits, r["target"], R, eng.dlogits, self.logp_rows, ctr, base)
        # the batch's G windows of R fp64 words each, as rows of fp32 pairs, to their window positions
        ops.scatter_rows_cursor(self.logp_rows.view(torch.float32)[:2 * G * R].view(G, 2 * R),
                                r["del_log_p"].view(torch.float32).view(-1, 2 * R), ctr, base)

    def run(self, source, target: Optional[int] = None, deletion: Sequence[int] = ()) -> dict:
        """source: an MR.Plan of windows of T events, or rolls (W, T, 4) float32 (every window of full length).  target: None
        (each window's own prediction) or one class.  deletion: counts of notes to remove.  Returns, on the host: attr (W, T,
        4), note (W, T), sums (W, 5), total, residual, log_p, log_p_silence (W,), probs (W, K), file_mean (F, K) fp64; logits
        (W, K) fp32; rank (W, T), win_pred, target (W,), file_pred, switches (F,) int32; loss (W, 8) int64; with deletion,
        del_log_p (W, 2 D) fp64: the D supporter removals, then the D opponent removals."""
        import torch
        from .. import ops
        from ..eval_pass import DeviceWindows, Packed
        eng, B, K, T, S, G, cur = self.eng, self.B, self.K, self.T, self.S, self.G, self.cur
        d = eng.dev
        is_plan = isinstance(source, MR.Plan)
        if is_plan:
            MR.check_plan(source, T, ExplainError)
            W = source.win_start.shape[0]
        else:
            x = np.asarray(source)
            if x.dtype != np.float32 or x.ndim != 3 or tuple(x.shape[1:]) != (T, 4) or x.shape[0] < 1 or not np.isfinite(x).all():
                raise ExplainError(f"run: finite float32 rolls (W >= 1, {T}, 4) expected")
            W = x.shape[0]
        if target is not None and not 0 <= int(target) < K:
            raise ExplainError(f"run: target = {target}: None or a class in 0..{K - 1}")
        deletion = tuple(int(n) for n in deletion)
        D = len(deletion)
        if D and (min(deletion) < 0 or max(deletion) > T or 2 * D > B):
            raise ExplainError(f"run: deletion counts {deletion}: in 0..{T}, at most {B // 2} of them")
        nb0 = (W + B - 1) // B
        with torch.cuda.stream(eng.stream):
            cur.graphs.clear()              # the captured graphs hold the addresses of the arrays below
            self.win = win = DeviceWindows(source if is_plan else (np.full(W, T, np.int32), np.array([0, W], np.int64), T), d)
            parts = [("attr", (W, T, 4), torch.float64), ("note", (W, T), torch.float64), ("sums", (W, ops.IG_SUMS), torch.float64),
                     ("log_p", (W,), torch.float64), ("log_p_silence", (W,), torch.float64),
                     ("del_log_p", (W, max(1, 2 * D)), torch.float64)] + win.vote_parts(K) + \
                    [("silence", (W, K), torch.float32), ("seed", (W, K), torch.float32), ("rank", (W, T), torch.int32),
                     ("target", (W,), torch.int32)]
            self.res = Packed(parts, d)
            r = self.res.dev
            self.n_del = torch.tensor(deletion, dtype=torch.int32, device=d) if D else None
            # ---- pass 0: the resident windows, their logits and votes, and the silent roll's logits ----
            Xp = torch.full((nb0 * B, T, 4), -1.0, device=d)        # whole chunks; the rows past W stay silent
            self.X = Xp[:W]
            if not is_plan:
                self.X.copy_(torch.from_numpy(x))
            for c in cur.each(nb0):         # eager: every chunk has its own rows of X
                rows = Xp[c * B:(c + 1) * B]
                if is_plan:
                    win.encode(rows, r["loss"], cur)
                eng._ed_fwd(rows)
                ops.scatter_rows_cursor(eng.logits, r["logits"], cur.ctr, cur.base)
            win.votes(r)
            if target is None:
                r["target"].copy_(r["win_pred"])
            else:
                r["target"].fill_(int(target))
            eng.notes.fill_(-1.0)           # one extra row gives F(b): every row of this batch is the silent roll
            eng._ed_fwd(eng.notes)
            r["silence"].copy_(eng.logits[:1].expand(W, K))
            cur.ctr.zero_()
            for z, lp in ((r["logits"], r["log_p"]), (r["silence"], r["log_p_silence"])):      # F(x) and F(b) at the targets
                ops.ig_seed(z, r["target"], 1, r["seed"], lp, cur.ctr, cur.base)
            # ---- pass 1: the path ----
            nb = (W + G - 1) // G
            t0, t1 = cur.replay("path", self._path_launches, nb)
            ops.ig_rank(r["note"], win.win_len, r["rank"])
            # ---- pass 2: the deletion test ----
            if D:
                G2 = B // (2 * D)
                cur.replay("deletion", self._deletion_launches, (W + G2 - 1) // G2)
            host = self.res.host()          # the run's one device -> host read; synchronises the stream
            self.replay_ms = t0.elapsed_time(t1) / nb
        out = {k: v.numpy().copy() for k, v in host.items() if k not in ("silence", "seed")}
        if not D:
            del out["del_log_p"]
        out["total"] = out["sums"][:, 0].copy()
        out["residual"] = out["total"] - (out["log_p"] - out["log_p_silence"])
        return out


# ---------------------------------------------------------------------------------------------------------------------
# the report
# ---------------------------------------------------------------------------------------------------------------------
def check_finite(res: dict, model: str):
    for k in ("attr", "log_p", "log_p_silence") + (("del_log_p",) if "del_log_p" in res else ()):
        if not np.isfinite(res[k]).all():
            raise ExplainError(f"{k} is not finite: is {model} a trained checkpoint?")


def decode_windows(X) -> dict:
    """The output contract's reading of the windows (gan.music_metrics.decode_rolls) and each event's onset in beats from the
    window's start."""
    from ..gan.music_metrics import decode_rolls
    dec = decode_rolls(np.ascontiguousarray(X, np.float32))
    step = np.where(dec["valid"], dec["step"], 0.0)
    dec["onset"] = np.cumsum(step, axis=-1) - step
    return dec


def report(p: MR.Plan, X, res: dict, names, top: int = DEFAULT_TOP, deletion: Sequence[int] = ()) -> dict:
    """explain.json's `files` from the plan, the windows' rolls X (W, T, 4) and Explainer.run's (or host_explain's) arrays."""
    dec = decode_windows(X)
    files = []
    for f, info in enumerate(p.files):
        lo, hi = int(p.file_off[f]), int(p.file_off[f + 1])
        windows = []
        for w in range(lo, hi):
            n, rank, note = int(p.win_len[w]), res["rank"][w], res["note"][w]
            order = np.full(n, -1, np.int64)
            real = np.nonzero(rank[:n] >= 0)[0]
            order[rank[real]] = real                    # order[q] = the event of rank q

            def entry(t):
                snd = bool(dec["sounding"][w, t])
                return {"event": int(t), "beat": float(p.start_beat[w] + dec["onset"][w, t]),
                        "pitch": int(dec["pitch"][w, t]) if snd else None, "velocity": int(dec["vel"][w, t]) if snd else None,
                        "attribution": float(note[t])}

            ranked = [int(t) for t in order if t >= 0]
            ch = res["sums"][w, 1:]
            blk = {"window": w - lo, "start_beat": float(p.start_beat[w]), "events": n, "target": names[int(res["target"][w])],
                   "prediction": names[int(res["win_pred"][w])] if "win_pred" in res else names[int(np.argmax(res["logits"][w]))],
                   "log_p": float(res["log_p"][w]), "log_p_silence": float(res["log_p_silence"][w]),
                   "total": float(res["total"][w]), "residual": float(res["residual"][w]),
                   "channels": {c: float(v) for c, v in zip(CHANNELS, ch)},
                   "supports": [entry(t) for t in ranked[:top]], "opposes": [entry(t) for t in ranked[::-1][:top]]}
            if len(deletion):
                D, dl = len(deletion), res["del_log_p"][w]
                blk["deletion"] = []
                for j, k in enumerate(deletion):
                    k = min(int(k), len(ranked))
                    blk["deletion"].append({"n": int(deletion[j]),
                                            "removed_support": {"log_p": float(dl[j]),
                                                                "predicted": float(res["log_p"][w] - note[ranked[:k]].sum())},
                                            "removed_oppose": {"log_p": float(dl[D + j]),
                                                               "predicted": float(res["log_p"][w] - note[ranked[len(ranked) - k:]].sum())}})
            windows.append(blk)
        ch = np.abs(res["sums"][lo:hi, 1:])
        tot = ch.sum(axis=1, keepdims=True)
        share = np.where(tot > 0, ch / np.where(tot > 0, tot, 1.0), 0.0).mean(axis=0) if hi > lo else np.zeros(4)
        files.append({"file": info["file"], "notes": info["notes"], "events": info["events"], "windows": hi - lo,
                      "channel_shares": {c: float(v) for c, v in zip(CHANNELS, share)},
                      "mean_abs_residual": float(np.abs(res["residual"][lo:hi]).mean()) if hi > lo else 0.0,
                      "timeline": windows})
        if "rows" in info:
            files[-1]["rows"] = info["rows"]
    return {"max_notes": p.T, "files": files}


def run(ep: ExplainPlan) -> dict:
    from .evaluate import class_names
    ex = Explainer(ep.cfg, "cuda", ep.batch, ep.steps)
    ex.load(ep.model)
    res = ex.run(ep.source, ep.target, ep.deletion)
    check_finite(res, ep.model)
    names = class_names(ex.K)
    X = ex.X.cpu().numpy()
    rep = report(ep.plan, X, res, names, ep.top, ep.deletion)
    rep.update(steps=ep.steps, classes=list(names), model=ep.model, replay_ms=ex.replay_ms)
    MR.write_report(ep.out, rep, ExplainError, f"the report holds a value that is not finite: is {ep.model} a trained checkpoint?")
    if ep.save:
        os.makedirs(os.path.dirname(os.path.abspath(ep.save)), exist_ok=True)
        np.save(ep.save, res["attr"])
    for b in rep["files"]:
        sh = b["channel_shares"]
        print(f"{b['file']}: {b['windows']} windows, " + ", ".join(f"{c} {sh[c]:.2f}" for c in CHANNELS) +
              f", mean |residual| {b['mean_abs_residual']:.2e} at {ep.steps} steps")
    print("report ->", ep.out)
    return rep


def main(argv=None) -> int:
    return run_tool("explain", ExplainError, plan, run, parse_args(argv), catch_run=True)


if __name__ == "__main__":
    sys.exit(main())
