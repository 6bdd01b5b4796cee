#!/usr/bin/env python3
"""Shared motifs between pieces, whatever key they are played in: the note-level copy check.

    python -m melo_gan_amd.motifs QUERY... --corpus CORPUS... [--baseline HELDOUT...] [--self]
        [--tokens interval+rhythm|interval] [--min-len 8] [--top 3] [--max-notes 512] [--hop <max-notes>]
        [--min-events 8] [--drums] [--batch 64] [--cpu] [--out motifs.json]

Every roll row becomes a row of tokens, one per pair of neighbouring sounding notes: the pitch interval and, in the default
mode, one of six classes of the time between the two onsets (include/melo_gan_hip.h, mg_motif_tokens).  A phrase keeps its
tokens when it is transposed or moved inside a row.  For every query row the tool finds, against every corpus row, the
longest run of equal tokens (mg_motif_lcs), keeps the --top corpus rows (mg_motif_rank), and computes `copied_share`: the
share of the row's tokens that lie inside a run of at least --min-len tokens shared with any corpus row.

QUERY, CORPUS and HELDOUT are .mid / .midi files, directories that hold a notes.npy (a split directory, as midi_import writes
it), other directories (searched for MIDI files) or a .npy of rolls (N, T, 4) float32.  MIDI is cut into windows and encoded
exactly as midi_import does it (midi_rolls.plan_files, then mg_roll_encode or midi_rolls.host_roll_encode: the same bits), so
the files generate and morph write are valid queries.  Rows shorter than the longest T among the inputs are filled up with
the padding row, a rest, which adds no token.

--self matches the corpus against itself, the de-duplication and leakage check of a data set: the group of a row is its MIDI
file, the `file` of its index.json entry in a split directory, or else the row itself, and a pair of rows of one group is
skipped.  `pairs` then lists every pair of rows that share a run of at least --min-len tokens once.  Between a query and a
corpus no pair is skipped: windows of one file on both sides are the leakage this tool is there to show.

motifs.json holds per query row its number of tokens, its longest match, the --top matches of at least --min-len tokens as
{corpus_row, source, length, query_event, corpus_event, transposition, distinct_tokens} -- the events are the positions of the
motif's first note in the two rows, the transposition is the query's first pitch minus the corpus', and distinct_tokens is
small for a trivial run such as a repeated note -- and copied_share; `summary` holds the mean and maximum longest match, the
share of rows whose longest match reaches 4, 8, 12, 16, 24 and 32 tokens and the mean copied share.  --baseline computes the
same summary for a held-out set against the same corpus: generated against train is to be read beside validation against
train.

host_tokens, host_lcs and host_rank restate the three kernels in numpy, bit for bit (all integers): they are the --cpu path
and the tests' oracle, vectorised over the corpus rows and meant for small inputs.  Motifs.match is the device path.  Every
check runs on the host before any GPU use and raises MotifError; the tool prints `motifs: error: ...` and returns status 2.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import midi_rolls as MR
from .gan.music_metrics import decode_rolls
from .midi_in import GRID
from .pieces import run_tool

MODES = {"interval+rhythm": 0, "interval": 1}
PAD = 0xFFFF
MAX_T = 4096
RHYTHM_EDGES = (12, 24, 48, 96, 192)        # ticks of 1/64 beat: a 16th triplet .. three beats
SHARE_AT = (4, 8, 12, 16, 24, 32)
DEFAULT_MIN_LEN, DEFAULT_TOP, DEFAULT_BATCH = 8, 3, 64


class MotifError(ValueError):
    """An argument or an input the tool cannot work with."""


def event_ticks(decoded: dict) -> np.ndarray:
    """The ticks every position takes, int64 (..., T): floor(step * 64 + 0.5) in fp64 where the event is valid, else 0."""
    with np.errstate(all="ignore"):
        return np.where(decoded["valid"], np.floor(decoded["step"] * float(GRID) + 0.5), 0.0).astype(np.int64)


def host_tokens(rolls, mode: int = 0):
    """mg_motif_tokens on the host: rolls (N, T, 4) float32 -> (tokens uint16 (N, T), PAD from a row's length on; lengths
    int32 (N,))."""
    x = np.asarray(rolls)
    if x.ndim != 3 or x.shape[2] != 4 or x.dtype != np.float32:
        raise ValueError(f"host_tokens: (N, T, 4) float32 rolls expected, got {x.dtype} {x.shape}")
    if mode not in (0, 1):
        raise ValueError(f"host_tokens: mode = {mode}: 0 (interval+rhythm) or 1 (interval)")
    N, T = x.shape[0], x.shape[1]
    d = decode_rolls(x)
    ticks = event_ticks(d)
    onset = np.cumsum(ticks, axis=1) - ticks
    tokens = np.full((N, T), PAD, np.uint16)
    lengths = np.zeros(N, np.int32)
    for n in range(N):
        s = np.flatnonzero(d["sounding"][n])
        if s.size < 2:
            continue
        interval = np.diff(d["pitch"][n, s].astype(np.int64))
        ioi = np.diff(onset[n, s])
        rhythm = sum((ioi >= e).astype(np.int64) for e in RHYTHM_EDGES) if mode == 0 else 0
        tokens[n, :s.size - 1] = ((interval + 64) | (rhythm << 7)).astype(np.uint16)
        lengths[n] = s.size - 1
    return tokens, lengths


def pack(L, i_end, j_end):
    L, i_end, j_end = np.asarray(L, np.int64), np.asarray(i_end, np.int64), np.asarray(j_end, np.int64)
    return np.where(L > 0, (L << 32) | ((0xFFFF - i_end) << 16) | (0xFFFF - j_end), 0).astype(np.int64)


def unpack(packed):
    """A packed match as (L, i_end, j_end), int64 arrays of its shape; (0, -1, -1) where there is none."""
    p = np.asarray(packed, np.int64)
    L = p >> 32
    hit = L > 0
    return L, np.where(hit, 0xFFFF - ((p >> 16) & 0xFFFF), -1), np.where(hit, 0xFFFF - (p & 0xFFFF), -1)


def _token_rows(tokens, lengths, who):
    t, n = np.asarray(tokens), np.asarray(lengths)
    if t.ndim != 2 or t.dtype != np.uint16 or n.shape != (t.shape[0],):
        raise ValueError(f"{who}: tokens uint16 (N, T) and lengths (N,) expected, got {t.dtype} {t.shape} and {n.shape}")
    return t, np.clip(n.astype(np.int64), 0, t.shape[1])


def host_lcs(q_tokens, q_len, c_tokens, c_len, q_groups=None, c_groups=None):
    """mg_motif_lcs on the host: (packed int64 (Nq, Nc), reach int32 (Nq, T)).  One row of the run table per query position,
    all corpus rows at once."""
    qt, ql = _token_rows(q_tokens, q_len, "host_lcs: query")
    ct, cl = _token_rows(c_tokens, c_len, "host_lcs: corpus")
    if qt.shape[1] != ct.shape[1]:
        raise ValueError(f"host_lcs: the query's T = {qt.shape[1]}, the corpus' {ct.shape[1]}")
    if (q_groups is None) != (c_groups is None):
        raise ValueError("host_lcs: q_groups and c_groups go together")
    (Nq, T), Nc = qt.shape, ct.shape[0]
    packed = np.zeros((Nq, Nc), np.int64)
    reach = np.zeros((Nq, T), np.int32)
    if Nc == 0:
        return packed, reach
    live = np.arange(T)[None, :] < cl[:, None]
    for q in range(Nq):
        keep = live if q_groups is None else live & (np.asarray(c_groups) != np.asarray(q_groups)[q])[:, None]
        run = np.zeros((Nc, T + 1), np.int64)       # run[:, j + 1] = run(i, j)
        best, bi, bj = np.zeros(Nc, np.int64), np.full(Nc, -1, np.int64), np.full(Nc, -1, np.int64)
        for i in range(int(ql[q])):
            new = np.where((ct == qt[q, i]) & keep, run[:, :-1] + 1, 0)
            top, arg = new.max(axis=1), new.argmax(axis=1)      # the first maximum: the smallest j
            up = top > best                                     # strictly: the smallest i
            best[up], bi[up], bj[up] = top[up], i, arg[up]
            reach[q, i] = top.max()
            run[:, 1:] = new
        packed[q] = pack(best, bi, bj)
    return packed, reach


def host_rank(packed, k: int):
    """mg_motif_rank on the host: (vals int64 (Nq, k), idx int32 (Nq, k))."""
    p = np.asarray(packed, np.int64)
    if p.ndim != 2 or int(k) < 1:
        raise ValueError(f"host_rank: packed (Nq, Nc) and k >= 1 expected, got {p.shape}, k = {k}")
    Nq, Nc = p.shape
    vals, idx = np.zeros((Nq, k), np.int64), np.full((Nq, k), -1, np.int32)
    n = min(int(k), Nc)
    for q in range(Nq):
        order = np.argsort(-p[q], kind="stable")[:n]
        vals[q, :n], idx[q, :n] = p[q, order], order
    return vals, idx


def copied_share(reach_row, n_tokens: int, m: int) -> float:
    """The share of a row's tokens inside a run of at least m tokens shared with the corpus: a position i with r = reach[i] >=
    m covers i - r + 1 .. i."""
    n = int(n_tokens)
    if n < 1:
        return 0.0
    r = np.asarray(reach_row)[:n].astype(np.int64)
    covered = np.zeros(n + 1, np.int64)
    for i in np.flatnonzero(r >= m):
        covered[i - r[i] + 1] += 1
        covered[i + 1] -= 1
    return float(int((np.cumsum(covered)[:n] > 0).sum()) / n)


@dataclass
class Match:
    """What both paths return: the token rows of both sides, per query row its `top` best corpus rows (packed values,
    descending, and their rows; 0 and -1 past the corpus' size) and reach."""
    q_tokens: np.ndarray
    q_len: np.ndarray
    c_tokens: np.ndarray
    c_len: np.ndarray
    vals: np.ndarray
    idx: np.ndarray
    reach: np.ndarray


def _check_match_args(query_rolls, corpus_rolls, q_groups, c_groups):
    q, c = np.asarray(query_rolls), np.asarray(corpus_rolls)
    for name, x in (("query", q), ("corpus", c)):
        if x.ndim != 3 or x.shape[2] != 4 or x.dtype != np.float32 or x.shape[0] < 1:
            raise ValueError(f"match: {name} rolls (N >= 1, T, 4) float32 expected, got {x.dtype} {x.shape}")
    if q.shape[1] != c.shape[1] or not 1 <= q.shape[1] <= MAX_T:
        raise ValueError(f"match: the query's T = {q.shape[1]}, the corpus' {c.shape[1]}: equal and in 1..{MAX_T}")
    if (q_groups is None) != (c_groups is None):
        raise ValueError("match: q_groups and c_groups go together")
    if q_groups is not None:
        q_groups, c_groups = np.ascontiguousarray(q_groups, np.int32), np.ascontiguousarray(c_groups, np.int32)
        if q_groups.shape != (q.shape[0],) or c_groups.shape != (c.shape[0],):
            raise ValueError("match: one group id per row expected")
    return np.ascontiguousarray(q), np.ascontiguousarray(c), q_groups, c_groups


def host_match(query_rolls, corpus_rolls, q_groups=None, c_groups=None, mode: int = 0, top: int = DEFAULT_TOP) -> Match:
    """Motifs.match on the host."""
    q, c, qg, cg = _check_match_args(query_rolls, corpus_rolls, q_groups, c_groups)
    qt, ql = host_tokens(q, mode)
    ct, cl = host_tokens(c, mode)
    packed, reach = host_lcs(qt, ql, ct, cl, qg, cg)
    vals, idx = host_rank(packed, top)
    return Match(qt, ql, ct, cl, vals, idx, reach)


class Motifs:
    """The device path: the corpus' tokens once, then the queries in chunks of `batch` rows -- tokens, the (batch, Nc) pair
    matrix, the ranking -- with one device -> host read per chunk."""

    def __init__(self, mode: int = 0, top: int = DEFAULT_TOP, batch: int = DEFAULT_BATCH, device: str = "cuda"):
        from . import ops
        from .pieces import require_device
        require_device()
        if mode not in (0, 1) or not 1 <= int(top) <= ops.MOTIF_MAX_K or int(batch) < 1:
            raise ValueError(f"Motifs: mode = {mode}, top = {top}, batch = {batch}: mode 0 or 1, top in 1..{ops.MOTIF_MAX_K}, batch >= 1")
        self.mode, self.top, self.batch, self.device = int(mode), int(top), min(int(batch), ops.MOTIF_MAX_QUERIES), device

    def match(self, query_rolls, corpus_rolls, q_groups=None, c_groups=None) -> Match:
        import torch
        from . import ops
        q, c, qg, cg = _check_match_args(query_rolls, corpus_rolls, q_groups, c_groups)
        d = torch.device(self.device)
        Nq, T, k = q.shape[0], q.shape[1], self.top
        ct, cl = ops.motif_tokens(torch.from_numpy(c).to(d), self.mode)
        qg_d = cg_d = None
        if qg is not None:
            qg_d, cg_d = torch.from_numpy(qg).to(d), torch.from_numpy(cg).to(d)
        out = Match(np.empty((Nq, T), np.uint16), np.empty(Nq, np.int32), ct.cpu().numpy(), cl.cpu().numpy(),
                    np.empty((Nq, k), np.int64), np.empty((Nq, k), np.int32), np.empty((Nq, T), np.int32))
        for lo in range(0, Nq, self.batch):
            hi = min(Nq, lo + self.batch)
            qt, ql = ops.motif_tokens(torch.from_numpy(q[lo:hi]).to(d), self.mode)
            packed, reach = ops.motif_lcs(qt, ql, ct, cl, None if qg_d is None else qg_d[lo:hi], cg_d)
            vals, idx = ops.motif_rank(packed, k)
            parts = ((vals, out.vals), (idx, out.idx), (reach, out.reach), (ql, out.q_len), (qt, out.q_tokens))
            blob = torch.cat([t.reshape(-1).view(torch.uint8) for t, _ in parts]).cpu().numpy()     # the chunk's one read
            off = 0
            for t, dst in parts:
                n = t.numel() * t.element_size()
                dst[lo:hi] = blob[off:off + n].view(dst.dtype).reshape(dst[lo:hi].shape)
                off += n
        return out


# ---- the report ------------------------------------------------------------------------------------------------------------

@dataclass
class RollSet:
    """Rows of rolls with where they come from: `groups` one key per row (rows of one key are windows of one file), `sources`
    one display name per row, `units` the file or set a row is reported under on stdout."""
    rolls: np.ndarray
    groups: List[str] = field(default_factory=list)
    sources: List[str] = field(default_factory=list)
    units: List[str] = field(default_factory=list)


def describe(m: Match, q: RollSet, c: RollSet, min_len: int) -> List[dict]:
    """The rows of motifs.json from a Match and the two sets."""
    dq, dc = decode_rolls(q.rolls), decode_rolls(c.rolls)
    L, i_end, j_end = unpack(m.vals)
    rows = []
    for r in range(q.rolls.shape[0]):
        n = int(m.q_len[r])
        sq = np.flatnonzero(dq["sounding"][r])
        matches = []
        for t in range(m.vals.shape[1]):
            cr, ln = int(m.idx[r, t]), int(L[r, t])
            if cr < 0 or ln < max(1, min_len):
                continue
            i0, j0 = int(i_end[r, t]) - ln + 1, int(j_end[r, t]) - ln + 1
            sc = np.flatnonzero(dc["sounding"][cr])
            qe, ce = int(sq[i0]), int(sc[j0])       # token k lies between the sounding notes k and k + 1
            matches.append({"corpus_row": cr, "source": c.sources[cr], "length": ln, "query_event": qe, "corpus_event": ce,
                            "transposition": int(dq["pitch"][r, qe]) - int(dc["pitch"][cr, ce]),
                            "distinct_tokens": int(np.unique(m.q_tokens[r, i0:i0 + ln]).size)})
        rows.append({"row": r, "source": q.sources[r], "tokens": n, "longest": int(L[r, 0]), "matches": matches,
                     "copied_share": copied_share(m.reach[r], n, min_len)})
    return rows


def summarise(rows: Sequence[dict]) -> dict:
    longest = np.array([r["longest"] for r in rows], np.int64)
    share = [r["copied_share"] for r in rows]
    return {"rows": len(rows), "mean_longest": float(longest.mean()), "max_longest": int(longest.max()),
            "share_longest_at_least": {str(t): float((longest >= t).mean()) for t in SHARE_AT},
            "mean_copied_share": float(np.mean(share))}


def pairs_once(rows: Sequence[dict]) -> List[dict]:
    """--self: every pair of rows among the reported matches once, under its longer match (then the lower rows), longest
    first."""
    best = {}
    for r in rows:
        for m in r["matches"]:
            key = (min(r["row"], m["corpus_row"]), max(r["row"], m["corpus_row"]))
            cand = dict(m, row=r["row"], row_source=r["source"])
            old = best.get(key)
            if old is None or (cand["length"], -cand["row"]) > (old["length"], -old["row"]):
                best[key] = cand
    return sorted(best.values(), key=lambda p: (-p["length"], p["row"], p["corpus_row"]))


# ---- the tool --------------------------------------------------------------------------------------------------------------

def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Find motifs that pieces share, whatever key they are in")
    ap.add_argument("query", nargs="*", metavar="QUERY", help="MIDI files, directories, split directories or a .npy of rolls")
    ap.add_argument("--corpus", nargs="+", default=None, metavar="CORPUS", help="what the queries are matched against")
    ap.add_argument("--baseline", nargs="+", default=None, metavar="HELDOUT", help="a held-out set matched against the same corpus")
    ap.add_argument("--self", dest="self_match", action="store_true", help="match the corpus against itself")
    ap.add_argument("--tokens", type=str, default="interval+rhythm", help=" or ".join(MODES))
    ap.add_argument("--min-len", type=int, default=DEFAULT_MIN_LEN, help="tokens a shared run needs to be reported and to count as copied")
    ap.add_argument("--top", type=int, default=DEFAULT_TOP, help="corpus rows kept per query row")
    MR.add_window_arguments(ap, max_notes=True)
    ap.add_argument("--batch", type=int, default=DEFAULT_BATCH, help="query rows per pair matrix")
    ap.add_argument("--cpu", action="store_true", help="the numpy restatement instead of the device")
    ap.add_argument("--out", type=str, default="motifs.json")
    return ap.parse_args(argv)


def _split_rows(path: str, notes: np.ndarray):
    """Groups and display names of a split directory's rows: index.json's `file` and `window_start` where it has them."""
    n = notes.shape[0]
    keys, names = [f"{path}#{i}" for i in range(n)], [f"{path}#{i}" for i in range(n)]
    idx = os.path.join(path, "index.json")
    if os.path.isfile(idx):
        try:
            with open(idx) as fh:
                rows = json.load(fh).get("rows", [])
        except (OSError, ValueError) as e:
            raise MotifError(f"{idx}: {e}") from e
        if len(rows) == n and all(isinstance(r, dict) and "file" in r for r in rows):
            keys = [str(r["file"]) for r in rows]
            names = [f"{r['file']}@{int(r.get('window_start', 0))}" for r in rows]
    return keys, names


def _load_rolls(path: str) -> np.ndarray:
    try:
        x = np.load(path, allow_pickle=False)
    except (OSError, ValueError) as e:
        raise MotifError(f"{path}: {e}") from e
    if x.ndim != 3 or x.shape[2] != 4 or x.dtype != np.float32:
        raise MotifError(f"{path}: rolls (N, T, 4) float32 expected, got {x.dtype} {x.shape}")
    if not 1 <= x.shape[1] <= MAX_T:
        raise MotifError(f"{path}: T = {x.shape[1]}: 1..{MAX_T}")
    return x


def plan_set(paths: Sequence[str], args, what: str) -> list:
    """The parts of a set, host only: ("rolls", RollSet) for a .npy or a split directory, ("midi", midi_rolls.Plan) for MIDI
    files, which run() encodes."""
    parts = []
    for p in paths:
        if os.path.isdir(p) and os.path.isfile(os.path.join(p, "notes.npy")):
            x = _load_rolls(os.path.join(p, "notes.npy"))
            keys, names = _split_rows(p, x)
            parts.append(("rolls", RollSet(x, keys, names, [p] * x.shape[0])))
        elif os.path.isfile(p) and p.lower().endswith(".npy"):
            x = _load_rolls(p)
            names = [f"{p}#{i}" for i in range(x.shape[0])]
            parts.append(("rolls", RollSet(x, list(names), names, [p] * x.shape[0])))
        elif os.path.isdir(p) or (os.path.isfile(p) and p.lower().endswith(MR.EXTENSIONS)):
            parts.append(("midi", MR.plan_from_args([p], args.max_notes, args, lambda m: MotifError(f"{what}: {m}"), search=True)))
        elif os.path.exists(p):
            raise MotifError(f"{what}: {p}: not a MIDI file, a directory or a .npy of rolls")
        else:
            raise MotifError(f"{what}: {p}: no such file or directory")
    if sum(part[1].rolls.shape[0] if part[0] == "rolls" else part[1].win_start.shape[0] for part in parts) < 1:
        raise MotifError(f"{what}: no rows")
    return parts


@dataclass
class MotifPlan:
    query: Optional[list]
    corpus: list
    baseline: Optional[list]
    mode: int
    args: object
    device: bool


def plan(args) -> MotifPlan:
    if args.tokens not in MODES:
        raise MotifError(f"--tokens '{args.tokens}': one of {', '.join(MODES)}")
    if args.top < 1 or args.top > 1024:
        raise MotifError(f"--top = {args.top}: 1..1024")
    if args.min_len < 1 or args.batch < 1:
        raise MotifError(f"--min-len = {args.min_len}, --batch = {args.batch}: both must be positive")
    if not 1 <= args.max_notes <= MAX_T:
        raise MotifError(f"--max-notes = {args.max_notes}: 1..{MAX_T}")
    if not args.corpus:
        raise MotifError("--corpus is required")
    if args.self_match and (args.query or args.baseline):
        raise MotifError("--self matches the corpus against itself: it cannot go with QUERY or --baseline")
    if not args.self_match and not args.query:
        raise MotifError("no QUERY (or --self)")
    corpus = plan_set(args.corpus, args, "--corpus")
    query = None if args.self_match else plan_set(args.query, args, "QUERY")
    baseline = plan_set(args.baseline, args, "--baseline") if args.baseline else None
    device = False
    if not args.cpu:
        import torch
        device = torch.cuda.is_available()
        if not device:
            raise MotifError("no MI355X (ROCm) device: --cpu runs the numpy restatement")
    return MotifPlan(query, corpus, baseline, MODES[args.tokens], args, device)


def _materialise(parts: list, device: bool) -> List[RollSet]:
    out = []
    for kind, part in parts:
        if kind == "rolls":
            out.append(part)
            continue
        x, _ = MR.encode_plan(part, device)
        files = [part.files[f]["file"] for f in np.repeat(np.arange(len(part.files)), np.diff(part.file_off))]
        out.append(RollSet(x, list(files), [f"{f}@{int(s)}" for f, s in zip(files, part.win_local)], list(files)))
    return out


def _join(sets: List[RollSet], T: int) -> RollSet:
    """One set of rows of T positions: shorter rows are filled up with the padding row, a rest, which adds no token."""
    rolls = np.full((sum(s.rolls.shape[0] for s in sets), T, 4), -1.0, np.float32)
    at, out = 0, RollSet(rolls)
    for s in sets:
        n = s.rolls.shape[0]
        rolls[at:at + n, :s.rolls.shape[1]] = s.rolls
        at += n
        out.groups += s.groups
        out.sources += s.sources
        out.units += s.units
    return out


def _say(rows: Sequence[dict], q: RollSet):
    units = {}
    for r in rows:
        units.setdefault(q.units[r["row"]], []).append(r)
    for unit, rs in units.items():
        top = max(rs, key=lambda r: (r["longest"], -r["row"]))
        where = f" (row {top['row']} with {top['matches'][0]['source']})" if top["matches"] else ""
        print(f"motifs: {unit}: {len(rs)} rows, longest shared run {top['longest']} tokens{where}, "
              f"copied share {float(np.mean([r['copied_share'] for r in rs])):.3f}")


def run(p: MotifPlan) -> dict:
    a = p.args
    sets = {name: _materialise(parts, p.device) for name, parts in (("corpus", p.corpus), ("query", p.query), ("baseline", p.baseline))
            if parts is not None}
    T = max(s.rolls.shape[1] for ss in sets.values() for s in ss)
    corpus = _join(sets["corpus"], T)
    query = corpus if p.query is None else _join(sets["query"], T)
    matcher = Motifs(p.mode, a.top, a.batch).match if p.device else (lambda *x: host_match(*x, mode=p.mode, top=a.top))

    def one(q: RollSet) -> List[dict]:
        qg = cg = None
        if q is corpus:     # --self: a file's own windows, and the row itself, are skipped
            ids = {}
            qg = cg = np.array([ids.setdefault(k, len(ids)) for k in corpus.groups], np.int32)
        return describe(matcher(q.rolls, corpus.rolls, qg, cg), q, corpus, a.min_len)

    rows = one(query)
    rep = {"tokens": a.tokens, "min_len": a.min_len, "top": a.top, "max_notes": T, "self": bool(a.self_match),
           "device": bool(p.device), "corpus": {"rows": int(corpus.rolls.shape[0]), "files": len(set(corpus.groups))},
           "rows": rows, "summary": summarise(rows)}
    _say(rows, query)
    if a.self_match:
        rep["pairs"] = pairs_once(rows)
        print(f"motifs: {len(rep['pairs'])} pairs of rows share a run of at least {a.min_len} tokens")
    if p.baseline is not None:
        held = _join(sets["baseline"], T)
        brows = one(held)
        rep["baseline"] = {"rows": brows, "summary": summarise(brows)}
        _say(brows, held)
        print(f"motifs: mean longest {rep['summary']['mean_longest']:.2f} against the baseline's "
              f"{rep['baseline']['summary']['mean_longest']:.2f}; mean copied share {rep['summary']['mean_copied_share']:.3f} "
              f"against {rep['baseline']['summary']['mean_copied_share']:.3f}")
    MR.write_report(a.out, rep)
    return rep


def main(argv=None) -> int:
    return run_tool("motifs", MotifError, plan, run, parse_args(argv))


if __name__ == "__main__":
    sys.exit(main())
