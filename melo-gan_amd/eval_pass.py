"""What the held-out evaluators share (gan/evaluate.py, ae/evaluate.py, emotion_discriminator/evaluate.py): the check of a
resident split, the per-split state a captured batch holds the addresses of, one packed result buffer with one device -> host
read, the keyed cache of captured batches, and the pass itself -- reset, one replay per batch, one read.  What a batch
launches, and in which order, stays with each evaluator.  And what the tools that walk chunks behind a host-advanced cursor
share (predict, explain, midi_import, motifs, ae.edit): CursorPass, DeviceWindows and device_roll_encode."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from . import ops


def check_split(err, x, row, labels, noun: str = "the split has", labels_optional: bool = False) -> int:
    """A resident split against what the engine reads: x a contiguous fp32 device array (n >= 1, *row), labels an int64 device
    array of n entries (None where labels_optional).  Raises err; returns n."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous():
        raise err("evaluate: the split must be a contiguous fp32 array on the device")
    if x.dim() != len(row) + 1 or tuple(x.shape[1:]) != tuple(row):
        raise err(f"evaluate: {noun} shape {tuple(x.shape)}, the config implies (n, {', '.join(map(str, row))})")
    n = x.shape[0]
    if n < 1:
        raise err("evaluate: the split is empty")
    if labels is None and labels_optional:
        return n
    if not isinstance(labels, torch.Tensor) or not labels.is_cuda or labels.dtype != torch.int64 or tuple(labels.shape) != (n,):
        raise err(f"evaluate: labels must be an int64 device array of {n} entries")
    return n


class Packed(ops.Layout):
    """One int64 buffer that holds several typed arrays: `parts` is an ordered list of (name, shape, dtype in int64 / float64 /
    float32 / int32).  self.dev: the typed views of the device buffer by name; host(): the same views of one .cpu() copy --
    every result of a pass in one device -> host read, the sizes written once."""
    who = "Packed"

    def __init__(self, parts, device):
        super().__init__(parts)
        self.buf = self.new(device)
        self.dev = self.views(self.buf)

    def host(self) -> dict:
        return self.views(self.buf.cpu())


class GraphCache(dict):
    """key -> the captured graph of a set of launches.  A key seen for the first time runs its launches eagerly once, before
    the capture: other jobs or a switched metric can need workspaces that no earlier run allocated.  What that run wrote is
    the caller's to discard.  A capture that raises stores nothing."""

    def graph(self, key, launches):
        if key not in self:
            launches()
            self[key] = ops.Graph.capture(launches)
        return self[key]


class ResidentPass:
    """The pass over a resident split in row order: the batch cursor ctr / base (int64 device scalars; the batch's metrics
    launch advances ctr), the state of the last split, and the graphs captured over it."""

    def __init__(self, B: int, device, graphs: Optional[GraphCache] = None):
        self.B, self.dev = int(B), device
        self.ctr = torch.zeros(1, dtype=torch.int64, device=device)
        self.base = torch.zeros(1, dtype=torch.int64, device=device)
        self.graphs = GraphCache() if graphs is None else graphs
        self.key = self.split = None

    @staticmethod
    def key_of(held, *extra):
        """What a captured batch froze: the data pointers of the `held` arrays (None allowed) and the sizes / switches `extra`."""
        return tuple(None if t is None else t.data_ptr() for t in held) + extra

    def bind(self, held, extra, n: int, labels, build):
        """The state of the split under key_of(held, *extra): n rows in nb batches (rows = nb * B), the labels padded to whole
        batches with -1 (the staging clamps the other arrays' padding rows into the split), the row order, the `held` arrays
        (while they live no other array can take their addresses and pass for them) and, set by build(split), the stage jobs.
        A new key builds a new state and empties the graph cache: the captured graphs hold the addresses."""
        key = self.key_of(held, *extra)
        if self.key != key:
            nb = (n + self.B - 1) // self.B
            split = SimpleNamespace(n=n, nb=nb, rows=nb * self.B, jobs=None, held=tuple(held),
                                    labels=torch.full((nb * self.B,), -1, dtype=torch.int64, device=self.dev),
                                    order=torch.arange(nb * self.B, dtype=torch.int64, device=self.dev))
            split.labels[:n] = 0 if labels is None else labels
            build(split)
            self.graphs.clear()
            self.split, self.key = split, key
        return self.split

    def run(self, key, launches, reset=None):
        """One pass of the batch `launches`, captured under `key`: reset() (the accumulator and the stashes), the cursor to 0,
        one replay per batch; the caller reads.  A new key's eager run starts from cursor 0 too, so every split position it
        touches is in range, and goes in front of the reset, which discards what it wrote: a pass's result does not depend on
        whether its graph was new."""
        if key not in self.graphs:
            self.ctr.zero_()
        graph = self.graphs.graph(key, launches)
        if reset is not None:
            reset()
        self.ctr.zero_()
        for _ in range(self.split.nb):
            graph.launch()


class CursorPass:
    """A pass in chunks whose cursor the host advances: ctr (the chunks behind it) and base (0), int64 device scalars, and the
    graphs captured over them.  What a chunk launches stays with the caller."""

    def __init__(self, device, graphs: Optional[GraphCache] = None):
        self.ctr = torch.zeros(1, dtype=torch.int64, device=device)
        self.base = torch.zeros(1, dtype=torch.int64, device=device)
        self.graphs = GraphCache() if graphs is None else graphs

    def replay(self, key, launches, nb: int, reset=None):
        """nb chunks of `launches`, captured under `key`, the cursor advancing behind each replay.  As in ResidentPass.run, a
        new key's eager run starts from chunk 0 and goes in front of reset(), which discards what it wrote.  Returns the two
        events around the replays: their time can be read once the stream is synchronised."""
        if key not in self.graphs:
            self.ctr.zero_()
        graph = self.graphs.graph(key, launches)
        if reset is not None:
            reset()
        self.ctr.zero_()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(nb):
            graph.launch()
            self.ctr.add_(1)
        t1.record()
        return t0, t1

    def each(self, nb: int):
        """replay's eager twin: `for c in each(nb)` runs its body at chunk c = 0 .. nb - 1, the cursor advancing behind it."""
        self.ctr.zero_()
        for c in range(nb):
            yield c
            self.ctr.add_(1)


class DeviceWindows:
    """The windows of a midi_rolls.Plan on the device: events (E, 4) int32, win_start (W,) int64, win_len (W,) int32, file_off
    (F + 1,) int64, and W, F, T.  Windows that are rolls already are given as (win_len, file_off, T) and have no events to
    encode.  While this object lives, the addresses a captured graph holds stay its arrays'."""

    def __init__(self, p, device):
        up = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a, dtype)).to(device)  # noqa: E731
        self.events = self.win_start = None
        if isinstance(p, tuple):
            win_len, file_off, self.T = p
        else:
            win_len, file_off, self.T = p.win_len, p.file_off, p.T
            self.events, self.win_start = up(p.events, np.int32), up(p.win_start, np.int64)
        self.win_len, self.file_off = up(win_len, np.int32), up(file_off, np.int64)
        self.W, self.F = self.win_len.shape[0], self.file_off.shape[0] - 1

    def encode(self, x, loss, cur: CursorPass):
        """mg_roll_encode of the cursor's chunk of windows into x (B, T, 4), its clamp counts into loss (W, 8)."""
        return ops.roll_encode(self.events, self.win_start, self.win_len, x, loss, cur.ctr, cur.base)

    def vote_parts(self, K: int) -> list:
        """The Packed parts of the windows' clamp counts, logits and votes, the 8-byte ones first."""
        return [("loss", (self.W, ops.ROLL_LOSS_WORDS), torch.int64), ("probs", (self.W, K), torch.float64),
                ("file_mean", (self.F, K), torch.float64), ("logits", (self.W, K), torch.float32),
                ("win_pred", (self.W,), torch.int32), ("file_pred", (self.F,), torch.int32), ("switches", (self.F,), torch.int32)]

    def votes(self, r: dict):
        """mg_window_votes over r["logits"] into the other parts of vote_parts."""
        ops.window_votes(r["logits"], self.file_off, r["probs"], r["win_pred"], r["file_mean"], r["file_pred"], r["switches"])


def device_roll_encode(p, batch: int = 64):
    """midi_rolls.host_roll_encode's result from mg_roll_encode: chunks of `batch` windows, each scattered to its rows."""
    d = torch.device("cuda")
    win, cur, W, T = DeviceWindows(p, d), CursorPass(d), p.win_start.shape[0], p.T
    B = max(1, min(int(batch), W))
    x, out = torch.empty(B, T, 4, device=d), torch.empty(W, T * 4, device=d)
    loss = torch.zeros(W, ops.ROLL_LOSS_WORDS, dtype=torch.int64, device=d)
    for _ in cur.each((W + B - 1) // B):
        win.encode(x, loss, cur)
        ops.scatter_rows_cursor(x.view(B, T * 4), out, cur.ctr, cur.base)
    return out.cpu().numpy().reshape(W, T, 4), loss.cpu().numpy()
