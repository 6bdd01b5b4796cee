"""GPU: the chunk cursor and the device windows under predict, explain, midi_import, motifs and ae.edit (eval_pass.CursorPass,
DeviceWindows, device_roll_encode) with a stub in the classifier's place.  T = 8, B = 4, K = 3; two files of 4 and 2 windows:
two chunks, the second half empty, the last window shorter than T.  Every destination lies inside a canvas of sentinels."""
from contextlib import contextmanager

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import midi_rolls as MR  # noqa: E402
from melo_gan_amd import ops  # noqa: E402
from melo_gan_amd.eval_pass import CursorPass, DeviceWindows, device_roll_encode  # noqa: E402

T, B, K = 8, 4, 3
W, NB = 6, 2
SENT = 7                    # what every canvas is filled with


def make_plan() -> MR.Plan:
    g = np.random.default_rng(4)
    E = 45
    ev = np.stack([g.integers(30, 103, E), g.integers(40, 128, E), g.integers(8, 300, E), g.integers(0, 300, E)], axis=1)
    ev[11, 1] = -1          # a rest
    ws = np.array([0, 8, 16, 24, 32, 40], np.int64)
    files = [dict(file=n, notes=k, events=k, rests=0, beats=1.0, lead_q=0, dropped_drums=0, unpaired=0, dropped_events=0,
                  tempo_us=500000, division=480) for n, k in (("a.mid", 32), ("b.mid", 13))]
    return MR.Plan(np.ascontiguousarray(ev, np.int32), ws, np.array([8, 8, 8, 8, 8, 5], np.int32), ws % 32, np.zeros(W),
                   np.array([0, 4, 6], np.int64), files, T)


@pytest.fixture(scope="module")
def ref():
    """The plan and what the host makes of it, computed once and never written."""
    p = make_plan()
    MR.check_plan(p, T)                                         # every index below is in range
    hx, hl = MR.host_roll_encode(p.events, p.win_start, p.win_len, T)
    hz = hx[:, :K, 0] * np.float32(2.0) + hx[:, :K, 3]          # the stub: exact doubling, one fp32 rounding
    assert hz.dtype == np.float32 and hl[:, :7].sum() > 0 and hl[1, 7] == 1 and (hx[5, 5:] == -1.0).all()
    return dict(plan=p, rolls=hx.reshape(W, T * 4), loss=hl, logits=hz, **MR.host_window_votes(hz, p.file_off))


@contextmanager
def side_stream():
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        yield
        torch.cuda.synchronize()


class Rig:
    """The windows, a cursor, one batch's fixed buffers and every destination inside a canvas with one guard row on either
    side.  launches(): encode -> the stub forward -> scatter the rolls and the logits, as Predictor's chunk does."""

    def __init__(self, plan):
        self.win, self.cur = DeviceWindows(plan, "cuda"), CursorPass("cuda")
        assert (self.win.W, self.win.F, self.win.T) == (W, 2, T)
        self.x = torch.empty(B, T, 4, device="cuda")
        self.tmp, self.logits = torch.empty(B, K, device="cuda"), torch.empty(B, K, device="cuda")
        self.whole, self.r = {}, {}
        for name, shape, dtype in self.win.vote_parts(K) + [("rolls", (W, T * 4), torch.float32)]:
            self.whole[name] = torch.full((shape[0] + 2,) + tuple(shape[1:]), SENT, dtype=dtype, device="cuda")
            self.r[name] = self.whole[name][1:-1]

    def launches(self):
        r, cur = self.r, self.cur
        self.win.encode(self.x, r["loss"], cur)
        torch.mul(self.x[:, :K, 0], 2.0, out=self.tmp)          # out=: nothing is allocated inside a capture
        torch.add(self.tmp, self.x[:, :K, 3], out=self.logits)
        ops.scatter_rows_cursor(self.x.view(B, T * 4), r["rolls"], cur.ctr, cur.base)
        ops.scatter_rows_cursor(self.logits, r["logits"], cur.ctr, cur.base)

    def reset(self):
        for v in self.r.values():
            v.fill_(SENT)

    def host(self) -> dict:
        out = {k: v.cpu().numpy() for k, v in self.r.items()}
        out["guards"] = all(bool((w[0] == SENT).all() and (w[-1] == SENT).all()) for w in self.whole.values())
        return out


def captured(plan):
    with side_stream():
        rig = Rig(plan)
        events = rig.cur.replay("chunk", rig.launches, NB, rig.reset)
        rig.win.votes(rig.r)
        got = rig.host()
        assert events[0].elapsed_time(events[1]) >= 0.0 and int(rig.cur.ctr.item()) == NB and len(rig.cur.graphs) == 1
    return got


def same_bytes(a: dict, b: dict):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] is b[k] or a[k].tobytes() == b[k].tobytes(), k


def test_the_captured_pass_equals_the_host(ref):
    got = captured(ref["plan"])
    for k in ("rolls", "loss", "logits", "win_pred", "file_pred", "switches"):
        assert got[k].dtype == ref[k].dtype and got[k].tobytes() == ref[k].tobytes(), k
    assert np.abs(got["probs"] - ref["probs"]).max() <= 1e-12
    off = ref["plan"].file_off
    for f in range(2):
        lo, hi = int(off[f]), int(off[f + 1])
        bound = 1e-12 * np.abs(ref["probs"][lo:hi]).sum(axis=0) / (hi - lo)       # the project's bound for fp64 sums
        assert (np.abs(got["file_mean"][f] - ref["file_mean"][f]) <= bound).all(), f
    assert got["guards"]                                        # the second chunk's rows past W went nowhere


def test_the_eager_pass_leaves_the_captured_bytes(ref):
    with side_stream():
        rig = Rig(ref["plan"])
        rig.cur.ctr.fill_(NB)                                   # each starts from chunk 0 whatever came before
        seen = []
        for c in rig.cur.each(NB):
            seen.append(c)
            rig.launches()
        rig.win.votes(rig.r)
        got = rig.host()
        assert seen == [0, 1] and int(rig.cur.ctr.item()) == NB and not rig.cur.graphs
    assert got["guards"]
    same_bytes(got, captured(ref["plan"]))


def test_a_second_replay_repeats_itself_and_a_new_key_starts_at_chunk_0(ref):
    with side_stream():
        rig = Rig(ref["plan"])
        rig.cur.replay("chunk", rig.launches, NB, rig.reset)
        rig.win.votes(rig.r)
        first, graph = rig.host(), rig.cur.graphs["chunk"]
        rig.cur.replay("chunk", rig.launches, NB, rig.reset)
        rig.win.votes(rig.r)
        assert rig.cur.graphs["chunk"] is graph and len(rig.cur.graphs) == 1
        same_bytes(first, rig.host())
        # no replay at all: what is written is the new key's eager run, which must be chunk 0 although ctr stood at NB
        assert int(rig.cur.ctr.item()) == NB
        rig.reset()
        rig.cur.replay("other", rig.launches, 0)
        got = rig.host()
        assert len(rig.cur.graphs) == 2 and int(rig.cur.ctr.item()) == 0
    for k in ("rolls", "loss", "logits"):
        assert got[k][:B].tobytes() == ref[k][:B].tobytes() and (got[k][B:] == SENT).all(), k
    assert got["guards"]


def test_device_roll_encode_in_chunks_of_4_equals_the_host(ref):
    x, loss = device_roll_encode(ref["plan"], batch=B)
    assert x.dtype == np.float32 and x.shape == (W, T, 4) and x.tobytes() == ref["rolls"].tobytes()
    assert loss.dtype == np.int64 and loss.tobytes() == ref["loss"].tobytes()
    x1, loss1 = device_roll_encode(ref["plan"])                 # one chunk that holds every window
    assert x1.tobytes() == x.tobytes() and loss1.tobytes() == loss.tobytes()
