"""GPU: mg_roll_encode against midi_rolls.host_roll_encode bit for bit (counters included), mg_window_votes against
host_window_votes, both eager, rerun and replayed, and mg_path_probs' bits after its softmax moved into a shared header."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import ops  # noqa: E402
from melo_gan_amd import midi_rolls as MR  # noqa: E402
from melo_gan_amd.gan import morph_metrics as MM  # noqa: E402

T, B, W = 16, 4, 6


def events():
    """Notes inside the contract's image, notes outside every range, rests, chords and short steps."""
    g = np.random.default_rng(0)
    n = 70
    ev = np.stack([g.integers(36, 97, n), g.integers(60, 128, n), g.integers(16, 257, n), g.integers(7, 257, n)], axis=1)
    ev[3] = (20, 30, 5, 0)
    ev[7] = (120, 127, 300, 3)
    ev[9] = (0, -1, 0, 256)
    ev[20] = (0, -1, 0, 7)
    ev[33] = (96, 60, 256, 256)
    ev[34] = (36, 127, 16, 6)
    ev[40] = (97, 59, 15, 1)
    return np.ascontiguousarray(ev, np.int32)


# full, partial and empty windows; overlapping; the last reaches the list's end
WIN_START = np.array([0, 16, 30, 5, 54, 69], np.int64)
WIN_LEN = np.array([16, 9, 0, 16, 16, 1], np.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def encode(ev, ws, wl, counter, base=0, loss_rows=W, graph=False, poison=True):
    x = torch.full((B, T, 4), 7.0, device="cuda")
    loss = torch.full((loss_rows, 8), -7, dtype=torch.int64, device="cuda")
    e, s, n = dev(ev), dev(ws), dev(wl)
    ctr, bs = torch.tensor([counter], dtype=torch.int64).cuda(), torch.tensor([base], dtype=torch.int64).cuda()
    launch = lambda: ops.roll_encode(e, s, n, x, loss, ctr, bs)  # noqa: E731
    launch()
    if graph:
        torch.cuda.synchronize()
        x.fill_(7.0)
        loss.fill_(-7)
        with torch.cuda.stream(torch.cuda.Stream()):
            g = ops.Graph.capture(launch)
            g.launch()
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    return x.cpu().numpy(), loss.cpu().numpy()


@pytest.fixture(scope="module")
def host():
    return MR.host_roll_encode(events(), WIN_START, WIN_LEN, T, rows=2 * B)


def test_roll_encode_equals_the_host_bit_for_bit_at_two_cursor_positions(host):
    hx, hl = host
    ev = events()
    assert (hl[:, :7].sum(axis=0) > 0).all() and hl[:, 7].tolist() == [1, 1, 0, 2, 0, 0, 0, 0]
    x0, l0 = encode(ev, WIN_START, WIN_LEN, 0)
    assert x0.tobytes() == hx[:B].tobytes()
    assert (l0[:B] == hl[:B]).all() and (l0[B:] == -7).all()       # a launch writes its own rows' counts alone
    x1, l1 = encode(ev, WIN_START, WIN_LEN, 5, base=4)              # the cursor is counter - base
    assert x1.tobytes() == hx[B:].tobytes()
    assert (x1[W - B:] == -1.0).all()                               # rows past W: the padding row
    assert (l1[B:W] == hl[B:W]).all() and (l1[:B] == -7).all()
    # counts of rows past W are zeros where the loss array has room for them, and go nowhere where it has not
    _, l2 = encode(ev, WIN_START, WIN_LEN, 1, loss_rows=2 * B)
    assert (l2[B:] == hl[B:]).all() and (l2[W:] == 0).all()
    # a cursor far past the end: padding rows, nothing counted
    x3, l3 = encode(ev, WIN_START, WIN_LEN, 1 << 40)
    assert (x3 == -1.0).all() and (l3 == -7).all()


def test_roll_encode_eager_rerun_and_replay_leave_identical_bits(host):
    ev = events()
    a = encode(ev, WIN_START, WIN_LEN, 0)
    b = encode(ev, WIN_START, WIN_LEN, 0)
    c = encode(ev, WIN_START, WIN_LEN, 0, graph=True)
    for x, l in (b, c):
        assert x.tobytes() == a[0].tobytes() and l.tobytes() == a[1].tobytes()
    assert a[0].tobytes() == host[0][:B].tobytes()


def test_a_window_outside_the_events_is_nan_and_reads_nothing():
    ev = events()
    ws = np.array([0, 60, -1, 5], np.int64)
    wl = np.array([16, 16, 4, 17], np.int32)            # past the end; a negative start; longer than T
    x, loss = encode(ev, ws, wl, 0, loss_rows=4)
    hx, hl = MR.host_roll_encode(ev, ws[:1], wl[:1], T)
    assert x[0].tobytes() == hx[0].tobytes() and (loss[0] == hl[0]).all()
    assert np.isnan(x[1:]).all() and (loss[1:] == -1).all()
    with pytest.raises(ValueError):
        MR.host_roll_encode(ev, ws, wl, T)


def test_ops_roll_encode_checks_its_arguments():
    e, s, n = dev(events()), dev(WIN_START), dev(WIN_LEN)
    x = torch.zeros(B, T, 4, device="cuda")
    loss = torch.zeros(W, 8, dtype=torch.int64, device="cuda")
    c = torch.zeros(1, dtype=torch.int64, device="cuda")
    for bad in (lambda: ops.roll_encode(e.to(torch.int64), s, n, x, loss, c, c),
                lambda: ops.roll_encode(e[:, :3].contiguous(), s, n, x, loss, c, c),
                lambda: ops.roll_encode(e, s, n[:5], x, loss, c, c),
                lambda: ops.roll_encode(e, s.to(torch.int32), n, x, loss, c, c),
                lambda: ops.roll_encode(e, s, n, x[:, :, :3].contiguous(), loss, c, c),
                lambda: ops.roll_encode(e, s, n, x, loss[:, :7].contiguous(), c, c),
                lambda: ops.roll_encode(e, s, n, x, loss, c.to(torch.int32), c),
                lambda: ops.roll_encode(e.cpu(), s, n, x, loss, c, c)):
        with pytest.raises(ValueError):
            bad()


K = 4
FILE_OFF = np.array([0, 1, 5, 5], np.int64)         # F = 3 files of 1, 4 and 0 windows


def logits():
    z = np.random.default_rng(1).normal(0, 2, (5, K)).astype(np.float32)
    z[2] = (1.5, 1.5, -1.0, 1.5)                    # a tie: the lowest index
    z[3] = z[2]                                     # no switch between equal verdicts
    return z


def votes(z, off, graph=False):
    zd, od = dev(z), dev(off)
    Wn, F = z.shape[0], off.shape[0] - 1
    out = [torch.full((Wn, K), 7.0, dtype=torch.float64, device="cuda"), torch.full((Wn,), 7, dtype=torch.int32, device="cuda"),
           torch.full((F, K), 7.0, dtype=torch.float64, device="cuda"), torch.full((F,), 7, dtype=torch.int32, device="cuda"),
           torch.full((F,), 7, dtype=torch.int32, device="cuda")]
    launch = lambda: ops.window_votes(zd, od, *out)  # noqa: E731
    launch()
    if graph:
        torch.cuda.synchronize()
        for t in out:
            t.fill_(7)
        with torch.cuda.stream(torch.cuda.Stream()):
            g = ops.Graph.capture(launch)
            g.launch()
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    return dict(zip(("probs", "win_pred", "file_mean", "file_pred", "switches"), (t.cpu().numpy() for t in out)))


def test_window_votes_against_the_host():
    z = logits()
    h = MR.host_window_votes(z, FILE_OFF)
    d = votes(z, FILE_OFF)
    for k in ("win_pred", "file_pred", "switches"):
        assert d[k].dtype == np.int32 and (d[k] == h[k]).all(), k
    assert h["win_pred"][2] == 0 and h["file_pred"][2] == -1 and h["switches"][2] == 0
    # each probability is a quotient of at most K terms of size <= 1: a few fp64 ulps of exp and the division
    assert np.abs(d["probs"] - h["probs"]).max() <= 1e-12
    # the project's bound for fp64 sums: 1e-12 of the sum of |terms|
    for f in range(3):
        lo, hi = FILE_OFF[f], FILE_OFF[f + 1]
        if hi == lo:
            assert (d["file_mean"][f] == 0).all()
            continue
        bound = 1e-12 * np.abs(h["probs"][lo:hi]).sum(axis=0) / (hi - lo)
        assert (np.abs(d["file_mean"][f] - h["file_mean"][f]) <= bound).all(), f
    # the device's own means are the sum of ITS probabilities in window order over their number, exactly
    own = np.zeros(K)
    for w in range(1, 5):
        own = own + d["probs"][w]
    assert (d["file_mean"][1] == own / 4.0).all() and (d["file_mean"][0] == d["probs"][0]).all()


def test_window_votes_nan_counts_as_the_maximum_and_bad_offsets_read_nothing():
    z = logits()
    z[1, 2] = np.nan
    z[4, 1] = z[4, 3] = np.nan
    h = MR.host_window_votes(z, FILE_OFF)
    d = votes(z, FILE_OFF)
    assert d["win_pred"].tolist() == h["win_pred"].tolist() and d["win_pred"][1] == 2 and d["win_pred"][4] == 1
    assert np.isnan(d["probs"][[1, 4]]).all() and np.isnan(d["file_mean"][1]).all() and d["file_pred"][1] == h["file_pred"][1] == 0
    assert d["switches"].tolist() == h["switches"].tolist()
    bad = votes(logits(), np.array([0, 6, 3, 5], np.int64))        # past W; backwards; fine
    assert np.isnan(bad["file_mean"][:2]).all() and bad["file_pred"][:2].tolist() == [-1, -1] and bad["switches"][:2].tolist() == [-1, -1]
    assert bad["file_pred"][2] >= 0 and bad["switches"][2] >= 0 and np.isfinite(bad["file_mean"][2]).all()


def test_window_votes_eager_rerun_and_replay_leave_identical_bits():
    z = logits()
    a, b, c = votes(z, FILE_OFF), votes(z, FILE_OFF), votes(z, FILE_OFF, graph=True)
    for o in (b, c):
        for k in a:
            assert a[k].tobytes() == o[k].tobytes(), k


def test_ops_window_votes_checks_its_arguments():
    z, off = dev(logits()), dev(FILE_OFF)
    for bad in (lambda: ops.window_votes(z[:, :1].contiguous(), off), lambda: ops.window_votes(z, off.to(torch.int32)),
                lambda: ops.window_votes(z, off[:1]), lambda: ops.window_votes(z.double(), off),
                lambda: ops.window_votes(z, off, probs=torch.zeros(5, K, device="cuda")),
                lambda: ops.window_votes(torch.zeros(5, 33, device="cuda"), off)):
        with pytest.raises(ValueError):
            bad()


def test_path_probs_bits_are_those_of_the_numpy_restatement_and_of_window_votes():
    """mg_path_probs' softmax now lives in a header that mg_window_votes shares: on one fixed input both give the same bits,
    and they stay within fp64 rounding of the numpy restatement (tests/test_morph_gpu.py remains the yardstick)."""
    z = np.random.default_rng(2).normal(0, 3, (12, K)).astype(np.float32)
    z[5] = 0.25
    group = np.zeros(4, np.int32)
    probs, acc = ops.path_probs(dev(z), dev(group), 3, 1)
    torch.cuda.synchronize()
    hp, ha = MM.host_path_probs(z, group, 3, 1)
    assert np.abs(probs.cpu().numpy() - hp).max() <= 1e-12
    assert np.abs(acc.cpu().numpy() - ha).max() <= 1e-12 * 4
    assert (probs.cpu().numpy()[5] == 0.25).all()              # 1 / (1 + 3 exp(0)) and exp(0) / 4: exact
    d = votes(z, np.array([0, 12], np.int64))
    assert d["probs"].tobytes() == probs.cpu().numpy().tobytes()
