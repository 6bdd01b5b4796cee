"""GPU: mg_note_stats (csrc/note_metrics.hip) against its host reference music_metrics.host_stats -- every integer word equal,
the two fp64 sums within 1e-12 * sum |terms|, the split-position rules, eager == rerun == graph replay to the bit, and the
refusals before a launch."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import _lib, ops  # noqa: E402
from melo_gan_amd.gan import music_metrics as MM  # noqa: E402

K = 4
f32 = np.float32
SENTINEL = -7


def x0_of(pitch):
    return f32((pitch + 0.5) / 63.5 - 1.0)


def boundary_columns(T):
    """x0 at the integer pitch boundaries and x1 at float32(-0.2) and the integer velocity boundaries, each with its fp32
    neighbours and the values 1 and 4 ulps of 1.0 away (tests/test_music_metrics_cpu.py's set), cycled over T positions."""
    def around(v):
        v = np.asarray(v, dtype=f32)
        d = f32(2.0 ** -23)
        return np.concatenate([v - f32(4) * d, v - d, np.nextafter(v, f32(-4)), v, np.nextafter(v, f32(4)), v + d, v + f32(4) * d])
    x0 = around((np.arange(30, 101) / 63.5 - 1.0).astype(f32))
    x1 = np.concatenate([around([f32(-0.2)]), around((np.arange(0, 131) / 67.0 * 1.2 - 0.2).astype(f32))])
    return np.resize(x0, T), np.resize(np.roll(x1, 3), T)


def rests(x):
    x[:, 1] = -1.0


def plant(x, r, what, T):
    """The planted rows (x: one side's (B, T, 4) array)."""
    if what == "rests":
        rests(x[r])
    elif what == "chunk":          # a note at 255, rests to 300, a note: the previous pitch crosses the chunk and the wave
        if T > 300:
            rests(x[r])
            x[r, 255, :2] = (x0_of(48), 0.5)
            x[r, 300, :2] = (x0_of(79), 0.5)
    elif what == "wave":           # the last lane of one wave, then the first lane of the next
        if T > 64:
            rests(x[r])
            x[r, 63, :2] = (x0_of(40), 0.5)
            x[r, 64, :2] = (x0_of(90), 0.5)
    elif what == "edges":          # the decode boundaries, with NaN and +-inf positions among them
        x[r, :, 0], x[r, :, 1] = boundary_columns(T)
        x[r, 0, 2] = np.nan
        x[r, T // 2, 0] = np.inf
        x[r, T - 1, 3] = -np.inf
        if T > 5:
            x[r, 3, 1] = np.nan
            x[r, 4, 1] = np.inf


def kernel_inputs(B, T, call, g):
    real = g.uniform(-1.3, 1.3, (B, T, 4)).astype(f32)
    fake = (g.standard_normal((B, T, 4)) * 0.7).astype(f32)
    fake[:, :, 2:] *= 2.5                                                 # durations and steps beyond 1: bin 15
    labels = (np.arange(B) + call) % K
    if B >= 5:
        labels[call + 1::7] = -1                                          # padding rows, as tests/test_evaluate_gpu.py plants them
        side = real if call == 0 else fake
        for r, what in ((0, "rests"), (3, "chunk"), (4, "wave"), (2 if call == 0 else 1, "edges")):
            assert labels[r] >= 0
            plant(side, r, what, T)
    elif call == 1:
        labels[:] = -1                                                    # B = 1: the second call is all padding
    else:
        plant(real, 0, "edges", T)
    return real, fake, labels.astype(np.int64)


def new_outputs(dst_rows):
    return (ops.note_acc_new(K, "cuda"), torch.full((2, dst_rows, 8), SENTINEL, dtype=torch.int32, device="cuda"),
            torch.full((2, dst_rows, 2), float(SENTINEL), dtype=torch.float64, device="cuda"))


def compare(acc, row_i, row_beats, ref, written, what):
    """ref: host_stats over all the calls' rows in position order; written: which positions the kernel writes."""
    racc, ri, rb = ref
    dst = row_i.shape[1]
    assert np.array_equal(acc.cpu().numpy().reshape(2, K, -1), racc), what
    want_i = np.where(written[None, :dst, None], ri[:, :dst], SENTINEL)
    assert np.array_equal(row_i.cpu().numpy(), want_i), what
    got, want = row_beats.cpu().numpy(), np.where(written[None, :dst, None], rb[:, :dst], float(SENTINEL))
    finite = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), finite), what
    err, bound = np.abs(got - want)[finite], 1e-12 * np.abs(want)[finite]      # the terms are positive: sum |terms| is the sum
    print(f"{what}: max |err| / (1e-12 sum|terms|) = {float((err / np.maximum(bound, 1e-300)).max()):.3g}")
    assert (err <= bound).all(), what


@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("T", [1, 20, 63, 256, 257, 600, 512])
def test_note_stats_matches_the_host(T, B):
    g = np.random.default_rng(1000 * T + B)
    calls = [kernel_inputs(B, T, call, g) for call in (0, 1)]
    dev = [tuple(torch.from_numpy(a).cuda() for a in c) for c in calls]
    dst_rows = 2 * B - 3 if B >= 5 else 1                                  # the last positions of the second call fall off
    base = torch.full((1,), 7, dtype=torch.int64, device="cuda")         # a non-zero base
    counters = [torch.full((1,), 7 + call, dtype=torch.int64, device="cuda") for call in (0, 1)]

    def run(out):
        for (real, fake, labels), ctr in zip(dev, counters):              # two calls into one accumulator: it adds
            ops.note_stats(real, fake, labels, out[0], out[1], out[2], ctr, base, K)

    ref = MM.host_stats(np.concatenate([c[0] for c in calls]), np.concatenate([c[1] for c in calls]),
                        np.concatenate([c[2] for c in calls]), K)
    written = np.concatenate([c[2] for c in calls]) >= 0
    out = new_outputs(dst_rows)
    run(out)
    torch.cuda.synchronize()
    compare(*out, ref, written, "eager")
    v = MM.acc_views(ref[0])
    if B >= 5:
        assert v["counters"][:, :, 4].sum() >= 2 and v["counters"][0, 0, 3] >= T           # invalid positions; the row of rests
    if B >= 5 and T > 300:          # notes, rests, invalid, unique, lowest, highest, transitions of the two chaining rows
        cols = [0, 1, 2, 3, 4, 5, 7]
        assert ref[1][0, 3, cols].tolist() == [2, T - 2, 0, 2, 48, 79, 1] and ref[1][0, 4, cols].tolist() == [2, T - 2, 0, 2, 40, 90, 1]
    if B == 64 and T >= 256:
        assert (v["dur16"][1, :, 15] > 0).all() and (v["step16"][1, :, 15] > 0).all() and (v["pctm"].sum((0, 1)) > 0).all()
    # a rerun: the same bits
    out2 = new_outputs(dst_rows)
    run(out2)
    torch.cuda.synchronize()
    for a, b in zip(out, out2):
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)
    # a graph replay: the same bits
    out3 = new_outputs(dst_rows)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        gr = ops.Graph()
        gr.begin()
        try:
            run(out3)
        finally:
            gr.end()
        gr.launch()
    torch.cuda.synchronize()
    for a, b in zip(out, out3):
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)
    # reset: back to zeros
    ops.note_acc_reset(out3[0], K)
    torch.cuda.synchronize()
    assert int(out3[0].abs().sum()) == 0


def test_planted_rows_have_their_known_numbers():
    """The order-dependent part on rows whose answers are known without the host reference."""
    T, B = 600, 6
    x = np.zeros((B, T, 4), dtype=f32)
    x[:, :, 1] = -1.0                                                     # rests only: nothing chains
    x[1, 255, :2], x[1, 300, :2] = (x0_of(48), 0.5), (x0_of(79), 0.5)     # across the chunk
    x[2, 63, :2], x[2, 64, :2] = (x0_of(40), 0.5), (x0_of(90), 0.5)       # across the wave
    x[3, 10, :2], x[3, 599, :2] = (x0_of(60), 0.5), (x0_of(61), 0.5)      # across two chunks and three waves of rests
    x[4, 100, :2], x[4, 101, 1], x[4, 102, :2] = (x0_of(72), 0.5), np.nan, (x0_of(60), 0.5)      # an invalid position between
    x[5, :, 1], x[5, :, 0] = 0.5, x0_of(50)                               # every position sounds
    x[5, 511, 0], x[5, 512, 0] = x0_of(36), x0_of(96)
    labels = np.array([0, 1, 1, 2, 2, 3], dtype=np.int64)
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    acc, row_i, row_beats = new_outputs(B)
    xd = torch.from_numpy(x).cuda()
    ops.note_stats(xd, xd, torch.from_numpy(labels).cuda(), acc, row_i, row_beats, ctr, ctr, K)
    torch.cuda.synchronize()
    ri = row_i.cpu().numpy()
    assert np.array_equal(ri[0], ri[1])
    assert ri[0, 0].tolist() == [0, T, 0, 0, 0, 0, 0, 0]
    assert ri[0, 1].tolist() == [2, T - 2, 0, 2, 48, 79, 0, 1]
    assert ri[0, 2].tolist() == [2, T - 2, 0, 2, 40, 90, 0, 1]
    assert ri[0, 3].tolist() == [2, T - 2, 0, 2, 60, 61, 0, 1]
    assert ri[0, 4].tolist() == [2, T - 3, 1, 2, 60, 72, 0, 1]
    assert ri[0, 5].tolist() == [T, 0, 0, 3, 36, 96, 0, T - 1]                # dur = step = 2 beats: no overlap
    v = MM.acc_views(acc.cpu().numpy().reshape(2, K, -1))
    assert v["interval"][0, 1, 31] == 1 and v["interval"][0, 1, 50] == 1 and v["interval"][0, 1].sum() == 2
    assert v["pctm"][0, 1, 0, 7] == 1 and v["pctm"][0, 1, 4, 6] == 1
    assert v["interval"][0, 2, 1] == 1 and v["interval"][0, 2, 12] == 1 and v["interval"][0, 0].sum() == 0
    want = np.zeros(64, dtype=np.int64)
    want[[0, 14, 60, 46]] = (T - 4, 1, 1, 1)                              # 50 -> 36 -> 96 -> 50 among repeated 50s
    assert np.array_equal(v["interval"][0, 3], want)
    assert np.array_equal(row_beats.cpu().numpy()[0, :, 0], [2.0 * T] * 4 + [2.0 * (T - 1), 2.0 * T])
    assert np.array_equal(acc.cpu().numpy().reshape(2, K, -1), MM.host_stats(x, x, labels, K)[0])


def test_note_stats_at_the_longest_row():
    """T = 2^20, the domain's upper edge: 4096 chunks of carried pitch."""
    T = 1 << 20
    g = np.random.default_rng(9)
    real = g.uniform(-1.3, 1.3, (1, T, 4)).astype(f32)
    fake = real[:, ::-1].copy()
    fake[0, 1000:900000, 1] = -1.0                                        # a long run of rests to carry a pitch over
    labels = np.array([2], dtype=np.int64)
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = new_outputs(1)
    ops.note_stats(torch.from_numpy(real).cuda(), torch.from_numpy(fake).cuda(), torch.from_numpy(labels).cuda(), *out, ctr, ctr, K)
    torch.cuda.synchronize()
    compare(*out, MM.host_stats(real, fake, labels, K), np.array([True]), "T = 2^20")


def test_note_stats_refusals_before_a_launch():
    B, T = 4, 16
    real, fake = torch.zeros(B, T, 4, device="cuda"), torch.zeros(B, T, 4, device="cuda")
    labels, ctr = torch.zeros(B, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    acc, row_i, row_beats = new_outputs(B)
    before = [t.clone() for t in (acc, row_i, row_beats)]
    ok = (real, fake, labels, acc, row_i, row_beats, ctr, ctr, K)

    def refused(match, **kw):
        names = ("real", "fake", "emot_idx", "acc", "row_i", "row_beats", "counter", "base", "n_classes")
        args = dict(zip(names, ok), **kw)
        with pytest.raises(ValueError, match=match):
            ops.note_stats(**args)

    wide = torch.zeros(B, T, 8, device="cuda")
    refused("only the", real=wide, fake=wide)                             # C != 4
    flat = torch.zeros(B * T * 4 + 1, device="cuda")
    refused("16-byte aligned", real=flat[1:].view(B, T, 4))               # a misaligned pointer
    refused("CUDA/HIP tensor", real=real.cpu())                           # a CPU tensor
    refused("CUDA/HIP tensor", row_beats=row_beats.cpu())
    refused("1..32 classes", n_classes=33)
    refused("row_i", row_i=torch.zeros(2, B, 4, dtype=torch.int32, device="cuda"))
    refused("acc", acc=torch.zeros(7, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        ops.note_acc_layout(0)
    # the C entry point itself: -1 before any launch
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(Bc=B, Tc=T, Cc=4, Kc=K, realp=None, dst=B):
        return lib.mg_note_stats(p(real) if realp is None else realp, p(fake), Bc, Tc, Cc, p(labels), Kc, p(acc), p(row_i), p(row_beats), dst, p(ctr),
                                 p(ctr), st)

    assert call(Cc=8) == -1 and b"note-row" in lib.mg_last_error()
    assert call(Cc=128) == -1 and call(Bc=0) == -1 and call(Bc=32768) == -1 and call(Tc=0) == -1 and call(Tc=(1 << 20) + 1) == -1
    assert call(Kc=0) == -1 and call(Kc=33) == -1 and call(dst=0) == -1
    assert call(realp=ctypes.c_void_p(real.data_ptr() + 4)) == -1 and call(realp=ctypes.c_void_p(0)) == -1
    assert lib.mg_note_acc_words(0) == 0 and lib.mg_note_acc_words(33) == 0 and lib.mg_note_acc_words(K) == 2 * K * 504
    assert lib.mg_note_acc_reset(None, K, st) == -1 and lib.mg_note_acc_reset(p(acc), 33, st) == -1
    torch.cuda.synchronize()
    for t, b in zip((acc, row_i, row_beats), before):
        assert torch.equal(t, b)                                          # nothing ran
