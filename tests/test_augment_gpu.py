"""mg_stage_augment, mg_weighted_order and mg_ed_metrics_acc on the MI355X.

Every destination starts as NaN, every seed is fixed.  Statistical bounds are 5 standard errors derived from the sample size
in the test: 5/sqrt(N) for a mean of unit draws, 5/sqrt(2N) for their standard deviation, 5*sqrt(p(1-p)/N) for a share.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# (note_dim, T, samples): >= 1.1e5 time rows each; T = 1100 and T * 32 = 1184 are no multiples of the block's 1024 pieces
ROW_CASES = [(4, 512, 256), (4, 1100, 128), (128, 512, 256), (128, 37, 3072)]
# per-sample gates: >= 2e3 samples
GATE_CASES = [(4, 512, 2048), (128, 37, 2048)]


@pytest.fixture(scope="module")
def ops():
    import melo_gan_amd  # noqa: F401
    from melo_gan_amd import ops as _ops
    return _ops


def share_bound(p, n):
    return 5.0 * math.sqrt(p * (1.0 - p) / n)


def i64(v):
    return torch.tensor([v], dtype=torch.int64, device="cuda")


def bits(t):
    return t.contiguous().view(torch.int32)


def source(n, T, C, seed, nonzero=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand(n, T, C, generator=g, device="cuda") * 2 - 1
    if nonzero:          # |x| >= 0.1: a zero in the output is then the kernel's doing
        x = torch.where(x >= 0, x * 0.9 + 0.1, x * 0.9 - 0.1)
    return x.contiguous()


def stage(ops, x, aug, y=None, order=None, n_rows=None, batch=0, serial0=0, last=False, order_len=None):
    """One launch into NaN-poisoned destinations."""
    n_rows = x.shape[0] if n_rows is None else n_rows
    out = torch.full((n_rows,) + tuple(x.shape[1:]), float("nan"), device="cuda")
    yo = None if y is None else torch.full((n_rows,), -7, dtype=torch.int64, device="cuda")
    order_len = (x.shape[0] if order is None else order.numel()) if order_len is None else order_len
    ops.stage_augment(x, y, out, yo, n_rows, order, order_len, i64(batch + 3), i64(3), i64(serial0), aug, last=last)
    torch.cuda.synchronize()
    return out, yo


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("program", ["ed", "ae"])
@pytest.mark.parametrize("C,T", [(4, 512), (4, 1100), (128, 512), (128, 37)])
def test_everything_off_is_the_cursor_copy_bit_for_bit(ops, program, C, T):
    n, B = 29, 8
    x = source(n, T, C, 1)
    x[0, 0, 0], x[1, 1, 1] = -0.0, float("inf")
    y = torch.arange(n, dtype=torch.int64, device="cuda") % 4
    order = torch.randperm(n, generator=torch.Generator().manual_seed(2)).cuda()
    aug = ops.augment_spec(program, 5)
    for batch in (0, 2, 3):          # batch 3 wraps round the end of the order, like the cursor it restates
        out, yo = stage(ops, x, aug, y, order, B, batch)
        ref, yref = torch.full_like(out, float("nan")), torch.full_like(yo, -7)
        ops.stage_rows_cursor([(x, ref), (y, yref)], B, order, n, i64(batch + 3), i64(3))
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(ref)) and torch.equal(yo, yref), batch
    rows = 5                          # the tail rule: the fixed last `rows` positions, whatever the counter says
    out, yo = stage(ops, x, aug, y, order, rows, batch=17, last=True)
    assert torch.equal(bits(out), bits(x.index_select(0, order[-rows:]))) and torch.equal(yo, y.index_select(0, order[-rows:]))
    out, _ = stage(ops, x, aug, None, None, B, 1)                     # no labels, no order: the identity
    assert torch.equal(bits(out), bits(x[B:2 * B]))


@pytest.mark.parametrize("C,T,n", GATE_CASES)
def test_ed_pitch_shift(ops, C, T, n):
    x = source(n, T, C, 3)
    out, _ = stage(ops, x, ops.augment_spec("ed", 11, pitch_shift_prob=1.0))
    up, down = out[:, :, 0] == x[:, :, 0] + 1.0, out[:, :, 0] == x[:, :, 0] - 1.0
    s_up, s_down = up.all(dim=1), down.all(dim=1)
    assert bool((s_up ^ s_down).all())                                     # exactly x + 1 or x - 1 in fp32, one sign per sample
    assert torch.equal(bits(out[:, :, 1:]), bits(x[:, :, 1:]))
    share = s_up.float().mean().item()
    print(f"share of +1: {share:.4f} (bound {share_bound(0.5, n):.4f})")
    assert abs(share - 0.5) <= share_bound(0.5, n)
    out, _ = stage(ops, x, ops.augment_spec("ed", 12, pitch_shift_prob=0.3))
    same = (bits(out) == bits(x)).flatten(1).all(dim=1)
    moved = ((out[:, :, 0] == x[:, :, 0] + 1.0) | (out[:, :, 0] == x[:, :, 0] - 1.0)).all(dim=1) & ~same
    assert bool((same ^ moved).all()) and torch.equal(bits(out[:, :, 1:]), bits(x[:, :, 1:]))
    share = moved.float().mean().item()
    print(f"share of shifted samples: {share:.4f} (bound {share_bound(0.3, n):.4f})")
    assert abs(share - 0.3) <= share_bound(0.3, n)


@pytest.mark.parametrize("C,T,n", ROW_CASES)
def test_ed_row_dropout(ops, C, T, n):
    p = 0.25
    x = source(n, T, C, 4, nonzero=True)
    out, _ = stage(ops, x, ops.augment_spec("ed", 13, dropout_prob=p))
    kept = (bits(out) == bits(x)).all(dim=2)
    zero = (bits(out) == 0).all(dim=2)                                      # +0.0 in ALL columns, also beyond column 3
    assert bool((kept ^ zero).all())
    N = n * T
    share = zero.float().mean().item()
    print(f"dropped share {share:.5f} (p {p}, bound {share_bound(p, N):.5f})")
    assert abs(share - p) <= share_bound(p, N)


@pytest.mark.parametrize("C,T,n", ROW_CASES)
def test_ed_noise_on_a_zero_source(ops, C, T, n):
    std = 0.5                       # a power of two: out / std is exact
    x = torch.zeros(n, T, C, device="cuda")
    out, _ = stage(ops, x, ops.augment_spec("ed", 14, noise_std=std))
    assert bool((out[:, :, 0] == 0).all()) and bool((out[:, :, 4:] == 0).all())
    z = (out[:, :, 1:4] / std).double().reshape(-1, 3)
    N = z.shape[0]
    for c in range(3):
        m, s = z[:, c].mean().item(), z[:, c].std().item()
        print(f"column {c + 1}: mean {m:+.5f} (bound {5 / math.sqrt(N):.5f}) std {s:.5f} (bound 1 +- {5 / math.sqrt(2 * N):.5f})")
        assert abs(m) <= 5 / math.sqrt(N) and abs(s - 1.0) <= 5 / math.sqrt(2 * N)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        r = torch.corrcoef(z[:, [a, b]].T)[0, 1].item()
        print(f"corr({a + 1},{b + 1}) = {r:+.5f} (bound {5 / math.sqrt(N):.5f})")
        assert abs(r) <= 5 / math.sqrt(N)
    for b in range(0, n, max(1, n // 8)):          # no two time rows of a sample share their draws
        assert torch.unique(out[b, :, 1:4], dim=0).shape[0] == T, b
    assert not torch.equal(out[0], out[1])


@pytest.mark.parametrize("C,T,n", ROW_CASES[::2])
def test_ed_all_three_on_a_zero_source(ops, C, T, n):
    """The reference's order: noise, dropout, then the shift -- so a dropped row ends as (+-1, 0, 0, ...)."""
    p = 0.2
    x = torch.zeros(n, T, C, device="cuda")
    out, _ = stage(ops, x, ops.augment_spec("ed", 15, noise_std=0.5, dropout_prob=p, pitch_shift_prob=1.0))
    assert bool((out[:, :, 0].abs() == 1.0).all())
    assert bool((out[:, :, 0] == out[:, :1, 0]).all())                      # one sign per sample, dropped rows included
    assert bool((out[:, :, 4:] == 0).all())
    dropped = (out[:, :, 1:4] == 0).all(dim=2)       # a live row with three exact zeros: (2^-24)^3
    share = dropped.float().mean().item()
    print(f"rows that ended as (+-1, 0, 0, ...): {share:.5f} (p {p}, bound {share_bound(p, n * T):.5f})")
    assert abs(share - p) <= share_bound(p, n * T)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,T,n", GATE_CASES)
def test_ae_tempo_and_pitch_gates(ops, C, T, n):
    x = source(n, T, C, 6, nonzero=True)
    x[:, :, 0] = torch.randint(0, 128, (n, T), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) / 64.0 - 1.0
    j = 0.125
    out, _ = stage(ops, x, ops.augment_spec("ae", 21, tempo_jitter=j))
    assert torch.equal(bits(out[:, :, 0]), bits(x[:, :, 0])) and torch.equal(bits(out[:, :, 3:]), bits(x[:, :, 3:]))
    f1, f2 = (out[:, :, 1] / x[:, :, 1]).double(), (out[:, :, 2] / x[:, :, 2]).double()
    f = f1[:, 0]
    assert bool(((f1 - f[:, None]).abs() <= 4e-7).all()) and bool(((f2 - f[:, None]).abs() <= 4e-7).all())     # one factor per sample
    assert bool((f >= 1 - j - 4e-7).all()) and bool((f <= 1 + j + 4e-7).all())
    scaled = (bits(out[:, :, 1:3]) != bits(x[:, :, 1:3])).flatten(1).any(dim=1)
    share = scaled.float().mean().item()
    print(f"tempo gate {share:.4f} (bound {share_bound(0.3, n):.4f}); factors {f[scaled].min().item():.4f}..{f[scaled].max().item():.4f}")
    assert abs(share - 0.3) <= share_bound(0.3, n)
    u = ((f[scaled] - 1) / j)                                                 # U(-1, 1): mean 0, variance 1/3
    assert abs(u.mean().item()) <= 5 * math.sqrt(1 / 3 / u.numel()) and u.min().item() < -0.8 and u.max().item() > 0.8
    ps = 2
    out, _ = stage(ops, x, ops.augment_spec("ae", 22, pitch_shift=ps))
    assert torch.equal(bits(out[:, :, 1:]), bits(x[:, :, 1:]))
    d = out[:, :, 0] - x[:, :, 0]                                             # exact: column 0 holds multiples of 1/64
    assert bool((d == d[:, :1]).all()) and bool((d == d.round()).all()) and float(d.abs().max()) == ps
    d = d[:, 0]
    for k in range(-ps, ps + 1):              # gate 0.3, then uniform over the 2p + 1 values, 0 among them
        pk = 0.3 / (2 * ps + 1) + (0.7 if k == 0 else 0.0)
        share = (d == k).float().mean().item()
        print(f"shift {k:+d}: {share:.4f} (expected {pk:.4f}, bound {share_bound(pk, n):.4f})")
        assert abs(share - pk) <= share_bound(pk, n)


@pytest.mark.parametrize("C,T,n", GATE_CASES)
def test_ae_dropout_velocity_and_timing_gates(ops, C, T, n):
    x = source(n, T, C, 7, nonzero=True)
    p = 0.25
    out, _ = stage(ops, x, ops.augment_spec("ae", 23, note_dropout=p))
    kept, zero = (bits(out) == bits(x)).all(dim=2), (bits(out) == 0).all(dim=2)
    assert bool((kept ^ zero).all())
    gated = zero.any(dim=1)                   # a gated sample with no dropped row at all: 0.75^37 = 2e-5 of them
    share = gated.float().mean().item()
    print(f"dropout gate {share:.4f} (bound {share_bound(0.2, n):.4f})")
    assert abs(share - 0.2) <= share_bound(0.2, n)
    rows = zero[gated].float()
    print(f"dropped share inside gated samples {rows.mean().item():.5f} (bound {share_bound(p, rows.numel()):.5f})")
    assert abs(rows.mean().item() - p) <= share_bound(p, rows.numel())

    sig = 0.5
    x0 = torch.zeros_like(x)
    out, _ = stage(ops, x0, ops.augment_spec("ae", 24, velocity_jitter=sig))
    assert bool((out[:, :, :3] == 0).all()) and bool((out[:, :, 4:] == 0).all())
    gated = (out[:, :, 3] != 0).any(dim=1)
    share = gated.float().mean().item()
    z = (out[gated][:, :, 3] / sig).double().flatten()
    print(f"velocity gate {share:.4f} (bound {share_bound(0.3, n):.4f}); mean {z.mean().item():+.5f} std {z.std().item():.5f} over {z.numel()}")
    assert abs(share - 0.3) <= share_bound(0.3, n)
    assert abs(z.mean().item()) <= 5 / math.sqrt(z.numel()) and abs(z.std().item() - 1) <= 5 / math.sqrt(2 * z.numel())

    x1 = x.clone()
    x1[:, :, 1] = 0.25
    out, _ = stage(ops, x1, ops.augment_spec("ae", 25, timing_jitter=sig))
    assert torch.equal(bits(out[:, :, 0]), bits(x1[:, :, 0])) and torch.equal(bits(out[:, :, 2:]), bits(x1[:, :, 2:]))
    assert bool((out[:, :, 1] >= 0).all())                                   # clipped at 0 (ae/dataset.py:39)
    gated = (out[:, :, 1] != 0.25).any(dim=1)
    share = gated.float().mean().item()
    clipped = (out[gated][:, :, 1] == 0).float().mean().item()               # P(0.25 + 0.5 N < 0) = Phi(-0.5) = 0.3085
    rows_g = int(gated.sum()) * T
    print(f"timing gate {share:.4f} (bound {share_bound(0.2, n):.4f}); clipped {clipped:.4f} (bound {share_bound(0.3085, rows_g):.4f})")
    assert abs(share - 0.2) <= share_bound(0.2, n)
    assert abs(clipped - 0.30854) <= share_bound(0.30854, rows_g)

    # the last two gates also land on rows the dropout zeroed (the reference drops first, then jitters)
    out, _ = stage(ops, x, ops.augment_spec("ae", 26, note_dropout=p, velocity_jitter=sig))
    dropped = (out[:, :, :3] == 0).all(dim=2)
    jittered = (bits(out[:, :, 3]) != bits(x[:, :, 3])) & ~dropped
    both = dropped.any(dim=1) & jittered.any(dim=1)
    assert int(both.sum()) >= 0.06 * n - 5 * math.sqrt(0.06 * 0.94 * n)       # 0.2 * 0.3 of the samples pass both gates
    assert (out[both][:, :, 3][dropped[both]] != 0).float().mean().item() > 0.999      # a draw is exactly 0 once in 2^24
    only_drop = dropped.any(dim=1) & ~jittered.any(dim=1)
    assert bool((out[only_drop][:, :, 3][dropped[only_drop]] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("program,params", [("ed", dict(noise_std=0.05, dropout_prob=0.1, pitch_shift_prob=0.5)),
                                            ("ae", dict(tempo_jitter=0.07, pitch_shift=1, note_dropout=0.1, velocity_jitter=0.1,
                                                        timing_jitter=0.02))])
@pytest.mark.parametrize("C,T", [(4, 512), (128, 37)])
def test_draws_are_keyed_by_seed_serial_and_time_row_only(ops, program, params, C, T):
    n = 64
    x = source(n, T, C, 8, nonzero=True)
    aug = ops.augment_spec(program, 31, **params)
    full, _ = stage(ops, x, aug, serial0=1000)                                    # sample r <-> serial 1000 + r, place r of 64
    assert not torch.equal(bits(full), bits(x))
    part, _ = stage(ops, x, aug, n_rows=16, batch=2, serial0=1000)                # places 0..15 of 16 <-> serials 1032..1047
    assert torch.equal(bits(part), bits(full[32:48]))
    one, _ = stage(ops, x, aug, n_rows=1, batch=37, serial0=1000)
    assert torch.equal(bits(one), bits(full[37:38]))
    tail, _ = stage(ops, x, aug, n_rows=7, last=True, serial0=1000)
    assert torch.equal(bits(tail), bits(full[57:]))
    rolled = ((torch.arange(n) + 5) % n).cuda()                                   # sample r + 5 at position r: serial base 1005
    other, _ = stage(ops, x, aug, order=rolled, n_rows=16, batch=0, serial0=1005)
    assert torch.equal(bits(other), bits(full[5:21]))
    nxt, _ = stage(ops, x, aug, serial0=1000 + n)                                 # the next epoch's serials
    seed2, _ = stage(ops, x, ops.augment_spec(program, 32, **params), serial0=1000)
    assert not torch.equal(bits(nxt), bits(full)) and not torch.equal(bits(seed2), bits(full))
    differ = lambda a, b: (bits(a) != bits(b)).flatten(1).any(dim=1).float().mean().item()      # noqa: E731
    assert differ(nxt, full) > 0.3 and differ(seed2, full) > 0.3

    # captured: each replay stages the batch the counter then names, with the bytes of the eager launch
    counter, base, serial0 = i64(10), i64(10), i64(1000)
    out = torch.full((16, T, C), float("nan"), device="cuda")
    y = (torch.arange(n, device="cuda") % 4).to(torch.int64)
    yo = torch.full((16,), -7, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        g = ops.Graph()
        g.begin()
        try:
            ops.stage_augment(x, y, out, yo, 16, None, n, counter, base, serial0, aug)
        finally:
            g.end()
        got = []
        for _ in range(2):
            g.launch()
            got.append((out.clone(), yo.clone()))
            counter += 1
            out.fill_(float("nan"))
        stream.synchronize()
        g.release()
    torch.cuda.synchronize()
    for k, (o, lab) in enumerate(got):
        assert torch.equal(bits(o), bits(full[16 * k:16 * k + 16])) and torch.equal(lab, y[16 * k:16 * k + 16]), k
    assert not torch.equal(bits(got[0][0]), bits(got[1][0]))


# ---------------------------------------------------------------------------------------------------------------------------
def test_weighted_order_balances_the_reference_split(ops):
    sizes = [260, 228, 213, 196]
    n = sum(sizes)
    labels = torch.cat([torch.full((k,), c, dtype=torch.int64) for c, k in enumerate(sizes)])
    labels = labels[torch.randperm(n, generator=torch.Generator().manual_seed(0))].cuda()
    cdf = ops.sampler_cdf(labels)
    epochs = 400                               # per row: M p = 400 * 897 / (4 * 260) = 345 draws expected at the least
    counts = torch.zeros(n, dtype=torch.int64, device="cuda")
    orders = []
    for e in range(epochs):
        order = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        ops.weighted_order(cdf, order, 42, e)
        assert int(order.min()) >= 0 and int(order.max()) < n
        counts += torch.bincount(order, minlength=n)
        if e < 3:
            orders.append(order.clone())
    M = epochs * n
    again = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    ops.weighted_order(cdf, again, 42, 1)
    assert torch.equal(again, orders[1]) and not torch.equal(orders[0], orders[1]) and not torch.equal(orders[1], orders[2])
    ops.weighted_order(cdf, again, 43, 1)
    assert not torch.equal(again, orders[1])
    worst = 0.0
    for c, k in enumerate(sizes):
        share = counts[labels == c].sum().item() / M
        print(f"class {c}: share {share:.5f} (bound {share_bound(0.25, M):.5f})")
        assert abs(share - 0.25) <= share_bound(0.25, M)
        p = 0.25 / k
        assert M * p >= 100
        dev = (counts[labels == c].double() - M * p).abs().max().item() / math.sqrt(M * p * (1 - p))
        worst = max(worst, dev)
        assert dev <= 5.0, (c, dev)
    print(f"largest per-row deviation: {worst:.2f} standard errors")


def test_weighted_order_edge_cases(ops):
    labels = torch.tensor([0] * 50 + [1] + [2] * 49, dtype=torch.int64).cuda()        # a one-row class gets a third of the draws
    cdf = ops.sampler_cdf(labels)
    order = torch.full((30000,), -1, dtype=torch.int64, device="cuda")
    ops.weighted_order(cdf, order, 1, 0)
    share = (order == 50).float().mean().item()
    assert int(order.min()) >= 0 and int(order.max()) < 100
    assert abs(share - 1 / 3) <= share_bound(1 / 3, 30000), share
    one = torch.full((17,), -1, dtype=torch.int64, device="cuda")
    ops.weighted_order(ops.sampler_cdf(torch.zeros(1, dtype=torch.int64).cuda()), one, 1, 0)       # n = 1
    assert bool((one == 0).all())


def test_metrics_accumulate_like_the_torch_lines_they_replace(ops):
    g = torch.Generator().manual_seed(9)
    acc, ref = torch.zeros(2, device="cuda"), torch.zeros(2, device="cuda")
    for step, rows in enumerate([64, 64, 64, 7, 64, 33, 1, 64]):
        logits = torch.randn(64, 4, generator=g).cuda()
        logits[::5, 2] = logits[::5, 0] = logits[::5].max(dim=1).values + 1.0     # planted ties: the first index wins
        logits[3, 1] = logits[3, 3] = 9.0
        if step == 2:
            logits[1, 2] = float("nan")                                          # torch.argmax: NaN is the maximum
        y = torch.randint(0, 4, (64,), generator=g).cuda()
        y[::10] = 0
        loss = (torch.rand(1, generator=g) * 1.7 + 0.013).cuda()
        ops.ed_metrics_acc(logits, y, loss, rows, acc)
        ref[0:1] += loss * rows
        ref[1:2] += (logits[:rows].argmax(dim=1) == y[:rows]).float().sum()
        assert torch.equal(acc, ref), (step, acc.tolist(), ref.tolist())
    assert ref[1].item() > 50
