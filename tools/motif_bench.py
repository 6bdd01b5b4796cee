"""What mg_motif_lcs costs at the size of the copy check (csrc/motif.hip, melo_gan_amd/motifs.py):

    python tools/motif_bench.py [--queries 256 --corpus 897 --tokens 511] [--seed 7] [--out profiles/motif_bench.txt]

  the tokens   seeded random-walk melodies (tests/motif_cases.py, walk_tokens): intervals N(0, 3) clipped to +-12 and six
               unevenly weighted rhythm classes, every row full.  Cell updates = queries x corpus x tokens^2.
  kernel       us per replay of a graph over mg_motif_lcs (the clear of reach, the pair kernel, the finish of reach): two warm
               replays, then device events around enough replays for at least half a second, three times; the median.
  torch        the same recurrence in plain torch on the same device, the yardstick: an int16 run table (queries, corpus,
               tokens), one position of the queries per step -- compare, shift, add, two maxima -- which gives every pair's
               longest run and reach, not the positions.  One warm pass, then device events around each of three passes.
               Both results are compared before anything is timed.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import ops  # noqa: E402
import motif_cases as MC  # noqa: E402


def torch_lcs(qt, ct):
    """(longest (Nq, Nc) int16, reach (Nq, T) int16) of full token rows qt (Nq, T), ct (Nc, T) int32 on the device."""
    Nq, T = qt.shape
    run = torch.zeros(Nq, ct.shape[0], T + 1, dtype=torch.int16, device=qt.device)      # run[.., j + 1] = run(i, j)
    best = torch.zeros(Nq, ct.shape[0], dtype=torch.int16, device=qt.device)
    reach = torch.zeros(Nq, T, dtype=torch.int16, device=qt.device)
    for i in range(T):
        new = torch.where(ct[None] == qt[:, i, None, None], run[:, :, :-1] + 1, 0)
        row = new.amax(dim=2)
        best = torch.maximum(best, row)
        reach[:, i] = row.amax(dim=1)
        run[:, :, 1:] = new
    return best, reach


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--corpus", type=int, default=897)
    ap.add_argument("--tokens", type=int, default=511)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", type=str, default=None, help="also write the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("motif_bench measures the device path: a MI355X (ROCm) device is required")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    Nq, Nc, m = args.queries, args.corpus, args.tokens
    T = m + 1
    g = np.random.default_rng(args.seed)
    tok = np.full((Nq + Nc, T), 0xFFFF, np.uint16)
    tok[:, :m] = MC.walk_tokens(g, Nq + Nc, m)
    d = torch.device("cuda")
    qt, ct = torch.from_numpy(tok[:Nq]).to(d), torch.from_numpy(tok[Nq:]).to(d)
    ql = torch.full((Nq,), m, dtype=torch.int32, device=d)
    cl = torch.full((Nc,), m, dtype=torch.int32, device=d)
    packed = torch.empty(Nq, Nc, dtype=torch.int64, device=d)
    reach = torch.empty(Nq, T, dtype=torch.int32, device=d)
    cells = float(Nq) * Nc * m * m
    say(f"{Nq} x {Nc} rows of {m} tokens (seed {args.seed}): {cells:.3g} cell updates, on {torch.cuda.get_device_name(0)}")

    launch = lambda: ops.motif_lcs(qt, ql, ct, cl, None, None, packed, reach)  # noqa: E731
    launch()
    torch.cuda.synchronize()
    tq, tc = qt[:, :m].to(torch.int32), ct[:, :m].to(torch.int32)
    best, t_reach = torch_lcs(tq, tc)
    torch.cuda.synchronize()
    same = bool(((packed >> 32) == best.to(torch.int64)).all()) and bool((reach[:, :m] == t_reach.to(torch.int32)).all())
    say(f"  longest chance run {int(best.max())} tokens, mean {float(best.float().mean()):.2f}; the kernel's lengths and reach "
        f"{'equal' if same else 'DIFFER FROM'} the torch formulation's")
    if not same:
        raise RuntimeError("motif_bench: the kernel and the torch formulation disagree")

    with torch.cuda.stream(torch.cuda.Stream()):
        gr = ops.Graph.capture(launch)
        gr.launch()
        gr.launch()
        torch.cuda.synchronize()
        e0, e1 = ops.Event(), ops.Event()
        e0.record(); gr.launch(); e1.record()
        torch.cuda.synchronize()
        reps = max(3, int(500.0 / max(e0.elapsed_ms(e1), 1e-3)) + 1)
        times = []
        for _ in range(3):
            e0, e1 = ops.Event(), ops.Event()
            e0.record()
            for _ in range(reps):
                gr.launch()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_ms(e1) / reps * 1e3)
    us = sorted(times)[1]
    say(f"  mg_motif_lcs      {' '.join(f'{t:10.1f}' for t in times)} us per replay, median {us:10.1f}   ({reps} replays per window): "
        f"{cells / us / 1e3:.1f} G cell updates/s")
    times = []
    for _ in range(3):
        e0, e1 = ops.Event(), ops.Event()
        e0.record()
        torch_lcs(tq, tc)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_ms(e1) * 1e3)
    tus = sorted(times)[1]
    say(f"  torch formulation {' '.join(f'{t:10.1f}' for t in times)} us per pass,   median {tus:10.1f}: "
        f"{cells / tus / 1e3:.1f} G cell updates/s ({tus / us:.1f} x the kernel's time)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
