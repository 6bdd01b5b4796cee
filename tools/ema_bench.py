"""What the generator's moving average (EMA_DECAY, csrc/ema.hip) costs, at cfg2 size (B = 64, T = 256, C = 128) and at the
reference shape (B = 32, T = 512, C = 4):

    python tools/ema_bench.py [--repeats 3] [--out profiles/ema_bench.txt]

  step         us per replayed g_step_rng graph (draw -> E_num -> G -> emotion branch -> critic -> backward -> Adam [-> mg_ema_flat])
               of an engine with EMA_DECAY 0 and of one with 0.999, alternating, device events around 60 x 16 replays; their
               difference is the rider's cost inside the step, where it sits in the single-stream tail behind the update
  call alone   us per mg_ema_flat call over the flat generator + encoder buffer, 200 calls replayed as one graph
  floor        the bytes the call must move (4 read + 8 read + 8 written = 20 n) over the 6.29 TB/s measured HBM copy rate
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import ops  # noqa: E402
from melo_gan_amd.gan.config import default_ed_cfg, default_gan_cfg  # noqa: E402
from melo_gan_amd.gan.engine import GanEngine  # noqa: E402
from _timeit import alternate, timeit  # noqa: E402

HBM_BYTES_PER_S = 6.29e12
PASSES = 60


def engine(B, T, C, decay):
    cfg, ed_cfg = default_gan_cfg(B, T, C), default_ed_cfg(C)
    cfg["EMA_DECAY"] = decay
    eng = GanEngine(cfg, ed_cfg, "cuda", B)
    eng.init_weights(42)
    g = torch.Generator().manual_seed(1)
    eng.set_batch((torch.rand(B, T, C, generator=g) * 2 - 1).cuda(), torch.randn(B, 6, generator=g).cuda(),
                  torch.zeros(B, cfg["LATENT_DIM"]).cuda(), torch.randint(0, 4, (B,), generator=g).cuda())
    eng.seed(42)
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", type=str, default=None, help="also write the lines to this file")
    args = ap.parse_args()
    med = lambda ts: sorted(ts)[len(ts) // 2]  # noqa: E731
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for tag, (B, T, C) in (("cfg2", (64, 256, 128)), ("reference", (32, 512, 4))):
        engs = {"EMA_DECAY 0": engine(B, T, C, 0.0), "EMA_DECAY 0.999": engine(B, T, C, 0.999)}
        graphs = {}
        for name, eng in engs.items():
            # every engine captures on its own stream; the replays below run on one stream, which a graph launch allows
            with torch.cuda.stream(eng.stream):
                eng.g_step_rng()                         # eager: every workspace exists from here on
                eng.GE.ticked = False
                graphs[name] = ops.Graph.capture(eng.g_step_rng)
                eng.GE.ticked = False
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            times = alternate(graphs, lambda: None, args.repeats, PASSES)
        n = engs["EMA_DECAY 0.999"].GE.n
        say(f"{tag}: B={B} T={T} C={C}, {n} generator + encoder parameters: replayed g_step_rng, us "
            f"({graphs['EMA_DECAY 0'].kernel_nodes} / {graphs['EMA_DECAY 0.999'].kernel_nodes} kernel nodes)")
        for name, ts in times.items():
            say(f"  {name:16s} {' '.join(f'{t:8.2f}' for t in ts)}   median {med(ts):8.2f}")
        diff = med(times["EMA_DECAY 0.999"]) - med(times["EMA_DECAY 0"])
        say(f"  difference (mg_ema_flat inside the step): {diff:.2f} us = {100 * diff / med(times['EMA_DECAY 0']):.2f} % of the step")
        eng = engs["EMA_DECAY 0.999"]
        alone = [timeit(lambda: ops.ema_flat(eng.GE.data, eng.ema, n, 0.999, True, eng.GE.state, 0.0), reps=200)
                 for _ in range(args.repeats)]
        floor = 20 * n / HBM_BYTES_PER_S * 1e6
        say(f"  mg_ema_flat alone {' '.join(f'{t:8.2f}' for t in alone)}   median {med(alone):8.2f}")
        say(f"  bytes moved {20 * n / 1e6:.2f} MB -> floor {floor:.2f} us at 6.29 TB/s; the call alone is {med(alone) / floor:.2f} x its "
            f"floor = {20 * n / med(alone) / 1e6:.2f} TB/s")
        del engs, graphs
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
