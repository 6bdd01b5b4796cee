"""Wall time of one training epoch of the emotion discriminator (device synchronise at the end), three data planes:
  host    train_ed.run_epoch: per batch two index_selects, two copies, a graph replay of step_rng and four torch reductions
  staged  train_ed.run_epoch_staged, augmentation and sampler off: one graph replay of step_staged per batch
  aug     the same with all three ED augmentations and the weighted sampler on
at the reference's size (n = 897, B = 64, T = 512, note_dim 4) and at the bench size (n = 4096, B = 64, T = 256, note_dim 128).
Per size: two warm-up epochs per variant (eager pass, capture), then `--repeats` timed epochs per variant, alternating.

    python tools/ed_epoch_bench.py [--repeats 3] [--sizes ref bench] [--variants host staged aug]

Under `rocprofv3 --kernel-trace --stats` with one variant and one size, the stage_augment_kernel row of the kernel statistics
is that variant's staging launch alone.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import ops  # noqa: E402
from melo_gan_amd.emotion_discriminator import train_ed  # noqa: E402
from melo_gan_amd.emotion_discriminator.engine import EdEngine  # noqa: E402
from melo_gan_amd.gan.config import default_ed_cfg  # noqa: E402

SIZES = {"ref": (897, 64, 512, 4), "bench": (4096, 64, 256, 128)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", nargs="+", default=["ref", "bench"], choices=sorted(SIZES))
    ap.add_argument("--variants", nargs="+", default=["host", "staged", "aug"], choices=["host", "staged", "aug"])
    args = ap.parse_args()
    for name in args.sizes:
        n, B, T, C = SIZES[name]
        cfg = dict(default_ed_cfg(C), dropout=0.2, optimizer=dict(name="AdamW", lr=2e-4, betas=[0.5, 0.999], weight_decay=0.0))
        x, y = train_ed.synthetic_split(n, T, C, 0, "cuda")
        aug = ops.augment_spec("ed", 42, noise_std=0.01, dropout_prob=0.05, pitch_shift_prob=0.3)
        cdf = ops.sampler_cdf(y)
        engines = {}
        for v in args.variants:
            engines[v] = e = EdEngine(cfg, "cuda", B, T)
            e.init_weights(0)
            if v != "host":
                e.attach_split(x, y, aug if v == "aug" else None)
        gen = torch.Generator().manual_seed(0)
        epoch = [0]

        def run(v):
            e = engines[v]
            with torch.cuda.stream(e.stream):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if v == "host":
                    train_ed.run_epoch(e, x, y, True, True, gen)
                else:
                    train_ed.run_epoch_staged(e, epoch[0], True, gen, cdf if v == "aug" else None)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

        for _ in range(2):
            for v in engines:
                run(v)
                epoch[0] += 1
        times = {v: [] for v in engines}
        for _ in range(args.repeats):
            for v in engines:
                times[v].append(run(v))
                epoch[0] += 1
        steps = -(-n // B)
        for v, ts in times.items():
            med = sorted(ts)[len(ts) // 2]
            print(f"{name:5s} n={n} B={B} T={T} C={C} {v:6s}: epoch ms {' '.join(f'{t:8.2f}' for t in ts)}  median {med:8.2f}"
                  f"  ({1e3 * med / steps:7.1f} us/step, {n / med * 1e3:9.0f} samples/s)", flush=True)


if __name__ == "__main__":
    main()
