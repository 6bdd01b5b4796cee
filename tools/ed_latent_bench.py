"""The latent-mode emotion classifier's training step (EdLatentEngine.step_rng: mask draw, forward, cross-entropy, backward,
AdamW) as replayed hipGraphs, the fused two-launch engine against the per-layer comparator (fused=False) in the same process,
alternating, `--repeats` times each; then each fused launch on its own with its share of the larger of its FLOP and byte
bounds; then the wall time of one staged epoch at the reference's split size.

    python tools/ed_latent_bench.py [--repeats 3] [--epoch-n 897]

Sizes: B = 64, mlp_hidden [256, 128], latent_dim 64 and 8.  Bounds: FLOPs and bytes are computed from the shapes --
  A  2 B sum(in out) forward + 2 B sum over layers >= 1 of (in out) data gradient; every 16-row block streams the weights once
     per direction from L2, the activations z / a / dz / mask are written once and z / mask read back once
  B  2 B sum(in out) (+ bias sums); p / m / v read and written, g written, dz and the layer inputs read once per tile column / row
against 157.3 TFLOP/s (fp32 matrix pipe) and 8 TB/s (HBM3E); at these sizes both bounds are far below a microsecond, so the
share says how far a launch-latency-bound step is from either roof.  Under `rocprofv3 --kernel-trace --stats` the rows
mlp_rows_kernel and mlp_params_kernel of the kernel statistics are the two launches alone (add --profile: no comparator).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd.emotion_discriminator import train_ed  # noqa: E402
from melo_gan_amd.emotion_discriminator.latent_engine import EdLatentEngine  # noqa: E402
from melo_gan_amd.gan.config import default_ed_cfg  # noqa: E402
from _timeit import timeit  # noqa: E402

PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8.0e12
HIDDEN = [256, 128]


def cfg_for(D, B):
    return dict(default_ed_cfg(4), input_mode="latent", latent_dim=D, mlp_hidden=HIDDEN, dropout=0.2, batch_size=B,
                optimizer=dict(name="AdamW", lr=2e-4, betas=[0.5, 0.999], weight_decay=0.0))


def bounds(D, B, n_classes=4):
    dims = [D] + HIDDEN + [n_classes]
    mats = [i * o for i, o in zip(dims, dims[1:])]
    n_par = sum(mats) + sum(dims[1:])
    blocks = -(-B // 16)
    fl_a = 2 * B * sum(mats) + 2 * B * sum(mats[1:])
    by_a = 4 * (blocks * (sum(mats) + sum(mats[1:]) + sum(dims[1:])) + B * D + B * sum(HIDDEN) * 6 + 3 * B * n_classes)
    fl_b = 2 * B * (sum(mats) + sum(dims[1:]))
    tiles_o, tiles_i = [-(-o // 16) for o in dims[1:]], [-(-i // 16) for i in dims[:-1]]
    by_b = 4 * (7 * n_par + B * sum(16 * to * ti * 2 for to, ti in zip(tiles_o, tiles_i)))
    return dict(A=(fl_a, by_a), B=(fl_b, by_b))


def report(tag, us, fl, by):
    t_fl, t_by = fl / PEAK_FLOPS * 1e6, by / PEAK_BYTES * 1e6
    which = "FLOP" if t_fl >= t_by else "byte"
    print(f"  {tag}: {us:7.2f} us   {fl / 1e6:7.2f} MFLOP ({t_fl:6.3f} us)  {by / 1e3:8.1f} KB ({t_by:6.3f} us)   "
          f"{which} bound, share {100 * max(t_fl, t_by) / us:5.2f} %", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--epoch-n", type=int, default=897)
    ap.add_argument("--profile", action="store_true", help="fused engine only, 200 eager steps per size (for rocprofv3)")
    args = ap.parse_args()
    B = 64
    for D in (64, 8):
        engs = {}
        for name, fused in (("fused", True), ("layers", False)):
            if args.profile and not fused:
                continue
            engs[name] = e = EdLatentEngine(cfg_for(D, B), "cuda", B, fused=fused)
            e.init_weights(0)
            x, y = train_ed.synthetic_latent_split(B, D, 0, "cuda")
            e.set_batch(x, y)
        if args.profile:
            e = engs["fused"]
            with torch.cuda.stream(e.stream):
                for _ in range(200):
                    e.step_rng()
                torch.cuda.synchronize()
            print(f"latent_dim {D}: 200 eager fused steps done", flush=True)
            continue
        times = {k: [] for k in engs}
        for _ in range(args.repeats):
            for k, e in engs.items():
                times[k].append(timeit(e.step_rng))
        print(f"B={B} latent_dim={D} mlp_hidden={HIDDEN}: training step, graph replay, us per step", flush=True)
        for k, ts in times.items():
            print(f"  {k:7s} {' '.join(f'{t:7.2f}' for t in ts)}   median {sorted(ts)[len(ts) // 2]:7.2f}", flush=True)
        wins = sum(f <= c for f, c in zip(times["fused"], times["layers"]))
        print(f"  fused no slower than the comparator in {wins} of {args.repeats} alternations", flush=True)
        e, bd = engs["fused"], bounds(D, B)
        report("A mlp_cls_fwd_bwd (draw, tick)   ", timeit(lambda: e._launch_a(True, True, True)), *bd["A"])
        report("B mlp_cls_wgrad_update (apply)   ", timeit(lambda: e._launch_b(True)), *bd["B"])
        # one staged epoch at the reference's split size: wall time, device synchronised at the end
        n = args.epoch_n
        xs, ys = train_ed.synthetic_latent_split(n, D, 1, "cuda")
        gen = torch.Generator().manual_seed(0)
        for k in engs:
            ee = EdLatentEngine(cfg_for(D, B), "cuda", B, fused=(k == "fused"))
            ee.init_weights(0)
            ee.attach_split(xs, ys)
            ts = []
            with torch.cuda.stream(ee.stream):
                for ep in range(2 + args.repeats):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    train_ed.run_epoch_staged(ee, ep, True, gen)
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
            ts = ts[2:]          # eager pass, capture
            print(f"  staged epoch n={n} {k:7s}: ms {' '.join(f'{t:7.3f}' for t in ts)}  median {sorted(ts)[len(ts) // 2]:7.3f}"
                  f"  ({1e3 * sorted(ts)[len(ts) // 2] / -(-n // B):6.1f} us/step)", flush=True)


if __name__ == "__main__":
    main()
