"""The pairwise feature-space kernels (csrc/pair_metrics.hip) at D = 256, N = M in {192, 4096, 16384}:

    python tools/pair_bench.py [--repeats 5] [--sizes 192 4096 16384]

  mg_pair_*    us per call (norms + tile kernel + fold), `reps` calls replayed as one graph, median of --repeats; for the
               tile kernel's share, the algorithmic 2 N M D FLOP over the time against the 157 TFLOP/s fp32 matrix peak
  torch        the same result composed from torch device ops on the same arrays -- mm + the cube + an fp64 sum; cdist^2 + topk;
               cdist^2 - r2 + min -- eager, device events around the repetitions.  These materialise the N x M matrix (and an
               fp64 copy for the sum): sizes whose intermediates do not fit are reported as "does not fit".  A yardstick, not
               the code under test, and not the same arithmetic (torch's GEMM is free to reorder and to use other precision).
then the evaluator's rows/s over a whole pass with and without features=True at the shipped config's shape (wall clock of
evaluate(), which ends in the device -> host reads).  Rows are random normal features: the time does not depend on the data.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import ops  # noqa: E402
from melo_gan_amd.gan import evaluate as EV  # noqa: E402
from melo_gan_amd.gan.config import default_ed_cfg, default_gan_cfg  # noqa: E402
from melo_gan_amd.gan.dataset import GANDataset  # noqa: E402
from _timeit import timeit  # noqa: E402

D, K_NN = 256, 3
PEAK_F32_MATRIX = 157.3e12
TORCH_BUDGET = 8 << 30          # bytes of N x M intermediates the torch composition may allocate


def events_us(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[192, 4096, 16384])
    args = ap.parse_args()
    med = lambda ts: sorted(ts)[len(ts) // 2]  # noqa: E731
    row = lambda name, ts, extra="": print(f"  {name:28s} {' '.join(f'{t:10.2f}' for t in ts)}   median {med(ts):10.2f}{extra}",  # noqa: E731
                                           flush=True)
    g = torch.Generator(device="cuda").manual_seed(1)
    for n in args.sizes:
        A, B = torch.randn(n, D, device="cuda", generator=g), torch.randn(n, D, device="cuda", generator=g)
        r2 = torch.rand(n, device="cuda", generator=g) * D
        ks, nn, mg = torch.zeros(1, dtype=torch.float64, device="cuda"), torch.empty(n, K_NN, device="cuda"), torch.empty(n, device="cuda")
        reps = 200 if n <= 256 else (20 if n <= 4096 else 4)
        flop = 2.0 * n * n * D
        print(f"N = M = {n}, D = {D}: us per call ({reps} calls per replayed graph)", flush=True)
        one = torch.empty(n, 1, device="cuda")
        for name, fn in (("mg_pair_ksum", lambda: ops.pair_ksum(A, B, ks)), (f"mg_pair_knn k={K_NN}", lambda: ops.pair_knn(A, B, nn)),
                         ("mg_pair_knn k=1", lambda: ops.pair_knn(A, B, one)), ("mg_pair_margin", lambda: ops.pair_margin(A, B, r2, mg))):
            ts = [timeit(fn, reps=reps) for _ in range(args.repeats)]
            row(name, ts, f"   {flop / (med(ts) * 1e-6) / 1e12:6.1f} TFLOP/s = {100 * flop / (med(ts) * 1e-6) / PEAK_F32_MATRIX:4.1f} % of the fp32 matrix peak")
        need = n * n * (4 + 8)
        if need > TORCH_BUDGET:
            print(f"  torch device ops: the N x M intermediates ({need / 2 ** 30:.1f} GiB) do not fit the {TORCH_BUDGET >> 30} GiB budget", flush=True)
            continue
        treps = max(2, reps // 2)
        row("torch mm + cube + fp64 sum", [events_us(lambda: ((A @ B.T).double() / D + 1.0).pow(3).sum(), treps) for _ in range(args.repeats)])
        row(f"torch cdist^2 + topk {K_NN}", [events_us(lambda: torch.topk(torch.cdist(A, B).square_(), K_NN, dim=1, largest=False), treps)
                                             for _ in range(args.repeats)])
        row("torch cdist^2 - r2 + min", [events_us(lambda: (torch.cdist(A, B).square_() - r2[None, :]).amin(1), treps)
                                         for _ in range(args.repeats)])
    # the evaluator with and without the feature metrics
    Bsz, T, C = 64, 512, 4
    cfg, ed_cfg = default_gan_cfg(Bsz, T, C), default_ed_cfg(C)
    n = 192
    ds = GANDataset.synthetic(n, T, C, cfg["LATENT_DIM"], 1, "cuda")
    for features in (False, True):
        ev = EV.Evaluator(cfg, ed_cfg, "cuda", Bsz, features=features)
        ev.has_d = True
        ev.evaluate(ds, 1)                               # builds the graph
        ws = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.evaluate(ds, 1)
            ws.append(time.perf_counter() - t0)
        print(f"evaluate(features={features}): {n} rows (B={Bsz} T={T} C={C}) in {med(ws) * 1e3:.3f} ms (median of {args.repeats}) = "
              f"{n / med(ws):,.0f} rows/s", flush=True)


if __name__ == "__main__":
    main()
