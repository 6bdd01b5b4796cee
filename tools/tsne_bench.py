"""Exact t-SNE on the device (csrc/tsne.hip) at D = 64, N in {192, 898, 4096, 16384} -- the validation split, the training
split, and generated sets of thousands of rows:

    python tools/tsne_bench.py [--repeats 5] [--sizes 192 898 4096 16384] [--out profiles/tsne_bench.txt]

  iteration      us per descent iteration (mg_tsne_step: forces + fold/update), `reps` iterations replayed as one graph, median
                 of --repeats; the same with the trace instantiation (fp64 logarithm per pair) on every iteration
  floor          N^2 x 4 bytes (one read of P per iteration) over the 6.29 TB/s measured HBM copy rate of the MI355X
  affinities     ms per mg_tsne_affinities call (norms, d2 tiles, per-row search, symmetric sum), device events, median
  fit            wall clock of Tsne().fit_transform at the defaults (1000 iterations, PCA on the host included), once per size
Rows are random normal features: the iteration's time does not depend on the data, the search's hardly.  The report is
printed and written to --out.
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
from melo_gan_amd.gan.tsne import Tsne  # noqa: E402
from _timeit import timeit  # noqa: E402

D, PERPLEXITY = 64, 30.0
HBM_BYTES_PER_S = 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[192, 898, 4096, 16384])
    ap.add_argument("--out", type=str, default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                            "profiles", "tsne_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tsne_bench measures on the GPU only")
    med = lambda ts: sorted(ts)[len(ts) // 2]  # noqa: E731
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/tsne_bench.py -- exact t-SNE on the device, D = {D}, perplexity {PERPLEXITY:g}; {torch.cuda.get_device_name(0)}")
    say(f"median of {args.repeats} repeats; the repeats are listed in front of it")
    g = torch.Generator(device="cuda").manual_seed(1)
    for n in args.sizes:
        X = torch.randn(n, D, device="cuda", generator=g)
        P = torch.empty(n, n, device="cuda")
        work = ops.tsne_workspace(n, "cuda")
        # the affinities
        ops.tsne_affinities(X, PERPLEXITY, P=P, work=work)
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.tsne_affinities(X, PERPLEXITY, P=P, work=work)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        floor_us = n * n * 4 / HBM_BYTES_PER_S * 1e6
        say(f"N = {n}: P is {n * n * 4 / 2 ** 20:.1f} MiB; floor of one read of P {floor_us:.2f} us")
        say(f"  affinities, ms per call      {' '.join(f'{t:9.3f}' for t in ts)}   median {med(ts):9.3f}")
        # the iteration
        Y = torch.randn(n, 2, device="cuda", generator=g) * 1e-4
        up, gn = torch.zeros_like(Y), torch.ones_like(Y)
        tr = torch.zeros(1, 4, dtype=torch.float64, device="cuda")
        lr = max(n / 12.0 / 4.0, 50.0)
        reps = 200 if n <= 1024 else (50 if n <= 4096 else 10)
        for name, trace in (("iteration", None), ("iteration with trace", tr)):
            fn = lambda: ops.tsne_step(P, Y, up, gn, 12.0, 0.5, lr, trace=trace, work=work)  # noqa: E731
            ts = [timeit(fn, reps=reps) for _ in range(args.repeats)]
            say(f"  {name + ', us':28s} {' '.join(f'{t:9.2f}' for t in ts)}   median {med(ts):9.2f}   = {med(ts) / floor_us:6.1f} x the floor"
                f"   ({reps} per replayed graph)")
        assert torch.isfinite(Y).all()
        del P, X, work
        Xh = torch.randn(n, D, generator=torch.Generator().manual_seed(2)).numpy()
        ts_ = Tsne()
        ts_.fit_transform(Xh[:64])                      # code objects and the allocator warm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ts_.fit_transform(Xh)
        say(f"  Tsne().fit_transform, s      {time.perf_counter() - t0:9.3f}   (1000 iterations, host PCA and copies included; "
            f"final KL {ts_.kl_:.4f})")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
