"""What evaluate --frechet costs (csrc/frechet.hip) at D = 256, n = 2048 rows per side:

    python tools/frechet_bench.py [--repeats 7] [--rows 2048]

  feature_space()   ms per call of Evaluator.feature_space with and without frechet=True on the same stashes: device events on
                    the engine's stream around the call (which ends in the block's one device -> host read), after two warm
                    calls, median of --repeats.  The stashes are random mixtures: 4 emotions, 10 sets, 17 pairs.
  the parts         the 10 mg_feat_moments launches, and one mg_frechet_pairs over 10 sets and 17 pairs, alone
  the pass          wall clock of evaluate() (features=True, no frechet) over the same number of rows at the shipped shape's
                    T = 512, C = 4, batch 64: the pass that produces the features, for scale
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import ops  # noqa: E402
from melo_gan_amd.gan import evaluate as EV  # noqa: E402
from melo_gan_amd.gan.config import default_ed_cfg, default_gan_cfg  # noqa: E402
from melo_gan_amd.gan.dataset import GANDataset  # noqa: E402


def events_ms(fn, repeats, stream):
    ts = []
    with torch.cuda.stream(stream):
        for _ in range(2):
            fn()
        for _ in range(repeats):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rows", type=int, default=2048)
    args = ap.parse_args()
    med = lambda ts: sorted(ts)[len(ts) // 2]  # noqa: E731
    Bsz, T, C, n = 64, 512, 4, args.rows
    cfg, ed_cfg = default_gan_cfg(Bsz, T, C), default_ed_cfg(C)
    ds = GANDataset.synthetic(n, T, C, cfg["LATENT_DIM"], 1, "cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    out = {}
    for frechet in (False, True):
        ev = EV.Evaluator(cfg, ed_cfg, "cuda", Bsz, features=True, frechet=frechet)
        ev.has_d = True
        ev.evaluate(ds, 1)                               # builds the graph and the stashes
        if not frechet:
            ws = []
            for _ in range(args.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ev.evaluate(ds, 1)
                ws.append(time.perf_counter() - t0)
            print(f"evaluate(features=True): {n} rows (B={Bsz} T={T} C={C}) in {med(ws) * 1e3:.2f} ms, its feature_space() call "
                  f"included (median of {args.repeats})", flush=True)
        D = ev.eng.ed_feat_dim
        labels = ev._labels_host
        centres = torch.randn(8, D, device="cuda", generator=g)
        for stash, lo in ((ev.feat_real, 0), (ev.feat_fake, 4)):     # the two sides around different centres
            pick = torch.randint(lo, lo + 4, (n,), device="cuda", generator=g)
            stash[:n].copy_(centres[pick] + 0.7 * torch.randn(n, D, device="cuda", generator=g))
        torch.cuda.synchronize()
        ts = events_ms(lambda: out.__setitem__(frechet, ev.feature_space(labels, n)), args.repeats, ev.eng.stream)
        print(f"feature_space(frechet={frechet}): D = {D}, {n} rows per side: {' '.join(f'{t:8.2f}' for t in ts)}   median "
              f"{med(ts):8.2f} ms", flush=True)
    fr = out[True]["frechet"]
    print(f"  fd {fr['fd']:.6g} (mean {fr['mean_term']:.6g}, trace {fr['trace_term']:.6g}, sqrt {fr['sqrt_term']:.6g}); effective rank "
          f"real {out[True]['spectrum']['real']['effective_rank']:.2f}, fake {out[True]['spectrum']['fake']['effective_rank']:.2f}")
    # the parts alone
    S, P, D = 10, 17, 256
    sets = [torch.randn(n if i < 2 else n // 4, D, device="cuda", generator=g) * (1 + 0.1 * i) for i in range(S)]
    means, covs = torch.empty(S, D, dtype=torch.float64, device="cuda"), torch.empty(S, D, D, dtype=torch.float64, device="cuda")
    pairs = torch.tensor([(0, 1)] + [(2 + e, 6 + f) for e in range(4) for f in range(4)], dtype=torch.int32).cuda()
    res = (torch.empty(P, 4, dtype=torch.float64, device="cuda"), torch.empty(S, 3, dtype=torch.float64, device="cuda"),
           torch.empty(S + P, 2, dtype=torch.int32, device="cuda"))
    s = torch.cuda.Stream()

    def moments():
        for i, X in enumerate(sets):
            ops.feat_moments(X, means[i], covs[i])

    for name, fn in (("10 x mg_feat_moments", moments), ("mg_frechet_pairs, 10 sets, 17 pairs", lambda: ops.frechet_pairs(means, covs, pairs, *res))):
        ts = events_ms(fn, args.repeats, s)
        print(f"{name}: {' '.join(f'{t:8.2f}' for t in ts)}   median {med(ts):8.2f} ms", flush=True)
    info = res[2].cpu()
    print(f"  sweeps of the 10 covariances {info[:S, 0].tolist()}, of the 17 products {info[S:, 0].tolist()}; converged "
          f"{bool(info[:, 1].all())}")


if __name__ == "__main__":
    main()
