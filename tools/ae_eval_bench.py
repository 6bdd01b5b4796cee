"""What the held-out VAE evaluation costs (melo_gan_amd/ae/evaluate.py) at the shipped config's size (MAX_NOTES 512,
LATENT_DIM 8, batch 64):

    python tools/ae_eval_bench.py [--repeats 5] [--rows 4096]

  batch        us per replayed evaluation batch (stage -> VAE eval forward -> scatter mu / logvar [-> mg_vae_eval_acc]), the
               graph with and the graph without the metrics call, alternating, device events around 60 passes of 16 batches;
               their difference is the call's cost inside the batch
  call alone   us per mg_vae_eval_acc call (both launches), 500 calls replayed as one graph
  pass         evaluate() over --rows rows: wall clock that ends in the accumulator's device->host read
and one yardstick that is not the code under test: the bytes the call must read (2 B T 16 + 2 B L 4) over the 6.3 TB/s of HBM
bandwidth a streaming kernel achieves (MI355X_MICROARCH.md).
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
from melo_gan_amd.ae.evaluate import VaeEvaluator  # noqa: E402
from _timeit import alternate, timeit  # noqa: E402

HBM_ACHIEVABLE = 6.3e12
PASSES = 60          # timed window: 60 passes of 16 batches = 960 replays
B, T, L, K = 64, 512, 8, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=4096)
    args = ap.parse_args()
    med = lambda ts: sorted(ts)[len(ts) // 2]  # noqa: E731
    n = args.rows
    g = torch.Generator().manual_seed(0)
    notes = (torch.rand(n, T, 4, generator=g) * 2 - 1).cuda()
    labels = (torch.arange(n, dtype=torch.int64) % K).cuda()
    ev = VaeEvaluator(dict(MAX_NOTES=T, LATENT_DIM=L), "cuda", B)
    ev.eng.init_weights(0)
    rep = ev.evaluate(notes, labels)                    # every buffer and workspace exists from here on
    assert rep["rows"] == n
    eng = ev.eng
    sp = ev.split_pass.split
    nb = sp.nb
    with torch.cuda.stream(eng.stream):
        graphs = {name: ops.Graph.capture(lambda m=m: ev._launches(sp.jobs, sp.order, sp.rows, False, metrics=m))
                  for name, m in (("with", True), ("without", False))}
        times = alternate(graphs, ev.ctr.zero_, args.repeats, PASSES)
        print(f"B={B} T={T} L={L}: replayed evaluation batch, us", flush=True)
        for name, ts in times.items():
            print(f"  {name:8s} metrics  {' '.join(f'{t:8.2f}' for t in ts)}   median {med(ts):8.2f}", flush=True)
        diff = med(times["with"]) - med(times["without"])
        print(f"  difference (mg_vae_eval_acc inside the batch): {diff:.2f} us = {100 * diff / med(times['with']):.1f} % of the batch",
              flush=True)
        ev.ctr.zero_()
        torch.cuda.synchronize()
        a = (eng.x, eng.recon, eng.mu, eng.lv, ev.labels, ev.acc, ev.row_i, ev.row_d, ev.ctr, ev.base, K)
        alone = [timeit(lambda: ops.vae_eval_acc(*a), reps=500) for _ in range(args.repeats)]
    print(f"  mg_vae_eval_acc alone      {' '.join(f'{t:8.2f}' for t in alone)}   median {med(alone):8.2f}", flush=True)
    nbytes = 2 * B * T * 16 + 2 * B * L * 4
    floor = nbytes / HBM_ACHIEVABLE * 1e6
    print(f"  bytes read {nbytes / 1e6:.2f} MB -> floor {floor:.2f} us at 6.3 TB/s; the call alone is {med(alone) / floor:.1f} x its floor "
          "(two dependent launches: launch-bound)", flush=True)
    ws = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.evaluate(notes, labels)
        ws.append(time.perf_counter() - t0)
    print(f"  evaluate(): {n} rows in {med(ws) * 1e3:.3f} ms (median of {args.repeats}) = {n / med(ws):,.0f} rows/s; the same "
          f"{nb} batches without the metrics call: {nb * med(times['without']) * 1e-3:.3f} ms of replays", flush=True)


if __name__ == "__main__":
    main()
