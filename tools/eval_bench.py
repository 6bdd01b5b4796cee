"""What the metrics accumulation costs in an evaluation batch (melo_gan_amd/gan/evaluate.py), at cfg2 size (B = 64, T = 256,
C = 128) and at the shipped config's (B = 64, T = 512, C = 4):

    python tools/eval_bench.py [--repeats 5] [--music]

  batch        us per replayed evaluation batch (stage -> noise -> E_num -> G -> critic -> classifier [-> mg_eval_acc]), the graph
               with and the graph without the metrics call, alternating, device events around 60 passes of 16 batches; their
               difference is the call's cost inside the batch
  call alone   us per mg_eval_acc call, 500 calls replayed as one graph, twice
and two yardsticks that are not the code under test:
  torch        the same reductions as torch device ops on the same buffers (per class index_add_ of the fp64 row sums of x and
               x * x, amin / amax with index_reduce_, bincount for the counts and the two confusion matrices, the critic sums):
               eager, device events around 500 repetitions
  floor        the bytes the pass must read (2 B T C floats) over the 6.3 TB/s of HBM bandwidth a streaming kernel achieves
               (MI355X_MICROARCH.md)
then the evaluator's rows/s over a whole pass (evaluate(): wall clock, ends in the accumulator's device->host read).
--music runs the leg of --music-metrics instead, at the shipped config's size (the note decode needs C = 4): us per replayed
batch of an Evaluator(music=True) with mg_note_stats in the graph and without it -- the latter is the batch as it was before
the launch existed -- alternating as above, and mg_note_stats alone, 500 calls replayed as one graph.
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
from _timeit import alternate, timeit  # noqa: E402

HBM_ACHIEVABLE = 6.3e12
PASSES = 60          # timed window: 60 passes of 16 batches = 960 replays, a few tenths of a second
K = 4


def torch_reductions(real, fake, labels, d_real, d_fake, lf, lr, out):
    B, T, C = real.shape
    for s, x in enumerate((real, fake)):
        xd = x.double()
        out["sum"][s].index_add_(0, labels, xd.sum(1))
        out["sq"][s].index_add_(0, labels, (xd * xd).sum(1))
        out["min"][s].index_reduce_(0, labels, x.amin(1), "amin")
        out["max"][s].index_reduce_(0, labels, x.amax(1), "amax")
    out["n"] += torch.bincount(labels, minlength=K)
    for s, lg in enumerate((lf, lr)):
        out["conf"][s] += torch.bincount(labels * K + torch.argmax(lg, 1), minlength=K * K)
        z = lg.double()
        ce = torch.logsumexp(z, 1) - z.gather(1, labels[:, None])[:, 0]
        p = torch.softmax(z, 1).gather(1, labels[:, None])[:, 0]
        out["cls"][s, 0].index_add_(0, labels, ce)
        out["cls"][s, 1].index_add_(0, labels, p)
    out["d"][0] += d_real.double().sum()
    out["d"][1] += d_fake.double().sum()


def events_us(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def batch_graphs(ev, ds, n, variants):
    """One captured evaluation batch per variant: name -> a function that sets the evaluator up for that variant's capture and
    returns the `metrics` argument of _launches."""
    eng = ev.eng
    sp = ev.split_pass.split
    jobs = [(ds.notes, eng.real), (ds.numeric, eng.numeric), (sp.labels, eng.emot_idx), (ds.latent, eng.latent)]
    graphs = {}
    for name, prepare in variants:
        metrics = prepare()
        graphs[name] = ops.Graph.capture(lambda: ev._launches(jobs, sp.order, n, n, 1, True, metrics=metrics))
    return graphs


def music_leg(repeats, med):
    B, T, C = 64, 512, 4
    cfg, ed_cfg = default_gan_cfg(B, T, C), default_ed_cfg(C)
    n = 16 * B
    ds = GANDataset.synthetic(n, T, C, cfg["LATENT_DIM"], 1, "cuda")
    ev = EV.Evaluator(cfg, ed_cfg, "cuda", B, music=True)
    ev.has_d = True
    rep = ev.evaluate(ds, 1)
    assert rep["n"] == n and "music" in rep
    eng = ev.eng

    def variant(music):
        def prepare():
            ev.music = music
            return True
        return prepare

    with torch.cuda.stream(eng.stream):
        graphs = batch_graphs(ev, ds, n, (("with", variant(True)), ("without", variant(False))))
        ev.music = True
        times = alternate(graphs, ev.ctr.zero_, repeats, PASSES)
    print(f"music: B={B} T={T} C={C}: replayed evaluation batch, us", flush=True)
    for name, ts in times.items():
        print(f"  {name:8s} note_stats  {' '.join(f'{t:8.2f}' for t in ts)}   median {med(ts):8.2f}", flush=True)
    diff = med(times["with"]) - med(times["without"])
    print(f"  difference (mg_note_stats inside the batch): {diff:.2f} us = {100 * diff / med(times['without']):.1f} % of the batch "
          "without it", flush=True)
    ev.ctr.zero_()                                        # split positions inside the stashes: the per-row stores happen
    torch.cuda.synchronize()
    a = (eng.real, eng.fake_d, eng.emot_idx, ev.note_acc, ev.note_row_i, ev.note_row_beats, ev.ctr, ev.base, K)
    alone = [timeit(lambda: ops.note_stats(*a), reps=500) for _ in range(repeats)]
    print(f"  mg_note_stats alone        {' '.join(f'{t:8.2f}' for t in alone)}   median {med(alone):8.2f}", flush=True)
    nbytes = 2 * B * T * 16
    floor = nbytes / HBM_ACHIEVABLE * 1e6
    print(f"  bytes read {nbytes / 1e6:.2f} MB -> floor {floor:.2f} us at 6.3 TB/s; the call alone is {med(alone) / floor:.1f} x its floor "
          "(launch-bound)", flush=True)
    ws = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.evaluate(ds, 1)
        ws.append(time.perf_counter() - t0)
    print(f"  evaluate(music=True): {n} rows in {med(ws) * 1e3:.3f} ms (median of {repeats}) = {n / med(ws):,.0f} rows/s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--music", action="store_true", help="time the --music-metrics launch (mg_note_stats) instead")
    args = ap.parse_args()
    med = lambda ts: sorted(ts)[len(ts) // 2]  # noqa: E731
    if args.music:
        music_leg(args.repeats, med)
        return
    for tag, (B, T, C) in (("cfg2", (64, 256, 128)), ("shipped", (64, 512, 4))):
        cfg, ed_cfg = default_gan_cfg(B, T, C), default_ed_cfg(C)
        n = 16 * B
        ds = GANDataset.synthetic(n, T, C, cfg["LATENT_DIM"], 1, "cuda")
        ev = EV.Evaluator(cfg, ed_cfg, "cuda", B)
        ev.has_d = True                                   # weights_init fills the critic: any weights time the same
        rep = ev.evaluate(ds, 1)                          # builds the pass's graph; every workspace exists from here on
        assert rep["n"] == n
        eng = ev.eng
        with torch.cuda.stream(eng.stream):
            graphs = batch_graphs(ev, ds, n, (("with", lambda: True), ("without", lambda: False)))
            times = alternate(graphs, ev.ctr.zero_, args.repeats, PASSES)
        print(f"{tag}: B={B} T={T} C={C}: replayed evaluation batch, us", flush=True)
        for name, ts in times.items():
            print(f"  {name:8s} metrics  {' '.join(f'{t:8.2f}' for t in ts)}   median {med(ts):8.2f}", flush=True)
        diff = med(times["with"]) - med(times["without"])
        print(f"  difference (the metrics call inside the batch): {diff:.2f} us = {100 * diff / med(times['with']):.1f} % of the batch",
              flush=True)
        # the call alone, on the engine's buffers as the pass left them
        acc = ops.eval_acc_new(K, C, "cuda")
        args_ = (eng.real, eng.fake_d, eng.emot_idx, eng.s[:B], eng.s[B:2 * B], eng.logits, ev.logits_real)
        alone = [timeit(lambda: ops.eval_acc(*args_, acc), reps=500) for _ in range(args.repeats)]
        print(f"  mg_eval_acc alone          {' '.join(f'{t:8.2f}' for t in alone)}   median {med(alone):8.2f}", flush=True)
        out = {"sum": torch.zeros(2, K, C, dtype=torch.float64, device="cuda"), "sq": torch.zeros(2, K, C, dtype=torch.float64, device="cuda"),
               "min": torch.full((2, K, C), float("inf"), device="cuda"), "max": torch.full((2, K, C), float("-inf"), device="cuda"),
               "n": torch.zeros(K, dtype=torch.int64, device="cuda"), "conf": torch.zeros(2, K * K, dtype=torch.int64, device="cuda"),
               "cls": torch.zeros(2, 2, K, dtype=torch.float64, device="cuda"), "d": torch.zeros(2, dtype=torch.float64, device="cuda")}
        lab = eng.emot_idx.clamp(min=0)
        tt = [events_us(lambda: torch_reductions(eng.real, eng.fake_d, lab, eng.s[:B], eng.s[B:2 * B], eng.logits, ev.logits_real, out),
                        500) for _ in range(args.repeats)]
        print(f"  torch device ops (eager)   {' '.join(f'{t:8.2f}' for t in tt)}   median {med(tt):8.2f}", flush=True)
        nbytes = 2 * B * T * C * 4
        floor = nbytes / HBM_ACHIEVABLE * 1e6
        print(f"  bytes read {nbytes / 1e6:.2f} MB -> floor {floor:.2f} us at 6.3 TB/s; the call alone is {med(alone) / floor:.1f} x its floor",
              flush=True)
        ws = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.evaluate(ds, 1)
            ws.append(time.perf_counter() - t0)
        print(f"  evaluate(): {n} rows in {med(ws) * 1e3:.3f} ms (median of {args.repeats}) = {n / med(ws):,.0f} rows/s", flush=True)


if __name__ == "__main__":
    main()
