"""What the held-out classifier evaluation costs (melo_gan_amd/emotion_discriminator/evaluate.py) at the reference's shape:
input_mode notes, max_notes 512, note_dim 4, batch 64, the 193 rows of the reference's test split.

    python tools/ed_eval_bench.py [--rows 193] [--replays 20] [--warmup 5]

  pass with / without   ms per pass of ceil(rows / 64) replays of the captured evaluation batch (stage -> eval forward ->
                        scatter logits [-> mg_cls_eval_acc]); device events around each pass, the median of --replays passes
                        after --warmup, one graph after the other
  metrics call alone    us per mg_cls_eval_acc call (both launches), one captured call replayed
  auroc alone           us per mg_cls_auroc_pairs call on the pass's stored probabilities
  run_epoch             ms of train_ed.run_epoch(train=False) over the same rows: the forward-only validation loop the
                        trainer has (host-indexed batches, its own trailing partial batch), wall clock to its host read
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
from melo_gan_amd.emotion_discriminator.evaluate import EdEvaluator  # noqa: E402

B, T, C, K = 64, 512, 4, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=193)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    med = lambda ts: sorted(ts)[len(ts) // 2]  # noqa: E731
    n = args.rows
    cfg = dict(input_mode="notes", note_dim=C, notes_hidden=256, notes_blocks=4, mlp_hidden=[256, 128], n_classes=K, dropout=0.2,
               max_notes=T, batch_size=B, seed=42)
    x, y = train_ed.synthetic_split(n, T, C, 0, "cuda")
    ev = EdEvaluator(cfg, "cuda", B)
    ev.eng.init_weights(0)
    rep = ev.evaluate(x, y)                             # every buffer and workspace exists from here on
    assert rep["rows"] == n
    eng = ev.eng
    sp = ev.split_pass.split
    nb = sp.nb

    def timed(fn):
        ts = []
        for i in range(args.warmup + args.replays):
            e0, e1 = ops.Event(), ops.Event()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ts.append(e0.elapsed_ms(e1))
        return ts

    with torch.cuda.stream(eng.stream):
        graphs = {name: ops.Graph.capture(lambda m=m: ev._batch(sp.jobs, sp.order, sp.rows, metrics=m))
                  for name, m in (("with", True), ("without", False))}

        def a_pass(gr):
            ev.ctr.zero_()
            for _ in range(nb):
                gr.launch()
            # without the call the cursor does not advance: every replay is batch 0, the same work

        times = {name: timed(lambda gr=gr: a_pass(gr)) for name, gr in graphs.items()}
        print(f"notes T={T} C={C} B={B}, {n} rows = {nb} batches: one pass, ms (median of {args.replays} after {args.warmup})", flush=True)
        for name, ts in times.items():
            print(f"  {name:8s} metrics  median {med(ts):8.4f}  min {min(ts):8.4f}  max {max(ts):8.4f}", flush=True)
        diff = med(times["with"]) - med(times["without"])
        print(f"  difference ({nb} mg_cls_eval_acc calls inside the pass): {diff * 1e3:.2f} us = {100 * diff / med(times['with']):.1f} % "
              "of the pass", flush=True)
        ev.ctr.zero_()
        call = ops.Graph.capture(lambda: ops.cls_eval_acc(eng.logits, ev.labels, ev.acc, ev.probs, ev.row_i, ev.row_d, ev.ctr, ev.base,
                                                          ev.n_bins, ev.inv_temps))
        alone = timed(call.launch)
        print(f"  mg_cls_eval_acc alone (two launches)   median {med(alone) * 1e3:8.2f} us", flush=True)
        pairs = ops.Graph.capture(lambda: ops.cls_auroc_pairs(ev.probs, y, ev.pair_out))
        auroc = timed(pairs.launch)
        print(f"  mg_cls_auroc_pairs alone ({n} rows)      median {med(auroc) * 1e3:8.2f} us", flush=True)
    ws = []
    for _ in range(args.warmup + args.replays):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.evaluate(x, y)
        ws.append(time.perf_counter() - t0)
    print(f"  evaluate() wall clock, calibration and report included: median {med(ws[args.warmup:]) * 1e3:.3f} ms", flush=True)
    tr = EdEngine(cfg, "cuda", B, T)
    tr.init_weights(0)
    rs = []
    with torch.cuda.stream(tr.stream):
        for _ in range(args.warmup + args.replays):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            train_ed.run_epoch(tr, x, y, False, True)
            rs.append(time.perf_counter() - t0)
    print(f"  train_ed.run_epoch(train=False) over the same rows, wall clock: median {med(rs[args.warmup:]) * 1e3:.3f} ms", flush=True)


if __name__ == "__main__":
    main()
