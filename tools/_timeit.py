"""hipGraph-replay timing helper of the tools/ benches (no Python launch overhead in the numbers)."""
import torch
from melo_gan_amd import ops


def timeit(fn, reps=20):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
        def body():
            for _ in range(reps):
                fn()
        g = ops.Graph.capture(body)
        g.launch(); torch.cuda.synchronize()
        e0, e1 = ops.Event(), ops.Event()
        e0.record(); g.launch(); g.launch(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_ms(e1) / (2 * reps) * 1e3


def alternate(graphs, rewind, repeats, passes=60, batches=16):
    """us per replay of each of `graphs` (name -> ops.Graph), one after the other, `repeats` times: 16 warm replays, then
    device events around `passes` passes of `batches` replays; rewind() (the cursor to 0) goes in front of every pass.
    Returns name -> the per-repeat times.  Runs on the caller's current stream."""
    times = {name: [] for name in graphs}
    for _ in range(repeats):
        for name, g in graphs.items():
            rewind()
            for _ in range(16):
                g.launch()
            torch.cuda.synchronize()
            e0, e1 = ops.Event(), ops.Event()
            e0.record()
            for _ in range(passes):
                rewind()
                for _ in range(batches):
                    g.launch()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_ms(e1) / (batches * passes) * 1e3)
    return times
