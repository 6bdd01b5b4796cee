"""What rendering one generated roll to audio costs (csrc/render.hip, melo_gan_amd/audio.py):

    python tools/render_bench.py [--config config/gan_config.yaml --ckpt gan_final.pth] [--seed 7] [--out profiles/render_bench.txt]

  the file     one 512-note roll through midi.notes_from_roll with the 'happy' style (major, 140 bpm), 44.1 kHz, the piano voice.
               With --ckpt the roll is generate's first happy sample of that checkpoint; without one it is a seeded uniform
               roll over the generator's tanh range (every fifth row a rest), and the output says so.
  device       us per replay of a graph over the whole file -- mg_render_notes alone, with its peak, and [render with peak ->
               mg_pcm_quantise], which is what a file costs: two warm replays, then device events around enough replays for at
               least half a second, three times.  Terms = (note, partial, sample) triples that sound; a term is one sinpif,
               one expf and about ten multiplies and adds.
  CPU fp64     seconds tests/render_ref.py (numpy, one thread of the host this runs on) takes for the first ten seconds of
               the same file.  A CPU number: it says what the device path replaces, nothing about the device.
"""
import argparse
import os
import platform
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import audio, midi, ops  # noqa: E402
import render_ref  # noqa: E402

FS, VOICE = 44100, "piano"


def roll_of(args):
    if args.ckpt:
        from melo_gan_amd.gan import generate as G
        a = G.parse_args(["--config", args.config, "--ckpt", args.ckpt, "--emotion", "happy", "--samples", "1", "--seed", str(args.seed)])
        p = G.plan(a)
        s = G.Sampler(p.cfg, None, "cuda", 1)
        s.load_generator(p.ckpt)
        return s.sample(["happy"], 1, p.seed).notes[0], f"generate's happy sample 1 of {args.ckpt} (seed {p.seed})"
    rng = np.random.default_rng(args.seed)
    roll = rng.uniform(-1.0, 1.0, (512, 4)).astype(np.float32)
    roll[::5, 1] = -1.0                                     # rests
    return roll, f"a seeded uniform roll over the generator's output range (seed {args.seed}; no checkpoint given)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, default=os.path.join(ROOT, "config", "gan_config.yaml"))
    ap.add_argument("--ckpt", type=str, default=None)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", type=str, default=None, help="also write the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("render_bench measures the device path: a MI355X (ROCm) device is required")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    roll, what = roll_of(args)
    notes, _ = midi.notes_from_roll(roll, bpm=140, scale="major", root_key=0)
    r = audio.Renderer("cuda", FS, VOICE)
    (ev,), (n,) = r.plan([notes])
    v = r.voice
    audible = np.array([sum(m * int(i) < 2 ** 31 for m in v.mult) for i in ev.inc])
    span = np.minimum(ev.release.astype(np.int64) + r.release_len, n) - np.minimum(ev.onset, n)
    terms = int((audible * span).sum())
    say(f"file: {what}")
    say(f"  {len(ev)} notes, {n} samples = {n / FS:.1f} s at {FS} Hz, voice {VOICE} ({len(v.mult)} partials), {terms / 1e6:.1f} M terms "
        f"= {terms / n:.1f} per sample")

    d = r._upload([ev], [n], [0])
    pcm = torch.empty(n, dtype=torch.float32, device="cuda")
    q = torch.empty(n, dtype=torch.int16, device="cuda")
    peak = torch.empty(1, dtype=torch.float32, device="cuda")

    def render(with_peak):
        ops.render_notes(d["onset"], d["release"], d["inc"], d["gain"], d["note_ptr"], d["pcm_ptr"], d["n_begin"], d["max_len"], n,
                         r._struct, pcm, peak if with_peak else None)

    def whole():
        render(True)
        ops.pcm_quantise(pcm, d["pcm_ptr"], peak, n, r.target, q)

    def replay_us(launches):
        """[us per replay] x 3: two warm replays, then device events around enough replays for half a second."""
        launches()
        g = ops.Graph.capture(launches)
        g.launch()
        g.launch()
        torch.cuda.synchronize()
        e0, e1 = ops.Event(), ops.Event()
        e0.record(); g.launch(); e1.record()
        torch.cuda.synchronize()
        reps = max(3, int(500.0 / max(e0.elapsed_ms(e1), 1e-3)) + 1)
        times = []
        for _ in range(3):
            e0, e1 = ops.Event(), ops.Event()
            e0.record()
            for _ in range(reps):
                g.launch()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_ms(e1) / reps * 1e3)
        return times, reps

    say(f"device ({torch.cuda.get_device_name(0)}): replayed graphs over the whole file, us per replay (three windows of >= 0.5 s)")
    with torch.cuda.stream(torch.cuda.Stream()):
        for name, fn in (("render", lambda: render(False)), ("render + peak", lambda: render(True)), ("render + peak -> quantise", whole)):
            times, reps = replay_us(fn)
            us = sorted(times)[1]
            say(f"  {name:26s} {' '.join(f'{t:8.1f}' for t in times)}   median {us:8.1f}   ({reps} replays per window)")
    say(f"  the file, rendered and quantised: {n / FS / (us * 1e-6):.0f} x real time, {terms / us / 1e3:.1f} G terms/s, {n / us:.1f} M samples/s")

    ten = min(n, 10 * FS)
    t0 = time.perf_counter()
    ref = render_ref.render({"onset": ev.onset, "release": ev.release, "inc": ev.inc, "gain": ev.gain}, 0, ten, mult=v.mult,
                            weight=v.weight, decay=v.decay, attack=v.attack(FS), release_tau=v.release_tau, release_len=r.release_len,
                            fs=FS)
    cpu_s = time.perf_counter() - t0
    err, b = np.abs(pcm[:ten].cpu().numpy().astype(np.float64) - ref[0]), render_ref.bound(*ref[1:])
    say(f"CPU fp64 (tests/render_ref.py, numpy {np.__version__}, one thread of {platform.processor() or platform.machine()}, "
        f"{os.cpu_count()} CPUs): {cpu_s:.3f} s for the first {ten / FS:.0f} s of the file = {cpu_s / (ten / FS):.4f} s per second of audio")
    say(f"  the device's samples against it: worst |y - ref| / bound = {float(np.max(err[b > 0] / b[b > 0], initial=0.0)):.3f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
