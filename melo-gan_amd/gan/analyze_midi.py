#!/usr/bin/env python3
"""The reference's src/gan/analyze_midi.py ("useful for checking if the GAN is actually learning different emotions") without
pretty_midi: per .mid file the duration, note count, mean pitch, pitch range, unique pitches, mean velocity and density,
read with midi.read_smf_notes (the files `generate` and the reference write: format 1, one tempo, one instrument).

    python -m melo_gan_amd.gan.analyze_midi FILE...

The same quantities over a whole split, per emotion and compared between real and generated rolls, are
`python -m melo_gan_amd.gan.evaluate --music-metrics` (gan/music_metrics.py).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from .. import midi


def analyze(path: str) -> dict:
    """The statistics of one file (analyze_midi.py:28-45); note_count 0 leaves the rest None.  Raises on an unreadable file."""
    (_, division), tempo_us, notes = midi.read_smf_notes(path)
    out = {"file": os.path.basename(path), "note_count": len(notes), "duration": None, "mean_pitch": None, "lowest_pitch": None,
           "highest_pitch": None, "unique_pitches": None, "mean_velocity": None, "density": None}
    if not notes:
        return out
    sec = (500000 if tempo_us is None else tempo_us) / 1e6 / division       # seconds per tick
    on, off, pitch, vel = (np.array(c) for c in zip(*notes))
    duration = float(off.max()) * sec                                        # pretty_midi's get_end_time()
    out.update(duration=duration, mean_pitch=float(pitch.mean()), lowest_pitch=int(pitch.min()), highest_pitch=int(pitch.max()),
               unique_pitches=int(len(np.unique(pitch))), mean_velocity=float(vel.mean()),
               density=len(notes) / duration if duration > 0 else 0.0)
    return out


def format_analysis(a: dict) -> str:
    """The reference's report lines (analyze_midi.py:47-55)."""
    return "\n".join([f"analysis for: {a['file']}",
                      f"  Duration:     {a['duration']:.2f} seconds",
                      f"  Note Count:   {a['note_count']}",
                      f"  Avg Pitch:    {a['mean_pitch']:.2f} (MIDI Note Number)",
                      f"  Pitch Range:  {a['lowest_pitch']} - {a['highest_pitch']}",
                      f"  Unique Notes: {a['unique_pitches']} (Variety check)",
                      f"  Avg Velocity: {a['mean_velocity']:.2f} (Volume)",
                      f"  Density:      {a['density']:.2f} notes/sec",
                      "-" * 40])


def analyze_file(path: str) -> None:
    try:
        a = analyze(path)
    except Exception as e:      # noqa: BLE001 -- the reference's catch-all: any unreadable file is one report line
        print(f"[ERROR] Could not analyze {path}: {e}")
        return
    if a["note_count"] == 0:
        print(f"[-] {path}: No notes found.")
        return
    print(format_analysis(a))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m melo_gan_amd.gan.analyze_midi")
    ap.add_argument("files", nargs="+", help="List of .mid files to analyze")
    args = ap.parse_args(argv)
    print("=" * 40)
    print("      MIDI ANALYSIS REPORT")
    print("=" * 40)
    for f in args.files:
        if os.path.exists(f):
            analyze_file(f)
        else:
            print(f"[WARN] File not found: {f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
