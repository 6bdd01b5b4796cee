#!/usr/bin/env python3
"""MIDI files -> WAV audio on the device, with the project's own synthesiser (melo_gan_amd/audio.py, csrc/render.hip):

    python -m melo_gan_amd.render FILE.mid... [--out DIR] [--fs 44100] [--voice piano|organ|sine] [--peak-db -1]
        [--max-seconds 600]

reads each file with midi.read_smf_notes -- the class of file this project and the reference write (format 1, one tempo,
note-ons with running status), as gan/analyze_midi.py does -- and writes <DIR>/<stem>.wav, mono 16-bit, normalised to
--peak-db dB full scale.  One line per file: seconds, notes, and whether --max-seconds cut it.  Every input from outside is
checked on the host before any GPU use; a bad one ends with status 2 and a `render: error:` line.
"""
from __future__ import annotations

import argparse
import os
import struct
import sys
from dataclasses import dataclass
from typing import List

from . import audio, midi, pieces


class RenderError(ValueError):
    """A bad input of the command, found on the host before any GPU use."""


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m melo_gan_amd.render", description="Render MIDI files to WAV audio on the device.")
    ap.add_argument("files", nargs="+", metavar="FILE.mid", help="Standard MIDI files as this project writes them")
    ap.add_argument("--out", type=str, default=".", help="output directory (default: the current one)")
    ap.add_argument("--fs", type=int, default=44100, help="sample rate in Hz")
    ap.add_argument("--voice", type=str, default="piano", help=" | ".join(audio.VOICES))
    ap.add_argument("--peak-db", type=float, default=-1.0, help="peak level in dB full scale (<= 0)")
    ap.add_argument("--max-seconds", type=float, default=600.0, help="longer files are cut here, and reported")
    return ap.parse_args(argv)


def notes_of_file(path: str) -> List[midi.Note]:
    """The file's notes in seconds, (velocity, pitch, start, end), at its one tempo (120 bpm when it sets none)."""
    if not os.path.isfile(path):
        raise RenderError(f"{path} does not exist")
    try:
        (_, div), tempo, notes = midi.read_smf_notes(path)
    except (AssertionError, ValueError, IndexError, KeyError, struct.error) as e:
        raise RenderError(f"{path}: not a MIDI file this project reads ({type(e).__name__}: {e})") from e
    if div <= 0 or div & 0x8000:
        raise RenderError(f"{path}: division {div:#x}: ticks per quarter note expected")
    sec = (tempo if tempo else 500000) / (div * 1e6)
    return [(vel, pitch, on * sec, off * sec) for on, off, pitch, vel in notes]


@dataclass
class Plan:
    files: List[str]
    wavs: List[str]
    notes: List[audio.Events]
    out: str
    fs: int
    voice: str
    peak_db: float
    max_seconds: float


def plan(args) -> Plan:
    """Every check of what comes from outside, on the host (no GPU needed); raises RenderError."""
    try:
        audio.check_settings(args.fs, args.voice, args.peak_db, args.max_seconds)
    except audio.AudioError as e:
        raise RenderError(str(e)) from e
    wavs, events = [], []
    for path in args.files:
        wav = os.path.join(args.out, os.path.splitext(os.path.basename(path))[0] + ".wav")
        if wav in wavs:
            raise RenderError(f"{path}: a second input that would be written to {wav}")
        wavs.append(wav)
        try:
            events.append(audio.events_from_notes(notes_of_file(path), args.fs))
        except audio.AudioError as e:
            raise RenderError(f"{path}: {e}") from e
    if os.path.exists(args.out) and not os.path.isdir(args.out):
        raise RenderError(f"--out {args.out} exists and is not a directory")
    return Plan(list(args.files), wavs, events, args.out, args.fs, args.voice, args.peak_db, args.max_seconds)


def run(p: Plan) -> None:
    os.makedirs(p.out, exist_ok=True)
    for wav, rep in zip(p.wavs, pieces.write_wavs(p.notes, p.wavs, p.fs, p.voice, p.peak_db, p.max_seconds)):
        cut = f"  truncated at {p.max_seconds:g} s" if rep.truncated else ""
        print(f"{wav}: {rep.seconds:.3f} s, {rep.notes} notes{cut}")


def main(argv=None) -> int:
    return pieces.run_tool("render", RenderError, plan, run, parse_args(argv))


if __name__ == "__main__":
    sys.exit(main())
