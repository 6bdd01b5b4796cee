#!/usr/bin/env python3
"""Import MIDI files as a split of note rolls: the first stage of MIDI -> split -> train_ae / train_ed / train_gan.

    python -m melo_gan_amd.midi_import PATH... --out SPLIT_DIR [--max-notes 512] [--hop <max-notes>] [--min-events 8]
        [--emotion E | --labels FILE.csv] [--drums]

PATH is a file or a directory, searched for *.mid and *.midi (sorted).  Every file is read by midi_in.read_midi, turned into
events on the 1/64-beat grid (midi_in.events_from_notes) and cut into windows of at most --max-notes events, --hop events
apart (midi_rolls.plan_windows); every window becomes one row of SPLIT_DIR/notes.npy (N, max_notes, 4) float32 in the
generator's output contract, padded with the reference's padding row (-1, -1, -1, -1).  The encode is mg_roll_encode when a
device is present and midi_rolls.host_roll_encode otherwise (midi_rolls.encode_plan): the bits are the same.

--emotion E labels every row; --labels FILE.csv holds lines `file name,emotion` (the file's base name; happy, sad, angry,
calm).  With labels, emotion.npy (N,) int64 holds the class index and numeric_features.npy (N, 6) generate.EMOTION_TABLE's row
of the label, without jitter: the points that generate's inputs scatter around.  Without labels numeric_features.npy holds the
reference loader's fallback, zeros, and no emotion.npy is written.  index.json holds per row the file, the window's first
event, its start beat and its loss counts, and per file the loss block and `faithful` (midi_rolls.faithful).  SPLIT_DIR is
then what train_ae, train_ed, ae.encode, ae.evaluate --split, ae.edit --split and GANDataset read.

Every check runs on the host before any GPU use and raises MidiImportError; the tool prints `midi_import: error: ...` and
returns status 2.
"""
from __future__ import annotations

import argparse
import csv
import os
import sys
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import midi_rolls as MR
from .midi_in import MidiImportError
from .pieces import EMOTIONS, run_tool


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Import MIDI files as a split of note rolls")
    ap.add_argument("paths", nargs="+", metavar="PATH", help="a .mid / .midi file, or a directory searched for them")
    ap.add_argument("--out", type=str, required=True, help="the split directory to write")
    MR.add_window_arguments(ap, max_notes=True)
    ap.add_argument("--emotion", type=str, default=None, help="one label for every file: " + ", ".join(EMOTIONS))
    ap.add_argument("--labels", type=str, default=None, help="CSV of lines `file name,emotion`")
    ap.add_argument("--cpu", action="store_true", help="encode on the host even when a device is present")
    return ap.parse_args(argv)


def read_labels(path: str) -> dict:
    if not os.path.isfile(path):
        raise MidiImportError(f"--labels: {path} does not exist")
    out = {}
    with open(path, newline="") as f:
        for ln, row in enumerate(csv.reader(f), 1):
            if not row or not "".join(row).strip():
                continue
            if len(row) != 2:
                raise MidiImportError(f"{path}: line {ln}: `file name,emotion` expected")
            name, emo = row[0].strip(), row[1].strip().lower()
            if emo not in EMOTIONS:
                if ln == 1:
                    continue        # a header line
                raise MidiImportError(f"{path}: line {ln}: emotion '{row[1].strip()}': one of {', '.join(EMOTIONS)}")
            out[os.path.basename(name)] = EMOTIONS.index(emo)
    return out


@dataclass
class ImportPlan:
    plan: MR.Plan
    out: str
    file_label: Optional[list]      # per file its class index, or None without labels
    device: bool


def plan(args) -> ImportPlan:
    if args.emotion is not None and args.labels is not None:
        raise MidiImportError("--emotion and --labels exclude each other")
    if args.max_notes < 1 or args.max_notes > (1 << 20):
        raise MidiImportError(f"--max-notes = {args.max_notes}: 1..2^20")
    if args.emotion is not None and args.emotion.lower() not in EMOTIONS:
        raise MidiImportError(f"--emotion '{args.emotion}': one of {', '.join(EMOTIONS)}")
    table = read_labels(args.labels) if args.labels is not None else None
    p = MR.plan_from_args(args.paths, args.max_notes, args, MidiImportError, search=True)
    files = [f["file"] for f in p.files]
    labels = None
    if args.emotion is not None:
        labels = [EMOTIONS.index(args.emotion.lower())] * len(files)
    elif table is not None:
        missing = [f for f in files if os.path.basename(f) not in table]
        if missing:
            raise MidiImportError(f"--labels: no line for {os.path.basename(missing[0])}" +
                                  (f" and {len(missing) - 1} more" if len(missing) > 1 else ""))
        labels = [table[os.path.basename(f)] for f in files]
    device = False
    if not args.cpu:
        import torch
        device = torch.cuda.is_available()
    return ImportPlan(p, args.out, labels, device)


def run(ip: ImportPlan) -> dict:
    from .gan.generate import EMOTION_TABLE
    p = ip.plan
    x, loss = MR.encode_plan(p, ip.device)
    W, F = x.shape[0], len(p.files)
    file_of = np.repeat(np.arange(F), np.diff(p.file_off))
    os.makedirs(ip.out, exist_ok=True)
    np.save(os.path.join(ip.out, "notes.npy"), x)
    numeric = np.zeros((W, len(EMOTION_TABLE[0])), np.float32)
    if ip.file_label is not None:
        lab = np.asarray(ip.file_label, np.int64)[file_of]
        np.save(os.path.join(ip.out, "emotion.npy"), lab)
        numeric = np.asarray(EMOTION_TABLE, np.float32)[lab]
    np.save(os.path.join(ip.out, "numeric_features.npy"), numeric)
    files = []
    for f, info in enumerate(p.files):
        lo, hi = int(p.file_off[f]), int(p.file_off[f + 1])
        blk = dict(info, windows=hi - lo, loss=MR.loss_block(loss[lo:hi], info), faithful=MR.faithful(loss[lo:hi], info))
        if ip.file_label is not None:
            blk["emotion"] = EMOTIONS[ip.file_label[f]]
        files.append(blk)
    rows = [{"file": p.files[int(file_of[w])]["file"], "window_start": int(p.win_local[w]), "events": int(p.win_len[w]),
             "start_beat": float(p.start_beat[w]), "loss": {n: int(v) for n, v in zip(MR.LOSS, loss[w])}} for w in range(W)]
    rep = {"max_notes": p.T, "rows": rows, "files": files, "encode": "device" if ip.device else "host"}
    MR.write_report(os.path.join(ip.out, "index.json"), rep)
    n_f = sum(1 for b in files if b["faithful"])
    print(f"midi_import: {F} files, {W} rows of {p.T} notes -> {ip.out} ({n_f} of {F} files faithful; "
          f"{'labelled' if ip.file_label is not None else 'no labels'})")
    return rep


def main(argv=None) -> int:
    return run_tool("midi_import", MidiImportError, plan, run, parse_args(argv))


if __name__ == "__main__":
    sys.exit(main())
