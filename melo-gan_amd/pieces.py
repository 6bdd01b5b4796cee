"""What the tools that turn rolls into files share (gan.generate, gan.morph, ae.edit, render): the emotions and their
(scale, bpm), the --wav arguments and their plan step, the writer of .mid and .wav files, the device check and main()'s
error line.  Nothing here touches the device before write_wavs; audio and midi are imported where they are used."""
from __future__ import annotations

import os
import sys
from typing import List, Optional, Sequence, Tuple

EMOTIONS = ("happy", "sad", "angry", "calm")          # emotion_to_index (gan/utils.py) = the classifier's class order
# app.py:109-110: (scale, bpm) per emotion; root key C, piano
STYLE = {"happy": ("major", 140), "sad": ("minor", 70), "angry": ("minor", 160), "calm": ("major", 90)}
WAV_PEAK_DB = -1.0
WAV_MAX_SECONDS = 3600.0      # where --wav would cut a sample: 512 steps of at most 4 beats at 60 bpm stay below it


def require_device(err=RuntimeError):
    import torch
    if not torch.cuda.is_available():
        raise err("melo_gan_amd has no CPU path: a MI355X (ROCm) device is required")


def run_tool(tool: str, err, plan, run, args, catch_run: bool = False) -> int:
    """A tool's main(): run(plan(args)) and status 0.  `err` raised by plan -- catch_run: or by run -- becomes the line
    "<tool>: error: <e>" on stderr and status 2."""
    try:
        p = plan(args)
        if catch_run:
            run(p)
    except err as e:
        print(f"{tool}: error: {e}", file=sys.stderr)
        return 2
    if not catch_run:
        run(p)
    return 0


def add_wav_arguments(ap, help_wav: str, help_fs: Optional[str] = "sample rate of the .wav files in Hz",
                      help_voice: Optional[str] = "the renderer's voice: piano, organ or sine"):
    ap.add_argument("--wav", action="store_true", help=help_wav)
    ap.add_argument("--wav-fs", type=int, default=44100, help=help_fs)
    ap.add_argument("--voice", type=str, default="piano", help=help_voice)


def plan_wav(args, err, files: bool = True, join: bool = False, report: str = "") -> Optional[dict]:
    """The --wav step of a plan, host only: the Renderer's settings {"fs", "voice", "peak_db"}, or None without --wav (an
    args without the attribute counts as without).  files: False under --no-files, which writes `report` only and so
    cannot go with join (--join) or --wav.  Raises err."""
    want = getattr(args, "wav", False)
    if (join or want) and not files:
        raise err(f"--no-files writes {report} only: it cannot go with --join or --wav")
    if not want:
        return None
    from . import audio
    wav = {"fs": args.wav_fs, "voice": args.voice, "peak_db": WAV_PEAK_DB}
    try:
        audio.check_settings(wav["fs"], wav["voice"], wav["peak_db"], WAV_MAX_SECONDS)
    except audio.AudioError as e:
        raise err(f"--wav: {e}") from e
    return wav


def joined_notes(rolls: Sequence, styles: Sequence[Tuple[str, int]], join_notes: int):
    """The note list of a joined path: every step's first join_notes rows decoded with the step's scale and bpm, offset by
    morph_metrics.join_offsets."""
    import numpy as np
    from . import midi
    from .gan.morph_metrics import join_offsets
    offsets = join_offsets(rolls, [bpm for _, bpm in styles], join_notes)
    out = []
    for roll, (scale, bpm), off in zip(rolls, styles, offsets):
        notes, _ = midi.notes_from_roll(np.asarray(roll)[:join_notes], bpm=bpm, scale=scale, root_key=0)
        out += [(vel, pitch, off + start, off + end) for vel, pitch, start, end in notes]
    return out


def write_wavs(lists, paths: Sequence[str], fs, voice, peak_db, max_seconds) -> list:
    """One Renderer and one render() call over all note lists (or audio.Events) in order; paths[i] receives file i.  Returns
    the Renderer's report, one audio.FileReport per file."""
    from . import audio
    r = audio.Renderer("cuda", fs, voice, peak_db, max_seconds)
    for path, pcm in zip(paths, r.render(lists)):
        audio.write_wav(path, pcm, fs)
    return r.report


def write_pieces(out_dir: str, pieces: Sequence[Tuple[dict, object]], wav: Optional[dict]) -> List[dict]:
    """The .mid (and, with the plan's wav settings, .wav) files of a run, in the order given.  A piece is (entry, payload):
    entry is the caller's files[] entry, whose "file" names the .mid; payload is (roll, scale, bpm), written by
    save_piano_roll_to_midi, or a ready note list (a joined path), written at 120 bpm.  With wav every piece's note list --
    a roll's is the one its .mid holds -- goes through write_wavs, and its entry gains wav, seconds and truncated.  Returns
    the entries."""
    from . import midi
    os.makedirs(out_dir, exist_ok=True)
    entries, lists = [], []
    for entry, payload in pieces:
        path = os.path.join(out_dir, entry["file"])
        if isinstance(payload, tuple):
            roll, scale, bpm = payload
            midi.save_piano_roll_to_midi(roll, path, bpm=bpm, scale=scale, root_key=0, instrument_name="Acoustic Grand Piano")
            if wav is not None:
                lists.append(midi.notes_from_roll(roll, bpm=bpm, scale=scale, root_key=0)[0])
        else:
            midi.write_smf(path, payload, 120.0, 0)
            lists.append(payload)
        entries.append(entry)
    if wav is not None:
        # x.mid -> x.wav: for generate's test_<emotion>_<k>.mid this is its wav_name(emotion, k)
        names = [f["file"][:-4] + ".wav" for f in entries]
        reports = write_wavs(lists, [os.path.join(out_dir, n) for n in names], wav["fs"], wav["voice"], wav["peak_db"], WAV_MAX_SECONDS)
        for f, name, rep in zip(entries, names, reports):
            f["wav"] = name
            f["seconds"], f["truncated"] = rep.seconds, rep.truncated
    return entries
