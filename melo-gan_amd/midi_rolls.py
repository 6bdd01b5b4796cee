"""From MIDI files to note rolls on the host: the window plan and its bounds check, the numpy restatements of mg_roll_encode
and mg_window_votes, what was lost on the way, and what predict, explain, midi_import and motifs share around the plan: the
window arguments, the plan of an argument list, the choice of the encode, the report writer.  numpy only: importing this
imports no torch and touches no GPU.

The roll contract's decode (csrc/note_decode.h, midi.notes_from_roll, gan.music_metrics.decode_rolls) is not injective, but on
its image -- pitches 36..96, velocities 60..127, durations 16..256 and steps 7..256 on the 1/64-beat grid -- it has an exact
inverse, and host_roll_encode is it: fp32, every operation rounded on its own, as csrc/note_decode.h's note_encode evaluates
it.  Outside the image the encode clamps and counts: LOSS names the eight counts per window.
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import List, Sequence

import numpy as np

from . import midi_in
from .gan.morph_metrics import host_path_probs

LOSS = ("pitch_raised", "pitch_lowered", "velocity_raised", "duration_lengthened", "duration_shortened", "steps_short",
        "steps_zero", "rests")
PITCH_LO, PITCH_HI, VEL_LO, VEL_HI, DUR_LO, Q_HI = 36, 96, 60, 127, 16, 256
EXTENSIONS = (".mid", ".midi")
DEFAULT_MAX_NOTES, DEFAULT_MIN_EVENTS = 512, 8


def plan_windows(E: int, T: int, hop: int, min_events: int):
    """The windows of a file of E events: window j starts at event j * hop and holds at most T events; the window that reaches
    the file's end is the last, and may be partial.  Windows shorter than min_events are dropped unless the file would be
    left with none.  Returns (start int64 (n,), length int32 (n,))."""
    E, T, hop, min_events = int(E), int(T), int(hop), int(min_events)
    if E < 1 or T < 1 or hop < 1 or min_events < 1:
        raise ValueError(f"plan_windows: E = {E}, T = {T}, hop = {hop}, min_events = {min_events}: all must be positive")
    starts, lens, s = [], [], 0
    while s < E:            # a hop above T leaves events outside every window
        starts.append(s)
        lens.append(min(T, E - s))
        if s + T >= E:
            break
        s += hop
    keep = [i for i, n in enumerate(lens) if n >= min_events] or [0]
    return np.array([starts[i] for i in keep], np.int64), np.array([lens[i] for i in keep], np.int32)


def encode_events(events):
    """note_encode over an (E, 4) int event list: (x float32 (E, 4), fired int64 (E, 8) of 0 / 1 in LOSS order)."""
    ev = np.asarray(events).astype(np.int64).reshape(-1, 4)
    f = np.float32
    pitch, vel, dur, step = ev[:, 0], ev[:, 1], ev[:, 2], ev[:, 3]
    rest = vel < 0
    s = np.clip(step, 0, Q_HI)
    p, v, d = np.clip(pitch, PITCH_LO, PITCH_HI), np.clip(vel, VEL_LO, VEL_HI), np.clip(dur, DUR_LO, Q_HI)
    x = np.empty((ev.shape[0], 4), f)
    x[:, 0] = (p.astype(f) + f(0.5)) / f(63.5) - f(1.0)
    q = ((v.astype(f) + f(0.5)) - f(60.0)) / f(67.0)
    x[:, 1] = np.where(v == VEL_HI, f(1.0), q * f(1.2) + f(-0.2))
    x[:, 2] = d.astype(f) / f(128.0) - f(1.0)
    x[rest, :3] = f(-1.0)
    x[:, 3] = s.astype(f) / f(128.0) - f(1.0)
    note = ~rest
    fired = np.stack([note & (pitch < p), note & (pitch > p), note & (vel < v), note & (dur < d), note & (dur > d),
                      (s > 0) & (s < midi_in.STEP_FLOOR), s == 0, rest], axis=1).astype(np.int64)
    return x, fired


def windows_outside(win_start, win_len, E: int, T: int) -> bool:
    """Whether a window begins in front of an event list of E events, ends past it or is longer than T."""
    ws, wl = np.asarray(win_start, np.int64), np.asarray(win_len, np.int64)
    return bool(((ws < 0) | (wl < 0) | (wl > T) | (ws + wl > E)).any())


def host_roll_encode(events, win_start, win_len, T: int, rows: int = None):
    """mg_roll_encode on the host, all windows at once: (x float32 (rows, T, 4), loss int64 (rows, 8)); rows defaults to the
    number of windows W, rows past W hold the padding row and zero counts.  A window that points outside `events` raises."""
    ev = np.asarray(events).reshape(-1, 4)
    ws, wl = np.asarray(win_start, np.int64), np.asarray(win_len, np.int64)
    W, T = ws.shape[0], int(T)
    rows = W if rows is None else int(rows)
    if wl.shape != (W,) or rows < W or windows_outside(ws, wl, ev.shape[0], T):
        raise ValueError("host_roll_encode: a window points outside the event list or is longer than T")
    code, fired = encode_events(ev)
    x = np.full((rows, T, 4), -1.0, np.float32)
    loss = np.zeros((rows, len(LOSS)), np.int64)
    for w in range(W):
        a, n = int(ws[w]), int(wl[w])
        x[w, :n] = code[a:a + n]
        loss[w] = fired[a:a + n].sum(axis=0)
    return x, loss


def first_argmax(v) -> int:
    """The first index of the maximum, NaN counting as the maximum (mg_emotion_score's rule; numpy's argmax agrees)."""
    return int(np.argmax(np.asarray(v)))


def host_window_votes(logits, file_off) -> dict:
    """mg_window_votes on the host: logits (W, K) fp32, file_off (F + 1,) -> {"probs" (W, K) fp64, "win_pred" (W,) int32,
    "file_mean" (F, K) fp64, "file_pred" (F,) int32, "switches" (F,) int32}."""
    z = np.asarray(logits, np.float32)
    off = np.asarray(file_off, np.int64)
    W, K = z.shape
    F = off.shape[0] - 1
    if F < 1 or off[0] < 0 or off[-1] > W or (np.diff(off) < 0).any():
        raise ValueError("host_window_votes: file_off must rise from >= 0 to <= W and name at least one file")
    with np.errstate(all="ignore"):
        probs = host_path_probs(z, np.zeros(W, np.int32), 1, 1)[0] if W else np.zeros((0, K))
    win_pred = np.array([first_argmax(r) for r in z], np.int32).reshape(W)
    mean, pred, sw = np.zeros((F, K)), np.full(F, -1, np.int32), np.zeros(F, np.int32)
    for f in range(F):
        lo, hi = int(off[f]), int(off[f + 1])
        if hi == lo:
            continue
        for k in range(K):
            s = 0.0
            for w in range(lo, hi):
                s = s + probs[w, k]
            mean[f, k] = s / float(hi - lo)
        pred[f] = first_argmax(mean[f])
        sw[f] = int((win_pred[lo + 1:hi] != win_pred[lo:hi - 1]).sum())
    return {"probs": probs, "win_pred": win_pred, "file_mean": mean, "file_pred": pred, "switches": sw}


def faithful(loss, info: dict) -> bool:
    """Whether decoding the encoded windows gives the file's own notes: nothing clamped (the first five counts), nothing
    spread to 0.1 beat (steps_short, steps_zero), nothing dropped (drum notes, the offset in front of the first note, events
    outside every window) and no note closed by the reader.  Rests lose nothing."""
    lost = np.asarray(loss, np.int64).reshape(-1, len(LOSS))[:, :7].sum()
    return bool(lost == 0 and not info.get("dropped_drums", 0) and not info.get("unpaired", 0) and not info.get("lead_q", 0)
                and not info.get("dropped_events", 0))


def find_files(paths: Sequence[str]) -> List[str]:
    """Every PATH as given when it is a file; a directory is searched, subdirectories included, for *.mid and *.midi, sorted."""
    out = []
    for p in paths:
        if os.path.isdir(p):
            found = []
            for root, _, names in os.walk(p):
                found += [os.path.join(root, n) for n in names if n.lower().endswith(EXTENSIONS)]
            out += sorted(found)
        elif os.path.isfile(p):
            out.append(p)
        else:
            raise midi_in.MidiImportError(f"{p}: no such file or directory")
    if not out:
        raise midi_in.MidiImportError("no .mid / .midi file among " + ", ".join(map(str, paths)))
    return out


@dataclass
class Plan:
    """All files' events in one array and their windows.  files[f]: {"file", "notes", "events", "rests", "beats", "lead_q",
    "dropped_drums", "unpaired", "dropped_events", "tempo_us", "division"}; window w of file f (file_off[f] <= w <
    file_off[f + 1]) holds the events win_start[w] .. win_start[w] + win_len[w] - 1 of `events` and begins start_beat[w] beats
    into its file."""
    events: np.ndarray          # int32 (E, 4)
    win_start: np.ndarray       # int64 (W,), into events
    win_len: np.ndarray         # int32 (W,)
    win_local: np.ndarray       # int64 (W,), the window's first event counted from its file's first
    start_beat: np.ndarray      # float64 (W,)
    file_off: np.ndarray        # int64 (F + 1,)
    files: List[dict]
    T: int


def plan_files(paths: Sequence[str], T: int, hop: int, min_events: int, drums: bool = False) -> Plan:
    """read_midi -> events_from_notes -> plan_windows over every file, in order.  Raises MidiImportError."""
    if int(T) < 1 or int(hop) < 1 or int(min_events) < 1:
        raise midi_in.MidiImportError(f"max_notes = {T}, hop = {hop}, min_events = {min_events}: all must be positive")
    evs, starts, lens, local, beats, off, files, base = [], [], [], [], [], [0], [], 0
    for path in paths:
        m = midi_in.read_midi(path, drums)
        ev, info = midi_in.events_from_notes(m.notes, m.division)
        ws, wl = plan_windows(ev.shape[0], T, hop, min_events)
        covered = np.zeros(ev.shape[0], bool)
        for a, n in zip(ws.tolist(), wl.tolist()):
            covered[a:a + n] = True
        evs.append(ev)
        starts.append(ws + base)
        lens.append(wl)
        local.append(ws)
        beats.append((info["lead_q"] + info["onset_q"][ws]) / float(midi_in.GRID))
        off.append(off[-1] + ws.shape[0])
        files.append({"file": path, "notes": info["notes"], "events": info["events"], "rests": info["rests"],
                      "beats": (info["lead_q"] + info["length_q"]) / float(midi_in.GRID), "lead_q": info["lead_q"],
                      "dropped_drums": m.dropped_drums, "unpaired": m.unpaired, "dropped_events": int((~covered).sum()),
                      "tempo_us": m.tempo_us, "division": m.division})
        base += ev.shape[0]
    return Plan(np.ascontiguousarray(np.concatenate(evs), np.int32), np.concatenate(starts).astype(np.int64),
                np.concatenate(lens).astype(np.int32), np.concatenate(local).astype(np.int64), np.concatenate(beats),
                np.array(off, np.int64), files, int(T))


def check_plan(p: Plan, T: int = None, err=ValueError):
    """The one bounds check of a Plan: at least one window, every window inside the event list and no longer than p.T,
    file_off rising from 0 to W; with T, windows of T events.  Raises err."""
    if not isinstance(p, Plan) or (T is not None and p.T != T):
        raise err("a plan of windows" + ("" if T is None else f" of {T} events") + " expected")
    W = p.win_start.shape[0]
    if W < 1 or p.win_len.shape != (W,) or windows_outside(p.win_start, p.win_len, p.events.shape[0], p.T) or \
            p.file_off[0] != 0 or p.file_off[-1] != W or (np.diff(p.file_off) < 0).any():
        raise err("a window points outside the event list, or the files' offsets do not cover the windows")


def add_window_arguments(ap, max_notes: bool):
    """--hop, --min-events and --drums; max_notes: --max-notes too, for a tool whose window length no config sets."""
    if max_notes:
        ap.add_argument("--max-notes", type=int, default=DEFAULT_MAX_NOTES, help="events per window of a MIDI file")
    ap.add_argument("--hop", type=int, default=None,
                    help="events between window starts (default: " + ("--max-notes)" if max_notes else "the config's max_notes)"))
    ap.add_argument("--min-events", type=int, default=DEFAULT_MIN_EVENTS)
    ap.add_argument("--drums", action="store_true", help="keep the notes of channel 10")


def plan_from_args(paths: Sequence[str], T: int, args, err, search: bool = False) -> Plan:
    """plan_files over a tool's PATH arguments, which search looks through with find_files and which otherwise must all be
    files, with its window arguments.  Every MidiImportError is raised again as err(its message)."""
    try:
        files = find_files(paths) if search else list(paths)
        for f in files:
            if not os.path.isfile(f):
                raise midi_in.MidiImportError(f"{f}: no such file")
        return plan_files(files, T, T if args.hop is None else args.hop, args.min_events, args.drums)
    except midi_in.MidiImportError as e:
        raise err(str(e)) from e


def encode_plan(p: Plan, device: bool):
    """(x float32 (W, T, 4), loss int64 (W, 8)) from mg_roll_encode on the device or from host_roll_encode: the same bits."""
    if device:
        from .eval_pass import device_roll_encode
        return device_roll_encode(p)
    return host_roll_encode(p.events, p.win_start, p.win_len, p.T)


def write_report(path: str, rep: dict, err=ValueError, what: str = "the report holds a value that is not finite"):
    """rep as JSON at path, whose directory is made.  The text is complete before the file is opened: a value that is not
    finite raises err("<what> (<json's words>)") and leaves no file."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    try:
        text = json.dumps(rep, indent=1, allow_nan=False)
    except ValueError as e:
        raise err(f"{what} ({e})") from e
    with open(path, "w") as f:
        f.write(text)


def loss_block(loss_rows, info: dict) -> dict:
    """A file's loss report: the encode's counts summed over its windows, and what the reader and the plan left out."""
    s = np.asarray(loss_rows, np.int64).reshape(-1, len(LOSS)).sum(axis=0)
    out = {n: int(v) for n, v in zip(LOSS, s)}
    out.update(dropped_drums=int(info["dropped_drums"]), unpaired=int(info["unpaired"]), lead_q=int(info["lead_q"]),
               dropped_events=int(info["dropped_events"]))
    return out
