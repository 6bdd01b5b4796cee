"""A general Standard MIDI File reader and the step from its notes to the event list the roll encode takes.  numpy only:
nothing here imports torch or touches a GPU.

midi.read_smf_notes parses the files this project writes (format 1, one tempo, note-ons only).  read_midi reads what other
programs write: formats 0 and 1, running status, 0x8n note-offs and velocity-0 note-ons, every other channel message, sysex
and meta event skipped by its length, all tracks merged.  Time is kept in ticks and leaves here in beats = ticks / division:
a tempo change moves seconds, never beats, and the roll contract (midi.notes_from_roll) counts beats.

events_from_notes turns the notes into (pitch, velocity, dur_q, step_q) events on the 1/64-beat grid, the order and the unit
of a roll's positions; melo_gan_amd/midi_rolls.py cuts them into windows and encodes them.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import Tuple

import numpy as np

GRID = 64                   # grid units per beat
STEP_MAX = 256              # the contract's longest step and duration, 4 beats
STEP_FLOOR = 7              # a step below 7/64 beat decodes as max(0.1, .) = 0.1 beat
DEFAULT_TEMPO_US = 500000   # 120 bpm, the SMF default when a file sets none
DRUM_CHANNEL = 9


class MidiImportError(ValueError):
    """A file that is not a readable SMF: the message carries the path and the byte offset."""


@dataclass
class MidiNotes:
    """What read_midi returns.  notes: int64 (N, 5) rows (tick_on, tick_off, pitch, velocity, channel), all tracks merged,
    sorted by (tick_on, pitch, track order)."""
    format: int
    division: int
    tempo_us: int               # the first set_tempo (the earliest; DEFAULT_TEMPO_US when there is none)
    notes: np.ndarray
    dropped_drums: int          # notes of channel index 9 left out (0 with drums=True)
    unpaired: int               # note-ons without a note-off, closed at their track's end


def _fail(path, pos, what):
    raise MidiImportError(f"{path}: byte {pos}: {what}")


def _vlq(data: bytes, p: int, end: int, path) -> Tuple[int, int]:
    v = 0
    for n in range(4):
        if p >= end:
            _fail(path, p, "truncated variable-length quantity")
        c = data[p]
        p += 1
        v = (v << 7) | (c & 0x7F)
        if not c & 0x80:
            return v, p
    _fail(path, p, "variable-length quantity longer than 4 bytes")


_DATA_LEN = {0x80: 2, 0x90: 2, 0xA0: 2, 0xB0: 2, 0xC0: 1, 0xD0: 1, 0xE0: 2}


def read_midi(path: str, drums: bool = False) -> MidiNotes:
    """Parses formats 0 and 1.  Note-off is 0x8n or a note-on of velocity 0, paired first-in-first-out per (channel, pitch); a
    note-off without a note-on is ignored.  Raises MidiImportError for an SMPTE division, a bad chunk tag, a truncated chunk
    or event, format 2, or a file without notes."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 14 or data[:4] != b"MThd":
        _fail(path, 0, "no MThd header chunk")
    hlen, fmt, ntrk, div = struct.unpack(">IHHH", data[4:14])
    if hlen < 6 or 8 + hlen > len(data):
        _fail(path, 4, f"header chunk of {hlen} bytes")
    if fmt not in (0, 1):
        _fail(path, 8, f"format {fmt}: formats 0 and 1 are read")
    if div & 0x8000:
        _fail(path, 12, "SMPTE division: beats are ticks / division, and this file counts frames")
    if div == 0:
        _fail(path, 12, "division 0")
    pos = 8 + hlen
    notes, tempos, dropped, unpaired = [], [], 0, 0
    for trk in range(ntrk):
        if pos + 8 > len(data):
            _fail(path, pos, f"truncated file: track {trk} of {ntrk} is missing")
        if data[pos:pos + 4] != b"MTrk":
            _fail(path, pos, f"chunk tag {data[pos:pos + 4]!r}, MTrk expected")
        ln = struct.unpack(">I", data[pos + 4:pos + 8])[0]
        p, end = pos + 8, pos + 8 + ln
        if end > len(data):
            _fail(path, pos + 4, f"truncated chunk: {ln} bytes declared, {len(data) - p} present")
        pos = end
        tick, status, on = 0, None, {}
        while p < end:
            delta, p = _vlq(data, p, end, path)
            tick += delta
            if p >= end:
                _fail(path, p, "truncated event: a delta time without an event")
            b = data[p]
            if b == 0xFF:
                if p + 2 > end:
                    _fail(path, p, "truncated meta event")
                kind = data[p + 1]
                n, q = _vlq(data, p + 2, end, path)
                if q + n > end:
                    _fail(path, p, f"truncated meta event: {n} bytes declared")
                if kind == 0x51 and n == 3:
                    tempos.append((tick, trk, int.from_bytes(data[q:q + 3], "big")))
                p, status = q + n, None
                if kind == 0x2F:
                    break
                continue
            if b in (0xF0, 0xF7):
                n, q = _vlq(data, p + 1, end, path)
                if q + n > end:
                    _fail(path, p, f"truncated sysex event: {n} bytes declared")
                p, status = q + n, None
                continue
            if b & 0x80:
                if b >= 0xF0:
                    _fail(path, p, f"status byte {b:#x} has no place in a file")
                status = b
                p += 1
            elif status is None:
                _fail(path, p, "data byte without a running status")
            n = _DATA_LEN[status & 0xF0]
            if p + n > end:
                _fail(path, p, "truncated event: data bytes missing")
            kind, ch = status & 0xF0, status & 0x0F
            if kind in (0x80, 0x90):
                pitch, vel = data[p], data[p + 1]
                if data[p] & 0x80 or data[p + 1] & 0x80:
                    _fail(path, p, "a status byte where a data byte belongs")
                if kind == 0x90 and vel:
                    on.setdefault((ch, pitch), []).append((tick, vel))
                else:
                    q_ = on.get((ch, pitch))
                    if q_:
                        t_on, v = q_.pop(0)
                        notes.append((t_on, tick, pitch, v, ch, trk))
            p += n
        for (ch, pitch), q_ in on.items():         # left sounding at the track's end: closed there
            for t_on, v in q_:
                notes.append((t_on, tick, pitch, v, ch, trk))
                unpaired += 1
    if not drums:
        kept = [n for n in notes if n[4] != DRUM_CHANNEL]
        dropped = len(notes) - len(kept)
        notes = kept
    if not notes:
        _fail(path, len(data), "no notes" + (f" ({dropped} on the drum channel left out; --drums keeps them)" if dropped else ""))
    order = sorted(range(len(notes)), key=lambda i: (notes[i][0], notes[i][2], notes[i][5], i))
    arr = np.array([notes[i][:5] for i in order], dtype=np.int64).reshape(-1, 5)
    tempo = min(tempos)[2] if tempos else DEFAULT_TEMPO_US
    return MidiNotes(fmt, div, tempo, arr, dropped, unpaired)


def quantise(ticks, division: int) -> np.ndarray:
    """ticks -> 1/64-beat grid units in integer arithmetic, half to even."""
    num = np.asarray(ticks, np.int64) * GRID
    q, r = np.divmod(num, int(division))
    up = (2 * r > division) | ((2 * r == division) & (q % 2 == 1))
    return q + up.astype(np.int64)


def split_step(step: int):
    """A step above 256 as (the note's step, the rests after it): the note keeps 256 and the remainder becomes rests of at
    most 256 each; a last rest below 7 takes the difference from what stands before it -- a rest, else the note -- so that it
    is exactly 7 and decodes to its own length."""
    if step <= STEP_MAX:
        return step, []
    r = step - STEP_MAX
    rests = [STEP_MAX] * (r // STEP_MAX) + ([r % STEP_MAX] if r % STEP_MAX else [])
    keep = STEP_MAX
    if rests[-1] < STEP_FLOOR:
        need = STEP_FLOOR - rests[-1]
        rests[-1] = STEP_FLOOR
        if len(rests) > 1:
            rests[-2] -= need
        else:
            keep -= need
    return keep, rests


def events_from_notes(notes, division: int):
    """notes (N, >= 4) rows (tick_on, tick_off, pitch, velocity, ..) sorted by tick_on -> (events int32 (E, 4) rows (pitch,
    velocity, dur_q, step_q), info).  step_q = the next onset minus this one on the grid; the last note's step is its duration.
    A rest event is (0, -1, 0, step_q).  The offset in front of the first note is dropped and reported.  Nothing is clamped
    here: what lies outside the contract's ranges is the encode's to clamp and count.  info: {"notes", "events", "rests",
    "lead_q", "length_q" (the sum of all steps), "onset_q" int64 (E,): every event's onset from the first note's}."""
    notes = np.asarray(notes, np.int64)
    if notes.ndim != 2 or notes.shape[1] < 4 or notes.shape[0] < 1 or int(division) < 1:
        raise ValueError("events_from_notes: notes (N >= 1, >= 4) and a positive division expected")
    on, off = quantise(notes[:, 0], division), quantise(notes[:, 1], division)
    if (np.diff(on) < 0).any():
        raise ValueError("events_from_notes: the notes must be sorted by tick_on")
    dur = off - on
    step = np.append(np.diff(on), dur[-1])
    ev = np.stack([notes[:, 2], notes[:, 3], dur, step], axis=1)
    long_ = np.flatnonzero(step > STEP_MAX)
    if long_.size:
        parts, done = [], 0
        for i in long_.tolist():
            keep, rests = split_step(int(step[i]))
            seg = ev[done:i + 1].copy()
            seg[-1, 3] = keep
            parts.append(seg)
            parts.append(np.array([(0, -1, 0, s) for s in rests], np.int64).reshape(-1, 4))
            done = i + 1
        parts.append(ev[done:])
        ev = np.concatenate(parts, axis=0)
    onset = np.concatenate([[0], np.cumsum(ev[:-1, 3])]).astype(np.int64)
    info = {"notes": int(notes.shape[0]), "events": int(ev.shape[0]), "rests": int(ev.shape[0] - notes.shape[0]),
            "lead_q": int(on[0]), "length_q": int(ev[:, 3].sum()), "onset_q": onset}
    return np.ascontiguousarray(ev, dtype=np.int32), info
