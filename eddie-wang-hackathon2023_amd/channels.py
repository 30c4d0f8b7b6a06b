"""Channels: the host statement of the contract.

Every other input path ends in a downmix.  A call recorded with one party per channel, or an interview with one microphone per
speaker, loses three things that way: who said what, overlapping speech (summed before the model hears it) and a second
language.  With `channels` a recording's channels are kept apart:

  mode "split"   every channel is transcribed on its own -- the channels take rows of the batch exactly as files do -- and the
                 results are merged by time (rule 6);
  mode "label"   whisper.cpp's `--diarize`: the downmix is transcribed as ever, and every segment (every word, with word
                 timestamps) is given the channel that was loudest while it was spoken (rule 5).

This is the one kind of speaker attribution Whisper can give without a second model: it separates CHANNELS, not speakers inside a
channel, and it compares ABSOLUTE loudness -- nothing matches the channels' levels first.  This module is the rule, stated in
numpy and in integers; the device (csrc/channels.hip: wm_channel_top; csrc/resample.hip: wm_resample_channels) must give the same
`top`, the same counts and the same gated mels bit for bit, and the CPU tests (tests/test_channels_cpu.py) exercise this
statement.  Nothing here touches the device.

Units: mel frames.  W = 2 * n_audio_ctx frames per window, fs = CHUNK_LENGTH / W seconds per frame (longform.py).  A recording
has C channels (1 .. 8); `mel_c` is the fp16 log-mel of channel c, [n_mels, ld], of which the first F <= ld frames are content.

  1. waveforms   channel c of a file of interleaved samples v[k][c] is x_c[k] = fp32(v[k][c]) * scale (scale as in wm_resample:
                 2^-(bits - 1) for integer PCM, 1 for float) filtered by the same polyphase table -- bit for bit what the mono
                 path gives for a mono file that holds that channel; at 16 kHz it is whisper_utils._mono_at_sr of the one column;
  2. loudness    s_c[t] = sections.smooth(sections.loudness(mel_c, F), h), h = round(smooth_seconds / fs) // 2 as
                 speech.SpeechOptions.frames derives it; all channels of a recording have the same F and the same ld;
  3. top         top[t] = the lowest c with s_c[t] = max over c' of s_c'[t], uint8 [F];
                 G = n_mels * (2h + 1) * step, step = round(bleed_db / 40 * 1024) in 1 .. speech.STEP_LIMIT (one unit of log-mel
                 is 40 dB and 1024 loudness steps per bin);
  4. gate        (`bleed_db`, split only: microphones that hear each other)  gated_c[t] = (max over c' != c of s_c'[t]) - s_c[t]
                 >= G in 64-bit arithmetic.  v_c is the smallest finite element of mel_c[:, :F] under the monotone integer key
                 of its fp16 bits (key = bits if bits >= 0 else bits ^ 0x7fff, bits as int16 -- how csrc/frontend.hip orders
                 floats -- so -0 sorts below +0); every bin of a gated frame becomes v_c.  Columns at or beyond F are not
                 touched; a channel without a finite element is never gated; with C = 1 or F = 0 nothing is gated.  No minimum
                 run length, no hysteresis;
  5. label       a span of time [start, end] in seconds covers the frames [a, b), a = max(0, floor(start / fs + EPS)),
                 b = min(F, ceil(end / fs - EPS)) (`span_frames`: EPS = 2^-20 frames keeps a time that IS a frame boundary on
                 it whatever its last bit says); its channel is the one that holds most of top[a:b], the lowest among equals, and
                 None when b <= a.  With `speech` the times are restored into the original file first;
  6. merge       segments = every channel's segments, copied with `channel: c`, sorted by (start, end, channel); turns = one
                 {channel, start, end, text} per maximal run of consecutive merged segments of one channel (start of its first,
                 end of its last, the stripped non-empty texts joined by a blank); text = the turns, one "[c] text" line each;
                 language = that of the first channel that has segments (None if none has).

Everything in 2 .. 5 is an integer or a copy, so no result depends on the order of a sum and the device can be held to it exactly.
The values (`bleed_db`, `smooth_seconds`) are PARAMETERS nobody has tuned on speech.
"""
from __future__ import annotations

import copy
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

import sections
import speech
from longform import CHUNK_LENGTH

MODES = ("split", "label")
MAX_CHANNELS = 8
EPS_FRAMES = 2.0 ** -20
NO_KEY = 0x7f7f7f7f            # the key of a channel without a finite element (every fp16 key lies in [-32768, 32767])


@dataclass(frozen=True)
class ChannelOptions:
    """How the channels of a recording are used (module docstring).  `bleed_db` (split only; None: off) silences a channel's
    frame when another channel is louder there by that much: it is for microphones that hear each other, and it is off by
    default because on a telephone line it would mute the quieter party of an overlap.  The loudness is smoothed over
    `smooth_seconds` first.

    The values are PARAMETERS, not measurements: nobody has tuned them on speech (the project has never had a trained checkpoint
    to transcribe with, nor a corpus)."""
    mode: str = "split"
    bleed_db: Optional[float] = None
    smooth_seconds: float = 0.2

    def check(self) -> "ChannelOptions":
        """ValueError for an unknown mode, bleed_db with "label", a bleed_db that is not finite or whose step leaves
        1 .. speech.STEP_LIMIT, a negative smooth_seconds."""
        if self.mode not in MODES:
            raise ValueError(f"channels: mode {self.mode!r} is not one of {MODES}")
        if not (isinstance(self.smooth_seconds, (int, float)) and math.isfinite(self.smooth_seconds) and self.smooth_seconds >= 0):
            raise ValueError(f"channels: smooth_seconds={self.smooth_seconds} must be finite and not negative")
        if self.bleed_db is not None:
            if self.mode != "split":
                raise ValueError(f"channels: bleed_db gates the channels of mode 'split'; mode {self.mode!r} transcribes the downmix")
            if isinstance(self.bleed_db, bool) or not isinstance(self.bleed_db, (int, float)) or not math.isfinite(self.bleed_db):
                raise ValueError(f"channels: bleed_db={self.bleed_db!r} must be a finite number")
            step = round(self.bleed_db / 40 * sections.Q_SCALE)
            if not 1 <= step <= speech.STEP_LIMIT:
                raise ValueError(f"channels: step = {step} must be in 1 .. {speech.STEP_LIMIT} (bleed_db)")
        return self

    def frames(self, window: int, n_mels: int = 1) -> Tuple[int, int]:
        """(h, step) for a model whose window is `window` = 2 * n_audio_ctx frames; step = 0: no gate.  ValueError as `check`,
        and unless n_mels * (2h + 1) < 131072."""
        self.check()
        if window < 1:
            raise ValueError(f"channels: window = {window} frames")
        fs = CHUNK_LENGTH / window
        h = round(self.smooth_seconds / fs) // 2
        step = 0 if self.bleed_db is None else round(self.bleed_db / 40 * sections.Q_SCALE)
        check_frames(h, step, n_mels)
        return h, step


def check_frames(h: int, step: int, n_mels: int) -> None:
    if not 0 <= step <= speech.STEP_LIMIT:
        raise ValueError(f"channels: step = {step} must be in 1 .. {speech.STEP_LIMIT} (0: no gate)")
    if h < 0 or n_mels < 1 or n_mels * (2 * h + 1) >= sections.SUM_LIMIT:
        raise ValueError(f"channels: n_mels * (2h + 1) = {n_mels} * {2 * h + 1} must be below {sections.SUM_LIMIT} (smooth_seconds)")


# ------------------------------------------------------------------------------------------------------------------- rule 1
def channel_waveform_ref(samples: np.ndarray, c: int, bits: Optional[int], rate: int, sr: int = 16000) -> np.ndarray:
    """Rule 1 on the host: channel c of samples [n, C] at `rate` Hz as a waveform at `sr` Hz -- at `sr` the fp32 column over
    2^(bits - 1), otherwise whisper_utils.resample_reference (fp64) of the scaled column."""
    import whisper_utils as wu
    col = np.asarray(samples).reshape(len(samples), -1)[:, c:c + 1]
    if rate == sr:
        return wu._mono_at_sr(col, bits)
    return wu.resample_reference(wu.downmix(col, bits), rate, sr)


# -------------------------------------------------------------------------------------------------------------- rules 2 .. 4
def smoothed(mels: Sequence[np.ndarray], F: int, h: int) -> np.ndarray:
    """Rule 2: s, int64 [C, F]."""
    mels = _recording(mels, F)
    return np.stack([sections.smooth(sections.loudness(m, F), h) for m in mels]).reshape(len(mels), F)


def _recording(mels: Sequence[np.ndarray], F: int) -> List[np.ndarray]:
    mels = [np.asarray(m) for m in mels]
    if not 1 <= len(mels) <= MAX_CHANNELS:
        raise ValueError(f"channels: {len(mels)} channels (1 .. {MAX_CHANNELS})")
    for m in mels:
        if m.dtype != np.float16 or m.ndim != 2 or m.shape != mels[0].shape or not 0 <= F <= m.shape[1]:
            raise ValueError(f"channels: every channel must be fp16 [n_mels, ld] of one shape with 0 <= F <= ld, got {m.dtype} "
                             f"{m.shape} beside {mels[0].shape}, F={F}")
    return mels


def top_channel(s: np.ndarray) -> np.ndarray:
    """Rule 3: uint8 [F], the lowest channel among the loudest."""
    s = np.asarray(s, dtype=np.int64)
    return np.argmax(s, axis=0).astype(np.uint8) if s.shape[1] else np.zeros(0, dtype=np.uint8)


def gate_threshold(n_mels: int, h: int, step: int) -> int:
    """G of rule 3."""
    return int(n_mels) * (2 * int(h) + 1) * int(step)


def gated_frames(s: np.ndarray, G: int) -> np.ndarray:
    """Rule 4's flags, bool [C, F], before the channels without a finite element are taken out."""
    s = np.asarray(s, dtype=np.int64)
    C, F = s.shape
    out = np.zeros((C, F), dtype=bool)
    for c in range(C):
        others = np.delete(s, c, axis=0)
        if others.shape[0] and F:
            out[c] = others.max(axis=0) - s[c] >= np.int64(G)
    return out


def fp16_key(x: np.ndarray) -> np.ndarray:
    """The monotone integer key of fp16 values (int32): the bits as int16, negative ones with their low 15 bits flipped."""
    b = np.asarray(x, dtype=np.float16).view(np.int16).astype(np.int32)
    return np.where(b >= 0, b, b ^ 0x7fff)


def quietest(mel: np.ndarray, F: int):
    """v_c of rule 4: (the fp16 value, its key), or (None, NO_KEY) for a channel without a finite element in mel[:, :F]."""
    x = np.asarray(mel)[:, :F]
    finite = np.isfinite(x.astype(np.float32))
    if not finite.any():
        return None, NO_KEY
    keys = fp16_key(x)[finite]
    values = x[finite]
    i = int(np.argmin(keys))
    return values[i], int(keys[i])


def channel_top_ref(mels: Sequence[np.ndarray], F: int, h: int, step: int = 0):
    """Rules 2 .. 4 over one recording: (top uint8 [F], gated counts int [C], the mels after the gate -- copies; the inputs are
    not modified).  step = 0: no gate, the counts are zero and the mels equal the inputs."""
    mels = _recording(mels, F)
    n_mels = mels[0].shape[0]
    check_frames(h, step, n_mels)
    s = smoothed(mels, F, h)
    top = top_channel(s)
    out = [m.copy() for m in mels]
    counts = [0] * len(mels)
    if step > 0:
        flags = gated_frames(s, gate_threshold(n_mels, h, step))
        for c, m in enumerate(out):
            v, _ = quietest(mels[c], F)
            if v is None:
                continue
            counts[c] = int(flags[c].sum())
            m[:, :F][:, flags[c]] = v
    return top, counts, out


def run_lengths(top: np.ndarray) -> List[List[int]]:
    """`top` as [[channel, frames], ...] (what the results carry as `channel_top`)."""
    top = np.asarray(top).reshape(-1)
    if len(top) == 0:
        return []
    edges = np.flatnonzero(np.diff(top.astype(np.int64))) + 1
    starts = np.concatenate([[0], edges])
    ends = np.concatenate([edges, [len(top)]])
    return [[int(top[a]), int(b - a)] for a, b in zip(starts, ends)]


def from_run_lengths(runs: Sequence[Sequence[int]]) -> np.ndarray:
    return np.concatenate([np.full(int(n), int(c), dtype=np.uint8) for c, n in runs] + [np.zeros(0, dtype=np.uint8)])


# ------------------------------------------------------------------------------------------------------------------- rule 5
def span_frames(start: float, end: float, fs: float, F: int) -> Tuple[int, int]:
    """The frames [a, b) of the span of time [start, end] seconds (rule 5); b <= a: none."""
    a = max(0, math.floor(start / fs + EPS_FRAMES))
    b = min(int(F), math.ceil(end / fs - EPS_FRAMES))
    return int(a), int(b)


def label_span(top: np.ndarray, start: float, end: float, fs: float, n_channels: int = MAX_CHANNELS) -> Optional[int]:
    """Rule 5: the channel of a span of time, None for a span without frames."""
    top = np.asarray(top).reshape(-1)
    a, b = span_frames(start, end, fs, len(top))
    if b <= a:
        return None
    return int(np.argmax(np.bincount(top[a:b], minlength=n_channels)))


def label_segments(segments: Sequence[dict], top: np.ndarray, fs: float, n_channels: int = MAX_CHANNELS) -> List[dict]:
    """The segments (a deep copy) with `channel` on every segment and on every word."""
    out = copy.deepcopy(list(segments))
    for s in out:
        s["channel"] = label_span(top, s["start"], s["end"], fs, n_channels)
        for w in s.get("words", ()):
            w["channel"] = label_span(top, w["start"], w["end"], fs, n_channels)
    return out


# ------------------------------------------------------------------------------------------------------------------- rule 6
def merge_channels(results: Sequence[dict]) -> dict:
    """Rule 6: the result of one recording from its channels' results (which are kept, as `channels`; nothing is modified)."""
    merged = []
    for c, r in enumerate(results):
        for s in r["segments"]:
            s = copy.deepcopy(s)
            s["channel"] = c
            merged.append(s)
    merged.sort(key=lambda s: (s["start"], s["end"], s["channel"]))
    turns: List[dict] = []
    for s in merged:
        text = s["text"].strip()
        if turns and turns[-1]["channel"] == s["channel"]:
            turns[-1]["end"] = s["end"]
            if text:
                turns[-1]["text"] = (turns[-1]["text"] + " " + text).strip()
        else:
            turns.append(dict(channel=s["channel"], start=s["start"], end=s["end"], text=text))
    language = next((r["language"] for r in results if r["segments"]), None)
    return dict(language=language, text="\n".join(f"[{t['channel']}] {t['text']}" for t in turns), segments=merged, turns=turns,
                channels=list(results))
