"""Skip silence: the host statement of the contract.

Whisper invents text over silence, music beds and dead air, and everything else `transcribe()` has against that acts after the
decoder has run on the quiet stretch.  With `speech` the quiet stretches are found first and cut out: the frames that remain
are packed into a shorter file, the path that exists transcribes the packed file, and `restore` moves every time back to where
it was in the original.  This module is the rule, stated in numpy and in integers; the device (csrc/speech.hip: wm_speech_spans,
wm_mel_gather) must give the same spans and the same packed mel bit for bit, and the CPU tests (tests/test_speech_cpu.py)
exercise this statement.  Nothing here touches the device.

The detector is an ENERGY RULE over the log-mel, not a trained voice-activity model (faster-whisper's `vad_filter` runs Silero
VAD; there is no such model here): a frame counts as speech when its smoothed loudness stands `margin_db` above the file's own
floor, the loudness that `floor_percent` of its frames stay below.  Music, noise and hum above the floor count as speech.

Units: mel frames.  W = 2 * n_audio_ctx frames per window, fs = CHUNK_LENGTH / W seconds per frame (longform.py).  `mel` is the
fp16 log-mel of a whole file, [n_mels, ld], of which the first F <= ld frames are content.

  1. q[t], s[t]   sections.loudness and sections.smooth (sections.py), s over 2h + 1 frames;
  2. floor        sorted(s)[min(F - 1, F * permille // 1000)]: an exact order statistic;
  3. flags        v[t] = (s[t] - floor >= M), M = n_mels * (2h + 1) * step, in 64-bit arithmetic (the difference of two 32-bit
                  sums does not fit 32 bits); one unit of log-mel is 4 units of log10 power = 40 dB and 1024 loudness steps per
                  bin, so step = round(margin_db / 40 * 1024);
  4. spans        (a) the maximal runs of v as [a, b); (b) neighbours whose gap a' - b is < min_silence are joined; (c) spans
                  with b - a < min_speech are dropped; (d) each is widened to [max(0, a - pad), min(F, b + pad)) and spans that
                  now touch or overlap are joined.  Ascending, disjoint, no two touching.  F == 0 or no flag: no spans; every
                  flag set: [0, F);
  5. packed mel   the spans' columns in order, then W copies of the file's last column mel[:, ld - 1] (what
                  sections.section_mel_ref appends, for the same reason).  P = sum(b - a); P_k = the packed start of span k;
  6. restore      a time t (seconds) of the packed file that belongs to span k becomes t + (a_k - P_k) * fs.  Which k: for a
                  segment's start the last k with P_k * fs <= t; for its `seek` the last k with P_k <= seek (integers); for its
                  end the last k with P_k * fs < t (an end on a joint stays with the earlier span); for a word the span of its
                  midpoint under the start rule, for both of its ends (faster-whisper's rule).  k is clamped to [0, K - 1] and
                  nothing else is: a last timestamp beyond the content stays beyond it.

Everything in 1 .. 5 is an integer or a copy, so no result depends on the order of a sum and the device can be held to it exactly.
"""
from __future__ import annotations

import copy
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np

import sections
from longform import CHUNK_LENGTH

STEP_LIMIT = 32768             # step stays at or below it: M = n_mels * (2h + 1) * step < 2^32

Span = Tuple[int, int]


@dataclass(frozen=True)
class SpeechOptions:
    """What counts as speech: a frame whose loudness, smoothed over `smooth_seconds`, stands `margin_db` or more above the
    file's floor -- the loudness that `floor_percent` of the file's frames stay below.  Pauses shorter than
    `min_silence_seconds` stay in, speech shorter than `min_speech_seconds` goes, and what remains keeps `speech_pad_seconds` on
    either side.

    The defaults are PARAMETERS, not measurements: nobody has tuned them on speech (the project has never had a trained
    checkpoint to transcribe with, nor a corpus).  The three durations are faster-whisper's VAD defaults (min_silence_duration_ms
    2000, min_speech_duration_ms 250, speech_pad_ms 400); `margin_db` and `floor_percent` are this project's own and untuned."""
    margin_db: float = 8.0
    floor_percent: float = 10.0
    smooth_seconds: float = 0.2
    min_silence_seconds: float = 2.0
    min_speech_seconds: float = 0.25
    speech_pad_seconds: float = 0.4

    def frames(self, window: int, n_mels: int = 1) -> Tuple[int, int, int, int, int, int]:
        """(h, step, permille, min_silence, min_speech, pad) for a model whose window is `window` = 2 * n_audio_ctx frames;
        ValueError unless 1 <= step <= 32768, 0 <= permille <= 1000, pad >= 0 and n_mels * (2h + 1) < 131072."""
        if window < 1:
            raise ValueError(f"speech: window = {window} frames")
        if not (self.smooth_seconds >= 0 and self.min_silence_seconds >= 0 and self.min_speech_seconds >= 0):
            raise ValueError(f"speech: smooth_seconds={self.smooth_seconds}, min_silence_seconds={self.min_silence_seconds} and "
                             f"min_speech_seconds={self.min_speech_seconds} must not be negative")
        fs = CHUNK_LENGTH / window
        h = round(self.smooth_seconds / fs) // 2
        step = round(self.margin_db / 40 * sections.Q_SCALE)
        permille = round(10 * self.floor_percent)
        min_silence = max(1, round(self.min_silence_seconds / fs))
        min_speech = max(1, round(self.min_speech_seconds / fs))
        pad = round(self.speech_pad_seconds / fs)
        check_frames(h, step, permille, min_silence, min_speech, pad, n_mels)
        return h, step, permille, min_silence, min_speech, pad


def check_frames(h: int, step: int, permille: int, min_silence: int, min_speech: int, pad: int, n_mels: int) -> None:
    if not 1 <= step <= STEP_LIMIT:
        raise ValueError(f"speech: step = {step} must be in 1 .. {STEP_LIMIT} (margin_db)")
    if not 0 <= permille <= 1000:
        raise ValueError(f"speech: permille = {permille} must be in 0 .. 1000 (floor_percent)")
    if pad < 0 or min_silence < 1 or min_speech < 1:
        raise ValueError(f"speech: need pad >= 0, min_silence >= 1 and min_speech >= 1 frames, got {pad}, {min_silence}, {min_speech}")
    if h < 0 or n_mels < 1 or n_mels * (2 * h + 1) >= sections.SUM_LIMIT:
        raise ValueError(f"speech: n_mels * (2h + 1) = {n_mels} * {2 * h + 1} must be below {sections.SUM_LIMIT} (smooth_seconds)")


def floor_of(s: np.ndarray, permille: int) -> int:
    """Rule 2; s must not be empty."""
    F = len(s)
    return int(np.sort(np.asarray(s, dtype=np.int64))[min(F - 1, F * permille // 1000)])


def flags(s: np.ndarray, floor: int, M: int) -> np.ndarray:
    """Rule 3, bool [F]."""
    return np.asarray(s, dtype=np.int64) - np.int64(floor) >= np.int64(M)


def spans_from_flags(v: np.ndarray, min_silence: int, min_speech: int, pad: int) -> List[Span]:
    """Rule 4 over the flags of one file."""
    F = len(v)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], np.asarray(v, dtype=np.int8), [0]]))).tolist()
    runs = list(zip(edges[0::2], edges[1::2]))                                   # (a)
    joined: List[List[int]] = []
    for a, b in runs:                                                            # (b)
        if joined and a - joined[-1][1] < min_silence:
            joined[-1][1] = b
        else:
            joined.append([a, b])
    kept = [(a, b) for a, b in joined if b - a >= min_speech]                    # (c)
    out: List[List[int]] = []
    for a, b in kept:                                                            # (d)
        a, b = max(0, a - pad), min(F, b + pad)
        if out and a <= out[-1][1]:
            out[-1][1] = b
        else:
            out.append([a, b])
    return [(int(a), int(b)) for a, b in out]


def speech_spans_ref(mel: np.ndarray, F: int, h: int, step: int, permille: int, min_silence: int, min_speech: int,
                     pad: int) -> List[Span]:
    """The speech spans of one file, ascending (module docstring, rules 1 .. 4)."""
    n_mels = int(np.asarray(mel).shape[0])
    check_frames(h, step, permille, min_silence, min_speech, pad, n_mels)
    s = sections.smooth(sections.loudness(mel, F), h)
    if F == 0:
        return []
    M = n_mels * (2 * h + 1) * step
    return spans_from_flags(flags(s, floor_of(s, permille), M), min_silence, min_speech, pad)


def packed_starts(spans: Sequence[Span]) -> List[int]:
    """P_k: the packed start of every span, and P itself as the last entry."""
    starts = [0]
    for a, b in spans:
        starts.append(starts[-1] + int(b) - int(a))
    return starts


def check_spans(spans: Sequence[Span], F: int) -> None:
    last = 0
    for k, (a, b) in enumerate(spans):
        if not (last <= a < b <= F) or (k > 0 and a == last):
            raise ValueError(f"speech: spans {list(spans)} must ascend inside [0, {F}] without touching")
        last = b


def taken_spans(spans: Sequence[Span], ld: int) -> List[Span]:
    """What wm_mel_gather takes of a span table it cannot trust (the table comes from device memory): span k is taken if
    0 <= a_k < b_k <= ld and a_k >= b_j for every EARLIER span j that itself lies in that range; every other span is skipped and
    never dereferenced.  The spans taken ascend and are disjoint, so their frames number ld at most.  Spans that rule 4 made are
    all taken."""
    out, high = [], 0
    for a, b in spans:
        if 0 <= a < b <= ld:
            if a >= high:
                out.append((int(a), int(b)))
            high = max(high, b)
    return out


def packed_mel_ref(mel: np.ndarray, F: int, spans: Sequence[Span], W: int) -> np.ndarray:
    """Rule 5: [n_mels, P + W] -- the spans' columns in order, then W copies of the file's last column mel[:, ld - 1]."""
    mel = np.asarray(mel)
    if mel.ndim != 2 or mel.shape[1] < 1 or not 0 <= F <= mel.shape[1]:
        raise ValueError(f"speech: mel {mel.shape} for {F} frames of content")
    check_spans(spans, F)
    return np.concatenate([mel[:, a:b] for a, b in spans] + [np.repeat(mel[:, -1:], W, axis=1)], axis=1)


def _span_of(starts: Sequence, t, strict: bool) -> int:
    """The last k with starts[k] <= t (strict: < t), clamped to [0, K - 1]; starts ascend."""
    k = 0
    for i, p in enumerate(starts):
        if (p < t) if strict else (p <= t):
            k = i
    return k


def restore(segments: Sequence[dict], spans: Sequence[Span], fs: float) -> List[dict]:
    """Rule 6: the segments of a packed file with their times in the original file (a deep copy; the input is not modified).
    `start`, `end`, `seek` and every word's `start` / `end` move; everything else is kept.  A segment whose start (end) was its
    first (last) word's -- where longform.add_word_timestamps had moved it -- takes the restored word's.  Without spans (a file
    with no speech has no segments) nothing moves."""
    out = copy.deepcopy(list(segments))
    if not spans:
        return out
    P = packed_starts(spans)[:-1]
    Pt = [p * fs for p in P]
    shift = [int(a) - p for (a, _), p in zip(spans, P)]
    for s in out:
        words = s.get("words") or []
        from_first = bool(words) and s["start"] == words[0]["start"]
        from_last = bool(words) and s["end"] == words[-1]["end"]
        s["seek"] += shift[_span_of(P, int(s["seek"]), False)]
        s["start"] += shift[_span_of(Pt, s["start"], False)] * fs
        s["end"] += shift[_span_of(Pt, s["end"], True)] * fs
        for w in words:
            move = shift[_span_of(Pt, (w["start"] + w["end"]) / 2, False)] * fs
            w["start"] += move
            w["end"] += move
        if from_first:
            s["start"] = words[0]["start"]
        if from_last:
            s["end"] = words[-1]["end"]
    return out


def restore_time(t: float, spans: Sequence[Span], fs: float, end: bool = False) -> float:
    """One time of the packed file under the start rule (end=True: the end rule); what `restore` does to a segment's bounds."""
    if not spans:
        return t
    P = packed_starts(spans)[:-1]
    k = _span_of([p * fs for p in P], t, end)
    return t + (int(spans[k][0]) - P[k]) * fs
