"""Parallel sections: the host statement of the contract.

`transcribe()` is sequential per file and batched across files, so one long recording is decoded at the batch-1 operating
point.  With `sections` a file is cut where it is quietest and the pieces are decoded side by side, as rows of the schedule that
exists (longform.transcribe_batched): every section is a "file" of its own, and `merge_sections` puts their results back
together.  This module is the rule for the cuts, stated in numpy and in integers; the device (csrc/sections.hip,
wm_section_cuts) must give the same cuts bit for bit, and the CPU tests (tests/test_sections_cpu.py) exercise this statement.
Nothing here touches the device.

Units: mel frames.  W = 2 * n_audio_ctx frames per window, fs = CHUNK_LENGTH / W seconds per frame (longform.py).  `mel` is the
fp16 log-mel of a whole file, [n_mels, ld], of which the first F <= ld frames are content.

  loudness   q[t] = sum over m of rint(clamp(float(mel[m, t]), -16, 16) * 1024), an integer (rint: half to even; an element that
             is not finite contributes 0), t in [0, F);
  smoothing  s[t] = sum over d in [-h, h] of q[clamp(t + d, 0, F - 1)];
  cuts       c = 0; while F - c > hi: the next cut is the t in [c + lo, c + hi] with the smallest s[t], the LARGEST such t among
             equal minima; c = t.

The sections are [c_i, c_{i+1}) and the last one [c_k, F): every section but the last has lo .. hi frames, the last 1 .. hi (it
may be shorter than lo).  F <= hi: one section, no cut; F == 0: no section.  Everything is an integer -- an fp16 value times
1024 is exact in fp32, |a term| <= 16384, and n_mels * (2h + 1) < 131072 keeps every sum inside 32 bits -- so no result depends
on the order of a sum and the device can be held to the exact cuts.

Difference from upstream: sections run side by side, so nothing crosses a cut -- `condition_on_previous_text` keeps its history
per section, and a timestamp or a word never reaches into the next section.
"""
from __future__ import annotations

import copy
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from longform import CHUNK_LENGTH

Q_SCALE = 1024                 # loudness steps per unit of log-mel
Q_CLAMP = 16.0                 # |log-mel| beyond this counts as this
SUM_LIMIT = 131072             # n_mels * (2h + 1) stays below it: 16384 * 131071 < 2^31


@dataclass(frozen=True)
class SectionOptions:
    """Where a file may be cut: a section is at most `max_seconds` and (but for a file's last) at least `min_seconds` long
    (None: half of max_seconds), and the loudness is smoothed over `smooth_seconds` before the quietest frame is looked for.

    The defaults are PARAMETERS, not measurements: nobody has tuned them on speech (the project has never had a trained
    checkpoint to transcribe with); 30 s is the decoder's window, so a default section is decoded in one or two windows."""
    max_seconds: float = 30.0
    min_seconds: Optional[float] = None
    smooth_seconds: float = 0.2

    def frames(self, window: int, n_mels: int = 1) -> Tuple[int, int, int]:
        """(lo, hi, h) in frames of a model whose window is `window` = 2 * n_audio_ctx frames; ValueError unless
        1 <= lo <= hi and n_mels * (2h + 1) < 131072.  hi may exceed the window: such a section seeks inside itself."""
        if window < 1:
            raise ValueError(f"sections: window = {window} frames")
        fs = CHUNK_LENGTH / window
        min_seconds = self.max_seconds / 2 if self.min_seconds is None else self.min_seconds
        if not (self.max_seconds > 0 and min_seconds >= 0 and self.smooth_seconds >= 0):
            raise ValueError(f"sections: max_seconds={self.max_seconds} must be positive, min_seconds={min_seconds} and "
                             f"smooth_seconds={self.smooth_seconds} not negative")
        hi, lo, h = round(self.max_seconds / fs), round(min_seconds / fs), round(self.smooth_seconds / fs) // 2
        check_frames(lo, hi, h, n_mels)
        return lo, hi, h


def check_frames(lo: int, hi: int, h: int, n_mels: int) -> None:
    if not 1 <= lo <= hi:
        raise ValueError(f"sections: need 1 <= lo <= hi frames, got lo={lo} hi={hi} (min_seconds / max_seconds)")
    if h < 0 or n_mels < 1 or n_mels * (2 * h + 1) >= SUM_LIMIT:
        raise ValueError(f"sections: n_mels * (2h + 1) = {n_mels} * {2 * h + 1} must be below {SUM_LIMIT} (smooth_seconds)")


def _content(mel: np.ndarray, F: int) -> np.ndarray:
    mel = np.asarray(mel)
    if mel.dtype != np.float16 or mel.ndim != 2 or not 0 <= F <= mel.shape[1]:
        raise ValueError(f"sections: mel must be fp16 [n_mels, ld] with 0 <= F <= ld, got {mel.dtype} {mel.shape}, F={F}")
    return mel[:, :F]


def loudness(mel: np.ndarray, F: int) -> np.ndarray:
    """q, int64 [F]."""
    x = _content(mel, F).astype(np.float32)
    finite = np.isfinite(x)
    x = np.clip(np.where(finite, x, np.float32(0)), -Q_CLAMP, Q_CLAMP) * np.float32(Q_SCALE)
    return np.rint(x).astype(np.int64).sum(axis=0)


def smooth(q: np.ndarray, h: int) -> np.ndarray:
    """s, int64 [F]: the sum of the 2h + 1 neighbours, the ends repeated."""
    F = len(q)
    if F == 0:
        return np.zeros(0, dtype=np.int64)
    t = np.arange(F)
    s = np.zeros(F, dtype=np.int64)
    for d in range(-h, h + 1):
        s += q[np.clip(t + d, 0, F - 1)]
    return s


def cuts_from_smoothed(s: np.ndarray, lo: int, hi: int) -> List[int]:
    F, c, cuts = len(s), 0, []
    while F - c > hi:
        piece = s[c + lo: c + hi + 1]
        c = c + lo + (len(piece) - 1 - int(np.argmin(piece[::-1])))          # the last of the equal minima
        cuts.append(c)
    return cuts


def section_cuts_ref(mel: np.ndarray, F: int, lo: int, hi: int, h: int) -> List[int]:
    """The interior cuts of one file, ascending (module docstring)."""
    check_frames(lo, hi, h, int(np.asarray(mel).shape[0]))
    return cuts_from_smoothed(smooth(loudness(mel, F), h), lo, hi)


def section_bounds(F: int, cuts: Sequence[int]) -> List[Tuple[int, int]]:
    """[(a, b)]: the sections [a, b) of a file of F frames cut at `cuts`; none for F == 0."""
    if F <= 0:
        return []
    edges = [0] + [int(c) for c in cuts] + [int(F)]
    if any(b <= a for a, b in zip(edges, edges[1:])):
        raise ValueError(f"sections: cuts {list(cuts)} do not ascend inside (0, {F})")
    return list(zip(edges[:-1], edges[1:]))


def section_mel_ref(mel: np.ndarray, F: int, a: int, b: int, W: int) -> np.ndarray:
    """The mel of the section [a, b) as transcribe_mel wants a file's mel, [n_mels, b - a + W]: mel[:, a:b] followed by W frames
    that are copies of the file's last column mel[:, ld - 1] -- the value the front end gives digital silence, which is what the
    W padding frames of a whole-file mel end in.  For the last section of a file with ld == F + W this is mel[:, a:]."""
    mel = np.asarray(mel)
    if not 0 <= a < b <= F <= mel.shape[1]:
        raise ValueError(f"sections: section [{a}, {b}) of {F} frames (ld {mel.shape[1]})")
    return np.concatenate([mel[:, a:b], np.repeat(mel[:, -1:], W, axis=1)], axis=1)


def merge_sections(results: Sequence[Sequence[dict]], starts: Sequence[int], fs: float) -> List[dict]:
    """One file's segments from its sections': results[i] are the segments of the section that begins at frame starts[i], in
    section order.  `start`, `end` and every word's `start` / `end` move by starts[i] * fs seconds, `seek` by starts[i] frames;
    everything else is kept (the inputs are not modified).  The file's text is the decode of the merged segments' tokens."""
    if len(results) != len(starts):
        raise ValueError(f"sections: {len(results)} results for {len(starts)} sections")
    merged: List[dict] = []
    for segments, start in zip(results, starts):
        shift = int(start) * fs
        for s in segments:
            s = copy.deepcopy(s)
            s["seek"] += int(start)
            s["start"] += shift
            s["end"] += shift
            for w in s.get("words", ()):
                w["start"] += shift
                w["end"] += shift
            merged.append(s)
    return merged


class SectionLanguages:
    """One language per file, shared by its sections (transcribe.py keeps every file's language here, sectioned or not).

    `owner[i]`: the file that "file" i of the schedule is a section of (None: every file is its own); the sections of a file stand
    together, in section order.  `initial`: the language every file starts with -- the one the options name, or None: then it is
    detected on the first window of the file's FIRST section and no other section ever detects.  The schedule hands rows out in
    order, so a file's first section runs no later than the others; a section that asks before it is an error."""

    def __init__(self, n: int, owner: Optional[Sequence[int]], initial: Optional[str]):
        self.group = list(range(n)) if owner is None else [int(o) for o in owner]
        if len(self.group) != n or any(b < a for a, b in zip(self.group, self.group[1:])):
            raise ValueError(f"sections: owners {self.group} for {n} sections must ascend")
        self.leads = [i == 0 or self.group[i] != self.group[i - 1] for i in range(n)]
        self.language: List[Optional[str]] = [initial] * (max(self.group) + 1 if n else 0)

    def fresh(self, rows: Sequence[Optional[Tuple[int, int]]]) -> List[int]:
        """The rows (indices into `rows`, entries (file, seek) or None) whose window decides a language this round."""
        return [i for i, r in enumerate(rows) if r is not None and self.leads[r[0]] and self.language[self.group[r[0]]] is None]

    def detected(self, i: int, language: str) -> None:
        self.language[self.group[i]] = language

    def of(self, i: int) -> Optional[str]:
        return self.language[self.group[i]]

    def known(self, i: int) -> str:
        language = self.of(i)
        if language is None:
            raise RuntimeError(f"sections: section {i} of file {self.group[i]} is decoded before the file's first section")
        return language
