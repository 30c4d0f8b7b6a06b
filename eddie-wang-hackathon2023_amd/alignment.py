"""Forced alignment: the host statement of the contract.

The caller HAS the text; the question is when each word of it was spoken, in a file of any length.  A 30-second window of a long
file holds an unknown prefix of the words still to place, so three rules are added to the word-timestamp contract of timing.py:

  window  the forced sequence of a window is  sot_sequence + <|notimestamps|> + whole words while their tokens fit `max_tokens`
          + <|endoftext|>  (`plan_window`);
  walk    dynamic time warping with an OPEN END on the token axis (`dtw_open_cpu`): timing.dtw_cpu's cost table, cell for cell, but
          the walk back starts at (i*, M), i* the smallest row whose cost in the last column is that column's minimum.  `end_row` =
          i* says how many rows of the matrix the path entered.  The costs are not normalised by the path's length;
  accept  (`accept_words`) word w, whose tokens are rows b_w .. b_{w+1} - 1, is PLACED iff the path entered row b_{w+1} -- the row of
          the token after it: b_{w+1} <= end_row - 1 -- and, unless this is the file's last window, it entered that row at a frame
          <= F - 1 - round(edge_seconds / seconds_per_frame): a word that ends at the window's edge is probably cut by it.  Its start
          and end are the jump times of rows b_w and b_{w+1}, exactly as timing.words_from_path reads them.  Placement stops at the
          first word that fails;
  seek    (`next_seek`) the next window starts at the end of the last word placed (the rule long-form transcription uses with word
          timestamps); a window that places no word is skipped whole (silence, music).  The seek always grows: a last word that
          ends in the window's first frame still moves it by one alignment frame.  A file ends when its words are placed or its
          audio is used up; the words left over come back unplaced: start = end = the file's duration, probability 0,
          aligned = False.

`align_reference` is the literal loop over one file; the device schedule (forced_align.py behind transcribe.align) runs the current
window of every unfinished file as one batch and is held to it: replaying the device's matrices through this module must give the
device's end rows, paths, words and seeks exactly.

`max_tokens` and `edge_seconds` are PARAMETERS, not measurements: nobody has tuned them on speech, and the same holds for the
un-normalised open end.  Out of scope: an open beginning (the text must start where the audio's speech starts), text in the middle
that the audio does not contain, and any claim about accuracy.

Pure numpy / python: nothing here touches a GPU.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

import timing

N_TEXT_CTX = 448           # of every Whisper model


@dataclass(frozen=True)
class AlignOptions:
    """max_tokens: text tokens forced on one window, 1 .. n_text_ctx - len(sot_sequence) - 2.  Construction knows no model and holds
    it to the most any Whisper model allows (448 - 1 - 2 = 445, an English-only model's one-token sot_sequence); `check` holds it to
    the model it is used with (443 for a multilingual one).  edge_seconds: 0 .. 15.  Both defaults are parameters nobody has tuned."""
    max_tokens: int = 128
    edge_seconds: float = 0.5

    def __post_init__(self):
        if isinstance(self.max_tokens, bool) or not isinstance(self.max_tokens, (int, np.integer)) or not 1 <= int(self.max_tokens) <= N_TEXT_CTX - 3:
            raise ValueError(f"AlignOptions: max_tokens = {self.max_tokens!r} must be an integer in 1 .. {N_TEXT_CTX - 3}")
        e = self.edge_seconds
        if isinstance(e, bool) or not isinstance(e, (int, float, np.integer, np.floating)) or not (0.0 <= float(e) <= 15.0):
            raise ValueError(f"AlignOptions: edge_seconds = {e!r} must lie in 0 .. 15")

    def check(self, n_text_ctx: int, n_sot: int) -> "AlignOptions":
        """Against a model: max_tokens <= n_text_ctx - len(sot_sequence) - 2."""
        top = int(n_text_ctx) - int(n_sot) - 2
        if not 1 <= int(self.max_tokens) <= top:
            raise ValueError(f"AlignOptions: max_tokens = {self.max_tokens} must lie in 1 .. n_text_ctx - len(sot_sequence) - 2 = {top}")
        return self

    def edge_frames(self, seconds_per_frame: float) -> int:
        return int(round(float(self.edge_seconds) / float(seconds_per_frame)))


@dataclass
class AlignedWord(timing.WordTiming):
    aligned: bool = True
    line: int = 0


@dataclass
class WindowPlan:
    forced: List[int]              # sot_sequence + <|notimestamps|> + text + <|endoftext|>
    n_words: int                   # words of the remaining ones that the window forces
    boundaries: List[int]          # b_0 = 0 < b_1 < ... < b_n_words = text tokens of the window


@dataclass
class WindowRecord:
    """What one window of one file did (the schedule's trace; the device side fills the same fields)."""
    seek: int                      # mel frames
    n_frames: int                  # F: alignment frames of real audio in the window
    last: bool
    first_word: int
    plan: WindowPlan
    end_row: int
    path_text: np.ndarray
    path_time: np.ndarray
    placed: int
    next_seek: int


# ---- the walk -------------------------------------------------------------------------------------------------------------------
def dtw_open_cpu(x: np.ndarray) -> Tuple[np.ndarray, np.ndarray, int]:
    """timing.dtw_cpu with an open end on the token axis: (text_indices, time_indices, end_row) of the cheapest monotone path from
    (0, 0) to (end_row - 1, M - 1), end_row = i* = the smallest i in 1 .. N with cost[i, M] <= cost[k, M] for every k in 1 .. N (fp32
    compares).  N < 1 or M < 1: empty paths and end_row 0.  The table and the trace codes are dtw_cpu's, cell for cell."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError(f"dtw_open_cpu: a matrix is expected, not shape {x.shape}")
    N, M = x.shape
    if N < 1 or M < 1:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 0
    cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    trace = np.full((N + 1, M + 1), -1, dtype=np.int8)
    cost[0, 0] = 0
    for d in range(2, N + M + 1):
        i = np.arange(max(1, d - M), min(N, d - 1) + 1)
        j = d - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        t0 = (c0 < c1) & (c0 < c2)
        t1 = ~t0 & (c1 < c0) & (c1 < c2)
        c = np.where(t0, c0, np.where(t1, c1, c2))
        cost[i, j] = x[i - 1, j - 1] + c
        trace[i, j] = np.where(t0, 0, np.where(t1, 1, 2))
    trace[0, :] = 2
    trace[:, 0] = 1
    end_row = 1
    for k in range(2, N + 1):                      # the smallest row among the minima: a later row must be strictly cheaper
        if cost[k, M] < cost[end_row, M]:
            end_row = k
    i, j = end_row, M
    text, time = [], []
    while i > 0 or j > 0:
        text.append(i - 1)
        time.append(j - 1)
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return np.array(text[::-1], dtype=np.int64), np.array(time[::-1], dtype=np.int64), int(end_row)


# ---- the window rule ------------------------------------------------------------------------------------------------------------
def check_words(word_tokens: Sequence[Sequence[int]], max_tokens: int) -> None:
    for k, toks in enumerate(word_tokens):
        if len(toks) < 1:
            raise ValueError(f"alignment: word {k} has no tokens")
        if len(toks) > max_tokens:
            raise ValueError(f"alignment: word {k} has {len(toks)} tokens, more than max_tokens = {max_tokens}")


def plan_window(word_tokens: Sequence[Sequence[int]], sot_sequence: Sequence[int], no_timestamps: int, eot: int,
                max_tokens: int) -> WindowPlan:
    """The forced sequence of a window over the words still to place (their token lists, Tokenizer.split_to_word_tokens): whole
    words while their tokens fit `max_tokens`.  A first word longer than max_tokens raises ValueError."""
    if not word_tokens:
        raise ValueError("alignment: a window needs at least one word to place")
    text, bounds = [], [0]
    for toks in word_tokens:
        if len(text) + len(toks) > max_tokens:
            break
        text += [int(t) for t in toks]
        bounds.append(len(text))
    if len(bounds) == 1:
        raise ValueError(f"alignment: a word of {len(word_tokens[0])} tokens is longer than max_tokens = {max_tokens}")
    return WindowPlan(list(sot_sequence) + [int(no_timestamps)] + text + [int(eot)], len(bounds) - 1, bounds)


# ---- the accept rule ------------------------------------------------------------------------------------------------------------
def jump_frames(text_indices, time_indices) -> np.ndarray:
    """The frame at which the path enters each row it visits, in row order (timing.words_from_path's jump times, as frames)."""
    text_indices, time_indices = np.asarray(text_indices), np.asarray(time_indices)
    if text_indices.size == 0:
        return np.zeros(0, dtype=np.int64)
    jumps = np.concatenate([[True], np.diff(text_indices) != 0])
    return time_indices[jumps].astype(np.int64)


def accept_words(text_indices, time_indices, end_row: int, boundaries: Sequence[int], n_frames: int, last_window: bool,
                 edge_frames: int) -> Tuple[int, List[Tuple[int, int]]]:
    """(number of words placed, [(start frame, end frame)] of each): the accept rule of the module docstring.  `boundaries`: b_0 = 0 <
    b_1 < ... (cumulative token counts of the window's words); the matrix has boundaries[-1] + 1 rows (the last is <|endoftext|>'s)."""
    jf = jump_frames(text_indices, time_indices)
    assert len(jf) == end_row, "a monotone path from row 0 enters every row up to its end"
    limit = int(n_frames) - 1 - int(edge_frames)
    out = []
    for w in range(len(boundaries) - 1):
        nxt = int(boundaries[w + 1])
        if nxt > end_row - 1:
            break
        if not last_window and int(jf[nxt]) > limit:
            break
        out.append((int(jf[int(boundaries[w])]), int(jf[nxt])))
    return len(out), out


# ---- the seek rule --------------------------------------------------------------------------------------------------------------
def next_seek(seek: int, window: int, spans: Sequence[Tuple[int, int]]) -> int:
    """Mel frames (two per alignment frame).  No word placed: the window is skipped whole; else the end of the last word placed, and
    at least one alignment frame on."""
    if not spans:
        return int(seek) + int(window)
    return max(int(seek) + 2 * int(spans[-1][1]), int(seek) + 2)


def window_frames(seek: int, window: int, content_frames: int) -> Tuple[int, bool]:
    """(F: alignment frames of real audio in the window at `seek`, whether it is the file's last window)."""
    return max(0, min(int(window), int(content_frames) - int(seek))) // 2, int(seek) + int(window) >= int(content_frames)


# ---- one file, literally --------------------------------------------------------------------------------------------------------
def settle_window(words: Sequence[str], word_tokens: Sequence[Sequence[int]], lines: Sequence[int], first_word: int, plan: WindowPlan,
                  text_indices, time_indices, end_row: int, token_probs: Sequence[float], seek: int, n_frames: int, last: bool,
                  window: int, seconds_per_frame: float, options: AlignOptions) -> Tuple[List[AlignedWord], int]:
    """The words a window places (with file times) and the file's next seek, from the window's path.  token_probs: the forced pass's
    probability of every text token of the window."""
    n, spans = accept_words(text_indices, time_indices, end_row, plan.boundaries, n_frames, last, options.edge_frames(seconds_per_frame))
    probs = np.asarray(token_probs, dtype=np.float64)
    t0 = seek * (seconds_per_frame / 2.0)
    out = []
    for w, (a, b) in enumerate(spans):
        lo, hi = plan.boundaries[w], plan.boundaries[w + 1]
        k = first_word + w
        out.append(AlignedWord(words[k], [int(t) for t in word_tokens[k]], float(t0 + a * seconds_per_frame), float(t0 + b * seconds_per_frame),
                               float(probs[lo:hi].mean()), True, int(lines[k])))
    return out, next_seek(seek, window, spans)


def leftover_words(words, word_tokens, lines, first_word: int, duration: float) -> List[AlignedWord]:
    return [AlignedWord(words[k], [int(t) for t in word_tokens[k]], float(duration), float(duration), 0.0, False, int(lines[k]))
            for k in range(first_word, len(words))]


MatrixSource = Callable[[int, List[int], int], Tuple[np.ndarray, Sequence[float]]]


def align_reference(source: MatrixSource, words: Sequence[str], word_tokens: Sequence[Sequence[int]], lines: Sequence[int],
                    content_frames: int, *, window: int, seconds_per_frame: float, sot_sequence: Sequence[int], no_timestamps: int,
                    eot: int, options: AlignOptions = AlignOptions(), records: Optional[List[WindowRecord]] = None) -> List[AlignedWord]:
    """The literal loop over ONE file.  source(seek, forced tokens, F) -> (the alignment matrix fp32 [text tokens + 1, >= F], the
    probability of every text token) for the window at mel frame `seek`.  Returns every word exactly once and in order (before
    the punctuation merge: `finish_words`)."""
    check_words(word_tokens, options.max_tokens)
    out: List[AlignedWord] = []
    seek, k = 0, 0
    while k < len(words) and seek < content_frames:
        F, last = window_frames(seek, window, content_frames)
        if F < 1:
            break
        plan = plan_window(word_tokens[k:], sot_sequence, no_timestamps, eot, options.max_tokens)
        matrix, probs = source(seek, plan.forced, F)
        n_rows = plan.boundaries[-1] + 1
        pt, pf, end_row = dtw_open_cpu(-np.asarray(matrix, dtype=np.float32)[:n_rows, :F])
        placed, new_seek = settle_window(words, word_tokens, lines, k, plan, pt, pf, end_row, probs, seek, F, last, window,
                                         seconds_per_frame, options)
        if records is not None:
            records.append(WindowRecord(seek, F, last, k, plan, end_row, pt, pf, len(placed), new_seek))
        assert new_seek > seek
        out += placed
        k += len(placed)
        seek = new_seek
    return out + leftover_words(words, word_tokens, lines, k, content_frames * (seconds_per_frame / 2.0))


# ---- texts and results ----------------------------------------------------------------------------------------------------------
def split_text(tokenizer, text, language: Optional[str]) -> Tuple[List[str], List[str], List[List[int]], List[int]]:
    """(the lines, words, word tokens, the line of every word) of a text: a string (one line) or a list of strings.  Every line is
    encoded as " " + line.strip() -- Whisper's text starts with a space -- and split by Tokenizer.split_to_word_tokens."""
    if isinstance(text, str):
        lines = [text]
    elif isinstance(text, (list, tuple)) and all(isinstance(t, str) for t in text):
        lines = list(text)
    else:
        raise ValueError("align: a text is a string or a list of strings (lines)")
    words, toks, owner = [], [], []
    for li, line in enumerate(lines):
        if not line.strip():
            continue
        ids = [t for t in tokenizer.encode(" " + line.strip()) if t < tokenizer.eot]
        w, wt = tokenizer.split_to_word_tokens(ids, language=language)
        for a, b in zip(w, wt):
            if len(b):
                words.append(a); toks.append([int(t) for t in b]); owner.append(li)
    return lines, words, toks, owner


def finish_words(placed: Sequence[AlignedWord], n_lines: int) -> List[List[AlignedWord]]:
    """Per line, the words after timing.merge_punctuations (times are not touched, as upstream; an absorbed mark disappears)."""
    per_line: List[List[AlignedWord]] = [[] for _ in range(n_lines)]
    for w in placed:
        per_line[w.line].append(AlignedWord(w.word, list(w.tokens), w.start, w.end, w.probability, w.aligned, w.line))
    for ws in per_line:
        timing.merge_punctuations(ws)
    return [[w for w in ws if w.word] for ws in per_line]


def word_dict(w: AlignedWord) -> dict:
    return dict(word=w.word, start=w.start, end=w.end, probability=w.probability, aligned=w.aligned)


def file_result(language: Optional[str], lines: Sequence[str], placed: Sequence[AlignedWord], duration: float) -> dict:
    """language, text, words, segments (one per given line): a segment's start and end are those of its placed words; with none placed
    it is aligned = False at the file's duration.  A text without a non-blank line gives an empty result: no words, no segments."""
    if not any(l.strip() for l in lines):
        return dict(language=language, text="", words=[], segments=[])
    per_line = finish_words(placed, len(lines))
    segments, all_words = [], []
    for line, ws in zip(lines, per_line):
        on = [w for w in ws if w.aligned]
        segments.append(dict(text=line.strip(), start=on[0].start if on else float(duration), end=on[-1].end if on else float(duration),
                             aligned=bool(on), words=[word_dict(w) for w in ws]))
        all_words += [word_dict(w) for w in ws]
    return dict(language=language, text=" ".join(l.strip() for l in lines if l.strip()), words=all_words, segments=segments)
