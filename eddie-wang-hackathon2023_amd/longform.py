"""Long-form transcription: the host statement of the contract.

Upstream Whisper's `transcribe()`, restated: a window of 30 seconds moves over the audio; where it goes next is read off the
timestamp tokens the decoder predicted (`cut_segments`), and a window whose text looks degenerate is decoded again at the next
temperature of a ladder (`needs_fallback`).  `transcribe_reference` is that loop for one file, literally; `transcribe_batched`
is the schedule the engine runs -- sequential per file, batched across files: every round decodes the current window of every
unfinished file -- and must give every file the segments of the literal loop.

Nothing here touches the device: the decoder is a callable handed in, so the rules and the scheduler are tested on the CPU
with scripted decoders (tests/test_longform_cpu.py).  A decoder's result is anything with the fields of `DecodingResult`
that the rules read: tokens, avg_logprob, no_speech_prob, compression_ratio, temperature.

Units: everything is in mel frames.  W = 2 * n_audio_ctx frames per window (3000), fs = CHUNK_LENGTH / W seconds per frame;
the timestamp token tb + k means k * 2 * fs seconds, 2 * k frames.

One deliberate difference from upstream: an advance that is <= 0 or > segment_size becomes segment_size.  Upstream stands still
for ever on <|0.00|><|0.00|>, and with random weights the timestamp indices run past the window.

Prompts (`condition_on_previous_text`, `initial_prompt`: DESIGN.md section 5f).  Upstream's rules, kept by `PromptHistory` per
file: the history starts as the initial prompt; a window is decoded with history[reset_since:] as its prompt (the decoder keeps
the last n_text_ctx // 2 - 1 of them); a window that settles appends its segments' tokens, timestamp tokens included, and then
forgets everything so far (reset_since = len(history)) when conditioning is off or the standing result was drawn above
temperature 0.5; a skipped window changes nothing.  Every call of a window's ladder sees the same prompt.  With neither option
set the decoder callbacks are called exactly as before; with either they receive the prompt(s) as one more argument.

Word timestamps ("words").  Upstream's `add_word_timestamps`, restated as `add_word_timestamps` below: a
window whose result stands and whose segments hold text is aligned once (the aligner is a callable handed in, like the decoder:
`align_one` / `align_call`), the words are handed out to the window's segments, a few duration heuristics move word and segment
boundaries, and the end of the window's last word, not the last timestamp pair, says where the next window begins
(`settle_words`).  `last_speech_timestamp` is kept per file.  Without an aligner nothing of this runs and a segment has no
"words" key.
"""
from __future__ import annotations

from collections import deque
from dataclasses import dataclass, field, replace
from typing import Callable, Dict, List, Optional, Sequence, Tuple

CHUNK_LENGTH = 30
TEMPERATURES = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)


@dataclass
class WindowResult:
    """What the rules read of a decoded window (DecodingResult has the same fields)."""
    tokens: List[int] = field(default_factory=list)
    avg_logprob: float = 0.0
    no_speech_prob: float = 0.0
    compression_ratio: float = 1.0
    temperature: float = 0.0


@dataclass(frozen=True)
class Thresholds:
    compression_ratio_threshold: Optional[float] = 2.4
    logprob_threshold: Optional[float] = -1.0
    no_speech_threshold: Optional[float] = 0.6


def _default_text(tokens: Sequence[int]) -> str:
    return " ".join(str(t) for t in tokens)


def _timestamp_pairs(tokens: Sequence[int], tb: int) -> Tuple[bool, List[int]]:
    """(single_end, consecutive): whether the last two tokens are (text, timestamp), and the indices i with tokens[i - 1] and
    tokens[i] both timestamps."""
    ts = [t >= tb for t in tokens]
    return ts[-2:] == [False, True], [i for i in range(1, len(tokens)) if ts[i - 1] and ts[i]]


def predicted_advance(tokens: Sequence[int], tb: int, segment_size: int) -> int:
    """Upstream's seek rule as it stands, BEFORE the guard: the frames of the last timestamp pair, or the whole window when
    there is no pair or the window ends on a single timestamp."""
    single_end, consecutive = _timestamp_pairs(tokens, tb)
    if not consecutive or single_end:
        return segment_size
    return 2 * (int(tokens[consecutive[-1] - 1]) - tb)


def cut_segments(tokens: Sequence[int], tb: int, seek: int, segment_size: int, fs: float,
                 decode_text: Optional[Callable[[List[int]], str]] = None) -> Tuple[List[dict], int]:
    """The segments of one window and how far the window moves: (segments, advance in frames).

    `tokens`: the sampled tokens of the window (no start sequence, cut before EOT); `tb`: the first timestamp token; `seek`:
    the window's first frame; `segment_size`: its frames of real audio.  A segment is {seek, start, end, text, tokens}, times in
    seconds; its text is `decode_text` of its tokens below `tb`.  A segment whose start equals its end, or whose text is blank,
    keeps its place with text = "" and tokens = []."""
    decode_text = decode_text or _default_text
    tokens = [int(t) for t in tokens]
    single_end, consecutive = _timestamp_pairs(tokens, tb)
    t0 = seek * fs
    pieces = []                                        # (start, end, tokens)
    if consecutive:
        slices = consecutive + ([len(tokens)] if single_end else [])
        last = 0
        for cur in slices:
            sl = tokens[last:cur]
            pieces.append((t0 + (sl[0] - tb) * 2 * fs, t0 + (sl[-1] - tb) * 2 * fs, sl))
            last = cur
        # (what follows the last slice is dropped)
    else:
        duration = segment_size * fs
        stamps = [t for t in tokens if t >= tb]
        if stamps and stamps[-1] != tb:
            duration = (stamps[-1] - tb) * 2 * fs
        pieces.append((t0, t0 + duration, tokens))
    advance = predicted_advance(tokens, tb, segment_size)
    if advance <= 0 or advance > segment_size:         # the guard (module docstring)
        advance = segment_size
    segments = []
    for start, end, sl in pieces:
        text = decode_text([t for t in sl if t < tb])
        if start == end or text.strip() == "":
            text, sl = "", []
        segments.append(dict(seek=seek, start=start, end=end, text=text, tokens=list(sl)))
    return segments, advance


def is_silence(result, logprob_threshold: Optional[float], no_speech_threshold: Optional[float]) -> bool:
    return (no_speech_threshold is not None and logprob_threshold is not None
            and result.no_speech_prob > no_speech_threshold and result.avg_logprob < logprob_threshold)


def needs_fallback(result, compression_ratio_threshold: Optional[float] = 2.4, logprob_threshold: Optional[float] = -1.0,
                   no_speech_threshold: Optional[float] = 0.6) -> bool:
    """Decode the window again at the next temperature?  Too repetitive (compression ratio above its threshold) or too
    unlikely (average log-probability below its threshold), each only when its threshold is given -- and never when the window
    is silence (`is_silence`)."""
    again = False
    if compression_ratio_threshold is not None and result.compression_ratio > compression_ratio_threshold:
        again = True
    if logprob_threshold is not None and result.avg_logprob < logprob_threshold:
        again = True
    if is_silence(result, logprob_threshold, no_speech_threshold):
        again = False
    return again


def skip_window(result, logprob_threshold: Optional[float] = -1.0, no_speech_threshold: Optional[float] = 0.6) -> bool:
    """No segment for this window?  The no-speech probability is above its threshold, unless the text is likely enough anyway
    (logprob_threshold given and the average log-probability above it)."""
    if no_speech_threshold is None or not result.no_speech_prob > no_speech_threshold:
        return False
    if logprob_threshold is not None and result.avg_logprob > logprob_threshold:
        return False
    return True


def settle_window(result, tb: int, seek: int, segment_size: int, fs: float, th: Thresholds,
                  decode_text: Optional[Callable[[List[int]], str]] = None) -> Tuple[List[dict], int]:
    """The segments and the advance of a window whose result stands: skip, or cut; every segment carries the result's figures."""
    if skip_window(result, th.logprob_threshold, th.no_speech_threshold):
        return [], segment_size
    segments, advance = cut_segments(result.tokens, tb, seek, segment_size, fs, decode_text)
    for s in segments:
        s.update(temperature=float(result.temperature), avg_logprob=float(result.avg_logprob),
                 compression_ratio=float(result.compression_ratio), no_speech_prob=float(result.no_speech_prob))
    return segments, advance


SENTENCE_END_MARKS = ".。!！?？"


def text_tokens(segments: Sequence[dict], eot: int) -> List[int]:
    """The tokens below `eot` of a window's segments, in order: what the aligner aligns."""
    return [int(t) for s in segments for t in s["tokens"] if int(t) < eot]


def add_word_timestamps(segments: List[dict], alignment: Sequence, last_speech_timestamp: float, *, eot: int, fs: float) -> float:
    """Upstream's add_word_timestamps for one window, in place on `segments`; returns the new last_speech_timestamp.

    `segments`: the window's segments from `cut_segments` (all of one seek); `alignment`: the window's words (timing.WordTiming:
    word, tokens, start, end, probability), times in seconds from the window's start; `eot`: tokens below it are text; `fs`:
    seconds per frame.  The alignment is read, never written: the entries the rules move are copies.

      1. a segment's text tokens are its tokens below `eot` (a cleared segment has none);
      2. durations = the nonzero end - start of the alignment; median = min(0.7, median(durations)), 0.0 without durations;
         max_duration = 2 * median;
      3. (only with durations) for i >= 1 with end_i - start_i > max_duration: word_i a sentence mark (one of .。!！?？):
         end_i = start_i + max_duration; else word_{i-1} a sentence mark: start_i = end_i - max_duration;
      4. one walk over the alignment: a segment takes words until the tokens taken reach its text-token count; a taken word
         becomes {word, start, end, probability}, times + seek * fs and rounded to 2 decimals;
      5. per segment with words, in this order: the after-pause clamp, the segment-start rule, the segment-end rule (the code
         below is their statement), then last_speech_timestamp = segment.end;
      6. every segment gets segment["words"], possibly [].

    Order of step 3 and the punctuation merge.  Upstream truncates first and merges afterwards; here the alignment arrives
    MERGED (timing.words_from_path has applied merge_punctuations and dropped the absorbed entries), and step 3 runs on it as it
    stands: merge, then truncate.  A closing mark that followed a word is part of that word by then ("end." is not a mark), so
    step 3 fires only for a mark that stands alone -- the first entry, or one behind a word that ends in a blank -- and for the
    word after such a mark.  Words are compared as they are, without stripping, as upstream."""
    words_in = [replace(w) for w in alignment]
    durations = sorted(w.end - w.start for w in words_in if w.end - w.start != 0)
    if durations:
        mid = len(durations) // 2
        median = durations[mid] if len(durations) % 2 else 0.5 * (durations[mid - 1] + durations[mid])
        median = min(0.7, float(median))
    else:
        median = 0.0
    max_duration = 2 * median

    def is_mark(word: str) -> bool:
        return len(word) == 1 and word in SENTENCE_END_MARKS

    if durations:
        for i in range(1, len(words_in)):
            w = words_in[i]
            if w.end - w.start > max_duration:
                if is_mark(w.word):
                    w.end = w.start + max_duration
                elif is_mark(words_in[i - 1].word):
                    w.start = w.end - max_duration

    time_offset = (segments[0]["seek"] * fs) if segments else 0.0
    index = 0
    for segment in segments:
        n_text = sum(1 for t in segment["tokens"] if int(t) < eot)
        taken = 0
        words: List[dict] = []
        while index < len(words_in) and taken < n_text:
            w = words_in[index]
            if w.word:
                words.append(dict(word=w.word, start=round(time_offset + w.start, 2), end=round(time_offset + w.end, 2),
                                  probability=w.probability))
            taken += len(w.tokens)
            index += 1
        if words:
            first = words[0]
            # after a pause: the first word (or the first two) of the segment cannot be longer than two medians
            if first["end"] - last_speech_timestamp > 4 * median and (
                    first["end"] - first["start"] > max_duration
                    or (len(words) > 1 and words[1]["end"] - first["start"] > 2 * max_duration)):
                if len(words) > 1 and words[1]["end"] - words[1]["start"] > max_duration:
                    boundary = max(words[1]["end"] / 2, words[1]["end"] - max_duration)
                    first["end"] = words[1]["start"] = boundary
                first["start"] = max(0, first["end"] - max_duration)
            # segment start: the timestamp token wins when it lies inside the first word and well behind its start
            if segment["start"] < first["end"] and segment["start"] - 0.5 > first["start"]:
                first["start"] = max(0, min(first["end"] - median, segment["start"]))
            else:
                segment["start"] = first["start"]
            # segment end, likewise
            last = words[-1]
            if segment["end"] > last["start"] and segment["end"] + 0.5 < last["end"]:
                last["end"] = max(last["start"] + median, segment["end"])
            else:
                segment["end"] = last["end"]
            last_speech_timestamp = segment["end"]
        segment["words"] = words
    return last_speech_timestamp


def settle_words(segments: List[dict], alignment: Sequence, tokens: Sequence[int], tb: int, seek: int, segment_size: int,
                 fs: float, eot: int, advance: int, last_speech_timestamp: float) -> Tuple[int, float]:
    """A window with segments, once aligned: `add_word_timestamps`, then upstream's seek rule for words -- (advance,
    last_speech_timestamp).  last_word_end is the end of the last word of the last segment that has words; unless the window
    ended on a single timestamp, a last_word_end behind the window's start moves the next window to round(last_word_end / fs),
    through the guard of `cut_segments` (<= 0 or > segment_size: the whole window); a last_word_end, wherever it lies, becomes
    the file's last_speech_timestamp.  Without segments nothing changes."""
    if not segments:
        return advance, last_speech_timestamp
    last_speech_timestamp = add_word_timestamps(segments, alignment, last_speech_timestamp, eot=eot, fs=fs)
    last_word_end = next((s["words"][-1]["end"] for s in reversed(segments) if s["words"]), None)
    if last_word_end is None:
        return advance, last_speech_timestamp
    single_end = _timestamp_pairs([int(t) for t in tokens], tb)[0]
    if not single_end and last_word_end > seek * fs:
        advance = round(last_word_end / fs) - seek
        if advance <= 0 or advance > segment_size:     # the guard (module docstring)
            advance = segment_size
    return advance, last_word_end


def _check_aligner(aligner, eot) -> None:
    if aligner is not None and eot is None:
        raise ValueError("word timestamps: an aligner needs `eot` (tokens below it are the text that is aligned)")


class PromptHistory:
    """The tokens a file's later windows are conditioned on (module docstring)."""

    def __init__(self, initial_prompt: Sequence[int] = (), condition_on_previous_text: bool = False):
        self.tokens: List[int] = [int(t) for t in initial_prompt]
        self.reset_since = 0
        self.condition = bool(condition_on_previous_text)

    def prompt(self) -> List[int]:
        return self.tokens[self.reset_since:]

    def settle(self, result, segments: Sequence[dict], skipped: bool) -> None:
        """After a window whose `result` stands and was cut into `segments` (or skipped)."""
        if skipped:
            return
        self.tokens += [int(t) for s in segments for t in s["tokens"]]
        if not self.condition or float(result.temperature) > 0.5:
            self.reset_since = len(self.tokens)


def _thresholds(compression_ratio_threshold, logprob_threshold, no_speech_threshold) -> Thresholds:
    return Thresholds(compression_ratio_threshold, logprob_threshold, no_speech_threshold)


def _check_ladder(temperatures: Sequence[float]) -> Tuple[float, ...]:
    temperatures = tuple(float(t) for t in temperatures)
    if not temperatures or len(set(temperatures)) != len(temperatures):
        raise ValueError(f"temperatures {temperatures}: need at least one, each once")
    return temperatures


def transcribe_reference(decode_one: Callable[[int, float], object], content_frames: int, *, window: int, timestamp_begin: int,
                         temperatures: Sequence[float] = TEMPERATURES, compression_ratio_threshold: Optional[float] = 2.4,
                         logprob_threshold: Optional[float] = -1.0, no_speech_threshold: Optional[float] = 0.6,
                         decode_text: Optional[Callable[[List[int]], str]] = None, condition_on_previous_text: bool = False,
                         initial_prompt: Sequence[int] = (), align_one: Optional[Callable[[int, int, List[dict]], Sequence]] = None,
                         eot: Optional[int] = None) -> List[dict]:
    """The literal loop for one file of `content_frames` frames: `decode_one(seek, temperature)` decodes the window at `seek`.
    With `condition_on_previous_text` or an `initial_prompt` (token ids): `decode_one(seek, temperature, prompt)`.
    With `align_one` (and `eot`): every segment gets "words".  `align_one(seek, segment_size, segments)` returns the alignment
    of a window (`add_word_timestamps`); it is asked once per window whose segments hold text, a window with segments but no
    text has the empty alignment, and a window that is skipped or has no segments is left alone (`settle_words`)."""
    temperatures = _check_ladder(temperatures)
    _check_aligner(align_one, eot)
    last_speech = 0.0
    prompted = bool(condition_on_previous_text) or len(initial_prompt) > 0
    history = PromptHistory(initial_prompt, condition_on_previous_text)
    th = _thresholds(compression_ratio_threshold, logprob_threshold, no_speech_threshold)
    fs = CHUNK_LENGTH / window
    segments: List[dict] = []
    seek = 0
    while seek < content_frames:
        segment_size = min(window, content_frames - seek)
        result = None
        prompt = history.prompt()
        for t in temperatures:                         # the ladder: the first result that passes stands, else the last
            result = decode_one(seek, t, list(prompt)) if prompted else decode_one(seek, t)
            if not needs_fallback(result, *_astuple(th)):
                break
        cut, advance = settle_window(result, timestamp_begin, seek, segment_size, fs, th, decode_text)
        history.settle(result, cut, skip_window(result, th.logprob_threshold, th.no_speech_threshold))
        if align_one is not None and cut:
            alignment = align_one(seek, segment_size, cut) if text_tokens(cut, eot) else []
            advance, last_speech = settle_words(cut, alignment, result.tokens, timestamp_begin, seek, segment_size, fs, eot,
                                                advance, last_speech)
        segments += cut
        seek += advance
    return segments


def _astuple(th: Thresholds):
    return th.compression_ratio_threshold, th.logprob_threshold, th.no_speech_threshold


def transcribe_batched(decode_call: Callable[[List[Optional[Tuple[int, int]]], float, List[bool]], Sequence[object]],
                       content_frames_list: Sequence[int], n_rows: int, *, window: int, timestamp_begin: int,
                       temperatures: Sequence[float] = TEMPERATURES, compression_ratio_threshold: Optional[float] = 2.4,
                       logprob_threshold: Optional[float] = -1.0, no_speech_threshold: Optional[float] = 0.6,
                       decode_text: Optional[Callable[[List[int]], str]] = None, condition_on_previous_text: bool = False,
                       initial_prompt: Sequence[int] = (),
                       align_call: Optional[Callable[[List[Optional[Tuple[int, int]]], List[Optional[Tuple[int, List[int]]]]],
                                                     Sequence[Sequence]]] = None,
                       eot: Optional[int] = None) -> List[List[dict]]:
    """The scheduler: up to `n_rows` files are active, one row each; every round decodes the current window of each.

    `decode_call(rows, temperature, live)`: rows[i] = (file, seek) of row i or None for an empty row, always n_rows of them;
    live[i]: whether row i's result is wanted; returns n_rows results (anything for a row that is not live).  Per round one call
    at temperatures[0] with every occupied row live, then, for each further temperature while any row still needs it, one call
    in which only those rows are live (the rows are the round's: same files, same seeks).  A call carries one temperature, and
    no (file, seek, temperature) is asked twice.  A finished file's row goes to the next waiting file from the following round
    on; files without content never take a row.  Per file the segments equal `transcribe_reference`'s for the same decoder.

    With `condition_on_previous_text` or an `initial_prompt` (token ids, the same for every file):
    `decode_call(rows, temperature, live, prompts)`, prompts[i] the prompt of row i's window ([] for an empty row); the fallback
    calls of a round carry the round's prompts.

    With `align_call` (and `eot`): every segment gets "words", as in `transcribe_reference`.  `align_call(rows, jobs)`: rows as
    above, jobs[i] = None or (segment_size, the text tokens of the segments of row i's standing result), always n_rows of them;
    returns n_rows alignments (anything for a row without a job).  It is asked at most once per round, after the ladder has
    settled every row, and not at all in a round in which no row has text."""
    temperatures = _check_ladder(temperatures)
    _check_aligner(align_call, eot)
    last_speech: Dict[int, float] = {}
    if n_rows < 1:
        raise ValueError(f"n_rows = {n_rows}: need at least one row")
    th = _thresholds(compression_ratio_threshold, logprob_threshold, no_speech_threshold)
    fs = CHUNK_LENGTH / window
    content = [int(c) for c in content_frames_list]
    segments: List[List[dict]] = [[] for _ in content]
    waiting = deque(f for f, c in enumerate(content) if c > 0)
    rows: List[Optional[int]] = [None] * n_rows        # the file of every row
    seek: Dict[int, int] = {}
    prompted = bool(condition_on_previous_text) or len(initial_prompt) > 0
    history: Dict[int, PromptHistory] = {}
    while True:
        for i in range(n_rows):
            if rows[i] is None and waiting:
                rows[i] = waiting.popleft()
                seek[rows[i]] = 0
                history[rows[i]] = PromptHistory(initial_prompt, condition_on_previous_text)
                last_speech[rows[i]] = 0.0
        if all(f is None for f in rows):
            break
        asked = [None if f is None else (f, seek[f]) for f in rows]
        live = [f is not None for f in rows]
        prompts = [[] if f is None else history[f].prompt() for f in rows]
        extra = ([list(p) for p in prompts],) if prompted else ()
        final = list(decode_call(list(asked), temperatures[0], list(live), *extra))
        need = [live[i] and needs_fallback(final[i], *_astuple(th)) for i in range(n_rows)]
        for t in temperatures[1:]:
            if not any(need):
                break
            extra = ([list(p) for p in prompts],) if prompted else ()
            again = decode_call(list(asked), t, list(need), *extra)
            for i in range(n_rows):
                if need[i]:
                    final[i] = again[i]
                    need[i] = needs_fallback(again[i], *_astuple(th))
        settled: List[Optional[Tuple[int, List[dict], int]]] = [None] * n_rows       # (segment_size, segments, advance)
        for i, f in enumerate(rows):
            if f is None:
                continue
            segment_size = min(window, content[f] - seek[f])
            cut, advance = settle_window(final[i], timestamp_begin, seek[f], segment_size, fs, th, decode_text)
            history[f].settle(final[i], cut, skip_window(final[i], th.logprob_threshold, th.no_speech_threshold))
            settled[i] = (segment_size, cut, advance)
        if align_call is not None:
            jobs: List[Optional[Tuple[int, List[int]]]] = [None] * n_rows
            for i, s in enumerate(settled):
                if s is not None and text_tokens(s[1], eot):
                    jobs[i] = (s[0], text_tokens(s[1], eot))
            alignments = list(align_call(list(asked), list(jobs))) if any(j is not None for j in jobs) else [None] * n_rows
            for i, f in enumerate(rows):
                if f is None or not settled[i][1]:
                    continue
                segment_size, cut, advance = settled[i]
                advance, last_speech[f] = settle_words(cut, alignments[i] if jobs[i] is not None else [], final[i].tokens,
                                                       timestamp_begin, seek[f], segment_size, fs, eot, advance, last_speech[f])
                settled[i] = (segment_size, cut, advance)
        for i, f in enumerate(rows):
            if f is None:
                continue
            _, cut, advance = settled[i]
            segments[f] += cut
            seek[f] += advance
            if seek[f] >= content[f]:
                rows[i] = None
    return segments
