"""Word timestamps in long-form transcription, the host contract (longform.add_word_timestamps, settle_words and the two loops),
on the CPU.  Every expected value below is worked out by hand from the rules as longform.py states them; nothing is produced by
the function under test.

W = 3000 frames per window, fs = 0.01 s per frame; tokens below EOT are text, TB + k is the timestamp k * 0.02 s.
"""
import copy

import numpy as np
import pytest

import longform as LF
import timing
from longform import WindowResult
from test_longform_cpu import scripted

EOT = 50257
TB = 50364
W = 3000
FS = LF.CHUNK_LENGTH / W


def t(k):
    return TB + k


def word(text, start, end, n_tokens=1, p=0.5):
    return timing.WordTiming(text, list(range(100, 100 + n_tokens)), float(start), float(end), float(p))


def seg(start, end, n_text, seek=0):
    return dict(seek=seek, start=float(start), end=float(end), text="x" if n_text else "", tokens=[t(0)] + list(range(1, n_text + 1)) + [t(1)] if n_text else [])


def add(segments, alignment, last=0.0):
    return LF.add_word_timestamps(segments, alignment, last, eot=EOT, fs=FS)


def times(words):
    return [(w["start"], w["end"]) for w in words]


def approx(x):
    return pytest.approx(x, abs=1e-9)


# ------------------------------------------------------------------------------------------------ step 2: median, max_duration
def test_median_is_capped_at_0_7():
    """durations 1, 2, 3: the median 2.0 becomes 0.7.  Seen through the segment-end rule: the segment ends (3.2) inside the last
    word (3.0 - 6.0) and more than 0.5 before its end, so the word ends at max(3.0 + median, 3.2) = 3.7 (uncapped: 5.0)."""
    s = [seg(0.0, 3.2, 3)]
    last = add(s, [word(" a", 0.0, 1.0), word(" b", 1.0, 3.0), word(" c", 3.0, 6.0)])
    assert times(s[0]["words"]) == [(0.0, 1.0), (1.0, 3.0), (3.0, approx(3.7))]
    assert (s[0]["start"], s[0]["end"]) == (0.0, 3.2) and last == 3.2


def test_median_below_the_cap_odd_and_even_counts():
    s = [seg(0.0, 0.61, 3)]                            # durations 0.2, 0.4, 0.6: median 0.4 -> the last word ends at 0.6 + 0.4
    add(s, [word(" a", 0.0, 0.2), word(" b", 0.2, 0.6), word(" c", 0.6, 1.2)])
    assert times(s[0]["words"])[-1] == (0.6, approx(1.0))
    s = [seg(0.0, 0.3, 2)]                             # durations 0.2, 1.0: the median of two is their mean, 0.6 -> 0.2 + 0.6
    add(s, [word(" a", 0.0, 0.2), word(" b", 0.2, 1.2)])
    assert times(s[0]["words"])[-1] == (0.2, approx(0.8))


def test_zero_durations_do_not_count_and_no_durations_give_zero():
    s = [seg(0.0, 0.1, 3)]                             # durations 0, 0, 1.0: only 1.0 counts -> 0.7 (with the zeros: median 0 -> 0.1)
    add(s, [word(" a", 0.0, 0.0), word(" b", 0.0, 0.0), word(" c", 0.0, 1.0)])
    assert times(s[0]["words"])[-1] == (0.0, approx(0.7))
    # no durations at all: median = max_duration = 0, step 3 is skipped; the after-pause clamp does not fire (0 > 0 is false),
    # the segment takes the words' start and end
    s = [seg(0.0, 5.0, 2)]
    last = add(s, [word(".", 1.0, 1.0), word(" b", 1.0, 1.0)])
    assert times(s[0]["words"]) == [(1.0, 1.0), (1.0, 1.0)] and (s[0]["start"], s[0]["end"]) == (1.0, 1.0) and last == 1.0
    # an empty alignment: no words, nothing moves
    s = [seg(0.0, 5.0, 2)]
    assert add(s, [], 3.25) == 3.25 and s[0]["words"] == [] and (s[0]["start"], s[0]["end"]) == (0.0, 5.0)


# ------------------------------------------------------------------------------------------ step 3: truncation at sentence ends
def test_truncation_of_a_long_mark_and_of_the_word_after_a_mark():
    # durations 0.2, 0.2, 2.6: median 0.2, max_duration 0.4.  "." (0.4 - 3.0) is a mark and too long: it ends at 0.4 + 0.4
    alignment = [word(" a", 0.0, 0.2), word(" b", 0.2, 0.4), word(".", 0.4, 3.0)]
    s = [seg(0.0, 3.0, 3)]
    add(s, alignment)
    assert times(s[0]["words"]) == [(0.0, 0.2), (0.2, 0.4), (0.4, approx(0.8))] and s[0]["end"] == approx(0.8)
    assert (alignment[2].start, alignment[2].end) == (0.4, 3.0), "the caller's alignment was written"
    # the word after a mark: " b" (0.4 - 3.0) follows "?" -> it starts at 3.0 - 0.4
    s = [seg(0.0, 3.0, 3)]
    add(s, [word(" a", 0.0, 0.2), word("?", 0.2, 0.4), word(" b", 0.4, 3.0)])
    assert times(s[0]["words"]) == [(0.0, 0.2), (0.2, 0.4), (approx(2.6), 3.0)] and s[0]["end"] == 3.0


def test_truncation_does_not_fire():
    # no mark in sight; a mark at index 0 (i >= 1 only); a long word that merely ENDS in a mark; a mark of ordinary length
    for alignment in ([word(" a", 0.0, 0.2), word(" c", 0.2, 0.4), word(" b", 0.4, 3.0)],
                      [word(".", 0.0, 3.0), word(" a", 3.0, 3.2), word(" b", 3.2, 3.4)],
                      [word(" a", 0.0, 0.2), word(" c", 0.2, 0.4), word(" b.", 0.4, 3.0)],
                      [word(" a", 0.0, 0.2), word(" c", 0.2, 0.4), word(".", 0.4, 0.8)]):
        s = [seg(0.0, alignment[-1].end, 3)]
        add(s, alignment, last=alignment[0].end)       # (last_speech_timestamp at the first word's end: no after-pause clamp)
        assert times(s[0]["words"]) == [(w.start, w.end) for w in alignment]


def test_truncation_runs_on_the_merged_alignment():
    """The order this project picked: merge_punctuations first (words_from_path), truncation afterwards.  " c" (0.6 - 3.0) is
    too long (median 0.2) and follows "." -- but the "." has been absorbed into " b.", which is not a mark, so " c" keeps its
    start (truncating first, as upstream does, would move it to 2.6)."""
    raw = [word(" a", 0.0, 0.2), word(" b", 0.2, 0.4), word(".", 0.4, 0.6), word(" c", 0.6, 3.0)]
    timing.merge_punctuations(raw)
    merged = [w for w in raw if w.word]
    assert [(w.word, len(w.tokens)) for w in merged] == [(" a", 1), (" b.", 2), (" c", 1)]
    s = [seg(0.0, 3.0, 4)]
    add(s, merged)
    assert [w["word"] for w in s[0]["words"]] == [" a", " b.", " c"]
    assert times(s[0]["words"]) == [(0.0, 0.2), (0.2, 0.4), (0.6, 3.0)]


# ----------------------------------------------------------------------------------------------------- step 5: after a pause
def test_after_pause_clamp_one_word():
    # one word 5.0 - 8.0: median 0.7 (capped), max_duration 1.4.  8.0 - 0 > 2.8 and 3.0 > 1.4: it starts at 8.0 - 1.4
    s = [seg(5.0, 8.0, 1)]
    last = add(s, [word(" a", 5.0, 8.0)])
    assert times(s[0]["words"]) == [(approx(6.6), 8.0)] and (s[0]["start"], s[0]["end"]) == (approx(6.6), 8.0) and last == 8.0
    # no pause (8.0 - 6.0 = 2.0 is not > 2.8): nothing moves
    s = [seg(5.0, 8.0, 1)]
    add(s, [word(" a", 5.0, 8.0)], last=6.0)
    assert times(s[0]["words"]) == [(5.0, 8.0)] and s[0]["start"] == 5.0
    # a pause, but the word is short (1.0 <= 1.4): nothing moves
    s = [seg(5.0, 6.0, 1)]
    add(s, [word(" a", 5.0, 6.0)])
    assert times(s[0]["words"]) == [(5.0, 6.0)]


def test_after_pause_clamp_two_words():
    # durations 0.2, 3.8: median 2.0 -> 0.7, max_duration 1.4.  5.2 > 2.8; the first word is short, but the two together span
    # 4.0 > 2.8: the clamp fires.  The second word is too long (3.8 > 1.4): the boundary moves to max(9.0 / 2, 9.0 - 1.4) = 7.6;
    # then the first word starts at 7.6 - 1.4 = 6.2
    s = [seg(5.0, 9.0, 2)]
    add(s, [word(" a", 5.0, 5.2), word(" b", 5.2, 9.0)])
    assert times(s[0]["words"]) == [(approx(6.2), approx(7.6)), (approx(7.6), 9.0)]
    assert (s[0]["start"], s[0]["end"]) == (approx(6.2), 9.0)
    # the second word of ordinary length (0.4): no boundary move, only the first word's start: 8.0 - 1.4
    s = [seg(5.0, 8.4, 2)]
    add(s, [word(" a", 5.0, 8.0), word(" b", 8.0, 8.4)])
    assert times(s[0]["words"]) == [(approx(6.6), 8.0), (8.0, 8.4)]


# ------------------------------------------------------------------------------------------- step 5: segment start and end
def test_segment_start_rule_both_directions():
    alignment = [word(" a", 1.0, 3.0), word(" b", 3.0, 3.4), word(" c", 3.4, 3.8)]       # median 0.4
    for seg_start, want_word, want_seg in ((2.0, 2.0, 2.0),          # inside the word, > 0.5 behind its start: min(3.0 - 0.4, 2.0)
                                           (2.8, 2.6, 2.8),          # likewise, but end - median is the smaller: 2.6
                                           (1.2, 1.0, 1.0),          # only 0.2 behind the word's start: the segment takes 1.0
                                           (3.5, 1.0, 1.0)):         # not before the word's end: the segment takes 1.0
        s = [seg(seg_start, 3.8, 3)]
        add(s, alignment, last=2.9)                    # (2.9: no pause)
        assert s[0]["words"][0]["start"] == approx(want_word) and s[0]["start"] == approx(want_seg), seg_start
        assert times(s[0]["words"])[1:] == [(3.0, 3.4), (3.4, 3.8)]


def test_segment_end_rule_both_directions():
    alignment = [word(" a", 0.0, 1.0), word(" b", 1.0, 3.0), word(" c", 3.0, 6.0)]       # median 0.7 (capped)
    for seg_end, want_word, want_seg in ((5.0, 5.0, 5.0),            # inside the word, > 0.5 before its end: max(3.7, 5.0)
                                         (3.2, 3.7, 3.2),            # likewise, start + median is the larger
                                         (5.8, 6.0, 6.0),            # only 0.2 before the word's end: the segment takes 6.0
                                         (2.5, 6.0, 6.0)):           # not behind the word's start: the segment takes 6.0
        s = [seg(0.0, seg_end, 3)]
        last = add(s, alignment)
        assert s[0]["words"][-1]["end"] == approx(want_word) and s[0]["end"] == approx(want_seg) == approx(last), seg_end


# ------------------------------------------------------------------------------------------------------- step 4: handing out
def test_words_go_to_three_segments_one_of_them_cleared():
    # seek 200: time_offset 2.0.  Segment 0 has two text tokens, segment 1 is cleared, segment 2 has three (one word of two tokens)
    s = [seg(2.0, 2.4, 2, seek=200), seg(2.4, 2.4, 0, seek=200), seg(2.6, 3.0, 3, seek=200)]
    alignment = [word(" a", 0.0, 0.2, p=0.1), word(" b", 0.2, 0.4, p=0.2), word(" cd", 0.6, 0.8, n_tokens=2, p=0.3), word(" e", 0.8, 1.0, p=0.4)]
    last = add(s, alignment, last=2.0)
    assert s[0]["words"] == [dict(word=" a", start=2.0, end=2.2, probability=0.1), dict(word=" b", start=2.2, end=2.4, probability=0.2)]
    assert s[1]["words"] == [] and (s[1]["start"], s[1]["end"]) == (2.4, 2.4)
    assert s[2]["words"] == [dict(word=" cd", start=2.6, end=2.8, probability=0.3), dict(word=" e", start=2.8, end=3.0, probability=0.4)]
    assert [(x["start"], x["end"]) for x in s] == [(2.0, 2.4), (2.4, 2.4), (2.6, 3.0)] and last == 3.0
    assert all(set(x) == {"seek", "start", "end", "text", "tokens", "words"} for x in s)


def test_a_word_that_overshoots_and_an_alignment_shorter_than_the_tokens():
    # segment 0 has one text token, the first word two: it is taken whole, segment 1 goes on with the next word
    s = [seg(0.0, 0.2, 1), seg(0.2, 0.6, 2)]
    add(s, [word(" ab", 0.0, 0.2, n_tokens=2), word(" c", 0.2, 0.4), word(" d", 0.4, 0.6)])
    assert [[w["word"] for w in x["words"]] for x in s] == [[" ab"], [" c", " d"]]
    # three words for 2 + 2 tokens: segment 1 gets the one that is left; one word for 2 + 2 tokens: segment 1 gets nothing and
    # keeps its times
    s = [seg(0.0, 0.4, 2), seg(0.4, 0.8, 2)]
    add(s, [word(" a", 0.0, 0.2), word(" b", 0.2, 0.4), word(" c", 0.4, 0.6)])
    assert [[w["word"] for w in x["words"]] for x in s] == [[" a", " b"], [" c"]] and s[1]["end"] == 0.6
    s = [seg(0.0, 0.4, 2), seg(0.4, 0.8, 2)]
    last = add(s, [word(" a", 0.0, 0.2)])
    assert [[w["word"] for w in x["words"]] for x in s] == [[" a"], []] and (s[1]["start"], s[1]["end"]) == (0.4, 0.8) and last == 0.2


def test_times_are_offset_by_the_seek_and_rounded_to_two_decimals():
    s = [seg(12.34, 13.0, 1, seek=1234)]               # time_offset 12.34
    add(s, [word(" a", 0.123, 0.456)], last=12.4)
    assert s[0]["words"] == [dict(word=" a", start=12.46, end=12.8, probability=0.5)]      # 12.463 -> 12.46, 12.796 -> 12.8
    assert (s[0]["start"], s[0]["end"]) == (12.46, 12.8)


# ------------------------------------------------------------------------------------------------------------ the seek rule
def settle(tokens, alignment, seek, size, advance, last=0.0):
    segments, adv = LF.cut_segments(tokens, TB, seek, size, FS)
    assert adv == advance
    return segments, LF.settle_words(segments, alignment, tokens, TB, seek, size, FS, EOT, adv, last)


def test_seek_rule():
    two = [word(" a", 4.0, 4.28), word(" b", 4.28, 4.56)]
    # the window ends on a single timestamp: the seek is the timestamps' business (the whole window), the clock still moves
    _, (advance, last) = settle([t(0), 1, 2, t(100)], two, 1000, W, W)
    assert advance == W and last == 14.56
    # no single ending: the last word ends at 10.0 + 4.56 -> frame 1456, 456 behind the seek
    segments, (advance, last) = settle([t(0), 1, 2], two, 1000, W, W)
    assert advance == 456 and last == 14.56 and segments[0]["words"][-1]["end"] == 14.56
    # ... and with a timestamp pair that said 400 frames: the word wins
    _, (advance, last) = settle([t(0), 1, 2, t(200), t(200)], two, 1000, W, 400)
    assert advance == 456
    # the last word ends at the window's start (not behind it): the seek stays with the timestamps; the clock is set
    _, (advance, last) = settle([t(0), 1, 2, t(200), t(200)], [word(" a", 0.0, 0.0), word(" b", 0.0, 0.0)], 1000, W, 400, last=7.0)
    assert advance == 400 and last == 10.0
    # beyond a tail window of 300 frames: the guard makes it the whole window
    _, (advance, last) = settle([t(0), 1, 2], two, 1000, 300, 300)
    assert advance == 300 and last == 14.56
    # no words at all (an empty alignment): nothing changes
    segments, (advance, last) = settle([t(0), 1, 2, t(200), t(200)], [], 1000, W, 400, last=7.0)
    assert advance == 400 and last == 7.0 and segments[0]["words"] == []
    # no segments (a skipped window): nothing changes
    assert LF.settle_words([], two, [t(0), 1, 2], TB, 1000, W, FS, EOT, W, 7.0) == (W, 7.0)


def test_last_speech_timestamp_chain_over_three_windows():
    """A file of 1100 frames, no timestamp pairs: the words decide the seeks -- 0, 200, 800.  The clock (last_speech_timestamp)
    is 0.0, then 2.0, then 8.0:
      window 0: words 1.0 - 1.5 - 2.0 (median 0.5): no clamp (1.5 - 0 is not > 2.0); the segment becomes 1.0 - 2.0; seek -> 200
      window 1: words at 2.0 + (3.0 - 5.5 - 6.0), median 0.7: 7.5 - 2.0 > 2.8 and 2.5 > 1.4: the first word starts at 7.5 - 1.4;
                seek -> 800
      window 2: words at 8.0 + (0.5 - 2.5 - 3.0): 10.5 - 8.0 = 2.5 is NOT > 2.8: no clamp (with a clock that stood still at 0.0
                or 2.0 it would fire); seek -> 1100, the end."""
    scripts = {0: [word(" a", 1.0, 1.5), word(" b", 1.5, 2.0)], 200: [word(" a", 3.0, 5.5), word(" b", 5.5, 6.0)],
               800: [word(" a", 0.5, 2.5), word(" b", 2.5, 3.0)]}
    asked = []

    def align_one(seek, size, segments):
        asked.append((seek, size, LF.text_tokens(segments, EOT)))
        return scripts[seek]

    got = LF.transcribe_reference(lambda seek, temp: WindowResult(tokens=[t(0), 1, 2]), 1100, window=W, timestamp_begin=TB,
                                  temperatures=(0.0,), align_one=align_one, eot=EOT)
    assert asked == [(0, 1100, [1, 2]), (200, 900, [1, 2]), (800, 300, [1, 2])]
    assert [(s["seek"], s["start"], s["end"]) for s in got] == [(0, 1.0, 2.0), (200, approx(6.1), 8.0), (800, 8.5, 11.0)]
    assert [times(s["words"]) for s in got] == [[(1.0, 1.5), (1.5, 2.0)], [(approx(6.1), 7.5), (7.5, 8.0)], [(8.5, 10.5), (10.5, 11.0)]]


def test_an_aligner_needs_eot():
    with pytest.raises(ValueError, match="eot"):
        LF.transcribe_reference(lambda seek, temp: WindowResult(), 10, window=W, timestamp_begin=TB, align_one=lambda *a: [])
    with pytest.raises(ValueError, match="eot"):
        LF.transcribe_batched(lambda *a: [], [10], 1, window=W, timestamp_begin=TB, align_call=lambda *a: [])


# ----------------------------------------------------------------------------------------- the loops, scripted on both sides
def scripted_aligner(seed):
    """align(file, seek, segment_size, text tokens) -> alignment, a pure function of its arguments: words of 1-3 tokens that
    cover the tokens, times that grow from a random start -- some of zero length, some far too long, some beyond the window,
    some bare sentence marks."""
    def align(f, seek, size, tokens):
        rng = np.random.Generator(np.random.PCG64([seed, f, seek, size, len(tokens)]))
        out, i, clock = [], 0, float(rng.random() * size * FS * 0.5)
        while i < len(tokens):
            n = min(int(rng.integers(1, 4)), len(tokens) - i)
            dur = float(rng.choice([0.0, 0.1, 0.3, 0.5, 4.0])) * float(rng.random() < 0.9)
            text = "." if rng.random() < 0.15 else f" w{tokens[i]}"
            out.append(timing.WordTiming(text, list(tokens[i:i + n]), round(clock, 3), round(clock + dur, 3), float(rng.random())))
            clock += dur + float(rng.choice([0.0, 0.0, 0.2, 3.0]))
            i += n
        return out
    return align


CONTENTS = [0, 1, W - 1, W + 1, 2 * W + 17, 0, W + 1, 700]           # more files than rows, for both n_rows below


@pytest.mark.parametrize("kind", ["timestamps", "adversarial"])
@pytest.mark.parametrize("n_rows", [1, 3])
@pytest.mark.parametrize("thresholds", [dict(), dict(compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None)])
def test_batched_equals_the_reference_with_words(kind, n_rows, thresholds):
    decode, align = scripted(kind, 11), scripted_aligner(13)
    ref_asked = []
    want = []
    for f, c in enumerate(CONTENTS):
        def align_one(seek, size, segments, f=f):
            ref_asked.append((f, seek, size))
            return align(f, seek, size, LF.text_tokens(segments, EOT))
        want.append(LF.transcribe_reference(lambda seek, temp, f=f: decode(f, seek, temp), c, window=W, timestamp_begin=TB,
                                            align_one=align_one, eot=EOT, **thresholds))
    events = []

    def decode_call(rows, temperature, live):
        events.append(("decode", list(rows), temperature))
        return [decode(r[0], r[1], temperature) if on else None for r, on in zip(rows, live)]

    def align_call(rows, jobs):
        assert len(rows) == n_rows == len(jobs)
        events.append(("align", list(rows), copy.deepcopy(jobs)))
        return [None if j is None else align(r[0], r[1], j[0], j[1]) for r, j in zip(rows, jobs)]

    got = LF.transcribe_batched(decode_call, CONTENTS, n_rows, window=W, timestamp_begin=TB, align_call=align_call, eot=EOT, **thresholds)
    assert got == want
    assert all("words" in s for segs in got for s in segs)
    assert any(s["words"] for segs in got for s in segs), "the scripts produced no words at all"
    # an alignment call follows the decoder calls of its round (same rows), at most one per round, and is followed by a new round
    ladder = thresholds.get("temperatures", LF.TEMPERATURES)
    batch_asked = []
    for k, ev in enumerate(events):
        if ev[0] != "align":
            continue
        assert events[k - 1][0] == "decode" and events[k - 1][1] == ev[1]
        assert k + 1 == len(events) or (events[k + 1][0] == "decode" and events[k + 1][2] == ladder[0])
        assert any(j is not None for j in ev[2])
        for r, j in zip(ev[1], ev[2]):
            assert j is None or (r is not None and len(j[1]) > 0 and j[0] == min(W, CONTENTS[r[0]] - r[1]))
            if j is not None:
                batch_asked.append((r[0], r[1], j[0]))
    assert sorted(batch_asked) == sorted(ref_asked) and len(set(batch_asked)) == len(batch_asked)
    # every word starts before it ends (the scripted words have gaps between them, which a DTW path never has: the after-pause
    # clamp may then put a word's start before its window, so that is not asserted here)
    for segs in got:
        for s in segs:
            assert all(0 <= w["start"] <= w["end"] for w in s["words"])


def test_align_call_once_per_round_and_never_without_text():
    rounds = []

    def decode_call(rows, temperature, live):
        if temperature == 0.0:
            rounds.append(dict(rows=list(rows), aligned=0))
        # file 1 never has text (a lone pair of timestamps); file 0 has text in its first window only
        return [None if not on else WindowResult(tokens=[t(0), 5, 6, t(50), t(50)] if r == (0, 0) else [t(10), t(10)])
                for r, on in zip(rows, live)]

    def align_call(rows, jobs):
        assert rows == rounds[-1]["rows"]
        rounds[-1]["aligned"] += 1
        rounds[-1]["jobs"] = jobs
        return [None if j is None else [word(" a", 0.0, 0.5), word(" b", 0.5, 1.0)] for j in jobs]

    got = LF.transcribe_batched(decode_call, [250, 150], 2, window=W, timestamp_begin=TB, temperatures=(0.0, 0.5), align_call=align_call,
                                eot=EOT, compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None)
    # round 0: file 0 at 0 has text -> one call, a job for row 0 only; the last word ends at 1.0 -> seek 100 (the pair said 100 too)
    assert rounds[0] == dict(rows=[(0, 0), (1, 0)], aligned=1, jobs=[(250, [5, 6]), None])
    # later rounds: nobody has text -> never asked; the windows move by the guard / their pairs
    assert len(rounds) > 1 and all(r["aligned"] == 0 for r in rounds[1:])
    assert [w["word"] for w in got[0][0]["words"]] == [" a", " b"] and got[0][0]["seek"] == 0
    assert all(s["words"] == [] for s in got[0][1:] + got[1]) and all("words" in s for s in got[0] + got[1])


@pytest.mark.parametrize("kind", ["timestamps", "adversarial", "still"])
def test_without_callbacks_nothing_changes(kind):
    decode = scripted(kind, 7)

    def decode_call(rows, temperature, live):
        return [decode(r[0], r[1], temperature) if on else None for r, on in zip(rows, live)]

    got = LF.transcribe_batched(decode_call, CONTENTS, 3, window=W, timestamp_begin=TB)
    want = [LF.transcribe_reference(lambda seek, temp, f=f: decode(f, seek, temp), c, window=W, timestamp_begin=TB)
            for f, c in enumerate(CONTENTS)]
    assert got == want
    keys = {"seek", "start", "end", "text", "tokens", "temperature", "avg_logprob", "compression_ratio", "no_speech_prob"}
    assert all(set(s) == keys for segs in got for s in segs)
    # and the windows are where the timestamps alone put them: every segment's seek is reachable by cut_segments' advances
    for f, c in enumerate(CONTENTS):
        seek, seeks = 0, set()
        while seek < c:
            seeks.add(seek)
            result = None
            for temp in LF.TEMPERATURES:
                result = decode(f, seek, temp)
                if not LF.needs_fallback(result):
                    break
            seek += LF.settle_window(result, TB, seek, min(W, c - seek), FS, LF.Thresholds())[1]
        assert {s["seek"] for s in got[f]} <= seeks


def test_transcribe_refuses_word_timestamps_with_beam_search():
    import types

    import native
    import transcribe as T
    opt = types.SimpleNamespace(prompt=None, prefix=None, temperature=0.0)
    plain = types.SimpleNamespace(options=opt, beam=False, n_group=1, use_int8_cross_kv=False)
    T.check_supported(plain, LF.TEMPERATURES, word_timestamps=True)
    with pytest.raises(ValueError, match="word_timestamps"):
        T.check_supported(types.SimpleNamespace(options=opt, beam=True, n_group=2, use_int8_cross_kv=False), (0.0,), word_timestamps=True)
    with pytest.raises(ValueError, match="word_timestamps"):
        T.check_supported(types.SimpleNamespace(options=opt, beam=False, n_group=3, use_int8_cross_kv=False), (0.0,), word_timestamps=True)
    with pytest.raises(native.WmError, match="int8"):
        T.check_supported(types.SimpleNamespace(options=opt, beam=False, n_group=1, use_int8_cross_kv=True), (0.0,), word_timestamps=True)
    assert T.parse_arguments(["--input_file", "a.flac", "--word_timestamps"]).word_timestamps
    assert not T.parse_arguments(["--input_file", "a.flac"]).word_timestamps
