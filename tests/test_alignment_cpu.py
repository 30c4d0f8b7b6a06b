"""Forced alignment on the host (alignment.py): the open-end walk against a brute-force table, the window, accept
and seek rules, the refusals, and the literal loop over a scripted matrix source.  Nothing here needs a GPU."""
import os
import re

import numpy as np
import pytest

import alignment as A
import native
import timing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- dtw_open_cpu ---------------------------------------------------------------------------------------------------------------
def brute_open(x):
    """The contract cell by cell, column-major loops, fp32: (text, time, end_row)."""
    x = np.asarray(x, dtype=np.float32)
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    trace = np.zeros((N + 1, M + 1), dtype=np.int8)
    cost[0, 0] = 0
    for j in range(1, M + 1):
        for i in range(1, N + 1):
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cost[i, j] = np.float32(x[i - 1, j - 1] + c)
            trace[i, j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    col = cost[1:, M]
    end = 1 + int(min(k for k in range(N) if all(col[k] <= col[m] for m in range(N))))
    i, j, text, time = end, M, [], []
    while i > 0 or j > 0:
        text.append(i - 1); time.append(j - 1)
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return text[::-1], time[::-1], end


def inputs(kind, N, M, seed):
    rng = np.random.default_rng(seed)
    if kind == "ties":
        return rng.integers(-2, 3, size=(N, M)).astype(np.float32)
    return rng.standard_normal((N, M)).astype(np.float32)


def band(N, M, k):
    """A diagonal band of -1 over the first k rows (row r holds frames r * M // k .. (r + 1) * M // k - 1), +1 elsewhere."""
    x = np.ones((N, M), dtype=np.float32)
    for r in range(k):
        x[r, r * M // k: (r + 1) * M // k] = -1
    return x


@pytest.mark.parametrize("kind", ["random", "ties"])
@pytest.mark.parametrize("N,M", [(1, 1), (1, 7), (5, 1), (7, 40), (33, 100), (40, 9)])
def test_dtw_open_equals_the_brute_force_table(kind, N, M):
    x = inputs(kind, N, M, 100 * N + M)
    ti, fi, end = A.dtw_open_cpu(x)
    bt, bf, bend = brute_open(x)
    assert (ti.tolist(), fi.tolist(), end) == (bt, bf, bend)
    assert ti[0] == 0 and fi[0] == 0 and ti[-1] == end - 1 and fi[-1] == M - 1
    assert set(np.diff(ti).tolist()) <= {0, 1} and set(np.diff(fi).tolist()) <= {0, 1}


def test_dtw_open_equals_dtw_cpu_when_the_minimum_is_in_the_last_row():
    x = band(12, 60, 12)
    ti, fi, end = A.dtw_open_cpu(x)
    ct, cf = timing.dtw_cpu(x)
    assert end == 12 and ti.tolist() == ct.tolist() and fi.tolist() == cf.tolist()


@pytest.mark.parametrize("k", [1, 6, 12])
def test_planted_band_ends_at_its_last_row(k):
    ti, fi, end = A.dtw_open_cpu(band(12, 60, k))
    assert end == k and ti[-1] == k - 1 and len(fi) >= 60


def test_ties_take_the_smallest_row():
    x = np.zeros((5, 7), dtype=np.float32)             # every cost of the last column is 0
    ti, fi, end = A.dtw_open_cpu(x)
    assert end == 1 and ti.tolist() == [0] * 7 and fi.tolist() == list(range(7))
    x[0, :] = 1                                        # rows 2 .. 5 tie below row 1
    assert A.dtw_open_cpu(x)[2] == 2


def test_dtw_open_empty():
    for shape in ((0, 5), (4, 0)):
        ti, fi, end = A.dtw_open_cpu(np.zeros(shape, dtype=np.float32))
        assert len(ti) == 0 and len(fi) == 0 and end == 0


# ---- the window rule ------------------------------------------------------------------------------------------------------------
SOT, NOTS, EOT = (50258, 50259, 50359), 50363, 50257


def test_plan_window_takes_whole_words_while_they_fit():
    wt = [[1, 2], [3], [4, 5, 6], [7]]
    p = A.plan_window(wt, SOT, NOTS, EOT, 4)
    assert p.n_words == 2 and p.boundaries == [0, 2, 3] and p.forced == list(SOT) + [NOTS, 1, 2, 3, EOT]
    p = A.plan_window(wt, SOT, NOTS, EOT, 6)
    assert p.n_words == 3 and p.boundaries == [0, 2, 3, 6]
    p = A.plan_window(wt, SOT, NOTS, EOT, 100)
    assert p.n_words == 4 and p.forced[-2:] == [7, EOT]
    with pytest.raises(ValueError, match="max_tokens"):
        A.plan_window([[1, 2, 3]], SOT, NOTS, EOT, 2)
    with pytest.raises(ValueError, match="max_tokens"):
        A.check_words([[1], [1, 2, 3]], 2)


# ---- the accept rule ------------------------------------------------------------------------------------------------------------
def stairs(frames_per_row, rows):
    """A path that stays `frames_per_row` frames in each of `rows` rows."""
    text = [r for r in range(rows) for _ in range(frames_per_row)]
    return np.array(text), np.arange(len(text))


def test_accept_needs_the_row_after_the_word():
    bounds = [0, 2, 3, 6]                              # three words, 6 text tokens, row 6 is <|endoftext|>'s
    text, time = stairs(5, 7)
    assert A.accept_words(text, time, 7, bounds, 35, True, 0) == (3, [(0, 10), (10, 15), (15, 30)])
    text, time = stairs(5, 6)                          # the path ends inside the last word's rows: it never entered row 6
    assert A.accept_words(text, time, 6, bounds, 30, True, 0) == (2, [(0, 10), (10, 15)])
    text, time = stairs(5, 3)                          # rows 0 .. 2: word 0 placed (row 2 entered), word 1 not (row 3 not entered)
    assert A.accept_words(text, time, 3, bounds, 15, True, 0)[0] == 1
    text, time = stairs(5, 2)
    assert A.accept_words(text, time, 2, bounds, 10, True, 0) == (0, [])


def test_edge_guard_on_off_and_the_last_window():
    bounds = [0, 2, 3, 6]
    text, time = stairs(5, 7)                          # entries at frames 0, 5, ..., 30; F = 35
    # guard of 4 frames: entry <= 35 - 1 - 4 = 30: the last word (ends at 30) passes; 5 frames: it fails
    assert A.accept_words(text, time, 7, bounds, 35, False, 4)[0] == 3
    assert A.accept_words(text, time, 7, bounds, 35, False, 5)[0] == 2
    assert A.accept_words(text, time, 7, bounds, 35, False, 20)[0] == 1          # 10 <= 14 < 15: placement stops at the first failure
    assert A.accept_words(text, time, 7, bounds, 35, False, 0)[0] == 3           # off
    assert A.accept_words(text, time, 7, bounds, 35, True, 20)[0] == 3           # the file's last window: no guard


def test_placement_stops_at_the_first_failure():
    """Word 1 ends past the guard, word 2 could not be placed anyway; a later word never overtakes one that failed."""
    bounds = [0, 1, 2, 3]
    text = np.array([0, 1, 1, 1, 1, 2, 3])
    time = np.array([0, 1, 2, 3, 4, 5, 5])             # rows 2 and 3 are entered at frame 5
    n, spans = A.accept_words(text, time, 4, bounds, 8, False, 3)               # limit 8 - 1 - 3 = 4
    assert n == 1 and spans == [(0, 1)]


def test_seek_rule_always_advances():
    assert A.next_seek(100, 3000, []) == 3100                                  # nothing placed: the window is skipped whole
    assert A.next_seek(100, 3000, [(0, 10), (10, 700)]) == 1500                # the end of the last word placed, in mel frames
    assert A.next_seek(100, 3000, [(0, 0)]) == 102                             # a word that ends in frame 0 still moves the seek
    assert A.window_frames(0, 3000, 7000) == (1500, False) and A.window_frames(4000, 3000, 7000) == (1500, True)
    assert A.window_frames(6001, 3000, 7000) == (499, True) and A.window_frames(7000, 3000, 7000) == (0, True)


def test_punctuation_merge_and_leftovers():
    words = [" Hello", ",", " (", "world", ")", " again"]
    toks = [[1], [2], [3], [4], [5], [6]]
    lines = [0, 0, 0, 0, 0, 1]
    plan = A.plan_window(toks, SOT, NOTS, EOT, 5)
    assert plan.n_words == 5
    text, time = stairs(4, 6)
    placed, seek = A.settle_window(words, toks, lines, 0, plan, text, time, 6, [0.5, 0.1, 0.2, 0.3, 0.4], 0, 24, True, 3000, 0.02,
                                   A.AlignOptions())
    assert len(placed) == 5 and seek == 2 * 20
    rest = A.leftover_words(words, toks, lines, 5, 12.5)
    assert [(w.word, w.start, w.end, w.probability, w.aligned) for w in rest] == [(" again", 12.5, 12.5, 0.0, False)]
    res = A.file_result("en", ["Hello, (world)", "again"], placed + rest, 12.5)
    assert [w["word"] for w in res["words"]] == [" Hello,", " (world)", " again"]
    hello, world, again = res["words"]
    assert (hello["start"], hello["end"]) == (0.0, 4 * 0.02) and hello["probability"] == 0.5      # times and probability are the word's own
    assert world["start"] == pytest.approx(12 * 0.02) and world["end"] == pytest.approx(16 * 0.02)
    assert [s["aligned"] for s in res["segments"]] == [True, False]
    assert res["segments"][0]["start"] == 0.0 and res["segments"][0]["end"] == pytest.approx(16 * 0.02)
    assert res["segments"][1]["start"] == res["segments"][1]["end"] == 12.5 and again["aligned"] is False
    assert [w for s in res["segments"] for w in s["words"]] == res["words"]


# ---- options and arguments ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(max_tokens=0), dict(max_tokens=446), dict(max_tokens=1.5), dict(max_tokens=True),
                                dict(edge_seconds=-0.1), dict(edge_seconds=15.5), dict(edge_seconds=float("nan")), dict(edge_seconds="1")])
def test_options_refuse(kw):
    with pytest.raises(ValueError):
        A.AlignOptions(**kw)


def test_options_accept_and_check_against_the_model():
    o = A.AlignOptions()
    assert (o.max_tokens, o.edge_seconds) == (128, 0.5) and o.edge_frames(0.02) == 25
    A.AlignOptions(max_tokens=1, edge_seconds=0)
    A.AlignOptions(max_tokens=445, edge_seconds=15).check(448, 1)
    with pytest.raises(ValueError, match="443"):
        A.AlignOptions(max_tokens=444).check(448, 3)
    with pytest.raises(ValueError):
        A.split_text(None, 5, None)


# ---- the literal loop -----------------------------------------------------------------------------------------------------------
def test_align_reference_over_three_windows():
    """Nine one-token words, four per window (max_tokens = 4), W = 100 mel frames (F = 50), 240 frames of content: window 0 speaks
    three words and a half, window 1 (at the end of word 2) holds only music, window 2 speaks two more words, window 3 (the tail) none;
    the rest is left over."""
    words = [f" w{k}" for k in range(9)]
    toks = [[10 + k] for k in range(9)]
    lines = [0] * 5 + [1] * 4
    calls = []

    def source(seek, forced, F):
        calls.append((seek, list(forced), F))
        n = len(forced) - len(SOT) - 2
        m = np.full((n + 1, F), -1.0, dtype=np.float32)                 # (the matrix is negated before the walk: high = aligned)
        if len(calls) == 1:
            for r in range(4):
                m[r, 10 * r: 10 * r + 10] = 1                          # words 0 .. 2 end at 10, 20, 30; word 3 runs to the edge
            m[3, 30:] = 1
        elif len(calls) in (2, 4):
            m[0, :] = 1                                                # one row swallows the window: nothing else is entered
        else:
            m[0, 0:5] = 1; m[1, 5:12] = 1; m[2, 12:] = 1               # 80 frames of content left: F = 40
        return m, [0.25] * n

    records = []
    out = A.align_reference(source, words, toks, lines, 240, window=100, seconds_per_frame=0.02, sot_sequence=SOT,
                            no_timestamps=NOTS, eot=EOT, options=A.AlignOptions(max_tokens=4, edge_seconds=0.1), records=records)
    assert [c[0] for c in calls] == [0, 60, 160, 184] and [c[2] for c in calls] == [50, 50, 40, 28]
    assert calls[0][1] == list(SOT) + [NOTS, 10, 11, 12, 13, EOT] and calls[1][1] == list(SOT) + [NOTS, 13, 14, 15, 16, EOT]
    assert [r.end_row for r in records] == [4, 1, 3, 1] and [r.placed for r in records] == [3, 0, 2, 0]
    assert [r.next_seek for r in records] == [60, 160, 184, 284] and [r.last for r in records] == [False, False, True, True]
    assert all(b.seek > a.seek for a, b in zip(records, records[1:]))
    assert [w.word for w in out] == words and [w.line for w in out] == lines
    assert [w.aligned for w in out] == [True] * 3 + [True] * 2 + [False] * 4
    assert [(round(w.start, 6), round(w.end, 6)) for w in out[:5]] == [(0.0, 0.2), (0.2, 0.4), (0.4, 0.6), (1.6, 1.7), (1.7, 1.84)]
    assert all((w.start, w.end, w.probability) == (2.4, 2.4, 0.0) for w in out[5:])
    res = A.file_result(None, ["w0 w1 w2 w3 w4", "w5 w6 w7 w8"], out, 2.4)
    assert res["segments"][0]["aligned"] and (res["segments"][0]["start"], round(res["segments"][0]["end"], 6)) == (0.0, 1.84)
    assert not res["segments"][1]["aligned"] and len(res["words"]) == 9


def test_align_reference_with_nothing_to_do():
    def never(*a):
        raise AssertionError("no window is cut")
    kw = dict(window=100, seconds_per_frame=0.02, sot_sequence=SOT, no_timestamps=NOTS, eot=EOT)
    assert A.align_reference(never, [], [], [], 500, **kw) == []
    out = A.align_reference(never, [" a"], [[5]], [0], 0, **kw)
    assert len(out) == 1 and not out[0].aligned
    with pytest.raises(ValueError, match="max_tokens"):
        A.align_reference(never, [" a"], [[5, 6, 7]], [0], 500, options=A.AlignOptions(max_tokens=2), **kw)


# ---- plumbing -------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_refuse_null():
    header = open(os.path.join(ROOT, "include", "whisper_mi355.h")).read()
    lib = native.load_library()
    for name in ("wm_dtw_open", "wm_align_open", "wm_decoder_prefill_tap"):
        assert re.search(r"\bint %s\s*\(" % name, header) and name in native.EXPORTS and hasattr(lib, name)
    assert lib.wm_decoder_prefill_tap(None, None, None, None) == 1 and b"wm_decoder_prefill_tap" in lib.wm_last_error()
    assert lib.wm_align_open(None, None, None) == 1 and b"wm_align_open" in lib.wm_last_error()
    assert lib.wm_dtw_open(None, 0, 0, 0, None, None, 0, 0, None, None, 0, None, None, None, 0, None) == 1
    assert b"wm_dtw_open" in lib.wm_last_error()
