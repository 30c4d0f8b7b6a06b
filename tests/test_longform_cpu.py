"""Long-form transcription, the host contract (longform.py): the seek rule, the fallback rules, the literal loop and the batched
scheduler, on the CPU with scripted decoders -- tokens are a seeded function of (file, seek, temperature), so a decoder can be
asked again, in any order, and the scheduler is held to the literal loop segment for segment.

W = 3000 frames per window (n_audio_ctx 1500), fs = 0.01 s per frame: the timestamp token tb + k is k * 0.02 s, 2 k frames.
"""
import itertools

import numpy as np
import pytest

import longform as LF
from longform import WindowResult

TB = 50364                 # <|0.00|> of the multilingual vocabulary
W = 3000
FS = LF.CHUNK_LENGTH / W
A, B, C = 11, 22, 33       # text ids


def t(k):
    return TB + k


def cut(tokens, seek=0, size=W):
    return LF.cut_segments(tokens, TB, seek, size, FS)


def spans(segments):
    return [(round(s["start"], 6), round(s["end"], 6)) for s in segments]


# ------------------------------------------------------------------------------------------------------------- cut_segments
def test_cut_two_segments_closed_by_a_single_timestamp():
    segs, adv = cut([t(0), A, B, t(100), t(100), C, t(225)])
    assert spans(segs) == [(0.0, 2.0), (2.0, 4.5)] and adv == W
    assert segs[0]["tokens"] == [t(0), A, B, t(100)] and segs[1]["tokens"] == [t(100), C, t(225)]
    assert segs[0]["text"] == f"{A} {B}" and segs[1]["text"] == f"{C}"


def test_cut_drops_what_follows_the_last_pair():
    segs, adv = cut([t(0), A, t(100), t(100), B, t(200), t(200), C])
    assert spans(segs) == [(0.0, 2.0), (2.0, 4.0)] and adv == 400
    assert [s["tokens"] for s in segs] == [[t(0), A, t(100)], [t(100), B, t(200)]]
    assert all(C not in s["tokens"] for s in segs)


def test_cut_offsets_by_the_seek():
    segs, adv = cut([t(0), A, t(100), t(100), B, t(200), t(200), C], seek=1234, size=W)
    assert spans(segs) == [(12.34, 14.34), (14.34, 16.34)] and adv == 400 and all(s["seek"] == 1234 for s in segs)


def test_cut_without_pairs():
    segs, adv = cut([t(0), A, B])
    assert spans(segs) == [(0.0, 30.0)] and adv == W and segs[0]["tokens"] == [t(0), A, B]
    segs, adv = cut([t(0), A, t(150)])
    assert spans(segs) == [(0.0, 3.0)] and adv == W
    segs, adv = cut([t(0), A, B], seek=W, size=700)                  # a tail window: its own size
    assert spans(segs) == [(30.0, 37.0)] and adv == 700
    segs, adv = cut([A, B], size=500)                                # no timestamp at all
    assert spans(segs) == [(0.0, 5.0)] and adv == 500


def test_cut_empty_window_gives_one_cleared_segment():
    segs, adv = cut([])
    assert len(segs) == 1 and segs[0]["text"] == "" and segs[0]["tokens"] == [] and adv == W
    assert spans(segs) == [(0.0, 30.0)]


def test_cut_clears_blank_and_empty_segments_in_place():
    segs, adv = cut([t(0), t(50), t(50), A, t(80)])
    # flags T T T F T: pairs end at 1 and 2, a single ending -> [t0] 0.00-0.00, [t50] 1.00-1.00, [t50 A t80] 1.00-1.60
    assert [s["text"] for s in segs] == ["", "", f"{A}"] and [s["tokens"] for s in segs] == [[], [], [t(50), A, t(80)]]
    assert spans(segs) == [(0.0, 0.0), (1.0, 1.0), (1.0, 1.6)]
    assert adv == W
    segs, adv = cut([t(0), t(40), t(40), t(60)])                     # [t0], [t40], [t40]: all cleared; advance to the last pair
    assert spans(segs) == [(0.0, 0.0), (0.8, 0.8), (0.8, 0.8)] and all(s["tokens"] == [] for s in segs) and adv == 80
    segs, _ = LF.cut_segments([t(0), A, t(10)], TB, 0, W, FS, decode_text=lambda toks: "   ")
    assert segs[0]["text"] == "" and segs[0]["tokens"] == []


def test_cut_guard_against_standing_still_and_running_past_the_window():
    segs, adv = cut([t(0), t(0), A])
    assert adv == W and len(segs) == 1 and segs[0]["text"] == "" and segs[0]["tokens"] == []       # 0.00 - 0.00: cleared
    segs, adv = cut([t(0), A, t(1400), t(1400), B], size=700)        # 2 * 1400 frames > the 700 of this window
    assert adv == 700 and spans(segs) == [(0.0, 28.0)]
    segs, adv = cut([t(0), A, t(1501), t(1501)], size=W)             # an index beyond the window (random weights)
    assert adv == W
    segs, adv = cut([t(0), A, t(1500), t(1500)], size=W)             # exactly the window: not the guard's business
    assert adv == W
    segs, adv = cut([t(0), A, t(350), t(350)], size=700)             # exactly the tail window
    assert adv == 700


# -------------------------------------------------------------------------------------------------------------- truth tables
def res(cr=1.0, lp=-0.5, nsp=0.1, tokens=(), temperature=0.0):
    return WindowResult(tokens=list(tokens), avg_logprob=lp, no_speech_prob=nsp, compression_ratio=cr, temperature=temperature)


@pytest.mark.parametrize("crt,lpt,nst", list(itertools.product([None, 2.4], [None, -1.0], [None, 0.6])))
def test_needs_fallback_truth_table(crt, lpt, nst):
    for cr, lp, nsp in itertools.product([1.0, 3.0], [-0.5, -1.5], [0.1, 0.9]):
        want = (crt is not None and cr > crt) or (lpt is not None and lp < lpt)
        if nst is not None and lpt is not None and nsp > nst and lp < lpt:
            want = False
        assert LF.needs_fallback(res(cr, lp, nsp), crt, lpt, nst) == want, (cr, lp, nsp)


@pytest.mark.parametrize("lpt,nst", list(itertools.product([None, -1.0], [None, 0.6])))
def test_skip_window_truth_table(lpt, nst):
    for lp, nsp in itertools.product([-0.5, -1.5], [0.1, 0.9]):
        want = nst is not None and nsp > nst and not (lpt is not None and lp > lpt)
        assert LF.skip_window(res(1.0, lp, nsp), lpt, nst) == want, (lp, nsp)


def test_thresholds_are_strict():
    assert not LF.needs_fallback(res(cr=2.4, lp=-1.0), 2.4, -1.0, 0.6)
    assert not LF.skip_window(res(nsp=0.6, lp=-2.0), -1.0, 0.6)
    assert LF.skip_window(res(nsp=0.7, lp=-1.0), -1.0, 0.6)           # "likely enough anyway" is strict too


# -------------------------------------------------------------------------------------------------------- scripted decoders
def scripted(kind, seed=0):
    """decode(file, seek, temperature) -> WindowResult, a pure function of its arguments."""
    def decode(f, seek, temperature):
        rng = np.random.Generator(np.random.PCG64([seed, f, seek, int(round(temperature * 1000))]))
        n = int(rng.integers(0, 12))
        if kind == "timestamps":           # well-formed: pairs that advance, sometimes a single ending, sometimes running past the window
            toks, k = [t(0)], 0
            for _ in range(int(rng.integers(1, 4))):
                toks += [int(x) for x in rng.integers(1, 1000, size=int(rng.integers(0, 4)))]
                k += int(rng.integers(0, 700))
                toks += [t(k), t(k)]
            if rng.random() < 0.4:
                toks = toks[:-1]
        elif kind == "adversarial":        # anything: timestamps out of order, zeros, far beyond the window, nothing at all
            toks = [int(x) if rng.random() < 0.5 else t(int(rng.integers(0, 3)) * int(rng.integers(0, 2000))) for x in rng.integers(1, 1000, size=n)]
        else:                              # "still": the pair upstream never gets past
            toks = [t(0), t(0)]
        return WindowResult(tokens=toks, avg_logprob=float(-2.0 * rng.random()), no_speech_prob=float(rng.random()),
                            compression_ratio=float(1.0 + 2.5 * rng.random()), temperature=temperature)
    return decode


def reference(decode, f, content, log=None, **kw):
    def one(seek, temperature):
        if log is not None:
            log.append((f, seek, temperature))
        return decode(f, seek, temperature)
    return LF.transcribe_reference(one, content, window=W, timestamp_begin=TB, **kw)


# ----------------------------------------------------------------------------------------------------- transcribe_reference
@pytest.mark.parametrize("kind", ["timestamps", "adversarial", "still"])
def test_reference_terminates_and_covers_the_file(kind):
    for content in (0, 1, W - 1, W, W + 1, 5 * W + 17):
        log = []
        segs = reference(scripted(kind, 3), 0, content, log)
        seeks = sorted({s for _, s, _ in log})
        assert (content == 0) == (not log) and (content > 0 or segs == [])
        assert all(0 <= s < content for s in seeks) and len(log) <= 6 * max(content, 1)
        assert all(s["seek"] in seeks for s in segs)
        assert [s["seek"] for s in segs] == sorted(s["seek"] for s in segs)


def test_reference_tail_window_has_its_own_size():
    """content = W + 700, no timestamps: two windows, the second 700 frames long -- its segment ends at the end of the file."""
    dec = lambda f, seek, temp: res(tokens=[t(0), A, B])
    segs = reference(dec, 0, W + 700, temperatures=(0.0,))
    assert spans(segs) == [(0.0, 30.0), (30.0, 37.0)]


def test_reference_skips_silent_windows():
    def dec(f, seek, temp):
        return res(tokens=[t(0), A, t(100), t(100)], nsp=0.9 if seek == 200 else 0.1, lp=-1.5 if seek == 200 else -0.2)
    log = []
    segs = reference(dec, 0, 1000, log)
    # window at 200 is silence: no fallback (one call), no segment, and the seek jumps by the whole rest, 800 frames
    assert [s for _, s, _ in log] == [0, 200] and [s["seek"] for s in segs] == [0]
    log = []
    segs = reference(dec, 0, 1000, log, no_speech_threshold=None, temperatures=(0.0, 0.5))
    assert (0, 200, 0.5) in log and 200 in [s["seek"] for s in segs]              # without the threshold: a fallback, a segment


def test_reference_ladder_stops_at_the_first_pass_and_keeps_the_last():
    ladder = (0.0, 0.2, 0.4, 0.6)

    def dec_pass_at(k):
        return lambda f, seek, temp: res(tokens=[t(0), A, t(50)], lp=-0.5 if temp >= ladder[k] else -3.0, temperature=temp)
    for k in range(4):
        log = []
        segs = reference(dec_pass_at(k), 0, W, log, temperatures=ladder)
        assert [x[2] for x in log] == list(ladder[:k + 1]) and segs[0]["temperature"] == ladder[k]
    log = []
    segs = reference(lambda f, seek, temp: res(tokens=[t(0), A, t(50)], lp=-3.0, temperature=temp), 0, W, log, temperatures=ladder)
    assert [x[2] for x in log] == list(ladder) and segs[0]["temperature"] == 0.6 and segs[0]["avg_logprob"] == -3.0
    with pytest.raises(ValueError):
        reference(dec_pass_at(0), 0, W, temperatures=(0.0, 0.0))


# ------------------------------------------------------------------------------------------------------- transcribe_batched
CONTENTS = [0, 1, W - 1, W, W + 1, 5 * W + 17, 2 * W, 0, 3 * W + 5, 7, W]       # more files than rows, for every n_rows below


@pytest.mark.parametrize("kind", ["timestamps", "adversarial", "still"])
@pytest.mark.parametrize("n_rows", [1, 3, 8])
@pytest.mark.parametrize("thresholds", [dict(), dict(compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None),
                                        dict(temperatures=(0.0,))])
def test_batched_equals_the_reference(kind, n_rows, thresholds):
    decode = scripted(kind, 5)
    ref_log = []
    want = [reference(decode, f, c, ref_log, **thresholds) for f, c in enumerate(CONTENTS)]
    calls = []

    def decode_call(rows, temperature, live):
        assert len(rows) == n_rows and len(live) == n_rows
        assert all(r is not None for r, on in zip(rows, live) if on), "a live row without a file"
        calls.append((list(rows), temperature, list(live)))
        return [decode(r[0], r[1], temperature) if on else None for r, on in zip(rows, live)]

    got = LF.transcribe_batched(decode_call, CONTENTS, n_rows, window=W, timestamp_begin=TB, **thresholds)
    assert got == want
    asked = [(r[0], r[1], temp) for rows, temp, live in calls for r, on in zip(rows, live) if on]
    assert len(asked) == len(set(asked)), "a (file, seek, temperature) was asked twice"
    assert set(asked) == set(ref_log)
    # per round: one call at the first temperature with every occupied row live, then calls over the SAME rows, rising temperature,
    # live rows a subset of those that were live before; a file sits in one row at a time and files start in order
    ladder = thresholds.get("temperatures", LF.TEMPERATURES)
    first = None
    for rows, temp, live in calls:
        if temp == ladder[0]:
            first, prev_live, prev_temp = rows, live, temp
            assert live == [r is not None for r in rows]
            files = [r[0] for r in rows if r is not None]
            assert len(files) == len(set(files)) and files
        else:
            assert rows == first and temp > prev_temp and any(live)
            assert all(p or not l for p, l in zip(prev_live, live))
            prev_live, prev_temp = live, temp
    started = [r[0] for rows, temp, _ in calls if temp == ladder[0] for r in rows if r is not None and r[1] == 0]
    assert started == [f for f, c in enumerate(CONTENTS) if c > 0]
    # a row keeps its file until the file is done
    row_of = {}
    for rows, temp, _ in calls:
        for i, r in enumerate(rows):
            if r is not None:
                assert row_of.setdefault(r[0], i) == i


def test_batched_without_content():
    def never(rows, temperature, live):
        raise AssertionError("nothing to decode")
    assert LF.transcribe_batched(never, [0, 0], 3, window=W, timestamp_begin=TB) == [[], []]
    assert LF.transcribe_batched(never, [], 2, window=W, timestamp_begin=TB) == []
    with pytest.raises(ValueError):
        LF.transcribe_batched(never, [5], 0, window=W, timestamp_begin=TB)


# ------------------------------------------------------------------------------------------------- transcribe.py, host side
def test_cli_arguments_timestamps_and_refusals():
    import types

    import transcribe as T
    args = T.parse_arguments(["--engine_dir", "eng", "--input_file", "a.flac", "b.wav", "--vocab", "v.tiktoken", "--temperature", "0", "0.4"])
    assert args.input_file == ["a.flac", "b.wav"] and args.temperature == [0.0, 0.4] and not args.no_fallback
    assert T.parse_arguments(["--input_file", "a.flac", "--no_fallback"]).temperature == list(LF.TEMPERATURES)
    assert [T.format_timestamp(x) for x in (0.0, 2.5, 59.9996, 75.5, 3723.004)] == ["00:00.000", "00:02.500", "01:00.000", "01:15.500", "62:03.004"]

    def instance(**options):
        opt = types.SimpleNamespace(**{**dict(prompt=None, prefix=None, temperature=0.0), **options})
        return types.SimpleNamespace(options=opt, beam=options.get("beam_size") is not None,
                                     n_group=options.get("beam_size") or options.get("best_of") or 1)
    T.check_supported(instance(), LF.TEMPERATURES)
    T.check_supported(instance(beam_size=5), (0.0,))                  # the instance's own temperature: fine, no fallback
    for bad, kw in ((instance(prompt="x"), {}), (instance(prefix=[1]), {}), (instance(), dict(condition_on_previous_text=True)),
                    (instance(beam_size=5), {}), (instance(best_of=3, temperature=0.5), {}), (instance(beam_size=2), dict(t=(0.2,)))):
        with pytest.raises(ValueError):
            T.check_supported(bad, kw.pop("t", LF.TEMPERATURES), **kw)
