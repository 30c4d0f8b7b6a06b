"""Skip silence on the host: the contract of speech.py, which the device (csrc/speech.hip,
tests/test_gpu_speech.py) is held to bit for bit.

* the spans against a second, independent statement written here FRAME BY FRAME in Python integers: the floor by counting (no
  sort), and for every frame on its own whether it survives rule (b), (c) and (d) -- no list of spans is ever joined or dropped;
* the edges: F in {0, 1, 2}, permille 0 and 1000, all-equal s, s - floor == M and M - 1, gap == min_silence and one less, length ==
  min_speech and one less, pads clipped at 0 and F, a pad that joins and one that makes spans touch exactly, non-finite and
  +-65504 values, smoothing wider than the file;
* packed_mel_ref, taken_spans, restore (joints for starts and ends, a word across a joint, seek, times beyond P, inputs
  untouched, restore of a packed segment inside one span = that span's shift);
* SpeechOptions.frames and its refusals; the header, the exports; the CLI flags;
* the schedule: longform.transcribe_batched over packed files with a scripted decoder, restored.
"""
import copy
import os

import numpy as np
import pytest

import longform as LF
import native
import sections as S
import speech as SP
from longform import WindowResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rng_of(seed):
    return np.random.Generator(np.random.Philox(seed))


# ------------------------------------------------------------------------------------------------ the independent statement
def frame_by_frame(mel, F, h, step, permille, min_silence, min_speech, pad):
    """(spans, facts): the contract once more, one frame at a time in Python integers."""
    n_mels = mel.shape[0]
    q = []
    for t in range(F):
        acc = 0
        for m in range(n_mels):
            x = float(mel[m, t])
            if x != x or x in (float("inf"), float("-inf")):
                continue
            acc += round(max(-16.0, min(16.0, x)) * 1024.0)          # exact product; Python rounds halves to even
        q.append(acc)
    s = [sum(q[min(max(t + d, 0), F - 1)] for d in range(-h, h + 1)) for t in range(F)]
    facts = dict(joined_gaps=0, dropped=0, pad_joins=0)
    if F == 0:
        return [], facts
    r = min(F - 1, F * permille // 1000)
    floor = next(x for x in s if sum(1 for y in s if y < x) <= r < sum(1 for y in s if y <= x))       # selection is counting
    M = n_mels * (2 * h + 1) * step
    v = [s[t] - floor >= M for t in range(F)]

    def run_around(keep, t):
        """[a, b): the maximal run of frames u with keep[u] == keep[t] that holds t."""
        a = t
        while a > 0 and keep[a - 1] == keep[t]:
            a -= 1
        b = t + 1
        while b < F and keep[b] == keep[t]:
            b += 1
        return a, b

    # (b) a frame survives if it is flagged, or lies in a gap shorter than min_silence BETWEEN two flagged frames
    after_b = []
    for t in range(F):
        if v[t]:
            after_b.append(True)
            continue
        a, b = run_around(v, t)
        after_b.append(a > 0 and b < F and b - a < min_silence)
    # (c) ... and if the run of survivors around it is at least min_speech long
    after_c = []
    for t in range(F):
        a, b = run_around(after_b, t)
        after_c.append(after_b[t] and b - a >= min_speech)
    # (d) ... and a frame is speech if a survivor lies within pad frames of it
    final = [any(after_c[u] for u in range(max(0, t - pad), min(F, t + pad + 1))) for t in range(F)]
    spans = [run_around(final, t) for t in range(F) if final[t] and (t == 0 or not final[t - 1])]
    gaps = [run_around(v, t) for t in range(F) if not v[t] and (t == 0 or v[t - 1])]
    facts["joined_gaps"] = sum(1 for a, b in gaps if a > 0 and b < F and b - a < min_silence)
    facts["dropped"] = sum(1 for t in range(F) if after_b[t] and (t == 0 or not after_b[t - 1]) and not after_c[t])
    kept = sum(1 for t in range(F) if after_c[t] and (t == 0 or not after_c[t - 1]))
    facts["pad_joins"] = kept - len(spans)
    return spans, facts


def bursty_mel(rng, n_mels, ld, F, amplitude):
    """Quiet noise with loud bursts of 1 .. 40 frames 1 .. 40 frames apart: every rule of (b), (c), (d) has work."""
    mel = (rng.standard_normal((n_mels, ld)) * 0.05 - 2.0).astype(np.float16)
    t = int(rng.integers(0, 20))
    while t < F:
        n = int(rng.integers(1, 40))
        mel[:, t:t + n] = (rng.standard_normal((n_mels, min(ld, t + n) - t)) * 0.2 + amplitude).astype(np.float16)
        t += n + int(rng.integers(1, 40))
    return mel


CASES = [(seed, n_mels, amplitude) for seed in range(6) for n_mels, amplitude in ((1, 1.0), (3, 0.5), (80, -1.0))]
CFG = (2, 205, 100, 12, 8, 7)             # 2 * pad >= min_silence: a pad can join what (b) kept apart


def test_spans_equal_the_frame_by_frame_statement():
    totals = dict(joined_gaps=0, dropped=0, pad_joins=0)
    multi = 0
    for seed, n_mels, amplitude in CASES:
        rng = rng_of(1000 + seed)
        F = 400 + 37 * seed
        mel = bursty_mel(rng, n_mels, F + 3, F, amplitude)
        want, facts = frame_by_frame(mel, F, *CFG)
        got = SP.speech_spans_ref(mel, F, *CFG)
        assert got == want, (seed, n_mels)
        SP.check_spans(got, F)
        assert len(want) >= 2, "a multi-span case with fewer than two surviving spans"
        multi += 1
        for k in totals:
            totals[k] += facts[k]
    # the reference alone has met every rule, so a detector that returns nothing cannot pass by agreeing with nothing
    assert multi == len(CASES) and totals["joined_gaps"] >= 1 and totals["dropped"] >= 1 and totals["pad_joins"] >= 1, totals


@pytest.mark.parametrize("cfg", [(0, 1, 0, 1, 1, 0), (0, 32768, 1000, 3, 2, 1), (50, 100, 500, 7, 7, 100), (1, 300, 250, 2, 3, 0)])
def test_other_parameters_and_small_files(cfg):
    rng = rng_of(sum(cfg))
    for F in (0, 1, 2, 3, 50, 333):
        for n_mels in (1, 3):
            mel = bursty_mel(rng, n_mels, max(1, F + int(rng.integers(0, 3))), F, 1.0)
            assert SP.speech_spans_ref(mel, F, *cfg) == frame_by_frame(mel, F, *cfg)[0], (F, n_mels)


def planted(n_mels, F, spans, loud=1.0, quiet=-2.0):
    mel = np.full((n_mels, max(F, 1)), quiet, dtype=np.float16)
    for a, b in spans:
        mel[:, a:b] = np.float16(loud)
    return mel


def both(mel, F, cfg):
    got = SP.speech_spans_ref(mel, F, *cfg)
    assert got == frame_by_frame(mel, F, *cfg)[0]
    return got


def test_edges():
    n_mels, F = 3, 600
    assert SP.speech_spans_ref(np.zeros((3, 5), dtype=np.float16), 0, 0, 100, 0, 5, 1, 3) == []            # F == 0
    for F2 in (1, 2):
        for permille in (0, 1000):
            assert both(np.full((3, F2), 1.0, dtype=np.float16), F2, (0, 100, permille, 5, 1, 3)) == []   # all equal: no flag
    assert both(planted(3, 2, [(1, 2)]), 2, (0, 100, 0, 5, 1, 0)) == [(1, 2)]
    assert both(planted(3, 2, [(1, 2)]), 2, (0, 100, 1000, 5, 1, 0)) == []                                  # the floor is the maximum
    assert both(planted(3, 600, [(0, 599)]), 600, (0, 100, 0, 5, 1, 1)) == [(0, 600)]                       # the pad closes the file
    # s - floor == M stays, M - 1 goes (h = 0, step 100: M = 300; a bin at k / 1024 adds k)
    mel = np.zeros((n_mels, F), dtype=np.float16)
    mel[0, 100:110] = np.float16(300 / 1024)
    mel[0, 200:210] = np.float16(299 / 1024)
    assert both(mel, F, (0, 100, 0, 5, 2, 0)) == [(100, 110)]
    # gap == min_silence stays a gap, one less is joined; length == min_speech stays, one less goes
    cfg = (0, 100, 0, 5, 4, 0)
    assert both(planted(3, F, [(10, 20), (25, 30), (34, 40)]), F, cfg) == [(10, 20), (25, 40)]
    assert both(planted(3, F, [(10, 14), (50, 53), (100, 102), (106, 108)]), F, cfg) == [(10, 14), (100, 108)]
    # (b) comes before (c): two short runs join into one that is long enough; (c) before (d): a dropped span pads nothing
    assert both(planted(3, F, [(10, 12), (14, 16)]), F, cfg) == [(10, 16)]
    assert both(planted(3, F, [(10, 13), (100, 110)]), F, (0, 100, 0, 5, 4, 50)) == [(50, 160)]
    # pads: clipped at 0 and at F, joining, touching exactly, one frame short of touching
    for spans, pad, want in (([(2, 10), (590, 598)], 5, [(0, 15), (585, 600)]), ([(100, 110), (130, 140)], 10, [(90, 150)]),
                             ([(100, 110), (131, 140)], 10, [(90, 120), (121, 150)]), ([(100, 110), (120, 140)], 10, [(90, 150)])):
        assert both(planted(3, F, spans), F, (0, 100, 0, 5, 2, pad)) == want
    # smoothing wider than the file; non-finite and huge values count as sections.loudness says
    rng = rng_of(5)
    short = bursty_mel(rng, 3, 9, 9, 1.0)
    both(short, 9, (50, 100, 100, 2, 1, 1))
    mel = bursty_mel(rng, 4, 300, 300, 1.0)
    what = np.array([np.inf, -np.inf, np.nan, 65504.0, -65504.0, 16.0, 17.0, 2.0 ** -11, 3 * 2.0 ** -11], dtype=np.float16)
    mel[rng.integers(0, 4, size=80), rng.integers(0, 300, size=80)] = what[rng.integers(0, len(what), size=80)]
    both(mel, 300, CFG)
    nothing = np.full((3, 100), np.nan, dtype=np.float16)
    assert both(nothing, 100, CFG) == []
    # the difference of two 32-bit sums needs 64 bits: s from -2^31 + ... to 2^31 - ...
    wide = np.full((128, 2100), -16.0, dtype=np.float16)
    wide[:, 1050:] = np.float16(16.0)
    h = 511                                                                      # 128 * 1023 = 130944 < 131072
    s = S.smooth(S.loudness(wide, 2100), h)
    assert int(s.max()) - int(s.min()) == 130944 * 32768 > 2 ** 32 - 2 ** 24     # == M at the largest step: the frames wholly on the right
    assert both(wide, 2100, (h, 32768, 0, 1, 1, 0)) == [(1050 + h, 2100)]


def test_floor_is_an_exact_order_statistic():
    rng = rng_of(9)
    s = rng.integers(-2 ** 31, 2 ** 31, size=1000)
    for permille in (0, 1, 500, 999, 1000):
        assert SP.floor_of(s, permille) == sorted(s.tolist())[min(999, permille)]
    assert SP.floor_of(np.array([7]), 1000) == 7 and SP.floor_of(np.array([3, 3, 3]), 500) == 3


# ------------------------------------------------------------------------------------------------- packed mel, taken spans
def test_packed_mel_ref_and_taken_spans():
    rng = rng_of(3)
    W, F = 16, 70
    mel = (rng.standard_normal((5, F + W)) * 2.0).astype(np.float16)
    mel[:, F:] = mel[:, -1:]                                                    # what a whole-file mel ends in: W equal frames
    spans = [(3, 10), (20, 21), (40, 70)]
    packed = SP.packed_mel_ref(mel, F, spans, W)
    assert packed.shape == (5, 38 + W) and packed.dtype == np.float16 and SP.packed_starts(spans) == [0, 7, 8, 38]
    assert np.array_equal(packed[:, :7], mel[:, 3:10]) and np.array_equal(packed[:, 7], mel[:, 20]) and np.array_equal(packed[:, 8:38], mel[:, 40:70])
    assert all(np.array_equal(packed[:, 38 + j], mel[:, -1]) for j in range(W))
    assert SP.packed_mel_ref(mel, F, [], W).shape == (5, W)
    assert np.array_equal(SP.packed_mel_ref(mel, F, [(0, F)], W), mel)           # everything speech: the file itself
    for bad in ([(10, 3)], [(0, 71)], [(0, 10), (10, 20)], [(20, 30), (0, 10)], [(-1, 5)]):
        with pytest.raises(ValueError):
            SP.packed_mel_ref(mel, F, bad, W)
    assert SP.taken_spans(spans, 86) == spans
    assert SP.taken_spans([(3, 10), (50, 90), (20, 21), (-5, 2), (15, 12), (40, 70)], 86) == [(3, 10), (20, 21), (40, 70)]
    assert SP.taken_spans([(3, 10), (5, 30), (20, 21), (40, 70)], 86) == [(3, 10), (40, 70)]      # in range, out of order: it still bars


# ------------------------------------------------------------------------------------------------------------------- restore
FS = 0.25
SPANS = [(10, 30), (100, 140), (500, 520)]               # packed starts 0, 20, 60; P = 80; shifts 10, 80, 440 frames


def seg(seek, start, end, **kw):
    return dict(seek=seek, start=start, end=end, text="x", tokens=[1, 2], **kw)


def test_restore_rules():
    a = seg(0, 0.0, 5.0)                                  # 5.0 s = frame 20: an end on the joint stays with span 0
    b = seg(20, 5.0, 15.0)                                # a start on the joint goes to span 1; 15.0 s = frame 60: end with span 1
    c = seg(60, 15.0, 19.0)
    d = seg(70, 19.0, 30.0)                               # an end beyond P = 80 frames (20 s) stays beyond the content
    before = copy.deepcopy([a, b, c, d])
    out = SP.restore([a, b, c, d], SPANS, FS)
    assert [a, b, c, d] == before and out[0] is not a
    assert (out[0]["seek"], out[0]["start"], out[0]["end"]) == (10, 2.5, 7.5)
    assert (out[1]["seek"], out[1]["start"], out[1]["end"]) == (100, 25.0, 35.0)
    assert (out[2]["seek"], out[2]["start"], out[2]["end"]) == (500, 125.0, 129.0)
    assert (out[3]["seek"], out[3]["start"], out[3]["end"]) == (510, 129.0, 140.0) and 140.0 > 520 * FS
    assert all(o["tokens"] == [1, 2] and o["text"] == "x" for o in out)
    assert SP.restore_time(5.0, SPANS, FS) == 25.0 and SP.restore_time(5.0, SPANS, FS, end=True) == 7.5
    assert SP.restore_time(0.0, SPANS, FS, end=True) == 2.5 and SP.restore_time(-1.0, SPANS, FS) == 1.5      # k clamped to 0
    assert SP.restore([a], [], FS) == [a] and SP.restore([], SPANS, FS) == [] and SP.restore_time(3.0, [], FS) == 3.0


def test_restore_words_by_their_midpoint():
    words = [dict(word=" a", start=4.0, end=4.75, probability=0.5),      # inside span 0
             dict(word=" b", start=4.75, end=5.5, probability=0.5),      # straddles the joint at 5.0, midpoint 5.125: span 1, both ends
             dict(word=" c", start=4.5, end=5.25, probability=0.5),      # straddles it, midpoint 4.875: span 0, both ends
             dict(word=" d", start=4.5, end=5.5, probability=0.5)]       # midpoint ON the joint: the start rule, span 1
    s = seg(0, 4.0, 5.5, words=copy.deepcopy(words))                      # start and end are the first and last word's
    t = seg(0, 3.0, 6.0, words=copy.deepcopy(words))                      # ... and here they are not: the timestamp tokens' rules
    before = copy.deepcopy([s, t])
    out = SP.restore([s, t], SPANS, FS)
    assert [s, t] == before
    for o in out:
        got = [(w["start"], w["end"]) for w in o["words"]]
        assert got == [(6.5, 7.25), (24.75, 25.5), (7.0, 7.75), (24.5, 25.5)]
        assert [w["word"] for w in o["words"]] == [" a", " b", " c", " d"] and all(w["probability"] == 0.5 for w in o["words"])
    assert (out[0]["start"], out[0]["end"]) == (6.5, 25.5)               # the restored first and last word
    assert (out[1]["start"], out[1]["end"]) == (5.5, 26.0)               # 3.0 in span 0, 6.0 in span 1
    assert SP.restore([seg(0, 1.0, 2.0, words=[])], SPANS, FS)[0]["words"] == []


def test_restore_of_a_packed_segment_is_the_identity_shift():
    """A segment that lies inside span k of the ORIGINAL file, written in packed time, comes back where it was."""
    P = SP.packed_starts(SPANS)
    for k, (a, b) in enumerate(SPANS):
        for u, v in ((a, b), (a + 1, b - 1), (a, a + 1)):
            packed = seg(P[k] + (u - a), (P[k] + (u - a)) * FS, (P[k] + (v - a)) * FS,
                         words=[dict(word=" w", start=(P[k] + (u - a)) * FS, end=(P[k] + (v - a)) * FS, probability=1.0)])
            back = SP.restore([packed], SPANS, FS)[0]
            assert (back["seek"], back["start"], back["end"]) == (u, u * FS, v * FS)
            assert (back["words"][0]["start"], back["words"][0]["end"]) == (u * FS, v * FS)


# ------------------------------------------------------------------------------------------------------------------ schedule
W, TB = 100, 1000


@pytest.mark.parametrize("n_rows", [1, 3])
def test_schedule_over_packed_files(n_rows):
    """Files of 0, 900, 90 and 400 frames with planted quiet stretches: the packed files are the scheduler's files, and the
    restored result is what the stub decoder said, moved: every seek is a frame of a span, no start lies in a removed stretch."""
    cfg = (0, 100, 0, 30, 5, 10)
    plants = [[], [(50, 300), (400, 420), (600, 880)], [], [(0, 100), (350, 400)]]
    contents = [0, 900, 90, 400]
    spans = [SP.speech_spans_ref(planted(3, F, p), F, *cfg) for F, p in zip(contents, plants)]
    assert spans == [[], [(40, 310), (390, 430), (590, 890)], [], [(0, 110), (340, 400)]]
    packed = [SP.packed_starts(sp)[-1] for sp in spans]
    assert packed == [0, 610, 0, 170]
    asked = []

    def decode_call(rows, temperature, live):
        out = []
        for r, on in zip(rows, live):
            if r is None or not on:
                out.append(None)
                continue
            asked.append(r)
            out.append(WindowResult(tokens=[TB, 5, TB + 30, TB + 30], avg_logprob=-0.5, temperature=temperature))      # advance 60 frames
        return out

    segments = LF.transcribe_batched(decode_call, packed, n_rows, window=W, timestamp_begin=TB, temperatures=(0.0,),
                                     compression_ratio_threshold=None, no_speech_threshold=None)
    fs = LF.CHUNK_LENGTH / W
    assert {f for f, _ in asked} == {1, 3}                                       # files without speech never take a row
    assert sorted(k for f, k in asked if f == 1) == list(range(0, 610, 60)) and sorted(k for f, k in asked if f == 3) == [0, 60, 120]
    for f, sp in enumerate(spans):
        out = SP.restore(segments[f], sp, fs)
        assert len(out) == len(segments[f]) and (len(out) > 0) == (f in (1, 3))
        P = SP.packed_starts(sp)
        for o, s in zip(out, segments[f]):
            k = max(i for i in range(len(sp)) if P[i] <= s["seek"])
            assert o["seek"] == s["seek"] + sp[k][0] - P[k] and sp[k][0] <= o["seek"] < sp[k][1]
            assert any(a * fs <= o["start"] < b * fs for a, b in sp), "a segment begins in a stretch that was removed"
            assert o["tokens"] == s["tokens"] and o["end"] - o["start"] >= s["end"] - s["start"] - 1e-9
        assert [o["seek"] for o in out] == sorted(o["seek"] for o in out)


# ------------------------------------------------------------------------------------------------------------ ABI and options
def test_speech_options():
    assert SP.SpeechOptions() == SP.SpeechOptions(8.0, 10.0, 0.2, 2.0, 0.25, 0.4)
    assert SP.SpeechOptions().frames(3000, 80) == (10, 205, 100, 200, 25, 40)   # 8 dB = 0.2 units of log-mel = 204.8 steps
    assert SP.SpeechOptions().frames(3000, 128) == (10, 205, 100, 200, 25, 40)
    assert SP.SpeechOptions().frames(128, 80) == (0, 205, 100, 9, 1, 2)         # a micro engine: 128 frames are 30 s
    assert SP.SpeechOptions(min_silence_seconds=0.0, min_speech_seconds=0.0, speech_pad_seconds=0.0).frames(3000)[3:] == (1, 1, 0)
    assert SP.SpeechOptions(margin_db=1280.0).frames(3000, 80)[1] == 32768
    for bad in (SP.SpeechOptions(margin_db=0.0), SP.SpeechOptions(margin_db=-3.0), SP.SpeechOptions(margin_db=1281.0),
                SP.SpeechOptions(floor_percent=-1.0), SP.SpeechOptions(floor_percent=100.1), SP.SpeechOptions(speech_pad_seconds=-1.0),
                SP.SpeechOptions(smooth_seconds=-0.1), SP.SpeechOptions(smooth_seconds=20.0), SP.SpeechOptions(min_silence_seconds=-1.0)):
        with pytest.raises(ValueError):
            bad.frames(3000, 80)
    SP.SpeechOptions(smooth_seconds=16.0).frames(3000, 80)                       # 80 * 1601 = 128080 < 131072
    with pytest.raises(ValueError):
        SP.SpeechOptions().frames(0, 80)
    with pytest.raises(ValueError):
        SP.speech_spans_ref(np.zeros((3, 5), dtype=np.float16), 5, 0, 0, 0, 1, 1, 0)
    with pytest.raises(ValueError):
        SP.speech_spans_ref(np.zeros((3, 5), dtype=np.float32), 5, 0, 1, 0, 1, 1, 0)
    assert "not measurements" in SP.SpeechOptions.__doc__ and "untuned" in SP.SpeechOptions.__doc__
    with pytest.raises(Exception):
        SP.SpeechOptions().margin_db = 3.0                                       # frozen


def test_header_exports_and_abi():
    header = open(os.path.join(ROOT, "include", "whisper_mi355.h")).read()
    assert "int wm_speech_spans(" in header and "size_t wm_speech_spans_workspace_bytes(" in header and "int wm_mel_gather(" in header
    assert "#define WM_ABI_VERSION 8" in header and native.ABI_VERSION == 8
    assert all(n in native.EXPORTS for n in ("wm_speech_spans", "wm_speech_spans_workspace_bytes", "wm_mel_gather"))
    csrc = os.path.join(ROOT, "eddie-wang-hackathon2023_amd", "csrc")
    assert "speech.hip" in open(os.path.join(csrc, "Makefile")).read()
    # one definition of the loudness arithmetic: both kernels files include it, neither restates it
    for name in ("sections.hip", "speech.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "loudness.h"' in text and "rintf" not in text
    assert "rintf" in open(os.path.join(csrc, "loudness.h")).read()


def test_the_library_exports_the_entries():
    lib = native.load_library()
    assert lib.wm_version() == 8
    assert hasattr(lib, "wm_speech_spans") and hasattr(lib, "wm_mel_gather")
    assert lib.wm_speech_spans_workspace_bytes(1, 100) >= 16 + 4 * 400 and lib.wm_speech_spans_workspace_bytes(0, 100) == 0


def test_cli_arguments_and_signature():
    import inspect

    import transcribe as T
    args = T.parse_arguments(["--input_file", "a.flac", "--skip_silence", "--silence_margin_db", "6", "--min_silence_seconds", "1",
                              "--min_speech_seconds", "0.5", "--speech_pad_seconds", "0.2"])
    assert args.skip_silence and (args.silence_margin_db, args.min_silence_seconds, args.min_speech_seconds, args.speech_pad_seconds) == (6.0, 1.0, 0.5, 0.2)
    args = T.parse_arguments(["--input_file", "a.flac"])
    assert not args.skip_silence and (args.silence_margin_db, args.min_silence_seconds, args.min_speech_seconds, args.speech_pad_seconds) == (8.0, 2.0, 0.25, 0.4)
    assert inspect.signature(T.transcribe_mel).parameters["speech"].default is None
