"""Channels on the host: the contract of channels.py, which the device (csrc/channels.hip,
csrc/resample.hip, tests/test_gpu_channels.py) is held to bit for bit.

* rules 2 .. 4 against a second statement written here FRAME BY FRAME in Python integers (loudness term by term, the smoothing
  tap by tap, the key from the bits), over C in {1, 2, 3, 8}, F in {0, 1, 2h, 2h + 1} and beyond, h in {0, 3};
* hand cases: ties go to the lowest channel, a difference of exactly G gates and of G - 1 does not, NaN / infinities count as 0
  and never become v_c, a channel without a finite element is never gated, -0 sorts below +0, columns at or beyond F stay;
* rule 5: the seconds-to-frames rule, majorities, ties, a span without frames; rule 6: merge order with equal starts, turns;
* ChannelOptions and every refusal (before any device work: the calls below pass no engine at all); the CLI flags; the header;
* rule 1 against resample_reference of the single column, and at 16 kHz against _mono_at_sr.

Everything is exact: integers, fp16 bit patterns, or one fp64 expression evaluated twice.
"""
import copy
import math
import os
import re

import numpy as np
import pytest

import channels as CH
import native
import sections as S
import speech as SP
import transcribe as T
import whisper_utils as wu
from channels import ChannelOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rng_of(seed):
    return np.random.Generator(np.random.Philox(seed))


def bits_of(x):
    return np.asarray(x, dtype=np.float16).view(np.int16)


# ------------------------------------------------------------------------------------------------ the independent statement
def frame_by_frame(mels, F, h, step):
    """(top, counts, gated mels) once more, one frame at a time in Python integers."""
    C, n_mels = len(mels), mels[0].shape[0]
    s = []
    for mel in mels:
        q = []
        for t in range(F):
            acc = 0
            for m in range(n_mels):
                v = float(mel[m, t])
                if math.isfinite(v):
                    acc += int(np.rint(np.float32(min(max(v, -16.0), 16.0)) * np.float32(1024)))
            q.append(acc)
        s.append([sum(q[min(max(t + d, 0), F - 1)] for d in range(-h, h + 1)) for t in range(F)])
    top = [min(c for c in range(C) if s[c][t] == max(s[k][t] for k in range(C))) for t in range(F)]
    out, counts = [m.copy() for m in mels], [0] * C
    if step > 0 and C > 1:
        G = n_mels * (2 * h + 1) * step
        for c, mel in enumerate(mels):
            best = None
            for m in range(n_mels):
                for t in range(F):
                    b = int(bits_of(mel[m, t]))
                    if (b & 0x7c00) == 0x7c00:
                        continue
                    key = b if b >= 0 else b ^ 0x7fff
                    if best is None or key < best[0]:
                        best = (key, mel[m, t])
            if best is None:
                continue
            for t in range(F):
                if max(s[k][t] for k in range(C) if k != c) - s[c][t] >= G:
                    counts[c] += 1
                    out[c][:, t] = best[1]
    return np.array(top, dtype=np.uint8), counts, out


def random_recording(rng, C, n_mels, ld, F):
    mels = [(rng.standard_normal((n_mels, ld)) * 0.5 + rng.uniform(-2, 1)).astype(np.float16) for _ in range(C)]
    for m in mels:                                                   # loud stretches, and some values nothing should trust
        a = int(rng.integers(0, max(1, F)))
        m[:, a: a + max(1, F // 3)] += np.float16(1.5)
        if F:
            m[rng.integers(0, n_mels, size=4), rng.integers(0, F, size=4)] = np.array([np.nan, np.inf, -np.inf, -0.0], dtype=np.float16)
    return mels


def same_bits(a, b):
    return all(x.shape == y.shape and np.array_equal(bits_of(x), bits_of(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("h", [0, 3])
@pytest.mark.parametrize("C", [1, 2, 3, 8])
def test_rules_2_to_4_equal_the_frame_by_frame_statement(C, h):
    rng = rng_of(100 * C + h)
    for F in sorted({0, 1, 2 * h, 2 * h + 1, 40}):
        for n_mels in (1, 5):
            mels = random_recording(rng, C, n_mels, F + 3, F)
            for step in (0, 1, 300):
                before = [m.copy() for m in mels]
                top, counts, out = CH.channel_top_ref(mels, F, h, step)
                want = frame_by_frame(mels, F, h, step)
                assert top.dtype == np.uint8 and np.array_equal(top, want[0]) and counts == want[1] and same_bits(out, want[2]), (C, h, F, n_mels, step)
                assert same_bits(mels, before)                       # the inputs are not modified
                assert all(np.array_equal(bits_of(o[:, F:]), bits_of(m[:, F:])) for o, m in zip(out, mels))
                if step == 0 or C == 1 or F == 0:
                    assert counts == [0] * C and same_bits(out, mels)
                assert np.array_equal(CH.from_run_lengths(CH.run_lengths(top)), top)


def test_ties_go_to_the_lowest_channel_and_G_is_sharp():
    n_mels, F, h, step = 3, 6, 0, 100
    G = CH.gate_threshold(n_mels, h, step)
    assert G == 300
    a = np.zeros((n_mels, F), dtype=np.float16)
    b = np.zeros((n_mels, F), dtype=np.float16)
    c = np.zeros((n_mels, F), dtype=np.float16)
    b[0, 1] = np.float16(300 / 1024)                                 # exactly G above the others
    b[0, 2] = np.float16(299 / 1024)                                 # G - 1
    c[0, 3] = np.float16(1.0)
    a[0, 4] = b[0, 4] = np.float16(0.5)                              # a tie of the loudest: channel 0
    a[:, 5] = np.float16(-1.0)                                       # the quietest value of channel 0 (and gated there)
    top, counts, out = CH.channel_top_ref([a, b, c], F, h, step)
    assert top.tolist() == [0, 1, 1, 2, 0, 1] and CH.run_lengths(top) == [[0, 1], [1, 2], [2, 1], [0, 1], [1, 1]]
    s = CH.smoothed([a, b, c], F, h)
    flags = CH.gated_frames(s, G)
    assert flags[0].tolist() == [False, True, False, True, False, True]
    assert flags[1].tolist() == [False, False, False, True, False, False]
    assert flags[2].tolist() == [False, True, False, False, True, False]
    assert counts == [3, 1, 2]
    assert (out[0][:, [1, 3, 5]] == np.float16(-1.0)).all() and out[0][0, 4] == np.float16(0.5)
    assert (out[1][:, 3] == 0).all() and out[1][0, 1] == b[0, 1]     # v_1 = 0, the other columns stay
    assert CH.gated_frames(s, G + 1)[0].tolist() == [False, False, False, True, False, True]


def test_quietest_orders_by_the_key_of_the_bits():
    x = np.array([[0.0, -0.0, 1.0, np.inf, -np.inf, np.nan]], dtype=np.float16)
    v, key = CH.quietest(x, 6)
    assert int(bits_of(v)) == -32768 and key == -1                   # -0 sorts below +0; the infinities and NaN take no part
    assert CH.quietest(x, 1)[1] == 0 and CH.quietest(x[:, 3:], 3) == (None, CH.NO_KEY)
    assert CH.fp16_key(np.array([-65504.0, -1.0, -0.0, 0.0, 2.0 ** -24, 65504.0], dtype=np.float16)).tolist() == sorted(
        CH.fp16_key(np.array([-65504.0, -1.0, -0.0, 0.0, 2.0 ** -24, 65504.0], dtype=np.float16)).tolist())
    # a channel without a finite element is never gated, however loud the other one is; and it counts as loudness 0
    dead = np.full((2, 4), np.nan, dtype=np.float16)
    loud = np.full((2, 4), 4.0, dtype=np.float16)
    top, counts, out = CH.channel_top_ref([dead, loud], 4, 1, 10)
    assert top.tolist() == [1] * 4 and counts == [0, 0] and same_bits(out, [dead, loud])
    quiet = np.full((2, 4), -4.0, dtype=np.float16)
    top, counts, out = CH.channel_top_ref([dead, quiet], 4, 1, 10)
    assert top.tolist() == [0] * 4 and counts == [0, 4]              # the dead channel's loudness is 0, far above the quiet one's
    # columns at or beyond F are not touched and do not lend their value
    m = np.zeros((1, 5), dtype=np.float16)
    m[0, 3:] = np.float16(-9.0)
    other = np.full((1, 5), 2.0, dtype=np.float16)
    _, counts, out = CH.channel_top_ref([m, other], 3, 0, 1)
    assert counts == [3, 0] and out[0][0].tolist() == [0, 0, 0, -9, -9]


def test_recordings_are_checked():
    m = np.zeros((2, 4), dtype=np.float16)
    for bad in ([], [m] * 9, [m, m[:, :3]], [m, m.astype(np.float32)]):
        with pytest.raises(ValueError):
            CH.channel_top_ref(bad, 2, 0, 0)
    with pytest.raises(ValueError):
        CH.channel_top_ref([m], 5, 0, 0)
    with pytest.raises(ValueError, match="step"):
        CH.channel_top_ref([m], 2, 0, SP.STEP_LIMIT + 1)
    with pytest.raises(ValueError, match="131072"):
        CH.channel_top_ref([m], 2, 40000, 0)


# --------------------------------------------------------------------------------------------------------------------- rule 5
def test_label_spans():
    fs = 0.25
    top = np.array([0, 0, 1, 1, 1, 2, 2, 0], dtype=np.uint8)
    assert CH.span_frames(0.0, 2.0, fs, 8) == (0, 8) and CH.span_frames(0.5, 0.5, fs, 8) == (2, 2)
    assert CH.span_frames(0.3, 0.3, fs, 8) == (1, 2)                 # an instant inside a frame is that frame
    assert CH.span_frames(-1.0, 9.0, fs, 8) == (0, 8) and CH.span_frames(3.0, 4.0, fs, 8) == (12, 8)
    assert CH.span_frames(3 * 0.1, 6 * 0.1, 0.1, 100) == (3, 6)      # 0.30000000000000004 / 0.1 is still frame 3
    assert CH.label_span(top, 0.0, 2.0, fs) == 0                     # 3, 3, 2: a tie of 0 and 1 goes to the lowest
    assert CH.label_span(top, 0.5, 1.75, fs) == 1 and CH.label_span(top, 1.25, 1.75, fs) == 2
    assert CH.label_span(top, 0.5, 0.5, fs) is None and CH.label_span(top, 5.0, 6.0, fs) is None
    assert CH.label_span(np.zeros(0, dtype=np.uint8), 0.0, 1.0, fs) is None
    segs = [dict(start=0.5, end=1.25, text="a", words=[dict(word="a", start=0.5, end=0.75), dict(word="b", start=1.25, end=1.75)]),
            dict(start=2.0, end=2.0, text="b")]
    before = copy.deepcopy(segs)
    out = CH.label_segments(segs, top, fs, 3)
    assert [s["channel"] for s in out] == [1, None] and [w["channel"] for w in out[0]["words"]] == [1, 2] and segs == before


# --------------------------------------------------------------------------------------------------------------------- rule 6
def seg(start, end, text, **kw):
    return dict(start=start, end=end, text=text, tokens=[1], **kw)


def test_merge_order_and_turns():
    ch0 = dict(language="en", text="x", segments=[seg(0.0, 1.0, " hello"), seg(1.0, 2.0, " there"), seg(5.0, 6.0, " bye")])
    ch1 = dict(language="de", text="y", segments=[seg(1.0, 2.0, " hallo"), seg(1.0, 1.5, " ja"), seg(2.0, 3.0, ""), seg(5.0, 6.0, " tschuess")])
    before = copy.deepcopy([ch0, ch1])
    out = CH.merge_channels([ch0, ch1])
    assert [(s["start"], s["end"], s["channel"]) for s in out["segments"]] == [
        (0.0, 1.0, 0), (1.0, 1.5, 1), (1.0, 2.0, 0), (1.0, 2.0, 1), (2.0, 3.0, 1), (5.0, 6.0, 0), (5.0, 6.0, 1)]
    assert out["turns"] == [dict(channel=0, start=0.0, end=1.0, text="hello"), dict(channel=1, start=1.0, end=1.5, text="ja"),
                            dict(channel=0, start=1.0, end=2.0, text="there"), dict(channel=1, start=1.0, end=3.0, text="hallo"),
                            dict(channel=0, start=5.0, end=6.0, text="bye"), dict(channel=1, start=5.0, end=6.0, text="tschuess")]
    assert out["text"] == "[0] hello\n[1] ja\n[0] there\n[1] hallo\n[0] bye\n[1] tschuess"
    assert out["language"] == "en" and out["channels"] == before and [ch0, ch1] == before
    assert all("channel" not in s for r in out["channels"] for s in r["segments"])
    empty = dict(language="fr", text="", segments=[])
    assert CH.merge_channels([empty, ch1])["language"] == "de"
    none = CH.merge_channels([empty])
    assert none["language"] is None and none["segments"] == [] and none["turns"] == [] and none["text"] == ""


# ------------------------------------------------------------------------------------------------------- options, refusals
def test_options_and_their_refusals():
    assert ChannelOptions() == ChannelOptions(mode="split", bleed_db=None, smooth_seconds=0.2)
    assert ChannelOptions().frames(3000, 80) == (SP.SpeechOptions().frames(3000, 80)[0], 0) == (10, 0)
    assert ChannelOptions(bleed_db=12.0).frames(3000, 80) == (10, 307)
    assert ChannelOptions(smooth_seconds=0.0, bleed_db=40.0 * SP.STEP_LIMIT / 1024).frames(128, 80) == (0, SP.STEP_LIMIT)
    assert ChannelOptions(mode="label").check().mode == "label"
    for bad in (ChannelOptions(mode="both"), ChannelOptions(mode="label", bleed_db=6.0), ChannelOptions(bleed_db=float("nan")),
                ChannelOptions(bleed_db=float("inf")), ChannelOptions(bleed_db=0.0), ChannelOptions(bleed_db=-3.0),
                ChannelOptions(bleed_db=0.01), ChannelOptions(bleed_db=1281.0), ChannelOptions(bleed_db="6"),
                ChannelOptions(smooth_seconds=-1.0)):
        with pytest.raises(ValueError, match="channels"):
            bad.check()
        with pytest.raises(ValueError):
            bad.frames(3000, 80)
    with pytest.raises(ValueError, match="131072"):
        ChannelOptions(smooth_seconds=60.0).frames(3000, 80)


def test_transcribe_refuses_before_any_decoding():
    """No engine is handed over: a refusal that came after the first use of one would be an AttributeError."""
    mono = np.zeros(1600, dtype=np.float32)
    with pytest.raises(ValueError, match="mono waveform"):
        T.transcribe(None, None, [mono], channels=ChannelOptions())
    with pytest.raises(ValueError, match="mode"):
        T.transcribe(None, None, ["a.wav"], channels=ChannelOptions(mode="both"))
    with pytest.raises(ValueError, match="bleed_db"):
        T.transcribe(None, None, ["a.wav"], channels=ChannelOptions(mode="label", bleed_db=6.0))
    with pytest.raises(ValueError, match="bleed_db"):
        T.transcribe(None, None, ["a.wav"], channels=ChannelOptions(bleed_db=float("nan")))
    with pytest.raises(ValueError, match="channel_counts"):
        T.transcribe_mel(None, None, [], [], channels=ChannelOptions())
    with pytest.raises(ValueError, match="channel_counts"):
        T.transcribe_mel(None, None, [], [], channel_counts=[2])
    with pytest.raises(ValueError, match="label"):
        T.transcribe_mel(None, None, [], [], channels=ChannelOptions(mode="label"), channel_counts=[2])
    with pytest.raises(ValueError, match="mode"):
        T.transcribe_mel(None, None, [], [], channels=ChannelOptions(mode="x"), channel_counts=[2])
    with pytest.raises(ValueError, match="channel_counts"):
        T._transcribe_channels(None, None, [None] * 3, [1, 1, 1], [2], ChannelOptions(), None, None)
    with pytest.raises(ValueError):
        wu.load_audio_device("a.wav", channels="label")


def test_cli_flags():
    base = ["--input_file", "a.wav"]
    args = T.parse_arguments(base)
    assert args.channels is None and args.bleed_db is None and T.channel_options_from_args(args) is None
    assert T.channel_options_from_args(T.parse_arguments(base + ["--channels", "split"])) == ChannelOptions()
    assert T.channel_options_from_args(T.parse_arguments(base + ["--channels", "label"])) == ChannelOptions(mode="label")
    assert T.channel_options_from_args(T.parse_arguments(base + ["--channels", "split", "--bleed_db", "12"])) == ChannelOptions(bleed_db=12.0)
    for bad in (["--channels", "stereo"], ["--bleed_db", "6"], ["--channels", "label", "--bleed_db", "6"],
                ["--channels", "split", "--bleed_db", "0"], ["--channels", "split", "--bleed_db", "nan"]):
        with pytest.raises(ValueError):
            T.channel_options_from_args(T.parse_arguments(base + bad))


def test_header_exports_and_abi():
    header = open(os.path.join(ROOT, "include", "whisper_mi355.h")).read()
    assert "int wm_channel_top(" in header and "size_t wm_channel_top_workspace_bytes(" in header and "int wm_resample_channels(" in header
    assert re.search(r"#define WM_ABI_VERSION 8\b", header) and native.ABI_VERSION == 8
    assert all(n in native.EXPORTS for n in ("wm_channel_top", "wm_channel_top_workspace_bytes", "wm_resample_channels"))
    csrc = os.path.join(ROOT, "eddie-wang-hackathon2023_amd", "csrc")
    assert "channels.hip" in open(os.path.join(csrc, "Makefile")).read()
    text = open(os.path.join(csrc, "channels.hip")).read()
    assert '#include "loudness.h"' in text and "rintf" not in text and "sc_launch_smoothed" in text      # one definition of the loudness


# --------------------------------------------------------------------------------------------------------------------- rule 1
@pytest.mark.parametrize("rate", [8000, 22050, 44100])
def test_channel_waveforms_are_the_mono_path_of_the_single_column(rate):
    rng = rng_of(rate)
    pcm = rng.integers(-2 ** 15, 2 ** 15, size=(700, 3)).astype(np.int32)
    for c in range(3):
        got = CH.channel_waveform_ref(pcm, c, 16, rate)
        want = wu.resample_reference(pcm[:, c].astype(np.float32) * np.float32(2.0 ** -15), rate)
        assert got.dtype == np.float64 and np.array_equal(got, want)
        assert np.array_equal(got, wu.resample_reference(wu.downmix(pcm[:, c], 16), rate))               # a mono file holding it
    flt = rng.standard_normal((300, 2)).astype(np.float32)
    assert np.array_equal(CH.channel_waveform_ref(flt, 1, None, rate), wu.resample_reference(flt[:, 1], rate))


def test_channel_waveforms_at_16_khz_are_mono_at_sr_of_the_column():
    rng = rng_of(16)
    pcm = rng.integers(-2 ** 15, 2 ** 15, size=(500, 4)).astype(np.int32)
    rows = wu.channels_at_sr(pcm, 16)
    assert rows.dtype == np.float32 and rows.shape == (4, 500)
    for c in range(4):
        assert np.array_equal(rows[c], wu._mono_at_sr(pcm[:, c:c + 1], 16)) and np.array_equal(rows[c], CH.channel_waveform_ref(pcm, c, 16, 16000))
        assert np.array_equal(rows[c], pcm[:, c].astype(np.float32) / 32768.0)
    assert np.array_equal(wu.channels_at_sr(pcm[:, :1], 16)[0], wu._mono_at_sr(pcm[:, :1], 16))          # a mono file is its own channel 0
