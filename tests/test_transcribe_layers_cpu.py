"""The layers of transcribe.py -- channels, speech, sections over files -- on the CPU: what each of the eight on/off combinations hands
the decoder's side and how it puts the results back together.

No GPU and no engine: the five device wrappers are replaced by the numpy contracts they are held to on the GPU (sections.py,
speech.py, channels.py), `_transcribe_files` by a stub that records what it is handed and returns two known segments per "file".
Everything that is expected is built here from those contracts, layer by layer, and a few figures are written out.
"""
import types

import numpy as np
import pytest
import torch

import channels as CH
import longform as LF
import sections as S
import speech as SP
import transcribe as T
from channels import ChannelOptions

N_MELS, W = 8, 20
FS = LF.CHUNK_LENGTH / W
CONTENTS = [57, 57, 0, 131]                  # as channels: a recording of two, then two of one; the third is empty
COUNTS = [2, 1, 1]
LOUD = [[(5, 25)], [(30, 50)], [], [(10, 40), (60, 75), (100, 131)]]
SECTIONS = S.SectionOptions(max_seconds=30.0)
SPEECH = SP.SpeechOptions(smooth_seconds=0.0, min_silence_seconds=4.5, min_speech_seconds=1.5, speech_pad_seconds=1.5)
CHANNELS = ChannelOptions(bleed_db=6.0, smooth_seconds=0.0)
KW = dict(temperatures=(0.0,), compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None)
KEYS = {"temperatures", "compression_ratio_threshold", "logprob_threshold", "no_speech_threshold", "n_rows", "trace",
        "condition_on_previous_text", "initial_prompt", "word_timestamps"}


def make_mels():
    rng = np.random.default_rng(11)
    out = []
    for c, loud in zip(CONTENTS, LOUD):
        m = (rng.standard_normal((N_MELS, c + W)) * 0.05 - 2.0).astype(np.float16)
        for a, b in loud:
            m[:, a:b] = (rng.standard_normal((N_MELS, b - a)) * 0.3 + 1.0).astype(np.float16)
        out.append(torch.from_numpy(m))
    return out


class FakeTokenizer:
    @staticmethod
    def decode(tokens):
        return "".join(f" t{int(t)}" for t in tokens)


def fake_decoding():
    options = types.SimpleNamespace(prompt=None, prefix=None, temperature=0.0, language=None)
    return types.SimpleNamespace(decoder_config=dict(num_audio_ctx=W // 2), tokenizer=FakeTokenizer(), options=options,
                                 is_multilingual=False, beam=False, n_group=1)


def stub_segments(i, c):
    """Two segments for "file" i of c frames (none for an empty one): [0, c // 2) and [c // 2, c), a word in each."""
    if c == 0:
        return []
    h = c // 2
    return [dict(seek=0, start=0.0, end=h * FS, text=f" t{1000 + i}", tokens=[1000 + i],
                 words=[dict(word=f" a{i}", start=0.0, end=h * FS, probability=0.5)]),
            dict(seek=h, start=h * FS, end=c * FS, text=f" t{2000 + i}", tokens=[2000 + i],
                 words=[dict(word=f" b{i}", start=(h + c) / 2 * FS, end=c * FS, probability=0.25)])]


def stub_results(contents):
    out = []
    for i, c in enumerate(contents):
        segments = stub_segments(i, c)
        out.append(dict(language="en", text=FakeTokenizer.decode([t for s in segments for t in s["tokens"]]).strip(), segments=segments))
    return out


@pytest.fixture
def layers(monkeypatch):
    """transcribe.py with the device wrappers on the numpy contracts and `_transcribe_files` recording: (calls, wrapper calls)."""
    calls, used = [], []

    def section_cuts(mels, content_frames, options, window=3000):
        used.append("section_cuts")
        lo, hi, h = options.frames(window, N_MELS)
        return [S.section_cuts_ref(m.numpy(), int(c), lo, hi, h) for m, c in zip(mels, content_frames)]

    def speech_spans(mels, content_frames, options, window=3000):
        used.append("speech_spans")
        cfg = options.frames(window, N_MELS)
        return [SP.speech_spans_ref(m.numpy(), int(c), *cfg) for m, c in zip(mels, content_frames)]

    def packed_mels(mels, content_frames, spans, window):
        used.append("packed_mels")
        out = [torch.from_numpy(SP.packed_mel_ref(m.numpy(), int(c), sp, window)) for m, c, sp in zip(mels, content_frames, spans)]
        return out, [sum(b - a for a, b in sp) for sp in spans]

    def section_mels(mels, content_frames, cuts, window):
        used.append("section_mels")
        out, content, owner, starts = [], [], [], []
        for f, (m, c) in enumerate(zip(mels, content_frames)):
            for a, b in S.section_bounds(int(c), cuts[f]):
                out.append(torch.from_numpy(S.section_mel_ref(m.numpy(), int(c), a, b, window)))
                content.append(b - a), owner.append(f), starts.append(a)
        return out, content, owner, starts

    def channel_top(mels, content_frames, channel_counts, options, window=3000):
        used.append("channel_top")
        h, step = options.frames(window, N_MELS)
        tops, gated, at = [], [], 0
        for C in channel_counts:
            top, counts, after = CH.channel_top_ref([m.numpy() for m in mels[at: at + C]], int(content_frames[at]), h, step)
            for m, g in zip(mels[at: at + C], after):
                m.copy_(torch.from_numpy(g))                                     # the gate writes in place
            tops.append(top), gated.extend(counts)
            at += C
        return tops, gated

    def transcribe_files(encoding, decoding, mels, content_frames, owner, **kw):
        mels = list(mels)
        assert all(m.dtype == torch.float16 and m.is_contiguous() for m in mels)
        calls.append(dict(mels=[m.numpy().copy() for m in mels], content=[int(c) for c in content_frames],
                          owner=None if owner is None else list(owner), kw=kw))
        return stub_results(calls[-1]["content"])

    for name, fn in (("section_cuts", section_cuts), ("speech_spans", speech_spans), ("packed_mels", packed_mels),
                     ("section_mels", section_mels), ("channel_top", channel_top), ("_transcribe_files", transcribe_files)):
        monkeypatch.setattr(T, name, fn)
    return calls, used


def expected(channels, speech, sections):
    """(what reaches the files' layer: mels, content, owner; the results) from the contracts, one layer after the other."""
    mels, content = [m.numpy().copy() for m in make_mels()], list(CONTENTS)
    tops, gated = [], []
    if channels:
        h, step = CHANNELS.frames(W, N_MELS)
        at = 0
        for C in COUNTS:
            top, counts, after = CH.channel_top_ref(mels[at: at + C], content[at], h, step)
            mels[at: at + C] = after
            tops.append(top), gated.extend(counts)
            at += C
    spans = None
    if speech:
        cfg = SPEECH.frames(W, N_MELS)
        spans = [SP.speech_spans_ref(m, c, *cfg) for m, c in zip(mels, content)]
        mels = [SP.packed_mel_ref(m, c, sp, W) for m, c, sp in zip(mels, content, spans)]
        content = [sum(b - a for a, b in sp) for sp in spans]
    owner = starts = None
    n_files = len(mels)
    if sections:
        lo, hi, h = SECTIONS.frames(W, N_MELS)
        pieces, piece_content, owner, starts = [], [], [], []
        for f, (m, c) in enumerate(zip(mels, content)):
            for a, b in S.section_bounds(c, S.section_cuts_ref(m, c, lo, hi, h)):
                pieces.append(S.section_mel_ref(m, c, a, b, W))
                piece_content.append(b - a), owner.append(f), starts.append(a)
        mels, content = pieces, piece_content
    results = stub_results(content)
    if sections:
        merged = []
        for f in range(n_files):
            mine = [i for i, o in enumerate(owner) if o == f]
            segments = S.merge_sections([results[i]["segments"] for i in mine], [starts[i] for i in mine], FS)
            merged.append(dict(language="en", text=FakeTokenizer.decode([t for s in segments for t in s["tokens"]]).strip(),
                               segments=segments, sections=[(starts[i] * FS, (starts[i] + content[i]) * FS) for i in mine]))
        results = merged
    if speech:
        for r, sp in zip(results, spans):
            r["segments"] = SP.restore(r["segments"], sp, FS)
            r["speech"] = [(a * FS, b * FS) for a, b in sp]
            if "sections" in r:
                r["sections"] = [(SP.restore_time(a, sp, FS), SP.restore_time(b, sp, FS, end=True)) for a, b in r["sections"]]
    if channels:
        recordings, at = [], 0
        for r, C in enumerate(COUNTS):
            res = CH.merge_channels(results[at: at + C])
            res["channel_top"] = CH.run_lengths(tops[r])
            res["channel_gated"] = gated[at: at + C]
            recordings.append(res)
            at += C
        results = recordings
    return (mels, content, owner), results


COMBINATIONS = [(c, sp, se) for c in (False, True) for sp in (False, True) for se in (False, True)]
# the content frames of the inner "files" and their owners, as the code gave them when this test was written (the cuts fall where the
# seeded noise is quietest, so they are recorded, not derived)
INNER = {
    (False, False, False): ([57, 57, 0, 131], None),
    (False, False, True): ([17, 11, 10, 19, 14, 15, 11, 17, 18, 12, 12, 11, 10, 12, 11, 11, 12, 14, 8], [0] * 4 + [1] * 4 + [3] * 11),
    (False, True, False): ([22, 22, 0, 81], None),
    (False, True, True): ([20, 2, 11, 11, 17, 14, 18, 10, 14, 8], [0, 0, 1, 1, 3, 3, 3, 3, 3, 3]),
    (True, False, False): ([57, 57, 0, 131], None),
    (True, False, True): ([17, 20, 20, 20, 15, 16, 6, 18, 12, 12, 11, 10, 12, 11, 11, 12, 14, 8], [0] * 3 + [1] * 4 + [3] * 11),
    (True, True, False): ([22, 22, 0, 81], None),
    (True, True, True): ([20, 2, 11, 11, 17, 14, 18, 10, 14, 8], [0, 0, 1, 1, 3, 3, 3, 3, 3, 3]),
}


@pytest.mark.parametrize("channels,speech,sections", COMBINATIONS)
def test_what_reaches_the_files_and_what_comes_back(layers, channels, speech, sections):
    calls, used = layers
    mels = make_mels()
    before = [m.clone() for m in mels]
    trace = []
    got = T.transcribe_mel(None, fake_decoding(), mels, CONTENTS, n_rows=3, trace=trace, speech=SPEECH if speech else None,
                           sections=SECTIONS if sections else None,
                           **(dict(channels=CHANNELS, channel_counts=COUNTS) if channels else {}), **KW)
    (want_mels, want_content, want_owner), want = expected(channels, speech, sections)

    # ---- what reached the files' layer: once, these mels bit for bit, these contents, this owner list, the caller's options
    assert len(calls) == 1
    call = calls[0]
    assert call["content"] == want_content and call["owner"] == want_owner
    assert len(call["mels"]) == len(want_mels)
    for a, b in zip(call["mels"], want_mels):
        assert a.shape == b.shape == (N_MELS, a.shape[1]) and np.array_equal(a.view(np.int16), b.view(np.int16))
    assert all(m.shape[1] == c + W for m, c in zip(call["mels"], call["content"]))
    assert set(call["kw"]) == KEYS and call["kw"]["trace"] is trace and call["kw"]["n_rows"] == 3
    assert call["kw"]["temperatures"] == (0.0,) and call["kw"]["word_timestamps"] is False
    assert (call["owner"] is not None) == sections
    assert used == (["channel_top"] if channels else []) + (["speech_spans", "packed_mels"] if speech else []) \
        + (["section_cuts", "section_mels"] if sections else [])
    assert all(torch.equal(a, b) for a, b in zip(mels, before)), "the gate wrote into the caller's mels"

    # ---- what came back: the complete dicts, their keys, the order of the merge
    assert got == want
    assert len(got) == (len(COUNTS) if channels else len(CONTENTS))
    keys = {"language", "text", "segments"} | ({"sections"} if sections and not channels else set()) \
        | ({"speech"} if speech and not channels else set()) | ({"channels", "turns", "channel_top", "channel_gated"} if channels else set())
    assert all(set(r) == keys for r in got)
    parts = [p for r in got for p in r["channels"]] if channels else got
    assert all(("sections" in p) == sections and ("speech" in p) == speech for p in parts)
    for r in got:
        order = [(s["start"], s["end"], s["channel"]) if channels else s["start"] for s in r["segments"]]
        assert order == sorted(order)
    if channels:
        assert sum(sum(r["channel_gated"]) for r in got) > 0 and [len(r["channels"]) for r in got] == COUNTS
        assert [sum(n for _, n in r["channel_top"]) for r in got] == [57, 0, 131]
    assert (call["content"], call["owner"]) == INNER[(channels, speech, sections)]


def test_figures_written_out(layers):
    """A few of the values above by hand, so that the expectation does not rest on the contracts' composition alone."""
    calls, _ = layers
    got = T.transcribe_mel(None, fake_decoding(), make_mels(), CONTENTS, speech=SPEECH, sections=SECTIONS, **KW)
    assert SPEECH.frames(W, N_MELS) == (0, 205, 100, 3, 1, 1) and SECTIONS.frames(W, N_MELS) == (10, 20, 0) and FS == 1.5
    # rule 4 of speech.py pads the planted stretches by one frame; a stretch that ends the file ends there
    assert [r["speech"] for r in got] == [[(4 * FS, 26 * FS)], [(29 * FS, 51 * FS)], [], [(9 * FS, 41 * FS), (59 * FS, 76 * FS), (99 * FS, 131 * FS)]]
    assert calls[0]["owner"] == [0, 0, 1, 1, 3, 3, 3, 3, 3, 3] and sum(calls[0]["content"]) == 22 + 22 + 0 + 81
    assert got[2] == dict(language="en", text="", segments=[], sections=[], speech=[])
    # file 0: 22 packed frames in two sections; the first section's first stub segment starts where the speech starts
    first = got[0]["segments"][0]
    assert first["start"] == 4 * FS and first["seek"] == 4 and first["words"][0]["start"] == 4 * FS
    assert got[0]["sections"][0][0] == 4 * FS and got[0]["sections"][-1][1] == 26 * FS
    assert got[0]["text"] == " ".join(f"t{k + i}" for i in (0, 1) for k in (1000, 2000))
