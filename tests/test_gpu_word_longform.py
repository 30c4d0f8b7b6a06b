"""Word timestamps in long-form transcription on the GPU: transcribe_mel(word_timestamps=True) end to end, and
WhisperDecoding.word_timestamps(token_probs="device") against token_probs="torch".

micro-fullvocab engine, W = 128 frames, sample_len 12, as tests/test_gpu_longform.py.  Near-ties in random-weight logits make a
row's arithmetic depend on the batch composition, so nothing is compared across batch shapes:
  1. the trace (decoder results AND the raw alignments of every alignment call) is replayed per file through
     longform.transcribe_reference -- the returned segments, words, moved starts / ends and seeks included, must come out;
  2. every alignment call is made again through the public path -- get_audio_features(the round's windows) -> word_timestamps with
     the same rows, tokens and frames, the same batch shape -- and must return the recorded alignments exactly;
  3. one buffer set, no graph captured after round 1, one encoder pass per round (the counts of tests/test_gpu_longform.py);
  4. every word lies inside or behind its window, seek * fs <= start <= end, and every segment has "words".
With random weights most windows advance by the end of their last word, which can be as little as 2 frames: the files are short
(0, 1, W - 1, W + 1, 2 W + 17 frames) so that the worst case stays at a few seconds.

Measured on MI355X (printed by the tests): token_probs "device" against "torch": max |diff| 1.4e-09 over 24 tokens (largest
probability 5e-3; bound 2^-21 = 4.8e-07).  End to end, 3 rows: language named, no thresholds: 11 windows in 5 rounds, 5 decoder and 5
alignment calls, 22 words, 6 windows advanced by the end of their last word; fallback and detected language: 12 windows in 8
rounds, 16 decoder and 8 alignment calls, 21 words, 7 windows advanced by a word; row_prompts with conditioning: 7 windows in 4
rounds, 7 words.  CLI on the golden FLAC: 11 segments, 26 words in 4 windows.  Every test takes under a second.
"""
import os
import re
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import longform as LF  # noqa: E402
import native  # noqa: E402
import synthetic  # noqa: E402
import transcribe as T  # noqa: E402
from decoding import DecodingOptions, WhisperDecoding  # noqa: E402
from encoding import WhisperEncoding  # noqa: E402
from oracle.whisper_oracle import Dims, synthetic_mel  # noqa: E402
from test_gpu_model import build_engine  # noqa: E402

W = 128
CONTENTS = [0, 1, W - 1, W + 1, 2 * W + 17]
SEGMENT_KEYS = {"seek", "start", "end", "text", "tokens", "temperature", "avg_logprob", "compression_ratio", "no_speech_prob", "words"}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return native.load_library()


@pytest.fixture(scope="module")
def tmpdir_module(tmp_path_factory):
    return str(tmp_path_factory.mktemp("engines"))


@pytest.fixture(scope="module")
def engines(tmpdir_module):
    dims = Dims(**synthetic.DIMS["micro-fullvocab"])
    assert 2 * dims.n_audio_ctx == W
    eng = build_engine(tmpdir_module, "micro-fullvocab", 3)
    mels = [synthetic_mel(1, c + W, dims.n_mels, 900 + i)[0].cuda().contiguous() for i, c in enumerate(CONTENTS)]
    return dims, eng, WhisperEncoding(eng), mels


def sampled_rows(jobs, languages):
    return [types.SimpleNamespace(tokens=[] if j is None else list(j[1]), language=lang) for j, lang in zip(jobs, languages)]


# ------------------------------------------------------------------------------------------------------------- token_probs
def test_token_probs_device_equals_torch(lib, engines):
    """One batch of two clips: the same words, tokens, paths and times; the probabilities agree to 2^-21.  Why 2^-21:
    tests/test_gpu_forced_probs.py holds the kernel to max(4 e, 2^-22) of the fp64 value, e being the PyTorch expression's own
    error; the PyTorch expression is within e of it.  With random weights a token's probability is of the order of 1 / V, where
    e is far below one fp32 ulp of 1 (the kernel test measures 5e-9 and less on such rows), so each side is within 2^-22."""
    dims, eng, enc, _ = engines
    dec = WhisperDecoding(eng)
    dec.sample_len = 12
    xa = enc.get_audio_features(synthetic_mel(2, W, dims.n_mels, 77).cuda())
    languages, _ = dec.detect_language(xa)
    results = dec.post_process(*dec.main_loop(xa), xa, languages)
    frames = [W, 2 * 45 + 1]
    words_t = dec.word_timestamps(xa, results, frames)
    torch_side = dec.last_alignment
    words_d = dec.word_timestamps(xa, results, frames, token_probs="device")
    dev_side = dec.last_alignment
    assert any(words_t) and [[(w.word, w.tokens, w.start, w.end) for w in ws] for ws in words_d] == \
        [[(w.word, w.tokens, w.start, w.end) for w in ws] for ws in words_t]
    assert np.array_equal(dev_side["path_text"], torch_side["path_text"]) and np.array_equal(dev_side["path_time"], torch_side["path_time"])
    assert dev_side["path_len"] == torch_side["path_len"]
    worst = float((dev_side["token_probs"] - torch_side["token_probs"]).abs().max())
    worst_w = max(abs(a.probability - b.probability) for x, y in zip(words_d, words_t) for a, b in zip(x, y))
    print(f"token_probs device vs torch: max |diff| = {worst:.3g} over {dev_side['token_probs'].numel()} tokens "
          f"(largest probability {float(torch_side['token_probs'].max()):.3g}), per word {worst_w:.3g}; bound {2.0 ** -21:.3g}")
    assert torch.isfinite(dev_side["token_probs"]).all() and worst <= 2.0 ** -21 and worst_w <= 2.0 ** -21
    assert dec.word_timestamps(xa, results, frames, token_probs="device") == words_d
    with pytest.raises(ValueError, match="token_probs"):
        dec.word_timestamps(xa, results, frames, token_probs="host")


# --------------------------------------------------------------------------------------------------------------- end to end
def run_words(enc, dec, mels, n_rows, **kw):
    tk = dec.tokenizer
    fs = LF.CHUNK_LENGTH / W
    trace, states, encoder_runs = [], [], []
    real_main_loop, real_features = dec.main_loop, enc.get_audio_features

    def main_loop(*a, **k):
        out = real_main_loop(*a, **k)
        states.append(list(dec._state.values()))
        return out

    def get_audio_features(mel):
        encoder_runs.append(tuple(mel.shape))
        return real_features(mel)

    dec.main_loop, enc.get_audio_features = main_loop, get_audio_features
    try:
        results = T.transcribe_mel(enc, dec, mels, CONTENTS, n_rows=n_rows, trace=trace, word_timestamps=True, **kw)
    finally:
        dec.main_loop, enc.get_audio_features = real_main_loop, real_features
    decodes = [e for e in trace if e.get("kind") != "align"]
    aligns = [e for e in trace if e.get("kind") == "align"]
    assert len(results) == len(CONTENTS) and results[0]["segments"] == []
    n_rounds = decodes[-1]["round"] + 1

    # 3. one buffer set, no graph captured after round 1, one encoder pass per round; at most one alignment call per round, after
    #    the round's last decoder call
    assert all(len(s) == 1 and s[0] is states[0][0] for s in states) and len(states) == len(decodes)
    assert all(e["n_states"] == 1 for e in decodes)
    assert [e for e in decodes if e["round"] == 0][-1]["n_graphs"] == decodes[-1]["n_graphs"] > 0
    assert encoder_runs == [(n_rows, mels[0].shape[0], W)] * n_rounds
    assert len({e["round"] for e in aligns}) == len(aligns)
    for k, e in enumerate(trace):
        if e.get("kind") == "align":
            assert set(e) == {"kind", "round", "rows", "jobs", "languages", "alignments"}
            assert trace[k - 1].get("kind") != "align" and trace[k - 1]["round"] == e["round"] and trace[k - 1]["rows"] == e["rows"]
            assert k + 1 == len(trace) or trace[k + 1]["new_round"]
            assert len(e["jobs"]) == n_rows == len(e["alignments"]) and any(j is not None for j in e["jobs"])

    # 1. the literal loop per file, from the recorded results and the recorded raw alignments
    recorded, prompts, aligned = {}, {}, {}
    for e in decodes:
        for i, (r, on, res) in enumerate(zip(e["rows"], e["live"], e["results"])):
            if on:
                assert (r[0], r[1], e["temperature"]) not in recorded
                recorded[(r[0], r[1], e["temperature"])] = res
                prompts[(r[0], r[1])] = None if e["prompts"] is None else e["prompts"][i]
    for e in aligns:
        for r, j, a in zip(e["rows"], e["jobs"], e["alignments"]):
            if j is not None:
                assert r not in aligned
                aligned[r] = (j, a)
    ladder = dict(temperatures=kw.get("temperatures", LF.TEMPERATURES), compression_ratio_threshold=kw.get("compression_ratio_threshold", 2.4),
                  logprob_threshold=kw.get("logprob_threshold", -1.0), no_speech_threshold=kw.get("no_speech_threshold", 0.6))
    prompted = {k: kw[k] for k in ("condition_on_previous_text", "initial_prompt") if k in kw}
    used, used_alignments = set(), set()
    for f, c in enumerate(CONTENTS):
        def decode_one(seek, temperature, prompt=None, f=f):
            used.add((f, seek, temperature))
            assert prompt is None or prompt == prompts[(f, seek)]
            return recorded[(f, seek, temperature)]

        def align_one(seek, size, segments, f=f):
            used_alignments.add((f, seek))
            job, alignment = aligned[(f, seek)]
            assert job[0] == size and list(job[1]) == LF.text_tokens(segments, tk.eot)
            return alignment
        want = LF.transcribe_reference(decode_one, c, window=W, timestamp_begin=tk.timestamp_begin, decode_text=tk.decode,
                                       align_one=align_one, eot=tk.eot, **ladder, **prompted)
        assert results[f]["segments"] == want, f
    assert used == set(recorded) and used_alignments == set(aligned)

    # 4. every segment has words; every word lies at or behind its window's start and starts before it ends
    n_words = 0
    for res in results:
        for s in res["segments"]:
            assert set(s) == SEGMENT_KEYS
            assert all(s["seek"] * fs - 0.005 <= w["start"] <= w["end"] and set(w) == {"word", "start", "end", "probability"} for w in s["words"])
            n_words += len(s["words"])
    assert n_words > 0

    # how the windows moved on
    windows = sorted({(r[0], r[1]) for e in decodes for r, on in zip(e["rows"], e["live"]) if on})
    by_word = 0
    for f, seek in windows:
        segs = [s for s in results[f]["segments"] if s["seek"] == seek]
        end = next((s["words"][-1]["end"] for s in reversed(segs) if s["words"]), None)
        final = max((t for (ff, sk, t) in recorded if (ff, sk) == (f, seek)))
        single = LF._timestamp_pairs(recorded[(f, seek, final)].tokens, tk.timestamp_begin)[0]
        by_word += end is not None and not single and end > seek * fs
    print(f"words end to end (n_rows {n_rows}): {len(windows)} windows in {n_rounds} rounds, {len(decodes)} decoder calls, "
          f"{len(aligns)} alignment calls, {n_words} words; {by_word} windows advanced by the end of their last word")
    return results, trace, decodes, aligns


def replay_alignments(enc, dec, decodes, aligns):
    """2. every alignment call again, through the public path, with the same batch shape."""
    first = {e["round"]: e for e in decodes if e["new_round"]}
    for e in aligns:
        xa = enc.get_audio_features(first[e["round"]]["windows"].cuda())
        frames = [0 if j is None else j[0] for j in e["jobs"]]
        again = dec.word_timestamps(xa, sampled_rows(e["jobs"], e["languages"]), frames, token_probs="device")
        assert again == e["alignments"], e["round"]
        assert all(a == [] for a, j in zip(again, e["jobs"]) if j is None)


def test_transcribe_words_language_named_no_thresholds(lib, engines):
    dims, eng, enc, mels = engines
    dec = WhisperDecoding(eng, options=DecodingOptions(language="en"))
    dec.sample_len = 12
    results, trace, decodes, aligns = run_words(enc, dec, mels, 3, compression_ratio_threshold=None, logprob_threshold=None,
                                                no_speech_threshold=None)
    assert all(r["language"] == "en" for r in results) and all(e["temperature"] == 0.0 for e in decodes)
    replay_alignments(enc, dec, decodes, aligns)
    assert len(dec._state) == 1


def test_transcribe_words_fallback_and_detected_language(lib, engines):
    dims, eng, enc, mels = engines
    dec = WhisperDecoding(eng)
    dec.sample_len = 12
    results, trace, decodes, aligns = run_words(enc, dec, mels, 3, temperatures=(0.0, 0.4), compression_ratio_threshold=None,
                                                logprob_threshold=-1.0, no_speech_threshold=None)
    assert {e["temperature"] for e in decodes} == {0.0, 0.4}
    assert all(s["temperature"] == 0.4 for r in results for s in r["segments"])
    # the alignment of a round follows its LAST decoder call (the ladder has settled)
    for e in aligns:
        assert [d["temperature"] for d in decodes if d["round"] == e["round"]] == [0.0, 0.4]
    replay_alignments(enc, dec, decodes, aligns)


def test_transcribe_words_on_a_row_prompts_instance(lib, engines):
    """condition_on_previous_text on an instance with right-aligned rows: the left-aligned tap pass runs on it, twice gives two
    replayable runs, and a word pass between two main_loop calls on the same features changes nothing."""
    dims, eng, enc, mels = engines
    dec = WhisperDecoding(eng, row_prompts=True, options=DecodingOptions(language="en"))
    dec.sample_len = 6
    kw = dict(temperatures=(0.0,), compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None,
              condition_on_previous_text=True, initial_prompt=[1500, 1501])
    for _ in range(2):
        results, trace, decodes, aligns = run_words(enc, dec, mels, 3, **kw)
    assert any(len(p) > 2 for e in decodes for p in e["prompts"]), "no window was conditioned on previous text"
    e = aligns[-1]
    d = [x for x in decodes if x["round"] == e["round"]][-1]
    xa = enc.get_audio_features([x for x in decodes if x["round"] == e["round"]][0]["windows"].cuda())
    if d["language_tokens"] is not None:
        dec.set_language_tokens(d["language_tokens"])
    dec.set_prompts(d["prompts"])
    t1, lp1, nsp1 = dec.main_loop(xa, row_limit=d["row_limit"], temperature=0.0)
    dec.word_timestamps(xa, sampled_rows(e["jobs"], e["languages"]), [0 if j is None else j[0] for j in e["jobs"]], token_probs="device")
    t2, lp2, _ = dec.main_loop(xa, row_limit=d["row_limit"], temperature=0.0)
    assert torch.equal(t1, t2) and torch.equal(lp1, lp2)
    again = dec.post_process(t1, lp1, nsp1, xa, d["languages"], temperature=0.0)
    assert all(again[i].tokens == d["results"][i].tokens for i, on in enumerate(d["live"]) if on)


def test_transcribe_words_refusals(lib, engines, tmpdir_module):
    dims, eng, enc, mels = engines
    calls = []
    real = enc.get_audio_features
    enc.get_audio_features = lambda mel: calls.append(1) or real(mel)
    try:
        with pytest.raises(ValueError, match="word_timestamps"):
            T.transcribe_mel(enc, WhisperDecoding(eng, options=DecodingOptions(beam_size=2)), mels, CONTENTS, temperatures=(0.0,),
                             word_timestamps=True)
        eng8 = build_engine(tmpdir_module, "micro-fullvocab", 3, cross_scales=[0.05] * dims.n_text_layer)
        dec8 = WhisperDecoding(eng8)
        assert dec8.use_int8_cross_kv
        with pytest.raises(native.WmError, match="int8"):
            T.transcribe_mel(enc, dec8, mels, CONTENTS, word_timestamps=True)
    finally:
        enc.get_audio_features = real
    assert calls == [], "refused only after decoding had begun"


def test_transcribe_cli_prints_words(lib, engines, golden_dir, capsys):
    dims, eng, enc, mels = engines
    flac = os.path.join(golden_dir, "librispeech_1089-134691-0000.flac")
    results = T.main(T.parse_arguments(["--engine_dir", str(eng), "--input_file", flac, "--no_fallback", "--language", "en",
                                        "--word_timestamps"]))
    out = capsys.readouterr().out
    segments = [s for s in results[0]["segments"] if s["text"].strip()]
    n_words = sum(len(s["words"]) for s in segments)
    assert segments and n_words > 0 and all("words" in s for s in results[0]["segments"])
    # (random weights: a word may hold a line break, so the output is compared as a whole, not line by line)
    want = ""
    for s in segments:
        want += f"[{T.format_timestamp(s['start'])} --> {T.format_timestamp(s['end'])}] {s['text'].strip()}\n"
        for w in s["words"]:
            line = f"{w['start']:.2f}\u2013{w['end']:.2f} {w['word'].strip()} ({w['probability']:.2f})"
            assert re.fullmatch(r"\d+\.\d\d\u2013\d+\.\d\d .*\(\d\.\d\d\)", line, flags=re.DOTALL), line
            want += line + "\n"
    assert out == want
    print(f"CLI: {len(segments)} segments, {n_words} words in {len({s['seek'] for s in results[0]['segments']})} windows")
