"""Forced alignment end to end on a real MI355X: transcribe.align_mel (forced_align.py) against the host contract (alignment.py), and
WhisperDecoding.word_timestamps(forced_pass="block").  DESIGN.md section 5o.

micro-fullvocab engine with the bundled vocabulary, W = 128 mel frames (64 alignment frames of 0.469 s), synthetic mels, random weights:
WHERE the words land means nothing, so nothing is compared with a known answer.  What is checked:
  1. the recorded rounds (keep_rounds: the device's matrices, token probabilities, paths and end rows) replayed per file through
     alignment.align_reference give the device's end rows, paths, placed words, seeks and final results EXACTLY -- the device matrix is
     the input of both sides, so no near-tie allowance is made and nothing is skipped;
  2. the schedule's invariants hold whatever the batch composition (a file alone, three files on three rows, three files on two rows);
  3. word_timestamps(forced_pass="block"): timing.dtw_cpu on the device's matrix gives the device's path, the words are words_from_path
     of it;
  4. the refusals.
Files: 2.5 windows (320 frames) with a three-line text, 100 frames (shorter than a window) with an empty text, 7 frames with a text that
outlasts it (at most three windows of at most 16 tokens: words must be left over).
"""
import copy
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import alignment as A  # noqa: E402
import native  # noqa: E402
import synthetic  # noqa: E402
import timing  # noqa: E402
import transcribe as T  # noqa: E402
from decoding import WhisperDecoding  # noqa: E402
from encoding import WhisperEncoding  # noqa: E402
from oracle.whisper_oracle import Dims, synthetic_mel  # noqa: E402
from test_gpu_model import build_engine  # noqa: E402

W = 128
FS = 30.0 / W
CONTENTS = [2 * W + W // 2, 100, 7]
LINES = ["The quick brown fox jumps over the lazy dog, and then (quite suddenly) it stops.",
         "Nobody had expected that: not the dog, not the fox, not even the narrator!",
         "So the story ends here, with sixteen more words than anybody needed to hear about a fox."]
LONG = " ".join(f"word{k} and" for k in range(40))
TEXTS = [LINES, "", LONG]
OPTIONS = A.AlignOptions(max_tokens=16, edge_seconds=0.5)


@pytest.fixture(scope="module")
def engines(tmp_path_factory):
    dims = Dims(**synthetic.DIMS["micro-fullvocab"])
    assert 2 * dims.n_audio_ctx == W
    eng = build_engine(str(tmp_path_factory.mktemp("align_engines")), "micro-fullvocab", 3)
    enc, dec = WhisperEncoding(eng), WhisperDecoding(eng)
    assert dec.tokenizer.bpe is not None
    mels = [synthetic_mel(1, c + W, dims.n_mels, 700 + i)[0].half().cuda().contiguous() for i, c in enumerate(CONTENTS)]
    return dims, eng, enc, dec, mels


def run(enc, dec, mels, contents, texts, rows, language="en"):
    rounds = []
    results = T.align_mel(enc, dec, mels, contents, texts, language=language, options=OPTIONS, rows=rows, keep_rounds=rounds)
    return results, rounds


def check_invariants(dec, results, rounds, contents, texts, rows):
    tk = dec.tokenizer
    seeks = {}
    for r in rounds:
        assert len(r["rows"]) == rows
        for row in r["rows"]:
            if row is None:
                continue
            f = row["file"]
            assert row["seek"] > seeks.get(f, -1) and row["next_seek"] > row["seek"]          # seeks strictly grow
            seeks[f] = row["seek"]
            assert 1 <= row["end_row"] <= row["boundaries"][-1] + 1 and 0 <= row["placed"] <= row["n_words"]
            assert len(row["forced"]) <= len(tk.sot_sequence) + 2 + OPTIONS.max_tokens
            assert row["path_time"][-1] == row["n_frames"] - 1 and row["path_text"][-1] == row["end_row"] - 1
    for f, (res, text, content) in enumerate(zip(results, texts, contents)):
        lines, words, toks, owner = A.split_text(tk, text, res["language"])
        duration = content * FS
        if not words:
            assert res["words"] == [] and res["segments"] == [] and res["text"] == ""
            continue
        # every word exactly once and in order (the punctuation merge glues marks to their words: the letters are all there)
        assert "".join(w["word"] for w in res["words"]) == "".join(words)
        flags = [w["aligned"] for w in res["words"]]
        assert flags == sorted(flags, reverse=True)                                           # placed words first, then the leftovers
        on = [w for w in res["words"] if w["aligned"]]
        assert all(0.0 <= w["start"] <= w["end"] <= duration + 1e-9 for w in on)
        assert all(a["end"] <= b["end"] and a["start"] <= b["start"] for a, b in zip(on, on[1:]))
        assert all((w["start"], w["end"], w["probability"]) == (duration, duration, 0.0) for w in res["words"] if not w["aligned"])
        assert all(0.0 <= w["probability"] <= 1.0 for w in res["words"])
        # segments partition the words, one per line
        assert len(res["segments"]) == len(lines) and [w for s in res["segments"] for w in s["words"]] == res["words"]
        for s, line in zip(res["segments"], lines):
            mine = [w for w in s["words"] if w["aligned"]]
            assert s["text"] == line.strip() and s["aligned"] == bool(mine)
            assert (s["start"], s["end"]) == ((mine[0]["start"], mine[-1]["end"]) if mine else (duration, duration))


def replay(dec, results, rounds, contents, texts):
    """Every file's windows again through alignment.align_reference, fed the device's matrices."""
    tk = dec.tokenizer
    for f, (res, text, content) in enumerate(zip(results, texts, contents)):
        mine = [row for r in rounds for row in r["rows"] if row is not None and row["file"] == f]
        lines, words, toks, owner = A.split_text(tk, text, res["language"])
        feed = iter(mine)

        def source(seek, forced, F):
            row = next(feed)
            assert (row["seek"], row["forced"], row["n_frames"]) == (seek, list(forced), F)
            return row["matrix"], row["token_probs"]

        sot = (tk.sot, tk.special_tokens[f"<|{res['language']}|>"], tk.transcribe) if words else tk.sot_sequence
        records = []
        placed = A.align_reference(source, words, toks, owner, content, window=W, seconds_per_frame=2 * FS, sot_sequence=sot,
                                   no_timestamps=tk.no_timestamps, eot=tk.eot, options=OPTIONS, records=records)
        assert next(feed, None) is None and len(records) == len(mine)
        for rec, row in zip(records, mine):
            assert (rec.seek, rec.n_frames, rec.last, rec.first_word) == (row["seek"], row["n_frames"], row["last"], row["first_word"])
            assert rec.end_row == row["end_row"] and rec.placed == row["placed"] and rec.next_seek == row["next_seek"]
            assert rec.path_text.tolist() == row["path_text"].tolist() and rec.path_time.tolist() == row["path_time"].tolist()
        assert A.file_result(res["language"], lines, placed, content * FS) == res


def test_align_replays_exactly_and_keeps_its_invariants(engines):
    dims, eng, enc, dec, mels = engines
    results, rounds = run(enc, dec, mels, CONTENTS, TEXTS, rows=3)
    check_invariants(dec, results, rounds, CONTENTS, TEXTS, 3)
    replay(dec, results, rounds, CONTENTS, TEXTS)
    assert len(dec._state) == 1                                                               # one buffer set for the call
    assert [r["language"] for r in results] == ["en"] * 3
    assert results[1] == dict(language="en", text="", words=[], segments=[])                  # an empty text: an empty result, no window cut
    assert all(row is None or row["file"] != 1 for r in rounds for row in r["rows"])
    assert any(not w["aligned"] for w in results[2]["words"])                                 # the text that outlasts its audio
    windows = [sum(1 for r in rounds for row in r["rows"] if row is not None and row["file"] == f) for f in range(3)]
    assert windows[0] >= 3 and 1 <= windows[2] <= 3
    placed = [sum(w["aligned"] for w in r["words"]) for r in results]
    print(f"align, 3 files on 3 rows: {len(rounds)} rounds, windows per file {windows}, words placed {placed} of "
          f"{[len(r['words']) for r in results]}")


@pytest.mark.parametrize("pick,rows", [([0], 1), ([0, 1, 2], 2), ([2, 0], 2)])
def test_align_batch_composition_leaves_the_invariants(engines, pick, rows):
    """Near-ties in random-weight logits make a row's arithmetic depend on the batch shape: the results are not compared across
    compositions, the contract is."""
    dims, eng, enc, dec, mels = engines
    texts = [LINES, "A short line. ", LONG]
    m, c, t = [mels[i] for i in pick], [CONTENTS[i] for i in pick], [texts[i] for i in pick]
    results, rounds = run(enc, dec, m, c, t, rows=rows, language=None)                       # (the language detected on the first window)
    check_invariants(dec, results, rounds, c, t, rows)
    replay(dec, results, rounds, c, t)
    assert all(r["language"] in dec.tokenizer.all_language_codes for r in results)


def test_word_timestamps_with_the_block_pass(engines):
    dims, eng, enc, dec, mels = engines
    dec = WhisperDecoding(eng)
    dec.sample_len = 12
    dec.keep_alignment_matrix = True
    xa = enc.get_audio_features(synthetic_mel(2, W, dims.n_mels, 77).cuda())
    languages, _ = dec.detect_language(xa)
    t, lp, nsp = dec.main_loop(xa)
    results = dec.post_process(t, lp, nsp, xa, languages)
    frames = [W, 2 * 45 + 1]
    steps = dec.word_timestamps(xa, results, frames, token_probs="device")
    m_steps = dec.last_alignment["matrix"].clone()
    words = dec.word_timestamps(xa, results, frames, token_probs="device", forced_pass="block")
    dev = dec.last_alignment
    assert any(len(w) > 0 for w in words)
    tk, n_prefix, spf = dec.tokenizer, len(dec.tokenizer.sot_sequence), 30.0 / dims.n_audio_ctx
    worst = 0.0
    for b in range(2):
        assert [(w.word, w.tokens) for w in words[b]] == [(w.word, w.tokens) for w in steps[b]]
        if not words[b]:
            continue
        n = dev["path_len"][b]
        text = [x for x in results[b].tokens if x < tk.eot]
        N, F = len(text) + 1, frames[b] // 2
        ti, fi = timing.dtw_cpu(-dev["matrix"][b, :N, :F].numpy())
        assert n == len(ti) and dev["path_text"][b, :n].tolist() == ti.tolist() and dev["path_time"][b, :n].tolist() == fi.tolist()
        ws, wt = dec._split_words(text + [tk.eot], results[b].language)
        own = timing.words_from_path(ti, fi, ws, wt, dev["token_probs"][b, n_prefix: n_prefix + len(text)].tolist(), spf)
        assert own == words[b]
        worst = max(worst, float((dev["matrix"][b, :N, :F] - m_steps[b, :N, :F]).abs().max()))
    print(f"word_timestamps, forced_pass block vs steps: max |matrix diff| = {worst:.3g} (z-scored attention weights; not asserted)")
    t2, lp2, _ = dec.main_loop(xa)
    assert torch.equal(t, t2) and torch.equal(lp, lp2)                                        # the pass leaves main_loop reproducible
    with pytest.raises(ValueError, match="forced_pass"):
        dec.word_timestamps(xa, results, frames, forced_pass="whole")


def test_align_refusals(engines, tmp_path_factory):
    dims, eng, enc, dec, mels = engines
    launched = []
    real = enc.get_audio_features
    enc.get_audio_features = lambda *a, **k: launched.append(1) or real(*a, **k)
    try:
        with pytest.raises(ValueError, match="texts"):
            T.align_mel(enc, dec, mels, CONTENTS, TEXTS[:2])
        with pytest.raises(ValueError, match="texts"):
            T.align_mel(enc, dec, mels[:1], CONTENTS[:1], "a bare string is not a list of texts")
        with pytest.raises(ValueError, match="no audio"):
            T.align_mel(enc, dec, mels, [CONTENTS[0], 0, CONTENTS[2]], TEXTS)
        with pytest.raises(ValueError, match="max_tokens"):
            T.align_mel(enc, dec, mels, CONTENTS, TEXTS, options=A.AlignOptions(max_tokens=445))      # 443 for a 3-token sot_sequence
        with pytest.raises(ValueError, match="max_tokens"):
            T.align_mel(enc, dec, mels, CONTENTS, TEXTS, language="en", options=A.AlignOptions(max_tokens=1))      # a word of two tokens
        with pytest.raises(ValueError, match="Unsupported language"):
            T.align_mel(enc, dec, mels, CONTENTS, TEXTS, language="klingon")
        with pytest.raises(ValueError, match="string"):
            T.align_mel(enc, dec, mels, CONTENTS, [LINES, 5, LONG])
        with pytest.raises(ValueError):
            T.align(enc, dec, [np.zeros(0, dtype=np.float32)], ["hello"])
        dec.cu_partition = True
        try:
            with pytest.raises(ValueError, match="cu_partition"):
                T.align_mel(enc, dec, mels, CONTENTS, TEXTS)
        finally:
            dec.cu_partition = False
        ids_only = copy.copy(dec.tokenizer)
        ids_only.bpe = None
        real_tk, dec.tokenizer = dec.tokenizer, ids_only
        try:
            with pytest.raises(ValueError, match="vocabulary"):
                T.align_mel(enc, dec, mels, CONTENTS, TEXTS)
        finally:
            dec.tokenizer = real_tk
        eng8 = build_engine(str(tmp_path_factory.mktemp("align_x8")), "micro-fullvocab", 3, cross_scales=[0.05] * dims.n_text_layer)
        with pytest.raises(native.WmError, match="int8"):
            T.align_mel(enc, WhisperDecoding(eng8), mels, CONTENTS, TEXTS)
        assert not launched, "a refused call ran the encoder"
    finally:
        enc.get_audio_features = real
    assert T.align_mel(enc, dec, [], [], []) == []


def test_align_cli_prints_a_line_per_line(engines, golden_dir, tmp_path, capsys):
    """align.py on the committed LibriSpeech clip (2.08 s: two windows of this model) with a two-line text file."""
    import align as cli
    dims, eng, enc, dec, mels = engines
    flac = os.path.join(golden_dir, "librispeech_1089-134691-0000.flac")
    txt = tmp_path / "clip.txt"
    txt.write_text("He could wait no longer.\n\nThat is all, he said.\n", encoding="utf-8")
    results = cli.main(cli.parse_arguments(["--engine_dir", str(eng), "--input_file", flac, "--text_file", str(txt), "--language", "en",
                                            "--max_tokens", "8", "--words"]))
    out = capsys.readouterr().out.splitlines()
    res = results[0]
    assert [s["text"] for s in res["segments"]] == ["He could wait no longer.", "That is all, he said."] and res["language"] == "en"
    heads = [l for l in out if l.startswith("[")]
    assert len(heads) == 2 and heads[0].endswith("He could wait no longer.") and heads[1].endswith("That is all, he said.")
    assert all(re.match(r"\[(\d\d:\d\d\.\d{3} --> \d\d:\d\d\.\d{3}|unplaced)\] ", l) for l in heads)
    words = [l for l in out if not l.startswith("[")]
    assert len(words) == len(res["words"]) == 10 and all(re.match(r"\d+\.\d\d–\d+\.\d\d \S+ \(\d\.\d\d\)( unplaced)?$", l) for l in words)
    with pytest.raises(ValueError, match="text files"):
        cli.main(cli.parse_arguments(["--engine_dir", str(eng), "--input_file", flac, flac, "--text_file", str(txt)]))
