"""Prompts per row, host side: upstream's conditioning rules in longform.py (scripted decoders whose output depends on the prompt
they are handed), the right-aligned start rows of decoding.py, and the C ABI's new field.  The device side is
tests/test_gpu_prompts.py.
"""
import ctypes as C
import os
import re
import subprocess
import types

import pytest

import build as B
import longform as LF
import native
import synthetic
from decoding import ROW_PAD_TOKEN, DecodingOptions, WhisperDecoding, right_aligned_rows, row_prompt_layout
from longform import WindowResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, TB = 100, 1000          # frames per window; first timestamp token
NO_THRESHOLDS = dict(compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None)


class Scripted:
    """A decoder whose tokens depend on (file, seek, temperature) AND on the prompt: the text token of a window is a hash of
    all four, so a wrong prompt anywhere changes every later window of the file.  Every window is <|0.00|> text <|a|><|a|>: it
    advances by a timestamp pair, 2 a frames.  `quality[(file, seek, temperature)]` overrides avg_logprob / no_speech_prob /
    compression_ratio; every call is recorded."""

    def __init__(self, advance=(30, 50, 20), quality=None):
        self.advance, self.quality, self.calls = advance, quality or {}, []

    def result(self, f, seek, t, prompt):
        self.calls.append((f, seek, t, tuple(prompt)))
        text = 1 + (hash((f, seek, round(t * 10), tuple(prompt))) % 900)
        a = TB + self.advance[(f + seek) % len(self.advance)] // 2
        return WindowResult(tokens=[TB, text, a, a], temperature=t, **self.quality.get((f, seek, t), {}))

    def one(self, f):
        return lambda seek, t, prompt: self.result(f, seek, t, prompt)

    def batch(self, rows, t, live, prompts):
        assert len(prompts) == len(rows) and all(p == [] for p, r in zip(prompts, rows) if r is None)
        return [self.result(r[0], r[1], t, p) if on else None for r, on, p in zip(rows, live, prompts)]


CONTENTS = [260, 0, 90, 333, 100, 45]


@pytest.mark.parametrize("condition,initial", [(True, ()), (True, (7, 8, 9)), (False, (7, 8, 9))])
@pytest.mark.parametrize("n_rows", [1, 2, 4, 7])
def test_batched_schedule_equals_the_literal_loop_with_prompts(n_rows, condition, initial):
    """Fallback included: some windows fail at temperature 0 and 0.4 and settle at 0.8 (which resets the history)."""
    quality = {(0, 0, 0.0): dict(avg_logprob=-2.0), (3, 30, 0.0): dict(avg_logprob=-2.0), (3, 30, 0.4): dict(compression_ratio=9.0),
               (2, 0, 0.0): dict(compression_ratio=5.0)}
    kw = dict(window=W, timestamp_begin=TB, temperatures=(0.0, 0.4, 0.8), condition_on_previous_text=condition, initial_prompt=initial)
    lit = Scripted(quality=quality)
    want = [LF.transcribe_reference(lit.one(f), c, **kw) for f, c in enumerate(CONTENTS)]
    bat = Scripted(quality=quality)
    got = LF.transcribe_batched(bat.batch, CONTENTS, n_rows, **kw)
    assert got == want and any(want)
    assert sorted(bat.calls) == sorted(lit.calls)                  # the same (file, seek, temperature, prompt) calls, each once
    assert len(set(c[:3] for c in bat.calls)) == len(bat.calls)
    # the fallback calls of a window carry the window's prompt
    by_window = {}
    for f, seek, t, prompt in bat.calls:
        by_window.setdefault((f, seek), set()).add(prompt)
    assert all(len(p) == 1 for p in by_window.values())
    assert any(t == 0.8 for _, _, t, _ in bat.calls)


def test_prompt_grows_by_the_settled_segments_tokens():
    dec = Scripted(advance=(40,))
    segs = LF.transcribe_reference(dec.one(0), 120, window=W, timestamp_begin=TB, temperatures=(0.0,), condition_on_previous_text=True,
                                   initial_prompt=(5, 6), **NO_THRESHOLDS)
    prompts = [list(c[3]) for c in dec.calls]
    assert [c[1] for c in dec.calls] == [0, 40, 80]
    assert prompts[0] == [5, 6]
    # a window's segment keeps its timestamp tokens: <|0.00|> text <|a|>; the second <|a|> opens a segment that is dropped
    w1 = segs[0]["tokens"]
    assert w1[0] == TB and w1[-1] == TB + 20 and len(w1) == 3
    assert prompts[1] == [5, 6] + w1
    assert prompts[2] == [5, 6] + w1 + segs[1]["tokens"]
    assert [s["seek"] for s in segs] == [0, 40, 80]


def test_history_is_forgotten_above_temperature_half_and_without_conditioning():
    # window 2 (seek 40) only settles at 0.8: window 3 starts from nothing; window 4 sees window 3 again
    quality = {(0, 40, 0.0): dict(avg_logprob=-3.0), (0, 40, 0.4): dict(avg_logprob=-3.0)}
    dec = Scripted(advance=(40,), quality=quality)
    segs = LF.transcribe_reference(dec.one(0), 160, window=W, timestamp_begin=TB, temperatures=(0.0, 0.4, 0.8),
                                   condition_on_previous_text=True, compression_ratio_threshold=None, no_speech_threshold=None)
    first = {}
    for f, seek, t, prompt in dec.calls:
        first.setdefault(seek, list(prompt))
    by_seek = {s["seek"]: s["tokens"] for s in segs}
    assert [s["temperature"] for s in segs] == [0.0, 0.8, 0.0, 0.0]
    assert first[0] == [] and first[40] == by_seek[0] and first[80] == [] and first[120] == by_seek[80]
    # a result at 0.4 keeps the history (the rule is > 0.5)
    dec = Scripted(advance=(40,), quality={(0, 40, 0.0): dict(avg_logprob=-3.0)})
    segs = LF.transcribe_reference(dec.one(0), 120, window=W, timestamp_begin=TB, temperatures=(0.0, 0.4, 0.8),
                                   condition_on_previous_text=True, compression_ratio_threshold=None, no_speech_threshold=None)
    assert [s["temperature"] for s in segs] == [0.0, 0.4, 0.0]
    assert list(dec.calls[-1][3]) == segs[0]["tokens"] + segs[1]["tokens"]
    # conditioning off: the initial prompt reaches the first window only, nothing reaches the others
    dec = Scripted(advance=(40,))
    LF.transcribe_reference(dec.one(0), 120, window=W, timestamp_begin=TB, temperatures=(0.0,), initial_prompt=(5, 6), **NO_THRESHOLDS)
    assert [list(c[3]) for c in dec.calls] == [[5, 6], [], []]


def test_a_skipped_window_adds_nothing_and_resets_nothing():
    # window 2 is silence (skipped): window 3 sees exactly what window 2 saw
    quality = {(0, 40, 0.0): dict(no_speech_prob=0.9, avg_logprob=-2.0)}
    dec = Scripted(advance=(40,), quality=quality)
    segs = LF.transcribe_reference(dec.one(0), 180, window=W, timestamp_begin=TB, temperatures=(0.0,), condition_on_previous_text=True)
    seeks = [c[1] for c in dec.calls]
    assert seeks == [0, 40, 140]                                   # a skipped window moves by the whole window
    prompts = [list(c[3]) for c in dec.calls]
    assert prompts[1] == segs[0]["tokens"] and prompts[2] == prompts[1]
    assert [s["seek"] for s in segs] == [0, 140]
    # ... also when conditioning is off: the initial prompt is still waiting for the first window that settles
    quality = {(0, 0, 0.0): dict(no_speech_prob=0.9, avg_logprob=-2.0)}
    dec = Scripted(advance=(40,), quality=quality)
    LF.transcribe_reference(dec.one(0), 180, window=W, timestamp_begin=TB, temperatures=(0.0,), initial_prompt=(5,))
    assert [(c[1], list(c[3])) for c in dec.calls] == [(0, [5]), (100, [5]), (140, [])]


def test_callbacks_without_prompts_are_called_as_before():
    calls = []

    def one(seek, t):
        calls.append((seek, t))
        return WindowResult(tokens=[TB, 5, TB + 20, TB + 20], temperature=t)
    LF.transcribe_reference(one, 80, window=W, timestamp_begin=TB, temperatures=(0.0,), **NO_THRESHOLDS)
    assert calls == [(0, 0.0), (40, 0.0)]


# ------------------------------------------------------------------------------------------------- right-aligned rows
SOT_SEQ, SOT_PREV = (50258, 50259, 50359), 50361


def test_right_aligned_rows():
    n_ctx = 448
    L0, sot_index, capacity = row_prompt_layout(n_ctx, SOT_SEQ, SOT_SEQ[0])
    assert (L0, sot_index, capacity) == (227, 224, 223)
    prompts = [[], [11], [11, 12], list(range(100, 323)), list(range(100, 324)), list(range(1000))]
    rows, starts = right_aligned_rows(prompts, SOT_SEQ, SOT_PREV, n_ctx)
    assert starts == [224, 222, 221, 0, 0, 0]
    for row, start, prompt in zip(rows, starts, prompts):
        assert len(row) == L0 and tuple(row[-3:]) == SOT_SEQ and row[:start] == [ROW_PAD_TOKEN] * start
        assert row[sot_index] == SOT_SEQ[0]
        if prompt:
            assert row[start] == SOT_PREV and row[start + 1:-3] == prompt[-capacity:] and len(row[start + 1:-3]) <= n_ctx // 2 - 1
        else:
            assert SOT_PREV not in row                             # an empty prompt: no <|startofprev|>, as upstream
    assert rows[5][1:-3] == list(range(777, 1000))                 # the LAST n_text_ctx // 2 - 1 tokens
    # an English-only start sequence (2 tokens), a small context
    rows, starts = right_aligned_rows([[], [1, 2, 3, 4, 5, 6, 7, 8, 9]], (50257, 50362), 50360, 16)
    assert starts == [8, 0] and rows[1] == [50360, 3, 4, 5, 6, 7, 8, 9, 50257, 50362] and len(rows[0]) == 10


@pytest.fixture(scope="module")
def engine_dir(tmp_path_factory):
    out = tmp_path_factory.mktemp("prompts_eng") / "eng"
    B.build_from_checkpoint(synthetic.synthetic_checkpoint("micro-fullvocab", 3), B.parse_arguments(["--output_dir", str(out), "--log_level", "error"]))
    return out


def test_instance_with_row_prompts(engine_dir):
    plain = WhisperDecoding(engine_dir, only_torch=True)
    dec = WhisperDecoding(engine_dir, only_torch=True, row_prompts=True)
    tk = dec.tokenizer
    n_ctx = dec.decoder_config['num_text_ctx']
    L0 = n_ctx // 2 + len(tk.sot_sequence)
    assert plain.sample_begin == len(tk.sot_sequence) and not plain.row_prompts
    assert dec.sample_begin == L0 == dec.initial_token_length and dec.sot_index == n_ctx // 2
    assert dec.sample_len == min(n_ctx // 2, n_ctx - L0) == n_ctx // 2 - len(tk.sot_sequence)
    assert WhisperDecoding(engine_dir, only_torch=True, row_prompts=True, options=DecodingOptions(sample_len=5)).sample_len == 5
    # the prompts and the language tokens compose, in either order; candidates share their utterance's start
    langs = [tk.special_tokens["<|de|>"], tk.special_tokens["<|fr|>"], tk.special_tokens["<|ja|>"]]
    prompts = [[], [11, 12], list(range(300))]
    for order in (0, 1):
        d = WhisperDecoding(engine_dir, only_torch=True, row_prompts=True, options=DecodingOptions(best_of=2, temperature=0.5))
        for step in ((d.set_prompts, prompts), (d.set_language_tokens, langs))[::1 if order == 0 else -1]:
            step[0](step[1])
        rows = d._initial_token_rows(3, "cpu")
        assert rows.shape == (6, L0) and d._row_starts.tolist() == [224, 224, 221, 221, 0, 0]
        assert rows[:, d.sot_index].tolist() == [tk.sot] * 6 and rows[:, d.sot_index + 1].tolist() == [l for l in langs for _ in (0, 1)]
        assert rows[2].tolist() == [ROW_PAD_TOKEN] * 221 + [tk.sot_prev, 11, 12, tk.sot, langs[1]] + list(tk.sot_sequence[2:])
        assert rows[4, 0] == tk.sot_prev and rows[4, 1:-3].tolist() == list(range(77, 300))
    # refusals
    with pytest.raises(ValueError, match="row_prompts"):
        plain.set_prompts([[1]])
    with pytest.raises(ValueError, match="prompt"):
        WhisperDecoding(engine_dir, only_torch=True, row_prompts=True, options=DecodingOptions(prompt=[1, 2]))
    dec.set_prompts([[1], [2]])
    with pytest.raises(ValueError, match="2 prompts"):
        dec._initial_token_rows(3, "cpu")
    with pytest.raises(ValueError):
        dec.set_prompts([[10 ** 7]])
    with pytest.raises(ValueError, match="device loop"):
        dec.main_loop_reference(None)
    dec.set_prompts(None)
    assert dec._initial_token_rows(3, "cpu").tolist() == [list(dec.initial_tokens)] * 3 and dec._row_starts.tolist() == [224] * 3
    # an instance without row_prompts is what it was
    assert plain._initial_token_rows(2, "cpu").tolist() == [list(tk.sot_sequence)] * 2
    with_prompt = WhisperDecoding(engine_dir, only_torch=True, options=DecodingOptions(prompt=[1, 2]))
    assert with_prompt.initial_tokens == (tk.sot_prev, 1, 2) + tuple(tk.sot_sequence)


# ------------------------------------------------------------------------------------------------- transcribe.py, C ABI
def test_transcribe_options_and_refusals():
    import transcribe as T
    args = T.parse_arguments(["--input_file", "a.flac", "--condition_on_previous_text", "--initial_prompt", "Dr. Okonkwo"])
    assert args.condition_on_previous_text and args.initial_prompt == "Dr. Okonkwo"
    args = T.parse_arguments(["--input_file", "a.flac"])
    assert not args.condition_on_previous_text and args.initial_prompt is None      # the default stays off

    def instance(row_prompts, **options):
        opt = types.SimpleNamespace(**{**dict(prompt=None, prefix=None, temperature=0.0), **options})
        return types.SimpleNamespace(options=opt, beam=False, n_group=1, row_prompts=row_prompts)
    T.check_supported(instance(True), LF.TEMPERATURES, condition_on_previous_text=True, initial_prompt=[1, 2])
    T.check_supported(instance(True), LF.TEMPERATURES)
    with pytest.raises(ValueError, match="row_prompts=True"):
        T.check_supported(instance(False), LF.TEMPERATURES, condition_on_previous_text=True)
    with pytest.raises(ValueError, match="row_prompts=True"):
        T.check_supported(instance(False), LF.TEMPERATURES, initial_prompt="x")
    with pytest.raises(ValueError, match="initial_prompt"):
        T.check_supported(instance(False, prompt=[1]), LF.TEMPERATURES)


def test_decoder_io_layout_and_abi(tmp_path):
    header = open(os.path.join(ROOT, "include", "whisper_mi355.h")).read()
    assert "#define WM_ABI_VERSION 8" in header and native.ABI_VERSION == 8
    assert re.search(r"\bwm_attn_decode_self_rows\s*\(", header) and "wm_attn_decode_self_rows" in native.EXPORTS
    fields = [n for n, _ in native.WmDecoderIO._fields_]
    assert fields[-2:] == ["not_alone", "row_start"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "whisper_mi355.h"', 'int main(void) {',
           'printf("size %zu\\n", sizeof(wm_decoder_io));']
    src += [f'printf("{f} %zu\\n", offsetof(wm_decoder_io, {f}));' for f in fields]
    src += ['return 0; }']
    (tmp_path / "t.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / "t")], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(native.WmDecoderIO)
    for f in fields:
        assert int(got[f]) == getattr(native.WmDecoderIO, f).offset, f
