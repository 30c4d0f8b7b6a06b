"""Repetition penalty and no-repeat n-grams on the host: the numpy contract (repetition.py) and the two torch filters of the literal
loops (decoding.RepetitionPenalty, decoding.NoRepeatNGram) against the brute force of tests/repeat_refs.py, bit for bit on fp16; the
option checks and refusals; the header and the binding; and the literal loop on the CPU torch path with the controls on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import build as B
import native
import repetition as R
import synthetic
import torch_model as TM
from decoding import DecodingOptions, NoRepeatNGram, RepetitionPenalty, WhisperDecoding, check_decoding_options
from encoding import WhisperEncoding
from oracle.whisper_oracle import Dims, synthetic_mel, synthetic_state_dict
from repeat_refs import controls_batch, controls_row, has_repeated_ngram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, EOT, SAMPLE_BEGIN = 96, 80, 3
PENALTIES = (0.5, 1.0, 1.3, 4.0)
NGRAMS = (0, 1, 2, 3, 5)
# a small alphabet, so that n-grams do come back: text tokens, EOT, a special and two "timestamps"
ALPHABET = np.array([2, 5, 5, 9, 17, 79, EOT, 83, 90, 91])
TINY = np.array([0x0001], dtype=np.uint16).view(np.float16)[0]           # the smallest fp16 subnormal, 2^-24
SPECIAL = [0.0, -0.0, TINY, -TINY, np.float16(3) * TINY, 65504.0, -65504.0, -np.inf, 1.0, -1.0, 0.3333, -7.17]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float16)).view(np.uint16)


def lengths(n):
    return sorted({0, 1, 223} | {k for k in (n - 2, n - 1, n, 2 * n) if k >= 0})


def make_case(rng, m, batch=3):
    """fp16 logits [batch, V] with the special values planted on the alphabet's ids (another rotation per row), and token rows
    [batch, SAMPLE_BEGIN + m] whose start sequence holds alphabet tokens too -- they must not count."""
    logits = (rng.standard_normal((batch, V)) * 4).astype(np.float16)
    ids = sorted(set(ALPHABET.tolist()))
    for b in range(batch):
        for k, t in enumerate(ids):
            logits[b, t] = np.float16(SPECIAL[(k + 3 * b) % len(SPECIAL)])
    hist = rng.choice(ALPHABET, size=(batch, m))
    for b in range(1, batch):                  # row 0 random; the others a phrase of 5 + b tokens over and over, a few slips in it
        phrase = rng.choice(ALPHABET[ALPHABET < EOT], size=5 + b)
        loop = np.resize(phrase, m)
        slip = rng.random(m) < 0.05
        slip[-8:] = False                      # (none near the end: the suffix is the phrase's)
        hist[b] = np.where(slip, hist[b], loop)
    tokens = np.concatenate([np.full((batch, SAMPLE_BEGIN), 5), hist], axis=1).astype(np.int64)
    return logits, tokens


def torch_filters(logits, tokens, p, n):
    """What the literal loops do: the two filters, first in the list, on a torch copy."""
    lg, tk = torch.from_numpy(logits.copy()), torch.from_numpy(tokens)
    if p != 1.0:
        RepetitionPenalty(p, EOT, SAMPLE_BEGIN).apply(lg, tk)
    if n != 0:
        NoRepeatNGram(n, EOT, SAMPLE_BEGIN).apply(lg, tk)
    return lg.numpy()


@pytest.mark.parametrize("n", NGRAMS)
@pytest.mark.parametrize("p", PENALTIES)
def test_contract_and_torch_filters_equal_the_brute_force_bit_for_bit(p, n):
    rng = np.random.default_rng(1000 * n + int(p * 10))
    for m in lengths(n):
        logits, tokens = make_case(rng, m)
        cur = SAMPLE_BEGIN + m
        want = controls_batch(logits, tokens, SAMPLE_BEGIN, cur, EOT, p, n)
        got = R.apply(logits.copy(), tokens, SAMPLE_BEGIN, cur, EOT, p, n)
        assert np.array_equal(bits(got), bits(want)), ("repetition.py", p, n, m)
        assert np.array_equal(bits(torch_filters(logits, tokens, p, n)), bits(want)), ("torch filters", p, n, m)
        if p == 1.0 and n == 0:
            assert np.array_equal(bits(want), bits(logits)), "both off: every bit stays"
        elif m == 223:
            assert not np.array_equal(bits(want), bits(logits)), "the case exercises nothing"
        # tokens >= EOT are never changed, and nothing outside H is
        touched = np.nonzero((bits(want) != bits(logits)).any(axis=0))[0]
        assert all(t < EOT and t in tokens[:, SAMPLE_BEGIN:] for t in touched)


def test_done_rows_are_left_alone():
    rng = np.random.default_rng(5)
    logits, tokens = make_case(rng, 40)
    got = R.apply(logits.copy(), tokens, SAMPLE_BEGIN, SAMPLE_BEGIN + 40, EOT, 1.3, 2, done=[0, 1, 0])
    want = controls_batch(logits, tokens, SAMPLE_BEGIN, SAMPLE_BEGIN + 40, EOT, 1.3, 2, done=[0, 1, 0])
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got[1]), bits(logits[1]))
    assert not np.array_equal(bits(got[0]), bits(logits[0]))


def test_a_token_repeated_fifty_times_is_penalised_once():
    logits = np.linspace(-4, 4, V).astype(np.float16)
    t_pos, t_neg = V - 20, 3
    assert logits[t_pos] > 0 > logits[t_neg]
    H = [t_pos] * 50 + [t_neg] * 50
    for p in (1.3, 0.5, 4.0):
        want = logits.copy()
        want[t_pos] = np.float16(np.float32(logits[t_pos]) / np.float32(p))
        want[t_neg] = np.float16(np.float32(logits[t_neg]) * np.float32(p))
        tokens = np.array([[0] * SAMPLE_BEGIN + H])
        for got in (controls_row(logits, H, EOT, p, 0), R.apply_row(logits.copy(), H, EOT, p, 0),
                    torch_filters(logits[None], tokens, p, 0)[0]):
            assert np.array_equal(bits(got), bits(want)), p


def test_special_tokens_take_part_in_matching_but_are_never_banned():
    ts, a, b = 90, 7, 11
    base = np.ones(V, dtype=np.float16)

    def banned(H, n):
        outs = [controls_row(base, H, EOT, 1.0, n), R.apply_row(base.copy(), H, EOT, 1.0, n),
                torch_filters(base[None], np.array([[0] * SAMPLE_BEGIN + H]), 1.0, n)[0]]
        assert all(np.array_equal(bits(o), bits(outs[0])) for o in outs)
        return set(np.nonzero(np.isneginf(outs[0].astype(np.float32)))[0].tolist())

    assert banned([a, ts, b, ts], 2) == {b}               # the bigram (ts, b) is matched through the timestamp
    assert banned([a, ts, a], 2) == set()                 # (a, ts) would repeat, but a timestamp is never banned
    assert banned([ts, a, EOT, ts, a], 3) == set()        # (ts, a, EOT) would repeat: EOT is not a text token
    assert banned([a, b, ts, a, b], 3) == set() and banned([a, b, 5, a, b], 3) == {5}
    assert banned([a, ts, EOT, b, a], 1) == {a, b}        # n = 1: every text token sampled, and only those


def test_penalty_and_ban_on_one_token_ends_at_minus_infinity():
    logits = np.full(V, 2.0, dtype=np.float16)
    H = [7, 11, 7]
    for fn in (lambda: controls_row(logits, H, EOT, 1.3, 2), lambda: R.apply_row(logits.copy(), H, EOT, 1.3, 2),
               lambda: torch_filters(logits[None], np.array([[0] * SAMPLE_BEGIN + H]), 1.3, 2)[0]):
        out = fn()
        assert np.isneginf(out[11]) and out[7] == np.float16(np.float32(2.0) / np.float32(1.3)) and out[12] == 2.0


# ---- options, refusals --------------------------------------------------------------------------------------------------------
def test_options_default_to_off_and_bad_values_are_refused():
    o = DecodingOptions()
    assert o.repetition_penalty == 1.0 and o.no_repeat_ngram_size == 0 and not R.controls_on(1.0, 0)
    check_decoding_options(DecodingOptions(repetition_penalty=1.2, no_repeat_ngram_size=3))
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.5), dict(repetition_penalty=float("inf")),
                dict(repetition_penalty=float("nan")), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=2.5)):
        with pytest.raises(ValueError, match="repetition_penalty|no_repeat_ngram_size"):
            check_decoding_options(DecodingOptions(**bad))


@pytest.fixture(scope="module")
def cpu_model(tmp_path_factory):
    """micro-fullvocab, model seed 3, on the CPU torch path (how tests/test_torch_path_cpu.py runs the literal loop)."""
    dims = Dims(**synthetic.DIMS["micro-fullvocab"])
    sd = synthetic_state_dict(dims, 3)
    out = tmp_path_factory.mktemp("repeat_cpu") / "eng"
    args = B.parse_arguments(["--output_dir", str(out), "--use_gpt_attention_plugin", "--use_gemm_plugin", "--use_layernorm_plugin", "--log_level", "error"])
    B.build_from_checkpoint({"dims": dims.to_dict(), "model_state_dict": sd}, args)
    model = TM.Whisper(TM.ModelDimensions(**dims.to_dict())).load_state_dict({k: v.float() for k, v in sd.items()})
    return dims, out, model


def test_construction_validates_and_the_partitioned_schedule_refuses(cpu_model):
    _, eng, _ = cpu_model
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=float("nan")), dict(no_repeat_ngram_size=-2)):
        with pytest.raises(ValueError):
            WhisperDecoding(eng, only_torch=True, options=DecodingOptions(**bad))
    off = WhisperDecoding(eng, only_torch=True)
    assert not off.repeat_controls_on and not any(isinstance(f, (RepetitionPenalty, NoRepeatNGram)) for f in off.logit_filters)
    off.cu_partition = True
    off._check_partition(2)                                # the defaults: the schedule serves them as ever
    for opts in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=3)):
        dec = WhisperDecoding(eng, only_torch=True, options=DecodingOptions(**opts))
        assert dec.repeat_controls_on
        # first in the list: the controls act on the raw logits, before Whisper's own filters
        assert isinstance(dec.logit_filters[0], (RepetitionPenalty, NoRepeatNGram))
        assert dec.logit_filters[0].sample_begin == dec.sample_begin and dec.logit_filters[0].eot == dec.tokenizer.eot
        dec._check_partition(2)
        dec.cu_partition = True
        for n_micro in (1, 2):
            with pytest.raises(ValueError, match="cu_partition"):
                dec._check_partition(n_micro)
    both = WhisperDecoding(eng, only_torch=True, options=DecodingOptions(repetition_penalty=1.2, no_repeat_ngram_size=3))
    assert [type(f) for f in both.logit_filters[:2]] == [RepetitionPenalty, NoRepeatNGram]


# ---- header, binding -------------------------------------------------------------------------------------------------------------
def test_header_entry_abi_and_struct_layout(tmp_path):
    header = open(os.path.join(ROOT, "include", "whisper_mi355.h")).read()
    assert "int wm_repeat_controls(" in header and "wm_repeat_controls" in native.EXPORTS
    assert re.search(r"#define WM_ABI_VERSION 8\b", header) and native.ABI_VERSION == 8
    bound = int(re.search(r"#define WM_REPEAT_MAX_HISTORY (\d+)", header).group(1))
    assert bound == R.MAX_HISTORY >= 448
    assert "repeat.hip" in open(os.path.join(ROOT, "eddie-wang-hackathon2023_amd", "csrc", "Makefile")).read()
    names = [n for n, _ in native.WmRepeatIO._fields_]
    assert names == ["logits", "row_stride", "batch", "n_vocab", "tokens", "tokens_ld", "cur_len", "n_past_dev", "sample_begin", "eot",
                     "repetition_penalty", "no_repeat_ngram_size", "done"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "whisper_mi355.h"', 'int main(void){',
           'printf("size %zu\\n", sizeof(wm_repeat_io));']
    src += [f'printf("{f} %zu\\n", offsetof(wm_repeat_io, {f}));' for f in names]
    src.append('return 0;}')
    (tmp_path / "l.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "l.c"), "-o",
                           str(tmp_path / "l")])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / "l")]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(native.WmRepeatIO)
    for f in names:
        assert int(got[f]) == getattr(native.WmRepeatIO, f).offset, f
    lib = native.load_library()
    assert hasattr(lib, "wm_repeat_controls") and lib.wm_version() == 8


# ---- the literal loop on the CPU torch path ----------------------------------------------------------------------------------------
# model seed 3 / mel seed 41 were picked here, on the CPU path, for the property test of tests/test_gpu_repeat.py: with the controls
# off every one of the three rows repeats text tokens (5 to 9 repeats in 24), so the property is not vacuous
MODEL_SEED, MEL_SEED = 3, 41


def _sampled_text(dec, tokens):
    return [[t for t in row[dec.sample_begin:].tolist() if t < dec.tokenizer.eot] for row in tokens]


def test_literal_loop_on_the_cpu_no_text_token_twice_with_unigram_bans(cpu_model):
    dims, eng, model = cpu_model
    enc = WhisperEncoding(eng, only_torch=True)
    mel = synthetic_mel(3, 2 * dims.n_audio_ctx, dims.n_mels, MEL_SEED).float()
    runs = {}
    for n in (0, 1):
        dec = WhisperDecoding(eng, only_torch=True, options=DecodingOptions(sample_len=24, language="en", no_repeat_ngram_size=n))
        tokens, sum_lp, _ = dec.torch_main_loop(model, enc.torch_get_audio_features(model, mel))
        runs[n] = _sampled_text(dec, tokens)
        assert tokens.shape == (3, dec.sample_begin + 24) and torch.isfinite(sum_lp).all()
    assert any(len(r) > len(set(r)) for r in runs[0]), "the baseline no longer repeats: pick other seeds"
    assert all(len(r) == len(set(r)) and len(r) >= 8 for r in runs[1])


def test_literal_loop_on_the_cpu_penalty_and_bigrams(cpu_model):
    dims, eng, model = cpu_model
    enc = WhisperEncoding(eng, only_torch=True)
    mel = synthetic_mel(3, 2 * dims.n_audio_ctx, dims.n_mels, MEL_SEED).float()
    dec = WhisperDecoding(eng, only_torch=True, options=DecodingOptions(sample_len=24, language="en", repetition_penalty=1.2, no_repeat_ngram_size=2))
    tokens, _, _ = dec.torch_main_loop(model, enc.torch_get_audio_features(model, mel))
    eot = dec.tokenizer.eot
    for row in tokens:
        assert not has_repeated_ngram(row[dec.sample_begin:].tolist(), 2, eot)
    ts = dec.tokenizer.timestamp_begin + 5
    assert has_repeated_ngram([7, 11, ts, 7, 11], 2, eot) and not has_repeated_ngram([7, ts, 11, 7, ts], 2, eot)      # (the checker itself)


def test_one_command_line_gives_the_three_clis_the_same_options(tmp_path, monkeypatch):
    """Every logit control set at once: run.py, summarize.py and transcribe.py read the flags through logit_controls and build
    the same DecodingOptions (transcribe.py's reaches its WhisperDecoding, which is recorded here: no engine)."""
    import logit_controls
    import run
    import summarize
    import transcribe
    seq = tmp_path / "bias.json"
    seq.write_text("[[[5, 6], -2.0]]")
    flags = ["--repetition_penalty", "1.3", "--no_repeat_ngram_size", "3", "--hotwords", "Kubernetes, MI355X", "--hotword_bias", "4.5",
             "--hotword_start_bias", "1.5", "--sequence_bias_file", str(seq), "--top_k", "50", "--top_p", "0.9", "--min_p", "0.05"]
    want = DecodingOptions(repetition_penalty=1.3, no_repeat_ngram_size=3, hotwords=("Kubernetes", "MI355X"), hotword_bias=4.5,
                           hotword_start_bias=1.5, sequence_bias=(((5, 6), -2.0),), top_k=50, top_p=0.9, min_p=0.05)
    assert run.decoding_options(run.parse_arguments(flags)) == want
    assert summarize.decoding_options(summarize.parse_arguments(flags)) == want
    built = []
    monkeypatch.setattr(transcribe, "WhisperDecoding", lambda *a, **k: built.append(k["options"]))
    transcribe.build_decoding(transcribe.parse_arguments(["--input_file", "a.wav"] + flags), "unused", False)
    assert built == [want]
    for mod, base in ((run, []), (summarize, []), (transcribe, ["--input_file", "a.wav"])):
        args = mod.parse_arguments(base)
        assert (args.repetition_penalty, args.no_repeat_ngram_size) == (1.0, 0)
        assert DecodingOptions(**logit_controls.options_from_args(args)) == DecodingOptions()
    # run.generate takes the flags as keywords and builds its options from them by parse_arguments' names: every flag is a keyword
    import inspect
    assert set(vars(run.parse_arguments([]))) == set(inspect.signature(run.generate).parameters)
