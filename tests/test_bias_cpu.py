"""Hotwords and sequence bias on the host: the numpy contract (biasing.py) and the torch filter of the literal loops
(decoding.SequenceBias) against the brute force of tests/bias_refs.py, bit for bit on fp16; the table builder, its order, merge rule
and refusals; the options, the three command lines, the header and the binding."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import biasing as BI
import build as B
import native
import repetition as R
import run
import summarize
import synthetic
import transcribe
from bias_refs import bias_batch, bias_row, bias_row_sparse
from decoding import DecodingOptions, NoRepeatNGram, RepetitionPenalty, SequenceBias, WhisperDecoding, check_decoding_options
from oracle.whisper_oracle import Dims, synthetic_state_dict
from tokenizer import Tokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, EOT, SAMPLE_BEGIN = 96, 80, 3
ALPHABET = np.array([2, 5, 5, 9, 17, 79])                       # text tokens a history is drawn from: phrases do come back
SPECIALS = np.array([EOT, 83, 90, 91])                          # EOT, a special, two "timestamps"
TINY = np.array([0x0001], dtype=np.uint16).view(np.float16)[0]
SPECIAL_VALUES = [0.0, -0.0, TINY, -TINY, 65504.0, -65504.0, -np.inf, 1.0, -1.0, 0.3333, -7.17, 65472.0]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float16)).view(np.uint16)


def random_items(rng, n, max_k=4):
    """Any list of items: several on one target, equal (target, prefix) twice, unsorted -- the contract's rule is defined on all of them."""
    items = []
    for _ in range(n):
        k = int(rng.integers(0, max_k + 1))
        items.append((int(rng.choice(ALPHABET)), k, tuple(int(t) for t in rng.choice(ALPHABET, size=k)), float(np.float32(rng.normal() * 4))))
    return items


def make_case(rng, m, batch=3):
    logits = (rng.standard_normal((batch, V)) * 4).astype(np.float16)
    ids = sorted(set(ALPHABET.tolist()) | set(SPECIALS.tolist()))
    for b in range(batch):
        for j, t in enumerate(ids):
            logits[b, t] = np.float16(SPECIAL_VALUES[(j + 3 * b) % len(SPECIAL_VALUES)])
    hist = rng.choice(ALPHABET, size=(batch, m))
    if m > 3:
        hist[0, rng.integers(0, m, size=m // 4)] = rng.choice(SPECIALS, size=m // 4)      # row 0: timestamps and specials in H
    tokens = np.concatenate([np.full((batch, SAMPLE_BEGIN), 5), hist], axis=1).astype(np.int64)  # the start sequence holds an alphabet token too
    return logits, tokens


def torch_filter(logits, tokens, items):
    lg = torch.from_numpy(logits.copy())
    table = type("T", (), {"items": items})()
    SequenceBias(table, EOT, SAMPLE_BEGIN).apply(lg, torch.from_numpy(tokens))
    return lg.numpy()


@pytest.mark.parametrize("n_items", [1, 7, 60])
def test_contract_and_torch_filter_equal_the_brute_force_bit_for_bit(n_items):
    rng = np.random.default_rng(n_items)
    changed = 0
    for m in (0, 1, 2, 3, 4, 5, 40):                             # max_k = 4: m = 0, m < k, m = k, m = k + 1 and beyond all occur
        for _ in range(4):
            items = random_items(rng, n_items)
            logits, tokens = make_case(rng, m)
            cur = SAMPLE_BEGIN + m
            want = bias_batch(logits, tokens, SAMPLE_BEGIN, cur, EOT, items, row=bias_row)
            got = BI.apply(logits.copy(), tokens, SAMPLE_BEGIN, cur, EOT, items)
            assert np.array_equal(bits(got), bits(want)), ("biasing.py", n_items, m)
            assert np.array_equal(bits(bias_batch(logits, tokens, SAMPLE_BEGIN, cur, EOT, items, row=bias_row_sparse)), bits(want)), "the one-pass form"
            assert np.array_equal(bits(torch_filter(logits, tokens, items)), bits(want)), ("torch filter", n_items, m)
            touched = np.nonzero((bits(want) != bits(logits)).any(axis=0))[0]
            assert all(t < EOT and t in [it[0] for it in items] for t in touched)
            changed += touched.size
    assert changed, "the cases exercise nothing"


def test_the_greatest_prefix_wins_and_one_bias_is_applied_not_four():
    a = 7
    table = BI.build_table(hotwords=((a, a, a, a),), hotword_bias=3.0, hotword_start_bias=1.5, eot=EOT)
    assert [(t, k) for t, k, _, _ in table.items] == [(a, 3), (a, 2), (a, 1), (a, 0)]
    base = np.full(V, 2.0, dtype=np.float16)
    for m, bias in ((0, 1.5), (1, 3.0), (2, 3.0), (3, 3.0), (9, 3.0)):
        H = [a] * m
        want = base.copy()
        want[a] = np.float16(np.float32(2.0) + np.float32(bias))          # one bias, whatever number of items match
        outs = [bias_row(base, H, EOT, table.items), BI.apply_row(base.copy(), H, EOT, table),
                torch_filter(base[None], np.array([[0] * SAMPLE_BEGIN + H]), table.items)[0]]
        for o in outs:
            assert np.array_equal(bits(o), bits(want)), m


def test_lengths_around_k_negative_bias_and_minus_infinity():
    a, b, c, ts = 7, 11, 13, 90
    items = BI.build_table(sequence_bias=(((a, b, c), -4.5),), eot=EOT).items
    assert items == [(c, 2, (a, b), -4.5)]
    base = np.full(V, 1.0, dtype=np.float16)

    def moved(H, lg=base):
        outs = [bias_row(lg, H, EOT, items), BI.apply_row(lg.copy(), H, EOT, items), torch_filter(lg[None], np.array([[0] * SAMPLE_BEGIN + H]), items)[0]]
        assert all(np.array_equal(bits(o), bits(outs[0])) for o in outs)
        return {int(t): float(outs[0][t]) for t in np.nonzero(bits(outs[0]) != bits(lg))[0]}

    assert moved([]) == {} and moved([b]) == {} and moved([a, a]) == {}        # m = 0, m < k, m = k without a match
    assert moved([a, b]) == {c: -3.5} and moved([5, a, b]) == {c: -3.5}        # m = k, m = k + 1
    assert moved([a, ts, b]) == {} and moved([a, b, ts]) == {}                 # a timestamp inside or behind the prefix breaks the match
    lg = base.copy()
    lg[c] = -np.inf
    assert moved([a, b], lg) == {}                                             # -inf stays -inf
    # the start sequence is not part of H
    tokens = np.array([[a, b, 0] + [5]])
    assert np.array_equal(bits(BI.apply(base[None].copy(), tokens, 3, 4, EOT, items)), bits(base[None]))
    tokens = np.array([[0, 0, 0] + [a, b]])
    assert BI.apply(base[None].copy(), tokens, 3, 5, EOT, items)[0, c] == np.float16(-3.5)


def test_phrases_that_share_a_prefix_or_a_target():
    table = BI.build_table(hotwords=((7, 11, 13), (7, 11, 17), (9, 2, 13)), eot=EOT)
    base = np.zeros(V, dtype=np.float16)
    out = BI.apply_row(base.copy(), [7, 11], EOT, table)
    assert np.array_equal(bits(out), bits(bias_row(base, [7, 11], EOT, table.items)))
    assert out[13] == 3.0 and out[17] == 3.0 and out[7] == 1.5 and out[9] == 1.5 and out[11] == 0.0 and out[2] == 0.0
    out = BI.apply_row(base.copy(), [9, 2], EOT, table)
    assert out[13] == 3.0 and out[17] == 0.0


def test_done_rows_are_left_alone():
    rng = np.random.default_rng(5)
    logits, tokens = make_case(rng, 12)
    items = [(int(t), 0, (), 2.0) for t in set(ALPHABET.tolist())]
    cur = SAMPLE_BEGIN + 12
    got = BI.apply(logits.copy(), tokens, SAMPLE_BEGIN, cur, EOT, items, done=[0, 1, 0])
    want = bias_batch(logits, tokens, SAMPLE_BEGIN, cur, EOT, items, done=[0, 1, 0])
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got[1]), bits(logits[1]))
    assert not np.array_equal(bits(got[0]), bits(logits[0]))


def test_a_banned_target_stays_banned_when_both_controls_run():
    a, b = 7, 11
    H = [a, b, 5, a]                                              # bigram (a, b) has occurred: b is banned; the hotword (a, b) boosts b
    table = BI.build_table(hotwords=((a, b),), hotword_bias=1000.0, eot=EOT)
    base = np.full(V, 2.0, dtype=np.float16)
    want = bias_row(R.apply_row(base.copy(), H, EOT, 1.0, 2), H, EOT, table.items)
    assert np.isneginf(want[b]) and want[a] == np.float16(3.5)
    lg, tk = torch.from_numpy(base.copy())[None], torch.tensor([[0] * SAMPLE_BEGIN + H])
    for f in (NoRepeatNGram(2, EOT, SAMPLE_BEGIN), SequenceBias(table, EOT, SAMPLE_BEGIN)):
        f.apply(lg, tk)
    assert np.array_equal(bits(lg.numpy()[0]), bits(want))


# ---- the builder --------------------------------------------------------------------------------------------------------------
def test_builder_sorts_merges_and_packs():
    table = BI.build_table(hotwords=((30, 31, 32), (30, 31, 33), (5, 6)), sequence_bias=(((30, 31, 32), 7.0), ((30, 31, 33), -2.0), ((40,), -1.0)),
                           hotword_bias=3.0, hotword_start_bias=1.5, eot=EOT)
    keys = [(t, k) for t, k, _, _ in table.items]
    assert keys == sorted(keys, key=lambda x: (x[0], -x[1])) and len(set((t, p) for t, _, p, _ in table.items)) == len(table)
    by = {(t, p): b for t, _, p, b in table.items}
    assert by[(32, (30, 31))] == 7.0                             # identical (target, prefix): the greater bias stands
    assert by[(33, (30, 31))] == 3.0                             # (3.0 > -2.0)
    assert by[(30, ())] == 1.5 and by[(5, ())] == 1.5 and by[(40, ())] == -1.0 and by[(31, (30,))] == 3.0 and by[(6, (5,))] == 3.0
    assert len(table) == 7
    assert table.packed.dtype.itemsize == 16 and table.packed.shape == (7,) and table.pool.dtype == np.int32
    for (t, k, p, b), rec in zip(table.items, table.packed):
        assert (rec["target"], rec["k"], rec["bias"]) == (t, k, np.float32(b))
        assert tuple(table.pool[rec["offset"]:rec["offset"] + k].tolist()) == p
    assert table.pool.size == 3                                  # (30, 31) once, (30,) is its head, (5,)
    assert len(BI.build_table(eot=EOT)) == 0 and not BI.bias_on(None, None) and not BI.bias_on((), ())


def test_string_hotwords_give_two_encodings():
    tk = Tokenizer.from_vocab(os.path.join(ROOT, "eddie-wang-hackathon2023_amd", "assets", "multilingual.tiktoken"))
    spaced, bare = tuple(tk.encode(" Kubernetes")), tuple(tk.encode("Kubernetes"))
    assert spaced != bare and tk.decode(spaced) == " Kubernetes" and tk.decode(bare) == "Kubernetes"
    table = BI.build_table(hotwords=("Kubernetes",), eot=tk.eot, tokenizer=tk)
    want = BI.build_table(hotwords=(spaced, bare), eot=tk.eot)
    assert table.items == want.items and len(table) == len(set([(p[k], p[:k]) for p in (spaced, bare) for k in range(len(p))]))
    assert {(t, p) for t, _, p, _ in table.items} >= {(spaced[0], ()), (bare[0], ()), (spaced[-1], spaced[:-1]), (bare[-1], bare[:-1])}
    mixed = BI.build_table(hotwords=("Kubernetes", (5, 6)), eot=tk.eot, tokenizer=tk)
    assert len(mixed) == len(table) + 2
    for ids_only in (None, Tokenizer.ids_only()):
        with pytest.raises(ValueError, match="vocabulary"):
            BI.build_table(hotwords=("Kubernetes",), eot=tk.eot, tokenizer=ids_only)
    assert len(BI.build_table(hotwords=((5, 6),), eot=tk.eot, tokenizer=Tokenizer.ids_only())) == 2


def test_builder_refusals():
    ok = dict(eot=EOT)
    BI.build_table(hotwords=(tuple(range(32)),), **ok)                                         # 32 tokens: taken
    BI.build_table(sequence_bias=tuple(((i // 70, i % 70 + 1), 1.0) for i in range(4096)), **ok)     # 4096 items: taken
    for bad in (dict(hotwords=(tuple(range(33)),)), dict(sequence_bias=((tuple(range(33)), 1.0),)),
                dict(hotwords=((5, EOT),)), dict(hotwords=((EOT,),)), dict(hotwords=((90, 5),)), dict(sequence_bias=(((5, 91), 1.0),)),
                dict(sequence_bias=(((91, 5), 1.0),)), dict(hotwords=((),)), dict(hotwords=((-1,),)), dict(hotwords=((1.5,),)), dict(hotwords="ab"),
                dict(hotwords=("",)), dict(sequence_bias=(((5,), float("inf")),)), dict(sequence_bias=(((5,), float("nan")),)),
                dict(sequence_bias=(((5,), 1.0001e4),)), dict(sequence_bias=(((5,), -2e4),)), dict(sequence_bias=((5, 1.0),)),
                dict(sequence_bias=(((5,),),)), dict(hotwords=((5,),), hotword_bias=float("nan")), dict(hotwords=((5,),), hotword_start_bias=1e5),
                dict(sequence_bias=tuple(((i // 70, i % 70 + 1), 1.0) for i in range(4097)))):
        with pytest.raises(ValueError):
            BI.build_table(**bad, **ok)
    with pytest.raises(ValueError, match="4097 items"):
        BI.build_table(sequence_bias=tuple(((i // 70, i % 70 + 1), 1.0) for i in range(4097)), **ok)
    with pytest.raises(ValueError, match="tokens, more than 4096"):                            # the pool: 200 distinct prefixes of 31 tokens
        BI.build_table(sequence_bias=tuple(((i,) * 31 + (i + 1,), 1.0) for i in range(200)), eot=1000)
    BI.build_table(sequence_bias=(((5,), 1e4), ((6,), -1e4)), **ok)                            # the bound itself: taken


# ---- options, construction ------------------------------------------------------------------------------------------------------
def test_options_default_to_off_and_bad_values_are_refused():
    o = DecodingOptions()
    assert o.hotwords is None and o.sequence_bias is None and o.hotword_bias == 3.0 and o.hotword_start_bias == 1.5
    check_decoding_options(DecodingOptions(hotwords=("Kubernetes", (5, 6)), sequence_bias=(((5, 6), -2.0),)))
    for bad in (dict(hotwords=((),)), dict(hotwords="Kubernetes"), dict(hotword_bias=float("nan")), dict(hotword_start_bias=1e5),
                dict(sequence_bias=(((5, 6), float("inf")),)), dict(sequence_bias=((5, 6),)), dict(hotwords=(tuple(range(33)),))):
        with pytest.raises(ValueError):
            check_decoding_options(DecodingOptions(**bad))


@pytest.fixture(scope="module")
def cpu_engine(tmp_path_factory):
    dims = Dims(**synthetic.DIMS["micro-fullvocab"])
    out = tmp_path_factory.mktemp("bias_cpu") / "eng"
    args = B.parse_arguments(["--output_dir", str(out), "--use_gpt_attention_plugin", "--use_gemm_plugin", "--use_layernorm_plugin", "--log_level", "error"])
    B.build_from_checkpoint({"dims": dims.to_dict(), "model_state_dict": synthetic_state_dict(dims, 3)}, args)
    return out


def test_construction_builds_the_table_places_the_filter_and_the_partitioned_schedule_refuses(cpu_engine):
    off = WhisperDecoding(cpu_engine, only_torch=True)
    assert not off.bias_on and off.bias_table is None and not any(isinstance(f, SequenceBias) for f in off.logit_filters)
    off.cu_partition = True
    off._check_partition(2)
    with pytest.raises(ValueError, match="built with"):
        off.set_bias(hotwords=((5, 6),))
    eot = off.tokenizer.eot
    for bad in (dict(hotwords=((5, eot),)), dict(sequence_bias=(((eot + 3, 5), 1.0),)), dict(hotwords=((5,),), hotword_bias=float("inf"))):
        with pytest.raises(ValueError):
            WhisperDecoding(cpu_engine, only_torch=True, options=DecodingOptions(**bad))
    dec = WhisperDecoding(cpu_engine, only_torch=True, options=DecodingOptions(hotwords=("Kubernetes", (5, 6)), sequence_bias=(((7, 8), -2.0),),
                                                                               repetition_penalty=1.2, no_repeat_ngram_size=3))
    assert dec.bias_on and [type(f) for f in dec.logit_filters[:3]] == [RepetitionPenalty, NoRepeatNGram, SequenceBias]
    f = dec.logit_filters[2]
    assert f.table is dec.bias_table and f.sample_begin == dec.sample_begin and f.eot == eot
    assert dec.bias_table.items == BI.build_table(("Kubernetes", (5, 6)), (((7, 8), -2.0),), eot=eot, tokenizer=dec.tokenizer).items
    dec.set_bias(sequence_bias=(((9, 10, 11), 4.0),))
    assert dec.bias_table.items == [(11, 2, (9, 10), 4.0)] and f.table is dec.bias_table
    dec.set_bias()
    assert len(dec.bias_table) == 0 and dec.bias_on
    only = WhisperDecoding(cpu_engine, only_torch=True, options=DecodingOptions(hotwords=((5, 6),)))
    assert isinstance(only.logit_filters[0], SequenceBias)
    only._check_partition(2)
    only.cu_partition = True
    for n_micro in (1, 2):
        with pytest.raises(ValueError, match="cu_partition"):
            only._check_partition(n_micro)


# ---- command lines, header, binding ----------------------------------------------------------------------------------------------
def test_the_three_parsers_accept_the_flags(tmp_path):
    path = tmp_path / "bias.json"
    path.write_text(json.dumps([[[5, 6, 7], -2.5], [[9], 4]]))
    flags = ["--hotwords", "Kubernetes, MI355X", "--hotword_bias", "4.5", "--hotword_start_bias", "0.5", "--sequence_bias_file", str(path)]
    want = dict(hotwords=("Kubernetes", "MI355X"), hotword_bias=4.5, hotword_start_bias=0.5, sequence_bias=(((5, 6, 7), -2.5), ((9,), 4)))
    for mod, extra in ((run, []), (summarize, []), (transcribe, ["--input_file", "a.wav"])):
        args = mod.parse_arguments(extra + flags)
        assert BI.options_from_args(args.hotwords, args.hotword_bias, args.hotword_start_bias, args.sequence_bias_file) == want
        d = mod.parse_arguments(extra)
        assert (d.hotwords, d.hotword_bias, d.hotword_start_bias, d.sequence_bias_file) == (None, 3.0, 1.5, None)
    for mod in (run, summarize):
        o = mod.decoding_options(mod.parse_arguments(flags))
        assert {k: getattr(o, k) for k in want} == want
        o = mod.decoding_options(mod.parse_arguments([]))
        assert o.hotwords is None and o.sequence_bias is None and o == DecodingOptions()
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps({"5": 1.0}))
    with pytest.raises(ValueError, match="JSON list"):
        BI.options_from_args(sequence_bias_file=str(bad))


def test_header_entry_abi_and_struct_layout(tmp_path):
    header = open(os.path.join(ROOT, "include", "whisper_mi355.h")).read()
    assert "int wm_sequence_bias(" in header and "wm_sequence_bias" in native.EXPORTS
    assert re.search(r"#define WM_ABI_VERSION 8\b", header) and native.ABI_VERSION == 8
    for name, value in (("WM_BIAS_MAX_ITEMS", BI.MAX_ITEMS), ("WM_BIAS_MAX_POOL", BI.MAX_POOL), ("WM_BIAS_MAX_K", BI.MAX_K)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value
    assert "bias.hip" in open(os.path.join(ROOT, "eddie-wang-hackathon2023_amd", "csrc", "Makefile")).read()
    names = [n for n, _ in native.WmBiasIO._fields_]
    assert names == ["logits", "row_stride", "batch", "n_vocab", "tokens", "tokens_ld", "cur_len", "n_past_dev", "sample_begin", "eot", "done",
                     "items", "pool", "capacity", "pool_capacity", "n_items_dev"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "whisper_mi355.h"', 'int main(void){',
           'printf("size %zu\\n", sizeof(wm_bias_io));', 'printf("item %zu\\n", sizeof(wm_bias_item));']
    src += [f'printf("{f} %zu\\n", offsetof(wm_bias_io, {f}));' for f in names]
    src += [f'printf("item_{f} %zu\\n", offsetof(wm_bias_item, {f}));' for f in ("target", "k", "offset", "bias")]
    src.append('return 0;}')
    (tmp_path / "l.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "l.c"), "-o",
                           str(tmp_path / "l")])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / "l")]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(native.WmBiasIO) and int(got["item"]) == BI.ITEM_DTYPE.itemsize == 16
    for f in names:
        assert int(got[f]) == getattr(native.WmBiasIO, f).offset, f
    for f in ("target", "k", "offset", "bias"):
        assert int(got["item_" + f]) == BI.ITEM_DTYPE.fields[f][1], f
    lib = native.load_library()
    assert hasattr(lib, "wm_sequence_bias") and lib.wm_version() == 8
