"""Block prefill without a GPU: the float64 contract of the two kernels (tests/prefill_refs.py) against the independent row-by-row
statement of tests/prompt_refs.py, the cache codes, the case lists of the GPU tests, the C ABI additions and the host option."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import build as B
import kernel_refs as KR
import native
import prefill_refs as FR
import prompt_refs as PR
import synthetic
from decoding import DecodingOptions, WhisperDecoding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("L,H,starts", [(1, 1, [0, 1]), (5, 2, [0, 3, 5]), (17, 1, [0, 16, 1]), (20, 2, [15, 19, 20]), (33, 1, [17, 0, 32])])
def test_matrix_mask_and_slot_numbers_state_the_same_contract(L, H, starts):
    """prefill_self_ref masks by matrix on attn_decode_ref (float64); self_attn_rows_ref(T = 0) picks the keys by slot numbers (fp32,
    token by token).  The two agree to an fp16 ulp of O(1) outputs (their softmax and dot products run in different precisions)."""
    Bn = len(starts)
    r = KR.philox(300 + L)
    rows = FR.fp16_normal(r, (Bn * L, 3 * H * 64))
    a = FR.prefill_self_ref(rows, starts, Bn, L, H).reshape(Bn, L, H * 64)
    qkv = rows.reshape(Bn, L, 3, H, 64)
    b = PR.self_attn_rows_ref(qkv, torch.zeros((Bn, 2, H, 1, 64)), 0, starts, H)
    assert float((a - b.double()).abs().max()) <= 2.0 ** -10 * max(1.0, float(a.abs().max()))
    for i, s in enumerate(starts):
        assert not a[i, :s].any() and not b[i, :s].any()          # pad queries: zeros in both
        assert a[i, s:].abs().sum() > 0 or s == L


def test_mask_shape():
    m = FR.causal_mask(5, 2)
    assert m[:2].eq(0).all()                                       # pad rows are left open (their output is overwritten)
    assert m[2].tolist() == [float("-inf")] * 2 + [0.0] + [float("-inf")] * 2
    assert m[4].tolist() == [float("-inf")] * 2 + [0.0] * 3
    assert FR.causal_mask(3, 0).eq(torch.zeros(3, 3).masked_fill(torch.ones(3, 3).triu(1).bool(), float("-inf"))).all()


@pytest.mark.parametrize("int8_kv", [0, 1])
def test_cache_rows_are_the_rows_or_their_codes(int8_kv):
    Bn, L, H, t = 2, 7, 2, 0.031
    r = KR.philox(8)
    rows = FR.fp16_normal(r, (Bn * L, 3 * H * 64)) * 3.0           # some values saturate at +-127 t = 3.9
    rows = rows.half().float()
    got = FR.cache_rows(rows, Bn, L, H, int8_kv, t)
    assert got.shape == (Bn, 2, H, L, 64)
    for b in range(Bn):
        for l in range(L):
            for kv in range(2):
                x = rows[b * L + l, (1 + kv) * H * 64:(2 + kv) * H * 64].reshape(H, 64)
                want = KR.self_cache_codes(x, t) if int8_kv else x.half()
                assert torch.equal(got[b, kv, :, l], want)
    if int8_kv:
        assert int(got.max()) == 127 and int(got.min()) == -128    # the saturation is exercised
        assert torch.equal(got, PR.quant_codes(rows[:, H * 64:].reshape(Bn, L, 2, H, 64).permute(0, 2, 3, 1, 4), t))


def test_cross_reference_is_the_unmasked_decode_contract():
    Bn, L, H, Tk = 2, 3, 2, 9
    r = KR.philox(9)
    q = FR.fp16_normal(r, (Bn * L, H * 64))
    kv = FR.fp16_normal(r, (Bn, 2, H, Tk, 64)).half()
    got = FR.prefill_cross_ref(q, kv, Bn, L, H)
    for b in range(Bn):                                            # a row's result is the row's alone
        alone = FR.prefill_cross_ref(q[b * L:(b + 1) * L], kv[b:b + 1], 1, L, H)
        assert torch.equal(got[b * L:(b + 1) * L], alone)


def test_case_lists_cover_what_the_issue_names():
    assert FR.SELF_LENGTHS == [1, 15, 16, 17, 63, 64, 65, 129, 227, 448]
    for L in FR.SELF_LENGTHS:
        sets = FR.start_sets(L)
        used = {s for t in sets for s in t}
        assert all(len(t) == 3 for t in sets) and max(used) == L
        assert used == {s for s in FR.START_POOL if s <= L} | {max(L - 1, 0), L}
    assert len(FR.CROSS_CASES) == 12
    assert {l for l, _ in FR.CROSS_CASES} == {1, 5, 17, 64, 65, 227} and {t for _, t in FR.CROSS_CASES} == {8, 63, 64, 65, 100, 1500}
    v = FR.geometry_values(130)
    assert float(v.abs().max()) <= 2.0 and torch.equal(v * 8, (v * 8).round()) and not torch.equal(v[:64], v[:64].T)


def test_prefill_io_layout_and_abi(tmp_path):
    header = open(os.path.join(ROOT, "include", "whisper_mi355.h")).read()
    assert "#define WM_ABI_VERSION 8" in header and native.ABI_VERSION == 8
    for name in ("wm_decoder_prefill", "wm_decoder_prefill_workspace_bytes", "wm_attn_prefill_self", "wm_attn_prefill_cross"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in native.EXPORTS
    assert [n for n, _ in native.WmPrefillIO._fields_] == ["io", "logits_from"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "whisper_mi355.h"', 'int main(void) {',
           'printf("size %zu\\n", sizeof(wm_prefill_io));', 'printf("io %zu\\n", offsetof(wm_prefill_io, io));',
           'printf("logits_from %zu\\n", offsetof(wm_prefill_io, logits_from));', 'printf("inner %zu\\n", sizeof(wm_decoder_io));', 'return 0; }']
    (tmp_path / "t.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / "t")], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(native.WmPrefillIO) and int(got["inner"]) == C.sizeof(native.WmDecoderIO)
    assert int(got["io"]) == native.WmPrefillIO.io.offset == 0 and int(got["logits_from"]) == native.WmPrefillIO.logits_from.offset
    lib = native.load_library()
    assert lib.wm_decoder_prefill_workspace_bytes(None, 1, 1) == 0          # no engine: no size
    assert lib.wm_decoder_prefill(None, None, None) == 1 and b"decoder engine" in lib.wm_last_error()


@pytest.fixture(scope="module")
def engine_dirs(tmp_path_factory):
    """A micro engine, and a copy whose decoder configuration says int8 cross K/V (the option check reads the configuration: building
    such an engine needs calibration scales, which no option check needs)."""
    import json
    import shutil
    plain = tmp_path_factory.mktemp("prefill_eng") / "eng"
    B.build_from_checkpoint(synthetic.synthetic_checkpoint("micro-fullvocab", 3), B.parse_arguments(["--output_dir", str(plain), "--log_level", "error"]))
    i8 = tmp_path_factory.mktemp("prefill_eng_i8cross") / "eng"
    shutil.copytree(plain, i8)
    cfg = json.load(open(i8 / "decoder_config.json"))
    cfg["builder_config"]["use_int8_cross_kv"] = True
    json.dump(cfg, open(i8 / "decoder_config.json", "w"))
    return {"plain": plain, "i8cross": i8}


def test_block_prefill_option(engine_dirs):
    plain = WhisperDecoding(engine_dirs["plain"], only_torch=True)
    assert plain.block_prefill is False                                     # the default stays off
    dec = WhisperDecoding(engine_dirs["plain"], only_torch=True, row_prompts=True, block_prefill=True)
    assert dec.block_prefill and dec.row_prompts and dec.sample_begin == dec.initial_token_length > 4
    # the option changes nothing of the layout the instance fixes at construction
    ref = WhisperDecoding(engine_dirs["plain"], only_torch=True, row_prompts=True)
    assert (dec.sample_begin, dec.sot_index, dec.sample_len, dec.initial_tokens) == (ref.sample_begin, ref.sot_index, ref.sample_len, ref.initial_tokens)
    with_prompt = WhisperDecoding(engine_dirs["plain"], only_torch=True, block_prefill=True, options=DecodingOptions(prompt=list(range(60))))
    assert with_prompt.initial_token_length == 64 and with_prompt.sot_index == 61
    with pytest.raises(ValueError, match="int8 cross K/V"):
        WhisperDecoding(engine_dirs["i8cross"], only_torch=True, block_prefill=True)
    WhisperDecoding(engine_dirs["i8cross"], only_torch=True)                # without the option such an engine is served as ever


def test_transcribe_flag():
    import transcribe as T
    assert T.parse_arguments(["--input_file", "a.flac"]).block_prefill is False
    args = T.parse_arguments(["--input_file", "a.flac", "--block_prefill"])
    assert args.block_prefill and not args.condition_on_previous_text      # implies nothing else
