"""CPU-only tests of the host side: the C-ABI library loads and exports every declared symbol,
weight preparation (quantiser, tile layouts, blob), tokenizer, synthetic checkpoints, build.py
artefacts, the host-side logit filters.  No kernel is launched here (no GPU in this container)."""
import ctypes as C
import json
import os
import re
import struct

import numpy as np
import pytest
import torch

import build as B
import native
import synthetic
import tokenizer as T
import weight as W
from oracle import decoding_rules as DR
from oracle import whisper_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- C ABI ----------------------------------------------------------------------------------------
def test_library_loads_and_exports_every_declared_symbol():
    lib = native.load_library()
    header = open(os.path.join(ROOT, "include", "whisper_mi355.h")).read()
    declared = set(re.findall(r"\b(wm_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations found"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/whisper_mi355.h but not exported"
    assert declared == set(native.EXPORTS)
    assert lib.wm_version() == native.ABI_VERSION == 8


def test_struct_layouts_match_header(tmp_path):
    """ctypes mirrors vs the C compiler's view of include/whisper_mi355.h (plain C, gcc)."""
    import subprocess
    fields = {"wm_dims": [n for n, _ in native.WmDims._fields_],
              "wm_decoder_io": [n for n, _ in native.WmDecoderIO._fields_],
              "wm_greedy_io": [n for n, _ in native.WmGreedyIO._fields_],
              "wm_gemv_io": [n for n, _ in native.WmGemvIO._fields_],
              "wm_chain_status": [n for n, _ in native.WmChainStatus._fields_],
              "wm_gemm_io": [n for n, _ in native.WmGemmIO._fields_],
              "wm_row_finish_io": [n for n, _ in native.WmRowFinishIO._fields_],
              "wm_attn_self_io": [n for n, _ in native.WmAttnSelfIO._fields_],
              "wm_attn_cross_io": [n for n, _ in native.WmAttnCrossIO._fields_],
              "wm_attn_encoder_io": [n for n, _ in native.WmAttnEncoderIO._fields_]}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "whisper_mi355.h"', 'int main(void){']
    for s, fs in fields.items():
        src.append(f'printf("{s} %zu\\n", sizeof({s}));')
        src += [f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f in fs]
    src.append('return 0;}')
    (tmp_path / "l.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / "l.c"), "-o", str(tmp_path / "l")])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / "l")]).decode().splitlines())
    for s, cls in (("wm_dims", native.WmDims), ("wm_decoder_io", native.WmDecoderIO), ("wm_greedy_io", native.WmGreedyIO),
                   ("wm_gemv_io", native.WmGemvIO), ("wm_chain_status", native.WmChainStatus),
                   ("wm_gemm_io", native.WmGemmIO), ("wm_row_finish_io", native.WmRowFinishIO),
                   ("wm_attn_self_io", native.WmAttnSelfIO), ("wm_attn_cross_io", native.WmAttnCrossIO),
                   ("wm_attn_encoder_io", native.WmAttnEncoderIO)):
        assert int(got[s]) == C.sizeof(cls), s
        for f in fields[s]:
            assert int(got[f"{s}.{f}"]) == getattr(cls, f).offset, f"{s}.{f}"


def test_engine_create_fails_loudly_on_garbage():
    with pytest.raises(native.WmError, match="bad magic|too small"):
        native.Engine(b"not an engine" * 20, 0)


def test_missing_library_is_an_error_not_a_fallback(tmp_path, monkeypatch):
    monkeypatch.setattr(native, "_lib", None)
    with pytest.raises(native.WmError, match="no fallback"):
        native.load_library(str(tmp_path / "nope.so"))


# ---- weights ----------------------------------------------------------------------------------------
def test_quantizer_is_bit_identical_to_oracle():
    rng = np.random.Generator(np.random.Philox(1))
    w = (rng.standard_normal((96, 320)) * 0.07).astype(np.float16)
    w[3] = 0
    q0, s0 = O.symmetric_quantize_int8(w)
    q1, s1 = W.symmetric_quantize(w)
    assert np.array_equal(q0, q1) and np.array_equal(s0, s1)


@pytest.mark.parametrize("dtype,kt,per", [(np.int8, 64, 16), (np.float16, 32, 8)])
def test_tile_linear_layout(dtype, kt, per):
    n, k = 40, 4 * kt                       # n not a multiple of 16: padded with zero channels
    w = (np.arange(n * k).reshape(n, k) % 251 - 125).astype(dtype)
    t = W.tile_linear(w)
    assert t.shape == (3, 4, 64, per)
    for (nb, tile, lane) in [(0, 0, 0), (1, 2, 37), (2, 3, 63), (2, 1, 8)]:
        ch, g = nb * 16 + (lane & 15), lane >> 4
        want = w[ch, tile * kt + g * per: tile * kt + (g + 1) * per] if ch < n else np.zeros(per, dtype)
        assert np.array_equal(t[nb, tile, lane], want)
    assert np.array_equal(W.untile_linear(t, n), w)


def _parse_blob(blob):
    hdr = struct.unpack_from("<8sIIII10iQQ", blob, 0)
    assert hdr[0] == b"WM355ENG" and hdr[1] == 1
    n, data_off = hdr[3], hdr[15]
    out, off = {}, struct.calcsize("<8sIIII10iQQ")
    for _ in range(n):
        e = struct.unpack_from("<64sII4QQQ", blob, off)
        off += struct.calcsize("<64sII4QQQ")
        out[e[0].rstrip(b"\0").decode()] = dict(dtype=e[1], shape=e[3:3 + e[2]], offset=e[7], nbytes=e[8])
    return dict(kind=hdr[2], flags=hdr[4], dims=hdr[5:15], data_off=data_off, tensors=out)


def test_build_writes_reference_artefacts(tmp_path):
    out = tmp_path / "eng"
    qdir = tmp_path / "quantize" / "1-gpu"
    os.makedirs(qdir)
    for i in range(2):
        np.array([0.01 * (i + 1)], dtype=np.float32).tofile(
            qdir / f"model.decoder.blocks.{i}.attn.query_key_value.scale_y_quant_orig.bin")
    args = B.parse_arguments(["--output_dir", str(out), "--use_gpt_attention_plugin", "--use_gemm_plugin",
                              "--use_layernorm_plugin", "--int8_kv_cache", "--use_weight_only",
                              "--quantize_dir", str(qdir), "--log_level", "error"])
    B.build_from_checkpoint(synthetic.synthetic_checkpoint("micro", 0), args)
    names = sorted(os.listdir(out))
    assert names == sorted(["whisper_encoder_float16_tp1_rank0.engine", "whisper_decoder_float16_tp1_rank0.engine",
                            "whsiper_crossattn_float16_tp1_rank0.engine", "encoder_config.json",
                            "decoder_config.json", "cross_attn_config.json", "positional_embedding.npy"])
    dec = json.load(open(out / "decoder_config.json"))
    for k in ("precision", "tensor_parallel", "num_layers", "num_heads", "num_audio", "num_audio_ctx",
              "num_text_ctx", "hidden_size", "vocab_size", "use_int8_kv_cache"):
        assert k in dec["builder_config"], k
    assert dec["builder_config"]["use_int8_kv_cache"] is True
    assert dec["plugin_config"]["gpt_attention_plugin"] == "float16"
    assert dec["plugin_config"]["weight_only_quant_matmul_plugin"] == "float16"
    enc = json.load(open(out / "encoder_config.json"))
    assert enc["builder_config"]["hidden_size"] == 128 and enc["builder_config"]["num_heads"] == 2
    pe = np.load(out / "positional_embedding.npy")
    assert pe.shape == (32, 128) and pe.dtype == np.float16
    blob = open(out / "whisper_decoder_float16_tp1_rank0.engine", "rb").read()
    p = _parse_blob(blob)
    assert p["kind"] == W.ENGINE_DECODER and p["flags"] == (W.FLAG_WEIGHT_ONLY_INT8 | W.FLAG_INT8_KV)
    assert p["dims"] == tuple(synthetic.DIMS["micro"].values())
    t = p["tensors"]
    assert t["blocks.0.qkv.t"]["dtype"] == 1 and tuple(t["blocks.0.qkv.t"]["shape"]) == (24, 2, 64, 16)
    assert t["emb.t"]["dtype"] == 0 and tuple(t["emb.t"]["shape"]) == (64, 4, 64, 8)       # never quantised
    off = p["data_off"] + t["blocks.1.kv_scale"]["offset"]
    assert abs(struct.unpack_from("<f", blob, off)[0] - 0.02) < 1e-9
    assert all(v["offset"] % 256 == 0 for v in t.values())
    encp = _parse_blob(open(out / "whisper_encoder_float16_tp1_rank0.engine", "rb").read())
    assert encp["tensors"]["conv1.w"]["dtype"] == 0 and tuple(encp["tensors"]["conv1.w"]["shape"]) == (128, 256)
    assert encp["tensors"]["blocks.0.mlp1.w"]["dtype"] == 1
    crs = _parse_blob(open(out / "whsiper_crossattn_float16_tp1_rank0.engine", "rb").read())
    assert tuple(crs["tensors"]["blocks.1.kv.w"]["shape"]) == (256, 128)


def test_int8_kv_build_needs_calibration_files(tmp_path):
    args = B.parse_arguments(["--output_dir", str(tmp_path / "e"), "--int8_kv_cache", "--quantize_dir",
                              str(tmp_path / "missing"), "--log_level", "error"])
    with pytest.raises(FileNotFoundError):
        B.build_from_checkpoint(synthetic.synthetic_checkpoint("micro", 0), args)


def test_fused_weights_follow_reference_fusion():
    ck = synthetic.synthetic_checkpoint("micro", 4)
    sd = ck["model_state_dict"]
    t = W.load_encoder_weight(ck["dims"], sd, 2)
    qkv = t["blocks.0.qkv.w"]
    assert np.array_equal(qkv[:128], sd["encoder.blocks.0.attn.query.weight"].numpy())
    assert np.array_equal(qkv[128:256], sd["encoder.blocks.0.attn.key.weight"].numpy())
    b = t["blocks.0.qkv.b"]
    assert np.array_equal(b[:128], sd["encoder.blocks.0.attn.query.bias"].numpy()) and not b[128:256].any()
    assert np.array_equal(b[256:], sd["encoder.blocks.0.attn.value.bias"].numpy())
    # conv weights: K index = tap * C_in + c_in, conv1 padded to a multiple of 64
    c1 = sd["encoder.conv1.weight"].numpy()
    assert np.array_equal(t["conv1.w"][:, 80:160], c1[:, :, 1]) and not t["conv1.w"][:, 240:].any()
    c = W.load_crossattn_linear_weight(sd, 2)
    assert np.array_equal(c["blocks.1.kv.w"][128:], sd["decoder.blocks.1.cross_attn.value.weight"].numpy())
    # the V bias is loaded (reference bug F3 is not reproduced)
    assert np.array_equal(c["blocks.1.kv.b"][128:], sd["decoder.blocks.1.cross_attn.value.bias"].numpy())
    assert not c["blocks.1.kv.b"][:128].any()


# ---- synthetic / tokenizer ------------------------------------------------------------------------------
def test_synthetic_checkpoint_equals_oracle_copy():
    a = synthetic.synthetic_state_dict(synthetic.DIMS["micro"], 7)
    b = O.synthetic_state_dict(O.MICRO, 7)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(synthetic.synthetic_mel(2, 128, 80, 9), O.synthetic_mel(2, 128, 80, 9))


def test_tokenizer_ids_only_matches_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "tokenizer.npz"))
    tk = T.Tokenizer.ids_only(True, "en", "transcribe")
    assert list(tk.non_speech_tokens) == g["multilingual_non_speech"].tolist()
    assert list(tk.blank_tokens()) == g["multilingual_blank"].tolist()
    assert list(tk.sot_sequence) == g["multilingual_sot_sequence"].tolist()
    assert [tk.eot, tk.sot, tk.translate, tk.transcribe, tk.sot_lm, tk.sot_prev, tk.no_speech, tk.no_timestamps,
            tk.timestamp_begin, tk.n_vocab] == g["multilingual_specials"].tolist()
    en = T.Tokenizer.ids_only(False)
    assert list(en.non_speech_tokens) == g["gpt2_non_speech"].tolist()
    assert en.sot_sequence == (50257,) and en.n_vocab == 51864
    assert len(tk.all_language_tokens) == 99 and tk.all_language_tokens[0] == 50259
    assert tk.decode_with_timestamps([50258, 50259, 50359, 50364]) == "<|startoftranscript|><|en|><|transcribe|><|0.00|>"
    with pytest.raises(RuntimeError):
        tk.encode("hello")


def test_bpe_on_a_toy_vocabulary(tmp_path):
    """Vocabulary mode without the real vocabulary file (it does not travel): 256 byte tokens plus a
    few merges, tiktoken file format."""
    import base64
    toks = [bytes([i]) for i in range(256)] + [b"he", b"ll", b"hell", b"hello", b" w", b" wo"]
    path = tmp_path / "toy.tiktoken"
    with open(path, "w") as f:
        for r, t in enumerate(toks):
            f.write(f"{base64.b64encode(t).decode()} {r}\n")
    tk = T.Tokenizer.from_vocab(str(path), multilingual=True)
    ids = tk.encode("hello world")
    assert ids[0] == 259 and ids[1] == 261 and tk.decode(ids) == "hello world"
    assert tk.eot == 262 and tk.timestamp_begin == 262 + 107


# ---- host-side logit filters vs the reference-generated golden ----------------------------------------------
def test_host_filters_match_reference_golden(golden_dir):
    import decoding as D
    fixr = np.load(os.path.join(golden_dir, "decoding_rules.npz"))
    tk = T.Tokenizer.ids_only(True, "en", "transcribe")
    filters = [D.SuppressBlank(tk, 3), D.SuppressTokens(fixr["suppress"].tolist()), D.ApplyTimestampRules(tk, 3, 50)]
    greedy = D.GreedyDecoder(0.0, tk.eot)
    cases = DR.golden_rule_cases()
    # batched: every history length separately (rows of one batch share cur_len)
    for c, (toks, logits) in enumerate(cases):
        lt = torch.from_numpy(logits.copy())[None]
        tt = torch.from_numpy(toks)[None]
        for f in filters:
            f.apply(lt, tt)
        isinf = np.unpackbits(fixr[f"c{c}_filtered_isinf"])[:lt.shape[1]].astype(bool)
        assert np.array_equal(torch.isinf(lt[0]).numpy(), isinf), c
        s = torch.zeros(1)
        new_tokens, done = greedy.update(tt, lt, s)
        assert int(new_tokens[0, -1]) == int(fixr[f"c{c}_next"]), c
        assert abs(float(s[0]) - float(fixr[f"c{c}_sumlp"])) < 1e-4
        assert done == bool(fixr[f"c{c}_done"])
    # a real batch: three rows with the same length but different histories
    same_len = [i for i, (t, _) in enumerate(cases) if len(t) == 6][:3]
    lt = torch.from_numpy(np.stack([cases[i][1] for i in same_len]))
    tt = torch.from_numpy(np.stack([cases[i][0] for i in same_len]))
    for f in filters:
        f.apply(lt, tt)
    for r, i in enumerate(same_len):
        isinf = np.unpackbits(fixr[f"c{i}_filtered_isinf"])[:lt.shape[1]].astype(bool)
        assert np.array_equal(torch.isinf(lt[r]).numpy(), isinf)


def test_decoding_wrapper_host_only(tmp_path):
    """only_torch=True constructs the wrapper without a GPU, like the reference's calibration path."""
    import decoding as D
    args = B.parse_arguments(["--output_dir", str(tmp_path / "e"), "--log_level", "error"])
    B.build_from_checkpoint(synthetic.synthetic_checkpoint("micro-fullvocab", 0), args)
    dec = D.WhisperDecoding(tmp_path / "e", only_torch=True)
    assert dec.sample_len == 224 and dec.sample_begin == 3 and dec.n_group == 1
    assert dec.initial_tokens == (50258, 50259, 50359)
    sup = dec._get_suppress_tokens()
    assert 50362 in sup and 50358 in sup and 220 not in sup and len(sup) == 82 + 6
    assert dec.max_initial_timestamp_index == round(1.0 / (30 / 64))     # precision = 30 s / n_audio_ctx (decoding.py:343-348)
    assert not dec.use_int8_kv_cache


def test_log_mel_matches_reference_golden(golden_dir, tmp_path):
    """whisper_utils against the reference's own log_mel_spectrogram + mel_filters.npz (tests/golden/mel.npz)."""
    import whisper_utils as wu
    g = np.load(os.path.join(golden_dir, "mel.npz"))
    filt = wu.mel_filters("cpu").numpy()
    assert filt.shape == (80, 201)
    np.testing.assert_allclose(filt.sum(axis=1), g["filters_rowsum"], rtol=1e-4, atol=1e-6)
    assert abs(float(np.abs(filt).sum()) - float(g["filters_checksum"])) < 1e-3
    rng = np.random.Generator(np.random.Philox(int(g["audio_seed"])))
    audio = (rng.standard_normal(int(g["n_audio"])) * 0.1).astype(np.float32)
    mel = wu.log_mel_spectrogram(wu.pad_or_trim(audio, int(g["n_padded"])))
    assert tuple(mel.shape) == g["mel"].shape
    np.testing.assert_allclose(mel.numpy(), g["mel"], atol=2e-4)
    # wav round trip + pad_or_trim on tensors
    import wave
    pcm = (np.clip(audio, -1, 1) * 32767).astype(np.int16)
    with wave.open(str(tmp_path / "a.wav"), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(pcm.tobytes())
    back = wu.load_audio(str(tmp_path / "a.wav"))
    assert back.shape == audio.shape and np.abs(back - pcm / 32768.0).max() == 0
    t = wu.pad_or_trim(torch.ones(2, 10), 14)
    assert tuple(t.shape) == (2, 14) and float(t[:, 10:].abs().sum()) == 0
    assert tuple(wu.pad_or_trim(torch.ones(2, 10), 4).shape) == (2, 4)
    with pytest.raises(RuntimeError):
        wu.load_audio("clip.m4a")          # needs ffmpeg: not decodable here


def test_int4_weight_only_quantiser_and_packing():
    """--weight_only_precision int4 (cutlass_preprocessors.cpp:641-708): scale = absmax / 8, round half away, clamp
    to [-8, 7]; the product quantiser equals the oracle's, and the packed tile layout round-trips."""
    import weight as W
    from oracle.whisper_oracle import symmetric_quantize_int4, dequantize_int8
    rng = np.random.default_rng(5)
    w = (rng.standard_normal((40, 256)) * 0.1).astype(np.float16)
    w[3] = 0                                           # an all-zero channel
    w[7, :4] = [0.35, -0.35, 0.05, -0.05]              # ties and the asymmetric ends of the range
    q, s = W.symmetric_quantize(w, bits=4)
    qo, so = symmetric_quantize_int4(w)
    np.testing.assert_array_equal(q, qo)
    np.testing.assert_array_equal(s, so)
    assert q.min() >= -8 and q.max() <= 7 and q.dtype == np.int8
    absmax = np.abs(w.astype(np.float32)).max(axis=1)
    np.testing.assert_array_equal(s, (absmax / 8).astype(np.float16))
    assert (q[3] == 0).all() and s[3] == 0
    # the channel maximum maps to +-8 before the clamp: +absmax -> 7 (clamped), -absmax -> -8
    ch = int(np.argmax(absmax))
    col = int(np.argmax(np.abs(w[ch].astype(np.float32))))
    assert q[ch, col] == (7 if w[ch, col] > 0 else -8)
    err = np.abs(dequantize_int8(q, s).astype(np.float32) - w.astype(np.float32))
    live = absmax > 0
    assert (err[live] <= (absmax[live, None] / 8) * 1.01 + 1e-3).all()       # within one step (the +7 clamp costs a full one)
    tiles = W.tile_linear_int4(q)
    assert tiles.shape == (3, 2, 64, 16) and tiles.dtype == np.uint8
    np.testing.assert_array_equal(W.untile_linear_int4(tiles, 40), q)
    # lane 16 g + n of tile (nb, kt): channel 16 nb + n, inputs 128 kt + 32 g ..: first word, first nibble = input 0
    assert (tiles[1, 1, 16 * 2 + 5, 0] & 15) == q[16 + 5, 128 + 64] + 8
    assert (tiles[1, 1, 16 * 2 + 5, 0] >> 4) == q[16 + 5, 128 + 64 + 2] + 8   # nibble 1 = input 2
    with pytest.raises(ValueError):
        W.tile_linear_int4(q[:, :192])


def test_balanced_order_deals_sorted_rows_over_the_groups(tmp_path):
    """WhisperDecoding.balanced_order: a batch sorted by expected length is permuted so that every utterance group (a
    contiguous slice, _groups) gets short and long rows alike -- a permutation, group sizes respected, per-group means equal
    to within one step of the sorted sequence."""
    from decoding import WhisperDecoding
    out = tmp_path / "eng"
    B.build_from_checkpoint(synthetic.synthetic_checkpoint("micro", 0), B.parse_arguments(["--output_dir", str(out), "--log_level", "error"]))
    dec = WhisperDecoding(out, only_torch=True)
    for n in (1, 7, 16, 100, 576, 577):
        order = dec.balanced_order(n)
        assert sorted(order) == list(range(n))
        n_micro, bounds = dec._groups(n)
        means = [np.mean(order[lo:hi]) for lo, hi in bounds]
        assert max(means) - min(means) <= n_micro + 2, (n, means)      # (ragged group sizes: the odd row out is the longest)
        for lo, hi in bounds:
            assert order[lo:hi] == sorted(order[lo:hi])            # inside a group the rows stay in sorted order


def test_gemm_rows_generated_code_keeps_the_request_order():
    """csrc/gemm_rows.hip waits for its input rows with a COUNTED `s_waitcnt vmcnt(10)`: correct only while every LDS-DMA request of
    the prologue precedes the ten weight loads in the generated code.  The order is pinned with sched_barriers in the source;
    this checks the ISA of all 24 variants (hipcc -S, no GPU)."""
    import shutil
    import subprocess
    import sys
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not installed")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "check_rows_isa.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    assert r.stdout.count("ok ") == 24


def test_graft_entry_build_runs():
    """`__graft_entry__.build()` is the driver's build check: make (a no-op when the library is current), load, ABI version, imports."""
    import importlib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import sys
    if root not in sys.path:
        sys.path.insert(0, root)
    entry = importlib.import_module("__graft_entry__")
    entry.build()


def test_persistent_gemm_generated_code_matches_its_store_count():
    """csrc/gemm_f16p.hip's generated code (hipcc -S, no GPU; scripts/check_gemm_isa.py): the encoder layers' kernels store 16 bytes per
    lane and instruction (16 per epilogue copy), none of them spills, and each holds the sixteen LDS-DMA requests of the two-slot
    operand stream (a slot in front of the K loop, a slot per slot inside it)."""
    import shutil
    import subprocess
    import sys
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not installed")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "check_gemm_isa.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:]
    assert r.stdout.count("ok ") == 6


def test_encoder_attention_main_loop_stays_at_its_instruction_floor():
    """csrc/attn_encoder.hip's tile loop is VALU-issue bound (one v_exp_f32, one mixed-precision fma, half a pair conversion each for
    the score and the probability, ... per score: the arithmetic contract's roundings): scripts/check_attn_isa.py counts the
    generated instructions per 64-key tile (hipcc -S, no GPU) and fails when the loop grows or spills."""
    import shutil
    import subprocess
    import sys
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not installed")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "check_attn_isa.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    assert r.stdout.count("ok ") == 2


def test_no_prefetch_load_is_waited_for_where_it_is_issued():
    """scripts/check_late_loads.py: in the generated code of the decode path's kernels no memory load is followed directly by a full
    `s_waitcnt vmcnt(0)` beyond the listed, explained sites -- the shape hipcc gives `p ? p[i] : 0` (a branch with the load and its
    wait inside), which cost the one-launch decoder 6 % and every small-batch launch a round trip before round 4 removed it."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_late_loads", os.path.join(ROOT, "scripts", "check_late_loads.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    bad, report = mod.check()
    assert report, "no kernel found"
    assert not bad, bad


def test_only_the_checkers_import_the_oracle():
    """oracle/ is test infrastructure: only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import it (the product
    path has no CPU fallback).  Every Python file of the package, of scripts/ and the two root scripts is read; an `oracle` import
    anywhere else -- or outside those two functions -- fails here (a script under scripts/ still did)."""
    import ast
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def oracle_imports(path):
        tree = ast.parse(open(path).read())
        hits = []
        for fn in ast.walk(tree):
            for node in ast.iter_child_nodes(fn):
                mod = node.module if isinstance(node, ast.ImportFrom) else None
                names = [a.name for a in node.names] if isinstance(node, ast.Import) else []
                if (mod and mod.split(".")[0] == "oracle") or any(n.split(".")[0] == "oracle" for n in names):
                    hits.append(getattr(fn, "name", "<module>"))
        return hits

    offenders = []
    for base in ("eddie-wang-hackathon2023_amd", "scripts"):
        for dirpath, _, files in os.walk(os.path.join(root, base)):
            for f in files:
                if f.endswith(".py") and oracle_imports(os.path.join(dirpath, f)):
                    offenders.append(os.path.relpath(os.path.join(dirpath, f), root))
    assert offenders == [], offenders
    assert set(oracle_imports(os.path.join(root, "bench.py"))) <= {"cpu_baseline"}
    assert set(oracle_imports(os.path.join(root, "__graft_entry__.py"))) <= {"smoke"}


def test_bench_wer_block_says_not_measured_without_real_weights(monkeypatch):
    """bench.py's `wer` block: without WM_CHECKPOINT / WM_LIBRISPEECH (no box of this project has real weights) it says "not measured" and
    why -- never a number; a checkpoint path that does not exist is treated the same."""
    import argparse
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    monkeypatch.delenv("WM_CHECKPOINT", raising=False)
    monkeypatch.delenv("WM_LIBRISPEECH", raising=False)
    b = bench.wer_block(argparse.Namespace(config="int8"))
    assert b["wer"] == "not measured" and "WM_CHECKPOINT missing" in b["wer_note"]
    monkeypatch.setenv("WM_CHECKPOINT", "/nonexistent/large-v2.pt")
    monkeypatch.setenv("WM_LIBRISPEECH", "/nonexistent/test-clean")
    assert bench.wer_block(argparse.Namespace(config="int8"))["wer"] == "not measured"
