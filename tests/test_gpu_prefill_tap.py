"""wm_decoder_prefill_tap on a real MI355X (csrc/decoder.hip, tap_q_kernel in csrc/align.hip): the block
prefill with the cross-attention queries of the alignment heads taped.  Logits and cache are wm_decoder_prefill's bit for bit, tape
rows beyond n_new keep their sentinel, and the tape is the oracle's cross-attention query (fed the block whole, as the block-prefill
tests feed it) within the project's teacher-forced bounds: LOGIT_TOL, and LOGIT_TOL_INT8_KV for an int8 self-K/V engine.

Measured on MI355X (printed by the tests): see DESIGN.md section 5o.
"""
import ctypes as C
import os
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

import build as B  # noqa: E402
import native  # noqa: E402
import synthetic  # noqa: E402
from decoding import WhisperDecoding  # noqa: E402
from encoding import WhisperEncoding  # noqa: E402
from oracle.whisper_oracle import Dims, OracleConfig, OracleModel, synthetic_mel, synthetic_state_dict  # noqa: E402
from test_gpu_model import LOGIT_TOL, LOGIT_TOL_INT8_KV, build_engine  # noqa: E402
from test_gpu_word_timestamps import oracle_cross_queries  # noqa: E402

SENT = 99.0
KV_SCALE = 0.05


@pytest.fixture(scope="module")
def tmpdir_module(tmp_path_factory):
    return str(tmp_path_factory.mktemp("tap_engines"))


def stream():
    return torch.cuda.current_stream().cuda_stream


def run_block(dec, tokens, cross, cap, logits_from, heads=None, tape_rows=None, int8_kv=False):
    """The block through wm_decoder_prefill (heads is None) or wm_decoder_prefill_tap: (logits, caches, tape)."""
    sess, d = dec.decoder_session, dec.decoder_session.dims
    Bn, L = tokens.shape
    kv = [torch.zeros((Bn, 2, d["n_text_head"], cap, 64), dtype=torch.int8 if int8_kv else torch.float16, device="cuda")
          for _ in range(d["n_text_layer"])]
    logits = torch.full((Bn, L, d["n_vocab"]), SENT, dtype=torch.float16, device="cuda")
    tape = None
    if heads is None:
        sess.decoder_prefill(tokens, dec.positional_embedding[0:L], cross, kv, cap, logits, stream(), logits_from)
    else:
        tape = torch.full((Bn, len(heads), tape_rows, 64), SENT, dtype=torch.float16, device="cuda")
        sess.decoder_prefill_tap(tokens, dec.positional_embedding[0:L], cross, kv, cap, logits, stream(), logits_from, tape,
                                 (C.c_int32 * len(heads))(*heads))
    torch.cuda.synchronize()
    return logits, kv, tape


def tape_error(tape, q, heads, H, L, rows=None):
    worst = 0.0
    for slot, hd in enumerate(heads):
        want = q[hd // H][:, :, 64 * (hd % H): 64 * (hd % H) + 64].float()
        got = tape[:, slot, :L].float().cpu()
        if rows is not None:
            want = want[rows]
        worst = max(worst, float((got - want).abs().max()))
    return worst


@pytest.mark.parametrize("weight_only,int8_kv", [(False, False), (True, False), (False, True)])
def test_block_tap_is_bit_identical_and_matches_the_oracle_query(tmpdir_module, weight_only, int8_kv):
    """micro, B = 3, 11 forced tokens in one block."""
    dims = Dims(**synthetic.DIMS["micro"])
    scales = [KV_SCALE] * dims.n_text_layer if int8_kv else None
    tol = LOGIT_TOL_INT8_KV if int8_kv else LOGIT_TOL
    eng = build_engine(tmpdir_module, "micro", 7, weight_only, int8_kv=int8_kv, kv_scales=scales)
    enc, dec = WhisperEncoding(eng), WhisperDecoding(eng)
    mel = synthetic_mel(3, 2 * dims.n_audio_ctx, dims.n_mels, 21)
    cross = dec.xa2cross_key_value(enc.get_audio_features(mel.cuda()))
    tokens = torch.randint(0, dims.n_vocab, (3, 11), generator=torch.Generator().manual_seed(4), dtype=torch.int32).cuda()
    heads = [0, 1, 3]                                                   # layer 0 both heads, layer 1 head 1
    for logits_from in (0, 8):
        plain, kv_plain, _ = run_block(dec, tokens, cross, dims.n_text_ctx, logits_from, int8_kv=int8_kv)
        tapped, kv_tap, tape = run_block(dec, tokens, cross, dims.n_text_ctx, logits_from, heads, 16, int8_kv=int8_kv)
        assert torch.equal(plain, tapped) and all(torch.equal(a, b) for a, b in zip(kv_plain, kv_tap))
        assert bool((plain[:, :logits_from] == SENT).all()) and not bool((plain[:, logits_from:] == SENT).any())
        assert bool((tape[:, :, 11:] == SENT).all()) and not bool((tape[:, :, :11] == SENT).any())      # rows 0 .. n_new - 1 only
    oracle = OracleModel(dims, synthetic_state_dict(dims, 7), OracleConfig(act="float16", weight_only=weight_only, int8_kv=int8_kv, kv_scales=scales))
    q = oracle_cross_queries(oracle, mel, tokens.cpu().long())
    worst = tape_error(tape, q, heads, dims.n_text_head, 11)
    print(f"block tap vs the oracle's cross-attention query (weight_only={weight_only}, int8_kv={int8_kv}): max |diff| = {worst:.3g}, bound {tol}")
    assert worst < tol, worst


def test_block_tap_of_the_split_k_form(tmpdir_module):
    """B = 20 rows x 11 tokens on the split-K chain (wm_set_rows_path(0)) of the 384-wide toy, where the cross-attention query arrives
    in several slabs: the tap adds them in the block cross-attention kernel's order."""
    lib = native.load_library()
    dd = dict(n_mels=80, n_audio_ctx=64, n_audio_state=384, n_audio_head=6, n_audio_layer=1, n_vocab=1024, n_text_ctx=32,
              n_text_state=384, n_text_head=6, n_text_layer=2)
    dims = Dims(**dd)
    out = os.path.join(tmpdir_module, "eng_wide")
    sd = synthetic_state_dict(dims, 9)
    B.build_from_checkpoint({"dims": dd, "model_state_dict": sd},
                            B.parse_arguments(["--output_dir", out, "--use_gpt_attention_plugin", "--use_gemm_plugin", "--use_layernorm_plugin", "--log_level", "error"]))
    enc, dec = WhisperEncoding(Path(out)), WhisperDecoding(Path(out))
    mel = synthetic_mel(20, 2 * dims.n_audio_ctx, dims.n_mels, 22)
    cross = dec.xa2cross_key_value(enc.get_audio_features(mel.cuda()))
    tokens = torch.randint(0, dims.n_vocab, (20, 11), generator=torch.Generator().manual_seed(6), dtype=torch.int32).cuda()
    heads = [1, 6, 11]
    prev = lib.wm_set_rows_path(0)
    try:
        plain, kv_plain, _ = run_block(dec, tokens, cross, dims.n_text_ctx, 0)
        tapped, kv_tap, tape = run_block(dec, tokens, cross, dims.n_text_ctx, 0, heads, 11)
    finally:
        lib.wm_set_rows_path(prev)
    assert torch.equal(plain, tapped) and all(torch.equal(a, b) for a, b in zip(kv_plain, kv_tap))
    q = oracle_cross_queries(OracleModel(dims, sd, OracleConfig(act="float16")), mel, tokens.cpu().long())
    worst = tape_error(tape, q, heads, dims.n_text_head, 11)
    print(f"block tap, split-K form (B = 20) vs the oracle's query: max |diff| = {worst:.3g}, bound {LOGIT_TOL}")
    assert worst < LOGIT_TOL and float(tape.float().abs().max()) > 0.1


def test_block_tap_folds_the_row_index_past_the_grid_limit(tmpdir_module):
    """micro, B = 2048 rows x L = 32 tokens = 65 536 tap rows, one more than a grid's y extent: the smallest block of this model that
    folds.  The rows are four distinct utterances repeated, so four oracle rows vouch for every row on either side of the fold."""
    dims = Dims(**synthetic.DIMS["micro"])
    eng = build_engine(tmpdir_module, "micro", 7)
    enc, dec = WhisperEncoding(eng), WhisperDecoding(eng)
    Bn, L, rep = 2048, dims.n_text_ctx, 512
    assert Bn * L == 65536 and (Bn - 1) * L <= 65535
    mel = synthetic_mel(4, 2 * dims.n_audio_ctx, dims.n_mels, 23)
    cross4 = dec.xa2cross_key_value(enc.get_audio_features(mel.cuda()))
    cross = [c.repeat(rep, 1, 1, 1, 1).contiguous() for c in cross4]
    tokens4 = torch.randint(0, dims.n_vocab, (4, L), generator=torch.Generator().manual_seed(8), dtype=torch.int32)
    tokens = tokens4.repeat(rep, 1).contiguous().cuda()
    heads = [1, 2]
    plain, kv_plain, _ = run_block(dec, tokens, cross, L, L - 1)
    tapped, kv_tap, tape = run_block(dec, tokens, cross, L, L - 1, heads, L)
    assert torch.equal(plain, tapped) and all(torch.equal(a, b) for a, b in zip(kv_plain, kv_tap))
    assert not bool((tape == SENT).any())                                # every one of the 65 536 rows was written
    q = oracle_cross_queries(OracleModel(dims, synthetic_state_dict(dims, 7), OracleConfig(act="float16")), mel, tokens4.long())
    rows = torch.arange(Bn) % 4
    worst = tape_error(tape, q, heads, dims.n_text_head, L, rows)
    last = tape_error(tape[-4:], q, heads, dims.n_text_head, L)          # the rows behind the fold, on their own
    print(f"block tap, 2048 x 32 rows (folded grid) vs the oracle's query: max |diff| = {worst:.3g} (last four rows {last:.3g}), bound {LOGIT_TOL}")
    assert worst < LOGIT_TOL and last < LOGIT_TOL


def test_block_tap_refusals(tmpdir_module):
    """What wm_decoder_prefill refuses, row_start, and the head lists wm_decoder_step_tap refuses: rc 1, nothing launched."""
    lib = native.load_library()
    dims = Dims(**synthetic.DIMS["micro"])
    dec = WhisperDecoding(build_engine(tmpdir_module, "micro", 7))
    sess, H = dec.decoder_session, dims.n_text_head
    Bn, L, cap = 2, 9, dims.n_text_ctx
    cross = [torch.zeros((Bn, 2, H, dims.n_audio_ctx, 64), dtype=torch.float16, device="cuda") for _ in range(dims.n_text_layer)]
    kv = [torch.full((Bn, 2, H, cap, 64), SENT, dtype=torch.float16, device="cuda") for _ in range(dims.n_text_layer)]
    logits = torch.full((Bn, L, dims.n_vocab), SENT, dtype=torch.float16, device="cuda")
    tape = torch.full((Bn, 2, 16, 64), SENT, dtype=torch.float16, device="cuda")
    tokens = torch.zeros((Bn, L), dtype=torch.int32, device="cuda")
    word = torch.zeros(4, dtype=torch.int32, device="cuda")

    def call(mut=None, heads=(0, 3), capacity=16):
        p = native.WmPrefillIO()
        p.io = sess.make_decoder_io(tokens, dec.positional_embedding[0:L], cross, None, 0, kv, cap, logits, 0, prefill=True)
        p.logits_from = 0
        if mut:
            mut(p)
        arr = (C.c_int32 * len(heads))(*heads)
        t = native.WmTapIO()
        t.q_tape, t.capacity, t.heads, t.n_heads = tape.data_ptr(), capacity, C.cast(arr, C.POINTER(C.c_int32)), len(heads)
        rc = lib.wm_decoder_prefill_tap(sess.engine.handle, C.byref(p), C.byref(t), stream())
        return rc, lib.wm_last_error().decode()

    def refused(match, **kw):
        rc, msg = call(**kw)
        assert rc == 1 and "wm_decoder_prefill_tap" in msg and match in msg, (rc, msg)

    refused("n_past", mut=lambda p: setattr(p.io, "n_past", 1))
    refused("n_past_dev", mut=lambda p: setattr(p.io, "n_past_dev", word.data_ptr()))
    refused("row_start", mut=lambda p: setattr(p.io, "row_start", word.data_ptr()))
    refused("logits_from", mut=lambda p: setattr(p, "logits_from", L))
    refused("present capacity", mut=lambda p: setattr(p.io, "present_capacity", L - 1))
    refused("ascending", heads=(3, 0))
    refused("ascending", heads=(0, 0))
    refused("ascending", heads=(0, dims.n_text_layer * H))
    refused("tape capacity", capacity=L - 1)
    torch.cuda.synchronize()
    assert bool((logits == SENT).all()) and bool((tape == SENT).all()) and all(bool((t == SENT).all()) for t in kv), "a refused call launched something"
    rc, msg = call()
    torch.cuda.synchronize()
    assert rc == 0, msg
    assert not bool((tape[:, :, :L] == SENT).any()) and bool((tape[:, :, L:] == SENT).all())
    # an engine with int8 cross K/V is refused as wm_decoder_prefill refuses it
    dec8 = WhisperDecoding(build_engine(tmpdir_module, "micro", 7, cross_scales=[0.05] * dims.n_text_layer))
    cross8 = [torch.zeros((Bn, 2, H, dims.n_audio_ctx, 64), dtype=torch.int8, device="cuda") for _ in range(dims.n_text_layer)]
    with pytest.raises(native.WmError, match="int8 cross K/V"):
        dec8.decoder_session.decoder_prefill_tap(tokens, dec8.positional_embedding[0:L], cross8, kv, cap, logits, stream(), 0, tape[:, :, :, :],
                                                 (C.c_int32 * 2)(0, 3))
