"""ctypes binding of libwhisper_mi355.so (include/whisper_mi355.h).

The counterpart of the reference's plugin loader (R/tensorrt_llm/plugin/plugin.py:10-22:
`ctypes.CDLL(libnvinfer_plugin_tensorrt_llm.so)` + `initLibNvInferPlugins`).  There is NO
fallback: if the HIP library is missing or fails to load, importing the engine raises.
"""
from __future__ import annotations

import atexit
import ctypes as C
import os
from typing import Optional, Sequence

# Decode steps are replayed as captured hipGraphs of ~300 dependent short kernels.  ROCm 7's default replays a graph from
# pre-built AQL packets (DEBUG_CLR_GRAPH_PACKET_CAPTURE=1); with the nodes enqueued one by one through the ordinary dispatch
# path instead, every kernel of the chain costs ~0.4 us less on the GPU side: token step B = 1 1.685 -> 1.570 ms, B = 8
# 2.262 -> 2.126, B = 32 3.504 -> 3.423, B = 576 unchanged (23.2 ms, 15.5-15.6 k tokens/s either way) --
# profiles/r3ah_bench_*.json, sweep of the other launch-path knobs in profiles/r3ag_launch_knobs.txt.  The flag is read when
# the HIP runtime initialises (first HIP call of the process), so it is set here, at import, unless the caller chose a value:
# import this package before the first torch.cuda call, or export the variable.  Same kernels, same results.
#
# DEBUG_CLR_GRAPH_PACKET_CAPTURE is a debug switch of the HIP runtime, not a documented interface: it is process-wide (every HIP
# user of the process replays its graphs node by node), it takes effect only if it is in the environment before the process's
# first HIP call, and a ROCm update may drop it.  So: a value chosen by the caller wins; WM_GRAPH_NODE_REPLAY=0 keeps this
# package from touching the variable at all; the package records what it did and whether it was in time (RUNTIME_KNOBS,
# runtime_report() -- bench.py and summarize.py print it) and warns when the runtime was already initialised; and
# tests/test_gpu_round4.py::test_graph_node_replay_still_pays fails when the switch stops making the batch-1 step faster.
import sys
import warnings


def _hip_already_initialised() -> bool:
    t = sys.modules.get("torch")
    try:
        return bool(t is not None and t.cuda.is_initialized())
    except Exception:       # noqa: BLE001
        return False


def _configure_runtime() -> dict:
    name = "DEBUG_CLR_GRAPH_PACKET_CAPTURE"
    late = _hip_already_initialised()
    if name in os.environ:
        return {"name": name, "value": os.environ[name], "set_by": "caller", "in_time": None}      # the caller's business, and timing
    if os.environ.get("WM_GRAPH_NODE_REPLAY", "1") == "0":
        return {"name": name, "value": None, "set_by": "nobody (WM_GRAPH_NODE_REPLAY=0)", "in_time": None}
    os.environ[name] = "0"
    if late:
        warnings.warn("whisper_mi355: the HIP runtime was initialised before this package was imported, so "
                      f"{name}=0 (node-by-node graph replay, 6-10 % of the small-batch token step) is NOT in effect: "
                      "import the package before the first torch.cuda call, or export the variable yourself", RuntimeWarning, stacklevel=3)
    return {"name": name, "value": "0", "set_by": "package", "in_time": not late}


RUNTIME_KNOBS = _configure_runtime()


def runtime_report() -> dict:
    """What this package did to the HIP runtime's environment, whether it was in time, and the lab knobs the library honoured."""
    rep = dict(RUNTIME_KNOBS)
    rep["effective_env"] = os.environ.get(RUNTIME_KNOBS["name"])
    if _lib is not None:
        buf = C.create_string_buffer(4096)
        _lib.wm_lab_knobs(buf, 4096)
        rep["lab_knobs_honoured"] = buf.value.decode() or None
    return rep


_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WM_LIBRARY_PATH") or os.path.join(_HERE, "libwhisper_mi355.so")

EXPORTS = (
    "wm_version", "wm_last_error", "wm_device_count", "wm_engine_create", "wm_engine_destroy",
    "wm_engine_info", "wm_engine_weight_bytes", "wm_encoder_workspace_bytes", "wm_encoder_forward",
    "wm_encoder_forward_shared", "wm_encoder_forward_range",
    "wm_cross_kv_workspace_bytes", "wm_cross_kv", "wm_decoder_workspace_bytes", "wm_decoder_step",
    "wm_greedy_step", "wm_gemm", "wm_gemm_skinny", "wm_gemm_skinny_default_ksplit", "wm_layernorm",
    "wm_attn_encoder", "wm_attn_decode_cross", "wm_attn_decode_self", "wm_quantize_i8",
    "wm_profile_configure", "wm_profile_read", "wm_step_advance", "wm_log_mel_workspace_bytes", "wm_log_mel",
    "wm_flac_info", "wm_flac_decode", "wm_conv1d_gelu", "wm_argmax", "wm_gemv_fused", "wm_gemm_rows", "wm_set_rows_path", "wm_set_small_batch_rows", "wm_set_self_attn_waves", "wm_set_gemm_small_tiles", "wm_lab_knobs", "wm_set_cross_v_skip", "wm_set_decode_chain", "wm_decode_chain_error", "wm_decode_chain_status", "wm_debug_occupy", "wm_decoder_step_multi", "wm_stream_create_cu_mask", "wm_stream_destroy", "wm_attn_decode_cross_i8", "wm_debug_timeline",
    "wm_step_finish",
    "wm_beam_workspace_bytes", "wm_beam_step", "wm_kv_reorder",
    "wm_gemm_ex", "wm_row_finish", "wm_embed", "wm_mel_transpose_pad", "wm_zero_pad_rows",
    "wm_decoder_step_tap", "wm_align_workspace_bytes", "wm_align", "wm_dtw_workspace_bytes", "wm_dtw",
    "wm_mel_windows", "wm_resample", "wm_attn_decode_self_rows",
    "wm_attn_self_ex", "wm_attn_cross_ex",
    "wm_forced_probs",
    "wm_section_cuts_workspace_bytes", "wm_section_cuts",
    "wm_speech_spans_workspace_bytes", "wm_speech_spans", "wm_mel_gather",
    "wm_step_finish_group", "wm_attn_cross_group_ex", "wm_decoder_step_group",
    "wm_decoder_prefill_workspace_bytes", "wm_decoder_prefill", "wm_attn_prefill_self", "wm_attn_prefill_cross",
    "wm_repeat_controls",
    "wm_attn_encoder_ex",
    "wm_sequence_bias",
    "wm_sample_step",
    "wm_resample_channels", "wm_channel_top_workspace_bytes", "wm_channel_top",
    "wm_dtw_open", "wm_align_open", "wm_decoder_prefill_tap",
    "wm_verify_workspace_bytes", "wm_verify_step",
)


ABI_VERSION = 8          # WM_ABI_VERSION of include/whisper_mi355.h this binding was written against

# Held by WhisperDecoding.main_loop for the length of a stream capture and by WhisperEncoding.prefetch's helper thread around every call
# it makes into the HIP runtime (event queries, launches): a runtime call from another thread while a capture is open can invalidate it.
import threading as _threading
CAPTURE_LOCK = _threading.RLock()


class WmError(RuntimeError):
    pass


class WmFlacStreamInfo(C.Structure):
    """wm_flac_streaminfo (include/whisper_mi355.h)."""
    _fields_ = [("sample_rate", C.c_int32), ("channels", C.c_int32), ("bits_per_sample", C.c_int32),
                ("max_block_size", C.c_int32), ("total_samples", C.c_int64), ("md5", C.c_uint8 * 16)]


class WmChainStatus(C.Structure):
    """wm_chain_status (include/whisper_mi355.h)."""
    _fields_ = [("mode", C.c_int32), ("declined", C.c_int32), ("error_pending", C.c_int32), ("pad_", C.c_int32),
                ("launches", C.c_int64), ("declined_calls", C.c_int64), ("reason", C.c_char * 200), ("footprint", C.c_char * 200)]


def chain_status() -> dict:
    """wm_decode_chain_status of the current device as a dict (tests, diagnostics)."""
    st = WmChainStatus()
    check(load_library().wm_decode_chain_status(C.byref(st)), "wm_decode_chain_status")
    return {"mode": st.mode, "declined": bool(st.declined), "error_pending": bool(st.error_pending), "launches": int(st.launches),
            "declined_calls": int(st.declined_calls), "reason": st.reason.decode(), "footprint": st.footprint.decode()}


class WmDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "n_mels", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer",
        "n_vocab", "n_text_ctx", "n_text_state", "n_text_head", "n_text_layer")]

    def to_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class WmDecoderIO(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("n_new", C.c_int32), ("n_past", C.c_int32),
        ("tokens", C.c_void_p), ("tokens_ld", C.c_int32), ("positional_embedding", C.c_void_p),
        ("past", C.POINTER(C.c_void_p)), ("past_capacity", C.c_int32),
        ("present", C.POINTER(C.c_void_p)), ("present_capacity", C.c_int32),
        ("cross", C.POINTER(C.c_void_p)),
        ("logits", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("qkv_amax", C.c_void_p),
        ("n_past_dev", C.c_void_p),
        ("live_rows", C.c_void_p),
        ("workspace_id", C.c_uint64),
        ("not_alone", C.c_int32),
        ("row_start", C.c_void_p),
    ]


class WmDecoderGroupIO(C.Structure):
    """wm_decoder_group_io (include/whisper_mi355.h): a decoder call whose rows share cross K/V in groups of `cross_group`."""
    _fields_ = [("io", WmDecoderIO), ("cross_group", C.c_int32), ("live_groups", C.c_void_p)]


class WmPrefillIO(C.Structure):
    """wm_prefill_io (include/whisper_mi355.h): a whole start block on an empty cache, logits from position `logits_from` on."""
    _fields_ = [("io", WmDecoderIO), ("logits_from", C.c_int32)]


class WmGemvIO(C.Structure):
    """wm_gemv_io (include/whisper_mi355.h)."""
    _fields_ = [
        ("a", C.c_void_p), ("lda", C.c_int32), ("m", C.c_int32), ("k", C.c_int32),
        ("wt", C.c_void_p), ("n_blocks", C.c_int32), ("w8", C.c_int32), ("scale", C.c_void_p),
        ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p),
        ("mode", C.c_int32), ("bias", C.c_void_p), ("gelu_kind", C.c_int32),
        ("out32", C.c_void_p), ("ld32", C.c_int32),
        ("out16", C.c_void_p), ("ld16", C.c_int32), ("n_valid", C.c_int32),
        ("x", C.c_void_p), ("ldx", C.c_int32),
    ]


class WmGreedyIO(C.Structure):
    _fields_ = [
        ("logits", C.c_void_p), ("row_stride", C.c_int64),
        ("batch", C.c_int32), ("n_vocab", C.c_int32),
        ("tokens", C.c_void_p), ("tokens_ld", C.c_int32), ("cur_len", C.c_int32),
        ("sum_logprobs", C.c_void_p),
        ("suppress", C.c_void_p), ("n_suppress", C.c_int32),
        ("blank", C.c_void_p), ("n_blank", C.c_int32),
        ("sample_begin", C.c_int32), ("eot", C.c_int32), ("timestamp_begin", C.c_int32),
        ("max_initial_timestamp_index", C.c_int32),
        ("apply_rules", C.c_int32),
        ("n_done", C.c_void_p),
        ("n_past_dev", C.c_void_p),
        ("done", C.c_void_p),
        ("row_limit", C.c_void_p),
        ("temperature", C.c_float), ("row0", C.c_int32),
        ("seed", C.c_uint64), ("seed_dev", C.c_void_p),
    ]


class WmRepeatIO(C.Structure):
    """wm_repeat_io (include/whisper_mi355.h): repetition penalty and no-repeat n-grams on the raw logits of a token step."""
    _fields_ = [
        ("logits", C.c_void_p), ("row_stride", C.c_int64),
        ("batch", C.c_int32), ("n_vocab", C.c_int32),
        ("tokens", C.c_void_p), ("tokens_ld", C.c_int32),
        ("cur_len", C.c_int32),
        ("n_past_dev", C.c_void_p),
        ("sample_begin", C.c_int32), ("eot", C.c_int32),
        ("repetition_penalty", C.c_float),
        ("no_repeat_ngram_size", C.c_int32),
        ("done", C.c_void_p),
    ]


class WmBiasIO(C.Structure):
    """wm_bias_io (include/whisper_mi355.h): hotwords and sequence bias on the raw logits of a token step."""
    _fields_ = [
        ("logits", C.c_void_p), ("row_stride", C.c_int64),
        ("batch", C.c_int32), ("n_vocab", C.c_int32),
        ("tokens", C.c_void_p), ("tokens_ld", C.c_int32),
        ("cur_len", C.c_int32),
        ("n_past_dev", C.c_void_p),
        ("sample_begin", C.c_int32), ("eot", C.c_int32),
        ("done", C.c_void_p),
        ("items", C.c_void_p), ("pool", C.c_void_p),
        ("capacity", C.c_int32), ("pool_capacity", C.c_int32),
        ("n_items_dev", C.c_void_p),
    ]


class WmSampleIO(C.Structure):
    """wm_sample_io (include/whisper_mi355.h): a sampled token step with the draw restricted by top-k / top-p / min-p."""
    _fields_ = [
        ("g", WmGreedyIO),
        ("top_k", C.c_int32), ("exp2_scale", C.c_float), ("top_p_q16", C.c_int32), ("min_p_gap", C.c_float),
        ("cut_out", C.c_void_p), ("kept_out", C.c_void_p),
    ]


class WmVerifyIO(C.Structure):
    """wm_verify_io (include/whisper_mi355.h): the verify step of speculative decoding over n_pos positions of every row."""
    _fields_ = [
        ("g", WmGreedyIO),
        ("pos_stride", C.c_int64), ("n_pos", C.c_int32),
        ("n_accept", C.c_void_p), ("workspace", C.c_void_p),
    ]


class WmBeamIO(C.Structure):
    """wm_beam_io (include/whisper_mi355.h)."""
    _fields_ = [
        ("logits", C.c_void_p), ("row_stride", C.c_int64),
        ("batch", C.c_int32), ("n_vocab", C.c_int32),
        ("tokens", C.c_void_p), ("tokens_ld", C.c_int32), ("cur_len", C.c_int32),
        ("sum_logprobs", C.c_void_p),
        ("suppress", C.c_void_p), ("n_suppress", C.c_int32),
        ("blank", C.c_void_p), ("n_blank", C.c_int32),
        ("sample_begin", C.c_int32), ("eot", C.c_int32), ("timestamp_begin", C.c_int32),
        ("max_initial_timestamp_index", C.c_int32),
        ("apply_rules", C.c_int32),
        ("beam_size", C.c_int32), ("max_candidates", C.c_int32), ("ignore_eot", C.c_int32),
        ("n_past_dev", C.c_void_p),
        ("row_limit", C.c_void_p),
        ("parent", C.c_void_p),
        ("fin_tokens", C.c_void_p), ("fin_scores", C.c_void_p), ("fin_len", C.c_void_p), ("fin_count", C.c_void_p),
        ("live_len", C.c_void_p),
        ("done", C.c_void_p),
        ("n_done", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


class WmGemmIO(C.Structure):
    """wm_gemm_io (include/whisper_mi355.h): the MFMA GEMM with every option the engines set (tests)."""
    _fields_ = [
        ("a", C.c_void_p), ("lda", C.c_int32), ("m", C.c_int32), ("k", C.c_int32),
        ("w", C.c_void_p), ("n", C.c_int32),
        ("bias", C.c_void_p),
        ("c", C.c_void_p), ("ldc", C.c_int32),
        ("residual", C.c_void_p), ("ldr", C.c_int32), ("res_mod", C.c_int32),
        ("act", C.c_int32),
        ("colscale_n", C.c_int32), ("colscale", C.c_float),
        ("out_mode", C.c_int32), ("hs_t", C.c_int32), ("hs_h", C.c_int32), ("hs_kv", C.c_int32),
        ("q8_inv_scale", C.c_float),
        ("a_rows", C.c_int32), ("a_bstride", C.c_int64),
        ("c_rows", C.c_int32), ("c_bstride", C.c_int64),
        ("max_wgs", C.c_int32), ("tile_rows", C.c_int32),
    ]


class WmRowFinishIO(C.Structure):
    """wm_row_finish_io (include/whisper_mi355.h): the row kernel of the split-K decode path (tests)."""
    _fields_ = [
        ("part", C.c_void_p), ("ksplit", C.c_int32), ("m", C.c_int32), ("n", C.c_int32), ("ldp", C.c_int32),
        ("part_sstride", C.c_int64),
        ("bias", C.c_void_p),
        ("mode", C.c_int32), ("gelu_kind", C.c_int32),
        ("x", C.c_void_p), ("ldx", C.c_int32),
        ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p),
        ("out", C.c_void_p), ("ldo", C.c_int32),
    ]


class WmAttnSelfIO(C.Structure):
    """wm_attn_self_io (include/whisper_mi355.h): the decode self-attention with every field the decoder engine sets (tests)."""
    _fields_ = [
        ("part", C.c_void_p), ("ksplit", C.c_int32), ("ldp", C.c_int32), ("part_sstride", C.c_int64),
        ("bias", C.c_void_p),
        ("B", C.c_int32), ("L", C.c_int32), ("T", C.c_int32), ("H", C.c_int32),
        ("past", C.c_void_p), ("past_bstride", C.c_int64), ("past_cap", C.c_int32),
        ("present", C.c_void_p), ("present_bstride", C.c_int64), ("present_cap", C.c_int32),
        ("int8_kv", C.c_int32), ("kv_scale", C.c_float),
        ("amax", C.c_void_p),
        ("t_dev", C.c_void_p),
        ("out", C.c_void_p), ("ldo", C.c_int32),
        ("live", C.c_void_p),
        ("row_start", C.c_void_p),
        ("waves", C.c_int32),
    ]


class WmAttnCrossIO(C.Structure):
    """wm_attn_cross_io (include/whisper_mi355.h): the decode cross-attention with every field the decoder engine sets (tests)."""
    _fields_ = [
        ("part", C.c_void_p), ("ksplit", C.c_int32), ("ldp", C.c_int32), ("part_sstride", C.c_int64),
        ("bias", C.c_void_p),
        ("B", C.c_int32), ("L", C.c_int32), ("H", C.c_int32), ("Tk", C.c_int32),
        ("kv", C.c_void_p), ("kv_bstride", C.c_int64),
        ("kv_q8_scale", C.c_float),
        ("out", C.c_void_p), ("ldo", C.c_int32),
        ("nsplit", C.c_int32),
        ("ws", C.c_void_p),
        ("live", C.c_void_p),
        ("skip_zero_rows", C.c_int32),
    ]


class WmAttnCrossGroupIO(C.Structure):
    """wm_attn_cross_group_io (include/whisper_mi355.h): wm_attn_cross_io for candidate groups that share one K/V row (tests)."""
    _fields_ = WmAttnCrossIO._fields_ + [("G", C.c_int32), ("live_utt", C.c_void_p)]


class WmAttnEncoderIO(C.Structure):
    """wm_attn_encoder_io (include/whisper_mi355.h): the encoder attention with every field the encoder engine sets (tests)."""
    _fields_ = [
        ("qkv", C.c_void_p), ("ld", C.c_int32),
        ("B", C.c_int32), ("T", C.c_int32), ("H", C.c_int32),
        ("out", C.c_void_p), ("ldo", C.c_int32),
        ("max_wgs", C.c_int32),
    ]


class WmTapIO(C.Structure):
    """wm_tap_io (include/whisper_mi355.h): where wm_decoder_step_tap writes the cross-attention queries."""
    _fields_ = [("q_tape", C.c_void_p), ("capacity", C.c_int32), ("heads", C.POINTER(C.c_int32)), ("n_heads", C.c_int32)]


class WmAlignIO(C.Structure):
    """wm_align_io (include/whisper_mi355.h): alignment matrix + DTW of a batch (word timestamps)."""
    _fields_ = [
        ("engine", C.c_void_p),
        ("batch", C.c_int32), ("n_text_head", C.c_int32), ("n_audio_ctx", C.c_int32),
        ("q_tape", C.c_void_p), ("capacity", C.c_int32),
        ("cross", C.POINTER(C.c_void_p)), ("n_layers", C.c_int32),
        ("heads", C.POINTER(C.c_int32)), ("n_heads", C.c_int32),
        ("n_tokens", C.c_void_p),
        ("n_frames", C.c_void_p),
        ("n_prefix", C.c_int32), ("filter_width", C.c_int32),
        ("cap_tokens", C.c_int32),
        ("matrix", C.c_void_p), ("ld", C.c_int32),
        ("path_text", C.c_void_p), ("path_time", C.c_void_p),
        ("path_len", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


_lib: Optional[C.CDLL] = None


def load_library(path: str = LIB_PATH) -> C.CDLL:
    """Load the HIP library, declare prototypes.  Raises WmError when it is absent: the product
    path has no CPU or PyTorch fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise WmError(f"{path} not found: build it with `python __graft_entry__.py` "
                      f"(hipcc --offload-arch=gfx950); there is no fallback path")
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise WmError(f"{path} does not export {name}")
    vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
    lib.wm_version.restype = i32
    if lib.wm_version() != ABI_VERSION:       # a stale .so: signatures moved (wm_gemm's workspace), arguments would be misread
        raise WmError(f"{path} has ABI version {lib.wm_version()}, this binding needs {ABI_VERSION}: rebuild it "
                      f"(python __graft_entry__.py)")
    lib.wm_last_error.restype = C.c_char_p
    lib.wm_device_count.argtypes = [C.POINTER(i32)]
    lib.wm_engine_create.argtypes = [vp, sz, i32, C.POINTER(vp)]
    lib.wm_engine_destroy.argtypes = [vp]
    lib.wm_engine_destroy.restype = None
    lib.wm_engine_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(WmDims)]
    lib.wm_engine_weight_bytes.argtypes = [vp]
    lib.wm_engine_weight_bytes.restype = sz
    lib.wm_encoder_workspace_bytes.argtypes = [vp, i32]
    lib.wm_encoder_workspace_bytes.restype = sz
    lib.wm_encoder_forward.argtypes = [vp, vp, i32, vp, vp, sz, vp]
    lib.wm_encoder_forward_shared.argtypes = [vp, vp, i32, vp, vp, sz, i32, vp]
    lib.wm_encoder_forward_range.argtypes = [vp, vp, i32, vp, vp, sz, i32, i32, i32, vp]
    lib.wm_cross_kv_workspace_bytes.argtypes = [vp, i32]
    lib.wm_cross_kv_workspace_bytes.restype = sz
    lib.wm_cross_kv.argtypes = [vp, vp, i32, C.POINTER(vp), vp, sz, vp]
    lib.wm_decoder_workspace_bytes.argtypes = [vp, i32, i32]
    lib.wm_decoder_workspace_bytes.restype = sz
    lib.wm_decoder_step.argtypes = [vp, C.POINTER(WmDecoderIO), vp]
    lib.wm_decoder_step_group.argtypes = [vp, C.POINTER(WmDecoderGroupIO), vp]
    lib.wm_decoder_prefill_workspace_bytes.restype = C.c_size_t
    lib.wm_decoder_prefill_workspace_bytes.argtypes = [vp, i32, i32]
    lib.wm_decoder_prefill.argtypes = [vp, C.POINTER(WmPrefillIO), vp]
    lib.wm_attn_prefill_self.argtypes = [vp, i32, i32, i32, vp, i32, i32, C.c_float, vp, vp, vp, vp]
    lib.wm_attn_prefill_cross.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.wm_greedy_step.argtypes = [C.POINTER(WmGreedyIO), vp]
    lib.wm_gemm.argtypes = [vp, i32, i32, i32, vp, i32, i32, vp, vp, vp, i32, i32, vp, i32, vp, sz, vp]
    lib.wm_conv1d_gelu.argtypes = [vp, i32, i32, i32, vp, i32, vp, i32, i32, i32, vp, vp]
    lib.wm_argmax.argtypes = [vp, C.c_int64, i32, i32, vp, vp]
    lib.wm_gemv_fused.argtypes = [C.POINTER(WmGemvIO), vp]
    lib.wm_set_small_batch_rows.argtypes = [i32]
    lib.wm_gemm_rows.argtypes = [C.POINTER(WmGemvIO), vp]
    lib.wm_set_rows_path.argtypes = [i32]
    lib.wm_set_self_attn_waves.argtypes = [i32]
    lib.wm_set_gemm_small_tiles.argtypes = [i32]
    lib.wm_lab_knobs.argtypes = [C.c_char_p, sz]
    lib.wm_set_cross_v_skip.argtypes = [i32]
    lib.wm_set_decode_chain.argtypes = [i32]
    lib.wm_decode_chain_error.argtypes = [C.POINTER(C.c_int)]
    lib.wm_decode_chain_status.argtypes = [C.POINTER(WmChainStatus)]
    lib.wm_debug_occupy.argtypes = [i32, sz, C.c_int64, vp]
    lib.wm_gemm_skinny.argtypes = [vp, i32, i32, i32, vp, i32, i32, vp, i32, vp, vp]
    lib.wm_gemm_skinny_default_ksplit.argtypes = [i32, i32, i32, i32]
    lib.wm_layernorm.argtypes = [vp, i32, i32, i32, vp, vp, vp, i32, vp]
    lib.wm_attn_encoder.argtypes = [vp, i32, i32, i32, i32, vp, i32, vp]
    lib.wm_attn_decode_cross.argtypes = [vp, i32, i32, i32, i32, vp, vp, i32, vp, vp]
    lib.wm_attn_decode_self.argtypes = [vp, i32, i32, i32, i32, vp, i32, vp, i32, i32, C.c_float, vp, vp]
    lib.wm_attn_decode_self_rows.argtypes = [vp, i32, i32, i32, i32, vp, i32, i32, C.c_float, vp, vp, vp, vp]
    lib.wm_quantize_i8.argtypes = [vp, vp, C.c_int64, C.c_float, vp]
    lib.wm_log_mel_workspace_bytes.argtypes = [i32, i32, i32]
    lib.wm_log_mel_workspace_bytes.restype = sz
    lib.wm_log_mel.argtypes = [vp, i32, i32, C.c_int64, vp, i32, vp, vp, vp, sz, vp]
    lib.wm_decoder_step_multi.argtypes = [vp, i32, C.POINTER(C.POINTER(WmDecoderIO)), C.POINTER(vp), vp]
    lib.wm_stream_create_cu_mask.argtypes = [C.POINTER(C.c_uint32), i32, C.POINTER(vp)]
    lib.wm_stream_destroy.argtypes = [vp]
    lib.wm_attn_decode_cross_i8.argtypes = [vp, i32, i32, i32, i32, vp, C.c_float, vp, i32, vp, vp]
    lib.wm_flac_info.argtypes = [vp, sz, C.POINTER(WmFlacStreamInfo)]
    lib.wm_flac_decode.argtypes = [vp, sz, vp, C.c_int64, C.POINTER(C.c_int64)]
    lib.wm_repeat_controls.argtypes = [C.POINTER(WmRepeatIO), vp]
    lib.wm_sequence_bias.argtypes = [C.POINTER(WmBiasIO), vp]
    lib.wm_sample_step.argtypes = [C.POINTER(WmSampleIO), vp]
    lib.wm_verify_workspace_bytes.argtypes = [i32, i32]
    lib.wm_verify_workspace_bytes.restype = sz
    lib.wm_verify_step.argtypes = [C.POINTER(WmVerifyIO), vp]
    lib.wm_step_advance.argtypes = [vp, vp]
    lib.wm_step_finish.argtypes = [vp, vp, i32, vp, vp]
    lib.wm_beam_workspace_bytes.argtypes = [i32, i32]
    lib.wm_beam_workspace_bytes.restype = sz
    lib.wm_beam_step.argtypes = [C.POINTER(WmBeamIO), vp]
    lib.wm_kv_reorder.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp]
    lib.wm_debug_timeline.argtypes = [vp, i32]
    lib.wm_gemm_ex.argtypes = [C.POINTER(WmGemmIO), vp]
    lib.wm_row_finish.argtypes = [C.POINTER(WmRowFinishIO), vp]
    lib.wm_attn_self_ex.argtypes = [C.POINTER(WmAttnSelfIO), vp]
    lib.wm_attn_cross_ex.argtypes = [C.POINTER(WmAttnCrossIO), vp]
    lib.wm_attn_cross_group_ex.argtypes = [C.POINTER(WmAttnCrossGroupIO), vp]
    lib.wm_attn_encoder_ex.argtypes = [C.POINTER(WmAttnEncoderIO), vp]
    lib.wm_step_finish_group.argtypes = [vp, vp, i32, i32, vp, vp, vp]
    lib.wm_embed.argtypes = [vp, i32, i32, i32, vp, i32, vp, vp, i32, i32, vp, vp, vp]
    lib.wm_mel_transpose_pad.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.wm_zero_pad_rows.argtypes = [vp, i32, i32, i32, vp]
    lib.wm_mel_windows.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    lib.wm_resample.argtypes = [vp, i32, i32, C.c_int64, C.c_float, vp, i32, i32, i32, vp, C.c_int64, vp]
    lib.wm_resample_channels.argtypes = [vp, i32, i32, C.c_int64, C.c_float, vp, i32, i32, i32, vp, C.c_int64, C.c_int64, vp]
    lib.wm_channel_top_workspace_bytes.argtypes = [i32, C.c_int64]
    lib.wm_channel_top_workspace_bytes.restype = sz
    lib.wm_channel_top.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, sz, C.c_int64, vp]
    lib.wm_forced_probs.argtypes = [vp, i32, i32, i32, C.c_int64, C.c_int64, i32, vp, i32, vp, i32, vp]
    lib.wm_section_cuts_workspace_bytes.argtypes = [i32, C.c_int64]
    lib.wm_section_cuts_workspace_bytes.restype = sz
    lib.wm_section_cuts.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, vp, vp, sz, C.c_int64, vp]
    lib.wm_speech_spans_workspace_bytes.argtypes = [i32, C.c_int64]
    lib.wm_speech_spans_workspace_bytes.restype = sz
    lib.wm_speech_spans.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, vp, vp, sz, C.c_int64, vp]
    lib.wm_mel_gather.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]
    lib.wm_decoder_step_tap.argtypes = [vp, C.POINTER(WmDecoderIO), C.POINTER(WmTapIO), vp]
    lib.wm_align_workspace_bytes.argtypes = [i32, i32, i32, i32]
    lib.wm_align_workspace_bytes.restype = sz
    lib.wm_align.argtypes = [C.POINTER(WmAlignIO), vp]
    lib.wm_dtw_workspace_bytes.argtypes = [i32, i32, i32]
    lib.wm_dtw_workspace_bytes.restype = sz
    lib.wm_dtw.argtypes = [vp, i32, C.c_int64, i32, vp, vp, i32, i32, vp, vp, i32, vp, vp, sz, vp]
    lib.wm_dtw_open.argtypes = [vp, i32, C.c_int64, i32, vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, sz, vp]
    lib.wm_align_open.argtypes = [C.POINTER(WmAlignIO), vp, vp]
    lib.wm_decoder_prefill_tap.argtypes = [vp, C.POINTER(WmPrefillIO), C.POINTER(WmTapIO), vp]
    lib.wm_profile_configure.argtypes = [i32, i32, i32]
    lib.wm_profile_read.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_int64), i32]
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load_library().wm_last_error().decode(errors="replace")
        raise WmError(f"{what or 'libwhisper_mi355'} failed (rc={rc}): {msg}")


def _ptr(t):
    return None if t is None else (t.data_ptr() if hasattr(t, "data_ptr") else int(t))


def align_io(engine, n_text_head: int, n_audio_ctx: int, tape, cross: Sequence, heads, n_tokens, n_frames, n_prefix: int,
             filter_width: int, cap_tokens: int, matrix, ld: int, path_text, path_time, path_len, workspace) -> WmAlignIO:
    """The wm_align_io of one wm_align / wm_align_open call.  `engine`: the decoder's handle, or None (the dims are then taken on trust);
    tape fp16 [batch, len(heads), capacity, 64]; cross: per layer fp16 [batch, 2, n_text_head, n_audio_ctx, 64]; heads: a ctypes int32
    array or a list; matrix: fp32 rows of `ld` elements, or None.  The struct keeps its pointer arrays alive (`io._keep`)."""
    if not isinstance(heads, C.Array):
        heads = (C.c_int32 * len(heads))(*heads)
    cross_arr = ptr_array(cross)
    io = WmAlignIO()
    io.engine = engine
    io.batch, io.n_text_head, io.n_audio_ctx = tape.shape[0], n_text_head, n_audio_ctx
    io.q_tape, io.capacity = tape.data_ptr(), tape.shape[2]
    io.cross, io.n_layers = C.cast(cross_arr, C.POINTER(C.c_void_p)), len(cross)
    io.heads, io.n_heads = C.cast(heads, C.POINTER(C.c_int32)), len(heads)
    io.n_tokens, io.n_frames = _ptr(n_tokens), _ptr(n_frames)
    io.n_prefix, io.filter_width, io.cap_tokens = n_prefix, filter_width, cap_tokens
    io.matrix, io.ld = (_ptr(matrix), ld) if matrix is not None else (None, 0)
    io.path_text, io.path_time, io.path_len = _ptr(path_text), _ptr(path_time), _ptr(path_len)
    io.workspace, io.workspace_bytes = workspace.data_ptr(), workspace.numel()
    io._keep = (cross_arr, heads)
    return io


def ptr_array(tensors: Sequence) -> "C.Array":
    """Device pointers of a list of torch tensors (or ints / None) as a void*[]."""
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = _ptr(t)
    return arr


class Engine:
    """Owns one wm_engine (device-resident weights of one *.engine file)."""

    def __init__(self, blob: bytes, device: int = 0):
        self.lib = load_library()
        handle = C.c_void_p()
        if not isinstance(blob, bytes):
            blob = bytes(blob)
        # c_char_p points at the bytes object's own buffer: no host copy of a multi-GB blob
        check(self.lib.wm_engine_create(C.cast(C.c_char_p(blob), C.c_void_p), len(blob), device, C.byref(handle)),
              "wm_engine_create")
        self.handle = handle
        kind, flags, dims = C.c_int32(), C.c_uint32(), WmDims()
        check(self.lib.wm_engine_info(self.handle, C.byref(kind), C.byref(flags), C.byref(dims)))
        self.kind, self.flags, self.dims, self.device = kind.value, flags.value, dims.to_dict(), device

    @property
    def weight_bytes(self) -> int:
        return int(self.lib.wm_engine_weight_bytes(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.wm_engine_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_MASKED_STREAMS = {}


def _destroy_masked_streams():
    """Interpreter exit: give the dedicated hardware queues back before the HIP runtime (and any profiler
    attached to it) tears down -- a process that exits with CU-masked queues alive crashes in rocprofv3's finaliser."""
    if not _MASKED_STREAMS or _lib is None:
        return
    try:
        import torch
        torch.cuda.synchronize()
    except Exception:      # noqa: BLE001 -- nothing useful to do at exit
        pass
    for st in _MASKED_STREAMS.values():
        _lib.wm_stream_destroy(st.cuda_stream)
    _MASKED_STREAMS.clear()


atexit.register(_destroy_masked_streams)


def create_masked_stream(cu_enabled, index: int = 0):
    """A torch stream whose kernels run only on the CUs with a true entry in `cu_enabled` (CU i = entry i):
    wm_stream_create_cu_mask wrapped as torch.cuda.ExternalStream (so wait_stream / synchronize work).
    Streams are cached per (device, mask, index) for the life of the process: hardware queues are a scarce
    resource (ROCm multiplexes streams onto GPU_MAX_HW_QUEUES of them), so callers share, never re-create."""
    import torch
    key = (torch.cuda.current_device(), tuple(bool(b) for b in cu_enabled), index)
    if key not in _MASKED_STREAMS:
        n_words = (len(cu_enabled) + 31) // 32
        words = (C.c_uint32 * n_words)()
        for i, on in enumerate(cu_enabled):
            if on:
                words[i // 32] |= 1 << (i % 32)
        handle = C.c_void_p()
        check(load_library().wm_stream_create_cu_mask(words, n_words, C.byref(handle)), "wm_stream_create_cu_mask")
        _MASKED_STREAMS[key] = torch.cuda.ExternalStream(handle.value)
    return _MASKED_STREAMS[key]
