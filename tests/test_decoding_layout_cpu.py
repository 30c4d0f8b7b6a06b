"""Where the decoding code lives (no GPU, no engine): decoding.py assembles `WhisperDecoding` from the literal loops of host_decoding.py,
the device loop of device_loop.py and the word alignment of word_align.py and re-exports their public names.  The lists below are written out: the names imported from
`decoding` anywhere in the repository before the split, and what `dir(WhisperDecoding)` held then."""
import ast
import os
import types

import decoding
import device_loop
import host_decoding
import word_align
from decoding import WhisperDecoding

# every name that tests/, scripts/, bench.py, oracle/, __graft_entry__.py or the package imports from `decoding`
# (`import decoding as D` included: the attributes tests/test_host_cpu.py reads off the module)
IMPORTED = ["ApplyTimestampRules", "BeamSearchDecoder", "DecodingOptions", "GreedyDecoder", "MaximumLikelihoodRanker", "NoRepeatNGram",
            "ROW_PAD_TOKEN", "RepetitionPenalty", "SuppressBlank", "SuppressTokens", "WhisperDecoding", "call_key", "candidate_mode",
            "check_candidate_options", "check_decoding_options", "groups_run_alone", "language_key", "partition_key", "prefill_key",
            "right_aligned_rows", "row_prompt_layout", "step_key", "steps_side_by_side"]
# ... and the other public names the module had
PUBLIC = ["BEAM_MAX", "BEAM_POOL_MAX", "CHUNK_LENGTH", "DecodingResult", "LogitFilter", "fork", "join"]

# dir(WhisperDecoding) before the split, without what every class has.  Two names left on purpose: `_live_list` and `_live_groups` were
# one-line wrappers of `_all_live`, which their two callers (device_loop._Group) now call with the key written out.
CLASS_ATTRIBUTES = [
    "_align_frames", "_all_live", "_beam", "_call_decoder", "_candidate_rows", "_capture", "_chain_gave_up", "_chain_warned",
    "_check_device_call", "_check_partition", "_cross_group", "_cross_persistent", "_detect_language_rows", "_fast_state", "_features_key",
    "_fill_rules", "_finish_beam_loop", "_finish_main_loop", "_forced_tokens", "_get_initial_tokens", "_get_suppress_tokens", "_greedy",
    "_group_streams", "_groups", "_host_call", "_host_step", "_initial_token_rows", "_instances", "_issue_step", "_language_from_logits",
    "_main_loop", "_main_loop_partitioned", "_may_run_alone", "_partition_streams", "_refuse_row_prompts", "_repeat_controls",
    "_replay_or_issue", "_require_device_loop", "_reset_state", "_result_tokens", "_run_groups", "_split_words", "alignment_heads",
    "balanced_order", "compression_ratio", "decode", "detect_language", "detect_language_reference", "get_config", "get_session",
    "get_tokenizer", "main_loop", "main_loop_reference", "post_process", "set_language_tokens", "set_prompts",
    "state_bytes_per_utterance", "torch_detect_language", "torch_main_loop", "torch_word_timestamps", "word_timestamps",
    "xa2cross_key_value"]

WORD_ALIGN_MIXIN = ["word_timestamps", "block_pass_rows", "BLOCK_LOGIT_BYTES", "_forced_pass", "_forced_pass_block", "_align",
                    "_words_from_paths"]

HOST_MIXIN = ["xa2cross_key_value", "_features_key", "decode", "_language_from_logits", "detect_language_reference", "torch_detect_language",
              "_host_call", "_host_step", "main_loop_reference", "torch_main_loop", "torch_word_timestamps"]


def _imported_modules(module):
    with open(module.__file__) as f:
        tree = ast.parse(f.read())
    found = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            found |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom) and node.module:
            found.add(node.module.split(".")[0])
    return found


def test_decoding_re_exports_every_name():
    missing = [n for n in IMPORTED + PUBLIC if not hasattr(decoding, n)]
    assert not missing, missing
    # the same objects, not copies: a class patched through one module is patched for the other
    for name in IMPORTED + PUBLIC:
        for module in (host_decoding, device_loop):
            if hasattr(module, name):
                assert getattr(decoding, name) is getattr(module, name), name


def test_the_class_keeps_its_names():
    missing = [n for n in CLASS_ATTRIBUTES if n not in dir(WhisperDecoding)]
    assert not missing, missing
    assert decoding.WhisperDecoding.__module__ == "decoding"
    assert all(n in vars(host_decoding.HostLoops) for n in HOST_MIXIN)
    assert all(n in vars(device_loop.DeviceLoop) for n in ("_fast_state", "_finish_beam_loop", "detect_language",
                                                           "_main_loop_partitioned", "_check_partition", "_chain_gave_up"))
    assert all(n in vars(word_align.WordAlign) for n in WORD_ALIGN_MIXIN)
    assert not any(n in vars(device_loop.DeviceLoop) or hasattr(device_loop, n) for n in WORD_ALIGN_MIXIN)
    assert WhisperDecoding.__mro__[1:4] == (host_decoding.HostLoops, device_loop.DeviceLoop, word_align.WordAlign)


def test_word_align_stands_beside_the_loops():
    assert not {"decoding", "device_loop"} & _imported_modules(word_align)
    assert "decoding" not in vars(word_align) and "device_loop" not in vars(word_align)
    assert os.path.dirname(word_align.__file__) == os.path.dirname(decoding.__file__)


def test_one_construction_of_the_align_io():
    """native.align_io fills the wm_align_io for every caller: forced alignment and the two GPU test files have no construction of
    their own, and the package has one."""
    here, pkg = os.path.dirname(os.path.abspath(__file__)), os.path.dirname(decoding.__file__)
    paths = [os.path.join(here, "test_gpu_word_timestamps.py"), os.path.join(here, "test_gpu_dtw_open.py")]
    paths += [os.path.join(pkg, f) for f in sorted(os.listdir(pkg)) if f.endswith(".py")]
    found = []
    for path in paths:
        with open(path) as f:
            tree = ast.parse(f.read())
        for node in ast.walk(tree):
            callee = node.func if isinstance(node, ast.Call) else None
            if getattr(callee, "attr", None) == "WmAlignIO" or getattr(callee, "id", None) == "WmAlignIO":
                found.append(os.path.basename(path))
    assert found == ["native.py"], found


def test_the_literal_loops_need_no_library():
    assert "native" not in vars(host_decoding) and "ctypes" not in vars(host_decoding) and "C" not in vars(host_decoding)
    assert not {"native", "ctypes"} & _imported_modules(host_decoding)
    assert "decoding" not in _imported_modules(host_decoding) and "decoding" not in _imported_modules(device_loop)
    assert "decoding" not in vars(host_decoding) and "decoding" not in vars(device_loop)
    assert os.path.dirname(host_decoding.__file__) == os.path.dirname(decoding.__file__) == os.path.dirname(device_loop.__file__)


def test_the_process_wide_words_live_in_the_class_body():
    for name in ("_chain_warned", "_instances"):
        assert name in WhisperDecoding.__dict__, name
        assert not any(name in vars(base) for base in WhisperDecoding.__mro__[1:]), name
    assert not any(hasattr(m, n) for m in (host_decoding, device_loop) for n in ("_chain_warned", "_instances"))


def test_the_give_up_warning_is_booked_on_the_class(monkeypatch):
    """`_chain_gave_up` (device_loop.py) reads and writes WhisperDecoding._chain_warned itself -- also through a subclass, whose own
    __dict__ must stay without a copy: tests re-arm the warning by assigning the class attribute.  (A stand-in library whose give-up
    word is set.)"""
    class Lib:
        def wm_decode_chain_error(self, ref):
            ref._obj.value = 1
            return 0

    class Sub(WhisperDecoding):
        pass

    monkeypatch.setattr(device_loop, "native", types.SimpleNamespace(load_library=Lib, check=lambda rc, what: None))
    monkeypatch.setattr(WhisperDecoding, "_chain_warned", False)
    dec = object.__new__(Sub)
    dec._state = {1: {"graphs": {"key": "graph"}}}
    WhisperDecoding._instances.add(dec)
    assert dec._chain_gave_up("layout test") is True
    assert WhisperDecoding.__dict__["_chain_warned"] is True and "_chain_warned" not in vars(Sub)
    assert dec._state[1]["graphs"] == {}                                  # every instance's graphs are dropped
