"""Word-level timestamps, host side (no GPU): timing.py's statement of the alignment contract (DESIGN.md "word timestamps"),
the tokenizer's word splitting, the PyTorch path's score capture and `WhisperDecoding.torch_word_timestamps`, and the new
C-ABI entries' declarations and struct layouts."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import build as B
import native
import synthetic
import timing
import torch_model as TM
from decoding import DecodingOptions, WhisperDecoding
from encoding import WhisperEncoding
from oracle.whisper_oracle import Dims, synthetic_mel, synthetic_state_dict
from tokenizer import Tokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, "eddie-wang-hackathon2023_amd", "assets", "multilingual.tiktoken")


# ---- DTW --------------------------------------------------------------------------------------------------------------
def dtw_loops(x):
    """Step 8 of the contract, cell by cell."""
    x = np.asarray(x, dtype=np.float32)
    N, M = x.shape
    inf = np.float32(np.inf)
    cost = [[inf] * (M + 1) for _ in range(N + 1)]
    trace = [[-1] * (M + 1) for _ in range(N + 1)]
    cost[0][0] = np.float32(0)
    for j in range(1, M + 1):
        for i in range(1, N + 1):
            c0, c1, c2 = cost[i - 1][j - 1], cost[i - 1][j], cost[i][j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cost[i][j] = np.float32(x[i - 1, j - 1] + c)
            trace[i][j] = t
    for j in range(M + 1):
        trace[0][j] = 2
    for i in range(N + 1):
        trace[i][0] = 1
    i, j, path = N, M, []
    while i > 0 or j > 0:
        path.append((i - 1, j - 1))
        t = trace[i][j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    path.reverse()
    return np.array([p[0] for p in path]), np.array([p[1] for p in path])


def monotone_paths(N, M):
    """Every path from (0, 0) to (N - 1, M - 1) by steps (1, 1), (1, 0), (0, 1)."""
    def walk(i, j):
        if (i, j) == (N - 1, M - 1):
            yield [(i, j)]
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < N and j + dj < M:
                for rest in walk(i + di, j + dj):
                    yield [(i, j)] + rest
    return walk(0, 0)


def test_dtw_cpu_finds_the_cheapest_monotone_path():
    rng = np.random.default_rng(0)
    for N, M in itertools.product(range(1, 5), range(1, 5)):
        for _ in range(4):
            x = rng.standard_normal((N, M)).astype(np.float32)
            ti, fi = timing.dtw_cpu(x)
            assert (ti[0], fi[0]) == (0, 0) and (ti[-1], fi[-1]) == (N - 1, M - 1)
            steps = set(zip(np.diff(ti).tolist(), np.diff(fi).tolist()))
            assert steps <= {(1, 1), (1, 0), (0, 1)}
            got = float(x[ti, fi].astype(np.float64).sum())
            best = min(sum(float(x[i, j]) for i, j in path) for path in monotone_paths(N, M))
            assert abs(got - best) <= 1e-5 * max(1.0, abs(best)), (N, M)


def test_dtw_cpu_breaks_ties_as_the_loops_do():
    rng = np.random.default_rng(1)
    for N, M in [(1, 1), (1, 6), (5, 1), (3, 3), (4, 9), (9, 4), (12, 30), (33, 20)]:
        for _ in range(3):
            x = rng.integers(-2, 3, size=(N, M)).astype(np.float32)
            ti, fi = timing.dtw_cpu(x)
            ri, rf = dtw_loops(x)
            assert ti.tolist() == ri.tolist() and fi.tolist() == rf.tolist(), (N, M)
    x = rng.standard_normal((7, 40)).astype(np.float32)
    assert [a.tolist() for a in timing.dtw_cpu(x)] == [a.tolist() for a in dtw_loops(x)]


# ---- median filter, alignment matrix ------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 3, 4, 7, 8, 40])
def test_median_filter_equals_the_sorted_window(F):
    g = torch.Generator().manual_seed(F)
    x = torch.randn(2, 5, F, generator=g)
    got = timing.median_filter(x, 7)
    if F <= 3:
        assert got is x or torch.equal(got, x)              # the padding would not fit: no filtering
        return
    want = torch.empty_like(x)
    for f in range(F):
        idx = []
        for k in range(f - 3, f + 4):
            idx.append(-k if k < 0 else (2 * (F - 1) - k if k >= F else k))
        want[..., f] = torch.sort(x[..., idx], dim=-1).values[..., 3]
    assert torch.equal(got, want)


def test_alignment_matrix_steps_and_the_zero_spread_rule():
    g = torch.Generator().manual_seed(3)
    S = [torch.randn(9, 20, generator=g) * 4 for _ in range(3)]
    S[1][:, 5] = -1e4                                     # a frame nobody attends to: W == 0 on every row, std == 0
    got = timing.alignment_matrix(S, 3)
    assert got.shape == (9 - 3 - 1, 20) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    tot = torch.zeros(9, 20, dtype=torch.float64)
    for s in S:
        w = s.double().softmax(-1)
        m, sd = w.mean(0, keepdim=True), w.std(0, unbiased=False, keepdim=True)
        z = torch.where(sd > 0, (w - m) / sd, torch.zeros_like(w))
        tot += timing.median_filter(z, 7)
    want = (tot / 3)[3:8]
    assert float((got.double() - want).abs().max()) < 1e-4


# ---- words --------------------------------------------------------------------------------------------------------------
def W(word, tokens=(0,), start=0.0, end=0.0):
    return timing.WordTiming(word, list(tokens), start, end, 1.0)


def test_merge_punctuations():
    a = [W(" Hello", [1]), W(",", [2]), W(" (", [3]), W("world", [4]), W(")", [5]), W("!", [6]), W(" \"", [7]), W(" ok", [8])]
    timing.merge_punctuations(a)
    assert [(w.word, w.tokens) for w in a if w.word] == [(" Hello,", [1, 2]), (" (world)!", [3, 4, 5, 6]), (" \" ok", [7, 8])]
    assert [w.word for w in a if not w.word] == ["", "", "", "", ""] and all(w.tokens == [] for w in a if not w.word)


@pytest.fixture(scope="module")
def tok():
    return Tokenizer.from_vocab(VOCAB, True, "en", "transcribe")


def test_split_to_word_tokens_english_multibyte_and_no_spaces(tok):
    text = " Hello, world! It's naïve."
    ids = tok.encode(text)
    words, word_tokens = tok.split_to_word_tokens(ids + [tok.eot])
    assert [t for ts in word_tokens for t in ts] == ids + [tok.eot]
    assert "".join(words[:-1]) == text and words[-1] == "<|endoftext|>"
    assert words[:4] == [" Hello", ",", " world", "!"] and " naïve" in words and words[-2] == "."
    # a multi-byte character that spans tokens stays in one word: the emoji is 4 bytes over several byte-level tokens
    ids = tok.encode(" ok 🫠 fine")
    pieces, piece_tokens = tok.split_tokens_on_unicode(ids)
    assert "".join(pieces) == " ok 🫠 fine" and all("�" not in p for p in pieces)
    assert any(len(ts) > 1 for ts in piece_tokens)
    words, word_tokens = tok.split_to_word_tokens(ids)
    assert words == [" ok", " 🫠", " fine"]
    # a language written without spaces: cut at characters, not at spaces
    ja = Tokenizer.from_vocab(VOCAB, True, "ja", "transcribe")
    ids = ja.encode("こんにちは世界")
    words, word_tokens = ja.split_to_word_tokens(ids)
    assert "".join(words) == "こんにちは世界" and len(words) > 1 and all("�" not in w for w in words)
    assert [t for ts in word_tokens for t in ts] == ids
    assert words == ja.split_tokens_on_unicode(ids)[0]
    assert tok.split_to_word_tokens(ids, language="ja")[0] == words              # the utterance's language overrides the tokenizer's
    assert tok.split_to_word_tokens(ids)[0] == ["こんにちは世界"]         # the same tokens under "en": one space-less word


def test_split_to_word_tokens_without_a_vocabulary():
    t = Tokenizer.ids_only(True, "en", "transcribe")
    words, word_tokens = t.split_to_word_tokens([440, 7, 9001, t.eot])
    assert word_tokens == [[440], [7], [9001], [t.eot]] and words == ["<|440|>", "<|7|>", "<|9001|>", "<|endoftext|>"]


def test_words_from_path():
    # 3 text tokens + eot -> N = 4 rows; words: [" a"], ["b", "c"] (one word of two tokens), eot
    ti = np.array([0, 0, 1, 2, 2, 2, 3])
    fi = np.array([0, 1, 2, 3, 4, 5, 6])
    out = timing.words_from_path(ti, fi, [" a", " bc", "<|endoftext|>"], [[10], [11, 12], [99]], [0.5, 0.25, 0.75], 0.02)
    assert [(w.word, w.tokens) for w in out] == [(" a", [10]), (" bc", [11, 12])]
    assert [w.start for w in out] == pytest.approx([0.0, 0.04]) and [w.end for w in out] == pytest.approx([0.04, 0.12])
    assert [w.probability for w in out] == pytest.approx([0.5, 0.5])
    assert timing.words_from_path(ti[:1], fi[:1], ["<|endoftext|>"], [[99]], [], 0.02) == []


# ---- the PyTorch statement ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_setup(tmp_path_factory):
    """The `micro` family's model with the full vocabulary (the tokenizer's ids need it), on CPU."""
    dims = Dims(**synthetic.DIMS["micro-fullvocab"])
    sd = synthetic_state_dict(dims, 5)
    out = tmp_path_factory.mktemp("timing_eng") / "eng"
    args = B.parse_arguments(["--output_dir", str(out), "--use_gpt_attention_plugin", "--use_gemm_plugin", "--use_layernorm_plugin",
                              "--log_level", "error"])
    B.build_from_checkpoint({"dims": dims.to_dict(), "model_state_dict": sd}, args)
    model = TM.Whisper(TM.ModelDimensions(**dims.to_dict())).load_state_dict({k: v.float() for k, v in sd.items()})
    mel = synthetic_mel(2, 2 * dims.n_audio_ctx, dims.n_mels, 77).float()
    enc = WhisperEncoding(out, only_torch=True)
    dec = WhisperDecoding(out, only_torch=True, options=DecodingOptions(sample_len=10))
    xa = enc.torch_get_audio_features(model, mel)
    return dims, model, dec, xa


def test_torch_word_timestamps_structure_and_repeatability(torch_setup):
    dims, model, dec, xa = torch_setup
    tk = dec.tokenizer
    text = tk.encode(" Hello, world! This is (a) test.")
    sampled = [[tk.timestamp_begin] + text + [tk.timestamp_begin + 40], text[:5]]
    frames = [2 * dims.n_audio_ctx, 2 * 41 + 1]
    got = dec.torch_word_timestamps(model, xa, sampled, frames)
    again = dec.torch_word_timestamps(model, xa, sampled, frames)
    assert got == again
    for b, words in enumerate(got):
        t = sampled[b] if b else text
        expect_words, expect_tokens = tk.split_to_word_tokens([x for x in t if x < tk.eot] + [tk.eot])
        merged = [timing.WordTiming(w, list(ts), 0, 0, 0) for w, ts in zip(expect_words[:-1], expect_tokens[:-1])]
        timing.merge_punctuations(merged)
        assert [(w.word, w.tokens) for w in words] == [(w.word, w.tokens) for w in merged if w.word]      # one timing per word
        F = frames[b] // 2
        starts = [w.start for w in words]
        # (a frame is CHUNK_LENGTH / n_audio_ctx seconds: the 0.02 s of the real models' 1500 frames, 30 / 64 s on this toy)
        assert all(0 <= w.start <= w.end <= F * (30.0 / dims.n_audio_ctx) + 1e-9 for w in words), words
        assert starts == sorted(starts) and all(0.0 <= w.probability <= 1.0 for w in words)
    assert dec.torch_word_timestamps(model, xa, [[tk.timestamp_begin], text], None)[0] == []           # no text tokens: no words
    # the default decode path is unchanged by the capture argument
    x = torch.tensor([list(tk.sot_sequence) + text[:3]])
    scores = []
    assert torch.equal(model.decoder(x, xa[:1]), model.decoder(x, xa[:1], cross_scores=scores)) and len(scores) == dims.n_text_layer


def test_captured_scores_are_q16_dot_k16(torch_setup):
    dims, model, dec, xa = torch_setup
    tk = dec.tokenizer
    x = torch.tensor([list(tk.sot_sequence) + [tk.no_timestamps, 440, 7, 9001, tk.eot]])
    seen = {}
    linear = model._linear

    def spy(name, inp):
        out = linear(name, inp)
        if name.endswith("cross_attn.query") or name.endswith("cross_attn.key"):
            seen[name] = out
        return out
    model._linear = spy
    try:
        scores = []
        model.decoder(x, xa[:1], cross_scores=scores)
    finally:
        del model._linear
    s = np.float32(64 ** -0.25)
    for layer in range(dims.n_text_layer):
        q = seen[f"decoder.blocks.{layer}.cross_attn.query"][0].numpy()
        k = seen[f"decoder.blocks.{layer}.cross_attn.key"][0].numpy()
        q16 = (q.astype(np.float16).astype(np.float32) * s).astype(np.float16).astype(np.float64)
        k16 = (k.astype(np.float16).astype(np.float32) * s).astype(np.float16).astype(np.float64)
        for h in range(dims.n_text_head):
            want = q16[:, 64 * h: 64 * h + 64] @ k16[:, 64 * h: 64 * h + 64].T
            got = scores[layer][0, h].numpy()
            assert got.dtype == np.float32 and np.abs(got - want).max() <= 2e-6 * max(1.0, np.abs(want).max())      # fp32 summation order only


def test_alignment_heads_default_and_explicit(tmp_path):
    assert timing.default_alignment_heads(4, 3) == [6, 7, 8, 9, 10, 11]
    assert timing.parse_alignment_heads("3:1,2:0", 4, 3) == [6, 10] and timing.parse_alignment_heads([[1, 2]], 4, 3) == [5]
    with pytest.raises(ValueError):
        timing.parse_alignment_heads("4:0", 4, 3)
    dims = Dims(**synthetic.DIMS["micro"])
    args = B.parse_arguments(["--output_dir", str(tmp_path / "eng"), "--alignment_heads", "1:1,0:1", "--log_level", "error"])
    B.build_from_checkpoint(synthetic.synthetic_checkpoint("micro", 7), args)
    dec = WhisperDecoding(tmp_path / "eng", only_torch=True)
    assert dec.decoder_config["alignment_heads"] == [[0, 1], [1, 1]] and dec.alignment_heads() == [1, 3]
    assert dims.n_text_layer == 2


# ---- ABI ------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("wm_decoder_step_tap", "wm_align_workspace_bytes", "wm_align", "wm_dtw_workspace_bytes", "wm_dtw")


def test_new_entries_are_declared_and_listed():
    header = open(os.path.join(ROOT, "include", "whisper_mi355.h")).read()
    assert "#define WM_ABI_VERSION 8" in header and native.ABI_VERSION == 8
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in native.EXPORTS, name


def test_new_entries_are_exported_by_the_library():
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not installed")
    lib = native.load_library()          # (built by the session start; a missing library is a failure here)
    assert lib.wm_version() == 8
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.wm_align_workspace_bytes(2, 3, 16, 100) > 0 and lib.wm_dtw_workspace_bytes(1, 7, 40) >= 8 * 41


def test_new_struct_layouts_match_header(tmp_path):
    """ctypes mirrors of the new structs vs the C compiler's view of include/whisper_mi355.h (plain C, gcc)."""
    structs = {"wm_tap_io": native.WmTapIO, "wm_align_io": native.WmAlignIO}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "whisper_mi355.h"', 'int main(void){']
    for s, cls in structs.items():
        src.append(f'printf("{s} %zu\\n", sizeof({s}));')
        src += [f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f, _ in cls._fields_]
    src.append('return 0;}')
    (tmp_path / "l.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "l.c"), "-o", str(tmp_path / "l")])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / "l")]).decode().splitlines())
    for s, cls in structs.items():
        assert int(got[s]) == C.sizeof(cls), s
        for f, _ in cls._fields_:
            assert int(got[f"{s}.{f}"]) == getattr(cls, f).offset, f"{s}.{f}"
