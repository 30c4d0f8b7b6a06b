"""The large-v3 generation on the host: 100 language tokens (every special behind the language block one id higher), 128 mel bins,
the `micro-v3` test model through build.py, WhisperDecoding's rules and the literal loop over the package's PyTorch model.

What the 99-language / 80-bin models do today is recorded here as literals and must not move."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import build as B
import synthetic
import tokenizer as TK
import torch_model as TM
import whisper_utils as wu
from decoding import DecodingOptions, WhisperDecoding
from encoding import WhisperEncoding
from host_decoding import SuppressTokens
from oracle.whisper_oracle import Dims, synthetic_mel, synthetic_state_dict

torch.set_num_threads(min(8, os.cpu_count() or 1))

# upstream Whisper's large-v3 vocabulary (the issue's table)
V3_IDS = {"<|translate|>": 50359, "<|transcribe|>": 50360, "<|startoflm|>": 50361, "<|startofprev|>": 50362, "<|nospeech|>": 50363,
          "<|notimestamps|>": 50364, "<|0.00|>": 50365}
# special_token_table(50257) as committed before the 100-language layout existed
V2_IDS = {"<|endoftext|>": 50257, "<|startoftranscript|>": 50258, "<|en|>": 50259, "<|su|>": 50357, "<|translate|>": 50358,
          "<|transcribe|>": 50359, "<|startoflm|>": 50360, "<|startofprev|>": 50361, "<|nospeech|>": 50362, "<|notimestamps|>": 50363,
          "<|0.00|>": 50364, "<|30.00|>": 51864}
MEL_80_SHA256 = "2150c30cbbeb6029f52002ffa666c1c72d83dbf53f463cb8462052055806e891"     # the bytes of the 80 x 201 fp32 bank, as committed


# ---------------------------------------------------------------------------------------------------------------- tokenizer
def test_v3_tokenizer_ids_are_upstreams():
    tk = TK.Tokenizer.ids_only(True, num_languages=100)
    assert tk.n_vocab == 51866 and tk.num_languages == 100
    for name, want in V3_IDS.items():
        assert tk.special_tokens[name] == want, name
    assert (tk.translate, tk.transcribe, tk.sot_lm, tk.sot_prev, tk.no_speech, tk.no_timestamps, tk.timestamp_begin) == tuple(V3_IDS.values())
    assert (tk.eot, tk.sot) == (50257, 50258) and tk.special_tokens["<|su|>"] == 50357 and tk.special_tokens["<|yue|>"] == 50358
    assert len(tk.all_language_tokens) == len(tk.all_language_codes) == 100 and tk.all_language_tokens == tuple(range(50259, 50359))
    assert tk.all_language_codes[-2:] == ("su", "yue")
    assert tk.sot_sequence == (50258, 50259, 50360) and tk.special_tokens["<|30.00|>"] == 51865
    # the same table from the vocabulary file (the ranks are the multilingual ones: no new asset)
    bundled = os.path.join(os.path.dirname(TK.__file__), "assets", "multilingual.tiktoken")
    full = TK.Tokenizer.from_vocab(bundled, True, num_languages=100)
    assert full.special_tokens == tk.special_tokens and full.n_vocab == 51866
    assert full.decode_with_timestamps([50258, 50358, 50360, 50365]) == "<|startoftranscript|><|yue|><|transcribe|><|0.00|>"


def test_99_language_tokenizer_ids_have_not_moved():
    table = TK.special_token_table(50257)
    for name, want in V2_IDS.items():
        assert table[name] == want, name
    assert len(table) + 50257 == 51865 and "<|yue|>" not in table and table == TK.special_token_table(50257, 99)
    tk = TK.Tokenizer.ids_only(True)                                            # the default stays 99
    assert tk.num_languages == 99 and tk.n_vocab == 51865 and tk.timestamp_begin == 50364 and tk.no_speech == 50362
    assert len(tk.all_language_tokens) == 99 and tk.all_language_codes[-1] == "su" and tk.sot_sequence == (50258, 50259, 50359)
    en = TK.Tokenizer.ids_only(False)
    assert en.n_vocab == 51864 and en.timestamp_begin == 50363 and en.sot_sequence == (50257,)
    with pytest.raises(ValueError):
        TK.special_token_table(50257, 101)


def test_yue_needs_a_100_language_vocabulary():
    assert TK.Tokenizer.ids_only(True, "yue", num_languages=100).sot_sequence == (50258, 50358, 50360)
    assert TK.Tokenizer.ids_only(True, "Cantonese", num_languages=100).language == "yue"
    assert TK.Tokenizer.ids_only(True, "mandarin", num_languages=100).language == "zh"
    assert TK.Tokenizer.ids_only(True, "mandarin").sot_sequence == (50258, 50260, 50359)
    for name in ("yue", "cantonese"):
        with pytest.raises(ValueError):
            TK.Tokenizer.ids_only(True, name)
        with pytest.raises(ValueError):
            TK.Tokenizer.ids_only(True, name, num_languages=99)
    with pytest.raises(ValueError):
        TK.Tokenizer(n_base=50257, language="yue", task="transcribe")           # the constructor itself refuses too
    with pytest.raises(ValueError):
        TK.Tokenizer.ids_only(True, "klingon", num_languages=100)


def test_num_languages_from_the_vocabulary_size():
    assert [TK.layout_from_vocab(v) for v in (51864, 51865, 51866)] == [(False, 99), (True, 99), (True, 100)]
    for bad in (51900, 51867, 151863):
        with pytest.raises(ValueError):
            TK.layout_from_vocab(bad)
    assert TK.layout_from_vocab(1024) == (False, 99)                            # no special fits: the `micro` test models' ids, as ever
    model = TM.Whisper(TM.ModelDimensions(**synthetic.DIMS["micro-v3"]))
    assert model.is_multilingual and model.num_languages == 100


# ---------------------------------------------------------------------------------------------------------------- mel bank
def slaney_bank_fp64(n_mels, n_fft=400, sr=16000):
    """The Slaney mel bank restated: linear below 1 kHz (200/3 Hz per mel), logarithmic above (6.4 ** (1 / 27) per mel); one triangle
    per bin between its neighbours' centres, scaled to unit area in Hz (2 / width).  Loops and scalars: nothing shared with the
    package's vectorised recipe."""
    import math

    def to_mel(f):
        return f / (200.0 / 3) if f < 1000.0 else 15.0 + math.log(f / 1000.0) * 27.0 / math.log(6.4)

    def to_hz(m):
        return m * (200.0 / 3) if m < 15.0 else 1000.0 * math.exp((m - 15.0) * math.log(6.4) / 27.0)

    top = to_mel(sr / 2.0)
    edges = [to_hz(top * i / (n_mels + 1)) for i in range(n_mels + 2)]
    bank = np.zeros((n_mels, n_fft // 2 + 1), dtype=np.float64)
    for m in range(n_mels):
        lo, mid, hi = edges[m], edges[m + 1], edges[m + 2]
        for k in range(n_fft // 2 + 1):
            f = k * sr / n_fft
            if lo < f < hi:
                bank[m, k] = min((f - lo) / (mid - lo), (hi - f) / (hi - mid)) * 2.0 / (hi - lo)
    return bank


def test_mel_filters_128():
    bank = wu.mel_filters("cpu", 128)
    assert tuple(bank.shape) == (128, 201) and bank.dtype == torch.float32
    ref = slaney_bank_fp64(128)
    assert np.abs(bank.numpy().astype(np.float64) - ref).max() < 1e-7
    assert (bank.numpy().sum(axis=1) > 0).all()                                 # no empty filter
    assert np.abs(wu.mel_filters("cpu", 80).numpy().astype(np.float64) - slaney_bank_fp64(80)).max() < 1e-7
    for n in (100, 0, 81):
        with pytest.raises(ValueError):
            wu.mel_filters("cpu", n)
    mel = wu.log_mel_spectrogram(np.zeros(3200, dtype=np.float32), n_mels=128)
    assert tuple(mel.shape) == (128, 20)


def test_mel_filters_128_equal_the_transformers_bank():
    audio_utils = pytest.importorskip("transformers.audio_utils")
    ref = audio_utils.mel_filter_bank(201, 128, 0.0, 8000.0, 16000, norm="slaney", mel_scale="slaney").T
    assert np.abs(wu.mel_filters("cpu", 128).numpy().astype(np.float64) - np.asarray(ref, dtype=np.float64)).max() < 1e-7


def test_mel_filters_80_are_bit_identical_to_the_committed_bank(golden_dir):
    bank = wu.mel_filters("cpu").numpy()
    assert bank.shape == (80, 201) and wu.N_MELS == 80
    assert hashlib.sha256(np.ascontiguousarray(bank).tobytes()).hexdigest() == MEL_80_SHA256
    g = np.load(os.path.join(golden_dir, "mel.npz"))                            # ... and what the reference's own bank sums to
    np.testing.assert_allclose(bank.sum(axis=1), g["filters_rowsum"], rtol=1e-4, atol=1e-6)
    assert abs(float(np.abs(bank).sum()) - float(g["filters_checksum"])) < 1e-3


# ---------------------------------------------------------------------------------------------------------------- engines
@pytest.fixture(scope="module")
def micro_v3(tmp_path_factory):
    out = tmp_path_factory.mktemp("v3") / "eng"
    B.run_build(["--synthetic", "micro-v3", "--seed", "5", "--output_dir", str(out), "--log_level", "error"])
    return out


def test_build_synthetic_micro_v3_writes_the_v3_configuration(micro_v3):
    with open(micro_v3 / "encoder_config.json") as f:
        enc = json.load(f)["builder_config"]
    with open(micro_v3 / "decoder_config.json") as f:
        dec = json.load(f)["builder_config"]
    assert enc["num_mels"] == 128 and dec["vocab_size"] == 51866
    assert (enc["num_layers"], dec["num_layers"]) == (2, 1)                     # unequal depths on purpose
    assert WhisperEncoding(micro_v3, only_torch=True).num_mels == 128
    for name in ("large-v3", "large-v3-turbo", "distil-large-v3"):
        d = synthetic.DIMS[name]
        assert (d["n_mels"], d["n_vocab"], d["n_audio_layer"], d["n_audio_state"], d["n_text_state"]) == (128, 51866, 32, 1280, 1280)
    assert [synthetic.DIMS[n]["n_text_layer"] for n in ("large-v3", "large-v3-turbo", "distil-large-v3")] == [32, 4, 2]


def test_conv1_of_128_bins_is_a_gemm_without_zero_columns():
    import weight as W
    w = np.arange(4 * 128 * 3, dtype=np.float32).reshape(4, 128, 3) / 1024
    g = W.conv_weight_as_gemm(w)
    assert g.shape == (4, 384)                                                  # 3 * 128: a multiple of the K tile, nothing appended
    assert np.array_equal(g.reshape(4, 3, 128), w.astype(np.float16).transpose(0, 2, 1))
    assert W.conv_weight_as_gemm(np.zeros((4, 80, 3), dtype=np.float32)).shape == (4, 256)


def test_decoding_rules_of_a_v3_engine_use_the_v3_ids(micro_v3):
    dec = WhisperDecoding(micro_v3, only_torch=True)
    tk = dec.tokenizer
    assert dec.is_multilingual and dec.num_languages == 100 and tk.num_languages == 100
    assert tk.timestamp_begin == 50365 and tk.no_speech == 50363 and tk.n_vocab == dec.decoder_config["vocab_size"] == 51866
    # the list the device loop uploads: SuppressTokens' plus <|notimestamps|>, which the host loops mask in ApplyTimestampRules
    suppress, blank = dec._device_suppress_lists()
    assert {50364, 50363, 50362, 50361, 50360, 50359, 50258} <= set(suppress) and 50365 not in suppress
    assert suppress == sorted(set(suppress)) and max(suppress) == 50364 and blank == [220, 50257]
    assert {50363, 50362, 50361, 50360, 50359, 50258} <= set(dec._get_suppress_tokens()) and 50365 not in dec._get_suppress_tokens()
    filters = [f for f in dec.logit_filters if isinstance(f, SuppressTokens)]
    logits = torch.zeros((1, 51866))
    tokens = torch.tensor([list(dec.initial_tokens)])
    for f in dec.logit_filters:
        f.apply(logits, tokens)
    masked = set(torch.nonzero(torch.isinf(logits[0])).flatten().tolist())
    assert len(filters) == 1 and {50364, 50363, 50362, 50361, 50360, 50359} <= masked and 50365 not in masked
    assert min(t for t in range(50259, 51866) if t not in masked) == 50365      # the first allowed special is <|0.00|>
    assert max(t for t in range(51866) if t not in masked) == 50365 + dec.max_initial_timestamp_index
    assert dec.initial_tokens == (50258, 50259, 50360)
    dec.set_language_tokens([50358, 50259])                                     # <|yue|> is a language of this vocabulary
    assert dec.tokens[:, 1].tolist() == [50358, 50259]
    with pytest.raises(ValueError):
        dec.set_language_tokens([50359])                                        # <|translate|> is not
    assert WhisperDecoding(micro_v3, only_torch=True, options=DecodingOptions(language="cantonese")).options.language == "cantonese"
    with pytest.raises(ValueError):                                             # the bias table refuses specials by the instance's eot
        WhisperDecoding(micro_v3, only_torch=True, options=DecodingOptions(sequence_bias=(((50365,), 1.0),)))


def test_a_99_language_engine_keeps_its_ids_and_an_unexplained_vocabulary_is_refused(tmp_path):
    out = tmp_path / "fv"
    B.run_build(["--synthetic", "micro-fullvocab", "--output_dir", str(out), "--log_level", "error"])
    dec = WhisperDecoding(out, only_torch=True)
    assert dec.num_languages == 99 and dec.tokenizer.timestamp_begin == 50364 and dec.tokenizer.no_speech == 50362
    assert 50363 not in dec._get_suppress_tokens() and 50362 in dec._get_suppress_tokens()
    with pytest.raises(ValueError):
        dec.set_language_tokens([50358])                                        # <|translate|> here, not a language
    with pytest.raises(ValueError):
        WhisperDecoding(out, only_torch=True, options=DecodingOptions(language="yue"))
    cfg_path = out / "decoder_config.json"
    cfg = json.loads(cfg_path.read_text())
    cfg["builder_config"]["vocab_size"] = 51900
    cfg_path.write_text(json.dumps(cfg))
    with pytest.raises(ValueError, match="51900"):
        WhisperDecoding(out, only_torch=True)


def test_literal_loop_on_micro_v3_through_the_torch_model(micro_v3):
    """detect a language among 100, decode two clips with Whisper's rules on the host; the first sampled token is a timestamp (the
    rules force one) and lies at or above the v3 <|0.00|>, never on <|notimestamps|> = 50364."""
    dims = Dims(**synthetic.DIMS["micro-v3"])
    sd = synthetic_state_dict(dims, 5)
    model = TM.Whisper(TM.ModelDimensions(**dims.to_dict())).load_state_dict({k: v.float() for k, v in sd.items()})
    mel = synthetic_mel(2, 2 * dims.n_audio_ctx, dims.n_mels, 77).float()
    assert tuple(mel.shape) == (2, 128, 128)
    enc = WhisperEncoding(micro_v3, only_torch=True)
    dec = WhisperDecoding(micro_v3, only_torch=True, options=DecodingOptions(sample_len=6))
    xa = enc.torch_get_audio_features(model, mel)
    languages, probs = dec.torch_detect_language(model, xa)
    assert len(languages) == 2 and all(code in dec.tokenizer.all_language_codes for code in languages)
    for p in probs:
        assert len(p) == 100 and "yue" in p and abs(sum(p.values()) - 1.0) < 1e-3
    assert all(50259 <= int(t) <= 50358 for t in dec.tokens[:, 1])
    tokens, sum_lp, nsp = dec.torch_main_loop(model, xa)
    assert tokens.shape == (2, 3 + 6) and tokens[:, 2].tolist() == [50360, 50360]
    first = tokens[:, 3]
    assert all(50365 <= int(t) <= 50365 + dec.max_initial_timestamp_index for t in first)
    sampled = tokens[:, 3:]
    assert not bool(((sampled >= 50359) & (sampled <= 50364)).any())            # no special between the languages and <|0.00|> is ever sampled
    nsp_want = model.logits(torch.tensor([[50258]] * 2), xa)[:, 0].float().softmax(-1)[:, 50363]
    assert np.allclose(nsp, nsp_want.tolist(), atol=1e-5)                       # the no-speech probability is read at 50363
    res = dec.post_process(tokens, sum_lp, nsp, xa, languages)
    assert len(res) == 2 and [r.language for r in res] == languages and all(isinstance(r.text, str) for r in res)
    assert all("<|notimestamps|>" not in dec.tokenizer.decode_with_timestamps(r.tokens) for r in res)
