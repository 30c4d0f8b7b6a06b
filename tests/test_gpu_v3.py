"""The large-v3 generation on a real MI355X: 128 mel bins, the 51 866-token vocabulary (100 languages), unequal encoder / decoder
depths.  Engines are built from `micro-v3` (128 / 64 / 128 / 2 / 2, vocab 51866, 448 / 128 / 2 / 1); the one test at product width
registers its own shape.  Every kernel here exists since before these models: the tests hold them at the new shapes --

  * the front end at 128 bins against the torch.stft mirror, at the bound of the 80-bin test (5e-4);
  * the frame kernels at 128 bins, bit for bit against their host contracts;
  * the encoder (conv1 as a GEMM with K = 3 * 128 = 384: no zero columns) and the decoder (logits over 51 866 columns) against the
    oracle, at the tolerances tests/test_gpu_model.py states (2e-2 features, 3e-2 logits, 6e-2 with the int8 KV cache);
  * the device loops (greedy, beam, sampling with top_k), the language pass over 100 tokens, word timestamps, forced probabilities,
    long-form transcription -- each against the literal statement the 99-language tests use;
  * the one-launch token step on a 4-layer decoder of large-v3's width.
"""
import ctypes as C
import os
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import build as B  # noqa: E402
import kernel_refs as KR  # noqa: E402
import longform as LF  # noqa: E402
import native  # noqa: E402
import sections as S  # noqa: E402
import speech as SP  # noqa: E402
import synthetic  # noqa: E402
import timing  # noqa: E402
import torch_model as TM  # noqa: E402
import transcribe as T  # noqa: E402
import truncation  # noqa: E402
import whisper_utils as wu  # noqa: E402
from decoding import DecodingOptions, WhisperDecoding  # noqa: E402
from encoding import WhisperEncoding  # noqa: E402
from oracle.whisper_oracle import (Dims, OracleConfig, OracleModel, greedy_reference_run, synthetic_mel,  # noqa: E402
                                   synthetic_state_dict)
from test_gpu_model import LOGIT_TOL, LOGIT_TOL_INT8_KV, build_engine  # noqa: E402

DIMS = Dims(**synthetic.DIMS["micro-v3"])
assert DIMS == Dims(128, 64, 128, 2, 2, 51866, 448, 128, 2, 1)
W = 2 * DIMS.n_audio_ctx
SEED, MEL_SEED = 5, 77
SOT_SEQUENCE = [50258, 50259, 50360]            # <|startoftranscript|> <|en|> <|transcribe|> with 100 languages
MEL_ATOL = 5e-4                                 # tests/test_gpu_kernels.py, tests/test_gpu_model.py: device front end vs host, 80 bins


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return native.load_library()


@pytest.fixture(scope="module")
def tmpdir_module(tmp_path_factory):
    return str(tmp_path_factory.mktemp("engines_v3"))


@pytest.fixture()
def chain_rearmed(lib):
    """The one-launch forms armed at the default mode before and after (tests/test_gpu_round5.py)."""
    lib.wm_set_decode_chain(-1)
    err = C.c_int(0)
    native.check(lib.wm_decode_chain_error(C.byref(err)))
    lib.wm_set_decode_chain(-1)
    yield
    native.check(lib.wm_decode_chain_error(C.byref(err)))
    lib.wm_set_decode_chain(-1)


# ---------------------------------------------------------------------------------------------------------------- front end
@pytest.mark.parametrize("n_samples", [4800, 16000])
def test_log_mel_128_bins_device_equals_host(lib, n_samples):
    """2 clips x 4 800 samples: 30 frames, one partly filled 32-frame workgroup; 2 x 16 000: 100 frames, the last one partly filled."""
    rng = KR.philox(n_samples)
    audio = (rng.standard_normal((2, n_samples)) * 0.1).astype(np.float32)
    audio[1, n_samples // 2:] *= 0.01                                           # a clip whose max - 8 clamp bites
    dev = wu.log_mel_spectrogram_device(torch.from_numpy(audio).cuda(), n_mels=128, dtype=torch.float32).cpu().numpy()
    assert dev.shape == (2, 128, n_samples // wu.HOP_LENGTH)
    for b in range(2):                                                          # the device clamps clip by clip: so does the reference here
        host = wu.log_mel_spectrogram(audio[b], n_mels=128).numpy()
        worst = float(np.abs(dev[b] - host).max())
        print(f"log-mel 128 bins, {n_samples} samples, clip {b}: max |device - host| = {worst:.3g} (bound {MEL_ATOL})")
        np.testing.assert_allclose(dev[b], host, atol=MEL_ATOL)
    half = wu.log_mel_spectrogram_device(torch.from_numpy(audio).cuda(), n_mels=128)
    assert half.dtype == torch.float16 and torch.equal(half.cpu(), torch.from_numpy(dev).half())
    with pytest.raises(ValueError):
        wu.log_mel_spectrogram_device(torch.from_numpy(audio).cuda(), n_mels=100)


# ------------------------------------------------------------------------------------------------------- frame kernels, 128 bins
def frame_files(seed):
    """Two files of 128 bins, 300 .. 700 frames, odd row lengths: (mel fp16 numpy [128, ld], content frames)."""
    from test_gpu_speech import speechlike
    rng = KR.philox(seed)
    return [(speechlike(rng, 128, 433 + 3, 433), 433), (speechlike(rng, 128, 698 + 1, 698, loud=((0.05, 0.2), (0.4, 0.45), (0.7, 0.95))), 698)]


def test_mel_windows_128_bins_bit_for_bit(lib):
    from test_gpu_longform import window_ref
    files = frame_files(1)
    dev = [torch.from_numpy(m).cuda() for m, _ in files]
    host = [m.view(np.int16) for m, _ in files]
    for seeks in ([0, 0], [131, 77], [433 - 5, 698 + 1], [305, 571]):           # odd seeks; across the end; behind it
        out = T.mel_windows([dev[0], None, dev[1]], [seeks[0], 9, seeks[1]], 128, W)
        torch.cuda.synchronize()
        got = out.cpu().view(torch.int16).numpy()
        want = np.stack([window_ref(host[0], seeks[0], 128, W), window_ref(None, 9, 128, W), window_ref(host[1], seeks[1], 128, W)])
        assert np.array_equal(got, want), seeks


def test_section_cuts_128_bins_equal_the_contract(lib):
    from test_gpu_sections import check_against_contract
    files = [(m, F, off) for (m, F), off in zip(frame_files(2), (1, 0))]
    for lo, hi, h in [(40, 96, 3), (64, 128, 10), (33, 77, 0)]:
        n, _ = check_against_contract(lib, files, 128, lo, hi, h)
        assert all(k >= 1 for k in n)


def test_speech_spans_and_gather_128_bins_equal_the_contract(lib):
    from test_gpu_speech import check_against_contract, device_gather
    files = [(m, F, off) for (m, F), off in zip(frame_files(3), (1, 3))]
    for cfg in [(3, 205, 100, 20, 5, 4), (10, 205, 100, 200, 25, 40), (0, 32768, 1000, 3, 2, 1)]:
        wants = check_against_contract(lib, files, 128, cfg)
        if cfg[0] == 3:
            assert [len(w) for w in wants] == [2, 3]                            # the loud stretches planted in each file
            for n_pad in (0, W):
                got = device_gather(lib, files, wants, 128, n_pad)
                for (mel, F, _), t, g in zip(files, wants, got):
                    assert np.array_equal(g, SP.packed_mel_ref(mel, F, t, n_pad).view(np.int16))


@pytest.mark.parametrize("gate", [False, True])
def test_channel_top_128_bins_equals_the_contract(lib, gate):
    from test_gpu_channels import check_against_contract, recording_of
    rng = KR.philox(40 + int(gate))
    gated = 0
    for h in (0, 10):
        recordings = [(recording_of(rng, n_ch, 128, F, h, 3), F) for n_ch, F in ((2, 433), (3, 698), (1, 301))]
        wants = check_against_contract(lib, recordings, 128, h, 3 if gate else 0)
        gated += sum(sum(c) for _, c in wants)
        assert wants[2][1] == [0]
    assert (gated > 0) == gate


# ---------------------------------------------------------------------------------------------------------------- the oracle's run
CONFIGS = [(False, False), (True, False), ("int4", False), (False, True), (True, True)]
N_ROWS_MAX, N_STEPS = 9, 5                       # prefill + four token steps


@pytest.fixture(scope="module")
def reference_runs():
    """Per configuration, computed once on first use and never changed: (kv scales, the oracle's greedy run over nine clips).  The rows
    of the oracle do not see each other, so the runs at 1 and 3 rows are the first rows of this one."""
    sd = synthetic_state_dict(DIMS, SEED)
    mel = synthetic_mel(N_ROWS_MAX, W, DIMS.n_mels, MEL_SEED)
    cache = {}

    def get(weight_only, int8_kv):
        key = (weight_only, int8_kv)
        if key not in cache:
            scales = None
            if int8_kv:
                scales = OracleModel(DIMS, sd, OracleConfig(act="float16", weight_only=weight_only)).calibrate_kv_scales(mel[:2], 6)
            oracle = OracleModel(DIMS, sd, OracleConfig(act="float16", weight_only=weight_only, int8_kv=int8_kv, kv_scales=scales))
            cache[key] = (scales, greedy_reference_run(oracle, mel, SOT_SEQUENCE, N_STEPS))
        return cache[key]
    return mel, get


@pytest.mark.parametrize("weight_only", [False, True])
def test_encoder_matches_oracle_conv1_k384(tmpdir_module, reference_runs, weight_only):
    """fp16 and int8 weight-only, batch 1 and 3: conv1 runs as a GEMM over K = 384 columns, a multiple of the 64-wide K tile -- the first
    engine whose conv1 matrix carries no zero columns (80 bins: 240, padded to 256)."""
    mel, get = reference_runs
    _, ref = get(weight_only, False)
    eng = build_engine(tmpdir_module, "micro-v3", SEED, weight_only)
    enc = WhisperEncoding(eng)
    assert enc.num_mels == 128 and enc.session.dims["n_mels"] == 128
    for batch in (1, 3):
        xa = enc.get_audio_features(mel[:batch].cuda())
        assert tuple(xa.shape) == (batch, DIMS.n_audio_ctx, DIMS.n_audio_state)
        worst = float((xa.float().cpu() - ref["xa"][:batch]).abs().max())
        print(f"micro-v3 encoder, weight_only={weight_only}, batch {batch}: max |xa - oracle| = {worst:.3g} (bound 2e-2)")
        assert worst < 2e-2
    with pytest.raises(ValueError, match="128"):                                # an 80-bin mel is refused before the encoder reads it
        enc.get_audio_features(synthetic_mel(1, W, 80, 1).cuda())
    with pytest.raises(ValueError, match="128"):
        enc.get_audio_features_async(synthetic_mel(1, W, 80, 1).cuda())


@pytest.mark.parametrize("weight_only,int8_kv", CONFIGS)
def test_decoder_matches_oracle_over_51866_columns(tmpdir_module, reference_runs, weight_only, int8_kv):
    """Prefill and four token steps, teacher-forced with the oracle's ids, at 1, 3 and 9 rows: every one of the 51 866 logits within the
    tolerance of tests/test_gpu_model.py, and the arg-max over the engine's row -- all the columns it hands out -- is the oracle's
    token wherever the oracle's top-1 margin exceeds twice the tolerance: nothing from the columns the logits GEMM pads to
    (51 866 .. 51 871) reaches a token."""
    mel, get = reference_runs
    scales, ref = get(weight_only, int8_kv)
    tol = LOGIT_TOL_INT8_KV if int8_kv else LOGIT_TOL
    eng = build_engine(tmpdir_module, "micro-v3", SEED, weight_only, int8_kv, scales)
    enc, dec = WhisperEncoding(eng), WhisperDecoding(eng)
    assert dec.decoder_config["vocab_size"] == 51866 and dec.use_int8_kv_cache == int8_kv
    for rows in (1, 3, 9):
        xa = enc.get_audio_features(mel[:rows].cuda())
        cross = dec.xa2cross_key_value(xa)
        assert len(cross) == DIMS.n_text_layer == 1
        logits, kv = dec.decode(torch.tensor([SOT_SEQUENCE] * rows).cuda(), cross)
        assert tuple(logits.shape) == (rows, 3, 51866) and bool(torch.isfinite(logits.float()).all())
        worst = float((logits.float().cpu() - ref["logits"][0][:rows]).abs().max())
        n_safe = n_ok = 0
        for s in range(N_STEPS - 1):
            logits, kv = dec.decode(ref["ids"][:rows, s:s + 1].cuda(), cross, kv)
            assert tuple(logits.shape) == (rows, 1, 51866)
            got = logits[:, 0].float().cpu()
            worst = max(worst, float((got - ref["logits"][s + 1][:rows, 0]).abs().max()))
            safe = (ref["margins"][:rows, s + 1] > 2 * tol).numpy()
            top = got.argmax(-1).numpy()
            assert (top < 51866).all() and bool(torch.isfinite(got).all())
            n_safe += int(safe.sum())
            n_ok += int((top[safe] == ref["ids"][:rows, s + 1].numpy()[safe]).sum())
        print(f"micro-v3 decoder, weight_only={weight_only}, int8_kv={int8_kv}, {rows} rows: max |logits - oracle| = {worst:.3g} "
              f"(bound {tol}), ids {n_ok}/{n_safe}")
        assert worst < tol
        assert n_ok == n_safe and n_safe > 0
        if int8_kv:
            assert kv[0].dtype == torch.int8


# ---------------------------------------------------------------------------------------------------------------- the loops
EOT = 50257
PEAKED_SEED, CLIP_SEED, N_CLIPS, SAMPLE_LEN = 3, 77, 3, 10


def peaked_checkpoint():
    """micro-v3 with logits of std 16, as tests/test_gpu_beam.py peaks micro-fullvocab: at the stock 1.5 a third of the adjacent
    candidates lie within 0.06 of each other and no loop comparison would be left."""
    sd = synthetic_state_dict(DIMS, PEAKED_SEED, logit_std=16.0)
    return {"dims": dict(synthetic.DIMS["micro-v3"]), "model_state_dict": sd}


@pytest.fixture(scope="module")
def loop_engine(tmpdir_module):
    from test_gpu_beam import build_engine as build_from_checkpoint
    eng = build_from_checkpoint(tmpdir_module, peaked_checkpoint(), "v3_peaked")
    mel = synthetic_mel(N_CLIPS, W, DIMS.n_mels, CLIP_SEED)
    return eng, WhisperEncoding(eng), mel


def literal_run_with_gaps(dec, xa):
    """main_loop_reference with, per row and step, the gap between the two best logits as the filters left them: the literal loop's own
    measure of how near a tie its arg-max was."""
    gaps = []
    update = dec.decoder.update

    def recording_update(tokens, logits, sum_logprobs):
        top2 = logits.float().topk(2, dim=-1).values
        gaps.append((top2[:, 0] - top2[:, 1]).cpu())
        return update(tokens, logits, sum_logprobs)
    dec.decoder.update = recording_update
    try:
        out = dec.main_loop_reference(xa)
    finally:
        dec.decoder.update = update
    return out, torch.stack(gaps, dim=1)                                        # [rows, steps]


def asserted_steps(gaps, guard):
    """Per row the number of leading steps that are compared: up to the first step whose gap is inside the guard (from there on the
    two loops may legitimately follow different histories).  At most half of a row's steps may be lost, and four must stay."""
    n = []
    for row in gaps:
        bad = (row < guard).nonzero()
        n.append(int(bad[0]) if len(bad) else len(row))
    assert all(k >= 4 and 2 * k >= gaps.shape[1] for k in n), (n, gaps)
    return n


def test_greedy_device_loop_equals_the_literal_loop(loop_engine, chain_rearmed):
    from test_gpu_beam import LOOP_TOL
    eng, enc, mel = loop_engine
    xa = enc.get_audio_features(mel.cuda())
    dec = WhisperDecoding(eng, options=DecodingOptions(sample_len=SAMPLE_LEN))
    languages, probs = dec.detect_language(xa)
    start = dec.tokens.clone()
    ref = WhisperDecoding(eng, options=DecodingOptions(sample_len=SAMPLE_LEN))
    languages_ref, probs_ref = ref.detect_language_reference(xa)
    assert languages == languages_ref and torch.equal(start, ref.tokens)
    for p, q in zip(probs, probs_ref):
        assert len(p) == 100 and set(p) == set(dec.tokenizer.all_language_codes) and "yue" in p
        assert abs(sum(p.values()) - 1.0) < 1e-3 and max(abs(p[k] - q[k]) for k in p) < 1e-3
    assert all(50259 <= int(t) <= 50358 for t in start[:, 1])
    (t_ref, lp_ref, nsp_ref), gaps = literal_run_with_gaps(ref, xa)
    n_cmp = asserted_steps(gaps, 2 * LOOP_TOL)
    print(f"greedy, micro-v3 peaked: literal loop's smallest top-2 gap {float(gaps.min()):.4g}, steps compared per row {n_cmp} of {gaps.shape[1]}")
    L0 = dec.sample_begin
    before = native.chain_status()["launches"]
    for _ in range(2):                                                          # eager + capture, then the replayed graphs
        t, lp, nsp = dec.main_loop(xa)
        assert int(t.max()) < 51866
        for r, k in enumerate(n_cmp):
            assert torch.equal(t[r, :L0 + k].cpu(), t_ref[r, :L0 + k].cpu()), r
        if all(k == gaps.shape[1] for k in n_cmp):
            assert torch.allclose(lp.cpu(), lp_ref.cpu(), atol=SAMPLE_LEN * LOOP_TOL)
        assert np.allclose(nsp, nsp_ref, atol=1e-3)
    status = native.chain_status()
    print(f"greedy, micro-v3 (ONE decoder layer), {N_CLIPS} rows: {status['launches'] - before} one-launch steps issued, declined={status['declined']}")
    assert status["launches"] > before and not status["declined"] and not status["error_pending"], status      # the one-launch step with n_layers = 1
    first = t[:, L0].cpu()
    assert bool(((first >= 50365) & (first <= 50365 + dec.max_initial_timestamp_index)).all())     # a v3 timestamp, never <|notimestamps|>
    sampled = t[:, L0:].cpu()
    assert not bool(((sampled > EOT) & (sampled < 50365)).any())
    # <|yue|> is a language here ...
    dec.set_language_tokens([50358] * N_CLIPS)
    t_yue, _, _ = dec.main_loop(xa)
    assert t_yue[:, 1].tolist() == [50358] * N_CLIPS
    ref.set_language_tokens([50358] * N_CLIPS)
    (t_yue_ref, _, _), gaps = literal_run_with_gaps(ref, xa)
    for r, k in enumerate(asserted_steps(gaps, 2 * LOOP_TOL)):
        assert torch.equal(t_yue[r, :L0 + k].cpu(), t_yue_ref[r, :L0 + k].cpu()), r
    dec._state.clear()


def test_set_language_tokens_yue_is_refused_with_99_languages(tmpdir_module):
    eng = build_engine(tmpdir_module, "micro-fullvocab", 3)
    dec = WhisperDecoding(eng)
    assert dec.tokenizer.num_languages == 99 and dec.tokenizer.timestamp_begin == 50364
    with pytest.raises(ValueError):
        dec.set_language_tokens([50358])
    dec.set_language_tokens([50357])


def test_beam_device_loop_equals_the_literal_loop(loop_engine):
    """beam_size 2, through the helpers of tests/test_gpu_beam.py: identical candidate lists and selected texts; the literal loop's run
    is itself a usable reference -- no two walked candidates closer than twice the sum bound, so no step is skipped."""
    from test_gpu_beam import LOOP_TOL, assert_same_candidates, run_both
    eng, enc, mel = loop_engine
    dec, out, ref, stats = run_both(dict(fp16=eng, mel=mel), "fp16", 2, N_CLIPS, sample_len=SAMPLE_LEN)
    print(f"beam 2, micro-v3 peaked: smallest candidate gap {stats['min_gap']:.4g}, {stats['reorders']} moved rows")
    assert stats["min_gap"] >= 2 * LOOP_TOL, stats
    for got in out:
        assert_same_candidates(got, ref)
    assert all(t < 51866 for res in out[0][1] for t in res.tokens)
    dec._state.clear()


def test_sampling_with_top_k_5_stays_inside_the_literal_kept_set(loop_engine):
    """temperature 0.8, top_k 5 through wm_sample_step.  The device's draws are its own generator's, so its tokens are held to the
    literal statement teacher-forced with them: every sampled token lies in the kept set truncation.keep_mask makes of the logits the
    literal path (decode() + the host filters) computes for the same history, and the booked log-probability is the untruncated
    one.  A step whose fifth and sixth candidate are closer than the guard is not asserted (at most half of a row's, four stay)."""
    from test_gpu_beam import LOOP_TOL
    eng, enc, mel = loop_engine
    xa = enc.get_audio_features(mel.cuda())
    opts = DecodingOptions(sample_len=SAMPLE_LEN, language="en", temperature=0.8, top_k=5)
    dec, ref = WhisperDecoding(eng, options=opts), WhisperDecoding(eng, options=opts)
    torch.manual_seed(11)
    t, lp, _ = dec.main_loop(xa)
    torch.manual_seed(11)
    t2, lp2, _ = dec.main_loop(xa)                                              # the replayed graphs follow the seed
    assert torch.equal(t, t2) and torch.equal(lp, lp2)
    t, L0 = t.cpu(), dec.sample_begin
    assert t.shape == (N_CLIPS, L0 + SAMPLE_LEN) and int(t.max()) < 51866
    cross = ref.xa2cross_key_value(xa)
    sums = torch.zeros(N_CLIPS)
    asserted = [0] * N_CLIPS
    for s in range(SAMPLE_LEN):
        prefix = t[:, :L0 + s].cuda()
        logits, _ = ref.decode(prefix, cross)
        last = logits[:, -1].clone()
        for f in ref.logit_filters:
            f.apply(last, prefix)
        x = last.float().cpu()
        keep = truncation.keep_mask(x.numpy(), 0.8, 5, 1.0, 0.0)
        top6 = x.topk(6, dim=-1).values
        alive = t[:, L0 + s - 1] != EOT if s else torch.ones(N_CLIPS, dtype=torch.bool)
        for r in range(N_CLIPS):
            if not alive[r]:
                assert int(t[r, L0 + s]) == EOT
                continue
            sums[r] += torch.log_softmax(x[r], dim=-1)[t[r, L0 + s]]
            if float(top6[r, 4] - top6[r, 5]) >= 2 * LOOP_TOL:
                assert keep[r, int(t[r, L0 + s])], (r, s)
                asserted[r] += 1
    assert all(k >= 4 and 2 * k >= SAMPLE_LEN for k in asserted), asserted
    assert torch.allclose(lp.cpu(), sums, atol=SAMPLE_LEN * LOOP_TOL)
    dec._state.clear()


# ------------------------------------------------------------------------------------------------- word timestamps, forced probs
def test_word_timestamps_agree_with_the_torch_statement(tmpdir_module):
    """tests/test_gpu_word_timestamps.py: test_word_timestamps_end_to_end on micro-v3: two rows, ragged frames; same words, the
    probabilities within the logit tolerance, and where the torch matrix's DTW path is unambiguous the same path and times.  The
    forced sequence carries the v3 <|notimestamps|> (50364) and the default heads are the upper half of ONE decoder layer: layer 0."""
    from test_gpu_word_timestamps import dtw_margin
    eng = build_engine(tmpdir_module, "micro-v3", SEED)
    enc, dec = WhisperEncoding(eng), WhisperDecoding(eng)
    assert dec.tokenizer.bpe is not None and dec.alignment_heads() == [0, 1]
    assert dec._forced_tokens([50365, 440, 50400])[1] == [50258, 50259, 50360, 50364, 440, 50257]
    dec.sample_len = 12
    dec.keep_alignment_matrix = True
    mel = synthetic_mel(2, W, DIMS.n_mels, MEL_SEED)
    xa = enc.get_audio_features(mel.cuda())
    languages, _ = dec.detect_language(xa)
    t, lp, nsp = dec.main_loop(xa)
    results = dec.post_process(t, lp, nsp, xa, languages)
    frames = [W, 2 * 45 + 1]
    words = dec.word_timestamps(xa, results, frames)
    dev = dec.last_alignment
    assert dec.word_timestamps(xa, results, frames) == words
    sd = synthetic_state_dict(DIMS, SEED)
    model = TM.Whisper(TM.ModelDimensions(**DIMS.to_dict())).load_state_dict({k: v.float() for k, v in sd.items()})
    ref_dec = WhisperDecoding(eng, only_torch=True)
    ref = ref_dec.torch_word_timestamps(model, xa.float().cpu(), results, frames)
    tor = ref_dec.last_alignment
    assert any(len(w) > 0 for w in words)
    tk, n_prefix, spf = dec.tokenizer, len(dec.tokenizer.sot_sequence), 30.0 / DIMS.n_audio_ctx
    compared = 0
    for b in range(2):
        assert [(w.word, w.tokens) for w in words[b]] == [(w.word, w.tokens) for w in ref[b]]
        if not words[b]:
            continue
        n = dev["path_len"][b]
        text = [x for x in results[b].tokens if x < tk.eot]
        ws, wt = dec._split_words(text + [tk.eot], results[b].language)
        own = timing.words_from_path(dev["path_text"][b, :n], dev["path_time"][b, :n], ws, wt,
                                     dev["token_probs"][b, n_prefix: n_prefix + len(text)].tolist(), spf)
        assert [(w.start, w.end) for w in own] == [(w.start, w.end) for w in words[b]]
        assert all(0 <= w.start <= w.end <= (frames[b] // 2) * spf + 1e-9 for w in words[b])
        assert np.allclose([w.probability for w in words[b]], [w.probability for w in ref[b]], atol=LOGIT_TOL)
        m32 = tor[b]["matrix"].numpy()
        tot = np.zeros(tor[b]["scores"][0].shape)
        for Sc in (s.double().numpy() for s in tor[b]["scores"]):
            e = np.exp(Sc - Sc.max(axis=1, keepdims=True))
            Wm = e / e.sum(axis=1, keepdims=True)
            mu, sdv = Wm.mean(0, keepdims=True), Wm.std(0, keepdims=True)
            Z = np.where(sdv > 0, (Wm - mu) / np.where(sdv > 0, sdv, 1), 0)
            if Z.shape[1] > 3:
                Z = np.sort(np.lib.stride_tricks.sliding_window_view(np.pad(Z, ((0, 0), (3, 3)), mode="reflect"), 7, axis=1), axis=-1)[..., 3]
            tot += Z
        m64 = (tot / len(tor[b]["scores"]))[n_prefix: tot.shape[0] - 1]
        bound = 4 * float(np.abs(m32 - m64).max())
        margin = dtw_margin(-m32, tor[b]["path_text"], tor[b]["path_time"])
        print(f"micro-v3 utterance {b}: matrix bound {bound:.3g}, smallest DTW margin on the reference path {margin:.3g}")
        if margin > 2 * bound:
            assert [(w.start, w.end) for w in words[b]] == [(w.start, w.end) for w in ref[b]]
            assert dev["path_text"][b, :n].tolist() == tor[b]["path_text"].tolist() and dev["path_time"][b, :n].tolist() == tor[b]["path_time"].tolist()
            compared += 1
    assert compared >= 1
    dec._state.clear()


@pytest.mark.parametrize("n_pos", [1, 4])
def test_forced_probs_over_the_v3_vocabulary(lib, n_pos):
    """wm_forced_probs with V = 51 866 and limit = <|endoftext|> = 50 257 -- logsumexp(x[:eot]) as word_timestamps calls it -- against
    the fp64 restatement at the bound of tests/test_gpu_forced_probs.py: max(4 x the fp32 PyTorch expression's error, 2^-22)."""
    from test_gpu_forced_probs import make_case, parent_expression, reference64, run
    V = 51866
    buf, view, x, nxt, dead, _, stride_b, stride_p = make_case(n_pos, V, 11, 3, 7000 + n_pos)
    for limit in (EOT, V - 4):
        got, nxt_buf = run(lib, view, nxt, n_pos, V, limit, stride_b, stride_p)
        ref = reference64(x, nxt, limit)
        parent = parent_expression(view, nxt_buf[:, :n_pos], limit).cpu().numpy().astype(np.float64)
        got = got.numpy().astype(np.float64)
        live = np.isfinite(parent)
        assert np.isfinite(got).all() and (got[~live] == 0.0).all() and (ref[~live] == 0.0).all()
        e_torch, e_dev = float(np.abs(parent[live] - ref[live]).max()), float(np.abs(got[live] - ref[live]).max())
        bound = max(4 * e_torch, 2.0 ** -22)
        print(f"forced probs V {V} limit {limit} n_pos {n_pos}: max |device - fp64| = {e_dev:.3g}, bound = {bound:.3g}")
        assert e_dev <= bound


# ---------------------------------------------------------------------------------------------------------------- long-form
LONG_CONTENTS = [W + W // 2, 2 * W + W // 2]     # 1.5 and 2.5 windows
LONG_KW = dict(temperatures=(0.0,), compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None)


def long_mels():
    """Two files of 1.5 and 2.5 windows (+ the window of padding), each with one stretch far below the rest (a pause for `speech` and
    `sections` to find)."""
    mels = []
    for i, c in enumerate(LONG_CONTENTS):
        m = synthetic_mel(1, c + W, DIMS.n_mels, 700 + i)[0].half()
        low = float(m.float().min()) - 3.0
        m[:, c // 2 - 20: c // 2 + 20] = low
        m[:, c:] = low
        mels.append(m.cuda().contiguous())
    return mels


def replay(trace, contents, tk):
    """The literal schedule (longform.transcribe_reference) per "file" of the traced run, fed with the results the run recorded."""
    recorded = {}
    for e in trace:
        if e.get("kind") == "align":
            continue
        for r, on, res in zip(e["rows"], e["live"], e["results"]):
            if on:
                recorded[(r[0], r[1], e["temperature"])] = res
    out, used = [], set()
    for f, c in enumerate(contents):
        def decode_one(seek, temperature, f=f):
            used.add((f, seek, temperature))
            return recorded[(f, seek, temperature)]
        out.append(LF.transcribe_reference(decode_one, c, window=W, timestamp_begin=tk.timestamp_begin, decode_text=tk.decode, **LONG_KW))
    assert used == set(recorded)
    return out


@pytest.mark.parametrize("layers", [False, True])
def test_long_form_returns_the_segments_of_the_literal_schedule(tmpdir_module, layers):
    eng = build_engine(tmpdir_module, "micro-v3", SEED)
    enc = WhisperEncoding(eng)
    dec = WhisperDecoding(eng)
    dec.sample_len = 12
    tk = dec.tokenizer
    assert tk.timestamp_begin == 50365
    mels, trace = long_mels(), []
    fs = LF.CHUNK_LENGTH / W
    if not layers:
        results = T.transcribe_mel(enc, dec, mels, LONG_CONTENTS, n_rows=2, trace=trace, **LONG_KW)
        want = replay(trace, LONG_CONTENTS, tk)
        for res, segs in zip(results, want):
            assert res["segments"] == segs and len({s["seek"] for s in segs}) >= 2
            assert res["text"] == tk.decode([t for s in segs for t in s["tokens"]]).strip()
            assert res["language"] in tk.all_language_codes
        assert {e["windows"].shape for e in trace} == {(2, 128, W)}
    else:
        speech = SP.SpeechOptions(margin_db=8.0, min_silence_seconds=20 * fs, min_speech_seconds=5 * fs, speech_pad_seconds=4 * fs)
        sec = S.SectionOptions(max_seconds=30.0)
        results = T.transcribe_mel(enc, dec, mels, LONG_CONTENTS, n_rows=2, trace=trace, speech=speech, sections=sec, **LONG_KW)
        # the layers on the host contracts: spans -> packed mels -> cuts -> sections; the sections are the "files" of the trace
        host = [m.cpu().numpy() for m in mels]
        spans = [SP.speech_spans_ref(m, F, *speech.frames(W, 128)) for m, F in zip(host, LONG_CONTENTS)]
        assert all(len(sp) == 2 for sp in spans)                                # the planted pause splits every file
        packed = [SP.packed_mel_ref(m, F, sp, W) for m, F, sp in zip(host, LONG_CONTENTS, spans)]
        frames = [sum(b - a for a, b in sp) for sp in spans]
        pieces, owner, starts = [], [], []
        for f, (m, F) in enumerate(zip(packed, frames)):
            for a, b in S.section_bounds(F, S.section_cuts_ref(m, F, *sec.frames(W, 128))):
                pieces.append(b - a), owner.append(f), starts.append(a)
        want = replay(trace, pieces, tk)
        for f, (res, sp) in enumerate(zip(results, spans)):
            mine = [i for i, o in enumerate(owner) if o == f]
            merged = S.merge_sections([want[i] for i in mine], [starts[i] for i in mine], fs)
            assert res["segments"] == SP.restore(merged, sp, fs)
            assert res["speech"] == [(a * fs, b * fs) for a, b in sp] and len(res["sections"]) == len(mine)
            assert res["segments"]
    assert all(t < 51866 for r in results for s in r["segments"] for t in s["tokens"])
    with pytest.raises(ValueError, match="128"):                                # an 80-bin mel never reaches a kernel
        T.transcribe_mel(enc, dec, [synthetic_mel(1, 2 * W, 80, 1)[0].cuda().contiguous()], [W], **LONG_KW)
    dec._state.clear()


# ---------------------------------------------------------------------------------------------------------------- width
@pytest.mark.parametrize("quantised", [True, False])
def test_four_layer_decoder_of_large_v3_width_takes_the_one_launch_step(lib, tmpdir_module, chain_rearmed, quantised):
    """large-v3-turbo's decoder (1280 wide, 20 heads, FOUR layers, 51 866 tokens) under one encoder layer: 1 and 8 rows, prefill and eight
    token steps teacher-forced with the GPU-resident oracle's ids through the in-place-cache call main_loop makes.  Logits within the
    tolerance tests/test_gpu_round5.py holds the full-depth model to; every token step was ONE launch (wm_decode_chain_status counts
    them), nothing was declined and nothing gave up."""
    dims_d = dict(synthetic.DIMS["large-v3"], n_audio_layer=1, n_text_layer=4)
    name = "large-v3-1x4layer"
    synthetic.DIMS[name] = dims_d
    dims = Dims(**dims_d)
    ck = synthetic.synthetic_checkpoint(name, 9, device="cuda")
    sd = {k: v.cpu() for k, v in ck["model_state_dict"].items()}
    mel = torch.cat([synthetic_mel(1, 3000, 128, 4242 + k) for k in range(8)]).cuda()
    scales = None
    if quantised:
        cal = OracleModel(dims, sd, OracleConfig(act="float16", weight_only=True)).to("cuda")
        scales = cal.calibrate_kv_scales(mel[:1], 3)
        del cal
    oracle = OracleModel(dims, sd, OracleConfig(act="float16", weight_only=quantised, int8_kv=quantised, kv_scales=scales)).to("cuda")
    del sd
    n_steps = 9
    ref = greedy_reference_run(oracle, mel, SOT_SEQUENCE, n_steps)
    del oracle
    out = os.path.join(tmpdir_module, f"eng_{name}_{int(quantised)}")
    argv = ["--output_dir", out, "--use_gpt_attention_plugin", "--use_gemm_plugin", "--use_layernorm_plugin", "--log_level", "error"]
    if quantised:
        from test_gpu_model import _write_kv_scales
        qdir = os.path.join(tmpdir_module, f"quantize_{name}", "1-gpu")
        _write_kv_scales(qdir, scales)
        argv += ["--use_weight_only", "--int8_kv_cache", "--quantize_dir", qdir]
    B.build_from_checkpoint(ck, B.parse_arguments(argv))
    del ck
    torch.cuda.empty_cache()
    tol = LOGIT_TOL_INT8_KV if quantised else LOGIT_TOL
    enc = WhisperEncoding(Path(out))
    assert enc.num_mels == 128
    xa8 = enc.get_audio_features(mel)
    assert float((xa8.float() - ref["xa"].to(xa8.device).float()).abs().max()) < 2e-2
    lib.wm_set_decode_chain(2)
    for rows in (1, 8):
        xa = xa8[:rows].contiguous()
        dec = WhisperDecoding(Path(out))
        cfg = dec.decoder_config
        cap, V = cfg['num_text_ctx'], cfg['vocab_size']
        assert (cfg['num_layers'], V) == (4, 51866)
        st = dec._fast_state(rows, xa.device)
        cross = dec._cross_persistent(xa, st)
        tokens = torch.zeros((rows, cap + 1), dtype=torch.int32, device="cuda")
        tokens[:, :3] = torch.tensor(SOT_SEQUENCE, dtype=torch.int32)
        tokens[:, 3:3 + n_steps - 1] = ref["ids"][:rows, :n_steps - 1].to(torch.int32)
        s = torch.cuda.current_stream().cuda_stream
        sess, pos = dec.decoder_session, dec.positional_embedding
        before = native.chain_status()["launches"]
        logits3 = torch.empty((rows, 3, V), dtype=torch.float16, device="cuda")
        sess.decoder_step(tokens[:, :3], pos[0:3], cross, None, cap, st['kv'], cap, logits3, 0, s)
        worst = float((logits3.float().cpu() - ref["logits"][0][:rows].cpu()).abs().max())
        logits1 = torch.empty((rows, 1, V), dtype=torch.float16, device="cuda")
        n_safe = n_ok = 0
        for k in range(n_steps - 1):
            cur = 3 + k + 1
            sess.decoder_step(tokens[:, cur - 1:cur], pos[cur - 1:cur], cross, st['kv'], cap, st['kv'], cap, logits1, cur - 1, s)
            got = logits1[:, 0].float().cpu()
            worst = max(worst, float((got - ref["logits"][k + 1][:rows, 0].cpu()).abs().max()))
            safe = (ref["margins"][:rows, k + 1].cpu() > 2 * tol).numpy()
            n_safe += int(safe.sum())
            n_ok += int((got.argmax(-1).numpy()[safe] == ref["ids"][:rows, k + 1].cpu().numpy()[safe]).sum())
        torch.cuda.synchronize()
        launches = native.chain_status()["launches"] - before
        status = native.chain_status()
        print(f"4-layer decoder at large-v3 width, quantised={quantised}, {rows} rows: max |logits - oracle| = {worst:.4f} (bound {tol}), "
              f"ids {n_ok}/{n_safe}, {launches} one-launch steps of {n_steps - 1}")
        assert launches == n_steps - 1, (rows, launches, status)               # the one-launch token step was taken at every step
        assert not status["error_pending"] and not status["declined"], status
        assert worst < tol, worst
        assert n_ok == n_safe and n_safe > 0
        del dec, st, cross
    synthetic.DIMS.pop(name, None)


# ---------------------------------------------------------------------------------------------------------------- front to back
def test_the_three_command_lines_feed_a_128_bin_mel_from_flac(tmpdir_module, golden_dir, tmp_path, capsys):
    """run.py's, transcribe.py's and summarize.py's `main` on the committed LibriSpeech clip with a micro-v3 engine of the real
    30-second window, no flag but the engine directory: every front end runs at the engine's 128 bins -- the encoder is fed
    [1, 128, 3000] by run.py and by transcribe.py, [2, 128, 3000] by summarize.py -- and the languages are the 100-language vocabulary's."""
    import shutil
    import run as R
    import summarize as SM
    name = "micro-v3-30s"
    synthetic.DIMS[name] = dict(synthetic.DIMS["micro-v3"], n_audio_ctx=1500)
    try:
        eng = build_engine(tmpdir_module, name, SEED)
    finally:
        synthetic.DIMS.pop(name, None)
    flac = os.path.join(golden_dir, "librispeech_1089-134691-0000.flac")
    codes = WhisperDecoding(eng, only_torch=True).tokenizer.all_language_codes
    assert len(codes) == 100
    fed = []
    real = WhisperEncoding.get_audio_features

    def spy(self, mel):
        fed.append((tuple(mel.shape), mel.dtype, self.num_mels))
        return real(self, mel)
    WhisperEncoding.get_audio_features = spy
    try:
        result = R.main(["--engine_dir", str(eng), "--input_file", flac])
        assert fed == [((1, 128, 3000), torch.float16, 128)]
        assert "transcribe time" in capsys.readouterr().out
        assert isinstance(result.text, str) and result.language in codes and all(t < 51866 for t in result.tokens)
        del fed[:]
        long = T.main(T.parse_arguments(["--engine_dir", str(eng), "--input_file", flac, "--no_fallback"]))
        assert fed and set(fed) == {((1, 128, 3000), torch.float16, 128)}
        assert len(long) == 1 and long[0]["language"] in codes and long[0]["segments"]
        with pytest.raises(ValueError):                                         # a language the vocabulary has no token for
            T.main(T.parse_arguments(["--engine_dir", str(eng), "--input_file", flac, "--language", "klingon"]))
        del fed[:]
        chapter = tmp_path / "ds" / "1089" / "134691"
        chapter.mkdir(parents=True)
        for i in range(2):
            shutil.copy(flac, chapter / f"1089-134691-000{i}.flac")
        (chapter / "1089-134691.trans.txt").write_text("".join(f"1089-134691-000{i} HE COULD WAIT NO LONGER\n" for i in range(2)))
        report = SM.main(SM.parse_arguments(["--test_trt_llm", "--engine_dir", str(eng), "--dataset_dir", str(tmp_path / "ds"),
                                             "--batch_size", "2", "--sample_len", "8", "--log_level", "error"]))["whisper-mi355"]
        assert fed == [((2, 128, 3000), torch.float16, 128)]
        assert report["utterances"] == 2 and report["hypotheses"][0] == report["hypotheses"][1]
    finally:
        WhisperEncoding.get_audio_features = real
