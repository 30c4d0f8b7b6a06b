"""One copy of the cross-attention K/V per utterance for beam / best_of candidates (wm_decoder_group_io::cross_group,
WhisperDecoding(shared_cross_kv=True)) and the recipe it unlocks (beam search at temperature 0, fallback_best_of samples above, word
timestamps, the full ladder in transcribe) on the micro-fullvocab engines of tests/test_gpu_beam.py and tests/test_gpu_model.py.

The harnesses are the project's own: tests/test_gpu_beam.py (device loop against the literal BeamSearchDecoder loop, with that
file's candidate-gap condition), tests/test_gpu_word_timestamps.py (the PyTorch alignment), tests/test_gpu_word_longform.py (a
transcribe run replayed file by file through longform.transcribe_reference) and tests/test_gpu_sections.py (a sectioned run against
its sections as files)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import longform as LF  # noqa: E402
import native  # noqa: E402
import synthetic  # noqa: E402
import timing  # noqa: E402
import torch_model as TM  # noqa: E402
import transcribe as T  # noqa: E402
import test_gpu_beam as BM  # noqa: E402  (helpers only)
import test_gpu_sections as SEC  # noqa: E402
import test_gpu_word_longform as WL  # noqa: E402
from decoding import DecodingOptions, WhisperDecoding  # noqa: E402
from encoding import WhisperEncoding  # noqa: E402
from oracle.whisper_oracle import Dims, synthetic_mel, synthetic_state_dict  # noqa: E402
from test_gpu_beam import engines  # noqa: E402,F401  (module fixture: the peaked fp16 / int8 engines and four clips)
from test_gpu_model import LOGIT_TOL, LOGIT_TOL_INT8_KV, build_engine  # noqa: E402
from test_gpu_word_timestamps import dtw_margin  # noqa: E402

DIMS = Dims(**synthetic.DIMS["micro-fullvocab"])
W = 2 * DIMS.n_audio_ctx


@pytest.fixture(scope="module")
def tmpdir_module(tmp_path_factory):
    return str(tmp_path_factory.mktemp("shared_engines"))


@pytest.fixture(scope="module")
def stock(tmpdir_module):
    """The stock micro-fullvocab engine (seed 3) of the long-form tests, its encoder, one with int8 cross K/V -- and, for the step
    tests, `kinds`: those two and a weight-only engine with an int8 self-attention cache (logits of std 1.5: the teacher-forced
    bound is meant for such, not for the peaked fixture of the beam tests, whose fp16 logits step by 0.03 and more)."""
    eng = build_engine(tmpdir_module, "micro-fullvocab", 3)
    eng8 = build_engine(tmpdir_module, "micro-fullvocab", 3, cross_scales=[0.05] * DIMS.n_text_layer)
    kv8 = build_engine(tmpdir_module, "micro-fullvocab", 3, weight_only=True, int8_kv=True, kv_scales=[0.031] * DIMS.n_text_layer)
    return eng, WhisperEncoding(eng), eng8, dict(fp16=eng, x8=eng8, int8=kv8)


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------------ the engine
class Steps:
    """B = n_audio * G rows with random tokens (so that the candidates differ).  A prefill of three tokens on cross K/V repeated G times
    fills the caches; from copies of them ONE decode step runs twice: with cross_group = G on the n_audio utterances' cross K/V, and
    on the repeated K/V with not_alone = 1 (neither takes a one-launch form).  Where G * 3 <= 8 the prefill runs grouped as well."""

    def __init__(self, eng, n_audio, G, live=None):
        enc, dec = WhisperEncoding(eng), WhisperDecoding(eng)
        cfg, sess = dec.decoder_config, dec.decoder_session
        B, cap, V, H = n_audio * G, 16, cfg['vocab_size'], cfg['num_heads']
        xa = enc.get_audio_features(synthetic_mel(n_audio, W, DIMS.n_mels, 77 + n_audio).cuda())
        cross = [torch.empty((n_audio, 2, H, cfg['num_audio_ctx'], 64), dtype=torch.int8 if dec.use_int8_cross_kv else torch.float16, device="cuda")
                 for _ in range(cfg['num_layers'])]
        dec.cross_attn_session.cross_kv(xa.half().contiguous(), cross, stream())
        rep = [t.repeat_interleave(G, 0).contiguous() for t in cross]
        tokens = torch.from_numpy(np.random.Generator(np.random.Philox(5)).integers(300, 30000, size=(B, 4)).astype(np.int32)).cuda()
        pos = dec.positional_embedding
        kv_dtype = torch.int8 if dec.use_int8_kv_cache else torch.float16
        self.tol = LOGIT_TOL_INT8_KV if dec.use_int8_kv_cache else LOGIT_TOL
        self.sess, self.pos, self.cross, self.tokens, self.cap, self.dec = sess, pos, cross, tokens, cap, dec

        def prefill(cr, **kw):
            kv = [torch.zeros((B, 2, H, cap, 64), dtype=kv_dtype, device="cuda") for _ in range(cfg['num_layers'])]
            l3 = torch.full((B, 3, V), float("nan"), dtype=torch.float16, device="cuda")
            sess.decoder_step(tokens[:, :3], pos[0:3], cr, None, cap, kv, cap, l3, 0, stream(), **kw)
            torch.cuda.synchronize()
            return kv, l3.float().cpu()
        kv0, self.prefill_repeated = prefill(rep, not_alone=True)
        self.prefill_shared = prefill(cross, cross_group=G)[1] if G * 3 <= 8 else None
        self.out = {}
        for name, cr, kw in (("shared", cross, dict(cross_group=G)), ("repeated", rep, dict(not_alone=True))):
            kv = [t.clone() for t in kv0]
            l1 = torch.full((B, 1, V), float("nan"), dtype=torch.float16, device="cuda")
            if live is not None:
                kw["live_rows"] = torch.tensor(live[0], dtype=torch.int32, device="cuda")
                if name == "shared":
                    kw["live_groups"] = torch.tensor(live[1], dtype=torch.int32, device="cuda")
            sess.decoder_step(tokens[:, 3:4], pos[3:4], cr, kv, cap, kv, cap, l1, 3, stream(), **kw)
            torch.cuda.synchronize()
            self.out[name] = l1.float().cpu()

    def diffs(self, rows=None):
        a1, b1 = self.out["shared"], self.out["repeated"]
        if rows is not None:
            a1, b1 = a1[rows], b1[rows]
        assert bool(torch.isfinite(a1).all()) and bool(torch.isfinite(b1).all())
        d3 = 0.0
        if self.prefill_shared is not None:
            assert bool(torch.isfinite(self.prefill_shared).all())
            d3 = float((self.prefill_shared - self.prefill_repeated).abs().max())
        return d3, float((a1 - b1).abs().max()), torch.equal(a1, b1)


@pytest.mark.parametrize("kind,n_audio,G", [("fp16", 2, 3), ("int8", 2, 5), ("fp16", 1, 8), ("fp16", 3, 2), ("x8", 2, 3), ("fp16", 60, 2)])
def test_decoder_step_with_cross_group_stays_within_the_logit_bound(stock, kind, n_audio, G):
    """wm_decoder_step with cross_group = G against the same call on repeated cross K/V: the decode step (and for G = 2 the three-token
    prefill, where a row's own item reads K/V row b / G) within the teacher-forced bound.  60 x 2 rows: the repeated call takes the single pass
    (240 (row, head) pairs), the shared one cuts the keys of its 120 items into four pieces.  Where both calls cut the key range alike
    (every other case here) the decode step is bit-identical, as include/whisper_mi355.h states."""
    s = Steps(stock[3][kind], n_audio, G)
    d3, d1, same = s.diffs()
    print(f"cross_group {kind} {n_audio} x {G}: prefill max |diff| {d3:.3g}, decode step {d1:.3g} (bound {s.tol:.0e}), step bit-identical: {same}")
    assert d3 <= s.tol and d1 <= s.tol
    if n_audio * DIMS.n_text_head * G <= 160:
        assert same, "same number of key-range pieces: the step must be bit-identical"


def test_decoder_step_is_bit_identical_when_both_calls_take_the_single_pass(stock):
    """81 utterances x 2: 162 (utterance, head) items shared, 324 repeated -- both above the 160 pairs below which the key range is cut."""
    s = Steps(stock[0], 81, 2)
    d3, d1, same = s.diffs()
    print(f"cross_group 81 x 2, single pass both: prefill max |diff| {d3:.3g}, decode step {d1:.3g}, bit-identical: {same}")
    assert same and d3 <= s.tol


def test_decoder_step_live_lists_and_refusals(stock):
    """Utterance 0 finished, utterance 1 with one finished row, utterance 2 live: the live rows' logits are those of the repeated call with
    the same live rows; a batch that is no multiple of the group, more than 8 queries per item and live rows without live utterances are refused."""
    s = Steps(stock[0], 3, 3, live=([5, 3, 5, 6, 7, 8, 0, 0, 0, 0], [2, 1, 2, 0]))
    d3, d1, same = s.diffs(rows=[3, 5, 6, 7, 8])
    assert same and d3 <= s.tol
    sess, lib, B, V = s.sess, native.load_library(), 9, s.dec.decoder_config['vocab_size']
    kv = [torch.zeros((B, 2, DIMS.n_text_head, s.cap, 64), dtype=torch.float16, device="cuda") for _ in range(DIMS.n_text_layer)]
    lg = torch.zeros((B, 1, V), dtype=torch.float16, device="cuda")
    l3 = torch.zeros((B, 3, V), dtype=torch.float16, device="cuda")

    def refused(gio, what):
        assert lib.wm_decoder_step_group(sess.engine.handle, C.byref(gio), stream()) == 1
        assert what in lib.wm_last_error(), lib.wm_last_error()
    gio = sess.make_decoder_group_io(s.tokens[:, :1], s.pos[0:1], s.cross, None, s.cap, kv, s.cap, lg, 0, cross_group=3)
    gio.cross_group = 2                                       # 9 rows are no multiple of 2
    refused(gio, b"cross_group")
    gio.cross_group = -1
    refused(gio, b"cross_group")
    all_live = torch.tensor([9] + list(range(9)), dtype=torch.int32, device="cuda")
    gio.cross_group, gio.io.live_rows = 3, all_live.data_ptr()
    refused(gio, b"live_groups")                              # the live rows without the live utterances
    refused(sess.make_decoder_group_io(s.tokens[:, :3], s.pos[0:3], s.cross, None, s.cap, kv, s.cap, l3, 0, cross_group=3), b"cross_group")      # 3 x 3 queries > 8
    torch.cuda.synchronize()
    assert bool((lg == 0).all()) and bool((l3 == 0).all()), "a refused call launched something"
    # wm_decoder_step_multi / wm_decoder_step_tap take a wm_decoder_io, which has no group size: a group cannot reach them
    assert not hasattr(native.WmDecoderIO, "cross_group")
    gio.cross_group, gio.io.live_rows = 0, None               # cross_group 0: wm_decoder_step itself -- and 9 rows on 3 rows of cross K/V are refused by the session
    with pytest.raises(native.WmError, match="cross"):
        sess.decoder_step(s.tokens[:, :1], s.pos[0:1], s.cross, None, s.cap, kv, s.cap, lg, 0, stream())


# ---------------------------------------------------------------------------------------------------------------- WhisperDecoding
def counting(dec):
    """Count the cross K/V projections of an instance (wm_cross_kv through the session)."""
    calls, real = [], dec.cross_attn_session.cross_kv

    def cross_kv(xa, outs, stream_):
        calls.append(tuple(xa.shape))
        return real(xa, outs, stream_)
    dec.cross_attn_session.cross_kv = cross_kv
    return calls


def cross_bytes(dec):
    st = next(iter(dec._state.values()))
    return sum(t.numel() * t.element_size() for t in st['cross'])


@pytest.mark.parametrize("kind", ["fp16", "int8"])
@pytest.mark.parametrize("K", [5, 3])
def test_shared_beam_loop_equals_the_literal_loop(engines, kind, K):
    """tests/test_gpu_beam.py::test_device_beam_loop_equals_literal_loop on a shared instance: the literal BeamSearchDecoder loop (whose
    own run must separate its candidates by twice the sum bound) gives the candidates, sums and texts of the device loop on one copy
    of the cross K/V -- eager and replayed; the language pass over the shared buffers detects what the unshared one does; one cross K/V
    projection per encoder output; 1 / K of the cross bytes."""
    plain, out, ref, stats = BM.run_both(engines, kind, K, 3)
    assert stats["min_gap"] >= 2 * BM.LOOP_TOL and stats["reorders"] > 0, stats
    eng = engines[kind]
    enc = WhisperEncoding(eng)
    dec = WhisperDecoding(eng, options=DecodingOptions(beam_size=K, sample_len=24), shared_cross_kv=True)
    calls = counting(dec)
    xa = enc.get_audio_features(engines["mel"][:3].cuda())
    languages, probs = dec.detect_language(xa)
    want_languages, want_probs = plain.detect_language(xa)
    assert languages == want_languages
    for p, q in zip(probs, want_probs):
        assert set(p) == set(q) and max(abs(float(p[c]) - float(q[c])) for c in p) <= 1e-3
    for _ in range(2):
        t, lp, nsp = dec.main_loop(xa)
        BM.assert_same_candidates((BM.candidates(dec, t, lp), dec.post_process(t, lp, nsp, xa, languages), nsp), ref)
    assert calls == [(3, DIMS.n_audio_ctx, DIMS.n_audio_state)], calls
    assert len(dec._state) == 1 and cross_bytes(dec) * K == cross_bytes(plain)
    plain._state.clear()


@pytest.mark.parametrize("n_audio,M", [(3, 3), (81, 2)])
def test_shared_best_of_draws_the_unshared_tokens(engines, n_audio, M):
    """best_of at temperature 0.7 under the same seed: the shared instance samples the tokens of the unshared one.  Both cut the key
    range alike here -- 3 x 3 rows: four pieces each; 81 x 2: the single pass each -- so the logits the draws see are the same bits."""
    eng = engines["fp16"]
    enc = WhisperEncoding(eng)
    xa = enc.get_audio_features(synthetic_mel(n_audio, W, DIMS.n_mels, 31).cuda())
    outs = []
    for shared in (False, True):
        dec = WhisperDecoding(eng, options=DecodingOptions(best_of=M, temperature=0.7, sample_len=8, language="en"), shared_cross_kv=shared)
        if n_audio > 3:
            dec.micro_batches = 1                            # one group of 162 rows: 324 / 162 (row or utterance, head) pairs, above the 160 both
        runs = []
        for _ in range(2):                                   # eager, then the replayed graphs
            torch.manual_seed(123)
            t, lp, nsp = dec.main_loop(xa)
            runs.append((t.cpu(), lp.cpu()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        res = dec.post_process(t, lp, nsp, xa, ["en"] * n_audio)
        outs.append((runs[0], [r.tokens for r in res], cross_bytes(dec)))
        dec._state.clear()
    (t0, lp0), picked0, bytes0 = outs[0]
    (t1, lp1), picked1, bytes1 = outs[1]
    assert torch.equal(t0, t1) and torch.equal(lp0, lp1) and picked0 == picked1
    assert bytes1 * M == bytes0
    rows = t0.reshape(n_audio, M, -1)
    assert any(not torch.equal(rows[a, 0], rows[a, 1]) for a in range(n_audio)), "the samples of an utterance must differ somewhere"


def torch_alignment(eng, xa, results, frames):
    sd = synthetic_state_dict(DIMS, 3)
    model = TM.Whisper(TM.ModelDimensions(**DIMS.to_dict())).load_state_dict({k: v.float() for k, v in sd.items()})
    ref_dec = WhisperDecoding(eng, only_torch=True)
    return ref_dec.torch_word_timestamps(model, xa.float().cpu(), results, frames), ref_dec.last_alignment


def test_recipe_on_one_instance_one_projection_and_word_timestamps(stock):
    """beam_size = 3, fallback_best_of = 2 on the stock engine: language pass, beam call, sampling call (closed rows end at once and are
    never ranked) and word_timestamps run on ONE cross K/V projection and one buffer set.  The words of the beam winners are the
    PyTorch alignment's (tests/test_gpu_word_timestamps.py: words and tokens always, probabilities within the logit bound, times and
    paths where the reference path is unambiguous) and exactly those of a greedy instance's device pass over the same tokens."""
    eng, enc = stock[0], stock[1]
    K, M, n = 3, 2, 2
    dec = WhisperDecoding(eng, options=DecodingOptions(beam_size=K), shared_cross_kv=True, fallback_best_of=M)
    dec.sample_len = 12
    dec.keep_alignment_matrix = True
    calls = counting(dec)
    xa = enc.get_audio_features(synthetic_mel(n, W, DIMS.n_mels, 77).cuda())
    languages, _ = dec.detect_language(xa)
    t, lp, nsp = dec.main_loop(xa, temperature=0.0)
    results = dec.post_process(t, lp, nsp, xa, languages, temperature=0.0)
    assert all(r.temperature == 0.0 and len(r.tokens) > 0 for r in results)
    torch.manual_seed(7)
    ts, lps, nsps = dec.main_loop(xa, temperature=0.4)
    eot = dec.tokenizer.eot
    rows = ts.reshape(n, K, -1)
    assert bool((rows[:, M:, dec.sample_begin:] == eot).all()) and bool((lps.reshape(n, K)[:, M:] == 0).all())
    assert bool((rows[:, :M, dec.sample_begin] != eot).all())
    sampled = dec.post_process(ts, lps, nsps, xa, languages, temperature=0.4)
    for a, r in enumerate(sampled):
        live = [x[dec.sample_begin:].tolist() for x in rows[a, :M]]
        assert r.temperature == 0.4 and r.tokens in [x[:x.index(eot)] if eot in x else x for x in live] and len(r.tokens) > 0
    t2, lp2, _ = dec.main_loop(xa, temperature=0.0)           # the beam call again, after a sampling call on the same buffers
    assert torch.equal(t, t2) and torch.equal(lp, lp2)
    frames = [W, 2 * 45 + 1]
    words = dec.word_timestamps(xa, results, frames)
    dev = dec.last_alignment
    assert calls == [(n, DIMS.n_audio_ctx, DIMS.n_audio_state)], calls
    assert len(dec._state) == 1 and next(iter(dec._state)) == n * K
    t3, lp3, _ = dec.main_loop(xa, temperature=0.0)           # the forced pass leaves the loop's results reproducible
    assert torch.equal(t, t3) and torch.equal(lp, lp3) and calls == [(n, DIMS.n_audio_ctx, DIMS.n_audio_state)]
    assert any(len(w) > 0 for w in words)
    greedy = WhisperDecoding(eng)
    assert greedy.word_timestamps(xa, results, frames) == words
    ref, tor = torch_alignment(eng, xa, results, frames)
    n_prefix, compared = len(dec.tokenizer.sot_sequence), 0
    for b in range(n):
        assert [(w.word, w.tokens) for w in words[b]] == [(w.word, w.tokens) for w in ref[b]]
        if not words[b]:
            continue
        assert np.allclose([w.probability for w in words[b]], [w.probability for w in ref[b]], atol=LOGIT_TOL)
        S64, m32 = [s.double().numpy() for s in tor[b]["scores"]], tor[b]["matrix"].numpy()
        tot = np.zeros(S64[0].shape)
        for S in S64:                                         # the alignment matrix in float64 (tests/test_gpu_word_timestamps.py)
            e = np.exp(S - S.max(axis=1, keepdims=True))
            Wm = e / e.sum(axis=1, keepdims=True)
            mu, sdv = Wm.mean(0, keepdims=True), Wm.std(0, keepdims=True)
            Z = np.where(sdv > 0, (Wm - mu) / np.where(sdv > 0, sdv, 1), 0)
            if Z.shape[1] > 3:
                Z = np.sort(np.lib.stride_tricks.sliding_window_view(np.pad(Z, ((0, 0), (3, 3)), mode="reflect"), 7, axis=1), axis=-1)[..., 3]
            tot += Z
        m64 = (tot / len(S64))[n_prefix: tot.shape[0] - 1]
        bound, margin = 4 * float(np.abs(m32 - m64).max()), dtw_margin(-m32, tor[b]["path_text"], tor[b]["path_time"])
        k = dev["path_len"][b]
        print(f"beam winner {b}: matrix bound {bound:.3g}, smallest DTW margin on the reference path {margin:.3g}")
        if margin > 2 * bound:
            assert [(w.start, w.end) for w in words[b]] == [(w.start, w.end) for w in ref[b]]
            assert dev["path_text"][b, :k].tolist() == tor[b]["path_text"].tolist() and dev["path_time"][b, :k].tolist() == tor[b]["path_time"].tolist()
            compared += 1
    assert compared >= 1


def test_word_timestamps_stay_refused_where_they_were(stock):
    eng, enc, eng8 = stock[:3]
    xa = enc.get_audio_features(synthetic_mel(2, W, DIMS.n_mels, 77).cuda())
    with pytest.raises(ValueError, match="beam_size"):
        WhisperDecoding(eng, options=DecodingOptions(beam_size=2, sample_len=4)).word_timestamps(xa, [[440, 7], [9001]])
    dec8 = WhisperDecoding(eng8, options=DecodingOptions(beam_size=2, sample_len=4), shared_cross_kv=True)
    with pytest.raises(native.WmError, match="int8"):
        dec8.word_timestamps(xa, [[440, 7], [9001]])
    t, lp, nsp = dec8.main_loop(xa)                           # ... while decoding on shared int8 cross K/V works
    assert len(dec8.post_process(t, lp, nsp, xa, ["en"] * 2)) == 2


# ------------------------------------------------------------------------------------------------------------------- transcribe
def threshold_for_a_fallback(run):
    """A logprob_threshold under which at least one window of the run falls back and at least one does not: between the two lowest
    distinct avg_logprob values the temperature-0 calls of a run WITHOUT thresholds gave (`run(**thresholds)` -> trace).  The choice
    of the fixture's threshold, not a tolerance: nothing is compared against it."""
    run(compression_ratio_threshold=None, logprob_threshold=0.0, no_speech_threshold=None)      # every window down the whole ladder: every call's graphs exist from here on
    trace = run(compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None)
    values = sorted({r.avg_logprob for e in trace if e.get("kind") != "align" and e["temperature"] == 0.0
                     for r, on in zip(e["results"], e["live"]) if on and len(r.tokens) > 0})
    assert len(values) >= 2, values
    return dict(compression_ratio_threshold=None, logprob_threshold=(values[0] + values[1]) / 2, no_speech_threshold=None)


def recipe(eng, **kw):
    dec = WhisperDecoding(eng, options=DecodingOptions(beam_size=2, language="en"), shared_cross_kv=True, fallback_best_of=2, **kw)
    dec.sample_len = 12
    return dec


def check_fallback(results, decodes):
    temps = {s["temperature"] for r in results for s in r["segments"]}
    assert 0.0 in temps and max(temps) > 0.0, temps
    final = {}
    for e in decodes:
        for r, on in zip(e["rows"], e["live"]):
            if on:
                final[r] = e["temperature"]                   # the calls of a window come in ladder order: the last one settles it
    for f, res in enumerate(results):
        for s in res["segments"]:
            assert s["temperature"] == final[(f, s["seek"])]
    assert all(e["temperature"] in LF.TEMPERATURES for e in decodes) and {e["temperature"] for e in decodes} >= {0.0, 0.2}


def test_transcribe_full_ladder_with_words_on_the_recipe(stock):
    """transcribe_mel, beam_size = 2 and fallback_best_of = 2, the full ladder, word_timestamps: the run is the literal loop's per file
    (test_gpu_word_longform.run_words replays trace and alignments through longform.transcribe_reference), a window that falls back
    reports the temperature that settled it, the others 0; one buffer set of n_rows x 2 rows."""
    eng, enc = stock[0], stock[1]
    mels = [synthetic_mel(1, c + W, DIMS.n_mels, 900 + i)[0].cuda().contiguous() for i, c in enumerate(WL.CONTENTS)]
    dec = recipe(eng)

    def plain_run(**th):
        trace = []
        T.transcribe_mel(enc, dec, mels, WL.CONTENTS, n_rows=3, trace=trace, temperatures=LF.TEMPERATURES, word_timestamps=True, **th)
        return trace
    th = threshold_for_a_fallback(plain_run)
    torch.manual_seed(3)
    results, trace, decodes, aligns = WL.run_words(enc, dec, mels, 3, temperatures=LF.TEMPERATURES, **th)
    check_fallback(results, decodes)
    WL.replay_alignments(enc, dec, decodes, aligns)
    assert len(dec._state) == 1 and next(iter(dec._state)) == 3 * 2


def test_transcribe_recipe_with_row_prompts(stock):
    eng, enc = stock[0], stock[1]
    mels = [synthetic_mel(1, c + W, DIMS.n_mels, 900 + i)[0].cuda().contiguous() for i, c in enumerate(WL.CONTENTS)]
    dec = recipe(eng, row_prompts=True)
    dec.sample_len = 6
    kw = dict(temperatures=LF.TEMPERATURES, condition_on_previous_text=True, initial_prompt=[1500, 1501])

    def plain_run(**th):
        trace = []
        T.transcribe_mel(enc, dec, mels, WL.CONTENTS, n_rows=3, trace=trace, word_timestamps=True, **kw, **th)
        return trace
    th = threshold_for_a_fallback(plain_run)
    torch.manual_seed(3)
    results, trace, decodes, aligns = WL.run_words(enc, dec, mels, 3, **kw, **th)
    check_fallback(results, decodes)
    assert any(len(p) > 2 for e in decodes for p in e["prompts"]), "no window was conditioned on previous text"


def test_transcribe_recipe_with_sections(stock):
    eng, enc = stock[0], stock[1]
    mels = [synthetic_mel(1, c + W, DIMS.n_mels, 700 + i)[0].cuda().half().contiguous() for i, c in enumerate(SEC.CONTENTS)]
    dec = recipe(eng)

    def plain_run(**th):
        trace = []
        T.transcribe_mel(enc, dec, mels, SEC.CONTENTS, n_rows=SEC.N_ROWS, trace=trace, sections=SEC.OPTS, temperatures=LF.TEMPERATURES,
                         word_timestamps=True, **th)
        return trace
    th = threshold_for_a_fallback(plain_run)
    kw = dict(temperatures=LF.TEMPERATURES, word_timestamps=True, **th)
    results, trace, reference, ref_trace, layout = SEC.run_both(enc, dec, DIMS, mels, **kw)
    decodes = SEC.compare_with_reference(DIMS, results, trace, reference, ref_trace, layout)
    temps = {s["temperature"] for r in results for s in r["segments"]}
    assert 0.0 in temps and max(temps) > 0.0, temps
