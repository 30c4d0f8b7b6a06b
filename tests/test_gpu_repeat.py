"""Repetition penalty and no-repeat n-grams on a real MI355X: wm_repeat_controls (csrc/repeat.hip) through the C entry, bit for bit
against the brute force of tests/repeat_refs.py, and the controls inside every device loop -- greedy, beam, sampling, per-row prompts,
long-form -- against the literal loops, whose filters the CPU tests (tests/test_repeat_cpu.py) hold to the same brute force.

Model seed 3 / mel seed 41 of the property test were picked on the CPU torch path (tests/test_repeat_cpu.py): with the controls off
every row repeats text tokens."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import longform as LF  # noqa: E402
import native  # noqa: E402
import synthetic  # noqa: E402
import test_gpu_beam as BM  # noqa: E402  (helpers only)
import transcribe as T  # noqa: E402
from decoding import DecodingOptions, WhisperDecoding  # noqa: E402
from encoding import WhisperEncoding  # noqa: E402
from oracle.whisper_oracle import Dims, synthetic_mel  # noqa: E402
from repeat_refs import controls_batch, has_repeated_ngram  # noqa: E402
from test_gpu_beam import engines  # noqa: E402,F401  (module fixture: the peaked fp16 / int8 engines and four clips)
from test_gpu_decode_loop import CASES as LOOP_CASES  # noqa: E402
from test_gpu_model import build_engine  # noqa: E402

DIMS = Dims(**synthetic.DIMS["micro-fullvocab"])
W = 2 * DIMS.n_audio_ctx
MODEL_SEED, MEL_SEED = 3, 41
SENTINEL = 0x7a5a                    # a finite fp16 pattern no case produces
BOUND = 512                          # WM_REPEAT_MAX_HISTORY


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return native.load_library()


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------ the kernel alone
def histories(rng, batch, m, eot, V):
    """Row b by b % 4: 0 a six-token alphabet (EOT and a timestamp in it), 1 ONE token throughout (every lane owns the same logit:
    the race the ownership rule exists for), 2 all distinct text tokens, 3 a phrase of seven over and over, a timestamp in it."""
    H = np.zeros((batch, m), dtype=np.int64)
    for b in range(batch):
        kind = b % 4
        if kind == 0:
            H[b] = rng.choice(np.array([1, 2, 3, eot - 1, eot, V - 2]), size=m)
        elif kind == 1:
            H[b] = int(rng.integers(0, eot))
        elif kind == 2:
            H[b] = rng.permutation(eot)[:m]
        else:
            phrase = np.concatenate([rng.integers(0, eot, size=6), [V - 1]])
            H[b] = np.resize(phrase, m)
    return H


def run_kernel(lib, logits_buf, first, stride, batch, V, tokens, ld, cur_len, sample_begin, eot, p, n, done=None, counter=False):
    io = native.WmRepeatIO()
    io.logits, io.row_stride = logits_buf.data_ptr() + 2 * first, stride
    io.batch, io.n_vocab = batch, V
    io.tokens, io.tokens_ld = tokens.data_ptr(), ld
    keep = None
    if counter:
        keep = torch.tensor([cur_len - 1], dtype=torch.int32, device="cuda")
        io.cur_len, io.n_past_dev = 0, keep.data_ptr()
    else:
        io.cur_len = cur_len
    io.sample_begin, io.eot = sample_begin, eot
    io.repetition_penalty, io.no_repeat_ngram_size = p, n
    io.done = done.data_ptr() if done is not None else None
    rc = lib.wm_repeat_controls(C.byref(io), stream())
    torch.cuda.synchronize()
    return rc


SPECIAL = [0.0, -0.0, 5.96e-8, -5.96e-8, 65504.0, -65504.0, -np.inf, 1.0]


KERNEL_CONTROLS = [(1.3, 0), (1.0, 3), (1.2, 2), (0.5, 1), (4.0, 5)]
FIRST, GUARD, LD, SAMPLE_BEGIN = 3, 64, 449, 2


def kernel_case(rng, V, pad, batch, k, m):
    """Case k of a parametrisation, on the host: the buffer handed to the kernel (sentinels around the rows and in their padding), the
    buffer wanted, the token rows, the `done` flags and the controls."""
    eot = 1000 if V == 1024 else 50257
    stride = V + pad
    p, n = KERNEL_CONTROLS[k % len(KERNEL_CONTROLS)]
    cur_len = SAMPLE_BEGIN + m
    H = histories(rng, batch, m, eot, V)
    tokens = np.full((batch, LD), 1, dtype=np.int64)                  # text token 1 everywhere else: before sample_begin, behind cur_len
    tokens[:, SAMPLE_BEGIN:cur_len] = H
    logits = (rng.standard_normal((batch, V)) * 4).astype(np.float16)
    for b in range(batch):                                            # every other token of H: zeros, subnormals, the largest values, -inf
        for i, t in enumerate(np.unique(H[b])[1::2][:len(SPECIAL)]):
            logits[b, t] = np.float16(SPECIAL[(i + b) % len(SPECIAL)])
    done = (rng.random(batch) < 0.3).astype(np.int32) if batch > 1 else np.zeros(1, dtype=np.int32)
    want_rows = controls_batch(logits, tokens, SAMPLE_BEGIN, cur_len, eot, p, n, done=done)
    if m >= 63 and not done.all():
        assert not np.array_equal(want_rows.view(np.uint16), logits.view(np.uint16)), "the case exercises nothing"
    buf = np.full(FIRST + GUARD + batch * stride + GUARD, SENTINEL, dtype=np.uint16)
    want = buf.copy()
    for b in range(batch):
        lo = FIRST + GUARD + b * stride
        buf[lo:lo + V] = logits[b].view(np.uint16)
        want[lo:lo + V] = want_rows[b].view(np.uint16)
    return buf, want, tokens.astype(np.int32), done, eot, cur_len, p, n


def kernel_lengths(batch):
    return [0, 1, 2, 63, 64, 65, 223, 447] if batch <= 3 else [0, 65, 447]


@pytest.mark.parametrize("batch", [1, 3, 70])
@pytest.mark.parametrize("V,pad", [(1024, 0), (1024, 37), (51865, 0), (51865, 11)])
def test_kernel_equals_the_brute_force_bit_for_bit(lib, V, pad, batch):
    """Sentinel guard bands in front of the logits, behind them and in every row's padding; rows at odd 2-byte offsets (stride
    V + pad, a first row 3 elements into the buffer); the start sequence and the slots behind cur_len hold text tokens that must not
    count; both ways of giving cur_len; `done` rows untouched."""
    rng = np.random.default_rng(V + 7 * pad + batch)
    for k, m in enumerate(kernel_lengths(batch)):
        buf, want, tokens, done, eot, cur_len, p, n = kernel_case(rng, V, pad, batch, k, m)
        dev = torch.from_numpy(buf.view(np.int16)).cuda()
        tok_dev = torch.from_numpy(tokens).cuda()
        rc = run_kernel(lib, dev, FIRST + GUARD, V + pad, batch, V, tok_dev, LD, cur_len, SAMPLE_BEGIN, eot, p, n,
                        done=torch.from_numpy(done).cuda(), counter=bool(k % 2))
        assert rc == 0, lib.wm_last_error().decode()
        got = dev.cpu().numpy().view(np.uint16)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (V, pad, batch, m, p, n, bad[:8], got[bad[:8]], want[bad[:8]])
        assert np.array_equal(tok_dev.cpu().numpy(), tokens)


def test_penalty_and_ban_on_one_token_and_both_off(lib):
    V, eot, ld = 1024, 1000, 64
    logits = torch.full((2, V), 2.0, dtype=torch.float16, device="cuda")
    tokens = torch.zeros((2, ld), dtype=torch.int32, device="cuda")
    tokens[:, 3:6] = torch.tensor([7, 11, 7], dtype=torch.int32)
    before = logits.clone()
    assert run_kernel(lib, logits, 0, V, 2, V, tokens, ld, 6, 3, eot, 1.0, 0) == 0
    assert torch.equal(logits.view(torch.int16), before.view(torch.int16))                     # both off: every bit stays
    assert run_kernel(lib, logits, 0, V, 2, V, tokens, ld, 6, 3, eot, 1.3, 2) == 0
    want = np.full(V, 2.0, dtype=np.float16)
    want[7] = np.float16(np.float32(2.0) / np.float32(1.3))
    want[11] = -np.inf                                                                        # penalised, then banned: -inf wins
    assert np.array_equal(logits.cpu().numpy().view(np.uint16), np.stack([want, want]).view(np.uint16))


def test_kernel_refusals(lib):
    V, eot, ld = 1024, 1000, 700
    logits = torch.zeros((1, V), dtype=torch.float16, device="cuda")
    tokens = torch.zeros((1, ld), dtype=torch.int32, device="cuda")

    def call(**kw):
        a = dict(logits_buf=logits, first=0, stride=V, batch=1, V=V, tokens=tokens, ld=ld, cur_len=10, sample_begin=3, eot=eot, p=1.2, n=2)
        a.update(kw)
        return run_kernel(lib, **a)

    assert call() == 0 and call(cur_len=3 + BOUND) == 0                                        # m = the bound: taken
    assert call(counter=True, ld=3 + BOUND) == 0                                               # a device counter: tokens_ld bounds m
    before = logits.clone()
    for bad in (dict(cur_len=3 + BOUND + 1), dict(counter=True), dict(p=0.0), dict(p=-1.0), dict(p=float("nan")), dict(p=float("inf")),
                dict(n=-1), dict(cur_len=2), dict(cur_len=ld + 1), dict(eot=V + 1), dict(batch=0)):
        assert call(**bad) == 1, bad
        assert "wm_repeat_controls" in lib.wm_last_error().decode(), bad
    io = native.WmRepeatIO()
    assert lib.wm_repeat_controls(None, stream()) == 1 and "null" in lib.wm_last_error().decode()
    assert lib.wm_repeat_controls(C.byref(io), stream()) == 1 and "null" in lib.wm_last_error().decode()
    io.logits, io.batch, io.n_vocab, io.repetition_penalty = logits.data_ptr(), 1, V, 1.2
    assert lib.wm_repeat_controls(C.byref(io), stream()) == 1 and "null" in lib.wm_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(logits.view(torch.int16), before.view(torch.int16))                     # refused: nothing was launched


# ------------------------------------------------------------------------------------------------------------ the engine loops
@pytest.fixture(scope="module")
def stock(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    eng = build_engine(str(tmp_path_factory.mktemp("repeat_engines")), "micro-fullvocab", MODEL_SEED)
    enc = WhisperEncoding(eng)
    return eng, enc, enc.get_audio_features(synthetic_mel(3, W, DIMS.n_mels, MEL_SEED).cuda())


def sampled_text(dec, tokens):
    return [[t for t in row[dec.sample_begin:].tolist() if t < dec.tokenizer.eot] for row in tokens.cpu()]


@pytest.mark.parametrize("p,n", [(1.3, 0), (1.0, 3), (1.2, 2)])
def test_device_loop_equals_the_literal_loop_and_its_three_phases_agree(stock, p, n):
    eng, enc, xa = stock
    dec = WhisperDecoding(eng, options=DecodingOptions(sample_len=24, language="en", repetition_penalty=p, no_repeat_ngram_size=n))
    base = WhisperDecoding(eng, options=DecodingOptions(sample_len=24, language="en"))
    t_fast, lp_fast, nsp_fast = dec.main_loop(xa)
    assert set(dec._state[3]['graphs']) == LOOP_CASES["one_group"]["keys"]                  # the options change no graph key
    t_ref, lp_ref, nsp_ref = dec.main_loop_reference(xa)
    assert torch.equal(t_fast.cpu(), t_ref.cpu())
    assert torch.allclose(lp_fast.cpu(), lp_ref.cpu(), atol=2e-3)
    assert np.allclose(nsp_fast, nsp_ref, atol=1e-4)
    t_off, _, _ = base.main_loop(xa)
    assert not torch.equal(t_off.cpu(), t_fast.cpu()), "the controls changed nothing: the comparison shows nothing"
    base._state.clear()
    # eager + capture, replay, no graphs: the same bits (the pattern of tests/test_gpu_decode_loop.py), here for sample_len steps
    runs = []
    for phase, use_graphs in (("eager + capture", True), ("replay", True), ("no graphs", False)):
        dec.use_graphs = use_graphs
        t, lp, _ = dec.main_loop(xa, ignore_eot=True)
        torch.cuda.synchronize()
        runs.append((phase, t.cpu(), lp.cpu(), [c.clone() for c in dec._state[3]['kv']]))
    _, t0, lp0, kv0 = runs[0]
    assert t0.shape == (3, dec.sample_begin + 24)
    for phase, t, lp, kv in runs[1:]:
        assert torch.equal(t, t0) and torch.equal(lp, lp0), phase
        for layer, (a, b) in enumerate(zip(kv, kv0)):
            assert torch.equal(a, b), (phase, layer)
    if n:
        assert not any(has_repeated_ngram(row[dec.sample_begin:].tolist(), n, dec.tokenizer.eot) for row in t0)
    dec._state.clear()


def test_unigram_bans_no_text_token_twice_on_the_device_loop(stock):
    eng, enc, xa = stock
    texts = {}
    for n in (0, 1):
        dec = WhisperDecoding(eng, options=DecodingOptions(sample_len=24, language="en", no_repeat_ngram_size=n))
        for _ in range(2):                                       # eager, then the replayed graphs
            t, lp, _ = dec.main_loop(xa, ignore_eot=True)
            assert t.shape == (3, dec.sample_begin + 24) and torch.isfinite(lp).all()
            texts.setdefault(n, []).append(sampled_text(dec, t))
        dec._state.clear()
    assert any(len(r) > len(set(r)) for r in texts[0][0]), "the baseline no longer repeats: pick other seeds (tests/test_repeat_cpu.py)"
    assert texts[1][0] == texts[1][1]
    assert all(len(r) == len(set(r)) and len(r) >= 8 for r in texts[1][0]), texts[1][0]


@pytest.mark.parametrize("shared", [False, True])
def test_beam_loop_with_the_controls_equals_the_literal_loop(engines, shared):
    K, n = 3, 2
    eng = engines["fp16"]
    enc = WhisperEncoding(eng)
    opts = DecodingOptions(beam_size=K, sample_len=24, repetition_penalty=1.2, no_repeat_ngram_size=n)
    dec = WhisperDecoding(eng, options=opts, shared_cross_kv=shared)
    xa = enc.get_audio_features(engines["mel"][:3].cuda())
    languages, _ = dec.detect_language(xa)
    out = []
    for _ in range(2):                                           # eager, then the replayed graphs
        t, lp, nsp = dec.main_loop(xa)
        out.append((BM.candidates(dec, t, lp), dec.post_process(t, lp, nsp, xa, languages), nsp))
    lit = dec if not shared else WhisperDecoding(eng, options=opts)
    if shared:
        lit.detect_language(xa)
    t, lp, nsp = lit.main_loop_reference(xa)
    ref = (BM.candidates(lit, t, lp), lit.post_process(t, lp, nsp, xa, languages), nsp)
    for got in out:
        BM.assert_same_candidates(got, ref)
    eot = dec.tokenizer.eot
    n_cands = 0
    for cands in ref[0][0]:
        for seq in cands:
            n_cands += 1
            assert not has_repeated_ngram(seq[dec.sample_begin:], n, eot), seq
    assert n_cands >= 3 * K
    plain = WhisperDecoding(eng, options=DecodingOptions(beam_size=K, sample_len=24))
    plain.detect_language(xa)
    t, lp, _ = plain.main_loop(xa)
    assert BM.candidates(plain, t, lp)[0] != ref[0][0], "the controls changed no candidate: the comparison shows nothing"
    plain._state.clear()
    dec._state.clear()
    lit._state.clear()


def literal_sums(dec, xa, tokens):
    """The sampled rows teacher-forced through the literal step (decode() + the host filters, the controls first): per row the sum of
    log_softmax(filtered logits)[token] over its tokens up to and including the first EOT, and whether every token was allowed."""
    feats = xa.repeat_interleave(dec.n_group, dim=0) if tokens.shape[0] != xa.shape[0] else xa
    cross = dec.xa2cross_key_value(feats)
    L0, eot = dec.sample_begin, dec.tokenizer.eot
    sums = torch.zeros(tokens.shape[0], dtype=torch.float64)
    allowed, alive, kv = True, torch.ones(tokens.shape[0], dtype=torch.bool), None
    for cur in range(L0, tokens.shape[1]):
        feed = tokens[:, :cur] if cur == L0 else tokens[:, cur - 1:cur]
        logits, kv = dec.decode(feed.cuda(), cross, kv)
        logits = logits[:, -1]
        for f in dec.logit_filters:
            f.apply(logits, tokens[:, :cur].cuda())
        lp = torch.log_softmax(logits.float(), dim=-1).cpu()
        step = lp[torch.arange(tokens.shape[0]), tokens[:, cur]]
        allowed = allowed and bool(torch.isfinite(step[alive]).all())
        sums += torch.where(alive, step.double(), torch.zeros_like(step, dtype=torch.float64))
        alive = alive & (tokens[:, cur] != eot)
    return sums.float(), allowed


def test_sampling_loop_with_the_controls_books_the_literal_log_probabilities(stock):
    """temperature 0.7, best_of 2, n = 2: the draws are the device generator's (a Gumbel-max, tests/test_gpu_round4.py), so the rows are
    held to what those tests hold them to -- repeatable under torch.manual_seed, every sampled token allowed by the filtered
    distribution, and the booked sums those of log_softmax(filtered logits) -- with the controls among the filters."""
    eng, enc, xa = stock
    dec = WhisperDecoding(eng, options=DecodingOptions(sample_len=24, language="en", temperature=0.7, best_of=2, repetition_penalty=1.2,
                                                       no_repeat_ngram_size=2))
    runs = []
    for _ in range(2):
        torch.manual_seed(1234)
        t, lp, nsp = dec.main_loop(xa)
        runs.append((t.cpu(), lp.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    t, lp = runs[0]
    assert t.shape[0] == 6 and any(not torch.equal(t[2 * a], t[2 * a + 1]) for a in range(3))
    eot = dec.tokenizer.eot
    for row in t:
        seq = row[dec.sample_begin:].tolist()
        end = seq.index(eot) if eot in seq else len(seq)
        assert not has_repeated_ngram(seq[:end], 2, eot), seq
    want, allowed = literal_sums(dec, xa, t)
    assert allowed, "a sampled token had probability 0 under the literal filters"
    assert torch.allclose(lp, want, atol=2e-3), (lp, want)
    res = dec.post_process(runs[0][0], runs[0][1], nsp, xa, ["en"] * 3)
    assert len(res) == 3 and all(np.isfinite(r.avg_logprob) for r in res)
    dec._state.clear()


def test_row_prompts_are_not_part_of_the_history(stock):
    eng, enc, xa = stock
    probe = WhisperDecoding(eng, options=DecodingOptions(sample_len=24, language="en"))
    t, _, _ = probe.main_loop(xa, ignore_eot=True)
    probe._state.clear()
    prompts = []
    for r in sampled_text(probe, t):                              # every row's prompt: the tokens its un-controlled run repeats, and more
        repeated = [x for x in dict.fromkeys(r) if r.count(x) > 1]
        assert repeated
        prompts.append((repeated * 8)[:40] + r[:20])
    opts = dict(sample_len=24, language="en")
    off = WhisperDecoding(eng, row_prompts=True, options=DecodingOptions(**opts))
    on = WhisperDecoding(eng, row_prompts=True, options=DecodingOptions(repetition_penalty=1.3, no_repeat_ngram_size=1, **opts))
    L0, V = on.sample_begin, DIMS.n_vocab
    assert L0 == DIMS.n_text_ctx // 2 + 3 == off.sample_begin
    got = {}
    for name, dec in (("off", off), ("on", on)):
        dec.set_prompts(prompts)
        dec.sample_len = 2
        t, lp, _ = dec.main_loop(xa, ignore_eot=True)
        torch.cuda.synchronize()
        lg = dec._state[3]['logits']
        # after two steps: rows [0, 3) x V at the buffer's start hold the second step's filtered logits (H = one timestamp: the controls
        # may change nothing), the last position of the prefill block the first step's (m = 0)
        got[name] = (t.cpu(), lp.cpu(), lg.reshape(-1)[:3 * V].clone().view(torch.int16).cpu(), lg[:, L0 - 1].clone().view(torch.int16).cpu())
    assert got["on"][0][:, L0].tolist() == got["off"][0][:, L0].tolist() and (got["on"][0][:, L0] >= on.tokenizer.timestamp_begin).all()
    assert torch.equal(got["on"][3], got["off"][3]), "m = 0: the first step's logits must keep their bits whatever the prompt holds"
    assert torch.equal(got["on"][2], got["off"][2]), "the prompt's tokens were counted"
    assert torch.equal(got["on"][0], got["off"][0]) and torch.equal(got["on"][1], got["off"][1])
    # and over a whole row: no text token twice among the SAMPLED tokens, though the prompt holds the row's favourites
    on.sample_len = 24
    for _ in range(2):
        t, _, _ = on.main_loop(xa, ignore_eot=True)
        rows = sampled_text(on, t)
        assert all(len(r) == len(set(r)) and len(r) >= 8 for r in rows), rows
    off._state.clear()
    on._state.clear()


def test_long_form_with_the_controls_equals_the_literal_schedule(stock):
    """transcribe_mel over two short files with the controls on: the segments are those of longform.transcribe_reference replayed on
    the recorded decoder results, and every temperature-0 call again through the public path gives the same tokens."""
    eng, enc, _ = stock
    contents = [100, 300]
    mels = [synthetic_mel(1, c + W, DIMS.n_mels, 900 + i)[0].cuda().contiguous() for i, c in enumerate(contents)]
    dec = WhisperDecoding(eng, options=DecodingOptions(language="en", repetition_penalty=1.2, no_repeat_ngram_size=3))
    dec.sample_len = 12
    calls = []
    real = dec._repeat_controls
    dec._repeat_controls = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    trace = []
    kw = dict(temperatures=(0.0, 0.4), compression_ratio_threshold=None, logprob_threshold=-1.0, no_speech_threshold=None)
    results = T.transcribe_mel(enc, dec, mels, contents, n_rows=2, trace=trace, **kw)
    assert calls and len(results) == 2 and all(r["segments"] for r in results)
    tk = dec.tokenizer
    recorded = {}
    for e in trace:
        for r, live, res in zip(e["rows"], e["live"], e["results"]):
            if live:
                recorded[(r[0], r[1], e["temperature"])] = res
    for f, c in enumerate(contents):
        want = LF.transcribe_reference(lambda seek, temperature, f=f: recorded[(f, seek, temperature)], c, window=W,
                                       timestamp_begin=tk.timestamp_begin, decode_text=tk.decode, **kw)
        assert results[f]["segments"] == want, f
        assert all(not has_repeated_ngram(s["tokens"], 3, tk.eot) for s in want)
    n_zero = 0
    for e in trace:
        if e["temperature"] != 0.0:
            continue
        n_zero += 1
        xa = enc.get_audio_features(e["windows"].cuda())
        if e["language_tokens"] is not None:
            dec.set_language_tokens(e["language_tokens"])
        tokens, sums, nsp = dec.main_loop(xa, row_limit=e["row_limit"])
        again = dec.post_process(tokens, sums, nsp, xa, e["languages"])
        for i, live in enumerate(e["live"]):
            assert again[i].tokens == (e["results"][i].tokens if live else []), (e["round"], i)
            assert not has_repeated_ngram(again[i].tokens, 3, tk.eot)
    assert n_zero >= 2
    dec._state.clear()


def test_defaults_never_reach_the_controls(stock, monkeypatch):
    """repetition_penalty = 1, no_repeat_ngram_size = 0: _repeat_controls is never called -- greedy, beam and a long-form round -- and
    the graph keys after a call are what tests/test_gpu_decode_loop.py expects."""
    eng, enc, xa = stock

    def boom(*a, **k):
        raise AssertionError("_repeat_controls called with the controls off")
    monkeypatch.setattr(WhisperDecoding, "_repeat_controls", boom)
    xa2 = enc.get_audio_features(synthetic_mel(2, W, DIMS.n_mels, 41).cuda())
    for case in ("one_group", "beam"):
        dec = WhisperDecoding(eng, options=DecodingOptions(sample_len=6, language="en", **LOOP_CASES[case]["options"]))
        assert not dec.repeat_controls_on
        for _ in range(2):
            dec.main_loop(xa2)
        assert set(dec._state[2 * dec.n_group]['graphs']) == LOOP_CASES[case]["keys"]
        dec._state.clear()
    dec = WhisperDecoding(eng, options=DecodingOptions(language="en"))
    dec.sample_len = 12
    mels = [synthetic_mel(1, 100 + W, DIMS.n_mels, 900)[0].cuda().contiguous()]
    results = T.transcribe_mel(enc, dec, mels, [100], n_rows=1, temperatures=(0.0,), compression_ratio_threshold=None, logprob_threshold=None,
                               no_speech_threshold=None)
    assert results[0]["segments"]
    dec._state.clear()
    on = WhisperDecoding(eng, options=DecodingOptions(sample_len=6, language="en", no_repeat_ngram_size=2))
    with pytest.raises(AssertionError, match="controls off"):      # (the patch does catch a call)
        on.main_loop(xa2)
    torch.cuda.synchronize()
    on._state.clear()
