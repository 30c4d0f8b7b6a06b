"""Speculative decoding through the engine (speculative_loop.py): `WhisperDecoding(draft_engine_dir=...)`.

Replay: the device loop's trace, replayed by a test-side loop on its own buffers with sequential wm_greedy_step calls, gives the
same tokens and sums exactly.  Lossless up to margin: every sampled token is the one the host rules (oracle/decoding_rules.py)
choose from the main engine's own logits, computed alone in 4-token passes from an empty cache -- or, at no more than one position
in ten, lies within twice the decoder's documented logit bound of it (the `micro-v3` decoder row: 3e-2 with an
fp16 cache, 6e-2 with int8 KV).  The seeds are ones for which the plain loop of the same engine, checked the same way, needs no such
excuse: chosen with the CPU oracle (oracle/whisper_oracle.py + decoding_rules.py) among model seeds 3-14 and clip seeds 41-46 as those
whose greedy path of 12 tokens over three clips keeps the two best allowed logits at least 0.03 apart at every position and the
text-versus-timestamp decision at least 0.06 from its threshold -- the synthetic models' logits are nearly flat (top-2 gaps of one
fp16 ulp are common), so most seeds have a position that a 4-token pass and a 1-token step decide differently."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import native  # noqa: E402
import synthetic  # noqa: E402
import transcribe as T  # noqa: E402
from decoding import DecodingOptions, WhisperDecoding  # noqa: E402
from encoding import WhisperEncoding  # noqa: E402
from oracle import decoding_rules as DR  # noqa: E402
from oracle.whisper_oracle import Dims, synthetic_mel  # noqa: E402
from test_gpu_model import build_engine  # noqa: E402

# (model seed, clip seed) per engine variant: oracle top-2 gap / decision margin along the greedy path 0.047 / 0.35, 0.051 / 0.078, 0.066 / 0.45, 0.047 / 0.44
SEEDS = {("micro-fullvocab", "fp16"): (7, 45), ("micro-fullvocab", "int8"): (12, 46), ("micro-v3", "fp16"): (4, 42), ("micro-v3", "int8"): (4, 42)}
MODEL_SEED, DRAFT_SEED = 4, 99
SAMPLE_LEN = 12
LOGIT_BOUND = {"fp16": 3e-2, "int8": 6e-2}       # DESIGN.md section 5n, decoder on `micro-v3`: fp16 cache / int8 KV
IDS = {"micro-fullvocab": DR.MULTILINGUAL, "micro-v3": DR.SpecialIds(50257, n_langs=100)}


@pytest.fixture(scope="module")
def engines(tmp_path_factory):
    """Per model: the main engine in fp16 and in weight-only int8 + int8 KV (each at its seed of SEEDS), a draft from another seed (a
    directory of its own: the engine's path does not carry the seed), and each engine's encoder features of its three clips."""
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    main_dir, draft_dir = str(tmp_path_factory.mktemp("spec_main")), str(tmp_path_factory.mktemp("spec_draft"))
    out = {}
    for model in ("micro-fullvocab", "micro-v3"):
        dims = Dims(**synthetic.DIMS[model])
        fp16 = build_engine(main_dir, model, SEEDS[model, "fp16"][0])
        int8 = build_engine(main_dir, model, SEEDS[model, "int8"][0], weight_only=True, int8_kv=True, kv_scales=[0.05] * dims.n_text_layer)
        other = build_engine(draft_dir, model, DRAFT_SEED)
        xa = {q: WhisperEncoding(eng).get_audio_features(synthetic_mel(3, 2 * dims.n_audio_ctx, dims.n_mels, SEEDS[model, q][1]).cuda())
              for q, eng in (("fp16", fp16), ("int8", int8))}
        out[model] = dict(fp16=fp16, int8=int8, other=other, xa=xa, dims=dims)
    return out


def options(**kw):
    return DecodingOptions(sample_len=SAMPLE_LEN, language="en", **kw)


def sm():
    return torch.cuda.current_stream().cuda_stream


def forced_logits(probe, xa_row, row):
    """The logits of the main engine ALONE for the tokens `row`, in 4-token passes from an empty cache: [len(row) - 1, V] fp32."""
    st = probe._fast_state(1, xa_row.device)
    cross = probe._cross_persistent(xa_row, st)
    cap, V = probe.decoder_config['num_text_ctx'], probe.decoder_config['vocab_size']
    tok = torch.tensor([row], dtype=torch.int32, device=xa_row.device)
    buf = torch.empty((1, 4, V), dtype=torch.float16, device=xa_row.device)
    out, n = [], len(row) - 1
    for p in range(0, n, 4):
        l = min(4, n - p)
        probe.decoder_session.decoder_step(tok[:, p:p + l], probe.positional_embedding[p:p + l], cross, st['kv'] if p else None, cap,
                                           st['kv'], cap, buf, p, sm(), slot=0)
        out.append(buf[0, :l].float().cpu().numpy().copy())
    torch.cuda.synchronize()
    return np.concatenate(out)


def excuses(probe, xa_row, row, ids, bound):
    """How many sampled positions of `row` are not the host rules' choice on the engine's own logits; each of them must lie within
    twice the logit bound of the best allowed token (else the test fails here).  Returns (excused, sampled)."""
    tk = probe.tokenizer
    rules = DR.RuleSet(ids, probe.sample_begin, list(probe._get_suppress_tokens()), list(tk.blank_tokens()) + [tk.eot],
                       probe.max_initial_timestamp_index)
    logits = forced_logits(probe, xa_row, row)
    excused = 0
    for s in range(probe.sample_begin, len(row)):
        allowed = DR.apply_filters(logits[s - 1][None], np.asarray([row[:s]], dtype=np.int64), rules)[0]
        best = int(allowed.argmax())
        if row[s] != best:
            gap = float(allowed[best] - allowed[row[s]])
            assert gap <= 2 * bound, f"position {s}: token {row[s]} is {gap:.4f} below the host rules' token {best} (bound {2 * bound})"
            excused += 1
    return excused, len(row) - probe.sample_begin


def rows_of(dec, tokens):
    """The token rows of a main_loop result, each cut behind its first sampled EOT (or whole)."""
    eot, out = dec.tokenizer.eot, []
    for r in tokens.cpu().tolist():
        tail = r[dec.sample_begin:]
        out.append(r[:dec.sample_begin + tail.index(eot) + 1] if eot in tail else r)
    return out


def check_lossless(probe, xa, tokens, ids, bound, allow_excuses=True):
    total = sampled = 0
    for r, row in enumerate(rows_of(probe, tokens)):
        e, n = excuses(probe, xa[r:r + 1], row, ids, bound)
        total, sampled = total + e, sampled + n
    assert total * 10 <= sampled, f"{total} of {sampled} positions needed the margin"
    if not allow_excuses:
        assert total == 0, f"the plain loop needed the margin at {total} positions: choose other seeds"


def replay(dec, ref, xa, tokens, sums):
    """The recorded rounds through `ref` (an instance without a draft on the same engine), on its own buffers: the same
    wm_decoder_step calls, the recorded proposals put in place, sequential wm_greedy_step calls up to the first mismatch."""
    stats = dec.speculative_stats
    n, dev = xa.shape[0], xa.device
    cap, V, L0, eot = ref.decoder_config['num_text_ctx'], ref.decoder_config['vocab_size'], ref.sample_begin, ref.tokenizer.eot
    st = ref._fast_state(n, dev)
    tokens0 = dec._initial_token_rows(n, dev)
    cross = ref._reset_state(st, xa, tokens0, None, 1, reseed=False)
    sess, pos = ref.decoder_session, ref.positional_embedding
    buf = torch.empty((1, 4, V), dtype=torch.float16, device=dev)
    final = tokens.cpu()
    for r in range(n):
        row, kv, crs = st['tokens'][r:r + 1], [t[r:r + 1] for t in st['kv']], [t[r:r + 1] for t in cross]
        sess.decoder_step(row[:, :L0], pos[0:L0], crs, None, cap, kv, cap, st['logits'][r:r + 1], 0, sm(), slot=0)
        ref._greedy(st, r, r + 1, st['logits'][r:r + 1].data_ptr() + (L0 - 1) * V * 2, L0 * V, L0, sm())
        cur = L0 + 1
        for T_, proposals, n_accept in stats['trace'][r]:
            assert T_ == cur - 1
            k = len(proposals)
            if k:
                row[0, cur:cur + k] = torch.tensor(proposals, dtype=torch.int32, device=dev)
            sess.decoder_step(row[:, cur - 1:cur + k], pos[cur - 1:cur + k], crs, kv, cap, kv, cap, buf, cur - 1, sm(), slot=0)
            written = 0
            for j in range(k + 1):
                ref._greedy(st, r, r + 1, buf.data_ptr() + j * V * 2, (k + 1) * V, cur + j, sm())
                t = int(row[0, cur + j])
                written += 1
                if t == eot or j == k or t != proposals[j]:
                    break
            assert written == n_accept, (r, T_, written, n_accept)
            cur += n_accept
            assert row[0, :cur].cpu().tolist() == final[r, :cur].tolist(), (r, T_)        # round by round
        assert cur - L0 == stats['tokens'][r] and len(stats['trace'][r]) == stats['rounds'][r]
        assert sum(len(p) for _, p, _ in stats['trace'][r]) == stats['proposals'][r]
        assert sum(a - 1 for _, _, a in stats['trace'][r]) == stats['accepted'][r]
    torch.cuda.synchronize()
    assert np.array_equal(st['sum_logprobs'].cpu().numpy().view(np.int32), sums.cpu().numpy().view(np.int32))
    ref._state.clear()


def speculative_run(engines, model, quant, draft, k, n_rows):
    e = engines[model]
    dec = WhisperDecoding(e[quant], options=options(), draft_engine_dir=e[quant] if draft == "itself" else e["other"], draft_tokens=k)
    dec.speculative_trace = True
    xa = e["xa"][quant][:n_rows]
    tokens, sums, nsp = dec.main_loop(xa)
    return dec, xa, tokens, sums, nsp


@pytest.mark.parametrize("n_rows", [1, 3])
@pytest.mark.parametrize("quant", ["fp16", "int8"])
@pytest.mark.parametrize("model", ["micro-fullvocab", "micro-v3"])
def test_replay_and_lossless_up_to_margin(engines, model, quant, n_rows):
    """The device loop with another seed's draft: replayed exactly; every token is the main engine's own choice up to the margin; the
    plain loop of the same engine on the same clips needs no margin at all (the condition on the seeds)."""
    e = engines[model]
    dec, xa, tokens, sums, nsp = speculative_run(engines, model, quant, "other", 3, n_rows)
    ref = WhisperDecoding(e[quant], options=options())
    plain_tokens, plain_sums, plain_nsp = ref.main_loop(xa)
    ref._state.clear()
    replay(dec, ref, xa, tokens, sums)
    check_lossless(ref, xa, plain_tokens, IDS[model], LOGIT_BOUND[quant], allow_excuses=False)
    check_lossless(ref, xa, tokens, IDS[model], LOGIT_BOUND[quant])
    assert len(nsp) == n_rows and np.allclose(nsp, plain_nsp, atol=1e-3)
    res = dec.post_process(tokens, sums, nsp, xa, ["en"] * n_rows)
    assert len(res) == n_rows and all(np.isfinite(r.avg_logprob) and len(r.tokens) <= SAMPLE_LEN for r in res)
    stats = dec.speculative_stats
    assert all(stats['rounds'][r] <= stats['tokens'][r] <= SAMPLE_LEN for r in range(n_rows))
    dec._state.clear(); dec.draft._state.clear(); ref._state.clear()


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("draft", ["itself", "other"])
def test_both_outcomes_are_seen(engines, draft, k):
    """The main engine as its own draft: at least one round keeps all k proposals.  A draft from another seed: at least one round
    rejects the first.  Either way the output is replayed exactly and lossless up to margin, with draft_tokens 1, 2 and 3."""
    e = engines["micro-fullvocab"]
    dec, xa, tokens, sums, nsp = speculative_run(engines, "micro-fullvocab", "fp16", draft, k, 3)
    rounds = [t for row in dec.speculative_stats['trace'] for t in row]
    assert all(len(p) <= k for _, p, _ in rounds) and any(len(p) == k for _, p, _ in rounds)
    if draft == "itself":
        assert any(len(p) == k and a == k + 1 for _, p, a in rounds)
    else:
        assert any(len(p) >= 1 and a == 1 for _, p, a in rounds)
    ref = WhisperDecoding(e["fp16"], options=options())
    replay(dec, ref, xa, tokens, sums)
    check_lossless(ref, xa, tokens, IDS["micro-fullvocab"], LOGIT_BOUND["fp16"])
    dec._state.clear(); dec.draft._state.clear(); ref._state.clear()


def test_transcribe_temperature_and_the_instance_without_a_draft(engines, monkeypatch):
    """transcribe_mel on a two-window file gives the kind of result it gives without a draft; a call at temperature 0.4 on the
    instance with a draft returns what an instance without one returns (the ordinary loop); an instance without a draft never
    reaches wm_verify_step."""
    e = engines["micro-fullvocab"]
    dims, W = e["dims"], 2 * e["dims"].n_audio_ctx
    enc = WhisperEncoding(e["fp16"])
    content = W + 60
    mel = synthetic_mel(1, content + W, dims.n_mels, 905)[0].cuda().contiguous()
    lib = native.load_library()
    calls = {"verify": 0}
    real = lib.wm_verify_step

    def counting(*a, **k):
        calls["verify"] += 1
        return real(*a, **k)
    monkeypatch.setattr(lib, "wm_verify_step", counting)
    results = {}
    for name, kw in (("plain", {}), ("draft", dict(draft_engine_dir=e["other"], draft_tokens=2))):
        dec = WhisperDecoding(e["fp16"], options=DecodingOptions(language="en"), **kw)
        dec.sample_len = 12
        before = calls["verify"]
        results[name] = T.transcribe_mel(enc, dec, [mel], [content], n_rows=1, temperatures=(0.0,), compression_ratio_threshold=None,
                                         logprob_threshold=None, no_speech_threshold=None)
        torch.manual_seed(11)
        sampled = dec.main_loop(e["xa"]["fp16"][:2], temperature=0.4)
        results[name + "_sampled"] = (sampled[0].cpu(), sampled[1].cpu())
        used = calls["verify"] - before
        assert (used > 0) == (name == "draft"), (name, used)
        if name == "draft":
            n_verify = used
            dec.main_loop(e["xa"]["fp16"][:2], temperature=0.4)
            assert calls["verify"] == before + n_verify           # a call above temperature 0 takes the ordinary loop
            dec.draft._state.clear()
        dec._state.clear()
    plain, draft = results["plain"][0], results["draft"][0]
    assert set(plain) == set(draft) and len(draft["segments"]) >= 2
    assert all(set(a) == set(b) for a, b in zip(plain["segments"], draft["segments"]))
    assert len({s["seek"] for s in draft["segments"]}) >= 2 and all(s["temperature"] == 0.0 for s in draft["segments"])
    assert torch.equal(results["plain_sampled"][0], results["draft_sampled"][0])
    assert torch.equal(results["plain_sampled"][1], results["draft_sampled"][1])


def test_refusals(engines):
    e = engines["micro-fullvocab"]
    eng, other = e["fp16"], e["other"]
    for k in (0, 4):
        with pytest.raises(ValueError, match="draft_tokens"):
            WhisperDecoding(eng, options=options(), draft_engine_dir=other, draft_tokens=k)
    with pytest.raises(ValueError, match="n_vocab"):
        WhisperDecoding(eng, options=options(), draft_engine_dir=engines["micro-v3"]["fp16"])
    for word, opt, kw in (("beam_size", options(beam_size=2), {}), ("best_of", options(best_of=2, temperature=0.5), {}),
                          ("fallback_best_of", options(beam_size=2), dict(shared_cross_kv=True, fallback_best_of=1)),
                          ("row_prompts", options(), dict(row_prompts=True)), ("shared_cross_kv", options(), dict(shared_cross_kv=True)),
                          ("repetition_penalty", options(repetition_penalty=1.3), {}), ("no_repeat_ngram_size", options(no_repeat_ngram_size=2), {}),
                          ("hotwords", options(hotwords=((300, 400),)), {}), ("sequence_bias", options(sequence_bias=(((300, 400), 2.0),)), {})):
        with pytest.raises(ValueError, match=word):
            WhisperDecoding(eng, options=opt, draft_engine_dir=other, **kw)
    dec = WhisperDecoding(eng, options=options(), draft_engine_dir=other)
    dec.cu_partition = True
    with pytest.raises(ValueError, match="cu_partition"):
        dec.main_loop(e["xa"]["fp16"][:1])
    dec.cu_partition = False
    assert dec.draft is not None and dec.draft.draft is None and dec.draft_tokens == 3
    dec._state.clear(); dec.draft._state.clear()


def test_the_command_lines_take_a_draft(tmp_path_factory, golden_dir, capsys, monkeypatch):
    """run.py and transcribe.py --draft_engine_dir on the committed LibriSpeech clip, synthetic engines with a 30-second window: a
    transcript is printed, the loop that produced it was the speculative one."""
    import os
    import run as R
    name = "micro-v3-30s"
    synthetic.DIMS[name] = dict(synthetic.DIMS["micro-v3"], n_audio_ctx=1500)
    try:
        eng = build_engine(str(tmp_path_factory.mktemp("spec_cli_main")), name, MODEL_SEED)
        draft = build_engine(str(tmp_path_factory.mktemp("spec_cli_draft")), name, DRAFT_SEED)
    finally:
        synthetic.DIMS.pop(name, None)
    flac = os.path.join(golden_dir, "librispeech_1089-134691-0000.flac")
    seen = []
    real = WhisperDecoding._speculative_loop

    def spy(self, *a, **k):
        out = real(self, *a, **k)
        seen.append(dict(self.speculative_stats))
        return out
    monkeypatch.setattr(WhisperDecoding, "_speculative_loop", spy)
    result = R.main(["--engine_dir", str(eng), "--input_file", flac, "--draft_engine_dir", str(draft), "--draft_tokens", "2"])
    assert "transcribe time" in capsys.readouterr().out
    assert isinstance(result.text, str) and result.tokens and all(t < 51866 for t in result.tokens)
    assert len(seen) == 1 and seen[0]["rounds"][0] >= 1 and seen[0]["proposals"][0] <= 2 * seen[0]["rounds"][0]
    long = T.main(T.parse_arguments(["--engine_dir", str(eng), "--input_file", flac, "--no_fallback", "--draft_engine_dir", str(draft)]))
    assert len(long) == 1 and long[0]["segments"] and len(seen) >= 2
