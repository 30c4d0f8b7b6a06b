"""Beam search, host side (no GPU): `decoding.BeamSearchDecoder` -- the literal statement of the contract the device step
implements (wm_beam_io in include/whisper_mi355.h) -- held to a brute-force restatement written here, the option checks,
the cache gather of `main_loop_reference`, and the C layout of wm_beam_io."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import build as B
import native
import synthetic
from decoding import BeamSearchDecoder, DecodingOptions, WhisperDecoding
from oracle import decoding_rules as DR
from oracle.whisper_oracle import Dims, synthetic_mel, synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOT = 7          # of the small vocabulary below


def seeded_logits(rng, rows, V, eot_bias):
    """fp16 logits on a coarse grid (exact ties inside a row are common), a few entries masked, EOT lifted by `eot_bias`."""
    x = np.round(rng.standard_normal((rows, V)) * 4) / 2
    x[:, EOT] += eot_bias
    x[rng.random((rows, V)) < 0.1] = -np.inf
    x[:, 0] = np.maximum(x[:, 0], -3.0)          # never a fully masked row
    return x.astype(np.float16)


def brute_force_step(tokens, logits, sums, K, first, pool, live_len, max_candidates):
    """One step of the contract by enumeration: ALL beam x V continuations of an utterance in float64, sorted under the total
    order (score descending, parent beam ascending, token ascending), walked until K live beams are saved.  Returns the new
    rows, sums and source rows; updates `pool` / `live_len` in place; also the smallest gap between two walked candidates that
    are not an exact tie inside one row (the condition under which fp32 and float64 must agree on the order)."""
    rows, cur = tokens.shape
    x = logits.astype(np.float64)
    m = x.max(axis=1, keepdims=True)
    logprobs = x - m - np.log(np.exp(x - m).sum(axis=1, keepdims=True))
    new_rows, new_sums, source, min_gap = [], [], [], np.inf
    for a in range(rows // K):
        r0 = a * K
        if live_len[a] is not None:
            new_rows += [list(tokens[r0 + j]) + [EOT] for j in range(K)]
            new_sums += [sums[r0 + j] for j in range(K)]
            source += [r0 + j for j in range(K)]
            continue
        cands = [(sums[r0 + j] + logprobs[r0 + j, t], j, t)
                 for j in range(1 if first else K) for t in range(x.shape[1]) if np.isfinite(x[r0 + j, t])]
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        live, finished, walked = [], [], []
        for c in cands:
            walked.append(c)
            if c[2] == EOT:
                finished.append(c)
            else:
                live.append(c)
                if len(live) == K:
                    break
        assert len(live) == K
        for c0, c1 in zip(walked, walked[1:]):
            if not (c0[1] == c1[1] and x[r0 + c0[1], c0[2]] == x[r0 + c1[1], c1[2]]):
                min_gap = min(min_gap, c0[0] - c1[0])
        for s, j, t in live:
            new_rows.append(list(tokens[r0 + j]) + [t])
            new_sums.append(s)
            source.append(r0 + j)
        for s, j, t in finished:
            if len(pool[a]) < max_candidates:
                pool[a].append((list(tokens[r0 + j]) + [EOT], s))
        if len(pool[a]) >= max_candidates:
            live_len[a] = cur + 1
    return np.array(new_rows), np.array(new_sums), source, min_gap


@pytest.mark.parametrize("K,patience,eot_bias,seed", [(1, None, 1.0, 0), (2, 1.0, 2.0, 1), (3, 2.0, 3.0, 2), (4, 0.5, 2.0, 3),
                                                      (5, 1.0, 2.5, 4), (8, 2.0, 4.0, 5), (3, 1.0, -50.0, 6)])
def test_beam_search_decoder_matches_brute_force(K, patience, eot_bias, seed):
    """Seeded multi-step runs: exact ties inside a row, EOT candidates, the first step, patience 1 / 2 / 0.5, pools that fill
    (the utterance freezes) and pools that stay short (finalize tops them up; eot_bias = -50: no beam ever ends)."""
    rng = np.random.Generator(np.random.Philox(seed))
    n_audio, V, sample_begin, steps = 3, 24, 3, 7
    dec = BeamSearchDecoder(K, EOT, sample_begin, patience)
    max_candidates = round(K * (patience or 1.0))
    assert dec.max_candidates == max_candidates
    tokens = torch.tensor([[20, 21, 22]] * (n_audio * K))
    sums = torch.zeros(n_audio * K)
    ref_tokens, ref_sums = tokens.numpy().copy(), np.zeros(n_audio * K)
    pool, live_len = [[] for _ in range(n_audio)], [None] * n_audio
    saw_tie = saw_eot = saw_reorder = False
    for step in range(steps):
        lg = seeded_logits(rng, n_audio * K, V, eot_bias)
        ref_tokens, ref_sums, ref_source, gap = brute_force_step(ref_tokens, lg, ref_sums, K, step == 0, pool, live_len, max_candidates)
        assert gap > 1e-4, "the seeded logits put two candidates closer than fp32 can order"
        tokens, completed, source = dec.update(tokens, torch.from_numpy(lg.copy()), sums)
        assert np.array_equal(tokens.numpy(), ref_tokens), step
        assert source.tolist() == ref_source, step
        np.testing.assert_allclose(sums.numpy(), ref_sums, rtol=0, atol=1e-6)
        assert [[s for s, _ in p] for p in dec.pool] == [[s for s, _ in p] for p in pool], step
        np.testing.assert_allclose([lp for p in dec.pool for _, lp in p], [lp for p in pool for _, lp in p], rtol=0, atol=1e-6)
        assert dec.completed == [n is not None for n in live_len] and dec.live_len == live_len
        assert completed == all(n is not None for n in live_len)
        for r in range(n_audio * K):
            top = np.sort(lg[r].astype(np.float32))[::-1][:K + 1]
            saw_tie |= bool(np.isfinite(top).all() and len(set(top.tolist())) < len(top))
        saw_eot |= any(pool)
        saw_reorder |= ref_source != list(range(n_audio * K))
    assert saw_tie, "no exact tie inside a row's best beam_size + 1: the fixture does not test the order"
    if eot_bias > 0:
        assert saw_eot
    if K > 1:
        assert saw_reorder
    # finalize: the pool, topped up with live beams (best sum first) to beam_size sequences
    got_tokens, got_sums = dec.finalize(tokens, sums)
    short = False
    for a in range(n_audio):
        want = list(pool[a])
        n_live = ref_tokens.shape[1] if live_len[a] is None else live_len[a]
        short |= len(want) < K
        for j in sorted(range(K), key=lambda j: (-ref_sums[a * K + j], j)):
            if len(want) >= K:
                break
            want.append((list(ref_tokens[a * K + j, :n_live]) + [EOT], ref_sums[a * K + j]))
        assert [t.tolist() for t in got_tokens[a]] == [list(map(int, s)) for s, _ in want]
        np.testing.assert_allclose(got_sums[a], [lp for _, lp in want], rtol=0, atol=1e-6)
        assert all(int(t[-1]) == EOT for t in got_tokens[a])
    if patience == 0.5 or eot_bias < 0:
        assert short, "no utterance needed the top-up"


def test_frozen_utterance_no_longer_changes():
    """An utterance whose pool is full is frozen: later steps change neither its beams nor its sums nor its pool, whatever its
    logits -- and the other utterance decodes on (a row's result does not depend on its neighbours)."""
    K, V = 2, 12
    dec = BeamSearchDecoder(K, EOT, 1)
    tokens, sums = torch.tensor([[9]] * 4), torch.zeros(4)
    lg = torch.full((4, V), -5.0)
    lg[0, EOT], lg[0, 1], lg[0, 2] = 5.0, 4.0, 3.0            # utterance 0: EOT is the best first candidate, the pool needs two
    lg[2, 3], lg[2, 4] = 5.0, 4.0
    tokens, completed, _ = dec.update(tokens, lg.clone(), sums)
    assert dec.completed == [False, False] and len(dec.pool[0]) == 1 and tokens[:2, -1].tolist() == [1, 2]
    lg = torch.full((4, V), -5.0)
    lg[0, EOT], lg[1, EOT], lg[2, 5], lg[3, 5] = 9.0, 1.0, 2.0, 2.0
    tokens, completed, _ = dec.update(tokens, lg.clone(), sums)
    assert dec.completed == [True, False] and not completed and dec.live_len == [3, None]
    frozen_tokens, frozen_sums, frozen_pool = tokens[:2, :3].clone(), sums[:2].clone(), list(dec.pool[0])
    tokens, completed, source = dec.update(tokens, torch.randn(4, V), sums)
    assert torch.equal(tokens[:2, :3], frozen_tokens) and torch.equal(sums[:2], frozen_sums) and dec.pool[0] == frozen_pool
    assert source[:2].tolist() == [0, 1] and tokens.shape[1] == 4 and (tokens[2:, -1] != EOT).all()


@pytest.fixture(scope="module")
def engine_dir(tmp_path_factory):
    out = tmp_path_factory.mktemp("beam") / "eng"
    args = B.parse_arguments(["--output_dir", str(out), "--log_level", "error"])
    B.build_from_checkpoint(synthetic.synthetic_checkpoint("micro-fullvocab", 3), args)
    cfg = json.load(open(out / "decoder_config.json"))
    cfg["builder_config"]["num_audio_ctx"] = 1500         # host rules only: 0.02 s per timestamp, as at large-v2
    json.dump(cfg, open(out / "decoder_config.json", "w"))
    return out


@pytest.mark.parametrize("kwargs,match", [
    (dict(beam_size=5, best_of=5), "best_of"),
    (dict(beam_size=5, temperature=0.5), "temperature"),
    (dict(patience=2.0), "patience"),
    (dict(beam_size=0), "beam_size"),
    (dict(beam_size=9), "beam_size"),
    (dict(beam_size=8, patience=2.5), "patience"),          # 20 finished candidates
    (dict(beam_size=1, patience=0.2), "patience"),          # none
])
def test_option_checks_raise(engine_dir, kwargs, match):
    with pytest.raises(ValueError, match=match):
        WhisperDecoding(engine_dir, only_torch=True, options=DecodingOptions(**kwargs))


def test_options_select_the_decoder(engine_dir):
    dec = WhisperDecoding(engine_dir, only_torch=True, options=DecodingOptions(beam_size=5, patience=2.0))
    assert isinstance(dec.decoder, BeamSearchDecoder) and dec.n_group == 5
    assert dec.decoder.max_candidates == 10                                   # patience = 2.0 doubles the pool
    assert WhisperDecoding(engine_dir, only_torch=True, options=DecodingOptions(beam_size=5)).decoder.max_candidates == 5
    assert not isinstance(WhisperDecoding(engine_dir, only_torch=True).decoder, BeamSearchDecoder)
    assert "wm_beam_step" in native.EXPORTS and "wm_kv_reorder" in native.EXPORTS
    # the beams of an utterance stay in one stream-parallel group
    for n_audio in (3, 4, 7, 26, 40):
        n_micro, bounds = dec._groups(n_audio * 5)
        assert bounds[0][0] == 0 and bounds[-1][1] == n_audio * 5 and all(lo % 5 == 0 and hi > lo for lo, hi in bounds)
        assert all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))


def test_reference_loop_gathers_its_cache_by_the_source_rows(engine_dir, monkeypatch):
    """main_loop_reference with beam_size = 3 on seeded logits: the KV it hands to `decode` at step i + 1 is the gather of what
    step i returned by that step's source rows; the run does reorder beams, ends some, and post_process picks a candidate."""
    n_audio, K = 2, 3
    dec = WhisperDecoding(engine_dir, only_torch=True, options=DecodingOptions(beam_size=K, sample_len=10))
    dec.tokenizer.decode = lambda t: " ".join(str(int(x)) for x in t)
    presents, pasts, sources = [], [], []

    def decode(x, cross, past=None):
        call, rows = len(presents), x.shape[0]
        pasts.append(past)
        new = (torch.arange(rows).float()[:, None] + 100.0 * call).reshape(rows, 1, 1, 1, 1).expand(rows, 2, 1, x.shape[1], 4)
        present = [new.clone() if past is None else torch.cat([past[0], new], dim=3)]
        presents.append(present)
        logits = torch.from_numpy(DR.sampling_logits(call, rows, x.shape[1])).clone()
        logits[:, -1, DR.MULTILINGUAL.eot] += 6.0 if call >= 4 else 0.0          # beams end from the fifth step on
        return logits, present

    update = dec.decoder.update

    def recording_update(tokens, logits, sum_logprobs):
        out = update(tokens, logits, sum_logprobs)
        sources.append(out[2].clone())
        return out
    monkeypatch.setattr(dec, "decode", decode)
    monkeypatch.setattr(dec.decoder, "update", recording_update)
    monkeypatch.setattr(dec, "xa2cross_key_value", lambda xa: None)
    dec.tokens = torch.tensor([dec.initial_tokens]).repeat(n_audio, 1)
    xa = torch.zeros(n_audio, 1, 1)
    tokens, sum_lp, nsp = dec.main_loop(xa)                   # CPU features -> main_loop_reference
    assert len(presents) >= 3 and pasts[0] is None
    for i in range(len(presents) - 1):
        assert torch.equal(pasts[i + 1][0], presents[i][0][sources[i]]), i
    assert sources[0].tolist() == [0, 0, 0, 3, 3, 3]          # first step: beam 0 of each utterance feeds every beam
    assert any(s.tolist() != list(range(n_audio * K)) for s in sources[1:])
    assert any(dec.decoder.pool)
    res = dec.post_process(tokens, sum_lp, nsp, xa, ["en"] * n_audio)
    cands, sums = dec.decoder.finalize(tokens, sum_lp)
    assert len(res) == n_audio and all(len(c) >= K for c in cands)
    for a in range(n_audio):
        assert len({tuple(c.tolist()) for c in cands[a]}) == len(cands[a])       # pairwise different candidates
        assert res[a].tokens in [c[dec.sample_begin:-1].tolist() for c in cands[a]]


def test_torch_main_loop_cache_follows_the_beams(tmp_path):
    """The PyTorch path with beam_size = 3 (a full-width vocabulary with peaked logits, so that beams reorder and end): the loop with
    the model's KV cache, gathered by the source rows after every step, equals the same loop on a model that keeps no cache
    at all and recomputes every step from the beams' whole token histories."""
    import torch_model as TM
    from encoding import WhisperEncoding
    dims = Dims(**synthetic.DIMS["micro-fullvocab"])
    sd = synthetic_state_dict(dims, 3, logit_std=16.0)
    E = sd["decoder.token_embedding.weight"]
    E[DR.MULTILINGUAL.eot] = (E[34532].float() * 1.05).half()
    out = tmp_path / "eng"
    B.build_from_checkpoint({"dims": dims.to_dict(), "model_state_dict": sd}, B.parse_arguments(["--output_dir", str(out), "--log_level", "error"]))
    model = TM.Whisper(TM.ModelDimensions(**dims.to_dict())).load_state_dict({k: v.float() for k, v in sd.items()})
    mel = synthetic_mel(2, 2 * dims.n_audio_ctx, dims.n_mels, 77).float()
    enc = WhisperEncoding(out, only_torch=True)
    dec = WhisperDecoding(out, only_torch=True, options=DecodingOptions(beam_size=3, sample_len=10))
    xa = enc.torch_get_audio_features(model, mel)
    dec.torch_detect_language(model, xa)
    start = dec.tokens.clone()
    sources = []
    update = dec.decoder.update

    class NoCache:
        history = None

        def decoder(self, feed, audio_features, kv_cache=None):
            full = feed if self.history is None else self.history
            return model.decoder(full, audio_features)[:, -feed.shape[1]:]

        def install_kv_cache_hooks(self):
            return {}, []
    plain = NoCache()

    def recording_update(tokens, logits, sum_logprobs):
        res = update(tokens, logits, sum_logprobs)
        plain.history = res[0]
        sources.append(res[2].tolist())
        return res
    dec.decoder.update = recording_update
    t1, lp1, nsp1 = dec.torch_main_loop(model, xa)
    cands1 = dec.decoder.finalize(t1, lp1)
    n_steps, moved = len(sources), sum(s != list(range(6)) for s in sources[1:])
    assert moved >= 2, "the beams never reordered after the first step: the gather is not exercised"
    dec.tokens, plain.history = start, None
    t2, lp2, nsp2 = dec.torch_main_loop(plain, xa)
    cands2 = dec.decoder.finalize(t2, lp2)
    assert sources[:n_steps] == sources[n_steps:] and torch.equal(t1, t2)
    assert torch.allclose(lp1, lp2, atol=1e-3)
    assert [[c.tolist() for c in u] for u in cands1[0]] == [[c.tolist() for c in u] for u in cands2[0]]
    res = dec.post_process(t2, lp2, nsp2, xa, ["en"] * 2)
    assert len(res) == 2 and all(isinstance(r.text, str) for r in res)


def test_wm_beam_io_layout_matches_header(tmp_path):
    """The ctypes mirror vs the C compiler's view of include/whisper_mi355.h (plain C, gcc)."""
    fs = [n for n, _ in native.WmBeamIO._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "whisper_mi355.h"', 'int main(void){',
           'printf("size %zu\\n", sizeof(wm_beam_io));']
    src += [f'printf("{f} %zu\\n", offsetof(wm_beam_io, {f}));' for f in fs]
    src.append('return 0;}')
    (tmp_path / "l.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / "l.c"), "-o", str(tmp_path / "l")])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / "l")]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(native.WmBeamIO)
    for f in fs:
        assert int(got[f]) == getattr(native.WmBeamIO, f).offset, f
    lib = native.load_library()
    assert lib.wm_beam_workspace_bytes(15, 5) == 15 * 6 * 8
