"""Shared cross K/V and the beam-at-0 / samples-above recipe, host side (no GPU): the mode rule (`decoding.candidate_mode`), every new
refusal, the host loops switching decoders per call and keeping closed rows out of the ranking, the row budget, the C layout of the
new structs, and the command-line flags."""
import ctypes as C
import json
import os
import subprocess

import pytest
import torch

import build as B
import native
import synthetic
from decoding import (BeamSearchDecoder, DecodingOptions, GreedyDecoder, WhisperDecoding, candidate_mode,
                      check_candidate_options)
from oracle import decoding_rules as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LADDER = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)


@pytest.fixture(scope="module")
def engine_dir(tmp_path_factory):
    out = tmp_path_factory.mktemp("shared") / "eng"
    args = B.parse_arguments(["--output_dir", str(out), "--log_level", "error"])
    B.build_from_checkpoint(synthetic.synthetic_checkpoint("micro-fullvocab", 3), args)
    cfg = json.load(open(out / "decoder_config.json"))
    cfg["builder_config"]["num_audio_ctx"] = 1500         # host rules only: 0.02 s per timestamp, as at large-v2
    json.dump(cfg, open(out / "decoder_config.json", "w"))
    return out


def test_candidate_mode_over_the_ladder():
    """Upstream's decode_with_fallback: beam_size / patience dropped above temperature 0, best_of dropped at 0."""
    beam = DecodingOptions(beam_size=5, patience=2.0)
    assert [candidate_mode(beam, 3, t) for t in LADDER] == [("beam", 5)] + [("sample", 3)] * 5
    assert [candidate_mode(beam, 5, t) for t in LADDER] == [("beam", 5)] + [("sample", 5)] * 5
    assert [candidate_mode(beam, 1, t) for t in LADDER] == [("beam", 5)] + [("sample", 1)] * 5
    # without fallback_best_of an instance keeps its own mode at every temperature
    assert {candidate_mode(beam, None, t) for t in LADDER} == {("beam", 5)}
    assert {candidate_mode(DecodingOptions(best_of=4, temperature=0.4), None, t) for t in LADDER} == {("sample", 4)}
    assert {candidate_mode(DecodingOptions(), None, t) for t in LADDER} == {("sample", 1)}


@pytest.mark.parametrize("options,kw,match", [
    (DecodingOptions(), dict(shared_cross_kv=True, fallback_best_of=2), "needs beam_size"),
    (DecodingOptions(best_of=3, temperature=0.5), dict(shared_cross_kv=True, fallback_best_of=2), "best_of"),
    (DecodingOptions(beam_size=3), dict(fallback_best_of=2), "shared_cross_kv"),
    (DecodingOptions(beam_size=3), dict(shared_cross_kv=True, fallback_best_of=4), "outside 1..beam_size"),
    (DecodingOptions(beam_size=3), dict(shared_cross_kv=True, fallback_best_of=0), "outside 1..beam_size"),
])
def test_new_option_checks_raise(engine_dir, options, kw, match):
    with pytest.raises(ValueError, match=match):
        check_candidate_options(options, bool(kw.get("shared_cross_kv")), kw.get("fallback_best_of"))
    with pytest.raises(ValueError, match=match):
        WhisperDecoding(engine_dir, only_torch=True, options=options, **kw)


def test_shared_instances_refuse_the_host_loop_and_the_cu_partition(engine_dir):
    xa = torch.zeros(2, 1, 1)
    for options in (DecodingOptions(beam_size=3), DecodingOptions(best_of=3, temperature=0.5)):
        dec = WhisperDecoding(engine_dir, only_torch=True, options=options, shared_cross_kv=True)
        assert dec.shared_cross_kv and dec._cross_group() == 3
        with pytest.raises(ValueError, match="features on the GPU"):
            dec.main_loop(xa)                                 # CPU features would mean the literal host loop, which repeats the features
        dec.device_sampling = False
        with pytest.raises(ValueError, match="device_sampling"):
            dec.main_loop(xa)
        dec.device_sampling, dec.cu_partition = True, True
        with pytest.raises(ValueError, match="cu_partition"):
            dec.main_loop(xa)
    # an instance built as before knows none of this, and a shared greedy instance has nothing to share
    assert WhisperDecoding(engine_dir, only_torch=True, options=DecodingOptions(beam_size=3))._cross_group() == 1
    assert WhisperDecoding(engine_dir, only_torch=True, shared_cross_kv=True)._cross_group() == 1


def test_transcribe_accepts_what_the_instance_can_do(engine_dir):
    import transcribe as T
    plain = WhisperDecoding(engine_dir, only_torch=True, options=DecodingOptions(beam_size=2))
    shared = WhisperDecoding(engine_dir, only_torch=True, options=DecodingOptions(beam_size=2), shared_cross_kv=True)
    recipe = WhisperDecoding(engine_dir, only_torch=True, options=DecodingOptions(beam_size=2), shared_cross_kv=True, fallback_best_of=2)
    samples = WhisperDecoding(engine_dir, only_torch=True, options=DecodingOptions(best_of=2, temperature=0.4), shared_cross_kv=True)
    for dec in (plain, shared, samples):                      # the per-call temperature stays refused without fallback_best_of
        with pytest.raises(ValueError, match="instance's temperature"):
            T.check_supported(dec, LADDER)
    with pytest.raises(ValueError, match="word_timestamps"):
        T.check_supported(plain, (0.0,), word_timestamps=True)
    T.check_supported(shared, (0.0,), word_timestamps=True)
    T.check_supported(samples, (0.4,), word_timestamps=True)
    T.check_supported(recipe, LADDER, word_timestamps=True)


def test_groups_and_row_budget_count_the_cross_kv_once_per_utterance(engine_dir):
    cfg = json.load(open(engine_dir / "decoder_config.json"))["builder_config"]
    cross = 2 * cfg["num_heads"] * cfg["num_audio_ctx"] * 64 * 2
    for G, options in ((5, DecodingOptions(beam_size=5)), (4, DecodingOptions(best_of=4, temperature=0.4))):
        plain = WhisperDecoding(engine_dir, only_torch=True, options=options)
        shared = WhisperDecoding(engine_dir, only_torch=True, options=options, shared_cross_kv=True)
        saved = plain.state_bytes_per_utterance() - shared.state_bytes_per_utterance()
        prefill_logits = -(-shared.initial_token_length * cfg["vocab_size"] * 2 // G)      # one prefilled row per utterance, a candidate's share
        assert saved == cfg["num_layers"] * (cross - -(-cross // G)) - prefill_logits > 0
        for n_audio in (3, 4, 7, 26, 40):                     # best_of too: the groups are cut in whole utterances
            n_micro, bounds = shared._groups(n_audio * G)
            assert bounds[0][0] == 0 and bounds[-1][1] == n_audio * G and all(lo % G == 0 and hi > lo for lo, hi in bounds)
            assert sorted(shared.balanced_order(n_audio)) == list(range(n_audio))


def seeded_decode(presents):
    def decode(x, cross, past=None):
        call, rows = len(presents), x.shape[0]
        presents.append(rows)
        logits = torch.from_numpy(DR.sampling_logits(call, rows, x.shape[1])).clone()
        logits[:, -1, DR.MULTILINGUAL.eot] += 6.0 if call >= 4 else 0.0
        return logits, [torch.zeros(rows, 2, 1, call + 1, 4)]
    return decode


def test_host_loop_switches_decoders_per_call_and_ranks_live_candidates_only(engine_dir, monkeypatch):
    """main_loop_reference on seeded logits with beam_size = 3, fallback_best_of = 2: at temperature 0 the beam decoder runs (beams are
    gathered, a pool fills); at 0.4 the same rows are sampled independently, candidate 2 of every utterance is closed before its first
    token with a sum of 0 -- which would win the ranking -- and post_process ranks candidates 0 and 1 only."""
    n_audio, K, M = 2, 3, 2
    dec = WhisperDecoding(engine_dir, only_torch=True, options=DecodingOptions(beam_size=K, sample_len=10), shared_cross_kv=True, fallback_best_of=M)
    dec.tokenizer.decode = lambda t: " ".join(str(int(x)) for x in t)
    monkeypatch.setattr(dec, "xa2cross_key_value", lambda xa: None)
    xa = torch.zeros(n_audio, 1, 1)
    eot = dec.tokenizer.eot

    beam_updates = []
    update = dec.decoder.update
    monkeypatch.setattr(dec.decoder, "update", lambda *a: (beam_updates.append(1), update(*a))[1])
    calls = []
    monkeypatch.setattr(dec, "decode", seeded_decode(calls))
    dec.tokens = torch.tensor([dec.initial_tokens]).repeat(n_audio, 1)
    t0, lp0, nsp0 = dec.main_loop_reference(xa, temperature=0.0)
    assert beam_updates and len(beam_updates) == len(calls) and any(dec.decoder.pool)
    res0 = dec.post_process(t0, lp0, nsp0, xa, ["en"] * n_audio, temperature=0.0)
    cands, _ = dec.decoder.finalize(t0, lp0)
    assert all(res0[a].tokens in [c[dec.sample_begin:-1].tolist() for c in cands[a]] and res0[a].temperature == 0.0 for a in range(n_audio))

    del beam_updates[:]
    calls2 = []
    monkeypatch.setattr(dec, "decode", seeded_decode(calls2))
    torch.manual_seed(11)
    t1, lp1, nsp1 = dec.main_loop_reference(xa, temperature=0.4)
    assert not beam_updates, "a sampling call must not go through the beam decoder"
    assert set(calls2) == {n_audio * K}, "the rows stay n_audio x beam_size in both modes"
    rows = t1.reshape(n_audio, K, -1)
    sums = lp1.reshape(n_audio, K)
    assert bool((rows[:, M:, dec.sample_begin:] == eot).all()) and bool((sums[:, M:] == 0).all()), "closed rows: EOT at once, nothing booked"
    assert bool((rows[:, :M, dec.sample_begin] != eot).all()) and bool((sums[:, :M] < 0).all())
    assert len({tuple(r.tolist()) for r in rows[:, :M].reshape(n_audio * M, -1)}) > n_audio, "the samples of an utterance are drawn independently"
    res1 = dec.post_process(t1, lp1, nsp1, xa, ["en"] * n_audio, temperature=0.4)
    for a in range(n_audio):
        live = [r[dec.sample_begin:].tolist() for r in rows[a, :M]]
        live = [r[:r.index(eot)] if eot in r else r for r in live]
        assert res1[a].tokens in live and len(res1[a].tokens) >= 1 and res1[a].temperature == 0.4
        best = max(range(M), key=lambda j: float(sums[a, j]) / len(live[j]))          # MaximumLikelihoodRanker without a length penalty
        assert res1[a].tokens == live[best] and abs(res1[a].avg_logprob - float(sums[a, best]) / (len(live[best]) + 1)) < 1e-6
    # the decoders of the two modes
    assert isinstance(dec._call_decoder(0.0)[0], BeamSearchDecoder) and dec._call_decoder(0.0)[1] == K
    d, n = dec._call_decoder(0.6)
    assert isinstance(d, GreedyDecoder) and d.temperature == 0.6 and n == M
    # an instance without the fallback decodes with its own decoder whatever temperature a caller names
    own = WhisperDecoding(engine_dir, only_torch=True, options=DecodingOptions(beam_size=K))
    assert own._call_decoder(0.6) == (own.decoder, K)


def test_new_struct_layouts_match_header(tmp_path):
    """ctypes mirrors of the structs this change added (and of the ones they extend) vs the C compiler's view of include/whisper_mi355.h."""
    structs = {"wm_decoder_io": native.WmDecoderIO, "wm_decoder_group_io": native.WmDecoderGroupIO,
               "wm_attn_cross_group_io": native.WmAttnCrossGroupIO, "wm_attn_cross_io": native.WmAttnCrossIO}
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
    # the group size travels in a struct of its own: wm_decoder_io keeps the layout tests/test_prompts_cpu.py pins
    assert [f for f, _ in native.WmDecoderIO._fields_][-2:] == ["not_alone", "row_start"]
    assert [f for f, _ in native.WmDecoderGroupIO._fields_] == ["io", "cross_group", "live_groups"] and native.WmDecoderGroupIO.io.offset == 0
    assert [f for f, _ in native.WmAttnCrossGroupIO._fields_][:-2] == [f for f, _ in native.WmAttnCrossIO._fields_]
    assert {"wm_attn_cross_group_ex", "wm_step_finish_group", "wm_decoder_step_group"} <= set(native.EXPORTS)


def test_command_line_flags_parse(capsys):
    import run as R
    import summarize as S
    import transcribe as T
    a = T.parse_arguments(["--input_file", "a.flac"])
    assert a.beam_size is None and a.patience is None and a.best_of is None          # off by default: greedy, as before
    a = T.parse_arguments(["--input_file", "a.flac", "--beam_size", "5", "--patience", "2", "--best_of", "3", "--word_timestamps"])
    assert (a.beam_size, a.patience, a.best_of, a.word_timestamps) == (5, 2.0, 3, True)
    a = T.parse_arguments(["--input_file", "a.flac", "--best_of", "4", "--temperature", "0.4"])
    assert (a.beam_size, a.best_of, a.temperature) == (None, 4, [0.4])
    with pytest.raises(SystemExit):
        T.parse_arguments(["--help"])
    assert "a per-call temperature, i.e. the ladder, is refused" in " ".join(capsys.readouterr().out.split())
    assert R.parse_arguments([]).shared_cross_kv is False and R.parse_arguments(["--shared_cross_kv", "--beam_size", "3"]).shared_cross_kv is True
    assert S.parse_arguments([]).shared_cross_kv is False and S.parse_arguments(["--shared_cross_kv"]).shared_cross_kv is True
    with pytest.raises(ValueError, match="--patience needs --beam_size"):
        T.build_decoding(T.parse_arguments(["--input_file", "a.flac", "--patience", "2"]), "unused", False)
