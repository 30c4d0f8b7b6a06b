"""The device loop's plan, host side (no GPU): the graph keys in their literal form, the "may a group take the one-launch step"
decision, and the logit-rule fields that the greedy and the beam step are handed by one filler."""
import json

import pytest
import torch

import build as B
import native
import synthetic
from decoding import (DecodingOptions, WhisperDecoding, call_key, groups_run_alone, language_key, partition_key, prefill_key,
                      step_key, steps_side_by_side)


def test_graph_keys_keep_their_literal_form():
    """st['graphs'] is read by bench.py, the lab scripts and the tests: the keys are written out here, not derived."""
    greedy = call_key(False, False, 1, 0.0, 0.0)
    assert greedy == ()
    assert step_key(2, 1, True, greedy) == (2, 1, True)
    assert prefill_key(2, 1, True, 3, True, greedy) == (2, 1, True, 'prefill', 3, True)
    assert call_key(False, True, 1, 0.0, 0.0) == ()                       # ignore_eot is an argument of the beam step only
    for ignore_eot in (False, True):
        beam = call_key(True, ignore_eot, 1, 0.0, 0.0)
        assert beam == ('beam', ignore_eot)
        assert step_key(1, 0, False, beam) == (1, 0, False, 'beam', ignore_eot)
        assert prefill_key(1, 0, False, 4, False, beam) == (1, 0, False, 'prefill', 4, False, 'beam', ignore_eot)
    # shared cross K/V: G = 1 leaves no mark, G = 5 does, behind the beam's
    assert call_key(True, False, 1, 0.0, 0.0) == ('beam', False)
    assert call_key(True, False, 5, 0.0, 0.0) == ('beam', False, ('cross_group', 5))
    assert call_key(False, False, 5, 0.0, 0.0) == (('cross_group', 5),)
    # a per-call temperature: equal to the instance's none, another one last
    assert call_key(False, False, 1, 0.4, 0.4) == ()
    assert call_key(False, False, 1, 0.4, 0.0) == (('temperature', 0.4),)
    assert call_key(False, False, 5, 0.4, 0.0) == (('cross_group', 5), ('temperature', 0.4))
    assert call_key(True, True, 5, 0.0, 0.2) == ('beam', True, ('cross_group', 5), ('temperature', 0.0))
    assert step_key(3, 2, True, call_key(False, False, 5, 0.4, 0.0)) == (3, 2, True, ('cross_group', 5), ('temperature', 0.4))
    assert prefill_key(3, 2, True, 227, True, call_key(False, False, 5, 0.4, 0.0)) == \
        (3, 2, True, 'prefill', 227, True, ('cross_group', 5), ('temperature', 0.4))
    assert language_key(2, 1, True) == (2, 1, 'lang', True)
    assert language_key(1, 0, False) == (1, 0, 'lang', False)
    assert partition_key(3) == ('partition', 3)


@pytest.mark.parametrize("bounds,n_micro,sequential,force_not_alone,alone,not_alone", [
    ([(0, 8)], 1, False, False, True, False),                  # one group of 8: the one-launch step
    ([(0, 9)], 1, False, False, False, False),                 # one group of 9: too many rows for it
    ([(0, 4), (4, 8)], 2, False, False, False, True),          # two groups of 4 side by side: never
    ([(0, 4), (4, 8)], 2, True, False, True, False),           # ... stepped one after the other: each is alone
    ([(0, 8)], 1, False, True, False, True),                   # force_not_alone: the kernels of the parallel schedule
    ([(0, 4), (4, 8)], 2, True, True, False, True),
    ([(0, 8), (8, 24)], 2, True, False, True, False),          # one group of the pass within eight rows is enough
    ([(0, 12), (12, 24)], 2, True, False, False, False),
])
def test_the_alone_decision(bounds, n_micro, sequential, force_not_alone, alone, not_alone):
    assert groups_run_alone(bounds, n_micro, sequential, force_not_alone) is alone
    assert steps_side_by_side(n_micro, sequential, force_not_alone) is not_alone
    assert not (alone and not_alone)          # a pass whose launches say not_alone never looks for a give-up of its own


@pytest.fixture(scope="module")
def engine_dir(tmp_path_factory):
    out = tmp_path_factory.mktemp("plan") / "eng"
    args = B.parse_arguments(["--output_dir", str(out), "--log_level", "error"])
    B.build_from_checkpoint(synthetic.synthetic_checkpoint("micro-fullvocab", 3), args)
    cfg = json.load(open(out / "decoder_config.json"))
    cfg["builder_config"]["num_audio_ctx"] = 1500         # host rules only: 0.02 s per timestamp, as at large-v2
    json.dump(cfg, open(out / "decoder_config.json", "w"))
    return out


COMMON = ("logits", "row_stride", "batch", "n_vocab", "tokens", "tokens_ld", "cur_len", "sum_logprobs", "suppress", "n_suppress",
          "blank", "n_blank", "sample_begin", "eot", "timestamp_begin", "max_initial_timestamp_index", "apply_rules", "n_past_dev",
          "row_limit", "done", "n_done")


@pytest.mark.parametrize("options,apply_rules,max_initial", [
    (dict(), 1, 50),                                           # 1.0 s / 0.02 s
    (dict(without_timestamps=True), 2, -1),
    (dict(max_initial_timestamp=None), 1, -1),
    (dict(suppress_blank=False, suppress_tokens=None), 1, 50),
])
def test_greedy_and_beam_step_get_the_same_rule_fields(engine_dir, options, apply_rules, max_initial):
    greedy_names = {n for n, _ in native.WmGreedyIO._fields_}
    beam_names = {n for n, _ in native.WmBeamIO._fields_}
    assert set(COMMON) == (greedy_names & beam_names), "the structs share other fields than the filler writes"
    dec = WhisperDecoding(engine_dir, only_torch=True, options=DecodingOptions(beam_size=2, **options))
    st = dec._fast_state(6, torch.device("cpu"))
    counter = torch.zeros(1, dtype=torch.int32)
    V = dec.decoder_config['vocab_size']
    for lo, hi, n_past_dev in ((0, 6, None), (2, 4, counter)):
        g, b = native.WmGreedyIO(), native.WmBeamIO()
        for io in (g, b):
            dec._fill_rules(io, st, lo, hi, st['logits'].data_ptr() + 2 * V, 3 * V, 7, n_past_dev)
        for name in COMMON:
            assert getattr(g, name) == getattr(b, name), name
        assert (g.batch, g.n_vocab, g.cur_len, g.row_stride, g.tokens_ld) == (hi - lo, V, 7, 3 * V, st['tokens'].shape[1])
        assert (g.logits, g.tokens) == (st['logits'].data_ptr() + 2 * V, st['tokens'][lo:hi].data_ptr())
        assert (g.sum_logprobs, g.done, g.row_limit) == (st['sum_logprobs'][lo:hi].data_ptr(), st['done'][lo:hi].data_ptr(),
                                                          st['row_limit'][lo:hi].data_ptr())
        assert g.n_done == st['n_done'].data_ptr() and g.n_past_dev == (None if n_past_dev is None else counter.data_ptr())
        assert (g.apply_rules, g.max_initial_timestamp_index) == (apply_rules, max_initial)
        assert (g.sample_begin, g.eot, g.timestamp_begin) == (dec.sample_begin, dec.tokenizer.eot, dec.tokenizer.timestamp_begin)
        assert (g.n_suppress, g.n_blank) == (st['n_suppress'], st['n_blank'])
        assert (g.suppress, g.blank) == (st['suppress'].data_ptr(), st['blank'].data_ptr())
