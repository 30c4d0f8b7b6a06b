"""Speculative decoding, the host contract (speculative.py): the accept rule, the round bookkeeping, the literal loop over two toy models
and the refusals.  No GPU."""
import os
import random
import re

import pytest

import native
import speculative as S
from decoding import DecodingOptions

EOT, V = 19, 20
START = [1, 2, 3]


def toy_model(seed, eot_bias=0.0):
    """A deterministic function from a token history to a logits row of V entries (a fresh pseudo-random row per history)."""
    def model(history):
        rnd = random.Random(f"{seed}:{','.join(map(str, history))}")
        row = [rnd.random() for _ in range(V)]
        row[EOT] += eot_bias
        return row
    return model


def wrong_at(model, positions):
    """`model`, but at the scripted history lengths it proposes another token than the model's arg-max."""
    def draft(history):
        row = list(model(history))
        if len(history) in positions:
            best = max(range(V), key=lambda i: (row[i], -i))
            row[(best + 1) % (V - 1)] = row[best] + 1.0          # never EOT: the scripted error is a wrong text token
        return row
    return draft


@pytest.mark.parametrize("k", [1, 2, 3])
def test_accept_rule_and_bookkeeping_at_every_accept_length(k):
    """n_accept 1 .. k + 1 from a mismatch at every position, from an EOT at every position and from full agreement; the cache lengths
    after the round; a row that is done (n_accept 0) and lengths outside the round are no round at all."""
    proposals = [5 + j for j in range(k)]
    T = 7
    for j in range(k):                                     # the main model disagrees at position j: j + 1 slots are written
        picks = proposals[:j] + [4] + [9] * (k - j)
        assert S.accept_length(picks, proposals, EOT) == j + 1
        assert S.after_round(T, k, j + 1) == (T + j + 1, T + j + 1)          # both caches are one behind the row: a 1-token catch-up
    assert S.accept_length(proposals + [11], proposals, EOT) == k + 1        # all proposals kept and the token behind them
    assert S.after_round(T, k, k + 1) == (T + k + 1, T + k)                  # the draft never saw the last proposal: 2 tokens behind the row
    for j in range(k + 1):                                 # EOT at position j ends the round there, proposed or not
        picks = proposals[:j] + [EOT] + [9] * (k - j)
        assert S.accept_length(picks, proposals, EOT) == j + 1
        with_eot = proposals[:j] + [EOT] + proposals[j + 1:]
        assert S.accept_length(picks, with_eot[:k], EOT) == j + 1
    for n_accept in (0, k + 2):
        with pytest.raises(ValueError):
            S.after_round(T, k, n_accept)
    with pytest.raises(ValueError):
        S.accept_length([1, 2], [1, 2], EOT)


def test_proposals_per_round_shrinks_with_the_room():
    """k = min(draft_tokens, room - 1): the room is what sample_len and the context leave; 0 is a plain step, None the end."""
    assert S.proposals_per_round(3, 1, 100, 5, 448) == 3
    assert S.proposals_per_round(2, 1, 100, 5, 448) == 2
    assert [S.proposals_per_round(3, n, 10, 5 + n, 448) for n in (6, 7, 8, 9, 10)] == [3, 2, 1, 0, None]       # sample_len
    assert [S.proposals_per_round(3, 1, 100, n, 32) for n in (28, 29, 30, 31, 32, 33)] == [3, 3, 2, 1, 0, None]  # the context's end
    assert S.MAX_DRAFT_TOKENS == 3 and S.MAX_PASS_TOKENS == 4


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("draft_kind", ["itself", "unrelated", "scripted"])
def test_the_literal_loop_is_plain_greedy_decoding(draft_kind, k):
    """Whatever the draft proposes, the tokens are EXACTLY those of the main model's greedy decoding; rounds never exceed tokens; with
    the main model as its own draft every round keeps all its proposals, with an unrelated one (almost) none."""
    for seed in range(6):
        main = toy_model(seed, eot_bias=0.12 if seed % 2 else -5.0)          # odd seeds end by EOT, even ones by sample_len
        draft = {"itself": main, "unrelated": toy_model(1000 + seed), "scripted": wrong_at(main, {5, 6, 9, 14, 15, 16, 22})}[draft_kind]
        for sample_len in (1, 2, 5, 17, 40):
            trace = []
            row, stats = S.speculative_greedy(main, draft, START, EOT, sample_len, 64, k, trace)
            plain = S.plain_greedy(main, START, EOT, sample_len, 64)
            assert row == plain, (seed, sample_len)
            assert stats["tokens"] == len(row) - len(START) and stats["rounds"] <= stats["tokens"]
            assert stats["rounds"] == len(trace) and stats["proposals"] == sum(len(p) for _, p, _ in trace)
            assert 1 + sum(n for _, _, n in trace) == stats["tokens"] and stats["accepted"] == sum(n - 1 for _, _, n in trace)
            at = len(START)                                # T of every round is the main cache's length: the row's length - 1
            for T, proposals, n in trace:
                assert T == at and 1 <= n <= len(proposals) + 1 and row[T + 1:T + n] == list(proposals[:n - 1])
                at += n
            if draft_kind == "itself":
                full = [n == len(p) + 1 or row[T + n] == EOT for T, p, n in trace]
                assert all(full)
                if sample_len == 40 and seed % 2 == 0:
                    assert stats["rounds"] == -(-39 // (k + 1))              # k + 1 tokens per round, the last one what is left
            if draft_kind == "scripted" and sample_len == 40 and seed % 2 == 0:
                assert any(n == 1 for _, p, n in trace if p) and any(n == len(p) + 1 for _, p, n in trace if p)


def test_the_loop_ends_by_eot_by_sample_len_and_at_the_contexts_end():
    main = toy_model(3, eot_bias=-5.0)
    trace = []
    row, stats = S.speculative_greedy(main, main, START, EOT, 100, 12, 3, trace)          # the context's end: the row grows to 13 tokens
    assert len(row) == 13 and row == S.plain_greedy(main, START, EOT, 100, 12)
    assert [len(p) for _, p, _ in trace] == [3, 3, 0]          # 4 -> 8 -> 12 -> 13 tokens: k shrinks with the room, down to 0
    for n_ctx in range(5, 14):
        tr = []
        row, _ = S.speculative_greedy(main, toy_model(77), START, EOT, 100, n_ctx, 3, tr)
        assert row == S.plain_greedy(main, START, EOT, 100, n_ctx) and len(row) == n_ctx + 1
        assert all(T + 1 + len(p) <= n_ctx for T, p, _ in tr)          # no pass feeds a position beyond the context
    assert any(len(p) == 0 for _, p, _ in tr)
    ender = toy_model(5, eot_bias=0.3)
    row, stats = S.speculative_greedy(ender, ender, START, EOT, 100, 64, 3)
    assert row[-1] == EOT and row.count(EOT) == 1 and row == S.plain_greedy(ender, START, EOT, 100, 64)
    row, stats = S.speculative_greedy(main, main, START, EOT, 7, 64, 3)
    assert len(row) == len(START) + 7 and stats["tokens"] == 7
    assert S.speculative_greedy(main, main, START, EOT, 0, 64, 3)[0] == START


def test_refusals():
    ok = DecodingOptions()
    S.check_draft(3, ok)
    for bad in (0, 4, -1, 2.0, None, True):
        with pytest.raises(ValueError, match="draft_tokens"):
            S.check_draft(bad, ok)
    for name, options in (("beam_size", DecodingOptions(beam_size=2)), ("best_of", DecodingOptions(best_of=2, temperature=0.5)),
                          ("repetition_penalty", DecodingOptions(repetition_penalty=1.2)),
                          ("no_repeat_ngram_size", DecodingOptions(no_repeat_ngram_size=3)),
                          ("hotwords", DecodingOptions(hotwords=((1, 2),))), ("sequence_bias", DecodingOptions(sequence_bias=(((1, 2), 1.0),)))):
        with pytest.raises(ValueError, match=name):
            S.check_draft(3, options)
    for kw, word in ((dict(row_prompts=True), "row_prompts"), (dict(shared_cross_kv=True), "shared_cross_kv"),
                     (dict(fallback_best_of=1), "fallback_best_of")):
        with pytest.raises(ValueError, match=word):
            S.check_draft(3, ok, **kw)
    dims = dict(n_audio_state=1280, n_audio_ctx=1500, n_text_ctx=448, n_vocab=51866, n_text_layer=32)
    S.check_draft(3, ok, main_dims=dims, draft_dims=dict(dims, n_text_layer=2))
    for name in S.SHARED_DIMS:
        with pytest.raises(ValueError, match=name):
            S.check_draft(3, ok, main_dims=dims, draft_dims=dict(dims, **{name: dims[name] - 1}))


def test_binding_header_and_makefile_name_the_entry():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "whisper_mi355.h")) as f:
        header = f.read()
    assert "int wm_verify_step(" in header and "size_t wm_verify_workspace_bytes(" in header and "typedef struct wm_verify_io" in header
    assert re.search(r"#define WM_ABI_VERSION 8\b", header) and native.ABI_VERSION == 8
    assert "wm_verify_step" in native.EXPORTS and "wm_verify_workspace_bytes" in native.EXPORTS
    fields = [name for name, _ in native.WmVerifyIO._fields_]
    assert fields == ["g", "pos_stride", "n_pos", "n_accept", "workspace"]
    with open(os.path.join(os.path.dirname(native.__file__), "csrc", "Makefile")) as f:
        assert "speculative.hip" in f.read()
    lib = native.load_library()
    assert lib.wm_verify_workspace_bytes(5, 4) == 5 * 4 * 8
