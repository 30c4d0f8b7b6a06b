"""Speculative decoding: the host contract (plain Python, no GPU, no torch).

A small DRAFT model proposes the next k tokens one at a time; ONE pass of the MAIN model over "last token + k proposals" gives the
main model's own choice at k + 1 positions; the longest prefix of proposals the main model agrees with is kept, plus the main
model's token at the first disagreement (or behind the last proposal).  At temperature 0 the result is the main model's greedy
decoding, whatever the draft proposes: every token that stays in the row is the main model's arg-max on a history of tokens that
are themselves the main model's.  The draft only decides how many tokens a pass yields: 1 to k + 1.

This module states, for csrc/speculative.hip (wm_verify_step), speculative_loop.py (the device loop) and the tests:
  * `accept_length`: the accept rule of one row of one round;
  * `proposals_per_round`, `after_round`: the round bookkeeping -- cache lengths of the two models and the proposals that fit;
  * `speculative_greedy`: the literal loop over two abstract models given as functions from a token history to a logits row;
  * `check_draft`: what an instance with a draft refuses.

Differences from Hugging Face's `assistant_model`:
  * Whisper's logit rules (suppress lists, timestamp rules) apply to the draft's proposals as well: a proposal the rules forbid
    could never be accepted;
  * at most MAX_DRAFT_TOKENS = 3 proposals per round, fixed: a verify pass holds 4 tokens (wm_decoder_step's n_new);
  * the rows of a batch are decoded one after another (a latency mode: the cost is linear in the rows).
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

MAX_PASS_TOKENS = 4                       # wm_decoder_step takes n_new = 1 .. 4 on a cache that holds tokens already
MAX_DRAFT_TOKENS = MAX_PASS_TOKENS - 1    # the pass also carries the last accepted token

SHARED_DIMS = ("n_audio_state", "n_audio_ctx", "n_text_ctx", "n_vocab")      # what a draft must share with the main engine


def accept_length(picks: Sequence[int], proposals: Sequence[int], eot: int) -> int:
    """The slots one row fills in one round.  picks[j] is the main model's token at position j GIVEN that proposals[0 .. j - 1] were
    kept (len(picks) = len(proposals) + 1 = n_pos); the walk writes picks[j] and stops when it is EOT, when j is the last position,
    or when it differs from proposals[j].  1 .. n_pos."""
    n_pos = len(picks)
    if n_pos != len(proposals) + 1 or n_pos < 1:
        raise ValueError(f"accept_length: {n_pos} picks need {n_pos - 1} proposals, got {len(proposals)}")
    for j in range(n_pos):
        if picks[j] == eot or j == n_pos - 1 or picks[j] != proposals[j]:
            return j + 1
    raise AssertionError("unreachable")


def proposals_per_round(draft_tokens: int, n_sampled: int, sample_len: int, n_tokens: int, n_text_ctx: int) -> Optional[int]:
    """k of the next round of a row that holds `n_tokens` tokens, `n_sampled` of them sampled: min(draft_tokens, room - 1), where room
    is what may still be sampled -- sample_len - n_sampled, and slots up to n_text_ctx (the row may grow to n_text_ctx + 1 tokens, as in
    the plain loop: the token at position n_text_ctx - 1 is the last one fed).  None: no room, the row has ended.  k = 0 is a plain
    step through the verify entry (one position, no proposal)."""
    room = min(sample_len - n_sampled, n_text_ctx + 1 - n_tokens)
    if room <= 0:
        return None
    return min(int(draft_tokens), room - 1)


def after_round(T: int, k: int, n_accept: int) -> Tuple[int, int]:
    """(T', Td'): the tokens the main and the draft cache hold VALID entries for after a round that began with a main cache of T tokens
    (the row held T + 1), proposed k and wrote n_accept slots.  The main pass wrote k + 1 cache entries, the draft k (k >= 1) on top
    of T; an entry is valid when the token it was computed from stayed in the row.  T' = T + n_accept; Td' = T + min(n_accept, k):
    after a fully accepted round (n_accept = k + 1) the draft is two tokens behind the row and catches up with a 2-token pass, else
    one.  With k = 0 the draft cache is not touched."""
    if not 0 <= k <= MAX_DRAFT_TOKENS or not 1 <= n_accept <= k + 1:
        raise ValueError(f"after_round: k = {k}, n_accept = {n_accept}")
    return T + n_accept, T + min(n_accept, k)


Model = Callable[[List[int]], Sequence[float]]       # token history -> one logits row (rules applied: -inf = not allowed)


def _argmax(row: Sequence[float]) -> int:
    best, at = None, -1
    for i, x in enumerate(row):
        if best is None or x > best:                 # first index wins ties, as the kernels do
            best, at = x, i
    return at


def plain_greedy(main: Model, start: Sequence[int], eot: int, sample_len: int, n_text_ctx: int) -> List[int]:
    """Greedy decoding of `main` alone: what speculative_greedy must reproduce."""
    row = list(start)
    for _ in range(sample_len):
        if len(row) > n_text_ctx:
            break
        row.append(_argmax(main(row)))
        if row[-1] == eot:
            break
    return row


def speculative_greedy(main: Model, draft: Model, start: Sequence[int], eot: int, sample_len: int, n_text_ctx: int,
                       draft_tokens: int = MAX_DRAFT_TOKENS, trace: Optional[list] = None) -> Tuple[List[int], dict]:
    """The literal loop.  Returns the row and the counts of `speculative_stats` (rounds, proposals, accepted = the
    tokens the rounds yielded beyond one each, tokens = all sampled tokens).  `trace` collects (T, proposals, n_accept) per round,
    T = the main cache's length when the round began.  The first sampled token is the main model's (the prefill's token step)."""
    check_draft_tokens(draft_tokens)
    row = list(start)
    stats = dict(rounds=0, proposals=0, accepted=0, tokens=0)
    if sample_len < 1 or len(row) > n_text_ctx:
        return row, stats
    row.append(_argmax(main(row)))
    stats["tokens"] = 1
    T = Td = len(row) - 1
    while row[-1] != eot:
        k = proposals_per_round(draft_tokens, stats["tokens"], sample_len, len(row), n_text_ctx)
        if k is None:
            break
        assert len(row) - Td in (1, 2) or k == 0         # the draft catches up with one pass of 1 or 2 tokens
        proposals: List[int] = []
        for _ in range(k):
            proposals.append(_argmax(draft(row + proposals)))
        picks = [_argmax(main(row + proposals[:j])) for j in range(k + 1)]
        n = accept_length(picks, proposals, eot)
        if trace is not None:
            trace.append((T, tuple(proposals), n))
        row += picks[:n]
        T, Td = after_round(T, k, n) if k else (T + n, Td)
        stats["rounds"] += 1
        stats["proposals"] += k
        stats["accepted"] += n - 1                     # what the round yields beyond the one token a main pass gives anyway
        stats["tokens"] += n
    return row, stats


def check_draft_tokens(draft_tokens) -> int:
    if isinstance(draft_tokens, bool) or not isinstance(draft_tokens, int) or not 1 <= draft_tokens <= MAX_DRAFT_TOKENS:
        raise ValueError(f"draft_tokens {draft_tokens!r} outside 1..{MAX_DRAFT_TOKENS}: a verify pass holds {MAX_PASS_TOKENS} tokens, "
                         f"the last accepted one and the proposals")
    return draft_tokens


def check_draft(draft_tokens, options, *, row_prompts: bool = False, shared_cross_kv: bool = False, fallback_best_of=None,
                main_dims: Optional[dict] = None, draft_dims: Optional[dict] = None) -> None:
    """What an instance with a draft engine refuses (ValueError).  `options`: anything with DecodingOptions' fields."""
    check_draft_tokens(draft_tokens)
    if options.beam_size is not None or options.best_of is not None or fallback_best_of is not None:
        raise ValueError("draft_engine_dir: beam_size / best_of / fallback_best_of are not supported (one row, one greedy candidate is verified)")
    if row_prompts:
        raise ValueError("draft_engine_dir: row_prompts is not supported")
    if shared_cross_kv:
        raise ValueError("draft_engine_dir: shared_cross_kv is not supported (there are no candidate groups to share with)")
    if options.repetition_penalty != 1.0 or options.no_repeat_ngram_size != 0:
        raise ValueError("draft_engine_dir: repetition_penalty / no_repeat_ngram_size are not supported (they would need a launch per "
                         "position in front of the verify step)")
    if options.hotwords or options.sequence_bias:
        raise ValueError("draft_engine_dir: hotwords / sequence_bias are not supported (they would need a launch per position in front of "
                         "the verify step)")
    if main_dims is not None and draft_dims is not None:
        bad = [f"{name}: {main_dims[name]} against {draft_dims[name]}" for name in SHARED_DIMS if main_dims[name] != draft_dims[name]]
        if bad:
            raise ValueError("draft_engine_dir: the draft must share the main engine's encoder output, context and vocabulary (" + "; ".join(bad) + ")")
