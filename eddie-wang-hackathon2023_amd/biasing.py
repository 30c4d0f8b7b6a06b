"""Hotwords and sequence bias: the contract, in numpy.

The lever for vocabulary -- product names, surnames, drug names, part numbers that Whisper spells phonetically -- that acts inside the
decode loop, token by token: a bias on the logits.  Two forms exist elsewhere and both fill ONE table here: Hugging Face's
`sequence_bias` raises or lowers the token that would COMPLETE a listed sequence; contextual biasing ("shallow fusion") boosts every
token that CONTINUES a listed phrase (`hotwords`).  This module is their statement on the host: the device kernel (csrc/bias.hip,
wm_sequence_bias) and the torch filter of the literal loops (host_decoding.SequenceBias) must give the same fp16 bits, and the CPU
tests (tests/test_bias_cpu.py) hold all of them to a brute-force restatement (tests/bias_refs.py).

The table is a list of items (target, k, prefix, bias): "if the last k tokens of H equal `prefix` (k tokens; k = 0 always matches,
also on an empty H), token `target` gets `bias`".  H = tokens[sample_begin : cur_len] is what the row has SAMPLED, exactly as in
repetition.py: the start sequence and any prompt are not in it, and matching runs over H as it is, timestamps included -- a timestamp
between two words breaks a phrase.

For one row at a token step:
  for every text token t, among the matching items whose target is t the one with the greatest k wins; two at equal k: the earlier
  one in table order.  Exactly ONE update is applied per token:  x = float32(logits[t]);  y = x + bias, one correctly rounded float32
  addition;  logits[t] = float16(y), round to nearest even.  -inf stays -inf.  Biases are never summed across items: the result does
  not depend on the order of evaluation.  Only text tokens (id < eot) may be targets or stand in a prefix (`build_table` refuses
  anything else).  A row whose `done` flag is set is left untouched.

Order in the step: the repetition controls (penalty, then bans), then this bias, then Whisper's own rules (suppress lists, timestamp
rules).  A token banned by the n-gram rule stays banned (-inf + bias = -inf), a suppressed token stays suppressed.  The
log-probabilities the token step books (sum_logprobs, hence avg_logprob and the logprob_threshold of the fallback ladder) are those
of the distribution AFTER the bias, exactly as they already are after the repetition controls.

Two ways to fill the table, one builder (`build_table`):
  sequence_bias  ((s, v), ...): one item (s[-1], len(s) - 1, s[:-1], v) per sequence -- Hugging Face's rule; v may be negative.
  hotwords       (p, ...): for a phrase p the items (p[k], k, p[:k], hotword_bias) for k >= 1 and (p[0], 0, (), hotword_start_bias):
                 a boost at every position.  A string w is encoded twice, as " " + w and as w, and both token sequences are phrases
                 (needs a tokenizer with a vocabulary); a tuple of token ids is one phrase.
Items with identical (target, prefix) are merged, the greater bias stands.  The items are sorted by (target ascending, k descending):
the order the kernel's single-writer rule needs.  Bounds, all ValueError at construction: k <= 31 (a phrase has at most 32 tokens), at
most MAX_ITEMS = 4096 items, at most MAX_POOL = 4096 prefix tokens (a prefix that is the head of a stored one shares its tokens: a
hotword of n tokens takes n - 1), every bias finite with |bias| <= 1e4.

The defaults hotword_bias = 3.0 and hotword_start_bias = 1.5 are parameters, not measurements: nobody has tuned them on speech.

A difference from shallow-fusion implementations: the rule is STATELESS.  A partial match that then fails gets nothing taken back, and
under beam search the boosted log-probabilities stay in the beam scores.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

MAX_ITEMS = 4096         # WM_BIAS_MAX_ITEMS of include/whisper_mi355.h
MAX_POOL = 4096          # WM_BIAS_MAX_POOL: prefix tokens
MAX_K = 31               # WM_BIAS_MAX_K: the longest prefix (a phrase has at most 32 tokens)
MAX_BIAS = 1e4
HOTWORD_BIAS = 3.0
HOTWORD_START_BIAS = 1.5
ITEM_DTYPE = np.dtype([("target", "<i4"), ("k", "<i4"), ("offset", "<i4"), ("bias", "<f4")])      # wm_bias_item, 16 bytes

Item = Tuple[int, int, Tuple[int, ...], float]


def _bias_value(v, what: str) -> float:
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{what} {v!r} is not a number") from None
    if isinstance(v, bool) or not math.isfinite(f) or abs(f) > MAX_BIAS:
        raise ValueError(f"{what} {v!r} must be finite with |bias| <= {MAX_BIAS:g}")
    return float(np.float32(f))


def _ids(seq, what: str) -> Tuple[int, ...]:
    if isinstance(seq, (str, bytes)) or not isinstance(seq, (tuple, list, np.ndarray)):
        raise ValueError(f"{what} {seq!r} must be a tuple of token ids")
    out = []
    for t in seq:
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or t < 0:
            raise ValueError(f"{what} {seq!r}: {t!r} is not a token id")
        out.append(int(t))
    if not 1 <= len(out) <= MAX_K + 1:
        raise ValueError(f"{what}: a phrase has 1 .. {MAX_K + 1} tokens, not {len(out)}")
    return tuple(out)


def check_options(hotwords, hotword_bias, hotword_start_bias, sequence_bias) -> None:
    """ValueError unless the four options have the shapes `build_table` takes (what can be said without a tokenizer: that the ids are
    text tokens and that the table fits its bounds is checked where the table is built, at construction of the decoder)."""
    _bias_value(hotword_bias, "hotword_bias")
    _bias_value(hotword_start_bias, "hotword_start_bias")
    if hotwords is not None:
        if isinstance(hotwords, (str, bytes)) or not isinstance(hotwords, (tuple, list)):
            raise ValueError(f"hotwords {hotwords!r} must be a tuple of strings and / or token tuples")
        for w in hotwords:
            if isinstance(w, str):
                if not w.strip():
                    raise ValueError("hotwords: an empty string")
            else:
                _ids(w, "hotwords:")
    if sequence_bias is not None:
        if isinstance(sequence_bias, (str, bytes)) or not isinstance(sequence_bias, (tuple, list)):
            raise ValueError(f"sequence_bias {sequence_bias!r} must be a tuple of (token tuple, bias) pairs")
        for pair in sequence_bias:
            if not isinstance(pair, (tuple, list)) or len(pair) != 2:
                raise ValueError(f"sequence_bias: {pair!r} is not a (token tuple, bias) pair")
            _ids(pair[0], "sequence_bias:")
            _bias_value(pair[1], "sequence_bias: bias")


def bias_on(hotwords, sequence_bias) -> bool:
    return bool(hotwords) or bool(sequence_bias)


def add_arguments(parser) -> None:
    """The four flags run.py, summarize.py and transcribe.py share."""
    parser.add_argument('--hotwords', type=str, default=None,
                        help='comma-separated words or phrases (names, part numbers) whose tokens are boosted inside the decode loop at every '
                             'position, e.g. "Kubernetes,MI355X" (needs a vocabulary: --vocab)')
    parser.add_argument('--hotword_bias', type=float, default=HOTWORD_BIAS,
                        help=f'added to the logit of the token that continues a hotword (default {HOTWORD_BIAS}: a parameter, not tuned on speech)')
    parser.add_argument('--hotword_start_bias', type=float, default=HOTWORD_START_BIAS,
                        help=f'added to the logit of the first token of every hotword, at every step (default {HOTWORD_START_BIAS})')
    parser.add_argument('--sequence_bias_file', type=str, default=None,
                        help='JSON list of [[token, ...], bias]: the token that would complete a listed sequence gets the bias (may be negative)')


def options_from_args(hotwords=None, hotword_bias=HOTWORD_BIAS, hotword_start_bias=HOTWORD_START_BIAS, sequence_bias_file=None) -> dict:
    """The DecodingOptions fields of the four flags (`add_arguments`)."""
    import json
    words = tuple(w.strip() for w in hotwords.split(",") if w.strip()) if hotwords else None
    seqs = None
    if sequence_bias_file:
        with open(sequence_bias_file) as f:
            entries = json.load(f)
        if not isinstance(entries, list) or any(not isinstance(e, list) or len(e) != 2 or not isinstance(e[0], list) for e in entries):
            raise ValueError(f"{sequence_bias_file}: need a JSON list of [[token, ...], bias]")
        seqs = tuple((tuple(e[0]), e[1]) for e in entries) or None
    return dict(hotwords=words or None, hotword_bias=hotword_bias, hotword_start_bias=hotword_start_bias, sequence_bias=seqs)


class Table:
    """A built table: `items` [(target, k, prefix, bias)] sorted by (target ascending, k descending), and the two arrays the device
    reads -- `packed` (ITEM_DTYPE [n]: target, k, offset into the pool, fp32 bias) and `pool` (int32: the prefixes' tokens)."""

    def __init__(self, items: List[Item]):
        self.items = items
        pool: List[int] = []
        where = {(): 0}
        packed = np.zeros(len(items), dtype=ITEM_DTYPE)
        for i in sorted(range(len(items)), key=lambda i: -items[i][1]):          # longest prefixes first: the shorter ones are heads of them
            prefix = items[i][2]
            if prefix not in where:
                off = len(pool)
                pool.extend(prefix)
                for n in range(1, len(prefix) + 1):
                    where.setdefault(prefix[:n], off)
            packed[i] = (items[i][0], items[i][1], where[prefix], items[i][3])
        if len(pool) > MAX_POOL:
            raise ValueError(f"the bias table's prefixes hold {len(pool)} tokens, more than {MAX_POOL}")
        self.packed, self.pool = packed, np.asarray(pool, dtype=np.int32)

    def __len__(self) -> int:
        return len(self.items)


def phrases_of(hotword, tokenizer) -> List[Tuple[int, ...]]:
    """The token sequences of one hotword: a string is encoded as " " + w and as w; a tuple of ids is itself."""
    if not isinstance(hotword, str):
        return [_ids(hotword, "hotwords:")]
    if tokenizer is None or getattr(tokenizer, "bpe", None) is None:
        raise ValueError(f"hotwords: the string {hotword!r} needs a tokenizer built with a vocabulary (an ids-only tokenizer takes token tuples)")
    w = hotword.strip()
    if not w:
        raise ValueError("hotwords: an empty string")
    out = []
    for text in (" " + w, w):
        p = _ids(tuple(tokenizer.encode(text)), f"hotwords: {hotword!r} ->")
        if p not in out:
            out.append(p)
    return out


def build_table(hotwords=None, sequence_bias=None, hotword_bias: float = HOTWORD_BIAS, hotword_start_bias: float = HOTWORD_START_BIAS, *,
                eot: int, tokenizer=None) -> Table:
    """The table of the two options (module docstring): merged, sorted, within its bounds -- or ValueError."""
    check_options(hotwords, hotword_bias, hotword_start_bias, sequence_bias)
    hb, sb = _bias_value(hotword_bias, "hotword_bias"), _bias_value(hotword_start_bias, "hotword_start_bias")
    raw: List[Item] = []
    for seq, v in (sequence_bias or ()):
        s = _ids(seq, "sequence_bias:")
        raw.append((s[-1], len(s) - 1, s[:-1], _bias_value(v, "sequence_bias: bias")))
    for w in (hotwords or ()):
        for p in phrases_of(w, tokenizer):
            raw.append((p[0], 0, (), sb))
            raw.extend((p[k], k, p[:k], hb) for k in range(1, len(p)))
    merged = {}
    for target, k, prefix, bias in raw:
        bad = [t for t in (target,) + prefix if t >= eot]
        if bad:
            raise ValueError(f"bias table: token {bad[0]} is not a text token (id < eot = {eot}): specials and timestamps can be neither "
                             "biased nor matched")
        key = (target, prefix)
        merged[key] = max(merged.get(key, -math.inf), bias)                     # identical (target, prefix): the greater bias stands
    if len(merged) > MAX_ITEMS:
        raise ValueError(f"the bias table holds {len(merged)} items, more than {MAX_ITEMS}")
    items = [(t, len(p), p, b) for (t, p), b in merged.items()]
    items.sort(key=lambda it: (it[0], -it[1]))                                  # (stable: equal (target, k) keep their order)
    return Table(items)


def winners(items: Sequence[Item], history: Sequence[int]) -> dict:
    """{target: bias} of the items that win on H: per target the matching item of greatest k, the earlier one at equal k."""
    h = [int(t) for t in history]
    m = len(h)
    best = {}
    for target, k, prefix, bias in items:
        if k > m or tuple(h[m - k:]) != tuple(prefix):
            continue
        if target not in best or k > best[target][0]:
            best[target] = (k, bias)
    return {t: b for t, (_, b) in best.items()}


def apply_row(logits: np.ndarray, history: Sequence[int], eot: int, table) -> np.ndarray:
    """The bias on one row of float16 logits [n_vocab], in place (and returned): `history` is H, `table` a Table or a list of items."""
    assert logits.dtype == np.float16 and logits.ndim == 1
    items = table.items if isinstance(table, Table) else table
    won = {t: b for t, b in winners(items, history).items() if 0 <= t < eot}
    if won:
        t = np.fromiter(won.keys(), dtype=np.int64, count=len(won))
        b = np.fromiter(won.values(), dtype=np.float32, count=len(won))
        with np.errstate(over="ignore", invalid="ignore"):
            y = (logits[t].astype(np.float32) + b).astype(np.float32)
            logits[t] = y.astype(np.float16)
    return logits


def apply(logits: np.ndarray, tokens: np.ndarray, sample_begin: int, cur_len: int, eot: int, table, done: Optional[Sequence[int]] = None) -> np.ndarray:
    """The bias on a batch, as wm_sequence_bias takes it: float16 logits [batch, n_vocab] (the last position's), tokens
    [batch, >= cur_len]; a row whose `done` flag is set is left untouched."""
    for b in range(logits.shape[0]):
        if done is not None and done[b]:
            continue
        apply_row(logits[b], tokens[b, sample_begin:cur_len], eot, table)
    return logits
