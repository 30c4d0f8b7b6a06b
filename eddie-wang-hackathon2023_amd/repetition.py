"""Repetition penalty and no-repeat n-grams: the contract, in numpy.

The two controls of CTranslate2 / faster-whisper and Hugging Face generation that act inside the decode loop, token by token, against
Whisper's commonest failure on real recordings -- the same phrase emitted window after window over music, silence or noise.  This
module is their statement on the host: the device kernel (csrc/repeat.hip, wm_repeat_controls) and the torch filters of the literal
loops (decoding.RepetitionPenalty, decoding.NoRepeatNGram) must give the same fp16 bits, and the CPU tests
(tests/test_repeat_cpu.py) hold all of them to a brute-force restatement.

For one row at a token step:
  H = tokens[sample_begin : cur_len], m = len(H): what the row has SAMPLED so far.  The start sequence and the prompt
  (initial_prompt, the previous text of long-form transcription, row_prompts) are not part of H: a prompt exists to make its words
  more likely, not less.  (Hugging Face counts the whole input, prompt included.)
  Only text tokens (id < eot) are ever changed: EOT, the specials and the timestamps belong to Whisper's own rules -- a closing /
  opening timestamp pair repeats by design.

  repetition penalty p (finite, > 0; 1.0 = off): for every DISTINCT t of H with t < eot, once however often it occurs,
      x = float32(logits[t]);  y = x / p if x > 0 else x * p, one float32 operation, correctly rounded;  logits[t] = float16(y),
      round to nearest even.  -inf stays -inf.  (The rule of Hugging Face's RepetitionPenaltyLogitsProcessor and CTranslate2.)
  no-repeat n-grams n (integer >= 0; 0 = off): if m >= n - 1, for every i in 0 .. m - n with H[i : i + n - 1] == H[m - n + 1 : m]
      the token H[i + n - 1] is banned if it is < eot: logits[t] = -inf.  Matching runs over H as it is, timestamps included; only
      text tokens are banned.  n = 1 bans every text token already sampled.

Penalty first, then bans, both on the raw fp16 logits of the last position, in place, BEFORE Whisper's own filters (suppress lists,
timestamp rules), the order Hugging Face uses.  The log-probabilities the token step books (sum_logprobs, hence avg_logprob and the
logprob_threshold of the fallback ladder) are those of the distribution after the controls, exactly as they already are after the
suppress lists.  Text bans can never empty a row: Whisper's rules never depend on a particular text token being available.
"""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np

MAX_HISTORY = 512        # WM_REPEAT_MAX_HISTORY of include/whisper_mi355.h: the longest H the kernel takes (>= n_text_ctx = 448)


def check_controls(repetition_penalty, no_repeat_ngram_size) -> None:
    """ValueError unless the penalty is finite and > 0 and the n-gram size an integer >= 0."""
    try:
        p = float(repetition_penalty)
    except (TypeError, ValueError):
        raise ValueError(f"repetition_penalty {repetition_penalty!r} is not a number") from None
    if not math.isfinite(p) or p <= 0:
        raise ValueError(f"repetition_penalty {repetition_penalty!r} must be finite and > 0 (1.0 = off)")
    n = no_repeat_ngram_size
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
        raise ValueError(f"no_repeat_ngram_size {no_repeat_ngram_size!r} must be an integer >= 0 (0 = off)")


def controls_on(repetition_penalty, no_repeat_ngram_size) -> bool:
    return float(repetition_penalty) != 1.0 or int(no_repeat_ngram_size) != 0


def add_arguments(parser) -> None:
    """The two flags run.py, summarize.py and transcribe.py share."""
    parser.add_argument('--repetition_penalty', type=float, default=1.0, help='repetition penalty inside the decode loop: logits of text tokens already sampled are divided (positive) / multiplied (else) by it (1.0 = off; the prompt is not counted)')
    parser.add_argument('--no_repeat_ngram_size', type=int, default=0, help='no n-gram of sampled tokens of this size may end in the same text token twice (0 = off; the prompt is not counted)')


def options_from_args(repetition_penalty=1.0, no_repeat_ngram_size=0) -> dict:
    """The DecodingOptions fields of the two flags (`add_arguments`)."""
    return dict(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size)


def penalized_tokens(history: np.ndarray, eot: int) -> np.ndarray:
    """The distinct text tokens of H, ascending: each is penalised once."""
    h = np.asarray(history, dtype=np.int64).reshape(-1)
    return np.unique(h[(h >= 0) & (h < eot)])


def banned_tokens(history: np.ndarray, n: int, eot: int) -> np.ndarray:
    """The text tokens that would complete an n-gram H already holds, ascending (empty for n = 0 or m < n - 1)."""
    h = np.asarray(history, dtype=np.int64).reshape(-1)
    m = h.shape[0]
    if n <= 0 or m < n - 1 or m - n + 1 <= 0:
        return np.zeros(0, dtype=np.int64)
    nxt = h[n - 1:]                                              # H[i + n - 1] for i = 0 .. m - n
    match = np.ones(m - n + 1, dtype=bool)
    for k in range(n - 1):                                       # H[i + k] == H[m - n + 1 + k]
        match &= h[k: k + m - n + 1] == h[m - n + 1 + k]
    t = nxt[match]
    return np.unique(t[(t >= 0) & (t < eot)])


def apply_row(logits: np.ndarray, history: Sequence[int], eot: int, repetition_penalty: float = 1.0,
              no_repeat_ngram_size: int = 0) -> np.ndarray:
    """The controls on one row of float16 logits [n_vocab], in place (and returned): `history` is H."""
    assert logits.dtype == np.float16 and logits.ndim == 1
    check_controls(repetition_penalty, no_repeat_ngram_size)
    h = np.asarray(history, dtype=np.int64).reshape(-1)
    p = np.float32(repetition_penalty)
    if p != np.float32(1.0):
        t = penalized_tokens(h, eot)
        x = logits[t].astype(np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            y = np.where(x > 0, x / p, x * p).astype(np.float32)
            logits[t] = y.astype(np.float16)
    logits[banned_tokens(h, int(no_repeat_ngram_size), eot)] = -np.inf
    return logits


def apply(logits: np.ndarray, tokens: np.ndarray, sample_begin: int, cur_len: int, eot: int, repetition_penalty: float = 1.0,
          no_repeat_ngram_size: int = 0, done: Sequence[int] = None) -> np.ndarray:
    """The controls on a batch, as wm_repeat_controls takes it: float16 logits [batch, n_vocab] (the last position's), tokens
    [batch, >= cur_len]; a row whose `done` flag is set is left untouched."""
    for b in range(logits.shape[0]):
        if done is not None and done[b]:
            continue
        apply_row(logits[b], tokens[b, sample_begin:cur_len], eot, repetition_penalty, no_repeat_ngram_size)
    return logits
