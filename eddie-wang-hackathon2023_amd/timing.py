"""Word-level timestamps: the host statement of the alignment contract (DESIGN.md "word timestamps").

Upstream Whisper's `find_alignment`, restated: the cross-attention scores of the alignment heads over one teacher-forced pass
are soft-maxed over frames, z-scored over tokens, median-filtered over frames and averaged over heads; dynamic time warping on
the negated matrix pairs every token with frames, and the frames at which the token index jumps are the word boundaries.

Everything here runs on the CPU and is what the device path (csrc/align.hip: wm_align, wm_dtw) is held to:
  `alignment_matrix`  steps 4-7 in torch, fp32
  `dtw_cpu`           step 8 in numpy, fp32, with the tie rule spelled out
  `words_from_path`   step 9

Two deliberate differences from upstream: a frame whose weights have no spread over the tokens (std == 0) gets Z = 0 where
upstream divides by zero, and nothing of upstream's long-form heuristics (`add_word_timestamps`' duration clamps) is applied
here: they are longform.add_word_timestamps, which long-form transcription applies to what `words_from_path` returns.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np
import torch

PREPEND_PUNCTUATIONS = "\"'“¿([{-"
APPEND_PUNCTUATIONS = "\"'.。,，!！?？:：”)]}、"
MEDIAN_FILTER_WIDTH = 7


@dataclass
class WordTiming:
    word: str
    tokens: List[int]
    start: float
    end: float
    probability: float


def median_filter(x: torch.Tensor, width: int) -> torch.Tensor:
    """Median of `width` (odd) along the last dimension with reflect padding of width // 2; a tensor whose last dimension is
    no longer than the padding comes back unfiltered (F <= 3 at width 7)."""
    pad = width // 2
    n = x.shape[-1]
    if pad == 0 or n <= pad:
        return x
    assert width % 2 == 1, "the filter width must be odd"
    g = torch.arange(-pad, n + pad)
    g = torch.where(g < 0, -g, torch.where(g >= n, 2 * (n - 1) - g, g))          # reflection about 0 and n - 1
    windows = x[..., g].unfold(-1, width, 1)                                     # [..., n, width]
    return windows.sort(dim=-1).values[..., pad]


def alignment_matrix(S_list: Sequence[torch.Tensor], n_prefix: int, width: int = MEDIAN_FILTER_WIDTH) -> torch.Tensor:
    """Steps 4-7.  `S_list`: per alignment head, in ascending (layer, head) order, the fp32 scores [N_all, F] of the forced
    sequence over the F valid frames.  Returns Mtx[n_prefix : N_all - 1], fp32 [N, F]."""
    total = None
    for S in S_list:
        W = S.float().softmax(dim=-1)
        mean = W.mean(dim=-2, keepdim=True)
        std = ((W - mean) ** 2).mean(dim=-2, keepdim=True).sqrt()                 # population std over the token rows
        Z = torch.where(std > 0, (W - mean) / std, torch.zeros_like(W))          # upstream: NaN where std == 0
        Z = median_filter(Z, width)
        total = Z if total is None else total + Z
    mtx = total / float(len(S_list))
    return mtx[n_prefix: mtx.shape[0] - 1]


def dtw_cpu(x: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Step 8 on an fp32 cost matrix x [N, M]: (text_indices, time_indices) of the cheapest monotone path from (0, 0) to
    (N - 1, M - 1).  cost[0, 0] = 0, borders +inf, cost[i, j] = fp32(x[i-1, j-1] + c) with the predecessor
        c0 = cost[i-1, j-1] if c0 < c1 and c0 < c2      (trace 0)
        c1 = cost[i-1, j]   elif c1 < c0 and c1 < c2    (trace 1)
        c2 = cost[i, j-1]   else                        (trace 2)
    Cells of one anti-diagonal do not depend on each other, so the table is filled a diagonal at a time (what the device does,
    too); every cell's arithmetic is the loop's."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    N, M = x.shape
    if N < 1 or M < 1:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    trace = np.full((N + 1, M + 1), -1, dtype=np.int8)
    cost[0, 0] = 0
    for d in range(2, N + M + 1):
        i = np.arange(max(1, d - M), min(N, d - 1) + 1)
        j = d - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        t0 = (c0 < c1) & (c0 < c2)
        t1 = ~t0 & (c1 < c0) & (c1 < c2)
        c = np.where(t0, c0, np.where(t1, c1, c2))
        cost[i, j] = x[i - 1, j - 1] + c
        trace[i, j] = np.where(t0, 0, np.where(t1, 1, 2))
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j = N, M
    text, time = [], []
    while i > 0 or j > 0:
        text.append(i - 1)
        time.append(j - 1)
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return np.array(text[::-1], dtype=np.int64), np.array(time[::-1], dtype=np.int64)


def merge_punctuations(alignment: List[WordTiming], prepended: str = PREPEND_PUNCTUATIONS,
                       appended: str = APPEND_PUNCTUATIONS) -> None:
    """Upstream's rule, in place: an opening mark (a word " (" and the like) joins the word after it, a closing mark the word
    before it; the absorbed entry is left with an empty word and no tokens.  Times are not touched, as upstream."""
    # opening marks, walking backwards: `target` is the nearest later entry that has not been absorbed
    target = len(alignment) - 1
    for k in range(len(alignment) - 2, -1, -1):
        mark, nxt = alignment[k], alignment[target]
        if mark.word.startswith(" ") and mark.word.strip() in prepended:
            nxt.word, nxt.tokens = mark.word + nxt.word, mark.tokens + nxt.tokens
            mark.word, mark.tokens = "", []
        else:
            target = k
    # closing marks, walking forwards: `target` is the nearest earlier entry that has not been absorbed
    target = 0
    for k in range(1, len(alignment)):
        prev, mark = alignment[target], alignment[k]
        if not prev.word.endswith(" ") and mark.word in appended:
            prev.word, prev.tokens = prev.word + mark.word, prev.tokens + mark.tokens
            mark.word, mark.tokens = "", []
        else:
            target = k


def words_from_path(text_indices, time_indices, words: Sequence[str], word_tokens: Sequence[Sequence[int]],
                    token_probs: Sequence[float], seconds_per_frame: float) -> List[WordTiming]:
    """Step 9.  `words` / `word_tokens`: the split of text + [eot] (Tokenizer.split_to_word_tokens); `token_probs`: the forced
    pass's probability of every text token.  The closing <|endoftext|> word only lends its start as the last word's end."""
    if len(word_tokens) <= 1:
        return []
    text_indices, time_indices = np.asarray(text_indices), np.asarray(time_indices)
    boundaries = np.concatenate([[0], np.cumsum([len(t) for t in word_tokens[:-1]])]).astype(np.int64)
    jumps = np.concatenate([[True], np.diff(text_indices) != 0])
    jump_times = time_indices[jumps] * float(seconds_per_frame)
    starts, ends = jump_times[boundaries[:-1]], jump_times[boundaries[1:]]
    probs = np.asarray(token_probs, dtype=np.float64)
    out = [WordTiming(word, list(toks), float(s), float(e), float(probs[a:b].mean()))
           for word, toks, s, e, a, b in zip(words, word_tokens, starts, ends, boundaries[:-1], boundaries[1:])]
    merge_punctuations(out)
    return [w for w in out if w.word]


def default_alignment_heads(n_text_layer: int, n_text_head: int) -> List[int]:
    """Upstream's default: every head of the upper half of the decoder layers, as layer * n_text_head + head, ascending (32 layers:
    16 .. 31; large-v3-turbo's 4: 2 and 3; one layer: layer 0).  Upstream ships measured per-model heads for its released checkpoints
    (large-v3 and turbo among them) as data this project does not have: `build.py --alignment_heads` is the way to supply them."""
    return [l * n_text_head + h for l in range(n_text_layer // 2, n_text_layer) for h in range(n_text_head)]


def parse_alignment_heads(spec, n_text_layer: int, n_text_head: int) -> List[int]:
    """"l:h,l:h,..." or a list of [l, h] pairs -> sorted flat indices; None -> the default."""
    if spec is None:
        return default_alignment_heads(n_text_layer, n_text_head)
    if isinstance(spec, str):
        pairs = [tuple(int(v) for v in item.split(":")) for item in spec.split(",") if item.strip()]
    else:
        pairs = [tuple(int(v) for v in item) for item in spec]
    flat = set()
    for pair in pairs:
        if len(pair) != 2 or not (0 <= pair[0] < n_text_layer and 0 <= pair[1] < n_text_head):
            raise ValueError(f"alignment head {pair} does not exist in a decoder of {n_text_layer} layers x {n_text_head} heads")
        flat.add(pair[0] * n_text_head + pair[1])
    if not flat:
        raise ValueError("the list of alignment heads is empty")
    return sorted(flat)
