"""WhisperDecoding: decoder + cross-K/V session wrapper and Whisper's greedy decoding rules.

Same classes, constructor, attributes and method names as the reference's
examples/whisper/decoding.py (W/decoding.py; W = /root/reference/tensorrt_llm_july-release-v1/
examples/whisper): `DecodingOptions`, `DecodingResult`, `MaximumLikelihoodRanker`,
`SuppressBlank`, `SuppressTokens`, `ApplyTimestampRules`, `GreedyDecoder`, and
`WhisperDecoding.{xa2cross_key_value, decode, detect_language, main_loop, post_process,
torch_detect_language, torch_main_loop}` (W/decoding.py:303-878).

What differs underneath:
* any batch size and model size (the reference hard-wires batch 1 / large-v2);
* `main_loop` runs the fast path: KV cache pre-allocated `[B,2,H,n_text_ctx,64]` and appended in
  place (the reference concatenates a fresh cache per layer per step), logit rules +
  arg-max + log-prob + token append fused in one device kernel (csrc/greedy.hip), no host
  synchronisation inside the loop except a completion poll every `poll_every` steps.
  `main_loop_reference` is the literal per-step loop through `decode()` and the host-side filter
  classes, kept for parity tests: both must return identical tokens;
* the cross-attention K/V computed by `detect_language` are re-used by `main_loop` for the same
  audio features (the reference runs that engine twice per utterance);
* `beam_size` / `patience` select beam search (upstream Whisper's BeamSearchDecoder; the reference carries the options
  but no such class): `BeamSearchDecoder` in the literal loops, wm_beam_step + wm_kv_reorder (csrc/beam.hip) after
  every decoder launch of `main_loop`;
* `repetition_penalty` / `no_repeat_ngram_size` (CTranslate2 / Hugging Face; repetition.py states the contract): `RepetitionPenalty` and
  `NoRepeatNGram` first in the filter list of the literal loops, wm_repeat_controls (csrc/repeat.hip) in front of the token step of
  `main_loop` -- only when one of them is on.
"""
from __future__ import annotations

import json
import os
import weakref
import zlib
from collections import OrderedDict
from dataclasses import dataclass, field
from functools import lru_cache
from pathlib import Path
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import ctypes as C
import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor

import native
import repetition
import timing
from build import get_engine_name
from session import Session, TensorInfo, str_dtype_to_trt, trt_dtype_to_torch, logger
from tokenizer import LANGUAGES, TO_LANGUAGE_CODE, Tokenizer

CHUNK_LENGTH = 30


@dataclass(frozen=True)
class DecodingOptions:
    task: str = "transcribe"            # "transcribe" (X->X) or "translate" (X->English)
    language: Optional[str] = None      # detected when None
    temperature: float = 0.0
    sample_len: Optional[int] = None    # maximum number of tokens to sample
    best_of: Optional[int] = None
    beam_size: Optional[int] = None
    patience: Optional[float] = None
    length_penalty: Optional[float] = None
    prompt: Optional[Union[str, List[int]]] = None
    prefix: Optional[Union[str, List[int]]] = None
    suppress_tokens: Optional[Union[str, Iterable[int]]] = "-1"
    suppress_blank: bool = True
    without_timestamps: bool = False
    max_initial_timestamp: Optional[float] = 1.0
    fp16: bool = True
    # the in-loop controls against repeated phrases (repetition.py states the contract): they count the tokens a row has SAMPLED --
    # never the start sequence or a prompt -- and change text tokens only
    repetition_penalty: float = 1.0     # > 0; logits of sampled text tokens are divided (positive) / multiplied (else) by it; 1.0 = off
    no_repeat_ngram_size: int = 0       # >= 0; no n-gram of sampled tokens may end in the same text token twice; 0 = off


@dataclass(frozen=True)
class DecodingResult:
    audio_features: Tensor
    language: str
    language_probs: Optional[Dict[str, float]] = None
    tokens: List[int] = field(default_factory=list)
    text: str = ""
    avg_logprob: float = np.nan
    no_speech_prob: float = np.nan
    temperature: float = np.nan
    compression_ratio: float = np.nan


class MaximumLikelihoodRanker:
    """Pick the sample with the highest length-normalised log-probability (W/decoding.py:92-115)."""

    def __init__(self, length_penalty: Optional[float]):
        self.length_penalty = length_penalty

    def rank(self, tokens: List[List[Tensor]], sum_logprobs: List[List[float]]):
        picks = []
        for group, lps in zip(tokens, sum_logprobs):
            scores = []
            for t, lp in zip(group, lps):
                n = len(t)
                # (n = 0: a row closed before its first token, row_limit = 0 -- the empty rows of a long-form round; its sum is 0)
                penalty = max(n, 1) if self.length_penalty is None else ((5 + n) / 6) ** self.length_penalty
                scores.append(lp / penalty)
            picks.append(int(np.argmax(scores)))
        return picks


# ---- host-side logit filters (the reference-faithful loop; vectorised over the batch) -----------

class LogitFilter:
    def apply(self, logits: Tensor, tokens: Tensor) -> None:
        raise NotImplementedError


class SuppressBlank(LogitFilter):
    def __init__(self, tokenizer: Tokenizer, sample_begin: int):
        self.tokenizer, self.sample_begin = tokenizer, sample_begin

    def apply(self, logits: Tensor, tokens: Tensor):
        if tokens.shape[1] == self.sample_begin:
            logits[:, list(self.tokenizer.blank_tokens()) + [self.tokenizer.eot]] = -np.inf


class SuppressTokens(LogitFilter):
    def __init__(self, suppress_tokens: Sequence[int]):
        self.suppress_tokens = list(suppress_tokens)

    def apply(self, logits: Tensor, tokens: Tensor):
        logits[:, self.suppress_tokens] = -np.inf


class ApplyTimestampRules(LogitFilter):
    """Timestamp pairing / monotonicity / initial-timestamp rules (W/decoding.py:134-199)."""

    def __init__(self, tokenizer: Tokenizer, sample_begin: int, max_initial_timestamp_index: Optional[int]):
        self.tokenizer, self.sample_begin = tokenizer, sample_begin
        self.max_initial_timestamp_index = max_initial_timestamp_index

    def apply(self, logits: Tensor, tokens: Tensor):
        tk = self.tokenizer
        tb, eot = tk.timestamp_begin, tk.eot
        V = logits.shape[1]
        if tk.no_timestamps is not None:
            logits[:, tk.no_timestamps] = -np.inf
        sampled = tokens[:, self.sample_begin:]
        n = sampled.shape[1]
        is_ts = sampled >= tb
        col = torch.arange(V, device=logits.device)[None, :]
        last_ts = is_ts[:, -1] if n >= 1 else torch.zeros(tokens.shape[0], dtype=torch.bool, device=tokens.device)
        pen_ts = is_ts[:, -2] if n >= 2 else torch.ones(tokens.shape[0], dtype=torch.bool, device=tokens.device)
        # timestamps come in pairs (except right before EOT)
        kill = (last_ts & pen_ts)[:, None] & (col >= tb)
        kill |= (last_ts & ~pen_ts)[:, None] & (col < eot)
        if n >= 1:
            # no decreasing timestamps; a closed segment must have non-zero length
            has_ts = is_ts.any(dim=1)
            idx = torch.arange(n, device=tokens.device)[None, :].expand_as(is_ts)
            last_pos = torch.where(is_ts, idx, torch.full_like(idx, -1)).max(dim=1).values.clamp(min=0)
            last_val = sampled.gather(1, last_pos[:, None])[:, 0]
            bound = torch.where(last_ts & ~pen_ts, last_val, last_val + 1)
            kill |= has_ts[:, None] & (col >= tb) & (col < bound[:, None])
        logits.masked_fill_(kill.to(logits.device), -np.inf)
        if tokens.shape[1] == self.sample_begin:
            logits[:, :tb] = -np.inf
            if self.max_initial_timestamp_index is not None:
                logits[:, tb + self.max_initial_timestamp_index + 1:] = -np.inf
        # if the timestamps together outweigh every text token, sample a timestamp
        logprobs = F.log_softmax(logits.float(), dim=-1)
        ts_lp = logprobs[:, tb:].logsumexp(dim=-1)
        text_lp = logprobs[:, :tb].max(dim=-1).values
        logits[:, :tb] = torch.where((ts_lp > text_lp)[:, None], torch.full_like(logits[:, :tb], -np.inf),
                                     logits[:, :tb])


class RepetitionPenalty(LogitFilter):
    """The repetition penalty of repetition.py in torch: every distinct text token (id < eot) a row has sampled has its logit
    divided by the penalty when positive, multiplied otherwise -- once, in fp32, rounded to fp16.  The arithmetic runs on the host
    whatever device the logits live on: the contract is the correctly rounded IEEE quotient, and a device's elementwise division
    need not be (a scalar divisor becomes a multiplication by its reciprocal)."""

    def __init__(self, penalty: float, eot: int, sample_begin: int):
        self.penalty, self.eot, self.sample_begin = float(penalty), eot, sample_begin

    def apply(self, logits: Tensor, tokens: Tensor):
        sampled = tokens[:, self.sample_begin:].to(logits.device).long()
        text = (sampled >= 0) & (sampled < self.eot)
        if self.penalty == 1.0 or not bool(text.any()):
            return
        rows, cols = text.nonzero(as_tuple=True)
        ids = sampled[rows, cols]
        x = logits[rows, ids].float().cpu()                      # every occurrence reads the logit BEFORE anything is written ...
        p = torch.tensor(self.penalty, dtype=torch.float32)
        y = torch.where(x > 0, x / p, x * p).to(logits.dtype)
        logits[rows, ids] = y.to(logits.device)                  # ... so the occurrences of a token store equal values: penalised once


class NoRepeatNGram(LogitFilter):
    """The no-repeat n-gram rule of repetition.py in torch: with H the tokens a row has sampled and m of them, every text token
    H[i + n - 1] whose (n - 1)-gram H[i : i + n - 1] equals the last n - 1 tokens is set to -inf.  Matching runs over H as it is
    (timestamps included); only text tokens (id < eot) are banned."""

    def __init__(self, n: int, eot: int, sample_begin: int):
        self.n, self.eot, self.sample_begin = int(n), eot, sample_begin

    def apply(self, logits: Tensor, tokens: Tensor):
        n = self.n
        sampled = tokens[:, self.sample_begin:].to(logits.device).long()
        m = sampled.shape[1]
        if n <= 0 or m < n:                                       # (m == n - 1: the suffix is all of H, no earlier n-gram)
            return
        nxt = sampled[:, n - 1:]                                  # H[i + n - 1], i = 0 .. m - n
        match = torch.ones_like(nxt, dtype=torch.bool)
        for k in range(n - 1):                                    # H[i + k] == H[m - n + 1 + k]
            match &= sampled[:, k: k + m - n + 1] == sampled[:, m - n + 1 + k, None]
        rows, cols = (match & (nxt >= 0) & (nxt < self.eot)).nonzero(as_tuple=True)
        logits[rows, nxt[rows, cols]] = -np.inf


class GreedyDecoder:
    def __init__(self, temperature: float, eot: int):
        self.temperature, self.eot = temperature, eot

    def update(self, tokens: Tensor, logits: Tensor, sum_logprobs: Tensor) -> Tuple[Tensor, bool]:
        if self.temperature == 0:
            next_tokens = logits.argmax(dim=-1)
        else:
            next_tokens = torch.distributions.Categorical(logits=logits / self.temperature).sample()
        logprobs = F.log_softmax(logits.float(), dim=-1)
        current = logprobs[torch.arange(logprobs.shape[0]), next_tokens]
        alive = tokens[:, -1] != self.eot
        sum_logprobs += current * alive
        next_tokens[~alive] = self.eot
        tokens = torch.cat([tokens, next_tokens[:, None]], dim=-1)
        return tokens, bool((tokens[:, -1] == self.eot).all())

    def finalize(self, tokens: Tensor, sum_logprobs: Tensor):
        # make sure each sequence has at least one EOT token at the end
        return F.pad(tokens, (0, 1), value=self.eot), sum_logprobs.tolist()


BEAM_MAX, BEAM_POOL_MAX = 8, 16          # bounds of csrc/beam.hip


def check_decoding_options(options: DecodingOptions) -> None:
    """The combinations of sampling options the decoders take (upstream Whisper refuses the same ones)."""
    if options.beam_size is not None:
        if options.best_of is not None:
            raise ValueError("beam_size and best_of can't be given together")
        if options.temperature != 0:
            raise ValueError("beam_size needs temperature = 0 (beam search does not sample)")
        if not 1 <= options.beam_size <= BEAM_MAX:
            raise ValueError(f"beam_size {options.beam_size} outside 1..{BEAM_MAX}")
        n = round(options.beam_size * (options.patience or 1.0))
        if not 1 <= n <= BEAM_POOL_MAX:
            raise ValueError(f"beam_size * patience = {n} finished candidates per utterance, outside 1..{BEAM_POOL_MAX}")
    elif options.patience is not None:
        raise ValueError("patience requires beam_size to be given")
    repetition.check_controls(options.repetition_penalty, options.no_repeat_ngram_size)


def candidate_mode(options: DecodingOptions, fallback_best_of: Optional[int], temperature: float) -> Tuple[str, int]:
    """How one main_loop call at `temperature` decodes, and how many candidates per utterance it ranks: ("beam", beam_size) or
    ("sample", n).  Upstream's decode_with_fallback drops beam_size / patience above temperature 0 and best_of at 0; an instance
    built with `fallback_best_of = M` follows it: beam search at 0, M independent samples above.  Without it the instance's own
    options hold at every temperature (beam search, or best_of / one sample)."""
    if options.beam_size is not None:
        if fallback_best_of is not None and temperature > 0:
            return "sample", int(fallback_best_of)
        return "beam", int(options.beam_size)
    return "sample", int(options.best_of or 1)


def check_candidate_options(options: DecodingOptions, shared_cross_kv: bool, fallback_best_of: Optional[int]) -> None:
    """The combinations `shared_cross_kv` / `fallback_best_of` take (WhisperDecoding)."""
    if fallback_best_of is None:
        return
    if options.best_of is not None:
        raise ValueError("fallback_best_of and best_of can't be given together (best_of alone samples at every temperature)")
    if options.beam_size is None:
        raise ValueError("fallback_best_of needs beam_size: it is the number of samples a beam-search instance draws above temperature 0")
    if not shared_cross_kv:
        raise ValueError("fallback_best_of needs shared_cross_kv=True (the candidates of both modes share one copy of the cross K/V)")
    if not 1 <= int(fallback_best_of) <= options.beam_size:
        raise ValueError(f"fallback_best_of {fallback_best_of} outside 1..beam_size = {options.beam_size} (the rows are n_audio x beam_size in both modes)")


class BeamSearchDecoder:
    """Beam search with the semantics of upstream Whisper's BeamSearchDecoder, in torch on the host: the literal statement of
    the contract that the device step (csrc/beam.hip, wm_beam_io in include/whisper_mi355.h) implements.

    Rows are n_audio x beam_size, beam j of utterance a is row a * beam_size + j.  Per `update`, per utterance:
    every live beam proposes its beam_size + 1 best tokens (at the first sampled step only beam 0: the beams are identical);
    candidates are walked in the TOTAL order score descending, parent beam ascending, token ascending (within a beam: equal
    log-probabilities, lower token first; tokens at -inf are never proposed) -- fp16 logits tie exactly often enough that the
    order must be a rule; EOT candidates go to the step's finished list, others become the next live beams until beam_size
    are saved; the finished ones join the utterance's pool while it holds fewer than max_candidates = round(beam_size *
    patience).

    One deliberate difference from upstream: an utterance whose pool is full is FROZEN -- its live beams, sums and pool no
    longer change.  Upstream keeps stepping it until the whole batch is complete, which (with patience < 1) makes an
    utterance's candidates depend on its neighbours in the batch; here a row's result never depends on the other rows."""

    def __init__(self, beam_size: int, eot: int, sample_begin: int, patience: Optional[float] = None):
        self.beam_size, self.eot, self.sample_begin = beam_size, eot, sample_begin
        self.patience = patience or 1.0
        self.max_candidates: int = round(beam_size * self.patience)
        assert self.max_candidates > 0, f"Invalid beam size ({beam_size}) or patience ({patience})"
        self.reset()

    def reset(self, n_audio: int = 0):
        self.pool: List[List[Tuple[List[int], float]]] = [[] for _ in range(n_audio)]     # per utterance: (tokens with EOT, score)
        self.live_len: List[Optional[int]] = [None] * n_audio                             # length of a frozen utterance's live beams
        self.source_indices = None

    @property
    def completed(self) -> List[bool]:
        return [n is not None for n in self.live_len]

    def propose(self, logprobs: np.ndarray) -> List[int]:
        """The beam_size + 1 best tokens of one row: log-probability descending, token ascending among equals."""
        k = min(self.beam_size + 1, logprobs.shape[0])
        kth = np.partition(logprobs, -k)[-k]                       # everything >= the k-th largest value, ties included
        idx = np.nonzero((logprobs >= kth) & (logprobs > -np.inf))[0]
        idx = idx[np.lexsort((idx, -logprobs[idx]))]               # (last key first: value, then token id)
        return [int(t) for t in idx[:k]]

    def update(self, tokens: Tensor, logits: Tensor, sum_logprobs: Tensor) -> Tuple[Tensor, bool, Tensor]:
        """One token step.  Returns (tokens with the new column, every utterance complete, source row of every row) and
        overwrites `sum_logprobs`; the caller gathers its self-attention cache by the source rows."""
        K, eot = self.beam_size, self.eot
        n_rows, cur = tokens.shape
        assert n_rows % K == 0, f"{n_rows} rows are not a multiple of beam_size {K}"
        n_audio = n_rows // K
        if len(self.pool) != n_audio:
            self.reset(n_audio)
        logprobs = F.log_softmax(logits.float(), dim=-1).cpu().numpy()
        sums = sum_logprobs.detach().cpu().numpy().astype(np.float32)
        old = tokens.cpu().tolist()
        rows, new_sums, source = [], [], []
        for a in range(n_audio):
            r0 = a * K
            if self.live_len[a] is not None:                      # frozen: rows keep their content (the new column is padding)
                rows += [old[r0 + j] + [eot] for j in range(K)]
                new_sums += [float(sums[r0 + j]) for j in range(K)]
                source += [r0 + j for j in range(K)]
                continue
            cands = []                                            # (score, beam, token)
            for j in range(1 if cur == self.sample_begin else K):
                for t in self.propose(logprobs[r0 + j]):
                    cands.append((np.float32(sums[r0 + j] + logprobs[r0 + j, t]), j, t))
            cands.sort(key=lambda c: (-c[0], c[1], c[2]))
            live, finished = [], []
            for score, j, t in cands:
                if t == eot:
                    finished.append((old[r0 + j] + [eot], float(score)))
                else:
                    live.append((score, j, t))
                    if len(live) == K:
                        break
            while len(live) < K:                                  # fewer finite proposals than beams (never under Whisper's rules)
                live.append((np.float32(-np.inf), len(live), eot))
            for score, j, t in live:
                rows.append(old[r0 + j] + [t])
                new_sums.append(float(score))
                source.append(r0 + j)
            for seq in finished:
                if len(self.pool[a]) >= self.max_candidates:
                    break
                self.pool[a].append(seq)
            if len(self.pool[a]) >= self.max_candidates:
                self.live_len[a] = cur + 1
        sum_logprobs[:] = torch.tensor(new_sums, dtype=sum_logprobs.dtype, device=sum_logprobs.device)
        self.source_indices = torch.tensor(source, dtype=torch.long, device=tokens.device)
        tokens = torch.tensor(rows, dtype=tokens.dtype, device=tokens.device)
        return tokens, all(self.completed), self.source_indices

    def finalize(self, tokens: Tensor, sum_logprobs: Tensor):
        """Per utterance: the pool, topped up with the live beams (best sum first, each closed with EOT) while it holds
        fewer than beam_size sequences.  Lists per utterance, of differing lengths."""
        K = self.beam_size
        tokens = tokens.reshape(-1, K, tokens.shape[-1]).cpu()
        sums = sum_logprobs.reshape(-1, K).cpu().tolist()
        if len(self.pool) != tokens.shape[0]:
            self.reset(tokens.shape[0])
        out_tokens, out_sums = [], []
        for a in range(tokens.shape[0]):
            seqs = list(self.pool[a])
            n_live = tokens.shape[-1] if self.live_len[a] is None else self.live_len[a]
            for j in sorted(range(K), key=lambda j: (-sums[a][j], j)):
                if len(seqs) >= K:
                    break
                seqs.append((tokens[a, j, :n_live].tolist() + [self.eot], sums[a][j]))
            out_tokens.append([torch.tensor(s, dtype=torch.long) for s, _ in seqs])
            out_sums.append([lp for _, lp in seqs])
        return out_tokens, out_sums


ROW_PAD_TOKEN = 0        # what the pad slots of a right-aligned row hold: any token but EOT (post_process cuts a row at its first EOT)


def row_prompt_layout(n_text_ctx: int, sot_sequence: Sequence[int], sot: int) -> Tuple[int, int, int]:
    """(L0, sot_index, prompt_capacity) of an instance with per-row prompts: every row of a call is L0 = n_text_ctx // 2 +
    len(sot_sequence) tokens long whatever its prompt -- the room <|startofprev|> and upstream's longest prompt
    (n_text_ctx // 2 - 1 tokens) need -- so `sample_begin` = L0 and `sot_index` are one value per instance."""
    half = n_text_ctx // 2
    return half + len(sot_sequence), half + list(sot_sequence).index(sot), half - 1


def right_aligned_rows(prompts: Sequence[Sequence[int]], sot_sequence: Sequence[int], sot_prev: int, n_text_ctx: int,
                       pad: int = ROW_PAD_TOKEN) -> Tuple[List[List[int]], List[int]]:
    """The start rows of a call with a prompt per utterance, and where each row begins:

        [pad x start[b]] [<|startofprev|> prompt_b[-(n_text_ctx // 2 - 1):]] [sot_sequence]

    every row L0 tokens long (row_prompt_layout).  An empty prompt has no <|startofprev|>, as upstream (W/decoding.py:508-511):
    its row begins at the sot_sequence.  The decoder treats slot start[b] of row b as position 0 (wm_decoder_io::row_start)."""
    sot_sequence = [int(t) for t in sot_sequence]
    L0, _, capacity = row_prompt_layout(n_text_ctx, sot_sequence, sot_sequence[0])
    rows, starts = [], []
    for prompt in prompts:
        prompt = [int(t) for t in prompt]
        body = ([int(sot_prev)] + prompt[-capacity:] if prompt else []) + sot_sequence
        starts.append(L0 - len(body))
        rows.append([int(pad)] * (L0 - len(body)) + body)
    return rows, starts


# ---- the device loop's schedule: streams, the "alone" decision, graph keys (pure: tests/test_decode_plan_cpu.py) ---------------

def fork(main, streams) -> None:
    """Every stream of `streams` waits for what `main` holds so far."""
    for s in streams:
        s.wait_stream(main)


def join(main, streams) -> None:
    """`main` waits for what every stream of `streams` holds so far."""
    for s in streams:
        main.wait_stream(s)


def steps_side_by_side(n_micro: int, sequential: bool, force_not_alone: bool) -> bool:
    """The `not_alone` of every launch of a pass: stream-parallel groups have the steps of two groups in flight at once, so none of
    them may take a one-launch form (two 256-workgroup launches side by side can each hold half of the chip and wait for the other
    half: ADVICE r5, whisper_mi355.h `not_alone`).  `force_not_alone`: bench.py's probes step the groups one after the other but
    must run the kernels of the parallel schedule."""
    return (n_micro > 1 and not sequential) or force_not_alone


def groups_run_alone(bounds: Sequence[Tuple[int, int]], n_micro: int, sequential: bool, force_not_alone: bool) -> bool:
    """May a group of this pass take the one-launch step (csrc/gemv_chain.hip)?  Groups of up to eight rows stepped one at a time."""
    return (n_micro == 1 or sequential) and not force_not_alone and any(hi - lo <= 8 for lo, hi in bounds)


def call_key(beam: bool, ignore_eot: bool, cross_group: int, temperature: float, own_temperature: float) -> tuple:
    """What of a main_loop call its captured graphs bake in, as the tail of their keys."""
    key = ('beam', bool(ignore_eot)) if beam else ()         # (ignore_eot is an argument of the captured beam step)
    if cross_group > 1:
        key += (('cross_group', cross_group),)
    if temperature != own_temperature:
        key += (('temperature', temperature),)               # (so is the temperature: a per-call one has graphs of its own)
    return key


def step_key(n_micro: int, slot: int, use_live: bool, bkey: tuple = ()) -> tuple:
    return (n_micro, slot, use_live) + bkey


def prefill_key(n_micro: int, slot: int, use_live: bool, L0: int, not_alone: bool, bkey: tuple = ()) -> tuple:
    return (n_micro, slot, use_live, 'prefill', L0, not_alone) + bkey


def language_key(n_micro: int, slot: int, not_alone: bool) -> tuple:
    return (n_micro, slot, 'lang', not_alone)


def partition_key(n_micro: int) -> tuple:
    return ('partition', n_micro)


@dataclass
class _Call:
    """What the groups of one device-loop call share."""
    st: dict
    cross: list
    L0: int
    n_micro: int
    use_live: bool
    not_alone: bool
    beam: bool              # this call's decoder (fallback_best_of: samples above temperature 0)
    ignore_eot: bool
    temperature: float
    bkey: tuple
    use_graph: bool
    block: bool             # one pass over the whole start block (wm_decoder_prefill), logits from sot_index on
    graph_prefill: bool     # (longer start sequences run as 4-token passes with copies between them: eager -- unless `block`)


class _Group:
    """One utterance group of a device-loop call: rows [lo, hi) of the batch state on a stream of their own, and the group's step in
    its three forms -- `prefill`, `step`, `step_counted` -- each "decoder launch, token step, step finish"."""

    def __init__(self, dec: "WhisperDecoding", call: _Call, slot: int, lo: int, hi: int, stream):
        st, G, n_micro = call.st, dec._cross_group(), call.n_micro
        self.dec, self.call, self.slot, self.lo, self.hi = dec, call, slot, lo, hi
        self.stream, self.sm, self.active = stream, stream.cuda_stream, True
        self.kv = [t[lo:hi] for t in st['kv']]
        self.cross = [t[lo // G:hi // G] for t in call.cross]
        self.live_groups = dec._live_groups(st, n_micro, slot, lo, hi) if call.use_live and G > 1 else None
        self.logits, self.tokens, self.done = st['logits'][lo:hi], st['tokens'][lo:hi], st['done'][lo:hi]
        self.live = dec._live_list(st, n_micro, slot, lo, hi) if call.use_live else None
        self.row_start = st['row_start'][lo:hi] if dec.row_prompts else None
        if dec.beam:       # the group's cache rows per layer as a device-resident pointer table (wm_kv_reorder; stable like the buffers)
            if (n_micro, slot) not in st['kv_tables']:
                st['kv_tables'][(n_micro, slot)] = torch.tensor([t.data_ptr() for t in self.kv], dtype=torch.int64, device=self.done.device)
            self.kv_table = st['kv_tables'][(n_micro, slot)]
        self.step_key = step_key(n_micro, slot, call.use_live, call.bkey)
        self.fresh_key = self.step_key + ('fresh',)
        self.prefill_key = prefill_key(n_micro, slot, call.use_live, call.L0, call.not_alone, call.bkey)

    def prefill(self, L0: int) -> None:
        """The L0 start tokens on the empty cache, and the first token step."""
        dec, st, G = self.dec, self.call.st, self.dec._cross_group()
        if G > 1:
            # shared cross K/V: the candidates of an utterance begin with the same tokens over the same audio, so ONE row per
            # utterance is prefilled (group 1, on the utterances' cross K/V and the group's first cache rows: what each candidate's
            # row would compute) and its cache slots and logits are copied to the G candidates
            a_lo, a_hi = self.lo // G, self.hi // G
            logits_u = st['logits_u'][a_lo:a_hi]
            with torch.cuda.stream(self.stream):
                self._launch_prefill(L0, st['tokens'][self.lo:self.hi:G, :L0], [t[:a_hi - a_lo] for t in self.kv], logits_u, None,
                                     st['row_start_u'][a_lo:a_hi] if dec.row_prompts else None)
                self._spread_to_candidates(L0, logits_u)
        else:
            self._launch_prefill(L0, self.tokens[:, :L0], self.kv, self.logits, self.live, self.row_start)
        V = self.logits.shape[-1]
        self._token_step(self.logits.data_ptr() + (L0 - 1) * V * 2, L0 * V, L0)
        self._finish(None)

    def _launch_prefill(self, L0, tokens, kv, logits, live, row_start) -> None:
        dec, cap = self.dec, self.dec.decoder_config['num_text_ctx']
        sess, pos = dec.decoder_session, dec.positional_embedding[0:L0]
        if self.call.block:
            sess.decoder_prefill(tokens, pos, self.cross, kv, cap, logits, self.sm, dec.sot_index, slot=self.slot, live_rows=live,
                                 row_start=row_start)
        else:
            sess.decoder_step(tokens, pos, self.cross, None, cap, kv, cap, logits, 0, self.sm, slot=self.slot, live_rows=live,
                              not_alone=self.call.not_alone, row_start=row_start)

    def _spread_to_candidates(self, L0, logits_u) -> None:
        """Shared cross K/V: the first L0 cache slots and the logits of every utterance's prefilled row, to its G candidates."""
        n_u, G = logits_u.shape[0], self.dec._cross_group()
        for t in self.kv:
            first = t[:n_u, :, :, :L0].clone()
            t.view(n_u, G, *t.shape[1:])[:, :, :, :, :L0] = first[:, None]
        self.logits.view(n_u, G, L0, self.logits.shape[-1])[:] = logits_u[:, None]

    def step(self, cur: int) -> None:
        """One token step issued eagerly: token cur - 1 at the host's n_past = cur - 1."""
        self._launch_step(self.tokens[:, cur - 1:cur], self.dec.positional_embedding[cur - 1:cur], cur - 1)
        self._token_step(self.logits.data_ptr(), self.logits.shape[-1], cur)
        self._finish(None)

    def step_counted(self, counter: Tensor) -> None:
        """The token step in the form that is captured: the whole token buffer, n_past read from the device counter, which the
        step's finish advances -- the call is the same for every token."""
        self._launch_step(self.tokens, self.dec.positional_embedding, 1, n_past_dev=counter, n_new=1)
        self._token_step(self.logits.data_ptr(), self.logits.shape[-1], 0, n_past_dev=counter)
        self._finish(counter)

    def _launch_step(self, tokens, pos, n_past, **counted) -> None:
        cap = self.dec.decoder_config['num_text_ctx']
        self.dec.decoder_session.decoder_step(tokens, pos, self.cross, self.kv, cap, self.kv, cap, self.logits, n_past, self.sm,
                                              slot=self.slot, live_rows=self.live, not_alone=self.call.not_alone,
                                              row_start=self.row_start, cross_group=self.dec._cross_group(),
                                              live_groups=self.live_groups, **counted)

    def _token_step(self, logits_ptr, row_stride, cur_len, n_past_dev=None) -> None:
        """What follows a group's decoder launch: the repetition controls where one is on, then the fused greedy step, or the beam
        step and the cache reorder."""
        dec, call = self.dec, self.call
        if dec.repeat_controls_on:
            dec._repeat_controls(call.st, self.lo, self.hi, logits_ptr, row_stride, cur_len, self.sm, n_past_dev=n_past_dev)
        if call.beam:
            dec._beam(call.st, self.lo, self.hi, logits_ptr, row_stride, cur_len, self.sm, self.kv_table, call.ignore_eot, n_past_dev=n_past_dev)
        else:
            dec._greedy(call.st, self.lo, self.hi, logits_ptr, row_stride, cur_len, self.sm, n_past_dev=n_past_dev, temperature=call.temperature)

    def _finish(self, counter: Optional[Tensor]) -> None:
        """End of a group's step: advance its device step counter (graph replay) and, with per-row completion, rebuild its list of
        live rows from the flags the token step has just updated."""
        lib, n = native.load_library(), self.hi - self.lo
        counter_ptr = counter.data_ptr() if counter is not None else None
        if self.live is not None and self.live_groups is not None:
            native.check(lib.wm_step_finish_group(counter_ptr, self.done.data_ptr(), n, self.dec._cross_group(), self.live.data_ptr(),
                                                  self.live_groups.data_ptr(), self.sm), "wm_step_finish_group")
        elif self.live is not None:
            native.check(lib.wm_step_finish(counter_ptr, self.done.data_ptr(), n, self.live.data_ptr(), self.sm), "wm_step_finish")
        elif counter is not None:
            native.check(lib.wm_step_advance(counter_ptr, self.sm), "wm_step_advance")


class WhisperDecoding:
    def __init__(self, engine_dir, only_torch: bool = False, vocab_path: Optional[str] = None,
                 options: Optional[DecodingOptions] = None, row_prompts: bool = False, shared_cross_kv: bool = False,
                 fallback_best_of: Optional[int] = None, block_prefill: bool = False):
        """`shared_cross_kv` (opt-in): the n_group candidates of an utterance (beams, best_of samples) read ONE copy of its
        cross-attention K/V (wm_decoder_group_io::cross_group) instead of a copy each: the cross K/V are projected once from the
        un-repeated features, held once per utterance and streamed once per utterance and token step.  Device loop only; not
        with `cu_partition`.  `fallback_best_of = M` (with beam_size = K >= M and shared_cross_kv): main_loop(temperature = t)
        runs beam search at t == 0 and M independent samples per utterance at t > 0 (`candidate_mode`), on the same n_audio x K
        rows, buffers and cross K/V -- upstream's decode_with_fallback.
        `row_prompts`: every utterance of a main_loop call may carry a prompt of its own (`set_prompts`: the previous text of
        long-form transcription, names and spellings).  The rows are right-aligned (`right_aligned_rows`): all of them are
        L0 = n_text_ctx // 2 + len(sot_sequence) tokens long and `sample_begin`, `sot_index`, the buffers and the captured graphs
        are fixed at construction; only where a row begins differs.  The price is the room for sampling: the effective
        sample_len is min(sample_len, n_text_ctx - L0) -- a row with a full prompt is cut exactly where upstream cuts it, a row
        with a short or no prompt loses at most len(sot_sequence) tokens against upstream's n_text_ctx // 2 (and pays for a
        prefill of L0 tokens).  Device loop only (greedy, temperature, best_of, beam search); not with `options.prompt` /
        `options.prefix`, not with `cu_partition`; word_timestamps stays prompt-free, as upstream.
        `block_prefill` (opt-in): every start block longer than 4 tokens -- the L0 tokens of a `row_prompts` instance, an
        `options.prompt` / `options.prefix` block -- runs through wm_decoder_prefill, ONE pass over the block with logits from
        `sot_index` on, instead of ceil(L0 / 4) passes of wm_decoder_step that each stream the weights and the cross K/V again; the call
        is captured and replayed like the 3-token prefill.  Inside the block the attention is un-quantised whatever the cache type
        (what upstream computes; the 4-token passes see earlier prompt tokens through their int8 codes), so with an int8 KV cache the
        logits differ from the default's within the int8-KV bound.  Start blocks of up to 4 tokens, the language pass, the forced
        pass of word_timestamps and every decode step are unchanged.  Not with int8 cross K/V engines, not with `cu_partition`.
        It pays at every row count measured (scripts/bench_prompts.py, large-v2 int8, L0 = 227): time to the first
        token 117.6 -> 5.4 ms at one row, 202.9 -> 17.8 ms at 8, 613.3 -> 91.9 ms at 64 with full prompts, and as much without prompts;
        no row count was found where it is not lower.  A start block of up to 4 tokens never takes it."""
        engine_dir = Path(engine_dir)
        self.decoder_config = None
        self.cross_attn_config = None
        self.get_config(engine_dir)
        self.only_torch = only_torch
        if not only_torch:
            self.decoder_session, self.cross_attn_session = self.get_session(engine_dir)
        self.vocab_path = vocab_path
        multilingual = self.decoder_config.get('vocab_size', 51865) >= 51865
        self.tokenizer = self.get_tokenizer(multilingual, 'en', 'transcribe')
        self.is_multilingual = multilingual

        self.sot_sequence = self.tokenizer.sot_sequence
        self.initial_tokens = tuple(list(self.sot_sequence))
        self.initial_token_length = len(self.initial_tokens)
        self.tokens = torch.tensor([self.initial_tokens]).repeat(self.decoder_config['num_audio'], 1)
        self.sot_index = self.initial_tokens.index(self.tokenizer.sot)
        self.options = options or DecodingOptions()
        check_decoding_options(self.options)

        check_candidate_options(self.options, bool(shared_cross_kv), fallback_best_of)
        self.shared_cross_kv = bool(shared_cross_kv)
        self.fallback_best_of = None if fallback_best_of is None else int(fallback_best_of)

        self.n_group = self.options.beam_size or self.options.best_of or 1
        self.sample_len: int = self.options.sample_len or self.decoder_config['num_text_ctx'] // 2
        if self.options.prompt or self.options.prefix:
            # the reference carries _get_initial_tokens (W/decoding.py:485-513) but never calls it (its options are the
            # defaults); with caller-supplied options the start sequence is <|startofprev|> prompt <|sot|> .. prefix
            self.initial_tokens = self._get_initial_tokens()
            self.initial_token_length = len(self.initial_tokens)
            self.tokens = torch.tensor([self.initial_tokens]).repeat(self.decoder_config['num_audio'], 1)
            self.sot_index = self.initial_tokens.index(self.tokenizer.sot)
        self.row_prompts = bool(row_prompts)
        self._prompts = None              # set_prompts: one token list per utterance of the next main_loop calls
        if self.row_prompts:
            if self.options.prompt or self.options.prefix:
                raise ValueError("row_prompts: the prompt is per row (set_prompts); options.prompt / options.prefix are not supported with it")
            n_ctx = self.decoder_config['num_text_ctx']
            L0, self.sot_index, self.prompt_capacity = row_prompt_layout(n_ctx, self.sot_sequence, self.tokenizer.sot)
            self.initial_tokens = tuple(right_aligned_rows([()], self.sot_sequence, self.tokenizer.sot_prev, n_ctx)[0][0])
            self.initial_token_length = L0
            self.tokens = torch.tensor([self.initial_tokens]).repeat(self.decoder_config['num_audio'], 1)
            self.sample_len = min(self.sample_len, n_ctx - L0)
        self.sample_begin: int = len(self.initial_tokens)
        self.use_int8_kv_cache = self.decoder_config['use_int8_kv_cache']
        self.use_int8_cross_kv = bool(self.decoder_config.get('use_int8_cross_kv', False))     # opt-in, beyond the reference
        self.block_prefill = bool(block_prefill)
        if self.block_prefill and self.use_int8_cross_kv:
            raise ValueError("block_prefill: engines with int8 cross K/V are not supported (wm_decoder_prefill reads fp16 cross K/V)")

        pe = np.load(engine_dir / 'positional_embedding.npy')
        self.positional_embedding = torch.tensor(pe)
        if not only_torch:
            self.positional_embedding = self.positional_embedding.to('cuda').type(torch.float16).contiguous()

        # repetition penalty / no-repeat n-grams (repetition.py): per instance, first in the filter list of the literal loops and one
        # launch in front of the token step of the device loop (_Group._token_step) -- with the defaults neither exists
        self.repeat_controls_on = repetition.controls_on(self.options.repetition_penalty, self.options.no_repeat_ngram_size)
        self.logit_filters = []
        if self.options.repetition_penalty != 1.0:
            self.logit_filters.append(RepetitionPenalty(self.options.repetition_penalty, self.tokenizer.eot, self.sample_begin))
        if self.options.no_repeat_ngram_size != 0:
            self.logit_filters.append(NoRepeatNGram(self.options.no_repeat_ngram_size, self.tokenizer.eot, self.sample_begin))
        self.max_initial_timestamp_index = None
        if self.options.suppress_blank:
            self.logit_filters.append(SuppressBlank(self.tokenizer, self.sample_begin))
        if self.options.suppress_tokens:
            self.logit_filters.append(SuppressTokens(self._get_suppress_tokens()))
        if not self.options.without_timestamps:
            precision = CHUNK_LENGTH / self.decoder_config['num_audio_ctx']  # usually 0.02 seconds
            if self.options.max_initial_timestamp:
                self.max_initial_timestamp_index = round(self.options.max_initial_timestamp / precision)
            self.logit_filters.append(
                ApplyTimestampRules(self.tokenizer, self.sample_begin, self.max_initial_timestamp_index))
        self.sequence_ranker = MaximumLikelihoodRanker(self.options.length_penalty)
        if self.options.beam_size is not None:
            self.decoder = BeamSearchDecoder(self.options.beam_size, self.tokenizer.eot, self.sample_begin, self.options.patience)
        else:
            self.decoder = GreedyDecoder(self.options.temperature, self.tokenizer.eot)
        self.beam = self.options.beam_size is not None     # (beam_size = 1 is beam search too: one beam, a pool of finished candidates)

        self.kv_cache = {}
        self.hooks = []
        self._cross_cache = None          # (key, list of cross K/V) from the last xa2cross_key_value
        self._state = {}                  # per-batch-size device buffers of the fast path
        self.poll_every = 8
        self.micro_batches = None         # stream-parallel utterance groups: None = by batch size (_groups), or a fixed count
        self.lang_id_sequential = False   # bench.py: run the language pass group by group (0.2 % of a step) so that its
                                          # HIP-event kernel timings are not inflated by the other group's HBM share
        self.groups_sequential = False    # bench.py's roofline probe: main_loop steps the utterance groups one AFTER the other (each group's
                                          # step waits for the previous group's), so that a launch is timed with the chip to itself
        # experimental schedule (off by default): cross-attention on its own CU set
        # (wm_decoder_step_multi).  Steady state 12.9 ms/step vs 13.9 for the captured graphs at B = 256, but the
        # cross-queue event hand-offs cost 12 us each and only resolve quickly while the host is busy issuing.
        self.cu_partition = False
        self.light_cus = 96               # CUs reserved for the latency-bound kernels of all groups
        self.run_ahead = 3                # decode steps the host may be ahead of the GPU in the partitioned loop
        self._partition = None            # (light streams, heavy stream), created on first use
        self.use_graphs = True            # replay one captured decode step per token (hipGraph)
        self.device_sampling = True       # temperature > 0 / best_of > 1 through the fused device loop (False: the literal host loop)
        # Per-row completion (W/decoding.py:817-819 stops its single utterance at EOT): rows that have emitted EOT drop out
        # of the attention kernels (their cross K/V -- 245.76 MB per token at large-v2 -- and KV cache are no longer read)
        # and a group whose rows have all finished is no longer stepped.  Results are unchanged: a finished row is kept at
        # EOT whatever its logits.  Off for `ignore_eot` loops (benchmarks decode a fixed number of tokens).
        self.skip_finished_rows = True
        self.profile_eager_passes = False  # bench.py's roofline probe: keep the language pass eager (its launches carry the profiling events)
        self.graph_prefill = True         # replay the language pass and the prefill from captured graphs too (they are host-bound eagerly)
        self.force_not_alone = False      # bench.py's probes step the groups one after the other but must run the kernels of the parallel schedule
        self.first_token_event = None     # bench.py: an event recorded (current stream) when the first sampled token of a main_loop call exists
        self._streams = []
        self._no_dedicated_queues = False
        self._decode_in_flight = 0        # main_loop calls under way (word_timestamps reuses the loop's buffers)
        self.last_alignment = None        # word_timestamps: the device's paths of the last call (and the matrices, with keep_alignment_matrix)
        self.keep_alignment_matrix = False
        WhisperDecoding._instances.add(self)      # (weak: a give-up of a one-launch step drops the graphs of EVERY instance, _chain_gave_up)

    # ---- configuration / sessions -----------------------------------------------------------------
    def get_config(self, engine_dir):
        for attr, fname in (('decoder_config', 'decoder_config.json'), ('cross_attn_config', 'cross_attn_config.json')):
            with open(engine_dir / fname, 'r') as f:
                config = json.load(f)
            merged = OrderedDict()
            merged.update(config['plugin_config'])
            merged.update(config['builder_config'])
            setattr(self, attr, merged)

    def get_session(self, engine_dir):
        path = engine_dir / get_engine_name('whisper_decoder', self.decoder_config['precision'],
                                            self.decoder_config['tensor_parallel'], 0)
        with open(path, 'rb') as f:
            decoder_session = Session.from_serialized_engine(f.read())
        path = engine_dir / get_engine_name('whsiper_crossattn', self.cross_attn_config['precision'],
                                            self.cross_attn_config['tensor_parallel'], 0)
        with open(path, 'rb') as f:
            cross_attn_session = Session.from_serialized_engine(f.read())
        return decoder_session, cross_attn_session

    def _get_suppress_tokens(self) -> Tuple[int]:
        suppress_tokens = self.options.suppress_tokens
        if isinstance(suppress_tokens, str):
            suppress_tokens = [int(t) for t in suppress_tokens.split(",")]
        if -1 in suppress_tokens:
            suppress_tokens = [t for t in suppress_tokens if t >= 0]
            suppress_tokens.extend(self.tokenizer.non_speech_tokens)
        elif suppress_tokens is None or len(suppress_tokens) == 0:
            suppress_tokens = []
        else:
            assert isinstance(suppress_tokens, list), "suppress_tokens must be a list"
        tk = self.tokenizer
        suppress_tokens.extend([tk.transcribe, tk.translate, tk.sot, tk.sot_prev, tk.sot_lm])
        if tk.no_speech is not None:
            suppress_tokens.append(tk.no_speech)       # no-speech probability is collected separately
        return tuple(sorted(set(suppress_tokens)))

    def get_tokenizer(self, multilingual: bool, language: Optional[str] = None, task: Optional[str] = None) -> Tokenizer:
        path = self.vocab_path
        if not path:      # the vendored vocabulary (assets/ASSETS.md), like the reference's assets/ (W/decoding.py:423-431)
            bundled = Path(__file__).resolve().parent / 'assets' / ('multilingual.tiktoken' if multilingual else 'gpt2.tiktoken')
            path = str(bundled) if bundled.exists() else None
        if path:
            return Tokenizer.from_vocab(path, multilingual, language, task)
        return Tokenizer.ids_only(multilingual, language, task)

    def _get_initial_tokens(self) -> Tuple[int]:
        tokens = list(self.sot_sequence)
        if prefix := self.options.prefix:
            prefix_tokens = self.tokenizer.encode(" " + prefix.strip()) if isinstance(prefix, str) else prefix
            if self.sample_len is not None:
                max_prefix_len = self.decoder_config['num_text_ctx'] // 2 - self.sample_len
                prefix_tokens = prefix_tokens[-max_prefix_len:]
            tokens = tokens + prefix_tokens
        if prompt := self.options.prompt:
            prompt_tokens = self.tokenizer.encode(" " + prompt.strip()) if isinstance(prompt, str) else prompt
            tokens = [self.tokenizer.sot_prev] + prompt_tokens[-(self.decoder_config['num_text_ctx'] // 2 - 1):] + tokens
        return tuple(tokens)

    # ---- engine calls with the reference's by-name protocol ------------------------------------------
    @staticmethod
    def _features_key(xa):
        """Identity of an audio-features tensor's CONTENT, or None when it cannot be known: the generation number
        the encoder stamped on it (encoding.stamp_generation) plus pointer, shape and torch's version counter.
        Pointer and version alone are not enough -- the engine writes through raw pointers, so a second batch
        encoded into the same buffer looks unchanged to torch.  A tensor without a stamp (a slice, a clone, a
        tensor from elsewhere) is never assumed to be one seen before."""
        gen = getattr(xa, 'wm_generation', None)
        return None if gen is None else (gen, xa.data_ptr(), tuple(xa.shape), xa._version)

    def xa2cross_key_value(self, xa):
        key = self._features_key(xa)
        if key is not None and self._cross_cache is not None and self._cross_cache[0] == key:
            return self._cross_cache[1]
        inputs = OrderedDict()
        xa16 = xa.type(torch.float16).contiguous()
        inputs.update({'xa': xa16})
        output_info = self.cross_attn_session.infer_shapes([TensorInfo('xa', str_dtype_to_trt("float16"), xa16.shape)])
        logger.debug(f'output info {output_info}')
        outputs = {t.name: torch.empty(tuple(t.shape), dtype=trt_dtype_to_torch(t.dtype), device=xa.device)
                   for t in output_info}
        stream = torch.cuda.current_stream()
        ok = self.cross_attn_session.run(inputs=inputs, outputs=outputs, stream=stream.cuda_stream)
        assert ok, 'Engine execution failed'
        stream.synchronize()
        cross = [outputs['cross_present_key_value_' + str(i)] for i in range(self.cross_attn_config['num_layers'])]
        self._cross_cache = (key, cross, xa)      # keep xa alive so the pointer key stays valid
        return cross

    def decode(self, x, cross_past_key_value, past_key_value=None):
        """One decoder call with the reference's I/O protocol (W/decoding.py:543-659): returns
        (logits fp16 [B, L, n_vocab], list of present_key_value [B,2,H,T+L,64])."""
        dev = x.device
        n_layer = self.decoder_config['num_layers']
        kv_dtype = 'int8' if self.use_int8_kv_cache else 'float16'
        inputs = OrderedDict()
        infos = []

        def add(name, tensor, dtype, shape=None):
            inputs[name] = tensor
            infos.append(TensorInfo(name, str_dtype_to_trt(dtype), tuple(shape if shape is not None else tensor.shape)))

        x = x.type(torch.int32).contiguous()
        input_len = x.shape[-1]
        add('x', x, 'int32')
        lens = torch.tensor((input_len,), dtype=torch.int32, device=dev)
        add('input_lengths', lens, 'int32')
        add('max_input_length', lens, 'int32')
        if not self.decoder_config['gpt_attention_plugin']:
            n_ctx = self.decoder_config['num_text_ctx']
            mask = torch.full((n_ctx, n_ctx), -50000.0, dtype=torch.float32).triu_(1)[:input_len, :input_len].contiguous().to(dev)
            add('mask', mask, 'float32')          # causality is applied inside the kernel; kept for I/O parity
        else:
            add('masked_tokens', torch.zeros((1, input_len), dtype=torch.int32, device=dev), 'int32')
            add('cache_indirection', torch.zeros((x.shape[0], 1, input_len), dtype=torch.int32, device=dev), 'int32')
            add('past_key_value_length', torch.tensor([0, 1], dtype=torch.int32, device=dev), 'int32')
            add('sequence_length', lens, 'int32')
        offset = past_key_value[0].shape[3] if past_key_value else 0
        pos = self.positional_embedding[offset: offset + input_len].type(torch.float16).contiguous()
        add('positional_embedding', pos, 'float16')
        n_head = self.decoder_config['num_heads']
        for i in range(n_layer):
            if past_key_value is None:
                dummy = torch.ones((1,), dtype=trt_dtype_to_torch(kv_dtype), device=dev)
                add('past_key_value_' + str(i), dummy, kv_dtype, (x.shape[0], 2, n_head, 0, 64))
            else:
                add('past_key_value_' + str(i), past_key_value[i].contiguous(), kv_dtype)
        for i in range(n_layer):
            add('cross_past_key_value_' + str(i), cross_past_key_value[i].contiguous(),
                'int8' if self.use_int8_cross_kv else 'float16')

        output_info = self.decoder_session.infer_shapes(infos)
        assert output_info is not None, 'infer_shapes failed'
        logger.debug(f'output info {output_info}')
        outputs = {t.name: torch.empty(tuple(t.shape), dtype=trt_dtype_to_torch(t.dtype), device=dev) for t in output_info}
        stream = torch.cuda.current_stream()
        ok = self.decoder_session.run(inputs=inputs, outputs=outputs, stream=stream.cuda_stream)
        assert ok, 'Engine execution failed'
        stream.synchronize()
        # a first call of one token for up to eight utterances (the language pass) may have run as ONE launch (gemv_chain.hip): this path
        # has synchronised, so a look at the give-up word is free -- and nobody else would look (the caller decoded on from garbage)
        if x.is_cuda and input_len == 1 and x.shape[0] <= 8 and self._chain_gave_up("decode()"):
            ok = self.decoder_session.run(inputs=inputs, outputs=outputs, stream=stream.cuda_stream)     # launch per kernel now
            assert ok, 'Engine execution failed'
            stream.synchronize()
        return outputs['output'], [outputs['present_key_value_' + str(i)] for i in range(n_layer)]

    # ---- language detection ---------------------------------------------------------------------------
    def _language_from_logits(self, logits, n_audio, single):
        """Mask everything but the language tokens, arg-max and softmax (W/decoding.py:724-735).  Same arithmetic as the
        reference (softmax over the full, masked row); only the language columns travel to the host, as one block --
        one `.item()` per (utterance, language) took 100 ms per batch of 576."""
        tk = self.tokenizer
        lang_tokens, codes = list(tk.all_language_tokens), list(tk.all_language_codes)
        key = (str(logits.device), logits.shape[-1])
        cache = getattr(self, "_lang_mask_cache", None)
        if cache is None or cache[0] != key:
            mask = torch.ones(logits.shape[-1], dtype=torch.bool)
            mask[lang_tokens] = False
            cache = (key, mask.to(logits.device), torch.tensor(lang_tokens, dtype=torch.long, device=logits.device))
            self._lang_mask_cache = cache
        _, mask_dev, idx = cache
        logits.masked_fill_(mask_dev, -np.inf)
        language_tokens = logits.argmax(dim=-1)
        probs = logits.softmax(dim=-1).index_select(-1, idx).cpu().tolist()
        language_probs = [dict(zip(codes, row)) for row in probs]
        if single:
            language_tokens, language_probs = language_tokens[0], language_probs[0]
            languages = [max(language_probs, key=language_probs.get)]
        else:
            languages = [max(p, key=p.get) for p in language_probs]
        return language_tokens, language_probs, languages

    def detect_language_reference(self, audio_features):
        """The reference's language-ID pass literally (W/decoding.py:703-741): cross K/V engine, one
        `decode()` of the single <|sot|> token through the by-name protocol."""
        if not self.is_multilingual:
            return ['en'] * audio_features.shape[0], None      # English-only vocabulary: no language tokens
        languages = [self.options.language] * audio_features.shape[0]
        language_probs = None
        if self.options.language is None or self.options.task == "lang_id":
            single = audio_features.ndim == 2
            if single:
                audio_features = audio_features.unsqueeze(0)
            n_audio = audio_features.shape[0]
            x = torch.tensor([[self.tokenizer.sot]] * n_audio).to(audio_features.device)    # [n_audio, 1]
            cross = self.xa2cross_key_value(audio_features)
            logits, _ = self.decode(x, cross)
            language_tokens, language_probs, languages = self._language_from_logits(logits[:, 0].float(), n_audio, single)
            if self.options.language is None:
                self.tokens = torch.tensor([self.initial_tokens]).repeat(n_audio, 1)
                self.tokens[:, self.sot_index + 1] = language_tokens.cpu()        # write language tokens
        return languages, language_probs

    def detect_language(self, audio_features, _retry: bool = False):
        """Language-ID pass, fast path: same arithmetic as detect_language_reference, but the cross
        K/V land in the persistent buffers main_loop re-uses (the reference computes them twice,
        SURVEY F6) and the one-token decoder call runs per utterance group on its stream."""
        if not self.is_multilingual:
            return ['en'] * audio_features.shape[0], None      # English-only vocabulary: no language tokens
        languages = [self.options.language] * audio_features.shape[0]
        language_probs = None
        if self.options.language is None or self.options.task == "lang_id":
            single = audio_features.ndim == 2
            if single:
                gen = getattr(audio_features, 'wm_generation', None)
                audio_features = audio_features.unsqueeze(0)
                if gen is not None:          # the view is the same encoder output: it keeps the stamp (_features_key; else the cross K/V
                    audio_features.wm_generation = gen      # of one clip would be projected twice, once per view)
            n_audio, dev = audio_features.shape[0], audio_features.device
            cfg = self.decoder_config
            if self._cross_group() > 1 and audio_features.is_cuda:
                # shared cross K/V: the pass runs over the n_audio utterances themselves (group 1), on the cross K/V and the first
                # n_audio cache rows of the buffer set main_loop will use -- nothing is repeated, nothing projected twice
                self._require_device_loop("detect_language")
                return self._detect_language_rows(audio_features, single, _retry)
            if self.n_group > 1 and self.device_sampling and audio_features.is_cuda:
                # best_of / beam candidates: main_loop decodes n_audio x n_group rows.  The state keeps ONE buffer set at a time, so a
                # language pass over n_audio rows would free and re-allocate the caches, the cross K/V buffers and the graphs on every
                # clip.  The pass runs over the candidates' rows instead -- the SAME repeated tensor main_loop will use
                # (_candidate_rows): one buffer set, the cross K/V computed once for both calls -- and reads every n_group-th row
                languages_r, probs_r = self._detect_language_rows(self._candidate_rows(audio_features), False, _retry)
                languages = languages_r[:: self.n_group]
                language_probs = probs_r[:: self.n_group] if probs_r is not None else None
                if self.options.language is None:
                    self.tokens = self.tokens[:: self.n_group].contiguous()
                if single:
                    language_probs = language_probs[0] if language_probs is not None else None
                return languages, language_probs
            return self._detect_language_rows(audio_features, single, _retry)
        return languages, language_probs

    def _cross_group(self) -> int:
        """Candidate rows that share one cross K/V row (wm_decoder_group_io::cross_group): n_group on a `shared_cross_kv` instance, else 1."""
        return self.n_group if self.shared_cross_kv else 1

    def _require_device_loop(self, what: str) -> None:
        if self.shared_cross_kv and self.n_group > 1:
            if not self.device_sampling:
                raise ValueError(f"{what}: shared_cross_kv needs the device loop (device_sampling = False is the literal host loop, which repeats the features)")
            if self.cu_partition:
                raise ValueError(f"{what}: shared_cross_kv is not supported by the CU-partitioned schedule (cu_partition = True)")

    def _candidate_rows(self, audio_features):
        """The audio features with every clip repeated n_group times (best_of / beam candidates share their utterance's audio: the
        reference repeats the features too, W/decoding.py:538-539) -- ONE tensor per encoder run, so that the language pass and the
        decode loop key the same cross K/V (`_features_key`) and the same buffer set."""
        from encoding import stamp_generation
        key = self._features_key(audio_features)
        c = getattr(self, "_rep_cache", None)
        if key is not None and c is not None and c[0] == key:
            return c[1]
        rep = stamp_generation(audio_features.repeat_interleave(self.n_group, dim=0))
        self._rep_cache = (key, rep, audio_features)       # (the original kept alive: its pointer is part of the key)
        return rep

    def _detect_language_rows(self, audio_features, single, _retry):
        """The pass itself over the rows of `audio_features` [n, n_audio_ctx, C] (detect_language)."""
        languages, language_probs = None, None
        n_audio, dev = audio_features.shape[0], audio_features.device
        cfg = self.decoder_config
        st = self._fast_state(n_audio * self._cross_group(), dev)     # (shared cross K/V: the candidates' buffer set, its first n_audio rows)
        n_micro, bounds = self._groups(n_audio, unit=1)
        one_row = self._may_run_alone(bounds, n_micro, self.lang_id_sequential, "found before the language pass")
        cross = self._cross_persistent(audio_features, st)
        if 'lang_logits' not in st:
            st['lang_logits'] = torch.empty((n_audio, 1, cfg['vocab_size']), dtype=torch.float16, device=dev)
            st['sot'] = torch.full((n_audio, 1), self.tokenizer.sot, dtype=torch.int32, device=dev)
        main = torch.cuda.current_stream()
        streams = self._group_streams(n_micro, dev)
        cap = cfg['num_text_ctx']
        use_graph = self.use_graphs and self.graph_prefill and self.decoder_session.qkv_amax is None and not self.profile_eager_passes
        na = steps_side_by_side(n_micro, self.lang_id_sequential, self.force_not_alone)
        for g, (lo, hi) in enumerate(bounds):
            fork(main, streams[g:g + 1])
            if self.lang_id_sequential and g > 0:
                streams[g].wait_stream(streams[g - 1])     # one group at a time: kernels are timed un-shared (bench.py)

            def issue_lang(g=g, lo=lo, hi=hi):
                self.decoder_session.decoder_step(st['sot'][lo:hi], self.positional_embedding[0:1],
                                                  [t[lo:hi] for t in cross], None, cap, [t[lo:hi] for t in st['kv']], cap,
                                                  st['lang_logits'][lo:hi], 0, streams[g].cuda_stream, slot=g, not_alone=na)
            # a launch per kernel (more than eight rows, or groups side by side): ~ 290 eager launches per group -> a replayed graph from the
            # second batch on.  (Up to eight rows alone the pass is the one-launch step: four launches, nothing to replay.)
            self._replay_or_issue(st, language_key(n_micro, g, na), streams[g], issue_lang, use_graph and (na or hi - lo > 8))
            join(main, streams[g:g + 1])
        language_tokens, language_probs, languages = self._language_from_logits(
            st['lang_logits'][:, 0].float(), n_audio, single)                # (brings the logits to the host: the pass has finished)
        if one_row and not _retry and self._chain_gave_up("language pass"):
            return self._detect_language_rows(audio_features, single, True)
        if self.options.language is None:
            self.tokens = torch.tensor([self.initial_tokens]).repeat(n_audio, 1)
            self.tokens[:, self.sot_index + 1] = language_tokens.cpu()        # write language tokens
        return languages, language_probs

    def torch_detect_language(self, model, audio_features):
        """PyTorch path (W/decoding.py:661-701): `model.logits(tokens, audio_features)`."""
        if not self.is_multilingual:
            return ['en'] * audio_features.shape[0], None
        with torch.no_grad():
            languages = [self.options.language] * audio_features.shape[0]
            language_probs = None
            if self.options.language is None or self.options.task == "lang_id":
                single = audio_features.ndim == 2
                if single:
                    audio_features = audio_features.unsqueeze(0)
                n_audio = audio_features.shape[0]
                x = torch.tensor([[self.tokenizer.sot]] * n_audio).to(audio_features.device)
                logits = model.logits(x, audio_features)[:, 0]
                language_tokens, language_probs, languages = self._language_from_logits(logits, n_audio, single)
                if self.options.language is None:
                    self.tokens = torch.tensor([self.initial_tokens]).repeat(n_audio, 1)
                    self.tokens[:, self.sot_index + 1] = language_tokens.cpu()
        for hook in self.hooks:
            hook.remove()
        self.kv_cache, self.hooks = {}, []
        return languages, language_probs

    def set_language_tokens(self, language_tokens: Sequence[int]) -> None:
        """Hand in the language token of every row of the next main_loop call instead of running detect_language: for rows whose
        language is known already (the later windows of a file, transcribe.py).  Same effect on the start sequences as the
        language pass has: one row of initial tokens per utterance with its language token behind <|startoftranscript|>."""
        if not self.is_multilingual:
            raise ValueError("set_language_tokens: an English-only vocabulary has no language tokens")
        valid = set(self.tokenizer.all_language_tokens)
        language_tokens = [int(t) for t in language_tokens]
        if not language_tokens or any(t not in valid for t in language_tokens):
            raise ValueError("set_language_tokens: need one language token of the vocabulary per row")
        self.tokens = torch.tensor([self.initial_tokens]).repeat(len(language_tokens), 1)
        self.tokens[:, self.sot_index + 1] = torch.tensor(language_tokens, dtype=self.tokens.dtype)

    def set_prompts(self, prompts: Optional[Sequence[Sequence[int]]]) -> None:
        """Hand in the prompt (token ids) of every utterance of the next main_loop calls -- the previous windows' text of a
        file, names and spellings -- for an instance built with `row_prompts=True`.  A prompt's last n_text_ctx // 2 - 1
        tokens are used, behind <|startofprev|>; an empty one leaves its row without <|startofprev|>, as upstream.  The prompts
        stay in force until they are set again (None: no prompts); they compose with `set_language_tokens` /
        `detect_language` in either order.  A main_loop call over another number of utterances is refused."""
        if not self.row_prompts:
            raise ValueError("set_prompts: needs an instance built with row_prompts=True (the start length is fixed at construction)")
        if prompts is None:
            self._prompts = None
            return
        prompts = [[int(t) for t in p] for p in prompts]
        V = self.decoder_config['vocab_size']
        if not prompts or any(t < 0 or t >= V for p in prompts for t in p):
            raise ValueError("set_prompts: need one list of token ids of the vocabulary per utterance")
        self._prompts = prompts

    # ---- decoding loops ---------------------------------------------------------------------------------
    def _initial_token_rows(self, n_audio, device):
        tokens = self.tokens
        if tokens.shape[0] != n_audio:
            tokens = torch.tensor([self.initial_tokens]).repeat(n_audio, 1)
        if self.row_prompts:
            # the rows so far carry the sot_sequence (with its language token) at their right end; the prompts go in front of it
            n_sot = len(self.sot_sequence)
            prompts = self._prompts if self._prompts is not None else [()] * n_audio
            if len(prompts) != n_audio:
                raise ValueError(f"set_prompts gave {len(prompts)} prompts, this call decodes {n_audio} utterances")
            rows, starts = right_aligned_rows(prompts, self.sot_sequence, self.tokenizer.sot_prev, self.decoder_config['num_text_ctx'])
            tokens = tokens.clone()
            tokens[:, :-n_sot] = torch.tensor(rows, dtype=tokens.dtype)[:, :-n_sot]
            self._row_starts = torch.tensor(starts, dtype=torch.int32).repeat_interleave(self.n_group)
        return tokens.repeat_interleave(self.n_group, dim=0).to(device)

    def _refuse_row_prompts(self, what: str) -> None:
        if self.row_prompts:
            raise ValueError(f"{what}: an instance built with row_prompts=True decodes through the device loop only "
                             "(main_loop with features on the GPU, device_sampling on)")

    def _host_call(self, temperature, n_rows):
        """What a host loop's call at `temperature` decodes with (`_call_decoder`), and the rows it keeps closed: in a sampling call of
        a beam instance (`fallback_best_of`) candidates j >= fallback_best_of of every utterance end before their first token."""
        decoder, n_cand = self._call_decoder(temperature)
        closed = None
        if n_cand < self.n_group:
            closed = (torch.arange(n_rows) % self.n_group) >= n_cand
        return decoder, closed

    def _host_step(self, i, logits, tokens, sum_logprobs, no_speech_probs, decoder=None, closed=None):
        if i == 0 and self.tokenizer.no_speech is not None:       # save no_speech_probs
            probs_at_sot = logits[:, self.sot_index].float().softmax(dim=-1)
            no_speech_probs[:] = probs_at_sot[:, self.tokenizer.no_speech].tolist()
        logits = logits[:, -1]
        for logit_filter in self.logit_filters:
            logit_filter.apply(logits, tokens)
        out = (decoder or self.decoder).update(tokens, logits, sum_logprobs)
        if closed is not None:          # closed rows: EOT from their first token on, nothing booked (the device loop's row_limit = 0)
            new_tokens = out[0]
            new_tokens[closed.to(new_tokens.device), -1] = self.tokenizer.eot
            sum_logprobs[closed.to(sum_logprobs.device)] = 0
            out = (new_tokens, bool((new_tokens[:, -1] == self.tokenizer.eot).all()), *out[2:])
        return out if len(out) == 3 else (*out, None)       # (tokens, completed, source rows of a beam step or None)

    def main_loop_reference(self, audio_features, temperature: Optional[float] = None):
        """The reference's loop verbatim in structure (W/decoding.py:785-821): one `decode()` per token,
        host-side filters, concat KV.  `temperature`: this call's (an instance with `fallback_best_of` samples above 0,
        `candidate_mode`; any other instance decodes with its own decoder whatever is passed)."""
        self._refuse_row_prompts("main_loop_reference")
        tokens = self._initial_token_rows(audio_features.shape[0], audio_features.device)
        n_batch = tokens.shape[0]
        decoder, closed = self._host_call(temperature, n_batch)
        sum_logprobs: Tensor = torch.zeros(n_batch, device=audio_features.device)
        no_speech_probs = [np.nan] * n_batch
        past_key_value = None
        if self.n_group > 1:        # best_of / beam candidates share their utterance's audio (upstream Whisper repeats it too)
            audio_features = audio_features.repeat_interleave(self.n_group, dim=0)
        cross = self.xa2cross_key_value(audio_features)
        if self.beam and decoder is self.decoder:
            self.decoder.reset(audio_features.shape[0] // self.n_group)
        for i in range(self.sample_len):
            feed = tokens if tokens.shape[-1] <= self.initial_token_length else tokens[:, -1:]
            logits, past_key_value = self.decode(feed, cross, past_key_value)
            tokens, completed, source = self._host_step(i, logits, tokens, sum_logprobs, no_speech_probs, decoder, closed)
            if source is not None and past_key_value is not None:       # the caches follow their beams
                past_key_value = [kv[source.to(kv.device)] for kv in past_key_value]
            if completed or tokens.shape[-1] > self.decoder_config['num_text_ctx']:
                break
        return tokens, sum_logprobs, no_speech_probs

    def torch_main_loop(self, model, audio_features, temperature: Optional[float] = None):
        """PyTorch path (W/decoding.py:743-783): `model.decoder(tokens, xa, kv_cache=)` with hooks.  `temperature`: as
        main_loop_reference."""
        self._refuse_row_prompts("torch_main_loop")
        with torch.no_grad():
            tokens = self._initial_token_rows(audio_features.shape[0], audio_features.device)
            n_batch = tokens.shape[0]
            sum_logprobs: Tensor = torch.zeros(n_batch, device=audio_features.device)
            no_speech_probs = [np.nan] * n_batch
            decoder, closed = self._host_call(temperature, n_batch)
            if self.beam:
                if decoder is self.decoder:
                    self.decoder.reset(audio_features.shape[0])
                audio_features = audio_features.repeat_interleave(self.n_group, dim=0)     # beams share their utterance's audio
            for i in range(self.sample_len):
                if not self.kv_cache:
                    self.kv_cache, self.hooks = model.install_kv_cache_hooks()
                feed = tokens if tokens.shape[-1] <= self.initial_token_length else tokens[:, -1:]
                logits = model.decoder(feed, audio_features, kv_cache=self.kv_cache)
                tokens, completed, source = self._host_step(i, logits, tokens, sum_logprobs, no_speech_probs, decoder, closed)
                if source is not None:                                   # the cached keys / values follow their beams (every per-row entry, as upstream)
                    for key, value in list(self.kv_cache.items()):
                        if torch.is_tensor(value) and value.shape[0] == source.shape[0]:
                            self.kv_cache[key] = value[source]
                if completed or tokens.shape[-1] > self.decoder_config['num_text_ctx']:
                    break
        for hook in self.hooks:
            hook.remove()
        self.kv_cache, self.hooks = {}, []
        return tokens, sum_logprobs, no_speech_probs

    # ---- fast path ----------------------------------------------------------------------------------------
    def _fast_state(self, n_batch, device):
        st = self._state.get(n_batch)
        if st is not None:
            return st
        # One buffer set at a time: a set holds the KV cache, the persistent cross K/V (245.76 MB per utterance at
        # large-v2: 141 GB at B = 576) and the captured graphs that point into them; a ragged last batch must not
        # allocate a second set next to the first.  Graphs go first (they reference the buffers).
        for old in self._state.values():
            old['graphs'].clear()
        self._state.clear()
        if device.type == 'cuda':
            torch.cuda.empty_cache()
        cfg = self.decoder_config
        n_layer, n_head, cap, V = cfg['num_layers'], cfg['num_heads'], cfg['num_text_ctx'], cfg['vocab_size']
        kv_dtype = torch.int8 if self.use_int8_kv_cache else torch.float16
        if device.type == 'cuda':
            # the batch ceiling is a property of the free memory, said up front instead of an allocator error half way through
            per_row = self.state_bytes_per_utterance()
            free, _ = torch.cuda.mem_get_info(device)
            if n_batch * per_row > free:
                raise RuntimeError(
                    f"WhisperDecoding: a batch of {n_batch} utterances needs {n_batch * per_row / 2**30:.1f} GiB of decoder state "
                    f"({per_row / 2**20:.1f} MiB per utterance: self-attention cache + cross-attention K/V of {n_layer} layers), "
                    f"{free / 2**30:.1f} GiB are free on {device}: at most {int(free // per_row)} utterances per batch fit "
                    f"(another WhisperDecoding's buffer set in this process counts against it)")
        tk = self.tokenizer
        suppress = []
        for f in self.logit_filters:
            if isinstance(f, SuppressTokens):
                suppress += list(f.suppress_tokens)
        if not self.options.without_timestamps and tk.no_timestamps is not None:
            suppress.append(tk.no_timestamps)
        suppress = sorted(set(suppress))
        blank = list(tk.blank_tokens()) + [tk.eot] if self.options.suppress_blank else []
        st = dict(
            kv=[torch.zeros((n_batch, 2, n_head, cap, 64), dtype=kv_dtype, device=device) for _ in range(n_layer)],
            cross=[torch.empty((n_batch // self._cross_group(), 2, n_head, cfg['num_audio_ctx'], 64),
                               dtype=torch.int8 if self.use_int8_cross_kv else torch.float16, device=device)
                   for _ in range(n_layer)],
            cross_key=None, cross_xa=None, graphs={}, counters={},
            tokens=torch.zeros((n_batch, cap + 1), dtype=torch.int32, device=device),
            logits=torch.empty((n_batch, self.initial_token_length, V), dtype=torch.float16, device=device),
            sum_logprobs=torch.zeros(n_batch, dtype=torch.float32, device=device),
            n_done=torch.zeros(1, dtype=torch.int32, device=device),
            done=torch.zeros(n_batch, dtype=torch.int32, device=device),          # per row: 1 once it has emitted EOT
            seed=torch.zeros(2, dtype=torch.int32, device=device),                # the sampling generator's seed (temperature > 0)
            live={},
            # per-row sample_len (stable address: the captured graphs read it); 2^30 = no limit
            row_limit=torch.full((n_batch,), 1 << 30, dtype=torch.int32, device=device),
            # per-row first slot (row_prompts; stable address: the captured graphs read it)
            row_start=torch.zeros(n_batch, dtype=torch.int32, device=device) if self.row_prompts else None,
            suppress=torch.tensor(suppress or [0], dtype=torch.int32, device=device), n_suppress=len(suppress),
            blank=torch.tensor(blank or [0], dtype=torch.int32, device=device), n_blank=len(blank),
        )
        if self._cross_group() > 1:
            # shared cross K/V: the prefill runs on ONE row per utterance (the candidates begin alike); its logits, and the first slot of
            # every utterance, before they are copied to the candidates' rows (_Group.prefill)
            n_utt = n_batch // self._cross_group()
            st.update(logits_u=torch.empty((n_utt, self.initial_token_length, V), dtype=torch.float16, device=device),
                      row_start_u=torch.zeros(n_utt, dtype=torch.int32, device=device) if self.row_prompts else None)
        if self.beam:
            # the beam step's outputs: parents, the pool of finished candidates per utterance, the proposals between its two launches
            K, MC = self.decoder.beam_size, self.decoder.max_candidates
            n_audio = n_batch // K
            st.update(
                parent=torch.zeros(n_batch, dtype=torch.int32, device=device),
                fin_tokens=torch.zeros((n_audio, MC, cap + 1), dtype=torch.int32, device=device),
                fin_scores=torch.zeros((n_audio, MC), dtype=torch.float32, device=device),
                fin_len=torch.zeros((n_audio, MC), dtype=torch.int32, device=device),
                fin_count=torch.zeros(n_audio, dtype=torch.int32, device=device),
                live_len=torch.zeros(n_audio, dtype=torch.int32, device=device),
                beam_ws=torch.empty(max(1, native.load_library().wm_beam_workspace_bytes(n_batch, K)) if device.type == 'cuda' else 1,
                                    dtype=torch.uint8, device=device),
                kv_tables={},
            )
        self._state[n_batch] = st
        return st

    def state_bytes_per_utterance(self) -> int:
        """Device bytes of decoder state one utterance of a batch holds (what `_fast_state` allocates per row): the
        self-attention cache [2, H, n_text_ctx, 64] and the cross-attention K/V [2, H, n_audio_ctx, 64] of every layer
        (245.76 MB at large-v2 with fp16 cross K/V), tokens and the prefill logits."""
        cfg = self.decoder_config
        n_layer, n_head, cap, V = cfg['num_layers'], cfg['num_heads'], cfg['num_text_ctx'], cfg['vocab_size']
        kv = 2 * n_head * cap * 64 * (1 if self.use_int8_kv_cache else 2)
        cross = 2 * n_head * cfg['num_audio_ctx'] * 64 * (1 if self.use_int8_cross_kv else 2)
        cross = -(-cross // self._cross_group())        # (shared_cross_kv: one copy per utterance, a row's share of it)
        per_row = n_layer * (kv + cross) + (cap + 1) * 4 + self.initial_token_length * V * 2 + 64
        if self._cross_group() > 1:        # ... and of its utterance's prefill logits (one row per utterance is prefilled)
            per_row += -(-self.initial_token_length * V * 2 // self._cross_group())
        if self.beam:       # parent + proposals per row, and the row's share of its utterance's pool (tokens, score, length) and counters
            K, MC = self.decoder.beam_size, self.decoder.max_candidates
            per_row += 4 + (K + 1) * 8 + -(-(MC * ((cap + 1) * 4 + 8) + 8) // K)
        return per_row

    def _group_streams(self, n, dev):
        """Side streams of the utterance groups (never the legacy default stream: graphs are captured on them).

        Each group gets a HARDWARE QUEUE OF ITS OWN: a stream created with a full CU mask
        (wm_stream_create_cu_mask) is never multiplexed, whereas ordinary streams share ROCm's pool of
        GPU_MAX_HW_QUEUES (4) queues and which of them end up sharing depends on how many streams the process
        created before.  Measured (B = 384, three groups): 18.1 ms per decode step with a queue per group, 23.5 ms when
        two groups happen to share one -- e.g. in any process that used one more stream earlier (RCCL, a calibration
        pass).  WM_DEDICATED_QUEUES=0 falls back to torch's stream pool."""
        if os.environ.get("WM_DEDICATED_QUEUES", "1") != "0" and not self._no_dedicated_queues:
            n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
            try:
                with torch.cuda.device(dev):
                    return [native.create_masked_stream([True] * n_cu, k) for k in range(n)]
            except native.WmError as e:       # a scheduling nicety, not part of the compute path: fall back to pooled streams
                logger.warning("dedicated hardware queues unavailable (%s): utterance groups use pooled streams", e)
                self._no_dedicated_queues = True
        while len(self._streams) < n:
            self._streams.append(torch.cuda.Stream(device=dev))
        return self._streams[:n]

    def _partition_streams(self, n, dev):
        """CU-partitioned streams for wm_decoder_step_multi: `n` light streams that may only use the first
        `light_cus` CUs and one heavy stream that owns the rest.  Measured on MI355X (scripts/cumask_probe.py):
        192 CUs still pull 6.4 TB/s through the cross-attention kernel, 64 CUs run the weight-streaming chain
        at its full-chip speed, and only with disjoint CU sets do the two actually run at the same time."""
        if self._partition is None or len(self._partition[0]) < n:
            n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
            light_cus = max(8, min(self.light_cus, n_cu // 2))
            light_mask = [i < light_cus for i in range(n_cu)]
            heavy_mask = [not b for b in light_mask]
            with torch.cuda.device(dev):
                light = [native.create_masked_stream(light_mask, k) for k in range(n)]
                heavy = native.create_masked_stream(heavy_mask, n)
            self._partition = (light, heavy)
        return self._partition[0][:n], self._partition[1]

    def _groups(self, n_batch, unit=None):
        # three groups from 128 utterances up (two chains of short kernels hide under the third group's K/V stream;
        # four concurrent chains are slower again: 18.1 / 28.0 ms per step at B = 384), two from 13 (round 6: 14 utterances 2.29 against
        # 2.39 ms per token step, 12: 2.15 either way, 10: 2.05 / 2.08; rounds 1-5: from 16), else one
        if self.micro_batches is None:
            n_micro = 3 if n_batch >= 128 else 2 if n_batch >= 13 else 1
        else:
            n_micro = self.micro_batches if n_batch >= 4 * self.micro_batches else 1
        # the beams of an utterance stay in one group (the beam step and the cache reorder work per utterance): cut in whole utterances
        # (so do the candidates that share a cross K/V row: the launch reads row b / n_group of the group's slice)
        if unit is None:
            unit = self.n_group if (self.beam or self.shared_cross_kv) else 1
        n_units = n_batch // unit
        n_micro = max(1, min(n_micro, n_units))
        return n_micro, [(g * n_units // n_micro * unit, (g + 1) * n_units // n_micro * unit) for g in range(n_micro)]

    def balanced_order(self, n_batch: int) -> List[int]:
        """For a batch whose rows are sorted by expected decode length: the permutation that deals them over the
        utterance groups (contiguous slices of the batch, `_groups`) like cards, so that every group holds short and long
        rows alike.  All groups then shrink together as rows finish -- their K/V streams and chains keep overlapping --
        instead of the group of the longest clips running on alone.  `batch[i] = sorted_batch[order[i]]`."""
        unit = self.n_group if (self.beam or self.shared_cross_kv) else 1        # (beam search, shared cross K/V: the groups are cut over the clips' candidate rows, in whole clips)
        n_micro, bounds = self._groups(n_batch * unit)
        bounds = [(lo // unit, hi // unit) for lo, hi in bounds]
        room = [hi - lo for lo, hi in bounds]
        members = [[] for _ in bounds]
        g = 0
        for i in range(n_batch):
            while room[g] == 0:
                g = (g + 1) % n_micro
            members[g].append(i)
            room[g] -= 1
            g = (g + 1) % n_micro
        return [i for m in members for i in m]

    def _cross_persistent(self, xa, st):
        """Cross K/V of `xa` in the state's persistent buffers (stable addresses: the captured decode
        graphs point at them).  Computed once per encoder run (`_features_key`: detect_language and main_loop
        on the same encoder output share them; anything else is recomputed)."""
        key = self._features_key(xa)
        if key is None or st['cross_key'] != key:
            xa16 = xa.type(torch.float16).contiguous()
            self.cross_attn_session.cross_kv(xa16, st['cross'], torch.cuda.current_stream().cuda_stream)
            st['cross_key'], st['cross_xa'] = key, xa
        return st['cross']

    def _capture(self, st, key, stream, issue):
        """Capture what `issue()` enqueues on `stream` (it has just been issued eagerly once, so every buffer and every workspace state it
        touches exists) into st['graphs'][key]."""
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        # capture_error_mode "thread_local" + CAPTURE_LOCK: the encoder of the NEXT batch may be in flight on a helper thread
        # (WhisperEncoding.prefetch), which waits for events and issues launches on its own stream.  Under the default
        # "global" mode such a call from ANY thread while this capture is open invalidates it (hipErrorStreamCaptureInvalidated
        # -- seen once in ~ 25 bench runs: the window is three captures of a millisecond or two against one event wait per
        # encoder layer); the lock keeps the helper out of the driver for the length of the capture as well.
        # (torch.cuda.graph's __enter__ synchronises the DEVICE while the lock is held: during a group's first capture the
        # helper cannot issue its next encoder layer until the layer in flight has finished -- 45-135 ms at B = 576, once
        # per group and process; the group stream was synchronised just above, so nothing of this loop is waited for)
        with native.CAPTURE_LOCK, torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            issue()
        st['graphs'][key] = graph

    def _replay_or_issue(self, st, key, stream, issue, use_graph) -> None:
        """A pass whose call is the same every time, on `stream`: replayed from st['graphs'][key] where that exists, else issued -- and,
        with `use_graph`, captured for the next time."""
        if use_graph and key in st['graphs']:
            with torch.cuda.stream(stream):
                st['graphs'][key].replay()
        else:
            issue()
            if use_graph:
                self._capture(st, key, stream, issue)

    def _may_run_alone(self, bounds, n_micro, sequential, where: str, peek: bool = True) -> bool:
        """`groups_run_alone` for a pass about to be issued -- and, where it may, a look at the give-up word first: one found set now is
        somebody else's (said loudly, acknowledged, not ours to repeat).  A peek at a host word: no synchronisation."""
        alone = groups_run_alone(bounds, n_micro, sequential, self.force_not_alone)
        if alone and peek and native.chain_status()["error_pending"]:
            self._chain_gave_up(where, foreign=True)
        return alone

    def _chain_gave_up(self, where: str, foreign: bool = False) -> bool:
        """Did a one-launch decode step (csrc/gemv_chain.hip: groups of up to eight rows) give up waiting for its workgroups since the last look?
        The launch needs its workgroups resident together; another tenant holding CUs or LDS while it is dispatched makes its bounded
        waits expire, and everything decoded from that step is invalid.  The library then stops using the one-launch forms on this
        device (wm_decode_chain_error: acknowledged, the device takes a launch per kernel from now on); graphs captured with chain
        launches are dropped -- those of EVERY WhisperDecoding of the process (another instance would go on replaying chain launches on
        a device the library has taken off the form).  Returns True when the caller has to decode again.
        `foreign`: the word was found set BEFORE this call issued anything -- an earlier call on this device (another instance, a
        Session.run, a C caller) produced an invalid step and never looked.  That is said at error level EVERY time: acknowledging clears
        the word, and the earlier caller's results stay wrong without anybody else being told."""
        err = C.c_int(0)
        native.check(native.load_library().wm_decode_chain_error(C.byref(err)), "wm_decode_chain_error")
        if not err.value:
            return False
        for inst in list(WhisperDecoding._instances):
            for st in inst._state.values():
                st['graphs'].clear()
        if foreign:
            logger.error("whisper_mi355: a one-launch decode step issued BEFORE this call (%s) gave up waiting for its workgroups and nobody "
                         "looked: whatever that earlier call returned on this device is INVALID (decode it again).  Acknowledged here; the "
                         "device takes a launch per kernel from now on (wm_set_decode_chain re-arms the one-launch step)", where)
        elif not WhisperDecoding._chain_warned:
            WhisperDecoding._chain_warned = True
            logger.warning("whisper_mi355: a one-launch decode step gave up waiting for its workgroups (%s; the GPU was not free to hold them "
                           "together): decoding again with a launch per kernel, which this device uses from now on "
                           "(wm_set_decode_chain re-arms the one-launch step)", where)
        return True

    _chain_warned = False
    _instances = weakref.WeakSet()

    def _live_list(self, st, n_micro, slot, lo, hi):
        """The group's list of rows still decoding (int32 [1 + n]: count, indices relative to the group), reset to
        "all of them"; wm_step_finish rebuilds it after every step from the `done` flags."""
        return self._all_live(st, (n_micro, slot), hi - lo)

    def _live_groups(self, st, n_micro, slot, lo, hi):
        """... and, for candidates that share a cross K/V row, the group's list of utterances with a live row (int32 [1 + n / G]),
        reset likewise; wm_step_finish_group rebuilds both."""
        return self._all_live(st, (n_micro, slot, 'utterances'), (hi - lo) // self._cross_group())

    @staticmethod
    def _all_live(st, key, n):
        if key not in st['live']:
            st['live'][key] = torch.empty(1 + n, dtype=torch.int32, device=st['done'].device)
        live = st['live'][key]
        live[0] = n
        live[1:] = torch.arange(n, dtype=torch.int32, device=live.device)
        return live

    def _fill_rules(self, io, st, lo, hi, logits_ptr, row_stride, cur_len, n_past_dev):
        """The fields wm_greedy_io and wm_beam_io share: where rows [lo, hi) of the batch state `st` and their logits are, and the
        logit rules."""
        tk = self.tokenizer
        io.logits, io.row_stride = logits_ptr, row_stride
        io.batch, io.n_vocab = hi - lo, self.decoder_config['vocab_size']
        io.tokens, io.tokens_ld, io.cur_len = st['tokens'][lo:hi].data_ptr(), st['tokens'].shape[1], cur_len
        io.sum_logprobs = st['sum_logprobs'][lo:hi].data_ptr()
        io.suppress, io.n_suppress = st['suppress'].data_ptr(), st['n_suppress']
        io.blank, io.n_blank = st['blank'].data_ptr(), st['n_blank']
        io.sample_begin, io.eot, io.timestamp_begin = self.sample_begin, tk.eot, tk.timestamp_begin
        io.max_initial_timestamp_index = -1 if self.max_initial_timestamp_index is None else self.max_initial_timestamp_index
        # 1: SuppressBlank + SuppressTokens + ApplyTimestampRules; 2: without_timestamps -- the reference then builds no timestamp
        # filter (W/decoding.py:337-346) and samples from the whole suppressed vocabulary
        io.apply_rules = 2 if self.options.without_timestamps else 1
        io.n_past_dev = n_past_dev.data_ptr() if n_past_dev is not None else None
        io.done, io.n_done = st['done'][lo:hi].data_ptr(), st['n_done'].data_ptr()
        io.row_limit = st['row_limit'][lo:hi].data_ptr()

    def _repeat_controls(self, st, lo, hi, logits_ptr, row_stride, cur_len, stream, n_past_dev=None):
        """Repetition penalty and no-repeat n-grams (wm_repeat_controls, csrc/repeat.hip) on the raw logits of rows [lo, hi) of the
        batch state `st`, before the token step: the same rows, tokens and flags as `_fill_rules` hands to it."""
        io = native.WmRepeatIO()
        io.logits, io.row_stride = logits_ptr, row_stride
        io.batch, io.n_vocab = hi - lo, self.decoder_config['vocab_size']
        io.tokens, io.tokens_ld, io.cur_len = st['tokens'][lo:hi].data_ptr(), st['tokens'].shape[1], cur_len
        io.n_past_dev = n_past_dev.data_ptr() if n_past_dev is not None else None
        io.sample_begin, io.eot = self.sample_begin, self.tokenizer.eot
        io.repetition_penalty, io.no_repeat_ngram_size = float(self.options.repetition_penalty), int(self.options.no_repeat_ngram_size)
        io.done = st['done'][lo:hi].data_ptr()
        native.check(native.load_library().wm_repeat_controls(C.byref(io), stream), "wm_repeat_controls")

    def _greedy(self, st, lo, hi, logits_ptr, row_stride, cur_len, stream, n_past_dev=None, temperature=None):
        """Fused logit rules + arg-max + append for utterances [lo, hi) of the batch state `st`."""
        io = native.WmGreedyIO()
        self._fill_rules(io, st, lo, hi, logits_ptr, row_stride, cur_len, n_past_dev)
        # temperature > 0: the draw happens in the same kernel (Gumbel-max, counter-based generator keyed on the global row: lo + b);
        # the seed lives in device memory so that a replayed graph draws afresh in every main_loop call
        io.temperature = float(self.options.temperature if temperature is None else temperature)     # (a per-call temperature: main_loop)
        io.row0, io.seed_dev = lo, st['seed'].data_ptr()
        native.check(native.load_library().wm_greedy_step(C.byref(io), stream), "wm_greedy_step")

    def _beam(self, st, lo, hi, logits_ptr, row_stride, cur_len, stream, kv_table, ignore_eot, n_past_dev=None):
        """Beam step + cache reorder for rows [lo, hi) (whole utterances) of the batch state `st`: wm_beam_step applies the logit rules,
        picks and moves the beams, wm_kv_reorder lets every layer's self-attention cache rows follow their parents."""
        cfg, lib = self.decoder_config, native.load_library()
        K, MC = self.decoder.beam_size, self.decoder.max_candidates
        a_lo, a_hi = lo // K, hi // K
        io = native.WmBeamIO()
        self._fill_rules(io, st, lo, hi, logits_ptr, row_stride, cur_len, n_past_dev)
        io.beam_size, io.max_candidates, io.ignore_eot = K, MC, int(bool(ignore_eot))
        io.parent = st['parent'][lo:hi].data_ptr()
        io.fin_tokens, io.fin_scores = st['fin_tokens'][a_lo:a_hi].data_ptr(), st['fin_scores'][a_lo:a_hi].data_ptr()
        io.fin_len, io.fin_count = st['fin_len'][a_lo:a_hi].data_ptr(), st['fin_count'][a_lo:a_hi].data_ptr()
        io.live_len = st['live_len'][a_lo:a_hi].data_ptr()
        ws = st['beam_ws'][lo * (K + 1) * 8: hi * (K + 1) * 8]
        io.workspace, io.workspace_bytes = ws.data_ptr(), ws.numel()
        native.check(lib.wm_beam_step(C.byref(io), stream), "wm_beam_step")
        native.check(lib.wm_kv_reorder(kv_table.data_ptr(), cfg['num_layers'], hi - lo, K, cfg['num_heads'], cfg['num_text_ctx'],
                                       1 if self.use_int8_kv_cache else 2, st['parent'][lo:hi].data_ptr(), st['done'][lo:hi].data_ptr(),
                                       cur_len - 1, io.n_past_dev, stream), "wm_kv_reorder")

    def main_loop(self, audio_features, ignore_eot: bool = False, row_limit=None, _retry: bool = False,
                  temperature: Optional[float] = None):
        """`_main_loop` with the in-flight mark around it: word_timestamps reuses the loop's buffers and refuses to run inside it
        (a callback, another thread); the mark is cleared however the loop ends."""
        self._decode_in_flight += 1
        try:
            return self._main_loop(audio_features, ignore_eot=ignore_eot, row_limit=row_limit, _retry=_retry, temperature=temperature)
        finally:
            self._decode_in_flight -= 1

    def _main_loop(self, audio_features, ignore_eot: bool = False, row_limit=None, _retry: bool = False,
                   temperature: Optional[float] = None):
        """Greedy decoding, fast path.  Same return values as the reference's main_loop
        (tokens int64 [n, <=n_text_ctx+1], sum_logprobs fp32 [n], no_speech_probs list).
        `ignore_eot` (benchmarks with random weights) decodes `sample_len` tokens regardless.
        `row_limit` (optional, int [n]): a per-utterance `sample_len` -- row b ends with EOT after row_limit[b] sampled
        tokens (e.g. a bound from the clip's duration; bench.py's length distributions).
        `temperature` (optional): this call's sampling temperature instead of the options' (the fallback ladder of long-form
        transcription, transcribe.py).  The captured graphs bake the scalar in, so a call at another temperature has graphs of
        its own; beam search and best_of keep the instance's temperature.

        Utterances are independent, so the batch is cut into `micro_batches` groups that advance in
        lock-step on separate HIP streams: while one group streams its cross-attention K/V (the
        HBM-bound part of a step) the other group runs its latency-bound weight-streaming chain.
        Rows that have emitted EOT drop out of the attention kernels and a group whose rows are all
        finished is no longer stepped (`skip_finished_rows`): the loop's cost follows the live rows."""
        # 1. option checks and mode selection
        features_in = audio_features
        temp = float(self.options.temperature if temperature is None else temperature)
        mode, n_cand = candidate_mode(self.options, self.fallback_best_of, temp)
        beam = self.beam and mode == "beam"                 # this call's decoder (fallback_best_of: samples above temperature 0)
        G = self._cross_group()
        self._check_device_call(audio_features, temp)
        if temp != 0 or self.n_group != 1 or self.beam:
            # Sampling options (W/decoding.py:274-300 temperature, :92-115 best_of + ranker).  Round 4: the device loop takes them --
            # the draw is a Gumbel-max inside the greedy kernel, candidates are rows like any others.  `device_sampling = False`
            # (or tensors that are not on the GPU) keeps the literal host loop: torch's generator, the draws the goldens hold.
            if not self.device_sampling or not audio_features.is_cuda:
                return self.main_loop_reference(audio_features)
            if self.n_group > 1 and G == 1:      # candidates share their utterance's audio: the reference repeats the features too (:538-539 of this file)
                audio_features = self._candidate_rows(audio_features)
        n_batch, dev = audio_features.shape[0] * G, audio_features.device
        n_micro, bounds = self._groups(n_batch)
        self._check_partition(n_micro)
        # 2. state reset
        tokens0 = self._initial_token_rows(n_batch // self.n_group, dev)
        assert tokens0.shape[0] == n_batch
        L0 = tokens0.shape[1]
        st = self._fast_state(n_batch, dev)
        one_row = self._may_run_alone(bounds, n_micro, self.groups_sequential, "found before the decode loop", peek=not _retry)
        cross = self._reset_state(st, audio_features, tokens0, row_limit, n_cand, reseed=temp != 0 and not _retry)
        if self.cu_partition and n_micro > 1 and self.decoder_session.qkv_amax is None and row_limit is None and temp == self.options.temperature:
            return self._main_loop_partitioned(audio_features, st, cross, L0, n_micro, bounds, ignore_eot)
        # 3. group construction
        use_graph = self.use_graphs and self.decoder_session.qkv_amax is None
        block = self.block_prefill and L0 > 4
        call = _Call(st=st, cross=cross, L0=L0, n_micro=n_micro, beam=beam, ignore_eot=ignore_eot, temperature=temp,
                     use_live=bool(self.skip_finished_rows) and not ignore_eot and max(hi - lo for lo, hi in bounds) <= 1024,
                     not_alone=steps_side_by_side(n_micro, self.groups_sequential, self.force_not_alone),
                     bkey=call_key(beam, ignore_eot, G, temp, self.options.temperature),
                     use_graph=use_graph, block=block, graph_prefill=use_graph and self.graph_prefill and (L0 <= 4 or block))
        main = torch.cuda.current_stream()
        streams = self._group_streams(n_micro, dev)
        groups = [_Group(self, call, g, lo, hi, streams[g]) for g, (lo, hi) in enumerate(bounds)]
        fork(main, streams)
        # 4. the loop
        cur, nsp_dev = self._run_groups(call, groups, main, streams)
        # 5. finish
        join(main, streams)
        finish = self._finish_beam_loop if beam else self._finish_main_loop
        out = finish(st, cur, L0, n_batch, ignore_eot, nsp_dev)
        self._rep_cache = None        # the candidates' repeated features (best_of): the language pass and this loop have both used them
        # 6. the give-up retry
        if one_row and not _retry and self._chain_gave_up("decode loop"):
            # one-row groups run the token step as ONE launch whose workgroups wait for each other with bounded spins; a wait that was
            # given up invalidates the step and every token after it.  The utterance is decoded again, in this process, on the
            # launch-per-kernel path (the library has taken the device off the one-launch forms; the captured graphs are gone).
            return self.main_loop(features_in, ignore_eot=ignore_eot, row_limit=row_limit, _retry=True, temperature=temperature)
        return out

    def _check_device_call(self, audio_features, temp: float) -> None:
        """What a main_loop call at temperature `temp` over `audio_features` refuses before it touches anything."""
        self._require_device_loop("main_loop")
        if self._cross_group() > 1 and not audio_features.is_cuda:
            raise ValueError("main_loop: shared_cross_kv needs the device loop (features on the GPU)")
        if temp != self.options.temperature:
            if (self.beam or self.n_group != 1) and self.fallback_best_of is None:
                raise ValueError("a per-call temperature is not supported with beam_size / best_of: they decode at the instance's temperature")
            if not self.device_sampling or not audio_features.is_cuda:
                raise ValueError("a per-call temperature needs the device loop (device_sampling on, features on the GPU)")

    def _check_partition(self, n_micro: int) -> None:
        """What the CU-partitioned schedule does not serve."""
        if not self.cu_partition:
            return
        if self.repeat_controls_on:
            raise ValueError("repetition_penalty / no_repeat_ngram_size are not supported by the CU-partitioned schedule (cu_partition = True): "
                             "it has a loop of its own; use the default loop")
        if n_micro > 1 and self.beam:
            raise ValueError("beam_size is not supported by the CU-partitioned schedule (cu_partition = True): use the default loop")
        if self.block_prefill:
            raise ValueError("block_prefill is not supported by the CU-partitioned schedule (cu_partition = True): use the default loop")
        if n_micro > 1 and self.row_prompts:
            raise ValueError("row_prompts is not supported by the CU-partitioned schedule (cu_partition = True): use the default loop")

    def _reset_state(self, st, audio_features, tokens0, row_limit, n_cand: int, reseed: bool):
        """The batch state `st` as a device-loop call finds it: seed, tokens, flags, per-row limits and first slots.  Returns the cross
        K/V of `audio_features` in the state's persistent buffers."""
        n_batch, L0 = tokens0.shape
        if reseed:        # a fresh seed per call from torch's generator: torch.manual_seed makes a run repeatable
            st['seed'].copy_(torch.randint(0, 2 ** 31 - 1, (2,), dtype=torch.int32))
        cross = self._cross_persistent(audio_features, st)
        st['tokens'].zero_()
        st['tokens'][:, :L0] = tokens0.to(torch.int32)
        st['sum_logprobs'].zero_()
        st['n_done'].zero_()
        st['done'].zero_()
        if self.beam:
            st['fin_count'].zero_()
            st['live_len'].zero_()
        if row_limit is not None:
            row_limit = torch.as_tensor(row_limit).to(device=tokens0.device, dtype=torch.int32)
            assert row_limit.shape == (n_batch,)
            st['row_limit'].copy_(row_limit)
        else:
            st['row_limit'].fill_(1 << 30)
        if n_cand < self.n_group:
            # a sampling call of a beam instance: candidates j >= n_cand of every utterance are closed before their first token (EOT,
            # nothing booked): they drop out of the kernels with the first live list and never reach the ranker (post_process)
            st['row_limit'].view(-1, self.n_group)[:, n_cand:] = 0
        if self.row_prompts:
            st['row_start'].copy_(self._row_starts)
            if self._cross_group() > 1:
                st['row_start_u'].copy_(self._row_starts[::self._cross_group()])
        return cross

    def _issue_step(self, call: _Call, gr: _Group, i: int, cur: int) -> None:
        """Step `i` of one group, on its stream: replayed where a graph of it exists, else issued (and captured for the next time)."""
        st, graphs = call.st, call.st['graphs']
        if i == 0:
            # the prefill (L0 tokens on an empty cache) + the first token step.  Round 6: replayed from a graph from the second
            # batch on -- the call is the same for every batch (state buffers, L0 and the start position are fixed), and issued
            # eagerly its ~ 390 launches per group are HOST-bound at small and middle batches (7 us each: 2.7 ms per group where the
            # GPU needs 1.7 at one utterance; with the language pass 9.5 ms per batch of 2 x 8)
            self._replay_or_issue(st, gr.prefill_key, gr.stream, lambda: gr.prefill(call.L0), call.graph_prefill)
        elif call.use_graph and gr.step_key in graphs:
            if i == 1 or st['counters'][gr.fresh_key]:
                # the device step counter holds n_past = cur - 1; (re)seed it on the group's stream
                with torch.cuda.stream(gr.stream):
                    st['counters'][gr.step_key].fill_(cur - 1)
                st['counters'][gr.fresh_key] = False
            with torch.cuda.stream(gr.stream):
                graphs[gr.step_key].replay()
        else:
            gr.step(cur)
            if call.use_graph:
                # capture ONE decode step (decoder + token step + counter advance) of this group;
                # every later token replays it: T is read from a device counter inside the kernels
                counter = torch.zeros(1, dtype=torch.int32, device=gr.done.device)
                self._capture(st, gr.step_key, gr.stream, lambda: gr.step_counted(counter))
                st['counters'][gr.step_key] = counter
                st['counters'][gr.fresh_key] = True

    def _run_groups(self, call: _Call, groups: List[_Group], main, streams):
        """The loop itself: per token every active group's step, and the three points of it where the host looks.  Returns the length
        the rows have reached and the no-speech probabilities (on the device, or None)."""
        st, cap = call.st, self.decoder_config['num_text_ctx']
        cur, steps_done, nsp_dev, last_issued = call.L0, 0, None, None
        for i in range(self.sample_len):
            for gr in groups:
                if not gr.active:
                    continue
                if self.groups_sequential and call.n_micro > 1:
                    if last_issued is not None:
                        gr.stream.wait_stream(last_issued)
                    last_issued = gr.stream
                self._issue_step(call, gr, i, cur)
            if i == 0 and self.tokenizer.no_speech is not None:
                # the token step has already written -inf into the LAST position's row only;
                # the <|sot|> position (no-speech probability, decoding.py:803-807) is untouched
                join(main, streams)
                probs_at_sot = st['logits'][:, self.sot_index].float().softmax(dim=-1)
                nsp_dev = probs_at_sot[:, self.tokenizer.no_speech]
                fork(main, streams)
            if i == 0 and self.first_token_event is not None:
                # latency probe (bench.py): the first sampled token of every row exists once the groups' first steps have run
                join(main, streams)
                self.first_token_event.record(main)
                fork(main, streams)
            cur += 1
            steps_done += 1
            if cur > cap:
                break
            if not call.ignore_eot and (steps_done % self.poll_every == 0):
                # `done` is sticky (a finished row stays at EOT), so "every row is done" is monotone;
                # poll it now and then instead of synchronising every step
                join(main, streams)
                done_host = st['done'].bool().cpu()
                if bool(done_host.all()):
                    break
                if call.use_live:
                    for gr in groups:         # a group with no live row left costs a whole chain of launches per token: drop it
                        if gr.active and bool(done_host[gr.lo:gr.hi].all()):
                            gr.active = False
        return cur, nsp_dev

    def _main_loop_partitioned(self, audio_features, st, cross, L0, n_micro, bounds, ignore_eot):
        """The decode loop scheduled for the chip (wm_decoder_step_multi): every group's cross-attention kernel
        on one stream that owns most CUs, each group's short kernels on a stream confined to the remaining
        CUs, eager launches with the step counter on the device (the call is identical for every token).
        Same arithmetic, same tokens as the single-stream loop."""
        dev = audio_features.device
        cfg = self.decoder_config
        V, cap = cfg['vocab_size'], cfg['num_text_ctx']
        n_batch = st['tokens'].shape[0]
        sess, pos, lib = self.decoder_session, self.positional_embedding, native.load_library()
        main = torch.cuda.current_stream()
        light, heavy = self._partition_streams(n_micro, dev)
        fork(main, light + [heavy])
        light_ptrs, heavy_ptr = [s_.cuda_stream for s_ in light], heavy.cuda_stream
        key = partition_key(n_micro)
        if key not in st['graphs']:
            counters = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in bounds]
            views = [dict(kv=[t[lo:hi] for t in st['kv']], cross=[t[lo:hi] for t in cross], logits=st['logits'][lo:hi],
                          tokens=st['tokens'][lo:hi]) for lo, hi in bounds]
            prefill = [sess.make_decoder_io(v['tokens'][:, :L0], pos[0:L0], v['cross'], None, cap, v['kv'], cap, v['logits'], 0,
                                            slot=g) for g, v in enumerate(views)]
            step = [sess.make_decoder_io(v['tokens'], pos, v['cross'], v['kv'], cap, v['kv'], cap, v['logits'], 1, slot=g,
                                         n_past_dev=counters[g], n_new=1) for g, v in enumerate(views)]
            st['graphs'][key] = dict(counters=counters, prefill=prefill, step=step, views=views)
        plan = st['graphs'][key]
        cur = L0
        steps_done = 0
        in_flight = []            # one event per issued step: the three queues only interleave well while the host
        for i in range(self.sample_len):          # is a few steps ahead, not when it runs into a full queue mid-step
            if len(in_flight) >= self.run_ahead:
                in_flight.pop(0).synchronize()
            if i == 0:
                sess.decoder_step_multi(plan['prefill'], light_ptrs, heavy_ptr)
                for g, (lo, hi) in enumerate(bounds):
                    self._greedy(st, lo, hi, plan['views'][g]['logits'].data_ptr() + (L0 - 1) * V * 2, L0 * V, cur, light_ptrs[g])
                if self.tokenizer.no_speech is not None:
                    # the greedy kernel wrote -inf into the LAST position's row only; the <|sot|> row is untouched
                    join(main, light)
                    nsp_dev = st['logits'][:, self.sot_index].float().softmax(dim=-1)[:, self.tokenizer.no_speech]
                    fork(main, light)
            else:
                if i == 1:
                    for g, s_ in enumerate(light):
                        with torch.cuda.stream(s_):
                            plan['counters'][g].fill_(cur - 1)      # the device step counter holds n_past = cur - 1
                sess.decoder_step_multi(plan['step'], light_ptrs, heavy_ptr)
                for g, (lo, hi) in enumerate(bounds):
                    self._greedy(st, lo, hi, plan['views'][g]['logits'].data_ptr(), V, 0, light_ptrs[g],
                                 n_past_dev=plan['counters'][g])
                    native.check(lib.wm_step_advance(plan['counters'][g].data_ptr(), light_ptrs[g]), "wm_step_advance")
            done = torch.cuda.Event()
            done.record(light[0])
            in_flight.append(done)
            cur += 1
            steps_done += 1
            if cur > cap:
                break
            if not ignore_eot and (steps_done % self.poll_every == 0):
                join(main, light)
                if bool((st['tokens'][:, cur - 1] == self.tokenizer.eot).all()):
                    break
        join(main, light + [heavy])
        return self._finish_main_loop(st, cur, L0, n_batch, ignore_eot,
                                      nsp_dev if self.tokenizer.no_speech is not None else None)

    def _finish_main_loop(self, st, cur, L0, n_batch, ignore_eot, nsp_dev):
        tokens = st['tokens'][:, :cur].to(torch.int64)
        if not ignore_eot:
            # a finished row stays at EOT (W/decoding.py:295); the columns a dropped group no longer wrote are EOT too
            eot = self.tokenizer.eot
            after = (tokens[:, L0:] == eot).cumsum(dim=1) > 0
            tokens[:, L0:] = torch.where(after, torch.full_like(tokens[:, L0:], eot), tokens[:, L0:])
            # cut at the first column where every row is EOT: where the per-step check would have stopped
            all_eot = (tokens[:, L0:] == self.tokenizer.eot).all(dim=0)
            if bool(all_eot.any()):
                tokens = tokens[:, :L0 + int(all_eot.float().argmax()) + 1]
        no_speech_probs = [np.nan] * n_batch
        if nsp_dev is not None:
            no_speech_probs = nsp_dev.tolist()
        return tokens, st['sum_logprobs'].clone(), no_speech_probs

    def _finish_beam_loop(self, st, cur, L0, n_batch, ignore_eot, nsp_dev):
        """The beam loop's results: the live beams as the (tokens, sum_logprobs, no_speech_probs) triple, and the device's pools and
        freeze lengths handed to `self.decoder`, whose `finalize` (post_process) then builds the candidates exactly as after the
        literal loop."""
        K = self.decoder.beam_size
        tokens = st['tokens'][:, :cur].to(torch.int64)
        count, length = st['fin_count'].tolist(), st['fin_len'].tolist()
        scores, fin, live_len = st['fin_scores'].tolist(), st['fin_tokens'].cpu(), st['live_len'].tolist()
        self.decoder.reset(n_batch // K)
        for a in range(n_batch // K):
            self.decoder.pool[a] = [(fin[a, e, :length[a][e]].tolist(), scores[a][e]) for e in range(count[a])]
            self.decoder.live_len[a] = live_len[a] if live_len[a] > 0 else None
        no_speech_probs = nsp_dev.tolist() if nsp_dev is not None else [np.nan] * n_batch
        return tokens, st['sum_logprobs'].clone(), no_speech_probs

    # ---- word-level timestamps (timing.py states the contract; DESIGN.md "word timestamps") ---------------------------------
    def alignment_heads(self) -> List[int]:
        """The cross-attention heads to align on, as layer * n_head + head, ascending: the engine's `alignment_heads`
        (build.py --alignment_heads) or upstream's default, every head of the upper half of the decoder layers."""
        cfg = self.decoder_config
        return timing.parse_alignment_heads(cfg.get('alignment_heads'), cfg['num_layers'], cfg['num_heads'])

    def _forced_tokens(self, sampled: Sequence[int]) -> Tuple[List[int], List[int]]:
        """(text, forced sequence) of one utterance: the sampled tokens without the timestamp tokens, and
        sot_sequence + <|notimestamps|> + text + <|endoftext|> -- no prompt, no prefix, as upstream."""
        tk = self.tokenizer
        text = [int(t) for t in sampled if int(t) < tk.eot]
        return text, list(tk.sot_sequence) + [tk.no_timestamps] + text + [tk.eot]

    def _split_words(self, tokens: List[int], language: Optional[str]):
        """Words of `tokens` under the utterance's own language (the tokenizer carries the engine's default one)."""
        return self.tokenizer.split_to_word_tokens(tokens, language=language)

    def _align_frames(self, num_frames, n_audio) -> List[int]:
        """F per utterance: half the mel frames of real audio, at most n_audio_ctx (the default: the whole window)."""
        ctx = self.decoder_config['num_audio_ctx']
        if num_frames is None:
            return [ctx] * n_audio
        frames = [int(f) for f in (num_frames.tolist() if hasattr(num_frames, 'tolist') else num_frames)]
        if len(frames) != n_audio:
            raise ValueError(f"word timestamps: {len(frames)} num_frames for {n_audio} utterances")
        return [max(0, min(f, 2 * ctx)) // 2 for f in frames]

    @staticmethod
    def _result_tokens(results) -> List[List[int]]:
        return [list(r.tokens) if hasattr(r, 'tokens') else [int(t) for t in r] for r in results]

    def torch_word_timestamps(self, model, audio_features, tokens, num_frames=None) -> List[List[timing.WordTiming]]:
        """The literal statement of the word-timestamp contract, on the PyTorch model (any device, any dtype of the features):
        one teacher-forced `model.decoder` pass per utterance with the cross-attention scores captured, then timing.py's steps.
        `tokens`: per utterance the sampled tokens (or the DecodingResults of post_process); `num_frames`: mel frames of real
        audio per utterance (default: the whole window).  Differences from upstream: Z = 0 where a frame's weights have no
        spread over the tokens (upstream: NaN), and none of the long-form duration heuristics."""
        languages = [getattr(r, 'language', None) for r in tokens]
        tokens = self._result_tokens(tokens)
        frames = self._align_frames(num_frames, len(tokens))
        heads, n_head = self.alignment_heads(), self.decoder_config['num_heads']
        n_prefix, eot = len(self.tokenizer.sot_sequence), self.tokenizer.eot
        seconds_per_frame = CHUNK_LENGTH / self.decoder_config['num_audio_ctx']
        out, kept = [], []
        for b, sampled in enumerate(tokens):
            text, forced = self._forced_tokens(sampled)
            if not text or frames[b] < 1:
                out.append([])
                kept.append(None)
                continue
            scores: List[Tensor] = []
            with torch.no_grad():
                x = torch.tensor([forced], dtype=torch.long, device=audio_features.device)
                logits = model.decoder(x, audio_features[b:b + 1], cross_scores=scores)[0]
            S_list = [scores[i // n_head][0, i % n_head, :, :frames[b]].float().cpu() for i in heads]
            mtx = timing.alignment_matrix(S_list, n_prefix)
            text_idx, time_idx = timing.dtw_cpu(-mtx.numpy())
            probs = logits[n_prefix:, :eot].float().softmax(dim=-1).cpu()
            token_probs = probs[torch.arange(len(text)), torch.tensor(text)].tolist()
            words, word_tokens = self._split_words(text + [eot], languages[b])
            out.append(timing.words_from_path(text_idx, time_idx, words, word_tokens, token_probs, seconds_per_frame))
            kept.append(dict(scores=S_list, matrix=mtx, path_text=text_idx, path_time=time_idx, token_probs=token_probs))
        self.last_alignment = kept
        return out

    def word_timestamps(self, audio_features, results, num_frames=None, token_probs: str = "torch") -> List[List[timing.WordTiming]]:
        """When each word of `results` (the DecodingResults of post_process for `audio_features`) was spoken: upstream
        Whisper's find_alignment on the device.  A second, teacher-forced pass over sot_sequence + <|notimestamps|> + text + EOT
        (4 tokens per call, wm_decoder_step_tap) records the cross-attention queries of the alignment heads; wm_align turns
        them and the cross K/V that main_loop left in place into the alignment matrix and its DTW path; timing.words_from_path
        reads the word boundaries off the path.  The pass reuses main_loop's cross K/V (same features: nothing is recomputed)
        and its self-attention cache buffers, so no decode may be in flight.  `num_frames`: mel frames of real audio per
        utterance (default: the whole window).  Beam search / best_of (n_group > 1): on a `shared_cross_kv` instance the pass runs
        over the n_audio winners with group 1, on the one cross K/V set main_loop left in place and the first n_audio rows of its
        self-attention caches; an instance whose candidates hold a copy each is refused (their rows' cross K/V are interleaved per
        candidate): use torch_word_timestamps.
        `token_probs`: where the probability of every forced token is computed from the pass's logits -- "torch" (the default:
        an fp32 copy of each call's slab, logsumexp and gather) or "device" (wm_forced_probs, csrc/forced_probs.hip: the fp16
        logits read once; long-form transcription uses it).  The two agree to fp32 rounding, not bit for bit."""
        if token_probs not in ("torch", "device"):
            raise ValueError(f"word_timestamps: token_probs = {token_probs!r}: 'torch' or 'device'")
        if self.n_group > 1 and not self.shared_cross_kv:
            raise ValueError("word_timestamps: beam_size / best_of > 1 is not supported on the device path in this version "
                             "unless the instance shares its cross K/V (shared_cross_kv=True; torch_word_timestamps has no such limit)")
        if self.use_int8_cross_kv:
            raise native.WmError("word timestamps need fp16 cross-attention K/V; this engine stores int8 codes (WM_FLAG_INT8_CROSS_KV)")
        if self._decode_in_flight:
            raise RuntimeError("word_timestamps reuses main_loop's buffers: no decode may be in flight")
        if not audio_features.is_cuda:
            raise ValueError("word_timestamps runs on the GPU (torch_word_timestamps is the CPU statement)")
        dev = audio_features.device
        cfg = self.decoder_config
        n, V, cap, ctx = audio_features.shape[0], cfg['vocab_size'], cfg['num_text_ctx'], cfg['num_audio_ctx']
        sampled = self._result_tokens(results)
        if len(sampled) != n:
            raise ValueError(f"word_timestamps: {len(sampled)} results for {n} utterances")
        languages = [getattr(r, 'language', None) for r in results]
        tk = self.tokenizer
        eot, n_prefix = tk.eot, len(tk.sot_sequence)
        forced = [self._forced_tokens(s) for s in sampled]
        frames = self._align_frames(num_frames, n)
        n_all = [len(f) if t else 0 for t, f in forced]          # no text: no words, nothing to align (n_tokens - n_prefix - 1 < 1)
        L = max(max(len(f) for _, f in forced), 1)
        if L > cap:
            raise ValueError(f"word_timestamps: a forced sequence of {L} tokens exceeds n_text_ctx = {cap}")
        rows = torch.full((n, L + 1), eot, dtype=torch.int32)
        for b, (_, f) in enumerate(forced):
            rows[b, :len(f)] = torch.tensor(f, dtype=torch.int32)
        rows = rows.to(dev)
        heads = self.alignment_heads()
        heads_arr = (C.c_int32 * len(heads))(*heads)
        lib, sess, pos = native.load_library(), self.decoder_session, self.positional_embedding
        st = self._fast_state(n * self._cross_group(), dev)      # (shared cross K/V: the candidates' buffer set; n rows of it are used)
        cross = self._cross_persistent(audio_features, st)
        stream = torch.cuda.current_stream().cuda_stream
        tape = torch.empty((n, len(heads), L, 64), dtype=torch.float16, device=dev)
        logits = torch.empty(n * 4 * V, dtype=torch.float16, device=dev)
        probs = torch.zeros((n, L), dtype=torch.float32, device=dev)
        _, bounds = self._groups(n, unit=1)
        for g, (lo, hi) in enumerate(bounds):
            kv, cr = [t[lo:hi] for t in st['kv']], [t[lo:hi] for t in cross]
            for off in range(0, L, 4):
                l = min(4, L - off)
                lg = logits[: (hi - lo) * l * V].view(hi - lo, l, V)
                sess.decoder_step_tap(rows[lo:hi, off:off + l], pos[off:off + l], cr, kv if off else None, cap, kv, cap, lg, off,
                                      stream, tape[lo:hi], heads_arr, slot=1000 + g)
                # the probability the pass gives the token that follows, over the text tokens only ([:eot]); no [B, L, V] tensor
                if token_probs == "device":
                    native.check(lib.wm_forced_probs(lg.data_ptr(), hi - lo, l, V, l * V, V, eot, rows[lo:hi, off + 1:].data_ptr(),
                                                     L + 1, probs[lo:hi, off:].data_ptr(), L, stream), "wm_forced_probs")
                    continue
                lf = lg[:, :, :eot].float()
                nxt = rows[lo:hi, off + 1: off + l + 1].long().clamp(max=eot - 1)
                probs[lo:hi, off:off + l] = (lf.gather(-1, nxt[..., None])[..., 0] - lf.logsumexp(dim=-1)).exp()
        n_tokens = torch.tensor(n_all, dtype=torch.int32, device=dev)
        n_frames = torch.tensor(frames, dtype=torch.int32, device=dev)
        path_ld = L + ctx
        path_text = torch.zeros((n, path_ld), dtype=torch.int32, device=dev)
        path_time = torch.zeros((n, path_ld), dtype=torch.int32, device=dev)
        path_len = torch.zeros(n, dtype=torch.int32, device=dev)
        matrix = torch.zeros((n, L, ctx), dtype=torch.float32, device=dev) if self.keep_alignment_matrix else None
        ws = torch.empty(max(256, lib.wm_align_workspace_bytes(n, len(heads), L, ctx)), dtype=torch.uint8, device=dev)
        io = native.WmAlignIO()
        io.engine = sess.engine.handle
        io.batch, io.n_text_head, io.n_audio_ctx = n, cfg['num_heads'], ctx
        io.q_tape, io.capacity = tape.data_ptr(), L
        cross_arr = native.ptr_array(cross)
        io.cross, io.n_layers = C.cast(cross_arr, C.POINTER(C.c_void_p)), cfg['num_layers']
        io.heads, io.n_heads = C.cast(heads_arr, C.POINTER(C.c_int32)), len(heads)
        io.n_tokens, io.n_frames = n_tokens.data_ptr(), n_frames.data_ptr()
        io.n_prefix, io.filter_width, io.cap_tokens = n_prefix, timing.MEDIAN_FILTER_WIDTH, L
        io.matrix, io.ld = (matrix.data_ptr(), ctx) if matrix is not None else (None, 0)
        io.path_text, io.path_time, io.path_len = path_text.data_ptr(), path_time.data_ptr(), path_len.data_ptr()
        io.workspace, io.workspace_bytes = ws.data_ptr(), ws.numel()
        native.check(lib.wm_align(C.byref(io), stream), "wm_align")
        lens = path_len.cpu().tolist()          # (synchronises: the workspace and the tape stay alive until here)
        pt, pf, probs = path_text.cpu().numpy(), path_time.cpu().numpy(), probs.cpu()
        self.last_alignment = dict(path_text=pt, path_time=pf, path_len=lens, n_tokens=n_all, n_frames=frames,
                                   matrix=matrix.cpu() if matrix is not None else None, token_probs=probs)
        out = []
        for b, (text, _) in enumerate(forced):
            if not text or lens[b] == 0:
                out.append([])
                continue
            words, word_tokens = self._split_words(text + [eot], languages[b])
            out.append(timing.words_from_path(pt[b, :lens[b]], pf[b, :lens[b]], words, word_tokens,
                                              probs[b, n_prefix: n_prefix + len(text)].tolist(), CHUNK_LENGTH / ctx))
        return out

    # ---- post-processing -------------------------------------------------------------------------------
    def _call_decoder(self, temperature: Optional[float]):
        """The decoder of a call at `temperature` (default: the options') and the candidates per utterance it ranks: the instance's
        own, or -- `fallback_best_of` above temperature 0 -- a sampler over the first fallback_best_of rows (`candidate_mode`)."""
        t = float(self.options.temperature if temperature is None else temperature)
        mode, n_cand = candidate_mode(self.options, self.fallback_best_of, t)
        if self.beam and mode == "sample":
            return GreedyDecoder(t, self.tokenizer.eot), n_cand
        return self.decoder, self.n_group

    def compression_ratio(self, text) -> float:
        text_bytes = text.encode("utf-8")
        return len(text_bytes) / len(zlib.compress(text_bytes))

    def post_process(self, tokens, sum_logprobs, no_speech_probs, audio_features, languages, temperature: Optional[float] = None):
        """Slice, rank, detokenise (W/decoding.py:827-878); n_audio comes from the batch, not the config.  `temperature`: what
        the results say they were decoded at (main_loop's per-call temperature; default: the options')."""
        if audio_features.shape[0] == len(no_speech_probs):          # already one row per candidate (the reference's convention)
            audio_features = audio_features[:: self.n_group]
        no_speech_probs = no_speech_probs[:: self.n_group]
        n_audio = audio_features.shape[0]
        assert n_audio == len(no_speech_probs)
        tokens = tokens.reshape(n_audio, self.n_group, -1)
        sum_logprobs = sum_logprobs.reshape(n_audio, self.n_group)
        decoder, n_cand = self._call_decoder(temperature)
        if n_cand < self.n_group:       # a sampling call of a beam instance: the closed rows (sum 0: they would win) never reach the ranker
            tokens, sum_logprobs = tokens[:, :n_cand], sum_logprobs[:, :n_cand]
        tokens, sum_logprobs = decoder.finalize(tokens, sum_logprobs)
        eot = self.tokenizer.eot
        tokens = [[t[self.sample_begin: (t == eot).nonzero()[0, 0]] for t in s] for s in tokens]
        selected = self.sequence_ranker.rank(tokens, sum_logprobs)
        tokens = [t[i].tolist() for i, t in zip(selected, tokens)]
        texts = [self.tokenizer.decode(t).strip() for t in tokens]
        sum_logprobs = [lp[i] for i, lp in zip(selected, sum_logprobs)]
        avg_logprobs = [lp / (len(t) + 1) for t, lp in zip(tokens, sum_logprobs)]
        fields = (texts, languages, tokens, audio_features, avg_logprobs, no_speech_probs)
        if len(set(map(len, fields))) != 1:
            raise RuntimeError(f"inconsistent result lengths: {list(map(len, fields))}")
        return [
            DecodingResult(audio_features=features, language=language, tokens=toks, text=text, avg_logprob=avg,
                           no_speech_prob=nsp, temperature=self.options.temperature if temperature is None else float(temperature),
                           compression_ratio=self.compression_ratio(text))
            for text, language, toks, features, avg, nsp in zip(*fields)
        ]
