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
  `main_loop` -- only when one of them is on;
* `hotwords` / `sequence_bias` (contextual biasing / Hugging Face; biasing.py states the contract and builds the table): `SequenceBias`
  directly behind the two repetition filters of the literal loops, wm_sequence_bias (csrc/bias.hip) behind wm_repeat_controls in the
  token step of `main_loop` -- only on an instance built with a bias; `set_bias` rewrites the table between calls;
* `top_k` / `top_p` / `min_p` (Hugging Face / CTranslate2; truncation.py states the contract): above temperature 0 the draw is restricted to
  a kept set -- `GreedyDecoder` masks its Categorical in the literal loops, wm_sample_step (csrc/truncate.hip) takes the place of
  wm_greedy_step in the token step of `main_loop`, only for calls at temperature > 0 on an instance with one of them on.  At
  temperature 0 and under beam search they are inert;
* `draft_engine_dir` / `draft_tokens` select speculative decoding (speculative.py states the contract, speculative_loop.py holds the loop):
  a draft engine proposes, one pass of this engine verifies, wm_verify_step (csrc/speculative.hip) keeps this engine's own tokens.

This module holds the options, the results and `WhisperDecoding`'s construction and call contract (start rows, prompts, post_process).
host_decoding.py holds the literal loops and the host filter / decoder classes and imports neither `native` nor `ctypes`;
device_loop.py holds the device loop and the device language pass; word_align.py holds the device word timestamps and the forced pass
that forced alignment shares.  Their public names are re-exported here.
"""
from __future__ import annotations

import json
import weakref
import zlib
from collections import OrderedDict
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

import biasing
import repetition
import truncation
from build import get_engine_name
from device_loop import (DeviceLoop, call_key, fork, groups_run_alone, join, language_key, partition_key,  # noqa: F401 (re-exported)
                         prefill_key, step_key, steps_side_by_side)
from host_decoding import (BEAM_MAX, BEAM_POOL_MAX, CHUNK_LENGTH, ApplyTimestampRules, BeamSearchDecoder,  # noqa: F401 (re-exported)
                           GreedyDecoder, HostLoops, LogitFilter, MaximumLikelihoodRanker, NoRepeatNGram, RepetitionPenalty,
                           SequenceBias, SuppressBlank, SuppressTokens)
from session import Session
from speculative_loop import SpeculativeLoop
from tokenizer import Tokenizer, layout_from_vocab
from word_align import WordAlign


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
    # the in-loop bias on vocabulary (biasing.py states the contract): one table per instance, matched against the tokens a row has
    # SAMPLED, applied behind the repetition controls and in front of Whisper's own rules; one bias per token, never a sum
    hotwords: Optional[Tuple[Union[str, Tuple[int, ...]], ...]] = None      # phrases boosted at every position: strings and / or token tuples
    hotword_bias: float = 3.0           # added to the token that continues a hotword (a parameter, not a measurement)
    hotword_start_bias: float = 1.5     # added to the first token of a hotword, at every step
    sequence_bias: Optional[Tuple[Tuple[Tuple[int, ...], float], ...]] = None   # ((token tuple, bias), ...): the token that completes a sequence
    # truncated sampling (truncation.py states the contract): which tokens a draw at temperature > 0 may take, decided on the distribution
    # AFTER Whisper's own rules; the booked log-probability stays that of the untruncated distribution.  Inert at temperature 0 / beam search
    top_k: int = 0                      # >= 0; only the k most likely tokens (ties at the k-th value are kept); 0 = off
    top_p: float = 1.0                  # (0, 1]; the smallest set of most likely tokens whose mass reaches p; 1.0 = off
    min_p: float = 0.0                  # [0, 1); tokens less likely than min_p times the most likely one are dropped; 0.0 = off


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
    biasing.check_options(options.hotwords, options.hotword_bias, options.hotword_start_bias, options.sequence_bias)
    truncation.check_options(options.top_k, options.top_p, options.min_p)


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


class WhisperDecoding(HostLoops, DeviceLoop, WordAlign, SpeculativeLoop):
    def __init__(self, engine_dir, only_torch: bool = False, vocab_path: Optional[str] = None,
                 options: Optional[DecodingOptions] = None, row_prompts: bool = False, shared_cross_kv: bool = False,
                 fallback_best_of: Optional[int] = None, block_prefill: bool = False, draft_engine_dir=None, draft_tokens: int = 3):
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
        no row count was found where it is not lower.  A start block of up to 4 tokens never takes it.
        `draft_engine_dir` (opt-in): speculative decoding (speculative.py states the contract).  A second decoder
        over the engines of that directory -- a model with the same encoder output, context and vocabulary and fewer decoder layers:
        distil-large-v3 or large-v3-turbo beside large-v3 -- proposes `draft_tokens` (1 .. 3) tokens per round under Whisper's rules, ONE
        wm_decoder_step of this instance's engine over the last token and the proposals verifies them, and wm_verify_step keeps the
        tokens this engine would have chosen itself: 1 to draft_tokens + 1 per pass over the weights.  `main_loop` at temperature 0
        then decodes the rows one after another (a latency mode for one long file, not a throughput mode); calls at temperature > 0
        take the ordinary loop.  The results are this engine's; `speculative_stats` holds the rounds, proposals, accepted proposals
        and sampled tokens per row of the last call.  Not with beam_size / best_of / fallback_best_of, row_prompts, shared_cross_kv,
        cu_partition, the repetition controls or hotwords / sequence_bias.  An instance without a draft launches what it always did."""
        engine_dir = Path(engine_dir)
        self.decoder_config = None
        self.cross_attn_config = None
        self.get_config(engine_dir)
        self.only_torch = only_torch
        if not only_torch:
            self.decoder_session, self.cross_attn_session = self.get_session(engine_dir)
        self.vocab_path = vocab_path
        # the ids of every special come from the vocabulary size: 99 languages up to large-v2 (51864 / 51865 tokens), 100 from
        # large-v3 on (51866: <|yue|>, every special behind the language block one id higher); any other real size is refused
        multilingual, self.num_languages = layout_from_vocab(self.decoder_config.get('vocab_size', 51865))
        self.tokenizer = self.get_tokenizer(multilingual, 'en', 'transcribe')
        self.is_multilingual = multilingual

        self.options = options or DecodingOptions()
        if multilingual and self.options.language is not None:       # a language this vocabulary has no token for (yue at 99) is refused here
            Tokenizer._defaults(True, self.options.language, None, self.num_languages)
        check_decoding_options(self.options)
        check_candidate_options(self.options, bool(shared_cross_kv), fallback_best_of)
        self.shared_cross_kv = bool(shared_cross_kv)
        self.fallback_best_of = None if fallback_best_of is None else int(fallback_best_of)
        self.n_group = self.options.beam_size or self.options.best_of or 1
        self._init_start_sequence(bool(row_prompts))
        self.use_int8_kv_cache = self.decoder_config['use_int8_kv_cache']
        self.use_int8_cross_kv = bool(self.decoder_config.get('use_int8_cross_kv', False))     # opt-in, beyond the reference
        self.block_prefill = bool(block_prefill)
        if self.block_prefill and self.use_int8_cross_kv:
            raise ValueError("block_prefill: engines with int8 cross K/V are not supported (wm_decoder_prefill reads fp16 cross K/V)")

        pe = np.load(engine_dir / 'positional_embedding.npy')
        self.positional_embedding = torch.tensor(pe)
        if not only_torch:
            self.positional_embedding = self.positional_embedding.to('cuda').type(torch.float16).contiguous()
        self._init_decoder()
        self._init_schedule()
        self._init_draft(draft_engine_dir, draft_tokens, bool(row_prompts), fallback_best_of)
        WhisperDecoding._instances.add(self)      # (weak: a give-up of a one-launch step drops the graphs of EVERY instance, _chain_gave_up)

    _chain_warned = False                 # the give-up warning of the device loop (_chain_gave_up): once per process, re-armed here
    _instances = weakref.WeakSet()

    def _init_start_sequence(self, row_prompts: bool) -> None:
        """The start sequence and the prompt layout: `initial_tokens`, `sot_index`, `sample_begin`, `sample_len` and the start rows."""
        n_ctx = self.decoder_config['num_text_ctx']
        self.sot_sequence = self.tokenizer.sot_sequence
        self.initial_tokens = tuple(list(self.sot_sequence))
        self.sot_index = self.initial_tokens.index(self.tokenizer.sot)
        self.sample_len: int = self.options.sample_len or n_ctx // 2
        self.row_prompts = row_prompts
        self._prompts = None              # set_prompts: one token list per utterance of the next main_loop calls
        self._row_starts = None           # _initial_token_rows: where every row of the call begins (row_prompts)
        if self.options.prompt or self.options.prefix:
            if row_prompts:
                raise ValueError("row_prompts: the prompt is per row (set_prompts); options.prompt / options.prefix are not supported with it")
            # the reference carries _get_initial_tokens (W/decoding.py:485-513) but never calls it (its options are the
            # defaults); with caller-supplied options the start sequence is <|startofprev|> prompt <|sot|> .. prefix
            self.initial_tokens = self._get_initial_tokens()
            self.sot_index = self.initial_tokens.index(self.tokenizer.sot)
        elif row_prompts:
            L0, self.sot_index, self.prompt_capacity = row_prompt_layout(n_ctx, self.sot_sequence, self.tokenizer.sot)
            self.initial_tokens = tuple(right_aligned_rows([()], self.sot_sequence, self.tokenizer.sot_prev, n_ctx)[0][0])
            self.sample_len = min(self.sample_len, n_ctx - L0)
        self.initial_token_length = self.sample_begin = len(self.initial_tokens)
        self.tokens = self._start_rows(self.decoder_config['num_audio'])

    def _init_decoder(self) -> None:
        """The logit filters, the ranker and the decoder of the literal loops (the device loop reads its rules off them)."""
        # repetition penalty / no-repeat n-grams (repetition.py): per instance, first in the filter list of the literal loops and one
        # launch in front of the token step of the device loop (_Group._token_step) -- with the defaults neither exists
        self.repeat_controls_on = repetition.controls_on(self.options.repetition_penalty, self.options.no_repeat_ngram_size)
        self.logit_filters = []
        if self.options.repetition_penalty != 1.0:
            self.logit_filters.append(RepetitionPenalty(self.options.repetition_penalty, self.tokenizer.eot, self.sample_begin))
        if self.options.no_repeat_ngram_size != 0:
            self.logit_filters.append(NoRepeatNGram(self.options.no_repeat_ngram_size, self.tokenizer.eot, self.sample_begin))
        # hotwords / sequence bias (biasing.py): one table per instance, built once; directly behind the repetition filters of the literal
        # loops and one launch behind wm_repeat_controls in the device loop (_Group._token_step) -- with the defaults neither exists
        self.bias_on = biasing.bias_on(self.options.hotwords, self.options.sequence_bias)
        self.bias_table = self._build_bias_table(self.options.hotwords, self.options.sequence_bias) if self.bias_on else None
        self._bias_dev = None             # (items, pool, count): device buffers of fixed capacity, allocated by the first device-loop call
        if self.bias_on:
            self.logit_filters.append(SequenceBias(self.bias_table, self.tokenizer.eot, self.sample_begin))
        # top-k / top-p / min-p (truncation.py): no filter -- the kept set is decided AFTER the rules, inside the sampler: GreedyDecoder masks
        # its draw in the literal loops, wm_sample_step takes wm_greedy_step's place in the device loop (_Group._token_step) for calls
        # at temperature > 0 -- with the defaults neither changes
        self.truncation_on = truncation.truncation_on(self.options.top_k, self.options.top_p, self.options.min_p)
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
            self.decoder = GreedyDecoder(self.options.temperature, self.tokenizer.eot, self._truncation())
        self.beam = self.options.beam_size is not None     # (beam_size = 1 is beam search too: one beam, a pool of finished candidates)

    def _init_schedule(self) -> None:
        """The state of the loops and the schedule knobs of the device loop (bench.py and the tests set them on the instance)."""
        self.kv_cache = {}
        self.hooks = []
        self._cross_cache = None          # (key, list of cross K/V) from the last xa2cross_key_value
        self._lang_mask_cache = None      # (key, mask, language token ids) of the last _language_from_logits
        self._rep_cache = None            # (key, repeated features, features) of the last _candidate_rows
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
            return Tokenizer.from_vocab(path, multilingual, language, task, num_languages=self.num_languages)
        return Tokenizer.ids_only(multilingual, language, task, num_languages=self.num_languages)

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

    # ---- start rows, language tokens, prompts ---------------------------------------------------------
    def _start_rows(self, n: int, language_tokens=None) -> Tensor:
        """n rows of `initial_tokens` [n, L0] on the host, optionally with these language tokens (one per row, or one for all) behind
        <|startoftranscript|>: what `self.tokens` holds."""
        rows = torch.tensor([self.initial_tokens]).repeat(n, 1)
        if language_tokens is not None:
            rows[:, self.sot_index + 1] = language_tokens
        return rows

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
        self.tokens = self._start_rows(len(language_tokens), torch.tensor(language_tokens, dtype=torch.long))
        if self.draft is not None:        # (the draft reads the main token rows; its own start rows follow for its literal loops)
            self.draft.set_language_tokens(language_tokens)

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

    # ---- hotwords / sequence bias ------------------------------------------------------------------------
    def _build_bias_table(self, hotwords, sequence_bias, hotword_bias=None, hotword_start_bias=None) -> "biasing.Table":
        o = self.options
        return biasing.build_table(hotwords, sequence_bias, o.hotword_bias if hotword_bias is None else hotword_bias,
                                   o.hotword_start_bias if hotword_start_bias is None else hotword_start_bias,
                                   eot=self.tokenizer.eot, tokenizer=self.tokenizer)

    def set_bias(self, hotwords=None, sequence_bias=None, hotword_bias: Optional[float] = None,
                 hotword_start_bias: Optional[float] = None) -> None:
        """Another table for the next main_loop calls -- a per-file vocabulary -- on an instance that was BUILT with a bias (its token
        steps and captured graphs contain the launch; an instance built without one has no launch to feed and refuses).  The table
        replaces the old one whole (neither option given: an empty table, nothing is biased); the biases default to the options'.  The
        device buffers have a fixed capacity and are rewritten in place on the current stream: no graph is rebuilt, a replayed step
        reads the new items and their number from device memory.  Call it between main_loop calls."""
        if not self.bias_on:
            raise ValueError("set_bias: needs an instance built with hotwords / sequence_bias (the token step of any other has no bias launch)")
        table = self._build_bias_table(hotwords, sequence_bias, hotword_bias, hotword_start_bias)
        self.bias_table = table
        for f in self.logit_filters:
            if isinstance(f, SequenceBias):
                f.table = table
        if self._bias_dev is not None:
            self._upload_bias(self._bias_dev[0].device)

    def _upload_bias(self, device):
        """The table in the instance's device buffers (allocated once, at the table's bounds), on the current stream."""
        if self._bias_dev is None:
            self._bias_dev = (torch.zeros(4 * biasing.MAX_ITEMS, dtype=torch.int32, device=device),
                              torch.zeros(biasing.MAX_POOL, dtype=torch.int32, device=device),
                              torch.zeros(1, dtype=torch.int32, device=device))
        items, pool, count = self._bias_dev
        t = self.bias_table
        if len(t):
            items[:4 * len(t)].copy_(torch.from_numpy(t.packed.view(np.int32).reshape(-1).copy()))
        if t.pool.size:
            pool[:t.pool.size].copy_(torch.from_numpy(t.pool.copy()))
        count.copy_(torch.tensor([len(t)], dtype=torch.int32))          # (items beyond it are stale and never read)
        return self._bias_dev

    def _initial_token_rows(self, n_audio, device):
        tokens = self.tokens if self.tokens.shape[0] == n_audio else self._start_rows(n_audio)
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

    # ---- post-processing -------------------------------------------------------------------------------
    def _call_decoder(self, temperature: Optional[float]):
        """The decoder of a call at `temperature` (default: the options') and the candidates per utterance it ranks: the instance's
        own, or -- `fallback_best_of` above temperature 0 -- a sampler over the first fallback_best_of rows (`candidate_mode`)."""
        t = float(self.options.temperature if temperature is None else temperature)
        mode, n_cand = candidate_mode(self.options, self.fallback_best_of, t)
        if self.beam and mode == "sample":
            return GreedyDecoder(t, self.tokenizer.eot, self._truncation()), n_cand
        return self.decoder, self.n_group

    def _truncation(self) -> Optional[Tuple[int, float, float]]:
        """(top_k, top_p, min_p) of an instance with one of them on, else None: what the samplers of the literal loops take."""
        o = self.options
        return (int(o.top_k), float(o.top_p), float(o.min_p)) if self.truncation_on else None

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
