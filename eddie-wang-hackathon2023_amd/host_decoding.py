"""The literal loops of WhisperDecoding: the statement of the decoding contract that the goldens test against.

The host-side filter classes, `GreedyDecoder` / `BeamSearchDecoder` and the ranker, and `HostLoops`, the part of `WhisperDecoding`
(decoding.py assembles the class) that decodes through them: the reference's by-name `decode()` protocol, `main_loop_reference`, the
`torch_*` paths on the PyTorch model and what word timestamps mean (`torch_word_timestamps`).  Nothing here needs the HIP library:
this module imports neither `native` nor `ctypes`; the device loop (device_loop.py) is tested against it.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor

import biasing
import truncation
import timing
from session import TensorInfo, str_dtype_to_trt, trt_dtype_to_torch, logger
from tokenizer import Tokenizer

CHUNK_LENGTH = 30


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


class SequenceBias(LogitFilter):
    """Hotwords and sequence bias of biasing.py in torch: per row and text token, the matching item of the table with the greatest
    prefix adds its bias -- once, in fp32, rounded to fp16; biases are never summed.  Placed directly behind the two repetition
    filters.  The match and the sum run on the host whatever device the logits live on, as RepetitionPenalty's arithmetic does.
    `table` (a biasing.Table) may be replaced between calls (WhisperDecoding.set_bias)."""

    def __init__(self, table, eot: int, sample_begin: int):
        self.table, self.eot, self.sample_begin = table, eot, sample_begin

    def apply(self, logits: Tensor, tokens: Tensor):
        rows, ids, bias = [], [], []
        for b, h in enumerate(tokens[:, self.sample_begin:].cpu().tolist()):
            for t, v in biasing.winners(self.table.items, h).items():
                if 0 <= t < self.eot:
                    rows.append(b), ids.append(t), bias.append(v)
        if not rows:
            return
        x = logits[rows, ids].float().cpu()                      # one winner per (row, token): every logit is read and written once
        y = (x + torch.tensor(bias, dtype=torch.float32)).to(logits.dtype)
        logits[rows, ids] = y.to(logits.device)


class GreedyDecoder:
    """`kept` (optional, (top_k, top_p, min_p) with one of them on): above temperature 0 the draw is restricted to the kept set of
    truncation.py, decided on the logits as the filters left them; the log-probability booked stays that of the unmasked logits."""

    def __init__(self, temperature: float, eot: int, kept: Optional[Tuple[int, float, float]] = None):
        self.temperature, self.eot, self.kept = temperature, eot, kept

    def update(self, tokens: Tensor, logits: Tensor, sum_logprobs: Tensor) -> Tuple[Tensor, bool]:
        if self.temperature == 0:
            next_tokens = logits.argmax(dim=-1)
        elif self.kept is None:
            next_tokens = torch.distributions.Categorical(logits=logits / self.temperature).sample()
        else:
            keep = truncation.keep_mask(logits.detach().float().cpu().numpy(), self.temperature, *self.kept)
            masked = (logits / self.temperature).masked_fill(~torch.from_numpy(keep).to(logits.device), -np.inf)
            next_tokens = torch.distributions.Categorical(logits=masked).sample()
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


class HostLoops:
    """The literal loops of WhisperDecoding (a mixin: decoding.py states the attributes its methods read)."""

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
        cache = self._lang_mask_cache
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

    def _language_rows(self, audio_features, keep_stamp: bool = False):
        """What every language pass begins with: (rows, single, answer).  `rows` is None where there is nothing to detect -- an
        English-only vocabulary, a language named in the options (unless the task is "lang_id") -- and `answer` is what the pass then
        returns; else the features as [n_audio, n_audio_ctx, C], `single` when they came without the batch axis."""
        if not self.is_multilingual:
            return None, False, (['en'] * audio_features.shape[0], None)      # English-only vocabulary: no language tokens
        if self.options.language is not None and self.options.task != "lang_id":
            return None, False, ([self.options.language] * audio_features.shape[0], None)
        single = audio_features.ndim == 2
        if single:
            gen = getattr(audio_features, 'wm_generation', None) if keep_stamp else None
            audio_features = audio_features.unsqueeze(0)
            if gen is not None:          # the view is the same encoder output: it keeps the stamp (_features_key; else the cross K/V
                audio_features.wm_generation = gen      # of one clip would be projected twice, once per view)
        return audio_features, single, None

    def _language_result(self, logits, single):
        """What every language pass ends with, from the logits [n_audio, n_vocab] of the <|sot|> row: (languages, probabilities), and --
        unless the options name the language -- the start rows of the next main_loop call, each with its language token."""
        n_audio = logits.shape[0]
        language_tokens, language_probs, languages = self._language_from_logits(logits, n_audio, single)
        if self.options.language is None:
            self.tokens = self._start_rows(n_audio, language_tokens.cpu())        # write language tokens
        return languages, language_probs

    def detect_language_reference(self, audio_features):
        """The reference's language-ID pass literally (W/decoding.py:703-741): cross K/V engine, one
        `decode()` of the single <|sot|> token through the by-name protocol."""
        audio_features, single, answer = self._language_rows(audio_features)
        if audio_features is None:
            return answer
        x = torch.tensor([[self.tokenizer.sot]] * audio_features.shape[0]).to(audio_features.device)    # [n_audio, 1]
        cross = self.xa2cross_key_value(audio_features)
        logits, _ = self.decode(x, cross)
        return self._language_result(logits[:, 0].float(), single)

    def torch_detect_language(self, model, audio_features):
        """PyTorch path (W/decoding.py:661-701): `model.logits(tokens, audio_features)`."""
        audio_features, single, answer = self._language_rows(audio_features)
        if audio_features is None and not self.is_multilingual:
            return answer
        if audio_features is not None:
            with torch.no_grad():
                x = torch.tensor([[self.tokenizer.sot]] * audio_features.shape[0]).to(audio_features.device)
                answer = self._language_result(model.logits(x, audio_features)[:, 0], single)
        for hook in self.hooks:
            hook.remove()
        self.kv_cache, self.hooks = {}, []
        return answer

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
