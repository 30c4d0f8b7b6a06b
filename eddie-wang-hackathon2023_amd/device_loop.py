"""The device loop of WhisperDecoding: `main_loop` and the device language pass.

The schedule functions and graph keys, `_Call` / `_Group`, and `DeviceLoop`, the part of `WhisperDecoding` (decoding.py assembles the
class) that drives the HIP library: batch state, group streams, graph capture and replay, the give-up handling, the token-step IO
structs, `_run_groups` and the CU-partitioned loop.  Everything here is tested against the literal loops of host_decoding.py.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

import native
import truncation
from host_decoding import SuppressTokens
from session import logger


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
        # per-row completion: the group's rows still decoding and, for candidates that share a cross K/V row, its utterances with a live row
        self.live_groups = dec._all_live(st, (n_micro, slot, 'utterances'), (hi - lo) // G) if call.use_live and G > 1 else None
        self.logits, self.tokens, self.done = st['logits'][lo:hi], st['tokens'][lo:hi], st['done'][lo:hi]
        self.live = dec._all_live(st, (n_micro, slot), hi - lo) if call.use_live else None
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
        """What follows a group's decoder launch: the repetition controls where one is on, the hotword / sequence bias of an instance
        built with one, then the fused greedy step -- the truncated sampling step in its place for a call at temperature > 0 on an
        instance with top_k / top_p / min_p on -- or the beam step and the cache reorder."""
        dec, call = self.dec, self.call
        if dec.repeat_controls_on:
            dec._repeat_controls(call.st, self.lo, self.hi, logits_ptr, row_stride, cur_len, self.sm, n_past_dev=n_past_dev)
        if dec.bias_on:
            dec._sequence_bias(call.st, self.lo, self.hi, logits_ptr, row_stride, cur_len, self.sm, n_past_dev=n_past_dev)
        if call.beam:
            dec._beam(call.st, self.lo, self.hi, logits_ptr, row_stride, cur_len, self.sm, self.kv_table, call.ignore_eot, n_past_dev=n_past_dev)
        elif call.temperature > 0 and dec.truncation_on:
            dec._sample(call.st, self.lo, self.hi, logits_ptr, row_stride, cur_len, self.sm, call.temperature, n_past_dev=n_past_dev)
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


class DeviceLoop:
    """The device loop of WhisperDecoding (a mixin: decoding.py states the attributes its methods read)."""

    # ---- language detection ---------------------------------------------------------------------------
    def detect_language(self, audio_features, _retry: bool = False):
        """Language-ID pass, fast path: same arithmetic as detect_language_reference, but the cross
        K/V land in the persistent buffers main_loop re-uses (the reference computes them twice,
        SURVEY F6) and the one-token decoder call runs per utterance group on its stream."""
        rows, single, answer = self._language_rows(audio_features, keep_stamp=True)
        if rows is None:
            return answer
        every = 1
        if self._cross_group() > 1 and rows.is_cuda:
            # shared cross K/V: the pass runs over the n_audio utterances themselves (group 1), on the cross K/V and the first
            # n_audio cache rows of the buffer set main_loop will use -- nothing is repeated, nothing projected twice
            self._require_device_loop("detect_language")
        elif self.n_group > 1 and self.device_sampling and rows.is_cuda:
            # best_of / beam candidates: main_loop decodes n_audio x n_group rows.  The state keeps ONE buffer set at a time, so a
            # language pass over n_audio rows would free and re-allocate the caches, the cross K/V buffers and the graphs on every
            # clip.  The pass runs over the candidates' rows instead -- the SAME repeated tensor main_loop will use
            # (_candidate_rows): one buffer set, the cross K/V computed once for both calls -- and reads every n_group-th row
            rows, every = self._candidate_rows(rows), self.n_group
        logits, one_row = self._detect_language_rows(rows, every)
        out = self._language_result(logits, single)                # (brings the logits to the host: the pass has finished)
        if one_row and not _retry and self._chain_gave_up("language pass"):
            return self.detect_language(audio_features, True)
        return out

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
        c = self._rep_cache
        if key is not None and c is not None and c[0] == key:
            return c[1]
        rep = stamp_generation(audio_features.repeat_interleave(self.n_group, dim=0))
        self._rep_cache = (key, rep, audio_features)       # (the original kept alive: its pointer is part of the key)
        return rep

    def _detect_language_rows(self, audio_features, every: int = 1):
        """The pass itself over the rows of `audio_features` [n, n_audio_ctx, C] (detect_language): the fp32 logits of the <|sot|> row
        of every `every`-th row, and whether a group of it may have run as one launch (the caller looks at the give-up word)."""
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
        return st['lang_logits'][::every, 0].float(), one_row

    # ---- fast path ----------------------------------------------------------------------------------------
    def _device_suppress_lists(self):
        """(suppress, blank): the two id lists the token-step kernels take -- SuppressTokens' list plus <|notimestamps|> (the host loops
        mask it in ApplyTimestampRules), and SuppressBlank's.  Every id is the instance's tokenizer's: 50363 for <|notimestamps|> with 99
        languages, 50364 with 100."""
        tk = self.tokenizer
        suppress = []
        for f in self.logit_filters:
            if isinstance(f, SuppressTokens):
                suppress += list(f.suppress_tokens)
        if not self.options.without_timestamps and tk.no_timestamps is not None:
            suppress.append(tk.no_timestamps)
        blank = list(tk.blank_tokens()) + [tk.eot] if self.options.suppress_blank else []
        return sorted(set(suppress)), blank

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
            self._check_state_fits(n_batch, device)
        suppress, blank = self._device_suppress_lists()
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
            st.update(self._beam_state(n_batch, device))
        self._state[n_batch] = st
        return st

    def _check_state_fits(self, n_batch, device) -> None:
        # the batch ceiling is a property of the free memory, said up front instead of an allocator error half way through
        per_row = self.state_bytes_per_utterance()
        free, _ = torch.cuda.mem_get_info(device)
        if n_batch * per_row > free:
            raise RuntimeError(
                f"WhisperDecoding: a batch of {n_batch} utterances needs {n_batch * per_row / 2**30:.1f} GiB of decoder state "
                f"({per_row / 2**20:.1f} MiB per utterance: self-attention cache + cross-attention K/V of {self.decoder_config['num_layers']} layers), "
                f"{free / 2**30:.1f} GiB are free on {device}: at most {int(free // per_row)} utterances per batch fit "
                f"(another WhisperDecoding's buffer set in this process counts against it)")

    def _beam_state(self, n_batch, device) -> dict:
        """The beam step's outputs: parents, the pool of finished candidates per utterance, the proposals between its two launches."""
        K, MC, cap = self.decoder.beam_size, self.decoder.max_candidates, self.decoder_config['num_text_ctx']
        n_audio = n_batch // K
        return dict(
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
        if unit is None:
            unit = self._group_unit()
        n_units = n_batch // unit
        n_micro = max(1, min(n_micro, n_units))
        return n_micro, [(g * n_units // n_micro * unit, (g + 1) * n_units // n_micro * unit) for g in range(n_micro)]

    def _group_unit(self) -> int:
        """The rows the groups are cut in multiples of.  The beams of an utterance stay in one group (the beam step and the cache reorder
        work per utterance): cut in whole utterances (so do the candidates that share a cross K/V row: the launch reads row b / n_group
        of the group's slice)."""
        return self.n_group if (self.beam or self.shared_cross_kv) else 1

    def balanced_order(self, n_batch: int) -> List[int]:
        """For a batch whose rows are sorted by expected decode length: the permutation that deals them over the
        utterance groups (contiguous slices of the batch, `_groups`) like cards, so that every group holds short and long
        rows alike.  All groups then shrink together as rows finish -- their K/V streams and chains keep overlapping --
        instead of the group of the longest clips running on alone.  `batch[i] = sorted_batch[order[i]]`."""
        unit = self._group_unit()        # (beam search, shared cross K/V: the groups are cut over the clips' candidate rows, in whole clips)
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
        for inst in list(self._instances):
            for st in inst._state.values():
                st['graphs'].clear()
        if foreign:
            logger.error("whisper_mi355: a one-launch decode step issued BEFORE this call (%s) gave up waiting for its workgroups and nobody "
                         "looked: whatever that earlier call returned on this device is INVALID (decode it again).  Acknowledged here; the "
                         "device takes a launch per kernel from now on (wm_set_decode_chain re-arms the one-launch step)", where)
        elif not self._chain_warned:
            # (one warning per process: the word lives in the body of WhisperDecoding, where it is re-armed, whatever class `self` is of)
            next(c for c in type(self).__mro__ if '_chain_warned' in vars(c))._chain_warned = True
            logger.warning("whisper_mi355: a one-launch decode step gave up waiting for its workgroups (%s; the GPU was not free to hold them "
                           "together): decoding again with a launch per kernel, which this device uses from now on "
                           "(wm_set_decode_chain re-arms the one-launch step)", where)
        return True

    @staticmethod
    def _all_live(st, key, n):
        """A group's list of rows still decoding (int32 [1 + n]: count, indices relative to the group; key (n_micro, slot)) or of
        utterances with a live row (key (n_micro, slot, 'utterances'): candidates that share a cross K/V row), reset to "all of them";
        wm_step_finish / wm_step_finish_group rebuild the lists after every step from the `done` flags."""
        if key not in st['live']:
            st['live'][key] = torch.empty(1 + n, dtype=torch.int32, device=st['done'].device)
        live = st['live'][key]
        live[0] = n
        live[1:] = torch.arange(n, dtype=torch.int32, device=live.device)
        return live

    def _fill_rows(self, io, st, lo, hi, logits_ptr, row_stride, cur_len, n_past_dev) -> None:
        """The fields wm_greedy_io, wm_beam_io, wm_repeat_io and wm_bias_io share: where rows [lo, hi) of the batch state `st` are -- their logits,
        tokens and `done` flags -- and how long they are (`cur_len`, or the device step counter of a captured step)."""
        io.logits, io.row_stride = logits_ptr, row_stride
        io.batch, io.n_vocab = hi - lo, self.decoder_config['vocab_size']
        io.tokens, io.tokens_ld, io.cur_len = st['tokens'][lo:hi].data_ptr(), st['tokens'].shape[1], cur_len
        io.n_past_dev = n_past_dev.data_ptr() if n_past_dev is not None else None
        io.done = st['done'][lo:hi].data_ptr()

    def _fill_rules(self, io, st, lo, hi, logits_ptr, row_stride, cur_len, n_past_dev):
        """The fields wm_greedy_io and wm_beam_io share: the row fields (`_fill_rows`) and the logit rules."""
        tk = self.tokenizer
        self._fill_rows(io, st, lo, hi, logits_ptr, row_stride, cur_len, n_past_dev)
        io.sum_logprobs = st['sum_logprobs'][lo:hi].data_ptr()
        io.suppress, io.n_suppress = st['suppress'].data_ptr(), st['n_suppress']
        io.blank, io.n_blank = st['blank'].data_ptr(), st['n_blank']
        io.sample_begin, io.eot, io.timestamp_begin = self.sample_begin, tk.eot, tk.timestamp_begin
        io.max_initial_timestamp_index = -1 if self.max_initial_timestamp_index is None else self.max_initial_timestamp_index
        # 1: SuppressBlank + SuppressTokens + ApplyTimestampRules; 2: without_timestamps -- the reference then builds no timestamp
        # filter (W/decoding.py:337-346) and samples from the whole suppressed vocabulary
        io.apply_rules = 2 if self.options.without_timestamps else 1
        io.n_done = st['n_done'].data_ptr()
        io.row_limit = st['row_limit'][lo:hi].data_ptr()

    def _repeat_controls(self, st, lo, hi, logits_ptr, row_stride, cur_len, stream, n_past_dev=None):
        """Repetition penalty and no-repeat n-grams (wm_repeat_controls, csrc/repeat.hip) on the raw logits of rows [lo, hi) of the
        batch state `st`, before the token step: the same rows, tokens and flags as `_fill_rules` hands to it."""
        io = native.WmRepeatIO()
        self._fill_rows(io, st, lo, hi, logits_ptr, row_stride, cur_len, n_past_dev)
        io.sample_begin, io.eot = self.sample_begin, self.tokenizer.eot
        io.repetition_penalty, io.no_repeat_ngram_size = float(self.options.repetition_penalty), int(self.options.no_repeat_ngram_size)
        native.check(native.load_library().wm_repeat_controls(C.byref(io), stream), "wm_repeat_controls")

    def _sequence_bias(self, st, lo, hi, logits_ptr, row_stride, cur_len, stream, n_past_dev=None):
        """Hotwords / sequence bias (wm_sequence_bias, csrc/bias.hip) on the raw logits of rows [lo, hi) of the batch state `st`, behind
        the repetition controls and before the token step: the instance's table, its item count read on the device."""
        items, pool, count = self._bias_dev
        io = native.WmBiasIO()
        self._fill_rows(io, st, lo, hi, logits_ptr, row_stride, cur_len, n_past_dev)
        io.sample_begin, io.eot = self.sample_begin, self.tokenizer.eot
        io.items, io.pool, io.n_items_dev = items.data_ptr(), pool.data_ptr(), count.data_ptr()
        io.capacity, io.pool_capacity = items.numel() // 4, pool.numel()
        native.check(native.load_library().wm_sequence_bias(C.byref(io), stream), "wm_sequence_bias")

    def _greedy(self, st, lo, hi, logits_ptr, row_stride, cur_len, stream, n_past_dev=None, temperature=None):
        """Fused logit rules + arg-max + append for utterances [lo, hi) of the batch state `st`."""
        io = native.WmGreedyIO()
        self._fill_rules(io, st, lo, hi, logits_ptr, row_stride, cur_len, n_past_dev)
        # temperature > 0: the draw happens in the same kernel (Gumbel-max, counter-based generator keyed on the global row: lo + b);
        # the seed lives in device memory so that a replayed graph draws afresh in every main_loop call
        io.temperature = float(self.options.temperature if temperature is None else temperature)     # (a per-call temperature: main_loop)
        io.row0, io.seed_dev = lo, st['seed'].data_ptr()
        native.check(native.load_library().wm_greedy_step(C.byref(io), stream), "wm_greedy_step")

    def _sample(self, st, lo, hi, logits_ptr, row_stride, cur_len, stream, temperature, n_past_dev=None):
        """The token step with the draw restricted by top_k / top_p / min_p (wm_sample_step, csrc/truncate.hip) for rows [lo, hi) of the
        batch state `st`: `_greedy`'s fields and the scalars of truncation.params, baked into a captured step like the temperature."""
        io = native.WmSampleIO()
        self._fill_rules(io.g, st, lo, hi, logits_ptr, row_stride, cur_len, n_past_dev)
        io.g.temperature = float(temperature)
        io.g.row0, io.g.seed_dev = lo, st['seed'].data_ptr()
        c, p_q16, gap = truncation.params(temperature, self.options.top_p, self.options.min_p)
        io.top_k, io.exp2_scale, io.top_p_q16, io.min_p_gap = int(self.options.top_k), float(c), int(p_q16), float(gap)
        native.check(native.load_library().wm_sample_step(C.byref(io), stream), "wm_sample_step")

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
        decoder, n_cand = self._call_decoder(temp)
        beam = self.beam and decoder is self.decoder        # this call's decoder (fallback_best_of: samples above temperature 0)
        G = self._cross_group()
        self._check_device_call(audio_features, temp)
        if getattr(self, 'draft', None) is not None and temp == 0 and not ignore_eot:
            # speculative decoding (speculative_loop.py): row after row, the draft proposes and one pass of this engine verifies.
            # Calls above temperature 0 (the long-form ladder) and fixed-length benchmark loops take the ordinary loop below
            return self._speculative_loop(audio_features, row_limit=row_limit, _retry=_retry)
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
        if self.bias_on and self._bias_dev is None:
            self._upload_bias(dev)        # (the first device-loop call: on this stream, before the groups' streams fork from it)
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
        if self.bias_on:
            raise ValueError("hotwords / sequence_bias are not supported by the CU-partitioned schedule (cu_partition = True): "
                             "it has a loop of its own; use the default loop")
        if self.truncation_on:
            raise ValueError("top_k / top_p / min_p are not supported by the CU-partitioned schedule (cu_partition = True): "
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
                nsp_dev = self._no_speech_probs(st, main, streams)
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

    def _no_speech_probs(self, st, main, streams):
        """The no-speech probability of every row (on the device), read on `main` once the groups' first steps on `streams` have run.
        The token step has already written -inf into the LAST position's row only; the <|sot|> position (no-speech probability,
        W/decoding.py:803-807) is untouched."""
        join(main, streams)
        nsp_dev = st['logits'][:, self.sot_index].float().softmax(dim=-1)[:, self.tokenizer.no_speech]
        fork(main, streams)
        return nsp_dev

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
                    nsp_dev = self._no_speech_probs(st, main, light)
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
        return self._result_triple(st, tokens, nsp_dev)

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
        return self._result_triple(st, tokens, nsp_dev)

    @staticmethod
    def _result_triple(st, tokens, nsp_dev):
        """What a main loop returns: (tokens, sum_logprobs, no_speech_probs), the last NaN where the vocabulary has no <|nospeech|>."""
        no_speech_probs = nsp_dev.tolist() if nsp_dev is not None else [np.nan] * tokens.shape[0]
        return tokens, st['sum_logprobs'].clone(), no_speech_probs
