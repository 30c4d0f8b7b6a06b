"""The device loop of speculative decoding: a draft engine proposes, one pass of the main engine verifies (speculative.py states the
contract; csrc/speculative.hip, wm_verify_step).

`SpeculativeLoop` is the part of `WhisperDecoding` (decoding.py assembles the class) that an instance built with `draft_engine_dir`
adds: a second WhisperDecoding over the draft engines (`self.draft`: its own sessions, positional embedding, self-attention cache
and cross K/V -- computed from the SAME audio features, the distil recipe of a shared encoder) and `_speculative_loop`, which
`main_loop` takes at temperature 0.  Rows are decoded one after another, eagerly, with host-side n_past as `_Group.step(cur)` issues
them; per round one copy of (n_accept, done) comes back (per ROW there is one more look, at the flag the prefill's token step left).
The batch states of both engines are allocated for all rows of the call, as the ordinary loop allocates them: the cross K/V of every
row are projected in one call up front and the results are read off the main state as ever; only the stepping is row by row.  A
calibration session (`decoder_session.qkv_amax`) needs nothing special here: every call is eager and `make_decoder_io` hands the hook on.

The two engines share ONE token row (the main state's): the draft's greedy steps write their proposals into the slots the verify
pass reads, and the verify step overwrites them with the main engine's tokens, so the draft's next catch-up pass reads the history
as it stands.  Everything else of the draft (sums, flags, logits) lives in its own state and is never read back.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

import native
import speculative
from device_loop import _Call, _Group


class SpeculativeLoop:
    """A mixin of WhisperDecoding: decoding.py states the attributes its methods read."""

    def _init_draft(self, draft_engine_dir, draft_tokens, row_prompts: bool, fallback_best_of) -> None:
        """`self.draft`, `self.draft_tokens`, `self.speculative_stats`; the refusals of an instance with a draft."""
        self.draft = None
        self.draft_tokens = speculative.check_draft_tokens(draft_tokens)
        self.speculative_stats = None     # the last speculative call: rounds, proposals, accepted, tokens per row (and `trace`)
        self.speculative_trace = False    # keep every round's (T, proposals, n_accept) too: one more copy per round
        self._spec_bufs = None
        if draft_engine_dir is None:
            return
        if self.only_torch:
            raise ValueError("draft_engine_dir: needs the device loop (only_torch has no sessions)")
        speculative.check_draft(draft_tokens, self.options, row_prompts=row_prompts, shared_cross_kv=self.shared_cross_kv,
                                fallback_best_of=fallback_best_of)
        self.draft = type(self)(draft_engine_dir, vocab_path=self.vocab_path, options=self.options, block_prefill=self.block_prefill)
        speculative.check_draft(draft_tokens, self.options, main_dims=self.decoder_session.dims, draft_dims=self.draft.decoder_session.dims)

    def _spec_buffers(self, device):
        """What the rounds need beside the two batch states: the logits of a verify pass (4 positions) and of a draft pass (2), the
        (n_accept, done) pair that comes back, the verify step's workspace."""
        if self._spec_bufs is None or self._spec_bufs['pair'].device != device:
            V = self.decoder_config['vocab_size']
            n = speculative.MAX_PASS_TOKENS
            self._spec_bufs = dict(
                logits=torch.empty((1, n, V), dtype=torch.float16, device=device),
                draft_logits=torch.empty((1, 2, V), dtype=torch.float16, device=device),
                pair=torch.zeros(2, dtype=torch.int32, device=device),
                ws=torch.empty(max(8, native.load_library().wm_verify_workspace_bytes(1, n)), dtype=torch.uint8, device=device))
        return self._spec_bufs

    def _verify(self, st, r: int, logits, n_pos: int, cur: int, pair, ws, stream) -> None:
        """wm_verify_step for row r of the batch state `st`: the logits [1, n_pos, V] of one main pass, slots cur .. cur + n_pos - 1.
        n_accept lands in pair[0], the row's done flag in pair[1]."""
        V = self.decoder_config['vocab_size']
        io = native.WmVerifyIO()
        self._fill_rules(io.g, st, r, r + 1, logits.data_ptr(), n_pos * V, cur, None)
        io.g.done = pair[1:].data_ptr()
        io.g.temperature, io.g.row0, io.g.seed_dev = 0.0, r, None
        io.pos_stride, io.n_pos = V, n_pos
        io.n_accept, io.workspace = pair.data_ptr(), ws.data_ptr()
        native.check(native.load_library().wm_verify_step(C.byref(io), stream), "wm_verify_step")

    def _speculative_loop(self, audio_features, row_limit=None, _retry: bool = False):
        """main_loop at temperature 0 on an instance with a draft: the same return values, the main engine's."""
        draft, S = self.draft, speculative
        if self.cu_partition:
            raise ValueError("draft_engine_dir: the CU-partitioned schedule (cu_partition = True) is not supported")
        if not audio_features.is_cuda:
            raise ValueError("draft_engine_dir: speculative decoding needs the device loop (features on the GPU)")
        n_batch, dev = audio_features.shape[0], audio_features.device
        cfg = self.decoder_config
        cap, V = cfg['num_text_ctx'], cfg['vocab_size']
        tokens0 = self._initial_token_rows(n_batch, dev)
        L0 = tokens0.shape[1]
        st, dst = self._fast_state(n_batch, dev), draft._fast_state(n_batch, dev)
        one_row = self._may_run_alone([(0, 1)], 1, False, "found before the speculative loop", peek=not _retry)
        cross = self._reset_state(st, audio_features, tokens0, row_limit, 1, reseed=False)
        dcross = draft._cross_persistent(audio_features, dst)
        for name in ('sum_logprobs', 'n_done', 'done'):
            dst[name].zero_()
        dst['row_limit'].fill_(1 << 30)
        dview = dict(dst, tokens=st['tokens'])        # the draft's token steps read and write the main token rows
        bufs = self._spec_buffers(dev)
        mlogits, dlogits, pair, ws = bufs['logits'], bufs['draft_logits'], bufs['pair'], bufs['ws']
        main = torch.cuda.current_stream()
        sm, na = main.cuda_stream, bool(self.force_not_alone)

        def one_row_call(dec, state, crs):
            block = dec.block_prefill and L0 > 4
            return _Call(st=state, cross=crs, L0=L0, n_micro=1, use_live=False, not_alone=na, beam=False, ignore_eot=False,
                         temperature=0.0, bkey=(), use_graph=False, block=block, graph_prefill=False)
        call, dcall = one_row_call(self, st, cross), one_row_call(draft, dst, dcross)
        pos, dpos, sess, dsess = self.positional_embedding, draft.positional_embedding, self.decoder_session, draft.decoder_session
        keep_trace = bool(self.speculative_trace)
        stats = dict(rounds=[], proposals=[], accepted=[], tokens=[])
        if keep_trace:
            stats['trace'] = []
        cur_max = L0 + 1
        for r in range(n_batch):
            gr, dgr = _Group(self, call, 0, r, r + 1, main), _Group(draft, dcall, 0, r, r + 1, main)
            row = st['tokens'][r:r + 1]
            # both engines take the start block; the main engine's first token step is the ordinary one (wm_greedy_step)
            dgr._launch_prefill(L0, row[:, :L0], dgr.kv, dgr.logits, None, None)
            gr.prefill(L0)
            pair.zero_()
            done = bool(st['done'][r].item())
            cur, Td, sampled = L0 + 1, L0, 1
            rounds = proposed = accepted = 0
            trace = []
            while not done:
                k = S.proposals_per_round(self.draft_tokens, sampled, self.sample_len, cur, cap)
                if k is None:
                    break
                # the draft: one pass over what it has not seen (1 token, 2 after a fully accepted round), then one token per step
                for i in range(k):
                    lo = Td if i == 0 else cur + i - 1
                    n_new = cur + i - lo
                    dsess.decoder_step(row[:, lo:cur + i], dpos[lo:cur + i], dgr.cross, dgr.kv, cap, dgr.kv, cap, dlogits, lo, sm,
                                       slot=0, not_alone=na)
                    draft._greedy(dview, r, r + 1, dlogits.data_ptr() + (n_new - 1) * V * 2, n_new * V, cur + i, sm, temperature=0.0)
                # the main engine: one pass over the last token and the k proposals, one verify step
                sess.decoder_step(row[:, cur - 1:cur + k], pos[cur - 1:cur + k], gr.cross, gr.kv, cap, gr.kv, cap, mlogits, cur - 1, sm,
                                  slot=0, not_alone=na)
                if keep_trace:
                    proposals = tuple(row[0, cur:cur + k].tolist())
                self._verify(st, r, mlogits, k + 1, cur, pair, ws, sm)
                n_acc, flag = pair.tolist()                    # the round's only synchronisation
                if keep_trace:
                    trace.append((cur - 1, proposals, n_acc))
                if k:
                    _, Td = S.after_round(cur - 1, k, n_acc)
                cur, sampled, done = cur + n_acc, sampled + n_acc, bool(flag)
                rounds, proposed, accepted = rounds + 1, proposed + k, accepted + n_acc - 1
            if done:
                st['done'][r] = 1
            cur_max = max(cur_max, cur)
            for name, value in (('rounds', rounds), ('proposals', proposed), ('accepted', accepted), ('tokens', sampled)):
                stats[name].append(value)
            if keep_trace:
                stats['trace'].append(trace)
        nsp_dev = self._no_speech_probs(st, main, []) if self.tokenizer.no_speech is not None else None
        out = self._finish_main_loop(st, cur_max, L0, n_batch, False, nsp_dev)
        self.speculative_stats = stats
        if one_row and not _retry and self._chain_gave_up("speculative loop"):
            return self._speculative_loop(audio_features, row_limit=row_limit, _retry=True)
        return out
