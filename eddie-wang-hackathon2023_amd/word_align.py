"""Word alignment on the device: `WordAlign`, the part of `WhisperDecoding` (decoding.py assembles the class) behind `word_timestamps`
and forced alignment (forced_align.py) -- DESIGN.md sections 5c and 5o: ONE teacher-forced pass (the tape of the alignment heads'
cross-attention queries, the probability of every forced token), wm_align over the tape, the words read off the paths.  Beside the
mixin: what transcribe.py and forced_align.py say alike about such a pass.  Tested against timing.py and alignment.py.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import torch

import native
import timing
from host_decoding import CHUNK_LENGTH
from tokenizer import Tokenizer


def require_fp16_cross_kv(decoding) -> None:
    """The tap's consumers read fp16 cross K/V: an engine that stores int8 codes is refused with wm_align's own words."""
    if getattr(decoding, 'use_int8_cross_kv', False):
        raise native.WmError("word timestamps need fp16 cross-attention K/V; this engine stores int8 codes (WM_FLAG_INT8_CROSS_KV)")


def named_language(decoding, language: Optional[str] = None) -> Optional[str]:
    """The language a call names (`language`, else the instance's options), as a code; 'en' for an English-only vocabulary; None:
    none is named -- detect per file."""
    if not decoding.is_multilingual:
        return 'en'
    named = language if language is not None else decoding.options.language
    if named is None:
        return None
    return Tokenizer._defaults(True, named, None, decoding.tokenizer.num_languages)[0]


def pass_bytes_per_row(decoding, L: int, paths: bool = False) -> int:
    """What a row of a forced pass of L tokens holds beside the decoder state: the tape (heads x L x 64 fp16 = 128 B each), and with
    `paths` the two paths [L + n_audio_ctx] and the L token probabilities a caller keeps per row."""
    return len(decoding.alignment_heads()) * L * 128 + (2 * (L + decoding.decoder_config['num_audio_ctx']) * 4 + L * 4 if paths else 0)


class WordAlign:
    def word_timestamps(self, audio_features, results, num_frames=None, token_probs: str = "torch",
                        forced_pass: str = "steps") -> List[List[timing.WordTiming]]:
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
        logits read once; long-form transcription uses it).  The two agree to fp32 rounding, not bit for bit.
        `forced_pass`: "steps" (the default: 4 tokens per wm_decoder_step_tap call) or "block" (ONE wm_decoder_prefill_tap over the
        whole forced sequence per row chunk, `_forced_pass_block`; forced alignment uses it).  The two tapes agree to the teacher-forced
        bound, not bit for bit: the block's Linears run at batch x L rows and its attention kernels are attn_prefill.hip's."""
        if token_probs not in ("torch", "device"):
            raise ValueError(f"word_timestamps: token_probs = {token_probs!r}: 'torch' or 'device'")
        if forced_pass not in ("steps", "block"):
            raise ValueError(f"word_timestamps: forced_pass = {forced_pass!r}: 'steps' or 'block'")
        if self.n_group > 1 and not self.shared_cross_kv:
            raise ValueError("word_timestamps: beam_size / best_of > 1 is not supported on the device path in this version "
                             "unless the instance shares its cross K/V (shared_cross_kv=True; torch_word_timestamps has no such limit)")
        require_fp16_cross_kv(self)
        if self._decode_in_flight:
            raise RuntimeError("word_timestamps reuses main_loop's buffers: no decode may be in flight")
        if not audio_features.is_cuda:
            raise ValueError("word_timestamps runs on the GPU (torch_word_timestamps is the CPU statement)")
        n, cap = audio_features.shape[0], self.decoder_config['num_text_ctx']
        sampled = self._result_tokens(results)
        if len(sampled) != n:
            raise ValueError(f"word_timestamps: {len(sampled)} results for {n} utterances")
        languages = [getattr(r, 'language', None) for r in results]
        forced = [self._forced_tokens(s) for s in sampled]
        frames = self._align_frames(num_frames, n)
        n_all = [len(f) if t else 0 for t, f in forced]          # no text: no words, nothing to align (n_tokens - n_prefix - 1 < 1)
        L = max(max(len(f) for _, f in forced), 1)
        if L > cap:
            raise ValueError(f"word_timestamps: a forced sequence of {L} tokens exceeds n_text_ctx = {cap}")
        heads = self.alignment_heads()
        heads_arr = (C.c_int32 * len(heads))(*heads)
        run = self._forced_pass_block if forced_pass == "block" else self._forced_pass
        tape, probs, cross = run(audio_features, forced, L, heads_arr, token_probs)
        pt, pf, lens, matrix = self._align(cross, tape, heads_arr, n_all, frames, L)
        probs = probs.cpu()
        self.last_alignment = dict(path_text=pt, path_time=pf, path_len=lens, n_tokens=n_all, n_frames=frames,
                                   matrix=matrix.cpu() if matrix is not None else None, token_probs=probs)
        return self._words_from_paths(forced, languages, pt, pf, lens, probs)

    BLOCK_LOGIT_BYTES = 1 << 30        # the fp16 logits [rows, L, V] of one wm_decoder_prefill_tap call: the rows are chunked to fit

    def block_pass_rows(self, L: int) -> int:
        """Rows of one block call: what keeps its [rows, L, V] fp16 logits within BLOCK_LOGIT_BYTES (77 rows at 133 tokens of a
        51 865-token vocabulary), at least one."""
        return max(1, self.BLOCK_LOGIT_BYTES // (max(1, L) * self.decoder_config['vocab_size'] * 2))

    def _forced_pass_block(self, audio_features, forced, L, heads_arr, token_probs: str, buffers: Optional[dict] = None):
        """`_forced_pass` as ONE block per row chunk (wm_decoder_prefill_tap, logits from position 0 on): the same three values."""
        return self._forced_pass(audio_features, forced, L, heads_arr, token_probs, block=True, buffers=buffers)

    def _forced_pass(self, audio_features, forced, L, heads_arr, token_probs: str, block: bool = False, buffers: Optional[dict] = None):
        """The teacher-forced pass over the `forced` sequences (padded to L tokens): (the alignment heads' queries [n, n_heads, L, 64],
        the probability of every forced token [n, L], the cross K/V it ran on).  Steps: the utterance groups of `_groups`, 4-token
        windows over each group's growing cache (wm_decoder_step_tap), the token probabilities from each call's whole slab.  `block`:
        row chunks of `block_pass_rows`, the whole sequence in one call on the empty cache, the token probabilities one row at a time
        (an fp32 copy of the slab would be [rows, L, eot]).  `buffers`: a dict the caller keeps between calls -- the tape [n, n_heads,
        capacity >= L, 64], `probs` fp32 [n, capacity] and the logits slab live there and are reused (forced alignment: fixed for the
        call); without it they are allocated here, the tape and the probabilities at [.., L]."""
        dev, cfg, eot = audio_features.device, self.decoder_config, self.tokenizer.eot
        n, V, cap = audio_features.shape[0], cfg['vocab_size'], cfg['num_text_ctx']
        rows = torch.full((n, L + 1), eot, dtype=torch.int32)
        for b, (_, f) in enumerate(forced):
            rows[b, :len(f)] = torch.tensor(f, dtype=torch.int32)
        rows = rows.to(dev)
        sess, pos = self.decoder_session, self.positional_embedding
        st = self._fast_state(n * self._cross_group(), dev)      # (shared cross K/V: the candidates' buffer set; n rows of it are used)
        cross = self._cross_persistent(audio_features, st)
        stream = torch.cuda.current_stream().cuda_stream
        chunk = min(n, self.block_pass_rows(L))
        slab = (chunk * L if block else n * 4) * V
        buffers = {} if buffers is None else buffers
        if 'tape' not in buffers:
            buffers['tape'] = torch.empty((n, len(heads_arr), L, 64), dtype=torch.float16, device=dev)
            buffers['probs'] = torch.zeros((n, L), dtype=torch.float32, device=dev)
        if buffers.get('logits') is None or buffers['logits'].numel() < slab:
            buffers['logits'] = torch.empty(slab, dtype=torch.float16, device=dev)
        tape, probs, logits = buffers['tape'], buffers['probs'], buffers['logits']
        assert tape.shape[0] == n and tape.shape[2] >= L and probs.shape[0] == n and probs.stride(0) >= L
        bounds = [(lo, min(n, lo + chunk)) for lo in range(0, n, chunk)] if block else self._groups(n, unit=1)[1]
        for g, (lo, hi) in enumerate(bounds):
            kv, cr = [t[lo:hi] for t in st['kv']], [t[lo:hi] for t in cross]
            for off in range(0, L, L if block else 4):
                l = min(L if block else 4, L - off)
                lg = logits[: (hi - lo) * l * V].view(hi - lo, l, V)
                if block:
                    sess.decoder_prefill_tap(rows[lo:hi, :L], pos[0:L], cr, kv, cap, lg, stream, 0, tape[lo:hi], heads_arr, slot=2000)
                else:
                    sess.decoder_step_tap(rows[lo:hi, off:off + l], pos[off:off + l], cr, kv if off else None, cap, kv, cap, lg, off,
                                          stream, tape[lo:hi], heads_arr, slot=1000 + g)
                self._forced_probs(lg, rows[lo:hi, off + 1:], probs[lo:hi, off:], token_probs, stream, row_by_row=block)
        return tape, probs, cross

    def _forced_probs(self, lg, nxt, out, token_probs: str, stream, row_by_row: bool) -> None:
        """The probability a call's logits `lg` fp16 [r, l, V] give the token that follows each position (`nxt` int32 [r, >= l]), over
        the text tokens only ([:eot]), into `out` fp32 [r, >= l]; no [B, L, V] fp32 tensor.  "device": wm_forced_probs with the strides
        of what it is given; "torch": gather less logsumexp, over the whole slab or (`row_by_row`) one row's [l, eot] at a time."""
        (r, l, V), eot = lg.shape, self.tokenizer.eot
        if token_probs == "device":
            native.check(native.load_library().wm_forced_probs(lg.data_ptr(), r, l, V, lg.stride(0), lg.stride(1), eot, nxt.data_ptr(),
                                                               nxt.stride(0), out.data_ptr(), out.stride(0), stream), "wm_forced_probs")
            return
        for b in range(r) if row_by_row else [slice(0, r)]:
            lf = lg[b, :, :eot].float()
            nx = nxt[b, :l].long().clamp(max=eot - 1)
            out[b, :l] = (lf.gather(-1, nx[..., None])[..., 0] - lf.logsumexp(dim=-1)).exp()

    def _align(self, cross, tape, heads_arr, n_all, frames, L):
        """wm_align over the recorded queries `tape` and the cross K/V: (path_text, path_time) as numpy [n, L + n_audio_ctx], the paths'
        lengths, and the alignment matrices on the device (`keep_alignment_matrix`) or None."""
        dev, cfg, lib = tape.device, self.decoder_config, native.load_library()
        n, ctx = tape.shape[0], cfg['num_audio_ctx']
        n_tokens = torch.tensor(n_all, dtype=torch.int32, device=dev)
        n_frames = torch.tensor(frames, dtype=torch.int32, device=dev)
        path_ld = L + ctx
        path_text = torch.zeros((n, path_ld), dtype=torch.int32, device=dev)
        path_time = torch.zeros((n, path_ld), dtype=torch.int32, device=dev)
        path_len = torch.zeros(n, dtype=torch.int32, device=dev)
        matrix = torch.zeros((n, L, ctx), dtype=torch.float32, device=dev) if self.keep_alignment_matrix else None
        ws = torch.empty(max(256, lib.wm_align_workspace_bytes(n, len(heads_arr), L, ctx)), dtype=torch.uint8, device=dev)
        io = native.align_io(self.decoder_session.engine.handle, cfg['num_heads'], ctx, tape, cross, heads_arr, n_tokens, n_frames,
                             len(self.tokenizer.sot_sequence), timing.MEDIAN_FILTER_WIDTH, L, matrix, ctx, path_text, path_time, path_len, ws)
        native.check(lib.wm_align(C.byref(io), torch.cuda.current_stream().cuda_stream), "wm_align")
        lens = path_len.cpu().tolist()          # (synchronises: the workspace and the tape stay alive until here)
        return path_text.cpu().numpy(), path_time.cpu().numpy(), lens, matrix

    def _words_from_paths(self, forced, languages, pt, pf, lens, probs) -> List[List[timing.WordTiming]]:
        """The words of every utterance with their times, read off its path (timing.words_from_path)."""
        eot, n_prefix = self.tokenizer.eot, len(self.tokenizer.sot_sequence)
        seconds_per_frame = CHUNK_LENGTH / self.decoder_config['num_audio_ctx']
        out = []
        for b, (text, _) in enumerate(forced):
            if not text or lens[b] == 0:
                out.append([])
                continue
            words, word_tokens = self._split_words(text + [eot], languages[b])
            out.append(timing.words_from_path(pt[b, :lens[b]], pf[b, :lens[b]], words, word_tokens,
                                              probs[b, n_prefix: n_prefix + len(text)].tolist(), seconds_per_frame))
        return out
