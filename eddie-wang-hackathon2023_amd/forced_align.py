"""forced_align.py: forced alignment on the device -- `transcribe.align` / `transcribe.align_mel`.

alignment.py states the contract (the window, accept and seek rules and the literal loop per file, on the host); this module is the
batched schedule, long-form transcription's: a file is strictly sequential, so every ROUND takes the current window of every
unfinished file, one file per row (with fewer rows than files: of the first `rows` unfinished files, in file order),

  * cuts the round's windows in one launch (wm_mel_windows), each at its own seek;
  * runs the encoder once;
  * detects the language of the files whose first window this is (unless one is named, or the vocabulary is English-only);
  * runs the forced sequences -- sot_sequence + <|notimestamps|> + whole words up to max_tokens + <|endoftext|>, one per row -- as
    ONE wm_decoder_prefill_tap block per row chunk, with wm_forced_probs on the block's logits;
  * builds every row's alignment matrix and walks it with an open end in one wm_align_open call;
  * copies ONE buffer back: the paths, their lengths, the end rows and the tokens' probabilities;
  * and lets alignment.settle_window place the words and move every file's seek.

The row count and every buffer are fixed for the call: the block always runs at L = len(sot_sequence) + 2 + max_tokens tokens (shorter
forced sequences are padded with <|endoftext|>, rows without a file have no tokens and are skipped by wm_align_open), so the decoder's
buffer set, the block's workspace, the tape and the logits slab are allocated once.

Memory per row, beside the decoder state (WhisperDecoding.state_bytes_per_utterance): the tape, heads x L x 128 B, and the paths; the
block's fp16 logits [rows, L, V] are the large item -- 13.8 MB a row at L = 133 and V = 51 865 -- and are NOT held per row: the rows
of a round go through the block in chunks whose logits fit WhisperDecoding.BLOCK_LOGIT_BYTES (1 GiB: 77 rows), one slab reused.
`default_align_rows` counts a row as state + tape and keeps four fifths of the free memory less the slab.

Refused before any kernel runs: an engine with int8 cross K/V (the error word timestamps raise), a `cu_partition` instance, beam_size /
best_of instances, len(texts) != files, a tokenizer without a vocabulary (ids only), empty audio, options out of range for the model.
An empty text gives an empty result.  Out of scope: `sections`, `speech` and `channels` together with `align`; an open beginning (the
text must start where the audio's speech starts); text the audio does not contain in the middle; any claim about accuracy -- there
are no trained weights here, and max_tokens, edge_seconds and the un-normalised open end are parameters nobody has tuned.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import List, Optional, Sequence

import numpy as np
import torch

import alignment
import longform
import native
import timing
from alignment import AlignOptions
from mel_batch import MelBatch, mel_windows
from word_align import named_language, pass_bytes_per_row, require_fp16_cross_kv


def check_align_supported(decoding, n_files: int, texts, options: AlignOptions) -> None:
    """The refusals of the module docstring that need no audio."""
    if not isinstance(options, AlignOptions):
        raise ValueError("align: options must be an alignment.AlignOptions")
    require_fp16_cross_kv(decoding)
    if getattr(decoding, 'cu_partition', False):
        raise ValueError("align: the CU-partitioned schedule (cu_partition = True) is not supported: the forced pass is one block on one stream")
    if decoding.beam or decoding.n_group != 1:
        raise ValueError("align: an instance built with beam_size / best_of is not supported (a forced pass has no candidates)")
    if isinstance(texts, str) or len(texts) != n_files:
        raise ValueError(f"align: {len(texts) if not isinstance(texts, str) else 1} texts for {n_files} files (one text per file: a string or a list of lines)")
    if decoding.tokenizer.bpe is None:
        raise ValueError("align: the tokenizer has no vocabulary (ids only): a text cannot be encoded; build WhisperDecoding with vocab_path")
    options.check(decoding.decoder_config['num_text_ctx'], len(decoding.tokenizer.sot_sequence))
    for t in texts:
        if not (isinstance(t, str) or (isinstance(t, (list, tuple)) and all(isinstance(x, str) for x in t))):
            raise ValueError("align: a text is a string or a list of strings (lines)")


def align_pass_bytes_per_row(decoding, options: AlignOptions) -> int:
    """What a row holds beside the decoder state: the tape (heads x L x 128 B) and its paths."""
    return pass_bytes_per_row(decoding, len(decoding.tokenizer.sot_sequence) + 2 + int(options.max_tokens), paths=True)


def default_align_rows(decoding, n_files: int, device, options: AlignOptions) -> int:
    """min(files, what fits): state + tape per row against four fifths of the free memory less the logits slab (module docstring)."""
    free, _ = torch.cuda.mem_get_info(device)
    per_row = decoding.state_bytes_per_utterance() + align_pass_bytes_per_row(decoding, options)
    L = len(decoding.tokenizer.sot_sequence) + 2 + int(options.max_tokens)
    slab = min(decoding.BLOCK_LOGIT_BYTES, n_files * L * decoding.decoder_config['vocab_size'] * 2)
    return max(1, min(n_files, int((0.8 * free - slab) // per_row)))


class _File:
    def __init__(self, text, content: int):
        self.text, self.content = text, int(content)
        self.language: Optional[str] = None
        self.lines: List[str] = [text] if isinstance(text, str) else list(text)
        self.words = self.word_tokens = self.owner = None
        self.k, self.seek, self.placed = 0, 0, []
        self.sot: Optional[tuple] = None

    def split(self, tk, language: Optional[str], max_tokens: int) -> None:
        self.language = language
        self.lines, self.words, self.word_tokens, self.owner = alignment.split_text(tk, self.text, language)
        alignment.check_words(self.word_tokens, max_tokens)
        self.sot = (tk.sot, tk.special_tokens[f"<|{language}|>"], tk.transcribe) if len(tk.sot_sequence) == 3 else tuple(tk.sot_sequence)

    def unfinished(self, window: int) -> bool:
        if self.words is not None and self.k >= len(self.words):
            return False
        if self.words is None and not any(l.strip() for l in self.lines):
            return False
        return self.seek < self.content and alignment.window_frames(self.seek, window, self.content)[0] >= 1


def align_mel(encoding, decoding, mels: Sequence[torch.Tensor], content_frames: Sequence[int], texts, language: Optional[str] = None,
              options: AlignOptions = AlignOptions(), rows: Optional[int] = None, keep_rounds=None) -> List[dict]:
    """Place `texts[f]` (a string, or a list of lines) on the file whose log-mel is mels[f] (fp16 [n_mels, content_frames[f] + W] on
    the GPU, as transcribe_mel takes them).  One dict per file: language, text, words ({word, start, end, probability, aligned}),
    segments (one per given line -- one in all for a string: text, start, end, aligned, words).  Words the audio had no room for
    come back unplaced: start = end = the file's duration, probability 0, aligned False.
    `language`: a code or a name (default: the instance's options'; neither: detected on every file's first window).
    `rows`: rows of every round (default: default_align_rows).  `keep_rounds`: True, or a list that receives one dict per round --
    rows (file, seek, F, last, first_word, forced, n_words, boundaries per row), the device's matrices, token probabilities, paths and
    end rows, what was placed and the next seeks (tests, diagnostics); True puts the list into every result as 'rounds'."""
    n_files = len(mels)
    if len(content_frames) != n_files:
        raise ValueError(f"align: {len(content_frames)} content_frames for {n_files} mels")
    check_align_supported(decoding, n_files, texts, options)
    named = named_language(decoding, language)
    for f, c in enumerate(content_frames):
        if int(c) <= 0:
            raise ValueError(f"align: file {f} has no audio")
    if decoding._decode_in_flight:
        raise RuntimeError("align reuses main_loop's buffers: no decode may be in flight")
    if n_files == 0:
        return []
    cfg, tk = decoding.decoder_config, decoding.tokenizer
    ctx, V = cfg['num_audio_ctx'], cfg['vocab_size']
    W = 2 * ctx
    fs = longform.CHUNK_LENGTH / W                      # seconds per mel frame; an alignment frame is two
    batch = MelBatch([m.to(torch.float16).contiguous() for m in mels], content_frames, "align")
    batch.check_bins(encoding.num_mels)
    n_mels, dev = batch.n_mels, batch.device
    for f, (m, c) in enumerate(zip(batch, batch.content_frames)):
        if m.dim() != 2 or m.shape[1] < c:
            raise ValueError(f"align: mel {f} has shape {tuple(m.shape)} for {c} frames of content")
    files = [_File(t, c) for t, c in zip(texts, batch.content_frames)]
    if named is not None:                               # a named language: every text is split (and every word measured) before a kernel runs
        for fl in files:
            fl.split(tk, named, options.max_tokens)
    n_work = sum(1 for fl in files if fl.unfinished(W))
    if rows is None:
        rows = default_align_rows(decoding, max(1, n_work), dev, options)
    n_rows = int(rows)
    if n_rows < 1:
        raise ValueError(f"align: rows = {rows}")
    trace = keep_rounds if isinstance(keep_rounds, list) else ([] if keep_rounds else None)

    n_sot = len(tk.sot_sequence)
    L = n_sot + 2 + int(options.max_tokens)
    heads = decoding.alignment_heads()
    heads_arr = (C.c_int32 * len(heads))(*heads)
    lib = native.load_library()
    path_ld = L + ctx
    win = torch.zeros((n_rows, n_mels, W), dtype=torch.float16, device=dev)
    buffers = dict(tape=torch.zeros((n_rows, len(heads), L, 64), dtype=torch.float16, device=dev), logits=None)
    # ONE buffer comes back per round: path_text | path_time | path_len | end_row | token probabilities (fp32 bits)
    o_time, o_len, o_end, o_prob = n_rows * path_ld, 2 * n_rows * path_ld, 2 * n_rows * path_ld + n_rows, 2 * n_rows * path_ld + 2 * n_rows
    back = torch.zeros(o_prob + n_rows * L, dtype=torch.int32, device=dev)
    buffers['probs'] = back[o_prob:].view(torch.float32).view(n_rows, L)
    matrix = torch.zeros((n_rows, L, ctx), dtype=torch.float32, device=dev) if trace is not None else None
    ws = torch.empty(max(256, lib.wm_align_workspace_bytes(n_rows, len(heads), L, ctx)), dtype=torch.uint8, device=dev)
    n_tokens = torch.zeros(n_rows, dtype=torch.int32, device=dev)
    n_frames = torch.zeros(n_rows, dtype=torch.int32, device=dev)

    round_no = 0
    while True:
        active = [f for f, fl in enumerate(files) if fl.unfinished(W)][:n_rows]
        if not active:
            break
        slots: List[Optional[int]] = active + [None] * (n_rows - len(active))
        mel_windows([None if f is None else batch[f] for f in slots], [0 if f is None else files[f].seek for f in slots], n_mels, W, out=win)
        features = encoding.get_audio_features(win)
        fresh = [i for i, f in enumerate(slots) if f is not None and files[f].words is None]
        if fresh:                                       # (only without a named language: the files whose first window this is)
            langs, _ = decoding.detect_language(features)
            for i in fresh:
                files[slots[i]].split(tk, langs[i], options.max_tokens)
        plans, forced, n_all, frames, lasts = [], [], [], [], []
        for f in slots:
            fl = None if f is None else files[f]
            if fl is None or fl.k >= len(fl.words):     # (a file whose text turned out empty once it was split)
                plans.append(None); forced.append(([], [])); n_all.append(0); frames.append(0); lasts.append(False)
                continue
            plan = alignment.plan_window(fl.word_tokens[fl.k:], fl.sot, tk.no_timestamps, tk.eot, options.max_tokens)
            F, last = alignment.window_frames(fl.seek, W, fl.content)
            plans.append(plan); forced.append((plan.forced[n_sot + 1:-1], plan.forced)); n_all.append(len(plan.forced)); frames.append(F); lasts.append(last)
        tape, probs, cross = decoding._forced_pass_block(features, forced, L, heads_arr, "device", buffers)
        n_tokens.copy_(torch.tensor(n_all, dtype=torch.int32))
        n_frames.copy_(torch.tensor(frames, dtype=torch.int32))
        io = native.align_io(decoding.decoder_session.engine.handle, cfg['num_heads'], ctx, tape, cross, heads_arr, n_tokens, n_frames,
                             n_sot, timing.MEDIAN_FILTER_WIDTH, L, matrix, ctx, back, back[o_time:], back[o_len:], ws)
        native.check(lib.wm_align_open(C.byref(io), back[o_end:].data_ptr(), torch.cuda.current_stream().cuda_stream), "wm_align_open")
        host = back.cpu().numpy()                       # the round's one copy back (synchronises)
        pt, pf = host[:o_time].reshape(n_rows, path_ld), host[o_time:o_len].reshape(n_rows, path_ld)
        lens, ends = host[o_len:o_end], host[o_end:o_prob]
        pr = host[o_prob:].view(np.float32).reshape(n_rows, L)
        mtx = matrix.cpu().numpy() if matrix is not None else None
        record = dict(round=round_no, rows=[]) if trace is not None else None
        for i, f in enumerate(slots):
            if plans[i] is None:
                if record is not None:
                    record['rows'].append(None)
                continue
            fl, plan = files[f], plans[i]
            n_text = plan.boundaries[-1]
            n = int(lens[i])
            text_idx, time_idx, end_row = pt[i, :n].astype(np.int64), pf[i, :n].astype(np.int64), int(ends[i])
            token_probs = pr[i, n_sot: n_sot + n_text].copy()
            placed, new_seek = alignment.settle_window(fl.words, fl.word_tokens, fl.owner, fl.k, plan, text_idx, time_idx, end_row, token_probs,
                                                       fl.seek, frames[i], lasts[i], W, 2 * fs, options)
            if record is not None:
                record['rows'].append(dict(file=f, seek=fl.seek, n_frames=frames[i], last=lasts[i], first_word=fl.k, forced=list(plan.forced),
                                           n_words=plan.n_words, boundaries=list(plan.boundaries), language=fl.language,
                                           matrix=mtx[i, :n_text + 1, :frames[i]].copy(), token_probs=token_probs,
                                           path_text=text_idx, path_time=time_idx, end_row=end_row, placed=len(placed), next_seek=new_seek))
            assert new_seek > fl.seek
            fl.placed += placed
            fl.k += len(placed)
            fl.seek = new_seek
        if record is not None:
            trace.append(record)
        round_no += 1

    out = []
    for fl in files:
        duration = fl.content * fs
        if fl.words is None:                            # an empty text: nothing was cut, nothing detected
            fl.language = named
            fl.lines, fl.words, fl.word_tokens, fl.owner = (fl.lines, [], [], [])
        res = alignment.file_result(fl.language, fl.lines, fl.placed + alignment.leftover_words(fl.words, fl.word_tokens, fl.owner, fl.k, duration),
                                    duration)
        if keep_rounds is True:
            res['rounds'] = trace
        out.append(res)
    return out


def align(encoding, decoding, audio_or_paths, texts, language: Optional[str] = None, options: AlignOptions = AlignOptions(),
          rows: Optional[int] = None, keep_rounds=None) -> List[dict]:
    """`align_mel` over files (FLAC / WAV paths at any rate, any channel count) or waveforms (float arrays or tensors at 16 kHz), as
    `transcribe` takes them."""
    import whisper_utils as wu
    audio_or_paths = list(audio_or_paths)
    check_align_supported(decoding, len(audio_or_paths), texts, options)      # before anything is loaded
    named_language(decoding, language)
    mels, content = [], []
    for f, a in enumerate(audio_or_paths):
        if isinstance(a, (str, Path)):
            a = wu.load_audio_device(str(a))
        a = a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a, dtype=np.float32))
        if a.numel() == 0:
            raise ValueError(f"align: file {f} has no audio")
        mel, frames = wu.long_log_mel_device(a.float().flatten().cuda(), n_mels=encoding.num_mels)
        mels.append(mel)
        content.append(frames)
    return align_mel(encoding, decoding, mels, content, texts, language=language, options=options, rows=rows, keep_rounds=keep_rounds)
