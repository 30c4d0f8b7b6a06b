"""transcribe.py: long-form transcription -- files of any length, several at a time.

Upstream Whisper's `transcribe()` over the engines: a 30-second window moves over each file, seeking by the timestamp tokens
the decoder predicted, and a window whose text looks degenerate is decoded again at the next temperature of a ladder.
longform.py states the contract (the rules and the schedule, on the host, tested on the CPU); this module is the device side of
`longform.transcribe_batched`'s `decode_call`:

  * one file is strictly sequential, the engines' strength is the batch: every round decodes the CURRENT window of every
    unfinished file, one file per row;
  * the round's windows are cut on the device in one launch (wm_mel_windows, csrc/windows.hip) from the files' log-mels, each
    at its own position and of its own length;
  * the encoder runs once per round; a fallback call hands main_loop the SAME features tensor, so the cross K/V stay in place;
  * every decoder call has the same number of rows: rows that are empty or already settled get row_limit = 0 -- the greedy
    kernel closes them with EOT at the first step and the attention kernels drop them -- because a change of batch size makes
    WhisperDecoding free and re-allocate its whole buffer set and its graphs;
  * a file's language is detected on its first window (unless the options name one) and kept for all of its windows.
  * the engine says what it is fed and how its tokens are numbered: the log-mels are computed at `WhisperEncoding.num_mels` bins
    (80 up to large-v2, 128 for large-v3 / large-v3-turbo / distil-large-v3) and a mel of another bin count is refused before a
    kernel reads it (MelBatch.check_bins); the languages and every special id are the decoder's tokenizer's (99 languages up to
    large-v2, 100 with `yue` from large-v3 on: tokenizer.layout_from_vocab); `--language yue` on a 99-language engine is refused.

  * `condition_on_previous_text` / `initial_prompt` (upstream's options; default here: off -- upstream's default is on): every
    file carries its own history (longform.PromptHistory), a round hands the decoder one prompt per row
    (WhisperDecoding.set_prompts: right-aligned rows).  They need an instance built with `row_prompts=True`, whose start
    length is fixed at construction.

  * `word_timestamps`: after a round's ladder has settled every row, ONE WhisperDecoding.word_timestamps call over the round's
    rows (token_probs="device": wm_forced_probs) aligns the text of every row's standing segments on the round's own features --
    the cross K/V stay in place, the encoder still runs once per round -- and longform.settle_words hands the words to the
    segments and lets the last word's end say where the file's next window begins.  Rows without text have no tokens and are
    skipped by wm_align.  The tap pass is left-aligned and starts from sot_sequence, so it runs on a `row_prompts` instance too.

  * `sections` (sections.SectionOptions): a long file is cut where it is quietest (wm_section_cuts,
    csrc/sections.hip: one launch and one copy back for all files) and its sections take the rows that files take otherwise, so
    ONE long recording fills the batch.  A file has one language -- named, or detected on the first window of its FIRST section
    and used by all of them; `initial_prompt` heads every section; word timestamps are aligned per section; the sections'
    segments are shifted and joined by sections.merge_sections.  Unlike upstream, nothing crosses a cut: sections run side by
    side, so `condition_on_previous_text` keeps its history per section.  Without the option nothing of this runs.

  * `speech` (speech.SpeechOptions): skip silence.  The frames that an energy rule over the log-mel takes
    for speech are found on the device (wm_speech_spans, csrc/speech.hip: one launch and one copy back for all files), packed
    into shorter files (wm_mel_gather: one launch) and transcribed by everything above -- sections included: the cuts are found
    on the packed mel -- and speech.restore moves every time back into the original file.  The decoder never sees the quiet
    stretches, so it cannot invent text over them, and a file with 40 % pauses has 40 % fewer windows.  An energy rule, not a
    trained voice-activity model, and its defaults are parameters, not measurements.  Without the option nothing of this runs.

  * `channels` (channels.ChannelOptions): a recording's channels are kept apart instead of downmixed.
    "split": every channel has a log-mel of its own (resampled by wm_resample_channels: all channels in one launch), the channels
    take the rows that files take otherwise -- through `speech`, `sections` and everything above -- and channels.merge_channels
    sorts their segments by time into `segments` and `turns`; `bleed_db` first silences a channel where another one is much
    louder.  "label": the downmix is transcribed as ever and every segment and word gets the channel that was loudest while it was
    spoken.  Both rest on ONE wm_channel_top call for all recordings (csrc/channels.hip).  It tells CHANNELS apart, not speakers
    inside one, by absolute loudness; the values are parameters nobody has tuned.  Without the option nothing of this runs.

This module is the orchestration and the CLI.  Every entry point runs ONE preamble (`_prepare`: the lengths, the refusals below, the
fp16 batch); `channels`, `speech` and `sections` each split the prepared batch into the batch of the layer below and a function that
puts its results back, and `_transcribe_layers` composes them once over `_transcribe_files`.  What touches a `wm_*` mel entry point
-- the ragged batch with its validation and its device table (uploaded once, read by every layer), and the wrappers `mel_windows`,
`section_cuts`, `speech_spans`, `packed_mels`, `section_mels`, `channel_top` -- is mel_batch.py; the names are re-exported here.

Refused (ValueError): an instance built with `prompt` / `prefix` (use `initial_prompt`), conditioning or an initial prompt on
an instance without `row_prompts`, beam_size / best_of together with a ladder of more than one temperature, and word timestamps
with beam_size / best_of -- unless the instance shares its cross K/V (WhisperDecoding(shared_cross_kv=True): word timestamps for
candidates) and names its sampling mode (beam_size with fallback_best_of: beam search at temperature 0, samples above -- upstream's
`whisper audio.wav` recipe with the full ladder, conditioning and sections; best_of alone keeps the one-temperature rule); word
timestamps on an engine with int8 cross K/V raise WhisperDecoding.word_timestamps' own error.  Out of
scope: clip_timestamps, the hallucination-silence heuristics (hallucination_silence_threshold; `speech` removes silence ahead of
the decoder instead), a learned voice-activity model.  Files at any rate from 4 kHz to 192 kHz and with
several channels are downmixed and resampled to 16 kHz on the device (whisper_utils.load_audio_device, wm_resample).

CLI: python transcribe.py --engine_dir eng --input_file a.flac [b.flac ...] --vocab multilingual.tiktoken [--temperature T ...]
[--no_fallback] [--condition_on_previous_text] [--initial_prompt TEXT] [--word_timestamps] [--sections [--section_seconds S]
[--min_section_seconds S]] [--skip_silence [--silence_margin_db D] [--min_silence_seconds S] [--min_speech_seconds S]
[--speech_pad_seconds S]] [--channels split|label [--bleed_db D]] [--beam_size K [--patience P]] [--best_of M] prints one "[mm:ss.mmm --> mm:ss.mmm] text"
line per non-empty segment, and with --word_timestamps one "start-end word (probability)" line per word under it.
"""
from __future__ import annotations

import argparse
import copy
import logging
import types
from pathlib import Path
from typing import List, Optional, Sequence

import numpy as np
import torch

import channels as channels_mod
import logit_controls
import longform
import sections as sections_mod
import speech as speech_mod
from channels import ChannelOptions
from decoding import DecodingOptions, WhisperDecoding
from encoding import WhisperEncoding
from mel_batch import MelBatch, channel_top, mel_windows, packed_mels, section_cuts, section_mels, speech_spans  # noqa: F401 (re-exported)
from sections import SectionOptions
from speech import SpeechOptions
from word_align import named_language, pass_bytes_per_row, require_fp16_cross_kv


def check_supported(decoding: WhisperDecoding, temperatures: Sequence[float], condition_on_previous_text: bool = False,
                    initial_prompt=None, word_timestamps: bool = False) -> None:
    """The combinations this version refuses (module docstring)."""
    opt = decoding.options
    if word_timestamps:
        if (decoding.beam or decoding.n_group != 1) and not getattr(decoding, 'shared_cross_kv', False):
            raise ValueError("transcribe: word_timestamps with beam_size / best_of is not supported in this version (the device "
                             "alignment reads one row of cross K/V per file) unless the instance was built with shared_cross_kv=True")
        require_fp16_cross_kv(decoding)
    if opt.prompt or opt.prefix:
        raise ValueError("transcribe: an instance built with options.prompt / options.prefix is not supported: hand the prompt to "
                         "transcribe(initial_prompt=...) with an instance built with row_prompts=True")
    if (condition_on_previous_text or initial_prompt) and not getattr(decoding, 'row_prompts', False):
        raise ValueError("transcribe: condition_on_previous_text / initial_prompt need a WhisperDecoding built with row_prompts=True "
                         "(every row carries its own prompt; the start length is fixed at construction)")
    if (decoding.beam or decoding.n_group != 1) and getattr(decoding, 'fallback_best_of', None) is None:
        if len(temperatures) != 1 or float(temperatures[0]) != float(opt.temperature):
            raise ValueError("transcribe: beam_size / best_of decode at the instance's temperature: give that one temperature "
                             f"({opt.temperature}; no fallback), not the ladder {tuple(temperatures)}")


def word_pass_bytes_per_row(decoding: WhisperDecoding) -> int:
    """What a row of the word-timestamp pass holds beside the decoder state: the tape of the alignment heads' queries
    (heads x L_max x 64 fp16 = 128 B each, L_max the longest forced sequence: sot_sequence + <|notimestamps|> + sample_len + EOT,
    at most n_text_ctx) and the fp16 logits of a 4-token call."""
    cfg = decoding.decoder_config
    l_max = min(cfg['num_text_ctx'], len(decoding.tokenizer.sot_sequence) + 2 + int(decoding.sample_len))
    return pass_bytes_per_row(decoding, l_max) + 4 * cfg['vocab_size'] * 2


def default_rows(decoding: WhisperDecoding, n_files: int, device, word_timestamps: bool = False) -> int:
    """min(files, what fits): the decoder state of a row (state_bytes_per_utterance; with word timestamps plus
    word_pass_bytes_per_row) against four fifths of the free memory."""
    free, _ = torch.cuda.mem_get_info(device)
    per_row = decoding.state_bytes_per_utterance() * decoding.n_group
    if word_timestamps:
        per_row += word_pass_bytes_per_row(decoding)
    return max(1, min(n_files, int(0.8 * free // per_row)))


def _checked(decoding, kw: dict) -> dict:
    """`kw` with the ladder as a tuple of floats, once check_supported has let it pass: before any tensor is touched."""
    ladder = kw['temperatures']
    kw = dict(kw, temperatures=tuple(float(t) for t in (ladder if isinstance(ladder, (tuple, list)) else [ladder])))
    check_supported(decoding, kw['temperatures'], kw['condition_on_previous_text'], kw['initial_prompt'], kw['word_timestamps'])
    return kw


def _batch(decoding, mels, content_frames, own: bool = False):
    """(the MelBatch of the mels as contiguous fp16, W = 2 * n_audio_ctx, the seconds per frame).  `own`: no mel of the batch is
    the caller's tensor (the gate of `channels` writes in place)."""
    W = 2 * decoding.decoder_config['num_audio_ctx']
    half = [m.to(torch.float16).contiguous() for m in mels]
    if own:
        half = [h.clone() if h is m else h for h, m in zip(half, mels)]
    return MelBatch(half, content_frames), W, longform.CHUNK_LENGTH / W


def _prepare(decoding, mels, content_frames, kw: dict, own: bool = False):
    """The preamble of every entry point, run once: the lengths, the refusals, then (batch, W, seconds per frame, kw)."""
    if len(content_frames) != len(mels):
        raise ValueError(f"transcribe: {len(content_frames)} content_frames for {len(mels)} mels")
    kw = _checked(decoding, kw)
    return (*_batch(decoding, mels, content_frames, own), kw)


# A layer splits a prepared batch into the batch the layer below transcribes and the function that puts those results back.
def _split_channels(batch: MelBatch, W: int, fs: float, options: ChannelOptions, channel_counts, downmix: Optional[MelBatch]):
    """`channels`.  batch: the channels of all recordings (channel_counts[r] adjacent ones per recording).  "split": one
    wm_channel_top call (with `bleed_db` it gates the mels, which are copies), the channels transcribed as files,
    channels.merge_channels per recording.  "label": the recordings' downmixes are transcribed as ever and
    channels.label_segments names every segment's and word's channel."""
    tops, gated = channel_top(batch, batch.content_frames, channel_counts, options, window=W)

    def label(results):
        out = []
        for r, (res, C) in enumerate(zip(results, channel_counts)):
            res = dict(res)
            res['segments'] = channels_mod.label_segments(res['segments'], tops[r], fs, int(C))
            res['channel_top'] = channels_mod.run_lengths(tops[r])
            out.append(res)
        return out

    def merge(parts):
        out, at = [], 0
        for r, C in enumerate(channel_counts):
            res = channels_mod.merge_channels(parts[at: at + int(C)])
            res['channel_top'] = channels_mod.run_lengths(tops[r])
            res['channel_gated'] = gated[at: at + int(C)]
            out.append(res)
            at += int(C)
        return out

    return (downmix, label) if options.mode == "label" else (batch, merge)


def _split_speech(batch: MelBatch, W: int, fs: float, options: SpeechOptions):
    """`speech`: find the spans, pack them; the times of the packed files' results are moved back."""
    spans = speech_spans(batch, batch.content_frames, options, window=W)

    def restore(results):
        for r, sp in zip(results, spans):
            r['segments'] = speech_mod.restore(r['segments'], sp, fs)
            r['speech'] = [(a * fs, b * fs) for a, b in sp]
            if 'sections' in r:
                r['sections'] = [(speech_mod.restore_time(a, sp, fs), speech_mod.restore_time(b, sp, fs, end=True)) for a, b in r['sections']]
        return results

    return MelBatch(*packed_mels(batch, batch.content_frames, spans, W)), restore


def _split_sections(batch: MelBatch, W: int, fs: float, options: SectionOptions, decoding):
    """`sections`: cut; the sections are files that share their owner's language (`owner`, the third value), merged per file."""
    cuts = section_cuts(batch, batch.content_frames, options, window=W)
    pieces, piece_frames, owner, starts = section_mels(batch, batch.content_frames, cuts, W)

    def merge(parts):
        out = []
        for f in range(len(batch)):
            mine = [i for i, o in enumerate(owner) if o == f]
            segments = sections_mod.merge_sections([parts[i]['segments'] for i in mine], [starts[i] for i in mine], fs)
            text = decoding.tokenizer.decode([t for s in segments for t in s['tokens']]).strip()
            language = parts[mine[0]]['language'] if mine else named_language(decoding)
            out.append(dict(language=language, text=text, segments=segments,
                            sections=[(starts[i] * fs, (starts[i] + piece_frames[i]) * fs) for i in mine]))
        return out

    return MelBatch(pieces, piece_frames), merge, owner


def _transcribe_layers(encoding, decoding, batch: MelBatch, W: int, fs: float, kw: dict, channels=None, speech=None,
                       sections=None) -> List[dict]:
    """channels o speech o sections o files over a prepared batch: every layer that is asked for splits the batch of the one above
    (`sections` inside `speech` cuts the packed mels), `_transcribe_files` decodes what is left, and the layers put the results
    back, innermost first.  `channels`: (ChannelOptions, channel_counts, the downmixes' batch or None)."""
    if len(batch) == 0:
        return []
    if encoding is not None:            # (the engine's bin count, before any kernel reads a mel; without an encoder there is none to hold them to)
        batch.check_bins(encoding.num_mels)
    joins, owner = [], None
    if channels is not None:
        batch, join = _split_channels(batch, W, fs, *channels)
        joins.append(join)
    if speech is not None:
        batch, join = _split_speech(batch, W, fs, speech)
        joins.append(join)
    if sections is not None:
        batch, join, owner = _split_sections(batch, W, fs, sections, decoding)
        joins.append(join)
    results = _transcribe_files(encoding, decoding, batch, batch.content_frames, owner, **kw)
    for join in reversed(joins):
        results = join(results)
    return results


def _transcribe_channels(encoding, decoding, mels, content_frames, channel_counts, options: ChannelOptions, speech, sections,
                         downmix=None, **kw) -> List[dict]:
    """transcribe_mel with `channels` over the channels' mels; "label" also takes `downmix` = (mels, content frames) of the
    recordings' downmixes."""
    options.check()
    if sum(int(c) for c in channel_counts) != len(mels):
        raise ValueError(f"transcribe: channel_counts {list(channel_counts)} for {len(mels)} channel mels")
    batch, W, fs, kw = _prepare(decoding, mels, content_frames, kw, own=options.bleed_db is not None)
    if options.mode == "label":
        downmix = _batch(decoding, *downmix)[0]
    return _transcribe_layers(encoding, decoding, batch, W, fs, kw, (options, channel_counts, downmix), speech, sections)


def transcribe_mel(encoding: WhisperEncoding, decoding: WhisperDecoding, mels: Sequence[torch.Tensor],
                   content_frames: Sequence[int], *, temperatures: Sequence[float] = longform.TEMPERATURES,
                   compression_ratio_threshold: Optional[float] = 2.4, logprob_threshold: Optional[float] = -1.0,
                   no_speech_threshold: Optional[float] = 0.6, n_rows: Optional[int] = None, trace: Optional[list] = None,
                   condition_on_previous_text: bool = False, initial_prompt=None, word_timestamps: bool = False,
                   sections: Optional[SectionOptions] = None, speech: Optional[SpeechOptions] = None,
                   channels: Optional[ChannelOptions] = None, channel_counts: Optional[Sequence[int]] = None) -> List[dict]:
    """Transcribe files given as log-mels: mels[f] fp16 [n_mels, content_frames[f] + W] on the GPU (W = 2 * n_audio_ctx; the last
    W frames are the log-mel of 30 s of padding: whisper_utils.long_log_mel_device).  One dict per file: language, text, segments;
    a segment: seek, start, end (seconds), text, tokens, temperature, avg_logprob, compression_ratio, no_speech_prob.
    `n_rows`: rows of every decoder call (default: min(files, what fits)).  `trace`: a list that receives one dict per decoder
    call (rows, live, temperature, windows, results, prompts, ...: tests, diagnostics).
    `condition_on_previous_text`: every window of a file is decoded with the file's text so far as its prompt (upstream's rules,
    longform.py; off by default, unlike upstream).  `initial_prompt`: a string or token ids, the prompt of every file's first
    window (and, with conditioning, the head of its history).
    `word_timestamps`: every segment also carries `words`, a list of {word, start, end (seconds), probability} (possibly empty);
    segment starts and ends and the seeks follow the words (longform.add_word_timestamps / settle_words).  `trace` then also
    receives one dict per alignment call: kind = "align", round, rows, jobs, languages, alignments (as the device returned them).
    `sections`: cut every file where it is quietest and decode the sections side by side (module docstring; sections.py).  The
    rows' "files" are then the sections, in file order and section order -- `n_rows` defaults to min(sections, what fits), and
    `trace` speaks of sections; a file's result also carries "sections": [(start, end), ...] in seconds.  Unlike upstream,
    `condition_on_previous_text` keeps its history per section: the sections run side by side, so no text crosses a cut.
    `speech`: skip silence (module docstring; speech.py) -- the spans an energy rule takes for speech are packed into shorter
    files, those are transcribed as above (`trace`, `seek` inside it and the sections' cuts speak of the packed files), and every
    time of the result is moved back into the original file (speech.restore); a file's result also carries "speech":
    [(start, end), ...] in seconds.  A file without speech has no segments, an empty text and the language the options name
    (None if none is named).
    `channels` with `channel_counts` = [C_r, ...] (module docstring; channels.py): the mels are the CHANNELS of recordings,
    channel_counts[r] adjacent ones per recording, and the result is one dict per recording -- mode "split" only (its `channels`,
    merged `segments`, `turns`, `text`, `language`, `channel_top` as run lengths, `channel_gated`); the rows' "files" are the
    channels.  Mode "label" needs the downmix beside the channels: `transcribe()` over files has both.  Either argument without
    the other is refused."""
    kw = dict(temperatures=temperatures, compression_ratio_threshold=compression_ratio_threshold, logprob_threshold=logprob_threshold,
              no_speech_threshold=no_speech_threshold, n_rows=n_rows, trace=trace, condition_on_previous_text=condition_on_previous_text,
              initial_prompt=initial_prompt, word_timestamps=word_timestamps)
    if channels is not None or channel_counts is not None:
        if channels is None or channel_counts is None:
            raise ValueError("transcribe_mel: `channels` goes with `channel_counts` (the mels given per channel); mels of downmixes have "
                             "no channels to tell apart")
        if channels.check().mode != "split":
            raise ValueError("transcribe_mel: channels mode 'label' needs the downmix beside the channels: use transcribe() over files")
        return _transcribe_channels(encoding, decoding, mels, content_frames, channel_counts, channels, speech, sections, **kw)
    batch, W, fs, kw = _prepare(decoding, mels, content_frames, kw)
    return _transcribe_layers(encoding, decoding, batch, W, fs, kw, None, speech, sections)


def _transcribe_files(encoding: WhisperEncoding, decoding: WhisperDecoding, mels: Sequence[torch.Tensor],
                      content_frames: Sequence[int], owner: Optional[Sequence[int]], *, temperatures, compression_ratio_threshold,
                      logprob_threshold, no_speech_threshold, n_rows, trace, condition_on_previous_text, initial_prompt,
                      word_timestamps) -> List[dict]:
    """transcribe_mel's body.  `owner`: None, or per "file" the file it is a section of: the sections of a file stand together
    in section order and share ONE language, detected (unless named) on the first window of the first of them.  The layers hand
    it the batch they prepared; called on its own with lists it runs the preamble itself."""
    if not isinstance(mels, MelBatch):
        mels, _, _, kw = _prepare(decoding, mels, content_frames, dict(
            temperatures=temperatures, condition_on_previous_text=condition_on_previous_text, initial_prompt=initial_prompt,
            word_timestamps=word_timestamps))
        temperatures = kw['temperatures']
    content_frames = mels.content_frames
    if isinstance(initial_prompt, str):
        initial_prompt = decoding.tokenizer.encode(" " + initial_prompt.strip())
    initial_prompt = [int(t) for t in (initial_prompt if initial_prompt is not None else ())]
    prompted = bool(condition_on_previous_text) or len(initial_prompt) > 0
    n_files = len(mels)
    W = 2 * decoding.decoder_config['num_audio_ctx']
    tk = decoding.tokenizer
    if n_files == 0:
        return []
    n_mels, dev = mels.n_mels, mels.device
    mels.check_bins(encoding.num_mels)
    for f, (m, c) in enumerate(zip(mels, content_frames)):
        if m.dim() != 2 or m.shape[0] != n_mels or m.shape[1] < c or c < 0:
            raise ValueError(f"transcribe: mel {f} has shape {tuple(m.shape)} for {c} frames of content")
    if n_rows is None:
        n_rows = default_rows(decoding, max(1, sum(1 for c in content_frames if c > 0)), dev, word_timestamps)
    n_group = decoding.n_group

    # the language of every file: named by the options, or detected on the file's first window (of its first section)
    multilingual = decoding.is_multilingual
    named = named_language(decoding)                    # (what a file says before any window of it was heard: None until detected)
    languages = sections_mod.SectionLanguages(n_files, owner, named)
    default_token = tk.special_tokens[f"<|{named or 'en'}|>"] if multilingual else None

    win = torch.zeros((n_rows, n_mels, W), dtype=torch.float16, device=dev)
    state = dict(rows=None, features=None, round=-1, languages=None, tokens=None, windows_host=None, detected={})

    def begin_round(rows):
        state['round'] += 1
        state['rows'] = list(rows)
        mel_windows([None if r is None else mels[r[0]] for r in rows], [0 if r is None else r[1] for r in rows], n_mels, W, out=win)
        state['features'] = features = encoding.get_audio_features(win)
        state['windows_host'] = win.cpu() if trace is not None else None
        state['detected'] = {}
        if multilingual:
            fresh = languages.fresh(rows)
            if fresh:
                langs, _ = decoding.detect_language(features)
                for i in fresh:
                    languages.detected(rows[i][0], langs[i])
                    state['detected'][rows[i][0]] = (i, langs[i])
            state['languages'] = [(named or 'en') if r is None else languages.known(r[0]) for r in rows]
            state['tokens'] = [default_token if r is None else tk.special_tokens[f"<|{languages.known(r[0])}|>"] for r in rows]
        else:
            state['languages'], state['tokens'] = ['en'] * len(rows), None

    def decode_call(rows, temperature, live, prompts=None):
        assert len(rows) == n_rows and len(live) == n_rows
        new_round = state['rows'] != list(rows)
        if new_round:
            begin_round(rows)
        features = state['features']
        if state['tokens'] is not None:
            decoding.set_language_tokens(state['tokens'])
        if getattr(decoding, 'row_prompts', False):
            decoding.set_prompts(prompts)                # (None without conditioning / an initial prompt: every row starts bare)
        limit = torch.tensor([(1 << 30) if on else 0 for on in live], dtype=torch.int32).repeat_interleave(n_group)
        # (candidates decode at the instance's temperature -- but for beam search with fallback_best_of, whose calls name theirs)
        per_call = None if ((decoding.beam or n_group != 1) and getattr(decoding, 'fallback_best_of', None) is None) else temperature
        tokens, sum_logprobs, no_speech_probs = decoding.main_loop(features, row_limit=limit, temperature=per_call)
        results = decoding.post_process(tokens, sum_logprobs, no_speech_probs, features, state['languages'], temperature=temperature)
        results = [r if on else None for r, on in zip(results, live)]
        if trace is not None:
            st = next(iter(decoding._state.values()))
            trace.append(dict(round=state['round'], new_round=new_round, temperature=temperature, rows=list(rows), live=list(live),
                              row_limit=limit.clone(), windows=state['windows_host'], languages=list(state['languages']),
                              language_tokens=None if state['tokens'] is None else list(state['tokens']),
                              detected=dict(state['detected']) if new_round else {}, results=results,
                              prompts=None if prompts is None else [list(p) for p in prompts],
                              n_states=len(decoding._state), n_graphs=len(st['graphs'])))
        return results

    def align_call(rows, jobs):
        assert len(jobs) == n_rows and state['rows'] == list(rows), "an alignment belongs to the round that was decoded last"
        sampled = [types.SimpleNamespace(tokens=[] if j is None else list(j[1]), language=lang)
                   for j, lang in zip(jobs, state['languages'])]
        frames = [0 if j is None else int(j[0]) for j in jobs]
        alignments = decoding.word_timestamps(state['features'], sampled, frames, token_probs="device")
        if trace is not None:
            trace.append(dict(kind="align", round=state['round'], rows=list(rows), jobs=copy.deepcopy(list(jobs)),
                              languages=list(state['languages']), alignments=copy.deepcopy(alignments)))
        return alignments

    words = dict(align_call=align_call, eot=tk.eot) if word_timestamps else {}
    segments = longform.transcribe_batched(
        decode_call, [int(c) for c in content_frames], n_rows, window=W, timestamp_begin=tk.timestamp_begin,
        temperatures=temperatures, compression_ratio_threshold=compression_ratio_threshold, logprob_threshold=logprob_threshold,
        no_speech_threshold=no_speech_threshold, decode_text=tk.decode, **words,
        **(dict(condition_on_previous_text=bool(condition_on_previous_text), initial_prompt=initial_prompt) if prompted else {}))
    out = []
    for f in range(n_files):
        text = tk.decode([t for s in segments[f] for t in s['tokens']]).strip()
        out.append(dict(language=languages.of(f), text=text, segments=segments[f]))
    return out


def _transcribe_recordings(encoding, decoding, audio_or_paths, options: ChannelOptions, **kw) -> List[dict]:
    """`transcribe` with `channels`: the channels of every file as waveforms (whisper_utils.load_audio_device(channels="split")),
    one log-mel per channel -- each clamped to its own max - 8, as a mono file holding that channel is -- and for "label" the
    downmix as `transcribe` has always made it."""
    import whisper_utils as wu
    options.check()
    if not all(isinstance(a, (str, Path)) for a in audio_or_paths):             # refused before anything is loaded or decoded
        raise ValueError("transcribe: `channels` needs files: a waveform handed over is a mono waveform at 16 kHz and has no channels to "
                         "tell apart (mels per channel: transcribe_mel(..., channel_counts=...))")
    speech, sections = kw.pop('speech', None), kw.pop('sections', None)
    defaults = dict(temperatures=longform.TEMPERATURES, compression_ratio_threshold=2.4, logprob_threshold=-1.0, no_speech_threshold=0.6,
                    n_rows=None, trace=None, condition_on_previous_text=False, initial_prompt=None, word_timestamps=False)
    unknown = set(kw) - set(defaults)
    if unknown:
        raise TypeError(f"transcribe: unexpected arguments {sorted(unknown)}")
    kw = _checked(decoding, {**defaults, **kw})                                 # the preamble's refusals, before anything is loaded
    mels, content, counts, mono_mels, mono_content = [], [], [], [], []
    for a in audio_or_paths:
        wave = wu.load_audio_device(str(a), channels="split")
        mono = wu.load_audio_device(str(a)) if options.mode == "label" else None
        for c in range(wave.shape[0]):
            mel, frames = wu.long_log_mel_device(wave[c].contiguous(), n_mels=encoding.num_mels)
            mels.append(mel)
            content.append(frames)
        counts.append(int(wave.shape[0]))
        if mono is not None:
            mel, frames = wu.long_log_mel_device(mono.float().flatten(), n_mels=encoding.num_mels)
            mono_mels.append(mel)
            mono_content.append(frames)
    batch, W, fs = _batch(decoding, mels, content, own=options.bleed_db is not None)      # (and its batch, once they are)
    downmix = _batch(decoding, mono_mels, mono_content)[0] if options.mode == "label" else None
    return _transcribe_layers(encoding, decoding, batch, W, fs, kw, (options, counts, downmix), speech, sections)


def transcribe(encoding: WhisperEncoding, decoding: WhisperDecoding, audio_or_paths, channels: Optional[ChannelOptions] = None,
               **kw) -> List[dict]:
    """`transcribe_mel` over files (FLAC / WAV paths at any rate, any channel count: whisper_utils.load_audio_device resamples on
    the GPU) or waveforms (float arrays or tensors at 16 kHz): the log-mel of each whole file comes from one wm_log_mel call
    (whisper_utils.long_log_mel_device).  `channels` (channels.ChannelOptions): the channels of a recording
    are kept apart -- "split": transcribed one by one and merged by time, "label": the downmix with every segment's loudest
    channel; a mono waveform is refused, a one-channel file is its own channel 0.  Without it nothing of that runs."""
    if channels is not None:
        return _transcribe_recordings(encoding, decoding, list(audio_or_paths), channels, **kw)
    import whisper_utils as wu
    mels, content = [], []
    for a in audio_or_paths:
        if isinstance(a, (str, Path)):
            a = wu.load_audio_device(str(a))
        a = a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a, dtype=np.float32))
        mel, frames = wu.long_log_mel_device(a.float().flatten().cuda(), n_mels=encoding.num_mels)
        mels.append(mel)
        content.append(frames)
    return transcribe_mel(encoding, decoding, mels, content, **kw)


# Forced alignment -- the text is given, the times are asked for -- shares the schedule, not the code: forced_align.py (alignment.py
# states its contract).  `sections`, `speech` and `channels` do not combine with it.
from alignment import AlignOptions  # noqa: E402,F401 (re-exported)
from forced_align import align, align_mel  # noqa: E402,F401 (re-exported)


def format_timestamp(seconds: float) -> str:
    ms = round(seconds * 1000.0)
    return f"{ms // 60000:02d}:{ms % 60000 // 1000:02d}.{ms % 1000:03d}"


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--log_level', type=str, default='error')
    parser.add_argument('--engine_dir', type=str, default='whisper_outputs')
    parser.add_argument('--input_file', type=str, nargs='+', required=True, help='.flac / .wav files of any length, 4 kHz .. 192 kHz, any channel count (resampled to 16 kHz mono on the GPU)')
    parser.add_argument('--vocab', type=str, default=None, help='path to multilingual.tiktoken (text output)')
    parser.add_argument('--language', type=str, default=None,
                        help="language of the files, a code or a name of the engine's vocabulary (default: detected per file; yue / "
                             "cantonese only with a 100-language engine: large-v3 and after)")
    parser.add_argument('--temperature', type=float, nargs='+', default=list(longform.TEMPERATURES),
                        help='the fallback ladder (default: 0 0.2 0.4 0.6 0.8 1)')
    parser.add_argument('--no_fallback', default=False, action='store_true', help='decode every window once, at the first temperature')
    parser.add_argument('--rows', type=int, default=None, help='rows of a decoder call (default: min(files, what fits))')
    parser.add_argument('--condition_on_previous_text', default=False, action='store_true',
                        help="decode every window with the file's text so far as its prompt (upstream's default; off here)")
    parser.add_argument('--block_prefill', default=False, action='store_true',
                        help='run start blocks of more than 4 tokens (a prompt per row) in one pass (WhisperDecoding(block_prefill=True)); implies nothing else')
    parser.add_argument('--initial_prompt', type=str, default=None, help="text in front of every file's first window: names, spelling, style")
    parser.add_argument('--word_timestamps', default=False, action='store_true',
                        help='print "start-end word (probability)" lines under every segment (cross-attention alignment + DTW on the device)')
    parser.add_argument('--sections', default=False, action='store_true',
                        help='cut every file where it is quietest and decode the sections side by side: one long file fills the batch '
                             '(no text or timestamp crosses a cut; conditioning keeps its history per section)')
    parser.add_argument('--section_seconds', type=float, default=SectionOptions.max_seconds, help='longest section (default: 30)')
    parser.add_argument('--min_section_seconds', type=float, default=None, help='shortest section but for the last (default: half the longest)')
    parser.add_argument('--skip_silence', default=False, action='store_true',
                        help='cut out what an energy rule over the log-mel takes for silence before anything is decoded, and move the '
                             'timestamps back (not a trained voice-activity model; the defaults are untuned parameters)')
    parser.add_argument('--silence_margin_db', type=float, default=SpeechOptions.margin_db,
                        help="speech stands this far above the file's loudness floor (default: 8)")
    parser.add_argument('--min_silence_seconds', type=float, default=SpeechOptions.min_silence_seconds, help='shorter pauses stay in (default: 2)')
    parser.add_argument('--min_speech_seconds', type=float, default=SpeechOptions.min_speech_seconds, help='shorter speech goes (default: 0.25)')
    parser.add_argument('--speech_pad_seconds', type=float, default=SpeechOptions.speech_pad_seconds, help='kept on either side of speech (default: 0.4)')
    parser.add_argument('--beam_size', type=int, default=None,
                        help='beam search at temperature 0 with this many beams (default: greedy); the beams share one copy of the cross K/V, '
                             'and above temperature 0 the ladder draws --best_of samples per window (default 1), at most beam_size')
    parser.add_argument('--patience', type=float, default=None, help='beam search patience (needs --beam_size)')
    parser.add_argument('--best_of', type=int, default=None,
                        help='samples per window above temperature 0.  Without --beam_size every window is decoded as best_of samples at '
                             'ONE temperature: give exactly one --temperature above 0 (a per-call temperature, i.e. the ladder, is refused)')
    parser.add_argument('--channels', type=str, default=None, metavar='split|label',
                        help="keep a recording's channels apart: 'split' transcribes every channel on its own and merges by time, 'label' "
                             "transcribes the downmix and names every segment's loudest channel (whisper.cpp's --diarize); prints 'chN:' "
                             'in front of every segment.  Channels, not speakers; absolute loudness, no level matching')
    parser.add_argument('--bleed_db', type=float, default=None,
                        help="with --channels split: silence a channel's frames where another channel is louder by this many dB "
                             '(microphones that hear each other; off by default -- on a telephone line it would mute the quieter party '
                             'of an overlap; an untuned parameter)')
    parser.add_argument('--draft_engine_dir', type=str, default=None,
                        help='speculative decoding at temperature 0 (WhisperDecoding(draft_engine_dir=...)): the engines of a draft model with '
                             'the same encoder output, context and vocabulary; rows are decoded one after another, so it serves one long '
                             'file without --sections; not with --beam_size / --best_of, prompts, the repetition controls or a bias')
    parser.add_argument('--draft_tokens', type=int, default=3, help='speculative decoding: proposals per round (1..3)')
    logit_controls.add_arguments(parser)
    return parser.parse_args(argv)


def channel_options_from_args(args) -> Optional[ChannelOptions]:
    """The ChannelOptions of the command line (None without --channels); ValueError for an unknown mode, --bleed_db without
    --channels split, or a --bleed_db out of range."""
    mode, bleed = getattr(args, 'channels', None), getattr(args, 'bleed_db', None)
    if mode is None:
        if bleed is not None:
            raise ValueError("--bleed_db needs --channels split")
        return None
    return ChannelOptions(mode=mode, bleed_db=bleed).check()


def build_decoding(args, engine_dir, prompted: bool) -> WhisperDecoding:
    """The WhisperDecoding of the command line: greedy as ever; --beam_size: beam search at 0 and --best_of samples above on one
    shared copy of the cross K/V; --best_of alone: best_of samples at the one temperature given.  --repetition_penalty /
    --no_repeat_ngram_size, --hotwords / --sequence_bias_file and --top_k / --top_p / --min_p go into the instance's options: every window, temperature and section
    decodes through it."""
    repeat = logit_controls.options_from_args(args)
    draft = getattr(args, 'draft_engine_dir', None)
    draft = dict(draft_engine_dir=Path(draft), draft_tokens=getattr(args, 'draft_tokens', 3)) if draft else {}    # (refusals: WhisperDecoding's)
    if args.beam_size is not None:
        options = DecodingOptions(language=args.language, beam_size=args.beam_size, patience=args.patience, **repeat)
        return WhisperDecoding(engine_dir, vocab_path=args.vocab, options=options, row_prompts=prompted, shared_cross_kv=True,
                               fallback_best_of=args.best_of if args.best_of is not None else 1, block_prefill=args.block_prefill, **draft)
    if args.patience is not None:
        raise ValueError("--patience needs --beam_size")
    if args.best_of is not None:
        options = DecodingOptions(language=args.language, best_of=args.best_of, temperature=float(args.temperature[0]), **repeat)
        return WhisperDecoding(engine_dir, vocab_path=args.vocab, options=options, row_prompts=prompted, shared_cross_kv=True,
                               block_prefill=args.block_prefill, **draft)
    return WhisperDecoding(engine_dir, vocab_path=args.vocab, options=DecodingOptions(language=args.language, **repeat), row_prompts=prompted,
                           block_prefill=args.block_prefill, **draft)


def main(args) -> List[dict]:
    logging.basicConfig(level=getattr(logging, args.log_level.upper(), logging.ERROR))
    channel_options = channel_options_from_args(args)
    torch.cuda.set_device(0)
    engine_dir = Path(args.engine_dir)
    encoding = WhisperEncoding(engine_dir)
    prompted = bool(args.condition_on_previous_text or args.initial_prompt)
    decoding = build_decoding(args, engine_dir, prompted)
    temperatures = tuple(args.temperature[:1] if args.no_fallback else args.temperature)
    results = transcribe(encoding, decoding, args.input_file, temperatures=temperatures, n_rows=args.rows,
                         condition_on_previous_text=args.condition_on_previous_text, initial_prompt=args.initial_prompt,
                         word_timestamps=args.word_timestamps,
                         sections=SectionOptions(args.section_seconds, args.min_section_seconds) if args.sections else None,
                         **(dict(channels=channel_options) if channel_options is not None else {}),
                         **(dict(speech=SpeechOptions(margin_db=args.silence_margin_db, min_silence_seconds=args.min_silence_seconds,
                                                      min_speech_seconds=args.min_speech_seconds,
                                                      speech_pad_seconds=args.speech_pad_seconds)) if args.skip_silence else {}))
    for path, result in zip(args.input_file, results):
        if len(results) > 1:
            print(f"{path} ({result['language']})")
        if args.skip_silence:
            for c, part in enumerate(result['channels']) if 'speech' not in result else [(None, result)]:
                print(("speech: " if c is None else f"speech ch{c}: ")
                      + (", ".join(f"{format_timestamp(a)} --> {format_timestamp(b)}" for a, b in part['speech']) or "none"))
        for s in result['segments']:
            if s['text'].strip():
                who = "" if channel_options is None else ("ch?: " if s['channel'] is None else f"ch{s['channel']}: ")
                print(f"[{format_timestamp(s['start'])} --> {format_timestamp(s['end'])}] {who}{s['text'].strip()}")
                for w in s.get('words', ()):
                    print(f"{w['start']:.2f}\u2013{w['end']:.2f} {w['word'].strip()} ({w['probability']:.2f})")
    return results


if __name__ == '__main__':
    main(parse_arguments())
