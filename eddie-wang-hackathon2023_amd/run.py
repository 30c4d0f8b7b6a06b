"""run.py: transcribe one input with a built engine directory.  Same CLI and output as the
reference (W/run.py:21-63): prints "transcribe time <s>" and the text.

Audio front-end: the reference shells out to ffmpeg and computes the log-mel on the GPU with
torch.stft (W/whisper_utils.py:17-146).  ffmpeg is not on these boxes; `--input_file` accepts a
`.flac` (wm_flac_decode, csrc/flac_decode.hip -- LibriSpeech's format), a `.wav` (PCM 8 / 16 / 24 / 32
bit or float32), a `.npy` log-mel `[num_mels, 3000]` (80 bins up to large-v2, 128 from large-v3 on: the engine's own count, read from
`WhisperEncoding.num_mels`) or the keyword `synthetic`; a file at another rate than
16 kHz (4 kHz .. 192 kHz) or with several channels is downmixed and resampled on the device
(wm_resample, csrc/resample.hip: ffmpeg's `-ar 16000 -ac 1`, with this project's own filter); the log-mel itself is the HIP front end (wm_log_mel, csrc/frontend.hip: STFT + mel +
log on the device), held to the reference's golden mel in
tests/test_gpu_model.py.  m4a and the other compressed formats (ffmpeg's job in the reference) stay out of scope.
"""
from __future__ import annotations

import argparse
import logging
import time
from pathlib import Path

import numpy as np
import torch

import biasing
import logit_controls
from decoding import DecodingOptions, WhisperDecoding
from encoding import WhisperEncoding


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--log_level', type=str, default='error')
    parser.add_argument('--engine_dir', type=str, default='whisper_outputs')
    parser.add_argument('--input_file', type=str, default='synthetic',
                        help="'synthetic', a .npy log-mel, or a .flac / .wav at any rate from 4 kHz to 192 kHz (resampled to 16 kHz mono)")
    parser.add_argument('--vocab', type=str, default=None, help='path to multilingual.tiktoken (text output)')
    parser.add_argument('--beam_size', type=int, default=None, help='beam search with that many beams (1..8; default: greedy)')
    parser.add_argument('--patience', type=float, default=None, help='beam search: finished candidates per utterance = beam_size * patience')
    parser.add_argument('--shared_cross_kv', default=False, action='store_true',
                        help="beam search: the beams of an utterance read one copy of its cross-attention K/V (off by default); lets --word_timestamps run with --beam_size")
    parser.add_argument('--word_timestamps', default=False, action='store_true',
                        help='print "start-end word (probability)" lines after the text (cross-attention alignment + DTW on the device; with --beam_size it needs --shared_cross_kv)')
    parser.add_argument('--draft_engine_dir', type=str, default=None,
                        help='speculative decoding: the engines of a draft model with the same encoder output, context and vocabulary '
                             '(distil-large-v3 / large-v3-turbo beside large-v3); greedy only')
    parser.add_argument('--draft_tokens', type=int, default=3, help='speculative decoding: proposals per round (1..3)')
    logit_controls.add_arguments(parser)
    return parser.parse_args(argv)


def decoding_options(args) -> DecodingOptions:
    return DecodingOptions(beam_size=args.beam_size, patience=args.patience, **logit_controls.options_from_args(args))


def load_mel(input_file: str, n_mels: int = 80) -> torch.Tensor:
    """The fp32 log-mel [n_mels, 3000] of the input; `n_mels`: the engine's (WhisperEncoding.num_mels)."""
    if input_file == 'synthetic':
        import synthetic
        return synthetic.synthetic_mel(1, n_mels=n_mels)[0].float()
    if input_file.endswith('.npy'):
        return torch.from_numpy(np.load(input_file)).float()
    import whisper_utils
    audio = whisper_utils.pad_or_trim(whisper_utils.load_audio(input_file))
    # STFT + mel projection on the GPU (wm_log_mel); the torch.stft path stays in whisper_utils as the CPU mirror
    return whisper_utils.log_mel_spectrogram_device(torch.from_numpy(audio).float().cuda(), n_mels=n_mels, dtype=torch.float32)


def real_mel_frames(input_file: str):
    """Mel frames of real audio in the 30-second window (None: unknown, the whole window counts) -- what the alignment of
    --word_timestamps is restricted to."""
    if input_file == 'synthetic' or input_file.endswith('.npy'):
        return None
    import whisper_utils
    return min(len(whisper_utils.load_audio(input_file)) // whisper_utils.HOP_LENGTH, whisper_utils.N_FRAMES)


def generate(log_level: str = 'error', engine_dir: str = 'whisper_outputs', input_file: str = 'synthetic',
             vocab: str = None, beam_size: int = None, patience: float = None, word_timestamps: bool = False,
             shared_cross_kv: bool = False, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0,
             hotwords: str = None, hotword_bias: float = biasing.HOTWORD_BIAS, hotword_start_bias: float = biasing.HOTWORD_START_BIAS,
             sequence_bias_file: str = None, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0,
             draft_engine_dir: str = None, draft_tokens: int = 3):
    options = decoding_options(argparse.Namespace(**locals()))                  # (the keywords are parse_arguments' names)
    logging.basicConfig(level=getattr(logging, log_level.upper(), logging.ERROR))
    torch.cuda.set_device(0)
    engine_dir = Path(engine_dir)
    whisper_encoding = WhisperEncoding(engine_dir)
    mel = load_mel(input_file, whisper_encoding.num_mels).to('cuda').type(torch.float16).unsqueeze(0)
    whisper_decoding = WhisperDecoding(engine_dir, vocab_path=vocab, options=options, shared_cross_kv=shared_cross_kv,
                                       draft_engine_dir=Path(draft_engine_dir) if draft_engine_dir else None, draft_tokens=draft_tokens)
    begin_time = time.time()
    audio_features = whisper_encoding.get_audio_features(mel)
    languages, language_probs = whisper_decoding.detect_language(audio_features)
    tokens, sum_logprobs, no_speech_probs = whisper_decoding.main_loop(audio_features)
    result = whisper_decoding.post_process(tokens, sum_logprobs, no_speech_probs, audio_features, languages)
    print("transcribe time " + str(time.time() - begin_time))
    result = result[0]
    print(result.text)
    if word_timestamps:
        frames = real_mel_frames(input_file)
        words = whisper_decoding.word_timestamps(audio_features, [result], None if frames is None else [frames])[0]
        for w in words:
            print(f"{w.start:.2f}\u2013{w.end:.2f} {w.word.strip()} ({w.probability:.2f})")
    return result


def main(argv=None):
    return generate(**vars(parse_arguments(argv)))


if __name__ == '__main__':
    main()
