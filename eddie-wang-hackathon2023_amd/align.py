"""align.py: forced alignment from the command line -- the transcript is given, the times are asked for (transcribe.align;
alignment.py states the contract).

python align.py --engine_dir eng --input_file a.flac [b.flac ...] --text_file a.txt [b.txt ...] --vocab multilingual.tiktoken
                [--language L] [--max_tokens N] [--edge_seconds S] [--rows R] [--words]

prints one "[mm:ss.mmm --> mm:ss.mmm] line" per non-blank line of every text file ("[unplaced]" where none of the line's words found
room in the audio), and with --words one "start-end word (probability)" line per word under it.  The text must start where the
audio's speech starts; max_tokens and edge_seconds are parameters nobody has tuned on speech.
"""
from __future__ import annotations

import argparse
import logging
from pathlib import Path
from typing import List

import torch

from alignment import AlignOptions


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--log_level', type=str, default='error')
    parser.add_argument('--engine_dir', type=str, default='whisper_outputs')
    parser.add_argument('--input_file', type=str, nargs='+', required=True, help='.flac / .wav files of any length')
    parser.add_argument('--text_file', type=str, nargs='+', required=True, help='one UTF-8 text file per input file: a line is a segment')
    parser.add_argument('--vocab', type=str, default=None, help='path to multilingual.tiktoken / gpt2.tiktoken (default: the bundled vocabulary of the engine\'s size)')
    parser.add_argument('--language', type=str, default=None, help='language of the files (default: detected on every file\'s first window)')
    parser.add_argument('--max_tokens', type=int, default=AlignOptions.max_tokens, help='text tokens forced on one window (default: 128; untuned)')
    parser.add_argument('--edge_seconds', type=float, default=AlignOptions.edge_seconds,
                        help='a word that ends closer than this to a window\'s end waits for the next window (default: 0.5; untuned)')
    parser.add_argument('--rows', type=int, default=None, help='rows of a round (default: min(files, what fits))')
    parser.add_argument('--words', default=False, action='store_true', help='print "start-end word (probability)" under every line')
    return parser.parse_args(argv)


def read_lines(path: str) -> List[str]:
    with open(path, encoding='utf-8') as fh:
        return [line.strip() for line in fh.read().splitlines() if line.strip()]


def format_result(result: dict, words: bool) -> List[str]:
    from transcribe import format_timestamp
    out = []
    for s in result['segments']:
        span = f"[{format_timestamp(s['start'])} --> {format_timestamp(s['end'])}]" if s['aligned'] else "[unplaced]"
        out.append(f"{span} {s['text']}")
        if words:
            for w in s['words']:
                mark = "" if w['aligned'] else " unplaced"
                out.append(f"{w['start']:.2f}–{w['end']:.2f} {w['word'].strip()} ({w['probability']:.2f}){mark}")
    return out


def main(args) -> List[dict]:
    logging.basicConfig(level=getattr(logging, args.log_level.upper(), logging.ERROR))
    if len(args.text_file) != len(args.input_file):
        raise ValueError(f"align: {len(args.text_file)} text files for {len(args.input_file)} input files")
    options = AlignOptions(max_tokens=args.max_tokens, edge_seconds=args.edge_seconds)
    texts = [read_lines(p) for p in args.text_file]
    import transcribe
    from decoding import DecodingOptions, WhisperDecoding
    from encoding import WhisperEncoding
    torch.cuda.set_device(0)
    engine_dir = Path(args.engine_dir)
    encoding = WhisperEncoding(engine_dir)
    decoding = WhisperDecoding(engine_dir, vocab_path=args.vocab, options=DecodingOptions(language=args.language))
    results = transcribe.align(encoding, decoding, args.input_file, texts, language=args.language, options=options, rows=args.rows)
    for path, result in zip(args.input_file, results):
        if len(results) > 1:
            print(f"{path} ({result['language']})")
        for line in format_result(result, args.words):
            print(line)
    return results


if __name__ == '__main__':
    main(parse_arguments())
