"""Word timestamps beside the decode loop: milliseconds of `WhisperDecoding.word_timestamps` (the teacher-forced pass with
the query tap, wm_align: alignment matrix + DTW, the host's word boundaries) and of `main_loop` for the same batch.  Reports
only.      python scripts/bench_word_timestamps.py [batch=8] [tokens=32] [engine_dir]
Without an engine directory: the large-v2 engines `bench.py --engine-cache /tmp/wm_bench_engines` keeps when they exist, else
a `tiny`-shaped engine with seeded random weights built into a temporary directory."""
import json, os, sys, tempfile, time
from pathlib import Path
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "eddie-wang-hackathon2023_amd")]
import native  # noqa: F401
import torch
import build as B
import synthetic
from decoding import DecodingOptions, WhisperDecoding
from encoding import WhisperEncoding

N = int(sys.argv[1]) if len(sys.argv) > 1 else 8
T = int(sys.argv[2]) if len(sys.argv) > 2 else 32
tmp = None
if len(sys.argv) > 3:
    eng, shape = Path(sys.argv[3]), None
elif (Path("/tmp/wm_bench_engines/large-v2-int8-seed0") / "decoder_config.json").exists():
    eng, shape = Path("/tmp/wm_bench_engines/large-v2-int8-seed0"), "large-v2"
else:
    tmp = tempfile.TemporaryDirectory()
    eng, shape = Path(tmp.name) / "eng", "tiny"
    B.build_from_checkpoint(synthetic.synthetic_checkpoint("tiny", 0), B.parse_arguments(["--output_dir", str(eng), "--log_level", "error"]))
enc = WhisperEncoding(eng)
dec = WhisperDecoding(eng, options=DecodingOptions(sample_len=T))
cfg = dec.decoder_config
g = torch.Generator(device="cuda").manual_seed(1234)
mel = (torch.randn((N, 80, 2 * cfg["num_audio_ctx"]), generator=g, device="cuda") * 0.5).clamp_(-0.5, 1.5).half()
xa = enc.get_audio_features(mel)


def timed(fn, reps=3):
    fn()                                          # warm-up (graph capture, workspaces)
    total = 0.0
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        total += time.perf_counter() - t0
    return total / reps * 1e3


dec.detect_language(xa)
ms_loop = timed(lambda: dec.main_loop(xa, ignore_eot=True))
tokens, _, _ = dec.main_loop(xa, ignore_eot=True)
eot = dec.tokenizer.eot
sampled = [[t if t < eot else 11 for t in row[dec.sample_begin:]] for row in tokens.tolist()]     # T text tokens per clip
ms_words = timed(lambda: dec.word_timestamps(xa, sampled))
heads = len(dec.alignment_heads())
print(f"{shape or eng}: {N} clips x {T} tokens, {heads} alignment heads: main_loop {ms_loop:.1f} ms, word_timestamps {ms_words:.1f} ms "
      f"({ms_words / ms_loop:.2f} x the decode loop)")
print(json.dumps({"engine": shape or str(eng), "clips": N, "tokens": T, "alignment_heads": heads, "main_loop_ms": ms_loop,
                  "word_timestamps_ms": ms_words}))
