"""Word timestamps beside the decode loop: milliseconds of `WhisperDecoding.word_timestamps` (the teacher-forced pass with
the query tap, wm_align: alignment matrix + DTW, the host's word boundaries) and of `main_loop` for the same batch, with the
forced tokens' probabilities from PyTorch (token_probs="torch") and from wm_forced_probs (token_probs="device"); then the kernel
alone on one 4-token slab of 576 rows, 576 x 4 x 51865 fp16 logits, beside the PyTorch expression on the same slab.  Reports
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
ms_words_dev = timed(lambda: dec.word_timestamps(xa, sampled, token_probs="device"))
ms_words = 0.5 * (ms_words + timed(lambda: dec.word_timestamps(xa, sampled)))                       # (alternating: torch, device, torch, device)
ms_words_dev = 0.5 * (ms_words_dev + timed(lambda: dec.word_timestamps(xa, sampled, token_probs="device")))
heads = len(dec.alignment_heads())
print(f"{shape or eng}: {N} clips x {T} tokens, {heads} alignment heads: main_loop {ms_loop:.1f} ms, word_timestamps {ms_words:.1f} ms "
      f"({ms_words / ms_loop:.2f} x the decode loop), with token_probs='device' {ms_words_dev:.1f} ms ({ms_words_dev / ms_loop:.2f} x)")

# ---- wm_forced_probs alone: one call's slab at 576 rows
Bk, Pk, V = 576, 4, 51865
limit = V - 1608                                                                                   # eot of the multilingual vocabulary
lib, stream = native.load_library(), torch.cuda.current_stream().cuda_stream
slab = (torch.randn((Bk, Pk, V), generator=g, device="cuda") * 2).half()
nxt = torch.randint(0, V, (Bk, Pk), generator=torch.Generator().manual_seed(5)).to(torch.int32).cuda()
out = torch.zeros((Bk, Pk), dtype=torch.float32, device="cuda")


def gpu_ms(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        t0.record(); fn(); t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    return sorted(times)[len(times) // 2]


def kernel():
    native.check(lib.wm_forced_probs(slab.data_ptr(), Bk, Pk, V, Pk * V, V, limit, nxt.data_ptr(), Pk, out.data_ptr(), Pk, stream), "wm_forced_probs")


def expression():
    lf = slab[:, :, :limit].float()
    return (lf.gather(-1, nxt.long().clamp(max=limit - 1)[..., None])[..., 0] - lf.logsumexp(dim=-1)).exp()


ms_k, ms_t = gpu_ms(kernel), gpu_ms(expression)
diff = float((out - expression()).abs().max())
read = Bk * Pk * limit * 2 / 1e9
print(f"wm_forced_probs {Bk} x {Pk} x {V} (limit {limit}): {ms_k:.3f} ms = {read / ms_k * 1e3:.0f} GB/s of logits read; the PyTorch expression "
      f"on the same slab {ms_t:.3f} ms ({ms_t / ms_k:.1f} x; medians of 20); max |kernel - expression| = {diff:.3g}")
print(json.dumps({"engine": shape or str(eng), "clips": N, "tokens": T, "alignment_heads": heads, "main_loop_ms": ms_loop,
                  "word_timestamps_ms": ms_words, "word_timestamps_device_probs_ms": ms_words_dev,
                  "forced_probs": dict(shape=[Bk, Pk, V], limit=limit, kernel_ms=ms_k, kernel_GBps=read / ms_k * 1e3, torch_ms=ms_t)}))
