"""Long-form transcription, two figures.  Reports only.
  (1) wm_mel_windows at the product shape, 576 x 80 x 3000 with odd seeks into files of odd length, beside a hipMemcpyAsync
      (torch's device-to-device copy_) of the same bytes, both in GB/s of bytes read + written;
  (2) a job of N synthetic files through transcribe.transcribe_mel with the fallback off, beside the same windows, round by
      round, through get_audio_features -> main_loop -> post_process at the same row count;
  (3) the same job with word_timestamps=True (one alignment call per round; the last word's end moves the windows, so the job
      has windows and rounds of its own: both are reported, and the time per round beside (2)'s).
      python scripts/bench_longform.py [files=16] [windows_per_file=3] [tokens=32] [engine_dir]
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
import transcribe as T
from decoding import DecodingOptions, WhisperDecoding
from encoding import WhisperEncoding

N = int(sys.argv[1]) if len(sys.argv) > 1 else 16
WINDOWS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
TOKENS = int(sys.argv[3]) if len(sys.argv) > 3 else 32
report = {}


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


# ---- (1) the kernel beside a copy of the same bytes
Bn, M, W, F = 576, 80, 3000, 6731
g = torch.Generator(device="cuda").manual_seed(7)
files = [torch.randn((M, F), generator=g, device="cuda").half() for _ in range(Bn)]
seeks = [2 * int(s) + 1 for s in torch.randint(0, (F - W) // 2, (Bn,), generator=torch.Generator().manual_seed(8))]
table = torch.tensor([[f.data_ptr() for f in files], [F] * Bn, seeks], dtype=torch.int64, device="cuda")
frames, seek = table[1].to(torch.int32), table[2].to(torch.int32)
out = torch.empty((Bn, M, W), dtype=torch.float16, device="cuda")
lib, stream = native.load_library(), torch.cuda.current_stream().cuda_stream
ms_k = gpu_ms(lambda: native.check(lib.wm_mel_windows(table[0].data_ptr(), frames.data_ptr(), seek.data_ptr(), Bn, M, W, out.data_ptr(), stream)))
assert torch.equal(out[5], files[5][:, seeks[5]:seeks[5] + W])
flat = torch.randn(out.numel(), generator=g, device="cuda").half().view_as(out)
ms_c = gpu_ms(lambda: out.copy_(flat))
moved = 2 * out.numel() * 2 / 1e9
report["mel_windows"] = dict(shape=[Bn, M, W], src_frames=F, kernel_ms=ms_k, kernel_GBps=moved / ms_k * 1e3, memcpy_ms=ms_c, memcpy_GBps=moved / ms_c * 1e3)
print(f"wm_mel_windows {Bn} x {M} x {W}, odd seeks, src_frames {F}: {ms_k:.3f} ms = {moved / ms_k * 1e3:.0f} GB/s; "
      f"hipMemcpyAsync of the same bytes: {ms_c:.3f} ms = {moved / ms_c * 1e3:.0f} GB/s (median of 20)")
del files, flat, out

# ---- (2) a job of N files beside the same windows through plain main_loop
tmp = None
if len(sys.argv) > 4:
    eng, shape = Path(sys.argv[4]), None
elif (Path("/tmp/wm_bench_engines/large-v2-int8-seed0") / "decoder_config.json").exists():
    eng, shape = Path("/tmp/wm_bench_engines/large-v2-int8-seed0"), "large-v2"
else:
    tmp = tempfile.TemporaryDirectory()
    eng, shape = Path(tmp.name) / "eng", "tiny"
    B.build_from_checkpoint(synthetic.synthetic_checkpoint("tiny", 0), B.parse_arguments(["--output_dir", str(eng), "--log_level", "error"]))
enc = WhisperEncoding(eng)
dec = WhisperDecoding(eng, options=DecodingOptions(sample_len=TOKENS, language="en"))
Wn = 2 * dec.decoder_config["num_audio_ctx"]
content = [WINDOWS * Wn - 17 * (i % 5) for i in range(N)]
mels = [(torch.randn((80, c + Wn), generator=g, device="cuda") * 0.5).clamp_(-0.5, 1.5).half() for c in content]
kw = dict(temperatures=(0.0,), n_rows=N, compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None)


def wall_ms(fn, reps=3):
    fn()                                          # warm-up (graph capture, workspaces)
    total = 0.0
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        total += time.perf_counter() - t0
    return total / reps * 1e3


trace = []
T.transcribe_mel(enc, dec, mels, content, trace=trace, **kw)
rounds = [e for e in trace if e["new_round"]]
n_windows = sum(sum(e["live"]) for e in rounds)
ms_job = wall_ms(lambda: T.transcribe_mel(enc, dec, mels, content, **kw))
wins = [e["windows"].cuda() for e in rounds]
limits = [e["row_limit"] for e in rounds]


def plain():
    for w, lim in zip(wins, limits):
        xa = enc.get_audio_features(w)
        tokens, sums, nsp = dec.main_loop(xa, row_limit=lim)
        dec.post_process(tokens, sums, nsp, xa, ["en"] * N)


ms_plain = wall_ms(plain)
report["job"] = dict(engine=shape or str(eng), files=N, rows=N, windows=n_windows, rounds=len(rounds), tokens=TOKENS,
                     transcribe_mel_ms=ms_job, plain_main_loop_ms=ms_plain)
print(f"{shape or eng}: {N} files, {n_windows} windows in {len(rounds)} rounds of {N} rows, sample_len {TOKENS}: transcribe_mel {ms_job:.1f} ms, "
      f"the same windows through get_audio_features + main_loop + post_process {ms_plain:.1f} ms ({ms_job / ms_plain:.2f} x)")

# ---- (3) the same job with word timestamps
trace_w = []
T.transcribe_mel(enc, dec, mels, content, trace=trace_w, word_timestamps=True, **kw)
rounds_w = [e for e in trace_w if e.get("kind") != "align" and e["new_round"]]
aligns_w = [e for e in trace_w if e.get("kind") == "align"]
windows_w = sum(sum(e["live"]) for e in rounds_w)
ms_words = wall_ms(lambda: T.transcribe_mel(enc, dec, mels, content, word_timestamps=True, **kw), reps=2)
report["job_words"] = dict(engine=shape or str(eng), files=N, rows=N, windows=windows_w, rounds=len(rounds_w), alignment_calls=len(aligns_w),
                           tokens=TOKENS, transcribe_mel_ms=ms_words, ms_per_round=ms_words / len(rounds_w),
                           ms_per_round_without_words=ms_job / len(rounds))
print(f"{shape or eng}: the same files with word_timestamps=True: {windows_w} windows in {len(rounds_w)} rounds, {len(aligns_w)} alignment calls: "
      f"transcribe_mel {ms_words:.1f} ms = {ms_words / len(rounds_w):.2f} ms per round (without words: {ms_job / len(rounds):.2f} ms per round)")
print(json.dumps(report))
