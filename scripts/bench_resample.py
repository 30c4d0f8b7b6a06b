"""Micro-benchmark: the device resampler (wm_resample, csrc/resample.hip) on one hour of stereo int32 PCM, beside wm_log_mel on
its result.

Per rate: the time of one resample_device CALL -- the launch plus the allocation of the output and the look-up of the cached
table, not the kernel alone -- from device events around REPEAT calls after WARMUP calls (the table is uploaded before the
window), the bytes the algorithm needs -- the PCM read once plus the output written once, counted from the shapes -- over that time, and the multiply-adds (T per output).  Then whisper_utils.long_log_mel_device on the resampled hour, timed the
same way (MEL_REPEAT calls).  Needs a GPU: there is no fallback.  Prints one JSON line per rate.

    python scripts/bench_resample.py [--seconds 3600] [--rates 44100 48000] [--channels 2]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "eddie-wang-hackathon2023_amd")]
import native  # noqa: E402,F401  (before the first torch.cuda call: sets the package's runtime defaults)
import torch  # noqa: E402

import whisper_utils as wu  # noqa: E402

WARMUP, REPEAT, MEL_REPEAT = 2, 10, 3


def timed_ms(fn, repeat=REPEAT):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(repeat):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / repeat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--rates", type=int, nargs="+", default=[44100, 48000])
    ap.add_argument("--channels", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_resample needs a GPU"
    native.load_library()
    for rate in args.rates:
        L, M, half, H = wu.resample_filter(rate)
        T = 2 * half + 1
        n_in = args.seconds * rate
        g = torch.Generator(device="cuda")
        g.manual_seed(rate)
        pcm = torch.randint(-(1 << 23), 1 << 23, (n_in, args.channels), generator=g, device="cuda", dtype=torch.int32)
        out = wu.resample_device(pcm, rate, 24)
        n_out = int(out.shape[0])
        ms = timed_ms(lambda: wu.resample_device(pcm, rate, 24))
        bytes_moved = pcm.numel() * 4 + n_out * 4
        macs = n_out * T
        mel_ms = timed_ms(lambda: wu.long_log_mel_device(out), repeat=MEL_REPEAT)
        print(json.dumps({
            "bench": "resample", "rate": rate, "seconds": args.seconds, "channels": args.channels, "dtype": "int32/24",
            "L": L, "M": M, "taps": T, "n_in": n_in, "n_out": n_out,
            "resample_ms": round(ms, 3), "bytes_pcm_plus_out": bytes_moved, "GBps_pcm_plus_out": round(bytes_moved / ms / 1e6, 1),
            "multiply_adds": macs, "GMACps": round(macs / ms / 1e6, 1),
            "audio_seconds_per_second": round(args.seconds / (ms / 1e3)),
            "long_log_mel_ms": round(mel_ms, 3), "warmup": WARMUP, "resample_repeat": REPEAT, "long_log_mel_repeat": MEL_REPEAT}), flush=True)
        del pcm, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
