"""bench.py's headline pipeline (576 clips, 128 tokens, int8 weight-only + int8 KV, random weights) for large-v2, large-v3 and
large-v3-turbo in ONE session on one board: the models take turns, `--runs` runs each, every run a fresh `bench.py` process (bench.py
itself is not touched: it has always taken `--model`).  Then the token step of turbo at 1 / 8 / 64 / 576 rows, and the device front end
at 80 and 128 bins.

Reported, as measurements and not pass marks: tokens/s, the encoder pass in the open, prefill + decode loop per token (the token
step), the front end; and whether two expectations stated before anything was measured held:

  (1) large-v3 is within the session's run-to-run spread of large-v2 everywhere but the front end and conv1 (128 bins instead of 80);
  (2) turbo's token step is far below large-v2's (4 decoder layers instead of 32), so the encoder's share of a step rises.

    python scripts/bench_v3.py --out v3_figures.json            # ~ 10 minutes on an MI355X

A child that fails ends the session: nothing more is started on the device behind a run that did not end well.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ("large-v2", "large-v3", "large-v3-turbo")


def bench(model, batch, args, cache):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--model", model, "--batch", str(batch), "--decode-steps", str(args.decode_steps), "--engine-cache", cache] + (["--stub-engine"] if args.stub_engine else [])
    t0 = time.time()
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=args.child_timeout)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} ended with {r.returncode}:\n{r.stderr[-2000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    p = d["pipeline"]
    out = dict(model=model, batch=batch, tokens_per_s=d["value"], ms_per_step=d["ms_per_step"],
               encoder_in_the_open_ms=p["encoder_in_the_open_ms"], encoder_prefetch_ms=p["encoder_prefetch_ms"],
               cross_kv_and_language_ms=p["cross_kv_and_language_ms"], prefill_and_decode_loop_ms=p["prefill_and_decode_loop_ms"],
               token_step_ms=round(p["prefill_and_decode_loop_ms"] / args.decode_steps, 4),
               first_token_after_encoder_ms=p["first_token_after_encoder_ms"], token_checksum=(d.get("gathered") or {}).get("token_checksum"),
               decode_chain=d.get("decode_chain"), engine_build_s=d["engine_build_s"], wall_s=round(time.time() - t0, 1))
    print(json.dumps(out), flush=True)
    return out


def summary(runs, key):
    xs = [r[key] for r in runs if r[key] is not None]
    if not xs:
        return None
    med = statistics.median(xs)
    return dict(median=round(med, 4), min=round(min(xs), 4), max=round(max(xs), 4), spread=round((max(xs) - min(xs)) / med, 4) if med else None,
                runs=xs)


def front_end(batch):
    """wm_log_mel over `batch` clips of 30 s at 80 and 128 bins: ms per call (HIP events, 5 calls behind 2 warm-up calls)."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "eddie-wang-hackathon2023_amd")]
    import torch
    import whisper_utils as wu
    audio = torch.randn(batch, wu.N_SAMPLES, device="cuda") * 0.1
    out = {}
    for _ in range(2):                                                          # the bin counts take turns too
        for n_mels in (80, 128):
            for _ in range(2):
                wu.log_mel_spectrogram_device(audio, n_mels=n_mels)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                wu.log_mel_spectrogram_device(audio, n_mels=n_mels)
            e1.record()
            torch.cuda.synchronize()
            out.setdefault(n_mels, []).append(round(e0.elapsed_time(e1) / 5, 3))
    return {f"{k}_bins_ms": v for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=576)
    ap.add_argument("--decode-steps", type=int, default=128)
    ap.add_argument("--models", nargs="+", default=list(MODELS))
    ap.add_argument("--turbo-rows", type=int, nargs="*", default=[1, 8, 64])
    ap.add_argument("--engine-cache", type=str, default=None, help="keep the engines here (default: a directory of this session, removed at its end)")
    ap.add_argument("--child-timeout", type=float, default=600.0)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--stub-engine", action="store_true", help="self-test of this script without a GPU: bench.py's stand-in engines, no front end")
    args = ap.parse_args()
    tmp = None
    if args.engine_cache is None:
        tmp = tempfile.TemporaryDirectory(prefix="wm_bench_v3_")
    cache = args.engine_cache or tmp.name
    runs = {m: [] for m in args.models}
    for _ in range(args.runs):                                                  # the models take turns
        for m in args.models:
            runs[m].append(bench(m, args.batch, args, cache))
    keys = ("tokens_per_s", "ms_per_step", "encoder_in_the_open_ms", "encoder_prefetch_ms", "cross_kv_and_language_ms",
            "prefill_and_decode_loop_ms", "token_step_ms", "first_token_after_encoder_ms")
    report = {"pipeline": dict(batch=args.batch, decode_steps=args.decode_steps, steps=args.steps, warmup=args.warmup, runs=args.runs),
              "models": {m: {k: summary(rs, k) for k in keys} | {"token_checksum": sorted({r["token_checksum"] for r in rs}),
                                                                "decode_chain": rs[-1]["decode_chain"]} for m, rs in runs.items()}}
    turbo = "large-v3-turbo"
    if turbo in runs and args.turbo_rows is not None:
        rows = {}
        for n in args.turbo_rows:
            r = bench(turbo, n, args, cache)
            rows[n] = dict(token_step_ms=r["token_step_ms"], tokens_per_s=r["tokens_per_s"], encoder_in_the_open_ms=r["encoder_in_the_open_ms"],
                           decode_chain_launches=(r["decode_chain"] or {}).get("launches"), declined=(r["decode_chain"] or {}).get("declined"))
        rows[args.batch] = dict(token_step_ms=report["models"][turbo]["token_step_ms"]["median"],
                                tokens_per_s=report["models"][turbo]["tokens_per_s"]["median"],
                                encoder_in_the_open_ms=report["models"][turbo]["encoder_in_the_open_ms"]["median"])
        report["turbo_token_step_by_rows"] = rows
    report["front_end"] = None if args.stub_engine else front_end(args.batch)
    mm = report["models"]
    if "large-v2" in mm and "large-v3" in mm:
        held = {}
        for k in ("tokens_per_s", "encoder_in_the_open_ms", "encoder_prefetch_ms", "cross_kv_and_language_ms", "token_step_ms"):
            a, b = mm["large-v2"][k], mm["large-v3"][k]
            if a and b:
                d = abs(b["median"] - a["median"]) / a["median"]
                held[k] = dict(difference=round(d, 4), spread=max(a["spread"], b["spread"]), within_spread=bool(d <= max(a["spread"], b["spread"])))
        report["expectation_v3_within_spread_of_v2"] = held
    if "large-v2" in mm and turbo in mm:
        def share(m):           # the encoder pass with the chip to itself against the prefill + decode loop of the same batch
            return mm[m]["encoder_in_the_open_ms"]["median"] / (mm[m]["encoder_in_the_open_ms"]["median"] + mm[m]["prefill_and_decode_loop_ms"]["median"])
        report["expectation_turbo_token_step"] = dict(
            token_step_ms={m: mm[m]["token_step_ms"]["median"] for m in ("large-v2", turbo)},
            ratio=round(mm[turbo]["token_step_ms"]["median"] / mm["large-v2"]["token_step_ms"]["median"], 4),
            encoder_share_of_encoder_plus_loop={m: round(share(m), 4) for m in ("large-v2", turbo)})
    text = json.dumps(report, indent=1)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
