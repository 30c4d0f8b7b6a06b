"""What repetition_penalty / no_repeat_ngram_size cost in the device decode loop: ms per token step of the greedy loop at 1, 8, 64 and
576 rows with the controls off and with (1.2, 3) -- one extra launch, wm_repeat_controls, in front of every token step -- each
replayed from captured graphs; then the kernel's own time at histories of 16 and 223 tokens.  large-v2 shape, weight-only int8 +
int8 KV, random weights, `ignore_eot` (a fixed number of steps).  Engines: the ones `bench.py --engine-cache /tmp/wm_bench_engines`
keeps (built here when they are missing).

    python scripts/bench_repeat.py [tokens=128] [--rows 1,8,64,576] [--reps 5] [--off-only] [--no-kernel]

--off-only runs the defaults alone and names no option of the controls: the same file measures a tree from before they existed, for
the comparison that matters -- with the defaults the step time must not move."""
import argparse, json, os, statistics, sys, time
from pathlib import Path
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "eddie-wang-hackathon2023_amd")]
import native  # noqa: F401
import torch
import synthetic
from decoding import DecodingOptions, WhisperDecoding
from encoding import WhisperEncoding

ap = argparse.ArgumentParser()
ap.add_argument("tokens", type=int, nargs="?", default=128)
ap.add_argument("--rows", type=str, default="1,8,64,576")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--off-only", action="store_true")
ap.add_argument("--no-kernel", action="store_true")
ap.add_argument("--tag", type=str, default="")
args = ap.parse_args()
T, ROWS = args.tokens, [int(r) for r in args.rows.split(",")]
P, N = 1.2, 3

eng = Path("/tmp/wm_bench_engines/large-v2-int8-seed0")
if not (eng / "decoder_config.json").exists():
    import bench
    eng.parent.mkdir(parents=True, exist_ok=True)
    bench.build_engines(argparse.Namespace(model="large-v2", config="int8", seed=0), eng)
dims = synthetic.DIMS["large-v2"]
enc = WhisperEncoding(eng)


def step_ms(dec, feats):
    """ms per token step: a whole main_loop call (prefill, then T - 1 replayed steps) over T, the median of --reps calls after one
    that captures the graphs.  The cross K/V of the unchanged features are projected once, outside the clock."""
    dec.main_loop(feats, ignore_eot=True)
    dec.main_loop(feats, ignore_eot=True)
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.main_loop(feats, ignore_eot=True)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3 / T)
    return statistics.median(times), min(times), max(times)


report = {"tokens": T, "tag": args.tag, "steps": {}}
for rows in ROWS:
    g = torch.Generator(device="cuda").manual_seed(1234)
    mel = (torch.randn((rows, dims["n_mels"], 2 * dims["n_audio_ctx"]), generator=g, device="cuda") * 0.5).clamp_(-0.5, 1.5).half()
    xa = enc.get_audio_features_async(mel)
    torch.cuda.synchronize()
    del mel
    line = {}
    for name, controls in (("off", {}),) + (() if args.off_only else (("on", dict(repetition_penalty=P, no_repeat_ngram_size=N)),)):
        dec = WhisperDecoding(eng, options=DecodingOptions(sample_len=T, language="en", **controls))
        line[name] = step_ms(dec, xa)
        dec._state.clear()
        del dec
        torch.cuda.empty_cache()
    report["steps"][rows] = line
    msg = f"{rows:4d} rows, {T} tokens: controls off {line['off'][0]:.4f} ms per token step (min {line['off'][1]:.4f}, max {line['off'][2]:.4f})"
    if "on" in line:
        msg += (f" | ({P}, {N}) {line['on'][0]:.4f} ms (min {line['on'][1]:.4f}, max {line['on'][2]:.4f}): "
                f"+{(line['on'][0] - line['off'][0]) * 1e3:.1f} us, x {line['on'][0] / line['off'][0]:.4f}")
    print(msg, flush=True)
    del xa
    torch.cuda.empty_cache()

if not args.off_only and not args.no_kernel:
    # the kernel alone: 200 launches captured into one graph (how the loop issues it), replayed, between two events
    import ctypes as C
    lib = native.load_library()
    V, eot, ld, begin = dims["n_vocab"], 50257, dims["n_text_ctx"] + 1, 3
    report["kernel_us"] = {}
    for rows in (1, 576):
        logits = (torch.randn((rows, V), device="cuda") * 4).half()
        for m in (16, 223):
            tokens = torch.randint(0, 2000, (rows, ld), device="cuda", dtype=torch.int32)      # (a small range: repeats and n-gram matches)
            io = native.WmRepeatIO()
            io.logits, io.row_stride, io.batch, io.n_vocab = logits.data_ptr(), V, rows, V
            io.tokens, io.tokens_ld, io.cur_len = tokens.data_ptr(), ld, begin + m
            io.sample_begin, io.eot, io.repetition_penalty, io.no_repeat_ngram_size = begin, eot, P, N
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                native.check(lib.wm_repeat_controls(C.byref(io), s.cuda_stream), "wm_repeat_controls")
                s.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=s):
                    for _ in range(200):
                        native.check(lib.wm_repeat_controls(C.byref(io), s.cuda_stream), "wm_repeat_controls")
                graph.replay()
                s.synchronize()
                best = float("inf")
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    graph.replay()
                    e1.record(s)
                    s.synchronize()
                    best = min(best, e0.elapsed_time(e1) * 1e3 / 200)
            report["kernel_us"][f"{rows}x{m}"] = best
            print(f"wm_repeat_controls alone, {rows} rows, m = {m}, ({P}, {N}): {best:.2f} us per launch (200 in one replayed graph)", flush=True)
print(json.dumps(report))
