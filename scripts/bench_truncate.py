"""What top_k / top_p / min_p cost in the device decode loop: ms per token step of the sampling loop (temperature 0.6) at 1, 8, 64 and
576 rows with the controls off (wm_greedy_step) and with (50, 0.95, 0) (wm_sample_step in its place), each replayed from captured
graphs; then the two kernels alone on the same rows -- N(0, 1.5) logits and a peaked set -- for every combination of controls, which
shows what each pass of the selection costs.  large-v2 shape, weight-only int8 + int8 KV, random weights, `ignore_eot` (a fixed number
of steps).  Engines: the ones `bench.py --engine-cache /tmp/wm_bench_engines` keeps (built here when they are missing).

    python scripts/bench_truncate.py [tokens=128] [--rows 1,8,64,576] [--reps 5] [--off-only] [--no-kernel] [--no-loop]

--off-only runs the defaults alone and names no option of the controls: the same file measures a tree from before they existed
(DESIGN.md section 5l)."""
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
ap.add_argument("--no-loop", action="store_true")
ap.add_argument("--tag", type=str, default="")
args = ap.parse_args()
T, ROWS = args.tokens, [int(r) for r in args.rows.split(",")]
TEMP, K, P, Q = 0.6, 50, 0.95, 0.0
dims = synthetic.DIMS["large-v2"]
report = {"tokens": T, "tag": args.tag, "steps": {}}


def step_ms(dec, feats):
    """ms per token step: a whole main_loop call (prefill, then T - 1 replayed steps) over T, the median of --reps calls after two
    that capture the graphs.  The cross K/V of the unchanged features are projected once, outside the clock."""
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


if not args.no_loop:
    eng = Path("/tmp/wm_bench_engines/large-v2-int8-seed0")
    if not (eng / "decoder_config.json").exists():
        import bench
        eng.parent.mkdir(parents=True, exist_ok=True)
        bench.build_engines(argparse.Namespace(model="large-v2", config="int8", seed=0), eng)
    enc = WhisperEncoding(eng)
    for rows in ROWS:
        g = torch.Generator(device="cuda").manual_seed(1234)
        mel = (torch.randn((rows, dims["n_mels"], 2 * dims["n_audio_ctx"]), generator=g, device="cuda") * 0.5).clamp_(-0.5, 1.5).half()
        xa = enc.get_audio_features_async(mel)
        torch.cuda.synchronize()
        del mel
        line = {}
        for name, controls in (("off", {}),) + (() if args.off_only else (("on", dict(top_k=K, top_p=P, min_p=Q)),)):
            dec = WhisperDecoding(eng, options=DecodingOptions(sample_len=T, language="en", temperature=TEMP, **controls))
            line[name] = step_ms(dec, xa)
            dec._state.clear()
            del dec
            torch.cuda.empty_cache()
        report["steps"][rows] = line
        msg = f"{rows:4d} rows, {T} tokens, temperature {TEMP}: controls off {line['off'][0]:.4f} ms per token step (min {line['off'][1]:.4f}, max {line['off'][2]:.4f})"
        if "on" in line:
            msg += (f" | ({K}, {P}, {Q}) {line['on'][0]:.4f} ms (min {line['on'][1]:.4f}, max {line['on'][2]:.4f}): "
                    f"+{(line['on'][0] - line['off'][0]) * 1e3:.1f} us, x {line['on'][0] / line['off'][0]:.4f}")
        print(msg, flush=True)
        del xa
        torch.cuda.empty_cache()

if not args.off_only and not args.no_kernel:
    # the kernels alone: 100 launches captured into one graph (how the loop issues them), replayed, between two events
    import ctypes as C
    import truncation
    lib = native.load_library()
    V, ld, begin, cur = dims["n_vocab"], dims["n_text_ctx"] + 1, 3, 40
    eot, tb = 50257, 50364
    report["kernel_us"] = {}

    def timed(call, io):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            native.check(call(C.byref(io), s.cuda_stream))
            s.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                for _ in range(100):
                    native.check(call(C.byref(io), s.cuda_stream))
            graph.replay()
            s.synchronize()
            best = float("inf")
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                graph.replay()
                e1.record(s)
                s.synchronize()
                best = min(best, e0.elapsed_time(e1) * 1e3 / 100)
        return best

    for rows in ROWS:
        for kind in ("normal", "peaked"):
            g = torch.Generator(device="cuda").manual_seed(7)
            logits = torch.randn((rows, V), device="cuda", generator=g) * 1.5
            if kind == "peaked":
                logits[:, 1000] += 30.0
            logits[:, tb:] -= 8.0                                 # (text stays in play: the whole vocabulary is selected from)
            logits = logits.half()
            tokens = torch.randint(1000, 2000, (rows, ld), device="cuda", dtype=torch.int32)
            sums = torch.zeros(rows, device="cuda")
            n_done = torch.zeros(1, dtype=torch.int32, device="cuda")

            def fill(g_io):
                g_io.logits, g_io.row_stride, g_io.batch, g_io.n_vocab = logits.data_ptr(), V, rows, V
                g_io.tokens, g_io.tokens_ld, g_io.cur_len = tokens.data_ptr(), ld, cur
                g_io.sum_logprobs, g_io.n_done = sums.data_ptr(), n_done.data_ptr()
                g_io.sample_begin, g_io.eot, g_io.timestamp_begin = begin, eot, tb
                g_io.max_initial_timestamp_index, g_io.apply_rules = 50, 1
                g_io.temperature, g_io.seed = TEMP, 99

            gio = native.WmGreedyIO()
            fill(gio)
            line = {"greedy": timed(lib.wm_greedy_step, gio)}
            for name, (k, p, q) in (("off", (0, 1.0, 0.0)), ("k", (K, 1.0, 0.0)), ("p", (0, P, 0.0)), ("q", (0, 1.0, 0.05)), ("kp", (K, P, Q))):
                sio = native.WmSampleIO()
                fill(sio.g)
                c, p16, gap = truncation.params(TEMP, p, q)
                sio.top_k, sio.exp2_scale, sio.top_p_q16, sio.min_p_gap = k, float(c), p16, float(gap)
                line[name] = timed(lib.wm_sample_step, sio)
            report["kernel_us"][f"{rows}x{kind}"] = line
            print(f"{rows:4d} rows, {kind:6s}: wm_greedy_step {line['greedy']:.2f} us | wm_sample_step off {line['off']:.2f}, top_k {line['k']:.2f}, "
                  f"top_p {line['p']:.2f}, min_p {line['q']:.2f}, ({K}, {P}, {Q}) {line['kp']:.2f} us per launch (100 in one replayed graph)", flush=True)
print(json.dumps(report))
