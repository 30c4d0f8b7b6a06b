"""What hotwords / sequence_bias cost in the device decode loop: ms per token step of the greedy loop at 1, 8, 64 and 576 rows with the
options off and with 100 hotwords of 4 tokens (400 items) -- one extra launch, wm_sequence_bias, in front of every token step -- each
replayed from captured graphs; then the kernel's own time at histories of 16 and 223 tokens.  large-v2 shape, weight-only int8 +
int8 KV, random weights, `ignore_eot` (a fixed number of steps).  Engines: the ones `bench.py --engine-cache /tmp/wm_bench_engines`
keeps (built here when they are missing).

    python scripts/bench_bias.py [tokens=128] [--rows 1,8,64,576] [--reps 5] [--off-only] [--no-kernel] [--tree DIR]

--off-only runs the defaults alone and names no option of the bias: with --tree DIR (the root of another checkout, built) the same
file measures a tree from before the options existed, for the comparison that matters -- with the defaults nothing is launched, so
the step time must not move: run the two alternately in one session and compare the difference with the spread of either's own runs
(DESIGN.md section 5k)."""
import argparse, json, os, statistics, sys, time
from pathlib import Path
ap = argparse.ArgumentParser()
ap.add_argument("tokens", type=int, nargs="?", default=128)
ap.add_argument("--rows", type=str, default="1,8,64,576")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--off-only", action="store_true")
ap.add_argument("--no-kernel", action="store_true")
ap.add_argument("--tree", type=str, default=None)
ap.add_argument("--tag", type=str, default="")
args = ap.parse_args()
ROOT = os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "eddie-wang-hackathon2023_amd")]
import native  # noqa: E402,F401
import torch  # noqa: E402
import synthetic  # noqa: E402
from decoding import DecodingOptions, WhisperDecoding  # noqa: E402
from encoding import WhisperEncoding  # noqa: E402

T, ROWS = args.tokens, [int(r) for r in args.rows.split(",")]
N_HOT, HOT_LEN = 100, 4
# 100 phrases of 4 text tokens, every token distinct: 400 items, 300 prefix tokens
HOTWORDS = tuple(tuple(range(1000 + HOT_LEN * i, 1000 + HOT_LEN * (i + 1))) for i in range(N_HOT))

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


report = {"tokens": T, "tag": args.tag, "tree": ROOT if args.tree else "this", "steps": {}}
for rows in ROWS:
    g = torch.Generator(device="cuda").manual_seed(1234)
    mel = (torch.randn((rows, dims["n_mels"], 2 * dims["n_audio_ctx"]), generator=g, device="cuda") * 0.5).clamp_(-0.5, 1.5).half()
    xa = enc.get_audio_features_async(mel)
    torch.cuda.synchronize()
    del mel
    line = {}
    for name, bias in (("off", {}),) + (() if args.off_only else (("on", dict(hotwords=HOTWORDS)),)):
        dec = WhisperDecoding(eng, options=DecodingOptions(sample_len=T, language="en", **bias))
        line[name] = step_ms(dec, xa)
        dec._state.clear()
        del dec
        torch.cuda.empty_cache()
    report["steps"][rows] = line
    msg = f"{rows:4d} rows, {T} tokens: bias off {line['off'][0]:.4f} ms per token step (min {line['off'][1]:.4f}, max {line['off'][2]:.4f})"
    if "on" in line:
        msg += (f" | {N_HOT} hotwords of {HOT_LEN} tokens {line['on'][0]:.4f} ms (min {line['on'][1]:.4f}, max {line['on'][2]:.4f}): "
                f"+{(line['on'][0] - line['off'][0]) * 1e3:.1f} us, x {line['on'][0] / line['off'][0]:.4f}")
    print(msg, flush=True)
    del xa
    torch.cuda.empty_cache()

if not args.off_only and not args.no_kernel:
    # the kernel alone: 200 launches captured into one graph (how the loop issues it), replayed, between two events
    import ctypes as C
    import biasing
    lib = native.load_library()
    V, eot, ld, begin = dims["n_vocab"], 50257, dims["n_text_ctx"] + 1, 3
    table = biasing.build_table(hotwords=HOTWORDS, eot=eot)
    items = torch.zeros(4 * biasing.MAX_ITEMS, dtype=torch.int32, device="cuda")
    pool = torch.zeros(biasing.MAX_POOL, dtype=torch.int32, device="cuda")
    items[:4 * len(table)] = torch.from_numpy(table.packed.view("int32").reshape(-1).copy()).cuda()
    pool[:table.pool.size] = torch.from_numpy(table.pool.copy()).cuda()
    count = torch.tensor([len(table)], dtype=torch.int32, device="cuda")
    report["kernel_us"] = {}
    for rows in (1, 576):
        logits = (torch.randn((rows, V), device="cuda") * 4).half()
        for m in (16, 223):
            tokens = torch.randint(1000, 1000 + N_HOT * HOT_LEN, (rows, ld), device="cuda", dtype=torch.int32)    # (the hotwords' tokens: prefixes do match)
            io = native.WmBiasIO()
            io.logits, io.row_stride, io.batch, io.n_vocab = logits.data_ptr(), V, rows, V
            io.tokens, io.tokens_ld, io.cur_len = tokens.data_ptr(), ld, begin + m
            io.sample_begin, io.eot = begin, eot
            io.items, io.pool, io.n_items_dev = items.data_ptr(), pool.data_ptr(), count.data_ptr()
            io.capacity, io.pool_capacity = biasing.MAX_ITEMS, biasing.MAX_POOL
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                native.check(lib.wm_sequence_bias(C.byref(io), s.cuda_stream), "wm_sequence_bias")
                s.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=s):
                    for _ in range(200):
                        native.check(lib.wm_sequence_bias(C.byref(io), s.cuda_stream), "wm_sequence_bias")
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
            print(f"wm_sequence_bias alone, {rows} rows, m = {m}, {len(table)} items: {best:.2f} us per launch (200 in one replayed graph)", flush=True)
print(json.dumps(report))
