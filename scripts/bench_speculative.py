"""What a round of speculative decoding costs: reports, not pass marks.  One board, one session, the variants
take turns, `--reps` sessions each.

  * a `large-v3` main engine (weight-only int8 + int8 KV, random weights) with a `large-v3-turbo` draft, with a `distil-large-v3` draft
    and as its own draft, one row, draft_tokens 3: the whole loop on the wall clock -> ms per round, tokens per round;
  * the parts of a round between device events, each repeated on a cache that holds 40 tokens: the draft's 1-token step and 2-token
    catch-up pass (decoder pass + wm_greedy_step), the verify pass of 2 / 3 / 4 tokens, wm_verify_step (both launches), and the copy
    of (n_accept, done) back to the host on the host clock;
  * the plain one-row token step of the main engine in the same session (the replayed graphs of `main_loop`, and the eager pass +
    wm_greedy_step the round is built from);
  * from those: tokens per round at break-even = (3 draft steps + the 4-token pass + wm_verify_step + the copy) / the plain step, all from
    the parts; the wall clock of a whole call, which also holds both prefills and ends at EOT, is reported beside it and not used;
  * wm_verify_step alone at n_pos 1 .. 4 beside wm_greedy_step, 100 launches in one replayed graph each.

Random weights give an acceptance near 0 with a draft of other weights (the worst case) and near 1 with the engine as its own draft
(the cost side only: that draft is as dear as the engine).  No speed-up on speech is claimed from these numbers: there are no trained
weights here.

    python scripts/bench_speculative.py [--tokens 96] [--reps 3] [--model large-v3] [--out figures.json] [--no-loop] [--no-kernel]

Engines: the ones `bench.py --engine-cache /tmp/wm_bench_engines` keeps (built here when they are missing)."""
import argparse, ctypes as C, json, os, statistics, sys, time
from pathlib import Path
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "eddie-wang-hackathon2023_amd")]
import native  # noqa: F401
import torch
import synthetic
from decoding import DecodingOptions, WhisperDecoding
from encoding import WhisperEncoding

ap = argparse.ArgumentParser()
ap.add_argument("--tokens", type=int, default=96)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--model", type=str, default="large-v3")
ap.add_argument("--drafts", type=str, default="large-v3-turbo,distil-large-v3")
ap.add_argument("--cache", type=str, default="/tmp/wm_bench_engines")
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--no-loop", action="store_true")
ap.add_argument("--no-kernel", action="store_true")
args = ap.parse_args()
T, PAST, N = args.tokens, 40, 50
report = {"tokens": T, "model": args.model, "loop": {}, "parts_ms": {}, "kernel_us": {}}


def engine(model):
    eng = Path(args.cache) / f"{model}-int8-seed0"
    if not (eng / "decoder_config.json").exists():
        import bench
        print(f"building {model} (int8 weight-only + int8 KV, random weights) into {eng}", flush=True)
        eng.parent.mkdir(parents=True, exist_ok=True)
        bench.build_engines(argparse.Namespace(model=model, config="int8", seed=0), eng)
    return eng


def events_ms(fn, n=N):
    """ms per call of `fn` between two device events: n calls behind 5 warm-up calls."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def med(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4))


if not args.no_loop:
    dims = synthetic.DIMS[args.model]
    main_eng = engine(args.model)
    drafts = {name: engine(name) for name in args.drafts.split(",") if name}
    drafts["itself"] = main_eng
    enc = WhisperEncoding(main_eng)
    g = torch.Generator(device="cuda").manual_seed(1234)
    mel = (torch.randn((1, dims["n_mels"], 2 * dims["n_audio_ctx"]), generator=g, device="cuda") * 0.5).clamp_(-0.5, 1.5).half()
    xa = enc.get_audio_features(mel)
    torch.cuda.synchronize()
    del enc
    torch.cuda.empty_cache()
    opts = DecodingOptions(sample_len=T, language="en")
    plain = WhisperDecoding(main_eng, options=opts)
    decs = {name: WhisperDecoding(main_eng, options=opts, draft_engine_dir=d, draft_tokens=3) for name, d in drafts.items()}

    def plain_step():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plain.main_loop(xa, ignore_eot=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / T

    def rounds(dec):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.main_loop(xa)
        torch.cuda.synchronize()
        ms, s = (time.perf_counter() - t0) * 1e3, dec.speculative_stats
        return dict(ms=ms, rounds=s["rounds"][0], tokens=s["tokens"][0], proposals=s["proposals"][0], accepted=s["accepted"][0])

    for _ in range(2):                                   # warm-up: graphs captured, workspaces allocated
        plain_step()
        for dec in decs.values():
            rounds(dec)
    runs = {name: [] for name in ["plain"] + list(decs)}
    for _ in range(args.reps):                           # the variants take turns
        runs["plain"].append(plain_step())
        for name, dec in decs.items():
            runs[name].append(rounds(dec))
    report["loop"]["plain_token_step_ms"] = med(runs["plain"])
    print(f"plain loop, one row, {T} tokens (replayed graphs): {report['loop']['plain_token_step_ms']} ms per token", flush=True)
    for name in decs:
        rs = runs[name]
        # the prefill of both engines and the first token are inside the wall clock: a round's cost is read off the parts below
        line = dict(ms_per_round=med([r["ms"] / max(1, r["rounds"]) for r in rs]), ms_per_token=med([r["ms"] / r["tokens"] for r in rs]),
                    tokens_per_round=round(statistics.median([(r["tokens"] - 1) / max(1, r["rounds"]) for r in rs]), 3),
                    wall_ms=med([r["ms"] for r in rs]),
                    acceptance=round(statistics.median([r["accepted"] / max(1, r["proposals"]) for r in rs]), 3), rounds=rs[-1]["rounds"],
                    tokens=rs[-1]["tokens"])
        report["loop"][name] = line
        print(f"draft {name}: {line}", flush=True)

    # ---- the parts of a round, on the caches the loops have just filled (they hold T > PAST tokens) -------------------------------------------
    lib = native.load_library()
    cap, V = plain.decoder_config['num_text_ctx'], plain.decoder_config['vocab_size']
    sm = torch.cuda.current_stream().cuda_stream
    parts = {}

    def pass_fn(dec, st, n_new, logits):
        kv, cross, tok, pos = st['kv'], st['cross'], st['tokens'], dec.positional_embedding
        return lambda: dec.decoder_session.decoder_step(tok[:, PAST:PAST + n_new], pos[PAST:PAST + n_new], cross, kv, cap, kv, cap, logits,
                                                        PAST, sm, slot=0)

    for rep in range(args.reps):
        for name, dec in decs.items():
            st, bufs = dec._state[1], dec._spec_bufs
            dst = dec.draft._state[1]
            dview = dict(dst, tokens=st['tokens'])
            d1, d2 = pass_fn(dec.draft, dview, 1, bufs['draft_logits']), pass_fn(dec.draft, dview, 2, bufs['draft_logits'])
            greedy = lambda: dec.draft._greedy(dview, 0, 1, bufs['draft_logits'].data_ptr(), V, PAST + 1, sm, temperature=0.0)  # noqa: E731
            parts.setdefault(f"{name}: draft step (1-token pass + wm_greedy_step)", []).append(events_ms(lambda: (d1(), greedy())))
            parts.setdefault(f"{name}: draft catch-up (2-token pass + wm_greedy_step)", []).append(events_ms(lambda: (d2(), greedy())))
        dec = next(iter(decs.values()))
        st, bufs = dec._state[1], dec._spec_bufs
        for n_new in (1, 2, 3, 4):
            parts.setdefault(f"main pass of {n_new} token(s), eager", []).append(events_ms(pass_fn(dec, st, n_new, bufs['logits'])))
            verify = lambda n_new=n_new: dec._verify(st, 0, bufs['logits'], n_new, PAST + 1, bufs['pair'], bufs['ws'], sm)  # noqa: E731
            parts.setdefault(f"wm_verify_step n_pos {n_new} (both launches, eager)", []).append(events_ms(verify))
        plain_greedy = lambda: dec._greedy(st, 0, 1, bufs['logits'].data_ptr(), V, PAST + 1, sm, temperature=0.0)  # noqa: E731
        one = pass_fn(dec, st, 1, bufs['logits'])
        parts.setdefault("main token step, eager (1-token pass + wm_greedy_step)", []).append(events_ms(lambda: (one(), plain_greedy())))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(N):
            bufs['pair'].tolist()
        parts.setdefault("copy of (n_accept, done) to the host, idle queue (host clock)", []).append((time.perf_counter() - t0) * 1e3 / N)
    report["parts_ms"] = {k: med(v) for k, v in parts.items()}
    for k, v in report["parts_ms"].items():
        print(f"{k}: {v}", flush=True)
    P = {k: v["median"] for k, v in report["parts_ms"].items()}
    plain_ms = report["loop"]["plain_token_step_ms"]["median"]
    for name in decs:
        # a steady round of 3 proposals behind a rejected one: 3 draft steps (the first a 1-token catch-up), one 4-token pass, the verify step, the copy
        est = (3 * P[f"{name}: draft step (1-token pass + wm_greedy_step)"] + P["main pass of 4 token(s), eager"]
               + P["wm_verify_step n_pos 4 (both launches, eager)"] + P["copy of (n_accept, done) to the host, idle queue (host clock)"])
        measured = report["loop"][name]["ms_per_round"]["median"]
        # the headline comes from the parts: the wall clock of a whole call also holds both prefills and the first token step
        report["loop"][name].update(round_from_parts_ms=round(est, 4), break_even_tokens_per_round=round(est / plain_ms, 3),
                                    wall_over_rounds_over_plain_step=round(measured / plain_ms, 3))
        print(f"draft {name}: a round of 3 from its parts {est:.3f} ms; plain step {plain_ms:.3f} ms -> break-even at {est / plain_ms:.2f} tokens per "
              f"round (whole call over its rounds, prefills included: {measured:.3f} ms)", flush=True)
    for dec in list(decs.values()) + [plain]:
        dec._state.clear()
    torch.cuda.empty_cache()

if not args.no_kernel:
    lib = native.load_library()
    V, ld, begin, cur, eot, tb = synthetic.DIMS[args.model]["n_vocab"], 449, 3, 40, 50257, 50365

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

    for rows in (1, 8):
        gen = torch.Generator(device="cuda").manual_seed(7)
        logits = torch.randn((rows, 4, V), device="cuda", generator=gen) * 1.5
        logits[:, :, tb:] -= 8.0
        logits = logits.half()
        tokens = torch.randint(1000, 2000, (rows, ld), device="cuda", dtype=torch.int32)
        sums = torch.zeros(rows, device="cuda")
        n_done, n_acc = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(rows, dtype=torch.int32, device="cuda")
        ws = torch.empty(max(8, lib.wm_verify_workspace_bytes(rows, 4)), dtype=torch.uint8, device="cuda")

        def fill(g_io, stride):
            g_io.logits, g_io.row_stride, g_io.batch, g_io.n_vocab = logits.data_ptr(), stride, rows, V
            g_io.tokens, g_io.tokens_ld, g_io.cur_len = tokens.data_ptr(), ld, cur
            g_io.sum_logprobs, g_io.n_done = sums.data_ptr(), n_done.data_ptr()
            g_io.sample_begin, g_io.eot, g_io.timestamp_begin = begin, eot, tb
            g_io.max_initial_timestamp_index, g_io.apply_rules = 50, 1
            g_io.temperature, g_io.seed = 0.0, 99

        # make every proposal the token its position elects: each eager call keeps what matched and corrects the first slot that did
        # not, so after four calls slots cur .. cur + 3 hold the elected tokens and every later launch writes all n_pos slots (the most
        # work the second launch does); checked behind the timing
        vio = native.WmVerifyIO()
        fill(vio.g, 4 * V)
        vio.pos_stride, vio.n_pos, vio.n_accept, vio.workspace = V, 4, n_acc.data_ptr(), ws.data_ptr()
        for _ in range(5):
            native.check(lib.wm_verify_step(C.byref(vio), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert n_acc.tolist() == [4] * rows, n_acc.tolist()
        gio = native.WmGreedyIO()
        fill(gio, 4 * V)
        line = {"wm_greedy_step": round(timed(lib.wm_greedy_step, gio), 2)}
        for n_pos in (1, 2, 3, 4):
            vio = native.WmVerifyIO()
            fill(vio.g, 4 * V)
            vio.pos_stride, vio.n_pos, vio.n_accept, vio.workspace = V, n_pos, n_acc.data_ptr(), ws.data_ptr()
            line[f"wm_verify_step n_pos {n_pos}"] = round(timed(lib.wm_verify_step, vio), 2)
            assert n_acc.tolist() == [n_pos] * rows, (n_pos, n_acc.tolist())
        report["kernel_us"][rows] = line
        print(f"{rows} row(s), us per call (100 in one replayed graph): {line}", flush=True)

text = json.dumps(report, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
