"""Parallel sections, two figures.  Reports only.
  (a) wm_section_cuts (default SectionOptions at the large-v2 window: lo 1500, hi 3000, h 10) on one 2-hour mel and on 64
      ten-minute mels: the launch (median, min and max of 20, device events) with the bytes of mel it reads per second, beside the SAME cuts
      from torch expressions on the device plus the host loop that needs one device-to-host copy per cut (median of 3, host clock
      around a synchronise); the two results are compared;
  (b) one synthetic one-hour file through transcribe.transcribe_mel without and with `sections`, same options, sample_len fixed,
      fallback off: wall time (runs alternate, after a warm-up of each), rounds, decoder calls.
      python scripts/bench_sections.py [tokens=32] [minutes=60] [engine_dir]
Without an engine directory: the large-v2 int8 engine with seeded random weights that bench.py builds (kept under
/tmp/wm_bench_engines when it exists)."""
import argparse, json, os, sys, time
from pathlib import Path
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "eddie-wang-hackathon2023_amd")]
import native  # noqa: F401
import torch
import sections as S
import transcribe as T
from decoding import DecodingOptions, WhisperDecoding
from encoding import WhisperEncoding

TOKENS = int(sys.argv[1]) if len(sys.argv) > 1 else 32
MINUTES = int(sys.argv[2]) if len(sys.argv) > 2 else 60
W, M = 3000, 80
OPTS = S.SectionOptions()
LO, HI, H = OPTS.frames(W, M)
report = {}


def speechlike_mel(frames, seed):
    """Noise in the log-mel's usual range with a pause (the floor, 0.3 .. 0.6 s) every 4 .. 20 s, and W frames of silence behind."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    mel = (torch.randn((M, frames + W), generator=g, device="cuda") * 0.5).clamp_(-0.5, 1.5).half()
    cpu = torch.Generator().manual_seed(seed)
    t = 0
    while t < frames:
        t += int(torch.randint(400, 2000, (1,), generator=cpu))
        n = int(torch.randint(30, 60, (1,), generator=cpu))
        mel[:, t:t + n] = -0.5
        t += n
    mel[:, frames:] = -0.5
    return mel


def gpu_ms(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        t0.record(); fn(); t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def torch_cuts(mel, F):
    """sections.py in torch on the device; the walk over the cuts is a host loop with one .item() per cut."""
    x = mel[:, :F].float()
    x = torch.where(torch.isfinite(x), x, torch.zeros_like(x)).clamp_(-16.0, 16.0) * 1024.0
    q = torch.round(x).to(torch.int64).sum(dim=0)
    s = torch.cat([q[:1].expand(H), q, q[-1:].expand(H)]).unfold(0, 2 * H + 1, 1).sum(dim=-1)
    cuts, c = [], 0
    while F - c > HI:
        piece = s[c + LO: c + HI + 1]
        c = c + LO + (piece.numel() - 1 - int(torch.argmin(piece.flip(0))))
        cuts.append(c)
    return cuts


# ---- (a) the kernel beside torch + host loop
lib, stream = native.load_library(), torch.cuda.current_stream().cuda_stream
for name, frames_list in (("one 2-hour mel", [720000]), ("64 ten-minute mels", [60000 - 7 * (i % 9) for i in range(64)])):
    mels = [speechlike_mel(F, 100 + i) for i, F in enumerate(frames_list)]
    n, total = len(mels), sum(frames_list)
    cuts_ld = max(frames_list) // LO
    table = torch.tensor([[m.data_ptr() for m in mels], [m.shape[1] for m in mels], frames_list], dtype=torch.int64, device="cuda")
    ld, content = table[1].to(torch.int32), table[2].to(torch.int32)
    ws_bytes = int(lib.wm_section_cuts_workspace_bytes(n, total))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out = torch.empty(n * (1 + cuts_ld), dtype=torch.int32, device="cuda")
    launch = lambda: native.check(lib.wm_section_cuts(table[0].data_ptr(), ld.data_ptr(), content.data_ptr(), n, M, LO, HI, H,  # noqa: E731
                                                      out[n:].data_ptr(), cuts_ld, out.data_ptr(), ws.data_ptr(), ws_bytes, total, stream))
    ms_k, ms_k_min, ms_k_max = gpu_ms(launch)
    got = T.section_cuts(mels, frames_list, OPTS, window=W)

    def wrapper_wall():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        T.section_cuts(mels, frames_list, OPTS, window=W)
        return (time.perf_counter() - t0) * 1e3

    def torch_wall():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = [torch_cuts(m, F) for m, F in zip(mels, frames_list)]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, res

    walls = sorted(wrapper_wall() for _ in range(5))
    ms_w = walls[2]
    torch_wall()
    runs = sorted((torch_wall() for _ in range(3)), key=lambda r: r[0])
    ms_t, want = runs[1]
    assert got == want, "the kernel and the torch expression disagree"
    read = 2 * M * total
    report[name] = dict(files=n, frames=total, cuts=sum(len(c) for c in got), kernel_ms=ms_k, kernel_ms_min_max=[ms_k_min, ms_k_max],
                        mel_read_GBps=read / ms_k / 1e6, section_cuts_call_ms=ms_w, section_cuts_call_ms_min_max=[walls[0], walls[-1]],
                        torch_and_host_loop_ms=ms_t, torch_and_host_loop_ms_min_max=[runs[0][0], runs[-1][0]])
    print(f"wm_section_cuts, {name} ({total} frames x {M} bins, {sum(len(c) for c in got)} cuts; lo {LO} hi {HI} h {H}): launch {ms_k:.3f} ms "
          f"(median of 20 single calls between two events, {ms_k_min:.3f} .. {ms_k_max:.3f}) = {read / ms_k / 1e6:.0f} GB/s of mel READ over all "
          f"four kernels (wm_mel_windows' 4.6 TB/s counts bytes read + written; a mel below the last-level cache's size may be served from "
          f"it on the repeats); transcribe.section_cuts (table, launch, copy back) {ms_w:.2f} ms wall ({walls[0]:.2f} .. {walls[-1]:.2f}, 5 calls); "
          f"torch on the device + host loop {ms_t:.1f} ms wall (median of 3, {runs[0][0]:.1f} .. {runs[-1][0]:.1f}), the same cuts", flush=True)
    del mels, ws, out

# ---- (b) one long file without and with sections (minutes = 0: the kernel figures only, e.g. under a kernel trace)
if MINUTES == 0:
    print(json.dumps(report))
    sys.exit(0)
if len(sys.argv) > 3:
    eng = Path(sys.argv[3])
else:
    eng = Path("/tmp/wm_bench_engines/large-v2-int8-seed0")
    if not (eng / "decoder_config.json").exists():
        import bench
        eng.parent.mkdir(parents=True, exist_ok=True)
        bench.build_engines(argparse.Namespace(model="large-v2", config="int8", seed=0), eng)
enc = WhisperEncoding(eng)
# an instance per form: each keeps the buffer set and the graphs of its own batch size
decs = {label: WhisperDecoding(eng, options=DecodingOptions(sample_len=TOKENS, language="en")) for label in ("without", "with")}
assert 2 * decs["with"].decoder_config["num_audio_ctx"] == W
F = MINUTES * 60 * 100
mel = speechlike_mel(F, 1)
kw = dict(temperatures=(0.0,), compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None)


def job(sections, trace=None):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = T.transcribe_mel(enc, decs["without" if sections is None else "with"], [mel], [F], sections=sections, trace=trace, **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


figures = {}
for label, sections in (("without", None), ("with", OPTS)):            # warm-up of each form (graphs, workspaces) with its trace
    trace = []
    _, res = job(sections, trace)
    figures[label] = dict(rounds=trace[-1]["round"] + 1, decoder_calls=len(trace), rows=len(trace[0]["rows"]),
                          windows=sum(sum(e["live"]) for e in trace), segments=len(res[0]["segments"]), wall_ms=[])
    if sections is not None:
        figures[label]["sections"] = len(res[0]["sections"])
for _ in range(2):
    for label, sections in (("without", None), ("with", OPTS)):
        figures[label]["wall_ms"].append(job(sections)[0])
report["job"] = dict(engine=str(eng), minutes=MINUTES, frames=F, tokens=TOKENS, **{k: v for k, v in figures.items()})
a, b = figures["without"], figures["with"]
print(f"one file of {MINUTES} min ({F} frames), sample_len {TOKENS}, fallback off: without sections {min(a['wall_ms']):.0f} ms "
      f"(runs {[round(v) for v in a['wall_ms']]}; {a['windows']} windows in {a['rounds']} rounds of {a['rows']} row, {a['decoder_calls']} decoder calls); "
      f"with sections {min(b['wall_ms']):.0f} ms (runs {[round(v) for v in b['wall_ms']]}; {b['sections']} sections, {b['windows']} windows in "
      f"{b['rounds']} rounds of {b['rows']} rows, {b['decoder_calls']} decoder calls): {min(a['wall_ms']) / min(b['wall_ms']):.1f} x")
print(json.dumps(report))
