"""Skip silence, two figures.  Reports only.
  (a) wm_speech_spans and wm_mel_gather (default SpeechOptions at the large-v2 window: h 10, step 205, permille 100, min_silence 200,
      min_speech 25, pad 40) on one 2-hour mel and on 64 ten-minute mels, quiet stretches planted over half of the frames: each
      launch alone (median, min and max of 20, device events; DESIGN.md section 6: a warm-up of 3, every call between its own pair
      of events) with the bytes it reads plus writes per second, beside the SAME work from torch expressions on the device with a
      host loop -- the spans from a sort and one copy back, the packed mel from `torch.cat` of slices -- (median of 3, host clock
      around a synchronise); the results are compared.  hipMemcpyAsync of the packed bytes (a device-to-device copy_) stands
      beside the gather as the rate a plain copy reaches on the same buffers;
  (b) one synthetic one-hour file through transcribe.transcribe_mel without and with `speech`, same options, sample_len fixed,
      fallback off: wall time (runs alternate, after a warm-up of each), windows, rounds.
      python scripts/bench_speech.py [tokens=32] [minutes=60] [engine_dir]
Without an engine directory: the large-v2 int8 engine with seeded random weights that bench.py builds (kept under
/tmp/wm_bench_engines when it exists)."""
import argparse, json, os, sys, time
from pathlib import Path
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "eddie-wang-hackathon2023_amd")]
import native  # noqa: F401
import torch
import speech as SP
import transcribe as T
from decoding import DecodingOptions, WhisperDecoding
from encoding import WhisperEncoding

TOKENS = int(sys.argv[1]) if len(sys.argv) > 1 else 32
MINUTES = int(sys.argv[2]) if len(sys.argv) > 2 else 60
W, M = 3000, 80
OPTS = SP.SpeechOptions()
H, STEP, PERMILLE, MIN_SILENCE, MIN_SPEECH, PAD = OPTS.frames(W, M)
report = {}


def half_quiet_mel(frames, seed):
    """Noise in the log-mel's usual range; quiet stretches of 3 .. 30 s alternate with loud ones of the same lengths, so about half
    of the frames are quiet; W frames of silence behind."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    mel = (torch.randn((M, frames + W), generator=g, device="cuda") * 0.5).clamp_(-0.5, 1.5).half()
    cpu = torch.Generator().manual_seed(seed)
    t = 0
    while t < frames:
        t += int(torch.randint(300, 3000, (1,), generator=cpu))
        n = int(torch.randint(300, 3000, (1,), generator=cpu))
        mel[:, t:t + n] = -1.5
        t += n
    mel[:, frames:] = -1.5
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


def torch_spans(mel, F):
    """speech.py in torch on the device, then rule 4 on the host from one copy of the flags' edges."""
    x = mel[:, :F].float()
    x = torch.where(torch.isfinite(x), x, torch.zeros_like(x)).clamp_(-16.0, 16.0) * 1024.0
    q = torch.round(x).to(torch.int64).sum(dim=0)
    s = torch.cat([q[:1].expand(H), q, q[-1:].expand(H)]).unfold(0, 2 * H + 1, 1).sum(dim=-1)
    floor = torch.sort(s).values[min(F - 1, F * PERMILLE // 1000)]
    v = (s - floor >= M * (2 * H + 1) * STEP).to(torch.int8)
    edges = torch.nonzero(torch.diff(v, prepend=v.new_zeros(1), append=v.new_zeros(1))).flatten().cpu().tolist()
    out, joined = [], []
    for a, b in zip(edges[0::2], edges[1::2]):
        if joined and a - joined[-1][1] < MIN_SILENCE:
            joined[-1][1] = b
        else:
            joined.append([a, b])
    for a, b in joined:
        if b - a < MIN_SPEECH:
            continue
        a, b = max(0, a - PAD), min(F, b + PAD)
        if out and a <= out[-1][1]:
            out[-1][1] = b
        else:
            out.append([a, b])
    return [(a, b) for a, b in out]


def torch_pack(mel, spans):
    return torch.cat([mel[:, a:b] for a, b in spans] + [mel[:, -1:].expand(-1, W)], dim=1)


def wall_ms(fn, reps=3):
    fn()
    runs = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        runs.append(((time.perf_counter() - t0) * 1e3, res))
    runs.sort(key=lambda r: r[0])
    return runs[len(runs) // 2][0], runs[0][0], runs[-1][0], runs[len(runs) // 2][1]


# ---- (a) the kernels beside torch + host loop
lib, stream = native.load_library(), torch.cuda.current_stream().cuda_stream
for name, frames_list in (("one 2-hour mel", [720000]), ("64 ten-minute mels", [60000 - 7 * (i % 9) for i in range(64)])):
    mels = [half_quiet_mel(F, 100 + i) for i, F in enumerate(frames_list)]
    n, total = len(mels), sum(frames_list)
    spans_ld = (max(frames_list) + MIN_SILENCE) // (1 + MIN_SILENCE)
    table = torch.tensor([[m.data_ptr() for m in mels], [m.shape[1] for m in mels], frames_list], dtype=torch.int64, device="cuda")
    ld, content = table[1].to(torch.int32), table[2].to(torch.int32)
    ws_bytes = int(lib.wm_speech_spans_workspace_bytes(n, total))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out = torch.empty(n * (1 + 2 * spans_ld), dtype=torch.int32, device="cuda")
    find = lambda: native.check(lib.wm_speech_spans(table[0].data_ptr(), ld.data_ptr(), content.data_ptr(), n, M, H, STEP, PERMILLE,  # noqa: E731
                                                    MIN_SILENCE, MIN_SPEECH, PAD, out[n:].data_ptr(), spans_ld, out.data_ptr(),
                                                    ws.data_ptr(), ws_bytes, total, stream))
    ms_s = gpu_ms(find)
    spans = T.speech_spans(mels, frames_list, OPTS, window=W)
    packed, P = T.packed_mels(mels, frames_list, spans, W)
    dst = torch.tensor([p.data_ptr() for p in packed], dtype=torch.int64, device="cuda")
    dst_ld = torch.tensor([p.shape[1] for p in packed], dtype=torch.int32, device="cuda")
    pack = lambda: native.check(lib.wm_mel_gather(table[0].data_ptr(), ld.data_ptr(), out[n:].data_ptr(), out.data_ptr(), spans_ld, n, M, W,  # noqa: E731
                                                  dst.data_ptr(), dst_ld.data_ptr(), stream))
    ms_g = gpu_ms(pack)
    copies = [torch.empty_like(p) for p in packed]

    def plain_copy():
        for c, p in zip(copies, packed):
            c.copy_(p)

    ms_c = gpu_ms(plain_copy)
    ms_ts = wall_ms(lambda: [torch_spans(m, F) for m, F in zip(mels, frames_list)])
    assert [list(map(tuple, s)) for s in ms_ts[3]] == spans, "the kernel and the torch expression disagree on the spans"
    ms_tp = wall_ms(lambda: [torch_pack(m, s) for m, s in zip(mels, spans)])
    assert all(torch.equal(a, b) for a, b in zip(ms_tp[3], packed)), "the kernel and torch.cat disagree on the packed mel"
    ms_w = wall_ms(lambda: T.speech_spans(mels, frames_list, OPTS, window=W), reps=5)
    moved = 2 * 2 * M * sum(p + W for p in P)                    # bytes read plus written by the gather
    read = 2 * M * total                                         # bytes of mel the span call reads
    report[name] = dict(files=n, frames=total, spans=sum(len(s) for s in spans), packed_frames=sum(P),
                        speech_spans_ms=ms_s[0], speech_spans_ms_min_max=list(ms_s[1:]), mel_read_GBps=read / ms_s[0] / 1e6,
                        speech_spans_call_ms=ms_w[0], speech_spans_call_ms_min_max=list(ms_w[1:3]),
                        mel_gather_ms=ms_g[0], mel_gather_ms_min_max=list(ms_g[1:]), gather_read_plus_written_GBps=moved / ms_g[0] / 1e6,
                        plain_copy_ms=ms_c[0], plain_copy_ms_min_max=list(ms_c[1:]), plain_copy_read_plus_written_GBps=moved / ms_c[0] / 1e6,
                        torch_spans_ms=ms_ts[0], torch_spans_ms_min_max=list(ms_ts[1:3]), torch_cat_ms=ms_tp[0], torch_cat_ms_min_max=list(ms_tp[1:3]))
    r = report[name]
    print(f"{name} ({total} frames x {M} bins; {r['spans']} spans keep {sum(P)} frames): wm_speech_spans {ms_s[0]:.3f} ms ({ms_s[1]:.3f} .. {ms_s[2]:.3f}; "
          f"median of 20 single calls between two events) = {r['mel_read_GBps']:.0f} GB/s of mel READ over all four kernels; transcribe.speech_spans "
          f"(table, launch, copy back) {ms_w[0]:.2f} ms wall ({ms_w[1]:.2f} .. {ms_w[2]:.2f}); torch + host loop {ms_ts[0]:.1f} ms wall "
          f"({ms_ts[1]:.1f} .. {ms_ts[2]:.1f}), the same spans.  wm_mel_gather {ms_g[0]:.3f} ms ({ms_g[1]:.3f} .. {ms_g[2]:.3f}) = "
          f"{r['gather_read_plus_written_GBps']:.0f} GB/s read + written; copy_ of the packed mels {ms_c[0]:.3f} ms ({ms_c[1]:.3f} .. {ms_c[2]:.3f}) = "
          f"{r['plain_copy_read_plus_written_GBps']:.0f} GB/s; torch.cat of slices {ms_tp[0]:.1f} ms wall ({ms_tp[1]:.1f} .. {ms_tp[2]:.1f}), the same bits "
          f"(wm_mel_windows' 4.6 TB/s, DESIGN.md 5d, counts bytes read + written too; a mel below the last-level cache's size may be served from it on the repeats)",
          flush=True)
    del mels, ws, out, packed, copies

# ---- (b) one long file without and with `speech` (minutes = 0: the kernel figures only, e.g. under a kernel trace)
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
dec = WhisperDecoding(eng, options=DecodingOptions(sample_len=TOKENS, language="en"))
assert 2 * dec.decoder_config["num_audio_ctx"] == W
F = MINUTES * 60 * 100
mel = half_quiet_mel(F, 1)
kw = dict(temperatures=(0.0,), compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None)


def job(speech, trace=None):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = T.transcribe_mel(enc, dec, [mel], [F], speech=speech, trace=trace, **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


figures = {}
for label, speech in (("without", None), ("with", OPTS)):            # warm-up of each form (graphs, workspaces) with its trace
    trace = []
    _, res = job(speech, trace)
    figures[label] = dict(rounds=trace[-1]["round"] + 1, decoder_calls=len(trace), windows=sum(sum(e["live"]) for e in trace),
                          segments=len(res[0]["segments"]), wall_ms=[])
    if speech is not None:
        figures[label]["spans"] = len(res[0]["speech"])
        figures[label]["speech_seconds"] = sum(b - a for a, b in res[0]["speech"])
for _ in range(2):
    for label, speech in (("without", None), ("with", OPTS)):
        figures[label]["wall_ms"].append(job(speech)[0])
report["job"] = dict(engine=str(eng), minutes=MINUTES, frames=F, tokens=TOKENS, **figures)
a, b = figures["without"], figures["with"]
assert b["windows"] < a["windows"], "the filtered run must decode fewer windows"
print(f"one file of {MINUTES} min ({F} frames), sample_len {TOKENS}, fallback off: without speech {min(a['wall_ms']):.0f} ms "
      f"(runs {[round(v) for v in a['wall_ms']]}; {a['windows']} windows in {a['rounds']} rounds); with speech {min(b['wall_ms']):.0f} ms "
      f"(runs {[round(v) for v in b['wall_ms']]}; {b['spans']} spans keep {b['speech_seconds']:.0f} s, {b['windows']} windows in {b['rounds']} rounds): "
      f"{min(a['wall_ms']) / min(b['wall_ms']):.2f} x")
print(json.dumps(report))
