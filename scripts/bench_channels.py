"""Channels, three figures.  Reports only.
  (a) wm_resample_channels on ten minutes of int16 audio with 2 and 8 channels at 44.1 and 48 kHz, beside what there was before it:
      one wm_resample launch per channel over a strided mono COPY of that channel (the copies are timed with it: they are part of
      that way); median, min and max of 20, device events around each call; the rows are compared bit for bit;
  (b) wm_channel_top (default ChannelOptions at the large-v2 window: h 10) on 64 ten-minute two-channel recordings and on one
      two-hour one, gate off and gate on (bleed_db 12; the mels are restored before every gated call, outside the events), with
      the bytes of mel it reads per second, beside the SAME rule as torch expressions on the device (median of 3, host clock
      around a synchronise); `top` is compared;
  (c) one synthetic one-hour two-channel recording, each channel quiet over the complementary half, through transcribe's channel
      layer: the downmix alone, `split`, `split` with `speech`, and `label` -- windows decoded and wall seconds (runs alternate,
      after a warm-up of each).  Stated in advance: `split` with `speech` decodes about as many windows as the downmix alone.
      python scripts/bench_channels.py [tokens=32] [minutes=60] [engine_dir]
Without an engine directory: the large-v2 int8 engine with seeded random weights that bench.py builds (kept under
/tmp/wm_bench_engines when it exists).  minutes = 0: (a) and (b) only."""
import argparse, json, os, sys, time
from pathlib import Path
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "eddie-wang-hackathon2023_amd")]
import native  # noqa: F401
import torch
import channels as CH
import speech as SP
import transcribe as T
import whisper_utils as wu
from channels import ChannelOptions
from decoding import DecodingOptions, WhisperDecoding
from encoding import WhisperEncoding

TOKENS = int(sys.argv[1]) if len(sys.argv) > 1 else 32
MINUTES = int(sys.argv[2]) if len(sys.argv) > 2 else 60
W, M = 3000, 80
report = {}
lib, stream = native.load_library(), torch.cuda.current_stream().cuda_stream


def gpu_ms(fn, reps=20, warm=3, before=None):
    for _ in range(warm):
        before and before()
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        before and before()
        t0.record(); fn(); t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


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


# ---- (a) the channel form of the resampler beside one mono launch per channel
for rate in (44100, 48000):
    L, Mr, half, table = wu._device_table(rate, torch.device("cuda", torch.cuda.current_device()))
    for C in (2, 8):
        n_in = 600 * rate
        n_out = -(-n_in * L // Mr)
        g = torch.Generator(device="cuda").manual_seed(rate + C)
        pcm = torch.randint(-2 ** 15, 2 ** 15, (n_in, C), generator=g, device="cuda", dtype=torch.int32).to(torch.int16)
        out = torch.empty((C, n_out), dtype=torch.float32, device="cuda")
        ref = torch.empty((C, n_out), dtype=torch.float32, device="cuda")
        one = lambda: native.check(lib.wm_resample_channels(pcm.data_ptr(), 1, C, n_in, 2.0 ** -15, table.data_ptr(), L, Mr, half,  # noqa: E731
                                                            out.data_ptr(), n_out, n_out, stream))

        def per_channel():
            for c in range(C):
                mono = pcm[:, c].contiguous()
                native.check(lib.wm_resample(mono.data_ptr(), 1, 1, n_in, 2.0 ** -15, table.data_ptr(), L, Mr, half, ref[c].data_ptr(), n_out, stream))

        ms_one, ms_per = gpu_ms(one), gpu_ms(per_channel)
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), "the channel form and the mono launches disagree"
        name = f"resample {C} ch {rate} Hz"
        report[name] = dict(seconds=600, channels=C, rate=rate, channels_ms=ms_one[0], channels_ms_min_max=list(ms_one[1:]),
                            per_channel_ms=ms_per[0], per_channel_ms_min_max=list(ms_per[1:]))
        print(f"{name}, ten minutes of int16: wm_resample_channels {ms_one[0]:.3f} ms ({ms_one[1]:.3f} .. {ms_one[2]:.3f}); {C} strided copies + "
              f"{C} wm_resample launches {ms_per[0]:.3f} ms ({ms_per[1]:.3f} .. {ms_per[2]:.3f}): {ms_per[0] / ms_one[0]:.2f} x; the same bits", flush=True)
        del pcm, out, ref


# ---- (b) wm_channel_top beside torch
def two_channel_mels(frames, seed):
    """Two channels of noise in the log-mel's usual range, each quiet over the stretches where the other one is loud (3 .. 30 s)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = (torch.randn((M, frames + W), generator=g, device="cuda") * 0.5).clamp_(-0.5, 1.5).half()
    b = (torch.randn((M, frames + W), generator=g, device="cuda") * 0.5).clamp_(-0.5, 1.5).half()
    cpu = torch.Generator().manual_seed(seed)
    t, who = 0, 0
    while t < frames:
        n = int(torch.randint(300, 3000, (1,), generator=cpu))
        (b if who == 0 else a)[:, t:t + n] = -1.5
        t, who = t + n, 1 - who
    a[:, frames:] = -1.5
    b[:, frames:] = -1.5
    return [a, b]


def torch_top(mels, F, h, G):
    """channels.py, rules 2 .. 4, in torch on the device: (top, gated flags)."""
    s = []
    for mel in mels:
        x = mel[:, :F].float()
        x = torch.where(torch.isfinite(x), x, torch.zeros_like(x)).clamp_(-16.0, 16.0) * 1024.0
        q = torch.round(x).to(torch.int64).sum(dim=0)
        s.append(torch.cat([q[:1].expand(h), q, q[-1:].expand(h)]).unfold(0, 2 * h + 1, 1).sum(dim=-1))
    s = torch.stack(s)
    top = torch.argmax(s, dim=0).to(torch.uint8)                 # (two channels: the first of equal maxima is the lowest)
    flags = torch.stack([s[1] - s[0] >= G, s[0] - s[1] >= G]) if G else None
    return top, flags


for name, frames_list in (("64 ten-minute two-channel recordings", [60000 - 7 * (i % 9) for i in range(64)]),
                          ("one two-hour two-channel recording", [720000])):
    recs = [two_channel_mels(F, 100 + i) for i, F in enumerate(frames_list)]
    mels = [m for r in recs for m in r]
    content = [F for F in frames_list for _ in range(2)]
    keep = [m.clone() for m in mels]
    n_rec, n_ch, total = len(recs), len(mels), sum(content)
    table = torch.tensor([[m.data_ptr() for m in mels], [m.shape[1] for m in mels], content], dtype=torch.int64, device="cuda")
    ld, cont = table[1].to(torch.int32), table[2].to(torch.int32)
    first = torch.arange(0, n_ch + 1, 2, dtype=torch.int32, device="cuda")
    tops = torch.empty(sum(frames_list), dtype=torch.uint8, device="cuda")
    starts = [0]
    for F in frames_list:
        starts.append(starts[-1] + F)
    tptr = torch.tensor([tops.data_ptr() + a for a in starts[:-1]], dtype=torch.int64, device="cuda")
    ints = torch.empty(n_rec + n_ch, dtype=torch.int32, device="cuda")
    ws_bytes = int(lib.wm_channel_top_workspace_bytes(n_ch, total))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    h, step = ChannelOptions(bleed_db=12.0).frames(W, M)
    call = lambda st: native.check(lib.wm_channel_top(table[0].data_ptr(), ld.data_ptr(), cont.data_ptr(), first.data_ptr(), n_rec, n_ch, M, h,  # noqa: E731
                                                      st, tptr.data_ptr(), ints.data_ptr(), ints[n_rec:].data_ptr(), ws.data_ptr(), ws_bytes,
                                                      total, stream))

    def restore():
        for m, k in zip(mels, keep):
            m.copy_(k)

    ms_off = gpu_ms(lambda: call(0))
    off_top = tops.clone()
    ms_on = gpu_ms(lambda: call(step), before=restore)
    gated = int(ints[n_rec:].sum())
    restore()
    G = CH.gate_threshold(M, h, step)
    ms_t = wall_ms(lambda: [torch_top(r, F, h, G) for r, F in zip(recs, frames_list)])
    want = torch.cat([t for t, _ in ms_t[3]])
    assert torch.equal(off_top, want) and torch.equal(tops, want), "the kernel and the torch expression disagree on `top`"
    assert gated == sum(int(f.sum()) for _, f in ms_t[3]), "the kernel and the torch expression disagree on the gated frames"
    read = 2 * M * total
    report[name] = dict(recordings=n_rec, channel_frames=total, gated_frames=gated, gate_off_ms=ms_off[0], gate_off_ms_min_max=list(ms_off[1:]),
                        gate_off_mel_read_TBps=read / ms_off[0] / 1e9, gate_on_ms=ms_on[0], gate_on_ms_min_max=list(ms_on[1:]),
                        torch_ms=ms_t[0], torch_ms_min_max=list(ms_t[1:3]))
    print(f"{name} ({total} channel frames x {M} bins): wm_channel_top gate off {ms_off[0]:.3f} ms ({ms_off[1]:.3f} .. {ms_off[2]:.3f}; median of 20 "
          f"single calls between two events) = {read / ms_off[0] / 1e9:.2f} TB/s of mel READ once over all its launches; gate on (12 dB: {gated} "
          f"frames gated; reads the mel twice and writes the gated columns) {ms_on[0]:.3f} ms ({ms_on[1]:.3f} .. {ms_on[2]:.3f}); the same rule "
          f"as torch expressions {ms_t[0]:.1f} ms wall ({ms_t[1]:.1f} .. {ms_t[2]:.1f}), the same `top` and gated count "
          f"(a mel below the last-level cache's size may be served from it on the repeats)", flush=True)
    del recs, mels, keep, ws, tops

# ---- (c) one long two-channel recording: the downmix, split, split with speech, label
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
pair = two_channel_mels(F, 1)
mix = torch.maximum(pair[0], pair[1])                            # what a downmix of two parties who speak in turn looks like: loud throughout
kw = dict(temperatures=(0.0,), compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None)
full = dict(kw, n_rows=None, trace=None, condition_on_previous_text=False, initial_prompt=None, word_timestamps=False)
FORMS = {
    "downmix": lambda trace: T.transcribe_mel(enc, dec, [mix], [F], trace=trace, **kw),
    "split": lambda trace: T.transcribe_mel(enc, dec, pair, [F, F], channels=ChannelOptions(), channel_counts=[2], trace=trace, **kw),
    "split + speech": lambda trace: T.transcribe_mel(enc, dec, pair, [F, F], channels=ChannelOptions(), channel_counts=[2], speech=SP.SpeechOptions(),
                                                     trace=trace, **kw),
    "label": lambda trace: T._transcribe_channels(enc, dec, pair, [F, F], [2], ChannelOptions(mode="label"), None, None, downmix=([mix], [F]),
                                                  **dict(full, trace=trace)),
}


def job(form, trace=None):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = FORMS[form](trace)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


figures = {}
for form in FORMS:                                               # warm-up of each form (graphs, workspaces) with its trace
    trace = []
    _, res = job(form, trace)
    figures[form] = dict(decoder_calls=len(trace), windows=sum(sum(e["live"]) for e in trace), segments=len(res[0]["segments"]), wall_ms=[])
for _ in range(2):
    for form in FORMS:
        figures[form]["wall_ms"].append(job(form)[0])
report["job"] = dict(engine=str(eng), minutes=MINUTES, frames=F, tokens=TOKENS, **figures)
print(f"one two-channel recording of {MINUTES} min ({F} frames a channel), sample_len {TOKENS}, fallback off: "
      + "; ".join(f"{form} {min(v['wall_ms']) / 1e3:.1f} s (runs {[round(x) for x in v['wall_ms']]} ms; {v['windows']} windows in "
                  f"{v['decoder_calls']} decoder calls)" for form, v in figures.items()))
print(json.dumps(report))
