"""Forced alignment, measured (reports only):
  1. the forced pass as 4-token steps (wm_decoder_step_tap) against one block (wm_decoder_prefill_tap) at 1, 8 and 64 rows x 128
     tokens, token probabilities from wm_forced_probs in both; the two forms alternate in one session, three runs each;
  2. wm_dtw_open beside wm_dtw at 225 x 1500 and on 64 ragged rows (medians of 20 launches);
  3. one synthetic file (default: one hour) with a synthetic text through transcribe.align_mel on one row: rounds, seconds, and the
     share of the encoder and of the forced pass (both timed with a synchronisation around them, which the real schedule does not
     have) -- the rest is wm_align_open, the copy back and the host's rules.
      python scripts/bench_align.py [engine_dir] [--seconds S] [--words_per_minute N] [--skip_file]
Without an engine directory a large-v2 engine with seeded random weights, weight-only int8 and fp16 K/V is built into a temporary
directory.  Random weights: the alignment itself means nothing, only the time does."""
import argparse, json, os, sys, tempfile, time
from pathlib import Path
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "eddie-wang-hackathon2023_amd")]
import native  # noqa: F401
import ctypes as C
import numpy as np
import torch
import build as B
import synthetic
import transcribe as T
from alignment import AlignOptions
from decoding import WhisperDecoding
from encoding import WhisperEncoding

ap = argparse.ArgumentParser()
ap.add_argument("engine_dir", nargs="?", default=None)
ap.add_argument("--model", default="large-v2")
ap.add_argument("--seconds", type=float, default=3600.0)
ap.add_argument("--words_per_minute", type=float, default=150.0)
ap.add_argument("--skip_file", action="store_true")
args = ap.parse_args()
tmp = None
if args.engine_dir:
    eng = Path(args.engine_dir)
else:
    tmp = tempfile.TemporaryDirectory()
    eng = Path(tmp.name) / "eng"
    t0 = time.time()
    B.build_from_checkpoint(synthetic.synthetic_checkpoint(args.model, 0, device="cuda"),
                            B.parse_arguments(["--output_dir", str(eng), "--log_level", "error", "--use_gpt_attention_plugin", "--use_gemm_plugin",
                                               "--use_layernorm_plugin", "--use_weight_only"]))
    print(f"built a {args.model} weight-only int8 engine (random weights) in {time.time() - t0:.0f} s", flush=True)
enc, dec = WhisperEncoding(eng), WhisperDecoding(eng)
cfg, tk = dec.decoder_config, dec.tokenizer
lib, report = native.load_library(), {"engine": str(args.engine_dir or args.model + " weight-only int8, random weights")}
g = torch.Generator(device="cuda").manual_seed(1234)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


# ---- 1. the forced pass: steps against block
L = 128
heads = dec.alignment_heads()
heads_arr = (C.c_int32 * len(heads))(*heads)
report["forced_pass"] = []
for n in (1, 8, 64):
    mel = (torch.randn((n, enc.num_mels, 2 * cfg["num_audio_ctx"]), generator=g, device="cuda") * 0.5).clamp_(-0.5, 1.5).half()
    xa = enc.get_audio_features(mel)
    ids = torch.randint(0, tk.eot, (n, L - len(tk.sot_sequence) - 2), generator=torch.Generator().manual_seed(n)).tolist()
    forced = [(row, list(tk.sot_sequence) + [tk.no_timestamps] + row + [tk.eot]) for row in ids]
    steps = lambda: dec._forced_pass(xa, forced, L, heads_arr, "device")
    bufs = {}                                          # (the tape, the probabilities and the logits slab stay between calls, as in align_mel)
    block = lambda: dec._forced_pass_block(xa, forced, L, heads_arr, "device", bufs)
    steps(); block()                                   # warm-up: workspaces, the cross K/V of these features
    runs = {"steps": [], "block": []}
    for _ in range(3):
        runs["steps"].append(wall_ms(steps))
        runs["block"].append(wall_ms(block))
    d_tape = float((steps()[0].float() - block()[0].float()).abs().max())
    print(f"forced pass, {n} rows x {L} tokens, {len(heads)} heads: steps {[round(v, 2) for v in runs['steps']]} ms, block "
          f"{[round(v, 2) for v in runs['block']]} ms ({min(runs['steps']) / min(runs['block']):.1f} x at the best of each); max |tape diff| {d_tape:.3g}", flush=True)
    report["forced_pass"].append(dict(rows=n, tokens=L, steps_ms=runs["steps"], block_ms=runs["block"], tape_diff=d_tape))
    del xa, mel, bufs
dec._state.clear()
torch.cuda.empty_cache()


# ---- 2. the open end beside the closed walk
def gpu_ms(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return sorted(times)[len(times) // 2]


report["dtw"] = []
rng = np.random.default_rng(3)
for name, shapes in (("225 x 1500", [(225, 1500)]), ("64 ragged rows", [(int(a), int(b)) for a, b in zip(rng.integers(20, 226, 64), rng.integers(300, 1501, 64))])):
    Bn, R, Cc = len(shapes), max(s[0] for s in shapes), max(s[1] for s in shapes)
    x = torch.randn((Bn, R, Cc), generator=g, device="cuda")
    nr = torch.tensor([s[0] for s in shapes], dtype=torch.int32).cuda()
    nc = torch.tensor([s[1] for s in shapes], dtype=torch.int32).cuda()
    pt, pf = torch.zeros((Bn, R + Cc), dtype=torch.int32).cuda(), torch.zeros((Bn, R + Cc), dtype=torch.int32).cuda()
    pl, er = torch.zeros(Bn, dtype=torch.int32).cuda(), torch.zeros(Bn, dtype=torch.int32).cuda()
    ws = torch.empty(lib.wm_dtw_workspace_bytes(Bn, R, Cc), dtype=torch.uint8).cuda()
    s = torch.cuda.current_stream().cuda_stream
    lead = (x.data_ptr(), Cc, R * Cc, Bn, nr.data_ptr(), nc.data_ptr(), R, Cc, pt.data_ptr(), pf.data_ptr(), R + Cc, pl.data_ptr())
    closed = lambda: native.check(lib.wm_dtw(*lead, ws.data_ptr(), ws.numel(), s), "wm_dtw")
    opened = lambda: native.check(lib.wm_dtw_open(*lead, er.data_ptr(), ws.data_ptr(), ws.numel(), s), "wm_dtw_open")
    a = [gpu_ms(closed), gpu_ms(opened), gpu_ms(closed), gpu_ms(opened)]
    print(f"dtw {name}: wm_dtw {a[0]:.3f} / {a[2]:.3f} ms, wm_dtw_open {a[1]:.3f} / {a[3]:.3f} ms (medians of 20, alternating)", flush=True)
    report["dtw"].append(dict(shape=name, dtw_ms=[a[0], a[2]], dtw_open_ms=[a[1], a[3]]))

# ---- 3. one long file
if not args.skip_file:
    W = 2 * cfg["num_audio_ctx"]
    content = int(args.seconds * W / 30.0)
    mel = (torch.randn((enc.num_mels, content + W), generator=g, device="cuda") * 0.5).clamp_(-0.5, 1.5).half()
    vocab = ["the", "sound", "of", "a", "river", "carries", "over", "stones", "and", "nobody", "listens", "until", "evening", "comes", "again"]
    n_words = int(args.seconds / 60.0 * args.words_per_minute)
    pick = np.random.default_rng(5).integers(0, len(vocab), n_words)
    lines = [" ".join(vocab[k] for k in pick[a:a + 12]) + "." for a in range(0, n_words, 12)]
    spent, calls = {"encoder": 0.0, "forced": 0.0}, {"encoder": 0, "forced": 0}
    real_enc, real_forced = enc.get_audio_features, dec._forced_pass_block

    def timed(key, fn):
        def wrapper(*a, **k):
            out = []
            spent[key] += wall_ms(lambda: out.append(fn(*a, **k)))
            calls[key] += 1
            return out[0]
        return wrapper
    enc.get_audio_features, dec._forced_pass_block = timed("encoder", real_enc), timed("forced", real_forced)
    rounds = []
    total = wall_ms(lambda: rounds.append(T.align_mel(enc, dec, [mel], [content], [lines], language="en", options=AlignOptions(), rows=1, keep_rounds=None)))
    enc.get_audio_features, dec._forced_pass_block = real_enc, real_forced
    res = rounds[0][0]
    placed = sum(w["aligned"] for w in res["words"])
    n_rounds = calls["encoder"]                         # the encoder runs once per round
    rest = total - spent["encoder"] - spent["forced"]
    print(f"one file of {args.seconds:.0f} s, {n_words} words in {len(lines)} lines, one row: {n_rounds} rounds, {total / 1e3:.2f} s; encoder {spent['encoder'] / total:.0%}, "
          f"forced pass {spent['forced'] / total:.0%}, alignment + copy back + host {rest / total:.0%}; {placed} of {len(res['words'])} words placed", flush=True)
    report["file"] = dict(seconds=args.seconds, words=n_words, rounds=n_rounds, wall_s=total / 1e3, encoder_ms=spent["encoder"], forced_ms=spent["forced"], rest_ms=rest,
                          placed=placed, of=len(res["words"]))
print(json.dumps(report))
