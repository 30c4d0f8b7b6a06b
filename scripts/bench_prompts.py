"""What a conditioned decoder call costs.  Reports only.
A main_loop call of an instance built with row_prompts=True (every row carries a prompt: a prefill of
L0 = n_text_ctx // 2 + len(sot_sequence) tokens in 4-token passes, token steps that never take a one-launch form) beside the
same call of a plain instance on the same engine, at 1, 8 and 64 rows; the prefill (up to the first sampled token) and the
steps behind it are timed apart.  A third column is the same row_prompts call on an instance built with block_prefill=True (the L0
tokens in ONE pass, wm_decoder_prefill), without prompts and with full prompts, on the same rows.
      python scripts/bench_prompts.py [tokens=32] [rows=1,8,64] [engine_dir]
Without an engine directory: the large-v2 engines `bench.py --engine-cache /tmp/wm_bench_engines` keeps when they exist, else
a `tiny`-shaped engine with seeded random weights built into a temporary directory."""
import json, os, sys, tempfile, time
from pathlib import Path
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "eddie-wang-hackathon2023_amd")]
import native  # noqa: F401
import torch
import build as B
import synthetic
from decoding import DecodingOptions, WhisperDecoding
from encoding import WhisperEncoding

TOKENS = int(sys.argv[1]) if len(sys.argv) > 1 else 32
ROWS = [int(r) for r in (sys.argv[2] if len(sys.argv) > 2 else "1,8,64").split(",")]
tmp = None
if len(sys.argv) > 3:
    eng, shape = Path(sys.argv[3]), None
elif (Path("/tmp/wm_bench_engines/large-v2-int8-seed0") / "decoder_config.json").exists():
    eng, shape = Path("/tmp/wm_bench_engines/large-v2-int8-seed0"), "large-v2"
else:
    tmp = tempfile.TemporaryDirectory()
    eng, shape = Path(tmp.name) / "eng", "tiny"
    B.build_from_checkpoint(synthetic.synthetic_checkpoint("tiny", 0), B.parse_arguments(["--output_dir", str(eng), "--log_level", "error"]))
enc = WhisperEncoding(eng)
report = dict(engine=shape or str(eng), tokens=TOKENS, rows={})


def timed(dec, xa, reps=5):
    """(ms to the first sampled token, ms of the whole call): medians; two warm-up calls (workspaces, graph capture)."""
    first = torch.cuda.Event(enable_timing=True)
    dec.first_token_event = first
    for _ in range(2):
        dec.main_loop(xa, ignore_eot=True)
    pre, whole = [], []
    for _ in range(reps):
        t0 = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        t0.record()
        dec.main_loop(xa, ignore_eot=True)
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - w0) * 1e3)
        pre.append(t0.elapsed_time(first))
    dec.first_token_event = None
    return sorted(pre)[reps // 2], sorted(whole)[reps // 2]


for n in ROWS:
    g = torch.Generator(device="cuda").manual_seed(n)
    cfg_probe = WhisperDecoding(eng, options=DecodingOptions(sample_len=TOKENS, language="en"))
    Wn, n_mels = 2 * cfg_probe.decoder_config["num_audio_ctx"], enc.session.dims["n_mels"]
    mel = (torch.randn((n, n_mels, Wn), generator=g, device="cuda") * 0.5).clamp_(-0.5, 1.5).half()
    xa = enc.get_audio_features(mel)
    plain_pre, plain_all = timed(cfg_probe, xa)
    del cfg_probe
    dec = WhisperDecoding(eng, row_prompts=True, options=DecodingOptions(sample_len=TOKENS, language="en"))
    V = dec.decoder_config["vocab_size"]
    full = torch.randint(1000, min(V, 50000), (n, dec.prompt_capacity), generator=torch.Generator().manual_seed(n)).tolist()
    out = {}
    for name, prompts in (("no_prompt", [[] for _ in range(n)]), ("full_prompt", full)):
        dec.set_prompts(prompts)
        out[name] = timed(dec, xa)
    steps = min(TOKENS, dec.sample_len)
    del dec
    dec = WhisperDecoding(eng, row_prompts=True, block_prefill=True, options=DecodingOptions(sample_len=TOKENS, language="en"))
    for name, prompts in (("block_no_prompt", [[] for _ in range(n)]), ("block_full_prompt", full)):
        dec.set_prompts(prompts)
        out[name] = timed(dec, xa)
    report["rows"][n] = dict(L0=dec.sample_begin, steps=steps, plain_prefill_ms=plain_pre, plain_call_ms=plain_all,
                             **{f"{k}_prefill_ms": v[0] for k, v in out.items()}, **{f"{k}_call_ms": v[1] for k, v in out.items()})
    print(f"{shape or eng}, {n} rows, {steps} tokens: plain call {plain_all:.1f} ms (first token after {plain_pre:.2f} ms); "
          f"row_prompts (L0 = {dec.sample_begin}) without prompts {out['no_prompt'][1]:.1f} ms (first token after {out['no_prompt'][0]:.2f} ms), "
          f"with {dec.prompt_capacity}-token prompts {out['full_prompt'][1]:.1f} ms (first token after {out['full_prompt'][0]:.2f} ms); "
          f"block_prefill without prompts {out['block_no_prompt'][1]:.1f} ms (first token after {out['block_no_prompt'][0]:.2f} ms), "
          f"with prompts {out['block_full_prompt'][1]:.1f} ms (first token after {out['block_full_prompt'][0]:.2f} ms)")
    del dec
print(json.dumps(report))
