"""Beam search through the device loop: 64 clips x beam 5 (320 rows: beam step + cache reorder after every decoder launch)
against the greedy loop over the same 320 rows -- which is what `beam_size = 5` cost before the beam decoder existed (five
greedy copies per clip).  large-v2 shape, weight-only int8 + int8 KV, `ignore_eot` (random weights: a fixed number of
steps).  Engines: the ones `bench.py --engine-cache /tmp/wm_bench_engines` keeps.      python scripts/bench_beam.py [tokens=64]
Under `rocprofv3 --kernel-trace --stats -- python scripts/bench_beam.py 64 beam` only the beam loop runs (the new kernels'
share of a step: beam_propose_kernel, beam_merge_kernel, kv_reorder_kernel in the kernel statistics)."""
import json, os, sys, time
from pathlib import Path
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "eddie-wang-hackathon2023_amd")]
import native  # noqa: F401
import torch
import synthetic
from decoding import DecodingOptions, WhisperDecoding
from encoding import WhisperEncoding, stamp_generation
T = int(sys.argv[1]) if len(sys.argv) > 1 else 64
only_beam = len(sys.argv) > 2 and sys.argv[2] == "beam"
N_CLIPS, BEAM = 64, 5
eng = Path("/tmp/wm_bench_engines/large-v2-int8-seed0")
assert (eng / "decoder_config.json").exists(), "run bench.py --engine-cache /tmp/wm_bench_engines once first: it builds the engines and keeps them there"
dims = synthetic.DIMS["large-v2"]
enc = WhisperEncoding(eng)
g = torch.Generator(device="cuda").manual_seed(1234)
mel = (torch.randn((N_CLIPS * BEAM, dims["n_mels"], 2 * dims["n_audio_ctx"]), generator=g, device="cuda") * 0.5).clamp_(-0.5, 1.5).half()
xa = enc.get_audio_features_async(mel)
torch.cuda.synchronize()


def timed(dec, feats, reps=3, **kw):
    """ms per main_loop call.  The language pass before every call is outside the clock: it projects the clip's cross K/V (as it does
    once per batch of new audio), which a greedy call on unchanged features would otherwise reuse and a beam call -- whose candidate
    rows are rebuilt per call -- would not: the clock is to hold the token steps alone."""
    dec.detect_language(feats)
    dec.main_loop(feats, **kw)                    # warm-up: graph capture
    total = 0.0
    for _ in range(reps):
        dec.detect_language(feats)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.main_loop(feats, **kw)
        torch.cuda.synchronize()
        total += time.perf_counter() - t0
    return total / reps * 1e3


ms_g = float("nan")
if not only_beam:
    greedy = WhisperDecoding(eng, options=DecodingOptions(sample_len=T))
    ms_g = timed(greedy, xa, ignore_eot=True)
    del greedy
    torch.cuda.empty_cache()
beam = WhisperDecoding(eng, options=DecodingOptions(beam_size=BEAM, sample_len=T))
xa64 = stamp_generation(xa[:N_CLIPS].contiguous())        # (one stamp: the cross K/V of the 320 candidate rows are projected once)
ms_b = timed(beam, xa64, ignore_eot=True)
moved = int((beam._state[N_CLIPS * BEAM]['parent'].cpu() != torch.arange(N_CLIPS * BEAM)).sum())
print(f"{T} tokens, {N_CLIPS} clips x beam {BEAM} = {N_CLIPS * BEAM} rows: (a) greedy loop over the rows {ms_g:.1f} ms ({ms_g / T:.2f} ms per token step) | "
      f"(b) beam search {ms_b:.1f} ms ({ms_b / T:.2f} ms per token step, {ms_b / ms_g:.3f} x greedy); rows moved at the last step: {moved}")
print(json.dumps({"tokens": T, "rows": N_CLIPS * BEAM, "greedy_ms_per_step": ms_g / T, "beam_ms_per_step": ms_b / T}))
