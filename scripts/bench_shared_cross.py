"""One copy of the cross K/V per utterance (WhisperDecoding(shared_cross_kv=True)) against a copy per candidate: 64 clips x beam 5
(320 rows) through the device loop, and the same 320 rows as best_of = 5 samples at temperature 0.4.  large-v2 shape, weight-only
int8 + int8 KV, `ignore_eot` (random weights: a fixed number of steps).  Prints ms per token step with and without sharing and the
cross K/V bytes each instance allocates.  Engines: the ones `bench.py --engine-cache /tmp/wm_bench_engines` keeps.
      python scripts/bench_shared_cross.py [tokens=64] [beam|best_of]
Under `rocprofv3 --kernel-trace --stats -- python scripts/bench_shared_cross.py 64 beam` the kernel statistics show the grouped
cross-attention (attn_cross_kernel<5, ..., 1>) beside the chains it runs under."""
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
only = sys.argv[2] if len(sys.argv) > 2 else None
N_CLIPS, G = 64, 5
eng = Path("/tmp/wm_bench_engines/large-v2-int8-seed0")
assert (eng / "decoder_config.json").exists(), "run bench.py --engine-cache /tmp/wm_bench_engines once first: it builds the engines and keeps them there"
dims = synthetic.DIMS["large-v2"]
enc = WhisperEncoding(eng)
g = torch.Generator(device="cuda").manual_seed(1234)
mel = (torch.randn((N_CLIPS, dims["n_mels"], 2 * dims["n_audio_ctx"]), generator=g, device="cuda") * 0.5).clamp_(-0.5, 1.5).half()
xa = stamp_generation(enc.get_audio_features_async(mel).contiguous())
torch.cuda.synchronize()


def timed(dec, reps=3):
    """ms per main_loop call; the language pass before every call (it projects the clips' cross K/V, once per batch of new audio) is
    outside the clock, as in scripts/bench_beam.py: the clock holds the prefill and the token steps."""
    dec.detect_language(xa)
    dec.main_loop(xa, ignore_eot=True)            # warm-up: graph capture
    total = 0.0
    for _ in range(reps):
        dec.detect_language(xa)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.main_loop(xa, ignore_eot=True)
        torch.cuda.synchronize()
        total += time.perf_counter() - t0
    st = next(iter(dec._state.values()))
    return total / reps * 1e3, sum(t.numel() * t.element_size() for t in st['cross'])


out = {"tokens": T, "rows": N_CLIPS * G}
for name, options in (("beam", DecodingOptions(beam_size=G, sample_len=T)), ("best_of", DecodingOptions(best_of=G, temperature=0.4, sample_len=T))):
    if only not in (None, name):
        continue
    for shared in (False, True):
        dec = WhisperDecoding(eng, options=options, shared_cross_kv=shared)
        ms, nbytes = timed(dec)
        key = f"{name}_{'shared' if shared else 'per_candidate'}"
        out[key + "_ms_per_step"], out[key + "_cross_bytes"] = ms / T, nbytes
        print(f"{T} tokens, {N_CLIPS} clips x {name} {G} = {N_CLIPS * G} rows, cross K/V {'shared' if shared else 'per candidate'}: "
              f"{ms:.1f} ms ({ms / T:.2f} ms per token step), {nbytes / 1e9:.2f} GB of cross K/V")
        del dec
        torch.cuda.empty_cache()
print(json.dumps(out))
