"""What the alignment stack computes, as SHA-256 digests: one JSON line to compare between two commits on the same machine (a
refactor of word_align.py / align.hip / the tapped decoder entries must leave every digest as it was).  Nothing is compared with an
expected value here: the digests belong to a pair of commits and a compiler, not to the repository.
      python scripts/alignment_digest.py
      WM_LAB=1 WM_KSPLIT_CAP=8 python scripts/alignment_digest.py        # the case in which the tap's two slab orders differ
Seeded synthetic engines and mels, random weights.  Per case four `word_timestamps` runs (forced_pass steps / block x token_probs
torch / device) digest the tape and the token probabilities as `_forced_pass` / `_forced_pass_block` return them, and the paths, their
lengths, the alignment matrices, the token probabilities and the words of the call; the first case adds `align_mel(keep_rounds=True)`:
the results and every round's matrices, paths, end rows, token probabilities and placed words.
Cases without WM_KSPLIT_CAP: micro-fullvocab (B = 3, 11 forced tokens: tape offsets 0, 4 and 8) as fp16, weight-only int8 and int8
self-attention K/V; a 384-wide toy at B = 20 on the split-K chain (wm_set_rows_path(0)), where the cross-attention query waits in three
slabs.  With WM_LAB=1 WM_KSPLIT_CAP=8 (read once per process, hence a run of its own): that toy at 768 wide, 12 heads, whose query
waits in six slabs -- the fewest at which pairs (attn_decode.hip) and rounds of four (attn_prefill.hip) round differently.  The line
says how many slabs the library splits each toy's query into (`cq_slabs`)."""
import ctypes as C
import hashlib
import json
import os
import sys
import tempfile
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "eddie-wang-hackathon2023_amd")]
import native  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
import build as B  # noqa: E402
import synthetic  # noqa: E402
import transcribe as T  # noqa: E402
from alignment import AlignOptions  # noqa: E402
from decoding import WhisperDecoding  # noqa: E402
from encoding import WhisperEncoding  # noqa: E402


def feed(h, x):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    if isinstance(x, np.ndarray):
        h.update(f"<{x.dtype} {x.shape}>".encode())
        h.update(np.ascontiguousarray(x).tobytes())
    elif isinstance(x, dict):
        for k in sorted(x):
            h.update(f"{k}:".encode())
            feed(h, x[k])
    elif isinstance(x, (list, tuple)):
        h.update(f"[{len(x)}]".encode())
        for v in x:
            feed(h, v)
    elif hasattr(x, "_asdict") or hasattr(x, "__dataclass_fields__"):
        feed(h, {k: getattr(x, k) for k in (x._fields if hasattr(x, "_fields") else x.__dataclass_fields__)})
    else:
        h.update(repr(x.item() if isinstance(x, np.generic) else x).encode())


def digest(x) -> str:
    h = hashlib.sha256()
    feed(h, x)
    return h.hexdigest()[:16]


def synthetic_mel(batch, frames, n_mels, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((batch, n_mels, frames), generator=g) * 0.5).clamp_(-0.5, 1.5).half()


def toy(width, heads):
    return dict(n_mels=80, n_audio_ctx=64, n_audio_state=width, n_audio_head=heads, n_audio_layer=1, n_vocab=51865, n_text_ctx=32,
                n_text_state=width, n_text_head=heads, n_text_layer=2)


def engine(tmp, name, model, seed, extra=()):
    out = os.path.join(tmp, name)
    if "--int8_kv_cache" in extra:
        dims = synthetic.DIMS[model] if isinstance(model, str) else model
        qdir = os.path.join(tmp, name + "_quantize", "1-gpu")
        os.makedirs(qdir)
        for i in range(dims["n_text_layer"]):
            np.array([0.05 + 0.01 * i], dtype=np.float32).tofile(
                os.path.join(qdir, f"model.decoder.blocks.{i}.attn.query_key_value.scale_y_quant_orig.bin"))
        extra = list(extra) + ["--quantize_dir", qdir]
    B.build_from_checkpoint(synthetic.synthetic_checkpoint(model, seed),
                            B.parse_arguments(["--output_dir", out, "--use_gpt_attention_plugin", "--use_gemm_plugin", "--use_layernorm_plugin",
                                               "--log_level", "error"] + list(extra)))
    return WhisperEncoding(Path(out)), WhisperDecoding(Path(out))


def word_runs(enc, dec, batch, seed):
    cfg, tk = dec.decoder_config, dec.tokenizer
    xa = enc.get_audio_features(synthetic_mel(batch, 2 * cfg["num_audio_ctx"], enc.num_mels, seed).cuda())
    rng = np.random.default_rng(seed)
    n_text = 11 - len(tk.sot_sequence) - 2
    sampled = [rng.integers(300, 20000, n_text - (b % 3 == 1) * 2).tolist() for b in range(batch)]      # (ragged: every third row two short)
    frames = [2 * cfg["num_audio_ctx"] - 7 * (b % 4) for b in range(batch)]
    forced = [dec._forced_tokens(s) for s in sampled]
    L = max(len(f) for _, f in forced)
    heads = dec.alignment_heads()
    heads_arr = (C.c_int32 * len(heads))(*heads)
    dec.keep_alignment_matrix = True
    out = {}
    for form in ("steps", "block"):
        for probs in ("torch", "device"):
            run = dec._forced_pass if form == "steps" else dec._forced_pass_block
            tape, p, _ = run(xa, forced, L, heads_arr, probs)
            got = dict(tape=tape[:, :, :L], pass_probs=p[:, :L])
            got["words"] = dec.word_timestamps(xa, sampled, frames, token_probs=probs, forced_pass=form)
            got.update({k: dec.last_alignment[k] for k in ("path_text", "path_time", "path_len", "matrix", "token_probs")})
            out[f"{form}/{probs}"] = digest(got)
    return out


def align_run(enc, dec):
    W = 2 * dec.decoder_config["num_audio_ctx"]
    contents = [2 * W + W // 2, 100, 7]
    lines = ["The quick brown fox jumps over the lazy dog, and then (quite suddenly) it stops.",
             "Nobody had expected that: not the dog, not the fox, not even the narrator!",
             "So the story ends here, with sixteen more words than anybody needed to hear about a fox."]
    texts = [lines, "", " ".join(f"word{k} and" for k in range(40))]
    mels = [synthetic_mel(1, c + W, enc.num_mels, 700 + i)[0].half().cuda().contiguous() for i, c in enumerate(contents)]
    results = T.align_mel(enc, dec, mels, contents, texts, language="en", options=AlignOptions(max_tokens=16, edge_seconds=0.5), rows=2,
                          keep_rounds=True)
    rounds = results[0]["rounds"]
    return digest(dict(results=[{k: v for k, v in r.items() if k != "rounds"} for r in results], rounds=rounds)), len(rounds)


def main():
    lib = native.load_library()
    slabs = {w: lib.wm_gemm_skinny_default_ksplit(80, w, w // 16, 0) for w in (384, 768)}
    report = dict(cq_slabs=slabs, cases={})
    with tempfile.TemporaryDirectory() as tmp:
        if slabs[768] >= 6:
            cases = [("toy768-fp16-B20-rows-path-off", toy(768, 12), (), 20, True)]
        else:
            cases = [("micro-fp16-B3", "micro-fullvocab", (), 3, False),
                     ("micro-weight-only-B3", "micro-fullvocab", ("--use_weight_only",), 3, False),
                     ("micro-int8-kv-B3", "micro-fullvocab", ("--int8_kv_cache",), 3, False),
                     ("toy384-fp16-B20-rows-path-off", toy(384, 6), (), 20, True)]
        for k, (name, model, extra, batch, rows_off) in enumerate(cases):
            enc, dec = engine(tmp, name, model, 3 + k, extra)
            prev = lib.wm_set_rows_path(0) if rows_off else None
            try:
                report["cases"][name] = word_runs(enc, dec, batch, 77 + k)
                if k == 0 and slabs[768] < 6:
                    report["cases"][name]["align_mel"], report["align_rounds"] = align_run(enc, WhisperDecoding(Path(tmp) / name))
            finally:
                if prev is not None:
                    lib.wm_set_rows_path(prev)
            del enc, dec
            torch.cuda.empty_cache()
    print(json.dumps(report, sort_keys=True))


if __name__ == "__main__":
    main()
