"""Golden outputs of the encoder attention kernel (wm_attn_encoder) for tests/test_gpu_attn_encoder_bits.py.

Run on a build of the commit whose bits are to be kept.  The file in the tree came from commit 739f858 ("Add long-form
transcription: windows, timestamp seeking, fallback"), the parent of the change that removed the dead tail work and the LDS
exchanges of csrc/attn_encoder.hip; the hash is stored in the file as `source_commit` (pass another as the first argument):

    python scripts/gen_attn_encoder_golden.py            # writes tests/golden/attn_encoder_parent.npz

Inputs are seeded numpy PCG64 draws, fp16, q and k columns multiplied by 64^-0.25 and rounded as the QKV GEMM epilogue does;
the test regenerates them with make_qkv() below and finds the SHA-256 of the input bytes in the file, so a drift of the
generator shows as such and not as a kernel difference.

What is stored per case: the SHA-256 of the whole output (the byte-equality assertion), and rows of it to look at when the hash
differs.  Two clips x three heads of fp16 outputs are 768 bytes per frame, the thirteen small cases together 2.5 MB -- over the
1 MiB a committed file may have -- so only T = 100 and T = 128 are stored whole; the QB = 4 cases keep, per clip, the last
48 query rows (the last query tile's live blocks, where dead query blocks are skipped) and 16 sampled rows, T = 1500 keeps
64 sampled rows."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_encoder_parent.npz")

# name -> (B, T, H, late): late = eight key rows near the end of the sequence, one of them inside the tail tile, times 8
CASES = {}
for _T in (257, 272, 273, 288, 289, 300, 304, 320, 383, 100, 128):
    CASES[f"t{_T}"] = (2, _T, 3, False)
CASES["t273_late"] = (2, 273, 3, True)
CASES["t300_late"] = (2, 300, 3, True)
CASES["t300_b3h5"] = (3, 300, 5, False)       # 15 heads -> 32 items with one head of padding: 8 persistent workgroups take 4 each
CASES["t1500"] = (1, 1500, 2, False)
LATE_ROWS = (3, 50, 70, 80, 97, 110, 131, 150)          # counted back from T


def seed_of(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def make_qkv(name):
    """[B * T, 3 * H * 64] fp16, columns q | k | v."""
    B, T, H, late = CASES[name]
    r = np.random.Generator(np.random.PCG64(seed_of(name)))
    C = H * 64
    q, k, v = (r.standard_normal((B, T, C), dtype=np.float32).astype(np.float16) for _ in range(3))
    scale = np.float32(64 ** -0.25)
    qs = (q.astype(np.float32) * scale).astype(np.float16)
    ks = (k.astype(np.float32) * scale).astype(np.float16)
    if late:
        for back in LATE_ROWS:
            ks[:, T - back] = (ks[:, T - back].astype(np.float32) * np.float32(8)).astype(np.float16)
    return np.ascontiguousarray(np.concatenate([qs, ks, v], axis=2).reshape(B * T, 3 * C))


def kept_rows(name):
    """Row indices (inside a clip) whose outputs the golden file stores; None = all."""
    B, T, H, _ = CASES[name]
    if T <= 128:
        return None
    r = np.random.Generator(np.random.PCG64(seed_of(name) + 1))
    if name == "t1500":
        return np.sort(r.choice(T, 64, replace=False))
    return np.concatenate([np.sort(r.choice(T - 48, 16, replace=False)), np.arange(T - 48, T)])


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_kernel(lib, native, torch, qkv, B, T, H):
    """wm_attn_encoder on the current stream; [B, T, H * 64] fp16 numpy.  One guard row behind the output must stay as it was."""
    C = H * 64
    x = torch.from_numpy(qkv).cuda()
    out = torch.full((B * T + 1, C), 7.0, dtype=torch.float16, device="cuda")
    native.check(lib.wm_attn_encoder(x.data_ptr(), 3 * C, B, T, H, out.data_ptr(), C, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((out[B * T] == 7.0).all()), "attn_encoder wrote behind its output"
    return out[:B * T].cpu().numpy().reshape(B, T, C)


def main():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "eddie-wang-hackathon2023_amd")]
    import native
    import torch
    lib = native.load_library()
    store = {}
    for name, (B, T, H, _) in CASES.items():
        qkv = make_qkv(name)
        out = run_kernel(lib, native, torch, qkv, B, T, H)
        assert np.isfinite(out.astype(np.float32)).all(), name
        rows = kept_rows(name)
        store[name + "/in_sha256"] = np.array(sha(qkv))
        store[name + "/out_sha256"] = np.array(sha(out))
        store[name + "/rows"] = out if rows is None else out[:, rows]
        print(name, B, T, H, sha(out)[:16], flush=True)
    store["source_commit"] = np.array(sys.argv[1] if len(sys.argv) > 1 else "739f858")
    np.savez_compressed(GOLDEN, **store)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
    assert os.path.getsize(GOLDEN) < 1000000


if __name__ == "__main__":
    main()
