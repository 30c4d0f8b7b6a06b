"""The contract of the block-prefill attention kernels (csrc/attn_prefill.hip), restated in float64 on kernel_refs.attn_decode_ref:
the rounding points are that function's, the only addition is WHICH keys a query sees, written here as a matrix.

    self:  the query in slot t of utterance b sees the slots [start[b], t] of the block's own un-quantised k / v; a query in a pad
           slot (t < start[b]) yields an all-zero row; every slot 0 .. L - 1 is appended to the cache, pad slots included: the fp16
           row itself, or sat_s8(rne(x * (1 / t))) with 1 / t formed in fp32.
    cross: every query sees every key of its utterance's K/V; no row_start.

tests/test_prefill_cpu.py holds `prefill_self_ref` against prompt_refs.self_attn_rows_ref(T = 0), which decides the same thing by
slot numbers, row by row and token by token -- two independent statements -- and the codes against kernel_refs.self_cache_codes.
"""
import numpy as np
import torch

import kernel_refs as KR

OUT_TOL = 2e-3      # tests/test_gpu_kernels.py::test_attn_encoder's bound: the same online-softmax arithmetic at O(1) outputs


def causal_mask(L, start):
    """[L, L] additive, float64: 0 where start <= key <= query, -inf elsewhere.  The rows of pad queries (query < start) hold no
    visible key; they are left all-zero here (the caller overwrites their output with zeros) so that no softmax sees an empty row."""
    q = torch.arange(L)[:, None]
    k = torch.arange(L)[None, :]
    mask = torch.where((k >= start) & (k <= q), 0.0, float("-inf")).to(torch.float64)
    mask[:min(start, L)] = 0.0
    return mask


def prefill_self_ref(rows, starts, B, L, H):
    """rows float [B * L, 3 * H * 64] holding fp16 values (q | k | v); starts: B slot numbers in 0 .. L.  -> float64 [B * L, H * 64]."""
    C = H * 64
    rows = rows.to(torch.float64)
    q, k, v = (KR.split_heads(rows[:, i * C:(i + 1) * C], B, L, H) for i in range(3))
    out = torch.zeros((B, H, L, 64), dtype=torch.float64)
    for b in range(B):
        s = int(starts[b])
        out[b] = KR.attn_decode_ref(q[b:b + 1], k[b:b + 1], v[b:b + 1], causal_mask(L, s))[0]
        out[b, :, :min(s, L)] = 0.0
    return KR.merge_heads(out)


def prefill_cross_ref(qrows, kv, B, L, H):
    """qrows float [B * L, H * 64] (fp16 values), kv [B, 2, H, Tk, 64] fp16.  -> float64 [B * L, H * 64]."""
    q = KR.split_heads(qrows.to(torch.float64), B, L, H)
    return KR.merge_heads(KR.attn_decode_ref(q, kv[:, 0].to(torch.float64), kv[:, 1].to(torch.float64)))


def cache_rows(rows, B, L, H, int8_kv, t):
    """What slots 0 .. L - 1 of the cache hold after the call: [B, 2, H, L, 64], fp16 rows or int8 codes."""
    C = H * 64
    kv = rows[:, C:].reshape(B, L, 2, H, 64).permute(0, 2, 3, 1, 4).contiguous()
    return KR.self_cache_codes(kv, t) if int8_kv else kv.to(torch.float16)


def fp16_normal(r, shape):
    """Standard-normal fp16 values as fp32 (the inputs of test_attn_encoder)."""
    return torch.from_numpy(r.standard_normal(shape).astype(np.float16).astype(np.float32))


def geometry_values(L):
    """v[t][d]: small multiples of 1 / 8 within +-2, asymmetric in (t, d): a transposed tile or a key range shifted by one slot
    changes the mean over the visible slots by far more than the bound."""
    t = torch.arange(L)[:, None]
    d = torch.arange(64)[None, :]
    return (((t * 7 + d * 3 + (t * d) % 5) % 33) - 16).to(torch.float32) / 8.0


# (L, Tk) of the cross-attention cases: a dozen pairs out of {1, 5, 17, 64, 65, 227} x {8, 63, 64, 65, 100, 1500} -- every L (both
# instantiations: L <= 64 and above), every Tk (below a tile, a tile, a tile and one key, a masked tail behind full tiles, the product's)
CROSS_CASES = [(1, 8), (1, 1500), (5, 63), (5, 64), (17, 65), (17, 100), (64, 64), (64, 1500), (65, 63), (65, 1500), (227, 100), (227, 1500)]
SELF_LENGTHS = [1, 15, 16, 17, 63, 64, 65, 129, 227, 448]
START_POOL = [0, 1, 15, 16, 63, 64, 65]


def start_sets(L):
    """Triples of row starts for B = 3 that together use every value of {0, 1, 15, 16, 63, 64, 65, L - 1, L} that fits the block."""
    pool = sorted({s for s in START_POOL if s <= L} | {max(L - 1, 0), L})
    while len(pool) % 3:
        pool.append(pool[len(pool) % 2])
    return [pool[i:i + 3] for i in range(0, len(pool), 3)]
