"""References for right-aligned rows (wm_decoder_io::row_start), used by tests/test_gpu_prompts.py and tests/test_prompts_cpu.py.

`self_attn_rows_ref` restates the contract at the top of csrc/attn_decode.hip in fp32, row by row and token by token, without
any of the kernels' structure: which keys a query sees is decided here by slot numbers alone.

    q, k of the call are fp16 values; q * 64^-0.25 and k * 64^-0.25 are rounded to fp16; a score is the fp32 dot product rounded
    to fp16; the softmax runs in fp32 over the row's key range; probabilities are rounded to fp16; P.V accumulates in fp32 and is
    rounded to fp16.  Cached keys / values are what the cache holds (int8: fp16(code * t)), the call's own are un-quantised.
    Row b begins at slot s = starts[b]: a query in slot t < s yields zeros, any other attends to the slots [s, t].
"""
import numpy as np
import torch

SCALE = 0.35355339059327373          # 64^-0.25


def r16(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float32).to(torch.float16).to(torch.float32)


def quant_codes(x: torch.Tensor, t: float) -> torch.Tensor:
    """sat_s8(rne(x * (1 / t))), 1 / t formed in fp32 (the cache append)."""
    inv = np.float32(1.0) / np.float32(t)
    return torch.clamp(torch.round(x.to(torch.float32) * float(inv)), -128, 127).to(torch.int8)


def dequant(codes: torch.Tensor, t: float) -> torch.Tensor:
    """fp16(code * t) as fp32: what a cached int8 value is used as."""
    return r16(codes.to(torch.float32) * float(np.float32(t)))


def self_attn_rows_ref(qkv: torch.Tensor, cached: torch.Tensor, T: int, starts, H: int) -> torch.Tensor:
    """qkv fp32 [B, L, 3, H, 64] (fp16 values); cached fp32 [B, 2, H, >= T, 64]: the VALUES the cache holds in slots 0 .. T - 1
    (pad slots may hold anything, NaN included: they must not be read).  Returns fp32 [B, L, H * 64]."""
    B, L = qkv.shape[:2]
    out = torch.zeros((B, L, H, 64), dtype=torch.float32)
    for b in range(B):
        s = int(starts[b])
        for i in range(L):
            slot = T + i
            if slot < s:
                continue                                     # a pad query: zeros
            for h in range(H):
                keys, vals = [], []
                for t in range(s, slot + 1):
                    if t < T:
                        keys.append(cached[b, 0, h, t]); vals.append(cached[b, 1, h, t])
                    else:
                        keys.append(qkv[b, t - T, 1, h]); vals.append(qkv[b, t - T, 2, h])
                K, V = torch.stack(keys).float(), torch.stack(vals).float()
                q = r16(qkv[b, i, 0, h].float() * SCALE)
                sc = r16((r16(K * SCALE).double() @ q.double()).float())
                p = r16(torch.softmax(sc.float(), dim=0))
                out[b, i, h] = r16((p.double() @ V.double()).float())
    return out.reshape(B, L, H * 64)


def pass_bounds(start: int, length: int, chunk: int = 4):
    """How the 4-token passes of a block that fills slots [0, start + length) cut a row that begins at slot `start`: the
    (lo, hi) token ranges of the row, relative to its own first token."""
    cuts, t = [], start
    while t < start + length:
        nxt = min((t // chunk + 1) * chunk, start + length)
        cuts.append((t - start, nxt - start))
        t = nxt
    return cuts


def oracle_row(oracle, ckv_row, tokens, start: int):
    """The oracle's decoder over ONE row alone and un-padded, fed in the pieces the engine's 4-token passes cut it into (what is
    'past' and what is 'the current call' matters with an int8 cache: past keys are seen through their codes).
    Returns (logits fp32 [len(tokens), V], self_kv)."""
    kv, rows = None, []
    for lo, hi in pass_bounds(start, len(tokens)):
        logits, kv = oracle.decoder(torch.tensor([tokens[lo:hi]], dtype=torch.long), ckv_row, kv)
        rows.append(logits[0])
    return torch.cat(rows, dim=0), kv


def oracle_greedy_row(oracle, ckv_row, row_tokens, rules, sample_len: int):
    """Whisper's greedy loop (oracle/decoding_rules.py) over ONE un-padded row on the CPU oracle.  Returns (sampled tokens, margins):
    margins[i] is how decided step i was -- the gap between the two best filtered logits, or the margin of the timestamp-dominance
    rule when that is smaller.  `rules.sample_begin` must be len(row_tokens)."""
    import oracle.decoding_rules as DR
    tokens = np.array([list(row_tokens)], dtype=np.int64)
    kv, margins = None, []
    for i in range(sample_len):
        feed = tokens if i == 0 else tokens[:, -1:]
        logits, kv = oracle.decoder(torch.from_numpy(feed), ckv_row, kv)
        dom = []
        lg = DR.apply_filters(logits[:, -1].numpy(), tokens, rules, dominance_out=dom)
        top = np.sort(lg[0])[-2:]
        margins.append(min(float(top[1] - top[0]), abs(dom[0]) if dom else float("inf")))
        tokens = np.concatenate([tokens, [[int(lg[0].argmax())]]], axis=1)
        if tokens[0, -1] == rules.ids.eot:
            break
    return tokens[0, len(row_tokens):].tolist(), margins
