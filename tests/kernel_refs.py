"""Plain restatements of what the MFMA GEMM epilogue, the row kernels and the decode attention kernels compute, for the kernel-level
parity tests (tests/test_gpu_gemm_epilogue.py, tests/test_gpu_row_kernels.py, tests/test_gpu_attn_decode_contract.py), and the case
lists those tests run.

Everything here is torch in float64 over the fp16-rounded inputs, with the kernels' rounding points and nothing of their structure:
no tiles, no lanes, no summation order.  A rounding point is `r16`: the kernels hold an fp32 value there and convert it to fp16, so
the float64 value is rounded to fp32 and then to fp16 (for a sum or product of two fp16 / fp32 operands the float64 value is exact,
which makes this the kernel's own arithmetic; for a long dot product it differs from the kernel by the fp32 summation order only).

The helpers work on whatever device their inputs live on.  tests/test_kernel_refs_cpu.py checks them against torch's own operators
and tests/golden/ops.npz where no GPU exists, so the GPU tests compare the kernels with something that has been verified.

The second half restates the launchers' DISPATCH (which kernel template a call reaches) and the persistent kernel's tile order, so
that the case lists can be shown to reach every instantiation and every branch of the order -- on the CPU, before a GPU is needed.
"""
import itertools
import math

import numpy as np
import torch

SENTINEL = -1234.0                      # exactly representable in fp16; no kernel under test produces it
QK_SCALE = 0.35355339059327373          # 64^-0.25, the encoder's q / k column scale (csrc/engine.hip)


def philox(seed):
    return np.random.Generator(np.random.Philox(seed))


# ---------------------------------------------------------------------------------------------- arithmetic
def r16(x: torch.Tensor) -> torch.Tensor:
    """A rounding point: float64 -> fp32 -> fp16, back in float64."""
    return x.to(torch.float32).to(torch.float16).to(torch.float64)


def gelu64(x: torch.Tensor, kind: int) -> torch.Tensor:
    """kind 1: exact erf GELU; kind 2: the tanh formula.  float64 in, float64 out."""
    x = x.to(torch.float64)
    if kind == 1:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if kind == 2:
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)))
    raise ValueError(f"gelu kind {kind}")


def epilogue_ref(sums, bias=None, act=0, colscale_n=0, colscale=1.0, residual=None, res_mod=0):
    """The Linear epilogue on float64 sums [M, N], rounding points in the kernels' order:
    1. fp16(sum + bias)   2. fp16(act(.))   3. columns < colscale_n: fp16(. * colscale)   4. fp16(. + residual[row % res_mod or row])
    Returns float64 holding fp16 values."""
    M, N = sums.shape
    v = sums.to(torch.float64)
    if bias is not None:
        v = v + bias.to(torch.float64)[None, :N]
    v = r16(v)
    if act:
        v = r16(gelu64(v, act))
    if colscale_n > 0:
        sc = float(np.float32(colscale))                     # the kernel's scale is an fp32 argument
        v = torch.cat([r16(v[:, :colscale_n] * sc), v[:, colscale_n:]], dim=1)
    if residual is not None:
        rows = torch.arange(M, device=v.device)
        if res_mod > 0:
            rows = rows % res_mod
        v = r16(v + residual.to(torch.float64)[rows, :N])
    return v


def gemm_ref(A, W, **kw):
    """C = epilogue(A . W^T): A [M, K], W [N, K] fp16 values, the product in float64."""
    return epilogue_ref(A.to(torch.float64) @ W.to(torch.float64).T, **kw)


def head_split(c, B, T, H):
    """Row-major [B * T, 2 * H * 64] -> [B, 2, H, T, 64] (K | V side by side in a row, heads of 64 channels)."""
    return c.reshape(B, T, 2, H, 64).permute(0, 2, 3, 1, 4).contiguous()


def head_split_half(c, B, T, H):
    """Row-major [B * T, H * 64] -> [B, H, T, 64]: one of the two halves (hs_kv = 0 or 1)."""
    return c.reshape(B, T, H, 64).permute(0, 2, 1, 3).contiguous()


def quant_codes(x, inv_scale):
    """sat_s8(rne(fp16 value * inv_scale)), the product in fp32 as the kernels form it."""
    y = torch.round(x.to(torch.float32) * float(np.float32(inv_scale)))
    return torch.clamp(y, -128, 127).to(torch.int8)


def conv1d_gelu_ref(x_bct, w, b, stride, gelu_kind, pos=None):
    """Conv1d (kernel 3, padding 1, stride 1 | 2) + GELU [+ pos[t]] as the encoder runs it: x [B, C_in, T], w [C_out, C_in, 3],
    b [C_out], pos [T_out, C_out].  Returns token-major float64 [B, T_out, C_out] holding fp16 values."""
    y = torch.nn.functional.conv1d(x_bct.to(torch.float64), w.to(torch.float64), None, stride=stride, padding=1)
    v = r16(y.transpose(1, 2) + b.to(torch.float64)[None, None, :])
    v = r16(gelu64(v, gelu_kind))
    if pos is not None:
        v = r16(v + pos.to(torch.float64)[None])
    return v


def pad_token_major(x_bct, slack=512):
    """[B, C, T] -> the flat fp16 buffer the engine convolves: [B][T + 2][C] with zero rows 0 and T + 1, then `slack` finite elements."""
    B, Cn, T = x_bct.shape
    buf = torch.zeros(B * (T + 2) * Cn + slack, dtype=torch.float16)
    buf[:B * (T + 2) * Cn].view(B, T + 2, Cn)[:, 1:T + 1] = x_bct.transpose(1, 2).to(torch.float16)
    return buf


def layernorm_ref(x, g, b, eps=1e-5):
    """LayerNorm over the last axis in float64 (biased variance), one rounding at the end."""
    x = x.to(torch.float64)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return r16((x - mean) / torch.sqrt(var + eps) * g.to(torch.float64) + b.to(torch.float64))


def row_finish_ref(part, bias, mode, gelu_kind=1, x=None, g=None, b=None):
    """The row kernel of the split-K decode path: y16 = fp16(sum_s part[s] + bias), then by mode
    0: x = fp16(x + y16), out = LayerNorm(x)    1: out = fp16(gelu(y16))    2: out = LayerNorm(x)    3: x = fp16(x + y16).
    part [ksplit, M, N] fp32.  Returns {"x": ..., "out": ...} (float64 holding fp16 values; absent keys are None)."""
    res = {"x": None, "out": None}
    if mode != 2:
        y = part.to(torch.float64).sum(0)
        if bias is not None:
            y = y + bias.to(torch.float64)[None, :]
        y16 = r16(y)
        if mode == 1:
            res["out"] = r16(gelu64(y16, gelu_kind))
            return res
        res["x"] = r16(x.to(torch.float64) + y16)
    else:
        res["x"] = x.to(torch.float64)
    if mode in (0, 2):
        res["out"] = layernorm_ref(res["x"], g, b)
    return res


def embed_ref(E, pos, tokens, L, T=0):
    """x[r] = fp16(E[token of row r] + pos[r % L + T]); tokens [B, ld]: row r = (b, l) reads column l + T; ids clamped to the table."""
    B = tokens.shape[0]
    tok = tokens[:, T:T + L].reshape(-1).to(torch.long).clamp(0, E.shape[0] - 1)
    rows = (torch.arange(B * L) % L + T).to(torch.long)
    return r16(E[tok].to(torch.float64) + pos[rows].to(torch.float64))


def mel_transpose_pad_ref(mel):
    """[B, n_mels, T] -> [B, T + 2, n_mels] with zero rows 0 and T + 1."""
    B, n, T = mel.shape
    out = np.zeros((B, T + 2, n), dtype=mel.dtype)
    out[:, 1:T + 1] = mel.transpose(0, 2, 1)
    return out


def fp16_tol(ref):
    """The project's bound for an fp16 output: one fp16 ulp of the output magnitude (tests/test_gpu_kernels.py::test_gemm_big)."""
    return 2.0 ** -10 * max(1.0, float(ref.abs().max()))


def exact_grid(r, shape, steps, step):
    """Values k * step, |k| <= steps: sums of a few of them are exact in fp32 in any order."""
    return (r.integers(-steps, steps + 1, size=shape) * step).astype(np.float32)


# ---------------------------------------------------------------------------------------------- decode attention
def qkv_rows_ref(part, bias=None):
    """The prologue of the decode attention kernels: fp16(sum_s part[s] + bias).  part [ksplit, M, N] fp32, bias [N] fp16 or None."""
    y = part.to(torch.float64).sum(0)
    if bias is not None:
        y = y + bias.to(torch.float64)[None, :]
    return r16(y)


def attn_decode_ref(q, K, V, mask=None, k_exact=False):
    """The contract at the top of csrc/attn_decode.hip.  q [B, H, L, 64], K / V [B, H, Tk, 64] (fp16 values, or the exact products
    code * t of the int8 cross mode), mask [L, Tk] additive (0 | -inf) or None.  qh = fp16(q s), kh = fp16(k s) with s = 64^-0.25 as
    fp32 (k_exact: kh = k s, not rounded); scores fp16(qh . kh); softmax in float64, probabilities through fp16; out = fp16(P . V).
    Returns float64 [B, H, L, 64] holding fp16 values."""
    s = float(np.float32(QK_SCALE))
    qh = r16(q.to(torch.float64) * s)
    kh = K.to(torch.float64) * s
    if not k_exact:
        kh = r16(kh)
    sc = r16(qh @ kh.transpose(-1, -2))
    if mask is not None:
        sc = sc + mask.to(torch.float64)
    return r16(r16(torch.softmax(sc, dim=-1)) @ V.to(torch.float64))


def self_cache_codes(x, t):
    """The int8 self-attention cache: sat_s8(rne(x * (1 / t))), 1 / t formed in fp32."""
    return quant_codes(x, np.float32(1.0) / np.float32(t))


def self_cache_values(codes, t):
    """What a cached code is worth as a past key / value: fp16(code * t)."""
    return r16(codes.to(torch.float64) * float(np.float32(t)))


def cross_i8_values(codes, t):
    """int8 cross K/V: exactly code * t (no rounding of the dequantised tensor)."""
    return codes.to(torch.float64) * float(np.float32(t))


def split_heads(rows, B, L, H):
    """[B * L, H * 64] -> [B, H, L, 64]."""
    return rows.reshape(B, L, H, 64).permute(0, 2, 1, 3)


def merge_heads(x):
    """[B, H, L, 64] -> [B * L, H * 64]."""
    B, H, L, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * L, H * 64)


def attn_self_ref(rows, past_vals, B, L, T, H):
    """Decode self-attention on the fp16 rows [B * L, 3 * H * 64] (q | k | v) over past_vals [B, 2, H, T, 64] (the VALUES of the cached
    slots: fp16, or self_cache_values of the codes) followed by the call's own k / v, causal inside the call.  -> [B * L, H * 64]."""
    C = H * 64
    q, k, v = (split_heads(rows[:, i * C:(i + 1) * C], B, L, H) for i in range(3))
    K = torch.cat([past_vals[:, 0].to(torch.float64), k], dim=2)
    V = torch.cat([past_vals[:, 1].to(torch.float64), v], dim=2)
    mask = torch.zeros(L, T + L, dtype=torch.float64)
    mask[:, T:] = torch.full((L, L), float("-inf"), dtype=torch.float64).triu_(1)
    return merge_heads(attn_decode_ref(q, K, V, mask))


def amax_ref(rows):
    """The calibration hook: max |q|, |k|, |v| of the fp16 rows the launch processes (before the d^-0.25 scale), as fp32."""
    return np.float32(float(rows.abs().max()))


def ordinary_slabs(r, ksplit, M, N):
    """Random fp32 slabs off any grid, scaled by 1 / sqrt(ksplit), and a small fp16 bias: fp16(sum + bias) has about unit variance, like
    the inputs of tests/test_gpu_kernels.py::test_attn_decode_* whose bounds the ordinary-sum tests use.  -> part [ksplit, M, N], bias [N]"""
    part = (r.standard_normal((ksplit, M, N)) / math.sqrt(ksplit)).astype(np.float32)
    bias = (r.standard_normal(N) * 0.1).astype(np.float16)
    return torch.from_numpy(part), torch.from_numpy(bias)


def boundary_excused(part, bias=None):
    """Elements of fp16(sum_s part[s] + bias) whose fp16 rounding may legitimately depend on the ORDER of the fp32 additions: the
    float64 sum lies within one fp32 ulp of an fp16 rounding boundary (a midpoint of two neighbouring fp16 values).  The ulp is taken
    at A = sum_s |part[s]| + |bias|, which bounds every partial sum in every order: each fp32 addition is off by at most half an ulp of
    its own result, and no result exceeds A.  Computed from the float64 sum alone.  -> bool [M, N]."""
    p64 = part.to(torch.float64)
    y = p64.sum(0)
    A = p64.abs().sum(0)
    if bias is not None:
        y = y + bias.to(torch.float64)[None, :]
        A = A + bias.to(torch.float64).abs()[None, :]
    h = y.to(torch.float32).to(torch.float16)
    inf = torch.tensor(float("inf"), dtype=torch.float16)
    up, dn = torch.nextafter(h, inf).to(torch.float64), torch.nextafter(h, -inf).to(torch.float64)
    h = h.to(torch.float64)
    dist = torch.minimum((y - (h + up) / 2).abs(), (y - (h + dn) / 2).abs())
    ulp = torch.exp2(torch.floor(torch.log2(A.clamp_min(2.0 ** -126))) - 23)
    return dist <= ulp


# ---------------------------------------------------------------------------------------------- dispatch, restated
SMALL_TILES_DEFAULT, TINY_TILES = 150, 160
FORMS = ("f16<8,256>", "f16<8,128>", "f16<4,128>", "f16<2,128>")      # gemm_f16_kernel<NWAVE, BN>: 256x256, 256x128, 128x128, 64x128 tiles


def gemm_dispatch(M, N, K, small_tiles, act=0, residual=False, colscale=False, out_mode=0, q8=False, c_rows=0, res_mod=0,
                  max_wgs=0, aligned=True):
    """Which kernel template launch_gemm_f16 reaches (csrc/gemm_f16.hip, csrc/gemm_f16p.hip), as (kernel, act, epilogue variant)."""
    few = max_wgs <= 0 and N % 128 == 0 and ((M + 255) // 256) * ((N + 255) // 256) < small_tiles
    if not few and N % 256 == 0 and N <= 8192 and K % 64 == 0 and K >= 128:
        hs_fast = out_mode == 1 and act == 0 and not residual and not colscale
        simple = ((out_mode == 0 or hs_fast) and c_rows == 0 and res_mod == 0 and not q8 and not (residual and colscale)
                  and (act == 0 or (not residual and not colscale)) and aligned)
        if not simple:
            return ("f16p", act, "general+res" if residual else "general")
        if act != 0:
            return ("f16p", act, "simple")
        return ("f16p", 0, "simple+hs" if out_mode == 1 else "simple+res" if residual else "simple+scale" if colscale else "simple")
    tiles128 = ((M + 127) // 128) * (N // 128)
    form = (3 if tiles128 <= TINY_TILES else 2) if few else (0 if N % 256 == 0 else 1)
    return (FORMS[form], act, "head-split" if out_mode == 1 else "row-major")


def every_gemm_instantiation():
    """The kernel templates a shipped call can reach: four tile forms x three activations of gemm_f16_kernel, the general persistent
    kernel x three activations x (with | without residual), and the SIMPLE persistent kernel's five epilogues + its two GELU forms."""
    want = {(f, a) for f in FORMS for a in range(3)}
    want |= {("f16p", a, v) for a in range(3) for v in ("general", "general+res")}
    want |= {("f16p", 0, v) for v in ("simple", "simple+res", "simple+scale", "simple+hs")}
    want |= {("f16p", 1, "simple"), ("f16p", 2, "simple")}
    return want


# shapes of the activation matrix: (M, N, K) -> persistent | 64x128, persistent | 128x128, 256x128 | 64x128, 256x256 (K = 64: the
# persistent kernel declines) | 64x128, 256x128 | 128x128
ACT_SHAPES = [(1500, 1280, 1280), (3000, 1280, 128), (300, 384, 64), (520, 512, 64), (2900, 1152, 192)]
ACT_CASES = [(M, N, K, act, res, sc) for (M, N, K) in ACT_SHAPES for act, res, sc in itertools.product((0, 1, 2), (False, True), (False, True))]
ALIGN_SHAPE = (1500, 1280, 256)
RAGGED_M = [1, 63, 65, 255, 257, 1500]
HEAD_SPLIT_CASES = [(3, 1500, 2), (7, 100, 2), (4, 256, 2), (2, 1500, 20)]       # (B, hs_T, H): N = 2 * H * 64


# ---------------------------------------------------------------------------------------------- the persistent kernel's tile order
def band_order(M, N, K, tile_rows, xcd):
    """gemm_f16p_kernel's tile_of(): the tiles (row panel, channel tile) of XCD `xcd`'s band, in the order the band is walked, and what
    the band looks like: tiles of a partial head / tail tile row, full tile rows, and whether its last super-row is short."""
    nt_n, nt_m = N // 256, (M + 255) // 256
    n_tiles = nt_n * nt_m
    band = (n_tiles + 7) >> 3
    lo = min(n_tiles, xcd * band)
    hi = min(n_tiles, lo + band)
    R = tile_rows if tile_rows > 0 else max(1, min(8, (2816 << 10) // (K * 256 * 2)))
    row_first, row_last = (lo + nt_n - 1) // nt_n, hi // nt_n
    q_head = min(hi, row_first * nt_n) - lo
    q_mid = max(0, row_last - row_first) * nt_n
    order = []
    for q in range(hi - lo):
        if q < q_head:
            tile = lo + q
            order.append((tile // nt_n, tile % nt_n))
            continue
        q2 = q - q_head
        if q2 >= q_mid:
            tile = row_last * nt_n + (q2 - q_mid)
            order.append((tile // nt_n, tile % nt_n))
            continue
        sr, rem = divmod(q2, R * nt_n)
        rows_here = min(R, (row_last - row_first) - sr * R)
        tn = rem // rows_here
        order.append((row_first + sr * R + (rem - tn * rows_here), tn))
    full_rows = max(0, row_last - row_first)
    shape = {"tiles": hi - lo, "head": q_head, "tail": (hi - lo) - q_head - q_mid, "full_rows": full_rows,
             "short_last_super_row": full_rows > 0 and full_rows % R != 0, "lo": lo, "hi": hi, "nt_n": nt_n}
    return order, shape


# (M, N, K): 185 tiles in bands of 24 (heads of 1-4 tiles, tails, four full rows: short last super-row at R = 3 and 8; a ragged
# last row panel), 20 tiles in bands of 3 (no band holds a full tile row), 130 tiles of 10 channel tiles in bands of 17
TILE_ORDER_SHAPES = [(256 * 37 - 100, 1280, 128), (1024, 1280, 128), (256 * 13, 2560, 128)]
TILE_ROWS = [1, 2, 3, 8]
CU_BUDGET_SHAPES = [(6000, 1280, 1280), (12000, 2560, 1280)]
CU_BUDGETS = [1, 8, 20, 64, 100]


# ---------------------------------------------------------------------------------------------- decode attention: dispatch, cases
ATTN_KSPLITS = [1, 2, 3, 4, 5, 7, 8]              # every ksplit % 4, odd and even: full rounds of four, half rounds, scalar tails
CROSS_VARIANTS = ("fp16", "fp16+SKIP", "int8")
SELF_MAX_T, CROSS_MAX_KEYS, CROSS_MAX_SPLIT = 512, 1536, 16


def self_dispatch(int8_kv, row_start, waves):
    """launch_attn_self (csrc/attn_decode.hip): (I8, RS, form) of the kernel template a call reaches."""
    return (bool(int8_kv), bool(row_start), "workgroup" if waves == 4 else "one-wave")


def every_self_instantiation():
    return {(i8, rs, form) for i8 in (False, True) for rs in (False, True) for form in ("one-wave", "workgroup")}


def cross_per_split(Tk, nsplit):
    """Keys per split: the share rounded up to a multiple of 8 (attn_cross_kernel)."""
    return (((Tk + nsplit - 1) // nsplit) + 7) & ~7


def cross_empty_splits(Tk, nsplit):
    per = cross_per_split(Tk, nsplit)
    return sum(1 for sp in range(nsplit) if min(Tk, sp * per + per) - sp * per <= 0)


def cross_uq(L, int8):
    """Slabs per round of attn_cross_kernel's q prologue (even, at least 2)."""
    qv = 4 if int8 else 2
    return max(8 // (L * qv), 2)


def cross_dispatch(L, int8, skip, nsplit, H, B, n_cu):
    """launch_attn_cross: the kernel template (L, variant), the launch form and grid, and whether the combine kernel runs.  The grid is
    sized from B (not from a live-row list): one workgroup per (head, row, split) item, or -- from four items per CU -- at most two
    workgroups per CU, every one with the same number of items."""
    variant = "int8" if int8 else ("fp16+SKIP" if skip and nsplit == 1 else "fp16")
    n_items = H * B * nsplit
    wgs = 0
    if n_items >= 4 * n_cu:
        per = (n_items + 2 * n_cu - 1) // (2 * n_cu)
        wgs = (n_items + per - 1) // per
    grid = wgs if 0 < wgs < n_items else n_items
    return {"kernel": (L, variant), "launch": "persistent" if grid < n_items else "per-item", "grid": grid, "items": n_items,
            "combine": nsplit > 1}


def every_cross_instantiation():
    return {(L, v) for L in (1, 2, 3, 4) for v in CROSS_VARIANTS}


def persistent_batch(n_cu, H=2, nsplit=8):
    """The smallest B whose H * B * nsplit items make the launch persistent on a device of n_cu CUs."""
    return (4 * n_cu + H * nsplit - 1) // (H * nsplit)


def _self_exact_cases():
    """(ksplit, int8_kv, waves, rs, L, T, bias, strided, ldp_pad, ldo_pad, inplace): every ksplit x cache type x wave form x T; the
    other axes cycle with co-prime periods so that every value of every axis occurs (tests/test_kernel_refs_cpu.py counts them)."""
    cases, n = [], 0
    for ks in ATTN_KSPLITS:
        for i8 in (0, 1):
            for waves in (1, 4):
                for T in (0, 5, 64, 130):
                    L = (1, 3, 4)[n % 3]
                    cases.append((ks, i8, waves, 0, L, T, (n // 3) % 2 == 0, (n // 5) % 2 == 1, 4 * ((n // 2) % 2), 8 * ((n // 7) % 2),
                                  (n // 4 + n) % 2 == 0))
                    n += 1
    for ks in (4, 7):                              # right-aligned rows through the new entry (in place, as the decode loop runs them)
        for i8 in (0, 1):
            for waves in (1, 4):
                cases.append((ks, i8, waves, 1, 3, 5, True, True, 4, 8, True))
    return cases


def _cross_exact_cases():
    """(ksplit, L, variant, nsplit, Tk, H, bias): every ksplit at every L and variant (each slabs-per-round value meets a full round, a
    half round and a tail); the V-skip form exists for the single pass only."""
    cases, n = [], 0
    for ks in ATTN_KSPLITS:
        for L in (1, 2, 3, 4):
            for v in CROSS_VARIANTS:
                nsplit = 1 if v == "fp16+SKIP" else (1, 3)[(n // 3) % 2]
                cases.append((ks, L, v, nsplit, (100, 333)[(n // 2 + n // 5) % 2], 1 + n % 3, n % 5 != 4))
                n += 1
    return cases


SELF_EXACT_CASES = _self_exact_cases()
CROSS_EXACT_CASES = _cross_exact_cases()
SELF_ROW_START = [3, 6]                            # B = 2, T = 5, L = 3: pad slots inside the cache | the cache all pad and one pad token
# (Tk, nsplit, H): key ranges shorter than a load instruction's 8 rows, empty splits (5 of 8, 3 of 16), the maximum key count
CROSS_EDGE_CASES = [(1, 1, 2), (5, 1, 3), (7, 1, 2), (8, 1, 1), (9, 1, 2), (20, 8, 2), (100, 16, 3), (1536, 1, 1), (1536, 16, 1)]
CROSS_LIVE_CASES = [(L, nsplit, v) for L in (1, 3) for nsplit in (1, 4) for v in ("fp16", "int8")]      # B = 4, live = [2; 3, 1]
# ordinary (order-dependent) sums: (ksplit, int8_kv, waves, L, T) and (ksplit, L, variant, nsplit, Tk)
SELF_SUM_CASES = [(ks, i8, waves, L, T) for ks in (4, 7) for i8 in (0, 1) for waves, L, T in ((1, 3, 5), (4, 1, 130))]
CROSS_SUM_CASES = [(ks, L, v, ns, Tk) for ks in (4, 7) for L, v, ns, Tk in ((1, "fp16", 1, 100), (4, "fp16", 3, 333), (3, "int8", 1, 333),
                                                                            (2, "fp16+SKIP", 1, 100), (1, "int8", 3, 100))]
SUM_SEED = 20240                                   # tests/test_kernel_refs_cpu.py: the excused share of every case at this seed
