"""The reference restatements of tests/kernel_refs.py, checked where no GPU exists: against torch's own operators (F.linear,
F.conv1d, F.gelu, F.layer_norm, F.embedding) and against the reference's recorded outputs (tests/golden/ops.npz).  Also on the
CPU: the restated launcher dispatch shows that the GPU case lists reach every kernel instantiation, and the restated tile order of
the persistent kernel is a bijection on the shapes the GPU tests run, with every branch of the order taken."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_refs as KR
import weight as W


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dtype) if dtype is not None else t


def test_r16_is_round_to_nearest_even_fp16():
    x = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65519.0, 2.0 ** -25, -0.1], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0 + 2.0 ** -9, 65504.0, 0.0, float(np.float16(-0.1))], dtype=torch.float64)
    assert torch.equal(KR.r16(x), want)


@pytest.mark.parametrize("kind,approx", [(1, "none"), (2, "tanh")])
def test_gelu_matches_torch(kind, approx):
    x = torch.linspace(-9, 9, 4001, dtype=torch.float64)
    assert float((KR.gelu64(x, kind) - F.gelu(x, approximate=approx)).abs().max()) < 1e-14


def test_gelu_matches_reference_golden(golden_dir):
    ops = np.load(os.path.join(golden_dir, "ops.npz"))
    got = KR.gelu64(_t(ops["gelu_x"]), 1)
    assert float((got - _t(ops["gelu_out"]).double()).abs().max()) < 1e-6          # the recorded outputs are fp32


@pytest.mark.parametrize("act,approx", [(0, None), (1, "none"), (2, "tanh")])
def test_gemm_ref_matches_torch_linear(act, approx):
    r = KR.philox(11 + act)
    A = _t((r.standard_normal((37, 192)) * 0.5).astype(np.float16))
    Wt = _t((r.standard_normal((128, 192)) / np.sqrt(192)).astype(np.float16))
    bias = _t((r.standard_normal(128) * 0.1).astype(np.float16))
    res = _t((r.standard_normal((37, 128)) * 0.5).astype(np.float16))
    y = F.linear(A.double(), Wt.double(), bias.double())
    want = y.half().double()
    if act:
        want = F.gelu(want, approximate=approx).half().double()
    got = KR.gemm_ref(A, Wt, bias=bias, act=act)
    assert torch.equal(got, want)
    # the column scale touches the first columns only, through one more rounding; the residual is one rounding of the sum
    sc = KR.QK_SCALE
    got = KR.gemm_ref(A, Wt, bias=bias, act=act, colscale_n=64, colscale=sc, residual=res)
    scaled = torch.cat([(want[:, :64] * float(np.float32(sc))).half().double(), want[:, 64:]], 1)
    assert torch.equal(got, (scaled + res.double()).half().double())
    # res_mod: residual row m % T
    got = KR.gemm_ref(A, Wt, bias=bias, act=act, residual=res[:10], res_mod=10)
    assert torch.equal(got, (want + res[:10].double().repeat(4, 1)[:37]).half().double())
    # no bias
    assert torch.equal(KR.gemm_ref(A, Wt), F.linear(A.double(), Wt.double()).half().double())


def test_head_split_is_the_reference_permutation():
    B, T, H = 3, 5, 2
    c = torch.arange(B * T * 2 * H * 64, dtype=torch.float64).reshape(B * T, 2 * H * 64)
    hs = KR.head_split(c, B, T, H)
    assert hs.shape == (B, 2, H, T, 64)
    for (b, kv, h, t, d) in [(0, 0, 0, 0, 0), (2, 1, 1, 4, 63), (1, 0, 1, 3, 17), (1, 1, 0, 2, 5)]:
        assert hs[b, kv, h, t, d] == c[b * T + t, kv * H * 64 + h * 64 + d]
    half = KR.head_split_half(c[:, :H * 64], B, T, H)
    assert torch.equal(half, hs[:, 0])


def test_quant_codes_match_the_oracle_and_saturate():
    from oracle.whisper_oracle import kv_quantize
    r = KR.philox(5)
    x = _t((r.standard_normal(4096) * 2).astype(np.float16))
    t = 1.0 / 64
    inv = float(np.float32(1.0) / np.float32(t))
    q = KR.quant_codes(x, inv)
    assert torch.equal(q, kv_quantize(x, t))
    assert int(q.max()) == 127 and int(q.min()) == -128
    assert KR.quant_codes(torch.tensor([0.5, 1.5, 2.5, -0.5]), 1.0).tolist() == [0, 2, 2, 0]      # ties to even


def test_conv_ref_matches_reference_golden(golden_dir):
    """conv1 (k3 s1 p1) and conv2 (k3 s2 p1) + GELU against the reference's recorded fp32 outputs: the restatement rounds its
    inputs, weights and two intermediate values to fp16, so it agrees to the bound the kernel test uses (4e-3)."""
    ops = np.load(os.path.join(golden_dir, "ops.npz"))
    x = _t(ops["conv_x"]).half()
    y1 = KR.conv1d_gelu_ref(x, _t(ops["conv1_w"]).half(), _t(ops["conv1_b"]).half(), 1, 1)
    assert float((y1.transpose(1, 2) - _t(ops["conv1_out"]).double()).abs().max()) < 4e-3
    y2 = KR.conv1d_gelu_ref(_t(ops["conv1_out"]).half(), _t(ops["conv2_w"]).half(), _t(ops["conv2_b"]).half(), 2, 1)
    assert y2.shape == (2, 10, 16)
    assert float((y2.transpose(1, 2) - _t(ops["conv2_out"]).double()).abs().max()) < 4e-3


@pytest.mark.parametrize("stride", [1, 2])
def test_conv_ref_matches_torch_and_the_gemm_view(stride):
    """The restated convolution equals F.conv1d + F.gelu, and equals the GEMM over the strided view of the zero-padded token-major
    buffer that the engine runs (weight.conv_weight_as_gemm, rows of stride * C_in elements): the two formulations the GPU tests use
    for the same operation agree before a kernel is involved."""
    r = KR.philox(70 + stride)
    B, Cin, T, Cout = 2, 16, 12, 8
    x = _t((r.standard_normal((B, Cin, T))).astype(np.float16))
    w = _t((r.standard_normal((Cout, Cin, 3)) / np.sqrt(3 * Cin)).astype(np.float16))
    b = _t((r.standard_normal(Cout) * 0.1).astype(np.float16))
    pos = _t((r.standard_normal((T // stride, Cout))).astype(np.float16))
    got = KR.conv1d_gelu_ref(x, w, b, stride, 2, pos=pos)
    y = F.conv1d(x.double(), w.double(), b.double(), stride=stride, padding=1).half().double()
    want = (F.gelu(y, approximate="tanh").half().double().transpose(1, 2) + pos.double()[None]).half().double()
    assert torch.equal(got, want)
    buf = KR.pad_token_major(x, slack=64)
    wg = _t(W.conv_weight_as_gemm(w.numpy()))                 # [C_out, K], K = 3 * C_in padded to 64
    K, To = wg.shape[1], T // stride
    rows = torch.stack([buf[bb * (T + 2) * Cin + t * stride * Cin:][:K] for bb in range(B) for t in range(To)])
    view = KR.gemm_ref(rows, wg, bias=b, act=2, residual=pos, res_mod=To).reshape(B, To, Cout)
    assert float((view - got).abs().max()) <= 2.0 ** -10          # same values up to the float64 summation order at a rounding tie


def test_layernorm_ref_matches_torch_and_golden(golden_dir):
    ops = np.load(os.path.join(golden_dir, "ops.npz"))
    x, g, b = _t(ops["ln_x"]), _t(ops["ln_w"]), _t(ops["ln_b"])
    want = F.layer_norm(x.double(), (x.shape[-1],), g.double(), b.double(), 1e-5)
    got = KR.layernorm_ref(x, g, b)
    assert torch.equal(got, want.half().double())
    assert float((got - _t(ops["ln_out"]).double()).abs().max()) <= 2.0 ** -10 * max(1.0, float(np.abs(ops["ln_out"]).max()))


@pytest.mark.parametrize("gelu_kind", [1, 2])
def test_row_finish_ref_modes(gelu_kind):
    r = KR.philox(90 + gelu_kind)
    ks, M, N = 5, 6, 128
    part = _t(KR.exact_grid(r, (ks, M, N), 512, 2.0 ** -10))
    bias = _t(KR.exact_grid(r, (N,), 256, 2.0 ** -10)).half()
    x = _t((r.standard_normal((M, N)) * 1.5).astype(np.float16))
    g, b = _t(r.uniform(0.5, 1.5, N).astype(np.float16)), _t(r.uniform(-0.5, 0.5, N).astype(np.float16))
    assert torch.equal(part.sum(0), part.flip(0).sum(0))                       # the grid: fp32 sums are exact in any order
    y16 = (part.double().sum(0) + bias.double()).half().double()
    x1 = (x.double() + y16).half().double()
    ln = lambda v: F.layer_norm(v, (N,), g.double(), b.double(), 1e-5).half().double()      # noqa: E731
    approx = "none" if gelu_kind == 1 else "tanh"
    m0 = KR.row_finish_ref(part, bias, 0, x=x, g=g, b=b)
    assert torch.equal(m0["x"], x1) and torch.equal(m0["out"], ln(x1))
    m1 = KR.row_finish_ref(part, bias, 1, gelu_kind=gelu_kind)
    assert m1["x"] is None and torch.equal(m1["out"], F.gelu(y16, approximate=approx).half().double())
    m2 = KR.row_finish_ref(None, None, 2, x=x, g=g, b=b)
    assert torch.equal(m2["out"], ln(x.double()))
    m3 = KR.row_finish_ref(part, None, 3, x=x)
    assert m3["out"] is None and torch.equal(m3["x"], (x.double() + part.double().sum(0).half().double()).half().double())


def test_embed_ref_matches_torch_embedding_and_the_tile_layout():
    r = KR.philox(33)
    V, Cn, B, L, T = 100, 64, 3, 2, 1
    E = (r.standard_normal((V, Cn))).astype(np.float16)
    pos = _t((r.standard_normal((L + T, Cn))).astype(np.float16))
    tokens = _t(r.integers(0, V, size=(B, 6)).astype(np.int32))
    tokens[0, 1] = -3
    tokens[1, 2] = V + 7                                                       # out of range: clamped to the table
    tiles = W.tile_linear(E)
    assert tiles.shape == ((V + 15) // 16, Cn // 32, 64, 8)
    E_back = _t(W.untile_linear(tiles, V))
    assert torch.equal(E_back, _t(E))
    got = KR.embed_ref(E_back, pos, tokens, L, T)
    tok = tokens[:, T:T + L].reshape(-1).long().clamp(0, V - 1)
    want = (F.embedding(tok, _t(E).double()) + pos.double()[T:T + L].repeat(B, 1)).half().double()
    assert torch.equal(got, want)
    assert torch.equal(KR.embed_ref(E_back, pos, tokens, L, 0)[1], (_t(E).double()[0] + pos.double()[1]).half().double())      # id -3 -> row 0 of the table


def test_mel_transpose_pad_ref():
    mel = np.arange(2 * 3 * 5, dtype=np.float16).reshape(2, 3, 5)
    out = KR.mel_transpose_pad_ref(mel)
    assert out.shape == (2, 7, 3) and not out[:, 0].any() and not out[:, 6].any()
    assert out[1, 4, 2] == mel[1, 2, 3]


# ---------------------------------------------------------------------------------------------- coverage of the case lists
def test_gpu_cases_reach_every_gemm_instantiation():
    """Every kernel template a shipped call can reach is hit by a case of tests/test_gpu_gemm_epilogue.py, by the launchers' own
    dispatch conditions (restated in kernel_refs.gemm_dispatch).  Every case runs under wm_set_gemm_small_tiles(0) and (1 << 30)."""
    reached = set()
    for small in (0, 1 << 30):
        for (M, N, K, act, res, sc) in KR.ACT_CASES:
            reached.add(KR.gemm_dispatch(M, N, K, small, act=act, residual=res, colscale=sc))
        for (B, T, H) in KR.HEAD_SPLIT_CASES:
            for act in (0, 1):
                reached.add(KR.gemm_dispatch(B * T, 2 * H * 64, 256, small, act=act, out_mode=1))
        M, N, K = KR.ALIGN_SHAPE                               # ldc = ldr = N + 4: the persistent kernel's general epilogue at act 0
        for res in (False, True):
            reached.add(KR.gemm_dispatch(M, N, K, small, residual=res, aligned=False))
    f16 = {(k, a) for (k, a, _) in reached if k != "f16p"}
    f16p = {c for c in reached if c[0] == "f16p"}
    want = KR.every_gemm_instantiation()
    assert {w for w in want if len(w) == 2} <= f16, sorted({w for w in want if len(w) == 2} - f16)
    assert {w for w in want if len(w) == 3} <= f16p, sorted({w for w in want if len(w) == 3} - f16p)
    # the shapes the issue names: both tiny and small forms, the 256 x 128 form and the K = 64 shape the persistent kernel declines
    assert KR.gemm_dispatch(520, 512, 64, 0)[0] == "f16<8,256>" and KR.gemm_dispatch(300, 384, 64, 0)[0] == "f16<8,128>"
    assert KR.gemm_dispatch(2900, 1152, 192, 1 << 30)[0] == "f16<4,128>" and KR.gemm_dispatch(1500, 1280, 1280, 1 << 30)[0] == "f16<2,128>"


@pytest.mark.parametrize("M,N,K", KR.TILE_ORDER_SHAPES + KR.CU_BUDGET_SHAPES)
def test_restated_tile_order_is_a_bijection(M, N, K):
    nt_n, nt_m = N // 256, (M + 255) // 256
    for R in [0] + KR.TILE_ROWS:
        seen = []
        for xcd in range(8):
            order, shape = KR.band_order(M, N, K, R, xcd)
            assert len(order) == shape["tiles"]
            seen += order
        assert sorted(seen) == [(tm, tn) for tm in range(nt_m) for tn in range(nt_n)], (M, N, K, R)


def test_tile_order_shapes_take_every_branch():
    """The band shapes of the GPU tile-order test, from tile_of()'s own tile counts: a partial head tile row, a partial tail tile
    row, a last super-row with fewer than R tile rows, and a band without any full tile row all occur."""
    seen = {"head": False, "tail": False, "short": False, "no_full_row": False, "mid_reordered": False}
    for (M, N, K) in KR.TILE_ORDER_SHAPES:
        for R in KR.TILE_ROWS:
            for xcd in range(8):
                order, s = KR.band_order(M, N, K, R, xcd)
                if s["tiles"] == 0:
                    continue
                seen["head"] |= s["head"] > 0
                seen["tail"] |= s["tail"] > 0
                seen["short"] |= s["short_last_super_row"]
                seen["no_full_row"] |= s["full_rows"] == 0
                plain = [((s["lo"] + q) // s["nt_n"], (s["lo"] + q) % s["nt_n"]) for q in range(s["tiles"])]
                seen["mid_reordered"] |= order != plain
                if R == 1:
                    assert order == plain                      # tile_rows = 1 is the plain row-major order
    assert all(seen.values()), seen


# ---------------------------------------------------------------------------------------------- decode attention
def _oracle(H, Tk):
    from oracle.whisper_oracle import Dims, OracleConfig, OracleModel
    return OracleModel(Dims(80, Tk, H * 64, H, 0, 8, 512, H * 64, H, 0), {}, OracleConfig(act="float16"))


ATTEND_SHAPES = [(2, 1, 2, 100), (2, 3, 2, 37), (1, 4, 3, 333), (3, 2, 1, 8)]          # (B, L, H, Tk)


def test_attn_decode_ref_agrees_with_the_oracle():
    """attn_decode_ref (float64 softmax and dot products) against OracleModel._attend (fp32) on four shapes x (no mask | causal over
    the last L keys) x (k rounded | k_exact): equal after the final fp16 rounding except where a value sits on a rounding boundary.
    Measured here: 20 of 8704 elements differ (at most 6 of one comparison's 768), by 1.2e-4 at most (one fp16 ulp of the value, or the
    little more that one SCORE rounded the other way moves an output).  The oracle ALONE is no steadier: with nothing but the order of
    its keys changed (two permutations per shape) 15 of 8704 of its own outputs change, at most 5 of 768 = 0.65 % -- so the bound is
    1 % of a comparison's elements, each within 2.5e-4: a quarter of the 1e-3 the kernels are held to against either reference."""
    total = differ = 0
    for seed, (B, L, H, Tk) in enumerate(ATTEND_SHAPES):
        r = KR.philox(seed)
        q, k, v = (_t(r.standard_normal((B, n, H * 64)).astype(np.float16)).float() for n in (L, Tk, Tk))
        heads = lambda x: x.view(B, -1, H, 64).permute(0, 2, 1, 3)                     # noqa: E731
        m = _oracle(H, Tk)
        causal = torch.zeros(L, Tk)
        causal[:, Tk - L:] = torch.full((L, L), float("-inf")).triu_(1)
        for mask in (None, causal):
            for k_exact in (False, True):
                want = m._attend(q, k, v, H, mask, k_exact=k_exact).double()
                got = KR.merge_heads(KR.attn_decode_ref(heads(q), heads(k), heads(v), mask, k_exact)).reshape(B, L, H * 64)
                bad = got != want
                assert float((got - want).abs().max()) <= 2.5e-4, (B, L, H, Tk, k_exact)
                assert int(bad.sum()) <= 0.01 * want.numel(), (B, L, H, Tk, k_exact, int(bad.sum()))
                total, differ = total + want.numel(), differ + int(bad.sum())
    assert differ <= 0.005 * total, (differ, total)


@pytest.mark.parametrize("int8_kv", [0, 1])
def test_attn_self_ref_agrees_with_the_oracle_over_a_cache(int8_kv):
    """The int8 cache of the reference: self_cache_codes / self_cache_values are kv_quantize / kv_dequantize exactly, and the causal
    attention over [cached values, this call's k / v] agrees with the oracle as above (measured: 0 and 2 of 768 elements differ)."""
    from oracle.whisper_oracle import kv_dequantize, kv_quantize
    B, L, T, H, t = 2, 3, 7, 2, 0.031
    r = KR.philox(5 + int8_kv)
    rows = _t(r.standard_normal((B * L, 3 * H * 64)).astype(np.float16))
    past = _t((r.standard_normal((B, 2, H, T, 64)) * 1.2).astype(np.float16))
    if int8_kv:
        codes = KR.self_cache_codes(past, t)
        assert torch.equal(codes, kv_quantize(past.float(), t))
        vals = KR.self_cache_values(codes, t)
        assert torch.equal(vals, kv_dequantize(codes, t, "float16").double())
        exact = KR.cross_i8_values(codes, t)                                           # code * t in float64: no rounding at all
        assert torch.equal(exact.float(), codes.float() * float(np.float32(t)))        # ... the oracle's fp32 product is its rounding
    else:
        vals = past.double()
    got = KR.attn_self_ref(rows.double(), vals, B, L, T, H)
    qkv = rows.float().reshape(B, L, 3, H, 64)
    full = torch.cat([vals.float(), qkv[:, :, 1:].permute(0, 2, 3, 1, 4)], dim=3)
    mask = torch.zeros(L, T + L)
    mask[:, T:] = torch.full((L, L), float("-inf")).triu_(1)
    k_all, v_all = (full[:, i].permute(0, 2, 1, 3).reshape(B, T + L, H * 64) for i in (0, 1))
    want = _oracle(H, 8)._attend(qkv[:, :, 0].reshape(B, L, H * 64), k_all, v_all, H, mask).double().reshape(B * L, H * 64)
    assert float((got - want).abs().max()) <= 2.5e-4
    assert int((got != want).sum()) <= 0.01 * want.numel()


def test_qkv_rows_and_amax_refs():
    r = KR.philox(9)
    part = _t(KR.exact_grid(r, (5, 4, 64), 600, 2.0 ** -10))
    bias = _t(KR.exact_grid(r, (64,), 256, 2.0 ** -10)).half()
    want = (part.double().sum(0) + bias.double()).half().double()                      # exact on the grid: one rounding
    assert torch.equal(KR.qkv_rows_ref(part, bias), want)
    assert torch.equal(KR.qkv_rows_ref(part[:1]), part[0].half().double())
    assert KR.amax_ref(want) == np.float32(want.abs().max()) and KR.amax_ref(want).dtype == np.float32
    # a sum that sits exactly on the midpoint of two fp16 values is excused, its neighbours half an fp16 step away are not
    mid = torch.tensor([[[1.0 + 2.0 ** -11, 1.0 + 2.0 ** -10, 1.0 + 2.0 ** -11 + 2.0 ** -24]]], dtype=torch.float32)
    assert KR.boundary_excused(mid).tolist() == [[True, False, True]]


def test_decode_attention_cases_reach_every_instantiation():
    """By the launchers' own dispatch (kernel_refs.self_dispatch / cross_dispatch): the exactness lists of
    tests/test_gpu_attn_decode_contract.py reach all 8 self-attention and all 12 cross-attention kernel templates, with and without the
    combine kernel, and the two launch forms -- per item at the lists' sizes on any device, persistent for persistent_batch(n_cu)."""
    self_seen = {}
    for (ks, i8, waves, rs, *_rest) in KR.SELF_EXACT_CASES:
        self_seen.setdefault(KR.self_dispatch(i8, rs, waves), set()).add(ks)
    assert set(self_seen) == KR.every_self_instantiation() and len(self_seen) == 8
    assert all(ks >= {4, 7} for ks in self_seen.values())
    assert all(self_seen[(i8, False, f)] == set(KR.ATTN_KSPLITS) for i8 in (False, True) for f in ("one-wave", "workgroup"))
    cross_seen, combine = {}, set()
    for n_cu in (64, 256, 304):
        for (ks, L, v, nsplit, Tk, H, bias) in KR.CROSS_EXACT_CASES:
            d = KR.cross_dispatch(L, v == "int8", v == "fp16+SKIP", nsplit, H, 2, n_cu)
            assert d["kernel"] == (L, v) and d["launch"] == "per-item" and d["grid"] == H * 2 * nsplit
            cross_seen.setdefault(d["kernel"], set()).add(ks)
            combine.add((v, d["combine"]))
        B = KR.persistent_batch(n_cu)
        d = KR.cross_dispatch(1, False, False, 8, 2, B, n_cu)
        assert d["launch"] == "persistent" and d["grid"] <= 2 * n_cu and d["items"] % d["grid"] == 0 or d["grid"] < d["items"]
        assert KR.cross_dispatch(1, False, False, 8, 2, B - 1, n_cu)["launch"] == "per-item"
    assert KR.persistent_batch(256) == 64
    assert set(cross_seen) == KR.every_cross_instantiation() and len(cross_seen) == 12
    assert all(ks == set(KR.ATTN_KSPLITS) for ks in cross_seen.values())
    assert combine == {("fp16", False), ("fp16", True), ("int8", False), ("int8", True), ("fp16+SKIP", False)}
    # slabs per round of the cross prologue: 4, 2, 2, 2 (fp16) and 2 (int8); every list value meets a full round, a half round, a tail
    assert [KR.cross_uq(L, False) for L in (1, 2, 3, 4)] == [4, 2, 2, 2] and {KR.cross_uq(L, True) for L in (1, 2, 3, 4)} == {2}
    for L, v in cross_seen:
        uq = KR.cross_uq(L, v == "int8")
        assert {ks % uq for ks in cross_seen[(L, v)]} >= set(range(min(uq, 4))), (L, v)
    # every value of the other axes of the self list occurs
    axes = list(zip(*KR.SELF_EXACT_CASES))
    assert set(axes[4]) == {1, 3, 4} and set(axes[5]) == {0, 5, 64, 130}
    assert all(set(axes[i]) == {False, True} for i in (6, 7, 10)) and set(axes[8]) == {0, 4} and set(axes[9]) == {0, 8}
    for ks in KR.ATTN_KSPLITS:                     # ... and every ksplit meets both values of the bias / stride axes, in both wave forms
        mine = [c for c in KR.SELF_EXACT_CASES if c[0] == ks and not c[3]]
        assert {c[5] for c in mine} == {0, 5, 64, 130} and {c[4] for c in mine} == {1, 3, 4}
        for i in (6, 7, 8, 9, 10):
            assert len({(c[2], c[i]) for c in mine}) == 4, (ks, i)
    axes = list(zip(*KR.CROSS_EXACT_CASES))
    assert set(axes[3]) == {1, 3} and set(axes[4]) == {100, 333} and set(axes[5]) == {1, 2, 3} and set(axes[6]) == {False, True}
    for lst in (KR.SELF_SUM_CASES, KR.CROSS_SUM_CASES):
        assert {c[0] for c in lst} == {4, 7}
    assert {KR.self_dispatch(i8, False, w) for (_, i8, w, _, _) in KR.SELF_SUM_CASES} == {c for c in KR.every_self_instantiation() if not c[1]}
    assert {v for (_, _, v, _, _) in KR.CROSS_SUM_CASES} == set(KR.CROSS_VARIANTS)


def test_ksplit_lists_cover_every_remainder():
    for lst in (KR.ATTN_KSPLITS, sorted({c[0] for c in KR.SELF_EXACT_CASES}), sorted({c[0] for c in KR.CROSS_EXACT_CASES})):
        assert {ks % 4 for ks in lst} == {0, 1, 2, 3} and any(ks % 2 for ks in lst) and min(lst) == 1
    assert {c[0] % 4 for c in KR.SELF_SUM_CASES} == {0, 3} and {c[0] % 4 for c in KR.CROSS_SUM_CASES} == {0, 3}


def test_split_lists_contain_empty_splits():
    def empty(Tk, nsplit):
        per_split = (((Tk + nsplit - 1) // nsplit) + 7) & ~7
        assert per_split == KR.cross_per_split(Tk, nsplit)
        n = sum(1 for sp in range(nsplit) if max(0, min(Tk, sp * per_split + per_split) - sp * per_split) == 0)
        assert n == KR.cross_empty_splits(Tk, nsplit)
        return n
    assert empty(20, 8) == 5 and empty(100, 16) == 3 and empty(1536, 16) == 0 and empty(64, 8) == 0
    edges = {(Tk, ns): empty(Tk, ns) for (Tk, ns, _) in KR.CROSS_EDGE_CASES}
    assert edges[(20, 8)] == 5 and edges[(100, 16)] == 3
    assert {Tk for (Tk, ns, _) in KR.CROSS_EDGE_CASES if ns == 1} >= {1, 5, 7, 8, 9, KR.CROSS_MAX_KEYS}
    assert (KR.CROSS_MAX_KEYS, KR.CROSS_MAX_SPLIT, 1) in KR.CROSS_EDGE_CASES
    assert all(H == 1 for (Tk, _, H) in KR.CROSS_EDGE_CASES if Tk > 333) and all(H <= 3 for (_, _, H) in KR.CROSS_EDGE_CASES)
    # the exactness and live-row lists split their keys without an empty split (that is the edge list's business)
    assert all(empty(Tk, ns) == 0 for (_, _, _, ns, Tk, _, _) in KR.CROSS_EXACT_CASES)


def test_ordinary_sum_seed_keeps_the_excused_share_small():
    """The ordinary-sum GPU tests excuse an appended cache element only where boundary_excused() says the fp32 order may decide its
    rounding; from the reference alone, at the seed those tests use, that is well under 1 % of every case's elements (measured:
    0.13 % .. 0.52 %), and the rows have about unit variance (the tolerances of the comparisons rest on O(1) values)."""
    for (ks, i8, waves, L, T) in KR.SELF_SUM_CASES:
        part, bias = KR.ordinary_slabs(KR.philox(KR.SUM_SEED + ks), ks, 2 * L, 3 * 128)
        share = float(KR.boundary_excused(part, bias).double().mean())
        assert share < 0.01, (ks, L, share)
        assert 0.9 < float(KR.qkv_rows_ref(part, bias).std()) < 1.1
