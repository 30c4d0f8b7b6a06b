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
