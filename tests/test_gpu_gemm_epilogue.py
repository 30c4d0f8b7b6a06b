"""Kernel-level parity of the fp16 MFMA GEMM with EVERY epilogue option the engines use (csrc/gemm_f16.hip, csrc/gemm_f16p.hip),
through the test-only entry wm_gemm_ex: the three activations, column scale, residual and res_mod, head-split fp16 and int8
output, strided views of A and C (the convolutions), CU budgets, tile orders, unaligned leading dimensions, ragged M.

Reference: tests/kernel_refs.py -- float64 over the fp16 inputs with the kernels' rounding points, checked on the CPU by
tests/test_kernel_refs_cpu.py.  Bound for an fp16 output: one fp16 ulp of the output magnitude, 2**-10 * max(1, |ref|.max()), as
tests/test_gpu_kernels.py::test_gemm_big.  Where DESIGN.md and the header promise bit-identity (tile forms, CU budgets, tile
orders, output layouts) the raw bits are compared with torch.equal.

Every case runs twice, under wm_set_gemm_small_tiles(0) (the persistent kernel, or the 256-row forms where it declines) and under
wm_set_gemm_small_tiles(1 << 30) (128 x 128 or 64 x 128 tiles); the two runs must give equal bits.  Which kernel template each case
reaches is derived from the launchers' dispatch in tests/test_kernel_refs_cpu.py::test_gpu_cases_reach_every_gemm_instantiation.
Every output buffer is surrounded by a sentinel that must survive.

Kernel template -> a case that reaches it (from launch_gemm_f16 / launch_gemm_f16p's conditions, restated in kernel_refs.gemm_dispatch):

  gemm_f16_kernel<8, 256, act>  256 x 256      test_activation_residual_colscale_matrix[520-512-64-act-*]    (small_tiles 0; K = 64)
  gemm_f16_kernel<8, 128, act>  256 x 128      ...[300-384-64-act-*], ...[2900-1152-192-act-*]                (small_tiles 0; N % 256 != 0)
  gemm_f16_kernel<4, 128, act>  128 x 128      ...[3000-1280-128-act-*], ...[2900-1152-192-act-*]             (1 << 30; > 160 tiles)
  gemm_f16_kernel<2, 128, act>   64 x 128      ...[1500-1280-1280-act-*], ...[300-384-64-act-*]               (1 << 30; <= 160 tiles)
  gemm_f16p_kernel<0, SIMPLE>   plain | residual | column scale      ...[1500-1280-1280-0-False-False | 0-True-False | 0-False-True]
  gemm_f16p_kernel<0, SIMPLE>   head-split (16-byte stores)          test_head_split[0-*], test_cu_budget_is_bit_identical
  gemm_f16p_kernel<1|2, SIMPLE> GELU alone                           ...[1500-1280-1280-1|2-False-False]
  gemm_f16p_kernel<0>           general: residual + column scale, unaligned ldc / ldr, int8 head-split
                                                                     ...[1500-1280-1280-0-True-True], test_unaligned_ldc_and_ldr[0], test_head_split_int8
  gemm_f16p_kernel<1|2>         general: GELU + residual | column scale, c_rows, res_mod, head-split
                                ...[1500-1280-1280-1|2-True-*], test_conv1_strided_views_at_real_size[1280], test_conv2_...[1280], test_res_mod, test_head_split[1-*]
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_refs as KR  # noqa: E402
import native  # noqa: E402
import weight as W  # noqa: E402
from oracle.whisper_oracle import kv_quantize  # noqa: E402

FORMS = (0, 1 << 30)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return native.load_library()


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.cuda().contiguous()


def bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == torch.float16 else t


def data(seed, M, N, K, a_scale=0.5):
    r = KR.philox(seed)
    A = dev((r.standard_normal((M, K)) * a_scale).astype(np.float16))
    Wt = dev((r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float16))
    bias = dev((r.standard_normal(N) * 0.1).astype(np.float16))
    return r, A, Wt, bias


def gemm_ex(lib, A, Wt, M=None, lda=None, expect_rc=0, **kw):
    io = native.WmGemmIO()
    io.a, io.w = A.data_ptr(), Wt.data_ptr()
    io.m = A.shape[0] if M is None else M
    io.n, io.k = Wt.shape[0], Wt.shape[1]
    io.lda = (A.shape[1] if A.dim() == 2 else io.k) if lda is None else lda
    for k_, v in kw.items():
        assert hasattr(io, k_), k_
        setattr(io, k_, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    rc = lib.wm_gemm_ex(C.byref(io), stream())
    torch.cuda.synchronize()
    if expect_rc == 0:
        native.check(rc, "wm_gemm_ex")
    else:
        assert rc == expect_rc, (rc, lib.wm_last_error())
    return rc


def row_major(lib, A, Wt, M=None, pad=8, out_rows_extra=3, **kw):
    """One row-major run into a sentinel-filled [M + extra, N + pad] buffer (ldc = N + pad); the sentinel must survive past row
    M - 1 and outside the N columns.  Returns the [M, N] result."""
    M = A.shape[0] if M is None else M
    N = Wt.shape[0]
    out = torch.full((M + out_rows_extra, N + pad), KR.SENTINEL, dtype=torch.float16, device="cuda")
    gemm_ex(lib, A, Wt, M=M, c=out, ldc=N + pad, **kw)
    assert bool((out[M:] == KR.SENTINEL).all()), "written past row M - 1"
    assert bool((out[:, N:] == KR.SENTINEL).all()), "written outside the N columns"
    return out[:M, :N].contiguous()


def both_forms(lib, run):
    """run() under both tile-form settings; equal bits required.  Returns the result."""
    outs = []
    prev = lib.wm_set_gemm_small_tiles(-1)
    try:
        for tiles in FORMS:
            lib.wm_set_gemm_small_tiles(tiles)
            outs.append(run())
    finally:
        lib.wm_set_gemm_small_tiles(prev)
    assert torch.equal(bits(outs[0]), bits(outs[1])), "the tile forms disagree"
    return outs[0]


def check_close(got, ref, what=""):
    err, tol = float((got.double() - ref).abs().max()), KR.fp16_tol(ref)
    print(f"{what} max|got - ref| = {err:.3e} (bound {tol:.3e})")
    assert err <= tol, (what, err, tol)


# ---------------------------------------------------------------------------------------------- activations x residual x column scale
@pytest.mark.parametrize("M,N,K,act,resid,scale", KR.ACT_CASES)
def test_activation_residual_colscale_matrix(lib, M, N, K, act, resid, scale):
    """All three activations, each with and without a residual and a column scale, on shapes that reach the five kernels: the
    persistent launcher picks every SIMPLE variant and the general form (act 0 with both, GELU with either)."""
    r, A, Wt, bias = data(M + N + K + 7 * act, M, N, K)
    res = dev((r.standard_normal((M, N)) * 0.5).astype(np.float16)) if resid else None
    cs_n = (N // 2) // 64 * 64 if scale else 0
    kw = dict(bias=bias, act=act)
    if resid:
        kw.update(residual=res, ldr=N)
    if scale:
        kw.update(colscale_n=cs_n, colscale=KR.QK_SCALE)
    got = both_forms(lib, lambda: row_major(lib, A, Wt, **kw))
    ref = KR.gemm_ref(A, Wt, bias=bias, act=act, colscale_n=cs_n, colscale=KR.QK_SCALE, residual=res)
    check_close(got, ref, f"act={act} resid={resid} scale={scale}")


@pytest.mark.parametrize("act", [0, 2])
def test_no_bias(lib, act):
    r, A, Wt, _ = data(5, 700, 512, 128)
    got = both_forms(lib, lambda: row_major(lib, A, Wt, act=act))
    check_close(got, KR.gemm_ref(A, Wt, act=act), "no bias")


# ---------------------------------------------------------------------------------------------- ragged M
@pytest.mark.parametrize("M", KR.RAGGED_M)
@pytest.mark.parametrize("N,K", [(512, 128), (384, 64)])
def test_ragged_m_writes_nothing_outside(lib, M, N, K):
    """M = 1, 63, 65, 255, 257, 1500: the last row panel clamps its loads and must not store; row_major() checks the sentinel past
    row M - 1 and outside ldc.  With a residual, whose clamped rows are read too."""
    r, A, Wt, bias = data(M + N, M, N, K)
    res = dev((r.standard_normal((M, N)) * 0.5).astype(np.float16))
    for kw in (dict(), dict(residual=res, ldr=N), dict(act=1)):
        got = both_forms(lib, lambda: row_major(lib, A, Wt, bias=bias, **kw))
        ref = KR.gemm_ref(A, Wt, bias=bias, act=kw.get("act", 0), residual=res if "residual" in kw else None)
        check_close(got, ref, f"M={M} {sorted(kw)}")


# ---------------------------------------------------------------------------------------------- column scale
@pytest.mark.parametrize("N,cs_n", [(3 * 384, 2 * 384), (3 * 512, 2 * 512), (3 * 1280, 2 * 1280), (512, 192)])
def test_colscale_boundary(lib, N, cs_n):
    """The encoder's QKV projection: columns < colscale_n (2C of 3C; and one boundary that is a multiple of 64 but not of 128, inside
    a wave's column block) are scaled, through one more rounding; the columns at or beyond it equal the unscaled run bit for bit, and
    the scaled ones are exactly fp16(unscaled * scale)."""
    M, K = 700, 128
    r, A, Wt, bias = data(N + cs_n, M, N, K, a_scale=1.0)
    plain = both_forms(lib, lambda: row_major(lib, A, Wt, bias=bias))
    scaled = both_forms(lib, lambda: row_major(lib, A, Wt, bias=bias, colscale_n=cs_n, colscale=KR.QK_SCALE))
    assert torch.equal(bits(scaled[:, cs_n:]), bits(plain[:, cs_n:])), "columns beyond colscale_n changed"
    want = KR.r16(plain[:, :cs_n].double() * float(np.float32(KR.QK_SCALE)))
    assert torch.equal(scaled[:, :cs_n].double(), want), "scaled columns are not fp16(unscaled * scale)"
    assert not torch.equal(bits(scaled[:, :cs_n]), bits(plain[:, :cs_n]))
    check_close(scaled, KR.gemm_ref(A, Wt, bias=bias, colscale_n=cs_n, colscale=KR.QK_SCALE), f"colscale_n={cs_n}")


# ---------------------------------------------------------------------------------------------- res_mod
@pytest.mark.parametrize("T,B,N,K,act", [(1500, 2, 1280, 128, 1), (100, 5, 512, 128, 2), (100, 3, 384, 64, 0), (1500, 2, 384, 128, 1)])
def test_res_mod(lib, T, B, N, K, act):
    """conv2's positional embedding: residual row m % T (T = 1500 and T = 100, B >= 2: row panels cross utterance boundaries)."""
    M = B * T
    r, A, Wt, bias = data(T + B + N, M, N, K)
    pos = dev((r.standard_normal((T, N))).astype(np.float16))
    got = both_forms(lib, lambda: row_major(lib, A, Wt, bias=bias, act=act, residual=pos, ldr=N, res_mod=T))
    ref = KR.gemm_ref(A, Wt, bias=bias, act=act, residual=pos, res_mod=T)
    check_close(got, ref, f"res_mod={T}")
    # the same rows with the residual spelled out: bit-identical
    full = pos.repeat(B, 1).contiguous()
    same = both_forms(lib, lambda: row_major(lib, A, Wt, bias=bias, act=act, residual=full, ldr=N))
    assert torch.equal(bits(got), bits(same))


# ---------------------------------------------------------------------------------------------- head-split
def head_split_run(lib, A, Wt, bias, B, T, H, act=0, q8=0.0, hs_kv=-1, **kw):
    n_out = B * 2 * H * T * 64
    dt = torch.int8 if q8 > 0 else torch.float16
    fill = 77 if q8 > 0 else KR.SENTINEL
    out = torch.full((n_out + 4096,), fill, dtype=dt, device="cuda")
    gemm_ex(lib, A, Wt, bias=bias, act=act, c=out, out_mode=1, hs_t=T, hs_h=H, hs_kv=hs_kv, q8_inv_scale=q8, **kw)
    assert bool((out[n_out:] == fill).all()), "written past the head-split tensor"
    return out[:n_out].view(B, 2, H, T, 64)


@pytest.mark.parametrize("B,T,H", KR.HEAD_SPLIT_CASES)
@pytest.mark.parametrize("act", [0, 1])
def test_head_split(lib, B, T, H, act):
    """The cross-K/V projection's [B, 2, H, T, 64] output (hs_kv = -1, N = 2 * H * 64): T = 1500 with B = 3 puts utterance
    boundaries inside 256-row tiles, T = 100 with B = 7 several utterances into one tile, T = 256 a boundary on every tile edge.
    Compared with the permuted reference, and bit for bit with the row-major run of the same GEMM, permuted.  act = 1 forces the
    persistent kernel's general form (act = 0: its 16-byte head-split stores)."""
    M, N, K = B * T, 2 * H * 64, 256
    r, A, Wt, bias = data(B * T + H + act, M, N, K)
    rm = both_forms(lib, lambda: row_major(lib, A, Wt, bias=bias, act=act))
    hs = both_forms(lib, lambda: head_split_run(lib, A, Wt, bias, B, T, H, act=act))
    assert torch.equal(bits(hs), bits(KR.head_split(rm, B, T, H))), "head-split bytes differ from the permuted row-major run"
    check_close(hs, KR.head_split(KR.gemm_ref(A, Wt, bias=bias, act=act), B, T, H), f"head-split B={B} T={T} H={H}")


@pytest.mark.parametrize("hs_kv", [0, 1])
def test_head_split_one_half(lib, hs_kv):
    """hs_kv = 0 | 1 with N = H * 64: only that half of [B, 2, H, T, 64] is written."""
    B, T, H, K = 3, 300, 4, 128
    r, A, Wt, bias = data(40 + hs_kv, B * T, H * 64, K)
    rm = both_forms(lib, lambda: row_major(lib, A, Wt, bias=bias))
    hs = both_forms(lib, lambda: head_split_run(lib, A, Wt, bias, B, T, H, hs_kv=hs_kv))
    assert torch.equal(bits(hs[:, hs_kv]), bits(KR.head_split_half(rm, B, T, H)))
    assert bool((hs[:, 1 - hs_kv] == KR.SENTINEL).all()), "the other half was written"


@pytest.mark.parametrize("B,T,H", [(3, 1500, 2), (7, 100, 2), (2, 256, 4)])
def test_head_split_int8(lib, B, T, H):
    """int8 cross K/V: every code equals the oracle's kv_quantize of the fp16 head-split output of the same configuration, and is
    within 1 LSB of the float64 reference's code; the scale makes values saturate at both ends."""
    M, N, K = B * T, 2 * H * 64, 256
    r, A, Wt, bias = data(B * T + 3 * H, M, N, K, a_scale=1.0)
    t = float(np.float32(1.0 / 100.0))                       # outputs are ~N(0, 1): +-1.27 and beyond saturate
    inv = float(np.float32(1.0) / np.float32(t))
    hs = both_forms(lib, lambda: head_split_run(lib, A, Wt, bias, B, T, H))
    q = both_forms(lib, lambda: head_split_run(lib, A, Wt, bias, B, T, H, q8=inv))
    want = kv_quantize(hs.cpu(), t)
    assert torch.equal(q.cpu(), want), "codes differ from kv_quantize(fp16 output)"
    assert torch.equal(want, KR.quant_codes(hs.cpu(), inv))
    assert int(q.max()) == 127 and int(q.min()) == -128, "no saturation at both ends"
    assert float(((q != 127) & (q != -128)).float().mean()) > 0.5
    ref_q = KR.quant_codes(KR.head_split(KR.gemm_ref(A, Wt, bias=bias), B, T, H), inv)
    assert int((q.int() - ref_q.int()).abs().max()) <= 1


# ---------------------------------------------------------------------------------------------- strided views: the convolutions
@pytest.mark.parametrize("Cn", [384, 1280])
def test_conv1_strided_views_at_real_size(lib, Cn):
    """conv1 as the encoder runs it: n_mels = 80, K = 256, T_in = 3000, B = 2, a_rows and c_rows, written into the padded
    [B][T_in + 2][C] buffer at offset C.  The pad rows keep their sentinel; wm_zero_pad_rows then zeroes exactly rows 0 and T_in + 1
    of every utterance."""
    B, n_mels, Tin = 2, 80, 3000
    r = KR.philox(Cn)
    x = torch.from_numpy(r.standard_normal((B, n_mels, Tin)).astype(np.float16))
    w = torch.from_numpy((r.standard_normal((Cn, n_mels, 3)) / np.sqrt(3 * n_mels)).astype(np.float16))
    b = torch.from_numpy((r.standard_normal(Cn) * 0.1).astype(np.float16))
    xp, wg, bd = dev(KR.pad_token_major(x)), dev(W.conv_weight_as_gemm(w.numpy())), dev(b)
    assert wg.shape == (Cn, 256)
    ref = KR.conv1d_gelu_ref(x, w, b, 1, 1)                    # [B, Tin, C] on the CPU

    def run():
        out = torch.full((B * (Tin + 2) * Cn + 1024,), KR.SENTINEL, dtype=torch.float16, device="cuda")
        gemm_ex(lib, xp, wg, M=B * Tin, lda=n_mels, bias=bd, act=1, c=out.data_ptr() + 2 * Cn, ldc=Cn,
                a_rows=Tin, a_bstride=(Tin + 2) * n_mels, c_rows=Tin, c_bstride=(Tin + 2) * Cn)
        return out
    out = both_forms(lib, run)
    assert bool((out[B * (Tin + 2) * Cn:] == KR.SENTINEL).all())
    buf = out[:B * (Tin + 2) * Cn].view(B, Tin + 2, Cn)
    assert bool((buf[:, 0] == KR.SENTINEL).all()) and bool((buf[:, Tin + 1] == KR.SENTINEL).all()), "a pad row was written"
    check_close(buf[:, 1:Tin + 1].cpu(), ref, f"conv1 C={Cn}")
    before = out.clone()
    native.check(lib.wm_zero_pad_rows(out.data_ptr(), B, Tin + 2, Cn, stream()), "wm_zero_pad_rows")
    torch.cuda.synchronize()
    want = before.clone()
    wv = want[:B * (Tin + 2) * Cn].view(B, Tin + 2, Cn)
    wv[:, 0] = 0
    wv[:, Tin + 1] = 0
    assert torch.equal(bits(out), bits(want)), "wm_zero_pad_rows touched something else, or not the pad rows"


@pytest.mark.parametrize("Cn", [384, 1280])
def test_conv2_strided_view_with_res_mod_at_real_size(lib, Cn):
    """conv2: stride 2 (lda = 2C, a_rows = T), GELU, then the positional embedding through res_mod = T."""
    B, Tin = 2, 3000
    T = Tin // 2
    r = KR.philox(Cn + 2)
    x = torch.from_numpy((r.standard_normal((B, Cn, Tin)) * 0.5).astype(np.float16))
    w = torch.from_numpy((r.standard_normal((Cn, Cn, 3)) / np.sqrt(3 * Cn)).astype(np.float16))
    b = torch.from_numpy((r.standard_normal(Cn) * 0.1).astype(np.float16))
    pos = torch.from_numpy((r.standard_normal((T, Cn)) * 0.5).astype(np.float16))
    xp, wg, bd, pd = dev(KR.pad_token_major(x)), dev(W.conv_weight_as_gemm(w.numpy())), dev(b), dev(pos)
    assert wg.shape == (Cn, 3 * Cn)
    ref = KR.conv1d_gelu_ref(x, w, b, 2, 1, pos=pos).reshape(B * T, Cn)
    got = both_forms(lib, lambda: row_major(lib, xp, wg, M=B * T, lda=2 * Cn, bias=bd, act=1, a_rows=T, a_bstride=(Tin + 2) * Cn,
                                            residual=pd, ldr=Cn, res_mod=T))
    check_close(got.cpu(), ref, f"conv2 C={Cn}")


# ---------------------------------------------------------------------------------------------- CU budgets
@pytest.mark.parametrize("M,N,K", KR.CU_BUDGET_SHAPES)
def test_cu_budget_is_bit_identical(lib, M, N, K):
    """max_wgs in {1, 8, 20, 64, 100} against 0 (several tiles per workgroup): the same tiles and arithmetic, fewer workgroups
    walking over them -- plain, with a residual, and head-split."""
    r, A, Wt, bias = data(M + N, M, N, K)
    res = dev((r.standard_normal((M, N)) * 0.5).astype(np.float16))
    T = 1500
    B, H = M // T, N // 128
    variants = {"plain": lambda mw: row_major(lib, A, Wt, bias=bias, max_wgs=mw),
                "residual": lambda mw: row_major(lib, A, Wt, bias=bias, residual=res, ldr=N, max_wgs=mw),
                "head-split": lambda mw: head_split_run(lib, A, Wt, bias, B, T, H, max_wgs=mw)}
    for name, run in variants.items():
        base = both_forms(lib, lambda: run(0))
        for mw in KR.CU_BUDGETS:
            got = both_forms(lib, lambda: run(mw))
            assert torch.equal(bits(got), bits(base)), (name, mw)
        if name == "residual":
            check_close(base, KR.gemm_ref(A, Wt, bias=bias, residual=res), f"budget base {name}")
        if name == "head-split":
            assert torch.equal(bits(base), bits(KR.head_split(both_forms(lib, lambda: variants["plain"](0)), B, T, H)))


# ---------------------------------------------------------------------------------------------- tile order
@pytest.mark.parametrize("M,N,K", KR.TILE_ORDER_SHAPES)
def test_tile_order_is_bit_identical(lib, M, N, K):
    """tile_rows in {1, 2, 3, 8} against 0 on band shapes with a partial head tile row, a partial tail tile row, a short last
    super-row and no full tile row at all (tests/test_kernel_refs_cpu.py::test_tile_order_shapes_take_every_branch derives that from
    tile_of()'s tile counts).  A tile order that skips a tile leaves the sentinel, one that repeats a tile skips another."""
    r, A, Wt, bias = data(M + N + 1, M, N, K)
    res = dev((r.standard_normal((M, N)) * 0.5).astype(np.float16))
    base = both_forms(lib, lambda: row_major(lib, A, Wt, bias=bias, residual=res, ldr=N))
    check_close(base, KR.gemm_ref(A, Wt, bias=bias, residual=res), "tile order base")
    for R in KR.TILE_ROWS:
        got = both_forms(lib, lambda: row_major(lib, A, Wt, bias=bias, residual=res, ldr=N, tile_rows=R))
        assert torch.equal(bits(got), bits(base)), R
        for mw in (8, 24):                                        # several tiles per workgroup: the order decides which
            got = both_forms(lib, lambda: row_major(lib, A, Wt, bias=bias, residual=res, ldr=N, tile_rows=R, max_wgs=mw))
            assert torch.equal(bits(got), bits(base)), (R, mw)


# ---------------------------------------------------------------------------------------------- alignment
@pytest.mark.parametrize("act", [0, 1])
def test_unaligned_ldc_and_ldr(lib, act):
    """ldc = N + 4 and a residual with ldr = N + 4 (8-byte aligned rows only): the persistent kernel takes its general epilogue.
    Equal to the aligned run bit for bit."""
    M, N, K = KR.ALIGN_SHAPE
    r, A, Wt, bias = data(99 + act, M, N, K)
    res = dev((r.standard_normal((M, N)) * 0.5).astype(np.float16))
    res4 = torch.full((M, N + 4), KR.SENTINEL, dtype=torch.float16, device="cuda")
    res4[:, :N] = res
    for with_res in (False, True):
        aligned = both_forms(lib, lambda: row_major(lib, A, Wt, bias=bias, act=act, pad=8,
                                                    **(dict(residual=res, ldr=N) if with_res else {})))
        odd = both_forms(lib, lambda: row_major(lib, A, Wt, bias=bias, act=act, pad=4,
                                                **(dict(residual=res4, ldr=N + 4) if with_res else {})))
        assert torch.equal(bits(odd), bits(aligned)), (act, with_res)
        check_close(aligned, KR.gemm_ref(A, Wt, bias=bias, act=act, residual=res if with_res else None), "alignment")


# ---------------------------------------------------------------------------------------------- argument checks
def test_argument_checks_launch_nothing(lib):
    A = torch.zeros((64, 192), dtype=torch.float16, device="cuda")
    out = torch.full((64, 256), KR.SENTINEL, dtype=torch.float16, device="cuda")
    bad = [(torch.zeros((192, 128), dtype=torch.float16, device="cuda"), dict(), "multiple of 128"),          # N % 128 != 0
           (torch.zeros((128, 96), dtype=torch.float16, device="cuda"), dict(), "multiple of 64"),             # K % 64 != 0
           (torch.zeros((128, 128), dtype=torch.float16, device="cuda"), dict(act=3), "act=3"),
           (torch.zeros((128, 128), dtype=torch.float16, device="cuda"), dict(out_mode=1, hs_t=0, hs_h=1), "head-split"),
           (torch.zeros((128, 128), dtype=torch.float16, device="cuda"), dict(q8_inv_scale=1.0), "head-split output only")]
    for Wt, kw, msg in bad:
        for tiles in FORMS:
            prev = lib.wm_set_gemm_small_tiles(tiles)
            try:
                gemm_ex(lib, A, Wt, lda=192, c=out, ldc=256, expect_rc=1, **kw)
            finally:
                lib.wm_set_gemm_small_tiles(prev)
            assert msg in lib.wm_last_error().decode(), (msg, lib.wm_last_error())
    assert bool((out == KR.SENTINEL).all()), "a refused call launched something"
