"""Kernel-level parity of the row kernels of csrc/rowops.hip through their test-only entries: wm_row_finish (the epilogue of every
Linear on the big-batch split-K decode path: four modes, the latency form with eight slabs in flight below 64 rows and the gentle
form from 64, the column-cut GELU grid), wm_embed, wm_mel_transpose_pad.  (wm_zero_pad_rows: tests/test_gpu_gemm_epilogue.py, on
the buffer conv1 has just written.)

Reference: tests/kernel_refs.py (float64, the kernels' rounding points), checked on the CPU by tests/test_kernel_refs_cpu.py.
The slabs of the reference comparisons lie on a grid (multiples of 2**-10, |.| <= 0.5) so that their fp32 sum is exact in any order:
fp16(sum + bias) and the in-place residual x = fp16(x + y16) are then compared EXACTLY, LayerNorm at the bound of
tests/test_gpu_kernels.py::test_layernorm and GELU at one fp16 ulp.  The two forms are compared bit for bit on ordinary random
slabs as well, where the order of the fp32 sum matters.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_refs as KR  # noqa: E402
import native  # noqa: E402
import weight as W  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return native.load_library()


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.cuda().contiguous()


def row_finish(lib, mode, M, N, part=None, ksplit=0, ldp=0, sstride=0, bias=None, gelu_kind=1, x=None, ldx=0, g=None, b=None,
               out=None, ldo=0, expect_rc=0):
    io = native.WmRowFinishIO()
    io.part, io.ksplit, io.m, io.n, io.ldp, io.part_sstride = (part.data_ptr() if part is not None else None), ksplit, M, N, ldp, sstride
    io.bias = bias.data_ptr() if bias is not None else None
    io.mode, io.gelu_kind = mode, gelu_kind
    io.x, io.ldx = (x.data_ptr() if x is not None else None), ldx
    io.ln_gamma, io.ln_beta = (g.data_ptr() if g is not None else None), (b.data_ptr() if b is not None else None)
    io.out, io.ldo = (out.data_ptr() if out is not None else None), ldo
    rc = lib.wm_row_finish(C.byref(io), stream())
    torch.cuda.synchronize()
    if expect_rc == 0:
        native.check(rc, "wm_row_finish")
    else:
        assert rc == expect_rc
    return rc


ROWS = 64          # slabs are generated for 64 rows; M = 64 runs the gentle form, M = 63 the latency ("eager") form


def run_modes(lib, part, ksplit, N, ldp, sstride, bias, x0, g, b, M, gelu_kinds=(1, 2)):
    """Modes 0-3 on the first M rows; every output buffer has ROWS + 1 rows and a sentinel column block that must survive."""
    res = {}
    ld = N + 8
    def fresh(src=None):
        t = torch.full((ROWS + 1, ld), KR.SENTINEL, dtype=torch.float16, device="cuda")
        if src is not None:
            t[:ROWS, :N] = src
        return t
    def guard(t, rows_written):
        assert bool((t[rows_written:] == KR.SENTINEL).all()), "written past the last row"
        assert bool((t[:, N:] == KR.SENTINEL).all()), "written outside the N columns"
        return t[:rows_written, :N].contiguous()
    x, out = fresh(x0), fresh()
    row_finish(lib, 0, M, N, part, ksplit, ldp, sstride, bias, x=x, ldx=ld, g=g, b=b, out=out, ldo=ld)
    assert torch.equal(x[M:ROWS, :N], x0[M:]), "a row beyond M was changed"
    x[M:ROWS, :N] = KR.SENTINEL
    res["m0_x"], res["m0_out"] = guard(x, M), guard(out, M)
    for kind in gelu_kinds:
        out = fresh()
        row_finish(lib, 1, M, N, part, ksplit, ldp, sstride, bias, gelu_kind=kind, out=out, ldo=ld)
        res[f"m1_out_{kind}"] = guard(out, M)
    x, out = fresh(x0), fresh()
    row_finish(lib, 2, M, N, x=x, ldx=ld, g=g, b=b, out=out, ldo=ld)
    assert torch.equal(x[:ROWS, :N], x0), "mode 2 changed x"
    res["m2_out"] = guard(out, M)
    x = fresh(x0)
    row_finish(lib, 3, M, N, part, ksplit, ldp, sstride, bias, x=x, ldx=ld)
    assert torch.equal(x[M:ROWS, :N], x0[M:])
    x[M:ROWS, :N] = KR.SENTINEL
    res["m3_x"] = guard(x, M)
    return res


@pytest.mark.parametrize("N", [128, 1280, 5120])
@pytest.mark.parametrize("ksplit", [1, 3, 4, 7, 8, 11, 16])
def test_row_finish_modes_and_forms(lib, N, ksplit):
    r = KR.philox(1000 * ksplit + N)
    ldp = N + 16                                                 # padded slabs, as the skinny GEMM writes them
    sstride = ROWS * ldp + 64                                    # a non-zero slab stride (not the default M * ldp)
    slabs = torch.full((ksplit * sstride,), float("nan"), dtype=torch.float32)
    grid = torch.from_numpy(KR.exact_grid(r, (ksplit, ROWS, N), 512, 2.0 ** -10))
    view = slabs.as_strided((ksplit, ROWS, N), (sstride, ldp, 1))
    view.copy_(grid)                                             # everything outside the [ksplit, ROWS, N] block stays NaN: never read
    part = dev(slabs)
    bias_h = torch.from_numpy(KR.exact_grid(r, (N,), 256, 2.0 ** -10)).half()
    x0_h = torch.from_numpy((r.standard_normal((ROWS, N)) * 1.5).astype(np.float16))
    g_h = torch.from_numpy(r.uniform(0.5, 1.5, N).astype(np.float16))
    b_h = torch.from_numpy(r.uniform(-0.5, 0.5, N).astype(np.float16))
    bias, x0, g, b = dev(bias_h), dev(x0_h), dev(g_h), dev(b_h)

    gentle = run_modes(lib, part, ksplit, N, ldp, sstride, bias, x0, g, b, 64)
    eager = run_modes(lib, part, ksplit, N, ldp, sstride, bias, x0, g, b, 63)     # mode 1 at N = 5120: the grid is cut along y
    for k_ in gentle:
        assert torch.equal(eager[k_].view(torch.int16), gentle[k_][:63].view(torch.int16)), f"{k_}: the two forms disagree"

    ref0 = KR.row_finish_ref(grid, bias_h, 0, x=x0_h, g=g_h, b=b_h)
    assert torch.equal(gentle["m0_x"].cpu().double(), ref0["x"]), "mode 0: x = fp16(x + fp16(sum + bias)) is not exact"
    tol = KR.fp16_tol(ref0["out"])
    assert float((gentle["m0_out"].cpu().double() - ref0["out"]).abs().max()) <= tol
    for kind in (1, 2):
        ref1 = KR.row_finish_ref(grid, bias_h, 1, gelu_kind=kind)["out"]
        assert float((gentle[f"m1_out_{kind}"].cpu().double() - ref1).abs().max()) <= KR.fp16_tol(ref1), kind
    ref2 = KR.row_finish_ref(None, None, 2, x=x0_h, g=g_h, b=b_h)["out"]
    assert float((gentle["m2_out"].cpu().double() - ref2).abs().max()) <= KR.fp16_tol(ref2)
    assert torch.equal(gentle["m3_x"].cpu().double(), KR.row_finish_ref(grid, bias_h, 3, x=x0_h)["x"]), "mode 3 is not exact"
    assert torch.equal(gentle["m3_x"], gentle["m0_x"])

    # a null bias, and the default slab stride (part_sstride = 0: M * ldp) on a dense copy
    nb = run_modes(lib, part, ksplit, N, ldp, sstride, None, x0, g, b, 64, gelu_kinds=(1,))
    assert torch.equal(nb["m3_x"].cpu().double(), KR.row_finish_ref(grid, None, 3, x=x0_h)["x"]), "null bias"
    ref1 = KR.row_finish_ref(grid, None, 1, gelu_kind=1)["out"]
    assert float((nb["m1_out_1"].cpu().double() - ref1).abs().max()) <= KR.fp16_tol(ref1)
    dense = dev(grid[:, :, :].contiguous())
    for M in (64, 63):
        # with part_sstride = 0 the slabs lie M * N apart: lay them out so for this M
        packed = torch.zeros((ksplit, M, N), dtype=torch.float32, device="cuda")
        packed.copy_(dense[:, :M])
        d = run_modes(lib, packed, ksplit, N, N, 0, bias, x0, g, b, M, gelu_kinds=(2,))
        assert torch.equal(d["m0_x"], gentle["m0_x"][:M]) and torch.equal(d["m0_out"], gentle["m0_out"][:M])
        assert torch.equal(d["m1_out_2"], gentle["m1_out_2"][:M])


@pytest.mark.parametrize("N", [1280, 5120])
@pytest.mark.parametrize("ksplit", [7, 8, 11, 16])
def test_row_finish_forms_agree_on_ordinary_sums(lib, N, ksplit):
    """Random fp32 slabs (sums that depend on their order): the latency form's eight slabs in flight are added in the order of the
    gentle form's loop, so a row has the same bits in both; and both are within one fp16 ulp of the float64 restatement."""
    r = KR.philox(77 * ksplit + N)
    raw = (r.standard_normal((ksplit, ROWS, N)) * np.exp(r.uniform(-6, 2, (ksplit, 1, 1)))).astype(np.float32)
    part_h = torch.from_numpy(raw)
    bias_h = torch.from_numpy((r.standard_normal(N) * 0.1).astype(np.float16))
    x0_h = torch.from_numpy((r.standard_normal((ROWS, N)) * 1.5).astype(np.float16))
    g_h = torch.from_numpy(r.uniform(0.5, 1.5, N).astype(np.float16))
    b_h = torch.from_numpy(r.uniform(-0.5, 0.5, N).astype(np.float16))
    part, bias, x0, g, b = dev(part_h), dev(bias_h), dev(x0_h), dev(g_h), dev(b_h)
    gentle = run_modes(lib, part, ksplit, N, N, ROWS * N, bias, x0, g, b, 64)
    eager = run_modes(lib, part, ksplit, N, N, ROWS * N, bias, x0, g, b, 63)
    for k_ in gentle:
        assert torch.equal(eager[k_].view(torch.int16), gentle[k_][:63].view(torch.int16)), f"{k_}: the two forms disagree"
    for kind in (1, 2):
        ref1 = KR.row_finish_ref(part_h, bias_h, 1, gelu_kind=kind)["out"]
        assert float((gentle[f"m1_out_{kind}"].cpu().double() - ref1).abs().max()) <= KR.fp16_tol(ref1)
    ref3 = KR.row_finish_ref(part_h, bias_h, 3, x=x0_h)["x"]
    assert float((gentle["m3_x"].cpu().double() - ref3).abs().max()) <= KR.fp16_tol(ref3)


def test_row_finish_argument_checks(lib):
    out = torch.full((4, 128), KR.SENTINEL, dtype=torch.float16, device="cuda")
    part = torch.zeros((1, 4, 128), dtype=torch.float32, device="cuda")
    row_finish(lib, 4, 4, 128, part, 1, 128, out=out, ldo=128, expect_rc=1)                 # no such mode
    row_finish(lib, 1, 4, 128, None, 1, 128, out=out, ldo=128, expect_rc=1)                 # mode 1 without slabs
    row_finish(lib, 1, 4, 128, part, 1, 128, gelu_kind=0, out=out, ldo=128, expect_rc=1)    # no such GELU
    row_finish(lib, 0, 4, 128, part, 1, 128, out=out, ldo=128, expect_rc=1)                 # mode 0 without x / LayerNorm weights
    row_finish(lib, 1, 4, 126, part, 1, 128, out=out, ldo=128, expect_rc=1)                 # N % 4 != 0
    assert bool((out == KR.SENTINEL).all())


# ---------------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("Cn,V", [(384, 1000), (1280, 51865)])
@pytest.mark.parametrize("with_t_dev", [False, True])
def test_embed(lib, Cn, V, with_t_dev):
    """x = fp16(E[token] + pos[m % L (+ T)]) exactly, the table restated from the tile-linear layout the kernel gathers from;
    tokens_ld > L; ids outside the table are clamped; the generation counter goes up by exactly one per call."""
    r = KR.philox(Cn + V + with_t_dev)
    B, L, ld, T = 5, 3, 11, (4 if with_t_dev else 0)
    E = r.standard_normal((V, Cn)).astype(np.float16)
    tiles = W.tile_linear(E)
    E_back = torch.from_numpy(W.untile_linear(tiles, V))
    pos_h = torch.from_numpy(r.standard_normal((L + T, Cn)).astype(np.float16))
    tok_h = torch.from_numpy(r.integers(0, V, size=(B, ld)).astype(np.int32))
    tok_h[0, T] = 0
    tok_h[1, T + 1] = V - 1
    tok_h[2, T + 2] = V + 9                                     # clamped to V - 1
    tok_h[3, T] = -2                                            # clamped to 0
    tiles_d, pos, tok = dev(tiles.view(np.uint8)), dev(pos_h), dev(tok_h)
    t_dev = torch.tensor([T], dtype=torch.int32, device="cuda") if with_t_dev else None
    gen = torch.tensor([41, 7], dtype=torch.int32, device="cuda")
    M, ldx = B * L, Cn + 8
    want = KR.embed_ref(E_back, pos_h, tok_h, L, T)
    for use_gen in (True, False):
        x = torch.full((M + 1, ldx), KR.SENTINEL, dtype=torch.float16, device="cuda")
        native.check(lib.wm_embed(tok.data_ptr(), ld, M, L, tiles_d.data_ptr(), Cn, pos.data_ptr(), x.data_ptr(), ldx, V,
                                  t_dev.data_ptr() if with_t_dev else None, gen.data_ptr() if use_gen else None, stream()), "wm_embed")
        torch.cuda.synchronize()
        assert bool((x[M:] == KR.SENTINEL).all()) and bool((x[:, Cn:] == KR.SENTINEL).all())
        assert torch.equal(x[:M, :Cn].cpu().double(), want)
    assert gen.tolist() == [42, 7], "the generation counter must go up exactly once per call that is given it"
    assert lib.wm_embed(tok.data_ptr(), 2, M, L, tiles_d.data_ptr(), Cn, pos.data_ptr(), x.data_ptr(), ldx, V, None, None, stream()) == 1      # tokens_ld < L


# ---------------------------------------------------------------------------------------------- mel transpose
@pytest.mark.parametrize("n_mels", [80, 128])
def test_mel_transpose_pad(lib, n_mels):
    B, T = 3, 3000
    r = KR.philox(n_mels)
    mel = r.standard_normal((B, n_mels, T)).astype(np.float16)
    src = dev(mel)
    n = B * (T + 2) * n_mels
    out = torch.full((n + 4096,), KR.SENTINEL, dtype=torch.float16, device="cuda")
    native.check(lib.wm_mel_transpose_pad(src.data_ptr(), B, n_mels, T, out.data_ptr(), stream()), "wm_mel_transpose_pad")
    torch.cuda.synchronize()
    assert bool((out[n:] == KR.SENTINEL).all()), "written past the padded buffer"
    assert np.array_equal(out[:n].cpu().numpy().reshape(B, T + 2, n_mels), KR.mel_transpose_pad_ref(mel))
