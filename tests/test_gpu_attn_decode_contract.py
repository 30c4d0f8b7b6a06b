"""Kernel-level contract of the decode attention kernels (csrc/attn_decode.hip) as the decoder engine calls them, through the
test-only entries wm_attn_self_ex / wm_attn_cross_ex: q / k / v as fp32 split-K slabs with a bias, slab / row / cache / output
strides, the device step counter, the calibration maximum, live-row lists (per-item and persistent launch), empty key splits, key
ranges shorter than one load instruction and the maximum key count.

Reference: tests/kernel_refs.py (float64, the kernels' rounding points; checked on the CPU by tests/test_kernel_refs_cpu.py, which
also shows that the case lists reach every kernel template and both launch forms).

Exactness tests: slabs and bias lie on a grid (multiples of 2**-10) so that every partial sum is exact in fp32 in any order.  The
rows fp16(sum + bias) then do not depend on how a kernel adds the slabs, and a launch must agree BIT FOR BIT with the existing
single-slab entries (wm_attn_decode_self / _self_rows / _cross / _cross_i8) given the pre-added fp32 row.
Ordinary-sum tests: random slabs, where the fp32 order matters: outputs at the bounds of tests/test_gpu_kernels.py
(test_attn_decode_self: 1.5e-3; test_attn_decode_cross: 1e-3 single pass, 2e-3 split), appended cache rows exact except where the
float64 sum lies within an fp32 ulp of an fp16 rounding boundary (kernel_refs.boundary_excused, from the reference alone).

Every buffer is larger than the kernels' extent.  Surplus a kernel might WRITE holds a sentinel (kernel_refs.SENTINEL, 77 in int8
caches), surplus it must never READ holds NaN (slab columns beyond 3C, gaps between slabs and utterances, cache slots beyond
T + L): a read poisons the output, and every test asserts that the surplus has the same bits after the launch.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_refs as KR  # noqa: E402
import native  # noqa: E402

T_SCALE = 0.031                       # the int8 self-attention cache's scale (tests/test_gpu_kernels.py::test_attn_decode_self)
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return native.load_library()


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.cuda().contiguous()


def ptr(x):
    """None, a raw address, or a tensor's."""
    return x if x is None or isinstance(x, int) else x.data_ptr()


def bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.int8}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.contiguous()), bits(b.contiguous()))


def finish(lib, rc, what, expect_rc):
    torch.cuda.synchronize()
    if expect_rc == 0:
        native.check(rc, what)
    else:
        assert rc == expect_rc, (what, rc)
        assert what[3:-3] in lib.wm_last_error().decode(), lib.wm_last_error()      # "attn_self" / "attn_cross": the wrapper's or the launcher's
    return rc


def self_ex(lib, *, part, B, L, T, H, present, present_bstride, present_cap, out, ksplit=1, ldp=None, sstride=0, bias=None, past=None,
            past_bstride=0, past_cap=0, int8_kv=0, kv_scale=T_SCALE, amax=None, t_dev=None, ldo=None, live=None, row_start=None,
            waves=1, expect_rc=0):
    io = native.WmAttnSelfIO()
    io.part, io.ksplit, io.ldp, io.part_sstride, io.bias = ptr(part), ksplit, (3 * H * 64 if ldp is None else ldp), sstride, ptr(bias)
    io.B, io.L, io.T, io.H = B, L, T, H
    io.past, io.past_bstride, io.past_cap = ptr(past), past_bstride, past_cap
    io.present, io.present_bstride, io.present_cap = ptr(present), present_bstride, present_cap
    io.int8_kv, io.kv_scale, io.amax, io.t_dev = int8_kv, kv_scale, ptr(amax), ptr(t_dev)
    io.out, io.ldo, io.live, io.row_start, io.waves = ptr(out), (H * 64 if ldo is None else ldo), ptr(live), ptr(row_start), waves
    return finish(lib, lib.wm_attn_self_ex(C.byref(io), stream()), "wm_attn_self_ex", expect_rc)


def cross_ex(lib, *, part, B, L, H, Tk, kv, kv_bstride, out, ksplit=1, ldp=None, sstride=0, bias=None, kv_q8_scale=0.0, ldo=None,
             nsplit=1, ws=None, live=None, skip=0, expect_rc=0):
    io = native.WmAttnCrossIO()
    io.part, io.ksplit, io.ldp, io.part_sstride, io.bias = ptr(part), ksplit, (H * 64 if ldp is None else ldp), sstride, ptr(bias)
    io.B, io.L, io.H, io.Tk = B, L, H, Tk
    io.kv, io.kv_bstride, io.kv_q8_scale = ptr(kv), kv_bstride, kv_q8_scale
    io.out, io.ldo, io.nsplit, io.ws, io.live, io.skip_zero_rows = ptr(out), (H * 64 if ldo is None else ldo), nsplit, ptr(ws), ptr(live), skip
    return finish(lib, lib.wm_attn_cross_ex(C.byref(io), stream()), "wm_attn_cross_ex", expect_rc)


# ---------------------------------------------------------------------------------------------- buffers
def lay_slabs(vals, ldp, gap):
    """[ksplit, M, N] fp32 -> a flat device buffer with rows ldp apart and slabs M * ldp + gap apart; everything else is NaN (never read).
    Returns (buffer, slab stride)."""
    ks, M, N = vals.shape
    sstride = M * ldp + gap
    buf = torch.full((ks * sstride + 64,), NAN, dtype=torch.float32)
    buf.as_strided((ks, M, N), (sstride, ldp, 1)).copy_(vals)
    return dev(buf), sstride


def grid_slabs(r, ks, M, N):
    """Slabs and bias on the exact grid: |slab| <= 1800 / sqrt(ks) steps of 2**-10 (rows of about unit variance), |bias| <= 0.25.  The
    float64 row sum + bias is exact, and so is every fp32 partial sum (integers below 2**24 in units of 2**-10)."""
    part = torch.from_numpy(KR.exact_grid(r, (ks, M, N), int(1800 / math.sqrt(ks)), 2.0 ** -10))
    bias = torch.from_numpy(KR.exact_grid(r, (N,), 256, 2.0 ** -10)).half()
    return part, bias


def pre_added(part, bias):
    """The single fp32 slab the existing entries get: sum + bias (exact on the grid)."""
    y = part.double().sum(0)
    if bias is not None:
        y = y + bias.double()[None, :]
    assert torch.equal(y.float().double(), y), "the grid sum must be exact in fp32"
    return y.float()


def cache_view(buf, B, H, cap, bstride):
    return buf.as_strided((B, 2, H, cap, 64), (bstride, H * cap * 64, cap * 64, 64, 1))


def make_cache(B, H, cap, int8_kv, gap, filled=None):
    """A flat cache of B utterances [2][H][cap][64], `gap` elements apart beyond their extent: int8 77 / fp16 NaN everywhere except the
    first slots, which take `filled` [B, 2, H, T, 64].  Returns (device buffer, utterance stride)."""
    bstride = 2 * H * cap * 64 + gap
    if int8_kv:
        buf = torch.full((B * bstride + 128,), 77, dtype=torch.int8)
    else:
        buf = torch.full((B * bstride + 128,), NAN, dtype=torch.float16)
    if filled is not None and filled.shape[3] > 0:
        cache_view(buf, B, H, cap, bstride)[:, :, :, :filled.shape[3]] = filled
    return dev(buf), bstride


def out_buffer(M, ldo):
    return torch.full((M + 1, ldo), KR.SENTINEL, dtype=torch.float16, device="cuda")


def out_rows(out, M, Cn):
    assert bool((out[M:] == KR.SENTINEL).all()), "written past the last row"
    assert bool((out[:, Cn:] == KR.SENTINEL).all()), "written outside the C columns"
    return out[:M, :Cn].contiguous()


def past_values(r, B, H, T, int8_kv):
    """Cached slots: what is stored (fp16 values or int8 codes) and what it is worth as keys / values (float64)."""
    x = torch.from_numpy((r.standard_normal((B, 2, H, T, 64)) * 1.2).astype(np.float16))
    if int8_kv:
        codes = KR.self_cache_codes(x, T_SCALE)
        return codes, KR.self_cache_values(codes, T_SCALE)
    return x, x.double()


def new_slots(rows, B, L, H, int8_kv):
    """What the call appends: the k | v column blocks of the fp16 rows as [B, 2, H, L, 64] (stored form)."""
    Cn = H * 64
    kv = torch.stack([KR.split_heads(rows[:, Cn:2 * Cn], B, L, H), KR.split_heads(rows[:, 2 * Cn:], B, L, H)], dim=1)
    return KR.self_cache_codes(kv, T_SCALE) if int8_kv else kv.half()


class SelfRun:
    """One wm_attn_self_ex launch in a padded layout, with the surplus checks every test makes."""

    def __init__(self, lib, part, bias, B, L, T, H, stored_past, int8_kv, waves, *, strided=True, ldp_pad=4, ldo_pad=8, inplace=True,
                 row_start=None, live=None, t_dev=None, host_T=None, amax=None, cache_gap=64):
        ks, M, N = part.shape
        Cn = H * 64
        assert N == 3 * Cn and M == B * L
        ldp, ldo = 3 * Cn + ldp_pad, Cn + ldo_pad
        slabs, sstride = lay_slabs(part, ldp, 8 if strided else 0)
        cap = T + L + 5
        self.out = out_buffer(M, ldo)
        if inplace:
            self.present, bstride = make_cache(B, H, cap, int8_kv, cache_gap, stored_past)
            self.past, past_kw = None, dict(past=self.present, past_bstride=bstride, past_cap=cap)
        else:                                                    # another buffer, another capacity, another stride
            self.present, bstride = make_cache(B, H, cap, int8_kv, cache_gap)
            past_cap = T + 3
            self.past, past_bstride = make_cache(B, H, past_cap, int8_kv, 2 * cache_gap, stored_past)
            past_kw = dict(past=self.past if T > 0 else None, past_bstride=past_bstride, past_cap=past_cap)
        before, past_before = self.present.clone(), (self.past.clone() if self.past is not None else None)
        self_ex(lib, part=slabs, ksplit=ks, ldp=ldp, sstride=sstride if strided else 0, bias=dev(bias) if bias is not None else None,
                B=B, L=L, T=T if host_T is None else host_T, H=H, present=self.present, present_bstride=bstride, present_cap=cap,
                int8_kv=int8_kv, amax=amax, t_dev=t_dev, out=self.out, ldo=ldo, live=live, row_start=row_start, waves=waves, **past_kw)
        self.rows = out_rows(self.out, M, Cn)
        view = cache_view(self.present, B, H, cap, bstride)
        self.slots = view[:, :, :, :T + L].contiguous()          # cached + appended, as stored
        # the surplus: everything outside the slots the launch may write (appended; cached too when they were copied forward)
        masked = self.present.clone()
        cache_view(masked, B, H, cap, bstride)[:, :, :, (T if inplace else 0):T + L] = cache_view(before, B, H, cap, bstride)[:, :, :, (T if inplace else 0):T + L]
        assert same_bits(masked, before), "the cache was written outside the appended (and copied) slots"
        if inplace:
            assert same_bits(view[:, :, :, :T], cache_view(before, B, H, cap, bstride)[:, :, :, :T]), "cached slots changed in place"
        if past_before is not None:
            assert same_bits(self.past, past_before), "the past buffer was written"


def baseline_self(lib, rows32, B, L, T, H, stored_past, int8_kv, waves, inplace, row_start=None):
    """The existing entry on the pre-added rows, dense layout: (out rows, slots [:T + L])."""
    Cn = H * 64
    cap = T + L + 5
    present, _ = make_cache(B, H, cap, int8_kv, 0, stored_past if (inplace or row_start is not None) else None)
    present = present[:B * 2 * H * cap * 64].view(B, 2, H, cap, 64)
    out = torch.zeros((B * L, Cn), dtype=torch.float16, device="cuda")
    qd = dev(rows32)
    prev = lib.wm_set_self_attn_waves(waves)
    try:
        if row_start is not None:
            native.check(lib.wm_attn_decode_self_rows(qd.data_ptr(), B, L, T, H, present.data_ptr(), cap, int8_kv, T_SCALE, out.data_ptr(),
                                                      row_start.data_ptr(), None, stream()), "wm_attn_decode_self_rows")
        else:
            past = present if inplace else (dev(stored_past) if T > 0 else None)
            native.check(lib.wm_attn_decode_self(qd.data_ptr(), B, L, T, H, ptr(past), cap if inplace else T, present.data_ptr(), cap,
                                                 int8_kv, T_SCALE, out.data_ptr(), stream()), "wm_attn_decode_self")
        torch.cuda.synchronize()
    finally:
        lib.wm_set_self_attn_waves(prev)
    return out, present[:, :, :, :T + L].contiguous()


# ---------------------------------------------------------------------------------------------- self-attention: exactness
@pytest.mark.parametrize("ks,int8_kv,waves,rs,L,T,with_bias,strided,ldp_pad,ldo_pad,inplace", KR.SELF_EXACT_CASES)
def test_self_slabs_bias_and_strides_are_bit_identical_to_the_single_slab_entry(lib, ks, int8_kv, waves, rs, L, T, with_bias, strided,
                                                                                ldp_pad, ldo_pad, inplace):
    B, H = 2, 2
    r = KR.philox(((ks * 2 + int8_kv) * 8 + waves + rs) * 1000 + 10 * T + L)
    part, bias = grid_slabs(r, ks, B * L, 3 * H * 64)
    bias = bias if with_bias else None
    stored, _ = past_values(r, B, H, T, int8_kv)
    row_start = dev(np.array(KR.SELF_ROW_START, dtype=np.int32)) if rs else None
    run = SelfRun(lib, part, bias, B, L, T, H, stored, int8_kv, waves, strided=strided, ldp_pad=ldp_pad, ldo_pad=ldo_pad, inplace=inplace,
                  row_start=row_start)
    want_out, want_slots = baseline_self(lib, pre_added(part, bias), B, L, T, H, stored, int8_kv, waves, inplace, row_start)
    assert same_bits(run.rows, want_out), "output rows differ from the single-slab entry"
    assert same_bits(run.slots, want_slots), "cache slots differ from the single-slab entry"
    assert not bool(torch.isnan(run.rows.float()).any()), "a never-read region reached the output"
    # the appended rows are fp16(sum + bias) (and its int8 codes) exactly; the cached ones are the past, copied forward or left
    rows = KR.qkv_rows_ref(part, bias)
    assert torch.equal(run.slots[:, :, :, T:].cpu(), new_slots(rows, B, L, H, int8_kv)), "appended rows are not fp16(sum + bias)"
    assert torch.equal(run.slots[:, :, :, :T].cpu(), stored)


@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("int8_kv", [0, 1])
def test_self_device_step_counter_replaces_the_host_T(lib, int8_kv, waves):
    """T read from the device (graph replay): with a host T of 0 -- which still passes the launcher's capacity check -- and *t_dev = T
    the launch has the bits of the host-T launch: output rows, appended slots, untouched surplus."""
    B, L, T, H, ks = 2, 3, 69, 2, 4
    r = KR.philox(300 + int8_kv)
    part, bias = grid_slabs(r, ks, B * L, 3 * H * 64)
    stored, _ = past_values(r, B, H, T, int8_kv)
    host = SelfRun(lib, part, bias, B, L, T, H, stored, int8_kv, waves)
    t_dev = torch.tensor([T, 0, 0, 0], dtype=torch.int32, device="cuda")
    devT = SelfRun(lib, part, bias, B, L, T, H, stored, int8_kv, waves, t_dev=t_dev, host_T=0)
    assert same_bits(devT.rows, host.rows) and same_bits(devT.slots, host.slots)
    assert t_dev.tolist() == [T, 0, 0, 0]
    want_out, want_slots = baseline_self(lib, pre_added(part, bias), B, L, T, H, stored, int8_kv, waves, True)
    assert same_bits(host.rows, want_out) and same_bits(host.slots, want_slots)


@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("int8_kv", [0, 1])
def test_self_calibration_maximum_and_live_rows(lib, int8_kv, waves):
    """amax: the running maximum of |q|, |k|, |v| of the fp16 rows, exactly (an fp32 bit pattern), from 0; a larger value survives;
    with a live list only the live rows count -- and only they are written: out rows and caches of the others keep their bits."""
    B, L, T, H, ks = 3, 2, 5, 2, 5
    Cn = H * 64
    r = KR.philox(400 + int8_kv)
    part, bias = grid_slabs(r, ks, B * L, 3 * Cn)
    part[2, 1 * L + 1, Cn + 17] = 30.0                            # the largest value of all sits in a row of utterance 1
    stored, vals = past_values(r, B, H, T, int8_kv)
    rows = KR.qkv_rows_ref(part, bias)
    assert float(rows[L:2 * L].abs().max()) > float(torch.cat([rows[:L], rows[2 * L:]]).abs().max()) + 1.0

    def as_bits(x):
        return int(np.float32(x).view(np.int32))
    amax = torch.zeros(4, dtype=torch.float32, device="cuda")
    full = SelfRun(lib, part, bias, B, L, T, H, stored, int8_kv, waves, amax=amax)
    assert bits(amax).tolist() == [as_bits(KR.amax_ref(rows)), 0, 0, 0]
    want = KR.attn_self_ref(rows, vals, B, L, T, H)               # (the bound rests on O(1) values: utterances 0 and 2)
    assert float((full.rows.cpu().double() - want)[[0, 1, 4, 5]].abs().max()) <= 1.5e-3
    amax[0] = 1000.0
    SelfRun(lib, part, bias, B, L, T, H, stored, int8_kv, waves, amax=amax)
    assert bits(amax).tolist() == [as_bits(1000.0), 0, 0, 0], "a larger running maximum must survive"

    live = torch.tensor([2, 2, 0, 0], dtype=torch.int32, device="cuda")          # two rows live: 2 and 0
    amax.zero_()
    run = SelfRun(lib, part, bias, B, L, T, H, stored, int8_kv, waves, amax=amax, live=live)
    live_rows = torch.cat([rows[:L], rows[2 * L:]])
    assert bits(amax).tolist() == [as_bits(KR.amax_ref(live_rows)), 0, 0, 0], "only the live rows count"
    for b in (0, 2):
        assert same_bits(run.rows[b * L:(b + 1) * L], full.rows[b * L:(b + 1) * L]) and same_bits(run.slots[b], full.slots[b])
    assert bool((run.rows[L:2 * L] == KR.SENTINEL).all()), "a finished row's output was written"
    dead = run.slots[1, :, :, T:]
    assert bool((dead == 77).all()) if int8_kv else bool(torch.isnan(dead.float()).all()), "a finished row's cache was appended to"
    assert live.tolist() == [2, 2, 0, 0]


# ---------------------------------------------------------------------------------------------- self-attention: ordinary sums
@pytest.mark.parametrize("ks,int8_kv,waves,L,T", KR.SELF_SUM_CASES)
def test_self_ordinary_sums(lib, ks, int8_kv, waves, L, T):
    """Random slabs (the fp32 order of the additions matters; nothing is pinned bit for bit): the output against
    attn_self_ref(qkv_rows_ref(.)) at 1.5e-3, the bound of test_attn_decode_self; the appended rows equal to qkv_rows_ref except where
    kernel_refs.boundary_excused allows the order to decide (under 1 % of the elements, from the reference alone: checked on the CPU
    for this seed by tests/test_kernel_refs_cpu.py).  Measured on an MI355X: see the figures this test prints."""
    B, H = 2, 2
    r = KR.philox(KR.SUM_SEED + ks)
    part, bias = KR.ordinary_slabs(r, ks, B * L, 3 * H * 64)
    stored, vals = past_values(r, B, H, T, int8_kv)
    run = SelfRun(lib, part, bias, B, L, T, H, stored, int8_kv, waves)
    rows = KR.qkv_rows_ref(part, bias)
    err = float((run.rows.cpu().double() - KR.attn_self_ref(rows, vals, B, L, T, H)).abs().max())
    excused = KR.boundary_excused(part, bias)
    Cn = H * 64
    ex_kv = torch.stack([KR.split_heads(excused[:, Cn:2 * Cn], B, L, H), KR.split_heads(excused[:, 2 * Cn:], B, L, H)], dim=1)
    differ = run.slots[:, :, :, T:].cpu() != new_slots(rows, B, L, H, int8_kv)
    share = float(excused.double().mean())
    print(f"self ordinary sums ks={ks} int8={int8_kv} waves={waves} L={L} T={T}: max |out - ref| = {err:.3e} (bound 1.5e-3), "
          f"excused share = {100 * share:.3f} % (cap 1 %), appended elements that differ = {int(differ.sum())}")
    assert share < 0.01
    assert not bool((differ & ~ex_kv).any()), "an appended element differs where the order of the sum cannot explain it"
    assert torch.equal(run.slots[:, :, :, :T].cpu(), stored)
    assert err <= 1.5e-3, err


# ---------------------------------------------------------------------------------------------- cross-attention
def make_kv(r, B, H, Tk, int8, gap=64):
    """K/V [B][2][H][Tk][64], utterances `gap` elements further apart than their extent, the gap NaN (fp16) / 77 (int8 codes).
    Returns (device buffer, stride, scale, K values, V values [B, H, Tk, 64] float64, dense stored tensor)."""
    x = torch.from_numpy(r.standard_normal((B, 2, H, Tk, 64)).astype(np.float16))
    bstride = 2 * H * Tk * 64 + gap
    if int8:
        t = float(np.float32(x.abs().max()) / np.float32(127.0))
        stored = KR.quant_codes(x, np.float32(1.0) / np.float32(t))
        vals = KR.cross_i8_values(stored, t)
        buf = torch.full((B * bstride + 128,), 77, dtype=torch.int8)
    else:
        t, stored, vals = 0.0, x, x.double()
        buf = torch.full((B * bstride + 128,), NAN, dtype=torch.float16)
    buf.as_strided((B, 2, H, Tk, 64), (bstride, H * Tk * 64, Tk * 64, 64, 1)).copy_(stored)
    return dev(buf), bstride, t, vals[:, 0], vals[:, 1], stored


WS_PAD = 256


def make_ws(B, H, nsplit, L):
    return torch.full((B * H * nsplit * L * 66 + WS_PAD,), KR.SENTINEL, dtype=torch.float32, device="cuda")


class CrossRun:
    """One wm_attn_cross_ex launch in a padded layout: slabs ldp = C + 4 and a slab gap, ldo = C + 8, a workspace with a sentinel tail."""

    def __init__(self, lib, part, bias, B, L, H, Tk, kvbuf, kv_bstride, scale, nsplit, skip=0, live=None, padded=True):
        ks, M, N = part.shape
        Cn = H * 64
        assert N == Cn and M == B * L
        ldp, ldo = (Cn + 4, Cn + 8) if padded else (Cn, Cn)
        slabs, sstride = lay_slabs(part, ldp, 8 if padded else 0)
        self.out = out_buffer(M, ldo)
        self.ws = make_ws(B, H, nsplit, L)
        cross_ex(lib, part=slabs, ksplit=ks, ldp=ldp, sstride=sstride if padded else 0, bias=dev(bias) if bias is not None else None,
                 B=B, L=L, H=H, Tk=Tk, kv=kvbuf, kv_bstride=kv_bstride, kv_q8_scale=scale, out=self.out, ldo=ldo, nsplit=nsplit,
                 ws=self.ws if nsplit > 1 else None, live=live, skip=skip)
        self.rows = out_rows(self.out, M, Cn)
        n = B * H * nsplit * L * 66
        assert bool((self.ws[n if nsplit > 1 else 0:] == KR.SENTINEL).all()), "the workspace was written outside its blocks"
        self.ws_blocks = self.ws[:n].view(B, H * nsplit * L * 66)


def baseline_cross(lib, rows32, B, L, H, Tk, stored, scale, nsplit, skip):
    out = torch.zeros((B * L, H * 64), dtype=torch.float16, device="cuda")
    ws = torch.zeros(B * H * nsplit * L * 66, dtype=torch.float32, device="cuda")
    qd, kvd = dev(rows32), dev(stored)
    if scale > 0:
        native.check(lib.wm_attn_decode_cross_i8(qd.data_ptr(), B, L, H, Tk, kvd.data_ptr(), scale, out.data_ptr(), nsplit, ws.data_ptr(),
                                                 stream()), "wm_attn_decode_cross_i8")
        torch.cuda.synchronize()
        return out
    prev = lib.wm_set_cross_v_skip(skip)
    try:
        native.check(lib.wm_attn_decode_cross(qd.data_ptr(), B, L, H, Tk, kvd.data_ptr(), out.data_ptr(), nsplit, ws.data_ptr(), stream()),
                     "wm_attn_decode_cross")
        torch.cuda.synchronize()
    finally:
        lib.wm_set_cross_v_skip(prev)
    return out


def cross_bound(nsplit):
    return 1e-3 if nsplit == 1 else 2e-3                          # tests/test_gpu_kernels.py::test_attn_decode_cross


@pytest.mark.parametrize("ks,L,variant,nsplit,Tk,H,with_bias", KR.CROSS_EXACT_CASES)
def test_cross_slabs_bias_and_strides_are_bit_identical_to_the_single_slab_entry(lib, ks, L, variant, nsplit, Tk, H, with_bias):
    B = 2
    r = KR.philox((ks * 8 + L) * 4 + KR.CROSS_VARIANTS.index(variant))
    part, bias = grid_slabs(r, ks, B * L, H * 64)
    bias = bias if with_bias else None
    kvbuf, bstride, t, Kv, Vv, stored = make_kv(r, B, H, Tk, variant == "int8")
    skip = int(variant == "fp16+SKIP")
    run = CrossRun(lib, part, bias, B, L, H, Tk, kvbuf, bstride, t, nsplit, skip=skip)
    want = baseline_cross(lib, pre_added(part, bias), B, L, H, Tk, stored, t, nsplit, skip)
    assert same_bits(run.rows, want), "output rows differ from the single-slab entry"
    assert not bool(torch.isnan(run.rows.float()).any()), "a never-read region reached the output"


@pytest.mark.parametrize("L,nsplit,variant", KR.CROSS_LIVE_CASES)
def test_cross_live_rows(lib, L, nsplit, variant):
    """B = 4 with the live list [2; 3, 1]: the live rows have the bits of the same rows launched alone (B = 1); the out rows and the
    workspace blocks of the other rows -- the workspace is indexed by the ORIGINAL row -- keep their sentinel."""
    B, H, Tk, ks = 4, 2, 100, 3
    Cn = H * 64
    r = KR.philox(500 + L + nsplit)
    part, bias = grid_slabs(r, ks, B * L, Cn)
    kvbuf, bstride, t, Kv, Vv, stored = make_kv(r, B, H, Tk, variant == "int8")
    live = torch.tensor([2, 3, 1, 0, 0], dtype=torch.int32, device="cuda")
    run = CrossRun(lib, part, bias, B, L, H, Tk, kvbuf, bstride, t, nsplit, live=live)
    ref = KR.merge_heads(KR.attn_decode_ref(KR.split_heads(KR.qkv_rows_ref(part, bias), B, L, H), Kv, Vv, k_exact=variant == "int8"))
    for b in (3, 1):
        err = float((run.rows[b * L:(b + 1) * L].cpu().double() - ref[b * L:(b + 1) * L]).abs().max())
        assert err <= cross_bound(nsplit), (b, err)
        p1 = part[:, b * L:(b + 1) * L].contiguous()
        kv1, bs1, _, _, _, _ = make_kv(KR.philox(0), 1, H, Tk, variant == "int8")
        kv1[:2 * H * Tk * 64] = dev(stored[b].reshape(-1))
        alone = CrossRun(lib, p1, bias, 1, L, H, Tk, kv1, bs1, t, nsplit)
        assert same_bits(run.rows[b * L:(b + 1) * L], alone.rows), f"live row {b} differs from the row launched alone"
        if nsplit > 1:
            assert same_bits(run.ws_blocks[b], alone.ws_blocks[0])
    for b in (0, 2):
        assert bool((run.rows[b * L:(b + 1) * L] == KR.SENTINEL).all()), f"the output of finished row {b} was written"
        assert bool((run.ws_blocks[b] == KR.SENTINEL).all()), f"the workspace block of finished row {b} was written"
    assert live.tolist() == [2, 3, 1, 0, 0]


def test_cross_persistent_launch_with_a_live_list(lib):
    """H * B * nsplit >= 4 * CUs: two workgroups per CU walk the items.  With every row live, and with ~60 % of the rows on a
    scrambled list, a live row has the same bits -- also as in a per-item launch of two of them; finished rows keep their sentinels."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    H, nsplit, Tk, L, ks = 2, 8, 64, 1, 4
    B = KR.persistent_batch(n_cu, H, nsplit)
    d = KR.cross_dispatch(L, False, False, nsplit, H, B, n_cu)
    assert d["launch"] == "persistent" and d["grid"] < d["items"], d
    assert KR.cross_dispatch(L, False, False, nsplit, H, 2, n_cu)["launch"] == "per-item"
    Cn = H * 64
    r = KR.philox(600)
    part, bias = grid_slabs(r, ks, B * L, Cn)
    kvbuf, bstride, t, Kv, Vv, stored = make_kv(r, B, H, Tk, False)
    full = CrossRun(lib, part, bias, B, L, H, Tk, kvbuf, bstride, t, nsplit)
    ref = KR.merge_heads(KR.attn_decode_ref(KR.split_heads(KR.qkv_rows_ref(part, bias), B, L, H), Kv, Vv))
    assert float((full.rows.cpu().double() - ref).abs().max()) <= cross_bound(nsplit)
    n_live = (6 * B) // 10
    chosen = np.sort(r.permutation(B)[:n_live])                  # ascending indices ...
    order = chosen[r.permutation(n_live)]                        # ... on the list in a scrambled order
    lv = np.zeros(1 + B, dtype=np.int32)
    lv[0], lv[1:1 + n_live] = n_live, order
    live = dev(lv)
    run = CrossRun(lib, part, bias, B, L, H, Tk, kvbuf, bstride, t, nsplit, live=live)
    alive = torch.zeros(B, dtype=torch.bool)
    alive[torch.from_numpy(chosen.astype(np.int64))] = True
    rows, frows = run.rows.cpu().view(B, L * Cn), full.rows.cpu().view(B, L * Cn)
    assert same_bits(rows[alive], frows[alive]), "a live row differs from the all-live launch"
    assert same_bits(run.ws_blocks.cpu()[alive], full.ws_blocks.cpu()[alive])
    assert bool((rows[~alive] == KR.SENTINEL).all()), "a finished row's output was written"
    assert bool((run.ws_blocks.cpu()[~alive] == KR.SENTINEL).all()), "a finished row's workspace block was written"
    assert np.array_equal(live.cpu().numpy(), lv)
    two = [int(order[0]), int(order[-1])]
    p2 = torch.cat([part[:, b * L:(b + 1) * L] for b in two], dim=1).contiguous()
    kv2, bs2, _, _, _, _ = make_kv(KR.philox(0), 2, H, Tk, False)
    for i, b in enumerate(two):
        kv2[i * bs2:i * bs2 + 2 * H * Tk * 64] = dev(stored[b].reshape(-1))
    pair = CrossRun(lib, p2, bias, 2, L, H, Tk, kv2, bs2, t, nsplit)
    assert same_bits(pair.rows.cpu(), torch.stack([rows[b] for b in two]).view(2 * L, Cn)), "persistent and per-item launches differ"


@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("Tk,nsplit,H", KR.CROSS_EDGE_CASES)
def test_cross_key_range_edges(lib, Tk, nsplit, H, L):
    """Fewer keys than a load instruction's 8 rows, empty key splits (Tk = 20 in 8 splits: five write the neutral element and the merge
    must ignore them; Tk = 100 in 16: three), the maximum key count in 1 and 16 splits: fp16 and int8 K/V against attn_decode_ref at the
    bounds of test_attn_decode_cross; the V-skip form (single pass) has the bits of the plain one."""
    B = 1 if Tk > 333 else 2
    r = KR.philox(700 + Tk + nsplit + L)
    part = torch.from_numpy(r.standard_normal((1, B * L, H * 64)).astype(np.float16).astype(np.float32))
    q = KR.split_heads(KR.qkv_rows_ref(part), B, L, H)
    for int8 in (False, True):
        kvbuf, bstride, t, Kv, Vv, _ = make_kv(r, B, H, Tk, int8)
        run = CrossRun(lib, part, None, B, L, H, Tk, kvbuf, bstride, t, nsplit)
        ref = KR.merge_heads(KR.attn_decode_ref(q, Kv, Vv, k_exact=int8))
        err = float((run.rows.cpu().double() - ref).abs().max())
        assert err <= cross_bound(nsplit), (int8, err)
        if not int8 and nsplit == 1:
            skipped = CrossRun(lib, part, None, B, L, H, Tk, kvbuf, bstride, t, nsplit, skip=1)
            assert same_bits(skipped.rows, run.rows), "the V-skip form differs from the plain one"


@pytest.mark.parametrize("ks,L,variant,nsplit,Tk", KR.CROSS_SUM_CASES)
def test_cross_ordinary_sums(lib, ks, L, variant, nsplit, Tk):
    """Random slabs: the output against attn_decode_ref(qkv_rows_ref(.)) at the bounds of test_attn_decode_cross (1e-3 single pass,
    2e-3 split).  Measured on an MI355X: see the figures this test prints."""
    B, H = 2, 2
    r = KR.philox(KR.SUM_SEED + ks + L)
    part, bias = KR.ordinary_slabs(r, ks, B * L, H * 64)
    kvbuf, bstride, t, Kv, Vv, _ = make_kv(r, B, H, Tk, variant == "int8")
    run = CrossRun(lib, part, bias, B, L, H, Tk, kvbuf, bstride, t, nsplit, skip=int(variant == "fp16+SKIP"))
    ref = KR.merge_heads(KR.attn_decode_ref(KR.split_heads(KR.qkv_rows_ref(part, bias), B, L, H), Kv, Vv, k_exact=variant == "int8"))
    err = float((run.rows.cpu().double() - ref).abs().max())
    print(f"cross ordinary sums ks={ks} L={L} {variant} nsplit={nsplit} Tk={Tk}: max |out - ref| = {err:.3e} (bound {cross_bound(nsplit):.0e}), "
          f"q elements the sum order may decide = {100 * float(KR.boundary_excused(part, bias).double().mean()):.3f} %")
    assert err <= cross_bound(nsplit), err


# ---------------------------------------------------------------------------------------------- argument checks
def test_argument_checks_launch_nothing(lib):
    """Every violation the wrappers check returns non-zero, sets wm_last_error and launches nothing: sentinel-filled outputs, caches
    and workspaces keep their bits.  All pointers are valid and the buffers generous: only sizes, strides and alignments are wrong."""
    B, L, T, H, ks = 2, 2, 4, 2, 2
    Cn, M, cap = H * 64, 4, 16
    ext = 2 * H * cap * 64
    part = torch.zeros(8 * M * (3 * Cn + 64), dtype=torch.float32, device="cuda")
    bias = torch.zeros(4 * 3 * Cn, dtype=torch.float16, device="cuda")
    present = torch.full((4 * B * ext,), KR.SENTINEL, dtype=torch.float16, device="cuda")
    past = torch.full((4 * B * ext,), 3.0, dtype=torch.float16, device="cuda")
    out = torch.full((4 * M, 2 * Cn), KR.SENTINEL, dtype=torch.float16, device="cuda")
    ok = dict(part=part, ksplit=ks, ldp=3 * Cn + 4, sstride=M * (3 * Cn + 4) + 8, bias=bias, B=B, L=L, T=T, H=H, past=past,
              past_bstride=ext, past_cap=cap - 1, present=present, present_bstride=ext + 64, present_cap=cap, out=out, ldo=Cn + 8)
    bad_self = [dict(part=None), dict(present=None), dict(out=None), dict(ksplit=0), dict(B=0), dict(H=0), dict(T=-1),
                dict(ldp=3 * Cn + 2), dict(ldp=3 * Cn - 4), dict(sstride=M * (3 * Cn + 4) + 2), dict(sstride=M * (3 * Cn + 4) - 4),
                dict(part=part.data_ptr() + 4), dict(bias=bias.data_ptr() + 2), dict(past=past.data_ptr() + 8),
                dict(present=present.data_ptr() + 8), dict(ldo=Cn - 8), dict(present_bstride=ext - 16), dict(present_bstride=ext + 64 + 8),
                dict(past_bstride=2 * Cn * (cap - 1) - 16), dict(past_bstride=ext + 8), dict(past_cap=T - 1),
                dict(past=present, past_bstride=ext + 64, past_cap=cap - 1), dict(past=present, past_bstride=ext + 128, past_cap=cap),
                dict(L=5), dict(present_cap=T + L - 1), dict(waves=2), dict(int8_kv=1, kv_scale=0.0)]
    for kw in bad_self:
        self_ex(lib, **{**ok, **kw}, expect_rc=1)
    assert bool((out == KR.SENTINEL).all()) and bool((present == KR.SENTINEL).all()) and bool((past == 3.0).all()), \
        "a refused call launched something"
    self_ex(lib, **ok)                                            # ... and the arguments they were derived from are accepted
    assert not bool((out.view(-1)[:M * (Cn + 8)].view(M, Cn + 8)[:, :Cn] == KR.SENTINEL).any())
    out.fill_(KR.SENTINEL)
    present.fill_(KR.SENTINEL)

    Tk, ns = 40, 2
    kext = 2 * H * Tk * 64
    kv = torch.zeros(B * 2 * H * (KR.CROSS_MAX_KEYS + 8) * 64 + 4 * kext, dtype=torch.float16, device="cuda")
    ws = torch.full((4 * B * H * ns * L * 66,), KR.SENTINEL, dtype=torch.float32, device="cuda")
    okc = dict(part=part, ksplit=ks, ldp=Cn + 4, sstride=M * (Cn + 4) + 8, bias=bias, B=B, L=L, H=H, Tk=Tk, kv=kv, kv_bstride=kext + 64,
               out=out, ldo=Cn + 8, nsplit=ns, ws=ws)
    bad_cross = [dict(part=None), dict(kv=None), dict(out=None), dict(ws=None), dict(ksplit=0), dict(B=0), dict(H=0),
                 dict(ldp=Cn + 2), dict(ldp=Cn - 4), dict(sstride=M * (Cn + 4) + 2), dict(sstride=M * (Cn + 4) - 4),
                 dict(part=part.data_ptr() + 4), dict(bias=bias.data_ptr() + 2), dict(kv=kv.data_ptr() + 8), dict(ldo=Cn - 8),
                 dict(kv_bstride=kext - 16), dict(kv_bstride=kext + 8), dict(kv_q8_scale=-1.0),
                 dict(L=5), dict(Tk=0), dict(Tk=KR.CROSS_MAX_KEYS + 8, kv_bstride=2 * H * (KR.CROSS_MAX_KEYS + 8) * 64), dict(nsplit=0),
                 dict(nsplit=KR.CROSS_MAX_SPLIT + 1)]
    for kw in bad_cross:
        cross_ex(lib, **{**okc, **kw}, expect_rc=1)
    assert bool((out == KR.SENTINEL).all()) and bool((present == KR.SENTINEL).all()) and bool((ws == KR.SENTINEL).all()), \
        "a refused call launched something"
    assert bool((past == 3.0).all())
    cross_ex(lib, **okc)
    assert not bool((out.view(-1)[:M * (Cn + 8)].view(M, Cn + 8)[:, :Cn] == KR.SENTINEL).any())
