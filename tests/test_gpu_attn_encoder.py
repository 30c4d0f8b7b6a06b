"""Encoder attention (csrc/attn_encoder.hip) against its arithmetic contract, through the test-only entry wm_attn_encoder_ex:
every launch form the product reaches (QB = 2 below T = 129, QB = 4, the persistent form on any number of workgroups), at the
sequence lengths either side of every tile, block and wave edge, with padded rows, and in score regimes a flat softmax hides.

Reference, inputs, tolerance and the list of cases: tests/attn_encoder_refs.py (checked on the CPU by
tests/test_attn_encoder_refs_cpu.py: the kernel's stored outputs meet the tolerance, wrong kernels -- a lost, a doubled, a
leaked key, a missed rescale, unrounded scores -- do not).  tests/test_gpu_attn_encoder_bits.py pins today's bytes; this file
says whether bytes are right, and stays valid when an optimisation reorders a sum.

What the shapes are for (T; clips x heads):  QB = 2: one key (1), either side of a 16-key block (15, 16, 17), of the tile (63,
64, 65) and of the 128-query workgroup (127, 128); (2, 1) has six padding items in its group of eight heads, (3, 3) a second
group.  QB = 4: (1, 8) has no padding item; 384 an even tile count and no tail; 449 a tail of one key and one live query
block in the last tile's wave 3; at 513 the last query tile has one query, waves 1 - 3 only stage K/V.

Every launch has a guard row behind the output and checks it; the uniform plantings are exact: q = 0 makes every weight 1 / T,
so v = 1 gives fp16 1.0 and v = 1 in row T - 1 alone gives fp16(1 / T) -- 0 with one key too few, 2 / T with that row twice."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_encoder_refs as R  # noqa: E402
import native  # noqa: E402

SENTINEL = 7.0


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return native.load_library()


def attn_ex(lib, qkv, ld, B, T, H, out, ldo, max_wgs):
    """One wm_attn_encoder_ex call on the current stream (qkv, out: tensors or raw addresses); the return code."""
    io = native.WmAttnEncoderIO()
    io.qkv, io.ld = (qkv if qkv is None or isinstance(qkv, int) else qkv.data_ptr()), ld
    io.B, io.T, io.H = B, T, H
    io.out, io.ldo, io.max_wgs = (out if out is None or isinstance(out, int) else out.data_ptr()), ldo, max_wgs
    rc = lib.wm_attn_encoder_ex(C.byref(io), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def run(lib, qkv, B, T, H, max_wgs=0, ldo=None):
    """[B, T, H * 64] fp16 numpy.  The output buffer has ldo columns and one guard row, all SENTINEL before the launch: the gap
    columns and the guard row must still be."""
    Cc = H * 64
    ldo = Cc if ldo is None else ldo
    x = torch.from_numpy(qkv).cuda()
    out = torch.full((B * T + 1, ldo), SENTINEL, dtype=torch.float16, device="cuda")
    native.check(attn_ex(lib, x, qkv.shape[1], B, T, H, out, ldo, max_wgs), "wm_attn_encoder_ex")
    o = out.cpu().numpy()
    assert (o[B * T] == SENTINEL).all(), "attn_encoder wrote behind its output"
    assert (o[:, Cc:] == SENTINEL).all(), "attn_encoder wrote into the gap columns of its output"
    return np.ascontiguousarray(o[:B * T, :Cc]).reshape(B, T, Cc)


_plain = {}


def plain(lib, regime, B, T, H):
    """The plain launch's output of a case, computed once."""
    key = (regime, B, T, H)
    if key not in _plain:
        _plain[key] = run(lib, R.make_case(*key), B, T, H)
    return _plain[key]


def hold_to_reference(case, got, what=""):
    ref = R.cached_reference(*case)
    bad = ref.violations(got)
    ex = ref.excess(got)
    print(f"{R.case_name(*case)}{what}: largest excess over the output rounding and the tie slack {np.nanmax(ex):.4f} x 2^-10 A "
          f"(c = {R.C_PROB}); tie slack leads in {100 * ref.slack_share():.2f} % of {got.size} elements")
    assert len(bad) == 0, (f"{R.case_name(*case)}{what}: {len(bad)} of {got.size} elements miss the tolerance; first (clip, row, column): "
                           f"{bad[:6].tolist()}, got {[float(got[tuple(i)]) for i in bad[:6]]}, want {[float(ref.ref[tuple(i)]) for i in bad[:6]]}")


def exact_value(regime, T):
    return np.float16(1.0) if regime == "uniform_ones" else np.float16(1.0 / T)


@pytest.mark.parametrize("regime,B,T,H", R.gpu_cases(), ids=lambda v: str(v))
def test_contract(lib, regime, B, T, H):
    got = plain(lib, regime, B, T, H)
    if regime in R.EXACT:
        want = exact_value(regime, T)
        off = np.argwhere(got.view(np.uint16) != want.view(np.uint16))
        assert len(off) == 0, f"{len(off)} outputs are not fp16 {want}: first (clip, row, column) {off[:6].tolist()}, got {[float(got[tuple(i)]) for i in off[:6]]}"
    else:
        hold_to_reference((regime, B, T, H), got)


@pytest.mark.parametrize("regime,B,T,H", R.STRIDE_CASES, ids=lambda v: str(v))
def test_padded_rows(lib, regime, B, T, H):
    """ld = 3 C + 8 with NaN in the gap columns (never read: a NaN in the output is a failure, NaN misses every tolerance), ldo = C + 4
    with the gap columns and the guard row checked by run().  The same values as the dense case: the same bytes, too."""
    Cc = H * 64
    got = run(lib, R.make_case(regime, B, T, H, ld=3 * Cc + 8), B, T, H, ldo=Cc + 4)
    assert not np.isnan(got).any(), "a gap column of qkv was read"
    hold_to_reference((regime, B, T, H), got, " (padded rows)")
    assert np.array_equal(got.view(np.uint16), plain(lib, regime, B, T, H).view(np.uint16)), "padded rows change the result"


def items(B, T, H):
    return B * H * ((T + 255) // 256)


@pytest.mark.parametrize("regime,B,T,H,wgs", [c[:4] + (w,) for c in R.PERSISTENT for w in c[4]], ids=lambda v: str(v))
def test_persistent_form(lib, regime, B, T, H, wgs):
    """The form the product runs beside the decode loop (max_wgs = 2 * cu_budget, any integer): grids below 8 and off the multiples of
    8, workgroups without a live item, successors with other live-query counts than their predecessors (T = 513 on 8 workgroups).
    Held to the reference and byte-equal to the plain form."""
    assert wgs < items(B, T, H)
    got = run(lib, R.make_case(regime, B, T, H), B, T, H, max_wgs=wgs)
    hold_to_reference((regime, B, T, H), got, f" on {wgs} workgroups")
    assert np.array_equal(got.view(np.uint16), plain(lib, regime, B, T, H).view(np.uint16)), "the persistent form differs from the plain form"


@pytest.mark.parametrize("regime,B,T,H", [c[:4] for c in R.PERSISTENT], ids=lambda v: str(v))
def test_max_wgs_at_or_above_the_item_count_is_the_plain_launch(lib, regime, B, T, H):
    n = items(B, T, H)
    for wgs in (n, n + 1, 8 * n):
        got = run(lib, R.make_case(regime, B, T, H), B, T, H, max_wgs=wgs)
        assert np.array_equal(got.view(np.uint16), plain(lib, regime, B, T, H).view(np.uint16)), wgs


@pytest.mark.parametrize("T", R.BATCH_T)
def test_batch_independence(lib, T):
    """Clip 0 launched alone is byte-equal to clip 0 of three clips."""
    B, H = 3, 3
    qkv = R.make_case("late", B, T, H)
    alone = run(lib, np.ascontiguousarray(qkv[:T]), 1, T, H)
    assert np.array_equal(alone[0].view(np.uint16), plain(lib, "late", B, T, H)[0].view(np.uint16))


def test_argument_checks(lib):
    """Every refusal of wm_attn_encoder_ex: rc 1, wm_last_error names the argument, nothing is launched (the output keeps its bytes)."""
    B, T, H = 2, 65, 2
    Cc = H * 64
    x = torch.from_numpy(R.make_case("normal", B, T, H, ld=3 * Cc + 8)).cuda()
    out = torch.full((B * T + 1, Cc + 4), SENTINEL, dtype=torch.float16, device="cuda")
    ok = dict(qkv=x, ld=3 * Cc + 8, B=B, T=T, H=H, out=out, ldo=Cc + 4, max_wgs=0)
    refusals = [("qkv", dict(qkv=None)), ("qkv", dict(qkv=x.data_ptr() + 8)), ("qkv", dict(qkv=x.data_ptr() + 2)),
                ("out", dict(out=None)), ("out", dict(out=out.data_ptr() + 4)), ("out", dict(out=out.data_ptr() + 2)),
                ("ld", dict(ld=3 * Cc - 8)), ("ld", dict(ld=3 * Cc + 4)), ("ld", dict(ld=0)),
                ("ldo", dict(ldo=Cc - 4)), ("ldo", dict(ldo=Cc + 2)), ("ldo", dict(ldo=0)),
                ("B", dict(B=0)), ("T", dict(T=0)), ("H", dict(H=0)), ("B", dict(B=-1)), ("T", dict(T=-1)), ("H", dict(H=-1)),
                ("max_wgs", dict(max_wgs=-1))]
    for name, change in refusals:
        rc = attn_ex(lib, **dict(ok, **change))
        err = lib.wm_last_error().decode()
        assert rc == 1, (change, rc)
        assert "wm_attn_encoder_ex" in err and name in err.split(":", 1)[1], (change, err)
        assert bool((out == SENTINEL).all()), f"{change}: refused, but the output was written"
    assert lib.wm_attn_encoder_ex(None, torch.cuda.current_stream().cuda_stream) == 1 and "io" in lib.wm_last_error().decode()
    native.check(attn_ex(lib, **ok), "wm_attn_encoder_ex")                      # the unchanged arguments are accepted
    assert bool((out[:B * T, :Cc] != SENTINEL).any())
