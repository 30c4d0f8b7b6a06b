"""Decode cross-attention for candidate groups (csrc/attn_decode.hip, AttnCrossParams::G) through the test-only entry
wm_attn_cross_group_ex: the G candidate rows of an utterance (beams, best_of samples) read ONE copy of its K/V.

The contract is a bit contract: with the same nsplit, ksplit and skip setting, every live row of the grouped call has the bits
wm_attn_cross_ex gives for the same B rows on K/V repeated G times.  Inputs are on the exact grid of
tests/test_gpu_attn_decode_contract.py (whose buffer helpers this file uses), in that file's padded layout: slabs ldp = C + 4 with a
gap between slabs, ldo = C + 8, utterances of K/V 64 elements further apart than their extent, everything never read NaN.  The
fp32 reference is kernel_refs.attn_decode_ref at the bounds of tests/test_gpu_kernels.py::test_attn_decode_cross (1e-3 single pass,
2e-3 split)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_refs as KR  # noqa: E402
import native  # noqa: E402
import test_gpu_attn_decode_contract as AC  # noqa: E402  (helpers only: its tests are collected from its own file)

NAN = float("nan")
H = 2
CN = H * 64


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return native.load_library()


def group_ex(lib, *, part, B, L, Tk, kv, kv_bstride, out, G, ksplit=1, ldp=None, sstride=0, bias=None, kv_q8_scale=0.0, ldo=None,
             nsplit=1, ws=None, live=None, live_utt=None, skip=0, Hn=H, expect_rc=0):
    io = native.WmAttnCrossGroupIO()
    io.part, io.ksplit, io.ldp, io.part_sstride, io.bias = AC.ptr(part), ksplit, (Hn * 64 if ldp is None else ldp), sstride, AC.ptr(bias)
    io.B, io.L, io.H, io.Tk = B, L, Hn, Tk
    io.kv, io.kv_bstride, io.kv_q8_scale = AC.ptr(kv), kv_bstride, kv_q8_scale
    io.out, io.ldo, io.nsplit, io.ws, io.live, io.skip_zero_rows = AC.ptr(out), (Hn * 64 if ldo is None else ldo), nsplit, AC.ptr(ws), AC.ptr(live), skip
    io.G, io.live_utt = G, AC.ptr(live_utt)
    rc = lib.wm_attn_cross_group_ex(C.byref(io), AC.stream())
    torch.cuda.synchronize()
    if expect_rc == 0:
        native.check(rc, "wm_attn_cross_group_ex")
    else:
        assert rc == expect_rc, rc
        assert "attn_cross" in lib.wm_last_error().decode(), lib.wm_last_error()
    return rc


def lay_kv(stored, gap=64):
    """stored [A, 2, H, Tk, 64] (fp16 values or int8 codes) -> (device buffer, utterance stride): utterances `gap` elements further apart
    than their extent, the gaps NaN (fp16) / 77 (codes)."""
    A, _, Hn, Tk, _ = stored.shape
    bstride = 2 * Hn * Tk * 64 + gap
    if stored.dtype == torch.int8:
        buf = torch.full((A * bstride + 128,), 77, dtype=torch.int8)
    else:
        buf = torch.full((A * bstride + 128,), NAN, dtype=torch.float16)
    buf.as_strided((A, 2, Hn, Tk, 64), (bstride, Hn * Tk * 64, Tk * 64, 64, 1)).copy_(stored)
    return AC.dev(buf), bstride


class GroupRun:
    """One wm_attn_cross_group_ex launch in the padded layout of AC.CrossRun; the workspace carries a sentinel tail."""

    def __init__(self, lib, part, bias, B, L, Tk, kvbuf, kv_bstride, scale, nsplit, G, skip=0, live=None, live_utt=None):
        ks, M, N = part.shape
        assert N == CN and M == B * L
        ldp, ldo = CN + 4, CN + 8
        slabs, sstride = AC.lay_slabs(part, ldp, 8)
        self.out = AC.out_buffer(M, ldo)
        self.ws = AC.make_ws(B, H, nsplit, L)
        group_ex(lib, part=slabs, ksplit=ks, ldp=ldp, sstride=sstride, bias=AC.dev(bias) if bias is not None else None, B=B, L=L, Tk=Tk,
                 kv=kvbuf, kv_bstride=kv_bstride, kv_q8_scale=scale, out=self.out, ldo=ldo, nsplit=nsplit,
                 ws=self.ws if nsplit > 1 else None, live=live, live_utt=live_utt, skip=skip, G=G)
        self.rows = AC.out_rows(self.out, M, CN)
        n = B * H * nsplit * L * 66
        assert bool((self.ws[n if nsplit > 1 else 0:] == KR.SENTINEL).all()), "the workspace was written outside its blocks"
        self.ws_blocks = self.ws[:n].view(B, H * nsplit * L * 66)


def utterances(r, A, Tk, int8):
    """A utterances of random K/V: (stored [A, 2, H, Tk, 64], scale, K values, V values [A, H, Tk, 64] float64)."""
    _, _, t, Kv, Vv, stored = AC.make_kv(r, A, H, Tk, int8)
    return stored, t, Kv, Vv


def reference(part, bias, B, L, Kv, Vv, G, int8):
    q = KR.split_heads(KR.qkv_rows_ref(part, bias), B, L, H)
    return KR.merge_heads(KR.attn_decode_ref(q, Kv.repeat_interleave(G, 0), Vv.repeat_interleave(G, 0), k_exact=int8))


@pytest.mark.parametrize("variant", KR.CROSS_VARIANTS)
@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("Tk", [40, 1500])
@pytest.mark.parametrize("G", [2, 3, 5, 8])
def test_group_rows_have_the_bits_of_the_ungrouped_call_on_repeated_kv(lib, G, Tk, nsplit, variant):
    """3 utterances x G candidates, one token each: out rows and workspace blocks bit for bit those of wm_attn_cross_ex on the B = 3 G
    rows with every utterance's K/V repeated G times, for 1 and 3 q slabs with a bias; and within the kernel's bound of the reference."""
    A, int8, skip = 3, variant == "int8", int(variant == "fp16+SKIP")
    B = A * G
    for ks in (1, 3):
        r = KR.philox(((G * 4 + ks) * 2 + nsplit) * 3 + KR.CROSS_VARIANTS.index(variant) + Tk)
        part, bias = AC.grid_slabs(r, ks, B, CN)
        stored, t, Kv, Vv = utterances(r, A, Tk, int8)
        kv1, bs1 = lay_kv(stored)
        kvG, bsG = lay_kv(stored.repeat_interleave(G, 0))
        run = GroupRun(lib, part, bias, B, 1, Tk, kv1, bs1, t, nsplit, G, skip=skip)
        want = AC.CrossRun(lib, part, bias, B, 1, H, Tk, kvG, bsG, t, nsplit, skip=skip)
        assert AC.same_bits(run.rows, want.rows), f"ksplit {ks}: grouped rows differ from the ungrouped call on repeated K/V"
        if nsplit > 1:
            assert AC.same_bits(run.ws_blocks, want.ws_blocks), f"ksplit {ks}: workspace blocks differ (they are indexed by the original row)"
        err = float((run.rows.cpu().double() - reference(part, bias, B, 1, Kv, Vv, G, int8)).abs().max())
        assert err <= AC.cross_bound(nsplit), (ks, err)
        assert not bool(torch.isnan(run.rows.float()).any()), "a never-read region reached the output"


@pytest.mark.parametrize("variant", KR.CROSS_VARIANTS)
@pytest.mark.parametrize("G,L", [(2, 4), (4, 2)])
def test_group_prefill_passes_read_their_utterance(lib, G, L, variant):
    """L > 1: the row's own item reads K/V row b / G -- the bits of the per-row call on repeated K/V, single pass and split."""
    A, Tk, int8, skip = 3, 100, variant == "int8", int(variant == "fp16+SKIP")
    B = A * G
    for nsplit in (1, 3):
        r = KR.philox(900 + G * 8 + L + nsplit)
        part, bias = AC.grid_slabs(r, 3, B * L, CN)
        stored, t, Kv, Vv = utterances(r, A, Tk, int8)
        kv1, bs1 = lay_kv(stored)
        kvG, bsG = lay_kv(stored.repeat_interleave(G, 0))
        run = GroupRun(lib, part, bias, B, L, Tk, kv1, bs1, t, nsplit, G, skip=skip)
        want = AC.CrossRun(lib, part, bias, B, L, H, Tk, kvG, bsG, t, nsplit, skip=skip)
        assert AC.same_bits(run.rows, want.rows)
        if nsplit > 1:
            assert AC.same_bits(run.ws_blocks, want.ws_blocks)
        err = float((run.rows.cpu().double() - reference(part, bias, B, L, Kv, Vv, G, int8)).abs().max())
        assert err <= AC.cross_bound(nsplit), err


def test_group_v_skip_with_queries_peaked_on_different_keys(lib):
    """A peaked fixture, so that V rows really are skipped: every query's probabilities round to fp16 zero outside four keys of its own
    (scores of 288 there against ~ +-1 elsewhere), and the queries of a group peak on DIFFERENT keys -- a wave instruction's 8 rows may
    only be skipped when they weigh zero for every query of the group.  Skip on equals skip off, grouped equals ungrouped, bit for bit."""
    A, G, Tk = 2, 3, 1500
    B = A * G
    r = KR.philox(4242)
    signs = torch.from_numpy(r.integers(0, 2, size=(B, CN)).astype(np.float32) * 2 - 1)
    part = (signs * 6.0)[None]                                          # one slab, no bias: q = +-6 in every dim
    x = torch.from_numpy((r.standard_normal((A, 2, H, Tk, 64)) * 0.1).astype(np.float16))
    peaks = {}
    for b in range(B):
        a, j = divmod(b, G)
        k0 = 96 + 470 * j + 8 * a + 6                                   # rows k0 .. k0 + 3 straddle two groups of 8 rows
        peaks[b] = k0
        for h in range(H):
            x[a, 0, h, k0:k0 + 4] = (signs[b, h * 64:(h + 1) * 64] * 6.0).half()
    kv1, bs1 = lay_kv(x)
    kvG, bsG = lay_kv(x.repeat_interleave(G, 0))
    ref = reference(part, None, B, 1, x[:, 0].double(), x[:, 1].double(), G, False)
    p = KR.r16(torch.softmax(KR.r16(KR.r16(KR.split_heads(KR.qkv_rows_ref(part), B, 1, H).double() * float(np.float32(KR.QK_SCALE)))
                                       @ KR.r16(x[:, 0].double().repeat_interleave(G, 0) * float(np.float32(KR.QK_SCALE))).transpose(-1, -2)), dim=-1))
    assert int((p != 0).sum()) == B * H * 4, "the fixture must leave exactly four keys per query and head with a non-zero probability"
    plain = GroupRun(lib, part, None, B, 1, Tk, kv1, bs1, 0.0, 1, G, skip=0)
    skipped = GroupRun(lib, part, None, B, 1, Tk, kv1, bs1, 0.0, 1, G, skip=1)
    alone = AC.CrossRun(lib, part, None, B, 1, H, Tk, kvG, bsG, 0.0, 1, skip=1)
    assert AC.same_bits(skipped.rows, plain.rows), "the V-row skip changed a grouped row"
    assert AC.same_bits(skipped.rows, alone.rows), "grouped and ungrouped skip forms differ"
    err = float((skipped.rows.cpu().double() - ref).abs().max())
    assert err <= AC.cross_bound(1), err


@pytest.mark.parametrize("variant,nsplit", [("fp16", 1), ("fp16+SKIP", 1), ("fp16", 3), ("int8", 1), ("int8", 3)])
def test_group_live_lists(lib, variant, nsplit):
    """3 utterances x 3 candidates.  Utterance 0 has no live row and is not listed: its outputs and workspace blocks keep the sentinel.
    Utterance 1 has a dead row (4) between two live ones, utterance 2 is all live: every live row has the bits of the all-live launch,
    the dead row of the live utterance is finite.  The lists themselves are not written."""
    A, G, Tk, ks = 3, 3, 100, 3
    B, int8, skip = A * G, variant == "int8", int(variant == "fp16+SKIP")
    r = KR.philox(5100 + nsplit)
    part, bias = AC.grid_slabs(r, ks, B, CN)
    stored, t, Kv, Vv = utterances(r, A, Tk, int8)
    kv1, bs1 = lay_kv(stored)
    full = GroupRun(lib, part, bias, B, 1, Tk, kv1, bs1, t, nsplit, G, skip=skip)
    lv = [5, 3, 5, 6, 7, 8, 0, 0, 0, 0]
    lu = [2, 1, 2, 0]
    live, live_utt = torch.tensor(lv, dtype=torch.int32, device="cuda"), torch.tensor(lu, dtype=torch.int32, device="cuda")
    run = GroupRun(lib, part, bias, B, 1, Tk, kv1, bs1, t, nsplit, G, skip=skip, live=live, live_utt=live_utt)
    for b in (3, 5, 6, 7, 8):
        assert AC.same_bits(run.rows[b], full.rows[b]), f"live row {b} differs from the all-live launch"
        if nsplit > 1:
            assert AC.same_bits(run.ws_blocks[b], full.ws_blocks[b])
    for b in (0, 1, 2):
        assert bool((run.rows[b] == KR.SENTINEL).all()), f"row {b} of the finished utterance was written"
        assert bool((run.ws_blocks[b] == KR.SENTINEL).all()), f"the workspace block of row {b} of the finished utterance was written"
    assert bool(torch.isfinite(run.rows[4].float()).all()), "the dead row of a live utterance must stay finite"
    assert live.tolist() == lv and live_utt.tolist() == lu


def test_step_finish_group_writes_both_lists(lib):
    """wm_step_finish_group: the live rows as wm_step_finish writes them, the utterances with a live row beside them, the counter + 1."""
    B, G = 15, 3
    done = torch.tensor([1, 1, 1, 0, 1, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0], dtype=torch.int32, device="cuda")
    live = torch.full((1 + B,), -7, dtype=torch.int32, device="cuda")
    live_utt = torch.full((1 + B // G,), -7, dtype=torch.int32, device="cuda")
    counter = torch.tensor([41], dtype=torch.int32, device="cuda")
    native.check(lib.wm_step_finish_group(counter.data_ptr(), done.data_ptr(), B, G, live.data_ptr(), live_utt.data_ptr(), AC.stream()),
                 "wm_step_finish_group")
    torch.cuda.synchronize()
    assert live.tolist()[:7] == [6, 3, 5, 6, 7, 8, 14] and live_utt.tolist()[:4] == [3, 1, 2, 4] and int(counter) == 42
    want = live.clone().fill_(-7)
    native.check(lib.wm_step_finish(None, done.data_ptr(), B, want.data_ptr(), AC.stream()), "wm_step_finish")
    torch.cuda.synchronize()
    assert live.tolist()[:7] == want.tolist()[:7]
    assert lib.wm_step_finish_group(None, done.data_ptr(), B, 4, live.data_ptr(), live_utt.data_ptr(), AC.stream()) == 1


def test_group_argument_checks_launch_nothing(lib):
    """G < 1, B not a multiple of G, G * L > 8, a live list without its partner, and what wm_attn_cross_ex refuses: rc 1, wm_last_error
    set, nothing launched (sentinel-filled outputs and workspace keep their bits); the arguments they were derived from are accepted."""
    B, L, ks, Tk, ns, G = 4, 2, 2, 40, 2, 2
    M = B * L
    kext = 2 * H * Tk * 64
    part = torch.zeros(8 * M * (CN + 64), dtype=torch.float32, device="cuda")
    bias = torch.zeros(4 * CN, dtype=torch.float16, device="cuda")
    kv = torch.zeros(B * 2 * H * (KR.CROSS_MAX_KEYS + 8) * 64 + 4 * kext, dtype=torch.float16, device="cuda")
    out = torch.full((4 * M, 2 * CN), KR.SENTINEL, dtype=torch.float16, device="cuda")
    ws = torch.full((4 * B * H * ns * L * 66,), KR.SENTINEL, dtype=torch.float32, device="cuda")
    live = torch.tensor([B] + list(range(B)), dtype=torch.int32, device="cuda")
    live_utt = torch.tensor([B // G] + list(range(B // G)), dtype=torch.int32, device="cuda")
    ok = dict(part=part, ksplit=ks, ldp=CN + 4, sstride=M * (CN + 4) + 8, bias=bias, B=B, L=L, Tk=Tk, kv=kv, kv_bstride=kext + 64,
              out=out, ldo=CN + 8, nsplit=ns, ws=ws, G=G)
    bad = [dict(G=0), dict(G=-1), dict(G=3), dict(G=4, L=3), dict(G=2, L=5), dict(B=18, G=9, L=1), dict(L=1, live=live), dict(L=1, live_utt=live_utt),
           dict(live_utt=live_utt),
           dict(part=None), dict(kv=None), dict(out=None), dict(ws=None), dict(ksplit=0), dict(B=0), dict(Hn=0),
           dict(ldp=CN + 2), dict(ldp=CN - 4), dict(sstride=M * (CN + 4) + 2), dict(sstride=M * (CN + 4) - 4),
           dict(part=part.data_ptr() + 4), dict(bias=bias.data_ptr() + 2), dict(kv=kv.data_ptr() + 8), dict(ldo=CN - 8),
           dict(kv_bstride=kext - 16), dict(kv_bstride=kext + 8), dict(kv_q8_scale=-1.0),
           dict(L=5, G=1), dict(Tk=0), dict(Tk=KR.CROSS_MAX_KEYS + 8, kv_bstride=2 * H * (KR.CROSS_MAX_KEYS + 8) * 64), dict(nsplit=0),
           dict(nsplit=KR.CROSS_MAX_SPLIT + 1)]
    for kw in bad:
        group_ex(lib, **{**ok, **kw}, expect_rc=1)
    assert bool((out == KR.SENTINEL).all()) and bool((ws == KR.SENTINEL).all()), "a refused call launched something"
    group_ex(lib, **ok)
    assert not bool((out.view(-1)[:M * (CN + 8)].view(M, CN + 8)[:, :CN] == KR.SENTINEL).any())
    out.fill_(KR.SENTINEL)
    group_ex(lib, **{**ok, "L": 1, "live": live, "live_utt": live_utt})
    assert not bool((out.view(-1)[:B * (CN + 8)].view(B, CN + 8)[:, :CN] == KR.SENTINEL).any())
