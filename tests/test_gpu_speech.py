"""Skip silence on the GPU: wm_speech_spans and wm_mel_gather (csrc/speech.hip) and transcribe_mel(speech=...) end to end.

* The kernels against speech.py, EXACTLY (everything is an integer or a copy, so there is no tolerance): outputs pre-filled
  with a sentinel, guard bands around the tables and the workspace, every file of a case in ONE ragged launch.  n_mels 1 / 3 / 80 /
  128; F 0, 1, 255, 256, 257, 1000, 5000 (5000: more than one 4096-element round of the span kernel); odd strides and bases; null
  and empty files; planted spans and gaps across wave (64), workgroup (1024) and round (4096) boundaries; the contract's edges
  (threshold M and M - 1, gap min_silence and min_silence - 1, length min_speech and min_speech - 1, pads clipped, joining and
  touching); thousands of one-frame runs; the floor with every value equal and with the rank on a bin boundary of every radix
  pass; rooms too small; the gather with odd ld, odd starts, odd bases, the pad columns, a span table that cannot be trusted.
* End to end on the micro-fullvocab engine (W = 128 frames, sample_len 12), like with like only (tests/test_gpu_longform.py says
  why): transcribe_mel(speech=...) against transcribe_mel over the packed mels as plain files followed by speech.restore.

Tolerances: none anywhere; every comparison is of integers, of fp16 bit patterns, or of results of the same arithmetic.

Measured on MI355X (printed by the tests): files of 1000, 300 and 400 frames with planted quiet stretches give the spans
[(0, 209), (491, 709), (751, 1000)], [(0, 109), (131, 300)] and none; 9 windows with `speech`, 15 without.  The 39 tests take 5 s.
"""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_refs as KR  # noqa: E402
import longform as LF  # noqa: E402
import native  # noqa: E402
import sections as S  # noqa: E402
import speech as SP  # noqa: E402
import synthetic  # noqa: E402
import transcribe as T  # noqa: E402
from decoding import DecodingOptions, WhisperDecoding  # noqa: E402
from encoding import WhisperEncoding  # noqa: E402
from oracle.whisper_oracle import Dims, synthetic_mel  # noqa: E402
from test_gpu_model import build_engine  # noqa: E402

SENTINEL = -77777
GUARD = 32


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return native.load_library()


@pytest.fixture(scope="module")
def tmpdir_module(tmp_path_factory):
    return str(tmp_path_factory.mktemp("engines"))


def upload(files):
    """files: [(mel fp16 numpy [n_mels, ld] or None, F, elements the base pointer sits inside its buffer)] -> (buffers, pointers, lds)."""
    keep, ptrs, lds = [], [], []
    for mel, F, offset in files:
        if mel is None:
            ptrs.append(0), lds.append(0)
            continue
        buf = torch.full((offset + mel.size + 5,), KR.SENTINEL, dtype=torch.float16, device="cuda")
        buf[offset: offset + mel.size] = torch.from_numpy(np.ascontiguousarray(mel).reshape(-1)).cuda()
        keep.append(buf)
        ptrs.append(buf.data_ptr() + 2 * offset), lds.append(mel.shape[1])
    return keep, ptrs, lds


# ----------------------------------------------------------------------------------------------------------- wm_speech_spans
def device_spans(lib, files, n_mels, cfg, spans_ld=None, total=None):
    """cfg = (h, step, permille, min_silence, min_speech, pad).  Returns (n_spans list, spans int array [batch, spans_ld, 2]) after
    checking the guard bands and the sentinel behind every file's spans."""
    h, step, permille, min_silence, min_speech, pad = cfg
    batch = len(files)
    keep, ptrs, lds = upload(files)
    content = [F for _, F, _ in files]
    if spans_ld is None:
        spans_ld = max(1, (max(content) + min_silence) // (1 + min_silence))
    if total is None:
        total = sum(F for mel, F, _ in files if mel is not None)
    src = torch.tensor(ptrs, dtype=torch.int64, device="cuda")
    ld = torch.tensor(lds, dtype=torch.int32, device="cuda")
    cont = torch.tensor(content, dtype=torch.int32, device="cuda")
    out = torch.full((GUARD + batch * spans_ld * 2 + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    n_spans = torch.full((batch + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    ws_bytes = int(lib.wm_speech_spans_workspace_bytes(batch, total))
    ws = torch.empty(ws_bytes + 64, dtype=torch.uint8, device="cuda")
    ws[ws_bytes:] = 0xA5
    native.check(lib.wm_speech_spans(src.data_ptr(), ld.data_ptr(), cont.data_ptr(), batch, n_mels, h, step, permille, min_silence,
                                     min_speech, pad, out[GUARD:].data_ptr(), spans_ld, n_spans.data_ptr(), ws.data_ptr(), ws_bytes,
                                     total, torch.cuda.current_stream().cuda_stream), "wm_speech_spans")
    torch.cuda.synchronize()
    got, n = out.cpu().numpy(), n_spans.cpu().numpy()
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + batch * spans_ld * 2:] == SENTINEL).all(), "written outside `spans`"
    assert (n[batch:] == SENTINEL).all(), "written outside `n_spans`"
    assert bool((ws[ws_bytes:] == 0xA5).all()), "written outside the workspace"
    spans = got[GUARD: GUARD + batch * spans_ld * 2].reshape(batch, spans_ld, 2)
    for b in range(batch):
        if n[b] >= 0:
            assert (spans[b, min(int(n[b]), spans_ld):] == SENTINEL).all(), f"file {b}: written behind its spans"
    return [int(v) for v in n[:batch]], spans


def check_against_contract(lib, files, n_mels, cfg):
    n, spans = device_spans(lib, files, n_mels, cfg)
    wants = []
    for b, (mel, F, _) in enumerate(files):
        want = [] if mel is None else SP.speech_spans_ref(mel, F, *cfg)
        got = [tuple(x) for x in spans[b, :max(n[b], 0)].tolist()]
        assert n[b] == len(want) and got == want, (b, F, None if mel is None else mel.shape, n[b], got[:6], want[:6])
        wants.append(want)
    return wants


def speechlike(rng, n_mels, ld, F, loud=((0.1, 0.3), (0.5, 0.8)), quiet=-2.0):
    """A quiet mel with loud stretches at the given fractions of F (and noise on both), fp16."""
    mel = (rng.standard_normal((n_mels, ld)) * 0.05 + quiet).astype(np.float16)
    for a, b in loud:
        a, b = int(a * F), int(b * F)
        mel[:, a:b] = (rng.standard_normal((n_mels, b - a)) * 0.3 + 1.0).astype(np.float16)
    return mel


CONFIGS = [(3, 205, 100, 20, 5, 4), (0, 1, 0, 1, 1, 0), (10, 205, 100, 200, 25, 40), (0, 32768, 1000, 3, 2, 1), (50, 100, 500, 7, 7, 100)]


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("n_mels", [1, 3, 80, 128])
def test_speech_spans_equal_the_contract(lib, n_mels, cfg):
    rng = KR.philox(100 * n_mels + cfg[0] + cfg[3])
    sizes = [0, 1, 255, 256, 257, 1000, 5000]
    pads = [0, 1, 2, 7, 0, 3, 1]                    # src_ld = F + pad: equal and larger, odd and even
    offsets = [0, 1, 3, 0, 1, 3, 1]                 # the base pointer inside its buffer, in elements
    files = []
    for F, pad, off in zip(sizes, pads, offsets):
        files.append((speechlike(rng, n_mels, max(1, F + pad), F), F, off))
    files.append(((rng.standard_normal((n_mels, 4099)) * 3.0).astype(np.float16), 4099, 0))      # noise: many short runs
    wants = check_against_contract(lib, files, n_mels, cfg)
    assert wants[0] == []
    if cfg == CONFIGS[0]:
        assert len(wants[5]) == 2 and len(wants[6]) == 2          # the two loud stretches survive as two spans


def test_ragged_batch_with_a_null_file_and_an_empty_one(lib):
    rng = KR.philox(21)
    files = [(speechlike(rng, 80, 777, 777), 777, 0), (None, 500, 0), (speechlike(rng, 80, 64, 64), 0, 1),
             (speechlike(rng, 80, 1203, 1200), 1200, 3), (speechlike(rng, 80, 97, 97), 97, 0), (None, 0, 0),
             (speechlike(rng, 80, 5001, 5000), 5000, 1), (speechlike(rng, 80, 256, 256), 256, 0)]
    wants = check_against_contract(lib, files, 80, CONFIGS[0])
    assert wants[1] == [] and wants[2] == [] and wants[5] == [] and len(wants[0]) == 2 and len(wants[6]) == 2


def planted(n_mels, F, spans, loud=1.0, quiet=-2.0):
    mel = np.full((n_mels, F + 1), quiet, dtype=np.float16)
    for a, b in spans:
        mel[:, a:b] = np.float16(loud)
    return mel


def test_planted_spans_across_wave_workgroup_and_round_boundaries(lib):
    """h = 0, permille = 0 (the floor is the quietest frame), pad = 0: the spans come back as planted when they are min_speech long
    and min_silence apart -- spans that begin, end or have their gap on frame 64, 1024 and 4096, the boundaries of a wave, of the
    workgroup's threads and of a round of the span kernel."""
    cfg = (0, 100, 0, 3, 2, 0)
    spans = [(10, 64), (67, 128), (1000, 1024), (1027, 1030), (2046, 2050), (4090, 4096), (4099, 4100 + 60), (8190, 8194), (9000, 9216)]
    for n_mels in (1, 80):
        wants = check_against_contract(lib, [(planted(n_mels, 9216, spans), 9216, 1)], n_mels, cfg)
        assert wants[0] == spans
    # gaps of min_silence - 1 join, of min_silence do not; lengths of min_speech - 1 go, of min_speech stay
    spans = [(62, 64), (66, 70), (73, 74), (1022, 1024), (1026, 1027), (4095, 4096), (4099, 4101), (4104, 4105)]
    wants = check_against_contract(lib, [(planted(3, 5000, spans), 5000, 0)], 3, cfg)
    assert wants[0] == [(62, 70), (1022, 1027), (4099, 4101)]


def test_contract_edges(lib):
    n_mels, F = 3, 600
    # the threshold: s - floor == M stays, M - 1 goes (h = 0: s = q; step 100: M = 300; a bin at k / 1024 adds k)
    mel = np.zeros((n_mels, F), dtype=np.float16)
    mel[0, 100:110] = np.float16(300 / 1024)
    mel[0, 200:210] = np.float16(299 / 1024)
    wants = check_against_contract(lib, [(mel, F, 0)], n_mels, (0, 100, 0, 5, 2, 0))
    assert wants[0] == [(100, 110)]
    # pads: clipped at 0 and at F, joining, touching exactly, and one frame short of touching
    for spans, pad, want in (([(2, 10), (590, 598)], 5, [(0, 15), (585, 600)]),
                             ([(100, 110), (130, 140)], 10, [(90, 150)]),                        # touch exactly: joined
                             ([(100, 110), (131, 140)], 10, [(90, 120), (121, 150)]),
                             ([(100, 110), (120, 140)], 10, [(90, 150)])):                        # overlap
        wants = check_against_contract(lib, [(planted(n_mels, F, spans)[:, :F].copy(), F, 0)], n_mels, (0, 100, 0, 5, 2, pad))
        assert wants[0] == want, (spans, pad, wants[0])
    # F in {1, 2}, permille 0 and 1000, every value equal (every flag clear), every flag set
    for F2 in (1, 2):
        for permille in (0, 1000):
            check_against_contract(lib, [(np.full((n_mels, F2), 1.0, dtype=np.float16), F2, 0)], n_mels, (0, 100, permille, 5, 1, 3))
    loud = np.full((n_mels, 300), 1.0, dtype=np.float16)
    loud[:, 7] = np.float16(-4.0)                                      # one quiet frame is the floor; h = 2 spreads it over 5
    wants = check_against_contract(lib, [(loud, 300, 1)], n_mels, (2, 100, 0, 6, 1, 0))
    assert wants[0] == [(0, 300)]                                      # the gap of 5 is shorter than min_silence
    # smoothing wider than the file; non-finite and huge values
    rng = KR.philox(13)
    check_against_contract(lib, [(speechlike(rng, 3, 9, 9), 9, 1), (speechlike(rng, 3, 40, 37), 37, 0)], 3, (50, 100, 100, 2, 1, 1))
    mel = speechlike(rng, 3, 1501, 1500)
    what = np.array([np.inf, -np.inf, np.nan, 65504.0, -65504.0, 16.0, -16.0, 17.0, 2.0 ** -11, 3 * 2.0 ** -11], dtype=np.float16)
    mel[rng.integers(0, 3, size=200), rng.integers(0, 1500, size=200)] = what[rng.integers(0, len(what), size=200)]
    everything = np.full((3, 700), np.nan, dtype=np.float16)
    everything[1] = np.inf
    wants = check_against_contract(lib, [(mel, 1500, 1), (everything, 700, 0)], 3, CONFIGS[0])
    assert wants[1] == []


def test_thousands_of_one_frame_runs(lib):
    """Every other frame loud, 20 001 frames: 10 001 runs of one frame.  min_silence 1 keeps them apart (10 001 spans through all
    four stages, three rounds of the compaction); min_silence 2 joins them all."""
    F = 20001
    mel = np.full((1, F), -2.0, dtype=np.float16)
    mel[:, 0::2] = np.float16(1.0)
    wants = check_against_contract(lib, [(mel, F, 1)], 1, (0, 100, 0, 1, 1, 0))
    assert wants[0] == [(t, t + 1) for t in range(0, F, 2)]
    wants = check_against_contract(lib, [(mel, F, 0)], 1, (0, 100, 0, 2, 1, 0))
    assert wants[0] == [(0, F)]
    wants = check_against_contract(lib, [(mel, F, 0)], 1, (0, 100, 0, 1, 2, 0))
    assert wants[0] == []


def test_floor_selection(lib):
    """One bin of one mel: q = s = the bin's value * 1024, so the keys of the radix select can be planted.  With h = 0 and
    values k / 1024 for k in a range that crosses the low byte (..., 255, 256, ...) and, scaled, the second byte, the rank of
    every permille lands on, before and after a histogram-bin boundary; 16 * 1024 = 0x4000 and negative values reach the upper
    bytes and the sign."""
    cases = []
    rng = KR.philox(31)
    for values in (np.arange(0, 1000), np.arange(-500, 500), np.arange(0, 1000) * 16 - 8000, np.full(1000, 37), np.full(1000, -16384),
                   np.concatenate([np.full(500, 255), np.full(500, 256)]), np.concatenate([np.full(100, -1), np.full(900, 0)]),
                   rng.integers(-1024, 1025, size=1000) * 16):
        v = np.array(values, dtype=np.int64)
        rng.shuffle(v)
        mel = (v.astype(np.float32) / 1024.0).astype(np.float16).reshape(1, -1)
        assert (np.rint(mel.astype(np.float32) * 1024).astype(np.int64).reshape(-1) == v).all()
        cases.append(mel)
    for permille in (0, 1, 99, 100, 255, 256, 257, 500, 999, 1000):
        files = [(m, m.shape[1], i % 2) for i, m in enumerate(cases)]
        wants = check_against_contract(lib, files, 1, (0, 1, permille, 1, 1, 0))
        assert wants[3] == [] and wants[4] == []                       # every value equal: nothing stands above the floor
        floor = SP.floor_of(S.loudness(cases[0], 1000), permille)
        assert floor == min(999, permille)                             # (values 0 .. 999: the floor is the rank itself)


def test_rooms_too_small(lib):
    cfg = (0, 100, 0, 3, 2, 0)
    spans = [(10, 20), (30, 40), (50, 60), (70, 80), (90, 100)]
    mel = planted(3, 999, spans)
    n, got = device_spans(lib, [(mel, 1000, 0), (mel[:, :45].copy(), 45, 0)], 3, cfg, spans_ld=3)
    assert n == [-1, 2] and got[1, :2].tolist() == [[10, 20], [30, 40]]          # (device_spans checked the guards)
    # a file whose frames end beyond total_frames is left alone and says so, and so does every later file that has frames
    files = [(mel[:, :300].copy(), 300, 0), (mel, 1000, 0), (mel[:, :64].copy(), 0, 0), (None, 500, 0), (mel[:, :200].copy(), 200, 1)]
    n, got = device_spans(lib, files, 3, cfg, total=700)
    assert n == [5, -1, 0, 0, -1] and [tuple(x) for x in got[0, :5].tolist()] == spans


def test_speech_spans_bad_arguments(lib):
    s = torch.cuda.current_stream().cuda_stream
    z = torch.zeros(64, dtype=torch.int64, device="cuda")                       # a null file of no frames
    o = torch.zeros(256, dtype=torch.int32, device="cuda")
    ws_bytes = int(lib.wm_speech_spans_workspace_bytes(1, 100))
    assert ws_bytes >= 16 + 4 * 400 and lib.wm_speech_spans_workspace_bytes(0, 100) == 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    p, q = z.data_ptr(), o.data_ptr()

    def call(src=p, ld=p, content=p, batch=1, n_mels=80, h=3, step=205, permille=100, min_silence=20, min_speech=5, pad=4,
             spans=q + 64, spans_ld=4, n_spans=q, w=ws.data_ptr(), wb=ws_bytes, total=100):
        return lib.wm_speech_spans(src, ld, content, batch, n_mels, h, step, permille, min_silence, min_speech, pad, spans, spans_ld,
                                   n_spans, w, wb, total, s)

    assert call() == 0
    for bad in (dict(src=None), dict(ld=None), dict(content=None), dict(spans=None), dict(n_spans=None), dict(w=None), dict(batch=0),
                dict(n_mels=0), dict(step=0), dict(step=32769), dict(permille=-1), dict(permille=1001), dict(min_silence=0),
                dict(min_speech=0), dict(pad=-1), dict(h=-1), dict(h=819), dict(wb=ws_bytes - 1), dict(total=200), dict(total=-1),
                dict(spans_ld=-1), dict(spans=q + 2)):
        assert call(**bad) == 1, bad
        assert "wm_speech_spans" in lib.wm_last_error().decode(), bad
    assert call(h=818, step=32768) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- wm_mel_gather
def device_gather(lib, files, tables, n_mels, n_pad, spans_ld=None, dst_lds=None, dst_offsets=None):
    """files as above; tables[b]: the (a, b) pairs as they stand in the device table.  Returns per file the destination
    [n_mels, dst_ld] as int16 bit patterns (None for a null file), pre-filled with a sentinel; guard bands checked."""
    batch = len(files)
    keep, ptrs, lds = upload(files)
    if spans_ld is None:
        spans_ld = max(1, max(len(t) for t in tables))
    if dst_lds is None:
        dst_lds = [0 if mel is None else sum(b - a for a, b in SP.taken_spans(t, mel.shape[1])) + n_pad for (mel, _, _), t in zip(files, tables)]
    dst_offsets = dst_offsets or [i % 2 for i in range(batch)]
    flat = np.full((batch, spans_ld, 2), 123456789, dtype=np.int32)
    for b, t in enumerate(tables):
        for k, (a, e) in enumerate(t):
            flat[b, k] = (a, e)
    outs, dptr = [], []
    for (mel, _, _), dl, off in zip(files, dst_lds, dst_offsets):
        if mel is None:
            outs.append(None), dptr.append(0)
            continue
        buf = torch.full((GUARD + off + n_mels * dl + GUARD,), 0x7b7b, dtype=torch.int16, device="cuda")
        outs.append(buf)
        dptr.append(buf.data_ptr() + 2 * (GUARD + off))
    src = torch.tensor(ptrs, dtype=torch.int64, device="cuda")
    dst = torch.tensor(dptr, dtype=torch.int64, device="cuda")
    ld = torch.tensor(lds, dtype=torch.int32, device="cuda")
    dl = torch.tensor(dst_lds, dtype=torch.int32, device="cuda")
    tab = torch.from_numpy(flat).cuda()
    ns = torch.tensor([len(t) for t in tables], dtype=torch.int32, device="cuda")
    native.check(lib.wm_mel_gather(src.data_ptr(), ld.data_ptr(), tab.data_ptr(), ns.data_ptr(), spans_ld, batch, n_mels, n_pad,
                                   dst.data_ptr(), dl.data_ptr(), torch.cuda.current_stream().cuda_stream), "wm_mel_gather")
    torch.cuda.synchronize()
    result = []
    for buf, d, off in zip(outs, dst_lds, dst_offsets):
        if buf is None:
            result.append(None)
            continue
        host = buf.cpu().numpy()
        assert (host[:GUARD + off] == 0x7b7b).all() and (host[GUARD + off + n_mels * d:] == 0x7b7b).all(), "written outside a destination"
        result.append(host[GUARD + off: GUARD + off + n_mels * d].reshape(n_mels, d))
    return result


def expected_gather(mel, table, n_pad, dst_ld):
    taken = SP.taken_spans(table, mel.shape[1])
    want = np.concatenate([mel[:, a:b] for a, b in taken] + [np.repeat(mel[:, -1:], n_pad, axis=1)], axis=1).view(np.int16)
    out = np.full((mel.shape[0], dst_ld), 0x7b7b, dtype=np.int16)
    n = min(dst_ld, want.shape[1])
    out[:, :n] = want[:, :n]
    return out


@pytest.mark.parametrize("n_mels", [1, 3, 80, 128])
def test_gather_equals_the_contract(lib, n_mels):
    """Odd ld, odd span starts, odd bases of source and destination; a file of more than one window of 2048 packed frames; a file
    without spans (pad columns only); spans that touch; a null file."""
    rng = KR.philox(7 + n_mels)
    mk = lambda ld: (rng.standard_normal((n_mels, ld)) * 2.0).astype(np.float16)      # noqa: E731
    files = [(mk(1001), 990, 1), (mk(5200), 5200, 0), (mk(77), 70, 3), (None, 0, 0), (mk(300), 300, 1), (mk(6001), 6000, 0)]
    tables = [[(1, 2), (3, 300), (301, 990)], [(0, 2047), (2049, 2050), (2051, 5200)], [], [(5, 9)], [(7, 8), (8, 31), (200, 300)],
              [(k, k + 1) for k in range(1, 6000, 2)]]                                            # 3000 spans of one frame
    for n_pad in (0, 128):
        got = device_gather(lib, files, tables, n_mels, n_pad)
        for b, ((mel, F, _), t) in enumerate(zip(files, tables)):
            if mel is None:
                continue
            want = SP.packed_mel_ref(mel, F, t, n_pad).view(np.int16) if b != 4 else expected_gather(mel, t, n_pad, got[b].shape[1])
            assert got[b].shape == want.shape and np.array_equal(got[b], want), (b, n_pad)


def test_gather_skips_what_it_cannot_trust(lib):
    rng = KR.philox(41)
    mel = (rng.standard_normal((3, 501)) * 2.0).astype(np.float16)
    good = [(10, 20), (30, 41), (100, 200)]
    for bad in ((50, 502), (-5, 60), (60, 50), (2 ** 31 - 1, -2 ** 31), (70, 70), (-2 ** 31, 2 ** 31 - 1), (35, 60), (0, 5)):
        table = good[:2] + [bad] + good[2:]
        got = device_gather(lib, [(mel, 501, 1)], [table], 3, 16)[0]
        taken = SP.taken_spans(table, 501)
        assert taken == good or bad in ((35, 60), (0, 5))                 # out of range: the neighbours stand as they were
        assert np.array_equal(got, expected_gather(mel, table, 16, got.shape[1])), bad
    assert SP.taken_spans(good[:2] + [(35, 60)] + good[2:], 501) == good          # (in range but out of order: skipped, and 100 >= 60)
    # n_spans beyond the table's room and negative; a destination that is too short: nothing behind dst_ld
    got = device_gather(lib, [(mel, 501, 0)], [good], 3, 16, dst_lds=[100])[0]
    assert np.array_equal(got, expected_gather(mel, good, 16, 100))
    got = device_gather(lib, [(mel, 501, 0)], [good], 3, 16, dst_lds=[125])[0]      # (121 packed frames and 4 of the 16 pad columns)
    assert np.array_equal(got, expected_gather(mel, good, 16, 125))


def test_gather_bad_arguments(lib):
    s = torch.cuda.current_stream().cuda_stream
    z = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = z.data_ptr()

    def call(src=p, ld=p, spans=p, n_spans=p, spans_ld=4, batch=1, n_mels=80, n_pad=128, dst=p, dst_ld=p):
        return lib.wm_mel_gather(src, ld, spans, n_spans, spans_ld, batch, n_mels, n_pad, dst, dst_ld, s)

    assert call() == 0                                                           # (a null file: nothing to do)
    for bad in (dict(src=None), dict(ld=None), dict(spans=None), dict(n_spans=None), dict(dst=None), dict(dst_ld=None), dict(batch=0),
                dict(batch=65536), dict(n_mels=0), dict(spans_ld=-1), dict(n_pad=-1), dict(spans=p + 2), dict(n_spans=p + 1)):
        assert call(**bad) == 1, bad
        assert "wm_mel_gather" in lib.wm_last_error().decode(), bad
    torch.cuda.synchronize()


def test_wrappers_one_launch_for_all_files(lib):
    rng = KR.philox(29)
    content = [1000, 0, 300, 5000]
    host = [speechlike(rng, 80, F + 128, F) for F in content]
    host[2][:] = np.float16(-1.0)                                                # a file without speech
    mels = [torch.from_numpy(m).cuda() for m in host]
    opts = SP.SpeechOptions(min_silence_seconds=5.0, min_speech_seconds=1.0, speech_pad_seconds=2.0)
    cfg = opts.frames(128, 80)
    assert cfg == (0, 205, 100, 21, 4, 9)
    spans = T.speech_spans(mels, content, opts, window=128)
    assert spans == [SP.speech_spans_ref(m, F, *cfg) for m, F in zip(host, content)]
    assert len(spans[0]) == 2 and spans[1] == [] and spans[2] == [] and len(spans[3]) == 2
    packed, frames = T.packed_mels(mels, content, spans, 128)
    assert frames == [sum(b - a for a, b in sp) for sp in spans]
    for m, F, sp, p in zip(host, content, spans, packed):
        want = SP.packed_mel_ref(m, F, sp, 128)
        assert p.is_contiguous() and tuple(p.shape) == want.shape and np.array_equal(p.cpu().numpy().view(np.int16), want.view(np.int16))
    assert T.speech_spans([], [], opts) == [] and T.packed_mels([], [], [], 128) == ([], [])
    with pytest.raises(ValueError):
        T.packed_mels(mels[:1], content[:1], [[(5, 3)]], 128)


# --------------------------------------------------------------------------------------------------------------- end to end
CONTENTS = [1000, 300, 400]
OPTS = SP.SpeechOptions(min_silence_seconds=5.0, min_speech_seconds=1.0, speech_pad_seconds=2.0)       # at W = 128: 21, 4, 9 frames
QUIET = [[(200, 500), (700, 760)], [(100, 140)], [(0, 400)]]     # file 0: a stretch longer than a window; file 2: nothing but quiet
N_ROWS = 2
KW = dict(temperatures=(0.0,), compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None)


@pytest.fixture(scope="module")
def engines(tmpdir_module):
    dims = Dims(**synthetic.DIMS["micro-fullvocab"])
    eng = build_engine(tmpdir_module, "micro-fullvocab", 3)
    W = 2 * dims.n_audio_ctx
    mels = []
    for i, c in enumerate(CONTENTS):
        m = synthetic_mel(1, c + W, dims.n_mels, 700 + i)[0].half()
        low = float(m.float().min()) - 3.0
        for a, b in QUIET[i]:
            m[:, a:b] = low
        m[:, c:] = low
        mels.append(m.cuda().contiguous())
    return dims, eng, WhisperEncoding(eng), mels


def run_both(enc, dec, dims, mels, contents=None, sections=None, **kw):
    """The filtered run and the reference: the packed mels as plain files through the path without `speech`, then speech.restore."""
    contents = contents or CONTENTS
    W = 2 * dims.n_audio_ctx
    fs = LF.CHUNK_LENGTH / W
    spans = T.speech_spans(mels, contents, OPTS, window=W)
    packed, frames = T.packed_mels(mels, contents, spans, W)
    trace, ref_trace = [], []
    torch.manual_seed(5)
    results = T.transcribe_mel(enc, dec, mels, contents, n_rows=N_ROWS, trace=trace, speech=OPTS, sections=sections, **kw)
    torch.manual_seed(5)
    reference = T.transcribe_mel(enc, dec, packed, frames, n_rows=N_ROWS, trace=ref_trace, sections=sections, **kw)
    before = copy.deepcopy(reference)
    for res, ref, sp in zip(results, reference, spans):
        assert res["speech"] == [(a * fs, b * fs) for a, b in sp]
        assert res["segments"] == SP.restore(ref["segments"], sp, fs) and res["language"] == ref["language"] and res["text"] == ref["text"]
        assert [s["tokens"] for s in res["segments"]] == [s["tokens"] for s in ref["segments"]]
    assert reference == before                                                   # restore left its input alone
    assert len(trace) == len(ref_trace)
    for e, r in zip(trace, ref_trace):
        assert e.get("kind") == r.get("kind") and e["round"] == r["round"] and e["rows"] == r["rows"]
        if e.get("kind") != "align":
            assert torch.equal(e["windows"], r["windows"]) and e["live"] == r["live"]
    return results, trace, reference, spans


def test_filtered_run_equals_the_packed_files_restored(lib, engines):
    dims, eng, enc, mels = engines
    W = 2 * dims.n_audio_ctx
    fs = LF.CHUNK_LENGTH / W
    dec = WhisperDecoding(eng, options=DecodingOptions(language="en"))
    dec.sample_len = 12
    results, trace, reference, spans = run_both(enc, dec, dims, mels, **KW)
    host = [m.cpu().numpy() for m in mels]
    cfg = OPTS.frames(W, dims.n_mels)
    assert spans == [SP.speech_spans_ref(m, F, *cfg) for m, F in zip(host, CONTENTS)]
    # the planted quiet stretches are gone but for the pads
    assert len(spans[0]) == 3 and len(spans[1]) == 2
    assert spans[0][0][0] == 0 and spans[0][0][1] <= 200 + 9 + 1 and spans[0][1][0] >= 500 - 9 - 1 and spans[0][-1][1] == 1000
    assert spans[2] == [] and results[2]["segments"] == [] and results[2]["text"] == "" and results[2]["language"] == "en"
    assert all(r[0] != 2 for e in trace for r in e["rows"] if r is not None), "a decoder row for the file without speech"
    # fewer windows than the unfiltered run, and no segment begins inside the stretch that was removed
    plain = []
    T.transcribe_mel(enc, dec, mels, CONTENTS, n_rows=N_ROWS, trace=plain, **KW)
    windows = lambda tr: sum(sum(e["live"]) for e in tr)                         # noqa: E731
    print(f"speech end to end: spans {spans}; {windows(trace)} windows with `speech`, {windows(plain)} without")
    assert windows(trace) < windows(plain)
    a, b = spans[0][0][1] * fs, spans[0][1][0] * fs
    assert results[0]["segments"] and not any(a <= s["start"] < b for s in results[0]["segments"])
    assert all("speech" not in r for r in reference)


def test_with_sections_word_timestamps_and_conditioning(lib, engines):
    dims, eng, enc, mels = engines
    W = 2 * dims.n_audio_ctx
    fs = LF.CHUNK_LENGTH / W
    dec = WhisperDecoding(eng, options=DecodingOptions(language="en"))
    dec.sample_len = 12
    sec = S.SectionOptions(max_seconds=30.0)
    results, _, reference, spans = run_both(enc, dec, dims, mels, sections=sec, **KW)
    for res, ref, sp in zip(results, reference, spans):
        assert res["sections"] == [(SP.restore_time(a, sp, fs), SP.restore_time(b, sp, fs, end=True)) for a, b in ref["sections"]]
        if sp:
            assert res["sections"][0][0] == sp[0][0] * fs and res["sections"][-1][1] == sp[-1][1] * fs
    results, trace, reference, spans = run_both(enc, dec, dims, mels, word_timestamps=True, **KW)
    n_words = sum(len(s["words"]) for r in results for s in r["segments"])
    assert n_words > 0 and any(e.get("kind") == "align" for e in trace)
    for res, ref, sp in zip(results, reference, spans):
        P = SP.packed_starts(sp)
        for s, r in zip(res["segments"], ref["segments"]):
            for w, v in zip(s["words"], r["words"]):
                mid = (v["start"] + v["end"]) / 2
                k = max([i for i in range(len(sp)) if P[i] * fs <= mid] or [0])
                assert w["start"] == v["start"] + (sp[k][0] - P[k]) * fs and w["end"] == v["end"] + (sp[k][0] - P[k]) * fs
    prompted = WhisperDecoding(eng, row_prompts=True, options=DecodingOptions(language="en"))
    prompted.sample_len = 12
    results, trace, _, _ = run_both(enc, prompted, dims, mels, condition_on_previous_text=True, **KW)
    assert any(any(p for p in e["prompts"]) for e in trace if e.get("kind") != "align")


def test_refusals_stay_and_the_plain_path_is_what_it_was(lib, engines, monkeypatch):
    dims, eng, enc, mels = engines
    called = []
    monkeypatch.setattr(T, "speech_spans", lambda *a, **k: called.append(1))
    with pytest.raises(ValueError, match="prompt"):
        T.transcribe_mel(enc, WhisperDecoding(eng, options=DecodingOptions(prompt=[100, 200])), mels, CONTENTS, speech=OPTS)
    with pytest.raises(ValueError, match="condition_on_previous_text"):
        T.transcribe_mel(enc, WhisperDecoding(eng), mels, CONTENTS, speech=OPTS, condition_on_previous_text=True)
    assert called == []                                                          # refused before any device work
    monkeypatch.undo()
    with pytest.raises(ValueError, match="step"):
        T.transcribe_mel(enc, WhisperDecoding(eng), mels, CONTENTS, speech=SP.SpeechOptions(margin_db=0.0))
    dec = WhisperDecoding(eng, options=DecodingOptions(language="en"))
    dec.sample_len = 12
    a, b = [], []
    torch.manual_seed(5)
    one = T.transcribe_mel(enc, dec, mels, CONTENTS, n_rows=N_ROWS, trace=a, **KW)
    torch.manual_seed(5)
    two = T._transcribe_files(enc, dec, mels, CONTENTS, None, n_rows=N_ROWS, trace=b, condition_on_previous_text=False,
                              initial_prompt=None, word_timestamps=False, **KW)
    assert one == two and len(a) == len(b) and all("speech" not in r for r in one)
    for e, r in zip(a, b):
        assert e["rows"] == r["rows"] and e["live"] == r["live"] and torch.equal(e["windows"], r["windows"])
        assert [None if x is None else x.tokens for x in e["results"]] == [None if x is None else x.tokens for x in r["results"]]


def test_a_mel_batch_is_validated_and_uploaded_once(lib):
    """One mel_batch.MelBatch handed to the four wrappers that read a batch's table: each returns exactly what it returns for the
    lists, and the table the first call uploaded is the one the last call read.  Three ragged mels at the micro engine's
    n_mels: an odd row length, no content at all, a few hundred frames."""
    import channels as CH
    from mel_batch import MelBatch
    rng = KR.philox(41)
    n_mels, W, content = 16, 128, [77, 0, 300]
    host = [speechlike(rng, n_mels, F + W, F) for F in content]                  # row lengths 205, 128, 428
    mels = [torch.from_numpy(m).cuda() for m in host]
    sec, chan = S.SectionOptions(max_seconds=30.0), CH.ChannelOptions()
    want_cuts = T.section_cuts(mels, content, sec, window=W)
    want_spans = T.speech_spans(mels, content, OPTS, window=W)
    want_packed, want_frames = T.packed_mels(mels, content, want_spans, W)
    want_tops, want_gated = T.channel_top(mels, content, [1, 1, 1], chan, window=W)
    batch = MelBatch(mels, content)
    assert batch.table is None and len(batch) == 3 and batch.n_mels == n_mels and batch.content_frames == content
    assert T.section_cuts(batch, None, sec, window=W) == want_cuts and len(want_cuts[2]) >= 2
    table = batch.table
    assert table.is_cuda and table.dtype == torch.int64 and table.cpu().tolist() == [[m.data_ptr() for m in mels], [m.shape[1] for m in mels], content]
    spans = T.speech_spans(batch, None, OPTS, window=W)
    assert spans == want_spans == [SP.speech_spans_ref(m, F, *OPTS.frames(W, n_mels)) for m, F in zip(host, content)] and spans[1] == []
    packed, frames = T.packed_mels(batch, None, spans, W)
    assert frames == want_frames and all(torch.equal(a, b) for a, b in zip(packed, want_packed))
    tops, gated = T.channel_top(batch, None, [1, 1, 1], chan, window=W)
    assert gated == want_gated and all(np.array_equal(a, b) for a, b in zip(tops, want_tops))
    assert batch.table is table
    assert all(torch.equal(m, torch.from_numpy(h).cuda()) for m, h in zip(mels, host))
    with pytest.raises(ValueError, match="2 content_frames for 3 mels"):
        MelBatch(mels, content[:2], "speech_spans")
    with pytest.raises(ValueError, match="speech_spans: 999 frames of content in a mel of 128"):
        T.speech_spans(mels, [77, 999, 300], OPTS, window=W)
    with pytest.raises(AssertionError, match="a mel must be a contiguous fp16"):
        T.section_cuts([m.float() for m in mels], content, sec, window=W)


def test_cli_skip_silence_on_flac(lib, engines, golden_dir, capsys):
    import whisper_utils as wu
    dims, eng, enc, mels = engines
    flac = os.path.join(golden_dir, "librispeech_1089-134691-0000.flac")
    seconds = len(wu.load_audio(flac)) / wu.SAMPLE_RATE
    n_frames = len(wu.load_audio(flac)) // wu.HOP_LENGTH
    fs = LF.CHUNK_LENGTH / (2 * dims.n_audio_ctx)
    results = T.main(T.parse_arguments(["--engine_dir", str(eng), "--input_file", flac, "--no_fallback", "--language", "en", "--skip_silence",
                                        "--min_silence_seconds", "20", "--speech_pad_seconds", "2"]))
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[0].startswith("speech: ") and len(results) == 1
    spans = results[0]["speech"]
    print(f"--skip_silence on the LibriSpeech clip ({seconds:.2f} s, {n_frames} frames, micro engine: {fs:.4f} s a frame): {spans}")
    assert spans and all(0 <= a < b <= n_frames * fs + 1e-9 for a, b in spans) and all(b < c for (_, b), (c, _) in zip(spans, spans[1:]))
    assert results[0]["segments"]
