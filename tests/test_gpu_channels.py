"""Channels on the GPU: wm_resample_channels (csrc/resample.hip), wm_channel_top (csrc/channels.hip) and
transcribe(channels=...) end to end.

* wm_resample_channels: row c equals wm_resample of a mono copy of channel c BIT FOR BIT -- float32 / int16 / int32, 1 / 2 / 3 / 8
  channels, 8 / 22.05 / 44.1 / 48 kHz, n_in 1, a few hundred, and the two lengths either side of the first 1024-output tile's end;
  out_ld > n_out with the slack and guard bands untouched; the refusals.
* wm_channel_top against channels.py, exactly: ONE call holding three recordings of 2, 3 and 1 channels; n_mels 1 / 7 / 80; F 0, 1,
  255, 256, 257, 1000; odd ld > F, odd bases; h 0 / 10; planted ties, differences of exactly G and G - 1, NaN and infinities; the
  gate on (the mels equal the host's gated mels, the columns beyond F and the guard bands included) and off (the mels are not
  written); a workspace one frame short reports -1 for the last recording only; the refusals.
* End to end on the micro-fullvocab engine (W = 128 frames, sample_len 12), like with like only: a two-channel and a
  three-channel WAV built here from the committed LibriSpeech clip, noise and silence, at 16 kHz and at 44.1 kHz.  "split":
  result['channels'] equals ONE transcribe() call over the same channels as mono files with the same rows -- alone, with `speech`,
  with `sections`, with `word_timestamps`; `bleed_db` equals transcribe_mel over the host-gated mels; "label": the segments are
  the plain downmix run's and the labels are rule 5 over the device's `top`.  With the option off no new entry is reached and the
  decoder calls are what `_transcribe_files` makes.

Tolerances: none anywhere; every comparison is of integers, of bit patterns, or of results of the same arithmetic.

Measured on MI355X (printed by the tests): at 16 kHz the five channels give 9, 9, 8, 8 and 7 segments, 14 and 20 turns, and `top`
has 2 and 26 runs; `bleed_db` 6 gates 121 and 208 of 417 frames, and 187, 96 and 226 of 312; `label` names channels 0 and 1 in the
two-channel recording and leaves segments of no length without one.  The 36 tests take 4 s.
"""
import copy
import os
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import channels as CH  # noqa: E402
import kernel_refs as KR  # noqa: E402
import longform as LF  # noqa: E402
import native  # noqa: E402
import sections as S  # noqa: E402
import speech as SP  # noqa: E402
import synthetic  # noqa: E402
import transcribe as T  # noqa: E402
import whisper_utils as wu  # noqa: E402
from channels import ChannelOptions  # noqa: E402
from decoding import DecodingOptions, WhisperDecoding  # noqa: E402
from encoding import WhisperEncoding  # noqa: E402
from oracle.whisper_oracle import Dims  # noqa: E402
from test_gpu_model import build_engine  # noqa: E402

GUARD = 32
DTYPE_CODE = {torch.float32: 0, torch.int16: 1, torch.int32: 2}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return native.load_library()


@pytest.fixture(scope="module")
def tmpdir_module(tmp_path_factory):
    return str(tmp_path_factory.mktemp("channels"))


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------ wm_resample_channels
def pcm_of(rng, dtype, n, C):
    if dtype == torch.float32:
        x = rng.standard_normal((n, C)).astype(np.float32)
        x.reshape(-1)[:: 7] *= np.float32(1e-39)                     # subnormals, and a signed zero
        x.reshape(-1)[:: 11] = np.float32(-0.0)
        return x, 1.0
    if dtype == torch.int16:
        return rng.integers(-2 ** 15, 2 ** 15, size=(n, C)).astype(np.int16), 2.0 ** -15
    return rng.integers(-2 ** 23, 2 ** 23, size=(n, C)).astype(np.int32), 2.0 ** -23


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16, torch.int32])
@pytest.mark.parametrize("rate", [8000, 22050, 44100, 48000])
def test_resample_channels_rows_equal_the_mono_kernel(lib, rate, dtype):
    L, M, half, table = wu._device_table(rate, torch.device("cuda", torch.cuda.current_device()))
    edge = 1024 * M // L                                             # the longest input whose outputs fit one tile of 1024
    assert -(-edge * L // M) <= 1024 < -(-(edge + 1) * L // M)
    rng = KR.philox(rate + DTYPE_CODE[dtype])
    for C in (1, 2, 3, 8):
        for n_in in (1, 333, edge, edge + 1):
            host, scale = pcm_of(rng, dtype, n_in, C)
            pcm = torch.from_numpy(host).cuda()
            n_out = -(-n_in * L // M)
            out_ld = n_out + 5
            buf = torch.full((GUARD + C * out_ld + GUARD,), -12345.0, dtype=torch.float32, device="cuda")
            native.check(lib.wm_resample_channels(pcm.data_ptr(), DTYPE_CODE[dtype], C, n_in, scale, table.data_ptr(), L, M, half,
                                                  buf[GUARD:].data_ptr(), out_ld, n_out, stream()), "wm_resample_channels")
            got = buf.cpu().numpy()
            assert (got[:GUARD] == -12345.0).all() and (got[GUARD + C * out_ld:] == -12345.0).all(), "written outside `out`"
            rows = got[GUARD: GUARD + C * out_ld].reshape(C, out_ld)
            assert (rows[:, n_out:] == -12345.0).all(), "the slack behind n_out was written"
            for c in range(C):
                mono = torch.from_numpy(np.ascontiguousarray(host[:, c])).cuda()
                want = torch.empty(n_out, dtype=torch.float32, device="cuda")
                native.check(lib.wm_resample(mono.data_ptr(), DTYPE_CODE[dtype], 1, n_in, scale, table.data_ptr(), L, M, half,
                                             want.data_ptr(), n_out, stream()), "wm_resample")
                assert np.array_equal(rows[c, :n_out].view(np.int32), want.cpu().numpy().view(np.int32)), (rate, dtype, C, n_in, c)
            if n_in == 333:                                          # the wrapper: the same rows, contiguous [C, n_out]
                bits = None if dtype == torch.float32 else (16 if dtype == torch.int16 else 24)
                split = wu.resample_device(pcm, rate, bits, split=True)
                assert tuple(split.shape) == (C, n_out) and np.array_equal(split.cpu().numpy().view(np.int32), rows[:, :n_out].view(np.int32))


def test_resample_channels_bad_arguments(lib):
    L, M, half, table = wu._device_table(44100, torch.device("cuda", torch.cuda.current_device()))
    pcm = torch.zeros((100, 2), dtype=torch.float32, device="cuda")
    n_out = -(-100 * L // M)
    out = torch.zeros(2 * n_out + 8, dtype=torch.float32, device="cuda")

    def call(p=pcm.data_ptr(), dtype=0, channels=2, n_in=100, t=table.data_ptr(), l=L, m=M, hf=half, o=out.data_ptr(), out_ld=n_out, n=n_out):
        return lib.wm_resample_channels(p, dtype, channels, n_in, 1.0, t, l, m, hf, o, out_ld, n, stream())

    assert call() == 0
    for bad in (dict(p=None), dict(t=None), dict(o=None), dict(dtype=3), dict(dtype=-1), dict(channels=0), dict(channels=9), dict(l=0),
                dict(m=0), dict(hf=0), dict(l=M), dict(n_in=0), dict(n=n_out + 1), dict(n=n_out - 1), dict(out_ld=n_out - 1),
                dict(l=1, m=200, n=1)):                                      # (a ratio whose tile does not fit LDS)
        assert call(**bad) == 1, bad
        assert "wm_resample_channels" in lib.wm_last_error().decode(), bad
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ wm_channel_top
def device_channel_top(lib, recordings, n_mels, h, step, total=None):
    """recordings: [(mels: list of fp16 numpy [n_mels, ld], F)].  ONE wm_channel_top call for all of them; returns
    (n_top list, tops: uint8 arrays [F] or None where n_top < 0, counts list, the mels after the call as int16 bit patterns
    [n_mels, ld]) after checking every guard band: around the mels, the tops, n_top, counts and the workspace."""
    flat = [(m, F[c] if isinstance(F, list) else F) for mels, F in recordings for c, m in enumerate(mels)]      # (F: one, or per channel)
    recordings = [(mels, F[0] if isinstance(F, list) else F) for mels, F in recordings]
    n_rec, n_ch = len(recordings), len(flat)
    first = np.concatenate([[0], np.cumsum([len(mels) for mels, _ in recordings])]).astype(np.int32)
    bufs, ptrs = [], []
    for i, (m, _) in enumerate(flat):
        off = GUARD + (i % 2)                                        # odd and even bases
        buf = torch.full((off + m.size + GUARD,), 0x7b7b, dtype=torch.int16, device="cuda")
        buf[off: off + m.size] = torch.from_numpy(np.ascontiguousarray(m).view(np.int16).reshape(-1)).cuda()
        bufs.append((buf, off))
        ptrs.append(buf.data_ptr() + 2 * off)
    tops, tptr = [], []
    for _, F in recordings:
        t = torch.full((GUARD + F + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
        tops.append(t)
        tptr.append(t.data_ptr() + GUARD)
    if total is None:
        total = sum(F for _, F in flat)
    src = torch.tensor(ptrs, dtype=torch.int64, device="cuda")
    ld = torch.tensor([m.shape[1] for m, _ in flat], dtype=torch.int32, device="cuda")
    content = torch.tensor([F for _, F in flat], dtype=torch.int32, device="cuda")
    first_dev = torch.from_numpy(first).cuda()
    top_dev = torch.tensor(tptr, dtype=torch.int64, device="cuda")
    n_top = torch.full((n_rec + GUARD,), -77777, dtype=torch.int32, device="cuda")
    counts = torch.full((n_ch + GUARD,), -77777, dtype=torch.int32, device="cuda")
    ws_bytes = int(lib.wm_channel_top_workspace_bytes(n_ch, total))
    ws = torch.empty(ws_bytes + 64, dtype=torch.uint8, device="cuda")
    ws[ws_bytes:] = 0xA5
    native.check(lib.wm_channel_top(src.data_ptr(), ld.data_ptr(), content.data_ptr(), first_dev.data_ptr(), n_rec, n_ch, n_mels, h, step,
                                    top_dev.data_ptr(), n_top.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws_bytes, total, stream()),
                 "wm_channel_top")
    torch.cuda.synchronize()
    assert bool((ws[ws_bytes:] == 0xA5).all()), "written outside the workspace"
    n, k = n_top.cpu().numpy(), counts.cpu().numpy()
    assert (n[n_rec:] == -77777).all() and (k[n_ch:] == -77777).all(), "written outside n_top / counts"
    got_tops = []
    for (_, F), t, status in zip(recordings, tops, n[:n_rec]):
        host = t.cpu().numpy()
        assert (host[:GUARD] == 0xEE).all() and (host[GUARD + F:] == 0xEE).all(), "written outside a `top`"
        if status < 0:
            assert (host == 0xEE).all(), "a recording that reports -1 was written"
        got_tops.append(host[GUARD: GUARD + F] if status >= 0 else None)
    after = []
    for (m, _), (buf, off) in zip(flat, bufs):
        host = buf.cpu().numpy()
        assert (host[:off] == 0x7b7b).all() and (host[off + m.size:] == 0x7b7b).all(), "written outside a mel"
        after.append(host[off: off + m.size].reshape(m.shape))
    return [int(v) for v in n[:n_rec]], got_tops, [int(v) for v in k[:n_ch]], after


def check_against_contract(lib, recordings, n_mels, h, step):
    n_top, tops, counts, after = device_channel_top(lib, recordings, n_mels, h, step)
    at, wants = 0, []
    for r, (mels, F) in enumerate(recordings):
        top, want_counts, gated = CH.channel_top_ref(mels, F, h, step)
        assert n_top[r] == F and np.array_equal(tops[r], top), (r, F, n_mels, h, step)
        assert counts[at: at + len(mels)] == want_counts, (r, F, counts[at: at + len(mels)], want_counts)
        for c, g in enumerate(gated):
            assert np.array_equal(after[at + c], g.view(np.int16)), (r, c, F, "the mel after the call")
        wants.append((top, want_counts))
        at += len(mels)
    return wants


def odd_ld(F):
    return F + 1 if F % 2 == 0 else F + 2


def recording_of(rng, C, n_mels, F, h, step):
    """C channels of noise with loud stretches, non-finite values, and planted in channels 0 and 1 (where there is room), with
    w = 2h + 3: a tie at frame h + 1, a difference of exactly G at frame 2w and of G - 1 at frame 3w + h + 1."""
    ld = odd_ld(F)
    mels = [(rng.standard_normal((n_mels, ld)) * 0.4 + rng.uniform(-1.5, 0.5)).astype(np.float16) for _ in range(C)]
    for m in mels:
        a = int(rng.integers(0, max(1, F)))
        m[:, a: a + max(1, F // 4)] += np.float16(1.0)
        if F:
            k = min(12, F * n_mels)
            m[rng.integers(0, n_mels, size=k), rng.integers(0, F, size=k)] = np.array(
                [np.nan, np.inf, -np.inf, -0.0, 65504.0, -65504.0], dtype=np.float16)[rng.integers(0, 6, size=k)]
    w = 2 * h + 3
    if C >= 2 and F >= 4 * w and step > 0:
        for m in mels[2:]:
            m[:, : 4 * w] = np.float16(-3.0)                         # far below: channels 0 and 1 decide
        mels[0][:, : 4 * w] = np.float16(0.0)
        mels[1][:, : 4 * w] = np.float16(0.0)                        # frames 0 .. w: a tie (both 0)
        mels[1][:, w: 4 * w] = np.float16(step / 1024)               # every tap `step` above in every bin: exactly G ...
        mels[1][0, 3 * w + h + 1] = np.float16((step - 1) / 1024)    # ... and one bin of one column a step less: G - 1 around it
    return mels


@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("h", [0, 10])
@pytest.mark.parametrize("n_mels", [1, 7, 80])
def test_channel_top_equals_the_contract(lib, n_mels, h, gate):
    sizes = [0, 1, 255, 256, 257, 1000]
    step = 3 if gate else 0
    rng = KR.philox(1000 * n_mels + 10 * h + int(gate))
    gated_total = 0
    for i in range(len(sizes)):
        recordings = [(recording_of(rng, C, n_mels, F, h, 3), F) for C, F in zip((2, 3, 1), (sizes[i], sizes[(i + 1) % 6], sizes[(i + 2) % 6]))]
        wants = check_against_contract(lib, recordings, n_mels, h, step)
        gated_total += sum(sum(c) for _, c in wants)
        assert wants[2][1] == [0] and (wants[2][0] == 0).all()      # one channel: its own channel 0, never gated
        for (mels, F), (top, _) in zip(recordings[:2], wants[:2]):
            w = 2 * h + 3
            if F >= 4 * w:                                           # what was planted is there: the tie goes to channel 0, and G is sharp
                s = CH.smoothed(mels, F, h)
                G = CH.gate_threshold(n_mels, h, 3)
                assert s[1][h + 1] == s[0][h + 1] and top[h + 1] == 0
                assert s[1][2 * w] - s[0][2 * w] == G and top[2 * w] == 1
                assert s[1][3 * w + h + 1] - s[0][3 * w + h + 1] == G - 1 and top[3 * w + h + 1] == 1
                flags = CH.gated_frames(s, G)
                assert flags[0][2 * w] and not flags[0][3 * w + h + 1] and not flags[1][: 3 * w].any()
    assert (gated_total > 0) == gate


def test_channel_top_G_and_G_minus_1(lib):
    """h = 0, one planted bin: a difference of exactly G gates, G - 1 does not; equal channels tie to the lowest."""
    n_mels, F, step = 7, 300, 100
    G = CH.gate_threshold(n_mels, 0, step)
    a = np.zeros((n_mels, F + 1), dtype=np.float16)
    b = np.zeros((n_mels, F + 1), dtype=np.float16)
    b[:, 10] = np.float16(step / 1024)                               # G
    b[:, 20] = np.float16(step / 1024)
    b[0, 20] = np.float16((step - 1) / 1024)                         # G - 1
    a[:, 30] = np.float16(-1.0)
    (top, counts), = check_against_contract(lib, [([a, b], F)], n_mels, 0, step)
    s = CH.smoothed([a, b], F, 0)
    assert s[1][10] - s[0][10] == G and s[1][20] - s[0][20] == G - 1
    assert counts == [2, 0] and top[10] == 1 and top[20] == 1 and top[30] == 1 and top[0] == 0 and int(top.sum()) == 3


def test_a_workspace_one_frame_short(lib):
    rng = KR.philox(77)
    recordings = [(recording_of(rng, C, 7, F, 3, 3), F) for C, F in ((2, 300), (3, 257), (1, 100))]
    total = 2 * 300 + 3 * 257 + 100
    n_top, tops, counts, after = device_channel_top(lib, recordings, 7, 3, 3, total=total - 1)
    assert n_top == [300, 257, -1] and tops[2] is None and counts[5] == 0
    for r in range(2):
        assert np.array_equal(tops[r], CH.channel_top_ref(recordings[r][0], recordings[r][1], 3, 3)[0])
    assert np.array_equal(after[5], recordings[2][0][0].view(np.int16))
    n_top, _, _, _ = device_channel_top(lib, recordings, 7, 3, 3, total=total)
    assert n_top == [300, 257, 100]
    # channels of one recording that differ in content: -1 for that recording only, and nothing of it is written
    uneven = [(recordings[0][0], [300, 299]), recordings[1], recordings[2]]
    n_top, tops, counts, after = device_channel_top(lib, uneven, 7, 3, 3)
    assert n_top == [-1, 257, 100] and counts[:2] == [0, 0]
    assert all(np.array_equal(after[c], recordings[0][0][c].view(np.int16)) for c in range(2))
    assert np.array_equal(tops[2], np.zeros(100, dtype=np.uint8)) and np.array_equal(tops[1], CH.channel_top_ref(*recordings[1], 3, 3)[0])


def test_channel_top_bad_arguments(lib):
    z = torch.zeros(64, dtype=torch.int64, device="cuda")           # a null channel of no frames; first = [0, 0, ...]
    o = torch.zeros(256, dtype=torch.int32, device="cuda")
    ws_bytes = int(lib.wm_channel_top_workspace_bytes(1, 100))
    assert ws_bytes >= 16 + 2 * 400 + 4 and lib.wm_channel_top_workspace_bytes(0, 100) == 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    first = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    p, q = z.data_ptr(), o.data_ptr()

    def call(src=p, ld=p, content=p, fst=first.data_ptr(), n_rec=1, n_ch=1, n_mels=80, h=3, step=205, top=p, n_top=q, counts=q + 64,
             w=ws.data_ptr(), wb=ws_bytes, total=100):
        return lib.wm_channel_top(src, ld, content, fst, n_rec, n_ch, n_mels, h, step, top, n_top, counts, w, wb, total, stream())

    assert call() == 0 and call(step=0) == 0
    for bad in (dict(src=None), dict(ld=None), dict(content=None), dict(fst=None), dict(top=None), dict(n_top=None), dict(counts=None),
                dict(w=None), dict(n_rec=0), dict(n_ch=0), dict(n_mels=0), dict(step=-1), dict(step=32769), dict(h=-1), dict(h=819),
                dict(wb=ws_bytes - 1), dict(total=200), dict(total=-1), dict(n_top=q + 2), dict(counts=q + 1)):
        assert call(**bad) == 1, bad
        assert "wm_channel_top" in lib.wm_last_error().decode(), bad
    assert call(h=818, step=32768) == 0
    torch.cuda.synchronize()
    assert int(o[0]) == 0                                            # the null channel: a recording without frames


def test_wrapper_one_call_for_all_recordings(lib):
    rng = KR.philox(5)
    recordings = [(recording_of(rng, C, 80, F, 0, 3), F) for C, F in ((2, 500), (1, 0), (3, 257))]
    host = [m for mels, _ in recordings for m in mels]
    content = [F for mels, F in recordings for _ in mels]
    mels = [torch.from_numpy(m).cuda() for m in host]
    opts = ChannelOptions(bleed_db=3 * 40 / 1024, smooth_seconds=0.0)
    assert opts.frames(128, 80) == (0, 3)
    tops, gated = T.channel_top(mels, content, [2, 1, 3], opts, window=128)
    at = 0
    for r, (ms, F) in enumerate(recordings):
        top, counts, after = CH.channel_top_ref(ms, F, 0, 3)
        assert tops[r].dtype == np.uint8 and np.array_equal(tops[r], top) and gated[at: at + len(ms)] == counts
        for c, g in enumerate(after):
            assert np.array_equal(mels[at + c].cpu().numpy().view(np.int16), g.view(np.int16))
        at += len(ms)
    assert sum(gated) > 0 and T.channel_top([], [], [], opts) == ([], [])
    with pytest.raises(ValueError):
        T.channel_top(mels, content, [2, 2, 2], opts, window=128)           # the second "recording" would mix shapes
    with pytest.raises(ValueError):
        T.channel_top(mels, content, [2, 1], opts, window=128)
    with pytest.raises(ValueError):
        T.channel_top(mels[:1] * 9, content[:1] * 9, [9], opts, window=128)


# --------------------------------------------------------------------------------------------------------------- end to end
N_ROWS = 3
KW = dict(temperatures=(0.0,), compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None)
OPTS = SP.SpeechOptions(min_silence_seconds=5.0, min_speech_seconds=1.0, speech_pad_seconds=2.0)       # at W = 128: 21, 4, 9 frames


def write_wav(path, pcm, rate):
    """PCM16 RIFF/WAVE: pcm int16 [n, C]."""
    pcm = np.ascontiguousarray(pcm.astype("<i2"))
    n, C = pcm.shape
    body = pcm.tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, C, rate, rate * C * 2, C * 2, 16)
                + b"data" + struct.pack("<I", len(body)) + body)
    return str(path)


@pytest.fixture(scope="module")
def material(tmpdir_module, golden_dir):
    """{rate: (paths of the two recordings, [paths of their channels as mono files])} and the engine."""
    clip = wu.load_pcm(os.path.join(golden_dir, "librispeech_1089-134691-0000.flac"))[0][:, 0].astype(np.int64)
    n = len(clip)                                                     # (two seconds of speech)
    assert n >= 32000
    rng = KR.philox(2024)
    noise = lambda k, a: rng.integers(-a, a + 1, size=k)              # noqa: E731
    z = lambda k: np.zeros(k, dtype=np.int64)                         # noqa: E731
    # two parties who speak in turn, the second line digitally silent while it listens; then speech, noise, and late speech that overlaps
    two = np.stack([np.concatenate([clip, z(n)]) + noise(2 * n, 20), np.concatenate([z(n), clip])], axis=1)
    m = 50000
    three = np.stack([np.concatenate([clip, clip])[:m], noise(m, 300), np.concatenate([z(12000), clip, z(m)])[:m] + noise(m, 10)], axis=1)
    out = {}
    for rate in (16000, 44100):
        files, monos = [], []
        for name, rec in (("two", two), ("three", three)):
            rec = np.clip(rec, -32768, 32767).astype(np.int16)
            files.append(write_wav(os.path.join(tmpdir_module, f"{name}_{rate}.wav"), rec, rate))
            monos += [write_wav(os.path.join(tmpdir_module, f"{name}_{rate}_ch{c}.wav"), rec[:, c:c + 1], rate) for c in range(rec.shape[1])]
        out[rate] = (files, monos)
    dims = Dims(**synthetic.DIMS["micro-fullvocab"])
    eng = build_engine(tmpdir_module, "micro-fullvocab", 3)
    return dims, eng, WhisperEncoding(eng), out


def decoder(eng, **kw):
    dec = WhisperDecoding(eng, options=DecodingOptions(language="en"), **kw)
    dec.sample_len = 12
    return dec


def check_split(result, parts, top_ref=None):
    """One recording's result against its channels' results as mono files, and the merge against rule 6."""
    assert result["channels"] == parts
    want = CH.merge_channels(parts)
    for key in ("segments", "turns", "text", "language"):
        assert result[key] == want[key], key
    assert all(s["channel"] in range(len(parts)) for s in result["segments"])
    assert [(s["start"], s["end"], s["channel"]) for s in result["segments"]] == sorted((s["start"], s["end"], s["channel"]) for s in result["segments"])
    if top_ref is not None:
        assert result["channel_top"] == CH.run_lengths(top_ref)


def host_tops(files, h):
    """Rule 3 on the host over the channel mels the front end makes of the files."""
    tops = []
    for f in files:
        wave = wu.load_audio_device(f, channels="split")
        mels, F = [], None
        for c in range(wave.shape[0]):
            mel, F = wu.long_log_mel_device(wave[c].contiguous())
            mels.append(mel.cpu().numpy())
        tops.append(CH.channel_top_ref(mels, F, h, 0)[0])
    return tops


@pytest.mark.parametrize("rate", [16000, 44100])
def test_split_equals_the_channels_as_mono_files(lib, material, rate):
    dims, eng, enc, out = material
    files, monos = out[rate]
    W = 2 * dims.n_audio_ctx
    dec = decoder(eng)
    h, _ = ChannelOptions().frames(W, dims.n_mels)
    tops = host_tops(files, h)
    for extra in (dict(), dict(speech=OPTS), dict(sections=S.SectionOptions(max_seconds=30.0)), dict(word_timestamps=True)):
        trace, ref_trace = [], []
        results = T.transcribe(enc, dec, files, channels=ChannelOptions(), n_rows=N_ROWS, trace=trace, **extra, **KW)
        reference = T.transcribe(enc, dec, monos, n_rows=N_ROWS, trace=ref_trace, **extra, **KW)
        assert len(results) == 2 and len(reference) == 5 and len(trace) == len(ref_trace)
        check_split(results[0], reference[:2], tops[0])
        check_split(results[1], reference[2:], tops[1])
        assert results[0]["channel_gated"] == [0, 0] and results[1]["channel_gated"] == [0, 0, 0]
        for e, r in zip(trace, ref_trace):
            assert e["rows"] == r["rows"] and e.get("kind") == r.get("kind")
        if "speech" in extra:
            assert all("speech" in p for res in results for p in res["channels"])
        if "sections" in extra:
            assert all("sections" in p for res in results for p in res["channels"])
        if "word_timestamps" in extra:
            assert sum(len(s["words"]) for res in results for s in res["segments"]) > 0
        if not extra:
            n_seg = [len(p["segments"]) for res in results for p in res["channels"]]
            print(f"split at {rate} Hz: segments per channel {n_seg}; turns {[len(r['turns']) for r in results]}; "
                  f"top runs {[len(r['channel_top']) for r in results]}")
            assert sum(n_seg) > 0 and any(len(set(s["channel"] for s in r["segments"])) > 1 for r in results)
    # a one-channel file under the option is its own channel 0
    one = T.transcribe(enc, dec, monos[:1], channels=ChannelOptions(), n_rows=N_ROWS, **KW)[0]
    plain = T.transcribe(enc, dec, monos[:1], n_rows=N_ROWS, **KW)
    assert one["channels"] == plain and all(s["channel"] == 0 for s in one["segments"]) and [c for c, _ in one["channel_top"]] == [0]


def test_bleed_db_equals_the_host_gated_mels(lib, material):
    dims, eng, enc, out = material
    files, _ = out[16000]
    W = 2 * dims.n_audio_ctx
    dec = decoder(eng)
    mels, content, counts = [], [], []
    for f in files:
        wave = wu.load_audio_device(f, channels="split")
        for c in range(wave.shape[0]):
            mel, F = wu.long_log_mel_device(wave[c].contiguous())
            mels.append(mel)
            content.append(F)
        counts.append(int(wave.shape[0]))
    opts = ChannelOptions(bleed_db=6.0)
    h, step = opts.frames(W, dims.n_mels)
    before = [m.clone() for m in mels]
    host, at, gated_mels, want_counts, tops = [m.cpu().numpy() for m in mels], 0, [], [], []
    for C in counts:
        top, k, g = CH.channel_top_ref(host[at: at + C], content[at], h, step)
        gated_mels += [torch.from_numpy(x).cuda() for x in g]
        want_counts.append(k)
        tops.append(top)
        at += C
    results = T.transcribe_mel(enc, dec, mels, content, channels=opts, channel_counts=counts, n_rows=N_ROWS, **KW)
    reference = T.transcribe_mel(enc, dec, gated_mels, content, n_rows=N_ROWS, **KW)
    assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(mels, before)), "the caller's mels were written"
    check_split(results[0], reference[:2], tops[0])
    check_split(results[1], reference[2:], tops[1])
    assert [r["channel_gated"] for r in results] == want_counts
    print(f"bleed_db 6: gated frames per channel {want_counts} of {content[0]} and {content[2]}")
    assert sum(want_counts[0]) > 0 and sum(want_counts[1]) > 0
    # through files the same gate runs (the same mels: the front end is deterministic)
    assert T.transcribe(enc, dec, files, channels=opts, n_rows=N_ROWS, **KW) == results


@pytest.mark.parametrize("rate", [16000, 44100])
def test_label_names_the_loudest_channel_of_the_downmix_run(lib, material, rate):
    dims, eng, enc, out = material
    files, _ = out[rate]
    W = 2 * dims.n_audio_ctx
    fs = LF.CHUNK_LENGTH / W
    dec = decoder(eng)
    opts = ChannelOptions(mode="label")
    tops = host_tops(files, opts.frames(W, dims.n_mels)[0])
    for extra in (dict(), dict(word_timestamps=True), dict(speech=OPTS)):
        plain = T.transcribe(enc, dec, files, n_rows=N_ROWS, **extra, **KW)
        results = T.transcribe(enc, dec, files, channels=opts, n_rows=N_ROWS, **extra, **KW)
        labels = []
        for res, ref, top, C in zip(results, plain, tops, (2, 3)):
            assert res["channel_top"] == CH.run_lengths(top) and np.array_equal(CH.from_run_lengths(res["channel_top"]), top)
            stripped = copy.deepcopy(res["segments"])
            for s in stripped:
                assert s.pop("channel") == CH.label_span(top, s["start"], s["end"], fs, C)
                for w in s.get("words", ()):
                    assert w.pop("channel") == CH.label_span(top, w["start"], w["end"], fs, C)
            assert stripped == ref["segments"] and res["text"] == ref["text"] and res["language"] == ref["language"]
            assert ("speech" in res) == ("speech" in extra) and "channels" not in res
            labels.append([s["channel"] for s in res["segments"]])
        if not extra:
            print(f"label at {rate} Hz: {labels}")
            if rate == 16000:                # (the two-channel recording speaks on channel 0 in its first half, on 1 in its second)
                assert len(set(labels[0])) > 1, "every segment got the same channel"


def test_with_the_option_off_nothing_new_runs(lib, material, monkeypatch):
    dims, eng, enc, out = material
    files, monos = out[44100]
    dec = decoder(eng)
    reached = []
    for name in ("wm_channel_top", "wm_channel_top_workspace_bytes", "wm_resample_channels"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _n=name, _f=real: (reached.append(_n), _f(*a))[1])
    a, b = [], []
    one = T.transcribe(enc, dec, files + monos, n_rows=N_ROWS, trace=a, **KW)
    assert reached == []
    mels, content = [], []
    for f in files + monos:
        mel, F = wu.long_log_mel_device(wu.load_audio_device(f))
        mels.append(mel)
        content.append(F)
    two = T._transcribe_files(enc, dec, mels, content, None, n_rows=N_ROWS, trace=b, condition_on_previous_text=False,
                              initial_prompt=None, word_timestamps=False, **KW)
    assert one == two and len(a) == len(b) and all("channels" not in r and "channel_top" not in r for r in one)
    assert all("channel" not in s for r in one for s in r["segments"])
    for e, r in zip(a, b):
        assert e["rows"] == r["rows"] and e["live"] == r["live"] and torch.equal(e["windows"], r["windows"])
    assert reached == []
    T.transcribe(enc, dec, files[:1], channels=ChannelOptions(), n_rows=N_ROWS, **KW)
    assert reached.count("wm_channel_top") == 1 and reached.count("wm_resample_channels") == 1       # one call each for the recording


def test_cli_prints_the_channel(lib, material, capsys):
    dims, eng, enc, out = material
    files, _ = out[16000]
    results = T.main(T.parse_arguments(["--engine_dir", str(eng), "--input_file", files[0], "--no_fallback", "--language", "en",
                                        "--channels", "split"]))
    lines = [x for x in capsys.readouterr().out.strip().splitlines() if x.startswith("[")]
    spoken = [s for s in results[0]["segments"] if s["text"].strip()]
    assert len(lines) == len(spoken) > 0
    for line, s in zip(lines, spoken):
        assert line == f"[{T.format_timestamp(s['start'])} --> {T.format_timestamp(s['end'])}] ch{s['channel']}: {s['text'].strip()}"
    with pytest.raises(ValueError):
        T.main(T.parse_arguments(["--engine_dir", str(eng), "--input_file", files[0], "--channels", "label", "--bleed_db", "6"]))
