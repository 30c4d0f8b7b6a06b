"""wm_resample (csrc/resample.hip) through the C ABI, the host path over it (resample_device, load_audio_device, load_audio) and
transcription of files at foreign rates end to end.

The oracle is tests/resample_refs.py (h from the formula at exact integer time, fp64); "within the bound" is
|y - oracle| <= (T + 4) 2^-24 S per output, S = sum |h x| (derivation: resample_refs' docstring).  The table handed to the entry
is built HERE from resample_filter's H in the layout the header documents, table[j][r] = H[(r M) mod L][j].

* exact: unit impulses (fp32, mono, scale 1) -- every output is one table entry bit for bit, or exactly 0 out of reach;
* noise: six rates x {f32, i16, i32 holding 24-bit values, i32 full range} x {1, 2, 3 channels} x n_in in {1, 2, half - 1, 5000,
  44101}: inputs shorter than one filter half, a single sample, ragged last tiles; guard bands around the output stay untouched;
* int64: 13.6 M samples at 44.1 kHz, n M crosses 2^31 inside the output; 4096 outputs around the crossing and the last 4096;
* determinism, rejections, the host path, transcribe() on a 44.1 kHz stereo FLAC, run.load_mel on a 48 kHz WAV.
"""
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import native  # noqa: E402
import resample_refs as RR  # noqa: E402
import whisper_utils as wu  # noqa: E402

GUARD = 256
SENTINEL = -12345.0
DTYPE_CODE = {torch.float32: 0, torch.int16: 1, torch.int32: 2}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return native.load_library()


_TABLES = {}


def device_table(rate):
    if rate not in _TABLES:
        L, M, half, H = wu.resample_filter(rate)
        order = (np.arange(L, dtype=np.int64) * M) % L
        _TABLES[rate] = (L, M, half, H, torch.from_numpy(np.ascontiguousarray(H[order].T)).cuda())
    return _TABLES[rate]


def run(lib, pcm, rate, scale):
    """pcm: torch [n_in, C] on the GPU -> numpy fp32 [n_out]; the words either side of the output must keep their sentinel."""
    L, M, half, H, table = device_table(rate)
    n_in, ch = pcm.shape
    n_out = -(-n_in * L // M)
    buf = torch.full((GUARD + n_out + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    out = buf[GUARD:GUARD + n_out]
    native.check(lib.wm_resample(pcm.data_ptr(), DTYPE_CODE[pcm.dtype], ch, n_in, scale, table.data_ptr(), L, M, half,
                                 out.data_ptr(), n_out, torch.cuda.current_stream().cuda_stream), "wm_resample")
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + n_out:] == SENTINEL).all(), "written outside the output"
    return got[GUARD:GUARD + n_out]


# ------------------------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("rate", RR.RATES)
def test_impulses_give_the_table_bit_for_bit(lib, rate):
    L, M, half, H, _ = device_table(rate)
    T = 2 * half + 1
    n_in = 4001
    where = [0, 1000, 1777, 2900, n_in - 1]
    assert all(b - a > T for a, b in zip(where, where[1:]))
    x = np.zeros((n_in, 1), dtype=np.float32)
    x[where] = 1.0
    got = run(lib, torch.from_numpy(x).cuda(), rate, 1.0)
    n = np.arange(len(got), dtype=np.int64)
    i, p = n * M // L, n * M % L
    want = np.zeros(len(got), dtype=np.float32)
    hit = np.zeros(len(got), dtype=np.int64)
    for k in where:
        j = k - i + half
        ok = (j >= 0) & (j < T)
        want[ok] = H[p[ok], j[ok]]
        hit += ok
    assert hit.max() == 1 and (hit == 0).any() and hit.sum() >= 3 * ((T - 1) * L // M)      # the interior impulses are reached from both sides
    assert np.array_equal(got.view(np.int32)[hit == 1], want.view(np.int32)[hit == 1])
    assert not got[hit == 0].any()


# ------------------------------------------------------------------------------------------------------------------ noise
def variants(rng, n_in):
    """(label, samples [n_in, C] as numpy, bits or None) of the twelve dtype x channel combinations."""
    out = []
    for ch in (1, 2, 3):
        out.append((f"f32 x{ch}", rng.standard_normal((n_in, ch)).astype(np.float32), None))
        out.append((f"i16 x{ch}", rng.integers(-32768, 32768, size=(n_in, ch), dtype=np.int64).astype(np.int16), 16))
        out.append((f"i32/24 x{ch}", rng.integers(-(1 << 23), 1 << 23, size=(n_in, ch), dtype=np.int64).astype(np.int32), 24))
        out.append((f"i32/32 x{ch}", rng.integers(-(1 << 31), 1 << 31, size=(n_in, ch), dtype=np.int64).astype(np.int32), 32))
    return out


@pytest.mark.parametrize("n_in", [1, 2, "half-1", 5000, 44101])
@pytest.mark.parametrize("rate", RR.RATES)
def test_noise_within_the_bound(lib, rate, n_in):
    n_in = RR.params(rate)[3] - 1 if n_in == "half-1" else n_in
    rng = np.random.Generator(np.random.Philox(rate * 7 + n_in))
    cases = variants(rng, n_in)
    want, S = RR.oracle(np.stack([RR.mono64(s, bits) for _, s, bits in cases], axis=1), rate)
    worst = 0.0
    for v, (label, s, bits) in enumerate(cases):
        got = run(lib, torch.from_numpy(s).cuda(), rate, 1.0 if bits is None else 2.0 ** -(bits - 1))
        assert got.shape == want[:, v].shape, label
        err, lim = np.abs(got - want[:, v]), RR.bound(S[:, v], rate)
        worst = max(worst, float((err / np.maximum(lim, 1e-300)).max()))
        assert (err <= lim).all(), (label, float((err / np.maximum(lim, 1e-300)).max()))
    print(f"resample {rate} Hz, n_in {n_in}: worst error / bound = {worst:.3f}")


def test_int64_indices(lib):
    rate, n_in = 44100, 13_600_000
    L, M, fc, half, T = RR.params(rate)
    g = torch.Generator(device="cuda")
    g.manual_seed(2 ** 31)
    x = torch.randn((n_in, 1), generator=g, device="cuda", dtype=torch.float32)
    got = run(lib, x, rate, 1.0)
    n_out = len(got)
    cross = (1 << 31) // M
    assert 2048 < cross < n_out - 8192 and (n_out - 1) * M > 1 << 31
    for n in (np.arange(cross - 2048, cross + 2048, dtype=np.int64), np.arange(n_out - 4096, n_out, dtype=np.int64)):
        lo = max(0, int(n[0] * M // L) - half - 2)
        hi = min(n_in, int(n[-1] * M // L) + half + 3)
        want, S = RR.oracle(x[lo:hi, 0].cpu().numpy(), rate, n=n, n_in=n_in, x0=lo)
        err, lim = np.abs(got[n] - want), RR.bound(S, rate)
        print(f"int64 path, outputs {n[0]}..{n[-1]}: worst error / bound = {float((err / lim).max()):.3f}")
        assert S.min() > 0 and (err <= lim).all()


def test_two_runs_are_bitwise_equal(lib):
    rng = np.random.Generator(np.random.Philox(11))
    s = torch.from_numpy(rng.integers(-32768, 32768, size=(44101, 2), dtype=np.int64).astype(np.int16)).cuda()
    a, b = run(lib, s, 44100, 2.0 ** -15), run(lib, s, 44100, 2.0 ** -15)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_bad_arguments(lib):
    L, M, half, H, table = device_table(44100)
    n_in = 1000
    n_out = -(-n_in * L // M)
    x = torch.zeros((n_in, 8), dtype=torch.float32, device="cuda")
    out = torch.full((n_out + 8,), SENTINEL, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    good = dict(pcm=x.data_ptr(), dtype=0, channels=1, n_in=n_in, scale=1.0, table=table.data_ptr(), L=L, M=M, half=half,
                out=out.data_ptr(), n_out=n_out)
    bad = [dict(pcm=None), dict(table=None), dict(out=None), dict(channels=0), dict(channels=9), dict(channels=-1), dict(dtype=3),
           dict(dtype=-1), dict(M=L), dict(L=0), dict(L=-1), dict(M=0), dict(half=0), dict(half=-5), dict(n_out=n_out + 1),
           dict(n_out=n_out - 1), dict(n_out=0), dict(n_in=0, n_out=0), dict(n_in=-1, n_out=0)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.wm_resample(a["pcm"], a["dtype"], a["channels"], a["n_in"], a["scale"], a["table"], a["L"], a["M"], a["half"],
                             a["out"], a["n_out"], s)
        assert rc == 1, change
        assert b"wm_resample" in lib.wm_last_error()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all(), "a rejected call wrote to the output"
    assert lib.wm_resample(*[good[k] for k in ("pcm", "dtype", "channels", "n_in", "scale", "table", "L", "M", "half", "out", "n_out")], s) == 0
    torch.cuda.synchronize()
    assert not out[:n_out].any() and (out[n_out:] == SENTINEL).all()


# -------------------------------------------------------------------------------------------------------------- host path
def noise16(seed, n, ch, amplitude=8000):
    rng = np.random.Generator(np.random.Philox(seed))
    return np.clip(np.rint(rng.standard_normal((n, ch)) * amplitude), -32767, 32767).astype(np.int32)


def test_load_audio_device(lib, tmp_path):
    for ch in (1, 2):
        s = noise16(20 + ch, 9001, ch)
        path = tmp_path / f"k16_{ch}.flac"
        path.write_bytes(RR.quick_flac(s, 16000))
        host = wu.load_audio(str(path))
        dev = wu.load_audio_device(str(path))
        assert dev.is_cuda and dev.dtype == torch.float32 and np.array_equal(dev.cpu().numpy().view(np.int32), host.view(np.int32))
        assert np.array_equal(host, (s.astype(np.float32).mean(axis=1) / 32768.0).astype(np.float32))
    s = noise16(23, 30011, 2)
    path = tmp_path / "k44.flac"
    path.write_bytes(RR.quick_flac(s, 44100))
    dev = wu.load_audio_device(str(path))
    want, S = RR.oracle(RR.mono64(s, 16), 44100)
    assert dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == want.shape
    err = np.abs(dev.cpu().numpy() - want)
    assert (err <= RR.bound(S, 44100)).all()
    host = wu.load_audio(str(path))
    assert host.dtype == np.float32 and np.array_equal(host.view(np.int32), dev.cpu().numpy().view(np.int32))
    # resample_device takes what load_pcm returns, and a 1-D tensor as one channel
    pcm, rate, bits = wu.load_pcm(str(path))
    again = wu.resample_device(torch.from_numpy(pcm).cuda(), rate, bits)
    assert torch.equal(again, dev)
    mono = torch.from_numpy(pcm[:, 0].copy()).cuda()
    assert torch.equal(wu.resample_device(mono, rate, bits), wu.resample_device(mono[:, None], rate, bits))
    with pytest.raises(ValueError, match="16000"):
        wu.resample_device(mono, 16000, bits)


# -------------------------------------------------------------------------------------------------------------- end to end
def test_transcribe_and_run_take_foreign_rates(lib, tmp_path, capsys):
    import run as R
    import transcribe as T
    from decoding import DecodingOptions, WhisperDecoding
    from encoding import WhisperEncoding
    from test_gpu_model import build_engine

    eng = build_engine(str(tmp_path), "micro-fullvocab", 3)
    enc = WhisperEncoding(eng)
    dec = WhisperDecoding(eng, options=DecodingOptions(language="en"))
    dec.sample_len = 12
    n = 35 * 44100 + 17
    t = np.arange(n) / 44100.0
    tone = 6000 * np.sin(2 * np.pi * (300 + 40 * t) * t)
    s = noise16(31, n, 2, amplitude=1500) + np.rint(np.stack([tone, 0.5 * tone], axis=1)).astype(np.int32)
    path = tmp_path / "long_44k1_stereo.flac"
    path.write_bytes(RR.quick_flac(s, 44100))
    kw = dict(temperatures=(0.0,), compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None, n_rows=1)
    audio = wu.load_audio_device(str(path))
    assert tuple(audio.shape) == (-(-n * 160 // 441),)
    from_path = T.transcribe(enc, dec, [str(path)], **kw)
    from_audio = T.transcribe(enc, dec, [audio], **kw)
    assert len(from_path) == 1 and from_path[0]["segments"] and from_path[0]["segments"] == from_audio[0]["segments"]
    assert len({seg["seek"] for seg in from_path[0]["segments"]}) >= 2                       # more than one window

    # the CLI on a 48 kHz stereo FLAC prints segments
    short = tmp_path / "short_48k_stereo.flac"
    short.write_bytes(RR.quick_flac(s[:3 * 48000], 48000))
    capsys.readouterr()
    results = T.main(T.parse_arguments(["--engine_dir", str(eng), "--input_file", str(short), "--no_fallback", "--language", "en"]))
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("[")]
    assert results[0]["segments"] and len(lines) == sum(1 for seg in results[0]["segments"] if seg["text"].strip())

    # run.py's front end on a 48 kHz WAV
    wav = tmp_path / "a48.wav"
    with wave.open(str(wav), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(48000); w.writeframes(s[:48000].astype(np.int16).tobytes())
    mel = R.load_mel(str(wav))
    assert tuple(mel.shape) == (80, 3000) and bool(torch.isfinite(mel).all())
    assert R.real_mel_frames(str(wav)) == 100
