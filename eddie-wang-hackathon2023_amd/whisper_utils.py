"""Audio front-end: PCM loading, resampling, pad/trim, log-mel spectrogram.  Mirror of W/whisper_utils.py:17-146
(`load_audio`, `pad_or_trim`, `mel_filters`, `log_mel_spectrogram`, same constants).

Differences: the reference pipes every file through `ffmpeg -ar 16000 -ac 1` (absent here).  `load_audio` reads `.wav` (own
RIFF reader: PCM 8 / 16 / 24 / 32 bit, IEEE float32, WAVE_FORMAT_EXTENSIBLE), `.flac` (own decoder) and `.npy` waveforms; a file
at another rate than 16 kHz is resampled by a polyphase Kaiser-windowed sinc filter -- `resample_filter` / `resample_reference`
state it on the host in fp64, `resample_device` runs it on the GPU (wm_resample, csrc/resample.hip: downmix, conversion and filter
in one launch).  The filter is this project's design, not swresample's: outputs differ from ffmpeg's in the last bits and in the
transition band.  The 80x201 mel filterbank is regenerated with the recipe the reference quotes
(`librosa.filters.mel(sr=16000, n_fft=400, n_mels=80)`, W/whisper_utils.py:85-90: Slaney scale, Slaney area normalisation)
instead of shipping the `.npz`; tests/golden/mel.npz (made with the reference's own function and asset) pins both.  The same
recipe with n_mels=128 gives the 128x201 bank of large-v3 and after (upstream's `mel_128`); `mel_filters` takes 80 or 128 and
every caller passes its engine's `num_mels`.  The STFT of
`log_mel_spectrogram` runs through torch on whatever device the audio is on; `log_mel_spectrogram_device` is the HIP kernel.
"""
from __future__ import annotations

import math
import struct
from functools import lru_cache
from typing import Optional, Union

import numpy as np
import torch
import torch.nn.functional as F

SAMPLE_RATE = 16000
N_FFT = 400
N_MELS = 80
HOP_LENGTH = 160
CHUNK_LENGTH = 30
N_SAMPLES = CHUNK_LENGTH * SAMPLE_RATE  # 480000 samples in a 30-second chunk
N_FRAMES = N_SAMPLES // HOP_LENGTH       # 3000 frames in a mel spectrogram input


def decode_flac(data: bytes, verify_md5: bool = True):
    """FLAC bytes -> (int32 samples [n, channels], sample_rate, bits_per_sample) through the native decoder
    (wm_flac_decode, csrc/flac_decode.hip; frame CRCs checked there).  With `verify_md5` the decoded PCM is
    hashed and compared with the stream's own STREAMINFO signature (skipped when the encoder left it zero)."""
    import ctypes as C
    import hashlib
    import native
    lib = native.load_library()
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    info = native.WmFlacStreamInfo()
    native.check(lib.wm_flac_info(buf, len(data), C.byref(info)), "wm_flac_info")
    capacity = int(info.total_samples)
    if capacity == 0:      # unknown length: every frame holds at most max_block_size samples and at least 11 bytes
        capacity = (len(data) // 11 + 1) * max(int(info.max_block_size), 16)
    pcm = np.empty((capacity, info.channels), dtype=np.int32)
    n = C.c_int64(0)
    native.check(lib.wm_flac_decode(buf, len(data), pcm.ctypes.data, capacity, C.byref(n)), "wm_flac_decode")
    pcm = pcm[: n.value]
    signature = bytes(info.md5)
    if verify_md5 and any(signature):
        width = (info.bits_per_sample + 7) // 8
        raw = pcm.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :width].tobytes()
        if hashlib.md5(raw).digest() != signature:
            raise RuntimeError("FLAC MD5 signature mismatch: decoded audio differs from what the encoder saw")
    return pcm, int(info.sample_rate), int(info.bits_per_sample)


# ------------------------------------------------------------------------------------------------------------ resampling
# The contract (fp64), for an input rate `rate` and sr = 16000:  g = gcd(rate, sr), L = sr / g, M = rate / g;
#   fc = 0.9 * min(1, L / M)     cut-off as a fraction of the input Nyquist
#   half = ceil(32 / fc)         input samples each side: 32 zero crossings of the sinc
#   h(t) = fc * sinc(fc t) * I0(11 sqrt(1 - (t / half)^2)) / I0(11)   for |t| <= half, 0 outside   (Kaiser window, beta 11)
#   y[n] = sum_k x[k] h(n M / L - k),  x zero outside [0, n_in),  n_out = ceil(n_in L / M):  no delay, output n sits at input time n M / L.
# As a table, with i = floor(n M / L), p = (n M) mod L:  taps j = 0 .. T - 1, T = 2 half + 1, tap j reads x[i - half + j] and its
# coefficient is H[p][j] = fp32(h(p / L + half - j)).
RESAMPLE_MIN_RATE, RESAMPLE_MAX_RATE = 4000, 192000
RESAMPLE_KAISER_BETA = 11.0
RESAMPLE_ZERO_CROSSINGS = 32
RESAMPLE_ROLLOFF = 0.9
RESAMPLE_MAX_TABLE_BYTES = 16 << 20


def _check_rate(rate, sr: int):
    if isinstance(rate, bool) or not isinstance(rate, (int, np.integer)):
        raise ValueError(f"cannot resample from {rate!r} Hz: the rate must be an integer")
    rate = int(rate)
    if not RESAMPLE_MIN_RATE <= rate <= RESAMPLE_MAX_RATE or rate == sr:
        raise ValueError(f"cannot resample from {rate} Hz to {sr} Hz: rates from {RESAMPLE_MIN_RATE} to {RESAMPLE_MAX_RATE} Hz "
                         f"other than {sr} are supported")
    return rate


def resample_filter(rate: int, sr: int = SAMPLE_RATE):
    """(L, M, half, H): the polyphase table of the `rate` -> `sr` filter, H fp32 [L, 2 * half + 1], computed in fp64 and rounded
    once; cached per (rate, sr).  A rate that is not an integer from 4000 to 192000 other than `sr`, or whose table would exceed
    16 MiB, raises ValueError (checked before the cache: 44100.0 is refused whatever was asked before)."""
    return _resample_filter(_check_rate(rate, sr), int(sr))


@lru_cache(maxsize=16)
def _resample_filter(rate: int, sr: int):
    g = math.gcd(rate, sr)
    L, M = sr // g, rate // g
    fc = RESAMPLE_ROLLOFF * min(1.0, L / M)
    half = math.ceil(RESAMPLE_ZERO_CROSSINGS / fc)
    T = 2 * half + 1
    if L * T * 4 > RESAMPLE_MAX_TABLE_BYTES:
        raise ValueError(f"cannot resample from {rate} Hz to {sr} Hz: {L} phases of {T} taps are a table of {L * T * 4} bytes "
                         f"(at most {RESAMPLE_MAX_TABLE_BYTES})")
    # t = p / L + half - j with an exact integer numerator
    num = np.arange(L, dtype=np.int64)[:, None] + (half - np.arange(T, dtype=np.int64))[None, :] * L
    t = num.astype(np.float64) / L
    inside = np.abs(num) <= half * L
    w = np.i0(RESAMPLE_KAISER_BETA * np.sqrt(np.maximum(0.0, 1.0 - (t / half) ** 2))) / np.i0(RESAMPLE_KAISER_BETA)
    H = np.where(inside, fc * np.sinc(fc * t) * w, 0.0).astype(np.float32)
    H.setflags(write=False)
    return L, M, half, H


def resample_reference(x, rate: int, sr: int = SAMPLE_RATE, lo: int = 0, hi: Optional[int] = None) -> np.ndarray:
    """The host statement of the resampler: mono float `x` at `rate` Hz -> outputs [lo, hi) of the `sr` Hz signal in fp64
    (default: all ceil(n L / M) of them), from the fp32 table, with 64-bit indices, a bounded piece at a time."""
    L, M, half, H = resample_filter(rate, sr)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n_in = x.shape[0]
    n_out = -(-n_in * L // M)
    hi = n_out if hi is None else int(hi)
    lo = int(lo)
    if not 0 <= lo <= hi <= n_out:
        raise ValueError(f"resample_reference: outputs [{lo}, {hi}) of {n_out}")
    T = 2 * half + 1
    taps = np.arange(T, dtype=np.int64)
    H64 = H.astype(np.float64)
    y = np.empty(hi - lo, dtype=np.float64)
    step = max(1, (1 << 21) // T)
    for a in range(lo, hi, step):
        n = np.arange(a, min(hi, a + step), dtype=np.int64)
        nm = n * M
        k = (nm // L)[:, None] - half + taps[None, :]
        ok = (k >= 0) & (k < n_in)
        xs = np.where(ok, x[np.clip(k, 0, max(n_in - 1, 0))], 0.0) if n_in else np.zeros(k.shape)
        y[a - lo: a - lo + len(n)] = (xs * H64[nm % L]).sum(axis=1)
    return y


def downmix(samples: np.ndarray, bits: Optional[int]) -> np.ndarray:
    """samples [n, C] (or [n]) -> mono fp32 [n] the way wm_resample stages its input: the channels converted to fp32 and summed in
    channel order in fp32, divided by fp32(C), times 2^-(bits - 1) (integer PCM; float: 1)."""
    s = np.asarray(samples)
    s = s.reshape(s.shape[0], -1)
    acc = s[:, 0].astype(np.float32)
    for c in range(1, s.shape[1]):
        acc = acc + s[:, c].astype(np.float32)
    return acc / np.float32(s.shape[1]) * np.float32(1.0 if bits is None else 2.0 ** -(bits - 1))


_RESAMPLE_TABLES = {}          # (rate, device) -> (L, M, half, table on the device); the few most recent ones
_RESAMPLE_TABLES_KEPT = 8


def _device_table(rate: int, device: torch.device):
    """(L, M, half, the table on `device`): uploaded once per (rate, device), transposed and ordered by r = n mod L --
    Hr[j][r] = H[(r M) mod L][j], fp32 [T][L] -- so that consecutive outputs read consecutive coefficients (csrc/resample.hip)."""
    key = (rate, device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _RESAMPLE_TABLES:
        L, M, half, H = resample_filter(rate)
        order = (np.arange(L, dtype=np.int64) * M) % L
        while len(_RESAMPLE_TABLES) >= _RESAMPLE_TABLES_KEPT:          # a table is up to 16 MiB of device memory: drop the oldest
            del _RESAMPLE_TABLES[next(iter(_RESAMPLE_TABLES))]
        _RESAMPLE_TABLES[key] = (L, M, half, torch.from_numpy(np.ascontiguousarray(H[order].T)).to(device))
    return _RESAMPLE_TABLES[key]


_PCM_DTYPES = {torch.float32: 0, torch.int16: 1, torch.int32: 2}


def resample_device(pcm: torch.Tensor, rate: int, bits: Optional[int] = None, split: bool = False) -> torch.Tensor:
    """`pcm` [n, C] or [n] on the GPU (float32, or int16 / int32 PCM of `bits` bits; 1..8 interleaved channels) at `rate` Hz ->
    mono fp32 [ceil(n * 16000 / rate)] at 16 kHz on the GPU: downmix, conversion and the polyphase filter in one launch
    (wm_resample, csrc/resample.hip), on the current stream of the tensor's device.  `split`: the channels are kept apart --
    fp32 [C, ceil(n * 16000 / rate)], row c bit for bit what a mono input holding channel c gives (wm_resample_channels: all
    channels in one launch; channels.py, rule 1).  No CPU fallback: without the native library this raises."""
    import native
    assert pcm.is_cuda and pcm.dtype in _PCM_DTYPES, "pcm must be a float32 / int16 / int32 tensor on the GPU"
    assert pcm.dim() in (1, 2)
    rate = _check_rate(rate, SAMPLE_RATE)
    p = (pcm[:, None] if pcm.dim() == 1 else pcm).contiguous()
    n_in, channels = int(p.shape[0]), int(p.shape[1])
    if n_in < 1:
        raise ValueError("resample_device: no samples")
    if pcm.dtype == torch.float32:
        scale = 1.0
    else:
        bits = int(bits) if bits is not None else (16 if pcm.dtype == torch.int16 else 32)
        scale = 2.0 ** -(bits - 1)
    L, M, half, table = _device_table(rate, p.device)
    n_out = -(-n_in * L // M)
    s = torch.cuda.current_stream(p.device).cuda_stream
    if split:
        out = torch.empty((channels, n_out), dtype=torch.float32, device=p.device)
        native.check(native.load_library().wm_resample_channels(p.data_ptr(), _PCM_DTYPES[pcm.dtype], channels, n_in, scale,
                                                                table.data_ptr(), L, M, half, out.data_ptr(), n_out, n_out, s),
                     "wm_resample_channels")
        return out
    out = torch.empty(n_out, dtype=torch.float32, device=p.device)
    native.check(native.load_library().wm_resample(p.data_ptr(), _PCM_DTYPES[pcm.dtype], channels, n_in, scale, table.data_ptr(),
                                                   L, M, half, out.data_ptr(), n_out, s), "wm_resample")
    return out


# ------------------------------------------------------------------------------------------------------------ files
WAVE_FORMAT_PCM, WAVE_FORMAT_IEEE_FLOAT, WAVE_FORMAT_EXTENSIBLE = 1, 3, 0xFFFE


def read_wav(data: bytes, name: str = "wav"):
    """RIFF/WAVE bytes -> (samples [n, C], rate, bits): int32 for PCM (8 bit unsigned, 16 / 24 / 32 bit signed), float32 with
    bits None for IEEE float32; WAVE_FORMAT_EXTENSIBLE carrying either."""
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise RuntimeError(f"{name}: not a RIFF/WAVE file")
    pos, fmt, body = 12, None, None
    while pos + 8 <= len(data):
        tag, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        chunk = data[pos + 8: pos + 8 + size]
        if tag == b"fmt ":
            fmt = chunk
        elif tag == b"data":
            body = chunk                  # a streamed file's size field may overshoot: the slice ends with the file
            if fmt is not None:
                break
        pos += 8 + size + (size & 1)
    if fmt is None or body is None or len(fmt) < 16:
        raise RuntimeError(f"{name}: no fmt / data chunk")
    tag, channels, rate, _, align, bits = struct.unpack_from("<HHIIHH", fmt, 0)
    if tag == WAVE_FORMAT_EXTENSIBLE:
        if len(fmt) < 40:
            raise RuntimeError(f"{name}: truncated WAVE_FORMAT_EXTENSIBLE header")
        tag = struct.unpack_from("<H", fmt, 24)[0]          # the first two bytes of the SubFormat GUID are the format tag
    width = (bits + 7) // 8
    if channels < 1 or width < 1 or align != channels * width:
        raise RuntimeError(f"{name}: {channels} channels of {bits} bits with a block of {align} bytes")
    n = len(body) // align
    raw = np.frombuffer(body, np.uint8, n * align).reshape(n, channels, width)
    if tag == WAVE_FORMAT_IEEE_FLOAT and bits == 32:
        return raw.copy().view("<f4").reshape(n, channels).astype(np.float32), int(rate), None
    if tag != WAVE_FORMAT_PCM or bits not in (8, 16, 24, 32):
        raise RuntimeError(f"{name}: format tag {tag} with {bits} bits is not supported (PCM 8 / 16 / 24 / 32, IEEE float32)")
    if bits == 8:
        return raw[:, :, 0].astype(np.int32) - 128, int(rate), 8
    wide = np.zeros((n, channels, 4), dtype=np.uint8)
    wide[:, :, 4 - width:] = raw                             # into the top bytes, then an arithmetic shift: sign extension
    return (wide.view("<i4").reshape(n, channels) >> (8 * (4 - width))).astype(np.int32), int(rate), int(bits)


def load_pcm(file: str, sr: int = SAMPLE_RATE):
    """(samples [n, C], rate, bits) of a .flac / .wav / .npy file as stored: int32 for integer sources, float32 (bits None) for
    float ones; a .npy waveform counts as mono float at `sr` Hz."""
    file = str(file)
    if file.endswith(".npy"):
        return np.load(file).astype(np.float32).reshape(-1, 1), sr, None
    if file.endswith(".flac"):
        with open(file, "rb") as f:
            return decode_flac(f.read())
    if file.endswith(".wav"):
        with open(file, "rb") as f:
            return read_wav(f.read(), file)
    raise RuntimeError(f"cannot decode {file}: only .wav / .flac / .npy are supported without ffmpeg")


def _mono_at_sr(samples: np.ndarray, bits: Optional[int]) -> np.ndarray:
    """What load_audio returns for a file already at the wanted rate: the channels as fp32, their mean, over 2^(bits - 1) for
    integer PCM (for PCM16 this is the `pcm.astype(np.float32).mean(axis=1) / 32768.0` it always was, bit for bit)."""
    mono = samples.astype(np.float32).mean(axis=1)
    return mono.astype(np.float32) if bits is None else (mono / float(1 << (bits - 1))).astype(np.float32)


def _resample_host_or_device(pcm: np.ndarray, rate: int, bits: Optional[int], sr: int) -> np.ndarray:
    if sr == SAMPLE_RATE and torch.cuda.is_available():
        return resample_device(torch.from_numpy(np.ascontiguousarray(pcm)).cuda(), rate, bits).cpu().numpy()
    return resample_reference(downmix(pcm, bits), rate, sr).astype(np.float32)


def load_audio(file: str, sr: int = SAMPLE_RATE) -> np.ndarray:
    """Mono float32 waveform in [-1, 1] at `sr` Hz (W/whisper_utils.py:17-54, which pipes every file through ffmpeg).  Without
    ffmpeg: .wav (PCM 8 / 16 / 24 / 32 bit, float32), .flac (own decoder) and float .npy; several channels are averaged, and a file
    at another rate (4 kHz .. 192 kHz) is resampled -- on the GPU when there is one (resample_device), else by the host statement
    (resample_reference) rounded to fp32.  Every file is read and decoded once."""
    file = str(file)
    if file.endswith(".npy"):
        return np.load(file).astype(np.float32).flatten()
    samples, rate, bits = load_pcm(file, sr)
    if rate != sr:
        return _resample_host_or_device(samples, rate, bits, sr)
    return _mono_at_sr(samples, bits)


def channels_at_sr(samples: np.ndarray, bits: Optional[int]) -> np.ndarray:
    """fp32 [C, n]: every channel of a file already at the wanted rate, each `_mono_at_sr` of its one column (channels.py, rule 1)."""
    samples = samples.reshape(samples.shape[0], -1)
    return np.stack([_mono_at_sr(samples[:, c:c + 1], bits) for c in range(samples.shape[1])])


def load_audio_device(file: str, channels: Optional[str] = None) -> torch.Tensor:
    """`load_audio` with the result on the GPU, fp32 [n] at 16 kHz: a file at 16 kHz is the upload of load_audio's waveform; any
    other rate is resample_device of the uploaded PCM -- the samples never come back to the host.  One decode either way.
    `channels="split"`: fp32 [C, n], the channels kept apart (channels.py, rule 1: resample_device(split=True), or the host's
    channels_at_sr for a file at 16 kHz); at most 8 channels."""
    file = str(file)
    if channels not in (None, "split"):
        raise ValueError(f"load_audio_device: channels={channels!r} is not None or 'split'")
    if file.endswith(".npy"):
        mono = torch.from_numpy(load_audio(file)).cuda()
        return mono[None] if channels else mono
    samples, rate, bits = load_pcm(file)
    if channels:
        if not 1 <= samples.shape[1] <= 8:
            raise ValueError(f"load_audio_device: {file} has {samples.shape[1]} channels (1 .. 8 can be kept apart)")
        if rate == SAMPLE_RATE:
            return torch.from_numpy(channels_at_sr(samples, bits)).cuda()
        return resample_device(torch.from_numpy(np.ascontiguousarray(samples)).cuda(), rate, bits, split=True)
    if rate == SAMPLE_RATE:
        return torch.from_numpy(_mono_at_sr(samples, bits)).cuda()
    return resample_device(torch.from_numpy(np.ascontiguousarray(samples)).cuda(), rate, bits)


def pad_or_trim(array, length: int = N_SAMPLES, *, axis: int = -1):
    """Pad with zeros or cut to `length` samples along `axis` (W/whisper_utils.py:56-79)."""
    if torch.is_tensor(array):
        n = array.shape[axis]
        if n > length:
            array = array.narrow(axis, 0, length)
        elif n < length:
            pad = [0, 0] * array.ndim
            pad[2 * (array.ndim - 1 - (axis % array.ndim)) + 1] = length - n
            array = F.pad(array, pad)
        return array
    n = array.shape[axis]
    if n > length:
        array = np.take(array, np.arange(length), axis=axis)
    elif n < length:
        widths = [(0, 0)] * array.ndim
        widths[axis] = (0, length - n)
        array = np.pad(array, widths)
    return array


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


@lru_cache(maxsize=None)
def _mel_filterbank(n_mels: int = N_MELS, n_fft: int = N_FFT, sr: int = SAMPLE_RATE) -> np.ndarray:
    fft_freqs = np.linspace(0, sr / 2, 1 + n_fft // 2)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sr / 2), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_freqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    weights = np.maximum(0, np.minimum(lower, upper))
    weights *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return weights.astype(np.float32)


def mel_filters(device, n_mels: int = N_MELS) -> torch.Tensor:
    """[n_mels, 201] fp32: 80 bins (Whisper up to large-v2) or 128 (large-v3 and after), the two banks upstream ships."""
    if n_mels not in (80, 128):
        raise ValueError(f"Unsupported n_mels: {n_mels} (Whisper models take 80 or 128 mel bins)")
    return torch.from_numpy(_mel_filterbank(n_mels)).to(device)


def log_mel_spectrogram(audio: Union[str, np.ndarray, torch.Tensor], n_mels: int = N_MELS, padding: int = 0,
                        device: Optional[Union[str, torch.device]] = None) -> torch.Tensor:
    """[80, n_frames] log-mel: Hann STFT (n_fft 400, hop 160), |.|^2, mel projection, log10, clamp to
    max - 8, (x + 4) / 4  (W/whisper_utils.py:99-146)."""
    if not torch.is_tensor(audio):
        if isinstance(audio, str):
            audio = load_audio(audio)
        audio = torch.from_numpy(audio)
    if device is not None:
        audio = audio.to(device)
    if padding > 0:
        audio = F.pad(audio, (0, padding))
    window = torch.hann_window(N_FFT).to(audio.device)
    stft = torch.stft(audio, N_FFT, HOP_LENGTH, window=window, return_complex=True)
    magnitudes = stft[..., :-1].abs() ** 2
    mel_spec = mel_filters(audio.device, n_mels) @ magnitudes
    log_spec = torch.clamp(mel_spec, min=1e-10).log10()
    log_spec = torch.maximum(log_spec, log_spec.max() - 8.0)
    return (log_spec + 4.0) / 4.0


def log_mel_spectrogram_device(audio: torch.Tensor, n_mels: int = N_MELS, dtype: torch.dtype = torch.float16,
                               stream: Optional[int] = None) -> torch.Tensor:
    """The same transform as a HIP kernel (`wm_log_mel`, csrc/frontend.hip): `audio` fp32 [B, n] or [n]
    on the GPU, already padded / trimmed (n a multiple of HOP_LENGTH) -> [B, n_mels, n // HOP_LENGTH]
    (or [n_mels, frames] for a 1-D input) in `dtype` (fp16: what the encoder engine takes; fp32: what
    log_mel_spectrogram returns).  Each clip is clamped to its own max - 8, i.e. the reference applied
    per clip.  No CPU fallback: without the native library this raises."""
    import ctypes as C
    import native
    assert audio.is_cuda and audio.dtype == torch.float32, "audio must be an fp32 tensor on the GPU"
    assert dtype in (torch.float16, torch.float32)
    single = audio.dim() == 1
    a = (audio[None] if single else audio).contiguous()
    lib = native.load_library()
    B, n = a.shape
    filt = mel_filters(a.device, n_mels).float().contiguous()
    out = torch.empty((B, n_mels, n // HOP_LENGTH), dtype=dtype, device=a.device)
    ws_bytes = lib.wm_log_mel_workspace_bytes(B, n, n_mels)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=a.device)
    s = torch.cuda.current_stream(a.device).cuda_stream if stream is None else stream
    o16 = out.data_ptr() if dtype == torch.float16 else None
    o32 = out.data_ptr() if dtype == torch.float32 else None
    native.check(lib.wm_log_mel(a.data_ptr(), B, n, a.stride(0), filt.data_ptr(), n_mels, o16, o32, ws.data_ptr(),
                                C.c_size_t(ws_bytes), s), "wm_log_mel")
    return out[0] if single else out


def long_log_mel_device(audio: torch.Tensor, n_mels: int = N_MELS):
    """The log-mel of a whole file for long-form transcription (transcribe.py): `audio` fp32 [n] on the GPU, any length ->
    (mel fp16 [n_mels, content_frames + N_FRAMES], content_frames).  Upstream's `log_mel_spectrogram(audio, padding=N_SAMPLES)`
    as ONE wm_log_mel call: N_SAMPLES zeros are appended (and zeros up to a whole hop, which the kernel asks for), the first
    (n + N_SAMPLES) // HOP_LENGTH frames are kept -- the last N_FRAMES of them are the log-mel of the 30 s of padding -- and the
    clamp to max - 8 is taken over the whole file, as upstream does."""
    assert audio.is_cuda and audio.dtype == torch.float32 and audio.dim() == 1, "audio must be a 1-D fp32 tensor on the GPU"
    n = int(audio.shape[0])
    padded = -(-(n + N_SAMPLES) // HOP_LENGTH) * HOP_LENGTH
    mel = log_mel_spectrogram_device(F.pad(audio, (0, padded - n)), n_mels=n_mels, dtype=torch.float16)
    n_frames = (n + N_SAMPLES) // HOP_LENGTH
    return mel[:, :n_frames].contiguous(), n_frames - N_FRAMES
