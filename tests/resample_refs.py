"""The oracle of the resampler tests: an independent fp64 restatement of the filter, and the files the tests feed it.

`oracle` evaluates h directly from the formula at the exact time n M / L - k (an integer numerator n M - k L over L), never
through whisper_utils.resample_filter's table, and returns with every output y the sum S = sum |h x| its error bound is stated in:

    |y_device - y_oracle| <= (T + 4) * 2^-24 * S        T = 2 half + 1

the worst case of T fp32 FMAs in any order (T * 2^-24 * S, to first order), plus one rounding each for the coefficient (fp64 ->
fp32), the channel sum, the division by the channel count and the conversion of an integer above 24 bits: every one of them is a
relative error of at most 2^-24 on a term of S.  Derived, not tuned.  Test infrastructure only.
"""
import hashlib
import math
import struct

import numpy as np

SR = 16000
RATES = (48000, 44100, 8000, 22050, 24000, 11025)
EPS = 2.0 ** -24


def params(rate, sr=SR):
    """(L, M, fc, half, T) from the formulas."""
    g = math.gcd(rate, sr)
    L, M = sr // g, rate // g
    fc = 0.9 * min(1.0, L / M)
    half = math.ceil(32 / fc)
    return L, M, fc, half, 2 * half + 1


def h_exact(num, L, fc, half):
    """h at t = num / L (num: int64 array): fc sinc(fc t) I0(11 sqrt(1 - (t / half)^2)) / I0(11) inside |t| <= half, else 0."""
    num = np.asarray(num, dtype=np.int64)
    t = num.astype(np.float64) / L
    inside = np.abs(num) <= half * L
    a = np.pi * fc * t
    safe = np.where(num == 0, 1.0, a)
    s = np.where(num == 0, 1.0, np.sin(safe) / safe)
    u = np.where(inside, 1.0 - (t / half) ** 2, 0.0)
    w = np.i0(11.0 * np.sqrt(np.maximum(u, 0.0))) / np.i0(11.0)
    return np.where(inside, fc * s * w, 0.0)


def mono64(samples, bits):
    """The exact downmix in fp64: mean of the channels times 2^-(bits - 1) (float input: bits None)."""
    s = np.asarray(samples)
    s = s.reshape(s.shape[0], -1).astype(np.float64)
    return s.sum(axis=1) / s.shape[1] * (1.0 if bits is None else 2.0 ** -(bits - 1))


def _oracle_all(X, rate, sr):
    """Every output of whole signals, phase by phase.  Outputs n = r + L q (q = 0, 1, ...) share their coefficients exactly: with
    i_r = floor(r M / L), output n reads x[i_r + M q + o] at time (n M - (i_r + M q + o) L) / L = (r M - (i_r + o) L) / L, an
    integer identity -- so h is evaluated once per (r, o), still straight from the formula, and each phase is one product of a
    strided window view of the zero-padded signals with that row."""
    L, M, fc, half, T = params(rate, sr)
    n_in, V = X.shape
    n_out = -(-n_in * L // M)
    offs = np.arange(-half - 1, half + 2, dtype=np.int64)
    pad = half + 1
    Xp = np.zeros((n_in + 2 * pad + M + 1, V))
    Xp[pad:pad + n_in] = X
    Ap = np.abs(Xp)
    y, S = np.zeros((n_out, V)), np.zeros((n_out, V))
    s0, s1 = Xp.strides
    for r in range(min(L, n_out)):
        i_r = r * M // L
        h = h_exact(r * M - (i_r + offs) * L, L, fc, half)
        Q = len(range(r, n_out, L))
        assert i_r + M * (Q - 1) + offs[-1] + pad < Xp.shape[0]
        for src, dst, row in ((Xp, y, h), (Ap, S, np.abs(h))):
            win = np.lib.stride_tricks.as_strided(src[i_r:], shape=(Q, offs.size, V), strides=(M * s0, s0, s1), writeable=False)
            dst[r::L] = np.einsum("k,qkv->qv", row, win)
    return y, S


def oracle(x, rate, n=None, n_in=None, x0=0, sr=SR):
    """x fp64 [len] or [len, V] (V signals at once) holds samples x0 .. x0 + len of signals of n_in samples (default: all of them);
    outputs `n` (default: all ceil(n_in L / M)).  Returns (y, S), each [len(n)] or [len(n), V].  Every sample an output reaches
    must lie in x or outside [0, n_in)."""
    L, M, fc, half, T = params(rate, sr)
    x = np.asarray(x, dtype=np.float64)
    single = x.ndim == 1
    X = x[:, None] if single else x
    if n is None and n_in is None and x0 == 0:
        y, S = _oracle_all(X, rate, sr)
        return (y[:, 0], S[:, 0]) if single else (y, S)
    n_in = x0 + X.shape[0] if n_in is None else int(n_in)
    n_out = -(-n_in * L // M)
    n = np.arange(n_out, dtype=np.int64) if n is None else np.asarray(n, dtype=np.int64)
    assert n.size == 0 or (n.min() >= 0 and n.max() < n_out)
    offs = np.arange(-half - 1, half + 2, dtype=np.int64)           # one more each side than the filter reaches: h is 0 there
    y = np.zeros((n.size, X.shape[1]))
    S = np.zeros((n.size, X.shape[1]))
    step = max(1, (1 << 22) // (offs.size * X.shape[1]))
    for a in range(0, n.size, step):
        nn = n[a:a + step]
        nm = nn * M
        k = (nm // L)[:, None] + offs[None, :]
        h = h_exact(nm[:, None] - k * L, L, fc, half)
        live = (k >= 0) & (k < n_in) & (h != 0.0)
        assert not live.any() or (k[live].min() >= x0 and k[live].max() < x0 + X.shape[0]), "the oracle was given too short a slice"
        xs = np.where(live[:, :, None], X[np.clip(k - x0, 0, X.shape[0] - 1)], 0.0)
        prod = h[:, :, None] * xs
        y[a:a + step] = prod.sum(axis=1)
        S[a:a + step] = np.abs(prod).sum(axis=1)
    return (y[:, 0], S[:, 0]) if single else (y, S)


def bound(S, rate):
    return (params(rate)[4] + 4) * EPS * S


# ------------------------------------------------------------------------------------------------------------------ files
def wav_bytes(samples, rate, kind, extensible=False):
    """A RIFF/WAVE file of samples [n, C]: kind 'u8' | 'i16' | 'i24' | 'i32' (integers of that width) | 'f32'."""
    s = np.asarray(samples)
    n, ch = s.shape
    bits = {"u8": 8, "i16": 16, "i24": 24, "i32": 32, "f32": 32}[kind]
    if kind == "f32":
        body = s.astype("<f4").tobytes()
    elif kind == "u8":
        body = (s.astype(np.int64) + 128).astype(np.uint8).tobytes()
    else:
        body = s.astype("<i4").view(np.uint8).reshape(n, ch, 4)[:, :, :bits // 8].tobytes()
    tag = 3 if kind == "f32" else 1
    align = ch * bits // 8
    if extensible:
        guid = struct.pack("<H", tag) + bytes.fromhex("000000001000800000aa00389b71")
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, ch, rate, rate * align, align, bits, 22, bits, (1 << ch) - 1) + guid
    else:
        fmt = struct.pack("<HHIIHH", tag, ch, rate, rate * align, align, bits)
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt
    chunks += b"LIST" + struct.pack("<I", 5) + b"INFOx" + b"\0"           # an odd-sized chunk to step over (padded to even)
    chunks += b"data" + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


def _crc_table(poly, width):
    top, mask = 1 << (width - 1), (1 << width) - 1
    table = np.zeros(256, dtype=np.int64)
    for b in range(256):
        c = b << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        table[b] = c
    return table


_CRC8, _CRC16 = _crc_table(0x07, 8), _crc_table(0x8005, 16)


def _crc_rows(rows, table, width):
    """CRC of every row of a uint8 [frames, bytes] array at once (the loop runs over the byte position)."""
    crc = np.zeros(rows.shape[0], dtype=np.int64)
    mask, shift = (1 << width) - 1, width - 8
    for col in rows.T.astype(np.int64):
        crc = ((crc << 8) & mask) ^ table[(crc >> shift) ^ col]
    return crc


def quick_flac(samples, rate, block=4096):
    """A 16-bit FLAC stream of samples [n, C] (integers in int16 range) in VERBATIM subframes, written with numpy so that half a
    minute of stereo audio takes a fraction of a second (tests/flac_writer.py, which covers the format, goes bit by bit).  A
    16-bit verbatim frame is byte aligned throughout: header, CRC-8, per channel one subframe byte and big-endian samples, CRC-16."""
    from flac_writer import utf8_number
    s = np.asarray(samples, dtype=np.int64)
    n, ch = s.shape
    assert block in (4096,) and n >= 1 and 1 <= ch <= 8 and np.abs(s).max() < 32768
    raw = s.astype("<i2").tobytes()
    n_frames = -(-n // block)
    last = n - (n_frames - 1) * block
    si = ((last if n_frames == 1 else block) << 128 | block << 112 | rate << 44 | (ch - 1) << 41 | 15 << 36 | n).to_bytes(18, "big")
    out = [b"fLaC", bytes([0x80]), (34).to_bytes(3, "big"), si, hashlib.md5(raw).digest()]
    be = s.astype(">i2")
    groups = {}
    for f in range(n_frames):
        size = block if f < n_frames - 1 else last
        explicit = size != block
        head = bytes([0xFF, 0xF8, ((7 if explicit else 12) << 4), ((ch - 1) << 4) | (4 << 1)]) + utf8_number(f)
        if explicit:
            head += (size - 1).to_bytes(2, "big")
        groups.setdefault((len(head), size), []).append((f, head))
    frames = [None] * n_frames
    for (hl, size), members in groups.items():
        heads = np.frombuffer(b"".join(h for _, h in members), np.uint8).reshape(len(members), hl)
        rows = np.zeros((len(members), hl + 1 + ch * (1 + 2 * size) + 2), dtype=np.uint8)
        rows[:, :hl] = heads
        rows[:, hl] = _crc_rows(heads, _CRC8, 8)
        for i, (f, _) in enumerate(members):
            chunk = be[f * block: f * block + size]
            for c in range(ch):
                at = hl + 1 + c * (1 + 2 * size)
                rows[i, at] = 0x02                                   # subframe: verbatim, no wasted bits
                rows[i, at + 1: at + 1 + 2 * size] = np.ascontiguousarray(chunk[:, c]).view(np.uint8)
        crc = _crc_rows(rows[:, :-2], _CRC16, 16)
        rows[:, -2], rows[:, -1] = crc >> 8, crc & 0xFF
        for i, (f, _) in enumerate(members):
            frames[f] = rows[i].tobytes()
    return b"".join(out + frames)
