"""Brute-force restatement of the truncated-sampling contract (top-k, top-p, min-p), independent of truncation.py, and the fixture
rows of tests/test_truncate_cpu.py and tests/test_gpu_truncate.py.

The allowed tokens are sorted, equal values are grouped into classes, counts and weights are accumulated with Python integers and the
three rules are walked class by class.  The weight of a class is the fixed-point form of the contract, restated here operation by
operation on float32 arrays (numpy never fuses a multiplication with an addition)."""
import math

import numpy as np

F32 = np.float32
COEF = [F32(float.fromhex(h)) for h in ("0x1.62e430p-1", "0x1.ebfbe0p-3", "0x1.c6af6cp-5", "0x1.3b2a54p-7", "0x1.5f0890p-10", "0x1.44138ap-13")]


def scalars(T, top_p, min_p):
    """(c, P, gap): what the host hands to the kernel."""
    c = F32(math.log2(math.e) / T)
    P = 65536 if top_p >= 1.0 else max(1, int(round(top_p * 65536)))
    gap = F32(-np.inf) if min_p <= 0 else F32(T * math.log(min_p))
    return c, P, gap


def class_weights(v, m, c):
    """Python-int weights of the class values `v` (float16 array) under the maximum `m`."""
    d = v.astype(F32) - F32(m)
    s = d * F32(c)
    i = np.rint(s)
    f = s - i
    g = COEF[5] * f + COEF[4]
    for k in (3, 2, 1, 0):
        g = g * f
        g = g + COEF[k]
    p = g * f
    p = p + F32(1.0)
    assert s.dtype == f.dtype == g.dtype == p.dtype == F32
    out = []
    for ii, pp in zip(i.tolist(), p.tolist()):
        if not ii >= -31:
            out.append(0)
            continue
        u = int(np.rint(F32(pp) * F32(2.0 ** 30)))
        sh = int(-ii)
        out.append((u + ((1 << sh) >> 1)) >> sh)
    return out


class Row:
    """The classes of one row's allowed set at one temperature: `x` = the fp16 logits of A (finite, not empty)."""

    def __init__(self, x, T):
        x = np.asarray(x, dtype=np.float16)
        assert x.ndim == 1 and x.size and np.isfinite(x).all()
        srt = np.sort(x.astype(np.float64))[::-1]                      # (-0.0 == 0.0 as numbers)
        starts = np.flatnonzero(np.concatenate([[True], srt[1:] != srt[:-1]]))
        self.values = srt[starts].astype(np.float16)
        self.counts = [int(n) for n in np.diff(np.concatenate([starts, [srt.size]]))]
        self.T, self.m = T, self.values[0]
        self.d = self.values.astype(F32) - F32(self.m)
        self._w = {}

    def weights(self, c):
        key = float(c)
        if key not in self._w:
            self._w[key] = class_weights(self.values, self.m, c)
        return self._w[key]

    def cut(self, top_k=0, top_p=1.0, min_p=0.0):
        """(cut value as float16, kept tokens, index of the last kept class)."""
        c, P, gap = scalars(self.T, top_p, min_p)
        n = len(self.counts)
        jk = n - 1
        if top_k > 0:
            cum = 0
            for j in range(n):
                cum += self.counts[j]
                if cum >= top_k:
                    jk = j
                    break
        jp = jk
        if P < 65536:
            w = self.weights(c)
            Q = sum(self.counts[j] * w[j] for j in range(jk + 1))
            cum = 0
            for j in range(jk + 1):
                cum += self.counts[j] * w[j]
                if cum * 65536 >= P * Q:
                    jp = j
                    break
        jq = int(np.flatnonzero(self.d >= gap)[-1])                      # d descends; class 1 (d = 0) always passes
        last = min(jk, jp, jq)
        return self.values[last], sum(self.counts[:last + 1]), last


def hf_keep(x, T, top_k=0, top_p=1.0, min_p=0.0):
    """Hugging Face's three warpers in its order, in float64 on one row of allowed logits: (kept mask, margin) where margin is the
    distance of the nucleus boundary from p, in units of the mass (inf without top_p)."""
    z = np.asarray(x, dtype=np.float64) / T
    keep = np.ones(z.size, dtype=bool)
    if top_k > 0 and top_k < z.size:
        kth = np.sort(z)[-top_k]
        keep &= ~(z < kth)
    margin = math.inf
    if top_p < 1.0:
        zz = np.where(keep, z, -np.inf)
        order = np.argsort(zz, kind="stable")                            # ascending, as TopPLogitsWarper sorts
        pr = np.exp(zz[order] - zz.max())
        pr /= pr.sum()
        cum = np.cumsum(pr)
        remove = cum <= 1.0 - top_p
        remove[-1] = False
        keep[order[remove]] = False
        margin = float(np.abs(cum[:-1] - (1.0 - top_p)).min()) if z.size > 1 else math.inf
    if min_p > 0.0:
        zz = np.where(keep, z, -np.inf)
        pr = np.exp(zz - zz.max())
        pr /= pr.sum()
        keep &= ~(pr < min_p * pr.max())
    return keep, margin


# ---------------------------------------------------------------------------------------------------------------- fixtures
KINDS = ("normal15", "normal3", "peaked", "single", "equal", "coarse", "huge_max", "very_low", "ts_high", "ts_low")


def fixture_row(kind, V, seed, tb=None):
    """One row of fp16 logits [V].  `tb`: where the timestamps begin (ts_high / ts_low shift them by +-8)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.5, V)
    if kind == "normal3":
        x *= 2.0
    elif kind == "peaked":
        x[rng.integers(0, V, 1)] += 30.0
        if tb is not None:
            x[tb + 7] += 30.0
    elif kind == "single":
        x[:] = -np.inf                                                   # the test plants the one finite logit on an allowed token
    elif kind == "equal":
        x[:] = 1.5
    elif kind == "coarse":
        x = np.round(x * 4.0) / 4.0                                      # ties across every k-th place and every p-boundary
    elif kind == "huge_max":
        x[rng.integers(0, V if tb is None else tb, 3)] = 65504.0        # (text tokens only: one on each side would tie the timestamp rule)
    elif kind == "very_low":
        x = -60000.0 - np.abs(x) * 100.0
    elif kind in ("ts_high", "ts_low") and tb is not None:
        x[tb:] += 8.0 if kind == "ts_high" else -8.0
    return x.astype(np.float16)


CONTROLS_ALONE = ([(k, 1.0, 0.0) for k in (0, 1, 2, 50)] + [(0, p, 0.0) for p in (0.1, 0.5, 0.9, 0.999)]
                  + [(0, 1.0, q) for q in (0.05, 0.5)])
CONTROLS_COMBINED = [(50, 0.9, 0.0), (50, 0.5, 0.05), (2, 0.999, 0.5), (0, 0.9, 0.05), (50, 1.0, 0.5), (1, 0.1, 0.5)]


def controls(V):
    """Every (top_k, top_p, min_p) the kernel test runs at vocabulary size V."""
    return CONTROLS_ALONE + [(V, 1.0, 0.0), (V + 7, 1.0, 0.0), (V + 7, 0.5, 0.0)] + CONTROLS_COMBINED
