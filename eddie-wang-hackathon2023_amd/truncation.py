"""Top-k, top-p and min-p sampling: the contract, in numpy.

Every draw above temperature 0 -- `best_of`, the samples of `fallback_best_of`, every rung of the long-form ladder -- is otherwise
taken from the whole vocabulary.  The three options restrict the draw the way Hugging Face's `generate(top_k, top_p, min_p)` and
CTranslate2's `sampling_topk` / `sampling_topp` do.  This module is the statement of the rule on the host: the device kernel
(csrc/truncate.hip, wm_sample_step) and the literal loops (host_decoding.GreedyDecoder) are held to it, and the CPU tests
(tests/test_truncate_cpu.py) hold all of them to a brute-force restatement (tests/truncate_refs.py).

For one row at a token step, AFTER the rules of the step (suppress lists, timestamp rules, the text-versus-timestamp decision):
  A    the allowed tokens whose logit is not -inf (logits are finite or -inf);
  x_n  their fp16 logits, m their maximum, T > 0 the temperature of the call.
fp16 has at most 65 536 values, so A falls into VALUE CLASSES v_1 = m > v_2 > ... with counts c_j (-0 and +0 are one value).  A class
is kept whole or dropped whole, so the result is one number per row, the CUT: token n may be drawn iff x_n >= cut.

Weights are fixed-point integers, so that host and device agree bit for bit: q(v) ~ 2^30 * exp((v - m) / T), computed as

    d = fp32(v) - fp32(m)                     one fp32 subtraction (d <= 0)
    s = d * c                                 one fp32 multiplication; c = fp32(log2(e) / T) comes from the host (`params`)
    i = rint(s)                               round half to even, exact;  i < -31: q = 0
    f = s - i                                 exact, in [-0.5, 0.5]
    g = ((((K5*f + K4)*f + K3)*f + K2)*f + K1)*f + K0        Horner, every * and + one correctly rounded fp32 operation,
    p = g*f + 1                               NO fused multiply-add anywhere;  p ~ 2^f in [0.707, 1.415]
    u = uint32(rint(p * 2^30))                exact scaling, exact rounding
    q = (u + (2^(-i) >> 1)) >> -i             64-bit integer, round half up

K0..K5 (`EXP2_COEF`) are the fp32 values of the degree-5 Chebyshev interpolant of (2^f - 1) / f on [-0.5, 0.5]: the polynomial is
within 9.2e-9 of 2^f, and q(m) = 2^30 exactly.  Measured exhaustively (all fp16 v <= m, m in {65504, 11.5, 0, -3.25, -60000},
T in {0.2, 0.4, 1.0}; tests/test_truncate_cpu.py): |q - 2^30 e| <= 1.28e-6 * 2^30 e + 0.5 with e = exp((v - m) / T) in float64 -- the
relative part is the rounding of d, c and s (|s| ln 2 times three fp32 roundings: it grows towards the tail, where the weight is a
few units), the half unit is the final rounding.  The test asserts 1.5e-6 * 2^30 e + 0.5.  A token more than 31.5 / c below the
maximum (21.8 T) weighs 0: that is part of the contract.

Selection, in Hugging Face's order (top-k, then top-p on the survivors, then min-p):
  top_k  (int >= 0, 0 = off)   j_k = the smallest j with c_1 + ... + c_j >= k: ties at the k-th value are all kept (Hugging Face's
                               `scores < kth` does the same).  k >= |A| keeps everything.
  top_p  (0 < p <= 1, 1 = off) with Q_j = sum_{i<=j} c_i q(v_i) and Q = Q_{j_k}: j_p = the smallest j <= j_k with
                               Q_j * 2^16 >= P * Q, P = max(1, round(p * 2^16)) (`params`).  64-bit integers: Q < 2^46.
  min_p  (0 <= q < 1, 0 = off) classes with fp32(v) - fp32(m) >= gap are kept, gap = fp32(T * ln q), -inf when off (`params`).
The row keeps classes 1 .. min(j_k, j_p, j_q); class 1 is always kept.  `cut` is the value of the last kept class, `kept` the number
of tokens in the kept classes.

The draw is the Gumbel-max of the token step, same generator and coordinates, restricted to x_n >= cut: a row whose cut keeps
everything draws the token it draws without the options.  The log-probability that is booked is that of the UNTRUNCATED
distribution after the rules, log_softmax(x over A)[token] at temperature 1, as upstream books it: truncation never writes into the
logits.  (With top_k = 1 every token would otherwise have log-probability 0 and the ladder's logprob_threshold could never fire.)

Three differences from Hugging Face: a class is never split (HF keeps single tokens in sort order, so it may keep some of a tie at the
p-boundary); the booked log-probability is untruncated; the weights are fixed-point, so a boundary within ~1e-5 of a class's
cumulative share (half a step of P, 7.6e-6, plus the weights' measured 1.3e-6) may fall the other way.  Nobody has tuned any value on speech.

At temperature 0 and under beam search the options are inert, not refused: the long-form ladder starts at 0 and climbs.
"""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np

ONE = 1 << 30                # q(m)
P_ONE = 1 << 16              # top_p = 1 in the fixed-point form the kernel takes
MAX_SHIFT = 31               # i < -MAX_SHIFT: the weight is 0
# fp32 coefficients K0 .. K5 of (2^f - 1) / f on [-0.5, 0.5] (csrc/truncate.hip restates them)
EXP2_COEF = tuple(np.float32(float.fromhex(h)) for h in (
    "0x1.62e430p-1", "0x1.ebfbe0p-3", "0x1.c6af6cp-5", "0x1.3b2a54p-7", "0x1.5f0890p-10", "0x1.44138ap-13"))


def check_options(top_k, top_p, min_p) -> None:
    """ValueError unless top_k is an int >= 0, top_p a finite number in (0, 1] and min_p a finite number in [0, 1)."""
    if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or top_k < 0:
        raise ValueError(f"top_k {top_k!r} must be an integer >= 0 (0 = off)")
    for name, v in (("top_p", top_p), ("min_p", min_p)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
            raise ValueError(f"{name} {v!r} must be a finite number")
    if not 0.0 < float(top_p) <= 1.0:
        raise ValueError(f"top_p {top_p!r} outside (0, 1] (1 = off)")
    if not 0.0 <= float(min_p) < 1.0:
        raise ValueError(f"min_p {min_p!r} outside [0, 1) (0 = off)")


def truncation_on(top_k, top_p, min_p) -> bool:
    return int(top_k) > 0 or float(top_p) < 1.0 or float(min_p) > 0.0


def params(temperature: float, top_p: float = 1.0, min_p: float = 0.0) -> Tuple[np.float32, int, np.float32]:
    """(c, P, gap) of a call at `temperature` > 0: the three scalars wm_sample_io takes besides top_k."""
    t = float(temperature)
    if not (math.isfinite(t) and t > 0):
        raise ValueError(f"truncated sampling needs a temperature > 0, not {temperature!r}")
    c = np.float32(math.log2(math.e) / t)
    p_q16 = P_ONE if float(top_p) >= 1.0 else max(1, min(P_ONE, int(round(float(top_p) * P_ONE))))
    gap = np.float32(-np.inf) if float(min_p) <= 0.0 else np.float32(t * math.log(float(min_p)))
    return c, p_q16, gap


def weights(d: np.ndarray, c) -> np.ndarray:
    """q for d = fp32(v) - fp32(m) <= 0 (float32 array) and the scale c: int64, the arithmetic of the module docstring."""
    d = np.asarray(d, dtype=np.float32)
    k0, k1, k2, k3, k4, k5 = EXP2_COEF
    with np.errstate(over="ignore", invalid="ignore"):
        s = (d * np.float32(c)).astype(np.float32)
        i = np.rint(s).astype(np.float32)
        f = (s - i).astype(np.float32)
        g = (k5 * f + k4).astype(np.float32)
        for k in (k3, k2, k1, k0):
            g = ((g * f).astype(np.float32) + k).astype(np.float32)
        p = ((g * f).astype(np.float32) + np.float32(1.0)).astype(np.float32)
        dead = ~(i >= -MAX_SHIFT)
        u = np.rint(np.where(dead, np.float32(0), p) * np.float32(ONE)).astype(np.int64)
        sh = np.where(dead, 0, -i).astype(np.int64)
    q = (u + ((np.int64(1) << sh) >> 1)) >> sh
    return np.where(dead, 0, q).astype(np.int64)


def deltas(x: np.ndarray) -> np.ndarray:
    """fp32(x) - fp32(max x) of fp16 values: the d of the weights and of the min_p rule."""
    x32 = np.asarray(x, dtype=np.float16).astype(np.float32)
    return (x32 - x32.max()).astype(np.float32)


def cut(x: np.ndarray, temperature: float, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0) -> Tuple[np.float16, int]:
    """(cut, kept) of one row: `x` holds the fp16 logits of A (1-D, finite, not empty)."""
    x = np.asarray(x)
    assert x.dtype == np.float16 and x.ndim == 1 and x.size and np.isfinite(x).all()
    c, p_q16, gap = params(temperature, top_p, min_p)
    v, n = np.unique(x.astype(np.float32) + np.float32(0), return_counts=True)     # ascending, exact in fp32; -0 + 0 = +0: one class
    v, n = v[::-1].astype(np.float16), n[::-1].astype(np.int64)       # v_1 = m first
    d = deltas(v)
    last = len(v) - 1
    if top_k > 0:
        last = min(last, int(np.searchsorted(np.cumsum(n), top_k, side="left")))       # smallest j with c_1 + ... + c_j >= k
    if p_q16 < P_ONE:
        q_cum = np.cumsum(n[:last + 1] * weights(d[:last + 1], c))
        total = int(q_cum[-1])
        hit = np.nonzero(np.array([int(q) * P_ONE >= p_q16 * total for q in q_cum]))[0]
        last = min(last, int(hit[0]))
    last = min(last, int(np.nonzero(d >= gap)[0][-1]))                # d is descending; class 1 (d = 0 >= gap) always passes
    return v[last], int(n[:last + 1].sum())


def keep_mask(logits: np.ndarray, temperature: float, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0) -> np.ndarray:
    """bool [batch, n_vocab]: the tokens that may be drawn.  `logits` are the rows AFTER the rules of the step (-inf = not allowed),
    any float type holding fp16 values.  A row with nothing allowed keeps nothing."""
    x = np.asarray(logits).astype(np.float16)
    mask = np.zeros(x.shape, dtype=bool)
    for b in range(x.shape[0]):
        allowed = x[b] > -np.inf
        if allowed.any():
            row_cut, _ = cut(x[b][allowed], temperature, top_k, top_p, min_p)
            mask[b] = allowed & (x[b] >= row_cut)
    return mask


def add_arguments(parser) -> None:
    """The three flags run.py, summarize.py and transcribe.py share."""
    parser.add_argument('--top_k', type=int, default=0,
                        help='above temperature 0, draw among the K most likely tokens only (ties at the K-th value are kept; 0 = off)')
    parser.add_argument('--top_p', type=float, default=1.0,
                        help='above temperature 0, draw from the smallest set of most likely tokens whose mass reaches P (nucleus; 1 = off)')
    parser.add_argument('--min_p', type=float, default=0.0,
                        help='above temperature 0, drop tokens less likely than Q times the most likely one (0 = off)')


def options_from_args(top_k=0, top_p=1.0, min_p=0.0) -> dict:
    """The DecodingOptions fields of the three flags (`add_arguments`)."""
    return dict(top_k=int(top_k), top_p=float(top_p), min_p=float(min_p))
