// Whisper's logit rules for one vocabulary row, shared by the greedy step (greedy.hip) and the beam step (beam.hip):
// the suppress lists written into the row, the token-history facts and the allowed ranges of ApplyTimestampRules, plus the
// (max, sum-exp) / arg-max pair types and their wave reductions.  Integer logic only: both kernels then scan the row themselves.
#pragma once
#include "common.h"
#include "kernels.h"

namespace wm {

struct MS { float m, s; };                       // running max and sum of exp(x - m)
__device__ __forceinline__ MS ms_add(MS a, float x) {
    if (x == -INFINITY) return a;
    if (x > a.m) { a.s = a.s * __expf(a.m - x) + 1.f; a.m = x; }
    else a.s += __expf(x - a.m);
    return a;
}
__device__ __forceinline__ MS ms_merge(MS a, MS b) {
    if (b.m == -INFINITY) return a;
    if (a.m == -INFINITY) return b;
    const float m = fmaxf(a.m, b.m);
    return MS{m, a.s * __expf(a.m - m) + b.s * __expf(b.m - m)};
}
struct AM { float v; int i; };                   // arg-max with first-index tie break
__device__ __forceinline__ AM am_merge(AM a, AM b) {
    if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
    return a;
}

template <typename T, typename F>
__device__ __forceinline__ T wave_reduce(T v, F merge) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        T other;
        // shuffle the struct field-wise (two 32-bit words)
        static_assert(sizeof(T) == 8, "pair types only");
        unsigned long long bits = __builtin_bit_cast(unsigned long long, v);
        unsigned lo = __shfl_xor((unsigned)bits, o), hi = __shfl_xor((unsigned)(bits >> 32), o);
        other = __builtin_bit_cast(T, ((unsigned long long)hi << 32) | lo);
        v = merge(v, other);
    }
    return v;
}
template <typename T, typename F>
__device__ __forceinline__ T block_reduce(T v, F merge, T* scratch) {
    v = wave_reduce(v, merge);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) scratch[wid] = v;
    __syncthreads();
    T r = scratch[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = merge(r, scratch[w]);
    __syncthreads();
    return r;
}

// allowed = [lo_txt, hi_txt) U [lo_ts, hi_ts): every rule of ApplyTimestampRules is a range
struct RowRules { int lo_txt, hi_txt, lo_ts, hi_ts; bool ts_rules; };

// Called by every thread of a THREADS-wide workgroup that owns the row `lg` with token history `toks` (cur_len tokens).
// s_info: int[4], s_hist: int[THREADS / 64] of LDS.  Ends with a barrier that also orders the -inf stores before the caller's scan.
template <int THREADS>
__device__ __forceinline__ RowRules row_rules(const GreedyParams& p, h16* lg, const int32_t* toks, int cur_len, int* s_info, int* s_hist) {
    const int tid = threadIdx.x;
    const int tb = p.timestamp_begin;
    // apply_rules: 0 plain arg-max; 1 SuppressBlank + SuppressTokens + ApplyTimestampRules (the default decoding options);
    // 2 the two suppress filters WITHOUT the timestamp rules -- DecodingOptions.without_timestamps, where the reference builds no
    // ApplyTimestampRules filter (W/decoding.py:337-346) and samples from the whole (suppressed) vocabulary
    const bool lists = p.apply_rules != 0, ts_rules = p.apply_rules == 1;
    const bool first = lists && (cur_len == p.sample_begin);

    // ---- SuppressTokens (+ no_timestamps) and SuppressBlank: written into the logits row, exactly
    // like the reference's in-place filters (decoding.py:202-217); the scan below then sees -inf ----
    if (lists) {
        const h16 ninf = (h16)(-INFINITY);
        for (int i = tid; i < p.n_suppress; i += THREADS) lg[p.suppress[i]] = ninf;
        if (first) for (int i = tid; i < p.n_blank; i += THREADS) lg[p.blank[i]] = ninf;
    }
    // ---- token-history facts: last / penultimate sampled token, last timestamp.  Every thread looks at one sampled token
    // (a backwards scan by one thread was a chain of dependent loads: up to one L2 round trip per sampled token) ------------
    const int n_sampled = cur_len - p.sample_begin;
    int my_rel = -1, my_tok = -1;                  // this thread's latest timestamp among the sampled tokens it looked at
    if (ts_rules) {
        for (int j = tid; j < n_sampled; j += THREADS) {
            const int t = toks[p.sample_begin + j];
            if (t >= tb) { my_rel = j; my_tok = t; }
            if (j == n_sampled - 1) s_info[0] = t >= tb;
            if (j == n_sampled - 2) s_info[1] = t >= tb;
        }
    }
    {
        int r = my_rel;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) r = max(r, __shfl_xor(r, o));
        if ((tid & 63) == 0) s_hist[tid >> 6] = r;
    }
    __syncthreads();                       // also orders the -inf stores above before the scan
    int rel_last = -1;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) rel_last = max(rel_last, s_hist[w]);
    if (rel_last >= 0 && my_rel == rel_last) s_info[2] = my_tok;          // exactly one thread holds that position
    __syncthreads();
    const bool last_ts = ts_rules && n_sampled >= 1 && s_info[0];
    const bool pen_ts = ts_rules && (n_sampled < 2 || s_info[1]);
    int ts_last = rel_last >= 0 ? s_info[2] : -1;
    if (ts_last >= 0 && !(last_ts && !pen_ts)) ts_last += 1;

    RowRules r{0, ts_rules ? tb : p.V, ts_rules ? tb : p.V, p.V, ts_rules};
    if (ts_rules) {
        if (first) { r.hi_txt = 0; if (p.max_initial_ts >= 0) r.hi_ts = min(r.hi_ts, tb + p.max_initial_ts + 1); }
        if (last_ts) { if (pen_ts) r.lo_ts = p.V; else r.lo_txt = max(r.lo_txt, p.eot); }
        if (ts_last >= 0) r.lo_ts = max(r.lo_ts, ts_last);
    }
    return r;
}

}  // namespace wm
