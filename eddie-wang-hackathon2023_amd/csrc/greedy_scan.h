// The scan of the greedy token step, shared by greedy_kernel (greedy.hip) and the verify step of speculative decoding
// (speculative.hip): Whisper's rules on one vocabulary row (logit_rules.h), the masked two-class (max, sum-exp) / arg-max sweep, the
// text-versus-timestamp decision and the log-probability of the chosen token.  ONE definition, so that a position verified by
// wm_verify_step books bit for bit what wm_greedy_step books for it: both kernels instantiate this function and nothing else
// touches the arithmetic.  The append, EOT stickiness, row_limit and the done flags stay with each caller.
#pragma once
#include "common.h"
#include "kernels.h"
#include "logit_rules.h"
#include "sample_rng.h"

namespace wm {

constexpr int GREEDY_THREADS = 1024;

struct Pick { int tok; float lp; };              // tok = 0x7fffffff: the row has no finite allowed logit (lp is then not a number to book)

// Called by every thread of a GREEDY_THREADS-wide workgroup that owns the row `lg` with token history `toks` (cur_len tokens) of
// global row p.row0 + b.  The result is valid in thread 0 only.  temperature > 0: the Gumbel-max draw of greedy.hip's header.
__device__ __forceinline__ Pick greedy_pick(const GreedyParams& p, h16* lg, const int32_t* toks, int cur_len, int b) {
    __shared__ MS s_ms[2][GREEDY_THREADS / 64];
    __shared__ AM s_am[4][GREEDY_THREADS / 64];
    __shared__ int s_info[4], s_hist[GREEDY_THREADS / 64];
    const int tid = threadIdx.x;
    // suppress lists, token-history facts and the allowed ranges [lo_txt, hi_txt) U [lo_ts, hi_ts): logit_rules.h
    const RowRules rr = row_rules<GREEDY_THREADS>(p, lg, toks, cur_len, s_info, s_hist);
    const bool ts_rules = rr.ts_rules;
    const int lo_txt = rr.lo_txt, hi_txt = rr.hi_txt, lo_ts = rr.lo_ts, hi_ts = rr.hi_ts;

    MS txt{-INFINITY, 0.f}, tsm{-INFINITY, 0.f};
    AM atxt{-INFINITY, 0x7fffffff}, ats{-INFINITY, 0x7fffffff};
    // sampling: arg-max of the perturbed logits per class (wave-uniform switch; the greedy path is untouched)
    const bool sampling = p.temperature > 0.f;
    const float inv_temp = sampling ? 1.0f / p.temperature : 0.f;
    uint32_t rng_key = 0;
    if (sampling) {
        const uint32_t s_lo = p.seed_dev ? p.seed_dev[0] : p.seed_lo, s_hi = p.seed_dev ? p.seed_dev[1] : p.seed_hi;
        rng_key = fmix32(fmix32(s_lo ^ ((uint32_t)(p.row0 + b) * 0x9e3779b1u)) ^ s_hi ^ ((uint32_t)cur_len * 0x85ebca77u));
    }
    AM ptxt{-INFINITY, 0x7fffffff}, pts{-INFINITY, 0x7fffffff};
    auto perturb = [&](int n, float x) {                           // one token of an allowed class
        if (x == -INFINITY) return;
        const float y = x * inv_temp + gumbel_noise(rng_key, n);
        if (n < hi_txt) { if (y > ptxt.v) ptxt = AM{y, n}; }
        else if (y > pts.v) pts = AM{y, n};
    };
    auto visit = [&](int n, float x) {
        if (n < hi_txt) { if (n >= lo_txt) { txt = ms_add(txt, x); if (x > atxt.v) atxt = AM{x, n}; if (sampling) perturb(n, x); } }
        else if (n >= lo_ts && n < hi_ts) { tsm = ms_add(tsm, x); if (x > ats.v) ats = AM{x, n}; if (sampling) perturb(n, x); }
    };
    // eight logits that all belong to one class: one maximum, at most one rescale of the running sum, eight exponentials --
    // instead of eight dependent (compare, branch, exponential) updates
    auto visit8 = [&](MS& ms, AM& am, int n0, const float (&f)[8]) {
        const float m8 = fmaxf(fmaxf(fmaxf(f[0], f[1]), fmaxf(f[2], f[3])), fmaxf(fmaxf(f[4], f[5]), fmaxf(f[6], f[7])));
        if (m8 == -INFINITY) return;
        if (m8 > ms.m) { ms.s *= __expf(ms.m - m8); ms.m = m8; }         // (first finite value: 0 * exp(-inf) = 0)
        float e[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) e[i] = __expf(f[i] - ms.m);
        ms.s += ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
        if (m8 > am.v) {
            int first_e = 7;
#pragma unroll
            for (int i = 6; i >= 0; --i) if (f[i] == m8) first_e = i;
            am = AM{m8, n0 + first_e};
        }
    };
    // rows are only 2-byte aligned (odd vocabulary): scalar head up to a 16-byte boundary, 8-wide body
    const int head = min(p.V, (int)(((16 - ((size_t)lg & 15)) & 15) >> 1));
    for (int n = tid; n < head; n += GREEDY_THREADS) visit(n, (float)lg[n]);
    const int nvec = (p.V - head) >> 3;
    for (int c = tid; c < nvec; c += GREEDY_THREADS) {
        const int n0 = head + c * 8;
        const half8v v = *(const half8v*)(lg + n0);
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = (float)v[e];
        if (n0 >= lo_txt && n0 + 8 <= hi_txt) {
            visit8(txt, atxt, n0, f);
            if (sampling) {
#pragma unroll
                for (int e = 0; e < 8; ++e) perturb(n0 + e, f[e]);
            }
        } else if (n0 >= hi_txt && n0 >= lo_ts && n0 + 8 <= hi_ts) {
            visit8(tsm, ats, n0, f);
            if (sampling) {
#pragma unroll
                for (int e = 0; e < 8; ++e) perturb(n0 + e, f[e]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) visit(n0 + e, f[e]);
        }
    }
    for (int n = head + nvec * 8 + tid; n < p.V; n += GREEDY_THREADS) visit(n, (float)lg[n]);

    // the four results meet in one exchange: wave-level merges, one LDS round, wave 0 merges the sixteen partial results
    // (thread 0 alone uses them)
    txt = wave_reduce(txt, ms_merge); tsm = wave_reduce(tsm, ms_merge);
    atxt = wave_reduce(atxt, am_merge); ats = wave_reduce(ats, am_merge);
    if (sampling) { ptxt = wave_reduce(ptxt, am_merge); pts = wave_reduce(pts, am_merge); }
    if ((tid & 63) == 0) {
        s_ms[0][tid >> 6] = txt; s_ms[1][tid >> 6] = tsm; s_am[0][tid >> 6] = atxt; s_am[1][tid >> 6] = ats;
        if (sampling) { s_am[2][tid >> 6] = ptxt; s_am[3][tid >> 6] = pts; }
    }
    __syncthreads();
    if (tid >= 64) return Pick{0x7fffffff, 0.f};
    {
        constexpr int NW = GREEDY_THREADS / 64;
        txt = tid < NW ? s_ms[0][tid] : MS{-INFINITY, 0.f}; tsm = tid < NW ? s_ms[1][tid] : MS{-INFINITY, 0.f};
        atxt = tid < NW ? s_am[0][tid] : AM{-INFINITY, 0x7fffffff}; ats = tid < NW ? s_am[1][tid] : AM{-INFINITY, 0x7fffffff};
        txt = wave_reduce(txt, ms_merge); tsm = wave_reduce(tsm, ms_merge);
        atxt = wave_reduce(atxt, am_merge); ats = wave_reduce(ats, am_merge);
        if (sampling) {
            ptxt = tid < NW ? s_am[2][tid] : AM{-INFINITY, 0x7fffffff}; pts = tid < NW ? s_am[3][tid] : AM{-INFINITY, 0x7fffffff};
            ptxt = wave_reduce(ptxt, am_merge); pts = wave_reduce(pts, am_merge);
        }
    }
    if (tid != 0) return Pick{0x7fffffff, 0.f};

    bool ts_only = false;
    if (ts_rules) {
        const float lse_ts = (tsm.m == -INFINITY) ? -INFINITY : tsm.m + __logf(tsm.s);
        ts_only = lse_ts > txt.m;      // logsumexp(ts logprobs) > max(text logprobs)
    }
    AM best = ts_only ? ats : am_merge(atxt, ats);
    if (sampling) {                 // the draw among the allowed tokens; its log-probability is the UNperturbed logit's (T = 1)
        best = ts_only ? pts : am_merge(ptxt, pts);
        if (best.i != 0x7fffffff) best.v = (float)lg[best.i];
    }
    MS z = ts_only ? tsm : ms_merge(txt, tsm);
    const float logz = z.m + logf(z.s);
    return Pick{best.i, best.v - logz};
}

}  // namespace wm
