// Device-side sampled token step with top-k / top-p / min-p truncation (wm_sample_step; truncation.py states the contract on the
// host).  A WHOLE token step: it takes the place of wm_greedy_step for calls at temperature > 0 on an instance
// with a control on.  The nucleus is a property of the distribution AFTER Whisper's rules (suppress lists, timestamp rules, the
// text-versus-timestamp decision), and those live inside the step: the decision is made once and serves the weights, the cut and
// the draw.  One workgroup per row, as greedy_kernel; the row (51 865 fp16 logits = 104 KB) is re-read from L2 on each pass:
//   pass 1   greedy_kernel's masked scan, restated line by line: (max, sum-exp, arg-max) of text and timestamps, the decision,
//            m = the maximum of the allowed set A, log Z;
//   pass 2   (top_k or top_p on) level one of a radix selection over the 16-bit monotone key of the fp16 logit: a 256-bin histogram
//            over the HIGH byte of counts (u32) and fixed-point weights (u64), LDS atomics into ONE table per workgroup: the logits
//            of a row crowd into a couple of dozen bins, but a table per wave measured no faster;
//   walk     thread 0, descending from the bin of m: the bin where the k-search crosses;
//   pass 3   level two inside that bin: a 256-bin histogram over the LOW byte -> the class j_k and its mass Q;
//   walk     the p-search on the same level-one table against P * Q; pass 4: level two in its bin if it is another one;
//   pass 5   the Gumbel arg-max over the kept tokens (key >= the cut's, d >= gap: min_p needs no search), their number and their
//            minimum -- the `cut` and `kept` the tests read.
// Counts and weights are integers: the order of accumulation cannot matter, the result depends on the row alone.  No global atomics
// but greedy_kernel's n_done, no workspace, no allocation: capturable.  The logits row is not written (apart from the suppress
// lists, as greedy_kernel writes them); the log-probability booked is that of the untruncated distribution.
#include "common.h"
#include "kernels.h"
#include "logit_rules.h"
#include "sample_rng.h"

namespace wm {

constexpr int SAMPLE_THREADS = 1024;
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / 64;

// ascending 16-bit key of an fp16 value (-0 and +0 are one value)
__device__ __forceinline__ uint32_t f16_key(h16 x) {
    uint32_t b = __builtin_bit_cast(uint16_t, x);
    if (b == 0x8000u) b = 0;
    return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}

// q(v) ~ 2^30 * 2^(d * c), d = fp32(v) - fp32(m) <= 0: truncation.weights, operation by operation.  Every * and + is one correctly
// rounded fp32 operation: no contraction into a fused multiply-add.
__device__ __forceinline__ uint32_t trunc_weight(float d, float c) {
#pragma clang fp contract(off)
    const float s = d * c;
    const float i = rintf(s);
    if (!(i >= -31.f)) return 0;
    const float f = s - i;
    float g = 0x1.44138ap-13f * f + 0x1.5f0890p-10f;
    g = g * f + 0x1.3b2a54p-7f;
    g = g * f + 0x1.c6af6cp-5f;
    g = g * f + 0x1.ebfbe0p-3f;
    g = g * f + 0x1.62e430p-1f;
    const float p = g * f + 1.0f;
    const uint32_t u = (uint32_t)rintf(p * 1073741824.f);
    const int sh = -(int)i;
    return (uint32_t)(((uint64_t)u + ((1ull << sh) >> 1)) >> sh);
}

// f(n, x) for every token of the row, fp16 -> fp32: scalar head up to a 16-byte boundary, 8-wide body, scalar tail (greedy_kernel's walk)
template <typename F>
__device__ __forceinline__ void for_row(const h16* lg, int V, int tid, F f) {
    const int head = min(V, (int)(((16 - ((size_t)lg & 15)) & 15) >> 1));
    for (int n = tid; n < head; n += SAMPLE_THREADS) f(n, lg[n]);
    const int nvec = (V - head) >> 3;
    for (int c = tid; c < nvec; c += SAMPLE_THREADS) {
        const int n0 = head + c * 8;
        const half8v v = *(const half8v*)(lg + n0);
#pragma unroll
        for (int e = 0; e < 8; ++e) f(n0 + e, (h16)v[e]);
    }
    for (int n = head + nvec * 8 + tid; n < V; n += SAMPLE_THREADS) f(n, lg[n]);
}

__global__ __launch_bounds__(SAMPLE_THREADS) void sample_kernel(SampleParams sp) {
    const GreedyParams& p = sp.g;
    __shared__ MS s_ms[2][SAMPLE_WAVES];
    __shared__ AM s_am[2][SAMPLE_WAVES];
    __shared__ int s_info[4], s_hist[SAMPLE_WAVES];
    __shared__ uint32_t s_c1[256], s_c2[256];           // the histograms: level one (high byte), level two (low byte inside one bin)
    __shared__ unsigned long long s_w1[256], s_w2[256];
    __shared__ int s_sel[4];                            // 0: ts_only, 1: bin to refine (-1: none), 2: key of the cut
    __shared__ float s_m;
    __shared__ int s_red_cnt[SAMPLE_WAVES];
    __shared__ float s_red_min[SAMPLE_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, wid = tid >> 6;
    const int cur_len = p.t_dev ? *p.t_dev + 1 : p.cur_len;
    h16* lg = p.logits + (size_t)b * p.ld_row;
    int32_t* toks = p.tokens + (size_t)b * p.ld_tok;
    const RowRules rr = row_rules<SAMPLE_THREADS>(p, lg, toks, cur_len, s_info, s_hist);
    const bool ts_rules = rr.ts_rules;
    const int lo_txt = rr.lo_txt, hi_txt = rr.hi_txt, lo_ts = rr.lo_ts, hi_ts = rr.hi_ts;

    // ---- pass 1: greedy_kernel's scan (greedy.hip), without the perturbed arg-max: the draw waits for the cut -------------------------
    MS txt{-INFINITY, 0.f}, tsm{-INFINITY, 0.f};
    AM atxt{-INFINITY, 0x7fffffff}, ats{-INFINITY, 0x7fffffff};
    {
        auto visit = [&](int n, float x) {
            if (n < hi_txt) { if (n >= lo_txt) { txt = ms_add(txt, x); if (x > atxt.v) atxt = AM{x, n}; } }
            else if (n >= lo_ts && n < hi_ts) { tsm = ms_add(tsm, x); if (x > ats.v) ats = AM{x, n}; }
        };
        auto visit8 = [&](MS& ms, AM& am, int n0, const float (&f)[8]) {
            const float m8 = fmaxf(fmaxf(fmaxf(f[0], f[1]), fmaxf(f[2], f[3])), fmaxf(fmaxf(f[4], f[5]), fmaxf(f[6], f[7])));
            if (m8 == -INFINITY) return;
            if (m8 > ms.m) { ms.s *= __expf(ms.m - m8); ms.m = m8; }
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
        const int head = min(p.V, (int)(((16 - ((size_t)lg & 15)) & 15) >> 1));
        for (int n = tid; n < head; n += SAMPLE_THREADS) visit(n, (float)lg[n]);
        const int nvec = (p.V - head) >> 3;
        for (int c = tid; c < nvec; c += SAMPLE_THREADS) {
            const int n0 = head + c * 8;
            const half8v v = *(const half8v*)(lg + n0);
            float f[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = (float)v[e];
            if (n0 >= lo_txt && n0 + 8 <= hi_txt) visit8(txt, atxt, n0, f);
            else if (n0 >= hi_txt && n0 >= lo_ts && n0 + 8 <= hi_ts) visit8(tsm, ats, n0, f);
            else {
#pragma unroll
                for (int e = 0; e < 8; ++e) visit(n0 + e, f[e]);
            }
        }
        for (int n = head + nvec * 8 + tid; n < p.V; n += SAMPLE_THREADS) visit(n, (float)lg[n]);
    }
    txt = wave_reduce(txt, ms_merge); tsm = wave_reduce(tsm, ms_merge);
    atxt = wave_reduce(atxt, am_merge); ats = wave_reduce(ats, am_merge);
    if ((tid & 63) == 0) { s_ms[0][wid] = txt; s_ms[1][wid] = tsm; s_am[0][wid] = atxt; s_am[1][wid] = ats; }
    __syncthreads();
    float logz = 0.f;                                   // thread 0 keeps it for the bookkeeping
    if (tid < 64) {
        txt = tid < SAMPLE_WAVES ? s_ms[0][tid] : MS{-INFINITY, 0.f}; tsm = tid < SAMPLE_WAVES ? s_ms[1][tid] : MS{-INFINITY, 0.f};
        atxt = tid < SAMPLE_WAVES ? s_am[0][tid] : AM{-INFINITY, 0x7fffffff}; ats = tid < SAMPLE_WAVES ? s_am[1][tid] : AM{-INFINITY, 0x7fffffff};
        txt = wave_reduce(txt, ms_merge); tsm = wave_reduce(tsm, ms_merge);
        atxt = wave_reduce(atxt, am_merge); ats = wave_reduce(ats, am_merge);
        if (tid == 0) {
            bool ts_only = false;
            if (ts_rules) {
                const float lse_ts = (tsm.m == -INFINITY) ? -INFINITY : tsm.m + __logf(tsm.s);
                ts_only = lse_ts > txt.m;
            }
            const MS z = ts_only ? tsm : ms_merge(txt, tsm);
            logz = z.m + logf(z.s);
            s_sel[0] = ts_only;
            s_m = ts_only ? ats.v : fmaxf(atxt.v, ats.v);
        }
    }
    __syncthreads();
    const bool ts_only = s_sel[0] != 0;
    const float m = s_m;                                 // the maximum of A (-inf: nothing is allowed)
    auto allowed = [&](int n) { return n < hi_txt ? (!ts_only && n >= lo_txt) : (n >= lo_ts && n < hi_ts); };

    // ---- the cut of top_k / top_p: the two-level radix selection ---------------------------------------------------------------------
    const bool k_on = sp.top_k > 0, p_on = sp.top_p_q16 < 65536;
    const float c = sp.exp2_scale;
    // a histogram pass: `level` 1 over the high byte of every token of A, 2 over the low byte of the tokens whose high byte is `bin`
    auto histogram = [&](int level, int bin, uint32_t* out_c, unsigned long long* out_w) {
        if (tid < 256) { out_c[tid] = 0; out_w[tid] = 0; }
        __syncthreads();
        for_row(lg, p.V, tid, [&](int n, h16 xh) {
            const float x = (float)xh;
            if (!(x > -INFINITY) || !allowed(n)) return;
            const uint32_t key = f16_key(xh);
            if (level == 2 && (int)(key >> 8) != bin) return;
            const uint32_t slot = level == 1 ? key >> 8 : key & 255u;
            atomicAdd(&out_c[slot], 1u);
            if (p_on) atomicAdd(&out_w[slot], (unsigned long long)trunc_weight(x - m, c));
        });
        __syncthreads();
    };
    if ((k_on || p_on) && m > -INFINITY) {
        const int top = (int)(f16_key((h16)m) >> 8);
        histogram(1, 0, s_c1, s_w1);
        // thread 0's walk state: the count and the weight ABOVE the bin under refinement, the mass Q of the k survivors
        unsigned long long c_above = 0, w_above = 0, q_mass = 0;
        int key_cut = 0;
        if (tid == 0) {
            int bk = -1;
            if (k_on) {
                for (int h = top; h >= 0; --h) {
                    if (c_above + s_c1[h] >= (unsigned long long)sp.top_k) { bk = h; break; }
                    c_above += s_c1[h]; w_above += s_w1[h];
                }
            } else {
                for (int h = top; h >= 0; --h) w_above += s_w1[h];
            }
            s_sel[1] = bk;                               // -1: top_k is off or keeps everything; w_above is then the whole mass
        }
        __syncthreads();
        const int bk = s_sel[1];
        if (bk >= 0) {
            histogram(2, bk, s_c2, s_w2);
            if (tid == 0) {
                unsigned long long cc = c_above, ww = w_above;
                for (int l = 255; l >= 0; --l) {
                    cc += s_c2[l]; ww += s_w2[l];
                    if (cc >= (unsigned long long)sp.top_k) { key_cut = (bk << 8) | l; break; }
                }
                q_mass = ww;
            }
        } else if (tid == 0) q_mass = w_above;
        if (p_on) {
            __syncthreads();                             // (s_sel[1] has been read by everybody)
            const unsigned long long need = (unsigned long long)sp.top_p_q16 * q_mass;
            if (tid == 0) {
                int bp = top;
                w_above = 0;
                for (int h = top; h >= 0; --h) {
                    if (((w_above + s_w1[h]) << 16) >= need) { bp = h; break; }
                    w_above += s_w1[h];
                }
                s_sel[1] = bp;
            }
            __syncthreads();
            const int bp = s_sel[1];
            if (bp != bk) histogram(2, bp, s_c2, s_w2);
            if (tid == 0) {
                unsigned long long ww = w_above;
                for (int l = 255; l >= 0; --l) {
                    ww += s_w2[l];
                    if ((ww << 16) >= need) { key_cut = (bp << 8) | l; break; }
                }
            }
        }
        if (tid == 0) s_sel[2] = key_cut;
    } else if (tid == 0) s_sel[2] = 0;
    __syncthreads();
    const uint32_t key_cut = (uint32_t)s_sel[2];

    // ---- pass 5: the draw among the kept tokens, their number and their minimum -----------------------------------------------------
    const float inv_temp = 1.0f / p.temperature, gap = sp.min_p_gap;
    const uint32_t s_lo = p.seed_dev ? p.seed_dev[0] : p.seed_lo, s_hi = p.seed_dev ? p.seed_dev[1] : p.seed_hi;
    const uint32_t rng_key = fmix32(fmix32(s_lo ^ ((uint32_t)(p.row0 + b) * 0x9e3779b1u)) ^ s_hi ^ ((uint32_t)cur_len * 0x85ebca77u));
    AM best{-INFINITY, 0x7fffffff};
    int n_kept = 0;
    float v_min = INFINITY;
    for_row(lg, p.V, tid, [&](int n, h16 xh) {
        const float x = (float)xh;
        if (!(x > -INFINITY) || !allowed(n)) return;
        if (f16_key(xh) < key_cut || !(x - m >= gap)) return;
        ++n_kept; v_min = fminf(v_min, x);
        const float y = x * inv_temp + gumbel_noise(rng_key, n);
        if (y > best.v) best = AM{y, n};
    });
    best = wave_reduce(best, am_merge);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { n_kept += __shfl_xor(n_kept, o); v_min = fminf(v_min, __shfl_xor(v_min, o)); }
    if ((tid & 63) == 0) { s_am[0][wid] = best; s_red_cnt[wid] = n_kept; s_red_min[wid] = v_min; }
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < SAMPLE_WAVES; ++w) { best = am_merge(best, s_am[0][w]); n_kept += s_red_cnt[w]; v_min = fminf(v_min, s_red_min[w]); }
    if (sp.cut_out) sp.cut_out[b] = n_kept ? v_min : -INFINITY;
    if (sp.kept_out) sp.kept_out[b] = n_kept;

    // ---- bookkeeping and append: greedy_kernel's, the log-probability that of the UNtruncated distribution at T = 1 ----------------
    if (best.i != 0x7fffffff) best.v = (float)lg[best.i];
    const float lp = best.v - logz;
    const int prev = toks[cur_len - 1];
    const bool alive = (prev != p.eot);
    const bool capped = alive && p.row_limit && (cur_len - p.sample_begin >= p.row_limit[b]);
    // a row with no finite allowed logit ends, as in greedy_kernel: EOT at -inf, done, counted
    const bool empty = best.i == 0x7fffffff;
    if (alive && !capped) p.sum_logprobs[b] = empty ? -INFINITY : p.sum_logprobs[b] + lp;
    const int next = (alive && !capped && !empty) ? best.i : p.eot;
    toks[cur_len] = next;
    if (next == p.eot) {
        if (p.n_done) atomicAdd(p.n_done, 1);
        if (p.done) p.done[b] = 1;
    }
}

int launch_sample(const SampleParams& sp, hipStream_t stream) {
    const GreedyParams& p = sp.g;
    WM_REQUIRE(p.t_dev || (p.cur_len >= 1 && p.cur_len < p.ld_tok), "wm_sample_step: cur_len=%d does not fit ld_tok=%d", p.cur_len, p.ld_tok);
    WM_REQUIRE(p.n_suppress == 0 || p.suppress != nullptr, "wm_sample_step: suppress list is null");
    hipLaunchKernelGGL(sample_kernel, dim3(p.B), dim3(SAMPLE_THREADS), 0, stream, sp);
    WM_LAUNCH_CHECK(stream, "wm_sample_step");
    return 0;
}

}  // namespace wm
