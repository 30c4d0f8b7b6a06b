// Device-side greedy step: Whisper's logit filters + argmax + log-prob bookkeeping + token append
// in ONE kernel, so that a decode step never returns to the host.
//
// Restates for the device what the reference does in Python on every token (host loops,
// .tolist() and a stream sync per step -- W/decoding.py:785-821):
//   SuppressBlank (W/decoding.py:202-209), SuppressTokens (:212-217, list from :394-421),
//   ApplyTimestampRules (:134-199), GreedyDecoder.update (:274-300).
// One workgroup per utterance; two passes over the vocabulary row (51 865 fp16 logits = 104 KB,
// L2-resident right after the logits GEMM):
//   pass 1: masked running (max, sum-exp) separately for text tokens (< timestamp_begin) and
//           timestamp tokens, plus the arg-max of each class;
//   decide: timestamps win if logsumexp(timestamps) > max(text)  (:191-199; the common log Z
//           cancels), then the next token, its log-probability under the final mask, EOT
//           stickiness and the append.
// temperature > 0 (round 4): the reference draws next ~ Categorical(logits / T) on the host (GreedyDecoder.update, :282-285) and
// books log_softmax(logits)[next] at T = 1.  Here the draw is a Gumbel-max: next = argmax_n (x_n / T + g_n), g_n = -log(-log u_n),
// which has exactly that distribution; u_n comes from a counter-based generator keyed on (seed, global row, position, token), so
// a draw depends on nothing but its own coordinates (not on the batch, the utterance groups or the launch shape), the same
// kernel serves every step of a replayed graph (the seed sits in device memory) and the host can recompute any draw
// (tests/test_gpu_round4.py).  The draws cannot equal torch's generator's: the distribution, the masks and the log-probability
// bookkeeping are what the tests hold to the reference.
#include "common.h"
#include "kernels.h"
#include "logit_rules.h"
#include "sample_rng.h"

namespace wm {

constexpr int GREEDY_THREADS = 1024;

__global__ __launch_bounds__(GREEDY_THREADS) void greedy_kernel(GreedyParams p) {
    __shared__ MS s_ms[2][GREEDY_THREADS / 64];
    __shared__ AM s_am[4][GREEDY_THREADS / 64];
    __shared__ int s_info[4], s_hist[GREEDY_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int cur_len = p.t_dev ? *p.t_dev + 1 : p.cur_len;     // device step counter holds n_past = cur_len - 1
    h16* lg = p.logits + (size_t)b * p.ld_row;
    int32_t* toks = p.tokens + (size_t)b * p.ld_tok;
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
    if (tid >= 64) return;
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

    if (tid == 0) {
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
        const float lp = best.v - logz;
        const int prev = toks[cur_len - 1];
        const bool alive = (prev != p.eot);
        // per-row sample_len: the row has sampled its quota -> it ends here, like the reference's loop at sample_len
        // (no log-probability for the closing EOT, W/decoding.py:794,817-821 + finalize :296-300)
        const bool capped = alive && p.row_limit && (cur_len - p.sample_begin >= p.row_limit[b]);
        // a row with no finite allowed logit ends, as a beam without a live candidate does (beam.hip): EOT at -inf, done, counted
        const bool empty = best.i == 0x7fffffff;
        if (alive && !capped) p.sum_logprobs[b] = empty ? -INFINITY : p.sum_logprobs[b] + lp;
        const int next = (alive && !capped && !empty) ? best.i : p.eot;
        toks[cur_len] = next;
        if (next == p.eot) {
            if (p.n_done) atomicAdd(p.n_done, 1);
            if (p.done) p.done[b] = 1;
        }
    }
}

int launch_greedy(const GreedyParams& p, hipStream_t stream) {
    WM_REQUIRE(p.t_dev || (p.cur_len >= 1 && p.cur_len < p.ld_tok), "greedy: cur_len=%d does not fit ld_tok=%d", p.cur_len, p.ld_tok);
    WM_REQUIRE(p.n_suppress == 0 || p.suppress != nullptr, "greedy: suppress list is null");
    hipLaunchKernelGGL(greedy_kernel, dim3(p.B), dim3(GREEDY_THREADS), 0, stream, p);
    WM_LAUNCH_CHECK(stream, "greedy");
    return 0;
}

// plain arg-max of fp16 rows, first index wins ties (torch.argmax's convention; the kernel-level entry wm_argmax)
__global__ __launch_bounds__(GREEDY_THREADS) void argmax_kernel(const h16* logits, long ld_row, int V, int32_t* ids) {
    __shared__ AM s_am[GREEDY_THREADS / 64];
    const h16* lg = logits + (size_t)blockIdx.x * ld_row;
    AM a{-INFINITY, 0x7fffffff};
    for (int n = threadIdx.x; n < V; n += GREEDY_THREADS) {
        const float x = (float)lg[n];
        if (x > a.v) a = AM{x, n};
    }
    a = block_reduce(a, am_merge, s_am);
    if (threadIdx.x == 0) ids[blockIdx.x] = a.i;
}

int launch_argmax(const h16* logits, long ld_row, int B, int V, int32_t* ids, hipStream_t stream) {
    hipLaunchKernelGGL(argmax_kernel, dim3(B), dim3(GREEDY_THREADS), 0, stream, logits, ld_row, V, ids);
    WM_LAUNCH_CHECK(stream, "argmax");
    return 0;
}

__global__ void step_advance_kernel(int32_t* counter) { if (threadIdx.x == 0 && blockIdx.x == 0) *counter += 1; }

// End of a group's decode step: advance the step counter and rebuild the list of rows still decoding (ascending order:
// ballot + prefix count per wave, wave offsets through LDS).  One workgroup, B <= 1024.
__global__ __launch_bounds__(1024) void step_finish_kernel(int32_t* counter, const int32_t* done, int B, int32_t* live) {
    __shared__ int s_cnt[16];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid == 0 && counter) *counter += 1;
    const bool alive = tid < B && done[tid] == 0;
    const unsigned long long mask = __ballot(alive);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[wid] = __popcll(mask);
    __syncthreads();
    int base = 0, total = 0;
    for (int w = 0; w < 16; ++w) { if (w < wid) base += s_cnt[w]; total += s_cnt[w]; }
    if (alive) live[1 + base + before] = tid;
    if (tid == 0) live[0] = total;
}

int launch_step_finish(int32_t* counter, const int32_t* done, int B, int32_t* live, hipStream_t stream) {
    WM_REQUIRE(done && live && B >= 1 && B <= 1024, "step_finish: null argument or batch %d outside [1, 1024]", B);
    hipLaunchKernelGGL(step_finish_kernel, dim3(1), dim3(1024), 0, stream, counter, done, B, live);
    WM_LAUNCH_CHECK(stream, "step_finish");
    return 0;
}

// the same, and the list of the UTTERANCES (groups of G consecutive rows) that still have a live row
__global__ __launch_bounds__(1024) void step_finish_group_kernel(int32_t* counter, const int32_t* done, int B, int G, int32_t* live, int32_t* live_utt) {
    __shared__ int s_cnt[16];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid == 0 && counter) *counter += 1;
    auto compact = [&](bool alive, int32_t* list) {
        const unsigned long long mask = __ballot(alive);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        __syncthreads();                      // (the counts of the pass before have been read)
        if (lane == 0) s_cnt[wid] = __popcll(mask);
        __syncthreads();
        int base = 0, total = 0;
        for (int w = 0; w < 16; ++w) { if (w < wid) base += s_cnt[w]; total += s_cnt[w]; }
        if (alive) list[1 + base + before] = tid;
        if (tid == 0) list[0] = total;
    };
    compact(tid < B && done[tid] == 0, live);
    bool any = false;
    if (tid < B / G)
        for (int j = 0; j < G; ++j) any |= done[tid * G + j] == 0;
    compact(any, live_utt);
}

int launch_step_finish_group(int32_t* counter, const int32_t* done, int B, int G, int32_t* live, int32_t* live_utt, hipStream_t stream) {
    WM_REQUIRE(done && live && live_utt && B >= 1 && B <= 1024, "step_finish_group: null argument or batch %d outside [1, 1024]", B);
    WM_REQUIRE(G >= 1 && B % G == 0, "step_finish_group: batch %d is not a multiple of the group size %d", B, G);
    hipLaunchKernelGGL(step_finish_group_kernel, dim3(1), dim3(1024), 0, stream, counter, done, B, G, live, live_utt);
    WM_LAUNCH_CHECK(stream, "step_finish_group");
    return 0;
}

int launch_step_advance(int32_t* counter, hipStream_t stream) {
    WM_REQUIRE(counter, "step_advance: null counter");
    hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(64), 0, stream, counter);
    WM_LAUNCH_CHECK(stream, "step_advance");
    return 0;
}

}  // namespace wm
