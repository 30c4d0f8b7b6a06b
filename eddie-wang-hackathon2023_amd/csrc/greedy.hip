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
#include "greedy_scan.h"

namespace wm {

__global__ __launch_bounds__(GREEDY_THREADS) void greedy_kernel(GreedyParams p) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int cur_len = p.t_dev ? *p.t_dev + 1 : p.cur_len;     // device step counter holds n_past = cur_len - 1
    h16* lg = p.logits + (size_t)b * p.ld_row;
    int32_t* toks = p.tokens + (size_t)b * p.ld_tok;
    // the rules, the scan of the row, the decision and the log-probability: greedy_scan.h (shared with speculative.hip)
    const Pick best = greedy_pick(p, lg, toks, cur_len, b);

    if (tid == 0) {
        const float lp = best.lp;
        const int prev = toks[cur_len - 1];
        const bool alive = (prev != p.eot);
        // per-row sample_len: the row has sampled its quota -> it ends here, like the reference's loop at sample_len
        // (no log-probability for the closing EOT, W/decoding.py:794,817-821 + finalize :296-300)
        const bool capped = alive && p.row_limit && (cur_len - p.sample_begin >= p.row_limit[b]);
        // a row with no finite allowed logit ends, as a beam without a live candidate does (beam.hip): EOT at -inf, done, counted
        const bool empty = best.tok == 0x7fffffff;
        if (alive && !capped) p.sum_logprobs[b] = empty ? -INFINITY : p.sum_logprobs[b] + lp;
        const int next = (alive && !capped && !empty) ? best.tok : p.eot;
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
