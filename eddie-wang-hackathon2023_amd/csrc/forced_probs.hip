// wm_forced_probs: the probability a teacher-forced pass gives the token that follows (word timestamps, decoding.py:
// WhisperDecoding.word_timestamps(token_probs="device")).
//
//   out[b][p] = exp(x[b][p][min(next[b][p], limit - 1)] - logsumexp_{v < limit} x[b][p][v]),     x fp16, out fp32
//
// The PyTorch statement of it copies the [B][n_pos][limit] slab to fp32, reduces it and gathers from it; this kernel reads every
// logit once, as fp16, and writes one float per row.  One workgroup of 256 threads owns a row (b, p):
//   * the row starts at an arbitrary 2-byte offset (V is odd for real vocabularies), so it is read as a scalar head up to the
//     first 16-byte boundary, 16-byte loads (8 logits per lane), and a scalar tail of fewer than 8;
//   * every thread keeps an online (max, sum) pair in fp32: sum = sum_v exp(x_v - max) over the logits it has seen;
//   * the pairs are merged in a fixed order -- the xor butterfly inside a wave (wave_max_nomfma / wave_sum_nomfma), then the four
//     waves' pairs through LDS, summed 0, 1, 2, 3 by thread 0 -- so two runs give the same bits.  No atomics;
//   * a row whose maximum is -inf (every logit below the limit is -inf) gives 0, where the PyTorch statement gives NaN.
// exp inside the sums is the hardware's exp2 of (x - max) * log2(e): the rounding of that product is a relative error of
// |x - max| * 2^-24 in a term that is e^-(max - x) of the largest one.  The one exp of the result and the division are the exact
// ones (expf, IEEE division).
#include "kernels.h"

namespace wm {
namespace {

constexpr int FP_THREADS = 256;
constexpr int FP_WAVES = FP_THREADS / WAVE;
constexpr float FP_LOG2E = 1.4426950408889634f;
#define FP_NEG_INF (-__builtin_inff())

struct fp_pair {
    float m, s;        // running maximum (-inf: nothing finite seen yet) and sum of exp(x - m)
};

// s * exp(m - M) for M >= m; a pair that has seen nothing finite contributes nothing (and -inf - -inf never happens)
__device__ __forceinline__ float fp_rescaled(float m, float s, float M) {
    return m > FP_NEG_INF ? s * __builtin_amdgcn_exp2f((m - M) * FP_LOG2E) : 0.0f;
}

__device__ __forceinline__ void fp_add1(fp_pair& a, float v) {
    if (v > a.m) {
        a.s = fp_rescaled(a.m, a.s, v);
        a.m = v;
    }
    if (a.m > FP_NEG_INF) a.s += __builtin_amdgcn_exp2f((v - a.m) * FP_LOG2E);
}

// eight logits at once, without a branch (the loop below keeps four loads in flight across these): the pair moves to the new
// maximum first -- one more exp2 per eight logits -- and while that maximum is still -inf the sum stays 0
__device__ __forceinline__ void fp_add8(fp_pair& a, const half8v h) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (float)h[k];
    const float cm = fmaxf(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])), fmaxf(fmaxf(v[4], v[5]), fmaxf(v[6], v[7])));
    const float mn = fmaxf(a.m, cm);
    float e[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) e[k] = __builtin_amdgcn_exp2f((v[k] - mn) * FP_LOG2E);
    const float sum = ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
    a.s = mn > FP_NEG_INF ? fp_rescaled(a.m, a.s, mn) + sum : 0.0f;
    a.m = mn;
}

__global__ __launch_bounds__(FP_THREADS) void forced_probs_kernel(const h16* logits, long stride_b, long stride_p, int n_pos,
                                                                  int limit, const int32_t* next, int next_ld, float* out,
                                                                  int out_ld) {
    __shared__ float sh_m[FP_WAVES], sh_s[FP_WAVES];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / n_pos, p = blockIdx.x % n_pos;
    const h16* x = logits + (long)b * stride_b + (long)p * stride_p;

    fp_pair acc = {FP_NEG_INF, 0.0f};
    // head: up to the row's first 16-byte boundary (at most 7 logits)
    int head = (int)(((16 - ((uintptr_t)x & 15)) & 15) / 2);
    if (head > limit) head = limit;
    if (tid < head) fp_add1(acc, (float)x[tid]);
    const int n_chunks = (limit - head) / 8;
    const half8v* x8 = (const half8v*)(x + head);
    int c = tid;
    for (; c + 3 * FP_THREADS < n_chunks; c += 4 * FP_THREADS) {        // four 16-byte loads in flight per lane
        const half8v h0 = x8[c], h1 = x8[c + FP_THREADS], h2 = x8[c + 2 * FP_THREADS], h3 = x8[c + 3 * FP_THREADS];
        fp_add8(acc, h0);
        fp_add8(acc, h1);
        fp_add8(acc, h2);
        fp_add8(acc, h3);
    }
    for (; c < n_chunks; c += FP_THREADS) fp_add8(acc, x8[c]);
    // tail: fewer than 8 logits behind the last 16-byte piece
    const int t = head + n_chunks * 8 + tid;
    if (t < limit) fp_add1(acc, (float)x[t]);

    // wave: the maximum, every lane's sum brought to it, the sum
    const float wm_ = wave_max_nomfma(acc.m);
    const float ws = wave_sum_nomfma(fp_rescaled(acc.m, acc.s, wm_));
    if ((tid & (WAVE - 1)) == 0) {
        sh_m[tid / WAVE] = wm_;
        sh_s[tid / WAVE] = ws;
    }
    __syncthreads();
    if (tid == 0) {
        float M = sh_m[0];
#pragma unroll
        for (int w = 1; w < FP_WAVES; ++w) M = fmaxf(M, sh_m[w]);
        float S = 0.0f;
#pragma unroll
        for (int w = 0; w < FP_WAVES; ++w) S += fp_rescaled(sh_m[w], sh_s[w], M);
        int id = next[(long)b * next_ld + p];
        id = id < 0 ? 0 : id > limit - 1 ? limit - 1 : id;
        float r = 0.0f;
        if (M > FP_NEG_INF) r = expf((float)x[id] - M) / S;
        out[(long)b * out_ld + p] = r;
    }
}

}  // namespace

int launch_forced_probs(const h16* logits, long stride_b, long stride_p, int batch, int n_pos, int limit, const int32_t* next,
                        int next_ld, float* out, int out_ld, hipStream_t stream) {
    hipLaunchKernelGGL(forced_probs_kernel, dim3((unsigned)(batch * n_pos)), dim3(FP_THREADS), 0, stream, logits, stride_b,
                       stride_p, n_pos, limit, next, next_ld, out, out_ld);
    WM_LAUNCH_CHECK(stream, "forced_probs");
    return 0;
}

}  // namespace wm
