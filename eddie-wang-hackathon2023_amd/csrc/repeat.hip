// wm_repeat_controls: repetition penalty and no-repeat n-grams on the raw logits of a token step (repetition.py states the
// contract).  The launch sits between the decoder launch and wm_greedy_step / wm_beam_step, inside the
// captured step, and only when a control is on.
//
// Per row, H = tokens[sample_begin : cur_len] (m tokens: what the row has sampled; the start sequence and the prompt are not in it):
//   penalty p   every DISTINCT t of H with t < eot, once:  x = fp32(logits[t]);  y = x > 0 ? x / p : x * p  (one fp32 operation,
//               correctly rounded);  logits[t] = fp16(y), round to nearest even.  -inf stays -inf.
//   n-grams n   m >= n - 1: for every i in 0 .. m - n with H[i : i + n - 1] == H[m - n + 1 : m], t = H[i + n - 1] is banned if
//               t < eot: logits[t] = -inf.  Matching runs over H as it is (timestamps included); only text tokens are banned.
// Penalty first, then bans; tokens >= eot (EOT, the specials, the timestamps) are never changed.
//
// One workgroup per row, thread j owns position j of H (m <= REPEAT_THREADS; the entry refuses more).  H is staged once in LDS.
//   phase A  thread j owns the penalty of H[j] only if no j' < j holds the same token: it scans the earlier positions four at a time
//            (every lane of a wave reads the same LDS address: a broadcast, no bank conflict) and stops at the first equal one.  Each
//            logit is read and written by exactly one thread however often its token occurs -- a second application would be wrong,
//            and two threads on one 2-byte element a race.
//   barrier  (__syncthreads is a workgroup-scope release / acquire: a ban stored after it is ordered behind the penalty stored before
//            it by another wave of the workgroup -- both go through the CU's one vector-memory path in issue order -- so -inf wins)
//   phase B  thread i compares its (n - 1)-gram with the suffix (consecutive lanes read consecutive words; the suffix is a broadcast),
//            stops at the first difference and stores -inf.  Equal stores from several threads are benign.
// Indices: H[j] is read for j < m <= tokens_ld - sample_begin only; a logit is touched for 0 <= t < eot <= n_vocab <= row_stride only.
// Logit loads and stores are 2-byte vector accesses (rows may start at any 2-byte address).
#include "kernels.h"
#include "../../include/whisper_mi355.h"

#include <math.h>

namespace wm {
namespace {

constexpr int REPEAT_THREADS = WM_REPEAT_MAX_HISTORY;      // thread j <-> position j of H

struct RepeatParams {
    h16* logits; long ld_row;
    int B, V;
    const int32_t* tokens; int ld_tok;
    int cur_len; const int32_t* t_dev;          // t_dev (optional): cur_len = *t_dev + 1, as greedy.hip reads it
    int sample_begin, eot;
    float penalty; int ngram;
    const int32_t* done;                        // optional [B]: a row whose flag is set is left untouched
};

__global__ __launch_bounds__(REPEAT_THREADS) void repeat_kernel(RepeatParams p) {
    __shared__ __attribute__((aligned(16))) int32_t s_h[REPEAT_THREADS];
    const int b = blockIdx.x, j = threadIdx.x;
    if (p.done && p.done[b]) return;                               // (uniform over the workgroup, like every return before a barrier)
    const int cur_len = p.t_dev ? *p.t_dev + 1 : p.cur_len;       // device step counter holds n_past = cur_len - 1
    int m = min(cur_len, p.ld_tok) - p.sample_begin;              // (the entry has checked both; the clamps keep every index inside
    m = min(m, REPEAT_THREADS);                                    //  the row and the LDS array whatever a device counter holds)
    if (m <= 0) return;
    const int32_t* hist = p.tokens + (size_t)b * p.ld_tok + p.sample_begin;
    h16* lg = p.logits + (size_t)b * p.ld_row;
    const int t = j < m ? hist[j] : -1;
    s_h[j] = t;
    __syncthreads();

    // ---- phase A: the penalty, by the first position that holds the token
    if (p.penalty != 1.0f && t >= 0 && t < p.eot) {
        bool first = true;
        const int4* h4 = (const int4*)s_h;
        for (int q = 0; q < (j >> 2) && first; ++q) {
            const int4 v = h4[q];
            first = v.x != t && v.y != t && v.z != t && v.w != t;
        }
        for (int q = j & ~3; q < j && first; ++q) first = s_h[q] != t;
        if (first) {
            const float x = (float)lg[t];
            // one fp32 operation, rounded on its own, then one conversion: __fdiv_rn is the IEEE division whatever the flags say about
            // reciprocals; mul_rn / f32_as_is keep the compiler from folding product and conversion into one mixed-precision
            // instruction, which rounds once
            const float y = x > 0.f ? __fdiv_rn(x, p.penalty) : mul_rn(x, p.penalty);
            lg[t] = (h16)f32_as_is(y);
        }
    }
    const int n = p.ngram;
    if (n <= 0 || m < n - 1) return;
    __syncthreads();

    // ---- phase B: the bans.  Position i <= m - n: its (n - 1)-gram H[i .. i + n - 2] against the suffix H[m - n + 1 .. m - 1]
    if (j <= m - n) {
        bool match = true;
        for (int k = 0; k < n - 1 && match; ++k) match = s_h[j + k] == s_h[m - n + 1 + k];
        const int u = s_h[j + n - 1];
        if (match && u >= 0 && u < p.eot) lg[u] = (h16)(-INFINITY);
    }
}

}  // namespace
}  // namespace wm

using namespace wm;

extern "C" int wm_repeat_controls(const wm_repeat_io* io, wm_stream_t stream) {
    WM_REQUIRE(io && io->logits && io->tokens, "wm_repeat_controls: null argument");
    WM_REQUIRE(io->batch >= 1 && io->n_vocab >= 1, "wm_repeat_controls: batch=%d n_vocab=%d must be >= 1", io->batch, io->n_vocab);
    WM_REQUIRE(io->row_stride >= io->n_vocab || io->batch == 1, "wm_repeat_controls: row_stride=%lld lets rows of %d logits overlap",
               (long long)io->row_stride, io->n_vocab);
    WM_REQUIRE(io->eot >= 0 && io->eot <= io->n_vocab, "wm_repeat_controls: eot=%d must lie in [0, n_vocab=%d]", io->eot, io->n_vocab);
    WM_REQUIRE(io->repetition_penalty > 0.f && isfinite(io->repetition_penalty),
               "wm_repeat_controls: repetition_penalty=%g must be finite and > 0 (1: off)", (double)io->repetition_penalty);
    WM_REQUIRE(io->no_repeat_ngram_size >= 0, "wm_repeat_controls: no_repeat_ngram_size=%d must be >= 0 (0: off)", io->no_repeat_ngram_size);
    WM_REQUIRE(io->sample_begin >= 0 && io->tokens_ld >= 1 && io->sample_begin <= io->tokens_ld,
               "wm_repeat_controls: sample_begin=%d must lie in [0, tokens_ld=%d]", io->sample_begin, io->tokens_ld);
    // m = cur_len - sample_begin; with a device counter it can reach whatever the rows hold
    const int m_max = (io->n_past_dev ? io->tokens_ld : io->cur_len) - io->sample_begin;
    WM_REQUIRE(io->n_past_dev || (io->cur_len >= io->sample_begin && io->cur_len <= io->tokens_ld),
               "wm_repeat_controls: cur_len=%d must lie in [sample_begin=%d, tokens_ld=%d]", io->cur_len, io->sample_begin, io->tokens_ld);
    WM_REQUIRE(m_max <= WM_REPEAT_MAX_HISTORY, "wm_repeat_controls: a history of %d sampled tokens (%s - sample_begin) exceeds the bound of %d",
               m_max, io->n_past_dev ? "n_past_dev: tokens_ld" : "cur_len", WM_REPEAT_MAX_HISTORY);
    WM_REQUIRE(((uintptr_t)io->logits & 1) == 0 && ((uintptr_t)io->tokens & 3) == 0 && ((uintptr_t)io->n_past_dev & 3) == 0 &&
               ((uintptr_t)io->done & 3) == 0, "wm_repeat_controls: logits must be 2-byte aligned, tokens, n_past_dev and done 4-byte aligned");
    if (io->repetition_penalty == 1.0f && io->no_repeat_ngram_size == 0) return 0;      // both off: nothing is launched
    RepeatParams p{};
    p.logits = (h16*)io->logits; p.ld_row = (long)io->row_stride; p.B = io->batch; p.V = io->n_vocab;
    p.tokens = io->tokens; p.ld_tok = io->tokens_ld; p.cur_len = io->cur_len; p.t_dev = io->n_past_dev;
    p.sample_begin = io->sample_begin; p.eot = io->eot;
    p.penalty = io->repetition_penalty; p.ngram = io->no_repeat_ngram_size; p.done = io->done;
    hipLaunchKernelGGL(repeat_kernel, dim3((unsigned)p.B), dim3(REPEAT_THREADS), 0, (hipStream_t)stream, p);
    WM_LAUNCH_CHECK((hipStream_t)stream, "repeat_controls");
    return 0;
}
