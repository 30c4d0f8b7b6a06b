// wm_sequence_bias: hotwords and sequence bias on the raw logits of a token step (biasing.py states the contract and builds the table,
// DESIGN.md section 5k).  The launch sits behind wm_repeat_controls and in front of wm_greedy_step / wm_beam_step, inside the captured
// step, and only on an instance built with a bias.
//
// The table: items (target, k, offset, bias) sorted by (target ascending, k descending) and a pool of prefix tokens.  Per row, with
// H = tokens[sample_begin : cur_len] (m tokens: what the row has sampled), item i MATCHES if H[m - k : m] == pool[offset : offset + k]
// (k = 0: always).  Per target the first matching item in table order wins -- the greatest k, the earlier item at equal k -- and
//   x = fp32(logits[target]);  y = x + bias  (one fp32 addition);  logits[target] = fp16(y), round to nearest even.  -inf stays -inf.
// Biases are never summed: one update per token.
//
// One workgroup of BIAS_THREADS per row; H is staged once in LDS; threads stride over the items.
//   pass 1   thread of item i compares the suffix of H (LDS) with the item's prefix (neighbouring items read the same pool region: L2)
//            and writes ONE word to LDS: the target if the item matches, ~target if it does not, INERT if the item is not to be used.
//   barrier
//   pass 2   a matching item walks back over its target's segment (the words that hold target or ~target): it is the winner iff none
//            of them matched.  Only the winner reads and writes the logit, so every 2-byte element is touched by at most one thread of
//            the launch -- a second application of a bias would be wrong, and two threads on one element a race.
// On a table that is not sorted a target may have two segments and two winners: the results are unspecified, the indices are not.
// Indices, whatever the table and the device words hold: items i < n <= capacity <= WM_BIAS_MAX_ITEMS only; an item is INERT unless
// 0 <= target < eot, 0 <= k <= min(WM_BIAS_MAX_K, m) and 0 <= offset <= pool_capacity - k, so pool[offset + q] and H[m - k + q] are
// read for q < k only; H[j] for j < m <= min(tokens_ld - sample_begin, WM_REPEAT_MAX_HISTORY); a logit for 0 <= t < eot <= n_vocab.
// Logit loads and stores are 2-byte vector accesses (rows may start at any 2-byte address).
#include "kernels.h"
#include "../../include/whisper_mi355.h"

#include <limits.h>

namespace wm {
namespace {

constexpr int BIAS_THREADS = 256;
constexpr int32_t INERT = INT_MIN;          // never equal to a target (>= 0) or to ~target (>= -n_vocab)

struct BiasParams {
    h16* logits; long ld_row;
    int B, V;
    const int32_t* tokens; int ld_tok;
    int cur_len; const int32_t* t_dev;          // t_dev (optional): cur_len = *t_dev + 1, as greedy.hip reads it
    int sample_begin, eot;
    const int32_t* done;                        // optional [B]: a row whose flag is set is left untouched
    const int4* items; const int32_t* pool;     // (target, k, offset, bias bits)
    int cap, pool_cap;
    const int32_t* n_dev;                       // optional: the items in use
};

__global__ __launch_bounds__(BIAS_THREADS) void bias_kernel(BiasParams p) {
    __shared__ int32_t s_h[WM_REPEAT_MAX_HISTORY];
    __shared__ int32_t s_tgt[WM_BIAS_MAX_ITEMS];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (p.done && p.done[b]) return;                               // (uniform over the workgroup, like every return before a barrier)
    const int n = max(0, min(p.n_dev ? *p.n_dev : p.cap, p.cap));  // (the entry has checked cap; the clamp holds whatever the word holds)
    if (n == 0) return;
    const int cur_len = p.t_dev ? *p.t_dev + 1 : p.cur_len;       // device step counter holds n_past = cur_len - 1
    const int m = max(0, min(min(cur_len, p.ld_tok) - p.sample_begin, WM_REPEAT_MAX_HISTORY));
    const int32_t* hist = p.tokens + (size_t)b * p.ld_tok + p.sample_begin;
    h16* lg = p.logits + (size_t)b * p.ld_row;
    for (int j = tid; j < m; j += BIAS_THREADS) s_h[j] = hist[j];
    __syncthreads();

    // ---- pass 1: which items match
    for (int i = tid; i < n; i += BIAS_THREADS) {
        const int4 it = p.items[i];
        const int t = it.x, k = it.y, off = it.z;
        int32_t word = INERT;
        if (t >= 0 && t < p.eot && k >= 0 && k <= WM_BIAS_MAX_K && off >= 0 && off <= p.pool_cap - k) {
            bool match = k <= m;
            for (int q = 0; q < k && match; ++q) match = s_h[m - k + q] == p.pool[off + q];
            word = match ? t : ~t;
        }
        s_tgt[i] = word;
    }
    __syncthreads();

    // ---- pass 2: the first matching item of a target's segment owns the logit
    for (int i = tid; i < n; i += BIAS_THREADS) {
        const int32_t t = s_tgt[i];
        if (t < 0) continue;
        bool first = true;
        for (int j = i - 1; j >= 0 && first; --j) {
            const int32_t w = s_tgt[j];
            if (w == t) first = false;
            else if (w != ~t) break;
        }
        if (first) {
            const float x = (float)lg[t];
            // one fp32 addition, rounded on its own, then one conversion: f32_as_is keeps the compiler from folding sum and conversion
            // into one mixed-precision instruction, which rounds once
            const float y = f32_as_is(x + __int_as_float(p.items[i].w));
            lg[t] = (h16)y;
        }
    }
}

}  // namespace
}  // namespace wm

using namespace wm;

extern "C" int wm_sequence_bias(const wm_bias_io* io, wm_stream_t stream) {
    WM_REQUIRE(io && io->logits && io->tokens, "wm_sequence_bias: null argument");
    WM_REQUIRE(io->batch >= 1 && io->n_vocab >= 1, "wm_sequence_bias: batch=%d n_vocab=%d must be >= 1", io->batch, io->n_vocab);
    WM_REQUIRE(io->row_stride >= io->n_vocab || io->batch == 1, "wm_sequence_bias: row_stride=%lld lets rows of %d logits overlap",
               (long long)io->row_stride, io->n_vocab);
    WM_REQUIRE(io->eot >= 0 && io->eot <= io->n_vocab, "wm_sequence_bias: eot=%d must lie in [0, n_vocab=%d]", io->eot, io->n_vocab);
    WM_REQUIRE(io->sample_begin >= 0 && io->tokens_ld >= 1 && io->sample_begin <= io->tokens_ld,
               "wm_sequence_bias: sample_begin=%d must lie in [0, tokens_ld=%d]", io->sample_begin, io->tokens_ld);
    // m = cur_len - sample_begin; with a device counter it can reach whatever the rows hold
    const int m_max = (io->n_past_dev ? io->tokens_ld : io->cur_len) - io->sample_begin;
    WM_REQUIRE(io->n_past_dev || (io->cur_len >= io->sample_begin && io->cur_len <= io->tokens_ld),
               "wm_sequence_bias: cur_len=%d must lie in [sample_begin=%d, tokens_ld=%d]", io->cur_len, io->sample_begin, io->tokens_ld);
    WM_REQUIRE(m_max <= WM_REPEAT_MAX_HISTORY, "wm_sequence_bias: a history of %d sampled tokens (%s - sample_begin) exceeds the bound of %d",
               m_max, io->n_past_dev ? "n_past_dev: tokens_ld" : "cur_len", WM_REPEAT_MAX_HISTORY);
    WM_REQUIRE(io->capacity >= 0 && io->capacity <= WM_BIAS_MAX_ITEMS, "wm_sequence_bias: capacity=%d must lie in [0, %d]", io->capacity,
               WM_BIAS_MAX_ITEMS);
    WM_REQUIRE(io->pool_capacity >= 0 && io->pool_capacity <= WM_BIAS_MAX_POOL, "wm_sequence_bias: pool_capacity=%d must lie in [0, %d]",
               io->pool_capacity, WM_BIAS_MAX_POOL);
    WM_REQUIRE(io->capacity == 0 || (io->items && io->pool), "wm_sequence_bias: null items or pool with capacity=%d", io->capacity);
    WM_REQUIRE(((uintptr_t)io->logits & 1) == 0 && ((uintptr_t)io->tokens & 3) == 0 && ((uintptr_t)io->n_past_dev & 3) == 0 &&
               ((uintptr_t)io->done & 3) == 0, "wm_sequence_bias: logits must be 2-byte aligned, tokens, n_past_dev and done 4-byte aligned");
    WM_REQUIRE(((uintptr_t)io->items & 15) == 0 && ((uintptr_t)io->pool & 3) == 0 && ((uintptr_t)io->n_items_dev & 3) == 0,
               "wm_sequence_bias: items must be 16-byte aligned, pool and n_items_dev 4-byte aligned");
    if (io->capacity == 0 || io->eot == 0) return 0;                                    // an empty table, no text token: nothing is launched
    BiasParams p{};
    p.logits = (h16*)io->logits; p.ld_row = (long)io->row_stride; p.B = io->batch; p.V = io->n_vocab;
    p.tokens = io->tokens; p.ld_tok = io->tokens_ld; p.cur_len = io->cur_len; p.t_dev = io->n_past_dev;
    p.sample_begin = io->sample_begin; p.eot = io->eot; p.done = io->done;
    p.items = (const int4*)io->items; p.pool = io->pool; p.cap = io->capacity; p.pool_cap = io->pool_capacity; p.n_dev = io->n_items_dev;
    hipLaunchKernelGGL(bias_kernel, dim3((unsigned)p.B), dim3(BIAS_THREADS), 0, (hipStream_t)stream, p);
    WM_LAUNCH_CHECK((hipStream_t)stream, "sequence_bias");
    return 0;
}
