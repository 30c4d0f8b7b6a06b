// Device-side beam search step (upstream Whisper's BeamSearchDecoder.update; the contract is restated in
// include/whisper_mi355.h at wm_beam_io) and the self-attention cache reorder that follows it.  Like the greedy step it
// runs between two decoder launches of every token, reads the device step counter and never returns to the host.
//
// wm_beam_step is two launches:
//   beam_propose_kernel  one workgroup per row: the masking of the greedy kernel (logit_rules.h), one scan for the
//                        (max, sum-exp) of the text and timestamp classes, then beam_size + 1 rounds of "the best allowed
//                        logit after the previous pick" under (value descending, token ascending).  The row (51 865 fp16 =
//                        104 KB) is L2-resident right after the logits GEMM; a thread keeps its 51 logits in registers
//                        across the beam_size + 2 scans (wider vocabularies than 57 344 are re-read from L2).
//   beam_merge_kernel    one workgroup per utterance: ranks the at most 8 x 9 proposals under the total order (score
//                        descending, parent beam ascending, token ascending), walks them (EOT -> finished list, others
//                        -> next live beams), stages the beams' token histories in LDS (8 x 449 int32 = 14.4 KB) so that
//                        the move is safe in place, and maintains the pool and the completion flags.
// wm_kv_reorder (kv_reorder_kernel): row i of every layer's cache takes row parent[i]'s positions 0 .. n.  A workgroup owns
// the same (layer, K-or-V, head set) slice of ALL beams of one utterance; each thread loads its 16 bytes of every beam that
// moves, then stores them -- nobody else touches those bytes, so the copy needs no second cache set and no barrier.
#include "common.h"
#include "kernels.h"
#include "logit_rules.h"
#include "whisper_mi355.h"

namespace wm {

constexpr int BEAM_THREADS = 1024, MERGE_THREADS = 256, REORDER_THREADS = 256, REORDER_HEAD_SPLIT = 4;
constexpr int BEAM_CAND_MAX = BEAM_MAX * (BEAM_MAX + 1);
constexpr int PROPOSE_CHUNKS = 7;            // 16-byte pieces of the logits row a thread of beam_propose_kernel keeps in registers

// every logit of a row, each thread in ascending token order.  Rows are only 2-byte aligned (odd vocabulary): scalar head up
// to a 16-byte boundary, 8-wide body, scalar tail
template <typename F>
__device__ __forceinline__ void for_each_logit(const h16* lg, int V, F f) {
    const int tid = threadIdx.x;
    const int head = min(V, (int)(((16 - ((size_t)lg & 15)) & 15) >> 1));
    for (int n = tid; n < head; n += BEAM_THREADS) f(n, (float)lg[n]);
    const int nvec = (V - head) >> 3;
    for (int c = tid; c < nvec; c += BEAM_THREADS) {
        const int n0 = head + c * 8;
        const half8v v = *(const half8v*)(lg + n0);
#pragma unroll
        for (int e = 0; e < 8; ++e) f(n0 + e, (float)v[e]);
    }
    for (int n = head + nvec * 8 + tid; n < V; n += BEAM_THREADS) f(n, (float)lg[n]);
}

__global__ __launch_bounds__(BEAM_THREADS) void beam_propose_kernel(BeamParams p) {
    __shared__ MS s_ms[BEAM_THREADS / 64];
    __shared__ AM s_am[BEAM_THREADS / 64];
    __shared__ int s_info[4], s_hist[BEAM_THREADS / 64];
    const GreedyParams& g = p.g;
    const int b = blockIdx.x, tid = threadIdx.x, K = p.K;
    const int cur_len = g.t_dev ? *g.t_dev + 1 : g.cur_len;
    if (g.done[b]) return;                                        // frozen utterance
    if (cur_len == g.sample_begin && b % K != 0) return;          // first sampled step: the beams are identical, beam 0 proposes
    h16* lg = g.logits + (size_t)b * g.ld_row;
    const int32_t* toks = g.tokens + (size_t)b * g.ld_tok;
    BeamCand* out = p.cand + (size_t)b * (K + 1);

    RowRules rr = row_rules<BEAM_THREADS>(g, lg, toks, cur_len, s_info, s_hist);
    // The row is scanned beam_size + 2 times: a thread keeps its share in registers (one head and one tail element, PROPOSE_CHUNKS
    // 16-byte pieces: vocabularies up to 57 344, Whisper's has 51 865) and reads L2 once; wider rows are re-read every time.
    const int head = min(g.V, (int)(((16 - ((size_t)lg & 15)) & 15) >> 1)), nvec = (g.V - head) >> 3, n_tail = g.V - head - nvec * 8;
    const bool cached = nvec <= PROPOSE_CHUNKS * BEAM_THREADS;                // workgroup-uniform
    half8v piece[PROPOSE_CHUNKS];
    float x_head = -INFINITY, x_tail = -INFINITY;
    if (cached) {
        if (tid < head) x_head = (float)lg[tid];
#pragma unroll
        for (int k = 0; k < PROPOSE_CHUNKS; ++k)
            if (tid + k * BEAM_THREADS < nvec) piece[k] = *(const half8v*)(lg + head + (tid + k * BEAM_THREADS) * 8);
        if (tid < n_tail) x_tail = (float)lg[head + nvec * 8 + tid];
    }
    auto scan = [&](auto f) {               // every logit of the row, each thread in ascending token order
        if (!cached) { for_each_logit(lg, g.V, f); return; }
        if (tid < head) f(tid, x_head);
#pragma unroll
        for (int k = 0; k < PROPOSE_CHUNKS; ++k) {
            const int c = tid + k * BEAM_THREADS;
            if (c < nvec) {
#pragma unroll
                for (int e = 0; e < 8; ++e) f(head + c * 8 + e, (float)piece[k][e]);
            }
        }
        if (tid < n_tail) f(head + nvec * 8 + tid, x_tail);
    };
    MS txt{-INFINITY, 0.f}, tsm{-INFINITY, 0.f};
    scan([&](int n, float x) {
        if (n < rr.hi_txt) { if (n >= rr.lo_txt) txt = ms_add(txt, x); }
        else if (n >= rr.lo_ts && n < rr.hi_ts) tsm = ms_add(tsm, x);
    });
    txt = block_reduce(txt, ms_merge, s_ms);
    tsm = block_reduce(tsm, ms_merge, s_ms);
    bool ts_only = false;
    if (rr.ts_rules) {                     // logsumexp(timestamps) > max(text): only timestamps may follow (the common log Z cancels)
        const float lse_ts = (tsm.m == -INFINITY) ? -INFINITY : tsm.m + __logf(tsm.s);
        ts_only = lse_ts > txt.m;
    }
    const MS z = ts_only ? tsm : ms_merge(txt, tsm);
    const float logz = z.m + logf(z.s);
    if (ts_only) rr.lo_txt = rr.hi_txt;    // (hi_txt stays the class boundary)

    AM prev{INFINITY, -1};
    for (int r = 0; r <= K; ++r) {
        AM best{-INFINITY, 0x7fffffff};
        scan([&](int n, float x) {
            const bool allowed = n < rr.hi_txt ? n >= rr.lo_txt : (n >= rr.lo_ts && n < rr.hi_ts);
            const bool after = x < prev.v || (x == prev.v && n > prev.i);
            if (allowed && after && x > best.v) best = AM{x, n};          // (x > -inf: masked logits are never proposed)
        });
        best = block_reduce(best, am_merge, s_am);
        const bool none = best.i == 0x7fffffff;                           // workgroup-uniform
        if (tid == 0) {
            if (none) for (int q = r; q <= K; ++q) out[q] = BeamCand{-INFINITY, -1};
            else out[r] = BeamCand{best.v - logz, best.i};
        }
        if (none) break;
        prev = best;
    }
}

// does candidate (sa, ba, ta) come before (sb, bb, tb)?  score descending, beam ascending, token ascending; absent ones last
__device__ __forceinline__ bool cand_before(float sa, int ba, int ta, float sb, int bb, int tb) {
    if ((ta < 0) != (tb < 0)) return tb < 0;
    if (ta >= 0 && sa != sb) return sa > sb;
    if (ba != bb) return ba < bb;
    return ta < tb;
}

__global__ __launch_bounds__(MERGE_THREADS) void beam_merge_kernel(BeamParams p) {
    extern __shared__ int32_t s_tokens[];                     // [K][ld_tok]: the beams' histories before the move
    __shared__ float s_score[BEAM_CAND_MAX];
    __shared__ int s_beam[BEAM_CAND_MAX], s_tok[BEAM_CAND_MAX], s_order[BEAM_CAND_MAX];
    __shared__ int s_new[BEAM_MAX], s_fin[BEAM_MAX], s_n[3];   // walk results; s_n = {live, pooled this step, pool count before}
    const GreedyParams& g = p.g;
    const int a = blockIdx.x, tid = threadIdx.x, K = p.K, r0 = a * K, ld = g.ld_tok;
    const int cur_len = g.t_dev ? *g.t_dev + 1 : g.cur_len;
    int32_t* toks = g.tokens + (size_t)r0 * ld;
    if (g.done[r0]) {                                        // frozen: nothing moves
        if (tid < K) p.parent[r0 + tid] = r0 + tid;
        return;
    }
    if (g.row_limit && cur_len - g.sample_begin >= g.row_limit[r0]) {      // the utterance has sampled its quota: frozen before the step
        if (tid < K) { p.parent[r0 + tid] = r0 + tid; g.done[r0 + tid] = 1; }
        if (tid == 0) { p.live_len[a] = cur_len; if (g.n_done) atomicAdd(g.n_done, K); }
        return;
    }
    const int n_prop = cur_len == g.sample_begin ? 1 : K, NC = n_prop * (K + 1);
    if (tid < NC) {
        const int beam = tid / (K + 1);
        const BeamCand c = p.cand[(size_t)(r0 + beam) * (K + 1) + tid % (K + 1)];
        s_score[tid] = g.sum_logprobs[r0 + beam] + c.lp; s_beam[tid] = beam; s_tok[tid] = c.tok;
    }
    if (tid < BEAM_CAND_MAX) s_order[tid] = 0;              // (NaN scores would leave ranks unassigned: never an index out of range)
    for (int j = 0; j < K; ++j)
        for (int t = tid; t < cur_len; t += MERGE_THREADS) s_tokens[j * ld + t] = toks[(size_t)j * ld + t];
    __syncthreads();
    if (tid < NC) {                                          // rank by counting: the keys (beam, token) are distinct
        int rank = 0;
        for (int o = 0; o < NC; ++o)
            rank += cand_before(s_score[o], s_beam[o], s_tok[o], s_score[tid], s_beam[tid], s_tok[tid]) ? 1 : 0;
        s_order[rank] = tid;
    }
    __syncthreads();
    if (tid == 0) {
        int n_live = 0, n_fin = 0;
        for (int i = 0; i < NC && n_live < K; ++i) {
            const int c = s_order[i];
            if (s_tok[c] < 0) break;
            if (s_tok[c] == g.eot) { if (n_fin < BEAM_MAX) s_fin[n_fin++] = c; }
            else s_new[n_live++] = c;
        }
        const int before = p.fin_count[a];
        s_n[0] = n_live; s_n[1] = max(0, min(n_fin, p.max_cand - before)); s_n[2] = before;
    }
    __syncthreads();
    const int n_live = s_n[0], n_add = s_n[1], before = s_n[2];
    // the pool: history + EOT of the step's best finished candidates
    for (int e = 0; e < n_add; ++e) {
        const int c = s_fin[e], slot = before + e;
        int32_t* dst = p.fin_tokens + ((size_t)a * p.max_cand + slot) * ld;
        for (int t = tid; t < cur_len; t += MERGE_THREADS) dst[t] = s_tokens[s_beam[c] * ld + t];
        if (tid == 0) {
            dst[cur_len] = g.eot;
            p.fin_scores[a * p.max_cand + slot] = s_score[c];
            p.fin_len[a * p.max_cand + slot] = cur_len + 1;
        }
    }
    // the next live beams (a row with fewer finite proposals than the contract assumes ends: EOT at -inf)
    for (int i = 0; i < K; ++i) {
        const bool have = i < n_live;
        const int c = have ? s_new[i] : 0, pb = have ? s_beam[c] : i;
        if (pb != i)
            for (int t = tid; t < cur_len; t += MERGE_THREADS) toks[(size_t)i * ld + t] = s_tokens[pb * ld + t];
        if (tid == 0) {
            toks[(size_t)i * ld + cur_len] = have ? s_tok[c] : g.eot;
            g.sum_logprobs[r0 + i] = have ? s_score[c] : -INFINITY;
            p.parent[r0 + i] = r0 + pb;
        }
    }
    if (tid == 0) {
        p.fin_count[a] = before + n_add;
        if (!p.ignore_eot && before + n_add >= p.max_cand) {      // the pool is full: the utterance is complete, frozen from here on
            for (int j = 0; j < K; ++j) g.done[r0 + j] = 1;
            p.live_len[a] = cur_len + 1;
            if (g.n_done) atomicAdd(g.n_done, K);
        }
    }
}

int launch_beam_step(const BeamParams& p, hipStream_t stream) {
    const GreedyParams& g = p.g;
    WM_REQUIRE(p.K >= 1 && p.K <= BEAM_MAX, "beam: beam_size %d outside [1, %d]", p.K, BEAM_MAX);
    WM_REQUIRE(p.max_cand >= 1 && p.max_cand <= BEAM_POOL_MAX, "beam: max_candidates %d outside [1, %d]", p.max_cand, BEAM_POOL_MAX);
    WM_REQUIRE(g.B >= p.K && g.B % p.K == 0, "beam: %d rows are not a multiple of beam_size %d", g.B, p.K);
    WM_REQUIRE(g.t_dev || (g.cur_len >= 1 && g.cur_len < g.ld_tok), "beam: cur_len=%d does not fit ld_tok=%d", g.cur_len, g.ld_tok);
    WM_REQUIRE(g.n_suppress == 0 || g.suppress != nullptr, "beam: suppress list is null");
    const size_t lds = (size_t)p.K * g.ld_tok * sizeof(int32_t);
    WM_REQUIRE(lds <= 48 * 1024, "beam: %d beams x %d tokens do not fit the history staging buffer", p.K, g.ld_tok);
    hipLaunchKernelGGL(beam_propose_kernel, dim3(g.B), dim3(BEAM_THREADS), 0, stream, p);
    WM_LAUNCH_CHECK(stream, "beam_propose");
    hipLaunchKernelGGL(beam_merge_kernel, dim3(g.B / p.K), dim3(MERGE_THREADS), lds, stream, p);
    WM_LAUNCH_CHECK(stream, "beam_merge");
    return 0;
}

__global__ __launch_bounds__(REORDER_THREADS) void kv_reorder_kernel(KvReorderParams p) {
    const int a = blockIdx.z, K = p.K, r0 = a * K, tid = threadIdx.x;
    if (p.done && p.done[r0]) return;                        // a complete utterance decodes no further
    int par[BEAM_MAX];
    bool moves = false;
#pragma unroll
    for (int j = 0; j < BEAM_MAX; ++j) {
        int q = j < K ? p.parent[r0 + j] - r0 : j;
        if (q < 0 || q >= K) q = j;                          // never reach into another utterance's rows
        par[j] = q;
        moves |= q != j;
    }
    if (!moves) return;
    const int n = min(p.cap, (p.t_dev ? *p.t_dev : p.n_last) + 1);          // positions 0 .. n - 1
    const size_t slice = (size_t)p.cap * 64 * p.elem_bytes, row_stride = 2 * (size_t)p.H * slice;
    const int bytes = n * 64 * p.elem_bytes;                // contiguous per (row, K-or-V, head), a multiple of 64
    const int layer = blockIdx.y >> 1, kv = blockIdx.y & 1;
    char* base = (char*)p.layers[layer] + (size_t)r0 * row_stride + (size_t)kv * p.H * slice;
    for (int h = blockIdx.x; h < p.H; h += gridDim.x) {
        for (int off = tid * 16; off < bytes; off += REORDER_THREADS * 16) {
            char* q = base + (size_t)h * slice + off;
            uint4 v[BEAM_MAX];
#pragma unroll
            for (int j = 0; j < BEAM_MAX; ++j)
                if (j < K && par[j] != j) v[j] = *(const uint4*)(q + (size_t)par[j] * row_stride);
#pragma unroll
            for (int j = 0; j < BEAM_MAX; ++j)
                if (j < K && par[j] != j) *(uint4*)(q + (size_t)j * row_stride) = v[j];
        }
    }
}

int launch_kv_reorder(const KvReorderParams& p, hipStream_t stream) {
    WM_REQUIRE(p.layers && p.parent && p.n_layer >= 1, "kv_reorder: null argument");
    WM_REQUIRE(p.K >= 1 && p.K <= BEAM_MAX, "kv_reorder: beam_size %d outside [1, %d]", p.K, BEAM_MAX);
    WM_REQUIRE(p.rows >= p.K && p.rows % p.K == 0, "kv_reorder: %d rows are not a multiple of beam_size %d", p.rows, p.K);
    WM_REQUIRE(p.elem_bytes == 1 || p.elem_bytes == 2, "kv_reorder: elem_bytes %d is neither int8 nor fp16", p.elem_bytes);
    WM_REQUIRE(p.H >= 1 && p.cap >= 1 && (p.t_dev || (p.n_last >= 0 && p.n_last < p.cap)),
               "kv_reorder: position %d outside the cache capacity %d", p.n_last, p.cap);
    WM_REQUIRE(p.n_layer * 2 <= 65535 && p.rows / p.K <= 65535, "kv_reorder: grid too large");
    if (p.K == 1) return 0;                                  // one beam has no other parent
    hipLaunchKernelGGL(kv_reorder_kernel, dim3(min(p.H, REORDER_HEAD_SPLIT), p.n_layer * 2, p.rows / p.K), dim3(REORDER_THREADS), 0,
                       stream, p);
    WM_LAUNCH_CHECK(stream, "kv_reorder");
    return 0;
}

}  // namespace wm

using namespace wm;

size_t wm_beam_workspace_bytes(int batch, int beam_size) {
    return batch > 0 && beam_size > 0 ? (size_t)batch * (beam_size + 1) * sizeof(BeamCand) : 0;
}

int wm_beam_step(const wm_beam_io* io, wm_stream_t stream) {
    WM_REQUIRE(io && io->logits && io->tokens && io->sum_logprobs && io->parent && io->fin_tokens && io->fin_scores && io->fin_len &&
               io->fin_count && io->live_len && io->done, "wm_beam_step: null argument");
    WM_REQUIRE(io->workspace && io->workspace_bytes >= wm_beam_workspace_bytes(io->batch, io->beam_size),
               "wm_beam_step: workspace of %zu bytes, %zu needed", io->workspace_bytes, wm_beam_workspace_bytes(io->batch, io->beam_size));
    BeamParams p{};
    GreedyParams& g = p.g;
    g.logits = (h16*)io->logits; g.ld_row = io->row_stride; g.B = io->batch; g.V = io->n_vocab;
    g.tokens = io->tokens; g.ld_tok = io->tokens_ld; g.cur_len = io->cur_len; g.sum_logprobs = io->sum_logprobs;
    g.suppress = io->suppress; g.n_suppress = io->n_suppress; g.blank = io->blank; g.n_blank = io->n_blank;
    g.sample_begin = io->sample_begin; g.eot = io->eot; g.timestamp_begin = io->timestamp_begin;
    g.max_initial_ts = io->max_initial_timestamp_index; g.apply_rules = io->apply_rules; g.n_done = io->n_done;
    g.t_dev = io->n_past_dev; g.done = io->done; g.row_limit = io->row_limit;
    p.K = io->beam_size; p.max_cand = io->max_candidates; p.ignore_eot = io->ignore_eot;
    p.parent = io->parent; p.fin_tokens = io->fin_tokens; p.fin_scores = io->fin_scores; p.fin_len = io->fin_len;
    p.fin_count = io->fin_count; p.live_len = io->live_len; p.cand = (BeamCand*)io->workspace;
    return launch_beam_step(p, (hipStream_t)stream);
}

int wm_kv_reorder(void* const* layers_dev, int n_layer, int batch, int beam_size, int n_head, int capacity, int elem_bytes,
                  const int32_t* parent, const int32_t* done, int n_last, const int32_t* n_past_dev, wm_stream_t stream) {
    KvReorderParams p{layers_dev, n_layer, batch, beam_size, n_head, capacity, elem_bytes, parent, done, n_last, n_past_dev};
    return launch_kv_reorder(p, (hipStream_t)stream);
}
