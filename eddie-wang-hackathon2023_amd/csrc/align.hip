// Word-level timestamps: the cross-attention query tap, the alignment matrix and the DTW walk (wm_decoder_step_tap, wm_align,
// wm_dtw; the contract is DESIGN.md "word timestamps", its host form timing.py).
//
// The alignment matrix of one utterance is  Mtx = mean_heads medfilt_f( zscore_i( softmax_f( q16 . k16 ) ) ):  the softmax needs a
// token row's maximum and sum over ALL frames, the z-score a frame's mean and deviation over ALL token rows, and a head's
// N_all x F fp32 tile (448 x 1500 x 4 B) fits no LDS -- so the work is cut by frames and the scores are computed twice:
//   align_scale_q     the taped queries times 64^-0.25, rounded to fp16, rows past N_all zero (MFMA operand rows)
//   align_rowstats    per (utterance, head, 16 token rows): max and sum of exp over the F valid frames, one wave, S by MFMA
//   align_matrix      per (utterance, 32 frames + halo): for every head in ascending order S again (same operands, same
//                     instruction: the same bits), W, the columns' mean and deviation over the token rows, Z, the median over
//                     frames with reflection at 0 and F - 1, added to a running sum beside the tile in LDS (every element has one
//                     owner thread)
// No atomics, a fixed order of every sum: the result is deterministic.
//   dtw_kernel        one workgroup per utterance walks the anti-diagonals (the last three in LDS, one barrier each, trace bytes in
//                     the workspace), then walks back and writes the reversed path.
// Forced alignment (its host form alignment.py) adds the open end of that walk (wm_dtw_open, wm_align_open: the same
// kernel, templated).  The tap is ONE kernel behind a 4-token step (wm_decoder_step_tap) and a whole block (wm_decoder_prefill_tap).
#include "decode_math.h"
#include "kernels.h"
#include "../../include/whisper_mi355.h"

#include <atomic>
#include <math.h>

namespace wm {
namespace {

constexpr int A_OUT = 32;                              // frames a workgroup of align_matrix finishes
constexpr int A_COLS = 48;                             // frames it computes: A_OUT + 2 * halo (halo <= 7) in three MFMA column blocks
constexpr int A_ZS = 49;                               // LDS row stride of the tile (odd: a column walk is conflict-free)
constexpr int A_MAX_TOKENS = 448;                      // n_text_ctx of every Whisper model
constexpr int A_TAB = 32;                              // table entries per launch of align_table_kernel

__device__ __forceinline__ half8v scale8(half8v x) {
    half8v y;
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = (h16)mul_rn((float)x[e], ATTN_SCALE);      // the product rounded to fp32, then to fp16
    return y;
}

// ---- the tap ------------------------------------------------------------------------------------------------------------------------
struct TapLayer { int n; unsigned char head[64]; short slot[64]; };

// The tape has to hold the q its cross-attention kernel saw, so the split-K slabs are added in that kernel's order.  The two orders
// agree up to 5 slabs (the shipped cap is 4) and round differently from 6 on (WM_KSPLIT_CAP): they are not to be merged.
// TAP_PAIRS must match attn_cross_kernel in attn_decode.hip: qa += slab s + slab s+1, absent slabs add 0
__device__ __forceinline__ float slab_sum_pairs(const float* src, int ksplit, long sstride) {
    float qa = 0.f;
    for (int s = 0; s < ksplit; s += 2) {
        const float x0 = src[(size_t)s * sstride];
        const float x1 = s + 1 < ksplit ? src[(size_t)(s + 1) * sstride] : 0.f;
        qa += x0 + x1;
    }
    return qa;
}
// TAP_FOURS must match slab_row8 in attn_prefill.hip: rounds of four, then a tail one by one
__device__ __forceinline__ float slab_sum_fours(const float* src, int ksplit, long sstride) {
    float qa = 0.f;
    int s = 0;
    for (; s + 4 <= ksplit; s += 4) {
        const float x0 = src[(size_t)s * sstride], x1 = src[(size_t)(s + 1) * sstride];
        const float x2 = src[(size_t)(s + 2) * sstride], x3 = src[(size_t)(s + 3) * sstride];
        qa += (x0 + x1) + (x2 + x3);
    }
    for (; s < ksplit; ++s) qa += src[(size_t)s * sstride];
    return qa;
}

// q = r16(sum of the split-K slabs + bias) of the listed heads of one layer, for the n_rows = B * L rows of a call, to the tape rows
// T .. T + L - 1 of every utterance.  The row index is folded over blockIdx.y and .z (a block of 224 tokens x 576 rows passes 65 535).
template <TapOrder ORDER>
__global__ __launch_bounds__(64) void tap_q_kernel(const float* part, int ksplit, int ldp, long sstride, const h16* bias, int L, int T, int n_rows,
                                                   h16* tape, int n_tape_heads, int capacity, TapLayer tl) {
    const int d = threadIdx.x, hi = blockIdx.x;
    const unsigned folded = blockIdx.z * gridDim.y + blockIdx.y;           // (< 2^32: at most 32 769 planes of 65 535)
    if (folded >= (unsigned)n_rows) return;
    const int row = (int)folded, b = row / L, l = row - b * L;
    const int col = (int)tl.head[hi] * 64 + d;
    const float* src = part + (size_t)row * ldp + col;
    const float qa = ORDER == TAP_PAIRS ? slab_sum_pairs(src, ksplit, sstride) : slab_sum_fours(src, ksplit, sstride);
    const float bs = bias ? (float)bias[col] : 0.f;
    tape[(((size_t)b * n_tape_heads + tl.slot[hi]) * capacity + T + l) * 64 + d] = (h16)(qa + bs);
}

// ---- the alignment matrix -----------------------------------------------------------------------------------------------------------
struct AlignParams {
    const h16* tape; int capacity;
    const unsigned long long* ktab; long k_bstride;      // per head slot: K of utterance 0, fp16 [Tk][64]; elements between utterances
    const int* n_tokens; const int* n_frames;
    int n_heads, Tk, cap_tokens, n_pad, n_prefix, width;
    h16* qs;                                             // [batch][n_heads][n_pad][64]
    float2* stats;                                       // [batch][n_heads][n_pad]: row maximum, sum of exp
    float* out; int ld; long out_bstride;
};

struct TabChunk { unsigned long long v[A_TAB]; };
__global__ void align_table_kernel(unsigned long long* dst, TabChunk c, int n) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = c.v[threadIdx.x];
}

__global__ __launch_bounds__(256) void align_scale_q_kernel(AlignParams p) {
    const int b = blockIdx.z, slot = blockIdx.y;
    const int idx = blockIdx.x * 256 + threadIdx.x;                 // (row, 8-element chunk)
    const int row = idx >> 3, ch = idx & 7;
    if (row >= p.n_pad) return;
    const int n_all = min(p.n_tokens[b], p.cap_tokens);
    half8v v = half8v{0, 0, 0, 0, 0, 0, 0, 0};
    if (row < n_all) v = scale8(*(const half8v*)(p.tape + (((size_t)b * p.n_heads + slot) * p.capacity + row) * 64 + ch * 8));
    *(half8v*)(p.qs + (((size_t)b * p.n_heads + slot) * p.n_pad + row) * 64 + ch * 8) = v;
}

__device__ __forceinline__ float4v score_block(half8v a0, half8v a1, const h16* K, int frame_clamped, int lane) {
    const h16* kp = K + (size_t)frame_clamped * 64 + 8 * (lane >> 4);
    const half8v k0 = scale8(*(const half8v*)kp), k1 = scale8(*(const half8v*)(kp + 32));
    float4v acc = float4v{0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, k0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, k1, acc, 0, 0, 0);
    return acc;
}

// one wave per (16 token rows, head, utterance): lane l holds column l & 15 of rows 4 (l >> 4) .. + 3 of every 16 x 16 score block
__global__ __launch_bounds__(64) void align_rowstats_kernel(AlignParams p) {
    const int mb = blockIdx.x, slot = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
    const int n_all = min(p.n_tokens[b], p.cap_tokens), F = min(p.n_frames[b], p.Tk);
    if (mb * 16 >= n_all || F < 1) return;
    const h16* q = p.qs + (((size_t)b * p.n_heads + slot) * p.n_pad + mb * 16 + (lane & 15)) * 64 + 8 * (lane >> 4);
    const half8v a0 = *(const half8v*)q, a1 = *(const half8v*)(q + 32);
    const h16* K = (const h16*)p.ktab[slot] + (size_t)b * p.k_bstride;
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int f0 = 0; f0 < F; f0 += 16) {
        const int frame = f0 + (lane & 15);
        const float4v s = score_block(a0, a1, K, min(frame, F - 1), lane);
        if (frame < F) {
#pragma unroll
            for (int r = 0; r < 4; ++r) mx[r] = fmaxf(mx[r], s[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) mx[r] = fmaxf(mx[r], __shfl_xor(mx[r], m));
    float sm[4] = {0.f, 0.f, 0.f, 0.f};
    for (int f0 = 0; f0 < F; f0 += 16) {
        const int frame = f0 + (lane & 15);
        const float4v s = score_block(a0, a1, K, min(frame, F - 1), lane);
        if (frame < F) {
#pragma unroll
            for (int r = 0; r < 4; ++r) sm[r] += expf(s[r] - mx[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) sm[r] += __shfl_xor(sm[r], m);
    if ((lane & 15) == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            p.stats[((size_t)b * p.n_heads + slot) * p.n_pad + mb * 16 + 4 * (lane >> 4) + r] = make_float2(mx[r], sm[r]);
    }
}

// the median of `width` (odd, <= MAXW) values by rank: the value that `width / 2` others precede (equal values in index order)
template <int MAXW>
__device__ __forceinline__ float median_of(const float (&v)[MAXW], int width) {
    float med = v[0];
    const int want = width >> 1;
#pragma unroll
    for (int i = 0; i < MAXW; ++i) {
        int before = 0;
#pragma unroll
        for (int j = 0; j < MAXW; ++j)
            if (j < width && (v[j] < v[i] || (v[j] == v[i] && j < i))) ++before;
        if (i < width && before == want) med = v[i];
    }
    return med;
}

template <int MAXW>
__global__ __launch_bounds__(256) void align_matrix_kernel(AlignParams p) {
    extern __shared__ float lds[];
    const int b = blockIdx.y, t0 = blockIdx.x * A_OUT, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n_all = min(p.n_tokens[b], p.cap_tokens), F = min(p.n_frames[b], p.Tk);
    if (n_all - p.n_prefix - 1 < 1 || F < 1 || t0 >= F) return;
    const int halo = p.width >> 1;
    const bool filter = p.width > 1 && F > halo;            // upstream: no filtering when the padding would not fit
    const int c0 = t0 - halo;                               // frame of tile column 0
    const int n_mb = (n_all + 15) >> 4;
    float* Zt = lds;                                        // [n_pad][A_ZS]
    float* red = lds + (size_t)p.n_pad * A_ZS;              // [4][A_COLS]
    float* cmean = red + 4 * A_COLS;
    float* cstd = cmean + A_COLS;
    float* accL = cstd + A_COLS;                            // [n_pad][A_OUT]: the running sum over the heads (element idx is thread idx % 256's)
    const float inv_n = 1.0f / (float)n_all;
    for (int idx = tid; idx < n_all * A_OUT; idx += 256) accL[idx] = 0.f;

    for (int slot = 0; slot < p.n_heads; ++slot) {
        const h16* K = (const h16*)p.ktab[slot] + (size_t)b * p.k_bstride;
        const float2* st = p.stats + ((size_t)b * p.n_heads + slot) * p.n_pad;
        const h16* qbase = p.qs + ((size_t)b * p.n_heads + slot) * p.n_pad * 64;
        // ---- W = softmax_f(S) of the tile's columns, all token rows
        for (int mb = wv; mb < n_mb; mb += 4) {
            const h16* q = qbase + (size_t)(mb * 16 + (lane & 15)) * 64 + 8 * (lane >> 4);
            const half8v a0 = *(const half8v*)q, a1 = *(const half8v*)(q + 32);
#pragma unroll
            for (int nb = 0; nb < 3; ++nb) {
                const int col = nb * 16 + (lane & 15), frame = c0 + col;
                const float4v s = score_block(a0, a1, K, min(max(frame, 0), F - 1), lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = mb * 16 + 4 * (lane >> 4) + r;
                    float w = 0.f;
                    if (row < n_all && frame >= 0 && frame < F) {
                        const float2 ms = st[row];
                        w = expf(s[r] - ms.x) / ms.y;
                    }
                    Zt[row * A_ZS + col] = w;
                }
            }
        }
        __syncthreads();
        // ---- mean and population deviation of every column over the token rows (two passes, four partial sums each)
        if (tid < 4 * A_COLS) {
            const int col = tid % A_COLS, part = tid / A_COLS;
            float s = 0.f;
            for (int row = part; row < n_all; row += 4) s += Zt[row * A_ZS + col];
            red[part * A_COLS + col] = s;
        }
        __syncthreads();
        if (tid < A_COLS) cmean[tid] = ((red[tid] + red[A_COLS + tid]) + (red[2 * A_COLS + tid] + red[3 * A_COLS + tid])) * inv_n;
        __syncthreads();
        if (tid < 4 * A_COLS) {
            const int col = tid % A_COLS, part = tid / A_COLS;
            const float m = cmean[col];
            float s = 0.f;
            for (int row = part; row < n_all; row += 4) {
                const float dlt = Zt[row * A_ZS + col] - m;
                s += dlt * dlt;
            }
            red[part * A_COLS + col] = s;
        }
        __syncthreads();
        if (tid < A_COLS) cstd[tid] = sqrtf(((red[tid] + red[A_COLS + tid]) + (red[2 * A_COLS + tid] + red[3 * A_COLS + tid])) * inv_n);
        __syncthreads();
        // ---- Z in place (0 where the deviation is 0: upstream would give NaN)
        for (int idx = tid; idx < n_all * A_COLS; idx += 256) {
            const int row = idx / A_COLS, col = idx - row * A_COLS;
            const float sd = cstd[col];
            const float w = Zt[row * A_ZS + col];
            Zt[row * A_ZS + col] = sd > 0.f ? (w - cmean[col]) / sd : 0.f;
        }
        __syncthreads();
        // ---- median over frames (reflection at 0 and F - 1), added to the running sums
        for (int idx = tid; idx < n_all * A_OUT; idx += 256) {
            const int row = idx >> 5, f = t0 + (idx & 31);
            if (f < F) {
                float val;
                if (filter) {
                    float v[MAXW];
#pragma unroll
                    for (int j = 0; j < MAXW; ++j) {
                        int g = f - halo + j;
                        g = g < 0 ? -g : (g >= F ? 2 * (F - 1) - g : g);
                        v[j] = j < p.width ? Zt[row * A_ZS + (g - c0)] : 0.f;
                    }
                    val = median_of<MAXW>(v, p.width);
                } else {
                    val = Zt[row * A_ZS + (f - c0)];
                }
                accL[idx] += val;
            }
        }
        __syncthreads();
    }
    // ---- the mean over the heads; rows n_prefix .. N_all - 2 are the matrix
    const float n_heads_f = (float)p.n_heads;
    for (int idx = tid; idx < n_all * A_OUT; idx += 256) {
        const int row = idx >> 5, f = t0 + (idx & 31);
        if (row >= p.n_prefix && row < n_all - 1 && f < F)
            p.out[(size_t)b * p.out_bstride + (size_t)(row - p.n_prefix) * p.ld + f] = accL[idx] / n_heads_f;
    }
}

// ---- DTW ----------------------------------------------------------------------------------------------------------------------------
struct DtwParams {
    const float* x; int ldx; long x_bstride; int negate;
    const int* n_rows; int row_sub; const int* n_cols; int max_rows, max_cols;
    int* path_text; int* path_time; int path_ld; int* path_len;
    unsigned char* trace;                                // [batch][max_rows + 1][max_cols + 1]
};

// thread i owns row i of the cost table; on diagonal d it computes cell (i, d - i) from the two diagonals before.
// OPEN (wm_dtw_open, wm_align_open): the walk back starts at (i*, M), i* the smallest row whose cost in the last column is the
// column's minimum -- thread i keeps cost[i][M] from diagonal i + M in a register, a wave reduces (value, row) by shuffles and
// thread 0 reduces the waves' results from LDS: no second pass over the table.  Everything OPEN adds sits under `if constexpr`,
// and the closed instantiation takes DtwParams alone, so it is the kernel it was, argument layout included.
struct DtwOpenParams : DtwParams { int* end_row; };
template <bool OPEN> struct DtwArg { using type = DtwParams; };
template <> struct DtwArg<true> { using type = DtwOpenParams; };

template <bool OPEN>
__global__ __launch_bounds__(1024) void dtw_kernel(typename DtwArg<OPEN>::type p) {
    extern __shared__ float dl[];
    __shared__ int s_len;
    const int b = blockIdx.x, tid = threadIdx.x, i = tid;
    const int N = min(p.n_rows[b], p.max_rows) - p.row_sub, M = min(p.n_cols[b], p.max_cols);      // (the clip of the matrix kernels, then the cut rows)
    if (N < 1 || M < 1) {
        if (tid == 0) {
            p.path_len[b] = 0;
            if constexpr (OPEN) p.end_row[b] = 0;
        }
        return;
    }
    const int R = p.max_rows + 1, TS = p.max_cols + 1;
    int* rev = (int*)(dl + 3 * R);                       // [2][max_rows + max_cols]: the walk back, last cell first
    const int P = p.max_rows + p.max_cols;
    const float* x = p.x + (size_t)b * p.x_bstride;
    unsigned char* tr = p.trace + (size_t)b * R * TS;
    const float* xrow = x + (size_t)(i > 0 ? i - 1 : 0) * p.ldx;
    // x of this thread's cell on the NEXT diagonal is requested while the current one is computed
    float x_next = 0.f;
    [[maybe_unused]] float last = INFINITY;              // (OPEN) cost[i][M]
    for (int d = 0; d <= N + M; ++d) {
        float* cur = dl + (d % 3) * R;
        const float* prev1 = dl + ((d + 2) % 3) * R;
        const float* prev2 = dl + ((d + 1) % 3) * R;
        const int j = d - i;
        const float x_cur = x_next;
        if (i >= 1 && i <= N && j + 1 >= 1 && j + 1 <= M) x_next = xrow[j];      // cell (i, j + 1) reads x[i - 1][j]
        if (i <= N && j >= 0 && j <= M) {
            float v;
            if (i == 0) v = d == 0 ? 0.f : INFINITY;
            else if (j == 0) v = INFINITY;
            else {
                const float c0 = prev2[i - 1], c1 = prev1[i - 1], c2 = prev1[i];
                float c; unsigned char t;
                if (c0 < c1 && c0 < c2) { c = c0; t = 0; }
                else if (c1 < c0 && c1 < c2) { c = c1; t = 1; }
                else { c = c2; t = 2; }
                v = (p.negate ? -x_cur : x_cur) + c;
                tr[(size_t)i * TS + j] = t;
            }
            cur[i] = v;
            if constexpr (OPEN) {
                if (i >= 1 && j == M) last = v;
            }
        }
        __syncthreads();
    }
    [[maybe_unused]] int start_row = N;
    if constexpr (OPEN) {
        __shared__ float s_best[16];
        __shared__ int s_row[16];
        float bv = last; int bi = (i >= 1 && i <= N) ? i : 0x7fffffff;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float ov = __shfl_xor(bv, m); const int oi = __shfl_xor(bi, m);
            if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if ((tid & 63) == 0) { s_best[tid >> 6] = bv; s_row[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            const int n_waves = (int)blockDim.x >> 6;
            for (int k = 1; k < n_waves; ++k)
                if (s_best[k] < bv || (s_best[k] == bv && s_row[k] < bi)) { bv = s_best[k]; bi = s_row[k]; }
            start_row = (bi >= 1 && bi <= N) ? bi : 1;   // (NaN or +inf everywhere: row 1, the first candidate)
            p.end_row[b] = start_row;
        }
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        int a = OPEN ? start_row : N, c = M, n = 0;
        while ((a > 0 || c > 0) && n < P) {
            rev[n] = a - 1; rev[P + n] = c - 1; ++n;
            const int t = a == 0 ? 2 : (c == 0 ? 1 : (int)tr[(size_t)a * TS + c]);
            if (t == 0) { --a; --c; } else if (t == 1) --a; else --c;
        }
        s_len = n;
        p.path_len[b] = n < p.path_ld ? n : p.path_ld;
    }
    __syncthreads();
    const int n = s_len;
    for (int k = tid; k < n && k < p.path_ld; k += blockDim.x) {
        p.path_text[(size_t)b * p.path_ld + k] = rev[n - 1 - k];
        p.path_time[(size_t)b * p.path_ld + k] = rev[P + n - 1 - k];
    }
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct DtwWs { size_t trace, total; };
DtwWs carve_dtw(int batch, int max_rows, int max_cols) {
    DtwWs w{};
    w.trace = 0;
    w.total = up256((size_t)batch * (max_rows + 1) * (max_cols + 1));
    return w;
}

int launch_dtw(DtwParams p, int batch, hipStream_t s, int* end_row = nullptr) {
    WM_REQUIRE(p.max_rows >= 1 && p.max_rows <= 1023 && p.max_cols >= 1, "dtw: max_rows %d must be in 1 .. 1023, max_cols %d >= 1", p.max_rows, p.max_cols);
    const size_t lds = (size_t)3 * (p.max_rows + 1) * sizeof(float) + (size_t)2 * (p.max_rows + p.max_cols) * sizeof(int);
    WM_REQUIRE(lds <= 60 * 1024, "dtw: %d rows x %d columns need %zu bytes of LDS", p.max_rows, p.max_cols, lds);
    const int threads = p.max_rows + 1 <= 512 ? 512 : 1024;
    if (end_row) {
        DtwOpenParams po{};
        static_cast<DtwParams&>(po) = p;
        po.end_row = end_row;
        hipLaunchKernelGGL(dtw_kernel<true>, dim3(batch), dim3(threads), lds, s, po);
    } else {
        hipLaunchKernelGGL(dtw_kernel<false>, dim3(batch), dim3(threads), lds, s, p);
    }
    WM_LAUNCH_CHECK(s, "dtw");
    return 0;
}

struct AlignWs { size_t ktab, qs, stats, mtx, dtw, total; int n_pad, ldw; };
AlignWs carve_align(int batch, int n_heads, int cap_tokens, int Tk) {
    AlignWs w{};
    w.n_pad = (cap_tokens + 15) / 16 * 16;
    w.ldw = (Tk + 3) / 4 * 4;
    size_t off = 0;
    w.ktab = off; off += up256((size_t)n_heads * 8);
    w.qs = off; off += up256((size_t)batch * n_heads * w.n_pad * 64 * sizeof(h16));
    w.stats = off; off += up256((size_t)batch * n_heads * w.n_pad * sizeof(float2));
    w.mtx = off; off += up256((size_t)batch * cap_tokens * w.ldw * sizeof(float));
    w.dtw = off; off += carve_dtw(batch, cap_tokens, Tk).total;
    w.total = off;
    return w;
}

}  // namespace

int launch_tap_q(TapOrder order, const float* part, int ksplit, int ldp, long sstride, const h16* bias, int B, int L, int T, h16* tape,
                 int n_tape_heads, int capacity, const int* heads_in_layer, const int* slots, int n, hipStream_t s) {
    WM_REQUIRE(n >= 1 && n <= 64, "tap: %d heads in one layer", n);
    WM_REQUIRE(B >= 1 && L >= 1 && T >= 0 && T + L <= capacity && (long)B * L <= 0x7fffffffL,
               "tap: bad block (%d rows x %d tokens behind %d, capacity %d)", B, L, T, capacity);
    TapLayer tl{};
    tl.n = n;
    for (int k = 0; k < n; ++k) { tl.head[k] = (unsigned char)heads_in_layer[k]; tl.slot[k] = (short)slots[k]; }
    const int n_rows = B * L, gy = n_rows < 65535 ? n_rows : 65535, gz = (n_rows + gy - 1) / gy;      // (gz <= 32 769: n_rows is an int)
    const auto kernel = order == TAP_PAIRS ? tap_q_kernel<TAP_PAIRS> : tap_q_kernel<TAP_FOURS>;
    hipLaunchKernelGGL(kernel, dim3(n, gy, gz), dim3(64), 0, s, part, ksplit, ldp, sstride, bias, L, T, n_rows, tape, n_tape_heads, capacity, tl);
    WM_LAUNCH_CHECK(s, "tap_q");
    return 0;
}

}  // namespace wm

using namespace wm;

extern "C" {

size_t wm_dtw_workspace_bytes(int batch, int max_rows, int max_cols) {
    if (batch < 1 || max_rows < 1 || max_cols < 1) return 0;
    return carve_dtw(batch, max_rows, max_cols).total;
}

// wm_dtw (end_row == null) and wm_dtw_open
static int dtw_entry(const char* who, const float* x, int ldx, int64_t x_bstride, int batch, const int32_t* n_rows, const int32_t* n_cols,
                     int max_rows, int max_cols, int32_t* path_text, int32_t* path_time, int path_ld, int32_t* path_len, int32_t* end_row,
                     void* workspace, size_t workspace_bytes, wm_stream_t stream) {
    WM_REQUIRE(x && n_rows && n_cols && path_text && path_time && path_len && workspace, "%s: null argument", who);
    WM_REQUIRE(batch >= 1 && ldx >= max_cols && path_ld >= 1, "%s: bad batch / ldx / path_ld (%d, %d, %d)", who, batch, ldx, path_ld);
    WM_REQUIRE(max_rows >= 1 && max_cols >= 1, "%s: bad max_rows / max_cols (%d, %d)", who, max_rows, max_cols);
    WM_REQUIRE(workspace_bytes >= wm_dtw_workspace_bytes(batch, max_rows, max_cols), "%s: workspace too small: %zu < %zu", who,
               workspace_bytes, wm_dtw_workspace_bytes(batch, max_rows, max_cols));
    DtwParams p{};
    p.x = x; p.ldx = ldx; p.x_bstride = (long)x_bstride; p.negate = 0;
    p.n_rows = n_rows; p.row_sub = 0; p.n_cols = n_cols; p.max_rows = max_rows; p.max_cols = max_cols;
    p.path_text = path_text; p.path_time = path_time; p.path_ld = path_ld; p.path_len = path_len;
    p.trace = (unsigned char*)workspace;
    return launch_dtw(p, batch, (hipStream_t)stream, end_row);
}

int wm_dtw(const float* x, int ldx, int64_t x_bstride, int batch, const int32_t* n_rows, const int32_t* n_cols, int max_rows,
           int max_cols, int32_t* path_text, int32_t* path_time, int path_ld, int32_t* path_len, void* workspace,
           size_t workspace_bytes, wm_stream_t stream) {
    return dtw_entry("wm_dtw", x, ldx, x_bstride, batch, n_rows, n_cols, max_rows, max_cols, path_text, path_time, path_ld, path_len,
                     nullptr, workspace, workspace_bytes, stream);
}

int wm_dtw_open(const float* x, int ldx, int64_t x_bstride, int batch, const int32_t* n_rows, const int32_t* n_cols, int max_rows,
                int max_cols, int32_t* path_text, int32_t* path_time, int path_ld, int32_t* path_len, int32_t* end_row, void* workspace,
                size_t workspace_bytes, wm_stream_t stream) {
    WM_REQUIRE(end_row, "wm_dtw_open: null argument");
    return dtw_entry("wm_dtw_open", x, ldx, x_bstride, batch, n_rows, n_cols, max_rows, max_cols, path_text, path_time, path_ld, path_len,
                     end_row, workspace, workspace_bytes, stream);
}

size_t wm_align_workspace_bytes(int batch, int n_heads, int cap_tokens, int n_audio_ctx) {
    if (batch < 1 || n_heads < 1 || cap_tokens < 1 || n_audio_ctx < 1) return 0;
    return carve_align(batch, n_heads, cap_tokens, n_audio_ctx).total;
}

// wm_align (end_row == null: the closed walk) and wm_align_open
static int align_entry(const wm_align_io* io, int32_t* end_row, wm_stream_t stream) {
    WM_REQUIRE(io && io->q_tape && io->cross && io->heads && io->n_tokens && io->n_frames && io->path_text && io->path_time &&
               io->path_len && io->workspace, "wm_align: null argument");
    const int B = io->batch, H = io->n_text_head, Tk = io->n_audio_ctx, nh = io->n_heads, cap = io->cap_tokens;
    WM_REQUIRE(B >= 1 && H >= 1 && Tk >= 1 && nh >= 1 && io->n_layers >= 1, "wm_align: bad batch / heads / frames (%d, %d, %d, %d)", B, H, Tk, nh);
    if (io->engine) {
        int32_t kind = 0; uint32_t flags = 0; wm_dims d{};
        if (wm_engine_info(io->engine, &kind, &flags, &d)) return 1;
        WM_REQUIRE(kind == WM_ENGINE_DECODER, "wm_align: not a decoder engine");
        WM_REQUIRE(!(flags & WM_FLAG_INT8_CROSS_KV), "wm_align: word timestamps need fp16 cross-attention K/V; this engine stores int8 codes (WM_FLAG_INT8_CROSS_KV)");
        WM_REQUIRE(d.n_text_head == H && d.n_audio_ctx == Tk && d.n_text_layer == io->n_layers, "wm_align: the dimensions do not match the engine's");
    }
    WM_REQUIRE(cap >= 1 && cap <= A_MAX_TOKENS && cap <= io->capacity, "wm_align: cap_tokens %d must be in 1 .. %d and <= capacity %d", cap, A_MAX_TOKENS, io->capacity);
    WM_REQUIRE(io->n_prefix >= 0, "wm_align: bad n_prefix %d", io->n_prefix);
    WM_REQUIRE(io->filter_width >= 1 && io->filter_width <= 15 && (io->filter_width & 1), "wm_align: filter_width %d must be odd, 1 .. 15", io->filter_width);
    WM_REQUIRE(!io->matrix || io->ld >= Tk, "wm_align: ld %d < n_audio_ctx %d", io->ld, Tk);
    const AlignWs w = carve_align(B, nh, cap, Tk);
    WM_REQUIRE(io->workspace_bytes >= w.total, "wm_align: workspace too small: %zu < %zu", io->workspace_bytes, w.total);
    hipStream_t s = (hipStream_t)stream;
    unsigned char* base = (unsigned char*)io->workspace;
    // the heads' K pointers (utterance 0), written to the workspace by small launches with the values as arguments
    unsigned long long* ktab = (unsigned long long*)(base + w.ktab);
    int prev = -1;
    for (int k0 = 0; k0 < nh; k0 += A_TAB) {
        TabChunk c{};
        const int n = nh - k0 < A_TAB ? nh - k0 : A_TAB;
        for (int k = 0; k < n; ++k) {
            const int hd = io->heads[k0 + k];
            WM_REQUIRE(hd > prev && hd < io->n_layers * H, "wm_align: heads must be strictly ascending and below n_layers * n_text_head (entry %d = %d)", k0 + k, hd);
            prev = hd;
            const void* layer = io->cross[hd / H];
            WM_REQUIRE(layer, "wm_align: cross[%d] is null", hd / H);
            c.v[k] = (unsigned long long)(uintptr_t)((const h16*)layer + (size_t)(hd % H) * Tk * 64);
        }
        hipLaunchKernelGGL(align_table_kernel, dim3(1), dim3(64), 0, s, ktab + k0, c, n);
        WM_LAUNCH_CHECK(s, "align_table");
    }
    AlignParams p{};
    p.tape = (const h16*)io->q_tape; p.capacity = io->capacity;
    p.ktab = ktab; p.k_bstride = (long)2 * H * Tk * 64;
    p.n_tokens = io->n_tokens; p.n_frames = io->n_frames;
    p.n_heads = nh; p.Tk = Tk; p.cap_tokens = cap; p.n_pad = w.n_pad; p.n_prefix = io->n_prefix; p.width = io->filter_width;
    p.qs = (h16*)(base + w.qs); p.stats = (float2*)(base + w.stats);
    if (io->matrix) { p.out = io->matrix; p.ld = io->ld; p.out_bstride = (long)cap * io->ld; }
    else { p.out = (float*)(base + w.mtx); p.ld = w.ldw; p.out_bstride = (long)cap * w.ldw; }
    hipLaunchKernelGGL(align_scale_q_kernel, dim3((w.n_pad * 8 + 255) / 256, nh, B), dim3(256), 0, s, p);
    WM_LAUNCH_CHECK(s, "align_scale_q");
    hipLaunchKernelGGL(align_rowstats_kernel, dim3(w.n_pad / 16, nh, B), dim3(64), 0, s, p);
    WM_LAUNCH_CHECK(s, "align_rowstats");
    const size_t lds = ((size_t)w.n_pad * (A_ZS + A_OUT) + 6 * A_COLS) * sizeof(float);       // <= 146 KB at 448 tokens (a CU has 160 KB)
    static std::atomic<unsigned long long> attr_set{0};
    int dev = 0;
    WM_CHECK_HIP(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(attr_set.load(std::memory_order_acquire) & bit)) {
        WM_CHECK_HIP(hipFuncSetAttribute((const void*)align_matrix_kernel<7>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        WM_CHECK_HIP(hipFuncSetAttribute((const void*)align_matrix_kernel<15>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set.fetch_or(bit, std::memory_order_release);
    }
    const dim3 grid((Tk + A_OUT - 1) / A_OUT, B);
    if (io->filter_width <= 7) hipLaunchKernelGGL(align_matrix_kernel<7>, grid, dim3(256), lds, s, p);
    else hipLaunchKernelGGL(align_matrix_kernel<15>, grid, dim3(256), lds, s, p);
    WM_LAUNCH_CHECK(s, "align_matrix");
    DtwParams dp{};
    dp.x = p.out; dp.ldx = p.ld; dp.x_bstride = p.out_bstride; dp.negate = 1;
    dp.n_rows = io->n_tokens; dp.row_sub = io->n_prefix + 1; dp.n_cols = io->n_frames; dp.max_rows = cap; dp.max_cols = Tk;
    dp.path_text = io->path_text; dp.path_time = io->path_time; dp.path_ld = cap + Tk; dp.path_len = io->path_len;
    dp.trace = base + w.dtw;
    return launch_dtw(dp, B, s, end_row);
}

int wm_align(const wm_align_io* io, wm_stream_t stream) { return align_entry(io, nullptr, stream); }

int wm_align_open(const wm_align_io* io, int32_t* end_row, wm_stream_t stream) {
    WM_REQUIRE(end_row, "wm_align_open: null argument");
    return align_entry(io, end_row, stream);
}

}  // extern "C"
