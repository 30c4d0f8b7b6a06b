// Block prefill of the Whisper text decoder (wm_decoder_prefill): the two attention products of a whole start block -- L new tokens
// per utterance, 1 .. n_text_ctx, on an EMPTY cache -- in one launch each, where the decode kernels (attn_decode.hip, at most 4
// queries per utterance) need ceil(L / 4) passes over the growing cache.
//
//   attn_prefill_kernel<SELF = true, I8>     causal self-attention of the block over its OWN un-quantised k / v rows, and the append
//                                            of every slot 0 .. L - 1 to the cache [B, 2, H, cap, 64] (fp16 rows | int8 codes)
//   attn_prefill_kernel<SELF = false, ., QB> cross-attention of the block's L queries per utterance over fp16 K/V [B, 2, H, Tk, 64]
//
// Arithmetic contract (the rounding points of attn_decode.hip; tests/prefill_refs.py restates it in float64):
//   q, k, v rows = fp16(sum of the split-K slabs + bias); q and k times 64^-0.25, rounded to fp16; a score = the fp32 sum rounded to
//   fp16; softmax in fp32 (online form, as attn_encoder.hip); probabilities rounded to fp16; P.V in fp32, rounded to fp16.
//   int8 cache: code = sat_s8(rne(x * (1 / t))), 1 / t formed in fp32 -- the APPEND only: inside the block every key and value is the
//   un-quantised fp16 row ("the tokens of the current call are used un-quantised"), where the 4-token passes see the earlier tokens
//   of the same prompt through their codes.
//   Right-aligned rows (row_start): the query in slot t of utterance b attends to the slots [row_start[b], t]; a query in a pad slot
//   (t < row_start[b]) writes an all-zero row; pad slots are appended like any other (they are never read as keys later either).
//   Cross-attention knows no row_start: pad queries are computed like the others, finite and meaningless.
//   Rows that an optional `live` list (count, then indices) does not name are neither read nor written.
//   Inputs are expected to be finite.
//
// gfx950 design: attn_encoder.hip's.  S^T = K . Q^T (mfma_f32_16x16x32_f16), so a lane owns ONE query (column lane & 15) and holds 4
// keys per 16-key block: the row softmax is in-register plus two cross-lane steps, exp(S^T) in fp16 IS the B operand of
// O^T = V^T . P^T, and V^T comes out of the row-major [key][dim] LDS tile through ds_read_b64_tr_b16.  K/V tiles of 64 keys, rows of
// 128 B, 16-byte chunk c of key row r at position c ^ ((r >> 1) & 7).  A workgroup = 4 waves x QB blocks of 16 queries.
//  * cross: tiles go global -> LDS by DMA (global_load_lds, one tile ahead, double-buffered, one barrier per tile; the K rows, which
//    are stored un-scaled, are scaled in place by the lanes that fetched them, between their wait and the barrier); the key tail is
//    masked in the last tile, whose dead 16-key blocks are skipped.  Items are numbered as in the encoder kernel: the query tiles of
//    one (utterance, head) share blockIdx % 8 -- one XCD under round-robin placement -- and follow each other closely, so the
//    head's K/V (384 KB at Tk = 1500) leaves HBM once.  QB = 2 (128 queries per workgroup) for L > 64, else QB = 1: the choice
//    depends on L only, never on the batch.
//  * self: the k / v rows exist only as fp32 slabs, so a tile is summed, rounded and scaled in registers and written to LDS (one
//    buffer, two barriers per tile: the key range is at most 448 and this kernel is not the expensive one).  The workgroup of query
//    tile qt walks the key tiles [row_start / 64, qt]; tile qt holds its own 64 slots, which it appends to the cache while staging
//    them: every cache row is written exactly once, slots >= L never.
#include <type_traits>

#include "decode_math.h"
#include "kernels.h"

namespace wm {

namespace {

constexpr int PF_KEYS = 64;
constexpr int PF_AROW = 128;                       // LDS bytes per key row (64 halves, chunk-swizzled)
constexpr int PF_TILE = PF_KEYS * PF_AROW;         // 8192

struct PrefillParams {
    const float* part; int ksplit; int ldp; size_t sstride; const h16* bias;   // self: q | k | v slabs, cross: q slabs
    int B, L, H, Tk;
    const h16* kv; long kv_bstride;                  // cross: [B][2][H][Tk][64]
    void* cache; long cache_bstride; int cap; float kv_scale;      // self: [B][2][H][cap][64]
    h16* out; int ldo;
    const int32_t* live; const int32_t* row_start;
};

// fp16(sum_s slab[s][0 .. 7] + bias[0 .. 7]) of 8 consecutive columns (the slabs in attn_decode.hip's order: rounds of four, then a tail)
__device__ __forceinline__ void slab_row8(const float* src, int ksplit, size_t sstride, const h16* bias, float (&v)[8]) {
    float4 a = {0.f, 0.f, 0.f, 0.f}, c = {0.f, 0.f, 0.f, 0.f};
    int s = 0;
    for (; s + 4 <= ksplit; s += 4) {
        const float* r0 = src + (size_t)s * sstride;
        const float* r1 = r0 + sstride; const float* r2 = r1 + sstride; const float* r3 = r2 + sstride;
        const float4 a0 = ((const float4*)r0)[0], a1 = ((const float4*)r1)[0], a2 = ((const float4*)r2)[0], a3 = ((const float4*)r3)[0];
        const float4 c0 = ((const float4*)r0)[1], c1 = ((const float4*)r1)[1], c2 = ((const float4*)r2)[1], c3 = ((const float4*)r3)[1];
        a.x += (a0.x + a1.x) + (a2.x + a3.x); a.y += (a0.y + a1.y) + (a2.y + a3.y);
        a.z += (a0.z + a1.z) + (a2.z + a3.z); a.w += (a0.w + a1.w) + (a2.w + a3.w);
        c.x += (c0.x + c1.x) + (c2.x + c3.x); c.y += (c0.y + c1.y) + (c2.y + c3.y);
        c.z += (c0.z + c1.z) + (c2.z + c3.z); c.w += (c0.w + c1.w) + (c2.w + c3.w);
    }
    for (; s < ksplit; ++s) {
        const float* r0 = src + (size_t)s * sstride;
        const float4 a0 = ((const float4*)r0)[0], c0 = ((const float4*)r0)[1];
        a.x += a0.x; a.y += a0.y; a.z += a0.z; a.w += a0.w;
        c.x += c0.x; c.y += c0.y; c.z += c0.z; c.w += c0.w;
    }
    const float acc[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = r16_f32(acc[j] + (bias ? (float)bias[j] : 0.f));
}

template <bool SELF, bool I8, int QB>
__global__ __launch_bounds__(256, 2) void attn_prefill_kernel(PrefillParams p) {
    __shared__ __attribute__((aligned(1024))) unsigned char smem[(SELF ? 2 : 4) * PF_TILE];
    auto sK = [&](int b) { return smem + b * 2 * PF_TILE; };
    auto sV = [&](int b) { return smem + b * 2 * PF_TILE + PF_TILE; };

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = lane >> 4, li = lane & 15;
    const int C = p.H * 64;
    const int nx = (p.L + 64 * QB - 1) / (64 * QB), n_heads = p.H * p.B;
    int hh, qt;
    if constexpr (SELF) {                            // the long key ranges (late query tiles) first
        qt = nx - 1 - (int)(blockIdx.x % nx); hh = blockIdx.x / nx;
    } else {                                         // item = 8 j + x: head (j / nx) * 8 + x, tile j % nx (attn_encoder.hip)
        const int item = blockIdx.x;
        hh = ((item >> 3) / nx) * 8 + (item & 7); qt = (item >> 3) % nx;
    }
    if (hh >= n_heads) return;
    int b = hh / p.H;
    const int h = hh % p.H;
    if (p.live) {
        if (b >= p.live[0]) return;
        b = p.live[1 + b];
        if (b < 0 || b >= p.B) return;
    }

    // ---- Q^T fragments: B operand, lane -> query li, dims 32 s + 8 g .. + 8 ------------------------
    const int q_base = qt * (64 * QB) + wid * (16 * QB);
    half8v qf[QB][2];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        int qrow = q_base + qb * 16 + li;
        if (qrow > p.L - 1) qrow = p.L - 1;
        const size_t m = (size_t)b * p.L + qrow;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int col = h * 64 + s * 32 + g * 8;
            float v[8];
            slab_row8(p.part + m * p.ldp + col, p.ksplit, p.sstride, p.bias ? p.bias + col : nullptr, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) qf[qb][s][j] = (h16)r16_f32(v[j] * ATTN_SCALE);
        }
    }

    // ---- the keys a lane's queries see: [lo, hi[qb]] ------------------------------------------------
    int start = 0;
    if constexpr (SELF) {
        if (p.row_start) { start = p.row_start[b]; start = start < 0 ? 0 : (start > p.L ? p.L : start); }
    }
    const int lo = start;
    int hi[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) hi[qb] = SELF ? q_base + qb * 16 + li : p.Tk - 1;
    const int t_last = SELF ? qt : (p.Tk - 1) >> 6;
    const int t_first = SELF ? ((start >> 6) < qt ? (start >> 6) : qt) : 0;
    const bool has_q = q_base < p.L;                 // wave-uniform: a wave without a live query only takes part in the staging

    // ---- staging ---------------------------------------------------------------------------------------
    // cross: a tile is 8 wave-wide DMA pieces (8 key rows x 128 B each) per matrix; wave w issues pieces w and w + 4 of K and of V
    const h16* kbase = SELF ? nullptr : p.kv + (size_t)b * p.kv_bstride + (size_t)h * p.Tk * 64;
    const h16* vbase = SELF ? nullptr : kbase + (size_t)p.H * p.Tk * 64;
    auto load_kv = [&](int tile, int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int piece = wid + 4 * i;
            const int r = piece * 8 + (lane >> 3);
            int key = tile * PF_KEYS + r;
            if (key > p.Tk - 1) key = p.Tk - 1;
            const size_t off = (size_t)key * 64 + (((lane & 7) ^ ((r >> 1) & 7)) * 8);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(kbase + off),
                                             (__attribute__((address_space(3))) void*)(sK(buf) + piece * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vbase + off),
                                             (__attribute__((address_space(3))) void*)(sV(buf) + piece * 1024), 16, 0, 0);
        }
    };
    // The cross K arrives UN-scaled (wm_cross_kv stores the projection itself; the decode kernels scale it where they read it).  A DMA
    // cannot: once its own pieces of a tile have landed (vmcnt), every lane rewrites the 16 bytes it fetched with fp16(k * 64^-0.25),
    // in place -- elementwise, so the swizzle does not matter -- and the barrier that publishes the tile publishes the scaled rows.
    auto scale_k = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            half8v* ptr = (half8v*)(sK(buf) + (wid + 4 * i) * 1024 + lane * 16);
            half8v k = *ptr;
#pragma unroll
            for (int j = 0; j < 8; ++j) k[j] = (h16)r16_f32((float)k[j] * ATTN_SCALE);
            *ptr = k;
        }
    };
    // self: thread -> key row tid >> 2 of the tile, dims 16 (tid & 3) .. + 16 of k and of v; rows past L - 1 repeat row L - 1 (finite,
    // masked); the workgroup's own tile is appended to the cache on the way
    const float inv_t = 1.0f / p.kv_scale;
    auto stage_self = [&](int tile) __attribute__((always_inline)) {
        const int r = tid >> 2, c4 = tid & 3;
        const int slot = tile * PF_KEYS + r;
        const int key = slot > p.L - 1 ? p.L - 1 : slot;
        const size_t m = (size_t)b * p.L + key;
        const bool append = tile == qt && slot < p.L;
#pragma unroll
        for (int kv = 0; kv < 2; ++kv) {
            float x[16];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int col = (1 + kv) * C + h * 64 + c4 * 16 + i * 8;
                float v[8];
                slab_row8(p.part + m * p.ldp + col, p.ksplit, p.sstride, p.bias ? p.bias + col : nullptr, v);
#pragma unroll
                for (int j = 0; j < 8; ++j) x[i * 8 + j] = v[j];
            }
            unsigned char* dst = kv == 0 ? sK(0) : sV(0);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                half8v w;
#pragma unroll
                for (int j = 0; j < 8; ++j) w[j] = kv == 0 ? (h16)r16_f32(x[i * 8 + j] * ATTN_SCALE) : (h16)x[i * 8 + j];
                *(half8v*)(dst + r * PF_AROW + (((2 * c4 + i) ^ ((r >> 1) & 7)) << 4)) = w;
            }
            if (append) {
                const size_t off = (size_t)b * p.cache_bstride + ((size_t)(kv * p.H + h) * p.cap + slot) * 64 + c4 * 16;
                if constexpr (I8) {
                    union { int8_t c[16]; uint4 u; } q;
#pragma unroll
                    for (int j = 0; j < 16; ++j) q.c[j] = (int8_t)fminf(127.f, fmaxf(-128.f, rintf(mul_rn(x[j], inv_t))));
                    *(uint4*)((int8_t*)p.cache + off) = q.u;
                } else {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        half8v w;
#pragma unroll
                        for (int j = 0; j < 8; ++j) w[j] = (h16)x[i * 8 + j];
                        *(half8v*)((h16*)p.cache + off + i * 8) = w;
                    }
                }
            }
        }
    };

    float4v o[4][QB];
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) o[db][qb] = float4v{0.f, 0.f, 0.f, 0.f};
    float m_run[QB], l_run[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) { m_run[qb] = -INFINITY; l_run[qb] = 0.f; }

    // LDS addresses (attn_encoder.hip): K A-operand row = key li (+ 16 kb), chunks g and g + 4; V transposed read: lane i of its
    // 16-lane group supplies row 4 g + (i >> 2) (+ 16 for the upper half, + 32 c), 4 columns from 4 (i & 3) + 16 db
    const int k_swz = (li >> 1) & 7;
    const int k_off0 = li * PF_AROW + ((g ^ k_swz) << 4), k_off1 = li * PF_AROW + (((g + 4) ^ k_swz) << 4);
    const int v_row = 4 * g + (li >> 2), v_swz = (v_row >> 1) & 7;
    const int v_base = v_row * PF_AROW + (li & 1) * 8, v_chunk = (li & 3) >> 1;

    // one tile of 64 keys.  MASK: keys outside [lo, hi[qb]] get -inf; the 16-key blocks behind the wave's last visible key are
    // skipped outright (their exponentials would be +0, their P.V products 0 . v with v finite: every staged row is a real row)
    auto tile_body = [&](int t, const unsigned char* tK, const unsigned char* tV, auto MASK_) __attribute__((always_inline)) {
        constexpr bool MASK = decltype(MASK_)::value;
        int n_kb = 4;
        if constexpr (MASK) {
            const int kmax = SELF ? q_base + 16 * QB - 1 : p.Tk - 1;         // wave-uniform
            n_kb = ((kmax - t * PF_KEYS) >> 4) + 1;
            n_kb = n_kb > 4 ? 4 : (n_kb < 1 ? 1 : n_kb);
        }
        const int n_c = (n_kb + 1) >> 1;
        auto live_kb = [&](int kb) { return !MASK || kb < n_kb; };
        // ---- S^T = K . Q^T : [64 keys] x [16 QB queries] ------------------------------------------------
        float4v sacc[4][QB];
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            if (!live_kb(kb)) continue;
            const half8v k0 = *(const half8v*)(tK + k_off0 + kb * 16 * PF_AROW);
            const half8v k1 = *(const half8v*)(tK + k_off1 + kb * 16 * PF_AROW);
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
                float4v a = float4v{0.f, 0.f, 0.f, 0.f};
                a = __builtin_amdgcn_mfma_f32_16x16x32_f16(k0, qf[qb][0], a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_16x16x32_f16(k1, qf[qb][1], a, 0, 0, 0);
                sacc[kb][qb] = a;
            }
        }
        // ---- mask, round to fp16, online softmax (per lane = per query) ------------------------------------
        const int key0 = t * PF_KEYS + 4 * g;          // + 16 kb + r
        constexpr float LOG2E = 1.4426950408889634f;
        constexpr int NX = QB < 2 ? 2 : QB;            // (the swap helpers take 2 or 4 values)
        float mx[NX];
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            float m = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                if (!live_kb(kb)) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if constexpr (MASK) {
                        const int key = key0 + 16 * kb + r;
                        if (key < lo || key > hi[qb]) sacc[kb][qb][r] = -INFINITY;
                    }
                    m = fmaxf(m, sacc[kb][qb][r]);
                }
            }
            mx[qb] = m;
        }
#pragma unroll
        for (int qb = QB; qb < NX; ++qb) mx[qb] = mx[0];
        lane_xor_step<NX, true, false>(mx);
        lane_xor_step<NX, false, false>(mx);
        float mL[QB], alpha[QB];
        bool moved = false;
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            const float m_old = m_run[qb];
            const float m_new = fmaxf(m_old, r16(mx[qb]));
            // a query that has seen no key yet (pad slots, tiles in front of its row's start) keeps -inf as its maximum; its
            // exponentials are taken against 0 so that they are exp2(-inf) = 0, never exp2(-inf + inf)
            const float m_use = m_new == -INFINITY ? 0.f : m_new;
            float mn = __fmul_rn(m_use, LOG2E), mo = __fmul_rn(m_old, LOG2E);
            asm volatile("" : "+v"(mn), "+v"(mo));
            mL[qb] = mn;
            alpha[qb] = __builtin_amdgcn_exp2f(__fsub_rn(mo, mn));      // exp(m_old - m_new); 0 while m_old is -inf
            moved |= (m_new != m_old);
            m_run[qb] = m_new;
        }
        const bool any_moved = __builtin_amdgcn_ballot_w64(moved) != 0;     // wave-uniform
        half8v pf[2][QB];                              // P^T fragments per 32-key chunk
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            float ps = 0.f;
            const half2v one2 = {(h16)1.0f, (h16)1.0f};
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) {
                if (!live_kb(kb)) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) pf[kb >> 1][qb][(kb & 1) * 4 + r] = (h16)0.0f;
                    continue;
                }
#pragma unroll
                for (int r = 0; r < 4; r += 2) {
                    const half2v s2 = __builtin_convertvector(float2v{sacc[kb][qb][r], sacc[kb][qb][r + 1]}, half2v);
                    const float p0 = __builtin_amdgcn_exp2f(__fmaf_rn((float)s2[0], LOG2E, -mL[qb]));
                    const float p1 = __builtin_amdgcn_exp2f(__fmaf_rn((float)s2[1], LOG2E, -mL[qb]));
                    const half2v p2 = __builtin_convertvector(float2v{p0, p1}, half2v);
                    ps = __builtin_amdgcn_fdot2(p2, one2, ps, false);
                    pf[kb >> 1][qb][(kb & 1) * 4 + r] = p2[0];
                    pf[kb >> 1][qb][(kb & 1) * 4 + r + 1] = p2[1];
                }
            }
            l_run[qb] = __fmaf_rn(l_run[qb], alpha[qb], ps);     // this lane's keys only; the four lanes of a query meet at the end
        }
        if (any_moved) {
#pragma unroll
            for (int qb = 0; qb < QB; ++qb)
#pragma unroll
                for (int db = 0; db < 4; ++db) o[db][qb] *= alpha[qb];
        }
        // ---- O^T += V^T . P^T ----------------------------------------------------------------------------
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (MASK && c >= n_c) continue;
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                const unsigned char* va = tV + v_base + (c * 32) * PF_AROW + (((2 * db + v_chunk) ^ v_swz) << 4);
                const short4r lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4r*)(va));
                const short4r hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4r*)(va + 16 * PF_AROW));
                half8v vf;
                const half4v l4 = __builtin_bit_cast(half4v, lo4), h4 = __builtin_bit_cast(half4v, hi4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { vf[j] = l4[j]; vf[4 + j] = h4[j]; }
#pragma unroll
                for (int qb = 0; qb < QB; ++qb) o[db][qb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf[c][qb], o[db][qb], 0, 0, 0);
            }
        }
    };

    if constexpr (SELF) {
        for (int t = t_first; t <= t_last; ++t) {
            __syncthreads();                           // the tile before has been read
            stage_self(t);
            __syncthreads();
            if (has_q) tile_body(t, sK(0), sV(0), std::true_type{});
        }
    } else {
        load_kv(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        scale_k(0);
        __syncthreads();
        for (int t = 0; t <= t_last; ++t) {
            const int cur = t & 1;
            if (t < t_last) load_kv(t + 1, cur ^ 1);   // lands while this tile is multiplied; nobody reads that buffer before the barrier below
            if (has_q) {
                if (t == t_last && (p.Tk & 63) != 0) tile_body(t, sK(cur), sV(cur), std::true_type{});
                else tile_body(t, sK(cur), sV(cur), std::false_type{});
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (t < t_last) scale_k(cur ^ 1);          // this wave's pieces of the next tile have landed
            __syncthreads();
        }
    }
    if (!has_q) return;

    // ---- normalise and store: lane owns query li, dims 16 db + 4 g + r ------------------------------------
    {
        constexpr int NX = QB < 2 ? 2 : QB;
        float ls[NX];
#pragma unroll
        for (int qb = 0; qb < NX; ++qb) ls[qb] = l_run[qb < QB ? qb : 0];
        lane_xor_step<NX, true, true>(ls);
        lane_xor_step<NX, false, true>(ls);
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) l_run[qb] = ls[qb];
    }
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const int qrow = q_base + qb * 16 + li;
        if (qrow >= p.L) continue;
        const bool pad = SELF && qrow < start;
        const float inv = 1.0f / l_run[qb];
        h16* dst = p.out + ((size_t)b * p.L + qrow) * p.ldo + h * 64;
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            half4v w;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float t = o[db][qb][r] * inv;          // fp32 product, THEN fp16 (attn_encoder.hip: no mixed-precision fma here)
                asm volatile("" : "+v"(t));
                w[r] = pad ? (h16)0.0f : (h16)t;
            }
            *(half4v*)(dst + db * 16 + g * 4) = w;
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int launch_attn_prefill_self(const AttnSelfParams& a, hipStream_t stream) {
    WM_REQUIRE(a.part && a.present && a.out, "attn_prefill_self: null argument");
    WM_REQUIRE(a.B >= 1 && a.H >= 1 && a.L >= 1 && a.ksplit >= 1, "attn_prefill_self: bad shape (B %d, L %d, H %d, ksplit %d)", a.B, a.L, a.H, a.ksplit);
    WM_REQUIRE(a.T == 0 && !a.t_dev, "attn_prefill_self: the block goes on an empty cache (T = %d)", a.T);
    WM_REQUIRE(a.present_cap >= a.L, "attn_prefill_self: cache capacity %d < L = %d", a.present_cap, a.L);
    WM_REQUIRE(!a.amax, "attn_prefill_self: no calibration hook");
    WM_REQUIRE(!a.int8_kv || a.kv_scale > 0.f, "attn_prefill_self: the int8 cache needs a positive scale");
    WM_REQUIRE(a.ldp % 4 == 0 && a.ldo % 4 == 0 && a.part_sstride % 4 == 0 && a.present_bstride % 16 == 0 && aligned16(a.part) &&
               aligned16(a.present) && ((uintptr_t)a.out & 7) == 0, "attn_prefill_self: buffers and leading dimensions must keep 16-byte alignment");
    PrefillParams p{};
    p.part = a.part; p.ksplit = a.ksplit; p.ldp = a.ldp;
    p.sstride = a.part_sstride ? (size_t)a.part_sstride : (size_t)a.B * a.L * a.ldp;
    p.bias = a.bias; p.B = a.B; p.L = a.L; p.H = a.H;
    p.cache = a.present; p.cache_bstride = a.present_bstride; p.cap = a.present_cap; p.kv_scale = a.int8_kv ? a.kv_scale : 1.f;
    p.out = a.out; p.ldo = a.ldo; p.live = a.live; p.row_start = a.row_start;
    const int nx = (a.L + 63) / 64;
    const dim3 grid((unsigned)(a.B * a.H * nx));
    if (a.int8_kv) hipLaunchKernelGGL((attn_prefill_kernel<true, true, 1>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((attn_prefill_kernel<true, false, 1>), grid, dim3(256), 0, stream, p);
    WM_LAUNCH_CHECK(stream, "attn_prefill_self");
    return 0;
}

int launch_attn_prefill_cross(const AttnCrossParams& a, hipStream_t stream) {
    WM_REQUIRE(a.part && a.kv && a.out, "attn_prefill_cross: null argument");
    WM_REQUIRE(a.B >= 1 && a.H >= 1 && a.L >= 1 && a.Tk >= 1 && a.ksplit >= 1, "attn_prefill_cross: bad shape (B %d, L %d, H %d, Tk %d, ksplit %d)",
               a.B, a.L, a.H, a.Tk, a.ksplit);
    WM_REQUIRE(a.kv_q8_scale <= 0.f, "attn_prefill_cross: int8 cross K/V is not supported");
    WM_REQUIRE(a.G <= 1, "attn_prefill_cross: no candidate groups");
    WM_REQUIRE(a.ldp % 4 == 0 && a.ldo % 4 == 0 && a.part_sstride % 4 == 0 && a.kv_bstride % 8 == 0 && aligned16(a.part) && aligned16(a.kv) &&
               ((uintptr_t)a.out & 7) == 0, "attn_prefill_cross: buffers and leading dimensions must keep 16-byte alignment");
    PrefillParams p{};
    p.part = a.part; p.ksplit = a.ksplit; p.ldp = a.ldp;
    p.sstride = a.part_sstride ? (size_t)a.part_sstride : (size_t)a.B * a.L * a.ldp;
    p.bias = a.bias; p.B = a.B; p.L = a.L; p.H = a.H; p.Tk = a.Tk;
    p.kv = a.kv; p.kv_bstride = a.kv_bstride;
    p.out = a.out; p.ldo = a.ldo; p.live = a.live;
    const int heads8 = 8 * ((a.H * a.B + 7) / 8);
    // QB by L alone: the two instantiations need not agree bit for bit, and a row's result must not depend on the batch it is in
    if (a.L > 64) hipLaunchKernelGGL((attn_prefill_kernel<false, false, 2>), dim3((unsigned)(heads8 * ((a.L + 127) / 128))), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((attn_prefill_kernel<false, false, 1>), dim3((unsigned)heads8), dim3(256), 0, stream, p);
    WM_LAUNCH_CHECK(stream, "attn_prefill_cross");
    return 0;
}

}  // namespace wm
