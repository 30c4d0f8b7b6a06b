// The arithmetic of the decode attention, written ONCE: the stand-alone kernels (attn_decode.hip) and the stages of the one-launch
// step (gemv_chain.hip) keep their own data movement and inline these bodies, so two forms of a step cannot round differently.
// Every function states its rounding points; operation order is part of the contract (tests/kernel_refs.py restates it).  At the
// end: the weight-tile expansion the Linears around the attention share where it costs no register.
#pragma once
#include "common.h"

namespace wm {

constexpr float ATTN_SCALE = 0.35355339059327373f;    // 64^-0.25: q and k each carry half of d^-0.5

// ---- shared by self- and cross-attention ---------------------------------------------------------------------------------
// x * 64^-0.25: the fp32 product, then fp16 (x is an fp16 value: a projected q or k element)
__device__ __forceinline__ float attn_scaled(float x) { return r16(x * ATTN_SCALE); }
// a projected q / k / v element: the fp32 sum of the split-K slabs plus the bias, rounded to fp16
__device__ __forceinline__ float qkv_round(float sum, float bias) { return r16(sum + bias); }
// eight dims of one V row weighted into o: one fused multiply-add each, no intermediate rounding (pr and hv are fp16 values)
__device__ __forceinline__ void pv_row8(float pr, const half8v& hv, float* o) {
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = fmaf(pr, (float)hv[e], o[e]);
}

// ---- cross-attention, fp16 K/V: a lane holds 8 dims of a key row, 8 lanes share the row --------------------------------------
// q of ONE slab, bias added, rounded to fp16, scaled, rounded to fp16.  The two additions are attn_cross_kernel's pairing of
// slabs at ksplit = 1 (slab + absent, absent + absent): -0.0 sums come out as +0.0 there, so they do here.
__device__ __forceinline__ float cross_q_one_slab(float x, h16 bias) {
    float qa = 0.f;
    qa += x + 0.f;
    qa += 0.f + 0.f;
    return attn_scaled(qkv_round(qa, (float)bias));
}
// the lane's eight key values, each scaled and rounded to fp16 (once per row, whatever the number of queries)
__device__ __forceinline__ void cross_scaled_key(const half8v& hv, float* ks) {
#pragma unroll
    for (int e = 0; e < 8; ++e) ks[e] = attn_scaled((float)hv[e]);
}
// the lane's share of q . k: a chain of eight fused multiply-adds from 0, dims in ascending order, fp32 throughout
__device__ __forceinline__ float cross_dot8(const float* qf, const float* ks) {
    float acc = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = fmaf(qf[e], ks[e], acc);
    return acc;
}
// the row's score on each of its eight lanes: lane ^ 1, lane ^ 2, then the other quad (row_half_mirror), fp32 sums; the total is
// rounded to fp16 as a value of its own (f32_as_is: never folded into the last addition)
__device__ __forceinline__ float cross_row_score(float acc) {
    acc += wave_dpp<0xB1>(acc);
    acc += wave_dpp<0x4E>(acc);
    acc += wave_dpp<0x141>(acc);
    return r16(f32_as_is(acc));
}
// eight partial P.V sums of a lane added over the wave's eight rows: lane ^ 8 (row_ror:8), ^ 16, ^ 32 -- fp32, own + partner
__device__ __forceinline__ void cross_o_tail8(float* o) {
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] += wave_dpp<0x128>(o[e]);
    wave_add_xor16_x8_nomfma(o);          // (no matrix instruction of the wave is in flight at any call site)
    wave_add_xor32_x8_nomfma(o);
}

// ---- the merge of the cross-attention's key-range pieces -------------------------------------------------------------------
// a piece's weight against the maximum of all pieces (an empty piece: exp(-inf) = 0)
__device__ __forceinline__ float merge_weight(float m_piece, float m) { return __expf(m_piece - m); }
// four (max, sum, o) triples -> the output value: every product rounded to fp32 on its own (mul_rn), den and num summed in piece
// order from 0, one division, fp16
__device__ __forceinline__ h16 merge_pieces4(const float* mq, const float* lq, const float* oq) {
    const float m = fmaxf(fmaxf(mq[0], mq[1]), fmaxf(mq[2], mq[3]));
    float den = 0.f, num = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float f = merge_weight(mq[q], m);
        den += mul_rn(lq[q], f);
        num += mul_rn(oq[q], f);
    }
    return (h16)(num / den);
}

// ---- self-attention ------------------------------------------------------------------------------------------------------------
// int8 cache code of a new k / v element: x / t as x * (1 / t) in fp32, round to nearest even, saturate
__device__ __forceinline__ int8_t kv_cache_code(float x, float inv_t) { return (int8_t)fminf(127.f, fmaxf(-128.f, rintf(x * inv_t))); }
// eight dims of q . k onto acc: the key element scaled and rounded to fp16, then one fused multiply-add, dims in ascending order
__device__ __forceinline__ float self_score_chunk8(const h16* q8, const half8v& w, float acc) {
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = fmaf((float)q8[e], attn_scaled((float)w[e]), acc);
    return acc;
}

// ---- the Linears around the attention ----------------------------------------------------------------------------------------
// A lane's 16 bytes of a 1 KiB weight tile as the fp16 B operands of the 16x16x32 MFMA (one for fp16 weights, two for int8, four for
// int4): fp16 as stored; int8 / int4 codes through the 1024 + u trick, every step exact -- no rounding point at all.
template <int WB> struct WeightTile { half8v b[WB == 16 ? 1 : (WB == 8 ? 2 : 4)]; };
template <int WB>
__device__ __forceinline__ WeightTile<WB> expand_weight_tile(u32x4 w) {
    WeightTile<WB> t;
    if constexpr (WB == 16) {
        t.b[0] = __builtin_bit_cast(half8v, w);
    } else if constexpr (WB == 8) {
        half2v h[8];
        cvt_s8x4_f16x4(w.x, h[0], h[1]);
        cvt_s8x4_f16x4(w.y, h[2], h[3]);
        cvt_s8x4_f16x4(w.z, h[4], h[5]);
        cvt_s8x4_f16x4(w.w, h[6], h[7]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            t.b[0][2 * q] = h[q][0]; t.b[0][2 * q + 1] = h[q][1];
            t.b[1][2 * q] = h[4 + q][0]; t.b[1][2 * q + 1] = h[4 + q][1];
        }
    } else {
        const uint32_t wv[4] = {w.x, w.y, w.z, w.w};
        const half2v bias8 = {(h16)1032.0f, (h16)1032.0f};
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int sft = 0; sft < 4; ++sft) {
                const uint32_t bits = ((wv[m] >> (4 * sft)) & 0x000F000Fu) | 0x64006400u;   // fp16 (1024 + u) x 2
                const half2v pr = __builtin_bit_cast(half2v, bits) - bias8;                  // u - 8 = q, exact
                t.b[m][2 * sft] = pr[0]; t.b[m][2 * sft + 1] = pr[1];
            }
    }
    return t;
}

}  // namespace wm
