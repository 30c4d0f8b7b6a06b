// wm_resample: any-rate interleaved PCM -> mono fp32 at 16 kHz in one launch (whisper_utils.resample_device).
//
// The filter is whisper_utils.resample_filter's table (the contract, computed on the host in fp64 and rounded once to fp32): with
// L = 16000 / g, M = rate / g, g = gcd(rate, 16000), output n sits at input time n M / L; with i = floor(n M / L), p = (n M) mod L
//   y[n] = sum_{j = 0 .. T - 1} H[p][j] * x[i - half + j],   T = 2 half + 1,   x zero outside [0, n_in)
// and x is the downmix of the interleaved input, formed while it is staged:
//   x[k] = (fp32(v[k][0]) + fp32(v[k][1]) + ...  in channel order, in fp32) / fp32(channels) * scale.
//
// A workgroup owns RS_TILE consecutive outputs.  It stages the input span they reach, [i(first) - half, i(last) + half], in LDS
// as downmixed fp32 (zeros outside the file) -- at most (L - 1 + (RS_TILE - 1) M) / L + T floats, what the launcher asks for: 13131
// (51 KiB) at 192 kHz, 3017 at 44.1 kHz -- and then
// one lane owns one output: T fp32 FMAs in tap order j = 0 .. T - 1, nothing shared between lanes, so a result does not depend on
// the tile it fell into and two runs are bitwise equal.
//
// The table arrives transposed and ordered by r = n mod L:  table[j][r] = H[(r M) mod L][j], fp32 [T][L].  p depends on n only
// through n mod L, so lane n reads table[j][n mod L]: consecutive lanes read consecutive coefficients (wrapping at L) and write
// consecutive outputs; with L = 1 (48 kHz, 96 kHz, ...) the coefficient is the same for the whole wave.  At most a few hundred KiB
// for the common rates: it stays in L2.
//
// Indices: n M passes 2^31 after five minutes of 44.1 kHz audio.  The first output of a tile is split in 64-bit arithmetic,
// n0 M = q0 L + p0 and r0 = n0 mod L, once per workgroup; inside the tile p0 + d M and r0 + d, with d < RS_TILE, p0, r0 < L and
// L, M <= 2^20 (checked), stay below 2^31: one 32-bit division and one 32-bit remainder per output.
#include "kernels.h"
#include "../../include/whisper_mi355.h"

namespace wm {
namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_TILE = 1024;              // outputs per workgroup, RS_TILE / RS_THREADS per lane
constexpr long RS_MAX_SPAN = 15 * 1024;    // floats of LDS a tile may ask for (60 KiB)

template <typename V>
__device__ __forceinline__ float rs_downmix(const V* pcm, long k, int channels, float fch, float scale) {
    const V* v = pcm + k * channels;
    float s = (float)v[0];
    for (int c = 1; c < channels; ++c) s += (float)v[c];
    return s / fch * scale;
}

template <typename V>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const V* __restrict__ pcm, int channels, long n_in, float scale,
                                                              const float* __restrict__ table, int L, int M, int half,
                                                              float* __restrict__ out, long n_out) {
    extern __shared__ float xs[];
    const long n0 = (long)blockIdx.x * RS_TILE;
    const long nm0 = n0 * (long)M;
    const long q0 = nm0 / L;
    const int p0 = (int)(nm0 - q0 * L);
    const int r0 = (int)(n0 % L);
    const int count = (int)(n_out - n0 < RS_TILE ? n_out - n0 : RS_TILE);
    const int T = 2 * half + 1;
    // the last output's offset from q0, then the span [q0 - half, q0 + last + half]: p0 <= L - 1 and count <= RS_TILE, so span is
    // at most the (L - 1 + (RS_TILE - 1) M) / L + T floats of LDS the launcher asked for
    const int span = (p0 + (count - 1) * M) / L + T;
    const long k0 = q0 - half;
    const float fch = (float)channels;
    for (int s = threadIdx.x; s < span; s += RS_THREADS) {
        const long k = k0 + s;
        xs[s] = (k >= 0 && k < n_in) ? rs_downmix(pcm, k, channels, fch, scale) : 0.f;
    }
    __syncthreads();
    for (int d = threadIdx.x; d < count; d += RS_THREADS) {
        const int r = (r0 + d) % L;
        const int base = (p0 + d * M) / L;         // i(n) - q0: tap j reads xs[base + j]
        const float* h = table + r;
        float acc = 0.f;                           // base <= the last output's offset: base + T <= span
#pragma unroll 4
        for (int j = 0; j < T; ++j) acc = fmaf(xs[base + j], h[(long)j * L], acc);
        out[n0 + d] = acc;
    }
}

// The channel form (wm_resample_channels): the same tile, the same tap order and the same table, but the staging SELECTS channel
// blockIdx.y instead of summing -- x_c[k] = fp32(v[k][c]) / 1 * scale, the expression the downmix has for a mono file -- and the
// output is row c of out [channels][out_ld].  All channels in one launch: the interleaved input is read once per channel from L2
// instead of being copied apart first.
template <typename V>
__global__ __launch_bounds__(RS_THREADS) void resample_channels_kernel(const V* __restrict__ pcm, int channels, long n_in, float scale,
                                                                       const float* __restrict__ table, int L, int M, int half,
                                                                       float* __restrict__ out, long out_ld, long n_out) {
    extern __shared__ float xs[];
    const int c = blockIdx.y;
    const long n0 = (long)blockIdx.x * RS_TILE;
    const long nm0 = n0 * (long)M;
    const long q0 = nm0 / L;
    const int p0 = (int)(nm0 - q0 * L);
    const int r0 = (int)(n0 % L);
    const int count = (int)(n_out - n0 < RS_TILE ? n_out - n0 : RS_TILE);
    const int T = 2 * half + 1;
    const int span = (p0 + (count - 1) * M) / L + T;       // at most the launcher's span_cap, as in resample_kernel
    const long k0 = q0 - half;
    for (int s = threadIdx.x; s < span; s += RS_THREADS) {
        const long k = k0 + s;
        xs[s] = (k >= 0 && k < n_in) ? rs_downmix(pcm + c, k * channels, 1, 1.0f, scale) : 0.f;
    }
    __syncthreads();
    float* row = out + (long)c * out_ld;
    for (int d = threadIdx.x; d < count; d += RS_THREADS) {
        const int r = (r0 + d) % L;
        const int base = (p0 + d * M) / L;
        const float* h = table + r;
        float acc = 0.f;
#pragma unroll 4
        for (int j = 0; j < T; ++j) acc = fmaf(xs[base + j], h[(long)j * L], acc);
        row[n0 + d] = acc;
    }
}

}  // namespace

int launch_resample(const void* pcm, int dtype, int channels, long n_in, float scale, const float* table, int L, int M, int half,
                    float* out, long n_out, hipStream_t stream) {
    const long T = 2L * half + 1;
    const long span_cap = ((long)L - 1 + (long)(RS_TILE - 1) * M) / L + T;       // the widest tile: p0 = L - 1, RS_TILE outputs (the kernel's span never exceeds it)
    WM_REQUIRE(span_cap <= RS_MAX_SPAN, "wm_resample: L=%d M=%d half=%d need %ld floats of LDS per tile (at most %ld)", L, M, half,
               span_cap, RS_MAX_SPAN);
    const long grid = (n_out + RS_TILE - 1) / RS_TILE;
    WM_REQUIRE(grid <= 0x7fffffffL, "wm_resample: %ld outputs are more than one launch takes", n_out);
    const size_t lds = (size_t)span_cap * sizeof(float);
    const dim3 g((unsigned)grid), b(RS_THREADS);
    if (dtype == 0)
        hipLaunchKernelGGL(resample_kernel<float>, g, b, lds, stream, (const float*)pcm, channels, n_in, scale, table, L, M, half, out,
                           n_out);
    else if (dtype == 1)
        hipLaunchKernelGGL(resample_kernel<int16_t>, g, b, lds, stream, (const int16_t*)pcm, channels, n_in, scale, table, L, M, half,
                           out, n_out);
    else
        hipLaunchKernelGGL(resample_kernel<int32_t>, g, b, lds, stream, (const int32_t*)pcm, channels, n_in, scale, table, L, M, half,
                           out, n_out);
    WM_LAUNCH_CHECK(stream, "resample");
    return 0;
}

int launch_resample_channels(const void* pcm, int dtype, int channels, long n_in, float scale, const float* table, int L, int M,
                             int half, float* out, long out_ld, long n_out, hipStream_t stream) {
    const long T = 2L * half + 1;
    const long span_cap = ((long)L - 1 + (long)(RS_TILE - 1) * M) / L + T;
    WM_REQUIRE(span_cap <= RS_MAX_SPAN, "wm_resample_channels: L=%d M=%d half=%d need %ld floats of LDS per tile (at most %ld)", L, M,
               half, span_cap, RS_MAX_SPAN);
    const long grid = (n_out + RS_TILE - 1) / RS_TILE;
    WM_REQUIRE(grid <= 0x7fffffffL, "wm_resample_channels: %ld outputs are more than one launch takes", n_out);
    const size_t lds = (size_t)span_cap * sizeof(float);
    const dim3 g((unsigned)grid, (unsigned)channels), b(RS_THREADS);
    if (dtype == 0)
        hipLaunchKernelGGL(resample_channels_kernel<float>, g, b, lds, stream, (const float*)pcm, channels, n_in, scale, table, L, M,
                           half, out, out_ld, n_out);
    else if (dtype == 1)
        hipLaunchKernelGGL(resample_channels_kernel<int16_t>, g, b, lds, stream, (const int16_t*)pcm, channels, n_in, scale, table, L,
                           M, half, out, out_ld, n_out);
    else
        hipLaunchKernelGGL(resample_channels_kernel<int32_t>, g, b, lds, stream, (const int32_t*)pcm, channels, n_in, scale, table, L,
                           M, half, out, out_ld, n_out);
    WM_LAUNCH_CHECK(stream, "resample_channels");
    return 0;
}

}  // namespace wm

using namespace wm;

extern "C" int wm_resample(const void* pcm, int dtype, int channels, int64_t n_in, float scale, const float* table, int L, int M,
                           int half, float* out, int64_t n_out, wm_stream_t stream) {
    WM_REQUIRE(pcm && table && out, "wm_resample: null argument");
    WM_REQUIRE(dtype >= 0 && dtype <= 2, "wm_resample: dtype %d is not 0 (f32), 1 (i16) or 2 (i32)", dtype);
    WM_REQUIRE(channels >= 1 && channels <= 8, "wm_resample: %d channels (1..8)", channels);
    WM_REQUIRE(L >= 1 && M >= 1 && half >= 1, "wm_resample: L=%d M=%d half=%d must be >= 1", L, M, half);
    WM_REQUIRE(L != M, "wm_resample: L == M = %d is no rate change", L);
    WM_REQUIRE(L <= (1 << 20) && M <= (1 << 20) && half <= (1 << 16), "wm_resample: L=%d M=%d half=%d out of range", L, M, half);
    WM_REQUIRE(n_in >= 1 && n_in <= (int64_t)1 << 40, "wm_resample: n_in=%lld", (long long)n_in);
    const int64_t want = (n_in * L + M - 1) / M;
    WM_REQUIRE(n_out == want, "wm_resample: n_out=%lld, ceil(n_in L / M) = %lld", (long long)n_out, (long long)want);
    return launch_resample(pcm, dtype, channels, (long)n_in, scale, table, L, M, half, out, (long)n_out, (hipStream_t)stream);
}

extern "C" int wm_resample_channels(const void* pcm, int dtype, int channels, int64_t n_in, float scale, const float* table, int L,
                                    int M, int half, float* out, int64_t out_ld, int64_t n_out, wm_stream_t stream) {
    WM_REQUIRE(pcm && table && out, "wm_resample_channels: null argument");
    WM_REQUIRE(dtype >= 0 && dtype <= 2, "wm_resample_channels: dtype %d is not 0 (f32), 1 (i16) or 2 (i32)", dtype);
    WM_REQUIRE(channels >= 1 && channels <= 8, "wm_resample_channels: %d channels (1..8)", channels);
    WM_REQUIRE(L >= 1 && M >= 1 && half >= 1, "wm_resample_channels: L=%d M=%d half=%d must be >= 1", L, M, half);
    WM_REQUIRE(L != M, "wm_resample_channels: L == M = %d is no rate change", L);
    WM_REQUIRE(L <= (1 << 20) && M <= (1 << 20) && half <= (1 << 16), "wm_resample_channels: L=%d M=%d half=%d out of range", L, M, half);
    WM_REQUIRE(n_in >= 1 && n_in <= (int64_t)1 << 40, "wm_resample_channels: n_in=%lld", (long long)n_in);
    const int64_t want = (n_in * L + M - 1) / M;
    WM_REQUIRE(n_out == want, "wm_resample_channels: n_out=%lld, ceil(n_in L / M) = %lld", (long long)n_out, (long long)want);
    WM_REQUIRE(out_ld >= n_out, "wm_resample_channels: out_ld=%lld is below n_out=%lld", (long long)out_ld, (long long)n_out);
    return launch_resample_channels(pcm, dtype, channels, (long)n_in, scale, table, L, M, half, out, (long)out_ld, (long)n_out,
                                    (hipStream_t)stream);
}
