// The integer loudness of a ragged batch of whole-file log-mels: the passes that wm_section_cuts (sections.hip) and
// wm_speech_spans (speech.hip) share, so that the arithmetic has one definition (sections.py: loudness, smooth).
//
// Every file b of the batch is src[b] fp16 [n_mels][src_ld[b]] with content[b] frames of content.  In integers:
//   q[t] = sum_m rint(clamp(src[m][t], -16, 16) * 1024)        (a non-finite element: 0)
//   s[t] = sum_{d = -h .. h} q[clamp(t + d, 0, F - 1)]
// A term is at most 16384 in magnitude and n_mels * (2h + 1) < 131072, so every sum fits 32 bits and no order of summation can
// change a result.
//
// Three launches, everything per file read on the device; the files' frames stand one after the other in q and s:
//   offsets   one workgroup: the files' first frames in the workspace, a prefix sum of their content (clamped to [0, src_ld], 0
//             for a null file); a file WITH frames that end beyond total_frames takes no part (the caller reports -1 for it);
//   loudness  the bandwidth-bound pass: one thread per frame of the concatenated files, a loop over the mel bins; consecutive
//             lanes read consecutive frames of one row, 2-byte loads (src_ld and the base may be odd), eight rows in flight;
//             element m * src_ld + t with t < F <= src_ld, m < n_mels: never outside the file's array;
//   smoothing one thread per frame: the taps inside [0, F - 1] one by one (q is 4 bytes a frame: cache traffic), the taps clamped
//             to an end as a count times the end's value.
#pragma once
#include "kernels.h"

namespace wm {
namespace {

constexpr int SC_THREADS = 256;

#define SC_GLOBAL __attribute__((address_space(1)))

__host__ __device__ inline size_t sc_align(size_t n) { return (n + 255) & ~(size_t)255; }

// the frames of file b that take part: content clamped to [0, src_ld], none for a null file
__device__ __forceinline__ long sc_frames(const void* const* src, const int32_t* src_ld, const int32_t* content, int b) {
    if (!src[b]) return 0;
    const long ld = src_ld[b] > 0 ? src_ld[b] : 0, F = content[b] > 0 ? content[b] : 0;
    return F < ld ? F : ld;
}

// off[b] = sum_{i < b} frames(i), off[batch] the total: every thread sums a run of files, thread 0 scans the 256 sums
__global__ __launch_bounds__(SC_THREADS) void sc_offsets_kernel(const void* const* src, const int32_t* src_ld,
                                                                const int32_t* content, int batch, long long* off) {
    __shared__ long long part[SC_THREADS];
    const int per = (batch + SC_THREADS - 1) / SC_THREADS;
    const int b0 = min(batch, (int)threadIdx.x * per), b1 = min(batch, b0 + per);
    long long sum = 0;
    for (int b = b0; b < b1; ++b) sum += sc_frames(src, src_ld, content, b);
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int i = 0; i < SC_THREADS; ++i) {
            const long long v = part[i];
            part[i] = run;
            run += v;
        }
        off[batch] = run;
    }
    __syncthreads();
    long long run = part[threadIdx.x];
    for (int b = b0; b < b1; ++b) {
        off[b] = run;
        run += sc_frames(src, src_ld, content, b);
    }
}

// The file of frame g of the concatenation: the last b with off[b] <= g (files without frames share their offset with the next
// file and are never the answer).  The search starts from the workgroup's first frame, so it is the same for all its threads but
// the few that sit behind a file's end.
__device__ __forceinline__ int sc_file_of(const long long* off, int batch, long long g_first, long long g) {
    int lo = 0, hi = batch - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= g_first) lo = mid; else hi = mid - 1;
    }
    while (lo + 1 < batch && off[lo + 1] <= g) ++lo;
    return lo;
}

__device__ __forceinline__ int sc_term(h16 x) {
    const float v = (float)x;
    if (!(fabsf(v) <= 65504.0f)) return 0;                      // infinities and NaNs
    return (int)rintf(fminf(fmaxf(v, -16.0f), 16.0f) * 1024.0f);
}

__global__ __launch_bounds__(SC_THREADS) void sc_loudness_kernel(const void* const* src, const int32_t* src_ld, int batch,
                                                                 int n_mels, const long long* off, long long total_frames,
                                                                 int32_t* q) {
    const long long g_first = (long long)blockIdx.x * SC_THREADS, g = g_first + threadIdx.x;
    if (g >= off[batch] || g >= total_frames) return;
    const int b = sc_file_of(off, batch, g_first, g);
    if (off[b + 1] > total_frames) return;                      // the file does not fit the workspace: the caller reports -1
    const long t = (long)(g - off[b]), ld = src_ld[b];
    const SC_GLOBAL h16* p = (const SC_GLOBAL h16*)src[b] + t;
    int sum = 0, m = 0;
    for (; m + 8 <= n_mels; m += 8) {
        h16 x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = p[(long)(m + k) * ld];
#pragma unroll
        for (int k = 0; k < 8; ++k) sum += sc_term(x[k]);
    }
    for (; m < n_mels; ++m) sum += sc_term(p[(long)m * ld]);
    q[g] = sum;
}

__global__ __launch_bounds__(SC_THREADS) void sc_smooth_kernel(int batch, int h, const long long* off, long long total_frames,
                                                               const int32_t* q, int32_t* s) {
    const long long g_first = (long long)blockIdx.x * SC_THREADS, g = g_first + threadIdx.x;
    if (g >= off[batch] || g >= total_frames) return;
    const int b = sc_file_of(off, batch, g_first, g);
    if (off[b + 1] > total_frames) return;
    const long long base = off[b];
    const long F = (long)(off[b + 1] - base), t = (long)(g - base);
    const long first = t - h > 0 ? t - h : 0, last = t + h < F - 1 ? t + h : F - 1;
    // unsigned: the sum of the clamped taps may pass 2^31 on its way, the result does not
    uint32_t sum = (uint32_t)(first - (t - h)) * (uint32_t)q[base] + (uint32_t)(t + h - last) * (uint32_t)q[base + F - 1];
    for (long u = first; u <= last; ++u) sum += (uint32_t)q[base + u];
    s[g] = (int32_t)sum;
}

// off, q and s of `total_frames` frames at the head of a workspace: their bytes, and the three launches that fill them
__host__ inline size_t sc_smoothed_bytes(int batch, long long total_frames) {
    return sc_align((size_t)(batch + 1) * sizeof(long long)) + 2 * sc_align((size_t)total_frames * sizeof(int32_t));
}

struct ScSmoothed {
    long long* off;
    int32_t* q;
    int32_t* s;
};

__host__ inline ScSmoothed sc_smoothed_at(void* workspace, int batch, long long total_frames) {
    char* ws = (char*)workspace;
    ScSmoothed r;
    r.off = (long long*)ws;
    r.q = (int32_t*)(ws + sc_align((size_t)(batch + 1) * sizeof(long long)));
    r.s = (int32_t*)((char*)r.q + sc_align((size_t)total_frames * sizeof(int32_t)));
    return r;
}

// what[3]: the launches' names in an error message
__host__ inline int sc_launch_smoothed(const void* const* src, const int32_t* src_ld, const int32_t* content, int batch, int n_mels,
                                       int h, const ScSmoothed& w, long long total_frames, hipStream_t stream,
                                       const char* const* what) {
    hipLaunchKernelGGL(sc_offsets_kernel, dim3(1), dim3(SC_THREADS), 0, stream, src, src_ld, content, batch, w.off);
    WM_LAUNCH_CHECK(stream, what[0]);
    const long long grid = (total_frames + SC_THREADS - 1) / SC_THREADS;
    if (grid > 0) {
        hipLaunchKernelGGL(sc_loudness_kernel, dim3((unsigned)grid), dim3(SC_THREADS), 0, stream, src, src_ld, batch, n_mels, w.off,
                           total_frames, w.q);
        WM_LAUNCH_CHECK(stream, what[1]);
        hipLaunchKernelGGL(sc_smooth_kernel, dim3((unsigned)grid), dim3(SC_THREADS), 0, stream, batch, h, w.off, total_frames, w.q,
                           w.s);
        WM_LAUNCH_CHECK(stream, what[2]);
    }
    return 0;
}

}  // namespace
}  // namespace wm
