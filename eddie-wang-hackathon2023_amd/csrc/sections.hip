// wm_section_cuts: where to cut long files into sections that are decoded side by side (sections.py states the contract,
// DESIGN.md section 5g).
//
// Every file b of the batch is a whole-file log-mel src[b] fp16 [n_mels][src_ld[b]] with content[b] frames of content.  In integers:
//   q[t] = sum_m rint(clamp(src[m][t], -16, 16) * 1024)        (a non-finite element: 0)
//   s[t] = sum_{d = -h .. h} q[clamp(t + d, 0, F - 1)]
//   c = 0; while F - c > hi: c = the t of [c + lo, c + hi] with the smallest s[t], the largest t among equals; a cut.
// A term is at most 16384 in magnitude and n_mels * (2h + 1) < 131072, so every sum fits 32 bits and no order of summation can
// change a result: the cuts are sections.py's exactly.
//
// Four launches on the caller's stream, everything per file read on the device (the first three are loudness.h's, shared with
// wm_speech_spans):
//   offsets   one workgroup: the files' first frames in the workspace, a prefix sum of their content (clamped to [0, src_ld], 0
//             for a null file); a file WITH frames that end beyond total_frames takes no part and reports n_cuts = -1;
//   loudness  the bandwidth-bound pass: one thread per frame of the concatenated files, a loop over the mel bins; consecutive
//             lanes read consecutive frames of one row, 2-byte loads (src_ld and the base may be odd), eight rows in flight;
//             element m * src_ld + t with t < F <= src_ld, m < n_mels: never outside the file's array;
//   smoothing one thread per frame: the taps inside [0, F - 1] one by one (q is 4 bytes a frame: cache traffic), the taps clamped
//             to an end as a count times the end's value;
//   search    one workgroup per file walks the cuts: a strided scan of the hi - lo + 1 candidates (all below F: c + hi < F),
//             a minimum over (value, index) keys in the wave (xor butterfly) and across the waves through LDS.  The key is
//             value << 32 | (2^31 - 1 - index): the smaller value wins, then the larger index, whatever the order of the merge.
#include "loudness.h"
#include "../../include/whisper_mi355.h"

namespace wm {
namespace {

constexpr long long SC_NO_KEY = 0x7fffffffffffffffLL;

__device__ __forceinline__ long long sc_min(long long a, long long b) { return a < b ? a : b; }

__global__ __launch_bounds__(SC_THREADS) void sc_search_kernel(const void* const* src, const int32_t* src_ld,
                                                               const int32_t* content, int lo, int hi, const long long* off,
                                                               long long total_frames, const int32_t* s, int32_t* cuts,
                                                               int cuts_ld, int32_t* n_cuts) {
    __shared__ long long best[2][SC_THREADS / WAVE];
    const int b = blockIdx.x;
    const long F = sc_frames(src, src_ld, content, b);
    if (off[b + 1] > total_frames) {
        if (threadIdx.x == 0) n_cuts[b] = F > 0 ? -1 : 0;       // (a file without frames has nothing that could not fit)
        return;
    }
    const int32_t* sb = s + off[b];
    int32_t* out = cuts + (long)b * cuts_ld;
    long c = 0;
    int n = 0;
    for (; F - c > hi; ++n) {
        long long key = SC_NO_KEY;
        for (long t = c + lo + threadIdx.x; t <= c + hi; t += SC_THREADS)
            key = sc_min(key, (long long)(((unsigned long long)(uint32_t)sb[t] << 32) | (uint32_t)(0x7fffffff - (int)t)));
#pragma unroll
        for (int d = WAVE / 2; d >= 1; d >>= 1) key = sc_min(key, __shfl_xor(key, d, WAVE));
        if ((threadIdx.x & (WAVE - 1)) == 0) best[n & 1][threadIdx.x / WAVE] = key;
        __syncthreads();                                        // (the next step writes the other half of `best`)
        key = best[n & 1][0];
#pragma unroll
        for (int w = 1; w < SC_THREADS / WAVE; ++w) key = sc_min(key, best[n & 1][w]);
        c = 0x7fffffff - (long)(uint32_t)(key & 0xffffffffLL);
        if (threadIdx.x == 0 && n < cuts_ld) out[n] = (int32_t)c;
    }
    if (threadIdx.x == 0) n_cuts[b] = n;
}

}  // namespace

size_t section_cuts_workspace_bytes(int batch, long long total_frames) { return sc_smoothed_bytes(batch, total_frames); }

int launch_section_cuts(const void* const* src, const int32_t* src_ld, const int32_t* content, int batch, int n_mels, int lo,
                        int hi, int h, int32_t* cuts, int cuts_ld, int32_t* n_cuts, void* workspace, long long total_frames,
                        hipStream_t stream) {
    const ScSmoothed w = sc_smoothed_at(workspace, batch, total_frames);
    static const char* const what[3] = {"section_cuts offsets", "section_cuts loudness", "section_cuts smoothing"};
    if (const int r = sc_launch_smoothed(src, src_ld, content, batch, n_mels, h, w, total_frames, stream, what)) return r;
    const long long* off = w.off;
    const int32_t* s = w.s;
    hipLaunchKernelGGL(sc_search_kernel, dim3((unsigned)batch), dim3(SC_THREADS), 0, stream, src, src_ld, content, lo, hi, off,
                       total_frames, s, cuts, cuts_ld, n_cuts);
    WM_LAUNCH_CHECK(stream, "section_cuts search");
    return 0;
}

}  // namespace wm

using namespace wm;

extern "C" size_t wm_section_cuts_workspace_bytes(int batch, int64_t total_frames) {
    if (batch < 1 || total_frames < 0) return 0;
    return section_cuts_workspace_bytes(batch, total_frames);
}

extern "C" int wm_section_cuts(const void* const* src, const int32_t* src_ld, const int32_t* content, int batch, int n_mels, int lo,
                               int hi, int h, int32_t* cuts, int cuts_ld, int32_t* n_cuts, void* workspace, size_t workspace_bytes,
                               int64_t total_frames, wm_stream_t stream) {
    WM_REQUIRE(src && src_ld && content && cuts && n_cuts && workspace, "wm_section_cuts: null argument");
    WM_REQUIRE(batch >= 1 && n_mels >= 1 && cuts_ld >= 0, "wm_section_cuts: batch=%d n_mels=%d must be >= 1, cuts_ld=%d >= 0", batch,
               n_mels, cuts_ld);
    WM_REQUIRE(lo >= 1 && lo <= hi, "wm_section_cuts: need 1 <= lo <= hi, got lo=%d hi=%d", lo, hi);
    WM_REQUIRE(h >= 0 && (int64_t)n_mels * (2 * (int64_t)h + 1) < 131072, "wm_section_cuts: n_mels * (2h + 1) = %d * (2 * %d + 1) must be "
               "below 131072 (32-bit sums)", n_mels, h);
    WM_REQUIRE(total_frames >= 0 && total_frames < ((int64_t)1 << 40), "wm_section_cuts: total_frames=%lld", (long long)total_frames);
    WM_REQUIRE((total_frames + SC_THREADS - 1) / SC_THREADS <= 0x7fffffffLL, "wm_section_cuts: total_frames=%lld needs too many workgroups",
               (long long)total_frames);
    WM_REQUIRE(workspace_bytes >= section_cuts_workspace_bytes(batch, total_frames),
               "wm_section_cuts: workspace of %zu bytes, wm_section_cuts_workspace_bytes(%d, %lld) = %zu", workspace_bytes, batch,
               (long long)total_frames, section_cuts_workspace_bytes(batch, total_frames));
    WM_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)cuts & 3) == 0 && ((uintptr_t)n_cuts & 3) == 0,
               "wm_section_cuts: workspace must be 8-byte aligned, cuts and n_cuts 4-byte aligned");
    return launch_section_cuts(src, src_ld, content, batch, n_mels, lo, hi, h, cuts, cuts_ld, n_cuts, workspace, total_frames,
                               (hipStream_t)stream);
}
