// wm_channel_top: which channel of a recording is loudest at every frame, and the gate that silences a channel where another
// one is much louder (channels.py states the contract).
//
// The batch is ragged twice: n_rec recordings, recording r made of the C_r = first[r + 1] - first[r] adjacent channels
// first[r] .. first[r + 1] - 1 (1 <= C_r <= 8), every channel a whole-file log-mel src[c] fp16 [n_mels][src_ld[c]] with content[c]
// frames of content; the channels of a recording share F and src_ld.  In integers, with q and s of loudness.h over ALL channels as
// one batch (the passes wm_section_cuts and wm_speech_spans run):
//   top[t]     = the lowest c with s_c[t] = max_c' s_c'[t]
//   gated_c[t] = max_{c' != c} s_c'[t] - s_c[t] >= G,   G = n_mels * (2h + 1) * step   (64-bit: the difference needs 33 bits)
//   v_c        = the smallest finite element of src[c][:, :F] by the monotone integer key of its fp16 bits (frontend.hip's order)
// and every bin of a gated frame becomes v_c, in place.
//
// Launches on the caller's stream, nothing allocated: loudness.h's three; with a gate one memset of the keys and the counts and
// the key pass -- one thread per frame of the concatenated channels, a loop over the mel bins, eight rows in flight, the wave's
// minimum through shuffles and ONE integer atomicMin per wave into device memory (a minimum is order-free, so any order of the
// atomics gives the same key; a wave that straddles two channels lets every lane speak for itself); then the status pass (one
// thread per recording) and the top pass: one thread per frame of the concatenated channels, of which the threads of a
// recording's FIRST channel work -- the C_r smoothed sums of a frame are C_r coalesced 4-byte reads, `top` a 1-byte write, the
// gated columns 2-byte writes that consecutive lanes put at consecutive frames of one row, the counts one integer atomicAdd per
// wave and channel.  Bandwidth bound like sc_loudness_kernel.
//
// Bounds: element m * ld + t of a channel with t < F <= ld, m < n_mels -- never outside the channel's array; top[r][t] with t < F;
// q, s below total_frames (a recording whose last channel ends beyond it takes no part and reports -1).
#include "loudness.h"
#include "../../include/whisper_mi355.h"

namespace wm {
namespace {

constexpr int CT_MAX_CHANNELS = 8;
constexpr int CT_NO_KEY = 0x7f7f7f7f;          // what the memset leaves: above every fp16 key

__device__ __forceinline__ int ct_key(h16 x) {               // monotone fp16 -> int map (frontend.hip's float_key on 16 bits)
    const int b = (int)__builtin_bit_cast(short, x);
    return b >= 0 ? b : b ^ 0x7fff;
}
__device__ __forceinline__ h16 ct_key_value(int k) { return __builtin_bit_cast(h16, (short)(k >= 0 ? k : k ^ 0x7fff)); }
__device__ __forceinline__ bool ct_finite(h16 x) { return ((int)__builtin_bit_cast(unsigned short, x) & 0x7c00) != 0x7c00; }

// The frames of recording r, or -1: not 1 .. 8 channels inside the batch, channels that differ in frames or stride, or a last
// channel that ends beyond the workspace.  c0: its first channel, C: their number.
__device__ long ct_recording(const void* const* src, const int32_t* src_ld, const int32_t* content, const int32_t* first, int r,
                             int n_channels, const long long* off, long long total_frames, int& c0, int& C) {
    c0 = first[r];
    C = first[r + 1] - c0;
    if (c0 < 0 || C < 1 || C > CT_MAX_CHANNELS || c0 + C > n_channels) return -1;
    const long F = sc_frames(src, src_ld, content, c0);
    for (int c = 1; c < C; ++c)
        if (sc_frames(src, src_ld, content, c0 + c) != F || (F > 0 && src_ld[c0 + c] != src_ld[c0])) return -1;
    if (F > 0 && off[c0 + C] > total_frames) return -1;
    return F;
}

__global__ __launch_bounds__(SC_THREADS) void ct_status_kernel(const void* const* src, const int32_t* src_ld, const int32_t* content,
                                                               const int32_t* first, int n_rec, int n_channels, const long long* off,
                                                               long long total_frames, int32_t* n_top) {
    const int r = blockIdx.x * SC_THREADS + threadIdx.x;
    if (r >= n_rec) return;
    int c0, C;
    n_top[r] = (int32_t)ct_recording(src, src_ld, content, first, r, n_channels, off, total_frames, c0, C);
}

// key[c] = min over the finite elements of channel c's content of ct_key
__global__ __launch_bounds__(SC_THREADS) void ct_key_kernel(const void* const* src, const int32_t* src_ld, int batch, int n_mels,
                                                            const long long* off, long long total_frames, int* key) {
    const long long g_first = (long long)blockIdx.x * SC_THREADS, g = g_first + threadIdx.x;
    const bool on = g < off[batch] && g < total_frames;
    int b = -1, low = CT_NO_KEY;
    if (on) {
        b = sc_file_of(off, batch, g_first, g);
        if (off[b + 1] > total_frames) {
            b = -1;
        } else {
            const long t = (long)(g - off[b]), ld = src_ld[b];
            const SC_GLOBAL h16* p = (const SC_GLOBAL h16*)src[b] + t;
            int m = 0;
            for (; m + 8 <= n_mels; m += 8) {
                h16 x[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) x[k] = p[(long)(m + k) * ld];
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (ct_finite(x[k])) low = min(low, ct_key(x[k]));
            }
            for (; m < n_mels; ++m) {
                const h16 x = p[(long)m * ld];
                if (ct_finite(x)) low = min(low, ct_key(x));
            }
        }
    }
    // (every lane of the wave arrives here: the shuffles below are executed by all 64)
    const int b0 = __shfl(b, 0, WAVE);
    if (__all(b == b0)) {
        for (int d = WAVE / 2; d >= 1; d >>= 1) low = min(low, __shfl_xor(low, d, WAVE));
        if ((threadIdx.x & (WAVE - 1)) == 0 && b0 >= 0 && low != CT_NO_KEY) atomicMin(key + b0, low);
    } else if (b >= 0 && low != CT_NO_KEY) {
        atomicMin(key + b, low);
    }
}

__global__ __launch_bounds__(SC_THREADS) void ct_top_kernel(void* const* src, const int32_t* src_ld, const int32_t* content,
                                                            const int32_t* first, int n_rec, int batch, int n_mels, long long G,
                                                            int gate, const long long* off, long long total_frames, const int32_t* s,
                                                            const int* key, uint8_t* const* top, int32_t* counts) {
    const long long g_first = (long long)blockIdx.x * SC_THREADS, g = g_first + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1);
    int c0 = -1, C = 0;
    long t = 0;
    unsigned gated = 0;                         // bit c: channel c0 + c is gated at this thread's frame
    if (g < off[batch] && g < total_frames) {
        const int b = sc_file_of(off, batch, g_first, g);
        int lo = 0, hi = n_rec - 1;             // the last recording r with first[r] <= b
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (first[mid] <= b) lo = mid; else hi = mid - 1;
        }
        int rc0, rC;
        if (first[lo] == b && ct_recording((const void* const*)src, src_ld, content, first, lo, batch, off, total_frames, rc0, rC) > 0) {
            c0 = rc0, C = rC;
            t = (long)(g - off[b]);
            long long v[CT_MAX_CHANNELS];
            long long best = 0;
            int arg = 0;
            for (int c = 0; c < C; ++c) {
                v[c] = s[off[c0 + c] + t];
                if (c == 0 || v[c] > best) best = v[c], arg = c;
            }
            if (top[lo]) top[lo][t] = (uint8_t)arg;
            if (gate && C > 1) {
                for (int c = 0; c < C; ++c) {
                    long long others = 0;
                    bool any = false;
                    for (int o = 0; o < C; ++o)
                        if (o != c && (!any || v[o] > others)) others = v[o], any = true;
                    if (others - v[c] >= G && key[c0 + c] != CT_NO_KEY) gated |= 1u << c;
                }
            }
        }
    }
    if (!gate) return;                          // (the same for the whole grid)
    // the counts: one atomic per wave and channel where the wave stands inside one recording, a lane's own otherwise
    const unsigned long long at_work = __ballot(c0 >= 0);
    if (!at_work) return;                       // (the same for the whole wave)
    const int lead = __shfl(c0, __ffsll((long long)at_work) - 1, WAVE);
    const bool together = __all(c0 == lead || c0 < 0);
    for (int c = 0; c < CT_MAX_CHANNELS; ++c) {
        const bool mine = c0 >= 0 && (gated >> c & 1u);
        if (together) {
            const unsigned long long m = __ballot(mine);
            if (m && lane == __ffsll((long long)m) - 1) atomicAdd(counts + c0 + c, (int32_t)__popcll(m));
        } else if (mine) {
            atomicAdd(counts + c0 + c, 1);
        }
    }
    if (!gated) return;
    const long ld = src_ld[c0];
    for (int c = 0; c < C; ++c) {
        if (!(gated >> c & 1u)) continue;
        const h16 v = ct_key_value(key[c0 + c]);
        SC_GLOBAL h16* p = (SC_GLOBAL h16*)src[c0 + c] + t;
        for (int m = 0; m < n_mels; ++m) p[(long)m * ld] = v;
    }
}

// behind loudness.h's part of the workspace: the keys of the channels
size_t ct_workspace_bytes(int batch, long long total_frames) {
    return sc_smoothed_bytes(batch, total_frames) + sc_align((size_t)batch * sizeof(int));
}

int launch_channel_top(void* const* src, const int32_t* src_ld, const int32_t* content, const int32_t* first, int n_rec, int batch,
                       int n_mels, int h, int step, uint8_t* const* top, int32_t* n_top, int32_t* counts, void* workspace,
                       long long total_frames, hipStream_t stream) {
    const ScSmoothed w = sc_smoothed_at(workspace, batch, total_frames);
    static const char* const what[3] = {"channel_top offsets", "channel_top loudness", "channel_top smoothing"};
    if (const int r = sc_launch_smoothed((const void* const*)src, src_ld, content, batch, n_mels, h, w, total_frames, stream, what))
        return r;
    int* key = (int*)((char*)workspace + sc_smoothed_bytes(batch, total_frames));
    const long long grid = (total_frames + SC_THREADS - 1) / SC_THREADS;
    WM_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)batch * sizeof(int32_t), stream));
    if (step > 0) {
        WM_CHECK_HIP(hipMemsetAsync(key, 0x7f, (size_t)batch * sizeof(int), stream));
        if (grid > 0) {
            hipLaunchKernelGGL(ct_key_kernel, dim3((unsigned)grid), dim3(SC_THREADS), 0, stream, (const void* const*)src, src_ld, batch,
                               n_mels, (const long long*)w.off, total_frames, key);
            WM_LAUNCH_CHECK(stream, "channel_top keys");
        }
    }
    hipLaunchKernelGGL(ct_status_kernel, dim3((unsigned)((n_rec + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, stream,
                       (const void* const*)src, src_ld, content, first, n_rec, batch, (const long long*)w.off, total_frames, n_top);
    WM_LAUNCH_CHECK(stream, "channel_top status");
    if (grid > 0) {
        const long long G = (long long)n_mels * (2 * (long long)h + 1) * step;
        hipLaunchKernelGGL(ct_top_kernel, dim3((unsigned)grid), dim3(SC_THREADS), 0, stream, src, src_ld, content, first, n_rec, batch,
                           n_mels, G, step > 0 ? 1 : 0, (const long long*)w.off, total_frames, (const int32_t*)w.s, (const int*)key, top,
                           counts);
        WM_LAUNCH_CHECK(stream, "channel_top top");
    }
    return 0;
}

}  // namespace
}  // namespace wm

using namespace wm;

extern "C" size_t wm_channel_top_workspace_bytes(int n_channels, int64_t total_frames) {
    if (n_channels < 1 || total_frames < 0) return 0;
    return ct_workspace_bytes(n_channels, total_frames);
}

extern "C" int wm_channel_top(void* const* src, const int32_t* src_ld, const int32_t* content, const int32_t* first, int n_recordings,
                              int n_channels, int n_mels, int h, int step, uint8_t* const* top, int32_t* n_top, int32_t* counts,
                              void* workspace, size_t workspace_bytes, int64_t total_frames, wm_stream_t stream) {
    WM_REQUIRE(src && src_ld && content && first && top && n_top && counts && workspace, "wm_channel_top: null argument");
    WM_REQUIRE(n_recordings >= 1 && n_channels >= n_recordings && n_mels >= 1,
               "wm_channel_top: n_recordings=%d and n_mels=%d must be >= 1, n_channels=%d >= n_recordings", n_recordings, n_mels,
               n_channels);
    WM_REQUIRE(step >= 0 && step <= 32768, "wm_channel_top: need 0 <= step <= 32768 (0: no gate), got step=%d", step);
    WM_REQUIRE(h >= 0 && (int64_t)n_mels * (2 * (int64_t)h + 1) < 131072, "wm_channel_top: n_mels * (2h + 1) = %d * (2 * %d + 1) must be "
               "below 131072 (32-bit sums)", n_mels, h);
    WM_REQUIRE(total_frames >= 0 && total_frames < ((int64_t)1 << 40), "wm_channel_top: total_frames=%lld", (long long)total_frames);
    WM_REQUIRE((total_frames + SC_THREADS - 1) / SC_THREADS <= 0x7fffffffLL, "wm_channel_top: total_frames=%lld needs too many workgroups",
               (long long)total_frames);
    WM_REQUIRE(workspace_bytes >= ct_workspace_bytes(n_channels, total_frames),
               "wm_channel_top: workspace of %zu bytes, wm_channel_top_workspace_bytes(%d, %lld) = %zu", workspace_bytes, n_channels,
               (long long)total_frames, ct_workspace_bytes(n_channels, total_frames));
    WM_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)n_top & 3) == 0 && ((uintptr_t)counts & 3) == 0 &&
               ((uintptr_t)first & 3) == 0, "wm_channel_top: workspace must be 8-byte aligned, first, n_top and counts 4-byte aligned");
    return launch_channel_top(src, src_ld, content, first, n_recordings, n_channels, n_mels, h, step, top, n_top, counts, workspace,
                              (long long)total_frames, (hipStream_t)stream);
}
