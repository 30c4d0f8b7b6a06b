// wm_mel_windows: the windows of a round of long-form transcription (transcribe.py).
//
// Every row b of the batch is a file with a log-mel of its own length, src[b] fp16 [n_mels][src_frames[b]], and a position
// seek[b] in it; the encoder wants fp16 [batch][n_mels][n_window].  One launch cuts all of them:
//   out[b][m][j] = seek[b] + j < src_frames[b] ? src[b][m * src_frames[b] + seek[b] + j] : 0,   a null src[b]: a zero row.
// Pointers, lengths and positions are read on the device: no host synchronisation, and a captured launch follows the arrays.
//
// A copy, so the only question is the width of the accesses.  One wave owns one output row (b, m) and writes it in full: a scalar
// head up to the first 16-byte boundary of the OUTPUT, then 16-byte stores, then a scalar tail.  The source of such a 16-byte piece
// starts at an arbitrary 2-byte offset (seek and src_frames may be odd), the same one modulo 16 for the whole row:
//   16-byte aligned       one 16-byte load;
//   4-byte aligned        four dwords (one multi-dword load: those need dword alignment only);
//   2 bytes off a dword   the five ALIGNED dwords that cover the piece, joined by v_alignbyte -- taken only where all five lie
//                         inside the file's array (the first piece of the first row and the last of the last would look 2 bytes
//                         beyond it);
// and every piece that crosses the end of the file, or that the rule above excludes, is gathered element by element.
#include "kernels.h"
#include "../../include/whisper_mi355.h"

namespace wm {
namespace {

constexpr int MW_WAVES = 4;        // rows (waves) per workgroup

// The files' pointers come out of a table in memory, so the compiler cannot know their address space and would read through
// them with flat loads; they are device allocations: say so once, and every load below is a global one.
#define MW_GLOBAL __attribute__((address_space(1)))
typedef const MW_GLOBAL h16* mw_src;

__device__ __forceinline__ u32x4 mw_gather(mw_src s, long j, long n_valid) {
    // elements j .. j + 7 of the row one by one, zero from n_valid on
    const MW_GLOBAL uint16_t* u = (const MW_GLOBAL uint16_t*)s;
    u32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t lo = j + 2 * k < n_valid ? u[j + 2 * k] : 0u;
        const uint32_t hi = j + 2 * k + 1 < n_valid ? u[j + 2 * k + 1] : 0u;
        r[k] = lo | (hi << 16);
    }
    return r;
}

typedef u32x4 mw_dwords4 __attribute__((aligned(4)));        // four dwords at a dword-aligned address

__global__ __launch_bounds__(64 * MW_WAVES) void mel_windows_kernel(const h16* const* src, const int32_t* src_frames,
                                                                    const int32_t* seek, int n_rows, int n_mels, int n_window,
                                                                    h16* out) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * MW_WAVES + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const int b = (int)(row / n_mels), m = (int)(row % n_mels);
    const h16* base = src[b];
    const long F = src_frames[b], sk = seek[b];
    // elements of this row that come from the file: [0, n_valid); everything behind them is zero
    long n_valid = 0;
    if (base && F > 0 && sk >= 0 && sk < F) n_valid = F - sk < n_window ? F - sk : n_window;
    const long g0 = n_valid ? (long)m * F + sk : 0;            // index of the row's first element in the file's array
    const long total = (long)n_mels * F;
    const mw_src s = n_valid ? (mw_src)(base + g0) : (mw_src) nullptr;
    h16* dst = out + row * (long)n_window;

    // head: up to the output's first 16-byte boundary
    long head = (long)((16 - ((uintptr_t)dst & 15)) & 15) / 2;
    if (head > n_window) head = n_window;
    if (lane < head) dst[lane] = lane < n_valid ? s[lane] : (h16)0.f;
    const long n_chunks = (n_window - head) / 8;
    const uintptr_t sa = (uintptr_t)(s + head);                // address of the first piece's source: its low bits hold for the whole row
    const int cls = !n_valid ? 3 : (sa & 15) == 0 ? 0 : (sa & 3) == 0 ? 1 : 2;
    for (long c = lane; c < n_chunks; c += 64) {
        const long j = head + c * 8;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (j + 8 <= n_valid) {
            if (cls == 0) {
                v = *(const MW_GLOBAL u32x4*)(s + j);
            } else if (cls == 1) {
                v = *(const MW_GLOBAL mw_dwords4*)(s + j);
            } else if (g0 + j >= 1 && g0 + j + 9 <= total) {
                const MW_GLOBAL uint32_t* a = (const MW_GLOBAL uint32_t*)(s + j - 1);      // dword aligned: s + j sits 2 bytes behind it
                const u32x4 t = *(const MW_GLOBAL mw_dwords4*)a;
                const uint32_t t4 = a[4];
                v[0] = __builtin_amdgcn_alignbyte(t[1], t[0], 2);
                v[1] = __builtin_amdgcn_alignbyte(t[2], t[1], 2);
                v[2] = __builtin_amdgcn_alignbyte(t[3], t[2], 2);
                v[3] = __builtin_amdgcn_alignbyte(t4, t[3], 2);
            } else {
                v = mw_gather(s, j, n_valid);
            }
        } else if (j < n_valid) {
            v = mw_gather(s, j, n_valid);
        }
        *(u32x4*)(dst + j) = v;
    }
    // tail: what is left behind the last 16-byte piece (fewer than 8 elements)
    const long t = head + n_chunks * 8 + lane;
    if (t < n_window) dst[t] = t < n_valid ? s[t] : (h16)0.f;
}

}  // namespace

int launch_mel_windows(const h16* const* src, const int32_t* src_frames, const int32_t* seek, int batch, int n_mels,
                       int n_window, h16* out, hipStream_t stream) {
    const long n_rows = (long)batch * n_mels;
    const long grid = (n_rows + MW_WAVES - 1) / MW_WAVES;
    hipLaunchKernelGGL(mel_windows_kernel, dim3((unsigned)grid), dim3(64 * MW_WAVES), 0, stream, src, src_frames, seek,
                       (int)n_rows, n_mels, n_window, out);
    WM_LAUNCH_CHECK(stream, "mel_windows");
    return 0;
}

}  // namespace wm

using namespace wm;

extern "C" int wm_mel_windows(const void* const* src, const int32_t* src_frames, const int32_t* seek, int batch, int n_mels,
                              int n_window, void* out, wm_stream_t stream) {
    WM_REQUIRE(src && src_frames && seek && out, "wm_mel_windows: null argument");
    WM_REQUIRE(batch >= 1 && n_mels >= 1 && n_window >= 1, "wm_mel_windows: batch=%d n_mels=%d n_window=%d must be >= 1", batch,
               n_mels, n_window);
    WM_REQUIRE((long)batch * n_mels <= 0x7fffffffL, "wm_mel_windows: batch * n_mels = %ld rows exceed 2^31 - 1", (long)batch * n_mels);
    WM_REQUIRE(((uintptr_t)out & 1) == 0, "wm_mel_windows: out is not 2-byte aligned");
    return launch_mel_windows((const h16* const*)src, src_frames, seek, batch, n_mels, n_window, (h16*)out, (hipStream_t)stream);
}
