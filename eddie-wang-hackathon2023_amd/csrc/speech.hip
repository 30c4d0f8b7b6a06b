// wm_speech_spans, wm_mel_gather: find the speech of long files and pack it, so that the decoder never sees the quiet stretches
// (speech.py states the contract).
//
// wm_speech_spans.  Every file b of the batch is a whole-file log-mel src[b] fp16 [n_mels][src_ld[b]] with F = content[b] frames of
// content.  In integers, with q and s of loudness.h (the passes wm_section_cuts runs):
//   floor = sorted(s)[min(F - 1, F * permille / 1000)]
//   v[t]  = (int64)s[t] - floor >= M,   M = n_mels * (2h + 1) * step     (< 2^32; the difference needs 33 bits)
//   spans = (a) the maximal runs of v, (b) joined across gaps < min_silence, (c) those shorter than min_speech dropped,
//           (d) each widened by pad inside [0, F] and joined where they now touch or overlap.
// Four launches on the caller's stream: loudness.h's three, then ONE workgroup of 1024 threads per file for the rest:
//   floor   an exact selection: four passes of an 8-bit radix select over key = s ^ 2^31 (unsigned order = signed order); each
//           pass counts the keys that share the digits fixed so far in a 256-bin LDS histogram (integer atomics: any order gives
//           the same counts), thread 0 walks the bins to the one that holds the rank.  s is clustered -- in the first passes
//           nearly every key falls into one or two bins -- so a wave first takes out its two most forward bins with one atomic
//           each (a ballot and a population count) and only the lanes left add one by one;
//   (a)-(d) each a per-element decision and an ordered compaction, 4096 elements a round: a ballot per wave, the waves' counts
//           through LDS, two barriers a round.  (a) walks the F + 1 positions and keeps those where v changes (v[-1] = v[F] = 0):
//           the edges, alternately a start and an end.  (b) and (d) decide per span "a span begins here" (no join with the one
//           before) and "a span ends here" and compact the starts and the ends apiece -- the j-th start and the j-th end are one
//           span; (c) decides "kept".  The lists move between two arrays of the workspace of F + 1 entries each (at most F + 1
//           edges); (d) writes the caller's table, entries below spans_ld only, and more than spans_ld spans report -1.
//
// wm_mel_gather.  out[b] = the spans' columns of src[b] in order, then n_pad copies of its last column (speech.py, rule 5).  A
// copy at 2 bytes an element; consecutive lanes take consecutive PACKED frames of one mel row, so reads are contiguous inside a
// span and writes throughout.  A workgroup owns a window of 2048 packed frames and 16 mel rows of one file (and the windows a
// fixed stride further): it scans the file's span table once -- 256 entries a round: a prefix maximum of the ends decides which
// spans are taken (speech.taken_spans: in [0, src_ld] and not before an earlier one's end; anything else is skipped and never
// dereferenced), a prefix sum of the taken lengths gives the packed starts -- and keeps the spans that meet its window in LDS;
// every thread then finds its first frame's span by a binary search over those packed starts and walks on from it, and copies
// its frames row by row, eight rows in flight.  2-byte accesses only: src_ld, dst_ld, the span starts and both bases may be odd,
// so no wider alignment is proven for any row.  Element m * src_ld + t of the source with t < b_k <= src_ld and element
// m * dst_ld + p of the destination with p < dst_ld, m < n_mels: never outside either array.
#include "loudness.h"
#include "../../include/whisper_mi355.h"

namespace wm {
namespace {

// ------------------------------------------------------------------------------------------------------------ wm_speech_spans
constexpr int SP_THREADS = 1024;
constexpr int SP_WAVES = SP_THREADS / WAVE;
constexpr int SP_ITEMS = 4;                     // elements per thread and round
constexpr long SP_ROUND = (long)SP_THREADS * SP_ITEMS;

struct SpShared {
    uint32_t hist[256];
    uint32_t wave_count[SP_ITEMS][SP_WAVES];
    uint32_t bin;
    long long rank;
};

// the element of index rank (0-based, ascending) of sb[0 .. F)
__device__ int32_t sp_select(const int32_t* sb, long F, long long rank, SpShared& sh) {
    const int lane = threadIdx.x & (WAVE - 1);
    uint32_t prefix = 0, mask = 0;
    const long rounds = (F + SP_ROUND - 1) / SP_ROUND;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < 256; i += SP_THREADS) sh.hist[i] = 0;
        __syncthreads();
        for (long r = 0; r < rounds; ++r) {
            uint32_t key[SP_ITEMS];
#pragma unroll
            for (int j = 0; j < SP_ITEMS; ++j) {
                const long t = r * SP_ROUND + (long)j * SP_THREADS + threadIdx.x;
                key[j] = t < F ? (uint32_t)sb[t] ^ 0x80000000u : 0u;
            }
#pragma unroll
            for (int j = 0; j < SP_ITEMS; ++j) {
                const long t = r * SP_ROUND + (long)j * SP_THREADS + threadIdx.x;
                bool on = t < F && (key[j] & mask) == prefix;
                const uint32_t bin = (key[j] >> shift) & 255u;
                for (int peel = 0; peel < 2; ++peel) {
                    const unsigned long long todo = __ballot(on);
                    if (!todo) break;                                   // (the same for the whole wave)
                    const int leader = __ffsll((long long)todo) - 1;
                    const uint32_t lb = (uint32_t)__shfl((int)bin, leader, WAVE);
                    const unsigned long long same = __ballot(on && bin == lb);
                    if (lane == leader) atomicAdd(&sh.hist[lb], (uint32_t)__popcll(same));
                    if (bin == lb) on = false;
                }
                if (on) atomicAdd(&sh.hist[bin], 1u);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            long long before = 0;
            uint32_t b = 0;
            for (; b < 255; ++b) {
                if (before + sh.hist[b] > rank) break;
                before += sh.hist[b];
            }
            sh.bin = b;
            sh.rank = rank - before;
        }
        __syncthreads();
        prefix |= sh.bin << shift;
        mask |= 255u << shift;
        rank = sh.rank;
    }
    return (int32_t)(prefix ^ 0x80000000u);
}

// The ranks of the set flags of a round in index order -- element j * SP_THREADS + thread of the round is flag[j] -- and their
// number.  Two barriers: the second frees wave_count for the next call.
__device__ uint32_t sp_ranks(const bool (&flag)[SP_ITEMS], uint32_t (&rank)[SP_ITEMS], SpShared& sh) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    uint32_t below[SP_ITEMS];
#pragma unroll
    for (int j = 0; j < SP_ITEMS; ++j) {
        const unsigned long long m = __ballot(flag[j]);
        below[j] = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) sh.wave_count[j][wave] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    uint32_t run = 0;
#pragma unroll
    for (int j = 0; j < SP_ITEMS; ++j) {
        uint32_t before = 0, all = 0;
        for (int w = 0; w < SP_WAVES; ++w) {
            const uint32_t c = sh.wave_count[j][w];
            before += w < wave ? c : 0u;
            all += c;
        }
        rank[j] = run + before + below[j];
        run += all;
    }
    __syncthreads();
    return run;
}

__global__ __launch_bounds__(SP_THREADS) void sp_spans_kernel(const void* const* src, const int32_t* src_ld, const int32_t* content,
                                                              int permille, long long M, int min_silence, int min_speech, int pad,
                                                              const long long* off, long long total_frames, const int32_t* s,
                                                              int32_t* e0, int32_t* e1, int32_t* spans, int spans_ld,
                                                              int32_t* n_spans) {
    __shared__ SpShared sh;
    const int b = blockIdx.x;
    const long F = sc_frames(src, src_ld, content, b);
    if (off[b + 1] > total_frames || F == 0) {
        if (threadIdx.x == 0) n_spans[b] = F > 0 ? -1 : 0;      // (a file without frames has nothing that could not fit)
        return;
    }
    const int32_t* sb = s + off[b];
    int32_t* A = e0 + off[b] + b;                               // F + 1 entries each
    int32_t* B = e1 + off[b] + b;
    const long long at = (long long)F * permille / 1000;
    const long long floor = sp_select(sb, F, at < F - 1 ? at : F - 1, sh);

    bool flag[SP_ITEMS], flag2[SP_ITEMS];
    uint32_t rank[SP_ITEMS], rank2[SP_ITEMS];
    int32_t lo[SP_ITEMS], hi[SP_ITEMS];

    // (a) the edges of v over the positions 0 .. F -> A
    uint32_t n_edges = 0;
    for (long r0 = 0; r0 <= F; r0 += SP_ROUND) {
#pragma unroll
        for (int j = 0; j < SP_ITEMS; ++j) {
            const long t = r0 + (long)j * SP_THREADS + threadIdx.x;
            const bool here = t < F && (long long)sb[t] - floor >= M;
            const bool prev = t >= 1 && t <= F && (long long)sb[t - 1] - floor >= M;
            flag[j] = t <= F && here != prev;
        }
        const uint32_t found = sp_ranks(flag, rank, sh);
#pragma unroll
        for (int j = 0; j < SP_ITEMS; ++j)
            if (flag[j]) A[n_edges + rank[j]] = (int32_t)(r0 + (long)j * SP_THREADS + threadIdx.x);
        n_edges += found;
    }
    __syncthreads();

    // (b) runs A -> spans B: run k begins a span unless its gap to run k - 1 is < min_silence, and ends one likewise
    const long n_runs = n_edges / 2;
    uint32_t n_joined = 0, n_ends = 0;
    for (long r0 = 0; r0 < n_runs; r0 += SP_ROUND) {
#pragma unroll
        for (int j = 0; j < SP_ITEMS; ++j) {
            const long k = r0 + (long)j * SP_THREADS + threadIdx.x;
            flag[j] = flag2[j] = false;
            if (k < n_runs) {
                lo[j] = A[2 * k];
                hi[j] = A[2 * k + 1];
                flag[j] = k == 0 || lo[j] - A[2 * k - 1] >= min_silence;
                flag2[j] = k == n_runs - 1 || A[2 * k + 2] - hi[j] >= min_silence;
            }
        }
        const uint32_t found = sp_ranks(flag, rank, sh);
        const uint32_t found2 = sp_ranks(flag2, rank2, sh);
#pragma unroll
        for (int j = 0; j < SP_ITEMS; ++j) {
            if (flag[j]) B[2 * (long)(n_joined + rank[j])] = lo[j];
            if (flag2[j]) B[2 * (long)(n_ends + rank2[j]) + 1] = hi[j];
        }
        n_joined += found;                                      // (a span may begin in one round and end in a later one)
        n_ends += found2;
    }
    __syncthreads();

    // (c) spans B -> A: those of at least min_speech frames
    uint32_t n_kept = 0;
    for (long r0 = 0; r0 < (long)n_joined; r0 += SP_ROUND) {
#pragma unroll
        for (int j = 0; j < SP_ITEMS; ++j) {
            const long k = r0 + (long)j * SP_THREADS + threadIdx.x;
            flag[j] = false;
            if (k < (long)n_joined) {
                lo[j] = B[2 * k];
                hi[j] = B[2 * k + 1];
                flag[j] = hi[j] - lo[j] >= min_speech;
            }
        }
        const uint32_t found = sp_ranks(flag, rank, sh);
#pragma unroll
        for (int j = 0; j < SP_ITEMS; ++j) {
            if (flag[j]) {
                A[2 * (long)(n_kept + rank[j])] = lo[j];
                A[2 * (long)(n_kept + rank[j]) + 1] = hi[j];
            }
        }
        n_kept += found;
    }
    __syncthreads();

    // (d) spans A, widened by pad inside [0, F] -> the caller's table: joined where they touch or overlap
    int32_t* out = spans + (long)b * spans_ld * 2;
    uint32_t n_out = 0;
    n_ends = 0;
    for (long r0 = 0; r0 < (long)n_kept; r0 += SP_ROUND) {
#pragma unroll
        for (int j = 0; j < SP_ITEMS; ++j) {
            const long k = r0 + (long)j * SP_THREADS + threadIdx.x;
            flag[j] = flag2[j] = false;
            if (k < (long)n_kept) {
                const long long a = (long long)A[2 * k] - pad, e = (long long)A[2 * k + 1] + pad;
                lo[j] = (int32_t)(a > 0 ? a : 0);
                hi[j] = (int32_t)(e < F ? e : F);
                flag[j] = k == 0 || (long long)lo[j] > (long long)A[2 * k - 1] + pad;          // (an end beyond F is F: still below)
                flag2[j] = k == (long)n_kept - 1 || (long long)A[2 * k + 2] - pad > (long long)hi[j];
            }
        }
        const uint32_t found = sp_ranks(flag, rank, sh);
        const uint32_t found2 = sp_ranks(flag2, rank2, sh);
#pragma unroll
        for (int j = 0; j < SP_ITEMS; ++j) {
            if (flag[j] && n_out + rank[j] < (uint32_t)spans_ld) out[2 * (long)(n_out + rank[j])] = lo[j];
            if (flag2[j] && n_ends + rank2[j] < (uint32_t)spans_ld) out[2 * (long)(n_ends + rank2[j]) + 1] = hi[j];
        }
        n_out += found;
        n_ends += found2;
    }
    if (threadIdx.x == 0) n_spans[b] = n_out <= (uint32_t)spans_ld ? (int32_t)n_out : -1;
}

size_t sp_edges_bytes(int batch, long long total_frames) { return sc_align((size_t)(total_frames + batch) * sizeof(int32_t)); }

// --------------------------------------------------------------------------------------------------------------- wm_mel_gather
constexpr int MG_THREADS = 256;
constexpr int MG_WAVES = MG_THREADS / WAVE;
constexpr int MG_FRAMES = 2048;                 // packed frames of a window
constexpr int MG_ROWS = 16;                     // mel rows of a workgroup
constexpr int MG_TARGET_WGS = 2048;             // the grid: about this many workgroups, each walks its windows at a fixed stride

struct MgMax { __device__ int operator()(int a, int b) const { return a > b ? a : b; } };
struct MgSum { __device__ long long operator()(long long a, long long b) const { return a + b; } };

// exclusive scan over the workgroup's threads (and the total); two barriers, the second frees `wave_total` for the next call
template <typename T, typename Op>
__device__ T mg_scan(T v, Op op, T* wave_total, T& total) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const T o = __shfl_up(v, d, WAVE);
        if (lane >= d) v = op(o, v);
    }
    if (lane == WAVE - 1) wave_total[wave] = v;
    T ex = __shfl_up(v, 1, WAVE);
    if (lane == 0) ex = T(0);
    __syncthreads();
    T before = T(0);
    total = T(0);
    for (int w = 0; w < MG_WAVES; ++w) {
        const T c = wave_total[w];
        if (w < wave) before = op(before, c);
        total = op(total, c);
    }
    __syncthreads();
    return op(before, ex);
}

__global__ __launch_bounds__(MG_THREADS) void mel_gather_kernel(const void* const* src, const int32_t* src_ld, const int32_t* spans,
                                                                const int32_t* n_spans, int spans_ld, int n_mels, int n_pad,
                                                                void* const* dst, const int32_t* dst_ld) {
    __shared__ int32_t list_p[MG_FRAMES], list_a[MG_FRAMES];   // the spans that meet the window: packed start, first frame
    __shared__ long long sum_total[MG_WAVES];
    __shared__ int max_total[MG_WAVES];
    __shared__ int first_rank, list_n;
    const int b = blockIdx.y;
    const int m0 = blockIdx.z * MG_ROWS, m1 = min(n_mels, m0 + MG_ROWS);
    const SC_GLOBAL h16* s = (const SC_GLOBAL h16*)src[b];
    SC_GLOBAL h16* d = (SC_GLOBAL h16*)dst[b];
    const long ld = src_ld[b], dl = dst_ld[b];
    if (!s || !d || ld < 1 || dl < 1) return;
    int n = n_spans[b];
    n = n < 0 ? 0 : n > spans_ld ? spans_ld : n;
    const int32_t* tab = spans + (long)b * spans_ld * 2;

    for (long p0 = (long)blockIdx.x * MG_FRAMES; p0 < dl; p0 += (long)gridDim.x * MG_FRAMES) {
        // the table, 256 spans a round, until the packed frames pass the window's end
        if (threadIdx.x == 0) first_rank = 0, list_n = 0;
        __syncthreads();
        long long P = 0;                        // packed frames of the spans scanned
        int high = 0, taken = 0, c0 = 0;        // the largest end among the spans in range, the number of spans taken
        for (; c0 < n && P < p0 + MG_FRAMES; c0 += MG_THREADS) {
            const int k = c0 + threadIdx.x;
            int a = 0, e = 0;
            if (k < n) a = tab[2 * (long)k], e = tab[2 * (long)k + 1];
            const bool in_range = k < n && 0 <= a && a < e && e <= ld;
            int round_high;
            const int ends_before = mg_scan<int>(in_range ? e : 0, MgMax(), max_total, round_high);
            const bool take = in_range && a >= (high > ends_before ? high : ends_before);
            const long long len = take ? e - a : 0;
            long long round_sum;
            const long long ex = mg_scan<long long>((len << 20) | (take ? 1 : 0), MgSum(), sum_total, round_sum);
            const long long pk = P + (ex >> 20);
            const int rk = taken + (int)(ex & 0xfffff);
            if (take && pk <= p0 && p0 < pk + len) first_rank = rk;
            __syncthreads();
            if (take && pk < p0 + MG_FRAMES && pk + len > p0) {
                const int i = rk - first_rank;
                if (i >= 0 && i < MG_FRAMES) {
                    list_p[i] = (int32_t)pk;
                    list_a[i] = a;
                    atomicMax(&list_n, i + 1);
                }
            }
            P += round_sum >> 20;
            taken += (int)(round_sum & 0xfffff);
            high = high > round_high ? high : round_high;
        }
        __syncthreads();
        const bool whole_table = c0 >= n;       // P is the file's packed length: the pad columns stand at P .. P + n_pad
        const int nl = list_n;
        int k = -1;
        for (int j = 0; j < MG_FRAMES / MG_THREADS; ++j) {
            const long p = p0 + (long)j * MG_THREADS + threadIdx.x;
            if (p >= dl) break;
            long t;
            if (p < P) {
                if (nl < 1) break;
                if (k < 0) {
                    int lo = 0, hi = nl - 1;
                    while (lo < hi) {
                        const int mid = (lo + hi + 1) >> 1;
                        if (list_p[mid] <= p) lo = mid; else hi = mid - 1;
                    }
                    k = lo;
                }
                while (k + 1 < nl && list_p[k + 1] <= p) ++k;
                t = (long)list_a[k] + (p - list_p[k]);
                if (t < 0 || t >= ld) continue;                         // (cannot be: the frame lies inside a span taken)
            } else if (whole_table && p < P + n_pad) {
                t = ld - 1;
            } else {
                break;
            }
            const SC_GLOBAL h16* from = s + t;
            SC_GLOBAL h16* to = d + p;
            int m = m0;
            for (; m + 8 <= m1; m += 8) {
                h16 x[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) x[i] = from[(long)(m + i) * ld];
#pragma unroll
                for (int i = 0; i < 8; ++i) to[(long)(m + i) * dl] = x[i];
            }
            for (; m < m1; ++m) to[(long)m * dl] = from[(long)m * ld];
        }
        __syncthreads();                        // (the next window rewrites the list)
    }
}

}  // namespace

size_t speech_spans_workspace_bytes(int batch, long long total_frames) {
    return sc_smoothed_bytes(batch, total_frames) + 2 * sp_edges_bytes(batch, total_frames);
}

int launch_speech_spans(const void* const* src, const int32_t* src_ld, const int32_t* content, int batch, int n_mels, int h, int step,
                        int permille, int min_silence, int min_speech, int pad, int32_t* spans, int spans_ld, int32_t* n_spans,
                        void* workspace, long long total_frames, hipStream_t stream) {
    const ScSmoothed w = sc_smoothed_at(workspace, batch, total_frames);
    static const char* const what[3] = {"speech_spans offsets", "speech_spans loudness", "speech_spans smoothing"};
    if (const int r = sc_launch_smoothed(src, src_ld, content, batch, n_mels, h, w, total_frames, stream, what)) return r;
    int32_t* e0 = (int32_t*)((char*)workspace + sc_smoothed_bytes(batch, total_frames));
    int32_t* e1 = (int32_t*)((char*)e0 + sp_edges_bytes(batch, total_frames));
    const long long M = (long long)n_mels * (2 * (long long)h + 1) * step;
    hipLaunchKernelGGL(sp_spans_kernel, dim3((unsigned)batch), dim3(SP_THREADS), 0, stream, src, src_ld, content, permille, M,
                       min_silence, min_speech, pad, (const long long*)w.off, total_frames, (const int32_t*)w.s, e0, e1, spans,
                       spans_ld, n_spans);
    WM_LAUNCH_CHECK(stream, "speech_spans spans");
    return 0;
}

int launch_mel_gather(const void* const* src, const int32_t* src_ld, const int32_t* spans, const int32_t* n_spans, int spans_ld,
                      int batch, int n_mels, int n_pad, void* const* dst, const int32_t* dst_ld, hipStream_t stream) {
    const int groups = (n_mels + MG_ROWS - 1) / MG_ROWS;
    int windows = MG_TARGET_WGS / (batch * groups);
    windows = windows < 1 ? 1 : windows > 64 ? 64 : windows;
    hipLaunchKernelGGL(mel_gather_kernel, dim3((unsigned)windows, (unsigned)batch, (unsigned)groups), dim3(MG_THREADS), 0, stream, src,
                       src_ld, spans, n_spans, spans_ld, n_mels, n_pad, dst, dst_ld);
    WM_LAUNCH_CHECK(stream, "mel_gather");
    return 0;
}

}  // namespace wm

using namespace wm;

extern "C" size_t wm_speech_spans_workspace_bytes(int batch, int64_t total_frames) {
    if (batch < 1 || total_frames < 0) return 0;
    return speech_spans_workspace_bytes(batch, total_frames);
}

extern "C" int wm_speech_spans(const void* const* src, const int32_t* src_ld, const int32_t* content, int batch, int n_mels, int h,
                               int step, int permille, int min_silence, int min_speech, int pad, int32_t* spans, int spans_ld,
                               int32_t* n_spans, void* workspace, size_t workspace_bytes, int64_t total_frames, wm_stream_t stream) {
    WM_REQUIRE(src && src_ld && content && spans && n_spans && workspace, "wm_speech_spans: null argument");
    WM_REQUIRE(batch >= 1 && n_mels >= 1 && spans_ld >= 0, "wm_speech_spans: batch=%d n_mels=%d must be >= 1, spans_ld=%d >= 0", batch,
               n_mels, spans_ld);
    WM_REQUIRE(step >= 1 && step <= 32768 && permille >= 0 && permille <= 1000,
               "wm_speech_spans: need 1 <= step <= 32768 and 0 <= permille <= 1000, got step=%d permille=%d", step, permille);
    WM_REQUIRE(min_silence >= 1 && min_speech >= 1 && pad >= 0,
               "wm_speech_spans: need min_silence >= 1, min_speech >= 1 and pad >= 0, got %d, %d, %d", min_silence, min_speech, pad);
    WM_REQUIRE(h >= 0 && (int64_t)n_mels * (2 * (int64_t)h + 1) < 131072, "wm_speech_spans: n_mels * (2h + 1) = %d * (2 * %d + 1) must be "
               "below 131072 (32-bit sums)", n_mels, h);
    WM_REQUIRE(total_frames >= 0 && total_frames < ((int64_t)1 << 40), "wm_speech_spans: total_frames=%lld", (long long)total_frames);
    WM_REQUIRE((total_frames + SC_THREADS - 1) / SC_THREADS <= 0x7fffffffLL, "wm_speech_spans: total_frames=%lld needs too many workgroups",
               (long long)total_frames);
    WM_REQUIRE(workspace_bytes >= speech_spans_workspace_bytes(batch, total_frames),
               "wm_speech_spans: workspace of %zu bytes, wm_speech_spans_workspace_bytes(%d, %lld) = %zu", workspace_bytes, batch,
               (long long)total_frames, speech_spans_workspace_bytes(batch, total_frames));
    WM_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)spans & 3) == 0 && ((uintptr_t)n_spans & 3) == 0,
               "wm_speech_spans: workspace must be 8-byte aligned, spans and n_spans 4-byte aligned");
    return launch_speech_spans(src, src_ld, content, batch, n_mels, h, step, permille, min_silence, min_speech, pad, spans, spans_ld,
                               n_spans, workspace, total_frames, (hipStream_t)stream);
}

extern "C" int wm_mel_gather(const void* const* src, const int32_t* src_ld, const int32_t* spans, const int32_t* n_spans, int spans_ld,
                             int batch, int n_mels, int n_pad, void* const* dst, const int32_t* dst_ld, wm_stream_t stream) {
    WM_REQUIRE(src && src_ld && spans && n_spans && dst && dst_ld, "wm_mel_gather: null argument");
    WM_REQUIRE(batch >= 1 && batch <= 65535 && n_mels >= 1 && n_mels <= 65535 * MG_ROWS,
               "wm_mel_gather: batch=%d must be in 1 .. 65535, n_mels=%d in 1 .. %d", batch, n_mels, 65535 * MG_ROWS);
    WM_REQUIRE(spans_ld >= 0 && n_pad >= 0, "wm_mel_gather: spans_ld=%d and n_pad=%d must not be negative", spans_ld, n_pad);
    WM_REQUIRE(((uintptr_t)spans & 3) == 0 && ((uintptr_t)n_spans & 3) == 0, "wm_mel_gather: spans and n_spans must be 4-byte aligned");
    return launch_mel_gather(src, src_ld, spans, n_spans, spans_ld, batch, n_mels, n_pad, dst, dst_ld, (hipStream_t)stream);
}
