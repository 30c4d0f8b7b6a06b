// The decoder engine's token step (WhisperDecoder.forward, R/tensorrt_llm/models/whisper/model.py:241-299, block :61-122): the workspace
// layout, the switches between the forms of a step, GroupStep -- one utterance group's step as a sequence of launches -- and the
// wm_decoder_* / wm_step_* / wm_profile_* / wm_set_* entries of the C ABI.  Enqueued on the caller's stream, as engine.hip's sequences are.
#include <stdio.h>
#include <string.h>

#include <atomic>

#include "engine_internal.h"

using namespace wm;

namespace {
// ---- in-situ kernel timing for the roofline report (bench.py): HIP event pairs around sampled
// launches of the decode cross-attention kernel, on the stream it is launched on ------------------
// One sampler and one diagnostic timeline PER DEVICE (one process may drive several GPUs, each from its own
// thread): wm_profile_* / wm_debug_timeline act on the calling thread's current device, the decode step on its
// engine's device; the mutex covers slot allocation.
constexpr int MAX_DEVICES = 64;
struct Profiler {
    bool enabled = false; int layer_stride = 1;
    std::vector<hipEvent_t> start, stop; size_t used = 0;
    long long* timeline = nullptr; int timeline_cap = 0;
};
std::mutex g_prof_mu;
Profiler g_prof_dev[MAX_DEVICES];
int current_device_index() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) dev = 0;
    return dev;
}

// a free sample slot for an eager launch of layer `layer`, or -1; the launch itself stamps the slot's events
int prof_slot(Profiler& pr, int layer, hipStream_t s) {
    if (!pr.enabled) return -1;
    std::lock_guard<std::mutex> lock(g_prof_mu);
    if (layer % pr.layer_stride != 0 || pr.used >= pr.start.size()) return -1;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return -1;   // eager launches only
    return (int)pr.used++;
}

struct DecWs { h16 *x, *xn, *ctx, *hid; float* part; float* cross_ws; size_t part_elems; int nsplit; size_t total;
               h16* logit_stage;                // block prefill only: logits rows of a chunk of utterances before they are scattered
               unsigned long long *gran_x, *gran_h, *gran_q, *gran_c, *gran_p, *gran_s; wm::ChainLayerIo* layer_io; unsigned* generation; };      // granule edges of the one-row chain (gemv_chain.hip) and its call counter

int cross_nsplit(int B, int H) {
    // Pieces the key range of the decode cross-attention is cut into (one workgroup per (utterance, head, piece), partial
    // softmaxes merged by attn_cross_combine_kernel).  TWO classes only, by the number of (utterance, head) pairs of the group:
    // up to 160 pairs (8 utterances of large-v2; round 5: 8 included, so that the one-launch step of up to eight rows has ONE form of the
    // cross-attention to reproduce -- r3au below: 2.15 / 2.13 ms with 1 / 4 pieces at 8 utterances) -> 4 pieces, otherwise the exact single pass without a merge launch.
    // Within a class a row's result does not depend on the batch it is in.  Rounds 1-3 used ceil(512 / pairs) <= 8 pieces
    // ("two workgroups per CU"): 8 different counts below 26 utterances, i.e. 8 different roundings of the merged softmax,
    // and no faster -- forced counts, token step in ms (profiles/r3au_cross_nsplit_forced.txt): 1 utterance 1.74 /
    // 1.65 / 1.58 / 1.58 with 1 / 2 / 4 / 8 pieces, 4 utterances 2.00 / 1.92 / 1.89 / 1.88, 6: 2.09 / 2.04 / 2.01 / 2.06,
    // 8: 2.15 / 2.16 / 2.13 (4), 12: 2.33 / 2.37 / 2.38 (1 / 2 / 3), 2 x 12: 2.86 / 2.91 / 3.01, 2 x 16: 3.41 / 3.44 / 3.47.
    // WM_CROSS_NSPLIT=n forces a count (A/B runs), -1 = 8 pieces below 512 pairs, -2 = the old rule.
    static const int forced = lab_env_int("WM_CROSS_NSPLIT", 0);
    if (forced == -1) return B * H >= 512 ? 1 : 8;
    if (forced == -2) { int n = (512 + B * H - 1) / (B * H); return n < 1 ? 1 : (n > 8 ? 8 : n); }
    if (forced > 0) return forced > 8 ? 8 : forced;
    return B * H <= 160 ? 4 : 1;
}

// candidate groups (wm_decoder_group_io::cross_group = G > 1, one token per row): the cross-attention launch has H * B / G * nsplit items, so
// the key range is cut for B / G utterances.  The workspace is sized for the most pieces any group size of the batch takes, so that
// wm_decoder_workspace_bytes(batch, n_new) holds for every cross_group and the layout does not depend on it.
int cross_nsplit_group(int B, int H, int L, int G) { return (G > 1 && L == 1) ? cross_nsplit(B / G, H) : cross_nsplit(B, H); }
int cross_nsplit_most(int B, int H, int L) {
    int n = cross_nsplit(B, H);
    for (int G = 2; L == 1 && G <= CROSS_GROUP_MAX; ++G)
        if (B % G == 0) { const int m = cross_nsplit(B / G, H); n = n > m ? n : m; }
    return n;
}

// lean (wm_decoder_prefill): no key-range pieces and no one-launch state -- the block prefill never takes those forms -- and a staging
// block of at most SKINNY_MAX_M logits rows instead; everything else is the decode step's layout at M = B * L rows, linear in M
DecWs carve_decoder(const wm_engine* e, int B, int L, void* ws, int G = 1, bool lean = false) {
    const wm_dims& d = e->dims;
    const size_t C = d.n_text_state, M = (size_t)B * L;
    Carver c{(unsigned char*)ws, 0};
    DecWs w{};
    w.x = c.take<h16>(M * C); w.xn = c.take<h16>(M * C); w.ctx = c.take<h16>(M * C); w.hid = c.take<h16>(M * 4 * C);
    // split-K slabs: the widest product is ksplit * N over the six Linears; ksplit <= 24 by construction
    size_t widest = 0;
    const int Mc = (int)(M < SKINNY_MAX_M ? M : SKINNY_MAX_M);
    const int q = e->dec.empty() ? (e->w8() ? 1 : 0) : e->dec[0].qkv.wcode;     // every Linear of an engine shares one encoding
    const int Ns[6] = {(int)(3 * C), (int)C, (int)C, (int)C, (int)(4 * C), (int)C};
    const int Ks[6] = {(int)C, (int)C, (int)C, (int)C, (int)C, (int)(4 * C)};
    for (int i = 0; i < 6; ++i) {
        const int s = skinny_default_ksplit(Mc, Ks[i], Ns[i] / 16, q);
        widest = widest > (size_t)s * Ns[i] ? widest : (size_t)s * Ns[i];
    }
    w.part_elems = widest * M;
    w.part = c.take<float>(w.part_elems);
    w.nsplit = cross_nsplit_group(B, d.n_text_head, L, G);
    if (lean) {                // (cross_ws and the one-launch state stay null)
        w.logit_stage = c.take<h16>((M < (size_t)SKINNY_MAX_M ? M : (size_t)SKINNY_MAX_M) * d.n_vocab);
        w.total = align_up(c.off);
        return w;
    }
    w.cross_ws = c.take<float>((size_t)B * d.n_text_head * cross_nsplit_most(B, d.n_text_head, L) * L * 66);
    const size_t R = M < (size_t)CHAIN_MAX_ROWS ? M : (size_t)CHAIN_MAX_ROWS;      // rows the one-launch step serves (gemv_chain.hip): every edge [rows][...]
    w.gran_x = c.take<unsigned long long>(R * (C / 2) + 8);
    w.gran_h = c.take<unsigned long long>(R * 2 * C + 8);
    w.gran_q = c.take<unsigned long long>(R * C + 8);
    w.gran_c = c.take<unsigned long long>(R * (C / 2) + 8);
    w.gran_p = c.take<unsigned long long>(R * d.n_text_head * 66 * 4 + 8);
    w.gran_s = c.take<unsigned long long>(R * 3 * C + 8);
    w.layer_io = c.take<wm::ChainLayerIo>((size_t)d.n_text_layer);
    w.generation = c.take<unsigned>(4);
    w.total = align_up(c.off);
    return w;
}

// skinny GEMM over all M rows in chunks of SKINNY_MAX_M; slabs laid out [ksplit][M_total][ldp]
int skinny_all(const Lin& l, const h16* A, int lda, int M, float* part, int* ksplit_out, hipStream_t s) {
    const int Mc = M < SKINNY_MAX_M ? M : SKINNY_MAX_M;
    const int ks = skinny_default_ksplit(Mc, l.K, l.n_blocks, l.wcode);
    for (int r0 = 0; r0 < M; r0 += SKINNY_MAX_M) {
        GemmSkinnyParams p{};
        p.A = A + (size_t)r0 * lda; p.lda = lda; p.M = (M - r0) < SKINNY_MAX_M ? (M - r0) : SKINNY_MAX_M; p.K = l.K;
        p.Wt = l.w; p.n_blocks = l.n_blocks; p.w8 = l.wcode; p.scale = l.s; p.ksplit = ks;
        p.part = part + (size_t)r0 * l.N; p.part_sstride = (long)M * l.N;
        if (launch_gemm_skinny(p, s)) return 2;
    }
    *ksplit_out = ks;
    return 0;
}

constexpr int DEC_CHUNK = 4;      // query tokens per pass of the decoder kernels (attn_decode.hip: MAX_L)

// diagnostic timeline (wm_debug_timeline): Profiler::timeline of the engine's device
extern "C" __global__ void stamp_kernel(long long* tl, int cap, long long tag, long long what) {
    if (threadIdx.x != 0) return;
    const int i = atomicAdd((int*)tl, 1);
    if (i < cap) { tl[1 + 3 * i] = tag; tl[2 + 3 * i] = what; tl[3 + 3 * i] = wall_clock64(); }
}

// Round 2 put the switch at 8 rows (8 rows 2.43 vs 2.56 ms per token, 2 x 8 rows 2.79 vs 2.92; 2 x 16 rows 3.70 vs 3.52 the other way).  Re-measured
// at the end of round 3 (four-wave self-attention on this side of the switch, graphs replayed node by node; profiles/r3an_small_path_switch.txt):
// 12 rows 2.38 vs 2.60 ms on the split-K chain, 2 x 12 rows 3.00 vs 3.13, 16 rows 2.68 vs 2.79, 2 x 16 rows 3.43 either way -> 16 rows (one MFMA row tile).
constexpr int SMALL_PATH_DEFAULT_ROWS = 16;
// Small batches (M = B * L <= SMALL_PATH_DEFAULT_ROWS rows) take the fused path of gemv_small.hip: every Linear is ONE launch
// that also applies the LayerNorm of its input rows and its own epilogue (bias / GELU / residual) -- 8 launches per layer
// instead of 12, no fp32 slabs, no row kernels.  WM_SMALL_PATH=<rows> moves the switch (0: the big-batch kernels for every size).
// (For more rows the same fusion was built into gemm_skinny.hip and measured: without a K split its 10-40 workgroups each
// stage the whole activation block, 70 us per launch at M = 192 against 16 + 10 for the split GEMM + row kernel, and the
// decode step at B = 576 went from 26.1 to 30.3 ms -- profiles/r2d_b576_fused_skinny_ks1_kernel_stats.csv.  Not kept.)
// exact V-row skipping of the decode cross-attention (attn_decode.hip, SKIP): on unless switched off (wm_set_cross_v_skip)
std::atomic<int> g_cross_v_skip{CROSS_V_SKIP_DEFAULT};
// the one-row chain (gemv_chain.hip): a decoder layer at batch 1 in 5 launches instead of 9 (wm_set_decode_chain)
std::atomic<int> g_decode_chain{DECODE_CHAIN_DEFAULT};
// What the one-launch forms need to know about a DEVICE.  `err` is the word a wave of a chain sets when it gives up a bounded wait (a
// workgroup of the launch was not running): it lives in pinned host memory that the device reaches directly, so the host reads it
// without a copy or a synchronisation -- every decoder call looks at it.  `declined` is sticky: once a launch has given up, the device
// is not trusted to hold a chain's workgroups together any more and every later call takes the launch-per-kernel path
// (wm_set_decode_chain re-arms).  `resident` caches the occupancy verdict per kernel variant and LDS footprint.
struct ChainDev {
    std::mutex mu;
    int n_cu = 0;
    unsigned* err_host = nullptr; unsigned* err_dev = nullptr;
    bool declined = false; std::string reason, footprint;
    std::map<long long, bool> resident;
    std::atomic<long long> launches{0};
    std::atomic<long long> declined_calls{0};
};
ChainDev g_chain_dev[64];
static ChainDev& chain_dev_slot(int device) { return g_chain_dev[device >= 0 && device < 64 ? device : 0]; }
// first use on a device: the CU count and the error word (the calling thread's current device is the engine's)
int chain_dev_init(ChainDev& cd, int device) {
    std::lock_guard<std::mutex> lk(cd.mu);
    if (cd.n_cu > 0 && cd.err_host) return 0;
    int v = 0;
    WM_CHECK_HIP(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device));
    void* host = nullptr; void* dev = nullptr;
    WM_CHECK_HIP(hipHostMalloc(&host, 64, hipHostMallocMapped | hipHostMallocCoherent));
    memset(host, 0, 64);
    WM_CHECK_HIP(hipHostGetDevicePointer(&dev, host, 0));
    cd.err_host = (unsigned*)host; cd.err_dev = (unsigned*)dev;
    cd.n_cu = v > 0 ? v : 1;
    return 0;
}
inline unsigned chain_err_peek(const ChainDev& cd) {
    return cd.err_host ? __atomic_load_n(cd.err_host, __ATOMIC_RELAXED) : 0u;
}
// a stream created with a CU mask (wm_stream_create_cu_mask, hipExtStreamCreateWithCUMask) that leaves it fewer CUs than the device
// has cannot hold a chain's workgroups together.  A query that fails says nothing: the stream is taken for an ordinary one.
bool stream_has_all_cus(hipStream_t s, int n_cu) {
    uint32_t mask[32];
    memset(mask, 0, sizeof(mask));
    if (hipExtStreamGetCUMask(s, 32, mask) != hipSuccess) { (void)hipGetLastError(); return true; }
    int bits = 0;
    for (uint32_t m : mask) bits += __builtin_popcount(m);
    return bits == 0 || bits >= n_cu;        // (no bit at all: the runtime reports no mask)
}
std::atomic<int> g_small_rows{-1};        // -1: not yet read from the environment
int small_path_max_rows() {               // WM_SMALL_PATH=<rows> / wm_set_small_batch_rows: the fused path serves M <= rows (0: never)
    int r = g_small_rows.load(std::memory_order_relaxed);
    if (r < 0) {
        r = lab_env_int("WM_SMALL_PATH", SMALL_PATH_DEFAULT_ROWS);
        r = r < 0 ? 0 : (r > GEMV_SMALL_MAX_M ? GEMV_SMALL_MAX_M : r);
        g_small_rows.store(r, std::memory_order_relaxed);
    }
    return r;
}

// Groups of at least rows_path_min_rows() rows (above the small-batch switch) take the row-split form of the same fused Linears
// (gemm_rows.hip) for every projection whose input is n_state wide: 10 launches per layer instead of 12, fp32 slabs only
// behind the MLP's second Linear.  Default 40 rows (WM_ROWS_MIN; WM_ROWS_PATH=0 or wm_set_rows_path(0): never -- the split-K
// chain, gemm_skinny + row kernel, for every Linear as in rounds 1-2).  Measured per token step, large-v2 int8, split-K chain vs
// row-split form (profiles/r3k_batch_sweep.txt): 12 rows 2.81 / 2.99 ms, 2 x 16 rows 3.55 / 3.69, 2 x 32 rows 4.69 / 5.09,
// 3 x 43 rows 7.42 / 7.21, 3 x 192 rows 25.2 / 23.4 -- below ~40 rows a group's step is a chain of latencies and the split-K
// GEMM + row kernel pair (two short launches on 40-160 workgroups) is the quicker link; above, the hand-overs' bytes decide.
std::atomic<int> g_rows_min{-1};          // -1: not yet read from the environment; 0: never
int rows_path_min_rows() {
    int r = g_rows_min.load(std::memory_order_relaxed);
    if (r < 0) {
        r = lab_env_int("WM_ROWS_PATH", 1) == 0 ? 0 : lab_env_int("WM_ROWS_MIN", 40);
        if (r < 0) r = 0;
        g_rows_min.store(r, std::memory_order_relaxed);
    }
    return r;
}

// Waves per (b, h) of the decode self-attention: 0 = by size (the small-batch side of the switch above runs the four-wave
// workgroup form, attn_decode.hip), 1 / 4 = forced (WM_SELF_WAVES, wm_set_self_attn_waves).
std::atomic<int> g_self_waves{-1};
}  // namespace
int wm::cross_v_skip() { return g_cross_v_skip.load(std::memory_order_relaxed); }
int wm::self_attn_waves(int rows) {
    int w = g_self_waves.load(std::memory_order_relaxed);
    if (w < 0) {
        w = lab_env_int("WM_SELF_WAVES", 0);
        if (w != 1 && w != 4) w = 0;
        g_self_waves.store(w, std::memory_order_relaxed);
    }
    return w ? w : (rows <= small_path_max_rows() ? 4 : 1);
}
namespace {

// rows (utterances) of a group the one-launch step serves: CHAIN_MAX_ROWS (8) unless WM_CHAIN_ROWS=n keeps it to fewer (lab: A/B runs)
int chain_max_rows() {
    static const int r = [] { const int v = lab_env_int("WM_CHAIN_ROWS", CHAIN_MAX_ROWS); return v < 1 ? 1 : (v > CHAIN_MAX_ROWS ? CHAIN_MAX_ROWS : v); }();
    return r;
}

// One utterance group's decode step, cut into the phases between which the cross-attention kernel sits, so
// that several groups can be interleaved layer by layer (wm_decoder_step_multi).
// The step plan: a layer has three NORMED Linears -- qkv, cq, mlp1: l(LayerNorm(x)) -- and three RESIDUAL Linears --
// out, cout, mlp2: x += l(src).  The forms differ only in where the LayerNorm sits -- fused small: in the prologue of the consumer;
// split-K: in the row kernel of the producer, which leaves xn; row-split: as fused small, except that mlp2 goes through slabs and the row
// kernel, whose xn qkv then reads -- and are chosen in normed() and residual() only; pre_cross() and post_cross() are the layer in those words.
struct GroupStep {
    const wm_engine* e; const wm_decoder_io* io; DecWs w;
    int B, L, T, C, H, M;
    int G = 1;                                   // candidate rows per utterance that share one cross K/V row (wm_decoder_group_io::cross_group)
    const int32_t* live_groups = nullptr;        // ... and the utterances with a live row (beside io->live_rows)
    bool small = false;                          // the fused small-batch path (gemv_small.hip)
    bool chain = false;                          // ... with its Linears chained inside one launch (gemv_chain.hip): per decoder layer,
    bool whole = false;                          // ... or per token step (cross() and post_cross() have nothing left to do in either)
    int chain_wgs = 0; unsigned* chain_err = nullptr; ChainDev* chain_cd = nullptr;
    bool rows = false;                           // the fused row-split path (gemm_rows.hip)
    bool fused() const { return small || rows; }
    bool prefill = false; int logits_from = 0;   // wm_decoder_prefill: any L on an empty cache, attn_prefill.hip's kernels, logits from a position on
    bool capturing = false;                      // the call's stream is being captured: asked once per call, in init()
    int cq_ks = 0;                               // slabs the cq sums wait in for the cross-attention kernel (and wm_decoder_step_tap)
    Profiler* prof = nullptr;

    // one Linear of the small-batch path.  mode as epilogue.h; ln_g != null: LayerNorm of the input rows (the residual stream)
    // inside the kernel
    int gemv(const Lin& l, const h16* A, int lda, int mode, const h16* ln_g, const h16* ln_b, h16* out16, int ld16, hipStream_t s) {
        GemvSmallParams p{};
        p.A = A; p.lda = lda; p.M = M; p.K = l.K; p.Wt = l.w; p.n_blocks = l.n_blocks; p.w8 = l.wcode; p.scale = l.s;
        p.ln_g = ln_g; p.ln_b = ln_b;                // the kernel normalises the (few) input rows itself
        p.mode = mode; p.bias = l.b; p.gelu_kind = e->gelu();
        p.out32 = w.part; p.ld32 = l.N;
        p.out16 = out16; p.ld16 = ld16; p.n_valid = l.N;
        p.x = w.x; p.ldx = C;
        return small ? launch_gemv_small(p, s) : launch_gemm_rows(p, s);
    }

    int finish(const Lin& l, int ks, int mode, const h16* g, const h16* bta, h16* out, int ldo, int N, hipStream_t s) {
        RowFinishParams p{};
        p.part = w.part; p.ksplit = ks; p.M = M; p.N = N; p.ldp = l.N; p.part_sstride = (long)M * l.N;
        p.bias = l.b; p.mode = mode; p.gelu_kind = e->gelu(); p.x = w.x; p.ldx = C; p.ln_g = g; p.ln_b = bta;
        p.out = out; p.ldo = ldo;
        return launch_row_finish(p, s);
    }

    // diagnostic (WM_TIMELINE_FINE=1 with wm_debug_timeline): a stamp behind EVERY kernel of the chain, code 1000 + 32 * layer + position
    // (scripts/chain_probe.py turns them into in-situ durations per chain position); the K/V launch keeps its own pair of stamps
    void mark(int layer, int pos, hipStream_t s) {
        static const bool fine = lab_env_int("WM_TIMELINE_FINE", 0) == 1;
        if (fine && prof->timeline)
            hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(64), 0, s, prof->timeline, prof->timeline_cap, (long long)(uintptr_t)io->logits, (long long)(1000 + 32 * layer + pos));
    }

    // A normed Linear of layer i: the sums of l(LayerNorm(x; g, b)) wait in w.part (*ks slabs) for the attention kernel behind it, or, with `hid`
    // (mlp1), GELU(sums + bias) goes there.  from_xn: the row-split form finds LayerNorm(x) in w.xn (qkv).  Stamp `pos` behind the last launch.
    int normed(int i, int pos, const Lin& l, const h16* g, const h16* b, bool from_xn, h16* hid, int* ks, hipStream_t s) {
        if (fused()) {
            const bool pre = small || !from_xn;      // the LayerNorm in the kernel's prologue
            if (gemv(l, pre ? w.x : w.xn, C, hid ? 1 : 0, pre ? g : nullptr, pre ? b : nullptr, hid, hid ? l.N : 0, s)) return 2;
            *ks = 1;
        } else {
            if (skinny_all(l, w.xn, C, M, w.part, ks, s)) return 2;
            if (hid) {
                mark(i, pos - 1, s);
                if (finish(l, *ks, 1, nullptr, nullptr, hid, l.N, l.N, s)) return 2;
            }
        }
        mark(i, pos, s);
        return 0;
    }

    // A residual Linear of layer i: x += l(src) + bias, then -- where the form keeps an xn -- xn = LayerNorm(x; g, b) for the normed Linear
    // behind it (g == null: none, the sums are only added).  Stamps: `pos` behind the product, pos + 1 behind the row kernel.
    int residual(int i, int pos, const Lin& l, const h16* src, const h16* g, const h16* b, hipStream_t s) {
        const bool wide = l.K != C;                  // mlp2
        if (small || (rows && !wide)) {
            if (gemv(l, src, l.K, 2, nullptr, nullptr, nullptr, 0, s)) return 2;
            if (!wide) mark(i, pos, s);              // (behind the small form's mlp2 the next layer's position 0 is the stamp)
            return 0;
        }
        // split-K, and the row-split form's mlp2: K = 4 n_state: the hidden rows of a 32-row block do not fit one workgroup's LDS -- K
        // slices over workgroups (and row splits), the row kernel adds them to the residual stream and applies the next layer's first
        // LayerNorm, whose output 60-80 column groups of the qkv projection would otherwise each recompute
        int ks = 0;
        if (skinny_all(l, src, l.K, M, w.part, &ks, s)) return 2;
        mark(i, pos, s);
        if (finish(l, ks, g ? 0 : 3, g, b, g ? w.xn : nullptr, g ? C : 0, C, s)) return 2;
        mark(i, pos + 1, s);
        return 0;
    }

    // alone: no other group's step is issued beside this one.  The one-launch forms need their 256 workgroups resident TOGETHER (one
    // fills a CU's LDS); two such launches dispatched side by side on two streams could each get half of the chip and wait for the
    // other half until the bounded waits give up -- so only a step that runs alone takes them.
    int init(const wm_engine* e_, const wm_decoder_io* io_, hipStream_t stream, bool alone = true, int cross_group = 0,
             const int32_t* live_groups_ = nullptr) {
        e = e_; io = io_; live_groups = live_groups_;
        const char* who = prefill ? "wm_decoder_prefill" : "wm_decoder_step";      // the entry a refusal names
        prof = &g_prof_dev[e->device >= 0 && e->device < MAX_DEVICES ? e->device : 0];
        WM_REQUIRE(io && io->tokens && io->positional_embedding && io->present && io->cross && io->logits && io->workspace,
                   "%s: null argument", who);
        const wm_dims& d = e->dims;
        B = io->batch; L = io->n_new; T = io->n_past; C = d.n_text_state; H = d.n_text_head; M = B * L;
        WM_REQUIRE(B >= 1 && L >= 1 && (prefill || L <= 4) && T >= 0, "%s: bad batch/n_new/n_past (%d, %d, %d)", who, B, L, T);
        WM_REQUIRE(T + L <= d.n_text_ctx, "%s: T+L=%d exceeds n_text_ctx=%d", who, T + L, d.n_text_ctx);
        WM_REQUIRE(T == 0 || io->past, "%s: n_past > 0 needs past buffers", who);
        WM_REQUIRE(T == 0 || io->past_capacity >= T, "%s: past capacity %d < n_past %d", who, io->past_capacity, T);
        WM_REQUIRE(io->present_capacity >= T + L, "%s: present capacity %d < n_past + n_new = %d", who, io->present_capacity, T + L);
        WM_REQUIRE(!io->n_past_dev || (L == 1 && io->past), "%s: a device step counter needs n_new == 1 and past buffers", who);
        WM_REQUIRE(C == H * 64, "head size must be 64");
        G = cross_group > 1 ? cross_group : 1;
        WM_REQUIRE(cross_group >= 0 && B % G == 0 && (prefill || G * L <= CROSS_GROUP_MAX),
                   "wm_decoder_step_group: cross_group=%d needs batch=%d a multiple of it and cross_group * n_new=%d <= %d", cross_group, B, G * L, CROSS_GROUP_MAX);
        WM_REQUIRE(!(G > 1 && L == 1 && io->live_rows) || live_groups, "wm_decoder_step_group: cross_group with live_rows needs live_groups (wm_step_finish_group)");
        w = carve_decoder(e, B, L, io->workspace, G, prefill);
        WM_REQUIRE(io->workspace_bytes >= w.total, "decoder workspace too small: %zu < %zu", io->workspace_bytes, w.total);
        small = M <= small_path_max_rows();
        rows = !small && rows_path_min_rows() > 0 && M >= rows_path_min_rows() && !e->dec.empty() && gemm_rows_supports(C, e->dec[0].qkv.wcode);
        chain = whole = false;
        hipStreamCaptureStatus cap_st = hipStreamCaptureStatusNone;
        capturing = hipStreamIsCapturing(stream, &cap_st) == hipSuccess && cap_st != hipStreamCaptureStatusNone;
        ChainDev& cd = chain_dev_slot(e->device);
        // A chain launch on this device has given up a wait and nobody has acknowledged it (wm_decode_chain_error): the results of that
        // step -- and of everything decoded from it -- are invalid.  Every decoder call fails loudly until the caller has looked.
        // (Not while a stream is being captured: the call issues no work then, and failing it would abort the caller's capture.)
        if (!capturing && chain_err_peek(cd) != 0) {
            set_error("%s: a one-launch decode step on device %d gave up waiting for its workgroups (they were not resident "
                      "together): the results since then are invalid.  Call wm_decode_chain_error() to acknowledge and decode again -- the device "
                      "takes the launch-per-kernel path from then on (wm_set_decode_chain re-arms the one-launch forms)", who, e->device);
            return 1;
        }
        // the calls the one-launch forms exist for: a step of up to eight one-token rows that runs alone, without the calibration hook
        if (alone && small && L == 1 && M <= chain_max_rows() && !e->dec.empty() && e->chain_dev && g_decode_chain.load(std::memory_order_relaxed) && !io->qkv_amax)
            return admit_chain(cd, stream);
        return 0;
    }

    // One-launch admission: chain (and whole) for a call init() has found eligible.  One-row groups run a decoder layer (or the whole step)
    // as one launch -- with the in-place cache (past[i] == present[i]), four key-range pieces, fp16 cross K/V, the four-wave self-attention
    // form; anything else takes the launch-per-kernel path
    int admit_chain(ChainDev& cd, hipStream_t stream) {
        if (chain_dev_init(cd, e->device)) return 2;
        const int n_cu = cd.n_cu, wcode = e->dec[0].qkv.wcode;
        chain_wgs = n_cu > 256 ? 256 : n_cu; chain_err = cd.err_dev; chain_cd = &cd;
        const bool kernel_built = gemv_chain_supports(C, wcode, n_cu) && !(M > 2 && wcode == 4);        // (packed int4: one or two rows)
        const bool attention_forms = w.nsplit == 4 && !e->i8cross() && io->present_capacity <= 512;      // its copies of the attention kernels know one form each
        const int self_items = M * H, cross_items = M * H * w.nsplit;                                    // ... whose items all find a workgroup of the grid
        const bool grid_fits = M > 4 ? (self_items <= chain_wgs && cross_items <= 4 * chain_wgs)            // (5-8 rows: two items per workgroup and round, <= 2 rounds, beside the self-attention's heads)
                                     : self_items + (M > 2 ? (cross_items + 1) / 2 : cross_items) <= chain_wgs;      // (3, 4 rows: two cross-attention items per workgroup)
        bool ok = kernel_built && attention_forms && grid_fits && self_attn_waves(M) == 4;
        // the cache is appended to in place (the first step of a cache has no device step counter to follow)
        for (int i = 0; ok && i < e->dims.n_text_layer; ++i)
            ok = io->present[i] && io->cross[i] &&
                 (T == 0 ? io->n_past_dev == nullptr : (io->past[i] == io->present[i] && io->past_capacity == io->present_capacity));
        // ... and only where the launch's workgroups can be resident TOGETHER (they wait for each other): a device that has let a chain
        // down before is not asked again, the runtime's occupancy figure must cover the grid, and the stream must own every CU
        if (ok) {
            std::lock_guard<std::mutex> lk(cd.mu);
            ok = !cd.declined;
            const int i8 = e->i8kv() ? 1 : 0;
            const long long key = ((long long)M << 48) | ((long long)wcode << 40) | ((long long)i8 << 32) | ((long long)e->dims.n_audio_ctx << 8) | w.nsplit;
            auto it = cd.resident.find(key);
            if (ok && it == cd.resident.end()) {
                bool fits = false;
                char why[200] = "";
                if (gemv_chain_resident(wcode, i8, M, e->dims.n_audio_ctx, w.nsplit, chain_wgs, n_cu, &fits, why, sizeof(why))) return 2;
                it = cd.resident.emplace(key, fits).first;
                cd.footprint = why;
                if (!fits) cd.reason = why;
            }
            ok = ok && it->second;
        }
        if (ok && !stream_has_all_cus(stream, n_cu)) ok = false;
        if (!ok) cd.declined_calls.fetch_add(1, std::memory_order_relaxed);
        chain = ok;
        whole = chain && g_decode_chain.load(std::memory_order_relaxed) >= 2 && e->dims.n_text_layer <= 32 && e->chain_lstat;
        return 0;
    }

    // the arguments every chain launch shares
    void chain_common(GemvChainParams& p) {
        const wm_dims& d = e->dims;
        p.cross_Tk = d.n_audio_ctx; p.cross_heads = H; p.cross_nsplit = w.nsplit; p.gran_q = w.gran_q; p.cross_at = 1;
        p.gran_p = w.gran_p; p.merge_at = 2; p.merge_nsplit = w.nsplit; p.merge_heads = H;
        p.self_cap = io->present_capacity; p.self_T = T; p.self_t_dev = io->n_past_dev; p.self_heads = H; p.self_i8 = e->i8kv() ? 1 : 0;
        p.gran_c = w.gran_c;
        p.out32 = w.part; p.w8 = e->dec[0].out.wcode; p.gelu_kind = e->gelu();
        p.x = w.x; p.gran_x = w.gran_x; p.gran_h = w.gran_h; p.err = chain_err;
        p.generation = w.generation;
        p.rows = M;                                   // (L == 1: one row per utterance; the utterances' buffers are slices of [B, 2, H, T, 64])
        p.live = io->live_rows;                       // rows still decoding (optional): the others' attention stages read and append nothing
        p.cross_row_bytes = (long)2 * H * d.n_audio_ctx * 64 * 2;
        p.self_row_bytes = (long)2 * H * io->present_capacity * 64 * (e->i8kv() ? 1 : 2);
    }

    // decoder layer i of a one-row group as ONE launch (gemv_chain.hip): self-attention, out, cq, cross-attention, merge + cout, mlp1,
    // mlp2, the qkv sums of the next layer
    int run_layer(int i, hipStream_t s) {
        const DecLayer& Lr = e->dec[i];
        const bool more = i + 1 < e->dims.n_text_layer;
        GemvChainParams p{};
        chain_common(p);
        p.n_stages = more ? 6 : 5; p.st = e->chain_dev + 1 + (size_t)6 * i;
        p.cross_kv = (const h16*)io->cross[i]; p.cross_qbias = Lr.cq.b;
        p.self_part = w.part; p.self_bias = Lr.qkv.b; p.self_cache = io->present[i]; p.self_kv_scale = Lr.kv_scale;
        p.launch_id = i;
        chain_cd->launches.fetch_add(1, std::memory_order_relaxed);
        return launch_gemv_chain(p, &e->chain_host[1 + (size_t)6 * i], chain_wgs, s);
    }

    // The chain's state in the caller's workspace -- tagged granules, the call counter, the per-layer pointer table -- is the LIBRARY's to
    // initialise: the workspace arrives as the allocator left it (the reference's plugins get theirs the same way; INTEGRATION.md's stub
    // uses torch.empty).  A state the library has not initialised under this (address, workspace_id) is cleared by a memset ON THE
    // STREAM OF THE CALL, ahead of the embedding kernel that opens the call (which counts the cleared call counter up to 1: tag 0 is
    // never valid, and bit 31 of every epoch is set besides).  workspace_id == 0 vouches for nothing: cleared on every call.  Under
    // stream capture the nodes are recorded but not run, so a captured call is never REMEMBERED: one that meets a state no eager
    // call has initialised carries the initialisation inside its graph (every replay clears and rewrites: correct, slower), one that
    // follows an eager call on the same (address, id) -- decoding.py's order -- relies on the state that call left.
    // The whole step's per-layer cross K/V and cache pointers reach the kernel through the table, rewritten (small launches on this stream,
    // behind the embedding kernel) only when the caller's pointers differ from the ones last written there.  All of that bookkeeping is
    // here, under one lock and recorded before the work is enqueued; begin() and whole_step() only enqueue what it decided.
    bool ws_fresh = false, ws_table = false;     // clear the state ahead of the embedding launch / rewrite the table behind it
    std::vector<ChainLayerIo> ws_tab;            // (whole step) the caller's pointers of this call
    void plan_chain_workspace() {
        ws_fresh = true; ws_table = whole;
        ws_tab.resize(whole ? (size_t)e->dims.n_text_layer : 0);
        for (size_t i = 0; i < ws_tab.size(); ++i) ws_tab[i] = ChainLayerIo{io->cross[i], io->present[i]};
        if (io->workspace_id == 0) return;           // nothing is vouched for: cleared, and the table rewritten, on every call
        std::lock_guard<std::mutex> lk(e->chain_io_mu);
        auto it = e->chain_io_seen.find(w.layer_io);
        // known: an EAGER call has initialised this state under this id (it persists in the workspace: a call captured later
        // relies on it, like an eager one -- a memset node and four table launches in every replay cost the batch-1 step 2 %)
        ws_fresh = it == e->chain_io_seen.end() || it->second.id != io->workspace_id;
        if (ws_fresh) {
            if (capturing) return;                   // (a captured call enqueues nothing: it initialises inside its graph and is not remembered)
            if (e->chain_io_seen.size() > 4096) e->chain_io_seen.clear();
            it = e->chain_io_seen.emplace(w.layer_io, wm_engine::ChainWsSeen{}).first;
            it->second.id = io->workspace_id; it->second.tab.clear();
        }
        if (!whole) return;
        std::vector<ChainLayerIo>& seen = it->second.tab;
        ws_table = seen.size() != ws_tab.size() || memcmp(seen.data(), ws_tab.data(), ws_tab.size() * sizeof(ChainLayerIo)) != 0;
        if (ws_table && capturing) seen.clear();     // the replay will rewrite the table: what an eager call wrote is no longer known to be there
        else if (ws_table) seen = ws_tab;
    }

    // token + positional embedding, first LayerNorm
    int begin(hipStream_t s) {
        const wm_dims& d = e->dims;
        EmbedParams ep{io->tokens, io->tokens_ld > 0 ? io->tokens_ld : L, M, L, e->emb_t, C,
                       (const h16*)io->positional_embedding, w.x, C, d.n_vocab, io->n_past_dev, nullptr};
        ep.row_start = io->row_start; ep.T = T;
        ep.generation = chain ? w.generation : nullptr;      // the chain's granule epochs count the calls on this workspace
        if (chain) {
            plan_chain_workspace();
            unsigned char *lo = (unsigned char*)w.gran_x, *hi = (unsigned char*)(w.generation + 4);
            if (ws_fresh) WM_CHECK_HIP(hipMemsetAsync(lo, 0, (size_t)(hi - lo), s));
        }
        if (launch_embed(ep, s)) return 2;
        if (small) return 0;                         // the first LayerNorm happens inside the qkv projection
        return launch_layernorm(w.x, C, M, C, e->dec[0].ln1g, e->dec[0].ln1b, w.xn, C, s);
    }

    // The whole token step of a one-row group as ONE launch: [LayerNorm + qkv of layer 0], then per layer self-attention, out, cq,
    // cross-attention, merge + cout, mlp1, mlp2, qkv of the next layer -- gemv_chain.hip walks over the layers itself
    int whole_step(hipStream_t s) {
        if (ws_table && launch_chain_io_table(w.layer_io, ws_tab.data(), (int)ws_tab.size(), s)) return 2;
        GemvChainParams p{};
        chain_common(p);
        p.n_layers = e->dims.n_text_layer; p.lstat = e->chain_lstat; p.lio = w.layer_io; p.gran_s = w.gran_s;
        p.st = e->chain_dev; p.n_stages = 0; p.launch_id = 0;
        if (launch_gemv_chain(p, e->chain_host.data(), chain_wgs, s)) return 2;
        chain_cd->launches.fetch_add(1, std::memory_order_relaxed);
        return 0;
    }

    // self-attention block and the cross-attention query projection of layer i
    int pre_cross(int i, hipStream_t s) {
        const DecLayer& Lr = e->dec[i];
        if (whole) return i == 0 ? whole_step(s) : 0;
        mark(i, 0, s);
        int ks = 1;
        if (chain && i > 0) mark(i, 1, s);           // (chained: layers > 0 got their qkv sums from the chain that closed the layer before)
        else if (normed(i, 1, Lr.qkv, Lr.ln1g, Lr.ln1b, true, nullptr, &ks, s)) return 2;      // qkv sums -> w.part [M][3C]
        AttnSelfParams p{};
        p.part = w.part; p.ksplit = ks; p.ldp = Lr.qkv.N; p.part_sstride = (long)M * Lr.qkv.N; p.bias = Lr.qkv.b;
        p.B = B; p.L = L; p.T = T; p.H = H;
        WM_REQUIRE(io->present[i], "wm_decoder_step: present[%d] is null", i);
        p.present = io->present[i]; p.present_cap = io->present_capacity; p.present_bstride = (long)2 * H * io->present_capacity * 64;
        if (T > 0) {
            WM_REQUIRE(io->past[i], "wm_decoder_step: past[%d] is null", i);
            p.past = io->past[i]; p.past_cap = io->past_capacity; p.past_bstride = (long)2 * H * io->past_capacity * 64;
        } else { p.past = p.present; p.past_cap = p.present_cap; p.past_bstride = p.present_bstride; }
        p.int8_kv = e->i8kv(); p.kv_scale = Lr.kv_scale; p.out = w.ctx; p.ldo = C;
        p.amax = io->qkv_amax ? io->qkv_amax + i : nullptr;
        p.t_dev = io->n_past_dev;
        p.live = io->live_rows;
        p.row_start = io->row_start;
        p.waves = self_attn_waves(M);
        if (chain) {                   // the whole layer in one launch (a live-row list is not consulted: a one-row group is stepped while its
                                       // row decodes; the steps between the row's EOT and the host's next poll compute values nobody reads)
            if (run_layer(i, s)) return 2;
            mark(i, 12, s);
            return 0;
        }
        if (prefill ? launch_attn_prefill_self(p, s) : launch_attn_self(p, s)) return 2;
        mark(i, 2, s);
        if (residual(i, 3, Lr.out, w.ctx, Lr.lncg, Lr.lncb, s)) return 2;                       // x += out(ctx)
        return normed(i, 5, Lr.cq, Lr.lncg, Lr.lncb, false, nullptr, &cq_ks, s);                // q sums -> w.part [M][C]
    }

    // the HBM-bound kernel: K and V of every utterance of the group, once
    int cross(int i, hipStream_t s) {
        if (chain) return 0;                             // done by the chain launch
        if (!prof->timeline) return cross_launch(i, s);
        hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(64), 0, s, prof->timeline, prof->timeline_cap, (long long)(uintptr_t)io->logits, (long long)(2 * i));
        const int rc = cross_launch(i, s);
        hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(64), 0, s, prof->timeline, prof->timeline_cap, (long long)(uintptr_t)io->logits, (long long)(2 * i + 1));
        return rc;
    }

    int cross_launch(int i, hipStream_t s) {
        const DecLayer& Lr = e->dec[i];
        const wm_dims& d = e->dims;
        AttnCrossParams p{};
        p.part = w.part; p.ksplit = cq_ks; p.ldp = Lr.cq.N; p.part_sstride = (long)M * Lr.cq.N; p.bias = Lr.cq.b;
        p.B = B; p.L = L; p.H = H; p.Tk = d.n_audio_ctx;
        WM_REQUIRE(io->cross[i], "wm_decoder_step: cross[%d] is null", i);
        p.kv = (const h16*)io->cross[i]; p.kv_bstride = (long)2 * H * d.n_audio_ctx * 64;
        p.kv_q8_scale = e->i8cross() ? Lr.cross_scale : 0.f;
        p.out = w.ctx; p.ldo = C; p.nsplit = w.nsplit; p.ws = w.cross_ws;
        p.live = io->live_rows;
        if (prefill) return launch_attn_prefill_cross(p, s) ? 2 : 0;
        p.G = G; p.live_utt = (G > 1 && L == 1 && io->live_rows) ? live_groups : nullptr;
        p.skip_zero_rows = cross_v_skip();
        const int slot = (L == 1) ? prof_slot(*prof, i, s) : -1;
        if (launch_attn_cross(p, s, slot >= 0 ? prof->start[slot] : nullptr, slot >= 0 ? prof->stop[slot] : nullptr)) return 2;
        return 0;
    }

    // cross-attention output projection and the MLP of layer i (ends with the next layer's LayerNorm)
    int post_cross(int i, hipStream_t s) {
        const DecLayer& Lr = e->dec[i];
        int ks = 0;
        mark(i, 6, s);
        if (chain) return 0;                             // done by the chain launch
        if (residual(i, 7, Lr.cout, w.ctx, Lr.ln2g, Lr.ln2b, s)) return 2;
        if (normed(i, 10, Lr.mlp1, Lr.ln2g, Lr.ln2b, false, w.hid, &ks, s)) return 2;          // LN + GELU
        const bool last = (i + 1 == e->dims.n_text_layer);
        if (prefill && last) return residual(i, 11, Lr.mlp2, w.hid, nullptr, nullptr, s);       // (the final LayerNorm: end_prefill, on the rows it keeps)
        return residual(i, 11, Lr.mlp2, w.hid, last ? e->lnfg : e->dec[i + 1].ln1g, last ? e->lnfb : e->dec[i + 1].ln1b, s);
    }

    // logits = xn . E^T (fp16 out, whisper/model.py:288-290) for the R normalised rows in w.xn -> `dst` (row stride n_vocab): one
    // launch for few rows, else the vocabulary matrix streamed once per SKINNY_MAX_M rows
    int project_logits(int R, bool few, h16* dst, hipStream_t s) {
        const wm_dims& d = e->dims;
        if (few) {
            GemvSmallParams p{};
            p.A = w.xn; p.lda = C; p.M = R; p.K = C; p.Wt = e->emb_t; p.n_blocks = e->emb_blocks; p.w8 = 0;
            p.mode = 3; p.out16 = dst; p.ld16 = d.n_vocab; p.n_valid = d.n_vocab;
            return launch_gemv_small(p, s);
        }
        for (int r0 = 0; r0 < R; r0 += SKINNY_MAX_M) {
            GemmSkinnyParams p{};
            p.A = w.xn + (size_t)r0 * C; p.lda = C; p.M = (R - r0) < SKINNY_MAX_M ? (R - r0) : SKINNY_MAX_M; p.K = C;
            p.Wt = e->emb_t; p.n_blocks = e->emb_blocks; p.w8 = 0; p.ksplit = 1;
            p.out = dst + (size_t)r0 * d.n_vocab; p.ldc = d.n_vocab; p.n_valid = d.n_vocab;
            if (launch_gemm_skinny(p, s)) return 2;
        }
        return 0;
    }

    // final LayerNorm + logits of `R` consecutive rows of `src` (row stride C) -> `dst` (row stride n_vocab); w.xn holds the normalised rows
    int logits_rows(const h16* src, int R, h16* dst, hipStream_t s) {
        if (launch_layernorm(src, C, R, C, e->lnfg, e->lnfb, w.xn, C, s)) return 2;
        return project_logits(R, R <= small_path_max_rows(), dst, s);
    }

    // logits = ln(x) . E^T: the row kernel behind the last mlp2 has left ln(x) in w.xn, except in the small form -- there the final
    // LayerNorm is a launch of its own: 3 242 workgroups (16 vocabulary entries each) would all redo it
    int end(hipStream_t s) {
        if (small && launch_layernorm(w.x, C, M, C, e->lnfg, e->lnfb, w.xn, C, s)) return 2;
        return project_logits(M, small, (h16*)io->logits, s);
    }

    // block prefill: logits for the positions logits_from .. L - 1 of every utterance only; the others are left untouched.  The rows of
    // one utterance are consecutive in x and in `logits`; a few positions per utterance (logits_from = sot_index: three) are gathered
    // over as many utterances as fill one weight-streaming launch, so the vocabulary matrix is read once per SKINNY_MAX_M rows
    int end_prefill(hipStream_t s) {
        const wm_dims& d = e->dims;
        const int n = L - logits_from;
        h16* out = (h16*)io->logits;
        if (n == L) return logits_rows(w.x, M, out, s);
        if (n * 2 > SKINNY_MAX_M) {
            for (int b = 0; b < B; ++b)
                if (int rc = logits_rows(w.x + ((size_t)b * L + logits_from) * C, n, out + ((size_t)b * L + logits_from) * d.n_vocab, s)) return rc;
            return 0;
        }
        const int ub = SKINNY_MAX_M / n;
        for (int b0 = 0; b0 < B; b0 += ub) {
            const int nb = (B - b0) < ub ? (B - b0) : ub;
            if (launch_copy_rows2d(w.ctx, (long)n * C, w.x + ((size_t)b0 * L + logits_from) * C, (long)L * C, (long)n * C, nb, s)) return 2;
            if (int rc = logits_rows(w.ctx, nb * n, w.logit_stage, s)) return rc;
            if (launch_copy_rows2d(out + ((size_t)b0 * L + logits_from) * d.n_vocab, (long)L * d.n_vocab, w.logit_stage, (long)n * d.n_vocab,
                                   (long)n * d.n_vocab, nb, s)) return 2;
        }
        return 0;
    }

    // The walk over the layers that every entry with ONE group on ONE stream shares (wm_decoder_step_multi interleaves its groups itself);
    // between(i) runs behind pre_cross(i), when the cq sums of layer i wait in the workspace (wm_decoder_step_tap)
    template <typename Between> int run(hipStream_t s, Between between) {
        if (begin(s)) return 2;
        for (int i = 0; i < e->dims.n_text_layer; ++i) {
            if (pre_cross(i, s)) return 2;
            if (int rc = between(i)) return rc;
            if (cross(i, s)) return 2;
            if (post_cross(i, s)) return 2;
        }
        return prefill ? end_prefill(s) : end(s);
    }
    int run(hipStream_t s) { return run(s, [](int) { return 0; }); }
};

}  // namespace

extern "C" {
// ================================================================================================ decoder
// n_new <= 4: one pass.  Longer token blocks (prompts / prefixes, W/decoding.py:485-513) are run as 4-token
// passes over the growing cache; their logits pass through a [batch, 4, n_vocab] staging block at the end of the
// workspace and are copied into the caller's [batch, n_new, n_vocab] tensor.
size_t wm_decoder_workspace_bytes(const wm_engine* e, int batch, int n_new) {
    if (!e || e->kind != WM_ENGINE_DECODER || batch < 1 || n_new < 1) return 0;
    if (n_new <= DEC_CHUNK) return carve_decoder(e, batch, n_new, nullptr).total;
    return carve_decoder(e, batch, DEC_CHUNK, nullptr).total + align_up((size_t)batch * DEC_CHUNK * e->dims.n_vocab * sizeof(h16));
}

static int decoder_step(const wm_engine* e, const wm_decoder_io* io, int cross_group, const int32_t* live_groups, wm_stream_t stream_) {
    WM_REQUIRE(e && e->kind == WM_ENGINE_DECODER, "wm_decoder_step: not a decoder engine");
    hipStream_t s = (hipStream_t)stream_;
    if (io && io->n_new > DEC_CHUNK) {              // a long token block: 4-token passes over the growing cache
        WM_REQUIRE(!io->n_past_dev, "wm_decoder_step: a device step counter needs n_new == 1");
        WM_REQUIRE(io->tokens && io->positional_embedding && io->logits && io->workspace && io->present, "wm_decoder_step: null argument");
        const int L = io->n_new, B = io->batch, C = e->dims.n_text_state, V = e->dims.n_vocab;
        WM_REQUIRE(B >= 1 && io->n_past >= 0 && io->n_past + L <= e->dims.n_text_ctx, "wm_decoder_step: n_past+n_new=%d exceeds n_text_ctx=%d",
                   io->n_past + L, e->dims.n_text_ctx);
        const size_t base = carve_decoder(e, B, DEC_CHUNK, nullptr).total;
        const size_t need = base + align_up((size_t)B * DEC_CHUNK * V * sizeof(h16));
        WM_REQUIRE(io->workspace_bytes >= need, "decoder workspace too small: %zu < %zu", io->workspace_bytes, need);
        h16* stage = (h16*)((unsigned char*)io->workspace + base);
        for (int off = 0; off < L; off += DEC_CHUNK) {
            const int l = (L - off) < DEC_CHUNK ? (L - off) : DEC_CHUNK;
            wm_decoder_io sub = *io;
            sub.n_new = l; sub.n_past = io->n_past + off;
            sub.tokens = io->tokens + off; sub.tokens_ld = io->tokens_ld > 0 ? io->tokens_ld : L;
            sub.positional_embedding = (const h16*)io->positional_embedding + (size_t)off * C;
            sub.logits = stage; sub.workspace_bytes = base;
            if (off > 0) { sub.past = (const void* const*)io->present; sub.past_capacity = io->present_capacity; }   // the cache so far lives in `present`
            if (int rc = decoder_step(e, &sub, cross_group, live_groups, stream_)) return rc;
            // [B, l, V] -> rows off .. off+l of the caller's [B, L, V]
            WM_CHECK_HIP(hipMemcpy2DAsync((h16*)io->logits + (size_t)off * V, (size_t)L * V * sizeof(h16), stage, (size_t)l * V * sizeof(h16),
                                          (size_t)l * V * sizeof(h16), (size_t)B, hipMemcpyDeviceToDevice, s));
        }
        return 0;
    }
    GroupStep g;
    // (right-aligned rows: gemv_chain.hip's copy of the self-attention knows no row_start -- such a call is never `alone`)
    // (candidate groups: neither does its copy of the cross-attention know cross_group)
    if (int rc = g.init(e, io, s, !(io && (io->not_alone || io->row_start || cross_group > 1)), cross_group, live_groups)) return rc;
    return g.run(s);
}

int wm_decoder_step(const wm_engine* e, const wm_decoder_io* io, wm_stream_t stream) { return decoder_step(e, io, 0, nullptr, stream); }

// Block prefill: the whole start block in ONE pass of the launch-per-kernel sequence at M = batch * n_new rows (the Linear forms GroupStep
// picks for that M), with attn_prefill.hip's two kernels in place of the decode attention.  Every refusal comes before the first launch.
size_t wm_decoder_prefill_workspace_bytes(const wm_engine* e, int batch, int n_new) {
    if (!e || e->kind != WM_ENGINE_DECODER || batch < 1 || n_new < 1 || n_new > e->dims.n_text_ctx) return 0;
    return carve_decoder(e, batch, n_new, nullptr, 1, true).total;
}

// what wm_decoder_prefill and wm_decoder_prefill_tap refuse about the block itself; `who` is the entry a refusal names
static int check_block_call(const char* who, const wm_engine* e, const wm_prefill_io* pio) {
    WM_REQUIRE(e && e->kind == WM_ENGINE_DECODER, "%s: not a decoder engine", who);
    WM_REQUIRE(pio, "%s: null argument", who);
    const wm_decoder_io* io = &pio->io;
    const int L = io->n_new;
    WM_REQUIRE(!e->i8cross(), "%s: engines with int8 cross K/V are not supported (the block kernels read fp16 cross K/V)", who);
    WM_REQUIRE(io->batch >= 1 && L >= 1, "%s: bad batch/n_new (%d, %d)", who, io->batch, L);
    WM_REQUIRE(L <= e->dims.n_text_ctx, "%s: n_new=%d exceeds n_text_ctx=%d", who, L, e->dims.n_text_ctx);
    WM_REQUIRE(io->n_past == 0, "%s: n_past=%d: the block goes on an empty cache (n_past must be 0)", who, io->n_past);
    WM_REQUIRE(!io->n_past_dev, "%s: a device step counter (n_past_dev) is not supported", who);
    WM_REQUIRE(!io->qkv_amax, "%s: the calibration hook (qkv_amax) is not supported", who);
    WM_REQUIRE(io->present, "%s: present buffers are missing", who);
    for (int i = 0; i < e->dims.n_text_layer; ++i) {
        WM_REQUIRE(io->present[i], "%s: present[%d] is null", who, i);
        WM_REQUIRE(io->cross && io->cross[i], "%s: cross[%d] is null", who, i);
    }
    WM_REQUIRE(io->present_capacity >= L, "%s: present capacity %d < n_new = %d", who, io->present_capacity, L);
    WM_REQUIRE(pio->logits_from >= 0 && pio->logits_from < L, "%s: logits_from=%d is outside 0 .. n_new - 1 = %d", who, pio->logits_from, L - 1);
    return 0;
}

int wm_decoder_prefill(const wm_engine* e, const wm_prefill_io* pio, wm_stream_t stream_) {
    if (int rc = check_block_call("wm_decoder_prefill", e, pio)) return rc;
    hipStream_t s = (hipStream_t)stream_;
    GroupStep g;
    g.prefill = true; g.logits_from = pio->logits_from;
    if (int rc = g.init(e, &pio->io, s, false)) return rc;
    return g.run(s);
}

int wm_decoder_step_group(const wm_engine* e, const wm_decoder_group_io* gio, wm_stream_t stream) {
    WM_REQUIRE(gio, "wm_decoder_step_group: null argument");
    return decoder_step(e, &gio->io, gio->cross_group, gio->live_groups, stream);
}

// The tapped entries: wm_decoder_step / wm_decoder_prefill on the launch-per-kernel path, with the cross-attention queries of the
// listed heads written to the tape.  Behind the cq projection of a layer the sums wait in the workspace (w.part, cq_ks split-K slabs,
// or one slab from the fused forms) for the cross-attention kernel, where the tap kernel reads them too, in that kernel's order
// (align.hip).  Every refusal comes before the first launch.

// what both refuse about a wm_tap_io (e: a decoder engine); `who` is the entry a refusal names
static int check_tap(const char* who, const wm_engine* e, const wm_tap_io* tap) {
    WM_REQUIRE(tap && tap->q_tape && tap->heads && tap->n_heads >= 1, "%s: null argument", who);
    const int H = e->dims.n_text_head;
    WM_REQUIRE(H <= 64, "%s: %d heads per layer (at most 64)", who, H);
    for (int k = 0; k < tap->n_heads; ++k)
        WM_REQUIRE(tap->heads[k] >= 0 && tap->heads[k] < e->dims.n_text_layer * H && (k == 0 || tap->heads[k] > tap->heads[k - 1]),
                   "%s: heads must be strictly ascending and below n_text_layer * n_text_head (entry %d = %d)", who, k, tap->heads[k]);
    return 0;
}

// the walk over the layers with, behind pre_cross(i), the tap of the heads of layer i (tap->heads is ascending: layer by layer)
static int run_tapped(GroupStep& g, const wm_tap_io* tap, hipStream_t s) {
    const int H = g.H;
    int k = 0;
    return g.run(s, [&](int i) {
        int heads[64], slots[64], n = 0;
        for (; k < tap->n_heads && tap->heads[k] / H == i; ++k) { heads[n] = tap->heads[k] % H; slots[n] = k; ++n; }
        if (n == 0) return 0;
        const Lin& cq = g.e->dec[i].cq;
        return launch_tap_q(g.prefill ? TAP_FOURS : TAP_PAIRS, g.w.part, g.cq_ks, cq.N, (long)g.M * cq.N, cq.b, g.B, g.L, g.T,
                            (h16*)tap->q_tape, tap->n_heads, tap->capacity, heads, slots, n, s);
    });
}

int wm_decoder_step_tap(const wm_engine* e, const wm_decoder_io* io, const wm_tap_io* tap, wm_stream_t stream_) {
    const char* who = "wm_decoder_step_tap";
    WM_REQUIRE(e && e->kind == WM_ENGINE_DECODER, "%s: not a decoder engine", who);
    WM_REQUIRE(io, "%s: null argument", who);
    if (int rc = check_tap(who, e, tap)) return rc;
    WM_REQUIRE(io->n_new >= 1 && io->n_new <= DEC_CHUNK && !io->n_past_dev, "%s: n_new must be 1 .. %d, without a device step counter", who, DEC_CHUNK);
    WM_REQUIRE(!io->row_start, "%s: row_start (right-aligned rows) is not supported: word timestamps are computed without a prompt", who);
    WM_REQUIRE(io->n_past >= 0 && tap->capacity >= io->n_past + io->n_new, "%s: tape capacity %d < n_past + n_new = %d", who, tap->capacity,
               io->n_past + io->n_new);
    hipStream_t s = (hipStream_t)stream_;
    GroupStep g;
    if (int rc = g.init(e, io, s, false)) return rc;
    return run_tapped(g, tap, s);
}

int wm_decoder_prefill_tap(const wm_engine* e, const wm_prefill_io* pio, const wm_tap_io* tap, wm_stream_t stream_) {
    const char* who = "wm_decoder_prefill_tap";
    if (int rc = check_block_call(who, e, pio)) return rc;
    WM_REQUIRE(!pio->io.row_start, "%s: row_start (right-aligned rows) is not supported: the forced pass runs without a prompt", who);
    if (int rc = check_tap(who, e, tap)) return rc;
    WM_REQUIRE(tap->capacity >= pio->io.n_new, "%s: tape capacity %d < n_new = %d", who, tap->capacity, pio->io.n_new);
    hipStream_t s = (hipStream_t)stream_;
    GroupStep g;
    g.prefill = true; g.logits_from = pio->logits_from;
    if (int rc = g.init(e, &pio->io, s, false)) return rc;
    return run_tapped(g, tap, s);
}

int wm_decoder_step_multi(const wm_engine* e, int n_groups, const wm_decoder_io* const* ios,
                          const wm_stream_t* light_streams, wm_stream_t heavy_stream) {
    WM_REQUIRE(e && e->kind == WM_ENGINE_DECODER, "wm_decoder_step_multi: not a decoder engine");
    WM_REQUIRE(n_groups >= 1 && n_groups <= 8 && ios && light_streams && heavy_stream, "wm_decoder_step_multi: bad arguments");
    hipStream_t hs = (hipStream_t)heavy_stream;
    GroupStep g[8];
    for (int k = 0; k < n_groups; ++k) {
        WM_REQUIRE(light_streams[k] && light_streams[k] != heavy_stream, "wm_decoder_step_multi: group %d needs its own stream", k);
        WM_REQUIRE(!(ios[k] && ios[k]->row_start), "wm_decoder_step_multi: row_start (right-aligned rows) is not supported by the CU-partitioned schedule: use wm_decoder_step (group %d)", k);
        if (int rc = g[k].init(e, ios[k], (hipStream_t)light_streams[k], n_groups == 1 && !(ios[k] && ios[k]->not_alone))) return rc;
    }
    const int n_layer = e->dims.n_text_layer;
    for (int k = 0; k < n_groups; ++k)
        if (g[k].begin((hipStream_t)light_streams[k])) return 2;
    for (int i = 0; i < n_layer; ++i) {
        for (int k = 0; k < n_groups; ++k) {
            hipStream_t ls = (hipStream_t)light_streams[k];
            hipEvent_t q_ready = e->events.get(((size_t)k * n_layer + i) * 2), ctx_ready = e->events.get(((size_t)k * n_layer + i) * 2 + 1);
            WM_REQUIRE(q_ready && ctx_ready, "wm_decoder_step_multi: hipEventCreate failed");
            if (g[k].pre_cross(i, ls)) return 2;
            WM_CHECK_HIP(hipEventRecord(q_ready, ls));
            WM_CHECK_HIP(hipStreamWaitEvent(hs, q_ready, 0));
            if (g[k].cross(i, hs)) return 2;
            WM_CHECK_HIP(hipEventRecord(ctx_ready, hs));
            WM_CHECK_HIP(hipStreamWaitEvent(ls, ctx_ready, 0));
        }
        for (int k = 0; k < n_groups; ++k)
            if (g[k].post_cross(i, (hipStream_t)light_streams[k])) return 2;
    }
    for (int k = 0; k < n_groups; ++k)
        if (g[k].end((hipStream_t)light_streams[k])) return 2;
    return 0;
}

int wm_stream_create_cu_mask(const uint32_t* mask, int n_words, wm_stream_t* out) {
    WM_REQUIRE(mask && n_words >= 1 && out, "wm_stream_create_cu_mask: bad arguments");
    hipStream_t s = nullptr;
    WM_CHECK_HIP(hipExtStreamCreateWithCUMask(&s, (uint32_t)n_words, mask));
    *out = (wm_stream_t)s;
    return 0;
}

int wm_stream_destroy(wm_stream_t stream) {
    if (stream) WM_CHECK_HIP(hipStreamDestroy((hipStream_t)stream));
    return 0;
}

// ================================================================================================ profiling
int wm_profile_configure(int enabled, int layer_stride, int max_samples) {
    WM_REQUIRE(layer_stride >= 1 && max_samples >= 0, "wm_profile_configure: bad arguments");
    std::lock_guard<std::mutex> lock(g_prof_mu);
    Profiler& g_prof = g_prof_dev[current_device_index()];
    g_prof.enabled = false;
    for (size_t i = 0; i < g_prof.start.size(); ++i) { (void)hipEventDestroy(g_prof.start[i]); (void)hipEventDestroy(g_prof.stop[i]); }
    g_prof.start.clear(); g_prof.stop.clear(); g_prof.used = 0; g_prof.layer_stride = layer_stride;
    if (!enabled) return 0;
    g_prof.start.resize(max_samples); g_prof.stop.resize(max_samples);
    for (int i = 0; i < max_samples; ++i) {
        WM_CHECK_HIP(hipEventCreate(&g_prof.start[i]));
        WM_CHECK_HIP(hipEventCreate(&g_prof.stop[i]));
    }
    g_prof.enabled = true;
    return 0;
}

int wm_debug_timeline(void* buf, int capacity) {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    Profiler& pr = g_prof_dev[current_device_index()];
    pr.timeline = (long long*)buf;
    pr.timeline_cap = buf ? capacity : 0;
    return 0;
}

int wm_profile_read(double* total_ms, int64_t* count, int reset) {
    WM_REQUIRE(total_ms && count, "wm_profile_read: null argument");
    std::lock_guard<std::mutex> lock(g_prof_mu);
    Profiler& g_prof = g_prof_dev[current_device_index()];
    double sum = 0.0;
    for (size_t i = 0; i < g_prof.used; ++i) {
        float ms = 0.f;
        WM_CHECK_HIP(hipEventSynchronize(g_prof.stop[i]));
        WM_CHECK_HIP(hipEventElapsedTime(&ms, g_prof.start[i], g_prof.stop[i]));
        sum += ms;
    }
    *total_ms = sum; *count = (int64_t)g_prof.used;
    if (reset) g_prof.used = 0;
    return 0;
}

// ================================================================================================ greedy
static GreedyParams greedy_params(const wm_greedy_io* io) {
    GreedyParams p{};
    p.logits = (h16*)io->logits; p.ld_row = io->row_stride; p.B = io->batch; p.V = io->n_vocab;
    p.tokens = io->tokens; p.ld_tok = io->tokens_ld; p.cur_len = io->cur_len; p.sum_logprobs = io->sum_logprobs;
    p.suppress = io->suppress; p.n_suppress = io->n_suppress; p.blank = io->blank; p.n_blank = io->n_blank;
    p.sample_begin = io->sample_begin; p.eot = io->eot; p.timestamp_begin = io->timestamp_begin;
    p.max_initial_ts = io->max_initial_timestamp_index; p.apply_rules = io->apply_rules; p.n_done = io->n_done;
    p.t_dev = io->n_past_dev;
    p.done = io->done; p.row_limit = io->row_limit;
    p.temperature = io->temperature; p.seed_lo = (uint32_t)io->seed; p.seed_hi = (uint32_t)(io->seed >> 32);
    p.seed_dev = io->seed_dev; p.row0 = io->row0;
    return p;
}

int wm_greedy_step(const wm_greedy_io* io, wm_stream_t stream) {
    WM_REQUIRE(io && io->logits && io->tokens && io->sum_logprobs, "wm_greedy_step: null argument");
    WM_REQUIRE(io->temperature >= 0.f, "wm_greedy_step: negative temperature");
    return launch_greedy(greedy_params(io), (hipStream_t)stream);
}

// ================================================================================================ truncated sampling
int wm_sample_step(const wm_sample_io* io, wm_stream_t stream) {
    WM_REQUIRE(io && io->g.logits && io->g.tokens && io->g.sum_logprobs, "wm_sample_step: null argument");
    WM_REQUIRE(io->g.batch >= 1 && io->g.n_vocab >= 1, "wm_sample_step: batch %d or n_vocab %d below 1", io->g.batch, io->g.n_vocab);
    WM_REQUIRE(io->g.temperature > 0.f && std::isfinite(io->g.temperature), "wm_sample_step: temperature must be finite and > 0 (wm_greedy_step takes the arg-max)");
    WM_REQUIRE(io->top_k >= 0, "wm_sample_step: top_k %d is negative", io->top_k);
    WM_REQUIRE(io->exp2_scale > 0.f && std::isfinite(io->exp2_scale), "wm_sample_step: exp2_scale must be log2(e) / temperature, finite and > 0");
    WM_REQUIRE(io->top_p_q16 >= 1 && io->top_p_q16 <= 65536, "wm_sample_step: top_p_q16 %d outside [1, 65536]", io->top_p_q16);
    WM_REQUIRE(io->min_p_gap <= 0.f, "wm_sample_step: min_p_gap must be temperature * ln(min_p) <= 0, or -inf");
    SampleParams sp{};
    sp.g = greedy_params(&io->g);
    sp.top_k = io->top_k; sp.exp2_scale = io->exp2_scale; sp.top_p_q16 = io->top_p_q16; sp.min_p_gap = io->min_p_gap;
    sp.cut_out = io->cut_out; sp.kept_out = io->kept_out;
    return launch_sample(sp, (hipStream_t)stream);
}

// ================================================================================================ speculative decoding: verify
size_t wm_verify_workspace_bytes(int batch, int n_pos) { return verify_workspace_bytes(batch, n_pos); }

int wm_verify_step(const wm_verify_io* io, wm_stream_t stream) {
    WM_REQUIRE(io && io->g.logits && io->g.tokens && io->g.sum_logprobs && io->n_accept && io->workspace, "wm_verify_step: null argument");
    WM_REQUIRE(io->g.temperature == 0.f, "wm_verify_step: temperature must be 0 (a sampled token cannot be verified against a proposal)");
    WM_REQUIRE(!io->g.n_past_dev && !io->g.seed_dev, "wm_verify_step: n_past_dev / seed_dev must be NULL (cur_len is a host value)");
    VerifyParams vp{};
    vp.g = greedy_params(&io->g);
    vp.pos_stride = (long)io->pos_stride; vp.n_pos = io->n_pos;
    vp.n_accept = io->n_accept; vp.cand = (VerifyCand*)io->workspace;
    return launch_verify(vp, (hipStream_t)stream);
}

int wm_step_advance(int32_t* counter, wm_stream_t stream) { return launch_step_advance(counter, (hipStream_t)stream); }
int wm_step_finish(int32_t* counter, const int32_t* done, int batch, int32_t* live, wm_stream_t stream) {
    return launch_step_finish(counter, done, batch, live, (hipStream_t)stream);
}
int wm_step_finish_group(int32_t* counter, const int32_t* done, int batch, int group, int32_t* live, int32_t* live_groups, wm_stream_t stream) {
    return launch_step_finish_group(counter, done, batch, group, live, live_groups, (hipStream_t)stream);
}

// ================================================================================================ form switches
int wm_set_rows_path(int min_rows) {
    const int prev = rows_path_min_rows();
    g_rows_min.store(min_rows < 0 ? 0 : min_rows, std::memory_order_relaxed);
    return prev;
}

int wm_set_gemm_small_tiles(int tiles) {
    const int prev = get_gemm_small_tiles();
    set_gemm_small_tiles(tiles);
    return prev;
}

int wm_set_self_attn_waves(int waves) {
    self_attn_waves(1);                          // (reads the environment once)
    const int prev = g_self_waves.load(std::memory_order_relaxed);
    g_self_waves.store(waves == 1 || waves == 4 ? waves : 0, std::memory_order_relaxed);
    return prev;
}

int wm_set_small_batch_rows(int rows) {
    const int prev = small_path_max_rows();
    g_small_rows.store(rows < 0 ? 0 : (rows > GEMV_SMALL_MAX_M ? GEMV_SMALL_MAX_M : rows), std::memory_order_relaxed);
    return prev;
}

int wm_set_decode_chain(int on) {
    const int prev = g_decode_chain.load(std::memory_order_relaxed);
    g_decode_chain.store(on < 0 ? DECODE_CHAIN_DEFAULT : (on > 2 ? 2 : on), std::memory_order_relaxed);
    for (ChainDev& cd : g_chain_dev) {               // an explicit choice re-arms devices that had let a chain down
        std::lock_guard<std::mutex> lk(cd.mu);
        if (cd.declined) { cd.declined = false; cd.reason.clear(); }
    }
    return prev;
}

int wm_decode_chain_error(int* out) {
    WM_REQUIRE(out, "wm_decode_chain_error: null argument");
    ChainDev& cd = chain_dev_slot(current_device_index());
    // No synchronisation here (round 5: a device-wide one also waited for whatever ran beside the loop -- the next batch's encoder on its
    // own stream -- and cost the pipelined batch-1 job 3.5 %): the word is in host memory and current for every step whose results the
    // caller has already waited for.
    const unsigned v = chain_err_peek(cd);
    *out = (int)v;
    if (v) {
        std::lock_guard<std::mutex> lk(cd.mu);
        __atomic_store_n(cd.err_host, 0u, __ATOMIC_RELAXED);
        cd.declined = true;
        cd.reason = "a one-launch decode step gave up waiting for its workgroups (they were not resident together)";
    }
    return 0;
}

int wm_decode_chain_status(wm_chain_status* out) {
    WM_REQUIRE(out, "wm_decode_chain_status: null argument");
    ChainDev& cd = chain_dev_slot(current_device_index());
    std::lock_guard<std::mutex> lk(cd.mu);
    memset(out, 0, sizeof(*out));
    out->mode = g_decode_chain.load(std::memory_order_relaxed);
    out->launches = cd.launches.load(std::memory_order_relaxed);
    out->declined_calls = cd.declined_calls.load(std::memory_order_relaxed);
    out->declined = cd.declined ? 1 : 0;
    out->error_pending = chain_err_peek(cd) ? 1 : 0;
    snprintf(out->reason, sizeof(out->reason), "%s", cd.reason.c_str());
    snprintf(out->footprint, sizeof(out->footprint), "%s", cd.footprint.c_str());
    return 0;
}

int wm_set_cross_v_skip(int on) {
    const int prev = g_cross_v_skip.load(std::memory_order_relaxed);
    g_cross_v_skip.store(on < 0 ? CROSS_V_SKIP_DEFAULT : (on ? 1 : 0), std::memory_order_relaxed);
    return prev;
}

}  // extern "C"
