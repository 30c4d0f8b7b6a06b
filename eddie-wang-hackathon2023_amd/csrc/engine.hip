// Engine objects and the C ABI (include/whisper_mi355.h): blob parsing, weight residency and the
// kernel sequences of the three engines of the reference's Whisper example:
//   encoder        WhisperEncoder.forward   R/tensorrt_llm/models/whisper/model.py:149-172
//   cross K/V      CrossAttn_KV.forward     model.py:469-540
//   decoder step   WhisperDecoder.forward   model.py:241-299, block :61-122   (decoder.hip)
// Everything is enqueued on the caller's stream into caller-owned buffers; nothing allocates or
// synchronises here (the contract of Session.run, session.py:148-178).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "decode_math.h"
#include "engine_internal.h"

namespace wm {

static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
int post_launch_check(hipStream_t s, const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error("launch of %s failed: %s", what, hipGetErrorString(e)); return 2; }
    static int sync_check = -1;
    if (sync_check < 0) { const char* v = getenv("WM_SYNC_CHECK"); sync_check = (v && v[0] == '1') ? 1 : 0; }
    if (sync_check) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;       // a synchronise would invalidate a capture in progress
        if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return 0;
        e = hipStreamSynchronize(s);
        if (e != hipSuccess) { set_error("kernel %s faulted: %s", what, hipGetErrorString(e)); return 2; }
    }
    return 0;
}

// ---- lab knobs (common.h) ------------------------------------------------------------------------
namespace {
std::mutex g_lab_mu;
std::string g_lab_honoured;                 // "NAME=value;..." of every knob honoured so far
std::map<std::string, int> g_lab_seen;      // 1: honoured and logged, 2: ignored and warned
}  // namespace
const char* lab_env_str(const char* name) {
    const char* v = getenv(name);
    if (!v) return nullptr;
    const char* lab = getenv("WM_LAB");
    const bool on = lab && lab[0] == '1';
    std::lock_guard<std::mutex> lk(g_lab_mu);
    int& seen = g_lab_seen[name];
    if (on && seen != 1) {
        fprintf(stderr, "whisper_mi355: lab knob %s=%s honoured (WM_LAB=1): results or timings may differ from the product's\n", name, v);
        g_lab_honoured += std::string(name) + "=" + v + ";";
        seen = 1;
    } else if (!on && seen == 0) {
        fprintf(stderr, "whisper_mi355: %s=%s is set but WM_LAB is not 1: ignored (lab knobs are for A/B runs only)\n", name, v);
        seen = 2;
    }
    return on ? v : nullptr;
}
int lab_env_int(const char* name, int dflt) {
    const char* v = lab_env_str(name);
    return v ? atoi(v) : dflt;
}

// ---- blob format (written by weight.py: write_engine_blob) ---------------------------------------
#pragma pack(push, 1)
struct BlobHeader {
    char magic[8];            // "WM355ENG"
    uint32_t version;         // 1
    uint32_t kind;            // WM_ENGINE_*
    uint32_t n_tensors;
    uint32_t flags;           // WM_FLAG_*
    int32_t dims[10];         // wm_dims order
    uint64_t data_offset;     // from blob start, 256-byte aligned
    uint64_t data_bytes;
};
struct BlobTensor {
    char name[64];
    uint32_t dtype;           // 0 f16, 1 i8, 2 f32, 3 i32, 4 packed int4 (two biased nibbles per byte)
    uint32_t ndim;
    uint64_t shape[4];
    uint64_t offset;          // from data_offset, 256-byte aligned
    uint64_t nbytes;
};
#pragma pack(pop)

}  // namespace wm

using namespace wm;

namespace {

int find(const wm_engine* e, const std::string& name, Tensor* out, bool required = true) {
    auto it = e->t.find(name);
    if (it == e->t.end()) {
        if (required) { set_error("engine blob has no tensor '%s'", name.c_str()); return 1; }
        *out = Tensor{};
        return 0;
    }
    *out = it->second;
    return 0;
}

// weight `base`.w (+ .s when weight-only) + optional `base`.b
int get_lin(const wm_engine* e, const std::string& base, bool tiled, bool quantisable, bool need_bias, Lin* l) {
    Tensor w, s, b;
    if (find(e, base + (tiled ? ".t" : ".w"), &w)) return 1;
    l->w = w.ptr;
    // row-major (non-tiled) matrices belong to the M >> 16 stages: a weight-only blob's int8 copies of them stay int8 at
    // rest (round 3) and are expanded per use into the caller's workspace (big())
    const bool q = quantisable && e->w8();
    const bool packed4 = w.dtype == 4;
    if ((w.dtype == 1 || packed4) != q || (packed4 && !tiled)) {
        set_error("tensor %s: dtype does not match the engine's weight-only flag", base.c_str());
        return 1;
    }
    l->wcode = packed4 ? 4 : (q ? 1 : 0);
    if (tiled) {           // shape = [n_blocks, k_tiles, 64, 16 bytes]
        l->n_blocks = (int)w.shape[0];
        l->N = l->n_blocks * 16;
        l->K = (int)w.shape[1] * (packed4 ? 128 : (q ? 64 : 32));
    } else {
        l->N = (int)w.shape[0]; l->K = (int)w.shape[1];
    }
    if (q) { if (find(e, base + ".s", &s)) return 1; l->s = (const h16*)s.ptr; }
    if (find(e, base + ".b", &b, need_bias)) return 1;
    l->b = (const h16*)b.ptr;
    return 0;
}

int get_vec(const wm_engine* e, const std::string& name, const h16** out) {
    Tensor t;
    if (find(e, name, &t)) return 1;
    *out = (const h16*)t.ptr;
    return 0;
}

int resolve(wm_engine* e) {
    const wm_dims& d = e->dims;
    char buf[96];
    if (e->kind == WM_ENGINE_ENCODER) {
        if (get_lin(e, "conv1", false, false, true, &e->conv1)) return 1;
        if (get_lin(e, "conv2", false, false, true, &e->conv2)) return 1;
        if (get_vec(e, "pos", &e->enc_pos)) return 1;
        if (get_vec(e, "ln_post.g", &e->lnpg) || get_vec(e, "ln_post.b", &e->lnpb)) return 1;
        e->enc.resize(d.n_audio_layer);
        for (int i = 0; i < d.n_audio_layer; ++i) {
            EncLayer& L = e->enc[i];
            snprintf(buf, sizeof(buf), "blocks.%d.", i);
            const std::string p(buf);
            if (get_vec(e, p + "attn_ln.g", &L.ln1g) || get_vec(e, p + "attn_ln.b", &L.ln1b) ||
                get_vec(e, p + "mlp_ln.g", &L.ln2g) || get_vec(e, p + "mlp_ln.b", &L.ln2b)) return 1;
            if (get_lin(e, p + "qkv", false, true, true, &L.qkv) || get_lin(e, p + "out", false, true, true, &L.out) ||
                get_lin(e, p + "mlp1", false, true, true, &L.mlp1) || get_lin(e, p + "mlp2", false, true, true, &L.mlp2)) return 1;
        }
    } else if (e->kind == WM_ENGINE_CROSS_KV) {
        e->ckv.resize(d.n_text_layer);
        for (int i = 0; i < d.n_text_layer; ++i) {
            snprintf(buf, sizeof(buf), "blocks.%d.kv", i);
            if (get_lin(e, buf, false, true, true, &e->ckv[i])) return 1;
            if (e->i8cross()) {
                snprintf(buf, sizeof(buf), "blocks.%d.cross_kv_scale", i);
                auto it = e->scalars.find(buf);
                if (it == e->scalars.end() || !(it->second > 0.f)) { set_error("int8 cross-K/V engine lacks a positive %s", buf); return 1; }
                e->ckv_scale.push_back(it->second);
            }
        }
    } else if (e->kind == WM_ENGINE_DECODER) {
        Tensor emb;
        if (find(e, "emb.t", &emb)) return 1;
        e->emb_t = emb.ptr; e->emb_blocks = (int)emb.shape[0];
        if (get_vec(e, "ln.g", &e->lnfg) || get_vec(e, "ln.b", &e->lnfb)) return 1;
        e->dec.resize(d.n_text_layer);
        for (int i = 0; i < d.n_text_layer; ++i) {
            DecLayer& L = e->dec[i];
            snprintf(buf, sizeof(buf), "blocks.%d.", i);
            const std::string p(buf);
            if (get_vec(e, p + "attn_ln.g", &L.ln1g) || get_vec(e, p + "attn_ln.b", &L.ln1b) ||
                get_vec(e, p + "cross_ln.g", &L.lncg) || get_vec(e, p + "cross_ln.b", &L.lncb) ||
                get_vec(e, p + "mlp_ln.g", &L.ln2g) || get_vec(e, p + "mlp_ln.b", &L.ln2b)) return 1;
            if (get_lin(e, p + "qkv", true, true, true, &L.qkv) || get_lin(e, p + "out", true, true, true, &L.out) ||
                get_lin(e, p + "cq", true, true, true, &L.cq) || get_lin(e, p + "cout", true, true, true, &L.cout) ||
                get_lin(e, p + "mlp1", true, true, true, &L.mlp1) || get_lin(e, p + "mlp2", true, true, true, &L.mlp2)) return 1;
            if (e->i8kv()) {
                auto it = e->scalars.find(p + "kv_scale");
                if (it == e->scalars.end()) { set_error("int8-KV engine lacks %skv_scale", p.c_str()); return 1; }
                L.kv_scale = it->second;
                if (!(L.kv_scale > 0.f)) { set_error("%skv_scale must be positive", p.c_str()); return 1; }
            }
            if (e->i8cross()) {
                auto it = e->scalars.find(p + "cross_kv_scale");
                if (it == e->scalars.end() || !(it->second > 0.f)) { set_error("int8 cross-K/V engine lacks a positive %scross_kv_scale", p.c_str()); return 1; }
                L.cross_scale = it->second;
            }
        }
    } else {
        set_error("unknown engine kind %d", e->kind);
        return 1;
    }
    return 0;
}

// Device residency of a blob's tensors: one allocation, one copy, for every engine kind.  Weight-only ENCODER / CROSS-K/V
// engines keep their row-major int8 matrices and scales as stored (round 3; rounds 1-2 expanded them to fp16 at load, which
// left a weight-only engine with the memory of an fp16 one: 3.09 -> 2.35 GB where the reference's chart saves 1.7 GB,
// /root/reference/README.md:178-180).  Their GEMMs are MFMA-bound (M = 1500 x batch) and multiply fp16(fp16(q) * scale) -- the
// reference kernels' per-element dequantisation (fpA_intB_gemm_template.h:47-140 does it in registers) -- so each matrix is
// expanded right before its GEMM into a scratch block of the caller's workspace (big(): one pass over 1.6-6.6 MB, ~0.1 % of an
// encoder pass, the expansion staying in L2 / Infinity Cache for the GEMM behind it): same values, same GEMM, bit-identical.
int upload(wm_engine* e, const BlobHeader* h, const BlobTensor* tt, const unsigned char* data) {
    auto name_of = [&](uint32_t i) { char nm[65]; memcpy(nm, tt[i].name, 64); nm[64] = 0; return std::string(nm); };
    WM_CHECK_HIP(hipMalloc((void**)&e->dev, h->data_bytes ? h->data_bytes : 256));
    WM_CHECK_HIP(hipMemcpy(e->dev, data, h->data_bytes, hipMemcpyHostToDevice));
    e->dev_bytes = h->data_bytes;
    for (uint32_t i = 0; i < h->n_tensors; ++i) {
        Tensor t;
        t.ptr = e->dev + tt[i].offset; t.dtype = tt[i].dtype; t.nbytes = tt[i].nbytes;
        memcpy(t.shape, tt[i].shape, sizeof(t.shape));
        e->t[name_of(i)] = t;
    }
    return 0;
}

// ---- encoder -------------------------------------------------------------------------------------
struct EncWs { h16 *melT, *c1, *x, *xn, *qkv, *ctx, *hid, *wq; size_t total; };
EncWs carve_encoder(const wm_engine* e, int B, void* ws) {
    const wm_dims& d = e->dims;
    const size_t T = d.n_audio_ctx, Tin = 2 * T, C = d.n_audio_state;
    Carver c{(unsigned char*)ws, 0};
    EncWs w;
    w.melT = c.take<h16>(B * (Tin + 2) * d.n_mels + 512);
    w.c1 = c.take<h16>(B * (Tin + 2) * C + 512);
    w.x = c.take<h16>(B * T * C);
    w.xn = c.take<h16>(B * T * C);
    w.qkv = c.take<h16>(B * T * 3 * C);
    w.ctx = c.take<h16>(B * T * C);
    w.hid = c.take<h16>(B * T * 4 * C);
    w.wq = e->w8() ? c.take<h16>(4 * C * C) : nullptr;        // fp16 expansion of the int8 matrix in use (the widest: 4C x C)
    w.total = align_up(c.off);
    return w;
}

int big(const Lin& l, const wm_engine* e, const h16* A, int lda, int M, h16* Cout, int ldc, int act,
        const h16* residual, int ldr, hipStream_t s, GemmBigParams* custom = nullptr, int max_wgs = 0, h16* wq = nullptr) {
    GemmBigParams p{};
    if (custom) p = *custom;
    const void* W = l.w;
    if (l.s) {             // int8 at rest: fp16(fp16(q) * scale) into the scratch block, then the fp16 MFMA GEMM
        WM_REQUIRE(wq, "big GEMM: int8 weights need a scratch block for their expansion");
        if (launch_dequant_w8((const int8_t*)l.w, l.s, wq, l.N, l.K, s)) return 2;
        W = wq;
    }
    p.A = A; p.lda = lda; p.M = M; p.K = l.K; p.W = W; p.N = l.N;
    p.bias = l.b; p.C = Cout; p.ldc = ldc; p.act = act;
    if (!custom) { p.residual = residual; p.ldr = ldr; }
    p.max_wgs = max_wgs;
    return launch_gemm_f16(p, s);
}

}  // namespace

extern "C" {

int wm_version(void) { return WM_ABI_VERSION; }
const char* wm_last_error(void) { return g_err; }
int wm_device_count(int* out) {
    WM_CHECK_HIP(hipGetDeviceCount(out));
    return 0;
}

int wm_engine_create(const void* blob, size_t nbytes, int device, wm_engine** out) {
    WM_REQUIRE(blob && out, "wm_engine_create: null argument");
    WM_REQUIRE(nbytes >= sizeof(BlobHeader), "engine blob too small (%zu bytes)", nbytes);
    const BlobHeader* h = (const BlobHeader*)blob;
    WM_REQUIRE(memcmp(h->magic, "WM355ENG", 8) == 0, "not a whisper_mi355 engine blob (bad magic)");
    WM_REQUIRE(h->version == 1, "unsupported engine blob version %u", h->version);
    WM_REQUIRE(sizeof(BlobHeader) + (size_t)h->n_tensors * sizeof(BlobTensor) <= h->data_offset &&
                   h->data_offset + h->data_bytes <= nbytes, "engine blob is truncated");
    wm_engine* e = new wm_engine();
    e->kind = (int)h->kind; e->flags = h->flags; e->device = device;
    memcpy(&e->dims, h->dims, sizeof(wm_dims));
    const BlobTensor* tt = (const BlobTensor*)((const unsigned char*)blob + sizeof(BlobHeader));
    for (uint32_t i = 0; i < h->n_tensors; ++i)
        if (tt[i].offset + tt[i].nbytes > h->data_bytes) {
            set_error("tensor %.64s exceeds the blob", tt[i].name);
            delete e; return 1;
        }
    hipError_t err = hipSetDevice(device);
    if (err != hipSuccess) { set_error("wm_engine_create: device %d: %s", device, hipGetErrorString(err)); delete e; return 2; }
    if (int rc = upload(e, h, tt, (const unsigned char*)blob + h->data_offset)) {
        if (e->dev) (void)hipFree(e->dev);
        delete e;
        return rc;
    }
    for (uint32_t i = 0; i < h->n_tensors; ++i)
        if (tt[i].dtype == 2 && tt[i].nbytes == 4) {
            char nm[65]; memcpy(nm, tt[i].name, 64); nm[64] = 0;
            float v;
            memcpy(&v, (const unsigned char*)blob + h->data_offset + tt[i].offset, 4);
            e->scalars[nm] = v;
        }
    if (resolve(e)) { (void)hipFree(e->dev); delete e; return 1; }
    if (e->kind == WM_ENGINE_DECODER && !e->dec.empty()) {
        const int n = (int)e->dec.size();
        e->chain_host.resize((size_t)6 * n + 1);
        auto fill = [](wm::ChainStage& st, const Lin& l, const h16* g, const h16* b, int mode) {
            st.Wt = l.w; st.scale = l.s; st.bias = l.b; st.ln_g = g; st.ln_b = b; st.K = l.K; st.n_blocks = l.n_blocks; st.mode = mode; st.pad_ = 0;
        };
        for (int i = 0; i < n; ++i) {
            const DecLayer& L = e->dec[i];
            wm::ChainStage* st = &e->chain_host[(size_t)6 * i + 1];
            fill(st[0], L.out, nullptr, nullptr, 2);
            fill(st[1], L.cq, L.lncg, L.lncb, 0);
            fill(st[2], L.cout, nullptr, nullptr, 2);
            fill(st[3], L.mlp1, L.ln2g, L.ln2b, 1);
            fill(st[4], L.mlp2, nullptr, nullptr, 2);
            if (i + 1 < n) fill(st[5], e->dec[i + 1].qkv, e->dec[i + 1].ln1g, e->dec[i + 1].ln1b, 0);
            else st[5] = wm::ChainStage{};
        }
        fill(e->chain_host[0], e->dec[0].qkv, e->dec[0].ln1g, e->dec[0].ln1b, 0);
        std::vector<wm::ChainLayerStatic> lstat((size_t)n);
        for (int i = 0; i < n; ++i) lstat[i] = wm::ChainLayerStatic{e->dec[i].qkv.b, e->dec[i].cq.b, e->dec[i].kv_scale, 0};
        const size_t bytes = e->chain_host.size() * sizeof(wm::ChainStage), lbytes = lstat.size() * sizeof(wm::ChainLayerStatic);
        if (hipMalloc((void**)&e->chain_dev, bytes) != hipSuccess || hipMalloc((void**)&e->chain_lstat, lbytes) != hipSuccess ||
            hipMemcpy(e->chain_dev, e->chain_host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(e->chain_lstat, lstat.data(), lbytes, hipMemcpyHostToDevice) != hipSuccess) {
            set_error("wm_engine_create: the decode chain's descriptor tables could not be placed on the device");
            if (e->chain_dev) (void)hipFree(e->chain_dev);
            if (e->chain_lstat) (void)hipFree(e->chain_lstat);
            (void)hipFree(e->dev); delete e; return 2;
        }
    }
    *out = e;
    return 0;
}

void wm_engine_destroy(wm_engine* e) {
    if (!e) return;
    if (e->dev) { (void)hipSetDevice(e->device); (void)hipFree(e->dev); }
    if (e->chain_dev) (void)hipFree(e->chain_dev);
    if (e->chain_lstat) (void)hipFree(e->chain_lstat);
    delete e;
}

int wm_engine_info(const wm_engine* e, int32_t* kind, uint32_t* flags, wm_dims* dims) {
    WM_REQUIRE(e, "wm_engine_info: null engine");
    if (kind) *kind = e->kind;
    if (flags) *flags = e->flags;
    if (dims) *dims = e->dims;
    return 0;
}
size_t wm_engine_weight_bytes(const wm_engine* e) { return e ? e->dev_bytes : 0; }

// ================================================================================================ encoder
size_t wm_encoder_workspace_bytes(const wm_engine* e, int batch) {
    if (!e || e->kind != WM_ENGINE_ENCODER || batch < 1) return 0;
    return carve_encoder(e, batch, nullptr).total;
}

int wm_encoder_forward(const wm_engine* e, const void* mel, int B, void* out, void* workspace,
                       size_t workspace_bytes, wm_stream_t stream_) {
    return wm_encoder_forward_shared(e, mel, B, out, workspace, workspace_bytes, 0, stream_);
}

int wm_encoder_forward_shared(const wm_engine* e, const void* mel, int B, void* out, void* workspace,
                              size_t workspace_bytes, int cu_budget, wm_stream_t stream_) {
    return wm_encoder_forward_range(e, mel, B, out, workspace, workspace_bytes, cu_budget, 0, e ? e->dims.n_audio_layer : 0, stream_);
}

// Layers [layer_begin, layer_end) of the encoder pass: the convolutions belong to a range that starts at layer 0, the final LayerNorm
// (which writes `out`) to one that ends at n_audio_layer; between the calls of one pass the residual stream lives in the workspace.
int wm_encoder_forward_range(const wm_engine* e, const void* mel, int B, void* out, void* workspace,
                             size_t workspace_bytes, int cu_budget, int layer_begin, int layer_end, wm_stream_t stream_) {
    WM_REQUIRE(e && e->kind == WM_ENGINE_ENCODER, "wm_encoder_forward: not an encoder engine");
    WM_REQUIRE(mel && out && workspace && B >= 1, "wm_encoder_forward: null argument or empty batch");
    WM_REQUIRE(cu_budget >= 0, "wm_encoder_forward_shared: cu_budget=%d", cu_budget);
    hipStream_t s = (hipStream_t)stream_;
    const wm_dims& d = e->dims;
    WM_REQUIRE(layer_begin >= 0 && layer_begin <= layer_end && layer_end <= d.n_audio_layer, "wm_encoder_forward_range: layers [%d, %d) of %d",
               layer_begin, layer_end, d.n_audio_layer);
    const int T = d.n_audio_ctx, Tin = 2 * T, C = d.n_audio_state, H = d.n_audio_head, M = B * T;
    WM_REQUIRE(C == H * 64, "head size must be 64 (n_state %d, heads %d)", C, H);
    EncWs w = carve_encoder(e, B, workspace);
    WM_REQUIRE(workspace_bytes >= w.total, "encoder workspace too small: %zu < %zu", workspace_bytes, w.total);

    if (layer_begin == 0) {
        // mel -> token-major, zero padded; slack after the last row is read by the K=256 view (x 0 weights)
        WM_CHECK_HIP(hipMemsetAsync(w.melT + (size_t)B * (Tin + 2) * d.n_mels, 0, 512 * sizeof(h16), s));
        if (launch_mel_transpose_pad((const h16*)mel, B, d.n_mels, Tin, w.melT, s)) return 2;
        // conv1 (k3 s1 p1) + GELU as a GEMM over a strided view: row t = padded rows t, t+1, t+2
        {
            GemmBigParams p{};
            p.a_rows = Tin; p.a_bstride = (long)(Tin + 2) * d.n_mels;
            p.c_rows = Tin; p.c_bstride = (long)(Tin + 2) * C;
            WM_REQUIRE(e->conv1.K >= 3 * d.n_mels, "conv1 weight K=%d < 3*n_mels", e->conv1.K);
            if (big(e->conv1, e, w.melT, d.n_mels, B * Tin, w.c1 + C, C, e->gelu(), nullptr, 0, s, &p, cu_budget)) return 2;
            if (launch_zero_pad_rows(w.c1, B, Tin + 2, C, s)) return 2;
        }
        // conv2 (k3 s2 p1) + GELU + positional embedding: row t = padded rows 2t, 2t+1, 2t+2
        {
            GemmBigParams p{};
            p.a_rows = T; p.a_bstride = (long)(Tin + 2) * C;
            p.residual = e->enc_pos; p.ldr = C; p.res_mod = T;
            if (big(e->conv2, e, w.c1, 2 * C, M, w.x, C, e->gelu(), nullptr, 0, s, &p, cu_budget)) return 2;
        }
    }
    for (int i = layer_begin; i < layer_end; ++i) {
        const EncLayer& L = e->enc[i];
        if (launch_layernorm(w.x, C, M, C, L.ln1g, L.ln1b, w.xn, C, s)) return 2;
        {
            GemmBigParams p{};
            p.colscale_n = 2 * C; p.colscale = ATTN_SCALE;
            if (big(L.qkv, e, w.xn, C, M, w.qkv, 3 * C, 0, nullptr, 0, s, &p, cu_budget, w.wq)) return 2;
        }
        AttnEncParams ap{w.qkv, 3 * C, B, T, H, w.ctx, C, 2 * cu_budget};      // two workgroups fill a CU's registers
        if (launch_attn_encoder(ap, s)) return 2;
        if (big(L.out, e, w.ctx, C, M, w.x, C, 0, w.x, C, s, nullptr, cu_budget, w.wq)) return 2;
        if (launch_layernorm(w.x, C, M, C, L.ln2g, L.ln2b, w.xn, C, s)) return 2;
        if (big(L.mlp1, e, w.xn, C, M, w.hid, 4 * C, e->gelu(), nullptr, 0, s, nullptr, cu_budget, w.wq)) return 2;
        if (big(L.mlp2, e, w.hid, 4 * C, M, w.x, C, 0, w.x, C, s, nullptr, cu_budget, w.wq)) return 2;
    }
    if (layer_end == d.n_audio_layer)
        if (launch_layernorm(w.x, C, M, C, e->lnpg, e->lnpb, (h16*)out, C, s)) return 2;
    return 0;
}

// ================================================================================================ cross K/V
size_t wm_cross_kv_workspace_bytes(const wm_engine* e, int batch) {
    (void)batch;
    if (!e || e->kind != WM_ENGINE_CROSS_KV) return 0;
    size_t widest = 0;                                       // fp16 expansion of one layer's int8 [2C][C] matrix
    for (const Lin& l : e->ckv) if (l.s) widest = widest > (size_t)l.N * l.K ? widest : (size_t)l.N * l.K;
    return align_up(256 + widest * sizeof(h16));
}

int wm_cross_kv(const wm_engine* e, const void* xa, int B, void* const* out_layers, void* workspace,
                size_t workspace_bytes, wm_stream_t stream_) {
    WM_REQUIRE(e && e->kind == WM_ENGINE_CROSS_KV, "wm_cross_kv: not a cross-attention K/V engine");
    WM_REQUIRE(workspace_bytes >= wm_cross_kv_workspace_bytes(e, B) && (workspace || !e->w8()), "wm_cross_kv: workspace too small: %zu < %zu",
               workspace_bytes, wm_cross_kv_workspace_bytes(e, B));
    WM_REQUIRE(xa && out_layers && B >= 1, "wm_cross_kv: null argument or empty batch");
    hipStream_t s = (hipStream_t)stream_;
    const wm_dims& d = e->dims;
    const int T = d.n_audio_ctx, C = d.n_text_state, H = d.n_text_head;
    for (int i = 0; i < d.n_text_layer; ++i) {
        WM_REQUIRE(out_layers[i], "wm_cross_kv: output %d is null", i);
        GemmBigParams p{};
        p.out_mode = 1; p.hs_T = T; p.hs_H = H; p.hs_kv = -1;
        if (e->i8cross()) p.q8_inv_scale = 1.0f / e->ckv_scale[i];     // out_layers[i] is int8 [B,2,H,T,64]
        if (big(e->ckv[i], e, (const h16*)xa, C, B * T, (h16*)out_layers[i], 0, 0, nullptr, 0, s, &p, 0, (h16*)workspace)) return 2;
    }
    return 0;
}

int wm_lab_knobs(char* buf, size_t cap) {
    std::lock_guard<std::mutex> lk(g_lab_mu);
    if (buf && cap > 0) { strncpy(buf, g_lab_honoured.c_str(), cap - 1); buf[cap - 1] = 0; }
    return (int)g_lab_honoured.size();
}
}  // extern "C"
