// What the files that hold the engines and the C ABI share -- engine.hip (blob, encoder, cross K/V), decoder.hip (decoder step) and
// api_kernels.hip (kernel-level entries): the resident form of a blob's tensors, the engine object and the workspace carver.
// No kernel file includes this.
#pragma once
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/whisper_mi355.h"
#include "common.h"
#include "kernels.h"

namespace wm {

struct Tensor { const unsigned char* ptr = nullptr; uint32_t dtype = 0; uint64_t shape[4] = {0, 0, 0, 0}; uint64_t nbytes = 0; };

struct Lin {                  // one Linear: weight (row-major or tile-linear), optional scale, bias
    const void* w = nullptr; const h16* s = nullptr; const h16* b = nullptr;
    int N = 0, K = 0, n_blocks = 0;
    int wcode = 0;            // weight encoding for the skinny GEMM: 0 fp16, 1 int8, 4 packed int4
};
struct EncLayer { const h16 *ln1g, *ln1b, *ln2g, *ln2b; Lin qkv, out, mlp1, mlp2; };
struct DecLayer {
    const h16 *ln1g, *ln1b, *lncg, *lncb, *ln2g, *ln2b;
    Lin qkv, out, cq, cout, mlp1, mlp2;
    float kv_scale = 1.f;
    float cross_scale = 0.f;      // > 0: int8 cross K/V (WM_FLAG_INT8_CROSS_KV)
};

// events that order a group's light stream against the shared heavy stream (wm_decoder_step_multi):
// [group][layer][0: q ready, 1: ctx ready].  Owned by the engine, i.e. created on the engine's device; the mutex
// makes concurrent calls on one engine (threads driving different streams) safe.
struct EventPool {
    std::mutex mu;
    std::vector<hipEvent_t> ev;
    hipEvent_t get(size_t idx) {
        std::lock_guard<std::mutex> lock(mu);
        while (ev.size() <= idx) {
            hipEvent_t x = nullptr;
            if (hipEventCreateWithFlags(&x, hipEventDisableTiming) != hipSuccess) return nullptr;
            ev.push_back(x);
        }
        return ev[idx];
    }
    ~EventPool() { for (hipEvent_t x : ev) (void)hipEventDestroy(x); }
};

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

struct Carver {            // bump allocator over the caller's workspace
    unsigned char* base; size_t cap; size_t off = 0;
    template <typename T> T* take(size_t n) {
        off = align_up(off);
        T* p = (T*)(base + off);
        off += n * sizeof(T);
        return p;
    }
};

// the decoder's switches (decoder.hip) that the kernel-level entries follow too
int self_attn_waves(int rows);      // waves per (b, h) of the decode self-attention for a group of `rows` rows
int cross_v_skip();                 // exact V-row skipping of the decode cross-attention: 1 on, 0 off

}  // namespace wm
using wm::h16;

struct wm_engine {
    int kind = 0; uint32_t flags = 0; wm_dims dims{}; int device = 0;
    mutable wm::EventPool events;
    unsigned char* dev = nullptr; size_t dev_bytes = 0;
    std::map<std::string, wm::Tensor> t;
    std::map<std::string, float> scalars;      // host copies of 4-byte fp32 tensors (kv scales)
    // encoder
    wm::Lin conv1, conv2; const h16* enc_pos = nullptr; const h16 *lnpg = nullptr, *lnpb = nullptr;
    std::vector<wm::EncLayer> enc;
    // cross
    std::vector<wm::Lin> ckv; std::vector<float> ckv_scale;
    // decoder
    const void* emb_t = nullptr; int emb_blocks = 0; const h16 *lnfg = nullptr, *lnfb = nullptr;
    std::vector<wm::DecLayer> dec;
    // the one-row chain's stage descriptors (gemv_chain.hip), six per layer in chain order: out, cq | cout, mlp1, mlp2, qkv of the
    // next layer -- on the device (the kernels read them there) and on the host (the launcher's checks)
    wm::ChainStage* chain_dev = nullptr; std::vector<wm::ChainStage> chain_host;      // [qkv of layer 0] + 6 per layer (gemv_chain.hip)
    wm::ChainLayerStatic* chain_lstat = nullptr;                                       // per layer: biases of the attention stages, cache scale
    // what the library knows about the chain state it keeps in a caller's workspace (granules, call counter, pointer table), keyed by the
    // table's address: the workspace_id under which the state was initialised, and the per-layer pointers last written to the table.
    // Dies with the engine; capped (a caller that hands a new workspace to every call must not grow it without bound).
    struct ChainWsSeen { uint64_t id = 0; std::vector<wm::ChainLayerIo> tab; };
    mutable std::mutex chain_io_mu;
    mutable std::unordered_map<const void*, ChainWsSeen> chain_io_seen;
    bool w8() const { return flags & WM_FLAG_WEIGHT_ONLY_INT8; }
    bool i8kv() const { return flags & WM_FLAG_INT8_KV; }
    bool i8cross() const { return flags & WM_FLAG_INT8_CROSS_KV; }
    int gelu() const { return (flags & WM_FLAG_GELU_TANH) ? 2 : 1; }
};
