// The kernel-level entries of the C ABI (include/whisper_mi355.h): single launches with the engines' own parameter blocks, for the tests,
// the benchmarks of one kernel and the labs.  No engine is involved; the decoder's switches are followed where an engine would follow them.
#include "engine_internal.h"

using namespace wm;

extern "C" {

// ================================================================================================ kernel-level
int wm_gemm(const void* A, int lda, int M, int K, const void* W, int N, int w8, const void* scale,
            const void* bias, const void* residual, int ldr, int act, void* C, int ldc,
            void* workspace, size_t workspace_bytes, wm_stream_t stream) {
    GemmBigParams p{};
    p.A = (const h16*)A; p.lda = lda; p.M = M; p.K = K; p.W = W; p.N = N;
    p.bias = (const h16*)bias; p.C = (h16*)C; p.ldc = ldc;
    p.residual = (const h16*)residual; p.ldr = ldr; p.act = act;
    if (w8) {
        // exactly what the engines do with a weight-only matrix of an M >> 16 stage (expand_lin): one expansion to
        // fp16(fp16(q) * scale), then the fp16 MFMA GEMM -- here into the caller's workspace, per call
        WM_REQUIRE(scale && workspace, "wm_gemm: int8 weights need their scales and a workspace for the fp16 expansion");
        WM_REQUIRE(workspace_bytes >= (size_t)N * K * sizeof(h16), "wm_gemm: workspace too small: %zu < %zu", workspace_bytes, (size_t)N * K * sizeof(h16));
        if (launch_dequant_w8((const int8_t*)W, (const h16*)scale, (h16*)workspace, N, K, (hipStream_t)stream)) return 2;
        p.W = workspace;
    }
    return launch_gemm_f16(p, (hipStream_t)stream);
}

int wm_conv1d_gelu(const void* x_pad, int B, int T_in, int C_in, const void* W, int K, const void* bias, int C_out,
                   int stride, int gelu, void* out, wm_stream_t stream) {
    WM_REQUIRE(x_pad && W && out && B >= 1 && T_in >= 1, "wm_conv1d_gelu: null argument or empty input");
    WM_REQUIRE(stride == 1 || stride == 2, "wm_conv1d_gelu: stride %d (1 or 2)", stride);
    WM_REQUIRE(T_in % stride == 0 && K >= 3 * C_in, "wm_conv1d_gelu: T_in=%d, K=%d < 3*C_in=%d", T_in, K, 3 * C_in);
    const int T_out = T_in / stride;
    GemmBigParams p{};
    // output row t of utterance b = GELU(W . [x_pad[b][s*t], x_pad[b][s*t+1], x_pad[b][s*t+2]] + bias): a strided view
    p.A = (const h16*)x_pad; p.lda = stride * C_in; p.M = B * T_out; p.K = K; p.W = W; p.N = C_out;
    p.a_rows = T_out; p.a_bstride = (long)(T_in + 2) * C_in;
    p.bias = (const h16*)bias; p.C = (h16*)out; p.ldc = C_out; p.act = gelu;
    return launch_gemm_f16(p, (hipStream_t)stream);
}

// ---- test-only entries: the engines' own GemmBigParams / row-kernel options, reachable alone (tests/test_gpu_gemm_epilogue.py)
int wm_gemm_ex(const wm_gemm_io* io, wm_stream_t stream) {
    WM_REQUIRE(io && io->a && io->w && io->c, "wm_gemm_ex: null argument");
    WM_REQUIRE(io->m > 0 && io->n > 0 && io->k > 0, "wm_gemm_ex: empty shape m=%d n=%d k=%d", io->m, io->n, io->k);
    WM_REQUIRE(io->n % 128 == 0, "wm_gemm_ex: n=%d must be a multiple of 128", io->n);
    WM_REQUIRE(io->k % 64 == 0, "wm_gemm_ex: k=%d must be a multiple of 64", io->k);
    WM_REQUIRE(io->act >= 0 && io->act <= 2, "wm_gemm_ex: act=%d (0 none, 1 erf-GELU, 2 tanh-GELU)", io->act);
    WM_REQUIRE(io->lda % 8 == 0 && io->lda > 0, "wm_gemm_ex: lda=%d must be a positive multiple of 8", io->lda);
    WM_REQUIRE(io->colscale_n >= 0 && io->colscale_n <= io->n && io->colscale_n % 4 == 0, "wm_gemm_ex: colscale_n=%d must be a multiple of 4 in [0, n]", io->colscale_n);
    WM_REQUIRE(io->res_mod >= 0 && (!io->residual || (io->ldr >= io->n && io->ldr % 4 == 0)), "wm_gemm_ex: residual needs ldr >= n, a multiple of 4, and res_mod >= 0");
    WM_REQUIRE(io->a_rows >= 0 && io->c_rows >= 0 && io->max_wgs >= 0 && io->tile_rows >= 0, "wm_gemm_ex: negative a_rows / c_rows / max_wgs / tile_rows");
    WM_REQUIRE(io->out_mode == 0 || io->out_mode == 1, "wm_gemm_ex: out_mode=%d (0 row-major, 1 head-split)", io->out_mode);
    if (io->out_mode == 1) {
        WM_REQUIRE(io->hs_t > 0 && io->hs_h > 0 && io->m % io->hs_t == 0, "wm_gemm_ex: head-split needs hs_t > 0, hs_h > 0 and m a multiple of hs_t");
        WM_REQUIRE(io->hs_kv <= 1 && io->n == (io->hs_kv < 0 ? 2 : 1) * io->hs_h * 64, "wm_gemm_ex: head-split n=%d does not match hs_h=%d, hs_kv=%d", io->n, io->hs_h, io->hs_kv);
        WM_REQUIRE(io->c_rows == 0, "wm_gemm_ex: c_rows is for the row-major output only");
    } else {
        WM_REQUIRE(io->ldc >= io->n && io->ldc % 4 == 0, "wm_gemm_ex: ldc=%d must be a multiple of 4, >= n", io->ldc);
        WM_REQUIRE(!(io->q8_inv_scale > 0.f), "wm_gemm_ex: q8_inv_scale is for the head-split output only");
    }
    GemmBigParams p{};
    p.A = (const h16*)io->a; p.lda = io->lda; p.M = io->m; p.K = io->k; p.W = io->w; p.N = io->n;
    p.bias = (const h16*)io->bias; p.C = (h16*)io->c; p.ldc = io->out_mode == 1 ? 0 : io->ldc;
    p.residual = (const h16*)io->residual; p.ldr = io->residual ? io->ldr : 0; p.res_mod = io->res_mod; p.act = io->act;
    p.colscale_n = io->colscale_n; p.colscale = io->colscale;
    p.out_mode = io->out_mode; p.hs_T = io->hs_t; p.hs_H = io->hs_h; p.hs_kv = io->hs_kv; p.q8_inv_scale = io->q8_inv_scale;
    p.a_rows = io->a_rows; p.a_bstride = (long)io->a_bstride; p.c_rows = io->c_rows; p.c_bstride = (long)io->c_bstride;
    p.max_wgs = io->max_wgs; p.tile_rows = io->tile_rows;
    return launch_gemm_f16(p, (hipStream_t)stream);
}

int wm_row_finish(const wm_row_finish_io* io, wm_stream_t stream) {
    WM_REQUIRE(io, "wm_row_finish: null argument");
    WM_REQUIRE(io->mode >= 0 && io->mode <= 3, "wm_row_finish: mode=%d (0 .. 3)", io->mode);
    WM_REQUIRE(io->m > 0 && io->n > 0, "wm_row_finish: empty shape m=%d n=%d", io->m, io->n);
    if (io->mode != 2) {
        WM_REQUIRE(io->part && io->ksplit >= 1 && io->ldp >= io->n, "wm_row_finish: mode %d needs part, ksplit >= 1 and ldp >= n", io->mode);
        WM_REQUIRE(io->part_sstride >= 0 && io->part_sstride % 4 == 0, "wm_row_finish: part_sstride must be a non-negative multiple of 4");
    }
    if (io->mode != 1) WM_REQUIRE(io->x && io->ldx >= io->n, "wm_row_finish: mode %d needs x with ldx >= n", io->mode);
    if (io->mode != 3) WM_REQUIRE(io->out && io->ldo >= io->n, "wm_row_finish: mode %d needs out with ldo >= n", io->mode);
    if (io->mode == 0 || io->mode == 2) WM_REQUIRE(io->ln_gamma && io->ln_beta, "wm_row_finish: mode %d needs ln_gamma and ln_beta", io->mode);
    if (io->mode == 1) WM_REQUIRE(io->gelu_kind == 1 || io->gelu_kind == 2, "wm_row_finish: gelu_kind=%d (1 erf, 2 tanh)", io->gelu_kind);
    RowFinishParams p{};
    p.part = io->part; p.ksplit = io->ksplit; p.M = io->m; p.N = io->n; p.ldp = io->mode == 2 ? 0 : io->ldp; p.part_sstride = (long)io->part_sstride;
    p.bias = (const h16*)io->bias; p.mode = io->mode; p.gelu_kind = io->gelu_kind;
    p.x = (h16*)io->x; p.ldx = io->mode == 1 ? 0 : io->ldx; p.ln_g = (const h16*)io->ln_gamma; p.ln_b = (const h16*)io->ln_beta;
    p.out = (h16*)io->out; p.ldo = io->mode == 3 ? 0 : io->ldo;
    return launch_row_finish(p, (hipStream_t)stream);
}

// the decode attention kernels as the decoder engine calls them (tests/test_gpu_attn_decode_contract.py): what the kernels assume of
// their arguments is checked here, the launchers' own checks follow
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int wm_attn_self_ex(const wm_attn_self_io* io, wm_stream_t stream) {
    WM_REQUIRE(io && io->part && io->present && io->out, "wm_attn_self_ex: null argument");
    WM_REQUIRE(io->B >= 1 && io->H >= 1 && io->L >= 1 && io->T >= 0, "wm_attn_self_ex: bad B/L/T/H (%d, %d, %d, %d)", io->B, io->L, io->T, io->H);
    const int C = io->H * 64;
    WM_REQUIRE(io->ksplit >= 1, "wm_attn_self_ex: ksplit=%d must be >= 1", io->ksplit);
    WM_REQUIRE(io->ldp % 4 == 0 && io->ldp >= 3 * C, "wm_attn_self_ex: ldp=%d must be a multiple of 4, >= 3 * H * 64 = %d", io->ldp, 3 * C);
    WM_REQUIRE(io->part_sstride >= 0 && io->part_sstride % 4 == 0 && (io->part_sstride == 0 || io->part_sstride >= (int64_t)io->B * io->L * io->ldp),
               "wm_attn_self_ex: part_sstride must be 0 or a multiple of 4, >= B * L * ldp");
    WM_REQUIRE(aligned16(io->part) && aligned16(io->bias), "wm_attn_self_ex: part and bias must be 16-byte aligned");
    WM_REQUIRE(io->ldo >= C, "wm_attn_self_ex: ldo=%d < H * 64 = %d", io->ldo, C);
    WM_REQUIRE(io->present_cap >= 1 && io->present_bstride >= (int64_t)2 * C * io->present_cap && io->present_bstride % 16 == 0,
               "wm_attn_self_ex: present_bstride must be a multiple of 16, >= 2 * H * present_cap * 64");
    WM_REQUIRE(aligned16(io->present) && aligned16(io->past), "wm_attn_self_ex: past and present must be 16-byte aligned");
    if (io->past) {
        WM_REQUIRE(io->past_cap >= 1 && io->past_cap >= io->T, "wm_attn_self_ex: past capacity %d < T=%d", io->past_cap, io->T);
        WM_REQUIRE(io->past_bstride >= (int64_t)2 * C * io->past_cap && io->past_bstride % 16 == 0,
                   "wm_attn_self_ex: past_bstride must be a multiple of 16, >= 2 * H * past_cap * 64");
        WM_REQUIRE(io->past != io->present || (io->past_cap == io->present_cap && io->past_bstride == io->present_bstride),
                   "wm_attn_self_ex: past == present (in place) needs the same capacity and stride");
    }
    AttnSelfParams p{};
    p.part = io->part; p.ksplit = io->ksplit; p.ldp = io->ldp; p.part_sstride = (long)io->part_sstride; p.bias = (const h16*)io->bias;
    p.B = io->B; p.L = io->L; p.T = io->T; p.H = io->H;
    p.present = io->present; p.present_cap = io->present_cap; p.present_bstride = (long)io->present_bstride;
    if (io->past) { p.past = io->past; p.past_cap = io->past_cap; p.past_bstride = (long)io->past_bstride; }
    else { p.past = p.present; p.past_cap = p.present_cap; p.past_bstride = p.present_bstride; }      // (as the engine at T = 0)
    p.int8_kv = io->int8_kv ? 1 : 0; p.kv_scale = io->kv_scale; p.amax = io->amax; p.t_dev = io->t_dev;
    p.out = (h16*)io->out; p.ldo = io->ldo; p.live = io->live; p.row_start = io->row_start; p.waves = io->waves;
    return launch_attn_self(p, (hipStream_t)stream);
}

// the checks and the launch wm_attn_cross_ex and wm_attn_cross_group_ex share (G = 1, kvB = B: the ungrouped entry)
static int attn_cross_ex(const wm_attn_cross_io* io, int G, const int32_t* live_utt, wm_stream_t stream) {
    WM_REQUIRE(io && io->part && io->kv && io->out, "wm_attn_cross_ex: null argument");
    WM_REQUIRE(io->B >= 1 && io->H >= 1 && io->L >= 1 && io->Tk >= 1, "wm_attn_cross_ex: bad B/L/H/Tk (%d, %d, %d, %d)", io->B, io->L, io->H, io->Tk);
    const int C = io->H * 64;
    WM_REQUIRE(io->ksplit >= 1, "wm_attn_cross_ex: ksplit=%d must be >= 1", io->ksplit);
    WM_REQUIRE(io->ldp % 4 == 0 && io->ldp >= C, "wm_attn_cross_ex: ldp=%d must be a multiple of 4, >= H * 64 = %d", io->ldp, C);
    WM_REQUIRE(io->part_sstride >= 0 && io->part_sstride % 4 == 0 && (io->part_sstride == 0 || io->part_sstride >= (int64_t)io->B * io->L * io->ldp),
               "wm_attn_cross_ex: part_sstride must be 0 or a multiple of 4, >= B * L * ldp");
    WM_REQUIRE(aligned16(io->part) && aligned16(io->bias) && aligned16(io->kv), "wm_attn_cross_ex: part, bias and kv must be 16-byte aligned");
    WM_REQUIRE(io->ldo >= C, "wm_attn_cross_ex: ldo=%d < H * 64 = %d", io->ldo, C);
    WM_REQUIRE(io->kv_bstride >= (int64_t)2 * C * io->Tk && io->kv_bstride % 16 == 0,
               "wm_attn_cross_ex: kv_bstride must be a multiple of 16, >= 2 * H * Tk * 64");
    WM_REQUIRE(G >= 1 && io->B % G == 0 && G * io->L <= CROSS_GROUP_MAX, "wm_attn_cross_group_ex: G=%d needs G >= 1, B=%d a multiple of it, G * L=%d <= %d",
               G, io->B, G * io->L, CROSS_GROUP_MAX);
    WM_REQUIRE(!live_utt || (G > 1 && io->L == 1 && io->live), "wm_attn_cross_group_ex: live_utt goes with G > 1, L == 1 and a live list");
    WM_REQUIRE(!(G > 1 && io->L == 1 && io->live) || live_utt, "wm_attn_cross_group_ex: a live list needs live_utt when G > 1 and L == 1");
    WM_REQUIRE(io->kv_q8_scale >= 0.f, "wm_attn_cross_ex: kv_q8_scale must not be negative");
    WM_REQUIRE(io->nsplit >= 1 && (io->nsplit == 1 || io->ws), "wm_attn_cross_ex: nsplit=%d needs a workspace", io->nsplit);
    AttnCrossParams p{};
    p.part = io->part; p.ksplit = io->ksplit; p.ldp = io->ldp; p.part_sstride = (long)io->part_sstride; p.bias = (const h16*)io->bias;
    p.B = io->B; p.L = io->L; p.H = io->H; p.Tk = io->Tk; p.kv = (const h16*)io->kv; p.kv_bstride = (long)io->kv_bstride;
    p.kv_q8_scale = io->kv_q8_scale;
    p.out = (h16*)io->out; p.ldo = io->ldo; p.nsplit = io->nsplit; p.ws = io->ws; p.live = io->live;
    p.skip_zero_rows = io->skip_zero_rows ? 1 : 0;
    p.G = G; p.live_utt = live_utt;
    return launch_attn_cross(p, (hipStream_t)stream);
}

int wm_attn_cross_ex(const wm_attn_cross_io* io, wm_stream_t stream) { return attn_cross_ex(io, 1, nullptr, stream); }

int wm_attn_cross_group_ex(const wm_attn_cross_group_io* io, wm_stream_t stream) {
    WM_REQUIRE(io, "wm_attn_cross_group_ex: null argument");
    wm_attn_cross_io c{};
    c.part = io->part; c.ksplit = io->ksplit; c.ldp = io->ldp; c.part_sstride = io->part_sstride; c.bias = io->bias;
    c.B = io->B; c.L = io->L; c.H = io->H; c.Tk = io->Tk; c.kv = io->kv; c.kv_bstride = io->kv_bstride; c.kv_q8_scale = io->kv_q8_scale;
    c.out = io->out; c.ldo = io->ldo; c.nsplit = io->nsplit; c.ws = io->ws; c.live = io->live; c.skip_zero_rows = io->skip_zero_rows;
    return attn_cross_ex(&c, io->G, io->live_utt, stream);
}

int wm_embed(const int32_t* tokens, int tokens_ld, int M, int L, const void* emb_tiles, int C, const void* pos,
             void* x, int ldx, int n_vocab, const int32_t* t_dev, uint32_t* generation, wm_stream_t stream) {
    WM_REQUIRE(tokens && emb_tiles && pos && x, "wm_embed: null argument");
    WM_REQUIRE(M >= 1 && L >= 1 && M % L == 0 && tokens_ld >= L && n_vocab >= 1, "wm_embed: M=%d must be a multiple of L=%d >= 1, tokens_ld=%d >= L, n_vocab=%d >= 1", M, L, tokens_ld, n_vocab);
    WM_REQUIRE(C >= 32 && ldx >= C && ldx % 8 == 0, "wm_embed: ldx=%d must be a multiple of 8, >= C=%d", ldx, C);
    EmbedParams ep{tokens, tokens_ld, M, L, emb_tiles, C, (const h16*)pos, (h16*)x, ldx, n_vocab, t_dev, generation};
    return launch_embed(ep, (hipStream_t)stream);
}

int wm_mel_transpose_pad(const void* mel, int B, int n_mels, int T, void* out, wm_stream_t stream) {
    WM_REQUIRE(mel && out && B >= 1 && n_mels >= 1 && T >= 1, "wm_mel_transpose_pad: null argument or empty input");
    return launch_mel_transpose_pad((const h16*)mel, B, n_mels, T, (h16*)out, (hipStream_t)stream);
}

int wm_zero_pad_rows(void* buf, int B, int Tpad, int C, wm_stream_t stream) {
    WM_REQUIRE(buf && B >= 1 && Tpad >= 2 && C >= 1, "wm_zero_pad_rows: null argument or empty input");
    return launch_zero_pad_rows((h16*)buf, B, Tpad, C, (hipStream_t)stream);
}

int wm_argmax(const void* logits, int64_t row_stride, int batch, int n_vocab, int32_t* ids, wm_stream_t stream) {
    WM_REQUIRE(logits && ids && batch >= 1 && n_vocab >= 1, "wm_argmax: null argument or empty input");
    return launch_argmax((const h16*)logits, (long)row_stride, batch, n_vocab, ids, (hipStream_t)stream);
}

int wm_forced_probs(const void* logits, int batch, int n_pos, int n_vocab, int64_t stride_b, int64_t stride_p, int limit,
                    const int32_t* next, int next_ld, float* out, int out_ld, wm_stream_t stream) {
    WM_REQUIRE(logits && next && out, "wm_forced_probs: null argument");
    WM_REQUIRE(batch >= 1 && n_pos >= 1 && n_vocab >= 1, "wm_forced_probs: batch=%d n_pos=%d n_vocab=%d must be >= 1", batch, n_pos,
               n_vocab);
    WM_REQUIRE(limit >= 1 && limit <= n_vocab, "wm_forced_probs: limit=%d must lie in [1, n_vocab=%d]", limit, n_vocab);
    WM_REQUIRE(stride_p >= n_vocab && stride_b >= (int64_t)(n_pos - 1) * stride_p + n_vocab,
               "wm_forced_probs: strides (%lld, %lld) let rows of %d logits overlap (n_pos=%d)", (long long)stride_b,
               (long long)stride_p, n_vocab, n_pos);
    WM_REQUIRE(next_ld >= n_pos && out_ld >= n_pos, "wm_forced_probs: next_ld=%d / out_ld=%d are below n_pos=%d", next_ld, out_ld, n_pos);
    WM_REQUIRE((int64_t)batch * n_pos <= 0x7fffffffLL, "wm_forced_probs: batch * n_pos = %lld rows exceed 2^31 - 1",
               (long long)batch * n_pos);
    WM_REQUIRE(((uintptr_t)logits & 1) == 0 && ((uintptr_t)next & 3) == 0 && ((uintptr_t)out & 3) == 0,
               "wm_forced_probs: logits must be 2-byte aligned, next and out 4-byte aligned");
    return launch_forced_probs((const h16*)logits, (long)stride_b, (long)stride_p, batch, n_pos, limit, next, next_ld, out, out_ld,
                               (hipStream_t)stream);
}

int wm_gemm_skinny(const void* A, int lda, int M, int K, const void* Wt, int n_blocks, int w8,
                   const void* scale, int ksplit, float* part, wm_stream_t stream) {
    GemmSkinnyParams p{};
    p.A = (const h16*)A; p.lda = lda; p.M = M; p.K = K; p.Wt = Wt; p.n_blocks = n_blocks; p.w8 = w8;
    p.scale = (const h16*)scale; p.ksplit = ksplit; p.part = part;
    return launch_gemm_skinny(p, (hipStream_t)stream);
}
int wm_gemm_skinny_default_ksplit(int M, int K, int n_blocks, int w8) { return skinny_default_ksplit(M, K, n_blocks, w8); }

static GemvSmallParams gemv_params(const wm_gemv_io* io) {
    GemvSmallParams p{};
    p.A = (const h16*)io->a; p.lda = io->lda; p.M = io->m; p.K = io->k; p.Wt = io->wt; p.n_blocks = io->n_blocks; p.w8 = io->w8;
    p.scale = (const h16*)io->scale;
    p.ln_g = (const h16*)io->ln_gamma; p.ln_b = (const h16*)io->ln_beta;
    p.mode = io->mode; p.bias = (const h16*)io->bias; p.gelu_kind = io->gelu_kind;
    p.out32 = io->out32; p.ld32 = io->ld32; p.out16 = (h16*)io->out16; p.ld16 = io->ld16; p.n_valid = io->n_valid;
    p.x = (h16*)io->x; p.ldx = io->ldx;
    return p;
}

int wm_gemm_rows(const wm_gemv_io* io, wm_stream_t stream) {
    WM_REQUIRE(io && io->a && io->wt, "wm_gemm_rows: null argument");
    return launch_gemm_rows(gemv_params(io), (hipStream_t)stream);
}

int wm_gemv_fused(const wm_gemv_io* io, wm_stream_t stream) {
    WM_REQUIRE(io && io->a && io->wt, "wm_gemv_fused: null argument");
    return launch_gemv_small(gemv_params(io), (hipStream_t)stream);
}

int wm_layernorm(const void* x, int ldx, int M, int N, const void* gamma, const void* beta, void* out, int ldo,
                 wm_stream_t stream) {
    return launch_layernorm((const h16*)x, ldx, M, N, (const h16*)gamma, (const h16*)beta, (h16*)out, ldo, (hipStream_t)stream);
}

int wm_attn_encoder(const void* qkv, int ld, int B, int T, int H, void* out, int ldo, wm_stream_t stream) {
    AttnEncParams p{(const h16*)qkv, ld, B, T, H, (h16*)out, ldo};
    return launch_attn_encoder(p, (hipStream_t)stream);
}

// the encoder attention as encoder_forward fills its parameters, max_wgs included (tests/test_gpu_attn_encoder.py)
int wm_attn_encoder_ex(const wm_attn_encoder_io* io, wm_stream_t stream) {
    WM_REQUIRE(io, "wm_attn_encoder_ex: null io");
    WM_REQUIRE(io->qkv, "wm_attn_encoder_ex: null qkv");
    WM_REQUIRE(io->out, "wm_attn_encoder_ex: null out");
    WM_REQUIRE(io->B >= 1 && io->T >= 1 && io->H >= 1, "wm_attn_encoder_ex: bad B/T/H (%d, %d, %d)", io->B, io->T, io->H);
    const int C = io->H * 64;
    WM_REQUIRE(aligned16(io->qkv), "wm_attn_encoder_ex: qkv must be 16-byte aligned");
    WM_REQUIRE(((uintptr_t)io->out & 7) == 0, "wm_attn_encoder_ex: out must be 8-byte aligned");
    WM_REQUIRE(io->ld >= 3 * C && io->ld % 8 == 0, "wm_attn_encoder_ex: ld=%d must be a multiple of 8, >= 3 * H * 64 = %d", io->ld, 3 * C);
    WM_REQUIRE(io->ldo >= C && io->ldo % 4 == 0, "wm_attn_encoder_ex: ldo=%d must be a multiple of 4, >= H * 64 = %d", io->ldo, C);
    WM_REQUIRE(io->max_wgs >= 0, "wm_attn_encoder_ex: max_wgs=%d must not be negative", io->max_wgs);
    AttnEncParams p{(const h16*)io->qkv, io->ld, io->B, io->T, io->H, (h16*)io->out, io->ldo, io->max_wgs};
    return launch_attn_encoder(p, (hipStream_t)stream);
}

int wm_attn_decode_cross(const float* q, int B, int L, int H, int Tk, const void* kv, void* out, int nsplit,
                         float* ws, wm_stream_t stream) {
    AttnCrossParams p{};
    p.part = q; p.ksplit = 1; p.ldp = H * 64; p.bias = nullptr;
    p.B = B; p.L = L; p.H = H; p.Tk = Tk; p.kv = (const h16*)kv; p.kv_bstride = (long)2 * H * Tk * 64;
    p.out = (h16*)out; p.ldo = H * 64; p.nsplit = nsplit; p.ws = ws;
    p.skip_zero_rows = cross_v_skip();
    return launch_attn_cross(p, (hipStream_t)stream);
}

int wm_debug_occupy(int n_workgroups, size_t lds_bytes, int64_t microseconds, wm_stream_t stream) {
    return launch_occupy(n_workgroups, lds_bytes, (long long)microseconds, (hipStream_t)stream);
}

int wm_attn_decode_cross_i8(const float* q, int B, int L, int H, int Tk, const void* kv_i8, float kv_scale, void* out, int nsplit,
                            float* ws, wm_stream_t stream) {
    WM_REQUIRE(kv_scale > 0.f, "wm_attn_decode_cross_i8: the scale must be positive");
    AttnCrossParams p{};
    p.part = q; p.ksplit = 1; p.ldp = H * 64; p.bias = nullptr;
    p.B = B; p.L = L; p.H = H; p.Tk = Tk; p.kv = (const h16*)kv_i8; p.kv_bstride = (long)2 * H * Tk * 64;
    p.kv_q8_scale = kv_scale;
    p.out = (h16*)out; p.ldo = H * 64; p.nsplit = nsplit; p.ws = ws;
    return launch_attn_cross(p, (hipStream_t)stream);
}

int wm_attn_decode_self(const float* qkv, int B, int L, int T, int H, const void* past, int past_cap,
                        void* present, int present_cap, int int8_kv, float kv_scale, void* out, wm_stream_t stream) {
    AttnSelfParams p{};
    p.part = qkv; p.ksplit = 1; p.ldp = 3 * H * 64; p.bias = nullptr;
    p.B = B; p.L = L; p.T = T; p.H = H;
    p.present = present; p.present_cap = present_cap; p.present_bstride = (long)2 * H * present_cap * 64;
    if (T > 0 && past) { p.past = past; p.past_cap = past_cap; p.past_bstride = (long)2 * H * past_cap * 64; }
    else { p.past = present; p.past_cap = present_cap; p.past_bstride = p.present_bstride; }
    p.int8_kv = int8_kv; p.kv_scale = kv_scale; p.out = (h16*)out; p.ldo = H * 64;
    p.waves = self_attn_waves(B * L);
    return launch_attn_self(p, (hipStream_t)stream);
}

int wm_attn_prefill_self(const float* qkv, int B, int L, int H, void* cache, int cap, int int8_kv, float kv_scale, void* out,
                         const int32_t* row_start, const int32_t* live_rows, wm_stream_t stream) {
    WM_REQUIRE(qkv && cache && out, "wm_attn_prefill_self: null argument");
    AttnSelfParams p{};
    p.part = qkv; p.ksplit = 1; p.ldp = 3 * H * 64; p.bias = nullptr;
    p.B = B; p.L = L; p.T = 0; p.H = H;
    p.present = cache; p.present_cap = cap; p.present_bstride = (long)2 * H * cap * 64;
    p.past = cache; p.past_cap = cap; p.past_bstride = p.present_bstride;
    p.int8_kv = int8_kv; p.kv_scale = kv_scale; p.out = (h16*)out; p.ldo = H * 64;
    p.row_start = row_start; p.live = live_rows;
    return launch_attn_prefill_self(p, (hipStream_t)stream);
}

int wm_attn_prefill_cross(const float* q, int B, int L, int H, int Tk, const void* kv, void* out, const int32_t* live_rows, wm_stream_t stream) {
    WM_REQUIRE(q && kv && out, "wm_attn_prefill_cross: null argument");
    AttnCrossParams p{};
    p.part = q; p.ksplit = 1; p.ldp = H * 64; p.bias = nullptr;
    p.B = B; p.L = L; p.H = H; p.Tk = Tk; p.kv = (const h16*)kv; p.kv_bstride = (long)2 * H * Tk * 64;
    p.out = (h16*)out; p.ldo = H * 64; p.live = live_rows;
    return launch_attn_prefill_cross(p, (hipStream_t)stream);
}

int wm_attn_decode_self_rows(const float* qkv, int B, int L, int T, int H, void* cache, int cap, int int8_kv, float kv_scale, void* out,
                             const int32_t* row_start, const int32_t* live_rows, wm_stream_t stream) {
    WM_REQUIRE(qkv && cache && out, "wm_attn_decode_self_rows: null argument");
    WM_REQUIRE(B >= 1 && H >= 1 && T >= 0, "wm_attn_decode_self_rows: bad B/H/T (%d, %d, %d)", B, H, T);
    AttnSelfParams p{};
    p.part = qkv; p.ksplit = 1; p.ldp = 3 * H * 64; p.bias = nullptr;
    p.B = B; p.L = L; p.T = T; p.H = H;
    p.present = cache; p.present_cap = cap; p.present_bstride = (long)2 * H * cap * 64;
    p.past = cache; p.past_cap = cap; p.past_bstride = p.present_bstride;            // in place, as the decode loop runs it
    p.int8_kv = int8_kv; p.kv_scale = kv_scale; p.out = (h16*)out; p.ldo = H * 64;
    p.row_start = row_start; p.live = live_rows;
    p.waves = self_attn_waves(B * L);
    return launch_attn_self(p, (hipStream_t)stream);
}

int wm_quantize_i8(const void* x, void* q, int64_t n, float inv_scale, wm_stream_t stream) {
    return launch_quantize_i8((const h16*)x, (int8_t*)q, (long)n, inv_scale, (hipStream_t)stream);
}

size_t wm_log_mel_workspace_bytes(int batch, int n_samples, int n_mels) {
    return log_mel_workspace_bytes(batch, n_samples, n_mels);
}

int wm_log_mel(const float* audio, int batch, int n_samples, int64_t audio_ld, const float* filters, int n_mels,
               void* mel_f16, float* mel_f32, void* workspace, size_t workspace_bytes, wm_stream_t stream) {
    return launch_log_mel(audio, batch, n_samples, (long)audio_ld, filters, n_mels, (h16*)mel_f16, mel_f32, workspace,
                          workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
