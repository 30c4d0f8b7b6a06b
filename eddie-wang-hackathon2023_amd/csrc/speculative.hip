// The verify step of speculative decoding (wm_verify_step; speculative.py states the contract on the host).
//
// A draft engine has proposed tokens for slots cur_len .. cur_len + n_pos - 2 of every row and ONE decoder pass of the main engine
// has written logits for the n_pos positions cur_len - 1 .. cur_len + n_pos - 2.  The step appends what n_accept successive
// wm_greedy_step calls at temperature 0 would append: the main engine's own token m_j at every position up to and including the
// first one where it differs from the proposal, is EOT, or is the last.
//
// Whisper's rules at position j depend on the tokens before it only; under the assumption that every earlier proposal was accepted
// those tokens are the proposals, which are in the token row already.  So the positions are independent:
//   launch 1  one workgroup per (row, position): greedy_kernel's scan (greedy_scan.h, the SAME function: bit-for-bit the token and
//             the log-probability wm_greedy_step computes on that history) -> (token, log-probability) in the workspace;
//   launch 2  one thread per row walks its candidates in order: compare, append, sums, done.  The walk stops at the first position
//             whose assumption fails, so a candidate computed on a history that did not come true is never used.
// No inter-workgroup atomics, no tickets; the in-place -inf of the suppress lists lands in all n_pos logits rows of a live row.
#include "common.h"
#include "kernels.h"
#include "greedy_scan.h"

namespace wm {

__global__ __launch_bounds__(GREEDY_THREADS) void verify_scan_kernel(VerifyParams vp) {
    const GreedyParams& p = vp.g;
    const int j = blockIdx.x, b = blockIdx.y;
    int32_t* toks = p.tokens + (size_t)b * p.ld_tok;
    if (toks[p.cur_len - 1] == p.eot) return;                  // a finished row: nothing is verified, nothing written (uniform)
    h16* lg = p.logits + (size_t)b * p.ld_row + (size_t)j * vp.pos_stride;
    const Pick best = greedy_pick(p, lg, toks, p.cur_len + j, b);
    if (threadIdx.x == 0) vp.cand[(size_t)b * vp.n_pos + j] = VerifyCand{best.tok, best.lp};
}

constexpr int VERIFY_ACCEPT_THREADS = 256;

// one workgroup; thread t walks rows t, t + 256, ...  The bookkeeping per accepted position is greedy_kernel's.
__global__ __launch_bounds__(VERIFY_ACCEPT_THREADS) void verify_accept_kernel(VerifyParams vp) {
    const GreedyParams& p = vp.g;
    for (int b = threadIdx.x; b < p.B; b += VERIFY_ACCEPT_THREADS) {
        int32_t* toks = p.tokens + (size_t)b * p.ld_tok;
        int n = 0;
        if (toks[p.cur_len - 1] != p.eot) {
            float sum = p.sum_logprobs[b];
            for (int j = 0; j < vp.n_pos; ++j) {
                const int cur = p.cur_len + j;
                const VerifyCand c = vp.cand[(size_t)b * vp.n_pos + j];
                const bool capped = p.row_limit && (cur - p.sample_begin >= p.row_limit[b]);
                const bool empty = c.tok == 0x7fffffff;
                if (!capped) sum = empty ? -INFINITY : sum + c.lp;
                const int next = (!capped && !empty) ? c.tok : p.eot;
                const int proposal = toks[cur];                // (the last position holds no proposal: its value is not used)
                toks[cur] = next;
                ++n;
                if (next == p.eot) {
                    if (p.n_done) atomicAdd(p.n_done, 1);
                    if (p.done) p.done[b] = 1;
                    break;
                }
                if (j == vp.n_pos - 1 || next != proposal) break;
            }
            p.sum_logprobs[b] = sum;
        }
        vp.n_accept[b] = n;
    }
}

size_t verify_workspace_bytes(int batch, int n_pos) {
    return (size_t)(batch > 0 ? batch : 0) * (size_t)(n_pos > 0 ? n_pos : 0) * sizeof(VerifyCand);
}

int launch_verify(const VerifyParams& vp, hipStream_t stream) {
    const GreedyParams& p = vp.g;
    WM_REQUIRE(vp.n_pos >= 1 && vp.n_pos <= 4, "wm_verify_step: n_pos %d outside [1, 4]", vp.n_pos);
    WM_REQUIRE(p.B >= 1 && p.B <= 65535 && p.V >= 1, "wm_verify_step: batch %d outside [1, 65535] or n_vocab %d below 1", p.B, p.V);
    WM_REQUIRE(p.cur_len >= 1 && p.cur_len + vp.n_pos <= p.ld_tok, "wm_verify_step: slots cur_len=%d .. +%d do not fit tokens_ld=%d",
               p.cur_len, vp.n_pos - 1, p.ld_tok);
    WM_REQUIRE(vp.n_pos == 1 || vp.pos_stride >= p.V, "wm_verify_step: pos_stride %ld is below n_vocab %d", vp.pos_stride, p.V);
    // the suppress lists are written into every (row, position) in place: the n_pos logits rows of one row must end before the next row begins
    WM_REQUIRE(p.B == 1 || p.ld_row >= (long)(vp.n_pos - 1) * vp.pos_stride + p.V,
               "wm_verify_step: row_stride %ld is below (n_pos - 1) * pos_stride + n_vocab = %ld", p.ld_row, (long)(vp.n_pos - 1) * vp.pos_stride + p.V);
    WM_REQUIRE(((size_t)vp.cand & 7) == 0, "wm_verify_step: workspace is not 8-byte aligned");
    WM_REQUIRE(p.n_suppress == 0 || p.suppress != nullptr, "wm_verify_step: suppress list is null");
    WM_REQUIRE(vp.n_accept && vp.cand, "wm_verify_step: n_accept or workspace is null");
    hipLaunchKernelGGL(verify_scan_kernel, dim3(vp.n_pos, p.B), dim3(GREEDY_THREADS), 0, stream, vp);
    WM_LAUNCH_CHECK(stream, "wm_verify_step (scan)");
    hipLaunchKernelGGL(verify_accept_kernel, dim3(1), dim3(VERIFY_ACCEPT_THREADS), 0, stream, vp);
    WM_LAUNCH_CHECK(stream, "wm_verify_step (accept)");
    return 0;
}

}  // namespace wm
