/* whisper_mi355.h -- C ABI of libwhisper_mi355.so, the MI355X (gfx950) Whisper engine.
 *
 * This library is the drop-in for what sits under the reference's `Session` object
 * (R/tensorrt_llm/runtime/session.py:53-61,116-178; R = tensorrt_llm_july-release-v1): a
 * deserialised TensorRT engine plus the plugin library loaded by
 * `ctypes.CDLL(libnvinfer_plugin_tensorrt_llm.so); initLibNvInferPlugins(...)`
 * (R/tensorrt_llm/plugin/plugin.py:10-22, R/cpp/tensorrt_llm/plugins/api/InferPlugin.cpp:147-170).
 * TensorRT's IPluginV2DynamicExt vtable ABI is not reproducible without TensorRT, so the boundary
 * sits one level up: the three engines of examples/whisper (encoder, cross-attention K/V,
 * decoder; W/build.py:26-31) as three stateless entry points, with the same contract `Session.run`
 * has: asynchronous enqueue on the caller's stream, the CALLER owns every buffer (inputs, outputs
 * and workspace are raw device pointers), no hidden allocation, no hidden synchronisation.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; `wm_last_error()` then returns a
 *     thread-local message.  Nothing throws, nothing aborts (the reference's plugins are
 *     `noexcept` and report through caughtError, weightOnlyQuantMatmulPlugin.cpp:332-342).
 *   - all device pointers must belong to the device the engine was created on.
 *   - fp16 = IEEE binary16.  Tensors are dense row-major unless a leading dimension is given.
 *   - re-entrant for distinct (engine, stream, workspace); one host thread per GPU in the
 *     data-parallel design.  The only global state is the error string and WM_SYNC_CHECK.
 *     A caller that CAPTURES calls of this library into a hipGraph while another of its threads is inside the HIP runtime (the Python host
 *     issues the next batch's encoder from a helper thread) must capture with hipStreamCaptureModeThreadLocal or keep that thread out of
 *     the runtime for the length of the capture: in the global mode any thread's runtime call invalidates the capture (the Python host
 *     does both: decoding.py, encoding.py, native.CAPTURE_LOCK).
 */
#ifndef WHISPER_MI355_H
#define WHISPER_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wm_engine wm_engine;
typedef void* wm_stream_t; /* hipStream_t */

enum { WM_ENGINE_ENCODER = 0, WM_ENGINE_DECODER = 1, WM_ENGINE_CROSS_KV = 2 };
enum { WM_FLAG_WEIGHT_ONLY_INT8 = 1, WM_FLAG_INT8_KV = 2, WM_FLAG_GELU_TANH = 4,
       WM_FLAG_INT8_CROSS_KV = 16 /* opt-in, beyond the reference: cross-attention K/V stored as int8 codes */ };

/* Same ten fields, same order, as the OpenAI checkpoint `dims` (W/build.py:146-154). */
typedef struct wm_dims {
    int32_t n_mels, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer;
    int32_t n_vocab, n_text_ctx, n_text_state, n_text_head, n_text_layer;
} wm_dims;

/* ABI version of this header.  Callers built against another version must refuse to run (native.py does).
 *   2  wm_gemm takes a workspace before the stream; wm_decoder_io / wm_greedy_io carry the per-row `done` flags
 *   3  weight-only engines keep int8 at rest: wm_cross_kv takes (workspace, workspace_bytes) and REJECTS fewer than
 *      wm_cross_kv_workspace_bytes() bytes for every engine kind (256 B for fp16 engines; the fp16 expansion of one layer's
 *      matrix for weight-only ones) -- a caller that passed NULL / 0 to an fp16 engine before now gets rc 1;
 *      wm_gemm_rows, wm_set_rows_path
 *   4  wm_set_self_attn_waves
 *   5  (round 4) wm_set_gemm_small_tiles, wm_lab_knobs; environment knobs are honoured only under WM_LAB=1;
 *      wm_greedy_io gains the sampling fields (temperature, seed) and `without_timestamps` moves into the device rules
 *   6  (round 4) wm_set_decode_chain / wm_decode_chain_error; wm_decoder_io gains `workspace_id` (appended)
 *   7  (round 5) the decoder workspace needs NO initialisation by the caller any more (the library clears the state it keeps there,
 *      on the stream of the call); a one-launch step that gave up makes the NEXT wm_decoder_step fail (rc 1) until
 *      wm_decode_chain_error has been called; wm_decode_chain_status, wm_debug_occupy
 *   8  (round 6) wm_decoder_io gains `not_alone` (appended): the caller says when other decoder steps may run beside this one
 *      (still 8, like wm_mel_windows / wm_resample) wm_decoder_io gains `row_start` (appended; NULL = as before); wm_attn_decode_self_rows
 *      (still 8: test-only entries, no existing struct or signature changed) wm_attn_self_ex, wm_attn_cross_ex
 *      (still 8: entries and structs of their own, no existing struct or signature changed) wm_decoder_step_group / wm_decoder_group_io,
 *      wm_step_finish_group, wm_attn_cross_group_ex
 *      (still 8: an entry only) wm_forced_probs
 *      (still 8: entries only) wm_section_cuts, wm_section_cuts_workspace_bytes
 *      (still 8: entries only) wm_speech_spans, wm_speech_spans_workspace_bytes, wm_mel_gather
 *      (still 8: entries and a struct of their own, no existing struct or signature changed) wm_decoder_prefill / wm_prefill_io,
 *      wm_decoder_prefill_workspace_bytes; test-only entries wm_attn_prefill_self, wm_attn_prefill_cross
 *      (still 8: an entry and a struct of its own) wm_repeat_controls / wm_repeat_io
 *      (still 8: a test-only entry and a struct of its own) wm_attn_encoder_ex / wm_attn_encoder_io
 *      (still 8: an entry and structs of its own) wm_sequence_bias / wm_bias_io / wm_bias_item
 *      (still 8: an entry and a struct of its own) wm_sample_step / wm_sample_io
 *      (still 8: entries only) wm_resample_channels, wm_channel_top, wm_channel_top_workspace_bytes
 *      (still 8: entries only) wm_dtw_open, wm_align_open, wm_decoder_prefill_tap
 *      (still 8: entries and a struct of its own) wm_verify_step / wm_verify_io, wm_verify_workspace_bytes */
#define WM_ABI_VERSION 8
int wm_version(void);
const char* wm_last_error(void);
int wm_device_count(int* out);

/* ---- engines ------------------------------------------------------------------------------
 * `blob` is the content of one *.engine file written by build.py (our packed-weight format, see
 * DESIGN.md "engine blob").  Replaces Session.from_serialized_engine (session.py:53-61).
 * The library copies the weights to `device` and keeps only that copy. */
int wm_engine_create(const void* blob, size_t nbytes, int device, wm_engine** out);
void wm_engine_destroy(wm_engine* e);
int wm_engine_info(const wm_engine* e, int32_t* kind, uint32_t* flags, wm_dims* dims);
/* bytes of device memory holding this engine's weights.  Weight-only engines keep int8 (or int4 codes, one per byte for the
 * row-major matrices of the encoder / cross-K/V engines) + fp16 scales at rest; the encoder / cross-K/V engines expand one matrix
 * at a time to fp16(fp16(q) * scale) into the caller's workspace right before its GEMM (the workspace sizes below include that
 * scratch block): the reference dequantises in registers (fpA_intB_gemm_template.h:47-140), same values.                    */
size_t wm_engine_weight_bytes(const wm_engine* e);

/* ---- encoder engine: W/encoding.py:48-76 -> WhisperEncoder.forward (whisper/model.py:149-172) ---
 * mel  : fp16 [batch, n_mels, 2*n_audio_ctx]    ("x")
 * out  : fp16 [batch, n_audio_ctx, n_audio_state] ("output")                                      */
size_t wm_encoder_workspace_bytes(const wm_engine* e, int batch);
int wm_encoder_forward(const wm_engine* e, const void* mel, int batch, void* out,
                       void* workspace, size_t workspace_bytes, wm_stream_t stream);
/* The same forward pass, sharing the GPU with other work (the reference's run.py takes its batches one after the other,
 * W/run.py:109-169; here the encoder of batch n+1 can run UNDER the HBM-bound decode loop of batch n).
 * cu_budget > 0: the MFMA-bound kernels of this call occupy at most that many compute units -- their workgroups are
 * persistent and stay on their CU, so kernels of other streams are never queued behind them; the results are bit-identical
 * to wm_encoder_forward's (same tiles, same arithmetic, fewer workgroups walking over them).  0 = the whole chip. */
int wm_encoder_forward_shared(const wm_engine* e, const void* mel, int batch, void* out,
                              void* workspace, size_t workspace_bytes, int cu_budget, wm_stream_t stream);
/* The same pass in pieces (ABI 7): layers [layer_begin, layer_end) of the encoder on `cu_budget` CUs (0 = the whole chip).  A range
 * that starts at 0 runs the two convolutions first, one that ends at n_audio_layer the final LayerNorm, which writes `out`; between
 * the calls of one pass the residual stream lives in `workspace` (same workspace, same batch, calls in layer order on one stream
 * or ordered streams).  A caller that runs the pass beside a decode loop gives back the CU budget the moment the loop has ended:
 * the layers still to come are issued with cu_budget 0 (WhisperEncoding.prefetch does, layer by layer).  Bit-identical to
 * wm_encoder_forward whatever the cut and the budgets.                                                                        */
int wm_encoder_forward_range(const wm_engine* e, const void* mel, int batch, void* out, void* workspace, size_t workspace_bytes,
                             int cu_budget, int layer_begin, int layer_end, wm_stream_t stream);

/* ---- cross-attention K/V engine: W/decoding.py:515-541 -> CrossAttn_KV.forward (model.py:469-540)
 * xa          : fp16 [batch, n_audio_ctx, n_text_state]
 * out_layers  : n_text_layer device pointers, each fp16 [batch, 2, n_head, n_audio_ctx, 64]
 *               ("cross_present_key_value_{i}", dim 1: 0 = K, 1 = V)                              */
size_t wm_cross_kv_workspace_bytes(const wm_engine* e, int batch);
int wm_cross_kv(const wm_engine* e, const void* xa, int batch, void* const* out_layers,
                void* workspace, size_t workspace_bytes, wm_stream_t stream);

/* ---- decoder engine: W/decoding.py:543-659 -> WhisperDecoder.forward (model.py:241-299) ---------
 * One call = L new tokens for each of `batch` utterances on top of T cached tokens.               */
typedef struct wm_decoder_io {
    int32_t batch, n_new /* L: 1 for a decode step, len(sot_sequence) for the prefill; blocks longer than 4
                            (prompts, prefixes) run as 4-token passes over the growing cache */, n_past /* T */;
    const int32_t* tokens;            /* int32 [batch, L]                               "x" */
    int32_t tokens_ld;                /* elements between utterances in `tokens` (0 = L); lets a
                                         step read column cur-1 of a [batch, capacity] buffer   */
    const void* positional_embedding; /* fp16 [L, n_text_state], rows T..T+L of the table
                                         (the caller slices: decoding.py:604-608)            */
    /* self-attention KV cache, per layer [batch, 2, n_head, capacity, 64], int8 when the engine
     * has WM_FLAG_INT8_KV, else fp16.  past[i] may be NULL when n_past == 0.
     * present[i] == past[i] with equal capacities = in-place append (the fast path);
     * otherwise the T cached rows are copied and the L new ones appended (the reference's
     * concat semantics, attention.py:296-306, "present_key_value_{i}" of shape [.., T+L, 64]). */
    const void* const* past;  int32_t past_capacity;
    void* const* present;     int32_t present_capacity;
    const void* const* cross; /* per layer fp16 [batch, 2, n_head, n_audio_ctx, 64]          */
    void* logits;             /* fp16 [batch, L, n_vocab]                            "output" */
    void* workspace; size_t workspace_bytes;
    /* optional calibration hook (NULL in production): fp32 [n_text_layer], running
     * max(|q|,|k|,|v|) of each layer's self-attention projections, the statistic the reference's
     * int8-KV calibration collects with forward hooks (W/smoothquant.py:117-175,
     * W/torch_whisper_convert.py:145-167).  The caller zeroes it before the first call. */
    float* qkv_amax;
    /* optional device-resident step counter (NULL = use n_past): int32 holding T.  With it, one
     * captured hipGraph of a decode step can be replayed for every token: `tokens` is then the base
     * of the [batch, tokens_ld] buffer (column T is read), `positional_embedding` the base of the
     * table (row T is read), `n_past` only an upper bound for validation.  Requires n_new == 1 and
     * in-place KV append.  wm_step_advance increments the counter on the stream.                   */
    const int32_t* n_past_dev;
    /* optional list of the utterances that are still decoding (NULL = all of them): device int32 [1 + batch], word 0 =
     * their number n, words 1..n = their indices in ascending order (wm_step_finish maintains it from the `done` flags of
     * wm_greedy_step).  The reference stops its (single) utterance at EOT (W/decoding.py:817-819); in a batch the rows that
     * have finished drop out of the attention kernels this way: their cross K/V (245.76 MB per token at large-v2) and
     * their KV cache are no longer read, their rows of `logits` are left unspecified (finite) -- wm_greedy_step keeps such a
     * row at EOT whatever its logits.  A live row's result does not depend on which other rows are live. */
    const int32_t* live_rows;
    /* identity of the workspace's CONTENTS (ABI 6): 0 = unknown.  The one-launch token step of a one-row group (wm_set_decode_chain)
     * keeps state inside the workspace: tagged granules, a call counter, a table of the per-layer `cross` / `present` pointers.  The
     * workspace itself needs no preparation (ABI 7: hipMalloc / torch.empty memory is fine) -- the library initialises that state, on
     * the stream of the call: with 0 on EVERY call (a 120 KB memset node and four small launches: correct, a few microseconds slower),
     * with a non-zero id once per (address, id), and the table is rewritten only when the pointers differ from what the library last
     * wrote there.  A non-zero id is the caller's promise that since the id was first passed nothing but wm_decoder_step calls of this
     * engine with the same (batch, n_new) have written to the workspace: give every allocation a new id, and a new one whenever the
     * memory is reused for anything else.  A call that is being captured into a graph is never remembered: if no eager call has
     * initialised the state under this (address, id) before, the graph carries the initialisation and every replay repeats it --
     * issue one eager call first (as WhisperDecoding.main_loop does) to keep it out of the graph. */
    uint64_t workspace_id;
    /* (ABI 8) non-zero: steps of OTHER utterance groups may be in flight on this device while this one runs (stream-parallel groups, as
     * WhisperDecoding.main_loop issues them from 13 utterances up).  The one-launch forms of a group of up to eight rows need their 256
     * workgroups resident TOGETHER; two such launches dispatched side by side can each hold half of the chip and wait for the other
     * half until the bounded waits give up -- so a step that is not alone always takes a launch per kernel.  0 = the caller issues one
     * decoder step at a time on this device (the reference's own schedule, W/decoding.py:785-821).  */
    int32_t not_alone;
    /* (appended under ABI 8, like wm_mel_windows / wm_resample: NULL = every row begins at slot 0, the behaviour so far)
     * RIGHT-ALIGNED ROWS: device int32 [batch].  Utterance b's sequence begins at slot row_start[b] of its token row and of its KV
     * cache; the slots before it are pad (any valid token id).  All rows of the call still share n_past, n_new and the step counter --
     * only the front of a row moves, so rows with start sequences of different lengths (a prompt per row) fit one call:
     *   - the positional embedding of slot t of utterance b is row t - row_start[b] of the table (pad slots: row 0).  With n_past_dev
     *     `positional_embedding` is the table's base as ever; without, it is the table's row n_past AND rows 0 .. n_past - 1 must lie
     *     in front of it (a slice of the whole table: what decoding.py passes);
     *   - self-attention: utterance b sees the keys of slots [row_start[b], t] only; a query in a pad slot reads nothing and yields
     *     zeros (its logits are finite and meaningless); K / V rows are appended at slot t as ever.  A row computes exactly what it
     *     would compute alone, un-padded, with n_past - row_start[b] cached tokens (csrc/attn_decode.hip states the contract);
     *   - a call with row_start never takes a one-launch form (as if not_alone were set).
     * wm_decoder_step only: wm_decoder_step_multi and wm_decoder_step_tap refuse it (rc 1).                                          */
    const int32_t* row_start;
} wm_decoder_io;
size_t wm_decoder_workspace_bytes(const wm_engine* e, int batch, int n_new);
int wm_decoder_step(const wm_engine* e, const wm_decoder_io* io, wm_stream_t stream);

/* ---- candidate groups: one copy of the cross-attention K/V per utterance (added within ABI 8: a struct and entries of their own; wm_decoder_io
 * keeps its layout) ----
 * wm_decoder_step for rows that come in groups of G = cross_group consecutive rows -- the beams or best_of samples of utterance a are rows
 * a * G .. a * G + G - 1 -- which share ONE copy of the utterance's cross-attention K/V.  cross_group 0 or 1: exactly wm_decoder_step(io).
 * With G > 1, `io.cross[i]` is [batch / G, 2, n_head, n_audio_ctx, 64]; batch % G == 0 and G * min(n_new, 4) <= 8 (a call of more than 4
 * tokens runs as 4-token passes, so it takes G = 2 at most; the candidates of an utterance begin with the same tokens, so a caller prefills
 * ONE row per utterance with wm_decoder_step on the same buffers and copies its cache rows and logits to the candidates -- WhisperDecoding
 * does).  Everything else (tokens, caches, logits, live_rows) stays per row.
 *   - n_new == 1: one item of the cross-attention launch streams K/V row a once and serves the utterance's G rows; a row's context has the
 *     bits it has in wm_decoder_step on K/V repeated G times at the same number of key-range pieces.  The pieces are chosen for the items
 *     the launch has (n_head * batch / G * pieces), so that number may differ from the repeated call's: across it the logits agree within
 *     the decoder's usual bound, not bit for bit.
 *   - n_new > 1 (prefill passes): a row's own item reads K/V row b / G.
 *   - with io.live_rows, `live_groups` must be given: device int32 [1 + batch / G], word 0 = the number of utterances that still have a
 *     live row, then their indices, ascending (wm_step_finish_group maintains both lists).  An utterance that is not listed is not read; a
 *     finished row of a listed utterance gets finite, unspecified logits, as ever.  Read only when n_new == 1.
 *   - such a call never takes a one-launch form (as if io.not_alone were set); wm_decoder_workspace_bytes(batch, n_new) covers it.
 * wm_decoder_step_multi and wm_decoder_step_tap take a wm_decoder_io and so know no groups: the CU-partitioned schedule and the forced pass of
 * the word timestamps run one row per utterance.                                                                                      */
typedef struct wm_decoder_group_io {
    wm_decoder_io io;
    int32_t cross_group;
    const int32_t* live_groups;
} wm_decoder_group_io;
int wm_decoder_step_group(const wm_engine* e, const wm_decoder_group_io* gio, wm_stream_t stream);

/* ---- block prefill: a whole start block in ONE pass (added within ABI 8: a struct and entries of their own) ----
 * wm_decoder_step runs a block of more than 4 tokens as 4-token passes over the growing cache: a 227-token block (a prompt per row) is
 * 57 passes, each of which streams every decoder weight and every row's cross K/V again.  wm_decoder_prefill runs the block -- n_new = L
 * tokens, 1 .. n_text_ctx, on an EMPTY cache (n_past must be 0) -- through the launch-per-kernel layer sequence once, at batch * L rows
 * (the Linear forms the step picks for that many rows), with two attention kernels of its own (csrc/attn_prefill.hip):
 *   - self-attention is causal inside the block over the block's own UN-QUANTISED k / v, whatever the cache type -- what the reference
 *     computes for a block fed whole; the 4-token passes of wm_decoder_step see the earlier tokens of the same block through their int8
 *     codes when the engine has WM_FLAG_INT8_KV, so the two agree within the int8-KV bound, not bit for bit.  Every slot 0 .. L - 1 is
 *     appended to present[i] in place (fp16 rows, or int8 codes), pad slots included;
 *   - io.row_start and io.live_rows behave as in wm_decoder_step: a query in a pad slot yields zeros in the self-attention, its logits
 *     are finite and meaningless; rows that live_rows does not name are not read by the attention kernels and their cache is not
 *     written -- their rows of `logits` (from logits_from on) ARE written, with unspecified values (computed from whatever the workspace held);
 *   - io.logits keeps wm_decoder_step's layout, fp16 [batch, L, n_vocab], but only positions logits_from .. L - 1 of every utterance are
 *     written (the final LayerNorm and the vocabulary product run over batch * (L - logits_from) rows); positions below are untouched;
 *   - io.past / past_capacity are not read; workspace: wm_decoder_prefill_workspace_bytes(batch, n_new), linear in batch * n_new; no
 *     allocation, no synchronisation: the call can be captured into a hipGraph; it never takes a one-launch form.
 * rc 1 (nothing launched) for: n_past != 0, n_past_dev or qkv_amax set, present buffers missing or present_capacity < L,
 * L > n_text_ctx, logits_from outside 0 .. L - 1, an engine with WM_FLAG_INT8_CROSS_KV.  A following wm_decoder_step continues on
 * the cache with n_past = L.                                                                                                          */
typedef struct wm_prefill_io {
    wm_decoder_io io;        /* n_new = L, 1 .. n_text_ctx; n_past must be 0 */
    int32_t logits_from;     /* 0 .. L-1: logits are written for positions logits_from .. L-1 only */
} wm_prefill_io;
size_t wm_decoder_prefill_workspace_bytes(const wm_engine* e, int batch, int n_new);
int wm_decoder_prefill(const wm_engine* e, const wm_prefill_io* io, wm_stream_t stream);

/* The same step for n_groups (<= 8) independent utterance groups at once, scheduled for the chip:
 * group g's latency-bound kernels (weight-streaming GEMMs, row kernels, self-attention) are enqueued on
 * light_streams[g]; every group's cross-attention kernel -- the HBM-bound part, 245.76 MB per utterance --
 * goes to heavy_stream in (layer, group) order, tied to its group's stream by events.  With the light
 * streams confined to a few CUs and the heavy stream to the rest (wm_stream_create_cu_mask) the short
 * kernels of one group run at full speed WHILE another group streams its K/V; on ordinary streams the
 * hardware queues starve them (scripts/cumask_probe.py).  Results are identical to n_groups calls of
 * wm_decoder_step.  Eager launches only (CU masks do not survive hipGraph capture). */
int wm_decoder_step_multi(const wm_engine* e, int n_groups, const wm_decoder_io* const* ios,
                          const wm_stream_t* light_streams, wm_stream_t heavy_stream);
/* A stream whose kernels only run on the CUs whose bit is set in mask[0..n_words) (bit i of word i/32 =
 * CU i; MI355X: 256 CUs = 8 words).  hipExtStreamCreateWithCUMask behind the C ABI. */
int wm_stream_create_cu_mask(const uint32_t* mask, int n_words, wm_stream_t* out);
int wm_stream_destroy(wm_stream_t stream);

/* ---- fused greedy step (device-side restatement of W/decoding.py:134-217,274-300) ----------------
 * Applies SuppressBlank / SuppressTokens / ApplyTimestampRules to the last-position logits of each
 * utterance, picks the arg-max, accumulates its log-probability, keeps finished rows at EOT and
 * appends the token at tokens[b][cur_len].  n_done (device int32, caller zeroes it) counts rows
 * whose new token is EOT.
 * A live row with no finite allowed logit (everything the rules leave is -inf) ends, as a beam without a
 * live candidate does in wm_beam_step: EOT is appended, done[b] is set, the row counts in n_done and
 * sum_logprobs[b] becomes -inf.  wm_sample_step does the same (its kept_out is then 0, cut_out -inf). */
typedef struct wm_greedy_io {
    void* logits; int64_t row_stride; /* fp16; row b starts at logits + b*row_stride elements;
                                         suppressed entries are overwritten with -inf in place,
                                         like the reference's filters do (decoding.py:202-217) */
    int32_t batch, n_vocab;
    int32_t* tokens; int32_t tokens_ld; int32_t cur_len;
    float* sum_logprobs;
    const int32_t* suppress; int32_t n_suppress; /* token ids suppressed on every step */
    const int32_t* blank; int32_t n_blank; /* suppressed on the first sampled step only */
    int32_t sample_begin, eot, timestamp_begin, max_initial_timestamp_index /* -1: none */;
    int32_t apply_rules; /* 0: plain arg-max; 1: SuppressBlank + SuppressTokens + ApplyTimestampRules; 2: the two suppress filters only (without_timestamps, W/decoding.py:337-346) */
    int32_t* n_done;
    const int32_t* n_past_dev; /* optional device step counter: cur_len = *n_past_dev + 1 */
    int32_t* done;             /* optional int32 [batch]: set to 1 when the row's new token is EOT (never cleared here) */
    const int32_t* row_limit;  /* optional int32 [batch]: row b samples at most row_limit[b] tokens, then ends with EOT
                                  without adding to its log-probability -- a per-utterance `sample_len` (the reference has
                                  one for the whole loop, W/decoding.py:328, whose loop ends the same way: no EOT
                                  log-probability, finalize pads the EOT) */
    /* ABI 5: sampling (GreedyDecoder.update at temperature > 0, W/decoding.py:282-285).  temperature > 0: the next token is
     * drawn from softmax(filtered logits / temperature) by a Gumbel-max with a counter-based generator keyed on (seed, row0 + b,
     * position, token); sum_logprobs books log_softmax(filtered logits)[token] at temperature 1, as the reference does.
     * seed_dev (optional, two uint32 words in device memory: low, high) overrides `seed` -- a replayed graph then draws afresh. */
    float temperature; int32_t row0;
    uint64_t seed; const uint32_t* seed_dev;
} wm_greedy_io;
int wm_greedy_step(const wm_greedy_io* io, wm_stream_t stream);
int wm_step_advance(int32_t* counter, wm_stream_t stream);
/* End of a decode step of one utterance group: *counter += 1 (when counter is given) and the list of rows still decoding
 * is rebuilt from the flags: live[0] = number of rows with done[b] == 0, live[1..] = their indices, ascending.
 * batch <= 1024. */
int wm_step_finish(int32_t* counter, const int32_t* done, int batch, int32_t* live, wm_stream_t stream);
/* The same for candidate groups of `group` consecutive rows (batch % group == 0; wm_decoder_group_io::cross_group), and next to `live` the
 * list of the utterances that still have a live row: live_groups[0] = their number, live_groups[1..] = their indices, ascending
 * (int32 [1 + batch / group]).  Added under ABI 8 (an entry only). */
int wm_step_finish_group(int32_t* counter, const int32_t* done, int batch, int group, int32_t* live, int32_t* live_groups, wm_stream_t stream);

/* ---- repetition penalty and no-repeat n-grams (added within ABI 8: an entry and a struct of its own) ----------------
 * The two controls of CTranslate2 / Hugging Face generation on the raw logits of a token step, in place, BEFORE the logit
 * filters of wm_greedy_step / wm_beam_step: one launch between the decoder call and the token step (repetition.py states the
 * contract on the host).  Per row b, H = tokens[b][sample_begin .. cur_len - 1], m = cur_len - sample_begin
 * tokens: what the row has sampled -- the start sequence and the prompt are not part of it.
 *   repetition_penalty p (finite, > 0; 1 = off): for every DISTINCT t of H with t < eot, once however often it occurs,
 *     x = fp32(logits[t]); y = x > 0 ? x / p : x * p as one correctly rounded fp32 operation; logits[t] = fp16(y), round to
 *     nearest even.  -inf stays -inf.
 *   no_repeat_ngram_size n (>= 0; 0 = off): if m >= n - 1, for every i in 0 .. m - n with H[i .. i + n - 2] == H[m - n + 1 .. m - 1]
 *     the token t = H[i + n - 1] is banned if t < eot: logits[t] = -inf.  Matching runs over H as it is, timestamps included;
 *     n = 1 bans every text token of H.
 * Penalty first, then bans.  Only text tokens (0 <= id < eot) are ever changed: EOT, the specials and the timestamps belong to
 * Whisper's own rules.  The log-probabilities the token step books are therefore those of the distribution AFTER the controls,
 * exactly as they are after the suppress lists.  With both controls off nothing is launched.
 * Refused (rc 1, nothing launched): a null io / logits / tokens; batch or n_vocab < 1; row_stride < n_vocab with more than one row;
 * eot outside [0, n_vocab]; p <= 0 or not finite; n < 0; sample_begin outside [0, tokens_ld]; cur_len outside
 * [sample_begin, tokens_ld]; a history above WM_REPEAT_MAX_HISTORY tokens -- m for a host cur_len, tokens_ld - sample_begin with
 * n_past_dev (what m can reach: the device value is not known to the host).  Asynchronous on `stream`, no allocation, capturable. */
#define WM_REPEAT_MAX_HISTORY 512           /* >= n_text_ctx = 448 */
typedef struct wm_repeat_io {
    void* logits; int64_t row_stride;         /* fp16, the LAST position's rows; row b starts at logits + b*row_stride elements (any 2-byte address) */
    int32_t batch, n_vocab;
    const int32_t* tokens; int32_t tokens_ld; /* int32 [batch][tokens_ld] */
    int32_t cur_len;                          /* tokens each row holds so far (wm_greedy_io::cur_len) */
    const int32_t* n_past_dev;                /* optional device step counter: cur_len = *n_past_dev + 1, as wm_greedy_io reads it */
    int32_t sample_begin, eot;
    float repetition_penalty;                 /* 1: off */
    int32_t no_repeat_ngram_size;             /* 0: off */
    const int32_t* done;                      /* optional int32 [batch]: a row whose flag is set is left untouched */
} wm_repeat_io;
int wm_repeat_controls(const wm_repeat_io* io, wm_stream_t stream);

/* ---- hotwords and sequence bias (added within ABI 8: an entry and structs of its own) ----------------------------------
 * A bias on the raw logits of a token step, in place, AFTER wm_repeat_controls and BEFORE the logit filters of wm_greedy_step /
 * wm_beam_step: one launch inside the step (biasing.py states the contract on the host and builds the table).
 * The table: `items` (wm_bias_item: target, k, offset, bias) and `pool` (int32 tokens); item i reads "if the last k tokens of H
 * equal pool[offset .. offset + k - 1] (k = 0 always matches, also on an empty H), token `target` gets `bias`".  H is the history of
 * wm_repeat_io: tokens[b][sample_begin .. cur_len - 1], timestamps included.  Per row and target, among the matching items the one
 * with the greatest k wins (equal k: the earlier item), and exactly ONE update is applied: x = fp32(logits[target]); y = x + bias,
 * one correctly rounded fp32 addition; logits[target] = fp16(y), round to nearest even.  -inf stays -inf; biases are never summed.
 * The table must be sorted by (target ascending, k descending), as biasing.build_table leaves it: every logit is then read and
 * written by exactly one thread.  The results on an unsorted table are unspecified; on ANY table and whatever the device words hold
 * the kernel stays inside its arrays: items beyond `capacity`, a k outside [0, WM_BIAS_MAX_K] or above the row's history, a prefix
 * that leaves [0, pool_capacity) and a target outside [0, eot) make an item inert.
 * The number of items a launch sees is min(*n_items_dev, capacity) (all `capacity` items without the word), read on the device:
 * a captured launch follows a table rewritten in place.  capacity = 0: nothing is launched.
 * Refused (rc 1, nothing launched): the null / range / alignment refusals of wm_repeat_controls (its history bound included); a null
 * `items` or `pool` with capacity > 0; capacity outside [0, WM_BIAS_MAX_ITEMS]; pool_capacity outside [0, WM_BIAS_MAX_POOL]; `items`
 * not 16-byte aligned, `pool` / `n_items_dev` not 4-byte aligned.  Asynchronous on `stream`, no allocation, capturable. */
#define WM_BIAS_MAX_ITEMS 4096
#define WM_BIAS_MAX_POOL 4096
#define WM_BIAS_MAX_K 31                    /* a phrase has at most 32 tokens */
typedef struct wm_bias_item {
    int32_t target;                           /* the text token that gets `bias` */
    int32_t k;                                /* tokens of the prefix */
    int32_t offset;                           /* where the prefix starts in the pool */
    float bias;
} wm_bias_item;
typedef struct wm_bias_io {
    void* logits; int64_t row_stride;         /* as wm_repeat_io: fp16, the LAST position's rows, any 2-byte address */
    int32_t batch, n_vocab;
    const int32_t* tokens; int32_t tokens_ld;
    int32_t cur_len;
    const int32_t* n_past_dev;                /* optional device step counter: cur_len = *n_past_dev + 1 */
    int32_t sample_begin, eot;
    const int32_t* done;                      /* optional int32 [batch]: a row whose flag is set is left untouched */
    const wm_bias_item* items;                /* device, [capacity], 16-byte aligned */
    const int32_t* pool;                      /* device, int32 [pool_capacity] */
    int32_t capacity, pool_capacity;
    const int32_t* n_items_dev;               /* optional device word: the items in use */
} wm_bias_io;
int wm_sequence_bias(const wm_bias_io* io, wm_stream_t stream);

/* ---- top-k / top-p / min-p sampling (added within ABI 8: an entry and a struct of its own) ----------------------------
 * A WHOLE token step: wm_greedy_step at temperature > 0 with the draw restricted to a kept set (truncation.py states the contract
 * on the host).  It takes the place of wm_greedy_step, it is not a launch in front of it: the kept set is a
 * property of the distribution AFTER the step's own rules (suppress lists, timestamp rules, the text-versus-timestamp decision).
 * Per row: A = the allowed tokens whose logit is not -inf, x_n their fp16 logits, m their maximum.  The values of A form classes
 * v_1 = m > v_2 > ... with counts c_j; a class is kept or dropped whole, so the result is one number, the cut: token n may be
 * drawn iff x_n >= cut.  Weights are integers: q(v) ~ 2^30 exp((v - m) / T) from d = fp32(v) - fp32(m), s = d * exp2_scale,
 * i = rint(s), f = s - i, a degree-6 polynomial in f evaluated in single correctly rounded fp32 operations (no fused multiply-add),
 * rounded to an integer and shifted right by -i with rounding; i < -31 weighs 0 (truncation.py: the coefficients and the
 * measured error).  In Hugging Face's order:
 *   top_k (0 = off)              j_k = the smallest j with c_1 + ... + c_j >= top_k: ties at the k-th value are all kept;
 *   top_p_q16 = P (65536 = off)  with Q_j = sum_{i<=j} c_i q(v_i), Q = Q_{j_k}: j_p = the smallest j with Q_j * 2^16 >= P * Q;
 *   min_p_gap (-inf = off)       classes with fp32(v) - fp32(m) >= min_p_gap are kept (the host passes fp32(T ln min_p)).
 * The row keeps classes 1 .. min(j_k, j_p, j_q); class 1 always.  The draw is wm_greedy_step's Gumbel-max -- same generator, same
 * coordinates (seed, row0 + b, position, token) -- over the kept tokens: with all three off every row draws exactly the token
 * wm_greedy_step draws.  sum_logprobs books log_softmax over the UNTRUNCATED allowed set at temperature 1 and the logits row is
 * not written apart from the suppress lists.  EOT stickiness, row_limit, done, n_done and the append are wm_greedy_step's.
 * cut_out / kept_out (optional, [batch]): the value of the last kept class and the number of kept tokens (-inf and 0 for a row
 * with nothing allowed), for tests.  The result of a row depends on the row alone.
 * Refused (rc 1, nothing launched): what wm_greedy_step refuses; batch or n_vocab < 1; g.temperature <= 0 or not finite; top_k < 0;
 * exp2_scale <= 0 or not finite; top_p_q16 outside [1, 65536]; min_p_gap > 0 or NaN.  Asynchronous on `stream`, no workspace, no
 * allocation, capturable. */
typedef struct wm_sample_io {
    wm_greedy_io g;                           /* the token step; g.temperature = T > 0 */
    int32_t top_k;                            /* 0: off */
    float exp2_scale;                         /* c = fp32(log2(e) / T) */
    int32_t top_p_q16;                        /* P = max(1, round(top_p * 2^16)); 65536: off */
    float min_p_gap;                          /* fp32(T * ln(min_p)); -inf: off */
    float* cut_out;                           /* optional fp32 [batch] */
    int32_t* kept_out;                        /* optional int32 [batch] */
} wm_sample_io;
int wm_sample_step(const wm_sample_io* io, wm_stream_t stream);

/* ---- speculative decoding: the verify step (added within ABI 8: entries and a struct of its own) ----------------------
 * A draft engine has proposed tokens for slots cur_len .. cur_len + n_pos - 2 of every row; ONE wm_decoder_step of the main engine
 * with n_new = n_pos has written logits for the positions cur_len - 1 .. cur_len + n_pos - 2 (logits row j of a row decides slot
 * cur_len + j).  This step takes the place of n_pos wm_greedy_step calls (speculative.py states the contract on the host; DESIGN.md
 * section 5p).  Per row and j = 0, 1, ...: m_j = the token wm_greedy_step would pick at cur_len + j from logits row j given the history
 * as it then stands (rules included: apply_rules 0 / 1 / 2, the first sampled position, every state of the timestamp rules).  m_j is
 * written to slot cur_len + j and its log-probability added to the row's sum; the walk stops when m_j is EOT (done / n_done are set as
 * wm_greedy_step sets them), when j == n_pos - 1, or when m_j differs from the proposal that stood in that slot.  n_accept[b] = the
 * slots written, 1 .. n_pos.  A row whose previous token (slot cur_len - 1) is EOT writes nothing and reports 0 -- unlike
 * wm_greedy_step, which keeps appending EOT.  row_limit and the row with no finite allowed logit behave as in wm_greedy_step.
 * BIT FOR BIT: tokens, sum_logprobs, done and n_done after the call are what n_accept[b] successive wm_greedy_step calls at temperature
 * 0 leave behind (the two kernels share one definition of the scan, csrc/greedy_scan.h).  Slots behind the last one written keep the
 * proposals.  The suppress lists are written as -inf into all n_pos logits rows of a live row, whatever n_accept turns out to be.
 * Two launches: one workgroup per (row, position), then one small launch that walks every row's candidates; `workspace` carries the
 * candidates between them (wm_verify_workspace_bytes(batch, n_pos) bytes, 8-byte aligned, no initialisation).
 * Refused (rc 1, nothing launched): a null io / logits / tokens / sum_logprobs / n_accept / workspace; g.temperature != 0;
 * g.n_past_dev or g.seed_dev set; n_pos outside [1, 4]; batch outside [1, 65535]; n_vocab < 1; cur_len < 1 or
 * cur_len + n_pos > tokens_ld; pos_stride < n_vocab with n_pos > 1; g.row_stride < (n_pos - 1) * pos_stride + n_vocab with batch > 1 (the
 * positions of one row would run into the next row); a workspace that is not 8-byte aligned.  Asynchronous on `stream`, no allocation, capturable. */
typedef struct wm_verify_io {
    wm_greedy_io g;       /* g.logits = position 0 of row 0; g.cur_len = first slot to fill (host value);
                             g.temperature must be 0, g.n_past_dev and g.seed_dev NULL */
    int64_t pos_stride;   /* elements between the logits rows of consecutive positions of one utterance */
    int32_t n_pos;        /* 1 .. 4 */
    int32_t* n_accept;    /* device int32 [batch] */
    void* workspace;      /* wm_verify_workspace_bytes(batch, n_pos) */
} wm_verify_io;
size_t wm_verify_workspace_bytes(int batch, int n_pos);
int wm_verify_step(const wm_verify_io* io, wm_stream_t stream);

/* ---- beam search step (added within ABI 8: new entries only, no existing struct or signature changed) ----------------
 * The semantics of upstream Whisper's BeamSearchDecoder.update on the device, one call per token step of an utterance
 * group.  Rows are n_audio x beam_size; beam j of utterance a is row a * beam_size + j.  Per utterance:
 *   1. the logit filters of wm_greedy_step (same fields, same meaning) on every row's own history, log-softmax in fp32;
 *   2. every beam proposes its beam_size + 1 best tokens (equal log-probabilities: lower token id first; tokens at -inf are
 *      never proposed -- Whisper's rules always leave more than beam_size + 1 finite ones); score = sum_logprobs + logprob.
 *      At the first sampled step (cur_len == sample_begin) the beams are identical and only beam 0 proposes;
 *   3. candidates are walked by (score descending, parent beam ascending, token ascending).  One ending in EOT joins the
 *      step's finished list, any other becomes the next live beam until beam_size are saved, where the walk stops;
 *   4. live beam i takes its parent's token history plus the new token (moved in place), sum_logprobs[i] = the score and
 *      parent[i] = the parent's row index within this launch (wm_kv_reorder moves the self-attention cache accordingly);
 *   5. the finished candidates go to the utterance's pool (history + EOT, score, length), best first, while it holds
 *      fewer than max_candidates.  A full pool completes the utterance: done[] of all its rows is set, n_done grows by
 *      beam_size, live_len[a] = the live beams' length, and every later call leaves the utterance untouched (frozen;
 *      parent = identity).  row_limit (per row, the beams of an utterance carry the same value): after that many sampled
 *      tokens the utterance is frozen before the step.  ignore_eot: EOT candidates are pooled but nothing is frozen.
 * Bounds: 1 <= beam_size <= 8, 1 <= max_candidates <= 16, batch a multiple of beam_size.                              */
typedef struct wm_beam_io {
    void* logits; int64_t row_stride;   /* as wm_greedy_io */
    int32_t batch, n_vocab;             /* batch = rows = n_audio * beam_size */
    int32_t* tokens; int32_t tokens_ld; int32_t cur_len;
    float* sum_logprobs;
    const int32_t* suppress; int32_t n_suppress;
    const int32_t* blank; int32_t n_blank;
    int32_t sample_begin, eot, timestamp_begin, max_initial_timestamp_index;
    int32_t apply_rules;
    int32_t beam_size, max_candidates, ignore_eot;
    const int32_t* n_past_dev;          /* optional device step counter: cur_len = *n_past_dev + 1 */
    const int32_t* row_limit;           /* optional int32 [batch] */
    int32_t* parent;                    /* out, int32 [batch] */
    int32_t* fin_tokens;                /* pool: int32 [n_audio, max_candidates, tokens_ld] */
    float* fin_scores;                  /* float [n_audio, max_candidates] */
    int32_t* fin_len;                   /* int32 [n_audio, max_candidates]: tokens of the entry, the closing EOT included */
    int32_t* fin_count;                 /* int32 [n_audio], caller zeroes it */
    int32_t* live_len;                  /* int32 [n_audio]: length of a frozen utterance's live beams (written when it freezes) */
    int32_t* done;                      /* int32 [batch], caller zeroes it */
    int32_t* n_done;                    /* optional int32 [1] */
    void* workspace; size_t workspace_bytes;   /* >= wm_beam_workspace_bytes(batch, beam_size): the rows' proposals */
} wm_beam_io;
size_t wm_beam_workspace_bytes(int batch, int beam_size);
int wm_beam_step(const wm_beam_io* io, wm_stream_t stream);
/* The self-attention caches follow their beams: for every layer (layers_dev: n_layer DEVICE-resident pointers to
 * [batch, 2, n_head, capacity, 64] of elem_bytes 1 (int8) or 2 (fp16)) row i receives row parent[i]'s positions 0 .. n_last,
 * n_last = *n_past_dev when given.  In place: one workgroup owns the same slice of all beams of an utterance, loads, then
 * stores.  Utterances whose parents are the identity or whose done[] is set (optional) are skipped; nothing beyond n_last
 * is touched.  A parent outside its own utterance's rows is treated as the identity. */
int wm_kv_reorder(void* const* layers_dev, int n_layer, int batch, int beam_size, int n_head, int capacity, int elem_bytes,
                  const int32_t* parent, const int32_t* done, int n_last, const int32_t* n_past_dev, wm_stream_t stream);

/* ---- word-level timestamps (added within ABI 8: new entries only, no existing struct or signature changed) ------------
 * Upstream Whisper's find_alignment on the device: a teacher-forced pass that records the cross-attention queries of the
 * alignment heads (wm_decoder_step_tap), then softmax over frames, z-score over tokens, median filter over frames, mean over
 * heads and dynamic time warping (wm_align).  DESIGN.md "word timestamps" states the contract; timing.py is its host form.
 *
 * wm_decoder_step_tap = wm_decoder_step for n_new <= 4 on the launch-per-kernel path (as if io->not_alone were set; n_past_dev
 * must be NULL).  Behind the cross-attention query projection of every layer that has a listed head, one small kernel adds the
 * split-K slabs and the bias in the cross-attention kernel's own order and writes r16(q_sum + bias) -- the query BEFORE the
 * 64^-0.25 scaling -- of the listed heads to q_tape, rows n_past .. n_past + n_new.  Logits and cache append are bit-identical
 * to wm_decoder_step with not_alone = 1.                                                                                     */
typedef struct wm_tap_io {
    void* q_tape;            /* fp16 [batch][n_heads][capacity][64]: slot k of dim 1 belongs to heads[k] */
    int32_t capacity;        /* rows per (utterance, head), >= n_past + n_new */
    const int32_t* heads;    /* HOST array: layer * n_text_head + head, strictly ascending */
    int32_t n_heads;
} wm_tap_io;
int wm_decoder_step_tap(const wm_engine* e, const wm_decoder_io* io, const wm_tap_io* tap, wm_stream_t stream);
/* The alignment matrix and its DTW path for every utterance of a batch.  Per utterance b with N_all = n_tokens[b] forced
 * tokens and F = n_frames[b] valid frames, per listed head: S[i][f] = q16[i] . k16[f] in fp32 (q16 = r16(tape * 64^-0.25),
 * k16 = r16(K * 64^-0.25)), W = softmax over f < F, Z = (W - mean_i W) / std_i W (population std over the N_all rows; Z = 0
 * where std == 0), median of filter_width along f with reflection at 0 and F - 1 (no filter when F <= filter_width / 2);
 * Mtx = mean over the heads, added in the order of `heads`.  Rows n_prefix .. N_all - 2 of Mtx (N = N_all - n_prefix - 1 of
 * them) are row 0 .. N - 1 of `matrix`, and wm_dtw's walk over -Mtx gives the path.  Utterances with N < 1 or F < 1 get
 * path_len 0.  Nothing beyond row N - 1, column F - 1 of `matrix` and entry path_len - 1 of the paths is written.
 * fp16 cross K/V only: an `engine` with WM_FLAG_INT8_CROSS_KV is refused (rc 1).                                             */
typedef struct wm_align_io {
    const wm_engine* engine;          /* optional: the decoder engine the tape came from (its flags and dims are checked) */
    int32_t batch, n_text_head, n_audio_ctx;
    const void* q_tape; int32_t capacity;      /* as wm_tap_io */
    const void* const* cross; int32_t n_layers; /* HOST array of per-layer device pointers, fp16 [batch, 2, n_text_head, n_audio_ctx, 64] (layers without a listed head are not read) */
    const int32_t* heads; int32_t n_heads;     /* HOST array, as wm_tap_io */
    const int32_t* n_tokens;                   /* device int32 [batch]: N_all, clipped to cap_tokens */
    const int32_t* n_frames;                   /* device int32 [batch]: F, clipped to n_audio_ctx */
    int32_t n_prefix, filter_width;            /* filter_width odd, 1 .. 15 (1: no filter) */
    int32_t cap_tokens;                        /* >= every n_tokens[b], <= capacity, <= 448 */
    float* matrix; int32_t ld;                 /* optional fp32 [batch][cap_tokens][ld], ld >= n_audio_ctx (NULL: kept in the workspace) */
    int32_t* path_text; int32_t* path_time;    /* int32 [batch][cap_tokens + n_audio_ctx] */
    int32_t* path_len;                         /* int32 [batch] */
    void* workspace; size_t workspace_bytes;   /* >= wm_align_workspace_bytes(batch, n_heads, cap_tokens, n_audio_ctx) */
} wm_align_io;
size_t wm_align_workspace_bytes(int batch, int n_heads, int cap_tokens, int n_audio_ctx);
int wm_align(const wm_align_io* io, wm_stream_t stream);
/* The DTW stage alone (test entry): utterance b walks x_b = x + b * x_bstride, fp32 [n_rows[b]][ldx] with n_cols[b] valid
 * columns (device int32 arrays; values clipped to max_rows <= 1023 / max_cols).  cost[0][0] = 0, borders +inf,
 * cost[i][j] = fp32(x[i-1][j-1] + min(c0 = cost[i-1][j-1], c1 = cost[i-1][j], c2 = cost[i][j-1])) with the predecessor chosen by
 * "c0 < c1 and c0 < c2: diagonal; else c1 < c0 and c1 < c2: up; else left"; the walk back from (n_rows, n_cols) is reversed
 * into path_text / path_time [batch][path_ld], path_len[b] entries (0 when n_rows[b] < 1 or n_cols[b] < 1).               */
size_t wm_dtw_workspace_bytes(int batch, int max_rows, int max_cols);
int wm_dtw(const float* x, int ldx, int64_t x_bstride, int batch, const int32_t* n_rows, const int32_t* n_cols, int max_rows,
           int max_cols, int32_t* path_text, int32_t* path_time, int path_ld, int32_t* path_len, void* workspace,
           size_t workspace_bytes, wm_stream_t stream);

/* ---- forced alignment (added within ABI 8: new entries only, no existing struct or signature changed) ----------------------
 * Placing a transcript the caller already has: a window of a long file holds an unknown prefix of the remaining text, so the
 * walk's end is free on the token axis, and the forced pass is one block (alignment.py is the host form).
 *
 * wm_dtw_open = wm_dtw with an open end: the cost table and the trace codes are wm_dtw's, cell for cell; the walk back starts at
 * (i*, n_cols), i* = the smallest i in 1 .. n_rows with cost[i][n_cols] <= cost[k][n_cols] for every k in 1 .. n_rows (fp32
 * compares; the costs are not normalised by the path's length).  end_row (device int32 [batch]) receives i*, 0 (with path_len 0)
 * where n_rows[b] < 1 or n_cols[b] < 1.  One launch; thread i keeps cost[i][n_cols] when it computes it and the arg-min is one
 * shuffle reduction per wave plus one pass over the waves' results in LDS.  Shape limits, workspace (wm_dtw_workspace_bytes)
 * and everything else written: wm_dtw's.                                                                                   */
int wm_dtw_open(const float* x, int ldx, int64_t x_bstride, int batch, const int32_t* n_rows, const int32_t* n_cols, int max_rows,
                int max_cols, int32_t* path_text, int32_t* path_time, int path_ld, int32_t* path_len, int32_t* end_row,
                void* workspace, size_t workspace_bytes, wm_stream_t stream);
/* wm_align with wm_dtw_open's walk in place of the closed one: the matrix (the z-score runs over all n_tokens[b] rows) and the
 * median filter are wm_align's bit for bit; end_row[b] counts rows of `matrix` (1 .. N), 0 where the utterance has no path.   */
int wm_align_open(const wm_align_io* io, int32_t* end_row, wm_stream_t stream);
/* wm_decoder_prefill with wm_decoder_step_tap's hook: behind the cross-attention query projection of every layer that has a
 * listed head, one small kernel adds the block's split-K slabs and the bias in the block cross-attention kernel's own order
 * (rounds of four slabs, then the rest one by one) and writes r16(q_sum + bias) of the listed heads to rows 0 .. n_new - 1 of
 * q_tape; rows beyond are not touched.  Its grid folds the row index, so batch * n_new may pass 65 535.  Logits (from
 * logits_from on) and the appended cache are wm_decoder_prefill's bit for bit.  Refused (rc 1) before the first launch: whatever
 * wm_decoder_prefill refuses, io.row_start, and the head lists wm_decoder_step_tap refuses; tap->capacity >= n_new.
 * Workspace: wm_decoder_prefill_workspace_bytes.                                                                            */
int wm_decoder_prefill_tap(const wm_engine* e, const wm_prefill_io* io, const wm_tap_io* tap, wm_stream_t stream);

/* ---- kernel-level entry points (parity tests, micro-benchmarks, roofline measurement) -----------*/
/* C[M,N] = act(A[M,K] x W[N,K]^T * scale + bias) (+ residual); W fp16 or int8 (w8) row-major [N][K].
 * act: 0 none, 1 erf-GELU, 2 tanh-GELU.  Replaces CutlassFpAIntBGemmRunner::gemm /
 * the TRT MatMul (fpA_intB_gemm_template.h:47-140).  w8: the engines' own path for a weight-only
 * matrix of an M >> 16 stage -- W is expanded to fp16(fp16(q) * scale) (the reference kernels'
 * per-element dequantisation) into `workspace` (>= N*K*2 bytes), then the fp16 MFMA GEMM runs on it.
 * N a multiple of 128, K a multiple of 64.                                                         */
int wm_gemm(const void* A, int lda, int M, int K, const void* W, int N, int w8, const void* scale,
            const void* bias, const void* residual, int ldr, int act, void* C, int ldc,
            void* workspace, size_t workspace_bytes, wm_stream_t stream);
/* 1-D convolution, kernel 3, padding 1, stride 1 or 2, + GELU (gelu: 1 erf, 2 tanh), as the encoder
 * engine runs it (Conv1d, R/tensorrt_llm/layers/conv.py:52-94; W/torch_model.py:152-156): a GEMM over a
 * strided view of the zero-padded token-major input, no im2col.  x_pad fp16 [B][T_in+2][C_in] with rows 0
 * and T_in+1 of every utterance zero, followed by >= 512 finite elements of slack (the K padding is read
 * and multiplied by zero weights); W fp16 [C_out][K], K index = tap*C_in + c_in, zero columns up to a
 * multiple of 64 (weight.py: conv_weight_as_gemm); C_out a multiple of 128, C_in of 8.
 * out fp16 [B][T_in/stride][C_out].                                                                 */
int wm_conv1d_gelu(const void* x_pad, int B, int T_in, int C_in, const void* W, int K, const void* bias,
                   int C_out, int stride, int gelu, void* out, wm_stream_t stream);
/* ---- test-only entries (added within ABI 8: new entries only): the options of the MFMA GEMM and the row kernels that only the
 * engines set, reachable alone so that parity tests can hold each to one fp16 ulp (tests/test_gpu_gemm_epilogue.py,
 * tests/test_gpu_row_kernels.py).  Not used by the product path.
 * wm_gemm_ex: C = epilogue(A . W^T), W fp16 [n][k] row-major, with every option the encoder and the cross-K/V engine use:
 *   v = fp16(sum + bias); v = fp16(act(v)); columns < colscale_n: v = fp16(v * colscale); v = fp16(v + residual[row % res_mod or row])
 *   a_rows > 0: row m of A lives at a + (m / a_rows) * a_bstride + (m % a_rows) * lda (elements); c_rows / c_bstride: the same for C
 *   out_mode 1: C is head-split [m / hs_t, 2, hs_h, hs_t, 64]; hs_kv < 0: n = 2 * hs_h * 64 and the K | V index is col / (hs_h * 64),
 *     else n = hs_h * 64 and hs_kv (0 or 1) names the half; q8_inv_scale > 0 (head-split only): C holds int8 codes
 *     sat_s8(rne(fp16 result * q8_inv_scale))
 *   max_wgs > 0: the persistent kernel on at most that many workgroups; tile_rows > 0: its tile order (1 = plain row-major).
 * n a multiple of 128, k of 64, lda of 8, ldc / ldr of 4, colscale_n of 4. */
typedef struct wm_gemm_io {
    const void* a; int32_t lda, m, k;
    const void* w; int32_t n;
    const void* bias;                    /* fp16 [n], may be NULL */
    void* c; int32_t ldc;
    const void* residual; int32_t ldr, res_mod;
    int32_t act;                         /* 0 none, 1 erf-GELU, 2 tanh-GELU */
    int32_t colscale_n; float colscale;
    int32_t out_mode, hs_t, hs_h, hs_kv;
    float q8_inv_scale;
    int32_t a_rows; int64_t a_bstride;
    int32_t c_rows; int64_t c_bstride;
    int32_t max_wgs, tile_rows;
} wm_gemm_io;
int wm_gemm_ex(const wm_gemm_io* io, wm_stream_t stream);
/* The row kernel behind every Linear of the big-batch split-K decode path: y16 = fp16(sum_s part[s][row][:] + bias), then
 *   mode 0  x = fp16(x + y16) in place, out = LayerNorm(x) * ln_gamma + ln_beta      mode 1  out = fp16(gelu(y16)) (gelu_kind 1 erf, 2 tanh)
 *   mode 2  out = LayerNorm(x) * ln_gamma + ln_beta only (no partial sums)             mode 3  x = fp16(x + y16) only
 * part fp32 [ksplit][m][ldp], slabs part_sstride elements apart (0: m * ldp); bias may be NULL.  n a multiple of 4, <= 6144.
 * Fewer than 64 rows run the latency form (eight slabs in flight, the GELU mode cut into column ranges), more the gentle one:
 * the same bits per row. */
typedef struct wm_row_finish_io {
    const float* part; int32_t ksplit, m, n, ldp; int64_t part_sstride;
    const void* bias;
    int32_t mode, gelu_kind;
    void* x; int32_t ldx;
    const void* ln_gamma; const void* ln_beta;
    void* out; int32_t ldo;
} wm_row_finish_io;
int wm_row_finish(const wm_row_finish_io* io, wm_stream_t stream);
/* The decode attention kernels (csrc/attn_decode.hip) with every field of AttnSelfParams / AttnCrossParams that the decoder engine
 * sets, reachable alone (tests/test_gpu_attn_decode_contract.py; wm_attn_decode_self / _self_rows / _cross / _cross_i8 below fix
 * ksplit = 1, no bias, dense strides, ldo = C, a host T).  Not used by the product path.
 * Both: q (and k, v) rows arrive as fp32 split-K slabs part[ksplit][B * L][ldp], slabs part_sstride elements apart (0: B * L * ldp);
 *   row = fp16(sum_s part[s][row][:] + bias) (bias fp16, may be NULL); live (optional, DEVICE int32 [1 + B]): count, then the rows to
 *   process -- the other rows' outputs, caches and workspace blocks are not touched.
 * wm_attn_self_ex: slab columns q | k | v (3 * H * 64), bias [3 * H * 64]; the k / v rows are appended at slots T .. T + L - 1 of
 *   present [B][2][H][present_cap][64] (fp16, or int8 codes sat_s8(rne(x * (1 / kv_scale))) with int8_kv), utterances present_bstride
 *   elements apart; past (NULL: present) holds the T cached slots, and is copied forward when it is another buffer; t_dev (optional,
 *   DEVICE int32): T is read from it on the device (the host T must still fit present_cap); amax (optional, DEVICE fp32): atomic
 *   running maximum of |q|, |k|, |v| (the fp16 rows, before the d^-0.25 scale) over the rows processed; row_start (optional, DEVICE
 *   int32 [B]): right-aligned rows, as wm_attn_decode_self_rows; waves 0 / 1: one wave per (utterance, head), 4: the workgroup form
 *   -- passed straight through (wm_set_self_attn_waves is not consulted).
 * wm_attn_cross_ex: slab columns q (H * 64), bias [H * 64]; kv [B][2][H][Tk][64] fp16, or int8 codes with value code * kv_q8_scale
 *   when kv_q8_scale > 0, utterances kv_bstride elements apart; nsplit > 1 splits the key range and needs ws, fp32
 *   [B * H * nsplit * L * 66], indexed by the ORIGINAL row with a live list; skip_zero_rows is passed straight through
 *   (wm_set_cross_v_skip is not consulted).
 * Refused (rc 1, nothing launched): a null part / present / kv / out; B, H < 1, T < 0; ksplit < 1; ldp or part_sstride not a multiple
 *   of 4, ldp < 3 * H * 64 (self) / H * 64 (cross), 0 < part_sstride < B * L * ldp; part, bias, past, present, kv not 16-byte
 *   aligned; ldo < H * 64; past_bstride / present_bstride / kv_bstride below one utterance's extent or not a multiple of 16;
 *   past_cap < T; past == present with another capacity or stride; kv_q8_scale < 0; nsplit > 1 without ws; and whatever the
 *   launchers refuse (L outside 1 .. 4, T + L > 512 or > present_cap, Tk outside 1 .. 1536, nsplit outside 1 .. 16, waves). */
typedef struct wm_attn_self_io {
    const float* part; int32_t ksplit, ldp; int64_t part_sstride;
    const void* bias;
    int32_t B, L, T, H;
    const void* past; int64_t past_bstride; int32_t past_cap;
    void* present; int64_t present_bstride; int32_t present_cap;
    int32_t int8_kv; float kv_scale;
    float* amax;
    const int32_t* t_dev;
    void* out; int32_t ldo;
    const int32_t* live;
    const int32_t* row_start;
    int32_t waves;
} wm_attn_self_io;
int wm_attn_self_ex(const wm_attn_self_io* io, wm_stream_t stream);
typedef struct wm_attn_cross_io {
    const float* part; int32_t ksplit, ldp; int64_t part_sstride;
    const void* bias;
    int32_t B, L, H, Tk;
    const void* kv; int64_t kv_bstride;
    float kv_q8_scale;
    void* out; int32_t ldo;
    int32_t nsplit;
    float* ws;
    const int32_t* live;
    int32_t skip_zero_rows;
} wm_attn_cross_io;
int wm_attn_cross_ex(const wm_attn_cross_io* io, wm_stream_t stream);
/* wm_attn_cross_ex for candidate groups (AttnCrossParams::G; wm_decoder_group_io::cross_group): rows a * G .. a * G + G - 1 read K/V row a of
 * kv [B / G][2][H][Tk][64].  L == 1: one item per (head, utterance, key-range piece) serves the G queries of the utterance from one K/V
 * stream; with the same nsplit, ksplit and skip setting every live row has the bits wm_attn_cross_ex gives for B rows on K/V repeated
 * G times.  L > 1: the row's own item reads K/V row b / G.  ws stays indexed by the ORIGINAL row.  live_utt (DEVICE int32
 * [1 + B / G], L == 1 with `live` only): count, then the utterances to read -- an utterance that is not listed is not read and none of
 * its rows' outputs or workspace blocks are touched; a row of a listed utterance that is not on `live` gets finite, unspecified output.
 * Refused (rc 1, nothing launched): G < 1, B % G != 0, G * L > 8, live without live_utt (G > 1, L == 1) or live_utt without it, and
 * everything wm_attn_cross_ex refuses.  Added under ABI 8 (an entry and a struct of its own). */
typedef struct wm_attn_cross_group_io {
    const float* part; int32_t ksplit, ldp; int64_t part_sstride;
    const void* bias;
    int32_t B, L, H, Tk;
    const void* kv; int64_t kv_bstride;
    float kv_q8_scale;
    void* out; int32_t ldo;
    int32_t nsplit;
    float* ws;
    const int32_t* live;
    int32_t skip_zero_rows;
    int32_t G;
    const int32_t* live_utt;
} wm_attn_cross_group_io;
int wm_attn_cross_group_ex(const wm_attn_cross_group_io* io, wm_stream_t stream);
/* The encoder attention kernel (csrc/attn_encoder.hip) with every field of AttnEncParams that the encoder engine sets, reachable alone
 * (tests/test_gpu_attn_encoder.py; wm_attn_encoder below has no max_wgs).  Not used by the product path.  qkv fp16 [B * T][ld], columns
 * q | k | v of H * 64 each (q, k pre-scaled by 64^-0.25, as the QKV epilogue leaves them), columns 3 * H * 64 .. ld - 1 are not read;
 * out fp16 [B * T][ldo], columns H * 64 .. ldo - 1 are not written.  max_wgs as wm_encoder_forward_shared passes it (2 * cu_budget):
 * > 0 and below the B * H * ceil(T / 256) items of a T > 128 launch: the persistent form on at most that many workgroups (rounded
 * down to a multiple of 8 from 8 on); otherwise, and always with 0, the plain launch.  The lab knob WM_ATTN_MAX_WGS is consulted
 * only with max_wgs == 0, as by wm_attn_encoder.
 * Refused (rc 1, nothing launched): a null io / qkv / out; qkv not 16-byte aligned; out not 8-byte aligned; ld < 3 * H * 64 or not
 * a multiple of 8; ldo < H * 64 or not a multiple of 4; B, T or H < 1; max_wgs < 0.  Added under ABI 8 (an entry and a struct of
 * its own). */
typedef struct wm_attn_encoder_io {
    const void* qkv; int32_t ld;
    int32_t B, T, H;
    void* out; int32_t ldo;
    int32_t max_wgs;
} wm_attn_encoder_io;
int wm_attn_encoder_ex(const wm_attn_encoder_io* io, wm_stream_t stream);
/* x[r] = fp16(E[token of row r] + pos[r % L + T]), r < M = B * L; token of row r = tokens[(r / L) * tokens_ld + r % L + T];
 * T = *t_dev when given, else 0.  emb_tiles: the fp16 embedding in tile-linear layout (weight.py: tile_linear), C a multiple
 * of 32; token ids are clamped to [0, n_vocab).  generation (optional): incremented once per call. */
int wm_embed(const int32_t* tokens, int tokens_ld, int M, int L, const void* emb_tiles, int C, const void* pos,
             void* x, int ldx, int n_vocab, const int32_t* t_dev, uint32_t* generation, wm_stream_t stream);
/* mel fp16 [B][n_mels][T] -> out fp16 [B][T + 2][n_mels], rows 0 and T + 1 of every utterance zero. */
int wm_mel_transpose_pad(const void* mel, int B, int n_mels, int T, void* out, wm_stream_t stream);
/* The windows of a ragged batch of log-mels (long-form transcription: one file per row, each at its own position):
 *   out[b][m][j] = seek[b] + j < src_frames[b] ? src[b][m * src_frames[b] + seek[b] + j] : 0,   out fp16 [batch][n_mels][n_window].
 * src: DEVICE array of `batch` device pointers to fp16 [n_mels][src_frames[b]] (a null entry gives a zero row); src_frames, seek:
 * DEVICE int32 arrays (seek >= 0; any parity).  Everything per row is read on the device: one launch, no host synchronisation,
 * capturable.  Added under ABI 8 (an entry only; no struct changes). */
int wm_mel_windows(const void* const* src, const int32_t* src_frames, const int32_t* seek, int batch, int n_mels, int n_window,
                   void* out, wm_stream_t stream);
/* The probability a teacher-forced pass gives the token that follows, over the first `limit` entries of the vocabulary:
 *   out[b * out_ld + p] = exp(x[min(next[b * next_ld + p], limit - 1)] - logsumexp_{v < limit} x[v]),   x = logits + b * stride_b + p * stride_p
 * for b < batch, p < n_pos.  logits: fp16, strides in elements (stride_p >= n_vocab; rows may start at any 2-byte address); next:
 * DEVICE int32 (a negative entry reads x[0]); out: DEVICE fp32; 1 <= limit <= n_vocab.  The logits are read once, as fp16; sums are
 * fp32 and merged in a fixed order (the same bits on every run); a row whose logits below `limit` are all -inf gives 0.
 * Added under ABI 8 (an entry only; no struct changes). */
int wm_forced_probs(const void* logits, int batch, int n_pos, int n_vocab, int64_t stride_b, int64_t stride_p, int limit,
                    const int32_t* next, int next_ld, float* out, int out_ld, wm_stream_t stream);
/* Where to cut long files into sections that are decoded side by side (sections.py states the contract).
 * Per file b, in integers, with F = content[b] and x = src[b] fp16 [n_mels][src_ld[b]]:
 *   q[t] = sum_m rint(clamp(x[m][t], -16, 16) * 1024)   (half to even; a non-finite element contributes 0),   0 <= t < F
 *   s[t] = sum_{d = -h .. h} q[clamp(t + d, 0, F - 1)]
 *   c = 0; while F - c > hi: c = the t of [c + lo, c + hi] with the smallest s[t], the largest such t among equals; c is a cut.
 * cuts[b * cuts_ld + i] is the i-th cut of file b for i < min(n_cuts[b], cuts_ld); n_cuts[b] is the number of cuts FOUND, which
 * may exceed cuts_ld (nothing is written past cuts_ld: the caller compares).  src: DEVICE array of `batch` device pointers (a null
 * entry: a file without frames); src_ld, content: DEVICE int32 arrays, 0 <= content <= src_ld (content is clamped to that range);
 * rows may start at any 2-byte address.  total_frames: an upper bound on the sum of content; files are laid out in batch
 * order, and a file that has frames and whose last frame lies beyond total_frames in that order is not cut and reports
 * n_cuts = -1 (so does every later file with frames; a file without frames always reports 0).  Requires 1 <= lo <= hi, h >= 0
 * and n_mels * (2h + 1) < 131072 (every sum fits 32 bits, so the result does not depend on any order of summation).  The workspace (wm_section_cuts_workspace_bytes, 8-byte aligned) needs
 * no initialisation.  Asynchronous on `stream`: no allocation, no host synchronisation, capturable.
 * Added under ABI 8 (entries only; no struct changes). */
size_t wm_section_cuts_workspace_bytes(int batch, int64_t total_frames);
int wm_section_cuts(const void* const* src, const int32_t* src_ld, const int32_t* content, int batch, int n_mels, int lo, int hi,
                    int h, int32_t* cuts, int cuts_ld, int32_t* n_cuts, void* workspace, size_t workspace_bytes,
                    int64_t total_frames, wm_stream_t stream);
/* The speech of long files, so that the quiet stretches can be cut out before anything is decoded (speech.py states the contract;
 * DESIGN.md section 5j).  Per file b, in integers, with F = content[b], x = src[b] and q, s as in wm_section_cuts:
 *   floor = sorted(s)[min(F - 1, F * permille / 1000)]                                   (an exact order statistic)
 *   v[t]  = (int64)s[t] - floor >= n_mels * (2h + 1) * step
 *   spans = the maximal runs [a, b) of v; neighbours with a gap < min_silence joined; spans shorter than min_speech dropped; each
 *           widened to [max(0, a - pad), min(F, b + pad)) and joined where they now touch or overlap.
 * spans[(b * spans_ld + i) * 2 + {0, 1}] are the first frame and the end of span i of file b for i < n_spans[b].  The conventions are
 * wm_section_cuts': device arrays of pointers, strides and lengths; a null or empty file reports n_spans = 0; a file that has frames
 * and ends beyond total_frames, or that has more than spans_ld spans, reports n_spans = -1, and nothing is written outside a file's
 * spans_ld entries (with min_silence the spans number (F + min_silence) / (1 + min_silence) at most).  Requires 1 <= step <= 32768,
 * 0 <= permille <= 1000, min_silence >= 1, min_speech >= 1, pad >= 0, h >= 0 and n_mels * (2h + 1) < 131072.  The workspace
 * (wm_speech_spans_workspace_bytes, 8-byte aligned) needs no initialisation.  Asynchronous on `stream`: no allocation, no host
 * synchronisation, capturable.  Added under ABI 8 (entries only; no struct changes). */
size_t wm_speech_spans_workspace_bytes(int batch, int64_t total_frames);
int wm_speech_spans(const void* const* src, const int32_t* src_ld, const int32_t* content, int batch, int n_mels, int h, int step,
                    int permille, int min_silence, int min_speech, int pad, int32_t* spans, int spans_ld, int32_t* n_spans,
                    void* workspace, size_t workspace_bytes, int64_t total_frames, wm_stream_t stream);
/* The packed log-mels of a ragged batch, one launch for all files:
 *   dst[b][m * dst_ld[b] + p] = src[b][m * src_ld[b] + a_k + (p - P_k)]    for P_k <= p < P_k + (b_k - a_k), span k of file b
 *   dst[b][m * dst_ld[b] + P + j] = src[b][m * src_ld[b] + src_ld[b] - 1]  for j < n_pad, P the packed frames of the file
 * over the spans TAKEN from spans[(b * spans_ld + k) * 2 + {0, 1}], k < min(max(n_spans[b], 0), spans_ld): span k is taken if
 * 0 <= a_k < b_k <= src_ld[b] and a_k >= b_j for every earlier span j that lies in that range; any other span is skipped and never
 * dereferenced, and P_k counts the spans taken only.  Elements with p >= dst_ld[b] are not written; elements of dst that no rule
 * above names are left as they are.  src, dst: DEVICE arrays of `batch` device pointers (a null entry, src_ld < 1 or dst_ld < 1:
 * the file is skipped); src_ld, dst_ld, n_spans, spans: DEVICE int32.  Rows may start at any 2-byte address.  Asynchronous on
 * `stream`: no allocation, no host synchronisation, capturable.  Added under ABI 8 (an entry only; no struct changes). */
int wm_mel_gather(const void* const* src, const int32_t* src_ld, const int32_t* spans, const int32_t* n_spans, int spans_ld,
                  int batch, int n_mels, int n_pad, void* const* dst, const int32_t* dst_ld, wm_stream_t stream);
/* The loudest channel of every frame of multi-channel recordings, and the gate that silences a channel where another one is much
 * louder (channels.py states the contract).  The batch holds n_recordings recordings; recording r is the
 * adjacent channels first[r] .. first[r + 1] - 1 of the n_channels channels (first: DEVICE int32 [n_recordings + 1], ascending,
 * first[n_recordings] <= n_channels; 1 .. 8 channels each), every channel a whole-file log-mel src[c] fp16 [n_mels][src_ld[c]] with
 * content[c] frames, the channels of a recording equal in content and src_ld.  In integers, with q, s as in wm_section_cuts over
 * every channel:
 *   top[r][t]  = the lowest channel c (counted from first[r]) with s_c[t] = max_c' s_c'[t],              0 <= t < F
 *   and with step >= 1:   gated_c[t] = max_{c' != c} s_c'[t] - s_c[t] >= n_mels * (2h + 1) * step        (64-bit)
 *   v_c = the smallest finite element of src[c][:, :F] by the monotone integer key of its fp16 bits (-0 below +0); every bin of a
 *   gated frame of channel c is overwritten with v_c IN PLACE (columns at or beyond F are not touched; a channel without a finite
 *   element, and a recording of one channel, are never gated);  counts[c] = the gated frames of channel c (0 with step = 0).
 * n_top[r] = F; -1, and nothing written for it, for a recording that is not 1 .. 8 channels inside the batch, whose channels differ
 * in content or stride, or that has frames and whose last channel ends beyond total_frames in batch order (total_frames: an upper
 * bound on the sum of content over ALL channels).  top: DEVICE array of n_recordings device pointers to uint8 [>= F] (null: not
 * written); src, src_ld, content as in wm_section_cuts (a null channel has no frames); counts: DEVICE int32 [n_channels].
 * Requires 0 <= step <= 32768, h >= 0, n_mels * (2h + 1) < 131072.  The workspace (wm_channel_top_workspace_bytes, 8-byte aligned)
 * needs no initialisation.  One launch sequence for all recordings, asynchronous on `stream`: no allocation, no host
 * synchronisation, capturable.  Added under ABI 8 (entries only; no struct changes). */
size_t wm_channel_top_workspace_bytes(int n_channels, int64_t total_frames);
int wm_channel_top(void* const* src, const int32_t* src_ld, const int32_t* content, const int32_t* first, int n_recordings,
                   int n_channels, int n_mels, int h, int step, uint8_t* const* top, int32_t* n_top, int32_t* counts,
                   void* workspace, size_t workspace_bytes, int64_t total_frames, wm_stream_t stream);
/* zeroes rows 0 and Tpad - 1 of every utterance of buf fp16 [B][Tpad][C]. */
int wm_zero_pad_rows(void* buf, int B, int Tpad, int C, wm_stream_t stream);
/* ids[b] = arg-max of row b of fp16 logits (first index wins ties).  The decode loop itself uses
 * wm_greedy_step, which fuses this with Whisper's logit rules (apply_rules = 0: plain arg-max + append). */
int wm_argmax(const void* logits, int64_t row_stride, int batch, int n_vocab, int32_t* ids, wm_stream_t stream);
/* Weight-streaming GEMM, M <= 256, W in tile-linear layout (weight.py: tile_linear*).  w8: 0 = fp16
 * tiles, 1 = int8 tiles, 4 = packed int4 tiles (tile_linear_int4; K a multiple of 128).  `part` must
 * hold ksplit*M*n_blocks*16 floats; result[m][n] = sum_s part[s][m][n].  Replaces
 * weight_only_gemv_launcher (weightOnlyMatrixVectorMultiplication.cu:136-277,371-378).             */
int wm_gemm_skinny(const void* A, int lda, int M, int K, const void* Wt, int n_blocks, int w8,
                   const void* scale, int ksplit, float* part, wm_stream_t stream);
int wm_gemm_skinny_default_ksplit(int M, int K, int n_blocks, int w8);
/* One Linear of a SMALL decode batch (m <= 32 rows) in one launch -- what the decoder engine runs per projection at the
 * reference's own batch size of 1 (W/run.py:43-46): [LayerNorm of the input rows over k channels, eps 1e-5, when
 * ln_gamma is given] -> a . W^T (W as for wm_gemm_skinny, read once; K split over the waves of a workgroup, combined in
 * LDS) -> epilogue by `mode`:
 *   0  out32[row*ld32 + col] = the fp32 sums, scaled, without bias (the decode attention kernels add bias and round)
 *   1  out16 = fp16(gelu(fp16(y + bias)))                 (gelu_kind 1 erf, 2 tanh)
 *   2  x = fp16(x + fp16(y + bias)) in place              (residual stream)
 *   3  out16 = fp16(y), columns < n_valid                 (logits)
 * Replaces weight_only_gemv_launcher + bias / gelu / residual / LayerNorm layers (weightOnlyMatrixVectorMultiplication.cu:
 * 136-277,371-378; quantization/layer.py:311-312; functional.py:2044-2056; normalization.py:6-30).                      */
typedef struct wm_gemv_io {
    const void* a; int32_t lda, m, k;
    const void* wt; int32_t n_blocks, w8; const void* scale;
    const void* ln_gamma; const void* ln_beta;
    int32_t mode; const void* bias; int32_t gelu_kind;
    float* out32; int32_t ld32;
    void* out16; int32_t ld16, n_valid;
    void* x; int32_t ldx;
} wm_gemv_io;
int wm_gemv_fused(const wm_gemv_io* io, wm_stream_t stream);
/* Decoder calls with batch * n_new <= rows activation rows take the fused small-batch path (wm_gemv_fused per Linear);
 * default 16 (or WM_SMALL_PATH; 8 until the end of round 3), 0 = never, at most 32.  Returns the previous value.  A row's result does not depend on
 * the batch it is in on either side of the switch (one more boundary on both sides: groups of fewer than 160 (utterance, head)
 * pairs -- 8 utterances of large-v2 -- cut the cross-attention's key range into 4 pieces and merge the partial softmaxes,
 * larger ones run the exact single pass; across that boundary a row's context agrees to fp32 summation order); across the
 * switch the two paths agree to fp32 summation order (a last-bit
 * difference of fp16 values in rare cases).  Captured graphs keep the path they were captured with.                    */
int wm_set_small_batch_rows(int rows);
/* The same Linear (same wm_gemv_io, modes 0-2, optional LayerNorm prologue) for ANY number of rows m: the rows are split over
 * workgroups (16 or 32 rows x 64 channels each, the whole k per wave, the input block in LDS by DMA), so a row's sums never
 * leave the accumulators and there are neither fp32 slabs nor a row kernel.  k <= 1536.  What decoder calls with more rows
 * than the small-batch switch run for every projection whose input is n_state wide (csrc/gemm_rows.hip); replaces the same
 * reference code as wm_gemv_fused (the small-M branch of WeightOnlyQuantMatmulPlugin::enqueue,
 * weightOnlyQuantMatmulPlugin.cpp:182-197, + the element-wise layers around it).  A row's result does not depend on m or on
 * the row's position.                                                                                                      */
int wm_gemm_rows(const wm_gemv_io* io, wm_stream_t stream);
/* Decoder calls with at least min_rows activation rows (and more than the small-batch switch) use wm_gemm_rows where it
 * applies; default 40 (WM_ROWS_MIN), 0 (or WM_ROWS_PATH=0) = never: the split-K chain (wm_gemm_skinny + row kernel) for every
 * Linear, as rounds 1-2 did.  Returns the previous value.  On either side of the switch a row's result does not depend on the
 * batch it is in; across it the two forms agree to fp32 summation order.  Captured graphs keep the path they were captured with. */
int wm_set_rows_path(int min_rows);
/* Waves per (utterance, head) of the decode self-attention (wm_attn_decode_self and the decoder step): 0 (default, or
 * WM_SELF_WAVES) = by size -- calls on the small-batch side of wm_set_small_batch_rows' switch run four waves per head (key
 * range dealt over the waves, the cache read in one round trip), larger ones one wave per head; 1 or 4 = that form for every
 * size.  Returns the previous value.  The two forms round at the same points and add the softmax sum and P.V in different fp32
 * orders; the cache they append is identical.  Captured graphs keep the form they were captured with.                       */
int wm_set_self_attn_waves(int waves);
/* The MFMA-bound GEMMs (encoder layers, convolutions, cross-K/V projection; wm_gemm, wm_conv1d_gelu) pick their tile by the
 * size of the launch: with fewer than `tiles` 256 x 256 output tiles (default 150: one to four clips of large-v2, by shape) the launch
 * runs 128 x 128 tiles, two workgroups per CU (64 x 128 when even those would leave a third of the CUs idle: one clip's
 * n_state-wide projections), else the persistent 256 x 256 kernel.  0 = never the small form, < 0 = the
 * default.  Returns the previous value.  Both forms add an output element's products in the same order and share the
 * epilogue arithmetic: the results are bit-identical, a clip's encoder output does not depend on the batch it is in.     */
int wm_set_gemm_small_tiles(int tiles);
/* Batch 1 to 8 (one new token for each of up to eight utterances; batch 1 is the reference's own operating point, W/run.py:43-46;
 * 4-bit weights: one or two utterances): the decoder's kernels run as STAGES of one
 * launch (csrc/gemv_chain.hip: the stages hand the activation row over as tagged 8-byte granules -- no fences, no flags, no
 * barriers between workgroups; a stage's weights are requested before its input is waited for).  Same arithmetic as one launch
 * per kernel, bit for bit.  Modes:
 *   0  a launch per fused Linear and per attention kernel (9 per layer)
 *   1  a decoder layer as ONE launch: self-attention (cache append included), out + residual, LayerNorm + cross-attention q,
 *      the cross-attention over four key-range pieces (K / V rows by DMA into LDS while the stages before it run), the merge of
 *      the pieces + cross-attention out + residual, LayerNorm + mlp1 + GELU, mlp2 + residual, LayerNorm + qkv of the next layer
 *   2  the launch walks over the layers itself: ONE launch per token step besides the embedding and the vocabulary
 *      projection (default).  The per-layer cross K/V and cache pointers reach it through a table in the workspace.
 *      Rows: one and two utterances keep their cross-attention K / V pieces in LDS (requested a layer ahead); three to eight keep them in
 *      registers, requested at the head of the stage, two (row, head, piece) items per workgroup.  `live_rows` is honoured: a finished
 *      row's attention stages read nothing and append nothing to its cache.  A row's result is the launch-per-kernel path's, bit for bit.
 * Both need the in-place cache (past[i] == present[i], equal capacities <= 512), fp16 cross K/V and <= 32 layers for mode 2, and
 * a step that runs alone (wm_decoder_step, or wm_decoder_step_multi with one group: the launch needs all of its workgroups
 * resident together -- one per CU: do not issue such a step on a stream whose CU mask leaves it fewer CUs than the device has,
 * use mode 0 there); a call that does not qualify takes the launch-per-kernel path.
 * < 0 = default; returns the previous value.  Captured graphs keep the form they were captured with.
 * Robustness.  The launch's workgroups wait for each other, so they must be resident together.  The library therefore takes the
 * one-launch forms only when (a) a workgroup's footprint -- static + dynamic LDS and registers, from the function's attributes -- fits a
 * CU and the grid is no larger than the device's CUs (checked once per device and kernel variant; the runtime's occupancy call is
 * reported beside it but not trusted alone: ROCm 7.2's answers 0 for a footprint that runs), (b) the stream of the call owns every CU (a stream created with a CU mask that
 * leaves it fewer -- wm_stream_create_cu_mask, hipExtStreamCreateWithCUMask -- takes the launch-per-kernel path) and (c) no earlier
 * launch on the device has given up.  Every wait inside the launch is bounded (about a second): a wave that gives up sets a word in
 * pinned host memory and the rest of the launch falls through.
 * wm_decode_chain_error: *out != 0 when a workgroup of a chain gave up a wait since the last call -- the results of that step and of
 * everything decoded from it are NOT valid (another tenant held CUs or LDS while the launch was dispatched).  The call does not
 * synchronise (the word lives in host memory): ask after waiting for the steps in question, e.g. after reading their logits.  It
 * clears the word and takes the device off the one-launch forms (wm_set_decode_chain re-arms it): decode the
 * utterance again, it now runs a launch per kernel (WhisperDecoding.main_loop / detect_language do exactly that, with one warning).
 * Until it has been called, every wm_decoder_step / wm_decoder_step_multi on that device returns 1 (wm_last_error says why) -- a
 * caller that never looks cannot go on decoding from garbage.  (Calls under stream capture are exempt: they enqueue nothing.)
 * wm_decode_chain_status: what the calling thread's device has done so far (tests, diagnostics).                               */
typedef struct wm_chain_status {
    int32_t mode;               /* wm_set_decode_chain's current value */
    int32_t declined;           /* 1: the device is off the one-launch forms (a launch gave up, or the occupancy check said no) */
    int32_t error_pending;      /* 1: a give-up nobody has acknowledged yet */
    int32_t pad_;
    int64_t launches;           /* one-launch steps / layers issued (or captured) on this device */
    int64_t declined_calls;     /* decoder calls that qualified by shape but took the launch-per-kernel path for reasons (a)-(c) */
    char reason[200];           /* why the device is declined, or why the last residency check said no ("" otherwise) */
    char footprint[200];        /* the last residency check in words: LDS and registers of a workgroup against a CU's, the runtime's own figure */
} wm_chain_status;
int wm_set_decode_chain(int on);
int wm_decode_chain_error(int* out);
int wm_decode_chain_status(wm_chain_status* out);
/* Diagnostic: `n_workgroups` one-wave workgroups that each hold `lds_bytes` of LDS and sleep for `microseconds` on `stream` (a tenant
 * that keeps CUs' LDS busy: tests/test_gpu_round5.py provokes the give-up path of the one-launch step with it).                 */
int wm_debug_occupy(int n_workgroups, size_t lds_bytes, int64_t microseconds, wm_stream_t stream);
/* Exact V-row skipping in the decode cross-attention (fp16 K/V, single-pass form): a key whose softmax probability rounds to
 * fp16 zero contributes exactly nothing to P.V, so the wave instructions whose 8 rows all weigh zero do not fetch them from
 * HBM (they re-read 8 rows the workgroup has just used).  Outputs are bit-identical with it on or off for finite V
 * (tests/test_gpu_round4.py::test_cross_attention_v_skip_*, tests/test_gpu_attn_decode_contract.py).  1 = on
 * (default), 0 = off, < 0 = the default.  Returns the previous value.  Captured graphs keep the form they were captured with. */
int wm_set_cross_v_skip(int on);
/* Lab knobs (environment variables such as WM_CROSS_NSPLIT, WM_ROWS_MIN, WM_KSPLIT_CAP: DESIGN.md, scripts/README.md) change a
 * schedule or the order of fp32 sums for A/B runs.  They are honoured ONLY when WM_LAB=1 is set as well; every knob honoured by
 * this process is logged once on stderr and listed here as "NAME=value;..." (returns the length of the full list; buf may be
 * NULL).  Without WM_LAB=1 a set knob is ignored with one warning on stderr.                                                */
int wm_lab_knobs(char* buf, size_t cap);
/* fp16 LayerNorm rows, fp32 statistics, eps 1e-5 (layernormKernels.cu:62-188). */
int wm_layernorm(const void* x, int ldx, int M, int N, const void* gamma, const void* beta,
                 void* out, int ldo, wm_stream_t stream);
/* qkv fp16 [B*T, 3*H*64] with q and k pre-multiplied by 64^-0.25; out fp16 [B*T, H*64]. */
int wm_attn_encoder(const void* qkv, int ld, int B, int T, int H, void* out, int ldo, wm_stream_t stream);
/* Decode cross-attention: q fp32 [B*L, H*64] (un-scaled, bias included), kv fp16 [B,2,H,Tk,64].
 * nsplit = 1: one workgroup per (utterance, head), exact two-pass softmax.  1 < nsplit <= 16: the key range is cut into nsplit
 * pieces (ws: >= B*H*nsplit*L*66 floats) and the partial softmaxes are merged; nsplit > 16 is an error.                      */
int wm_attn_decode_cross(const float* q, int B, int L, int H, int Tk, const void* kv, void* out,
                         int nsplit, float* ws, wm_stream_t stream);
/* the same with int8 K/V codes [B,2,H,Tk,64] and one scale (value = fp16(code) * kv_scale, rounded to fp16) */
int wm_attn_decode_cross_i8(const float* q, int B, int L, int H, int Tk, const void* kv_i8, float kv_scale,
                            void* out, int nsplit, float* ws, wm_stream_t stream);
/* Decode self-attention with append: qkv fp32 [B*L, 3*H*64] (bias included); cache [B,2,H,cap,64]. */
int wm_attn_decode_self(const float* qkv, int B, int L, int T, int H, const void* past, int past_cap,
                        void* present, int present_cap, int int8_kv, float kv_scale, void* out,
                        wm_stream_t stream);
/* The same in place (past == present == cache, capacity cap) with right-aligned rows and / or a live-row list, as wm_decoder_step
 * launches it: row_start int32 [B] or NULL (wm_decoder_io::row_start), live_rows int32 [1 + B] or NULL (wm_decoder_io::live_rows:
 * rows not listed are neither read nor written).  L <= 4.                                                                          */
/* Kernel-level test entries of the block prefill (csrc/attn_prefill.hip), fp32 rows in, like wm_attn_decode_self / _cross.
 * self: qkv fp32 [B * L, 3 * H * 64] on an empty cache [B, 2, H, cap, 64] (appended in place: slots 0 .. L - 1), out fp16 [B * L, H * 64];
 * cross: q fp32 [B * L, H * 64] over kv fp16 [B, 2, H, Tk, 64].  row_start int32 [B] or NULL, live_rows int32 [1 + B] or NULL. */
int wm_attn_prefill_self(const float* qkv, int B, int L, int H, void* cache, int cap, int int8_kv, float kv_scale, void* out,
                         const int32_t* row_start, const int32_t* live_rows, wm_stream_t stream);
int wm_attn_prefill_cross(const float* q, int B, int L, int H, int Tk, const void* kv, void* out, const int32_t* live_rows,
                          wm_stream_t stream);
int wm_attn_decode_self_rows(const float* qkv, int B, int L, int T, int H, void* cache, int cap, int int8_kv, float kv_scale,
                             void* out, const int32_t* row_start, const int32_t* live_rows, wm_stream_t stream);
/* q = sat_s8(rne(x * inv_scale)) (quantizeTensorPlugin / attention.py:340-348). */
int wm_quantize_i8(const void* x, void* q, int64_t n, float inv_scale, wm_stream_t stream);

/* ---- audio front end ----------------------------------------------------------------
 * log_mel_spectrogram (W/whisper_utils.py:99-146) for a batch of equally long clips already padded /
 * trimmed by the caller (pad_or_trim, W/whisper_utils.py:56-81): audio fp32 [batch][audio_ld], 16 kHz,
 * n_samples a multiple of 160; filters fp32 [n_mels][201] (the mel_filters.npz matrix,
 * W/whisper_utils.py:84-96).  Writes n_frames = n_samples / 160 frames per clip as fp16 and/or fp32
 * [batch][n_mels][n_frames] (either pointer may be NULL); the max - 8 clamp is taken per clip. */
size_t wm_log_mel_workspace_bytes(int batch, int n_samples, int n_mels);
int wm_log_mel(const float* audio, int batch, int n_samples, int64_t audio_ld, const float* filters,
               int n_mels, void* mel_f16, float* mel_f32, void* workspace, size_t workspace_bytes,
               wm_stream_t stream);

/* Resampler of the front end (the `-ar 16000 -ac 1` of the reference's ffmpeg call, W/whisper_utils.py:17-54): interleaved PCM
 * pcm [n_in][channels] on the device (dtype 0: float32, 1: int16, 2: int32; 1..8 channels) -> out fp32 [n_out], mono, at L / M
 * times the input rate, n_out = ceil(n_in L / M).  The downmix is fused into the staging of the input:
 *   x[k] = (fp32(v[k][0]) + fp32(v[k][1]) + ...  in channel order, in fp32) / fp32(channels) * scale
 * (scale: 2^-(bits - 1) for integer PCM, 1 for float), and with i = floor(n M / L), p = (n M) mod L, T = 2 half + 1
 *   out[n] = sum_{j = 0 .. T - 1} H[p][j] * x[i - half + j]     fp32 FMAs in tap order, x zero outside [0, n_in):
 * no delay, output n sits at input time n M / L; deterministic.  `table` is the DEVICE copy of H, transposed and ordered by
 * r = n mod L:  table[j * L + r] = H[(r M) mod L][j], fp32 [T][L] (whisper_utils.resample_filter states H; resample_device builds
 * this layout).  All arithmetic on n M is 64-bit.  rc 1 without a launch: a null pointer, channels outside 1..8, an unknown dtype,
 * L == M, L / M / half < 1, n_in < 1, n_out != ceil(n_in L / M), or a ratio whose tile does not fit LDS (M / L above ~14).
 * Added under ABI 8 (an entry only; no struct changes). */
int wm_resample(const void* pcm, int dtype, int channels, int64_t n_in, float scale, const float* table, int L, int M, int half,
                float* out, int64_t n_out, wm_stream_t stream);
/* The channel form of wm_resample (channels.py, rule 1): out fp32 [channels][out_ld], row c the first n_out
 * elements of which are channel c of the input at the new rate -- the staging selects the channel instead of summing,
 *   x_c[k] = fp32(v[k][c]) * scale,
 * and everything else is wm_resample's: row c equals, bit for bit, wm_resample of a mono input that holds channel c.  All channels
 * in one launch; elements n_out .. out_ld - 1 of a row are not written.  rc 1 without a launch: what wm_resample refuses, and
 * out_ld < n_out.  Added under ABI 8 (an entry only; no struct changes). */
int wm_resample_channels(const void* pcm, int dtype, int channels, int64_t n_in, float scale, const float* table, int L, int M,
                         int half, float* out, int64_t out_ld, int64_t n_out, wm_stream_t stream);

/* FLAC decoder (host code, no GPU needed): replaces the ffmpeg subprocess of load_audio
 * (W/whisper_utils.py:17-54) for the LibriSpeech .flac files.  wm_flac_decode writes interleaved
 * int32 samples [n][channels]; frame CRC-8 / CRC-16 are verified, `md5` is the STREAMINFO signature of
 * the PCM (little-endian, ceil(bits/8) bytes per sample) for the caller to check. */
typedef struct wm_flac_streaminfo {
    int32_t sample_rate;
    int32_t channels;
    int32_t bits_per_sample;
    int32_t max_block_size;
    int64_t total_samples;      /* per channel; 0 = unknown */
    uint8_t md5[16];
} wm_flac_streaminfo;
int wm_flac_info(const void* data, size_t bytes, wm_flac_streaminfo* info);
int wm_flac_decode(const void* data, size_t bytes, int32_t* pcm, int64_t capacity_samples,
                   int64_t* n_decoded);

/* ---- in-situ timing of the dominant decode kernel (cross-attention), for the roofline report ------
 * When enabled, wm_decoder_step brackets the cross-attention launch of every `layer_stride`-th layer
 * with a HIP event pair on the launch stream, up to `max_samples` pairs.  wm_profile_read waits for
 * the recorded events and returns the summed duration and the number of samples.  Process-global,
 * off by default, not thread-safe (one host thread per GPU).                                        */
int wm_profile_configure(int enabled, int layer_stride, int max_samples);
int wm_profile_read(double* total_ms, int64_t* count, int reset);
/* Diagnostic: a device-side timeline of the decode step.  `buf` = int64 [1 + 3 * capacity] device words (NULL switches it
 * off): word 0 counts entries, entry i = {group tag (the step's logits pointer), 2 * layer + (0 = before, 1 = after the
 * cross-attention launch), wall clock (100 MHz)}, written by 1-thread kernels on the step's stream (graph-capturable; each
 * costs a launch, so the timeline perturbs what it shows by a few us per layer).  scripts/timeline_probe.py draws it. */
int wm_debug_timeline(void* buf, int capacity);

#ifdef __cplusplus
}
#endif
#endif /* WHISPER_MI355_H */
