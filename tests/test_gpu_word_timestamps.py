"""Word-level timestamps on a real MI355X (csrc/align.hip behind wm_dtw, wm_align, wm_decoder_step_tap; DESIGN.md "word
timestamps"): the DTW walk against timing.dtw_cpu exactly, the alignment matrix against an fp64 restatement within 4x the error
of the same restatement in fp32, the tapped cross-attention queries against the oracle's, and WhisperDecoding.word_timestamps
end to end against the PyTorch statement.

Measured on MI355X (printed by the tests):
  matrix stage, B = 3 / three heads:      max |GPU - fp64| 5.29e-07, fp32 numpy restatement 1.35e-06 (bound 5.41e-06)
  matrix stage, 225 tokens x 1500 frames: max |GPU - fp64| 1.29e-06, fp32 numpy restatement 3.22e-06 (bound 1.29e-05)
  tapped q against the oracle's query:    fp16 8.54e-03, weight-only int8 1.05e-02 (bound 3e-2, tests/test_gpu_model.py)
  tapped q, split-K form (three slabs) against the fused form: 4.39e-03
  end to end, two clips: DTW margins on the reference path 0.0645 / 0.0965 (matrix bounds 1.9e-06 / 2.1e-06), max |device
  matrix - torch matrix| 6.26e-03 / 6.73e-03; both clips' device times and paths equal the torch path's
"""
import ctypes as C
import os
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import build as B  # noqa: E402
import native  # noqa: E402
import synthetic  # noqa: E402
import timing  # noqa: E402
import torch_model as TM  # noqa: E402
from decoding import DecodingOptions, WhisperDecoding  # noqa: E402
from encoding import WhisperEncoding  # noqa: E402
from oracle.whisper_oracle import Dims, OracleConfig, OracleModel, synthetic_mel, synthetic_state_dict  # noqa: E402
from test_gpu_model import LOGIT_TOL, build_engine  # noqa: E402  (the project's teacher-forced bound and its engine builder)


@pytest.fixture(scope="module")
def tmpdir_module(tmp_path_factory):
    return str(tmp_path_factory.mktemp("wt_engines"))


# ---- wm_dtw -------------------------------------------------------------------------------------------------------------
def run_dtw(xs):
    """wm_dtw on a (ragged) batch of fp32 matrices -> [(text_indices, time_indices)] and the raw outputs."""
    lib = native.load_library()
    Bn = len(xs)
    R, Cc = max(x.shape[0] for x in xs), max(x.shape[1] for x in xs)
    ld = Cc + 3
    buf = torch.full((Bn, R, ld), 1e30, dtype=torch.float32)
    for b, x in enumerate(xs):
        buf[b, :x.shape[0], :x.shape[1]] = torch.from_numpy(x)
    buf = buf.cuda()
    n_rows = torch.tensor([x.shape[0] for x in xs], dtype=torch.int32).cuda()
    n_cols = torch.tensor([x.shape[1] for x in xs], dtype=torch.int32).cuda()
    path_ld = R + Cc
    pt = torch.full((Bn, path_ld), -7, dtype=torch.int32).cuda()
    pf = torch.full((Bn, path_ld), -7, dtype=torch.int32).cuda()
    pl = torch.full((Bn,), -7, dtype=torch.int32).cuda()
    ws = torch.empty(lib.wm_dtw_workspace_bytes(Bn, R, Cc), dtype=torch.uint8).cuda()
    native.check(lib.wm_dtw(buf.data_ptr(), ld, R * ld, Bn, n_rows.data_ptr(), n_cols.data_ptr(), R, Cc, pt.data_ptr(), pf.data_ptr(),
                            path_ld, pl.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "wm_dtw")
    torch.cuda.synchronize()
    pt, pf, pl = pt.cpu().numpy(), pf.cpu().numpy(), pl.cpu().tolist()
    return [(pt[b, :pl[b]], pf[b, :pl[b]]) for b in range(Bn)], (pt, pf, pl)


def dtw_inputs(kind, N, M, seed):
    rng = np.random.default_rng(seed)
    if kind == "ties":
        return rng.integers(-2, 3, size=(N, M)).astype(np.float32)
    return rng.standard_normal((N, M)).astype(np.float32)


@pytest.mark.parametrize("kind", ["random", "ties"])
@pytest.mark.parametrize("N,M", [(1, 1), (1, 7), (5, 1), (7, 40), (33, 100), (225, 1500)])
def test_dtw_equals_dtw_cpu(kind, N, M):
    x = dtw_inputs(kind, N, M, 100 * N + M)
    (got,), (pt, pf, pl) = run_dtw([x])
    ti, fi = timing.dtw_cpu(x)
    assert pl[0] == len(ti) and got[0].tolist() == ti.tolist() and got[1].tolist() == fi.tolist()
    assert (pt[0, pl[0]:] == -7).all() and (pf[0, pl[0]:] == -7).all()          # nothing past the path


@pytest.mark.parametrize("kind", ["random", "ties"])
def test_dtw_ragged_batch(kind):
    xs = [dtw_inputs(kind, n, m, 7 + n) for n, m in ((9, 61), (1, 5), (30, 17))]
    got, (_, _, pl) = run_dtw(xs)
    for x, (gt, gf), n in zip(xs, got, pl):
        ti, fi = timing.dtw_cpu(x)
        assert n == len(ti) and gt.tolist() == ti.tolist() and gf.tolist() == fi.tolist()


# ---- wm_align: the matrix stage ---------------------------------------------------------------------------------------------
def r16(a):
    return a.astype(np.float16)


def matrix_reference(tape, cross, heads, H, n_tok, F, n_prefix, dtype):
    """Steps 3-7 of the contract in numpy at `dtype` for one utterance: q16 / k16 rounded as specified, everything after the
    dot product in `dtype`.  Returns (Mtx[n_prefix : n_tok - 1], smallest column std / mean over the heads)."""
    s = np.float32(64 ** -0.25)
    total = np.zeros((n_tok, F), dtype=dtype)
    spread = np.inf
    for slot, hd in enumerate(heads):
        q16 = r16(tape[slot, :n_tok].astype(np.float32) * s).astype(dtype)
        k16 = r16(cross[hd // H][0, hd % H, :F].astype(np.float32) * s).astype(dtype)
        S = q16 @ k16.T
        e = np.exp(S - S.max(axis=1, keepdims=True))
        W = e / e.sum(axis=1, keepdims=True)
        mean = W.mean(axis=0, keepdims=True)
        std = np.sqrt(((W - mean) ** 2).mean(axis=0, keepdims=True))
        spread = min(spread, float((std / mean).min()))
        Z = np.where(std > 0, (W - mean) / np.where(std > 0, std, 1), 0).astype(dtype)
        if F > 3:
            Zp = np.pad(Z, ((0, 0), (3, 3)), mode="reflect")
            Z = np.sort(np.lib.stride_tricks.sliding_window_view(Zp, 7, axis=1), axis=-1)[..., 3]
        total = total + Z
    mtx = total / dtype(len(heads))
    return mtx[n_prefix: n_tok - 1], spread


def run_align(tape, cross, heads, H, Tk, n_tokens, n_frames, n_prefix, cap, want_matrix=True, engine=None):
    """tape fp16 [B, nh, cap, 64], cross: per layer fp16 [B, 2, H, Tk, 64] (cuda tensors).  Returns (matrix with guards, paths)."""
    lib = native.load_library()
    Bn, nh = tape.shape[0], len(heads)
    ld = Tk + 4
    matrix = torch.full((Bn, cap, ld), 777.0, dtype=torch.float32).cuda()
    path_ld = cap + Tk
    pt = torch.full((Bn, path_ld), -7, dtype=torch.int32).cuda()
    pf = torch.full((Bn, path_ld), -7, dtype=torch.int32).cuda()
    pl = torch.full((Bn,), -7, dtype=torch.int32).cuda()
    nt = torch.tensor(n_tokens, dtype=torch.int32).cuda()
    nf = torch.tensor(n_frames, dtype=torch.int32).cuda()
    ws = torch.empty(lib.wm_align_workspace_bytes(Bn, nh, cap, Tk), dtype=torch.uint8).cuda()
    io = native.align_io(engine, H, Tk, tape, cross, heads, nt, nf, n_prefix, 7, cap, matrix if want_matrix else None, ld, pt, pf, pl, ws)
    rc = lib.wm_align(C.byref(io), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, matrix.cpu().numpy(), pt.cpu().numpy(), pf.cpu().numpy(), pl.cpu().tolist()


def align_case(Bn, n_layers, H, heads, cap, Tk, n_tokens, n_frames, n_prefix, seed, gain=4.0):
    g = torch.Generator().manual_seed(seed)
    tape = (torch.randn(Bn, len(heads), cap, 64, generator=g) * gain).half()
    cross = [torch.randn(Bn, 2, H, Tk, 64, generator=g).half() for _ in range(n_layers)]
    rc, mtx, pt, pf, pl = run_align(tape.cuda(), [c.cuda() for c in cross], heads, H, Tk, n_tokens, n_frames, n_prefix, cap)
    assert rc == 0, native.load_library().wm_last_error()
    tape_n, cross_n = tape.numpy(), [c.numpy() for c in cross]
    worst_gpu, worst_f32 = 0.0, 0.0
    for b in range(Bn):
        N, F = n_tokens[b] - n_prefix - 1, n_frames[b]
        ref64, spread = matrix_reference(tape_n[b], [c[b] for c in cross_n], heads, H, n_tokens[b], F, n_prefix, np.float64)
        ref32, _ = matrix_reference(tape_n[b], [c[b] for c in cross_n], heads, H, n_tokens[b], F, n_prefix, np.float32)
        assert spread > 1e-3, spread                        # every column's std over the tokens: the z-score amplifies no noise
        worst_gpu = max(worst_gpu, float(np.abs(mtx[b, :N, :F] - ref64).max()))
        worst_f32 = max(worst_f32, float(np.abs(ref32.astype(np.float64) - ref64).max()))
        # storage: rows beyond the matrix, frames beyond F and the padding of every row are untouched
        assert (mtx[b, N:] == 777.0).all() and (mtx[b, :, F:] == 777.0).all()
        # the kernel's own path is dtw_cpu of the kernel's own matrix
        ti, fi = timing.dtw_cpu(-mtx[b, :N, :F])
        assert pl[b] == len(ti) and pt[b, :pl[b]].tolist() == ti.tolist() and pf[b, :pl[b]].tolist() == fi.tolist()
        assert (pt[b, pl[b]:] == -7).all() and (pf[b, pl[b]:] == -7).all()
    return worst_gpu, worst_f32


def test_align_matrix_three_heads_ragged():
    """B = 3, three heads over two layers (H = 2), cap 16, n_tokens [6, 16, 9], n_prefix 3, Tk = 100 with n_frames [100, 93, 3]: a
    tile edge (100 = 3 x 32 + 4), a ragged tail and the no-filter rule (F <= 3)."""
    worst_gpu, worst_f32 = align_case(3, 2, 2, [0, 2, 3], 16, 100, [6, 16, 9], [100, 93, 3], 3, seed=11)
    print(f"align matrix B=3: max |GPU - fp64| = {worst_gpu:.3g}, fp32 numpy restatement = {worst_f32:.3g}, bound = {4 * worst_f32:.3g}")
    assert worst_gpu <= 4 * worst_f32, (worst_gpu, worst_f32)


def test_align_matrix_one_head_full_size():
    """One head, 225 tokens x 1500 frames (more than one wave's rows per tile, 47 frame tiles)."""
    worst_gpu, worst_f32 = align_case(1, 1, 1, [0], 225, 1500, [225], [1500], 3, seed=12)
    print(f"align matrix 225 x 1500: max |GPU - fp64| = {worst_gpu:.3g}, fp32 numpy restatement = {worst_f32:.3g}, bound = {4 * worst_f32:.3g}")
    assert worst_gpu <= 4 * worst_f32, (worst_gpu, worst_f32)


def test_align_rows_without_tokens_or_frames_and_the_workspace_matrix():
    g = torch.Generator().manual_seed(5)
    tape = (torch.randn(3, 1, 8, 64, generator=g) * 4).half().cuda()
    cross = [torch.randn(3, 2, 1, 40, 64, generator=g).half().cuda()]
    rc, mtx, pt, pf, pl = run_align(tape, cross, [0], 1, 40, [4, 8, 8], [40, 0, 40], 3, 8)
    assert rc == 0 and pl[0] == 0 and pl[1] == 0 and pl[2] > 0                 # n_tokens - n_prefix - 1 < 1; n_frames < 1
    assert (mtx[:2] == 777.0).all()
    rc2, mtx2, pt2, pf2, pl2 = run_align(tape, cross, [0], 1, 40, [4, 8, 8], [40, 0, 40], 3, 8, want_matrix=False)
    assert rc2 == 0 and pl2 == pl and (pt2 == pt).all() and (pf2 == pf).all() and (mtx2 == 777.0).all()


# ---- wm_decoder_step_tap ------------------------------------------------------------------------------------------------------
def drive(sess, dec, tokens, cross, cap, chunks, tap=None, heads_arr=None):
    """The forced sequence through wm_decoder_step (not_alone = 1) or wm_decoder_step_tap in `chunks`: (logits per call, caches)."""
    Bn = tokens.shape[0]
    d = sess.dims
    kv = [torch.zeros((Bn, 2, d["n_text_head"], cap, 64), dtype=torch.float16, device="cuda") for _ in range(d["n_text_layer"])]
    stream = torch.cuda.current_stream().cuda_stream
    out, off = [], 0
    for l in chunks:
        lg = torch.zeros((Bn, l, d["n_vocab"]), dtype=torch.float16, device="cuda")
        args = (tokens[:, off:off + l], dec.positional_embedding[off:off + l], cross, kv if off else None, cap, kv, cap, lg, off, stream)
        if tap is None:
            sess.decoder_step(*args, not_alone=True)
        else:
            sess.decoder_step_tap(*args, tap, heads_arr)
        out.append(lg)
        off += l
    torch.cuda.synchronize()
    return out, kv


def oracle_cross_queries(oracle, mel, tokens):
    """The oracle's cross-attention query of every layer for the same tokens (a spy on OracleModel._linear, as
    kv_amax_on_token_path does): per layer [B, L, C]."""
    seen = []
    orig = oracle._linear

    def spy(x, wkey, bkey=None):
        y = orig(x, wkey, bkey)
        if wkey.endswith("cross_attn.query.weight"):
            seen.append(y.clone())
        return y
    oracle._linear = spy
    try:
        with torch.no_grad():
            oracle.decoder(tokens, oracle.cross_kv(oracle.encoder(mel)), None)
    finally:
        oracle._linear = orig
    return seen


@pytest.mark.parametrize("weight_only", [False, True])
def test_tap_is_bit_identical_and_matches_the_oracle_query(tmpdir_module, weight_only):
    """micro engine, B = 3, 11 forced tokens as 4 + 4 + 3: logits and the appended cache are wm_decoder_step's (not_alone = 1) bit
    for bit, and the tapped q is the oracle's cross-attention query within the teacher-forced bound of tests/test_gpu_model.py
    (3e-2; q is an activation of the same pass).  Measured maxima: fp16 8.54e-03, weight-only int8 1.05e-02."""
    dims = Dims(**synthetic.DIMS["micro"])
    eng = build_engine(tmpdir_module, "micro", 7, weight_only)
    enc, dec = WhisperEncoding(eng), WhisperDecoding(eng)
    sess = dec.decoder_session
    mel = synthetic_mel(3, 2 * dims.n_audio_ctx, dims.n_mels, 21)
    cross = dec.xa2cross_key_value(enc.get_audio_features(mel.cuda()))
    tokens = torch.randint(0, dims.n_vocab, (3, 11), generator=torch.Generator().manual_seed(4), dtype=torch.int32).cuda()
    heads = [0, 1, 3]                                                   # layer 0 both heads, layer 1 head 1
    heads_arr = (C.c_int32 * len(heads))(*heads)
    cap = dims.n_text_ctx
    tape = torch.full((3, len(heads), 16, 64), 99.0, dtype=torch.float16, device="cuda")
    plain, kv_plain = drive(sess, dec, tokens, cross, cap, (4, 4, 3))
    tapped, kv_tap = drive(sess, dec, tokens, cross, cap, (4, 4, 3), tape, heads_arr)
    assert all(torch.equal(a, b) for a, b in zip(plain, tapped)) and all(torch.equal(a, b) for a, b in zip(kv_plain, kv_tap))
    assert bool((tape[:, :, 11:] == 99.0).all())                         # rows n_past .. n_past + n_new only
    sd = synthetic_state_dict(dims, 7)
    oracle = OracleModel(dims, sd, OracleConfig(act="float16", weight_only=weight_only))
    q = oracle_cross_queries(oracle, mel, tokens.cpu().long())
    worst = 0.0
    for slot, hd in enumerate(heads):
        want = q[hd // dims.n_text_head][:, :, 64 * (hd % dims.n_text_head): 64 * (hd % dims.n_text_head) + 64]
        worst = max(worst, float((tape[:, slot, :11].float().cpu() - want.float()).abs().max()))
    print(f"tapped q vs the oracle's cross-attention query (weight_only={weight_only}): max |diff| = {worst:.3g}, bound {LOGIT_TOL}")
    assert worst < LOGIT_TOL, worst


def test_tap_of_the_split_k_form(tmpdir_module):
    """B = 20 rows x 4 tokens on the split-K chain (wm_set_rows_path(0): wm_gemm_skinny slabs + row kernels for every Linear) of a
    384-wide toy, where the cross-attention query arrives as three slabs (cq_ks = 3): logits and cache bit-identical to
    wm_decoder_step again, and the tape of rows 0 .. 2 agrees with a B = 3 run (the fused small-batch form, one slab)
    to the teacher-forced bound -- the two forms add the same products in another order."""
    lib = native.load_library()
    dd = dict(n_mels=80, n_audio_ctx=64, n_audio_state=384, n_audio_head=6, n_audio_layer=1, n_vocab=1024, n_text_ctx=32,
              n_text_state=384, n_text_head=6, n_text_layer=2)
    dims = Dims(**dd)
    out = os.path.join(tmpdir_module, "eng_wide")
    B.build_from_checkpoint({"dims": dd, "model_state_dict": synthetic_state_dict(dims, 9)},
                            B.parse_arguments(["--output_dir", out, "--use_gpt_attention_plugin", "--use_gemm_plugin", "--use_layernorm_plugin", "--log_level", "error"]))
    assert lib.wm_gemm_skinny_default_ksplit(80, 384, 24, 0) > 1
    enc, dec = WhisperEncoding(Path(out)), WhisperDecoding(Path(out))
    sess = dec.decoder_session
    mel = synthetic_mel(20, 2 * dims.n_audio_ctx, dims.n_mels, 22)
    cross = dec.xa2cross_key_value(enc.get_audio_features(mel.cuda()))
    tokens = torch.randint(0, dims.n_vocab, (20, 11), generator=torch.Generator().manual_seed(6), dtype=torch.int32).cuda()
    heads = [1, 6, 11]
    heads_arr = (C.c_int32 * len(heads))(*heads)
    tape = torch.zeros((20, len(heads), 11, 64), dtype=torch.float16, device="cuda")
    prev = lib.wm_set_rows_path(0)
    try:
        plain, kv_plain = drive(sess, dec, tokens, cross, dims.n_text_ctx, (4, 4, 3))
        tapped, kv_tap = drive(sess, dec, tokens, cross, dims.n_text_ctx, (4, 4, 3), tape, heads_arr)
    finally:
        lib.wm_set_rows_path(prev)
    assert all(torch.equal(a, b) for a, b in zip(plain, tapped)) and all(torch.equal(a, b) for a, b in zip(kv_plain, kv_tap))
    tape3 = torch.zeros((3, len(heads), 11, 64), dtype=torch.float16, device="cuda")
    drive(sess, dec, tokens[:3], [c[:3] for c in cross], dims.n_text_ctx, (4, 4, 3), tape3, heads_arr)
    worst = float((tape[:3].float() - tape3.float()).abs().max())
    print(f"tapped q, split-K form vs fused form: max |diff| = {worst:.3g}")
    assert worst < LOGIT_TOL and float(tape.float().abs().max()) > 0.1


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def dtw_margin(x, ti, fi):
    """The smallest gap, along the path, between the predecessor step 8 chose and the best one it turned down."""
    x = np.asarray(x, dtype=np.float32)
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    cost[0, 0] = 0
    for j in range(1, M + 1):
        for i in range(1, N + 1):
            cost[i, j] = x[i - 1, j - 1] + min(cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1])
    worst = np.inf
    for a, b in zip(ti, fi):
        c = sorted([cost[a, b], cost[a, b + 1], cost[a + 1, b]])
        if np.isfinite(c[1]):
            worst = min(worst, float(c[1] - c[0]))
    return worst


def test_word_timestamps_end_to_end(tmpdir_module):
    """micro-fullvocab + the bundled vocabulary, B = 2, ragged num_frames: detect_language -> main_loop -> post_process ->
    word_timestamps."""
    dims = Dims(**synthetic.DIMS["micro-fullvocab"])
    eng = build_engine(tmpdir_module, "micro-fullvocab", 3)
    enc, dec = WhisperEncoding(eng), WhisperDecoding(eng)
    assert dec.tokenizer.bpe is not None
    dec.sample_len = 12
    dec.keep_alignment_matrix = True
    mel = synthetic_mel(2, 2 * dims.n_audio_ctx, dims.n_mels, 77)
    xa = enc.get_audio_features(mel.cuda())
    languages, _ = dec.detect_language(xa)
    t, lp, nsp = dec.main_loop(xa)
    results = dec.post_process(t, lp, nsp, xa, languages)
    frames = [2 * dims.n_audio_ctx, 2 * 45 + 1]
    words = dec.word_timestamps(xa, results, frames)
    dev = dec.last_alignment
    # the forced pass leaves main_loop's results reproducible
    t2, lp2, _ = dec.main_loop(xa)
    assert torch.equal(t, t2) and torch.equal(lp, lp2) and dec._decode_in_flight == 0
    assert dec.word_timestamps(xa, results, frames) == words
    # the PyTorch statement on the same features
    sd = synthetic_state_dict(dims, 3)
    model = TM.Whisper(TM.ModelDimensions(**dims.to_dict())).load_state_dict({k: v.float() for k, v in sd.items()})
    ref_dec = WhisperDecoding(eng, only_torch=True)
    ref = ref_dec.torch_word_timestamps(model, xa.float().cpu(), results, frames)
    tor = ref_dec.last_alignment
    assert any(len(w) > 0 for w in words)
    tk, n_prefix, spf = dec.tokenizer, len(dec.tokenizer.sot_sequence), 30.0 / dims.n_audio_ctx
    compared = 0
    for b in range(2):
        assert [(w.word, w.tokens) for w in words[b]] == [(w.word, w.tokens) for w in ref[b]]
        if not words[b]:
            continue
        n = dev["path_len"][b]
        text = [x for x in results[b].tokens if x < tk.eot]
        ws, wt = dec._split_words(text + [tk.eot], results[b].language)
        own = timing.words_from_path(dev["path_text"][b, :n], dev["path_time"][b, :n], ws, wt,
                                     dev["token_probs"][b, n_prefix: n_prefix + len(text)].tolist(), spf)
        assert [(w.start, w.end) for w in own] == [(w.start, w.end) for w in words[b]]
        assert all(0 <= w.start <= w.end <= (frames[b] // 2) * spf + 1e-9 for w in words[b])
        assert np.allclose([w.probability for w in words[b]], [w.probability for w in ref[b]], atol=LOGIT_TOL)
        # where the reference matrix's path is unambiguous, the times are the torch path's
        S64 = [s.double().numpy() for s in tor[b]["scores"]]
        m32 = tor[b]["matrix"].numpy()
        tot = np.zeros(S64[0].shape)
        for S in S64:
            e = np.exp(S - S.max(axis=1, keepdims=True))
            Wm = e / e.sum(axis=1, keepdims=True)
            mu, sdv = Wm.mean(0, keepdims=True), Wm.std(0, keepdims=True)
            Z = np.where(sdv > 0, (Wm - mu) / np.where(sdv > 0, sdv, 1), 0)
            if Z.shape[1] > 3:
                Z = np.sort(np.lib.stride_tricks.sliding_window_view(np.pad(Z, ((0, 0), (3, 3)), mode="reflect"), 7, axis=1), axis=-1)[..., 3]
            tot += Z
        m64 = (tot / len(S64))[n_prefix: tot.shape[0] - 1]
        bound = 4 * float(np.abs(m32 - m64).max())
        margin = dtw_margin(-m32, tor[b]["path_text"], tor[b]["path_time"])
        d_dev = float(np.abs(dev["matrix"][b, :m32.shape[0], :m32.shape[1]].numpy() - m32).max())
        print(f"utterance {b}: matrix bound {bound:.3g}, smallest DTW margin on the reference path {margin:.3g}, "
              f"max |device matrix - torch matrix| {d_dev:.3g}")
        if margin > 2 * bound:
            assert [(w.start, w.end) for w in words[b]] == [(w.start, w.end) for w in ref[b]]
            assert dev["path_text"][b, :n].tolist() == tor[b]["path_text"].tolist() and dev["path_time"][b, :n].tolist() == tor[b]["path_time"].tolist()
            compared += 1
        else:
            print(f"utterance {b}: the synthetic clip's DTW path is ambiguous (margin {margin:.3g} <= 2 x {bound:.3g}); "
                  f"device path {dev['path_time'][b, :n].tolist()}, torch path {tor[b]['path_time'].tolist()}: times not compared")
    # this fixture's paths ARE unambiguous (measured: margins 0.0645 and 0.0965 against bounds of 1.9e-06 and 2.1e-06; the device
    # matrix within 6.3e-03 / 6.7e-03 of the torch one): the comparison above must have run, on real engine cross K/V, through the tap
    assert compared >= 1


def test_word_timestamps_refuses_int8_cross_kv_and_beams(tmpdir_module):
    dims = Dims(**synthetic.DIMS["micro-fullvocab"])
    mel = synthetic_mel(2, 2 * dims.n_audio_ctx, dims.n_mels, 77)
    eng = build_engine(tmpdir_module, "micro-fullvocab", 3)
    enc = WhisperEncoding(eng)
    xa = enc.get_audio_features(mel.cuda())
    beam = WhisperDecoding(eng, options=DecodingOptions(beam_size=2, sample_len=4))
    with pytest.raises(ValueError, match="beam_size"):
        beam.word_timestamps(xa, [[440, 7], [9001]])
    eng8 = build_engine(tmpdir_module, "micro-fullvocab", 3, cross_scales=[0.05] * dims.n_text_layer)
    dec8 = WhisperDecoding(eng8)
    assert dec8.use_int8_cross_kv
    with pytest.raises(native.WmError, match="int8"):
        dec8.word_timestamps(xa, [[440, 7], [9001]])
    # the library itself refuses such an engine: rc 1 and a message that says why
    tape = torch.zeros((1, 1, 8, 64), dtype=torch.float16, device="cuda")
    cross = [torch.zeros((1, 2, dims.n_text_head, dims.n_audio_ctx, 64), dtype=torch.float16, device="cuda") for _ in range(dims.n_text_layer)]
    rc, *_ = run_align(tape, cross, [0], dims.n_text_head, dims.n_audio_ctx, [8], [10], 3, 8, engine=dec8.decoder_session.engine.handle)
    assert rc == 1 and b"int8" in native.load_library().wm_last_error()
