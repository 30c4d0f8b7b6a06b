"""Block prefill on the GPU: wm_decoder_prefill (a whole start block in one pass, csrc/attn_prefill.hip) and
WhisperDecoding(block_prefill=True).  DESIGN.md section 5f.

* Engine (micro-fullvocab, L0 = 227), fp16 KV, int8 KV (scales 0.05) and weight-only int8: five right-aligned rows with prompts of
  0, 1, 2, 3 and 223 tokens through wm_decoder_prefill with logits_from = sot_index, then 4 single-token wm_decoder_step calls on the
  cache the prefill left.  Every row is compared with the CPU oracle over the row alone, un-padded, FED WHOLE in one decoder call
  (the block attends to itself un-quantised, as upstream does): logits at <|sot|>, at the last position and at every step, bounds
  LOGIT_TOL / LOGIT_TOL_INT8_KV.  Positions below logits_from keep a sentinel.
* tiny shape (384 wide, 6 heads, 1500 audio positions): B = 2, L = 227 against the oracle.
* Refusals: rc 1 with a message, nothing launched.
* main_loop on a row_prompts + block_prefill instance against the oracle's greedy decode of every row (a case whose smallest top-two
  margin is above 2 x the bound under both cache types: every token must match), with graphs (the second batch replays the
  prefill) and without; closed rows; shared cross K/V with beam search; options.prompt on a plain instance.
"""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_refs as KR  # noqa: E402
import native  # noqa: E402
import prompt_refs as PR  # noqa: E402
import synthetic  # noqa: E402
from decoding import DecodingOptions, WhisperDecoding, right_aligned_rows, row_prompt_layout  # noqa: E402
from encoding import WhisperEncoding  # noqa: E402
from oracle.whisper_oracle import Dims, OracleConfig, OracleModel, synthetic_mel, synthetic_state_dict  # noqa: E402
from test_gpu_model import LOGIT_TOL, LOGIT_TOL_INT8_KV, build_engine  # noqa: E402

CAP = 448
KV_SCALE = 0.05
SENT = KR.SENTINEL


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return native.load_library()


@pytest.fixture(scope="module")
def tmpdir_module(tmp_path_factory):
    return str(tmp_path_factory.mktemp("engines"))


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(autouse=True)
def leave_nothing_behind():
    yield
    gc.collect()
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------- engine
PROMPT_LENGTHS = [0, 1, 2, 3, 223]
N_STEPS = 4


@pytest.mark.parametrize("weight_only,int8_kv", [(False, False), (False, True), (True, False)])
def test_block_prefill_rows_match_the_oracle_fed_whole(lib, tmpdir_module, weight_only, int8_kv):
    dims = Dims(**synthetic.DIMS["micro-fullvocab"])
    sd = synthetic_state_dict(dims, 3)
    n = len(PROMPT_LENGTHS)
    mel = synthetic_mel(n, 2 * dims.n_audio_ctx, dims.n_mels, 4242)
    scales = [KV_SCALE] * dims.n_text_layer if int8_kv else None
    tol = LOGIT_TOL_INT8_KV if int8_kv else LOGIT_TOL
    eng = build_engine(tmpdir_module, "micro-fullvocab", 3, weight_only=weight_only, int8_kv=int8_kv, kv_scales=scales)
    enc, dec = WhisperEncoding(eng), WhisperDecoding(eng, row_prompts=True)
    tk = dec.tokenizer
    L0, sot_index, _ = row_prompt_layout(dims.n_text_ctx, tk.sot_sequence, tk.sot)
    assert L0 == 227 and dec.sot_index == sot_index
    r = KR.philox(11)
    prompts = [[int(t) for t in r.integers(0, 50000, size=k)] for k in PROMPT_LENGTHS]
    rows, starts = right_aligned_rows(prompts, tk.sot_sequence, tk.sot_prev, dims.n_text_ctx)

    oracle = OracleModel(dims, sd, OracleConfig(act="float16", weight_only=weight_only, int8_kv=int8_kv, kv_scales=scales))
    ckv = oracle.cross_kv(oracle.encoder(mel))
    ref_logits, ref_ids = [], []
    for b in range(n):
        ckv_b = [t[b:b + 1] for t in ckv]
        logits, kv = oracle.decoder(torch.tensor([rows[b][starts[b]:]], dtype=torch.long), ckv_b, None)     # the row WHOLE, one call
        logits = logits[0]
        per_step, ids = [logits[-1]], []
        for _ in range(N_STEPS):
            ids.append(int(per_step[-1].argmax()))
            lg, kv = oracle.decoder(torch.tensor([[ids[-1]]]), ckv_b, kv)
            per_step.append(lg[0, 0])
        ref_logits.append((logits[sot_index - starts[b]], per_step))
        ref_ids.append(ids)

    xa = enc.get_audio_features(mel.cuda())
    st = dec._fast_state(n, xa.device)
    cross = dec._cross_persistent(xa, st)
    tokens = torch.zeros((n, CAP + 1), dtype=torch.int32, device="cuda")
    tokens[:, :L0] = torch.tensor(rows, dtype=torch.int32)
    tokens[:, L0:L0 + N_STEPS] = torch.tensor(ref_ids, dtype=torch.int32)
    row_start = torch.tensor(starts, dtype=torch.int32, device="cuda")
    sess, pos, V = dec.decoder_session, dec.positional_embedding, dims.n_vocab
    st['logits'].fill_(SENT)
    sess.decoder_prefill(tokens[:, :L0], pos[0:L0], cross, st['kv'], CAP, st['logits'], stream(), sot_index, row_start=row_start)
    torch.cuda.synchronize()
    assert bool((st['logits'][:, :sot_index] == SENT).all()), "a position below logits_from was written"
    got = st['logits'][:, sot_index:].float().cpu()
    assert torch.isfinite(got).all()
    worst_sot = max(float((got[b, 0] - ref_logits[b][0]).abs().max()) for b in range(n))
    worst = [max(float((got[b, L0 - 1 - sot_index] - ref_logits[b][1][0]).abs().max()) for b in range(n))]
    step_logits = torch.empty((n, 1, V), dtype=torch.float16, device="cuda")
    for s in range(N_STEPS):
        cur = L0 + s
        sess.decoder_step(tokens[:, cur:cur + 1], pos[cur:cur + 1], cross, st['kv'], CAP, st['kv'], CAP, step_logits, cur, stream(),
                          row_start=row_start)
        torch.cuda.synchronize()
        g = step_logits[:, 0].float().cpu()
        worst.append(max(float((g[b] - ref_logits[b][1][s + 1]).abs().max()) for b in range(n)))
    print(f"block prefill vs oracle fed whole (weight_only={weight_only}, int8_kv={int8_kv}): max |dlogit| at <|sot|> {worst_sot:.4g}, "
          f"last position and {N_STEPS} steps {[round(w, 4) for w in worst]} (bound {tol})")
    assert worst_sot < tol and max(worst) < tol


def test_block_prefill_at_tiny_shape(lib, tmpdir_module):
    dims = Dims(**synthetic.DIMS["tiny"])
    eng = build_engine(tmpdir_module, "tiny", 5)
    enc, dec = WhisperEncoding(eng), WhisperDecoding(eng)
    Bn, L = 2, 227
    mel = synthetic_mel(Bn, 2 * dims.n_audio_ctx, dims.n_mels, 3)
    r = KR.philox(21)
    rows = torch.from_numpy(r.integers(0, 50000, size=(Bn, L))).to(torch.int32)
    oracle = OracleModel(dims, synthetic_state_dict(dims, 5), OracleConfig(act="float16"))
    ckv = oracle.cross_kv(oracle.encoder(mel))
    want, _ = oracle.decoder(rows.long(), ckv, None)
    xa = enc.get_audio_features(mel.cuda())
    cross = dec.xa2cross_key_value(xa)
    kv = [torch.zeros((Bn, 2, dims.n_text_head, CAP, 64), dtype=torch.float16, device="cuda") for _ in range(dims.n_text_layer)]
    logits = torch.full((Bn, L, dims.n_vocab), SENT, dtype=torch.float16, device="cuda")
    frm = L - 3
    dec.decoder_session.decoder_prefill(rows.cuda(), dec.positional_embedding[0:L], cross, kv, CAP, logits, stream(), frm)
    torch.cuda.synchronize()
    assert bool((logits[:, :frm] == SENT).all())
    worst = float((logits[:, frm:].float().cpu() - want[:, frm:]).abs().max())
    print(f"block prefill at tiny shape: max |dlogit| over the last 3 positions {worst:.4g} (bound {LOGIT_TOL})")
    assert worst < LOGIT_TOL


def test_block_prefill_refusals(lib, tmpdir_module):
    """Every refusal of the list: rc 1, a message, and nothing launched (logits and cache keep their sentinels)."""
    dims = Dims(**synthetic.DIMS["micro-fullvocab"])
    eng = build_engine(tmpdir_module, "micro-fullvocab", 3)
    dec = WhisperDecoding(eng)
    sess, pos = dec.decoder_session, dec.positional_embedding
    Bn, L = 2, 9
    cross = [torch.zeros((Bn, 2, dims.n_text_head, dims.n_audio_ctx, 64), dtype=torch.float16, device="cuda") for _ in range(dims.n_text_layer)]
    kv = [torch.full((Bn, 2, dims.n_text_head, CAP, 64), SENT, dtype=torch.float16, device="cuda") for _ in range(dims.n_text_layer)]
    made = []                                        # every logits buffer handed to a call: [Bn, L, V] and a guard row behind it
    tokens = torch.zeros((Bn, dims.n_text_ctx + 1), dtype=torch.int32, device="cuda")
    word = torch.zeros(4, dtype=torch.float32, device="cuda")

    def pio(L=L, logits_from=0, cap=CAP):
        p = native.WmPrefillIO()
        flat = torch.full((Bn * L * dims.n_vocab + dims.n_vocab,), SENT, dtype=torch.float16, device="cuda")
        made.append(flat)
        p.io = sess.make_decoder_io(tokens[:, :L], pos[0:min(L, dims.n_text_ctx)], cross, None, 0, kv, cap, flat[:Bn * L * dims.n_vocab].view(Bn, L, -1), 0,
                                    prefill=L <= dims.n_text_ctx)
        p.logits_from = logits_from
        p._keep = p.io
        return p

    def refused(p, match):
        rc = lib.wm_decoder_prefill(sess.engine.handle, C.byref(p), stream())
        msg = lib.wm_last_error().decode()
        assert rc == 1 and match in msg, (rc, msg)

    p = pio(); p.io.n_past = 1
    refused(p, "n_past")
    p = pio(); p.io.n_past_dev = word.data_ptr()
    refused(p, "n_past_dev")
    p = pio(); p.io.qkv_amax = word.data_ptr()
    refused(p, "qkv_amax")
    p = pio(); p.io.present = None
    refused(p, "present")
    refused(pio(cap=L - 1), "capacity")
    refused(pio(L=dims.n_text_ctx + 1), "n_text_ctx")
    refused(pio(logits_from=-1), "logits_from")
    refused(pio(logits_from=L), "logits_from")
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in made) and all(bool((t == SENT).all()) for t in kv), "a refused call launched something"
    # ... and the call they all were but for one field goes through
    native.check(lib.wm_decoder_prefill(sess.engine.handle, C.byref(pio()), stream()), "wm_decoder_prefill")
    torch.cuda.synchronize()
    n_out = Bn * L * dims.n_vocab
    assert torch.isfinite(made[-1][:n_out].float()).all() and not bool((made[-1][:n_out] == SENT).any()) and bool((made[-1][n_out:] == SENT).all())
    assert all(bool((t[:, :, :, L:] == SENT).all()) and not bool((t[:, :, :, :L] == SENT).any()) for t in kv)


def test_block_prefill_refuses_int8_cross_kv(lib, tmpdir_module):
    dims = Dims(**synthetic.DIMS["micro-fullvocab"])
    eng = build_engine(tmpdir_module, "micro-fullvocab", 3, cross_scales=[0.05] * dims.n_text_layer)
    with pytest.raises(ValueError, match="int8 cross K/V"):
        WhisperDecoding(eng, block_prefill=True)
    dec = WhisperDecoding(eng)
    sess = dec.decoder_session
    Bn, L = 1, 9
    cross = [torch.zeros((Bn, 2, dims.n_text_head, dims.n_audio_ctx, 64), dtype=torch.int8, device="cuda") for _ in range(dims.n_text_layer)]
    kv = [torch.zeros((Bn, 2, dims.n_text_head, CAP, 64), dtype=torch.float16, device="cuda") for _ in range(dims.n_text_layer)]
    logits = torch.full((Bn, L, dims.n_vocab), SENT, dtype=torch.float16, device="cuda")
    with pytest.raises(native.WmError, match="int8 cross K/V"):
        sess.decoder_prefill(torch.zeros((Bn, L), dtype=torch.int32, device="cuda"), dec.positional_embedding[0:L], cross, kv, CAP, logits, stream(), 0)
    torch.cuda.synchronize()
    assert bool((logits == SENT).all())


# --------------------------------------------------------------------------------------------------------- main_loop
# The case was chosen on the CPU oracle: with these prompt lengths, mel seed 9000 + 54, prompts philox(500 + 54) and state seed 3 the
# oracle's greedy decode (every row fed whole on its first step) leaves every row's smallest top-two margin over the 4 steps at
# >= 0.125 with an fp16 cache and >= 0.137 with an int8 cache (scales 0.05): above 2 x the bound (0.06 / 0.12) under both, so no row
# is excused -- all 8 x 4 tokens must be the oracle's.  The fixture recomputes the margins and fails if one falls below 2 x the bound.
LOOP_LENGTHS = [0, 1, 2, 3, 223, 5, 60, 130]
LOOP_SEED = 54
SAMPLE_LEN = 4


def sampled(tokens, begin, eot, n=SAMPLE_LEN):
    out = [r[begin:begin + n] for r in tokens.cpu().tolist()]
    return [r + [eot] * (n - len(r)) for r in out]


@pytest.fixture(scope="module")
def loop_case(lib, tmpdir_module):
    import oracle.decoding_rules as DR
    dims = Dims(**synthetic.DIMS["micro-fullvocab"])
    n = len(LOOP_LENGTHS)
    mel = synthetic_mel(n, 2 * dims.n_audio_ctx, dims.n_mels, 9000 + LOOP_SEED)
    r = KR.philox(500 + LOOP_SEED)
    prompts = [[int(t) for t in r.integers(0, 50000, size=k)] for k in LOOP_LENGTHS]
    scales = [KV_SCALE] * dims.n_text_layer
    engines = {False: build_engine(tmpdir_module, "micro-fullvocab", 3), True: build_engine(tmpdir_module, "micro-fullvocab", 3, int8_kv=True, kv_scales=scales)}
    enc = WhisperEncoding(engines[False])
    xa = enc.get_audio_features(mel.cuda())
    plain = WhisperDecoding(engines[False], only_torch=True)
    tk = plain.tokenizer
    rows, starts = right_aligned_rows(prompts, tk.sot_sequence, tk.sot_prev, dims.n_text_ctx)
    sd = synthetic_state_dict(dims, 3)
    cpu_tokens, cpu_margins = {}, {}
    for int8_kv in (False, True):
        tol = LOGIT_TOL_INT8_KV if int8_kv else LOGIT_TOL
        oracle = OracleModel(dims, sd, OracleConfig(act="float16", int8_kv=int8_kv, kv_scales=scales if int8_kv else None))
        ckv = oracle.cross_kv(oracle.encoder(mel))
        cpu_tokens[int8_kv], cpu_margins[int8_kv] = [], []
        for b in range(n):
            row = rows[b][starts[b]:]
            rules = DR.RuleSet(DR.MULTILINGUAL, len(row), list(plain._get_suppress_tokens()), list(tk.blank_tokens()) + [tk.eot],
                               plain.max_initial_timestamp_index)
            toks, margins = PR.oracle_greedy_row(oracle, [t[b:b + 1] for t in ckv], row, rules, SAMPLE_LEN)
            cpu_tokens[int8_kv].append(toks + [tk.eot] * (SAMPLE_LEN - len(toks)))
            cpu_margins[int8_kv].append(min(margins))
        print(f"CPU oracle (int8_kv={int8_kv}): smallest top-two margins per row {[round(m, 3) for m in cpu_margins[int8_kv]]} (2 x bound = {2 * tol})")
        assert min(cpu_margins[int8_kv]) >= 2 * tol, "the case no longer keeps every row's margin above twice the bound"
    yield dict(dims=dims, engines=engines, xa=xa, prompts=prompts, tk=tk, cpu_tokens=cpu_tokens, cpu_margins=cpu_margins)
    gc.collect()
    torch.cuda.synchronize()


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("int8_kv", [False, True])
def test_main_loop_with_block_prefill_decodes_the_oracles_tokens(lib, loop_case, int8_kv, graphs):
    c = loop_case
    dec = WhisperDecoding(c["engines"][int8_kv], row_prompts=True, block_prefill=True, options=DecodingOptions(sample_len=SAMPLE_LEN))
    dec.use_graphs = graphs
    dec.set_prompts(c["prompts"])
    sess = dec.decoder_session
    calls = {"prefill": 0}
    real_prefill = sess.decoder_prefill

    def counting_prefill(*a, **k):
        calls["prefill"] += 1
        return real_prefill(*a, **k)

    sess.decoder_prefill = counting_prefill
    runs, per_call = [], []
    for _ in range(2 if graphs else 1):
        before = calls["prefill"]
        t, lp, nsp = dec.main_loop(c["xa"])
        per_call.append(calls["prefill"] - before)
        runs.append(sampled(t, dec.sample_begin, c["tk"].eot))
    if graphs:
        # the first batch issues the prefill eagerly and captures it; the second replays the graph: no call reaches the session
        assert per_call[0] >= 1 and per_call[1] == 0, per_call
        st = next(iter(dec._state.values()))
        assert any('prefill' in key for key in st['graphs'])
        assert runs[0] == runs[1]
    else:
        assert per_call[0] >= 1
    assert native.chain_status()["error_pending"] is False
    assert runs[-1] == c["cpu_tokens"][int8_kv], (runs[-1], c["cpu_tokens"][int8_kv], c["cpu_margins"][int8_kv])


def test_main_loop_with_block_prefill_and_closed_rows(lib, loop_case):
    c = loop_case
    n = len(c["prompts"])
    dec = WhisperDecoding(c["engines"][False], row_prompts=True, block_prefill=True, options=DecodingOptions(sample_len=SAMPLE_LEN))
    dec.set_prompts(c["prompts"])
    closed = (1, 4, 7)
    limit = torch.tensor([0 if b in closed else 1 << 30 for b in range(n)], dtype=torch.int32)
    t, lp, nsp = dec.main_loop(c["xa"], row_limit=limit)
    got = sampled(t, dec.sample_begin, c["tk"].eot)
    for b in range(n):
        if b in closed:
            assert got[b] == [c["tk"].eot] * SAMPLE_LEN and float(lp[b]) == 0.0
        else:
            assert got[b] == c["cpu_tokens"][False][b], b
    # the CU-partitioned schedule is refused (cu_partition is an attribute set after construction, so the loop refuses it)
    dec.cu_partition = True
    with pytest.raises(ValueError, match="block_prefill is not supported by the CU-partitioned schedule"):
        dec.main_loop(c["xa"])
    dec.cu_partition = False


def test_shared_cross_kv_beam_search_with_block_prefill(lib, loop_case):
    """One shared_cross_kv, beam_size = 2 run over the 8 prompts against every utterance alone on the same kind of instance (the
    shared-cross-K/V branch prefills one row per utterance and copies it to the candidates).  A row may differ only at a step where
    the CPU oracle's margin is below 2 x LOGIT_TOL, and at most one row in eight does."""
    c = loop_case
    n, K = len(c["prompts"]), 2
    opts = dict(sample_len=SAMPLE_LEN, beam_size=K)
    dec = WhisperDecoding(c["engines"][False], row_prompts=True, block_prefill=True, shared_cross_kv=True, options=DecodingOptions(**opts))
    dec.set_prompts(c["prompts"])
    t, lp, nsp = dec.main_loop(c["xa"])
    got = dec.post_process(t, lp, nsp, c["xa"], ["en"] * n)
    one = WhisperDecoding(c["engines"][False], row_prompts=True, block_prefill=True, shared_cross_kv=True, options=DecodingOptions(**opts))
    dropped = []
    for b in range(n):
        xa_b = c["xa"][b:b + 1].contiguous()
        one.set_prompts([c["prompts"][b]])
        want = one.post_process(*one.main_loop(xa_b), xa_b, ["en"])[0]
        if got[b].tokens != want.tokens:
            assert c["cpu_margins"][False][b] < 2 * LOGIT_TOL, (b, got[b].tokens, want.tokens)
            dropped.append(b)
    assert len(dropped) <= n // 8, dropped
    assert any(len(r.tokens) > 0 for r in got)


def test_options_prompt_on_a_plain_instance_with_block_prefill(lib, loop_case):
    """options.prompt of 60 tokens: a start block of 64 tokens shared by the batch, left-aligned (no row_start)."""
    import oracle.decoding_rules as DR
    c = loop_case
    dims, tk = c["dims"], c["tk"]
    prompt = c["prompts"][6]
    assert len(prompt) == 60
    dec = WhisperDecoding(c["engines"][False], block_prefill=True, options=DecodingOptions(prompt=prompt, sample_len=SAMPLE_LEN))
    assert dec.sample_begin == 64
    xa = c["xa"][:3].contiguous()
    got = sampled(dec.main_loop(xa)[0], dec.sample_begin, tk.eot)
    mel = synthetic_mel(len(LOOP_LENGTHS), 2 * dims.n_audio_ctx, dims.n_mels, 9000 + LOOP_SEED)[:3]
    oracle = OracleModel(dims, synthetic_state_dict(dims, 3), OracleConfig(act="float16"))
    ckv = oracle.cross_kv(oracle.encoder(mel))
    row = list(dec.initial_tokens)
    excused = 0
    for b in range(3):
        rules = DR.RuleSet(DR.MULTILINGUAL, len(row), list(dec._get_suppress_tokens()), list(tk.blank_tokens()) + [tk.eot], dec.max_initial_timestamp_index)
        toks, margins = PR.oracle_greedy_row(oracle, [t[b:b + 1] for t in ckv], row, rules, SAMPLE_LEN)
        toks = toks + [tk.eot] * (SAMPLE_LEN - len(toks))
        if got[b] != toks:
            k = next(i for i in range(SAMPLE_LEN) if got[b][i] != toks[i])
            assert margins[k] < 2 * LOGIT_TOL, (b, k, got[b], toks, margins)
            excused += 1
    assert excused <= 1
