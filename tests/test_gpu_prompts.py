"""Right-aligned rows on the GPU: a prompt per row (wm_decoder_io::row_start, WhisperDecoding(row_prompts=True), transcribe's
condition_on_previous_text / initial_prompt).  DESIGN.md section 5f.

* Kernel, L = 1 (the decode step).  A row that begins at slot s of its cache must run EXACTLY the arithmetic of an un-padded row
  with T - s cached tokens: output and appended cache row are compared BIT FOR BIT with the row_start == NULL launch over the
  compacted cache, for both wave forms and both cache types, starts {0, 1, 63, 64, 65} x lengths {0, 1, 63, 64, 65, 130}, with and
  without a live-row list (rows off the list keep their sentinels).  The pad slots hold NaN (fp16) / -128 (int8).
* Kernel, L = 4 (a prefill pass), starts = 0, 1, 2, 3 (mod 4), passes wholly in front of a row's start, wholly behind it, and
  across it: against prompt_refs.self_attn_rows_ref (fp32, slot numbers only), bound 1.5e-3 = the bound of
  tests/test_gpu_kernels.py::test_attn_decode_self; pad queries give exact zeros; every token's k / v is appended.
* Engine (micro-fullvocab: L0 = 227 crosses 64, 128 and 192 keys), fp16 and int8 KV: a batch of 5 right-aligned rows with prompts
  of 0, 1, 2, 3 and 223 tokens against the CPU oracle over each row alone and un-padded, LOGIT_TOL / LOGIT_TOL_INT8_KV.
* main_loop with set_prompts against every row decoded alone through the shared-prompt instance (greedy with and without graphs,
  closed rows, beam search, best_of) and transcribe() with conditioning against longform.transcribe_reference over single-row calls:
  further down, each with its own note.

Measured on MI355X (printed by the tests): the L = 1 comparisons are bitwise; 4-token passes: max |out - ref| 4.9e-4 (four-wave form,
fp16 cache, T = 68; 0 or 1.2e-7 elsewhere; bound 1.5e-3); engine rows against the oracle: fp16 KV 0.0078 at <|sot|>, 0.0091 at the
last position and over 4 steps (bound 0.03), int8 KV 0.021 / 0.033 (bound 0.06); greedy loop: no row of the eight parted ways with
the row decoded alone (the CPU reference has one near-tie row, margin 0.027); best_of: booked sum_logprobs within 1.5e-6 of the
teacher-forced sums (bound 0.48).
"""
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

SELF_ATTN_TOL = 1.5e-3        # tests/test_gpu_kernels.py::test_attn_decode_self
CAP = 448
T_SCALE = 0.031


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
    """The decoder instances of a test hold captured graphs and device buffers, and some of them sit in reference cycles: they are
    collected HERE, at the end of the test that made them, not at some later allocation inside another module's test -- destroying
    a graph or returning memory synchronises the device, which a test that times tenants against each other
    (tests/test_gpu_round5.py: a step that gives up) must not meet half way."""
    yield
    gc.collect()
    torch.cuda.synchronize()


def self_rows(lib, qkv, B, L, T, H, cache, int8_kv, out, row_start, live, waves):
    prev = lib.wm_set_self_attn_waves(waves)
    try:
        native.check(lib.wm_attn_decode_self_rows(qkv.data_ptr(), B, L, T, H, cache.data_ptr(), cache.shape[3], int8_kv, T_SCALE,
                                                  out.data_ptr(), None if row_start is None else row_start.data_ptr(),
                                                  None if live is None else live.data_ptr(), stream()), "wm_attn_decode_self_rows")
        torch.cuda.synchronize()
    finally:
        lib.wm_set_self_attn_waves(prev)


def random_cache(r, B, H, n, int8_kv):
    """[B, 2, H, n, 64] of real content: fp16 values or int8 codes."""
    if int8_kv:
        return torch.from_numpy(r.integers(-127, 128, size=(B, 2, H, n, 64), dtype=np.int8))
    return torch.from_numpy((r.standard_normal((B, 2, H, n, 64)) * 1.2).astype(np.float16))


def pad_fill(int8_kv):
    return -128 if int8_kv else float("nan")


# --------------------------------------------------------------------------------------------------------- kernel, L = 1
STARTS = [0, 1, 63, 64, 65]
LENGTHS = [0, 1, 63, 64, 65, 130]


@pytest.mark.parametrize("use_live", [False, True])
@pytest.mark.parametrize("int8_kv", [0, 1])
@pytest.mark.parametrize("waves", [1, 4])
def test_decode_step_row_is_bit_identical_to_the_unpadded_row(lib, waves, int8_kv, use_live):
    """Three rows per launch at T = start + length: row 0 begins at `start`, row 1 at 0 (nothing padded: the RS instantiation must
    agree with the plain one there too), row 2 at T (an empty history: the new token attends to itself).  With a live list rows 0
    and 2 are on it and row 1 must keep its sentinels."""
    H, B, C_ = 2, 3, 128
    dt = torch.int8 if int8_kv else torch.float16
    r = KR.philox(100 * waves + 10 * int8_kv + use_live)
    sent_out = KR.SENTINEL
    sent_cache = 77 if int8_kv else KR.SENTINEL
    for start in STARTS:
        for length in LENGTHS:
            T = start + length
            starts = [start, 0, T]
            content = random_cache(r, B, H, T + 1, int8_kv)
            cache = torch.full((B, 2, H, CAP, 64), sent_cache, dtype=dt)
            cache[:, :, :, :T] = content[:, :, :, :T]
            for b, s in enumerate(starts):
                cache[b, :, :, :s] = pad_fill(int8_kv)
            cache = cache.cuda()
            before = cache.clone()
            qkv = torch.from_numpy(r.standard_normal((B, 3 * C_)).astype(np.float16).astype(np.float32)).cuda()
            out = torch.full((B, C_), sent_out, dtype=torch.float16, device="cuda")
            live_rows = [0, 2] if use_live else [0, 1, 2]
            live = torch.tensor([len(live_rows)] + live_rows + [0] * (B - len(live_rows)), dtype=torch.int32, device="cuda") if use_live else None
            self_rows(lib, qkv, B, 1, T, H, cache, int8_kv, out, torch.tensor(starts, dtype=torch.int32, device="cuda"), live, waves)
            for b in range(B):
                if b not in live_rows:
                    assert torch.equal(out[b].view(torch.int16), torch.full_like(out[b], sent_out).view(torch.int16)), (start, length, b)
                    assert torch.equal(cache[b].view(torch.uint8), before[b].view(torch.uint8)), (start, length, b)
                    continue
                # the same row alone, un-padded: its T - s cached tokens at the front of a cache of its own, row_start == NULL
                s = starts[b]
                alone = torch.full((1, 2, H, CAP, 64), sent_cache, dtype=dt, device="cuda")
                alone[0, :, :, :T - s] = before[b, :, :, s:T]
                want = torch.full((1, C_), sent_out, dtype=torch.float16, device="cuda")
                self_rows(lib, qkv[b:b + 1].contiguous(), 1, 1, T - s, H, alone, int8_kv, want, None, None, waves)
                assert torch.isfinite(want.float()).all()
                assert torch.equal(out[b].view(torch.int16), want[0].view(torch.int16)), (start, length, b)
                assert torch.equal(cache[b, :, :, T].view(torch.uint8), alone[0, :, :, T - s].view(torch.uint8)), (start, length, b)
                # nothing but slot T of the row's cache was written
                keep = torch.ones(CAP, dtype=torch.bool, device="cuda")
                keep[T] = False
                assert torch.equal(cache[b][:, :, keep].view(torch.uint8), before[b][:, :, keep].view(torch.uint8)), (start, length, b)


# --------------------------------------------------------------------------------------------------------- kernel, L = 4
@pytest.mark.parametrize("int8_kv", [0, 1])
@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("T", [0, 8, 68])
def test_prefill_pass_with_row_starts(lib, T, waves, int8_kv):
    """One 4-token pass over slots T .. T + 3 for rows that begin in front of the pass (shifted), at its first slot, inside it
    (1, 2, 3 pad queries: every residue mod 4) and behind it (the whole pass is pad)."""
    H, L, C_ = 2, 4, 128
    starts = sorted({0, max(T - 3, 0), max(T - 1, 0), T, T + 1, T + 2, T + 3, T + 4, T + 9, 1 if T else 0, 65 if T > 65 else 0})
    B = len(starts)
    assert {s % 4 for s in starts if T <= s < T + 4} == {0, 1, 2, 3}
    dt = torch.int8 if int8_kv else torch.float16
    r = KR.philox(7 + T + 10 * waves + int8_kv)
    content = random_cache(r, B, H, T + 1, int8_kv)
    cache = torch.full((B, 2, H, CAP, 64), 77 if int8_kv else KR.SENTINEL, dtype=dt)
    cache[:, :, :, :T] = content[:, :, :, :T]
    for b, s in enumerate(starts):
        cache[b, :, :, :min(s, T)] = pad_fill(int8_kv)
    held = PR.dequant(cache, T_SCALE) if int8_kv else cache.float()
    qkv = torch.from_numpy(r.standard_normal((B, L, 3, H, 64)).astype(np.float16).astype(np.float32))
    want = PR.self_attn_rows_ref(qkv, held, T, starts, H)
    dcache = cache.cuda()
    before = dcache.clone()
    out = torch.full((B * L, C_), KR.SENTINEL, dtype=torch.float16, device="cuda")
    self_rows(lib, qkv.reshape(B * L, 3 * C_).cuda(), B, L, T, H, dcache, int8_kv, out,
              torch.tensor(starts, dtype=torch.int32, device="cuda"), None, waves)
    got = out.float().cpu().reshape(B, L, C_)
    assert torch.isfinite(got).all()
    worst = 0.0
    for b, s in enumerate(starts):
        for i in range(L):
            if T + i < s:
                assert not got[b, i].any(), (s, i)                       # a pad query: exact zeros
            else:
                worst = max(worst, float((got[b, i] - want[b, i]).abs().max()))
    print(f"prefill pass T={T} waves={waves} int8={int8_kv}: max |out - ref| = {worst:.3g} (bound {SELF_ATTN_TOL})")
    assert worst <= SELF_ATTN_TOL
    # every token's k / v lands in its slot, pad tokens included; nothing else is written
    new = qkv[:, :, 1:].permute(0, 2, 3, 1, 4)                             # [B, 2, H, L, 64]
    want_new = PR.quant_codes(new, T_SCALE) if int8_kv else new.half()
    assert torch.equal(dcache[:, :, :, T:T + L].cpu().contiguous().view(torch.uint8), want_new.contiguous().view(torch.uint8))
    keep = torch.ones(CAP, dtype=torch.bool, device="cuda")
    keep[T:T + L] = False
    assert torch.equal(dcache[:, :, :, keep].view(torch.uint8), before[:, :, :, keep].view(torch.uint8))


# --------------------------------------------------------------------------------------------------------- engine
PROMPT_LENGTHS = [0, 1, 2, 3, 223]


@pytest.fixture(scope="module")
def model():
    dims = Dims(**synthetic.DIMS["micro-fullvocab"])
    return dims, synthetic_state_dict(dims, 3), synthetic_mel(len(PROMPT_LENGTHS), 2 * dims.n_audio_ctx, dims.n_mels, 4242)


@pytest.mark.parametrize("int8_kv", [False, True])
def test_engine_rows_with_prompts_match_the_oracle_row_by_row(lib, tmpdir_module, model, int8_kv):
    dims, sd, mel = model
    n = len(PROMPT_LENGTHS)
    scales = [0.05] * dims.n_text_layer if int8_kv else None
    tol = LOGIT_TOL_INT8_KV if int8_kv else LOGIT_TOL
    eng = build_engine(tmpdir_module, "micro-fullvocab", 3, int8_kv=int8_kv, kv_scales=scales)
    enc, dec = WhisperEncoding(eng), WhisperDecoding(eng, row_prompts=True)
    tk = dec.tokenizer
    L0, sot_index, capacity = row_prompt_layout(dims.n_text_ctx, tk.sot_sequence, tk.sot)
    assert (L0, capacity) == (227, 223) and dec.sample_begin == L0 and dec.sot_index == sot_index
    r = KR.philox(11)
    prompts = [[int(t) for t in r.integers(0, 50000, size=k)] for k in PROMPT_LENGTHS]
    rows, starts = right_aligned_rows(prompts, tk.sot_sequence, tk.sot_prev, dims.n_text_ctx)
    assert starts == [224, 222, 221, 220, 0]

    oracle = OracleModel(dims, sd, OracleConfig(act="float16", int8_kv=int8_kv, kv_scales=scales))
    ckv = oracle.cross_kv(oracle.encoder(mel))
    n_steps = 4
    ref_logits, ref_ids = [], []                    # per row: [1 + n_steps] last-position logits (+ the sot position), the tokens fed
    for b in range(n):
        ckv_b = [t[b:b + 1] for t in ckv]
        logits, kv = PR.oracle_row(oracle, ckv_b, rows[b][starts[b]:], starts[b])
        per_step, ids = [logits[-1]], []
        at_sot = logits[sot_index - starts[b]]
        for _ in range(n_steps):
            ids.append(int(per_step[-1].argmax()))
            lg, kv = oracle.decoder(torch.tensor([[ids[-1]]]), ckv_b, kv)
            per_step.append(lg[0, 0])
        ref_logits.append((at_sot, per_step))
        ref_ids.append(ids)

    xa = enc.get_audio_features(mel.cuda())
    st = dec._fast_state(n, xa.device)
    cross = dec._cross_persistent(xa, st)
    tokens = torch.zeros((n, CAP + 1), dtype=torch.int32, device="cuda")
    tokens[:, :L0] = torch.tensor(rows, dtype=torch.int32)
    tokens[:, L0:L0 + n_steps] = torch.tensor(ref_ids, dtype=torch.int32)
    row_start = torch.tensor(starts, dtype=torch.int32, device="cuda")
    sess, pos, V = dec.decoder_session, dec.positional_embedding, dims.n_vocab
    sess.decoder_step(tokens[:, :L0], pos[0:L0], cross, None, CAP, st['kv'], CAP, st['logits'], 0, stream(), row_start=row_start)
    torch.cuda.synchronize()
    got = st['logits'].float().cpu()
    assert torch.isfinite(got).all()                # pad positions included
    worst_sot = max(float((got[b, sot_index] - ref_logits[b][0]).abs().max()) for b in range(n))
    worst = [max(float((got[b, L0 - 1] - ref_logits[b][1][0]).abs().max()) for b in range(n))]
    step_logits = torch.empty((n, 1, V), dtype=torch.float16, device="cuda")
    for s in range(n_steps):
        cur = L0 + s
        sess.decoder_step(tokens[:, cur:cur + 1], pos[cur:cur + 1], cross, st['kv'], CAP, st['kv'], CAP, step_logits, cur, stream(),
                          row_start=row_start)
        torch.cuda.synchronize()
        g = step_logits[:, 0].float().cpu()
        worst.append(max(float((g[b] - ref_logits[b][1][s + 1]).abs().max()) for b in range(n)))
    print(f"engine rows vs oracle (int8_kv={int8_kv}): max |dlogit| at <|sot|> {worst_sot:.4g}, last position and {n_steps} steps "
          f"{[round(w, 4) for w in worst]} (bound {tol})")
    assert worst_sot < tol and max(worst) < tol
    # wm_decoder_step_tap and wm_decoder_step_multi refuse row_start
    io = sess.make_decoder_io(tokens[:, L0:L0 + 1], pos[L0:L0 + 1], cross, st['kv'], CAP, st['kv'], CAP, step_logits, L0, row_start=row_start)
    light, heavy = dec._group_streams(2, xa.device)          # (the process-wide cached group streams: no new stream, no new hardware queue)
    with pytest.raises(native.WmError, match="row_start"):
        sess.decoder_step_multi([io], [light.cuda_stream], heavy.cuda_stream)


# --------------------------------------------------------------------------------------------------------- main_loop
# Eight utterances, eight prompt lengths (none, 1, 2, 3: every pass alignment; 223: the longest a row can carry).  Random weights
# put the two best logits of a step close together again and again, so the case was picked ON THE CPU: of the seeds scanned
# (mel 9000 + seed, prompts philox(500 + seed)) this one leaves the CPU oracle's greedy decode of these rows with a top-two margin
# below 2 * LOGIT_TOL in ONE row of the eight over SAMPLE_LEN steps -- the share the comparison may drop, and only where the
# oracle's own margin says the step was a near-tie.  The fixture re-checks that count.
LOOP_LENGTHS = [0, 1, 2, 3, 223, 5, 60, 130]
LOOP_SEED = 164
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
    eng = build_engine(tmpdir_module, "micro-fullvocab", 3)
    enc = WhisperEncoding(eng)
    xa = enc.get_audio_features(mel.cuda())
    # the CPU reference: every row alone and un-padded through the oracle, with the loop's rules
    plain = WhisperDecoding(eng)
    tk = plain.tokenizer
    oracle = OracleModel(dims, synthetic_state_dict(dims, 3), OracleConfig(act="float16"))
    ckv = oracle.cross_kv(oracle.encoder(mel))
    rows, starts = right_aligned_rows(prompts, tk.sot_sequence, tk.sot_prev, dims.n_text_ctx)
    cpu_tokens, cpu_margins = [], []
    for b in range(n):
        row = rows[b][starts[b]:]
        rules = DR.RuleSet(DR.MULTILINGUAL, len(row), list(plain._get_suppress_tokens()), list(tk.blank_tokens()) + [tk.eot],
                           plain.max_initial_timestamp_index)
        toks, margins = PR.oracle_greedy_row(oracle, [t[b:b + 1] for t in ckv], row, rules, SAMPLE_LEN)
        cpu_tokens.append(toks + [tk.eot] * (SAMPLE_LEN - len(toks)))
        cpu_margins.append(margins + [float("inf")] * (SAMPLE_LEN - len(margins)))
    near = [b for b in range(n) if min(cpu_margins[b]) < 2 * LOGIT_TOL]
    print(f"CPU reference: rows with a near-tie (margin < {2 * LOGIT_TOL}) in {SAMPLE_LEN} steps: {near}, "
          f"smallest margins {[round(min(m), 3) for m in cpu_margins]}")
    assert len(near) <= n // 8, "the seed no longer keeps the reference's near-ties within one row in eight"
    # the device reference: every row ALONE through the shared-prompt instance (options.prompt), greedy
    alone = []
    for b in range(n):
        dec = WhisperDecoding(eng, options=DecodingOptions(prompt=prompts[b] or None, sample_len=SAMPLE_LEN))
        t, lp, nsp = dec.main_loop(xa[b:b + 1].contiguous())
        alone.append((sampled(t, dec.sample_begin, tk.eot)[0], float(lp[0]), float(nsp[0])))
        del dec
    del plain
    yield dict(dims=dims, eng=eng, enc=enc, xa=xa, mel=mel, prompts=prompts, tk=tk, cpu_tokens=cpu_tokens, cpu_margins=cpu_margins, alone=alone)
    gc.collect()
    torch.cuda.synchronize()


def compare_with_rows_alone(case, got_tokens, got_lp, got_nsp, rows=None):
    """Every row against the same row decoded alone.  A row may part ways only at a step where the CPU reference's own margin is
    below 2 * LOGIT_TOL, and at most one row in eight does."""
    n = len(case["prompts"])
    rows = list(range(n)) if rows is None else rows
    dropped = []
    for b in rows:
        want, want_lp, want_nsp = case["alone"][b]
        if got_tokens[b] != want:
            k = next(i for i in range(SAMPLE_LEN) if not (got_tokens[b][i] == want[i] == case["cpu_tokens"][b][i]))
            assert case["cpu_margins"][b][k] < 2 * LOGIT_TOL, (b, k, got_tokens[b], want, case["cpu_tokens"][b], case["cpu_margins"][b])
            dropped.append((b, k))
            continue
        # a log-probability moves by at most twice the logits' error; two device paths within LOGIT_TOL of the oracle each
        assert abs(got_lp[b] - want_lp) <= SAMPLE_LEN * 4 * LOGIT_TOL, (b, got_lp[b], want_lp)
        assert abs(got_nsp[b] - want_nsp) <= 1e-3, (b, got_nsp[b], want_nsp)
    print(f"rows that part ways with the row decoded alone, at a near-tie of the CPU reference: {dropped}")
    assert len(dropped) <= n // 8
    return dropped


@pytest.mark.parametrize("graphs", [True, False])
def test_main_loop_with_prompts_equals_every_row_alone(lib, loop_case, graphs):
    c = loop_case
    dec = WhisperDecoding(c["eng"], row_prompts=True, options=DecodingOptions(sample_len=SAMPLE_LEN))
    dec.use_graphs = graphs
    assert dec.sample_begin == 227 and dec.sample_len == SAMPLE_LEN
    dec.set_prompts(c["prompts"])
    runs = []
    for _ in range(2 if graphs else 1):              # with graphs: the second call replays what the first captured
        t, lp, nsp = dec.main_loop(c["xa"])
        assert t[:, :dec.sample_begin].tolist() == dec._initial_token_rows(len(c["prompts"]), "cpu").tolist()
        runs.append((sampled(t, dec.sample_begin, c["tk"].eot), lp.tolist(), list(nsp)))
    st = next(iter(dec._state.values()))
    assert (len(st['graphs']) > 0) == graphs
    assert native.chain_status()["error_pending"] is False
    if graphs:
        assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    compare_with_rows_alone(c, *runs[-1])
    # the results read like any others
    res = dec.post_process(t, lp, nsp, c["xa"], ["en"] * len(c["prompts"]))
    assert [r.tokens for r in res] == [row[:row.index(c["tk"].eot)] if c["tk"].eot in row else row for row in runs[-1][0]]
    assert all(len(r.tokens) <= SAMPLE_LEN for r in res)


def test_main_loop_with_prompts_and_closed_rows(lib, loop_case):
    """row_limit = 0 (transcribe's empty and settled rows): such a row ends at once, the others are what they are alone."""
    c = loop_case
    n = len(c["prompts"])
    dec = WhisperDecoding(c["eng"], row_prompts=True, options=DecodingOptions(sample_len=SAMPLE_LEN))
    dec.set_prompts(c["prompts"])
    limit = torch.tensor([0 if b in (1, 4, 7) else 1 << 30 for b in range(n)], dtype=torch.int32)
    t, lp, nsp = dec.main_loop(c["xa"], row_limit=limit)
    got = sampled(t, dec.sample_begin, c["tk"].eot)
    for b in (1, 4, 7):
        assert got[b] == [c["tk"].eot] * SAMPLE_LEN and float(lp[b]) == 0.0
    compare_with_rows_alone(c, got, lp.tolist(), list(nsp), rows=[b for b in range(n) if b not in (1, 4, 7)])


@pytest.fixture
def one_decode_path(lib):
    """One set of kernels for every batch size and pass length (as tests/test_gpu_model.py::one_decode_path): the candidates'
    draws and the beams' scores are compared exactly below."""
    prev, prev_rows = lib.wm_set_small_batch_rows(0), lib.wm_set_rows_path(0)
    yield
    lib.wm_set_small_batch_rows(prev)
    lib.wm_set_rows_path(prev_rows)


def shared_prompt_run(c, xa, prompt, options, seed=5):
    """The already-supported route: ONE prompt for the whole batch (options.prompt), over the same batch (a candidate's draws are
    keyed on its row)."""
    ref = WhisperDecoding(c["eng"], options=DecodingOptions(prompt=prompt or None, sample_len=SAMPLE_LEN, **options))
    torch.manual_seed(seed)
    rt, rlp, rnsp = ref.main_loop(xa)
    return sampled(rt, ref.sample_begin, c["tk"].eot), ref.post_process(rt, rlp, rnsp, xa, ["en"] * xa.shape[0])


def test_beam_search_with_prompts(lib, loop_case, one_decode_path):
    """The beams of an utterance share its start.  Reference: the shared-prompt instance, one prompt at a time, utterance u read from
    the run with prompt u.  With one set of kernels the arithmetic of a row does not depend on where its passes are cut (one-wave
    self-attention: keys in slot order), and beam search draws nothing: the comparison is exact."""
    c = loop_case
    sel = [0, 2, 5, 4]                                # prompts of 0, 2, 5 and 223 tokens
    xa = c["xa"][sel].contiguous()
    prompts = [c["prompts"][b] for b in sel]
    K = 2
    dec = WhisperDecoding(c["eng"], row_prompts=True, options=DecodingOptions(sample_len=SAMPLE_LEN, beam_size=K))
    dec.set_prompts(prompts)
    t, lp, nsp = dec.main_loop(xa)
    assert t.shape[0] == len(sel) * K
    got = dec.post_process(t, lp, nsp, xa, ["en"] * len(sel))
    got_rows = sampled(t, dec.sample_begin, c["tk"].eot)
    for u, prompt in enumerate(prompts):
        want_rows, want = shared_prompt_run(c, xa, prompt, dict(beam_size=K))
        assert got_rows[u * K:(u + 1) * K] == want_rows[u * K:(u + 1) * K], (u, got_rows[u * K:(u + 1) * K], want_rows[u * K:(u + 1) * K])
        assert got[u].tokens == want[u].tokens and abs(got[u].avg_logprob - want[u].avg_logprob) < 1e-5
        assert abs(got[u].no_speech_prob - want[u].no_speech_prob) < 1e-6
    assert len({tuple(r) for r in got_rows}) > len(sel)          # the beams differ: not vacuous


def test_best_of_with_prompts(lib, loop_case, one_decode_path):
    """Temperature sampling with two candidates per utterance.  The draw of a token is keyed on (seed, row, POSITION, token)
    (csrc/greedy.hip), and a right-aligned row samples at positions L0 .. whatever its prompt: only a row whose prompt fills the
    row (223 tokens: start 0) draws what the shared-prompt instance draws, and that row is compared exactly.  For every candidate
    of every utterance the context is checked through what the loop books: sum_logprobs must be the log-probabilities, under
    Whisper's rules, that the plain decoder gives the sampled tokens behind the un-padded row (teacher-forced through decode()) --
    a candidate that saw another prompt or start would be off by nats, the bound is the logits' (two device paths within
    LOGIT_TOL of the oracle each; a log-probability moves by at most twice the logits' error)."""
    import oracle.decoding_rules as DR
    c = loop_case
    tk = c["tk"]
    sel = [0, 2, 5, 4]
    xa = c["xa"][sel].contiguous()
    prompts = [c["prompts"][b] for b in sel]
    K = 2
    options = dict(best_of=K, temperature=0.6)
    dec = WhisperDecoding(c["eng"], row_prompts=True, options=DecodingOptions(sample_len=SAMPLE_LEN, **options))
    dec.set_prompts(prompts)
    torch.manual_seed(5)
    t, lp, nsp = dec.main_loop(xa)
    assert t.shape[0] == len(sel) * K and dec._row_starts.tolist() == [224, 224, 221, 221, 218, 218, 0, 0]
    got = dec.post_process(t, lp, nsp, xa, ["en"] * len(sel))
    got_rows = sampled(t, dec.sample_begin, tk.eot)
    assert len({tuple(r) for r in got_rows}) > len(sel)          # the candidates differ: not vacuous
    want_rows, want = shared_prompt_run(c, xa, prompts[3], options)
    assert got_rows[3 * K:] == want_rows[3 * K:] and got[3].tokens == want[3].tokens
    assert abs(got[3].avg_logprob - want[3].avg_logprob) < 1e-5
    plain = WhisperDecoding(c["eng"])
    rows, starts = right_aligned_rows(prompts, tk.sot_sequence, tk.sot_prev, c["dims"].n_text_ctx)
    worst = 0.0
    for u in range(len(sel)):
        head = rows[u][starts[u]:]
        cross = plain.xa2cross_key_value(xa[u:u + 1].contiguous())
        rules = DR.RuleSet(DR.MULTILINGUAL, len(head), list(plain._get_suppress_tokens()), list(tk.blank_tokens()) + [tk.eot],
                           plain.max_initial_timestamp_index)
        for k in range(K):
            seq = head + got_rows[u * K + k]
            logits, _ = plain.decode(torch.tensor([seq[:-1]]).cuda(), cross)
            logits = logits.float().cpu().numpy()[0]
            total = 0.0
            for i in range(SAMPLE_LEN):
                ctx = np.array([seq[:len(head) + i]], dtype=np.int64)
                if i > 0 and ctx[0, -1] == tk.eot:
                    break
                lg = DR.apply_filters(logits[None, len(head) + i - 1], ctx, rules)
                total += float(DR.log_softmax_f32(lg)[0, seq[len(head) + i]])
            worst = max(worst, abs(total - float(lp[u * K + k])))
    print(f"best_of: max |sum_logprobs - teacher-forced sum| = {worst:.4g} (bound {SAMPLE_LEN * 4 * LOGIT_TOL})")
    assert worst <= SAMPLE_LEN * 4 * LOGIT_TOL


# --------------------------------------------------------------------------------------------------------- transcribe()
def test_transcribe_conditions_every_file_on_its_own_previous_text(lib, loop_case):
    """Three files of different lengths, conditioning on, an initial prompt: the batched run must give every file the segments of
    longform.transcribe_reference driven by single-row device calls (one window, one prompt at a time), and the prompt a file's
    second window was decoded with is the initial prompt plus the tokens of its first window's segments."""
    import longform as LF
    import transcribe as T
    c = loop_case
    dims, eng, enc, tk = c["dims"], c["eng"], c["enc"], c["tk"]
    W = 2 * dims.n_audio_ctx
    contents = [300, 128, 200]
    mels = [synthetic_mel(1, cf + W, dims.n_mels, 70 + f)[0].half().cuda().contiguous() for f, cf in enumerate(contents)]
    initial = [1500, 1501]
    kw = dict(temperatures=(0.0,), compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None)

    def instance():
        d = WhisperDecoding(eng, row_prompts=True, options=DecodingOptions(language="en"))
        d.sample_len = 6
        return d
    trace = []
    results = T.transcribe_mel(enc, instance(), mels, contents, n_rows=3, trace=trace, condition_on_previous_text=True,
                               initial_prompt=initial, **kw)
    one = instance()
    seen = {}

    def decode_one(f, seek, t, prompt):
        seen.setdefault(f, []).append((seek, list(prompt)))
        xa = enc.get_audio_features(mels[f][None, :, seek:seek + W].contiguous())
        one.set_prompts([prompt])
        out = one.post_process(*one.main_loop(xa, temperature=t), xa, ["en"], temperature=t)
        return out[0]
    for f, cf in enumerate(contents):
        want = LF.transcribe_reference(lambda seek, t, prompt, f=f: decode_one(f, seek, t, prompt), cf, window=W,
                                       timestamp_begin=tk.timestamp_begin, decode_text=tk.decode, condition_on_previous_text=True,
                                       initial_prompt=initial, **kw)
        # tokens, times and text exactly; the two figures that are sums of fp32 logits to the project's bounds for them (a batch of
        # three and a single row add up in another order: tests/test_gpu_model.py compares the same quantities to 2e-3 and 1e-4)
        exact = ("seek", "start", "end", "text", "tokens", "temperature", "compression_ratio")
        assert [{k: s[k] for k in exact} for s in results[f]["segments"]] == [{k: s[k] for k in exact} for s in want], f
        for a, b in zip(results[f]["segments"], want):
            assert abs(a["avg_logprob"] - b["avg_logprob"]) <= 2e-3 and abs(a["no_speech_prob"] - b["no_speech_prob"]) <= 1e-4, (f, a, b)
    # what the batched run handed the decoder: per (file, seek) the prompt of the literal loop
    handed = {}
    for e in trace:
        assert len(e["prompts"]) == 3
        for r, on, p in zip(e["rows"], e["live"], e["prompts"]):
            if r is None:
                assert p == []
            elif on:
                handed[r] = p
    for f in range(3):
        assert [(s, handed[(f, s)]) for s, _ in seen[f]] == seen[f]
        first = [t for s in results[f]["segments"] if s["seek"] == 0 for t in s["tokens"]]
        assert seen[f][0] == (0, initial)
        if len(seen[f]) > 1:
            assert seen[f][1][1] == initial + first
    assert sum(len(seen[f]) > 1 and len(seen[f][1][1]) > len(initial) for f in range(3)) >= 1      # a second window saw previous text
    assert len(trace[0]["rows"]) == 3 and all(e["n_states"] == 1 for e in trace)
    # an instance without row_prompts refuses
    with pytest.raises(ValueError, match="row_prompts=True"):
        T.transcribe_mel(enc, WhisperDecoding(eng), mels, contents, initial_prompt=initial)
