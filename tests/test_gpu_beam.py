"""Beam search on the device (csrc/beam.hip): wm_beam_step and wm_kv_reorder against numpy restatements of their
contracts (include/whisper_mi355.h), and the device loop of WhisperDecoding.main_loop against the literal loop
(`main_loop_reference` + `decoding.BeamSearchDecoder`, itself held to a brute-force restatement in tests/test_beam_cpu.py).

Tolerances: tokens, parents, pools and flags are integer work and must be exact.  Sums: 2e-4 for one step's
log-probability (the bound of the greedy-step tests), 2e-3 over a loop (the bound of the fused-vs-literal greedy test).
The kernel and numpy differ only in the fp32 log-sum-exp, so two candidates closer than twice the bound that are not an
exact tie inside one row could legitimately swap: every test ASSERTS on the reference side that its inputs hold no such
pair among the walked candidates, and then leaves nothing out."""
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
from decoding import BeamSearchDecoder, DecodingOptions, WhisperDecoding  # noqa: E402
from encoding import WhisperEncoding  # noqa: E402
from oracle import decoding_rules as DR  # noqa: E402
from oracle.whisper_oracle import Dims, OracleConfig, OracleModel, synthetic_mel, synthetic_state_dict  # noqa: E402

IDS = DR.MULTILINGUAL
V, TB, EOT = IDS.n_vocab, IDS.timestamp_begin, IDS.eot
STEP_TOL, LOOP_TOL = 2e-4, 2e-3


@pytest.fixture(scope="module")
def lib():
    return native.load_library()


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def rules(golden_dir):
    fixr = np.load(os.path.join(golden_dir, "decoding_rules.npz"))
    sup = sorted(set(fixr["suppress"].tolist() + [IDS.no_timestamps]))
    return DR.RuleSet(IDS, 3, sup, fixr["blank"].tolist(), 50)


# ---- numpy restatement of the beam step ------------------------------------------------------------------------------
def np_propose(lp, k):
    """The k best tokens of a row: log-probability descending, token ascending among equals, finite only."""
    kth = np.partition(lp, -k)[-k]
    idx = np.nonzero((lp >= kth) & np.isfinite(lp))[0]
    return idx[np.lexsort((idx, -lp[idx]))][:k]


class NpBeam:
    """The state wm_beam_step keeps, as numpy mirrors of the device buffers (zero-initialised like them)."""

    def __init__(self, n_audio, K, MC, ld, init_rows, sums=None):
        self.n_audio, self.K, self.MC, self.ld = n_audio, K, MC, ld
        rows = n_audio * K
        self.tokens = np.zeros((rows, ld), np.int32)
        for r, t in enumerate(init_rows):
            self.tokens[r, :len(t)] = t
        self.sums = np.zeros(rows, np.float32) if sums is None else sums.astype(np.float32).copy()
        self.parent = np.zeros(rows, np.int32)
        self.fin_tokens = np.zeros((n_audio, MC, ld), np.int32)
        self.fin_scores = np.zeros((n_audio, MC), np.float32)
        self.fin_len = np.zeros((n_audio, MC), np.int32)
        self.fin_count = np.zeros(n_audio, np.int32)
        self.live_len = np.zeros(n_audio, np.int32)
        self.done = np.zeros(rows, np.int32)
        self.n_done = 0
        self.min_gap, self.events = np.inf, set()

    def step(self, logits, cur, rules, ignore_eot=False, row_limit=None):
        K, MC = self.K, self.MC
        dom = []
        filtered = DR.apply_filters(logits, self.tokens[:, :cur].astype(np.int64), rules, dominance_out=dom)
        lp = DR.log_softmax_f32(filtered)
        first = cur == rules.sample_begin
        old_tokens, old_sums = self.tokens.copy(), self.sums.copy()
        for a in range(self.n_audio):
            r0 = a * K
            self.parent[r0:r0 + K] = np.arange(r0, r0 + K)
            if self.done[r0]:
                continue
            if row_limit is not None and cur - rules.sample_begin >= row_limit[r0]:
                self.done[r0:r0 + K], self.live_len[a] = 1, cur
                self.n_done += K
                self.events.add("row_limit")
                continue
            cands = []
            for j in range(1 if first else K):
                assert not np.isfinite(dom[r0 + j]) or abs(dom[r0 + j]) > 0.05, "near-tie of the timestamp-dominance rule"
                props = np_propose(lp[r0 + j], K + 1)
                assert len(props) == K + 1
                vals = filtered[r0 + j, props]
                if len(set(vals.tolist())) < len(vals):
                    self.events.add("tie")
                cands += [(np.float32(old_sums[r0 + j] + lp[r0 + j, t]), j, int(t)) for t in props]
            cands.sort(key=lambda c: (-c[0], c[1], c[2]))
            live, fin, stop = [], [], len(cands) - 1
            for i, c in enumerate(cands):
                if c[2] == EOT:
                    fin.append(c)
                else:
                    live.append(c)
                    if len(live) == K:
                        stop = i
                        break
            assert len(live) == K
            for c0, c1 in zip(cands[:stop + 1], cands[1:stop + 2]):          # the walked candidates and the first one left out
                if not (c0[1] == c1[1] and filtered[r0 + c0[1], c0[2]] == filtered[r0 + c1[1], c1[2]]):
                    self.min_gap = min(self.min_gap, float(c0[0] - c1[0]))
            for i, (s, j, t) in enumerate(live):
                self.tokens[r0 + i, :cur] = old_tokens[r0 + j, :cur]
                self.tokens[r0 + i, cur] = t
                self.sums[r0 + i], self.parent[r0 + i] = s, r0 + j
            if len({c[1] for c in fin}) == 1:
                self.events.add("eot_one_beam")
            if len({c[1] for c in fin}) > 1:
                self.events.add("eot_several_beams")
            for s, j, t in fin:
                n = self.fin_count[a]
                if n >= MC:
                    self.events.add("pool_overflow")
                    break
                self.fin_tokens[a, n, :cur] = old_tokens[r0 + j, :cur]
                self.fin_tokens[a, n, cur] = EOT
                self.fin_scores[a, n], self.fin_len[a, n] = s, cur + 1
                self.fin_count[a] = n + 1
            if self.parent[r0:r0 + K].tolist() != list(range(r0, r0 + K)):
                self.events.add("reorder")
            if not ignore_eot and self.fin_count[a] >= MC:
                self.done[r0:r0 + K], self.live_len[a] = 1, cur + 1
                self.n_done += K
                self.events.add("complete")


class DevBeam:
    """The device buffers of one wm_beam_step sequence."""

    def __init__(self, lib, ref: NpBeam, rules):
        self.lib, self.rules = lib, rules
        self.K, self.MC, self.ld = ref.K, ref.MC, ref.ld
        self.tokens, self.sums = dev(ref.tokens), dev(ref.sums)
        rows = ref.tokens.shape[0]
        z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt, device="cuda")      # noqa: E731
        self.parent = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
        self.fin_tokens, self.fin_scores = z(ref.n_audio, ref.MC, ref.ld), z(ref.n_audio, ref.MC, dt=torch.float32)
        self.fin_len, self.fin_count, self.live_len = z(ref.n_audio, ref.MC), z(ref.n_audio), z(ref.n_audio)
        self.done, self.n_done, self.counter = z(rows), z(1), z(1)
        self.ws = torch.empty(lib.wm_beam_workspace_bytes(rows, ref.K), dtype=torch.uint8, device="cuda")
        self.sup = dev(np.array(rules.suppress_tokens, dtype=np.int32))
        self.blank = dev(np.array(rules.blank_tokens, dtype=np.int32))

    def step(self, logits, cur, use_counter, ignore_eot=False, row_limit=None):
        rows = self.tokens.shape[0]
        lg = dev(logits.astype(np.float16))
        io = native.WmBeamIO()
        io.logits, io.row_stride, io.batch, io.n_vocab = lg.data_ptr(), V, rows, V
        io.tokens, io.tokens_ld, io.sum_logprobs = self.tokens.data_ptr(), self.ld, self.sums.data_ptr()
        if use_counter:
            self.counter.fill_(cur - 1)
            io.cur_len, io.n_past_dev = 0, self.counter.data_ptr()
        else:
            io.cur_len = cur
        io.suppress, io.n_suppress = self.sup.data_ptr(), self.sup.numel()
        io.blank, io.n_blank = self.blank.data_ptr(), self.blank.numel()
        io.sample_begin, io.eot, io.timestamp_begin = self.rules.sample_begin, EOT, TB
        io.max_initial_timestamp_index, io.apply_rules = self.rules.max_initial_timestamp_index, 1
        io.beam_size, io.max_candidates, io.ignore_eot = self.K, self.MC, int(ignore_eot)
        if row_limit is not None:
            self.row_limit = dev(np.asarray(row_limit, dtype=np.int32))
            io.row_limit = self.row_limit.data_ptr()
        io.parent, io.fin_tokens, io.fin_scores = self.parent.data_ptr(), self.fin_tokens.data_ptr(), self.fin_scores.data_ptr()
        io.fin_len, io.fin_count, io.live_len = self.fin_len.data_ptr(), self.fin_count.data_ptr(), self.live_len.data_ptr()
        io.done, io.n_done = self.done.data_ptr(), self.n_done.data_ptr()
        io.workspace, io.workspace_bytes = self.ws.data_ptr(), self.ws.numel()
        native.check(self.lib.wm_beam_step(C.byref(io), stream()), "wm_beam_step")
        torch.cuda.synchronize()

    def assert_equals(self, ref: NpBeam, what):
        for name in ("tokens", "parent", "fin_tokens", "fin_len", "fin_count", "live_len", "done"):
            got = getattr(self, name).cpu().numpy()
            assert np.array_equal(got, getattr(ref, name)), (what, name, got, getattr(ref, name))
        assert int(self.n_done[0]) == ref.n_done, what
        np.testing.assert_allclose(self.sums.cpu().numpy(), ref.sums, rtol=0, atol=STEP_TOL, err_msg=str(what))
        np.testing.assert_allclose(self.fin_scores.cpu().numpy(), ref.fin_scores, rtol=0, atol=STEP_TOL, err_msg=str(what))
        self.sums.copy_(dev(ref.sums))                  # every step is compared on its own: the next one starts from the reference's sums
        self.fin_scores.copy_(dev(ref.fin_scores))


def draw_separated(ref, make_logits, cur, rules, need=frozenset(), **kw):
    """Logits from `make_logits()` whose step -- judged by the numpy restatement alone, on a copy of its state -- walks no two
    candidates closer than 1e-3 that are not an exact same-row tie, has no near-tie of the timestamp-dominance rule and shows
    the events in `need`.  A condition on the inputs: the kernel's results play no part in it."""
    import copy
    for _ in range(200):
        x = make_logits()
        trial = copy.deepcopy(ref)
        trial.min_gap, trial.events = np.inf, set()
        try:
            trial.step(x, cur, rules, **kw)
        except AssertionError:
            continue
        if trial.min_gap >= 1e-3 and need <= trial.events:
            return x
    raise AssertionError(f"no separated logits with {set(need)} in 200 draws")


def peaked_logits(r, rows, K, row_offsets):
    """Full-vocabulary fp16 logits with separated peaks (as the greedy tests' +12 / +9 bumps): per row K + 3 text tokens lifted
    by well-spaced amounts and one timestamp; `row_offsets` shifts a whole row's peaks so that the beams' scores differ."""
    x = (r.standard_normal((rows, V)) * 1.5).astype(np.float32)
    picks = []
    for b in range(rows):
        toks = r.choice(50000, size=K + 3, replace=False)
        for q, t in enumerate(toks):
            x[b, t] = 14.0 - 1.1 * q + row_offsets[b]
        x[b, TB + 100 + int(r.integers(0, 1300))] = 8.0 + row_offsets[b]
        picks.append(toks)
    return x, picks


@pytest.mark.parametrize("K,n_audio,patience,use_counter,seed", [(1, 1, None, False, 0), (3, 2, 1.0, True, 1), (5, 3, 1.0, False, 2),
                                                                 (8, 2, 2.0, True, 3), (5, 1, 0.6, True, 4)])
def test_beam_step_matches_numpy_contract(lib, rules, K, n_audio, patience, use_counter, seed):
    """A scripted run of wm_beam_step, every step compared in full with the numpy restatement: the first sampled step (only
    beam 0 proposes, only early timestamps allowed), text steps, an exact fp16 tie inside the best beam_size + 1 of a row, EOT
    proposed by one beam and by several, a pool that fills in the middle of a step's finished list, frozen utterances."""
    r = np.random.Generator(np.random.Philox(100 + seed))
    rows, MC, ld = n_audio * K, round(K * (patience or 1.0)), 64
    ref = NpBeam(n_audio, K, MC, ld, [[IDS.sot, IDS.lang0, IDS.transcribe]] * rows)
    gpu = DevBeam(lib, ref, rules)
    cur = 3

    def make(step):
        offs = r.permutation(rows) * 0.11 + r.random(rows) * 0.05
        x, picks = peaked_logits(r, rows, K, offs)
        if step == 0:                                   # allowed: timestamps 0.00 .. 1.00 s
            for b in range(rows):
                for q, t in enumerate(r.choice(51, size=min(K + 2, 12), replace=False)):
                    x[b, TB + t] = 12.0 - 0.8 * q
        if step == 2:                                   # an exact tie inside the best K + 1 of every row
            for b in range(rows):
                x[b, picks[b][1]] = x[b, picks[b][0]]
        if step == 3:                                   # the best beam of every utterance proposes EOT as its best token
            for a in range(n_audio):
                x[a * K, EOT] = 15.5 + offs[a * K]
        if step >= 5:                                   # every beam proposes EOT as its best token: the pools fill, some mid-list
            for b in range(rows):
                x[b, EOT] = 14.6 + offs[b]
        return x.astype(np.float16).astype(np.float32)

    for step in range(9):
        live = not ref.done.all()
        need = {2: {"tie"}, 3: {"eot_one_beam"}, 5: {"eot_several_beams"} if K > 1 else set()}.get(step, set()) if live else set()
        x = draw_separated(ref, lambda: make(step), cur, rules, frozenset(need))
        ref.step(x, cur, rules)
        gpu.step(x, cur, use_counter)
        gpu.assert_equals(ref, (K, step))
        cur += 1
    assert ref.min_gap >= 2 * STEP_TOL, f"the scripted logits hold two candidates {ref.min_gap} apart"
    want = {"tie", "eot_one_beam", "complete"} | ({"eot_several_beams", "reorder"} if K > 1 else set()) | ({"pool_overflow"} if K in (3, 5) else set())
    assert want <= ref.events, want - ref.events


def test_beam_step_long_histories_ignore_eot_and_row_limit(lib, rules):
    """Rows whose histories span several waves and carry timestamps at every kind of position (the construction of the greedy
    kernel's long-history test), different per beam; then the `ignore_eot` form (a full pool freezes nothing) and `row_limit`."""
    r = np.random.Generator(np.random.Philox(2027))
    K, n_audio, ld = 3, 2, 1500
    for n in (1, 2, 64, 65, 300, 1100):
        init = []
        for kind in range(6):
            hist = r.integers(0, 50000, n)
            if kind >= 1:
                pos = sorted(r.choice(n, size=min(n, 1 + kind), replace=False).tolist())
                t = int(r.integers(0, 700))
                for q in pos:
                    t += int(r.integers(0, 40)); hist[q] = TB + t
            if kind == 2: hist[-1] = TB + 1200
            if kind == 3 and n >= 2: hist[-1] = hist[-2] = TB + 1300
            if kind == 4: hist[0] = TB + 7; hist[1:] = r.integers(0, 50000, n - 1)
            if kind == 5 and n > 70: hist[63] = TB + 900; hist[64:] = r.integers(0, 50000, n - 64)
            init.append(np.concatenate([[IDS.sot, IDS.lang0, IDS.transcribe], hist]))
        sums = -r.random(6) * 3
        ref = NpBeam(n_audio, K, K, ld, init, sums)
        gpu = DevBeam(lib, ref, rules)

        def make():
            x, _ = peaked_logits(r, 6, K, r.permutation(6) * 0.13)
            for b in range(6):                            # several allowed timestamps with clear gaps (rows that must take one)
                for q in range(K + 2):
                    x[b, TB + 1400 + 7 * q + b] = (16.0 if b % 2 else 9.0) - 1.1 * q
            return x.astype(np.float16).astype(np.float32)
        x = draw_separated(ref, make, 3 + n, rules)
        ref.step(x, 3 + n, rules)
        gpu.step(x, 3 + n, use_counter=bool(n % 2))
        gpu.assert_equals(ref, n)
        assert ref.min_gap >= 2 * STEP_TOL, (n, ref.min_gap)
    # ignore_eot: the pool fills and stays full, nothing is frozen; row_limit: utterance 1 is frozen before its third step
    ref = NpBeam(2, 3, 3, 64, [[IDS.sot, IDS.lang0, IDS.transcribe]] * 6)
    gpu = DevBeam(lib, ref, rules)
    for step in range(5):
        limit = [1 << 30] * 3 + [2] * 3

        def make():
            offs = r.permutation(6) * 0.11
            x, _ = peaked_logits(r, 6, 3, offs)
            for b in range(6):
                for q, t in enumerate(r.choice(51, size=5, replace=False)):
                    x[b, TB + t] = 12.0 - 0.8 * q
                if step >= 1:
                    x[b, EOT] = 14.6 + offs[b]
            return x.astype(np.float16).astype(np.float32)
        x = draw_separated(ref, make, 3 + step, rules, ignore_eot=True, row_limit=limit)
        ref.step(x, 3 + step, rules, ignore_eot=True, row_limit=limit)
        gpu.step(x, 3 + step, step % 2 == 0, ignore_eot=True, row_limit=limit)
        gpu.assert_equals(ref, ("ignore_eot", step))
    assert ref.fin_count.tolist() == [3, 3] and ref.done.tolist() == [0, 0, 0, 1, 1, 1] and ref.live_len.tolist() == [0, 5]
    assert ref.min_gap >= 2 * STEP_TOL and {"row_limit", "pool_overflow"} <= ref.events


# ---- cache reorder ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.int8, torch.float16])
@pytest.mark.parametrize("n_head", [2, 20])
def test_kv_reorder_moves_exactly_the_parents_prefix(lib, dtype, n_head):
    K, n_audio, cap, n_layer = 4, 4, 448, 3
    rows = K * n_audio
    g = torch.Generator().manual_seed(n_head)
    # utterance 0: identity; 1: one cycle over all beams; 2: one parent feeds every beam; 3: a mix, flagged done in a second pass
    parent = torch.tensor([0, 1, 2, 3, 5, 6, 7, 4, 10, 10, 10, 10, 13, 13, 14, 12], dtype=torch.int32)
    for n_last, use_counter in ((1, False), (63, True), (64, False), (65, True), (300, False)):
        for done_rows in ((), (12, 13, 14, 15)):
            layers = [torch.randint(-128, 128, (rows, 2, n_head, cap, 64), generator=g, dtype=torch.int16).to(dtype).cuda()
                      for _ in range(n_layer)]
            before = [t.clone() for t in layers]
            table = torch.tensor([t.data_ptr() for t in layers], dtype=torch.int64, device="cuda")
            done = torch.zeros(rows, dtype=torch.int32)
            done[list(done_rows)] = 1
            counter = torch.tensor([n_last], dtype=torch.int32, device="cuda")
            pd, dd = parent.cuda(), done.cuda()
            native.check(lib.wm_kv_reorder(table.data_ptr(), n_layer, rows, K, n_head, cap, layers[0].element_size(), pd.data_ptr(),
                                           dd.data_ptr(), -1 if use_counter else n_last, counter.data_ptr() if use_counter else None,
                                           stream()), "wm_kv_reorder")
            torch.cuda.synchronize()
            src = parent.long().clone()
            src[list(done_rows)] = torch.tensor(list(done_rows), dtype=torch.long)      # a complete utterance is skipped
            for got, old in zip(layers, before):
                want = old.clone()
                want[:, :, :, :n_last + 1] = old[src.cuda()][:, :, :, :n_last + 1]
                assert torch.equal(got, want), (n_last, done_rows)                      # the prefix moved, every other byte untouched


# ---- end to end ------------------------------------------------------------------------------------------------------
def build_engine(tmp, checkpoint, tag, weight_only=False, kv_scales=None):
    out = os.path.join(tmp, f"eng_{tag}")
    argv = ["--output_dir", out, "--use_gpt_attention_plugin", "--use_gemm_plugin", "--use_layernorm_plugin", "--log_level", "error"]
    if weight_only:
        argv.append("--use_weight_only")
    if kv_scales is not None:
        qdir = os.path.join(tmp, f"quantize_{tag}", "1-gpu")
        os.makedirs(qdir, exist_ok=True)
        for i, s in enumerate(kv_scales):
            np.array([s], dtype=np.float32).tofile(os.path.join(qdir, f"model.decoder.blocks.{i}.attn.query_key_value.scale_y_quant_orig.bin"))
        argv += ["--int8_kv_cache", "--quantize_dir", qdir]
    B.build_from_checkpoint(checkpoint, B.parse_arguments(argv))
    return Path(out)


def peaked_checkpoint(seed=3):
    """micro-fullvocab with logits of std 16 (the stock 1.5 puts a third of the adjacent candidates within 0.06) and the EOT
    embedding at 1.05 x that of the token this random model proposes most often, so that EOT outbids it now and then."""
    dims = Dims(**synthetic.DIMS["micro-fullvocab"])
    sd = synthetic_state_dict(dims, seed, logit_std=16.0)
    E = sd["decoder.token_embedding.weight"]
    E[EOT] = (E[34532].float() * 1.05).half()
    return dims, sd


@pytest.fixture(scope="module")
def engines(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("beam_engines"))
    dims, sd = peaked_checkpoint()
    ck = {"dims": dict(synthetic.DIMS["micro-fullvocab"]), "model_state_dict": sd}
    mel = synthetic_mel(4, 2 * dims.n_audio_ctx, dims.n_mels, 77)
    scales = OracleModel(dims, sd, OracleConfig(act="float16", weight_only=True)).calibrate_kv_scales(mel[:2], 5)
    return dict(dims=dims, mel=mel, fp16=build_engine(tmp, ck, "fp16"), int8=build_engine(tmp, ck, "int8", True, scales))


def candidates(dec, tokens, sums):
    toks, lps = dec.decoder.finalize(tokens, sums)
    return [[t.tolist() for t in u] for u in toks], lps


def run_both(engines, kind, K, n_clips, patience=None, sample_len=24):
    """The device loop (twice: the second run replays the captured graphs) and the literal loop on the same features; the
    literal loop's own candidate gaps, reorders and completions are recorded on the way."""
    eng = engines[kind]
    opts = DecodingOptions(beam_size=K, patience=patience, sample_len=sample_len)
    enc, dec = WhisperEncoding(eng), WhisperDecoding(eng, options=opts)
    xa = enc.get_audio_features(engines["mel"][:n_clips].cuda())
    languages, _ = dec.detect_language(xa)
    out = []
    for _ in range(2):
        t, lp, nsp = dec.main_loop(xa)
        out.append((candidates(dec, t, lp), dec.post_process(t, lp, nsp, xa, languages), nsp))
    stats = dict(min_gap=np.inf, reorders=0)
    update = dec.decoder.update

    def recording_update(tokens, logits, sum_logprobs):
        lp_rows = torch.log_softmax(logits.float(), dim=-1).cpu().numpy()
        sums_in = sum_logprobs.cpu().numpy().astype(np.float32)
        frozen = list(dec.decoder.completed) if len(dec.decoder.pool) == tokens.shape[0] // K else [False] * (tokens.shape[0] // K)
        raw = logits.cpu().numpy()
        for a in range(tokens.shape[0] // K):
            if frozen[a]:
                continue
            cands = [(np.float32(sums_in[a * K + j] + lp_rows[a * K + j, t]), j, t)
                     for j in range(1 if tokens.shape[1] == dec.sample_begin else K) for t in dec.decoder.propose(lp_rows[a * K + j])]
            cands.sort(key=lambda c: (-c[0], c[1], c[2]))
            n_live, stop = 0, len(cands) - 1
            for i, c in enumerate(cands):
                n_live += c[2] != EOT
                if n_live == K:
                    stop = i
                    break
            for c0, c1 in zip(cands[:stop + 1], cands[1:stop + 2]):
                if not (c0[1] == c1[1] and raw[a * K + c0[1], c0[2]] == raw[a * K + c1[1], c1[2]]):
                    stats["min_gap"] = min(stats["min_gap"], float(c0[0] - c1[0]))
        res = update(tokens, logits, sum_logprobs)
        stats["reorders"] += int((res[2].cpu() != torch.arange(tokens.shape[0])).sum())
        return res
    dec.decoder.update = recording_update
    try:
        t, lp, nsp = dec.main_loop_reference(xa)
    finally:
        dec.decoder.update = update
    stats["completed"] = list(dec.decoder.completed)
    stats["pool"] = [len(p) for p in dec.decoder.pool]
    ref = (candidates(dec, t, lp), dec.post_process(t, lp, nsp, xa, languages), nsp)
    return dec, out, ref, stats


def assert_same_candidates(got, ref):
    (g_tok, g_lp), g_res, g_nsp = got
    (r_tok, r_lp), r_res, r_nsp = ref
    assert g_tok == r_tok
    for a, b in zip(g_lp, r_lp):
        np.testing.assert_allclose(a, b, rtol=0, atol=LOOP_TOL)
    assert [r.text for r in g_res] == [r.text for r in r_res] and [r.tokens for r in g_res] == [r.tokens for r in r_res]
    assert np.allclose(g_nsp, r_nsp, atol=1e-4)


@pytest.mark.parametrize("kind", ["fp16", "int8"])
@pytest.mark.parametrize("K", [5, 3])
def test_device_beam_loop_equals_literal_loop(engines, kind, K):
    """micro-fullvocab with peaked logits (`peaked_checkpoint`, seed 3), 3 clips, sample_len 24: main_loop (eager, then
    replayed graphs) and main_loop_reference give identical candidate lists per utterance and the same selected text.  The
    literal loop's run must itself be a usable reference: no two walked candidates closer than 4e-3 (twice the sum bound), beams
    that do reorder, an utterance that completes through its pool and one that finalize tops up (checked at beam 5, fp16)."""
    dec, out, ref, stats = run_both(engines, kind, K, 3)
    print(f"beam fixture {kind} K={K}: smallest candidate gap {stats['min_gap']:.4g}, {stats['reorders']} moved rows, "
          f"completed {stats['completed']}, pools {stats['pool']}")
    assert stats["min_gap"] >= 2 * LOOP_TOL, stats
    assert stats["reorders"] > 0
    if K == 5 and kind == "fp16":
        assert any(stats["completed"]) and any(n < K for n in stats["pool"]), stats
    for got in out:
        assert_same_candidates(got, ref)
    if K == 5:          # what beam_size did before this decoder existed: five copies of the greedy sequence
        for cands in ref[0][0]:
            assert len({tuple(c) for c in cands}) == len(cands) >= K


def test_one_clip_takes_the_one_launch_step_and_patience_doubles_the_pool(engines):
    """Five beams of one clip are a five-row group: the decoder step is the one-launch form and must not have given up.
    patience = 2.0: the pool takes ten finished candidates."""
    before = native.chain_status()
    dec, out, ref, stats = run_both(engines, "fp16", 5, 1, patience=2.0)
    after = native.chain_status()
    assert not after["error_pending"] and not after["declined"] and after["launches"] > before["launches"], (before, after)
    assert stats["min_gap"] >= 2 * LOOP_TOL, stats
    assert dec.decoder.max_candidates == 10
    for got in out:
        assert_same_candidates(got, ref)


def test_two_stream_parallel_groups_never_split_an_utterance(engines):
    dec, out, ref, stats = run_both(engines, "int8", 5, 4)
    n_micro, bounds = dec._groups(20)
    assert n_micro == 2 and all(lo % 5 == 0 and hi % 5 == 0 for lo, hi in bounds), bounds
    assert stats["min_gap"] >= 2 * LOOP_TOL, stats
    for got in out:
        assert_same_candidates(got, ref)


def test_row_limit_and_ignore_eot_in_the_device_loop(engines):
    """`row_limit` is per utterance: after that many sampled tokens the utterance is frozen with whatever its pool holds and finalize tops
    it up -- and the other utterances' candidates do not change (a row's result does not depend on its neighbours).  `ignore_eot`: the
    loop runs sample_len steps, EOT candidates are pooled, nothing is frozen."""
    K, n_clips = 5, 3
    enc = WhisperEncoding(engines["fp16"])
    dec = WhisperDecoding(engines["fp16"], options=DecodingOptions(beam_size=K, sample_len=24))
    xa = enc.get_audio_features(engines["mel"][:n_clips].cuda())
    dec.detect_language(xa)
    free, _ = candidates(dec, *dec.main_loop(xa)[:2])
    limit = [3] * K + [1 << 30] * (2 * K)
    t, lp, _ = dec.main_loop(xa, row_limit=limit)
    assert dec.decoder.live_len[0] == dec.sample_begin + 3
    capped, _ = candidates(dec, t, lp)
    assert len(capped[0]) == K and max(len(c) for c in capped[0]) == dec.sample_begin + 3 + 1 and all(c[-1] == EOT for c in capped[0])
    assert capped[1:] == free[1:]
    t, lp, _ = dec.main_loop(xa, ignore_eot=True)
    assert t.shape[1] == dec.sample_begin + 24 and dec.decoder.completed == [False] * n_clips
    assert any(len(p) == dec.decoder.max_candidates for p in dec.decoder.pool)
    assert not (t[:, dec.sample_begin:] == EOT).any()            # live beams never hold EOT: such candidates go to the pool


def test_beam_size_one_returns_the_greedy_tokens(tmp_path_factory):
    """beam_size = 1 on the stock fixture of test_main_loop_fast_equals_reference_loop_and_oracle: the single beam's best
    sequence is the greedy loop's."""
    tmp = str(tmp_path_factory.mktemp("beam1"))
    dims = Dims(**synthetic.DIMS["micro-fullvocab"])
    eng = build_engine(tmp, synthetic.synthetic_checkpoint("micro-fullvocab", 3), "stock")
    mel = synthetic_mel(3, 2 * dims.n_audio_ctx, dims.n_mels, 77)
    enc = WhisperEncoding(eng)
    xa = enc.get_audio_features(mel.cuda())
    greedy = WhisperDecoding(eng)
    greedy.sample_len = 12
    languages, _ = greedy.detect_language(xa)
    t_g, lp_g, nsp_g = greedy.main_loop(xa)
    res_g = greedy.post_process(t_g, lp_g, nsp_g, xa, languages)
    beam = WhisperDecoding(eng, options=DecodingOptions(beam_size=1, sample_len=12))
    beam.detect_language(xa)
    t_b, lp_b, nsp_b = beam.main_loop(xa)
    res_b = beam.post_process(t_b, lp_b, nsp_b, xa, languages)
    assert [r.tokens for r in res_b] == [r.tokens for r in res_g]
    assert np.allclose([r.avg_logprob for r in res_b], [r.avg_logprob for r in res_g], atol=LOOP_TOL)


def test_command_line_options_reach_the_decoder(engines, tmp_path, tmp_path_factory, golden_dir):
    """run.py --beam_size 5 and summarize.py --beam_size 5 --patience 2 build the beam decoder and return a transcript per clip;
    without the flags both build today's DecodingOptions."""
    import shutil
    import run as R
    import summarize as S
    assert S.decoding_options(S.parse_arguments([])) == DecodingOptions() == R.decoding_options(R.parse_arguments([]))
    opts = S.decoding_options(S.parse_arguments(["--beam_size", "5", "--patience", "2"]))
    assert opts.beam_size == 5 and opts.patience == 2.0
    args = R.parse_arguments(["--beam_size", "5", "--engine_dir", str(engines["fp16"]), "--input_file", str(tmp_path / "mel.npy")])
    assert R.decoding_options(args).beam_size == 5
    np.save(tmp_path / "mel.npy", engines["mel"][0].float().numpy())
    result = R.generate(**vars(args))
    assert isinstance(result.text, str) and np.isfinite(result.avg_logprob)
    eng = build_engine(str(tmp_path_factory.mktemp("beam_cli")), synthetic.synthetic_checkpoint("tiny.en", 21), "tiny_en")
    chapter = tmp_path / "ds" / "1089" / "134691"
    chapter.mkdir(parents=True)
    for i in range(3):
        shutil.copy(os.path.join(golden_dir, "librispeech_1089-134691-0000.flac"), chapter / f"1089-134691-000{i}.flac")
    (chapter / "1089-134691.trans.txt").write_text("".join(f"1089-134691-000{i} HE COULD WAIT NO LONGER\n" for i in range(3)))
    report = S.main(S.parse_arguments(["--test_trt_llm", "--engine_dir", str(eng), "--dataset_dir", str(tmp_path / "ds"), "--batch_size", "2",
                                       "--log_level", "error", "--sample_len", "8", "--beam_size", "5", "--patience", "2"]))["whisper-mi355"]
    assert report["utterances"] == 3 and len(report["hypotheses"]) == 3 and np.isfinite(report["wer"])
    assert len(set(report["hypotheses"])) == 1          # the same clip three times, in batches of 2 + 1
