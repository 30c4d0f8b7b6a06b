"""The token-step kernels (csrc/greedy.hip, csrc/beam.hip, csrc/truncate.hip over csrc/logit_rules.h) at the edges of the allowed
token ranges and at the seams of their row walk, on the planted rows of tests/rule_edge_refs.py (judged adequate on the CPU by
tests/test_rule_edges_cpu.py: a range bound off by one or an element lost at a seam changes a token or moves a sum by 10 x the bound).

References: oracle/decoding_rules.apply_filters + greedy_update for the token (pinned to the reference's classes by the golden), a
float64 log-softmax of the same masked row for the booked sum; tests/test_gpu_beam.NpBeam for the beam state.
Bounds (both taken from the existing tests, not fitted here): |sum - float64| <= 2e-4 for one greedy or sampled step
(tests/test_gpu_kernels.py::test_greedy_step_*), STEP_TOL = 2e-4 of tests/test_gpu_beam.py for beam sums; everything else is exact.
Every test prints its worst |sum - float64|.

Launch shape: one launch per (vocabulary, state, mode); every case sits on 8 consecutive rows of odd stride (V or V + 1), so that its
replicas start at all 8 phases of 16 bytes -- asserted from the addresses; the token and sum buffers lie between sentinels.
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import native  # noqa: E402
import rule_edge_refs as RE  # noqa: E402
import truncate_refs as TR  # noqa: E402
from oracle import decoding_rules as DR  # noqa: E402
from test_gpu_beam import STEP_TOL, DevBeam, NpBeam, draw_separated  # noqa: E402

SENT_TOK, SENT_SUM = -777, 12345.0
STATE_NAMES = [s.name for s in RE.states(RE.VOCABS["multilingual"])]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return native.load_library()


def stream():
    return torch.cuda.current_stream().cuda_stream


def head_of(addr):
    """Tokens in front of the first 16-byte boundary of a row that starts at `addr` (the kernels' `head`)."""
    return ((16 - (addr & 15)) & 15) >> 1


@functools.lru_cache(maxsize=None)
def lists(name):
    return RE.lists_for(name)


@functools.lru_cache(maxsize=4)
def prepared(name, state_name):
    """(state, cases, oracle results) of one (vocabulary, state): computed once and shared by the two temperatures, which run one
    after the other; never modified."""
    sup, blank = lists(name)
    st = next(s for s in RE.states(RE.VOCABS[name]) if s.name == state_name)
    cases = RE.planted_cases(name, st, sup, blank)
    rows = np.stack([c.row for c in cases])
    return st, cases, rows, RE.oracle_step(rows, name, st, sup, blank)


class Rows:
    """fp16 rows at an odd stride in one flat buffer, the token and sum buffers between sentinels."""

    def __init__(self, rows, context, ld=16):
        B, V = rows.shape
        self.B, self.V, self.cur, self.ld = B, V, len(context), ld
        self.stride = V if V % 2 else V + 1
        self.flat = torch.full((B * self.stride + 8,), 3.0, dtype=torch.float16, device="cuda")
        self.lg = torch.as_strided(self.flat, (B, V), (self.stride, 1))
        self.lg.copy_(torch.from_numpy(rows.astype(np.float16)))
        self.before = self.flat.clone()
        self.tok_all = torch.full((B + 2, ld), SENT_TOK, dtype=torch.int32, device="cuda")
        self.tok = self.tok_all[1:B + 1]
        self.tok[:, :self.cur] = torch.from_numpy(np.asarray(context, dtype=np.int32)).cuda()
        self.sum_all = torch.full((B + 2,), SENT_SUM, dtype=torch.float32, device="cuda")
        self.sums = self.sum_all[1:B + 1]
        self.sums.zero_()
        self.n_done = torch.zeros(3, dtype=torch.int32, device="cuda")           # [1] is the counter, its neighbours stay 0
        self.done_all = torch.full((B + 2,), SENT_TOK, dtype=torch.int32, device="cuda")
        self.done = self.done_all[1:B + 1]
        self.done.zero_()
        self.heads = [head_of(self.flat.data_ptr() + 2 * b * self.stride) for b in range(B)]

    def greedy_io(self, g, ids, sup_d, blank_d, apply_rules, T=0.0, seed=0, row0=0):
        g.logits, g.row_stride, g.batch, g.n_vocab = self.flat.data_ptr(), self.stride, self.B, self.V
        g.tokens, g.tokens_ld, g.cur_len = self.tok.data_ptr(), self.ld, self.cur
        g.sum_logprobs = self.sums.data_ptr()
        g.suppress, g.n_suppress = (sup_d.data_ptr(), sup_d.numel()) if sup_d is not None else (None, 0)
        g.blank, g.n_blank = (blank_d.data_ptr(), blank_d.numel()) if blank_d is not None else (None, 0)
        g.sample_begin, g.eot, g.timestamp_begin = RE.SAMPLE_BEGIN, ids.eot, ids.timestamp_begin
        g.max_initial_timestamp_index, g.apply_rules = RE.MAX_INITIAL, apply_rules
        g.n_done, g.done = self.n_done[1:].data_ptr(), self.done.data_ptr()
        g.temperature, g.row0, g.seed = T, row0, seed

    def greedy(self, lib, *a, **kw):
        io = native.WmGreedyIO()
        self.greedy_io(io, *a, **kw)
        native.check(lib.wm_greedy_step(C.byref(io), stream()), "wm_greedy_step")
        torch.cuda.synchronize()

    def sample(self, lib, ids, sup_d, blank_d, apply_rules, T, seed=0, row0=0, top_k=0):
        io = native.WmSampleIO()
        self.greedy_io(io.g, ids, sup_d, blank_d, apply_rules, T, seed, row0)
        c, P, gap = TR.scalars(T, 1.0, 0.0)
        io.top_k, io.exp2_scale, io.top_p_q16, io.min_p_gap = top_k, float(c), P, float(gap)
        self.cut = torch.full((self.B,), 7.0, dtype=torch.float32, device="cuda")
        self.kept = torch.full((self.B,), -7, dtype=torch.int32, device="cuda")
        io.cut_out, io.kept_out = self.cut.data_ptr(), self.kept.data_ptr()
        native.check(lib.wm_sample_step(C.byref(io), stream()), "wm_sample_step")
        torch.cuda.synchronize()

    def assert_sentinels(self):
        assert (self.tok_all[0] == SENT_TOK).all() and (self.tok_all[-1] == SENT_TOK).all()
        assert (self.tok[:, self.cur + 1:] == SENT_TOK).all()                    # one token appended per row, nothing behind it
        assert self.sum_all[0] == SENT_SUM and self.sum_all[-1] == SENT_SUM
        assert self.done_all[0] == SENT_TOK and self.done_all[-1] == SENT_TOK
        assert self.n_done[0] == 0 and self.n_done[2] == 0

    def assert_rows_written_only_where_listed(self, dead):
        """After the call the rows read -inf at the tokens the lists name (`dead`, bool [V]) and nowhere else; every other element
        of the buffer, the gaps between the rows included, holds the bits it held before."""
        want = self.before.clone()
        view = torch.as_strided(want, (self.B, self.V), (self.stride, 1))
        view[:, torch.from_numpy(np.nonzero(dead)[0]).cuda()] = float("-inf")
        assert torch.equal(self.flat.view(torch.int16), want.view(torch.int16))


def replicate(x, n=8):
    return np.repeat(x, n, axis=0)


def run_state(lib, name, state_name, T):
    ids = RE.VOCABS[name]
    sup, blank = lists(name)
    st, cases, rows, (tok, s32, s64, dom, masked) = prepared(name, state_name)
    keep = [i for i, c in enumerate(cases) if T == 0 or c.sample]
    io = Rows(replicate(rows[keep]), RE.context(ids, st))
    for i in range(len(keep)):                                      # input condition: the replicas of a case start at all 8 phases
        assert sorted(io.heads[8 * i:8 * i + 8]) == list(range(8))
    assert io.stride % 2 == 1 and io.flat.data_ptr() % 16 == 0
    sup_d = torch.tensor(sup, dtype=torch.int32, device="cuda")
    blank_d = torch.tensor(blank, dtype=torch.int32, device="cuda")
    io.greedy(lib, ids, sup_d, blank_d, st.apply_rules, T=T, seed=0xC0FFEE1234, row0=17)
    got = io.tok[:, io.cur].cpu().numpy().reshape(len(keep), 8)
    got_sum = io.sums.cpu().numpy().astype(np.float64).reshape(len(keep), 8)
    want, want_sum = tok[keep], s64[keep]
    worst = np.abs(got_sum - want_sum[:, None]).max()
    print(f"{name} / {state_name} / T = {T}: {len(keep)} cases x 8 phases, worst |sum - float64| = {worst:.3g} (bound {RE.SUM_TOL})")
    for i, k in enumerate(keep):
        assert (got[i] == want[i]).all(), (name, state_name, cases[k].kind, cases[k].planted, cases[k].trap, got[i], want[i])
    assert worst <= RE.SUM_TOL
    n_eot = int((want == ids.eot).sum()) * 8
    assert int(io.n_done[1]) == n_eot
    assert np.array_equal(io.done.cpu().numpy().reshape(len(keep), 8), np.repeat((want == ids.eot)[:, None], 8, axis=1).astype(np.int32))
    io.assert_rows_written_only_where_listed(RE.listed(name, st, sup, blank))
    io.assert_sentinels()
    return cases, keep


@pytest.mark.parametrize("T", [0.0, RE.T_SAMPLE])
@pytest.mark.parametrize("state_name", STATE_NAMES)
@pytest.mark.parametrize("name", list(RE.VOCABS))
def test_greedy_step_at_every_edge_and_phase(lib, name, state_name, T):
    """wm_greedy_step.  Temperature 0, every case: the oracle's token in every row (hence the same over the 8 replicas), the sum
    within the bound, -inf written exactly where the lists say, n_done and done right, sentinels intact.  Temperature 0.01 with a
    fixed seed, the inside, outside and mass cases: the scaled gaps exceed the whole range of the noise
    (tests/test_rule_edges_cpu.py), so the draw is the planted winner; the booked log-probability is the unperturbed one at
    temperature 1 -- and everything else as at temperature 0."""
    cases, keep = run_state(lib, name, state_name, T)
    kinds = {cases[k].kind for k in keep}
    assert {"inside", "mass"} <= kinds and (("tie" in kinds) == (T == 0)) and (T == 0 or "seam" not in kinds)


def test_largest_noise_does_not_override_the_logits(lib):
    """The one draw in 2^24 whose noise is the generator's largest (RE.EXTREME_DRAW, found by search on the host): the token it falls
    on has an ordinary logit, the planted winner leads by 20 / T.  (Without the bound in csrc/sample_rng.h that noise was +inf.)"""
    d, name = RE.EXTREME_DRAW, "multilingual"
    ids = RE.VOCABS[name]
    sup, blank = lists(name)
    st = next(s for s in RE.states(ids) if s.name == "ts_txt")
    assert len(RE.context(ids, st)) == d["cur_len"] and RE.allowed_mask(name, st, sup, blank)[d["token"]]
    x = RE.base_row(ids.n_vocab)[None].copy()
    x[0, 1000] = 20.0
    tok, s32, s64, dom, masked = RE.oracle_step(x, name, st, sup, blank)
    assert tok[0] == 1000 and np.isfinite(masked[0, d["token"]])
    sup_d, blank_d = torch.tensor(sup, dtype=torch.int32, device="cuda"), torch.tensor(blank, dtype=torch.int32, device="cuda")
    for step in ("greedy", "sample"):
        io = Rows(x, RE.context(ids, st))
        getattr(io, step)(lib, ids, sup_d, blank_d, 1, T=RE.T_SAMPLE, seed=d["seed"], row0=d["row"])
        assert int(io.tok[0, io.cur]) == 1000, (step, int(io.tok[0, io.cur]))
        assert abs(float(io.sums[0]) - s64[0]) <= RE.SUM_TOL
        io.assert_sentinels()


# ---- plain arg-max ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", RE.ARGMAX_SIZES)
def test_argmax_and_plain_greedy_step_at_every_seam(lib, V):
    """wm_argmax and wm_greedy_step(apply_rules = 0) on rows of V logits at all 8 phases: the winner at 0, head - 1, head, V - 1, exact
    ties across the head/body and the body/tail seam (the first index wins)."""
    stride = V if V % 2 else V + 1
    blocks = [RE.argmax_rows(V, h) for h in range(8)]
    n = max(len(b) for b in blocks)
    # row 8 * i + r holds case i of the head length that row has: with a 16-byte-aligned buffer row b starts b * stride tokens in
    heads = [head_of(2 * b * stride) for b in range(8)]
    assert sorted(heads) == list(range(8))
    rows, want = [], []
    for i in range(n):
        for r in range(8):
            blk = blocks[heads[r]]
            rows.append(blk[i % len(blk)])
            want.append(RE.argmax_skipping(rows[-1]))
    rows = np.stack(rows)
    io = Rows(rows, [7, 7, 7])
    assert io.flat.data_ptr() % 16 == 0 and io.heads == heads * n and io.stride == stride
    ids_out = torch.full((len(rows) + 2,), SENT_TOK, dtype=torch.int32, device="cuda")
    native.check(lib.wm_argmax(io.flat.data_ptr(), stride, len(rows), V, ids_out[1:].data_ptr(), stream()), "wm_argmax")
    torch.cuda.synchronize()
    assert ids_out[1:-1].tolist() == want and ids_out[0] == SENT_TOK and ids_out[-1] == SENT_TOK
    ids = DR.SpecialIds(V + 10)                                     # no token of the row is EOT or a timestamp
    io.greedy(lib, ids, None, None, 0)
    assert io.tok[:, io.cur].tolist() == want
    lp = RE.log_softmax_f64(rows)[np.arange(len(rows)), want]
    worst = np.abs(io.sums.cpu().numpy() - lp).max()
    print(f"plain arg-max, V = {V}: {len(rows)} rows, worst |sum - float64| = {worst:.3g} (bound {RE.SUM_TOL})")
    assert worst <= RE.SUM_TOL and int(io.n_done[1]) == 0 and not io.done.any()
    assert torch.equal(io.flat.view(torch.int16), io.before.view(torch.int16))
    io.assert_sentinels()


# ---- a row with nothing to choose from ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step,T", [("greedy", 0.0), ("greedy", 0.7), ("sample", 0.7)])
def test_row_without_a_finite_allowed_logit_ends(lib, step, T):
    """The contract of include/whisper_mi355.h: such a row takes EOT, is flagged done and counted, and its sum becomes -inf; the
    normal rows beside it are decided as if it were not there.  Row 2 has no finite logit at all; row 5 has finite logits only on
    tokens the rules forbid: timestamps that would run backwards and suppressed tokens.  (Before the contract was stated the
    kernels appended 0x7fffffff to such a row, booked NaN and neither flagged nor counted it.)"""
    name = "multilingual"
    ids = RE.VOCABS[name]
    V, tb = ids.n_vocab, ids.timestamp_begin
    sup, blank = lists(name)
    st = next(s for s in RE.states(ids) if s.name == "pair_txt")            # allowed: text, timestamps from tb + 41 on
    x = np.stack([RE.base_row(V, seed=40 + b) for b in range(8)])
    x[np.arange(8), 1000 + np.arange(8)] = 20.0
    x[2] = -np.inf
    x[5] = -np.inf
    x[5, [tb, tb + 40, sup[0], ids.no_timestamps]] = 9.0
    normal = [0, 1, 3, 4, 6, 7]
    tok, s32, s64, dom, masked = RE.oracle_step(x[normal], name, st, sup, blank)
    with np.errstate(invalid="ignore"):                              # (the oracle's log-softmax of a row without a finite value)
        assert not np.isfinite(RE.oracle_filter(x[[2, 5]], name, st, sup, blank)).any()
    io = Rows(x, RE.context(ids, st))
    io.sums[:] = torch.arange(8, device="cuda") * -0.5
    sup_d, blank_d = torch.tensor(sup, dtype=torch.int32, device="cuda"), torch.tensor(blank, dtype=torch.int32, device="cuda")
    getattr(io, step)(lib, ids, sup_d, blank_d, 1, T=T, seed=99)
    got, sums = io.tok[:, io.cur].cpu().numpy(), io.sums.cpu().numpy().astype(np.float64)
    print(f"{step} T = {T}: empty rows -> tokens {got[[2, 5]].tolist()}, sums {sums[[2, 5]].tolist()}, done {io.done[[2, 5]].tolist()}, "
          f"n_done {int(io.n_done[1])}")
    assert got[[2, 5]].tolist() == [ids.eot, ids.eot] and np.isneginf(sums[[2, 5]]).all()
    assert io.done.tolist() == [0, 0, 1, 0, 0, 1, 0, 0] and int(io.n_done[1]) == 2
    if T == 0:
        assert np.array_equal(got[normal], tok)
    else:                                       # a draw: any allowed token; its log-probability is booked at temperature 1
        assert np.isfinite(masked[np.arange(6), got[normal]]).all()
        s64 = RE.log_softmax_f64(masked)[np.arange(6), got[normal]]
    worst = np.abs(sums[normal] - (np.array(normal) * -0.5 + s64)).max()
    print(f"normal rows beside them: worst |sum - float64| = {worst:.3g} (bound {RE.SUM_TOL})")
    assert worst <= RE.SUM_TOL
    if step == "sample":
        assert io.kept[[2, 5]].tolist() == [0, 0] and torch.isneginf(io.cut[[2, 5]]).all()
    io.assert_sentinels()


# ---- beam --------------------------------------------------------------------------------------------------------------------------
def beam_rules(max_initial=RE.MAX_INITIAL):
    sup, blank = lists("multilingual")
    return DR.RuleSet(DR.MULTILINGUAL, RE.SAMPLE_BEGIN, list(sup), list(blank), max_initial)


def beam_sum_error(gpu, ref):
    a, b = gpu.sums.cpu().numpy().astype(np.float64), ref.sums.astype(np.float64)
    both = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(np.isneginf(a), np.isneginf(b)) and not np.isnan(a).any()
    return float(np.abs(a[both] - b[both]).max()) if both.any() else 0.0


@pytest.mark.parametrize("K", [1, 3, 8])
def test_beam_step_at_every_edge(lib, K):
    """wm_beam_step on rows whose beam_size + 1 best tokens are planted inside-edge tokens (the first and last finite token of each
    allowed class among them) under disallowed edge tokens at 30: the first sampled step and one later step per state, two
    utterances, the whole state against NpBeam.  The inputs satisfy draw_separated's conditions, judged by numpy alone."""
    name, n_audio, ld = "multilingual", 2, 16
    ids = RE.VOCABS[name]
    sup, blank = lists(name)
    rules = beam_rules()
    r = np.random.Generator(np.random.Philox(500 + K))
    worst, min_gap = 0.0, np.inf
    for n, st in enumerate(s for s in RE.states(ids) if s.apply_rules == 1):
        rows = n_audio * K
        sums = -0.37 * (np.arange(rows) % K) - 0.11 * (np.arange(rows) // K)
        ref = NpBeam(n_audio, K, K, ld, [RE.context(ids, st)] * rows, sums)
        gpu = DevBeam(lib, ref, rules)
        cur = RE.SAMPLE_BEGIN + len(st.hist)
        x = draw_separated(ref, lambda: RE.beam_rows(name, st, sup, blank, K, rows, r), cur, rules)
        full = RE.allowed_mask(name, st, sup, blank)
        traps = [t for t in RE.edge_tokens(name, st, sup, blank) if not full[t]]
        assert (x[:, traps] == 30.0).all() and x[:, full].max() <= 20.0
        ref.step(x, cur, rules)
        gpu.step(x, cur, use_counter=bool(n % 2))
        worst = max(worst, beam_sum_error(gpu, ref))
        gpu.assert_equals(ref, (K, st.name))
        ends = {t for e in RE.class_ends(full, ids.timestamp_begin) for t in e}
        if K > 1:                                                   # a class end is among the tokens the step appended or pooled
            assert ends & (set(ref.tokens[:, cur].tolist()) | ({ids.eot} if ref.fin_count.any() else set())), st.name
        min_gap = min(min_gap, ref.min_gap)
    print(f"beam K = {K}: worst |sum - reference| = {worst:.3g} (STEP_TOL {STEP_TOL}), smallest gap between walked candidates {min_gap:.3g}")
    assert min_gap >= 2 * STEP_TOL


@pytest.mark.parametrize("K", [1, 3, 8])
def test_beam_rows_with_too_few_proposals(lib, K):
    """The contract of csrc/beam.hip for rows with fewer than beam_size + 1 finite allowed logits (RE.scarce_beam_step): on the
    first sampled step with max_initial_timestamp_index in {0, 1, K - 1, K}, and on a later step where beam 0 of utterance 0 has only
    m in {1, K, K + 1} finite allowed logits, EOT among them, and its other beams EOT alone -- beside a normal utterance."""
    name, n_audio, ld = "multilingual", 2, 16
    ids = RE.VOCABS[name]
    V, tb, eot = ids.n_vocab, ids.timestamp_begin, ids.eot
    sup, blank = lists(name)
    rows = n_audio * K
    r = np.random.Generator(np.random.Philox(900 + K))
    worst, ended = 0.0, 0

    def run(ref, gpu, make, cur, rules, what):
        nonlocal worst, ended
        for _ in range(50):                                         # draw_separated's input conditions, judged by numpy alone
            x = make()
            trial = copy.deepcopy(ref)
            trial.min_gap, trial.events = np.inf, set()
            RE.scarce_beam_step(trial, x, cur, rules)
            if trial.min_gap >= 1e-3:
                break
        else:
            raise AssertionError(f"no separated logits for {what}")
        RE.scarce_beam_step(ref, x, cur, rules)
        gpu.step(x, cur, use_counter=False)
        worst = max(worst, beam_sum_error(gpu, ref))
        finite = np.isfinite(ref.sums)
        got = gpu.sums.cpu().numpy()
        assert np.array_equal(np.isneginf(got), ~finite), what
        gpu.sums[torch.from_numpy(~finite).cuda()] = 0.0            # assert_allclose cannot compare -inf with -inf - (-inf)
        shadow = copy.deepcopy(ref)
        shadow.sums[~finite] = 0.0
        gpu.assert_equals(shadow, what)
        ended += "ended" in ref.events

    first = next(s for s in RE.states(ids) if s.name == "first")
    for mi in sorted({0, 1, K - 1, K}):
        rules = beam_rules(mi)
        ref = NpBeam(n_audio, K, K, ld, [RE.context(ids, first)] * rows)
        gpu = DevBeam(lib, ref, rules)

        def make_first():
            x = np.stack([RE.base_row(V, seed=300 + b) for b in range(rows)])
            x[:, tb + mi + 1] = 30.0                                # the first timestamp past the bound: must be ignored
            for b in range(rows):
                x[b, tb:tb + mi + 1] = 12.0 - 0.75 * ((np.arange(mi + 1) + b) % (mi + 1))
            return x
        run(ref, gpu, make_first, RE.SAMPLE_BEGIN, rules, ("first", K, mi))
        assert ("ended" in ref.events) == (mi + 1 < K), (K, mi)
        assert sorted(set(ref.tokens[:K, RE.SAMPLE_BEGIN].tolist()) - {eot}) == list(range(tb, tb + min(mi + 1, K)))
    later = next(s for s in RE.states(ids) if s.name == "ts_txt")
    rules = beam_rules()
    for m in sorted({1, K, K + 1}):
        sums = -0.37 * (np.arange(rows) % K) - 0.11 * (np.arange(rows) // K)
        ref = NpBeam(n_audio, K, K, ld, [RE.context(ids, later)] * rows, sums)
        gpu = DevBeam(lib, ref, rules)
        cur = RE.SAMPLE_BEGIN + len(later.hist)
        few = 2000 + 5 * np.arange(m - 1)
        assert not set(few.tolist()) & set(sup)

        def make_later():
            x = RE.beam_rows(name, later, sup, blank, K, rows, r)   # utterance 1: normal rows
            x[:K] = -np.inf
            x[:K, eot] = 5.0 - 0.25 * np.arange(K) - 0.0625 * int(r.integers(0, 8))
            x[:K, [tb, tb + 3, sup[0]]] = 30.0                      # forbidden tokens are no proposals
            x[0, few] = 8.0 - 0.75 * np.arange(m - 1)
            return x
        run(ref, gpu, make_later, cur, rules, ("later", K, m))
        assert ("ended" in ref.events) == (m - 1 < K) and (ref.fin_count[0] >= 1 or m > K), (K, m)      # a beam that ends had EOT pooled
    print(f"scarce beam K = {K}: worst |sum - reference| = {worst:.3g} (STEP_TOL {STEP_TOL}), {ended} steps ended a beam")
    assert ended >= 1
