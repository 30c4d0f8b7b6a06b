"""The cases of tests/rule_edge_refs.py judged on the CPU, before tests/test_gpu_rule_edges.py runs them through the kernels:
the references agree with each other, every case is far from a near-tie, and the cases are ADEQUATE -- a token step whose range
bound is off by one, or that loses one element at a seam of its row walk, gives another token or another sum on at least one of them.
"""
import numpy as np
import pytest

import rule_edge_refs as RE

# a sum must move by more than 10 x the GPU bound for a mutant to count as killed: the GPU test would then fail by a wide margin
KILL_SUM = 10 * RE.SUM_TOL


@pytest.fixture(scope="module", params=list(RE.VOCABS))
def vocab(request):
    """(name, suppress, blank, [(state, cases, oracle results)]) of one vocabulary, computed once."""
    name = request.param
    sup, blank = RE.lists_for(name)
    ids = RE.VOCABS[name]
    base = RE.base_row(ids.n_vocab)
    per_state = []
    for st in RE.states(ids):
        cases = RE.planted_cases(name, st, sup, blank, base)
        rows = np.stack([c.row for c in cases])
        per_state.append((st, cases, rows, RE.oracle_step(rows, name, st, sup, blank)))
    return name, sup, blank, per_state


def test_vocabularies_states_and_edges_are_what_the_cases_claim(vocab):
    name, sup, blank, per_state = vocab
    ids = RE.VOCABS[name]
    V, tb = ids.n_vocab, ids.timestamp_begin
    assert V == {"multilingual": 51865, "gpt2": 51864, "v3": 51866}[name]
    assert ids.no_timestamps in sup and ids.eot in blank and 220 in blank
    assert len(per_state) == 13 and sum(st.apply_rules == 1 for st, *_ in per_state) == 11
    for st, cases, rows, _ in per_state:
        edges = RE.edge_tokens(name, st, sup, blank)
        assert {0, ids.eot - 1, ids.eot, tb - 1, tb, V - 1} <= set(edges)
        assert np.array_equal(rows, rows.astype(np.float16).astype(np.float32))            # fp16-exact
        kinds = {c.kind for c in cases}
        assert {"inside", "mass", "tie"} <= kinds and ("outside" in kinds or st.apply_rules == 0), (st.name, kinds)
        assert len(cases) * 8 <= 400                                                       # a launch stays a few hundred rows
    first = per_state[0][0]
    assert first.hist == () and set(RE.edge_tokens(name, first, sup, blank)) >= {tb + RE.MAX_INITIAL, tb + RE.MAX_INITIAL + 1}


def test_planted_winners_are_chosen_with_wide_margins(vocab):
    """Every case is decided by the oracle the way it was planted, no case is a near-tie of the dominance rule, and the winner leads
    the runner-up (exact planted ties apart) by at least WINNER_GAP_MIN; a mass case loses more than 0.4 with either token."""
    name, sup, blank, per_state = vocab
    worst_dom, worst_gap = np.inf, np.inf
    for st, cases, rows, (tok, s32, s64, dom, masked) in per_state:
        assert np.abs(dom).min() >= RE.DOMINANCE_MIN
        worst_dom = min(worst_dom, np.abs(dom).min())
        for c, t, m, lp in zip(cases, tok, masked, s64):
            assert t == c.planted[0], (st.name, c.kind, c.planted, t)
            if c.trap is not None:
                assert not np.isfinite(m[c.trap]) and c.row[c.trap] == 30.0
            rest = m.copy()
            rest[list(c.planted) if c.kind in ("tie", "seam") else [t]] = -np.inf
            gap = m[t] - rest.max()
            worst_gap = min(worst_gap, gap if c.kind != "mass" else np.inf)
            assert gap >= (0.5 if c.kind == "mass" else RE.WINNER_GAP_MIN), (st.name, c.kind, gap)
            if c.kind == "mass":
                for lost in c.planted:
                    less = m.copy()
                    less[lost] = -np.inf
                    t2 = int(np.argmax(less))
                    assert t2 != t or abs(RE.log_softmax_f64(less[None])[0, t2] - lp) > 0.4
    print(f"{name}: smallest |dominance| {worst_dom:.3g}, smallest winner gap {worst_gap:.3g}")


def test_range_evaluator_with_the_true_ranges_equals_the_oracle(vocab):
    name, sup, blank, per_state = vocab
    worst = 0.0
    for st, cases, rows, (tok, s32, s64, dom, masked) in per_state:
        dead, ranges = RE.listed(name, st, sup, blank), RE.true_ranges(name, st)
        for c, t, a, b in zip(cases, tok, s32, s64):
            got_t, got_lp = RE.range_eval(c.row, ranges, st.apply_rules == 1, dead)
            assert got_t == t, (st.name, c.kind, got_t, t)
            worst = max(worst, abs(got_lp - a), abs(got_lp - b))
            assert abs(got_lp - a) <= 2e-5 and abs(got_lp - b) <= 2e-5, (st.name, c.kind, got_lp, a, b)
    print(f"{name}: range evaluator vs oracle (fp32 and float64), worst |sum difference| {worst:.3g}")


def test_every_range_bound_off_by_one_is_noticed(vocab):
    """Mutation adequacy: of the 8 mutants "one bound +-1" of every state, each one that is not equivalent (same allowed set, same
    class for every allowed token -- judged from the masks alone) changes the token or moves the sum by more than KILL_SUM on at
    least one case of that state."""
    name, sup, blank, per_state = vocab
    V = RE.VOCABS[name].n_vocab
    n_live = n_equiv = 0
    for st, cases, rows, (tok, s32, s64, dom, masked) in per_state:
        dead, ranges = RE.listed(name, st, sup, blank), RE.true_ranges(name, st)
        for label, mutant in RE.range_mutants(ranges):
            if RE.mutant_is_equivalent(ranges, mutant, V, dead):
                n_equiv += 1
                continue
            n_live += 1
            killed = False
            for c, t, lp in zip(cases, tok, s64):
                got_t, got_lp = RE.range_eval(c.row, mutant, st.apply_rules == 1, dead)
                if got_t != t or abs(got_lp - lp) > KILL_SUM:
                    killed = True
                    break
            assert killed, f"{name} / {st.name}: no case notices {label} ({ranges} -> {mutant})"
    assert n_live >= 30, (n_live, n_equiv)             # the adequacy check is not vacuous
    print(f"{name}: {n_live} range mutants killed, {n_equiv} equivalent")


def test_every_element_lost_at_a_seam_is_noticed():
    """Seam mutants of the plain arg-max cases: for every size and each of the 8 head lengths, skipping element head - 1, head, the
    last one of the 8-wide body or V - 1 (where it exists) changes the token of at least one row."""
    n = 0
    for V in RE.ARGMAX_SIZES:
        for head in range(8):
            rows = RE.argmax_rows(V, head)
            want = [RE.argmax_skipping(x) for x in rows]
            for label, skip in RE.seam_mutants(V, head):
                assert any(RE.argmax_skipping(x, skip) != w for x, w in zip(rows, want)) or V == 1, (V, head, label)
                n += 1
    assert n > 150
    assert {len(RE.seam_mutants(1031, h)) for h in range(8)} == {3, 4}              # head 0 has no "head - 1"


def test_seam_ties_of_the_rule_cases_cover_every_head_length(vocab):
    """With the rules on, the exact ties across (head - 1, head) exist for every head length 1 .. 7 in some state of the vocabulary,
    and the ties across the body/tail seam for every head length whose tail is not empty; skipping the earlier element of a tie
    changes the token."""
    name, sup, blank, per_state = vocab
    V = RE.VOCABS[name].n_vocab
    head_pairs, tail_pairs = set(), set()
    for st, cases, rows, (tok, *_rest) in per_state:
        for c, t in zip(cases, tok):
            if c.kind == "seam":
                a, b = c.planted
                assert t == a and b == a + 1
                (head_pairs if b < 8 else tail_pairs).add(b)
    assert head_pairs == set(range(1, 8))
    assert tail_pairs == {h + 8 * ((V - h) // 8) for h in range(8)} - {V}


def test_sampled_draw_over_the_planted_rows_is_deterministic():
    """g = -log(-log u), u = min(k + 0.5, 2^24 - 1) / 2^24 in fp32 for a 24-bit k (csrc/sample_rng.h): g lies in [-2.853, 16.636].
    A planted winner leads by WINNER_GAP_MIN (0.5 between the two tokens of a mass case) at least, so at T_SAMPLE the scaled gap
    exceeds the whole range of the noise and the draw is the arg-max."""
    lo, hi = RE.gumbel_range()
    assert np.isfinite(lo) and np.isfinite(hi) and -2.86 < lo < -2.85 and 16.63 < hi < 16.64
    assert 0.5 / RE.T_SAMPLE > hi - lo and RE.WINNER_GAP_MIN / RE.T_SAMPLE > hi - lo
    # without the bound the largest k rounds to u = 1 and g = +inf: this is what the bound in sample_rng.h is for
    assert np.float32(16777215.0) + np.float32(0.5) == np.float32(16777216.0)
    u = RE.noise_u(np.arange((1 << 24) - 4, 1 << 24))
    assert (u < 1).all() and (np.diff(u) >= 0).all()
    # unchanged everywhere else: the draws of every other k are the ones the kernel made before
    k = np.random.Generator(np.random.Philox(1)).integers(0, (1 << 24) - 1, 100000)
    assert np.array_equal(RE.noise_u(k), (k.astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0))


def test_recorded_extreme_draw_has_the_largest_noise():
    d = RE.EXTREME_DRAW
    k = RE.noise_counts(d["seed"], d["row"], d["cur_len"], RE.VOCABS["multilingual"].n_vocab)
    assert k[d["token"]] == (1 << 24) - 1 and (k == (1 << 24) - 1).sum() == 1
    assert k.min() >= 0 and k.max() < (1 << 24)


@pytest.mark.parametrize("K", [1, 3, 8])
def test_beam_rows_are_separated_and_the_scarce_contract_agrees_with_npbeam(K):
    """The planted beam rows satisfy draw_separated's conditions in every state, their K + 1 best allowed tokens are planted ones, and
    on such rows -- where every row has its beam_size + 1 proposals -- RE.scarce_beam_step and NpBeam.step leave the same state."""
    import copy
    from test_gpu_beam import NpBeam, draw_separated
    name = "multilingual"
    ids = RE.VOCABS[name]
    sup, blank = RE.lists_for(name)
    rules = RE.rule_set(name, 1, sup, blank)
    r = np.random.Generator(np.random.Philox(500 + K))
    for st in (s for s in RE.states(ids) if s.apply_rules == 1):
        rows = 2 * K
        sums = -0.37 * (np.arange(rows) % K) - 0.11 * (np.arange(rows) // K)
        ref = NpBeam(2, K, K, 16, [RE.context(ids, st)] * rows, sums)
        cur = RE.SAMPLE_BEGIN + len(st.hist)
        x = draw_separated(ref, lambda: RE.beam_rows(name, st, sup, blank, K, rows, r), cur, rules)
        masked = RE.oracle_filter(x, name, st, sup, blank)
        assert (np.sort(masked, axis=1)[:, -(K + 1):] >= 20.0 - 0.75 * (K + 2) - 0.5).all()           # planted values, not the N(0, 1) base
        other = copy.deepcopy(ref)
        ref.step(x, cur, rules)
        RE.scarce_beam_step(other, x, cur, rules)
        for f in ("tokens", "sums", "parent", "fin_tokens", "fin_scores", "fin_len", "fin_count", "live_len", "done"):
            assert np.array_equal(getattr(ref, f), getattr(other, f)), (st.name, f)
        assert ref.n_done == other.n_done and ref.min_gap == other.min_gap and "ended" not in other.events
