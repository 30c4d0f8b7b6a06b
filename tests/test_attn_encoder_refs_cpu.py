"""tests/attn_encoder_refs.py checked without a GPU: the reference and its tolerance against the encoder attention kernel's stored
outputs, against wrong kernels, and the conditions the input generators promise.

Golden rows: tests/golden/attn_encoder_parent.npz holds outputs of the kernel (15 cases); tests/test_gpu_attn_encoder_bits.py holds
today's kernel to those bytes, this file holds those bytes to the contract: together they tie the kernel to the truth at the
golden shapes without a GPU.  The table the test prints is where c = 0.125 comes from (largest need: 0.03 with the tie slack,
0.33 without it -- one score of t272 that the kernel rounds the other way).

Mutants: the tolerance must be able to tell.  The REFERENCE is made wrong -- a key lost, doubled, leaked from the next clip, the
accumulator's rescale missed, the scores left in fp32 -- and must then miss its own tolerance.

Tie-slack cap (test_tie_slack_cap): the share of a case's elements in which tie_slack exceeds the rest of the tolerance is at most
1 % in every case the GPU tests hold to the reference.  A seed per case cannot bring that about: a key is a tie candidate when
its score lies within 64 * 2^-24 * sum |q_i| |k_i| of a boundary, which 2 to 8 % of all scores do under any seed, and a candidate
leads once w (1 - w) |s| is above about 0.1 -- never at T = 1500 (w < 0.01), in 1 - 4 % of the elements of a `normal` case at
T <= 129, in 3.5 - 6 % of those of a `late` case, whose rows have one to three heavy keys with scores of 8 to 20.  The seeds are
therefore chosen per (clip, query, head): attn_encoder_refs.settled; test_settled_cases_keep_the_recipe says what that leaves
of the draw."""
import numpy as np
import pytest

import attn_encoder_refs as R

gen = R.gen


def as_kernel_output(ref):
    return ref.ref.astype(np.float16)


# ================================================================================================ golden rows
def test_golden_rows_meet_the_tolerance():
    golden = np.load(gen.GOLDEN)
    print("\ncase          elements  misses  need for c (x 2^-10 A): with tie slack / without   tie slack leads")
    worst = 0.0
    for name, (B, T, H, _) in gen.CASES.items():
        qkv = gen.make_qkv(name)
        assert gen.sha(qkv) == str(golden[name + "/in_sha256"]), "the input generator moved"
        ref = R.reference(qkv, B, T, H, gen.kept_rows(name), keep=False)
        got = golden[name + "/rows"]
        ex = ref.excess(got)
        bare = ex + ref.slack / np.maximum(2.0 ** -10 * ref.A, 1e-300)
        bad = ref.violations(got)
        print(f"{name:12s} {got.size:9d} {len(bad):7d}   {ex.max():8.4f} / {bare.max():8.4f} {100 * ref.slack_share():26.2f} %")
        assert len(bad) == 0, f"{name}: first misses (clip, stored row, column) {bad[:6].tolist()}"
        worst = max(worst, ex.max())
    assert worst <= 0.054, "attn_encoder_refs.py derives c = 0.125 from a need of at most 0.054 on these cases"


def test_normal_generator_is_the_golden_one(monkeypatch):
    """draw("normal" / "late") is gen.make_qkv's recipe: given its seed it returns its bytes."""
    for name in ("t300", "t300_late"):
        B, T, H, late = gen.CASES[name]
        monkeypatch.setattr(gen, "seed_of", lambda _n, s=gen.seed_of(name): s)
        q, k, v = R.draw("late" if late else "normal", B, T, H)
        monkeypatch.undo()
        assert np.array_equal(np.concatenate([q, k, v], axis=2).reshape(B * T, -1).view(np.uint16), gen.make_qkv(name).view(np.uint16))


def test_settled_cases_keep_the_recipe():
    """What the choice of seeds per (clip, query, head) changes: never k or v; of q, under 15 % of the units even in the late regime,
    and a redrawn unit is 64 draws of the same distribution (mean 0, standard deviation 64^-0.25)."""
    for case, most in ((("late", 2, 300, 3), 0.15), (("normal", 3, 16, 3), 0.15), (("normal", 1, 1500, 2), 0.0)):
        q0, k0, v0 = R.draw(*case)
        (q, k, v), ref = R.settled(*case)
        assert np.array_equal(k.view(np.uint16), k0.view(np.uint16)) and np.array_equal(v.view(np.uint16), v0.view(np.uint16))
        changed = (q != q0).reshape(case[1], case[2], case[3], 64).any(axis=3)
        print(f"{R.case_name(*case)}: {changed.sum()} of {changed.size} units drawn again; tie slack leads in {100 * ref.slack_share():.2f} %")
        assert changed.mean() <= most
        if changed.sum() >= 30:
            new = q.reshape(case[1], case[2], case[3], 64)[changed].astype(np.float64)
            assert abs(new.mean()) < 0.02 and abs(new.std() - 64 ** -0.25) < 0.02
        assert ref.slack_share() <= R.SLACK_CAP


# ================================================================================================ mutants
def mutant_misses(regime, B, T, H, mutant, rows=None):
    """Share of the elements in which the wrong kernel's output misses the tolerance of the right one."""
    qkv = R.make_case(regime, B, T, H)
    ref = R.reference(qkv, B, T, H, rows, keep=False)
    assert len(ref.violations(as_kernel_output(ref))) == 0, "the reference misses its own tolerance"
    wrong = as_kernel_output(R.reference(qkv, B, T, H, rows, mutant=mutant))
    return len(ref.violations(wrong)) / wrong.size


ROWS_1500 = np.r_[0:16, 700:716, 1484:1500]


@pytest.mark.parametrize("mutant", ["drop_last", "double_last", "leak_next"])
@pytest.mark.parametrize("B,T,H", [(2, 17, 1), (2, 300, 3), (1, 1500, 2)])
def test_a_wrong_key_set_is_caught(B, T, H, mutant):
    """One key of T lost, doubled or leaked: at T = 1500 that moves an output by about 7e-4 |v - ref|, six times the tolerance."""
    share = mutant_misses("normal", B, T, H, mutant, ROWS_1500 if T == 1500 else None)
    print(f"{mutant} at T = {T}: {100 * share:.1f} % of the elements miss the tolerance")
    assert share > 0.5


@pytest.mark.parametrize("mutant", ["drop_last", "double_last", "leak_next"])
@pytest.mark.parametrize("B,T,H", [(2, 17, 1), (2, 300, 3), (1, 1500, 2)])
def test_a_wrong_key_set_is_caught_by_the_uniform_plantings(B, T, H, mutant):
    """v = 1 in row T - 1 alone counts keys: every output of the wrong kernel differs from fp16(1 / T).  (v = 1 everywhere gives 1.0
    for any key set; it is there for the sums and the mask.)"""
    rows = ROWS_1500 if T == 1500 else None
    for regime in ("uniform_ones", "uniform_last"):
        qkv = R.make_case(regime, B, T, H)
        want = np.float16(1.0) if regime == "uniform_ones" else np.float16(1.0 / T)
        right = as_kernel_output(R.reference(qkv, B, T, H, rows, keep=False))
        assert (right.view(np.uint16) == want.view(np.uint16)).all(), regime
    wrong = as_kernel_output(R.reference(qkv, B, T, H, rows, mutant=mutant))
    assert (wrong.view(np.uint16) != want.view(np.uint16)).all()


@pytest.mark.parametrize("regime", ["late", "ascending"])
@pytest.mark.parametrize("B,T,H", [(2, 300, 3), (1, 513, 1)])
def test_a_missed_rescale_is_caught(regime, B, T, H):
    share = mutant_misses(regime, B, T, H, "skip_rescale")
    print(f"{regime} T = {T}: {100 * share:.1f} % of the elements miss the tolerance")
    assert share > 0.5


@pytest.mark.parametrize("B,T,H", [(2, 300, 3), (1, 513, 1)])
def test_unrounded_scores_are_caught(B, T, H):
    """Scores left in fp32: nothing a flat softmax shows (scores of about 1, probabilities of about 1 / T); the late regime's heavy keys,
    with scores of 8 to 20 and fp16 steps of 2^-7 and 2^-6, do."""
    share = mutant_misses("late", B, T, H, "fp32_scores")
    print(f"late T = {T}: {100 * share:.1f} % of the elements miss the tolerance")
    assert share > 0.1


# ================================================================================================ what the generators promise
def cases_of(regime):
    return [c for c in R.referenced_cases() if c[0] == regime]


@pytest.mark.parametrize("regime", [g for g in R.REGIMES if g not in R.EXACT])
def test_tie_slack_cap(regime):
    over = []
    for c in cases_of(regime):
        share = R.cached_reference(*c).slack_share()
        print(f"{R.case_name(*c)}: tie slack leads in {100 * share:.2f} % of the elements")
        if share > R.SLACK_CAP:
            over.append((R.case_name(*c), round(share, 4)))
    assert not over, f"tie_slack exceeds the rest of the tolerance in more than 1 % of the elements of {len(over)} of {len(cases_of(regime))} cases: {over}"


def test_gpu_case_list():
    cases = R.gpu_cases()
    assert len(set(cases)) == len(cases)
    assert all((H <= 3 and B <= 3) or (B, H) == (1, 8) for _, B, _, H in cases)
    assert {T for _, _, T, _ in cases} == set(R.QB2_T) | set(R.QB4_T) | {1500}


def test_ascending_maximum_moves_in_every_tile():
    for c in cases_of("ascending"):
        moved = R.cached_reference(*c).moved[..., 1:]                   # (tile 0 always moves: from -inf)
        assert moved.mean() >= 0.9, (c, moved.mean())
        assert moved[..., :-1].all(), "every full tile behind tile 0 raises the maximum of every row"
        s = R.reference(R.make_case(*c), *c[1:]).scores if c[1:] == (1, 257, 1) else None
        assert s is None or 29 <= np.abs(s).max() <= 32


def test_descending_maximum_never_moves_after_tile_0():
    """Every row, so that no wave's ballot sees a moved maximum: the kernel's any_moved == false path in every tile but the first."""
    for c in cases_of("descending"):
        assert not R.cached_reference(*c).moved[..., 1:].any(), c


def test_one_hot_winners():
    for c in cases_of("one_hot"):
        _, B, T, H = c
        if T == 1500 or (B, H) == (1, 8):
            continue                                                        # (the same recipe; the smaller cases are checked)
        r = R.reference(R.make_case(*c), B, T, H)
        win = np.array(R.one_hot_winners(T))[np.arange(T) % 4]
        assert (r.w.argmax(axis=3) == win[None, None, :]).all(), c
        assert r.w.max(axis=3).min() >= 0.999, c
        s = np.take_along_axis(r.scores, np.broadcast_to(win[None, None, :, None], (B, H, T, 1)), axis=3)[..., 0]
        assert np.abs(s - 40).max() <= 5, "the winner's score is about 40"
        if T > 1:
            others = np.where(np.arange(T)[None, :] == win[:, None], -np.inf, r.scores)
            assert others.max() <= 6
    assert R.one_hot_winners(300) == (0, 299, 255, 256) and R.one_hot_winners(384) == (0, 383, 383, 383)


def test_uniform_expected_values_survive_the_fp32_division():
    """The kernel divides in fp32 and rounds to fp16 then: fp16(fp32(1 / T)) is fp16(1 / T) at every T the tests use."""
    for T in set(R.QB2_UNIFORM_T) | set(R.QB4_ALL_T) | {1500, 300, 17}:
        assert np.float16(np.float32(1.0) / np.float32(T)) == np.float16(1.0 / T), T


def test_padded_cases_hold_the_dense_values():
    B, T, H = 2, 65, 3
    dense, padded = R.make_case("late", B, T, H), R.make_case("late", B, T, H, ld=3 * H * 64 + 8)
    assert padded.shape == (B * T, 3 * H * 64 + 8) and np.isnan(padded[:, 3 * H * 64:]).all()
    assert np.array_equal(padded[:, :3 * H * 64].view(np.uint16), dense.view(np.uint16))
