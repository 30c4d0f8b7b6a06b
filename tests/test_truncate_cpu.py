"""Top-k / top-p / min-p sampling on the host: truncation.py (the contract) against the brute force of tests/truncate_refs.py and against a
float64 Hugging Face-style implementation, the error bound of the fixed-point weights, the refusals, the literal loop's sampler, the
command lines, the header and the binding."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import native
import run
import summarize
import transcribe
import truncate_refs as TR
import truncation as TN
from decoding import DecodingOptions, GreedyDecoder, WhisperDecoding, check_decoding_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TB = 50364                                   # where the timestamps of the full vocabulary begin


def both(x, T, k=0, p=1.0, q=0.0):
    """(cut, kept) of truncation.py after checking it against the brute force."""
    x = np.asarray(x, dtype=np.float16)
    got = TN.cut(x, T, k, p, q)
    want = TR.Row(x, T).cut(k, p, q)
    assert (float(got[0]), got[1]) == (float(want[0]), want[1]), (T, k, p, q)
    return float(got[0]), got[1]


# ---- the contract against the brute force -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [k for k in TR.KINDS if k != "single"])
def test_cut_equals_the_brute_force_on_the_fixtures(kind):
    for V in (1000, 51865):
        x = TR.fixture_row(kind, V, 17 + V, TB if V > TB else None)
        for T in (0.2, 1.0):
            for k, p, q in TR.controls(V):
                both(x, T, k, p, q)
    assert both(np.asarray([-2.5]), 0.7, 3, 0.4, 0.2) == (-2.5, 1)          # one single finite logit


def test_off_keeps_everything_and_top_k_1_keeps_the_maximum_class():
    x = TR.fixture_row("coarse", 5000, 2)
    x[[7, 70, 700]] = x.max()                                  # the maximum's class has four tokens
    assert both(x, 0.6) == (float(x.min()), x.size)
    assert both(x, 0.6, k=1) == (float(x.max()), 4)
    assert both(x, 0.6, k=x.size) == both(x, 0.6, k=x.size + 7) == (float(x.min()), x.size)       # k >= |A| is off
    assert both(np.asarray([0.0, -0.0, -1.0]), 1.0, k=1) == (0.0, 2)                                 # -0 and +0 are one class


def test_a_tie_across_the_kth_place_is_kept_whole():
    x = np.asarray([5.0, 4.0, 3.0, 3.0, 3.0, 3.0, 2.0, 1.0], dtype=np.float16)
    assert both(x, 1.0, k=2) == (4.0, 2)
    for k in (3, 4, 5, 6):
        assert both(x, 1.0, k=k) == (3.0, 6)
    assert both(x, 1.0, k=7) == (2.0, 7)


def test_top_p_moves_the_cut_by_exactly_one_class_around_a_cumulative_share():
    """Integer weights: T = log2(e) makes c = 1, so the values m, m - 1, m - 2 weigh exactly 2^30, 2^29, 2^28.
    With counts (1, 2, 4) the cumulative shares are 1/3, 2/3 and 1: P just below and just above a share."""
    T = math.log2(math.e)
    assert float(TN.params(T)[0]) == 1.0
    x = np.asarray([3.0] + [2.0] * 2 + [1.0] * 4, dtype=np.float16)
    assert TN.weights(TN.deltas(np.asarray([3.0, 2.0, 1.0], dtype=np.float16)), np.float32(1.0)).tolist() == [1 << 30, 1 << 29, 1 << 28]
    third = 65536 / 3                                          # P = 21845 < 65536 / 3 < 21846
    assert both(x, T, p=21845 / 65536) == (3.0, 1) and both(x, T, p=21846 / 65536) == (2.0, 3)
    assert both(x, T, p=43690 / 65536) == (2.0, 3) and both(x, T, p=43691 / 65536) == (1.0, 7)
    assert math.floor(third) == 21845
    # equal shares that are hit exactly: Q_j * 2^16 >= P * Q holds with equality
    y = np.asarray([3.0, 3.0, 2.0, 2.0, 2.0, 2.0], dtype=np.float16)        # shares 1/2, 1
    assert both(y, T, p=0.5) == (3.0, 2) and both(y, T, p=32769 / 65536) == (2.0, 6)
    # top-p counts the mass of the top-k survivors only
    assert both(x, T, k=3, p=0.6) == (2.0, 3) and both(x, T, k=3, p=0.5) == (3.0, 1) and both(x, T, p=0.5) == (2.0, 3)


def test_the_min_p_boundary_sits_at_the_gap_exactly():
    T, q = 0.5, 0.25
    c, P, gap = TN.params(T, 1.0, q)
    assert P == 65536 and gap == np.float32(T * math.log(q)) and gap < 0
    m = np.float16(4.0)
    at = np.float16(float(m) + float(gap))                     # 4 - 0.693...: round to fp16, then find the two neighbours of the gap
    vals = np.sort(np.asarray([np.nextafter(at, np.float16(-10)), at, np.nextafter(at, np.float16(10))], dtype=np.float16))
    inside = [v for v in vals if np.float32(v) - np.float32(m) >= gap]
    assert 0 < len(inside) < 3
    x = np.concatenate([[m], vals, [np.float16(-3.0)]]).astype(np.float16)
    assert both(x, T, q=q) == (float(min(inside)), 1 + len(inside))
    assert both(x, T, q=0.0) == (-3.0, 5)
    exact = np.asarray([2.0, 1.0, 0.5], dtype=np.float16)      # gap = -1 exactly: d = -1 is kept, d = -1.5 is not
    assert np.float32(1.0 * math.log(math.exp(-1.0))) == np.float32(-1.0)
    assert both(exact, 1.0, q=math.exp(-1.0)) == (1.0, 2)


def test_the_weights_meet_their_error_bound_exhaustively():
    """All fp16 v <= m for five maxima and three temperatures: |q - 2^30 e| <= 1.5e-6 * 2^30 e + 0.5, e = exp((v - m) / T) in float64
    (measured: 1.28e-6; truncation.py states where it comes from); q(m) = 2^30; a token far enough below weighs 0."""
    allv = np.arange(65536, dtype=np.uint16).view(np.float16)
    allv = allv[np.isfinite(allv)]
    worst = 0.0
    for m in (65504.0, 11.5, 0.0, -3.25, -60000.0):
        for T in (0.2, 0.4, 1.0):
            c = TN.params(T)[0]
            v = allv[allv <= np.float16(m)]
            d = v.astype(np.float32) - np.float32(m)
            q = TN.weights(d, c)
            assert q.dtype == np.int64 and q.max() == 1 << 30 and q[v == np.float16(m)].min() == 1 << 30
            e = np.exp((v.astype(np.float64) - m) / T) * 2.0 ** 30
            err = np.abs(q.astype(np.float64) - e)
            assert (err <= 1.5e-6 * e + 0.5).all(), (m, T)
            worst = max(worst, float((np.maximum(err - 0.5, 0.0) / e.clip(1e-300)).max()))
            assert (q[d < np.float32(-31.5) / c] == 0).all() and (q[d > np.float32(-30.4) / c] > 0).all()
            assert TR.class_weights(v[::97], np.float16(m), c) == q[::97].tolist()       # the brute force's restatement, bit for bit
    assert worst > 1e-7                                         # (the bound is not vacuous)


def test_kept_sets_equal_a_float64_hugging_face_implementation():
    """Sort, cumulative softmax and the three warpers in Hugging Face's order, in float64 (truncate_refs.hf_keep).  The kept set is
    identical on rows without a tie at the cut whenever the reference's own margin at the p-boundary exceeds 1e-5 of the mass: the rows
    are picked for that, and the test asserts that it picked enough of them."""
    checked = 0
    for seed in range(40):
        x = TR.fixture_row("normal15" if seed % 2 else "normal3", 1000, 300 + seed)
        for T, k, p, q in ((0.6, 50, 0.9, 0.0), (1.0, 0, 0.5, 0.0), (0.4, 0, 0.95, 0.05), (1.0, 20, 1.0, 0.0), (0.8, 0, 1.0, 0.1), (0.2, 7, 0.3, 0.5)):
            keep, margin = TR.hf_keep(x, T, k, p, q)
            if margin <= 1e-5:
                continue
            lowest = x[keep].min()
            if (x[~keep] == lowest).any():                      # a tie at the cut: Hugging Face splits the class, the contract does not
                continue
            if q > 0:                                           # (the min_p boundary: stay clear of it by the same relative margin)
                z = x.astype(np.float64) / T
                r = np.exp(z - z.max())
                if np.abs(r / q - 1.0).min() <= 1e-4:
                    continue
            cut, kept = TN.cut(x, T, k, p, q)
            assert np.array_equal(x >= cut, keep) and kept == int(keep.sum()), (seed, T, k, p, q)
            checked += 1
    assert checked >= 200


def test_keep_mask_takes_rows_with_forbidden_tokens():
    x = np.stack([TR.fixture_row("normal15", 300, 1), TR.fixture_row("coarse", 300, 2), np.full(300, -np.inf, dtype=np.float16)])
    x[0, ::3] = -np.inf
    mask = TN.keep_mask(x.astype(np.float32), 0.7, 10, 0.9, 0.01)
    assert mask.shape == x.shape and not mask[2].any() and not mask[0, ::3].any()
    for b in (0, 1):
        a = np.isfinite(x[b])
        cut, kept = TR.Row(x[b][a], 0.7).cut(10, 0.9, 0.01)[:2]
        assert np.array_equal(mask[b], a & (x[b] >= cut)) and int(mask[b].sum()) == kept
    assert TN.keep_mask(x[:2], 0.7).sum() == np.isfinite(x[:2]).sum()


# ---- options, refusals, params ----------------------------------------------------------------------------------------------------------
def test_params():
    c, P, gap = TN.params(0.5, 0.9, 0.05)
    assert c == np.float32(math.log2(math.e) / 0.5) and P == round(0.9 * 65536) and gap == np.float32(0.5 * math.log(0.05))
    assert TN.params(1.0) == (np.float32(math.log2(math.e)), 65536, np.float32(-np.inf))
    assert TN.params(1.0, 1e-9)[1] == 1 and TN.params(1.0, 0.9999999)[1] == 65536
    assert (c, P, gap) == TR.scalars(0.5, 0.9, 0.05)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            TN.params(bad)


def test_options_default_to_off_and_bad_values_are_refused():
    o = DecodingOptions()
    assert (o.top_k, o.top_p, o.min_p) == (0, 1.0, 0.0) and not TN.truncation_on(o.top_k, o.top_p, o.min_p)
    check_decoding_options(DecodingOptions(top_k=50, top_p=0.95, min_p=0.05))
    check_decoding_options(DecodingOptions(top_k=50, beam_size=4))                  # inert under beam search, not refused
    for bad in (dict(top_k=-1), dict(top_k=1.5), dict(top_k=True), dict(top_p=0.0), dict(top_p=1.01), dict(top_p=float("nan")),
                dict(top_p=-0.5), dict(min_p=1.0), dict(min_p=-0.1), dict(min_p=float("inf")), dict(min_p=float("nan")), dict(top_p="0.5")):
        with pytest.raises(ValueError):
            check_decoding_options(DecodingOptions(**bad))
    assert TN.truncation_on(1, 1.0, 0.0) and TN.truncation_on(0, 0.99, 0.0) and TN.truncation_on(0, 1.0, 0.01)


@pytest.fixture(scope="module")
def cpu_engine(tmp_path_factory):
    import build as B
    import synthetic
    from oracle.whisper_oracle import Dims, synthetic_state_dict
    dims = Dims(**synthetic.DIMS["micro-fullvocab"])
    out = tmp_path_factory.mktemp("truncate_cpu") / "eng"
    args = B.parse_arguments(["--output_dir", str(out), "--use_gpt_attention_plugin", "--use_gemm_plugin", "--use_layernorm_plugin", "--log_level", "error"])
    B.build_from_checkpoint({"dims": dims.to_dict(), "model_state_dict": synthetic_state_dict(dims, 3)}, args)
    return out


def test_construction_and_the_partitioned_schedule(cpu_engine):
    off = WhisperDecoding(cpu_engine, only_torch=True)
    assert not off.truncation_on and off.decoder.kept is None
    off.cu_partition = True
    off._check_partition(2)
    with pytest.raises(ValueError, match="top_p"):
        WhisperDecoding(cpu_engine, only_torch=True, options=DecodingOptions(top_p=1.5))
    on = WhisperDecoding(cpu_engine, only_torch=True, options=DecodingOptions(temperature=0.7, top_k=40, min_p=0.1))
    assert on.truncation_on and on.decoder.kept == (40, 1.0, 0.1) and on.decoder.temperature == 0.7
    on._check_partition(2)
    on.cu_partition = True
    for n_micro in (1, 2):
        with pytest.raises(ValueError, match="cu_partition"):
            on._check_partition(n_micro)
    inert = WhisperDecoding(cpu_engine, only_torch=True, options=DecodingOptions(top_k=5))     # temperature 0: built, inert
    assert inert.truncation_on and inert.decoder.temperature == 0


# ---- the literal loop's sampler -----------------------------------------------------------------------------------------------------------
def test_the_literal_sampler_stays_inside_the_kept_set_and_books_the_unmasked_log_probability():
    V, B, T, eot = 400, 64, 0.8, 390
    base = torch.from_numpy(np.stack([TR.fixture_row("normal3", V, 70 + b) for b in range(B)]))
    base[:, 5::7] = -np.inf                                     # what the filters forbid stays forbidden
    tokens = torch.full((B, 4), 7)
    tokens[3, -1] = eot                                         # a finished row stays at EOT
    for kept in ((5, 1.0, 0.0), (0, 0.6, 0.0), (0, 1.0, 0.2), (30, 0.9, 0.05)):
        mask = TN.keep_mask(base.numpy(), T, *kept)
        assert (mask.sum(axis=1) < np.isfinite(base.numpy()).sum(axis=1)).all()
        dec = GreedyDecoder(T, eot, kept)
        lp_ref = torch.log_softmax(base.float(), dim=-1)
        for draw in range(20):
            torch.manual_seed(draw)
            sums = torch.zeros(B)
            out, _ = dec.update(tokens, base.clone(), sums)
            nxt = out[:, -1]
            alive = torch.arange(B) != 3
            assert mask[np.arange(B), nxt.numpy()][alive.numpy()].all() and int(nxt[3]) == eot
            assert torch.equal(sums[alive], lp_ref[torch.arange(B), nxt][alive]) and float(sums[3]) == 0.0
    # off: the code path and the tokens of today for a fixed torch seed
    torch.manual_seed(11)
    want = torch.distributions.Categorical(logits=base / T).sample()
    torch.manual_seed(11)
    out, _ = GreedyDecoder(T, eot).update(tokens, base.clone(), torch.zeros(B))
    assert torch.equal(out[:, -1][alive], want[alive])
    top1, _ = GreedyDecoder(T, eot, (1, 1.0, 0.0)).update(tokens, base.clone(), torch.zeros(B))
    assert torch.equal(top1[:, -1][alive], base.argmax(dim=-1)[alive])               # (no ties at the maximum in these rows)


# ---- command lines, header, binding ----------------------------------------------------------------------------------------------
def test_the_three_parsers_accept_the_flags():
    flags = ["--top_k", "50", "--top_p", "0.95", "--min_p", "0.05"]
    want = dict(top_k=50, top_p=0.95, min_p=0.05)
    for mod, extra in ((run, []), (summarize, []), (transcribe, ["--input_file", "a.wav"])):
        args = mod.parse_arguments(extra + flags)
        assert TN.options_from_args(args.top_k, args.top_p, args.min_p) == want
        d = mod.parse_arguments(extra)
        assert (d.top_k, d.top_p, d.min_p) == (0, 1.0, 0.0)
    for mod in (run, summarize):
        o = mod.decoding_options(mod.parse_arguments(flags))
        assert {k: getattr(o, k) for k in want} == want
        assert mod.decoding_options(mod.parse_arguments([])) == DecodingOptions()


def test_header_entry_abi_and_struct_layout(tmp_path):
    header = open(os.path.join(ROOT, "include", "whisper_mi355.h")).read()
    assert "int wm_sample_step(" in header and "wm_sample_step" in native.EXPORTS
    assert re.search(r"#define WM_ABI_VERSION 8\b", header) and native.ABI_VERSION == 8
    assert "truncate.hip" in open(os.path.join(ROOT, "eddie-wang-hackathon2023_amd", "csrc", "Makefile")).read()
    names = [n for n, _ in native.WmSampleIO._fields_]
    assert names == ["g", "top_k", "exp2_scale", "top_p_q16", "min_p_gap", "cut_out", "kept_out"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "whisper_mi355.h"', 'int main(void){',
           'printf("size %zu\\n", sizeof(wm_sample_io));', 'printf("greedy %zu\\n", sizeof(wm_greedy_io));']
    src += [f'printf("{f} %zu\\n", offsetof(wm_sample_io, {f}));' for f in names]
    src.append('return 0;}')
    (tmp_path / "l.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "l.c"), "-o",
                           str(tmp_path / "l")])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / "l")]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(native.WmSampleIO) and int(got["greedy"]) == C.sizeof(native.WmGreedyIO)
    for f in names:
        assert int(got[f]) == getattr(native.WmSampleIO, f).offset, f
    lib = native.load_library()
    assert hasattr(lib, "wm_sample_step") and lib.wm_version() == 8
    # the kernel restates the coefficients of the contract
    kernel = open(os.path.join(ROOT, "eddie-wang-hackathon2023_amd", "csrc", "truncate.hip")).read()
    literals = {float.fromhex(h) for h in re.findall(r"(0x1\.[0-9a-f]+p-?\d+)f", kernel)}
    assert {float(k) for k in TN.EXP2_COEF} <= literals and TR.COEF == list(TN.EXP2_COEF)
