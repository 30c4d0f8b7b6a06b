"""Parallel sections on the GPU: wm_section_cuts (csrc/sections.hip) and transcribe_mel(sections=...) end to end.

* The kernel against sections.py, EXACTLY (cuts and n_cuts; everything is an integer, so there is no tolerance): outputs
  pre-filled with a sentinel, guard bands around `cuts`, every file of a case in ONE ragged launch.  n_mels 1 / 3 / 80 / 128 (the
  loudness loop's unrolled groups of 8 and its remainder); F 0, 1, hi, hi + 1, 1000, 4099 (no section, no cut, the first cut,
  more than one workgroup of frames, a file that ends inside a workgroup's run of frames); src_ld equal to F and larger, odd and
  even; the base pointer 0, 1 and 3 elements into its buffer (2-byte loads at any alignment); (lo, hi, h) from one candidate per
  cut to 701 candidates (the strided scan's three iterations over 256 threads and the minimum across four waves); h larger than
  F.  Mels: random with negative values, constant (everything ties: the last candidate wins), equal minima planted in different
  lanes, waves and scan iterations, infinities, NaNs and +-65504.
* End to end on the micro-fullvocab engine (W = 128 frames, sample_len 12), like with like only (tests/test_gpu_longform.py says
  why): the sectioned run against transcribe_mel WITHOUT sections over the materialised section mels as separate files, same
  n_rows, same temperatures, same torch seed, language named -- tokens, temperatures and avg_logprob identical, start / end / seek
  shifted as merge_sections says, the same rounds and decoder calls; with the language detected, every section decodes with the
  language of its file's first section and no other section detects; word timestamps per section; the section mels bit for bit
  sections.section_mel_ref's.

Measured on MI355X (printed by the tests): files of 1000 and 300 frames give 15 sections; language named, ladder (0, 0.4): 4 rounds
of 4 rows, 8 decoder calls (every window falls back once, as in tests/test_gpu_longform.py); with word timestamps, one temperature:
9 rounds, 9 decoder calls (the last word's end moves some sections to a second window).  The 37 tests take 4 s.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_refs as KR  # noqa: E402
import longform as LF  # noqa: E402
import native  # noqa: E402
import sections as S  # noqa: E402
import synthetic  # noqa: E402
import transcribe as T  # noqa: E402
from decoding import DecodingOptions, WhisperDecoding  # noqa: E402
from encoding import WhisperEncoding  # noqa: E402
from oracle.whisper_oracle import Dims, synthetic_mel  # noqa: E402
from test_gpu_model import build_engine  # noqa: E402

SENTINEL = -77777
GUARD = 32


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return native.load_library()


@pytest.fixture(scope="module")
def tmpdir_module(tmp_path_factory):
    return str(tmp_path_factory.mktemp("engines"))


# ----------------------------------------------------------------------------------------------------------- wm_section_cuts
def device_cuts(lib, files, n_mels, lo, hi, h, cuts_ld=None, total=None):
    """files: [(mel fp16 numpy [n_mels, ld] or None, F, elements the base pointer sits inside its buffer)].  Returns
    (n_cuts list, cuts int array [batch, cuts_ld]) after checking the guard bands and the sentinel behind every file's cuts."""
    batch = len(files)
    keep, ptrs, lds = [], [], []
    for mel, F, offset in files:
        if mel is None:
            ptrs.append(0), lds.append(0)
            continue
        buf = torch.full((offset + mel.size + 5,), KR.SENTINEL, dtype=torch.float16, device="cuda")
        buf[offset: offset + mel.size] = torch.from_numpy(np.ascontiguousarray(mel).reshape(-1)).cuda()
        keep.append(buf)
        ptrs.append(buf.data_ptr() + 2 * offset), lds.append(mel.shape[1])
    content = [F for _, F, _ in files]
    if cuts_ld is None:
        cuts_ld = max(1, max(content) // lo)
    if total is None:
        total = sum(F for mel, F, _ in files if mel is not None)
    src = torch.tensor(ptrs, dtype=torch.int64, device="cuda")
    ld = torch.tensor(lds, dtype=torch.int32, device="cuda")
    cont = torch.tensor(content, dtype=torch.int32, device="cuda")
    out = torch.full((GUARD + batch * cuts_ld + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    n_cuts = torch.full((batch + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    ws_bytes = int(lib.wm_section_cuts_workspace_bytes(batch, total))
    ws = torch.empty(ws_bytes + 64, dtype=torch.uint8, device="cuda")
    ws[ws_bytes:] = 0xA5
    native.check(lib.wm_section_cuts(src.data_ptr(), ld.data_ptr(), cont.data_ptr(), batch, n_mels, lo, hi, h,
                                     out[GUARD:].data_ptr(), cuts_ld, n_cuts.data_ptr(), ws.data_ptr(), ws_bytes, total,
                                     torch.cuda.current_stream().cuda_stream), "wm_section_cuts")
    torch.cuda.synchronize()
    got, n = out.cpu().numpy(), n_cuts.cpu().numpy()
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + batch * cuts_ld:] == SENTINEL).all(), "written outside `cuts`"
    assert (n[batch:] == SENTINEL).all(), "written outside `n_cuts`"
    assert bool((ws[ws_bytes:] == 0xA5).all()), "written outside the workspace"
    cuts = got[GUARD: GUARD + batch * cuts_ld].reshape(batch, cuts_ld)
    for b in range(batch):
        assert (cuts[b, max(0, min(int(n[b]), cuts_ld)):] == SENTINEL).all(), f"file {b}: written behind its cuts"
    return [int(v) for v in n[:batch]], cuts


def check_against_contract(lib, files, n_mels, lo, hi, h):
    n, cuts = device_cuts(lib, files, n_mels, lo, hi, h)
    for b, (mel, F, _) in enumerate(files):
        want = [] if mel is None else S.section_cuts_ref(mel, F, lo, hi, h)
        assert n[b] == len(want) and cuts[b, :n[b]].tolist() == want, (b, F, None if mel is None else mel.shape, n[b], len(want))
    return n, cuts


CONFIGS = [(40, 96, 3), (1, 1, 0), (96, 96, 0), (64, 128, 10), (300, 1000, 7)]


@pytest.mark.parametrize("lo,hi,h", CONFIGS)
@pytest.mark.parametrize("n_mels", [1, 3, 80, 128])
def test_section_cuts_equal_the_contract(lib, n_mels, lo, hi, h):
    rng = KR.philox(100 * n_mels + hi + h)
    sizes = [0, 1, hi, hi + 1, 1000, 4099]
    pads = [0, 1, 2, 7, 0, 3]                       # src_ld = F + pad: equal and larger, odd and even
    offsets = [0, 1, 3, 0, 1, 3]                    # the base pointer inside its buffer, in elements
    files = []
    for F, pad, off in zip(sizes, pads, offsets):
        ld = max(1, F + pad)
        mel = (rng.standard_normal((n_mels, ld)) * 3.0 - 1.0).astype(np.float16)
        files.append((mel, F, off))
    files.append(((rng.standard_normal((n_mels, 4099)) * 3.0).astype(np.float16), 4099, 0))      # src_ld == F, odd
    files.append(((rng.standard_normal((n_mels, 1000)) * 3.0).astype(np.float16), 1000, 1))      # src_ld == F, even, odd base
    n, _ = check_against_contract(lib, files, n_mels, lo, hi, h)
    assert n[:4] == [0, 0, 0, 1] and all((k >= 1) == (F > hi) for k, (_, F, _) in zip(n, files))


@pytest.mark.parametrize("lo,hi,h", CONFIGS)
def test_constant_mels_everything_ties(lib, lo, hi, h):
    files = [(np.full((3, 4099 + 2), v, dtype=np.float16), 4099, k) for k, v in enumerate((-1.5, 0.0, 2.25))]
    n, cuts = check_against_contract(lib, files, 3, lo, hi, h)
    assert cuts[0, :n[0]].tolist() == list(range(hi, 4099, hi))[:n[0]]           # the last candidate of every range
    if (lo, hi, h) == (40, 96, 3):
        n, cuts = check_against_contract(lib, [(np.full((80, 300), -1.5, dtype=np.float16), 300, 0)], 80, lo, hi, h)
        assert cuts[0, :n[0]].tolist() == [96, 192, 288]


def test_planted_equal_minima_across_lanes_waves_and_iterations(lib):
    """(300, 1000): 701 candidates per cut over 256 threads -- candidate i of a range sits in thread i % 256 (wave i % 256 // 64)
    and scan iteration i // 256.  Equal minima at candidates 5, 70, 200, 261, 600 and 700 of the FIRST range; with only the first
    k planted the winner is the k-th (the largest index), which walks through lanes, waves and iterations."""
    rng = KR.philox(9)
    lo, hi = 300, 1000
    spots = [5, 70, 200, 261, 600, 700]
    for n_mels, h in ((1, 0), (3, 7)):
        files = []
        for k in range(1, len(spots) + 1):
            mel = np.full((n_mels, 2400), 1.0, dtype=np.float16)
            mel[:, 1100:] = (rng.random((n_mels, 1300)) * 2.0 + 1.0).astype(np.float16)
            for i in spots[:k]:
                mel[:, lo + i - h: lo + i + h + 1] = np.float16(-2.0)             # 2h + 1 quiet frames: equal minima of s at lo + i
            files.append((mel, 2400, k % 2))
        n, cuts = check_against_contract(lib, files, n_mels, lo, hi, h)
        assert [int(cuts[k, 0]) for k in range(len(spots))] == [lo + i for i in spots], (n_mels, h)


def test_non_finite_and_large_values(lib):
    rng = KR.philox(13)
    files = []
    mel = (rng.standard_normal((3, 1501)) * 2.0).astype(np.float16)
    what = np.array([np.inf, -np.inf, np.nan, 65504.0, -65504.0, 16.0, -16.0, 17.0, 2.0 ** -11, 3 * 2.0 ** -11, -5 * 2.0 ** -11, 6e-8],
                    dtype=np.float16)
    mel[rng.integers(0, 3, size=200), rng.integers(0, 1500, size=200)] = what[rng.integers(0, len(what), size=200)]
    files.append((mel, 1500, 1))
    everything = np.full((3, 700), np.nan, dtype=np.float16)                      # nothing finite at all: q is zero everywhere
    everything[1] = np.inf
    files.append((everything, 700, 0))
    n, cuts = check_against_contract(lib, files, 3, 40, 96, 3)
    assert cuts[1, :n[1]].tolist() == list(range(96, 700, 96))[:n[1]]


def test_smoothing_wider_than_the_file(lib):
    rng = KR.philox(17)
    files = [((rng.standard_normal((3, 9)) * 2.0).astype(np.float16), 9, 1), ((rng.standard_normal((3, 40)) * 2.0).astype(np.float16), 37, 0)]
    check_against_contract(lib, files, 3, 2, 4, 50)
    check_against_contract(lib, files, 3, 1, 1, 1000)


def test_ragged_batch_with_a_null_file_and_an_empty_one(lib):
    rng = KR.philox(21)
    mk = lambda ld: (rng.standard_normal((80, ld)) * 2.0).astype(np.float16)      # noqa: E731
    files = [(mk(777), 777, 0), (None, 500, 0), (mk(64), 0, 1), (mk(1203), 1200, 3), (mk(97), 97, 0)]
    n, _ = check_against_contract(lib, files, 80, 40, 96, 3)
    assert n[1] == 0 and n[2] == 0 and n[4] == 1 and n[0] >= 8 and n[3] >= 12


def test_cuts_ld_too_small_and_total_frames_too_small(lib):
    rng = KR.philox(23)
    mel = (rng.standard_normal((3, 1000)) * 2.0).astype(np.float16)
    want = S.section_cuts_ref(mel, 1000, 40, 96, 3)
    assert len(want) > 3
    n, cuts = device_cuts(lib, [(mel, 1000, 0), (mel[:, :200].copy(), 200, 0)], 3, 40, 96, 3, cuts_ld=3)
    assert n[0] == len(want) and cuts[0].tolist() == want[:3]                    # the true count; nothing behind cuts_ld (guards)
    assert n[1] == len(S.section_cuts_ref(mel[:, :200].copy(), 200, 40, 96, 3)) <= 3
    # a file whose frames end beyond total_frames is left alone and says so, and so does every later file that has frames (the
    # offsets are cumulative); files without frames, empty or null, report 0 wherever they stand
    files = [(mel[:, :300].copy(), 300, 0), (mel, 1000, 0), (mel[:, :64].copy(), 0, 0), (None, 500, 0), (mel[:, :200].copy(), 200, 1)]
    n, cuts = device_cuts(lib, files, 3, 40, 96, 3, total=700)
    assert n[0] == len(S.section_cuts_ref(mel[:, :300].copy(), 300, 40, 96, 3)) and n[1:] == [-1, 0, 0, -1]


def test_bad_arguments(lib):
    s = torch.cuda.current_stream().cuda_stream
    z = torch.zeros(64, dtype=torch.int64, device="cuda")                       # a null file of no frames
    o = torch.zeros(64, dtype=torch.int32, device="cuda")
    ws_bytes = int(lib.wm_section_cuts_workspace_bytes(1, 100))
    assert ws_bytes >= 16 + 2 * 400
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    p, q = z.data_ptr(), o.data_ptr()

    def call(src=p, ld=p, content=p, batch=1, n_mels=80, lo=40, hi=96, h=3, cuts=q + 64, cuts_ld=4, n_cuts=q, w=ws.data_ptr(), wb=ws_bytes,
             total=100):
        return lib.wm_section_cuts(src, ld, content, batch, n_mels, lo, hi, h, cuts, cuts_ld, n_cuts, w, wb, total, s)

    assert call() == 0                                                           # (a null file: nothing to do)
    for bad in (dict(src=None), dict(ld=None), dict(content=None), dict(cuts=None), dict(n_cuts=None), dict(w=None), dict(batch=0),
                dict(n_mels=0), dict(lo=0), dict(lo=97), dict(h=-1), dict(h=819), dict(n_mels=1, h=65536), dict(wb=ws_bytes - 1),
                dict(total=200), dict(total=-1), dict(cuts_ld=-1)):
        assert call(**bad) == 1, bad
        assert "wm_section_cuts" in lib.wm_last_error().decode(), bad
    assert call(h=818) == 0                                                      # 80 * 1637 = 130960 < 131072
    torch.cuda.synchronize()


def test_wrapper_one_launch_for_all_files(lib):
    rng = KR.philox(29)
    host = [(rng.standard_normal((80, F + 128)) * 2.0).astype(np.float16) for F in (1000, 0, 300, 5000)]
    mels = [torch.from_numpy(m).cuda() for m in host]
    content = [1000, 0, 300, 5000]
    opts = S.SectionOptions(max_seconds=30.0)                                    # at W = 128: lo 64, hi 128, h 0
    assert opts.frames(128, 80) == (64, 128, 0)
    got = T.section_cuts(mels, content, opts, window=128)
    assert got == [S.section_cuts_ref(m, F, 64, 128, 0) for m, F in zip(host, content)]
    smooth = S.SectionOptions(max_seconds=30.0, min_seconds=10.0, smooth_seconds=1.5)
    lo, hi, h = smooth.frames(128, 80)
    assert h == 3 and T.section_cuts(mels, content, smooth, window=128) == [S.section_cuts_ref(m, F, lo, hi, h) for m, F in zip(host, content)]
    assert T.section_cuts([], [], opts) == []


# --------------------------------------------------------------------------------------------------------------- end to end
CONTENTS = [1000, 300]
OPTS = S.SectionOptions(max_seconds=30.0)
N_ROWS = 4


@pytest.fixture(scope="module")
def engines(tmpdir_module):
    dims = Dims(**synthetic.DIMS["micro-fullvocab"])
    eng = build_engine(tmpdir_module, "micro-fullvocab", 3)
    W = 2 * dims.n_audio_ctx
    mels = [synthetic_mel(1, c + W, dims.n_mels, 700 + i)[0].cuda().half().contiguous() for i, c in enumerate(CONTENTS)]
    return dims, eng, WhisperEncoding(eng), mels


def pieces_of(dims, mels):
    W = 2 * dims.n_audio_ctx
    assert OPTS.frames(W, dims.n_mels)[:2] == (64, 128)
    cuts = T.section_cuts(mels, CONTENTS, OPTS, window=W)
    return cuts, T.section_mels(mels, CONTENTS, cuts, W)


def run_both(enc, dec, dims, mels, **kw):
    """The sectioned run and the reference: the section mels as separate files through the unsectioned path."""
    _, (pieces, frames, owner, starts) = pieces_of(dims, mels)
    trace, ref_trace = [], []
    torch.manual_seed(5)
    results = T.transcribe_mel(enc, dec, mels, CONTENTS, n_rows=N_ROWS, trace=trace, sections=OPTS, **kw)
    torch.manual_seed(5)
    reference = T.transcribe_mel(enc, dec, pieces, frames, n_rows=N_ROWS, trace=ref_trace, **kw)
    return results, trace, reference, ref_trace, (pieces, frames, owner, starts)


def compare_with_reference(dims, results, trace, reference, ref_trace, layout):
    pieces, frames, owner, starts = layout
    fs = LF.CHUNK_LENGTH / (2 * dims.n_audio_ctx)
    assert len(results) == len(CONTENTS) and len(reference) == len(pieces)
    for f, res in enumerate(results):
        mine = [i for i, o in enumerate(owner) if o == f]
        assert res["sections"] == [(starts[i] * fs, (starts[i] + frames[i]) * fs) for i in mine]
        want = [s for i in mine for s in reference[i]["segments"]]
        shifts = [starts[i] for i in mine for _ in reference[i]["segments"]]
        assert len(res["segments"]) == len(want) > 0
        for got, ref, a in zip(res["segments"], want, shifts):
            assert got["tokens"] == ref["tokens"] and got["temperature"] == ref["temperature"] and got["avg_logprob"] == ref["avg_logprob"]
            assert got["text"] == ref["text"] and got["compression_ratio"] == ref["compression_ratio"]
            assert got["seek"] == ref["seek"] + a and got["start"] == ref["start"] + a * fs and got["end"] == ref["end"] + a * fs
            assert ("words" in got) == ("words" in ref)
            for gw, rw in zip(got.get("words", ()), ref.get("words", ())):
                assert gw == dict(word=rw["word"], start=rw["start"] + a * fs, end=rw["end"] + a * fs, probability=rw["probability"])
        assert res["segments"] == S.merge_sections([reference[i]["segments"] for i in mine], [starts[i] for i in mine], fs)
        assert res["language"] == reference[mine[0]]["language"]
    # the same rounds and the same decoder (and alignment) calls
    assert len(trace) == len(ref_trace)
    for e, r in zip(trace, ref_trace):
        assert e.get("kind") == r.get("kind") and e["round"] == r["round"] and e["rows"] == r["rows"]
        if e.get("kind") == "align":
            assert e["jobs"] == r["jobs"]
            continue
        assert e["new_round"] == r["new_round"] and e["temperature"] == r["temperature"] and e["live"] == r["live"]
        assert torch.equal(e["windows"], r["windows"]) and e["language_tokens"] == r["language_tokens"]
        assert [None if x is None else x.tokens for x in e["results"]] == [None if x is None else x.tokens for x in r["results"]]
    decodes = [e for e in trace if e.get("kind") != "align"]
    print(f"sections end to end: {len(pieces)} sections of {CONTENTS} frames in {decodes[-1]['round'] + 1} rounds, {len(decodes)} decoder calls")
    return decodes


def test_sectioned_run_equals_its_sections_as_files(lib, engines):
    dims, eng, enc, mels = engines
    dec = WhisperDecoding(eng, options=DecodingOptions(language="en"))
    dec.sample_len = 12
    kw = dict(temperatures=(0.0, 0.4), compression_ratio_threshold=None, logprob_threshold=-1.0, no_speech_threshold=None)
    results, trace, reference, ref_trace, layout = run_both(enc, dec, dims, mels, **kw)
    decodes = compare_with_reference(dims, results, trace, reference, ref_trace, layout)
    pieces, frames, owner, starts = layout
    assert len(pieces) >= 8 + 3 and all(64 <= n <= 128 for i, n in enumerate(frames) if i + 1 < len(frames) and owner[i + 1] == owner[i])
    # every section is one window here (hi == W): ceil(sections / n_rows) rounds, and each (section, seek, temperature) once
    assert decodes[-1]["round"] + 1 == -(-len(pieces) // N_ROWS)
    asked = [(r[0], r[1], e["temperature"]) for e in decodes for r, on in zip(e["rows"], e["live"]) if on]
    assert len(asked) == len(set(asked)) and {a[0] for a in asked} == set(range(len(pieces))) and all(a[1] == 0 for a in asked)
    assert all(r["language"] == "en" for r in results) and not any(e["detected"] for e in decodes)
    # and the unsectioned path is what it was: no "sections" key
    assert all("sections" not in r for r in reference)


def test_section_mels_are_the_reference_bit_for_bit(lib, engines):
    dims, eng, enc, mels = engines
    W = 2 * dims.n_audio_ctx
    cuts, (pieces, frames, owner, starts) = pieces_of(dims, mels)
    host = [m.cpu().numpy() for m in mels]
    assert cuts == [S.section_cuts_ref(m, F, 64, 128, 0) for m, F in zip(host, CONTENTS)]
    assert [(o, a, a + n) for o, a, n in zip(owner, starts, frames)] == \
        [(f, a, b) for f, F in enumerate(CONTENTS) for a, b in S.section_bounds(F, cuts[f])]
    for p, o, a, n in zip(pieces, owner, starts, frames):
        want = S.section_mel_ref(host[o], CONTENTS[o], a, a + n, W)
        assert p.is_contiguous() and np.array_equal(p.cpu().numpy().view(np.int16), want.view(np.int16))
    # what the run fed the encoder in round 0: the first W frames of the first n_rows sections
    dec = WhisperDecoding(eng, options=DecodingOptions(language="en"))
    dec.sample_len = 12
    trace = []
    T.transcribe_mel(enc, dec, mels, CONTENTS, n_rows=N_ROWS, trace=trace, sections=OPTS, temperatures=(0.0,),
                     compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None)
    first = trace[0]
    assert first["round"] == 0 and first["rows"] == [(i, 0) for i in range(N_ROWS)]
    for i in range(N_ROWS):
        want = S.section_mel_ref(host[owner[i]], CONTENTS[owner[i]], starts[i], starts[i] + frames[i], W)[:, :W]
        assert np.array_equal(first["windows"][i].numpy().view(np.int16), want.view(np.int16))


def test_one_detected_language_per_file(lib, engines):
    dims, eng, enc, mels = engines
    dec = WhisperDecoding(eng)
    dec.sample_len = 12
    trace = []
    results = T.transcribe_mel(enc, dec, mels, CONTENTS, n_rows=N_ROWS, trace=trace, sections=OPTS, temperatures=(0.0,),
                               compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None)
    _, (pieces, frames, owner, starts) = pieces_of(dims, mels)
    first = {o: owner.index(o) for o in set(owner)}
    detected = {}
    for e in trace:
        for section, (row, lang) in e["detected"].items():
            assert section in first.values() and e["rows"][row] == (section, 0) and section not in detected
            detected[section] = lang
    assert set(detected) == set(first.values())                                 # only a file's first section, each once
    tk = dec.tokenizer
    for e in trace:
        for r, lang, token in zip(e["rows"], e["languages"], e["language_tokens"]):
            if r is not None:
                want = detected[first[owner[r[0]]]]
                assert lang == want and token == tk.special_tokens[f"<|{want}|>"]
        for r, res in zip(e["rows"], e["results"]):
            if r is not None and res is not None:
                assert res.language == detected[first[owner[r[0]]]]
    assert [r["language"] for r in results] == [detected[first[f]] for f in range(len(CONTENTS))]


def test_word_timestamps_per_section(lib, engines):
    dims, eng, enc, mels = engines
    dec = WhisperDecoding(eng, options=DecodingOptions(language="en"))
    dec.sample_len = 12
    kw = dict(temperatures=(0.0,), compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None, word_timestamps=True)
    results, trace, reference, ref_trace, layout = run_both(enc, dec, dims, mels, **kw)
    compare_with_reference(dims, results, trace, reference, ref_trace, layout)
    W = 2 * dims.n_audio_ctx
    fs = LF.CHUNK_LENGTH / W
    n_words = 0
    for res in results:
        for s in res["segments"]:
            inside = [(a, b) for a, b in res["sections"] if round(a / fs) <= s["seek"] < round(b / fs)]
            assert len(inside) == 1
            a, b = inside[0]
            for w in s["words"]:
                n_words += 1
                assert a - 1e-9 <= w["start"] <= w["end"] <= b + W * fs + 1e-9, (w, a, b)
    assert n_words > 0 and any(e.get("kind") == "align" for e in trace)


def test_refusals_stay(lib, engines):
    dims, eng, enc, mels = engines
    with pytest.raises(ValueError, match="prompt"):
        T.transcribe_mel(enc, WhisperDecoding(eng, options=DecodingOptions(prompt=[100, 200])), mels, CONTENTS, sections=OPTS)
    with pytest.raises(ValueError, match="condition_on_previous_text"):
        T.transcribe_mel(enc, WhisperDecoding(eng), mels, CONTENTS, sections=OPTS, condition_on_previous_text=True)
    with pytest.raises(ValueError, match="lo <= hi"):
        T.transcribe_mel(enc, WhisperDecoding(eng), mels, CONTENTS, sections=S.SectionOptions(10.0, 20.0))
