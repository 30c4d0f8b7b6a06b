"""Parallel sections on the host: the contract of sections.py, which the device (csrc/sections.hip,
tests/test_gpu_sections.py) is held to bit for bit.

* the cuts: properties over random fp16 mels against an independently written smoothing and a brute-force arg-min with the
  last-of-equals rule; the boundaries F == hi / hi + 1, lo == hi, h == 0, h > F; a constant mel; quiet gaps planted so that every
  search range holds a whole one; non-finite elements and values beyond +-16;
* section_mel_ref, merge_sections;
* scheduling: longform.transcribe_batched over the sections of several files with a stub decoder that keeps languages the way
  transcribe.py does (sections.SectionLanguages);
* the header, the library's exports and the ABI version; SectionOptions' validation.
"""
import os

import numpy as np
import pytest

import longform as LF
import native
import sections as S
from longform import WindowResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rng_of(seed):
    return np.random.Generator(np.random.Philox(seed))


def random_mel(rng, n_mels, ld):
    return (rng.standard_normal((n_mels, ld)) * 2.0).astype(np.float16)


# ------------------------------------------------------------------------------------------------------------------ the cuts
def brute_force(mel, F, lo, hi, h):
    """The contract once more, frame by frame in Python integers (no numpy sums, no clip)."""
    q = []
    for t in range(F):
        acc = 0
        for m in range(mel.shape[0]):
            v = float(mel[m, t])
            if v != v or v in (float("inf"), float("-inf")):
                continue
            v = max(-16.0, min(16.0, v)) * 1024.0            # exact: an fp16 value times a power of two
            r = round(v)                                       # Python rounds halves to even
            acc += r
        q.append(acc)
    s = [sum(q[min(max(t + d, 0), F - 1)] for d in range(-h, h + 1)) for t in range(F)]
    cuts, c = [], 0
    while F - c > hi:
        best = None
        for t in range(c + lo, c + hi + 1):
            if best is None or s[t] <= s[best]:
                best = t
        c = best
        cuts.append(c)
    return cuts, q, s


def check_properties(F, lo, hi, cuts):
    assert all(b > a for a, b in zip(cuts, cuts[1:])), "cuts ascend strictly"
    bounds = S.section_bounds(F, cuts)
    if F == 0:
        assert bounds == [] and cuts == []
        return
    assert bounds[0][0] == 0 and bounds[-1][1] == F and all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))
    lengths = [b - a for a, b in bounds]
    assert all(lo <= n <= hi for n in lengths[:-1]) and 1 <= lengths[-1] <= hi
    assert (len(cuts) == 0) == (F <= hi)


@pytest.mark.parametrize("n_mels", [1, 3, 80, 128])
@pytest.mark.parametrize("lo,hi,h", [(40, 96, 3), (1, 1, 0), (7, 7, 2), (5, 23, 0), (64, 128, 10)])
def test_cuts_equal_the_brute_force(n_mels, lo, hi, h):
    rng = rng_of(1000 * n_mels + 10 * hi + h)
    for F in (0, 1, hi - 1, hi, hi + 1, 2 * hi + 1, 333, 1500 if n_mels <= 3 else 700):
        ld = F + int(rng.integers(0, 5))
        mel = random_mel(rng, n_mels, max(ld, 1))
        got = S.section_cuts_ref(mel, F, lo, hi, h)
        want, q, s = brute_force(mel, F, lo, hi, h)
        assert got == want, (F, lo, hi, h)
        assert S.loudness(mel, F).tolist() == q and S.smooth(S.loudness(mel, F), h).tolist() == s
        check_properties(F, lo, hi, got)


def test_boundaries():
    rng = rng_of(7)
    mel = random_mel(rng, 3, 400)
    assert S.section_cuts_ref(mel, 96, 40, 96, 3) == []                         # F == hi: one section
    one = S.section_cuts_ref(mel, 97, 40, 96, 3)                                # F == hi + 1: one cut
    assert len(one) == 1 and 40 <= one[0] <= 96
    assert S.section_cuts_ref(mel, 400, 50, 50, 2) == list(range(50, 400, 50))[:7]      # lo == hi: no choice
    assert S.section_cuts_ref(mel, 400, 50, 50, 2)[-1] == 350
    assert S.section_cuts_ref(mel, 0, 40, 96, 3) == [] and S.section_bounds(0, []) == []
    # h == 0: s is q itself
    q = S.loudness(mel, 400)
    assert S.smooth(q, 0).tolist() == q.tolist()
    # h > F: every tap that leaves the file repeats an end
    short = random_mel(rng, 3, 9)
    q9 = S.loudness(short, 9)
    s9 = S.smooth(q9, 20)
    assert s9.tolist() == [int(q9.sum() + (20 - t) * q9[0] + (20 - (8 - t)) * q9[8]) for t in range(9)]
    assert S.section_cuts_ref(short, 9, 2, 4, 20) == brute_force(short, 9, 2, 4, 20)[0]


def test_constant_mel_takes_the_last_of_equal_minima():
    mel = np.full((80, 300), -1.5, dtype=np.float16)
    assert S.section_cuts_ref(mel, 300, 40, 96, 3) == [96, 192, 288]
    assert S.section_bounds(300, [96, 192, 288]) == [(0, 96), (96, 192), (192, 288), (288, 300)]


@pytest.mark.parametrize("seed", range(20))
def test_cuts_fall_into_planted_gaps(seed):
    """Gaps of 2h + 5 floor-valued frames, planted so that every search range [c + lo, c + hi] holds a whole one wherever the
    last cut fell: every cut lies in a gap's core (the frames whose whole smoothing span is floor), every length is in bounds."""
    rng = rng_of(seed)
    n_mels, F, lo, hi, h = 80, 5000, 40, 96, 3
    gap = 2 * h + 5
    mel = (rng.random((n_mels, F)) * 2.0 + 0.5).astype(np.float16)               # loud: 0.5 .. 2.5
    starts, p = [], int(rng.integers(10, 30))
    while p + gap < F:
        starts.append(p)
        mel[:, p:p + gap] = np.float16(-4.0)                                     # the floor
        p += gap + int(rng.integers(1, hi - lo - 2 * gap))                       # next gap starts at most hi - lo - gap - 1 later
    core = set(t for a in starts for t in range(a + h, a + gap - h))
    cuts = S.section_cuts_ref(mel, F, lo, hi, h)
    assert cuts and all(c in core for c in cuts), [c for c in cuts if c not in core]
    check_properties(F, lo, hi, cuts)


def test_non_finite_and_large_values():
    mel = np.zeros((4, 50), dtype=np.float16)
    mel[0, 10], mel[1, 10], mel[2, 10], mel[3, 10] = np.inf, -np.inf, np.nan, 65504.0
    mel[0, 11], mel[1, 11] = -65504.0, 100.0
    mel[0, 12], mel[1, 12] = 16.0, 17.0
    mel[0, 13] = np.float16(2.0 ** -11)              # * 1024 = 0.5: half to even -> 0
    mel[0, 14] = np.float16(3 * 2.0 ** -11)          # 1.5 -> 2
    mel[0, 15] = np.float16(-5 * 2.0 ** -11)         # -2.5 -> -2
    mel[0, 16] = np.float16(6e-8)                    # a subnormal: 6.1e-5 -> 0
    q = S.loudness(mel, 50)
    assert q[10] == 16384 and q[11] == 0 and q[12] == 32768 and q[13] == 0 and q[14] == 2 and q[15] == -2 and q[16] == 0
    assert brute_force(mel, 50, 5, 20, 2)[1] == q.tolist()
    assert S.section_cuts_ref(mel, 50, 5, 20, 2) == brute_force(mel, 50, 5, 20, 2)[0]
    with pytest.raises(ValueError):
        S.loudness(mel.astype(np.float32), 50)
    with pytest.raises(ValueError):
        S.loudness(mel, 51)


# ----------------------------------------------------------------------------------------------------------- section_mel_ref
def test_section_mel_ref():
    rng = rng_of(3)
    W, F = 16, 70
    mel = random_mel(rng, 5, F + W)
    mel[:, F:] = mel[:, -1:]                                                    # what a whole-file mel ends in: W equal frames
    piece = S.section_mel_ref(mel, F, 20, 45, W)
    assert piece.shape == (5, 25 + W) and piece.dtype == np.float16
    assert np.array_equal(piece[:, :25], mel[:, 20:45]) and all(np.array_equal(piece[:, 25 + j], mel[:, -1]) for j in range(W))
    assert np.array_equal(S.section_mel_ref(mel, F, 45, F, W), mel[:, 45:])     # the last section: the file's own tail
    with pytest.raises(ValueError):
        S.section_mel_ref(mel, F, 45, 45, W)
    with pytest.raises(ValueError):
        S.section_mel_ref(mel, F, 45, F + 1, W)


# ------------------------------------------------------------------------------------------------------------ merge_sections
def test_merge_sections():
    fs = 0.02
    a = [dict(seek=0, start=0.0, end=1.0, text="a", tokens=[1, 2], words=[dict(word="a", start=0.1, end=0.9, probability=0.5)]),
         dict(seek=50, start=1.0, end=2.5, text="b", tokens=[3], words=[])]
    c = [dict(seek=7, start=0.5, end=0.75, text="c", tokens=[4, 5])]
    keep = [[dict(s) for s in a], [], [dict(s) for s in c]]
    merged = S.merge_sections([a, [], c], [0, 100, 250], fs)
    assert [s["text"] for s in merged] == ["a", "b", "c"]                       # order; the empty section leaves nothing
    assert merged[:2] == a and merged[0] is not a[0]                            # section 0 moves by nothing
    assert merged[2] == dict(seek=257, start=0.5 + 250 * fs, end=0.75 + 250 * fs, text="c", tokens=[4, 5])
    shifted = S.merge_sections([a], [100], fs)
    assert [s["seek"] for s in shifted] == [100, 150] and shifted[1]["start"] == 1.0 + 100 * fs and shifted[1]["end"] == 2.5 + 100 * fs
    assert shifted[0]["words"] == [dict(word="a", start=0.1 + 100 * fs, end=0.9 + 100 * fs, probability=0.5)]
    assert [a, [], c] == keep and a[0]["words"][0]["start"] == 0.1              # the inputs are untouched
    assert [t for s in merged for t in s["tokens"]] == [1, 2, 3, 4, 5]
    assert S.merge_sections([], [], fs) == []
    with pytest.raises(ValueError):
        S.merge_sections([a], [0, 1], fs)


# --------------------------------------------------------------------------------------------------- scheduling and language
W, TB = 100, 1000


@pytest.mark.parametrize("n_rows", [1, 2, 3, 8])
@pytest.mark.parametrize("named", [None, "de"])
def test_schedule_over_sections_and_one_language_per_file(n_rows, named):
    """Files of 0, 450, 90 and 260 frames cut at 60 .. 120 frames: the sections are the scheduler's files.  The stub decoder
    "detects" a language that depends on the SECTION, so a section that detected for itself would show."""
    rng = rng_of(11)
    contents = [0, 450, 90, 260]
    cuts = [S.section_cuts_ref(random_mel(rng, 3, max(F, 1)), F, 60, 120, 2) for F in contents]
    frames, owner, starts = [], [], []
    for f, F in enumerate(contents):
        for a, b in S.section_bounds(F, cuts[f]):
            frames.append(b - a), owner.append(f), starts.append(a)
    assert owner.count(1) >= 4 and owner.count(3) >= 3 and owner.count(2) == 1 and 0 not in owner
    languages = S.SectionLanguages(len(frames), owner, named)
    asked, used_language, detections, rounds = [], {}, [], []

    def decode_call(rows, temperature, live):
        assert len(rows) == n_rows
        if not rounds or rounds[-1] != rows:
            rounds.append(list(rows))
            for i in languages.fresh(rows):
                assert rows[i][1] == 0
                languages.detected(rows[i][0], f"lang{rows[i][0]}")
                detections.append(rows[i][0])
        out = []
        for r, on in zip(rows, live):
            if r is None or not on:
                out.append(None)
                continue
            asked.append((r[0], r[1], temperature))
            used_language.setdefault(r[0], set()).add(languages.known(r[0]))
            # a window of 100 frames advances by 60 (timestamp pair at 30 * 2 frames); low log-probability at temperature 0
            out.append(WindowResult(tokens=[TB, 5, TB + 30, TB + 30], avg_logprob=-2.0 if temperature == 0.0 else -0.5, temperature=temperature))
        return out

    segments = LF.transcribe_batched(decode_call, frames, n_rows, window=W, timestamp_begin=TB, temperatures=(0.0, 0.4),
                                     compression_ratio_threshold=None, no_speech_threshold=None)
    assert len(asked) == len(set(asked)), "a (section, seek, temperature) was asked twice"
    first = [i for i in range(len(owner)) if i == 0 or owner[i] != owner[i - 1]]
    if named is None:
        assert sorted(detections) == first                                       # only a file's first section detects
        for i, o in enumerate(owner):
            assert used_language[i] == {f"lang{first[[owner[j] for j in first].index(o)]}"}
    else:
        assert detections == [] and all(v == {"de"} for v in used_language.values())
    # every section was decoded to its end, at both temperatures, and merges back in order
    fs = LF.CHUNK_LENGTH / W
    for f, F in enumerate(contents):
        mine = [i for i, o in enumerate(owner) if o == f]
        merged = S.merge_sections([segments[i] for i in mine], [starts[i] for i in mine], fs)
        seeks = [s["seek"] for s in merged]
        assert seeks == sorted(seeks) and (not mine or (seeks[0] == 0 and seeks[-1] < F))
        for i in mine:
            want = set(range(0, frames[i], 60))
            assert {k[1] for k in asked if k[0] == i and k[2] == 0.0} == want == {k[1] for k in asked if k[0] == i and k[2] == 0.4}


def test_section_languages_refuse_a_section_before_its_first():
    languages = S.SectionLanguages(3, [0, 0, 1], None)
    assert languages.fresh([(1, 0), (2, 0), None]) == [1]                       # section 1 is not its file's first
    with pytest.raises(RuntimeError, match="first section"):
        languages.known(1)
    with pytest.raises(ValueError):
        S.SectionLanguages(3, [1, 0, 1], None)
    own = S.SectionLanguages(2, None, None)                                     # unsectioned: every file detects for itself
    assert own.fresh([(0, 0), (1, 5)]) == [0, 1]


# ------------------------------------------------------------------------------------------------------------ ABI and options
def test_header_exports_and_abi():
    header = open(os.path.join(ROOT, "include", "whisper_mi355.h")).read()
    assert "int wm_section_cuts(" in header and "size_t wm_section_cuts_workspace_bytes(" in header
    assert "#define WM_ABI_VERSION 8" in header and native.ABI_VERSION == 8
    assert "wm_section_cuts" in native.EXPORTS and "wm_section_cuts_workspace_bytes" in native.EXPORTS
    assert "sections.hip" in open(os.path.join(ROOT, "eddie-wang-hackathon2023_amd", "csrc", "Makefile")).read()


def test_the_library_exports_the_entries():
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not installed")
    lib = native.load_library()          # (built by the session start; a missing library is a failure here)
    assert lib.wm_version() == 8
    assert hasattr(lib, "wm_section_cuts") and hasattr(lib, "wm_section_cuts_workspace_bytes")
    assert lib.wm_section_cuts_workspace_bytes(1, 100) >= 16 + 2 * 400 and lib.wm_section_cuts_workspace_bytes(0, 100) == 0


def test_section_options():
    assert S.SectionOptions().frames(3000, 80) == (1500, 3000, 10)              # 15 s / 30 s / 0.2 s in frames of 10 ms
    assert S.SectionOptions().frames(3000, 128) == (1500, 3000, 10)
    assert S.SectionOptions(max_seconds=30.0).frames(128, 80) == (64, 128, 0)   # a micro engine: 128 frames are 30 s
    assert S.SectionOptions(10.0, 10.0, 0.0).frames(3000) == (1000, 1000, 0)
    assert S.SectionOptions(60.0, 1.0).frames(3000, 80)[:2] == (100, 6000)      # hi beyond the window is allowed
    for bad in (S.SectionOptions(10.0, 20.0), S.SectionOptions(10.0, 0.0), S.SectionOptions(0.0), S.SectionOptions(-1.0),
                S.SectionOptions(30.0, None, -0.1), S.SectionOptions(30.0, 15.0, 20.0)):
        with pytest.raises(ValueError):
            bad.frames(3000, 80)
    S.SectionOptions(30.0, 15.0, 16.0).frames(3000, 80)                         # 80 * 1601 = 128080 < 131072
    with pytest.raises(ValueError):
        S.SectionOptions(30.0, 15.0, 16.5).frames(3000, 80)                     # 80 * 1651
    with pytest.raises(ValueError):
        S.check_frames(0, 5, 0, 80)
    with pytest.raises(ValueError):
        S.check_frames(6, 5, 0, 80)
    with pytest.raises(ValueError):
        S.check_frames(1, 5, 0, 131072)
    assert "not measurements" in S.SectionOptions.__doc__


def test_cli_arguments():
    import transcribe as T
    args = T.parse_arguments(["--input_file", "a.flac", "--sections", "--section_seconds", "20", "--min_section_seconds", "5"])
    assert args.sections and args.section_seconds == 20.0 and args.min_section_seconds == 5.0
    args = T.parse_arguments(["--input_file", "a.flac"])
    assert not args.sections and args.section_seconds == 30.0 and args.min_section_seconds is None
