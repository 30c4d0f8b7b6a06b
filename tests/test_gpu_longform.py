"""Long-form transcription on the GPU: wm_mel_windows (csrc/windows.hip), the whole-file log-mel, and transcribe_mel end to end.

* wm_mel_windows is a copy: compared BIT FOR BIT with numpy slicing, sources of random bit patterns (NaNs included), the output
  pre-filled with a sentinel and guard bands on both sides of it.  Every alignment class of the kernel is hit: output rows whose
  start is and is not 16-byte aligned (n_window 7; an output pointer 3 elements into its buffer), sources 16-, 4- and 2-byte
  aligned (even / odd seek, even / odd src_frames), windows crossing the end of the file, behind it, and a null source.
* long_log_mel_device against log_mel_spectrogram(audio, padding=N_SAMPLES) on the CPU: the project's own front-end bound, 5e-4
  (tests/test_gpu_kernels.py::test_log_mel_device, fp32 direct DFT against pocketfft after log10 and / 4), in fp32; the fp16
  output must be that fp32 result after the same cast.
* End to end on the micro-fullvocab engine (W = 128 frames, sample_len 12).  Near-ties in random-weight logits make tokens depend
  on the batch composition, so nothing is compared across batch shapes: the trace of decoder calls is replayed through
  longform.transcribe_reference, every temperature-0 call is run again through get_audio_features -> main_loop(row_limit) ->
  post_process with the same windows in the same order, and the buffer set / graphs / encoder runs are counted.

Measured on MI355X (printed by the tests): long mel, 37.3 s: max |device fp32 - CPU| = 4.77e-06 over 80 x 6730 values (bound
5e-4), content_frames 3730; the fp16 output equals the fp32 one after the cast (against the CPU result after the cast: one fp16
step, 4.88e-04, at a handful of values that sit on a rounding boundary).  End to end: run 1 (n_rows 4, language named, no
thresholds) 13 windows in 7 rounds, 7 decoder calls; run 2 (n_rows 3, fallback, language detected) 13 windows in 7 rounds, 14
decoder calls, every segment at temperature 0.4.  With random weights no window advanced by a timestamp pair: 12 / 13 of the 13
went through the guard (pairs whose index lies beyond the window), the rest ended without a pair -- the seek rule itself is
covered on the CPU (tests/test_longform_cpu.py).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_refs as KR  # noqa: E402
import longform as LF  # noqa: E402
import native  # noqa: E402
import synthetic  # noqa: E402
import transcribe as T  # noqa: E402
import whisper_utils as wu  # noqa: E402
from decoding import DecodingOptions, WhisperDecoding  # noqa: E402
from encoding import WhisperEncoding  # noqa: E402
from oracle.whisper_oracle import Dims, synthetic_mel  # noqa: E402
from test_gpu_model import build_engine  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return native.load_library()


@pytest.fixture(scope="module")
def tmpdir_module(tmp_path_factory):
    return str(tmp_path_factory.mktemp("engines"))


def bits(t):
    return t.contiguous().view(torch.int16)


# ----------------------------------------------------------------------------------------------------------- wm_mel_windows
def window_ref(src, seek, n_mels, n_window):
    """numpy: src int16 [n_mels, F] or None -> [n_mels, n_window]"""
    out = np.zeros((n_mels, n_window), dtype=np.int16)
    if src is not None and seek < src.shape[1]:
        piece = src[:, seek:seek + n_window]
        out[:, :piece.shape[1]] = piece
    return out


def row_cases(Wn):
    """(src_frames or None, seek): odd and even lengths, shorter than the window, seek 0 / odd / even / a multiple of 8, crossing
    the end, at the end, behind it; a null source."""
    short = max(1, Wn - 3)
    return [(Wn + 37, 0), (Wn + 37, 13), (2 * Wn + 4, 2 * Wn + 4 - Wn // 2 - 1), (short, 0), (short, 1),
            (Wn + 10, Wn + 10), (Wn + 10, Wn + 999), (None, 5), (2 * Wn + 5, 3), (2 * Wn + 6, 2), (2 * Wn + 16, 8), (2 * Wn + 5, Wn + 4)]


@pytest.mark.parametrize("out_offset", [0, 3])
@pytest.mark.parametrize("n_window", [7, 128, 3000])
@pytest.mark.parametrize("n_mels", [1, 80])
@pytest.mark.parametrize("batch", [1, 5])
def test_mel_windows_bit_exact(lib, batch, n_mels, n_window, out_offset):
    rng = KR.philox(1000 * batch + 10 * n_mels + n_window + out_offset)
    cases = row_cases(n_window)
    while len(cases) % batch:
        cases.append(cases[len(cases) % 7])
    host = {F: rng.integers(-32768, 32768, size=(n_mels, F), dtype=np.int16) for F, _ in cases if F is not None}
    dev_src = {F: torch.from_numpy(a).cuda().view(torch.float16) for F, a in host.items()}
    guard = 64
    n_out = batch * n_mels * n_window
    sentinel = bits(torch.tensor([KR.SENTINEL], dtype=torch.float16))[0].item()
    for k in range(0, len(cases), batch):
        group = cases[k:k + batch]
        buf = torch.full((guard + out_offset + n_out + guard,), KR.SENTINEL, dtype=torch.float16, device="cuda")
        out = buf[guard + out_offset: guard + out_offset + n_out]
        ptrs = torch.tensor([0 if F is None else dev_src[F].data_ptr() for F, _ in group], dtype=torch.int64, device="cuda")
        frames = torch.tensor([0 if F is None else F for F, _ in group], dtype=torch.int32, device="cuda")
        seeks = torch.tensor([s for _, s in group], dtype=torch.int32, device="cuda")
        native.check(lib.wm_mel_windows(ptrs.data_ptr(), frames.data_ptr(), seeks.data_ptr(), batch, n_mels, n_window,
                                        out.data_ptr(), torch.cuda.current_stream().cuda_stream), "wm_mel_windows")
        torch.cuda.synchronize()
        got = bits(buf).cpu().numpy()
        assert (got[:guard + out_offset] == sentinel).all() and (got[guard + out_offset + n_out:] == sentinel).all(), \
            f"written outside the output ({group})"
        want = np.stack([window_ref(None if F is None else host[F], s, n_mels, n_window) for F, s in group])
        assert np.array_equal(got[guard + out_offset: guard + out_offset + n_out].reshape(batch, n_mels, n_window), want), group


def test_mel_windows_wrapper_and_bad_arguments(lib):
    """transcribe.mel_windows (the call transcribe_mel makes) and the argument checks."""
    rng = KR.philox(5)
    a = torch.from_numpy(rng.standard_normal((80, 333)).astype(np.float16)).cuda()
    b = torch.from_numpy(rng.standard_normal((80, 128)).astype(np.float16)).cuda()
    out = T.mel_windows([a, None, b], [301, 0, 0], 80, 128)
    torch.cuda.synchronize()
    assert torch.equal(out[0, :, :32], a[:, 301:]) and not out[0, :, 32:].any() and not out[1].any() and torch.equal(out[2], b)
    s = torch.cuda.current_stream().cuda_stream
    z = torch.zeros(8, dtype=torch.int64, device="cuda")
    assert lib.wm_mel_windows(None, z.data_ptr(), z.data_ptr(), 1, 80, 128, out.data_ptr(), s) == 1
    assert lib.wm_mel_windows(z.data_ptr(), z.data_ptr(), z.data_ptr(), 0, 80, 128, out.data_ptr(), s) == 1
    assert lib.wm_mel_windows(z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 80, 0, out.data_ptr(), s) == 1
    assert lib.wm_mel_windows(z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 80, 128, None, s) == 1


# ----------------------------------------------------------------------------------------------------------------- long mel
def test_long_log_mel_device(lib, golden_dir):
    import os
    g = np.load(os.path.join(golden_dir, "mel.npz"))
    rng = np.random.Generator(np.random.Philox(int(g["audio_seed"])))          # the golden-mel test's audio, 37.3 s of it
    n = round(37.3 * wu.SAMPLE_RATE)
    audio = (rng.standard_normal(n) * 0.1).astype(np.float32)
    ref = wu.log_mel_spectrogram(audio, padding=wu.N_SAMPLES)                   # CPU, fp32 [80, 6730]
    mel16, content = wu.long_log_mel_device(torch.from_numpy(audio).cuda())
    assert content == ref.shape[1] - wu.N_FRAMES == 3730 and tuple(mel16.shape) == tuple(ref.shape) and mel16.dtype == torch.float16
    padded = torch.nn.functional.pad(torch.from_numpy(audio), (0, wu.N_SAMPLES)).cuda()
    mel32 = wu.log_mel_spectrogram_device(padded, dtype=torch.float32)         # the same call with fp32 output
    d = float((mel32.cpu() - ref).abs().max())
    d16 = float((mel16.float().cpu() - ref.half().float()).abs().max())
    print(f"long mel: max |device fp32 - CPU| = {d:.3g} over {ref.shape[0]} x {ref.shape[1]} values, content_frames {content}; "
          f"max |fp16 - fp16(CPU)| = {d16:.3g}")
    assert d < 5e-4
    assert torch.equal(mel16, mel32.half()), "the fp16 output is not the fp32 result after the cast"


# --------------------------------------------------------------------------------------------------------------- end to end
CONTENTS = [0, 100, 128, 129, 300, 700]


def make_mels(dims):
    W = 2 * dims.n_audio_ctx
    return [synthetic_mel(1, c + W, dims.n_mels, 900 + i)[0].cuda().contiguous() for i, c in enumerate(CONTENTS)]


def run_and_check(enc, dec, mels, n_rows, expect_temperature, **kw):
    W = mels[0].shape[1] - CONTENTS[0]
    tk = dec.tokenizer
    trace, states, encoder_runs = [], [], []
    real_main_loop, real_features = dec.main_loop, enc.get_audio_features

    def main_loop(*a, **k):
        out = real_main_loop(*a, **k)
        states.append(list(dec._state.values()))
        return out

    def get_audio_features(mel):
        encoder_runs.append(tuple(mel.shape))
        return real_features(mel)

    dec.main_loop, enc.get_audio_features = main_loop, get_audio_features
    try:
        results = T.transcribe_mel(enc, dec, mels, CONTENTS, n_rows=n_rows, trace=trace, **kw)
    finally:
        dec.main_loop, enc.get_audio_features = real_main_loop, real_features

    assert len(results) == len(CONTENTS) and results[0]["segments"] == [] and results[0]["text"] == ""
    n_rounds = trace[-1]["round"] + 1
    # the shape of the calls: n_rows rows each, one temperature, rounds in order
    assert all(len(e["rows"]) == n_rows == len(e["live"]) == len(e["results"]) for e in trace)
    assert [e["round"] for e in trace if e["new_round"]] == list(range(n_rounds))
    # one buffer set, the same object after the first and the last call; no graph captured after round 1; one encoder pass per round
    assert all(len(s) == 1 for s in states) and all(s[0] is states[0][0] for s in states) and len(states) == len(trace)
    assert all(e["n_states"] == 1 for e in trace)
    after_round_1 = [e for e in trace if e["round"] == 0][-1]["n_graphs"]
    assert after_round_1 == trace[-1]["n_graphs"] and after_round_1 > 0
    assert encoder_runs == [(n_rows, mels[0].shape[0], W)] * n_rounds

    # the windows fed equal the slices
    host = [m.cpu().view(torch.int16).numpy() for m in mels]
    for e in trace:
        if e["new_round"]:
            want = np.stack([window_ref(None if r is None else host[r[0]], 0 if r is None else r[1], mels[0].shape[0], W) for r in e["rows"]])
            assert np.array_equal(e["windows"].view(torch.int16).numpy(), want), e["rows"]

    # replaying the literal loop per file from the recorded results gives the same segments, and asks only for recorded keys
    recorded = {}
    for e in trace:
        for r, on, res in zip(e["rows"], e["live"], e["results"]):
            if on:
                assert (r[0], r[1], e["temperature"]) not in recorded
                recorded[(r[0], r[1], e["temperature"])] = res
    ladder = dict(temperatures=kw.get("temperatures", LF.TEMPERATURES), compression_ratio_threshold=kw.get("compression_ratio_threshold", 2.4),
                  logprob_threshold=kw.get("logprob_threshold", -1.0), no_speech_threshold=kw.get("no_speech_threshold", 0.6))
    used = set()
    for f, c in enumerate(CONTENTS):
        def decode_one(seek, temperature, f=f):
            used.add((f, seek, temperature))
            return recorded[(f, seek, temperature)]
        want = LF.transcribe_reference(decode_one, c, window=W, timestamp_begin=tk.timestamp_begin, decode_text=tk.decode, **ladder)
        assert results[f]["segments"] == want, f
        assert results[f]["text"] == tk.decode([t for s in want for t in s["tokens"]]).strip()
    assert used == set(recorded)
    for res in results:
        for s in res["segments"]:
            assert set(s) == {"seek", "start", "end", "text", "tokens", "temperature", "avg_logprob", "compression_ratio", "no_speech_prob"}
            assert s["temperature"] == expect_temperature

    # every temperature-0 call again through the public path: same windows, same order, same row limits -> the same tokens;
    # and every file's language is what detect_language says on the features of the round it started in
    detected_files = []
    for e in trace:
        if e["temperature"] != 0.0:
            continue
        xa = enc.get_audio_features(e["windows"].cuda())
        if e["detected"]:
            langs, _ = dec.detect_language(xa)
            for f, (row, lang) in e["detected"].items():
                assert e["rows"][row][0] == f and e["rows"][row][1] == 0
                assert langs[row] == lang == results[f]["language"]
                detected_files.append(f)
        if e["language_tokens"] is not None:
            dec.set_language_tokens(e["language_tokens"])
        tokens, sums, nsp = dec.main_loop(xa, row_limit=e["row_limit"])
        again = dec.post_process(tokens, sums, nsp, xa, e["languages"])
        for i, on in enumerate(e["live"]):
            if on:
                assert again[i].tokens == e["results"][i].tokens, (e["round"], i)
                assert again[i].language == e["results"][i].language
            else:
                assert again[i].tokens == []                  # row_limit 0: closed at the first step
    assert len(dec._state) == 1 and next(iter(dec._state.values())) is states[0][0]

    # how the windows moved on
    by_timestamp = whole = guarded = 0
    final = {}
    for (f, seek, temp), res in recorded.items():
        if (f, seek) not in final or temp > final[(f, seek)][0]:
            final[(f, seek)] = (temp, res)
    for (f, seek), (_, res) in final.items():
        size = min(W, CONTENTS[f] - seek)
        raw = LF.predicted_advance(res.tokens, tk.timestamp_begin, size)
        if raw <= 0 or raw > size:
            guarded += 1
        if 0 < raw < size:
            by_timestamp += 1
        else:
            whole += 1
    print(f"end to end (n_rows {n_rows}): {len(final)} windows in {n_rounds} rounds, {len(trace)} decoder calls; "
          f"{by_timestamp} advanced by timestamp, {whole} by the whole window ({guarded} of them through the guard)")
    return results, trace, detected_files


@pytest.fixture(scope="module")
def engines(tmpdir_module):
    dims = Dims(**synthetic.DIMS["micro-fullvocab"])
    eng = build_engine(tmpdir_module, "micro-fullvocab", 3)
    return dims, eng, WhisperEncoding(eng), make_mels(dims)


def test_transcribe_language_named_no_fallback(lib, engines):
    dims, eng, enc, mels = engines
    dec = WhisperDecoding(eng, options=DecodingOptions(language="en"))
    dec.sample_len = 12
    results, trace, detected = run_and_check(enc, dec, mels, 4, 0.0, compression_ratio_threshold=None, logprob_threshold=None,
                                             no_speech_threshold=None)
    assert detected == [] and all(r["language"] == "en" for r in results)
    assert all(e["temperature"] == 0.0 for e in trace)                        # thresholds None: nothing ever falls back
    # files 1 and 2 are one window each; every file with content has segments up to its end
    assert [len({s["seek"] for s in r["segments"]}) for r in results[:3]] == [0, 1, 1]
    fs = LF.CHUNK_LENGTH / (2 * dims.n_audio_ctx)
    for r, c in zip(results, CONTENTS):
        assert all(0 <= s["seek"] < c and s["start"] >= s["seek"] * fs - 1e-9 for s in r["segments"])


def test_transcribe_fallback_and_detected_language(lib, engines):
    dims, eng, enc, mels = engines
    dec = WhisperDecoding(eng)
    dec.sample_len = 12
    results, trace, detected = run_and_check(enc, dec, mels, 3, 0.4, temperatures=(0.0, 0.4), compression_ratio_threshold=None,
                                             logprob_threshold=-1.0, no_speech_threshold=None)
    assert sorted(detected) == [f for f, c in enumerate(CONTENTS) if c > 0]
    # random weights sit near -log V: every window falls back once -- per round one call at 0 and one at 0.4 over the same live rows
    assert len(trace) % 2 == 0
    for first, second in zip(trace[0::2], trace[1::2]):
        assert (first["temperature"], second["temperature"]) == (0.0, 0.4) and first["round"] == second["round"]
        assert first["rows"] == second["rows"] and first["live"] == second["live"] == [r is not None for r in first["rows"]]
        assert all(r.avg_logprob < -1.0 for r in first["results"] if r is not None)
        assert all(r.temperature == 0.4 for r in second["results"] if r is not None)


def test_transcribe_refusals(lib, engines):
    dims, eng, enc, mels = engines
    with pytest.raises(ValueError, match="prompt"):
        T.transcribe_mel(enc, WhisperDecoding(eng, options=DecodingOptions(prompt=[100, 200])), mels, CONTENTS)
    with pytest.raises(ValueError, match="beam_size"):
        T.transcribe_mel(enc, WhisperDecoding(eng, options=DecodingOptions(beam_size=2)), mels, CONTENTS)
    with pytest.raises(ValueError, match="condition_on_previous_text"):
        T.transcribe_mel(enc, WhisperDecoding(eng), mels, CONTENTS, condition_on_previous_text=True)


def test_transcribe_beam_search_at_its_own_temperature(lib, engines):
    """beam_size with the one temperature of the instance: no fallback, n_rows files x beam_size decoder rows per call."""
    dims, eng, enc, mels = engines
    dec = WhisperDecoding(eng, options=DecodingOptions(beam_size=2, language="en"))
    dec.sample_len = 12
    trace = []
    results = T.transcribe_mel(enc, dec, mels[:4], CONTENTS[:4], temperatures=(0.0,), n_rows=2, trace=trace,
                               compression_ratio_threshold=None, logprob_threshold=None, no_speech_threshold=None)
    assert len(dec._state) == 1 and next(iter(dec._state)) == 4
    assert results[0]["segments"] == [] and all(r["segments"] for r in results[1:])
    assert all(s["temperature"] == 0.0 for r in results for s in r["segments"])


def test_transcribe_cli_on_flac(lib, engines, golden_dir, capsys):
    """python transcribe.py on a real FLAC, twice in one job: load -> whole-file log-mel -> windows -> segments -> printed lines.
    (Random weights: the text is noise; the window of this engine is 128 frames, so the clip takes many rounds.)"""
    import os
    import re
    dims, eng, enc, mels = engines
    flac = os.path.join(golden_dir, "librispeech_1089-134691-0000.flac")
    n_frames = len(wu.load_audio(flac)) // wu.HOP_LENGTH
    results = T.main(T.parse_arguments(["--engine_dir", str(eng), "--input_file", flac, flac, "--no_fallback", "--language", "en"]))
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(results) == 2 and all(r["language"] == "en" and r["segments"] for r in results)
    fs = LF.CHUNK_LENGTH / (2 * dims.n_audio_ctx)
    for r in results:
        seeks = sorted({s["seek"] for s in r["segments"]})
        assert seeks[0] == 0 and seeks[-1] < n_frames and all(s["start"] >= s["seek"] * fs - 1e-9 for s in r["segments"])
        assert all(s["temperature"] == 0.0 for s in r["segments"])
    stamped = [l for l in lines if l.startswith("[")]
    assert len(stamped) == sum(1 for r in results for s in r["segments"] if s["text"].strip())
    assert all(re.fullmatch(r"\[\d\d:\d\d\.\d{3} --> \d\d:\d\d\.\d{3}\] \S.*", l) for l in stamped)
    assert [l for l in lines if not l.startswith("[")] == [f"{flac} (en)"] * 2
