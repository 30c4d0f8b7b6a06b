"""The device decode loop in its three phases on a real MI355X: a call that issues eagerly and captures, a call that replays, and a call
with graphs off give the same bits -- tokens, log-probability sums and every layer's self-attention cache -- and the captured graphs
are filed under the keys bench.py, the lab scripts and the other suites look them up by."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import synthetic  # noqa: E402
from decoding import DecodingOptions, WhisperDecoding  # noqa: E402
from encoding import WhisperEncoding  # noqa: E402
from oracle.whisper_oracle import Dims, synthetic_mel  # noqa: E402
from test_gpu_model import build_engine  # noqa: E402

DIMS = Dims(**synthetic.DIMS["micro-fullvocab"])
L0 = 3          # <|startoftranscript|> <|en|> <|transcribe|>


@pytest.fixture(scope="module")
def stock(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    eng = build_engine(str(tmp_path_factory.mktemp("loop_engines")), "micro-fullvocab", 3)
    return eng, WhisperEncoding(eng)


# keys: per group the token step's (n_micro, slot, use_live) and the prefill's (n_micro, slot, use_live, 'prefill', L0, not_alone),
# then what the call bakes in
CASES = {
    # one group of two rows: the one-launch step
    "one_group": dict(n_audio=2, options=dict(), keys={(1, 0, True), (1, 0, True, 'prefill', 3, False)}),
    # two groups of four side by side: every launch says not_alone
    "two_groups": dict(n_audio=8, options=dict(), micro=2,
                       keys={(2, 0, True), (2, 0, True, 'prefill', 3, True), (2, 1, True), (2, 1, True, 'prefill', 3, True)}),
    "beam": dict(n_audio=2, options=dict(beam_size=2),
                 keys={(1, 0, True, 'beam', False), (1, 0, True, 'prefill', 3, False, 'beam', False)}),
    "shared_best_of": dict(n_audio=2, options=dict(best_of=2, temperature=0.7), kw=dict(shared_cross_kv=True), seed=11,
                           keys={(1, 0, True, ('cross_group', 2)), (1, 0, True, 'prefill', 3, False, ('cross_group', 2))}),
    # a sampling call of a beam instance: three rows per utterance, the third closed before its first token
    "per_call_temperature": dict(n_audio=2, options=dict(beam_size=3), kw=dict(shared_cross_kv=True, fallback_best_of=2), seed=12,
                                 temperature=0.4,
                                 keys={(1, 0, True, ('cross_group', 3), ('temperature', 0.4)),
                                       (1, 0, True, 'prefill', 3, False, ('cross_group', 3), ('temperature', 0.4))}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_eager_capture_replay_and_graphless_calls_give_the_same_bits(stock, name):
    case = CASES[name]
    eng, enc = stock
    n_audio = case["n_audio"]
    xa = enc.get_audio_features(synthetic_mel(n_audio, 2 * DIMS.n_audio_ctx, DIMS.n_mels, 41).cuda())
    dec = WhisperDecoding(eng, options=DecodingOptions(sample_len=6, language="en", **case["options"]), **case.get("kw", {}))
    dec.micro_batches = case.get("micro")
    assert dec.sample_begin == L0
    n_batch = n_audio * dec.n_group
    runs = []
    for phase, use_graphs in (("eager + capture", True), ("replay", True), ("no graphs", False)):
        dec.use_graphs = use_graphs
        if "seed" in case:
            torch.manual_seed(case["seed"])
        t, lp, _ = dec.main_loop(xa, temperature=case.get("temperature"))
        torch.cuda.synchronize()
        st = dec._state[n_batch]
        runs.append((phase, t.cpu(), lp.cpu(), [c.clone() for c in st['kv']]))
        if phase == "eager + capture":
            assert set(st['graphs']) == case["keys"], "after the first call"
    assert set(dec._state[n_batch]['graphs']) == case["keys"]
    assert runs[0][1].shape[0] == n_batch and runs[0][1].shape[1] > L0
    _, t0, lp0, kv0 = runs[0]
    for phase, t, lp, kv in runs[1:]:
        assert torch.equal(t, t0), phase
        assert torch.equal(lp, lp0), phase
        for layer, (a, b) in enumerate(zip(kv, kv0)):
            assert torch.equal(a, b), (phase, layer)
    dec._state.clear()
