"""Top-k / top-p / min-p sampling on the device (csrc/truncate.hip, wm_sample_step), through the C entry and through the engine.

The kernel's cut and kept count are held EXACTLY to the brute force of tests/truncate_refs.py (sorted tokens, Python integers); the
draw to the host's recomputation of the Gumbel arg-max over the kept set with the generator restated in tests/test_gpu_round4.py; the
bookkeeping to log_softmax over the UNtruncated allowed set."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import native  # noqa: E402
import truncate_refs as TR  # noqa: E402
from oracle import decoding_rules as DR  # noqa: E402
from test_gpu_round4 import _host_gumbel  # noqa: E402

IDS = DR.MULTILINGUAL
SB = 3                                      # sample_begin of the kernel-level calls


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return native.load_library()


@pytest.fixture(scope="module")
def lists(golden_dir):
    fixr = np.load(os.path.join(golden_dir, "decoding_rules.npz"))
    sup = sorted(set(fixr["suppress"].tolist() + [IDS.no_timestamps]))
    return sup, [int(t) for t in fixr["blank"]]


def stream():
    return torch.cuda.current_stream().cuda_stream


class Call:
    """One wm_sample_step / wm_greedy_step call on copies of `logits` [B, V] (numpy fp16) and `tokens` [B, cur] (numpy)."""

    def __init__(self, logits, tokens, rules, lists=None, ld=None, tok_ld=24, done=None, row_limit=None, sums=None):
        B, V = logits.shape
        self.B, self.V, self.rules, self.cur = B, V, rules, tokens.shape[1]
        ld = ld or V
        flat = torch.zeros(B * ld + 8, dtype=torch.float16, device="cuda")
        self.lg = torch.as_strided(flat, (B, V), (ld, 1))
        self.lg.copy_(torch.from_numpy(logits))
        self.ld = ld
        self.tok = torch.zeros((B, tok_ld), dtype=torch.int32, device="cuda")
        self.tok[:, :self.cur] = torch.from_numpy(np.asarray(tokens, dtype=np.int32))
        self.sums = torch.zeros(B, dtype=torch.float32, device="cuda") if sums is None else sums
        self.n_done = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.done = torch.zeros(B, dtype=torch.int32, device="cuda") if done is None else done
        self.row_limit = row_limit
        self.sup = torch.tensor(lists[0], dtype=torch.int32, device="cuda") if lists else None
        self.blank = torch.tensor(lists[1], dtype=torch.int32, device="cuda") if lists else None
        self.cut = torch.full((B,), 7.0, dtype=torch.float32, device="cuda")
        self.kept = torch.full((B,), -7, dtype=torch.int32, device="cuda")

    def greedy_io(self, g, T, seed, row0=0, seed_dev=None, n_past_dev=None, cur=None):
        g.logits, g.row_stride, g.batch, g.n_vocab = self.lg.data_ptr(), self.ld, self.B, self.V
        g.tokens, g.tokens_ld, g.cur_len = self.tok.data_ptr(), self.tok.shape[1], self.cur if cur is None else cur
        g.sum_logprobs = self.sums.data_ptr()
        g.suppress, g.n_suppress = (self.sup.data_ptr(), self.sup.numel()) if self.sup is not None else (None, 0)
        g.blank, g.n_blank = (self.blank.data_ptr(), self.blank.numel()) if self.blank is not None else (None, 0)
        g.sample_begin, g.eot, g.timestamp_begin = SB, IDS.eot, IDS.timestamp_begin
        g.max_initial_timestamp_index, g.apply_rules, g.n_done = 50, self.rules, self.n_done.data_ptr()
        g.done = self.done.data_ptr()
        g.row_limit = self.row_limit.data_ptr() if self.row_limit is not None else None
        g.temperature, g.row0, g.seed = T, row0, seed
        g.seed_dev = seed_dev.data_ptr() if seed_dev is not None else None
        g.n_past_dev = n_past_dev.data_ptr() if n_past_dev is not None else None

    def sample_io(self, T, top_k=0, top_p=1.0, min_p=0.0, seed=1, **kw):
        io = native.WmSampleIO()
        self.greedy_io(io.g, T, seed, **kw)
        c, P, gap = TR.scalars(T, top_p, min_p)
        io.top_k, io.exp2_scale, io.top_p_q16, io.min_p_gap = top_k, float(c), P, float(gap)
        io.cut_out, io.kept_out = self.cut.data_ptr(), self.kept.data_ptr()
        return io

    def sample(self, lib, T, top_k=0, top_p=1.0, min_p=0.0, seed=1, st=None, **kw):
        io = self.sample_io(T, top_k, top_p, min_p, seed, **kw)
        native.check(lib.wm_sample_step(C.byref(io), stream() if st is None else st), "wm_sample_step")

    def greedy(self, lib, T, seed=1, **kw):
        io = native.WmGreedyIO()
        self.greedy_io(io, T, seed, **kw)
        native.check(lib.wm_greedy_step(C.byref(io), stream()), "wm_greedy_step")


def allowed_rows(logits, tokens, rules, lists, dominance=None):
    """The logits after the step's rules on the host (oracle/decoding_rules.py): -inf = not allowed."""
    if rules == 0:
        return logits.astype(np.float32)
    rs = DR.RuleSet(IDS, SB, lists[0] if rules == 1 else [t for t in lists[0] if t != IDS.no_timestamps] + [IDS.no_timestamps], lists[1],
                    max_initial_timestamp_index=50, timestamps=rules == 1)
    return DR.apply_filters(logits, np.asarray(tokens), rs, dominance_out=dominance)


def histories(kind_of_row, cur):
    """Token rows [B, cur]: the start sequence and, from sample_begin on, histories that set every state of the timestamp rules."""
    tb = IDS.timestamp_begin
    pat = ([tb + 5, 300, 400], [300, 400, tb + 9], [300, tb + 9, tb + 9], [300, 400, 500])
    rows = []
    for b in range(kind_of_row):
        rows.append([IDS.sot, IDS.lang0, IDS.transcribe] + pat[b % len(pat)][:cur - SB])
    return np.asarray(rows, dtype=np.int32)


def build_rows(B, V, rules, lists, cur, seed):
    """B fixture rows cycling through every kind of truncate_refs.KINDS, their histories and their allowed sets."""
    tb = IDS.timestamp_begin if rules == 1 else None
    tokens = histories(B, cur)
    logits = np.stack([TR.fixture_row(TR.KINDS[b % len(TR.KINDS)], V, seed + b, tb) for b in range(B)])
    probe = allowed_rows(np.zeros((B, V), dtype=np.float16), tokens, rules, lists)
    for b in range(B):
        if TR.KINDS[b % len(TR.KINDS)] == "single":
            logits[b, np.flatnonzero(np.isfinite(probe[b]))[min(11, int(np.isfinite(probe[b]).sum()) - 1)]] = np.float16(-2.5)
    dom = []
    allowed = allowed_rows(logits, tokens, rules, lists, dominance=dom)
    return logits, tokens, allowed, dom


SHAPES = [(1000, 0, 3, SB + 3), (51864, 1, 1, SB + 3), (51865, 1, 3, SB), (51865, 1, 64, SB + 3), (51865, 2, 3, SB + 2), (51865, 1, 12, SB + 2)]


@pytest.mark.parametrize("V,rules,B,cur", SHAPES)
def test_cut_and_kept_equal_the_brute_force(lib, lists, V, rules, B, cur):
    """cut_out / kept_out of every row equal the brute force: no tolerance, no row left out.  Every kind of row (two widths of
    normal rows, a peaked row, one finite logit, all-equal logits, coarse rows with ties across every k-th place and p-boundary, a
    maximum of 65504, everything below -60000, timestamps raised and lowered so that the timestamp rule decides both ways), the first
    sampled step (cur = sample_begin: timestamps up to max_initial_timestamp_index only), every state of the timestamp rules,
    apply_rules 0 / 1 / 2, an even and an odd row stride (rows of 51865 are only 2-byte aligned), 1 / 3 / 12 / 64 rows, every control
    alone and combined at two temperatures (64 rows: every third entry of that list, which still has each control alone and combined).
    The drawn token is never below the cut and the logits row is unchanged apart from the suppress lists."""
    use_lists = lists if rules else None
    logits, tokens, allowed, dom = build_rows(B, V, rules, lists, cur, 100 * B + rules)
    if rules == 1 and cur > SB:
        assert all(abs(d) > 1e-2 for d in dom)                # no row sits on the text-versus-timestamp decision
        if B >= 12:
            assert any(d > 0 for d in dom) and any(d < 0 for d in dom)      # the rule decides for timestamps, and against
    finite = [np.isfinite(allowed[b]) for b in range(B)]
    assert all(f.any() for f in finite)
    ctl = TR.controls(V) if B <= 12 else TR.controls(V)[::3]
    keep = np.ones(V, dtype=bool)                             # where the row must be unchanged: everywhere but the suppress lists
    if rules:
        keep[lists[0]] = False
        if cur == SB:
            keep[lists[1]] = False
    for T in (0.2, 1.0):
        ref_rows = [TR.Row(allowed[b][finite[b]].astype(np.float16), T) for b in range(B)]
        for top_k, top_p, min_p in ctl:
            call = Call(logits, tokens, rules, use_lists)
            call.sample(lib, T, top_k, top_p, min_p, seed=5 + top_k)
            torch.cuda.synchronize()
            cut, kept, drawn = call.cut.cpu().numpy(), call.kept.cpu().numpy(), call.tok[:, cur].cpu().numpy()
            for b in range(B):
                want_cut, want_kept, _ = ref_rows[b].cut(top_k, top_p, min_p)
                assert (float(cut[b]), int(kept[b])) == (float(want_cut), want_kept), (T, top_k, top_p, min_p, b, TR.KINDS[b % len(TR.KINDS)])
                assert finite[b][drawn[b]] and allowed[b][drawn[b]] >= cut[b]
            assert np.array_equal(call.lg.cpu().numpy()[:, keep].view(np.uint16), logits[:, keep].view(np.uint16))


def test_draws_are_the_gumbel_arg_max_over_the_kept_set(lib):
    """4096 equal rows, V = 1000, top_p = 0.9: every token of every row equals the host's recomputation of the arg-max of x / T + g over the kept
    set (the generator of tests/test_gpu_round4.py, to that test's 1e-3); nothing below the cut is ever drawn; the same global rows in
    another launch shape draw the same; another seed draws differently; the frequencies of the kept tokens follow the renormalised
    softmax(x / T) within 4.5 sigma; sum_logprobs books log_softmax over the UNtruncated set within 2e-4 (that test's bound)."""
    V, T, seed, cur, B = 1000, 0.8, 0x1234567890ABCDEF, 9, 4096
    base = TR.fixture_row("normal3", V, 3)
    logits = np.repeat(base[None], B, axis=0)
    tokens = np.full((B, cur), 7, dtype=np.int32)
    call = Call(logits, tokens, 0, tok_ld=16)
    call.sample(lib, T, top_p=0.9, seed=seed, row0=100)
    torch.cuda.synchronize()
    got = call.tok[:, cur].cpu().numpy()
    want_cut, want_kept, _ = TR.Row(base, T).cut(0, 0.9, 0.0)
    assert (call.cut.cpu().numpy() == float(want_cut)).all() and (call.kept.cpu().numpy() == want_kept).all()
    x = base.astype(np.float64)
    kept = x >= float(want_cut)
    assert 1 < want_kept < V and kept[got].all()
    lp = x - (x.max() + np.log(np.exp(x - x.max()).sum()))
    assert np.abs(call.sums.cpu().numpy() - lp[got]).max() < 2e-4
    for b in range(B):                                          # every row: the draw recomputed on the host
        y = np.where(kept, x / T + _host_gumbel(seed & 0xffffffff, seed >> 32, 100 + b, cur, V), -np.inf)
        assert y[got[b]] >= y.max() - 1e-3, b
    small = Call(logits[:64], tokens[:64], 0, tok_ld=16)
    small.sample(lib, T, top_p=0.9, seed=seed, row0=100 + 512)
    assert np.array_equal(small.tok[:, cur].cpu().numpy(), got[512:576])
    pr = np.where(kept, np.exp(x / T - (x / T).max()), 0.0)
    pr /= pr.sum()
    freq = np.bincount(got, minlength=V) / B
    top = np.argsort(-pr)[:20]
    assert (np.abs(freq[top] - pr[top]) <= 4.5 * np.sqrt(pr[top] * (1 - pr[top]) / B) + 1e-4).all()
    other = Call(logits, tokens, 0, tok_ld=16)
    other.sample(lib, T, top_p=0.9, seed=seed + 1, row0=100)
    assert (other.tok[:, cur].cpu().numpy() != got).mean() > 0.5


@pytest.mark.parametrize("top_k,top_p,min_p", [(40, 1.0, 0.02), (40, 0.9, 0.02), (0, 1.0, 0.3), (3, 1.0, 0.0)])
def test_draws_with_top_k_and_min_p_under_the_rules(lib, lists, top_k, top_p, min_p):
    """The same recomputation for EVERY row with top_k and min_p on (alone, together and with top_p), the full vocabulary, Whisper's
    rules on and every state of the timestamp rules: the token is the arg-max of x / T + g over the tokens the brute force keeps.
    Rows of moderate magnitude only: at |x| / T of 8e4 the fp32 spacing of x / T + g is above that test's 1e-3."""
    V, T, seed, cur, B = IDS.n_vocab, 0.7, 0xFEDCBA9876543210, SB + 3, 32
    kinds = ("normal15", "normal3", "peaked", "coarse", "equal", "ts_high", "ts_low")
    tokens = histories(B, cur)
    logits = np.stack([TR.fixture_row(kinds[b % len(kinds)], V, 500 + b, IDS.timestamp_begin) for b in range(B)])
    allowed = allowed_rows(logits, tokens, 1, lists)
    call = Call(logits, tokens, 1, lists)
    call.sample(lib, T, top_k, top_p, min_p, seed=seed, row0=40)
    torch.cuda.synchronize()
    got, cut, n_kept = call.tok[:, cur].cpu().numpy(), call.cut.cpu().numpy(), call.kept.cpu().numpy()
    truncated = 0
    for b in range(B):
        fin = np.isfinite(allowed[b])
        want_cut, want_kept, _ = TR.Row(allowed[b][fin].astype(np.float16), T).cut(top_k, top_p, min_p)
        assert (float(cut[b]), int(n_kept[b])) == (float(want_cut), want_kept), b
        kept = fin & (allowed[b] >= float(want_cut))
        truncated += int(kept.sum()) < int(fin.sum())
        x = allowed[b].astype(np.float64)
        y = np.where(kept, x / T + _host_gumbel(seed & 0xffffffff, seed >> 32, 40 + b, cur, V), -np.inf)
        assert kept[got[b]] and y[got[b]] >= y.max() - 1e-3, b
        lp = x[got[b]] - (x[fin].max() + np.log(np.exp(x[fin] - x[fin].max()).sum()))
        assert abs(float(call.sums[b]) - lp) < 2e-4, b               # the UNtruncated log-probability
    assert truncated >= B // 2


def test_seed_in_device_memory_under_a_replayed_graph(lib):
    """`seed_dev` and `n_past_dev` under a captured, replayed graph: every replay appends one token at the device counter's position
    and draws with the seed the device words hold at that time; each equals the eager call with the same coordinates."""
    V, T, B = 1000, 0.7, 8
    logits = np.stack([TR.fixture_row("normal15", V, 40 + b) for b in range(B)])
    tokens = np.full((B, 4), 7, dtype=np.int32)
    seed_dev = torch.tensor([11, 22], dtype=torch.int32, device="cuda")
    counter = torch.tensor([3], dtype=torch.int32, device="cuda")        # n_past = cur_len - 1
    call = Call(logits, tokens, 0, tok_ld=16)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        call.sample(lib, T, top_k=5, seed_dev=seed_dev, n_past_dev=counter, cur=0, st=side.cuda_stream)     # warm-up on the side stream
        side.synchronize()
        first = call.tok[:, 4].clone()
        with torch.cuda.graph(graph, stream=side):
            call.sample(lib, T, top_k=5, seed_dev=seed_dev, n_past_dev=counter, cur=0, st=torch.cuda.current_stream().cuda_stream)
            native.check(lib.wm_step_advance(counter.data_ptr(), torch.cuda.current_stream().cuda_stream))
    seeds = [(11, 22), (12, 22), (11, 22)]
    pos = 4
    for lo, hi in seeds:
        seed_dev.copy_(torch.tensor([lo, hi], dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        eager = Call(logits, call.tok[:, :pos].cpu().numpy(), 0, tok_ld=16)
        eager.sample(lib, T, top_k=5, seed=(hi << 32) | lo)
        torch.cuda.synchronize()
        assert torch.equal(call.tok[:, pos], eager.tok[:, pos])
        pos += 1
    assert int(counter[0]) == 6 and torch.equal(first, call.tok[:, 4])
    fifth = np.sort(logits.astype(np.float32), axis=1)[:, -5]
    drawn = call.tok[:, 4:7].cpu().numpy()
    assert all(logits[b, drawn[b, j]] >= fifth[b] for b in range(B) for j in range(3))


def test_all_controls_off_is_the_greedy_step(lib, lists):
    """wm_sample_step with all controls off and wm_greedy_step at the same temperature and seed over 8 consecutive steps, with rows
    that end (an EOT raised so that it is drawn), rows at their row_limit and a row already done: tokens, done and n_done are
    identical.  The scan is restated in truncate.hip, not shared with greedy.hip, so sum_logprobs is held to 2e-4, not to equality."""
    V, B, T, steps = IDS.n_vocab, 12, 0.9, 8
    rng = np.random.default_rng(8)
    start = np.asarray([[IDS.sot, IDS.lang0, IDS.transcribe]] * B, dtype=np.int32)
    start[5, SB - 1] = IDS.eot                                # a row that is already done: its last token is EOT
    limit = torch.tensor([100, 2, 100, 0, 5, 100, 100, 3, 100, 100, 100, 100], dtype=torch.int32, device="cuda")
    state = {}
    for name in ("greedy", "sample"):
        done = torch.zeros(B, dtype=torch.int32, device="cuda")
        done[5] = 1
        state[name] = dict(tok=start.copy(), done=done, sums=torch.zeros(B, dtype=torch.float32, device="cuda"), n_done=0)
    for step in range(steps):
        logits = rng.normal(0.0, 1.5, (B, V)).astype(np.float16)
        logits[(step + 5) % B, IDS.eot] = 40.0                # a row ends wherever the rules allow EOT
        for name, st in state.items():
            call = Call(logits, st["tok"], 1, lists, done=st["done"], row_limit=limit, sums=st["sums"], tok_ld=32)
            (call.greedy if name == "greedy" else call.sample)(lib, T, seed=99 + step, row0=7)
            torch.cuda.synchronize()
            st["tok"], st["n_done"] = call.tok[:, :call.cur + 1].cpu().numpy(), int(call.n_done[0])
        g, s = state["greedy"], state["sample"]
        assert np.array_equal(g["tok"], s["tok"]), step
        assert torch.equal(g["done"], s["done"]) and g["n_done"] == s["n_done"], step
        assert float((g["sums"] - s["sums"]).abs().max()) <= 2e-4, step
    s = state["sample"]
    assert int(s["done"].sum()) >= 6 and s["n_done"] >= 6 and int(s["done"].sum()) < B
    assert (s["tok"][3, SB:] == IDS.eot).all() and float(s["sums"][3]) == 0.0          # row_limit 0: EOT at once, nothing booked
    assert (s["tok"][5, SB:] == IDS.eot).all() and float(s["sums"][5]) == 0.0          # the row that was done stays at EOT


def test_refusals_launch_nothing(lib):
    """rc 1, the message names the entry, nothing is written."""
    V, B = 1000, 2
    logits = np.stack([TR.fixture_row("normal15", V, 60 + b) for b in range(B)])
    tokens = np.full((B, 5), 7, dtype=np.int32)
    bad = [dict(T=0.0), dict(T=-1.0), dict(top_k=-1), dict(P=0), dict(P=65537), dict(gap=0.5), dict(gap=float("nan")),
           dict(c=0.0), dict(c=float("inf")), dict(null="logits"), dict(null="tokens"), dict(null="sum_logprobs"), dict(cur=24)]
    for case in bad:
        call = Call(logits, tokens, 0)
        io = call.sample_io(0.8, top_k=case.get("top_k", 3), top_p=0.9)
        if "T" in case:
            io.g.temperature = case["T"]
        if "P" in case:
            io.top_p_q16 = case["P"]
        if "gap" in case:
            io.min_p_gap = case["gap"]
        if "c" in case:
            io.exp2_scale = case["c"]
        if "null" in case:
            setattr(io.g, case["null"], None)
        if "cur" in case:
            io.g.cur_len = case["cur"]
        before = call.tok.clone()
        rc = lib.wm_sample_step(C.byref(io), stream())
        torch.cuda.synchronize()
        assert rc == 1, case
        assert "wm_sample_step" in lib.wm_last_error().decode(), case
        assert torch.equal(call.tok, before) and float(call.sums.abs().sum()) == 0.0 and int(call.n_done[0]) == 0, case
        assert (call.kept == -7).all() and (call.cut == 7.0).all(), case
    ok = Call(logits, tokens, 0)
    ok.sample(lib, 0.8)                                       # all controls off is accepted
    torch.cuda.synchronize()
    assert (ok.kept.cpu().numpy() == V).all()


# ------------------------------------------------------------------------------------------------------------ the engine loops
# micro-fullvocab only: the 1024-token vocabulary of `micro` holds none of the special tokens Whisper's rules index, so no loop of
# WhisperDecoding runs on it (the suite's other loop tests use micro-fullvocab for the same reason).
import synthetic  # noqa: E402
import transcribe as T  # noqa: E402
from decoding import DecodingOptions, WhisperDecoding  # noqa: E402
from encoding import WhisperEncoding  # noqa: E402
from oracle.whisper_oracle import Dims, synthetic_mel  # noqa: E402
from test_gpu_model import build_engine  # noqa: E402

DIMS = Dims(**synthetic.DIMS["micro-fullvocab"])
W = 2 * DIMS.n_audio_ctx


@pytest.fixture(scope="module")
def stock(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    eng = build_engine(str(tmp_path_factory.mktemp("truncate_engines")), "micro-fullvocab", 3)
    enc = WhisperEncoding(eng)
    xa = enc.get_audio_features(synthetic_mel(3, W, DIMS.n_mels, 41).cuda())
    return eng, enc, xa


def counted(dec):
    """Count the token steps `dec` issues through each entry (eager calls and captures: a replayed graph issues none)."""
    n = {"sample": 0, "greedy": 0}
    sample, greedy = dec._sample, dec._greedy
    dec._sample = lambda *a, **k: (n.__setitem__("sample", n["sample"] + 1), sample(*a, **k))[1]
    dec._greedy = lambda *a, **k: (n.__setitem__("greedy", n["greedy"] + 1), greedy(*a, **k))[1]
    return n


def test_top_k_1_at_temperature_07_decodes_the_tokens_of_temperature_0(stock):
    """top_k = 1 keeps the class of the maximum, so a draw at any temperature is the arg-max (model seed 3, clips of seed 41: no row's
    maximum is tied at any step, or the arg-max would not be the only candidate).  Eager + capture, then the replayed graphs, then
    the literal loop with the masked Categorical.  The booked log-probabilities are those of temperature 0: untruncated."""
    eng, enc, xa = stock
    base = WhisperDecoding(eng, options=DecodingOptions(sample_len=16, language="en"))
    t0, lp0, _ = base.main_loop(xa)
    base._state.clear()
    dec = WhisperDecoding(eng, options=DecodingOptions(sample_len=16, language="en", temperature=0.7, top_k=1))
    n = counted(dec)
    for seed in (1, 2):
        torch.manual_seed(seed)
        t1, lp1, _ = dec.main_loop(xa)
        assert torch.equal(t1.cpu(), t0.cpu()) and torch.allclose(lp1.cpu(), lp0.cpu(), atol=2e-3)
    assert n["sample"] > 0 and n["greedy"] == 0
    t_ref, lp_ref, _ = dec.main_loop_reference(xa)
    assert torch.equal(t_ref.cpu(), t0.cpu()) and torch.allclose(lp_ref.cpu(), lp0.cpu(), atol=2e-3)
    assert float(lp0.max()) < -1.0                              # (not the zeros a truncated distribution would book)
    dec._state.clear()


def test_two_calls_replay_the_graph_and_follow_the_seed(stock):
    eng, enc, xa = stock
    dec = WhisperDecoding(eng, options=DecodingOptions(sample_len=16, language="en", temperature=0.8, top_k=50, top_p=0.9, min_p=0.01))
    n = counted(dec)
    torch.manual_seed(5)
    t1, lp1, _ = dec.main_loop(xa)
    assert n["sample"] > 0
    graphs = dict(dec._state[3]['graphs'])
    torch.manual_seed(5)
    t2, lp2, _ = dec.main_loop(xa)
    assert torch.equal(t1.cpu(), t2.cpu()) and torch.equal(lp1.cpu(), lp2.cpu())
    assert graphs and all(dec._state[3]['graphs'][k] is g for k, g in graphs.items()) and n["greedy"] == 0
    torch.manual_seed(6)
    t3, _, _ = dec.main_loop(xa)
    assert not torch.equal(t1.cpu(), t3.cpu())
    plain = WhisperDecoding(eng, options=DecodingOptions(sample_len=16, language="en", temperature=0.8))
    torch.manual_seed(5)
    t4, _, _ = plain.main_loop(xa)
    assert not torch.equal(t1.cpu(), t4.cpu())                  # near-uniform logits: the untruncated draw leaves the kept set at once
    dec._state.clear()
    plain._state.clear()


@pytest.mark.parametrize("shared", [False, True])
def test_best_of_3_with_top_p(stock, shared):
    eng, enc, xa = stock
    dec = WhisperDecoding(eng, options=DecodingOptions(sample_len=8, language="en", temperature=0.9, best_of=3, top_p=0.8), shared_cross_kv=shared)
    n = counted(dec)
    out = []
    for _ in range(2):
        torch.manual_seed(7)
        t, lp, nsp = dec.main_loop(xa)
        out.append((t.cpu(), lp.cpu()))
        assert t.shape[0] == 9 and len(nsp) == 9
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert n["sample"] > 0 and n["greedy"] == 0
    grp = out[0][0].numpy().reshape(3, 3, -1)
    assert sum(len({tuple(r) for r in g.tolist()}) > 1 for g in grp) >= 2          # candidates of an utterance differ
    res = dec.post_process(t, lp, nsp, xa, ["en"] * 3)
    assert len(res) == 3 and all(np.isfinite(r.avg_logprob) and r.temperature == 0.9 for r in res)
    dec._state.clear()


def test_the_long_form_ladder_climbs_through_the_sampling_step(stock):
    """transcribe_mel with temperatures (0.0, 0.6) and top_p on: the calls at 0 take wm_greedy_step, the calls at 0.6 wm_sample_step,
    and every row settles."""
    eng, enc, _ = stock
    contents = [100, 300]
    mels = [synthetic_mel(1, c + W, DIMS.n_mels, 900 + i)[0].cuda().contiguous() for i, c in enumerate(contents)]
    dec = WhisperDecoding(eng, options=DecodingOptions(language="en", top_p=0.9))
    dec.sample_len = 12
    n = counted(dec)
    trace = []
    results = T.transcribe_mel(enc, dec, mels, contents, n_rows=2, trace=trace, temperatures=(0.0, 0.6), compression_ratio_threshold=None,
                               logprob_threshold=-1.0, no_speech_threshold=None)
    assert len(results) == 2 and all(r["segments"] for r in results)
    assert {e["temperature"] for e in trace} == {0.0, 0.6} and n["sample"] > 0 and n["greedy"] > 0
    for r, c in zip(results, contents):
        assert all(s["temperature"] in (0.0, 0.6) for s in r["segments"]) and max(s["seek"] for s in r["segments"]) < c
    dec._state.clear()


def test_defaults_and_temperature_0_never_reach_the_entry(stock, monkeypatch):
    eng, enc, xa = stock
    lib = native.load_library()

    def boom(*a, **k):
        raise AssertionError("wm_sample_step called without a reason")
    monkeypatch.setattr(lib, "wm_sample_step", boom)
    cases = [dict(), dict(temperature=0.7), dict(temperature=0.7, best_of=2), dict(top_k=5, top_p=0.5, min_p=0.1),
             dict(beam_size=2, top_k=5, top_p=0.5)]
    for options in cases:
        dec = WhisperDecoding(eng, options=DecodingOptions(sample_len=6, language="en", **options))
        for _ in range(2):
            dec.main_loop(xa)
        dec._state.clear()
    on = WhisperDecoding(eng, options=DecodingOptions(sample_len=6, language="en", temperature=0.7, top_k=5))
    on.cu_partition = True
    with pytest.raises(ValueError, match="cu_partition"):
        on.main_loop(xa)
    on.cu_partition = False
    with pytest.raises(AssertionError, match="without a reason"):       # (the patch does catch a call)
        on.main_loop(xa)
    torch.cuda.synchronize()
