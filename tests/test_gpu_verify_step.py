"""wm_verify_step (csrc/speculative.hip) through the C entry: the verify step of speculative decoding.

The contract is bit for bit: after the call, tokens, sum_logprobs (as fp32 bits), done and n_done are what n_accept successive
wm_greedy_step calls at temperature 0 leave behind, made here on copies of the same buffers (one row, one position per call, the
logits row at the same offset from a 16-byte boundary: the scan's scalar head, and with it the order of its fp32 sums, depends on
it).  n_accept is the host rule's (speculative.accept_length) on tokens the logits were built to elect by a clear margin, checked
with the host rules of oracle/decoding_rules.py.  Built on tests/test_gpu_truncate.py's `Call`."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import native  # noqa: E402
import speculative as S  # noqa: E402
from test_gpu_truncate import IDS, SB, Call, allowed_rows, lib, lists, stream  # noqa: E402,F401 (fixtures)

TOK_LD = 24
EOT, TB = IDS.eot, IDS.timestamp_begin
WANTED, DECOY, MARGIN = 14.0, 30.0, 3.0      # the elected token's logit, a forbidden token's, and the least lead of the elected one


class RefCall(Call):
    """`Call` with the logits row `offset` elements behind a 16-byte boundary."""

    def __init__(self, logits, tokens, rules, lists=None, offset=0, **kw):
        super().__init__(logits, tokens, rules, lists, **kw)
        B, V = logits.shape
        flat = torch.zeros(B * self.ld + 16, dtype=torch.float16, device="cuda")
        self.lg = torch.as_strided(flat, (B, V), (self.ld, 1), storage_offset=offset)
        self.lg.copy_(torch.from_numpy(logits))


# the states of the timestamp rules (test_gpu_truncate.histories) and, per state, kinds of tokens the rules allow position by position
STATES = (([TB + 5, 300, 400], ("text", "text", "ts", "ts")),          # text, text: anything; an accepted timestamp at 2 forces one at 3
          ([300, 400, TB + 9], ("ts", "text", "ts", "ts")),            # text, timestamp: a timestamp (or EOT) must follow
          ([300, TB + 9, TB + 9], ("text", "ts", "ts", "text")),       # timestamp pair: text only, then a pair again
          ([300, 400, 500], ("ts", "ts", "text", "text")))             # all text: a pair opens at 0, closes at 1, text after it


def structural_mask(V, history, rules, lists):
    """Which tokens the rules allow behind `history`, the text-versus-timestamp decision aside (timestamps far below the text)."""
    probe = np.zeros((1, V), dtype=np.float16)
    probe[0, TB:] = -20.0
    return np.isfinite(allowed_rows(probe, np.asarray([history], dtype=np.int32), rules, lists)[0])


def choose(kind, mask, b, j):
    if kind == "eot":
        return EOT
    if kind == "ts":
        return int(np.flatnonzero(mask[TB:])[0]) + TB + 3
    t = 1000 + 97 * b + 13 * j
    while not mask[t]:
        t += 1
    return t


def build_case(V, rules, lists, rows, n_pos, cur, seed):
    """Logits [B, n_pos, V], token rows [B, TOK_LD] with the proposals in place, and per row the tokens the logits elect."""
    rng = np.random.default_rng(seed)
    B = len(rows)
    logits = rng.normal(0.0, 1.5, (B, n_pos, V)).astype(np.float16)
    tokens = np.zeros((B, TOK_LD), dtype=np.int32)
    elected = []
    decoys = [301, TB + 1, TB + 1400, IDS.no_timestamps, IDS.sot] + ([lists[1][0]] if rules else [])
    for b, row in enumerate(rows):
        hist, wanted = [int(t) for t in row["history"]], []
        assert len(hist) == cur
        for j in range(n_pos):
            mask = structural_mask(V, hist + wanted, rules, lists if rules else None)
            t = choose(row["kinds"][j], mask, b, j)
            assert mask[t], (b, j, row["kinds"][j])
            for d in decoys:                       # tokens the rules forbid here, far above everything: a rule not applied shows
                if not mask[d]:
                    logits[b, j, d] = DECOY
            logits[b, j, t] = WANTED
            wanted.append(t)
        if row.get("inf_at") is not None:
            logits[b, row["inf_at"], :] = -np.inf
        proposals = wanted[:n_pos - 1]
        if row.get("mismatch_at") is not None and row["mismatch_at"] < n_pos - 1:
            m = row["mismatch_at"]
            proposals[m] = proposals[m] + 1 if proposals[m] != EOT else 300
        tokens[b, :cur] = hist
        tokens[b, cur:cur + n_pos - 1] = proposals
        elected.append(wanted)
    return logits, tokens, elected


def expected_picks(rows, elected, tokens, rules, lists, logits, n_pos, cur, limit):
    """Per row the main engine's token at every position on the accepted path (None for a finished row), from the host rules: the
    elected token, EOT at a reached row_limit or on a row of -inf.  Checks the clear margin with oracle/decoding_rules.py."""
    out = []
    for b, row in enumerate(rows):
        if tokens[b, cur - 1] == EOT:
            out.append(None)
            continue
        picks = []
        for j in range(n_pos):
            capped = limit is not None and cur + j - SB >= int(limit[b])
            if capped or row.get("inf_at") == j:
                picks.append(EOT)
                continue
            hist = np.asarray([list(tokens[b, :cur]) + elected[b][:j]], dtype=np.int32)
            allowed = allowed_rows(logits[b, j][None], hist, rules, lists if rules else None)[0]
            order = np.argsort(-allowed)
            assert order[0] == elected[b][j] and allowed[order[0]] - allowed[order[1]] >= MARGIN, (b, j)
            picks.append(elected[b][j])
        out.append(picks)
    return out


def verify_io(lib, call, lg, row_stride, pos_stride, n_pos, n_acc, ws, cur):
    io = native.WmVerifyIO()
    call.greedy_io(io.g, 0.0, 1, cur=cur)
    io.g.logits, io.g.row_stride = lg.data_ptr(), row_stride
    io.pos_stride, io.n_pos = pos_stride, n_pos
    io.n_accept, io.workspace = n_acc.data_ptr(), ws.data_ptr()
    return io


class Verify:
    """One wm_verify_step call: logits [B, n_pos, V] laid out with `pos_stride` between positions, `base_off` elements behind a 16-byte
    boundary; the token rows hold history and proposals."""

    def __init__(self, lib, logits, tokens, rules, lists, cur, pad=3, base_off=0, done=None, limit=None, sums=None):
        B, n_pos, V = logits.shape
        self.pos_stride, self.base_off = V + pad, base_off
        self.row_stride = n_pos * self.pos_stride + 5
        flat = torch.zeros(base_off + B * self.row_stride + 8, dtype=torch.float16, device="cuda")
        self.lg = torch.as_strided(flat, (B, n_pos, V), (self.row_stride, self.pos_stride, 1), storage_offset=base_off)
        self.lg.copy_(torch.from_numpy(logits))
        self.call = Call(logits[:, 0], tokens[:, :cur], rules, lists if rules else None, tok_ld=TOK_LD, done=done, row_limit=limit, sums=sums)
        self.call.tok.copy_(torch.from_numpy(tokens))
        self.n_acc = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        self.ws = torch.empty(max(8, lib.wm_verify_workspace_bytes(B, n_pos)), dtype=torch.uint8, device="cuda")
        self.io = verify_io(lib, self.call, self.lg, self.row_stride, self.pos_stride, n_pos, self.n_acc, self.ws, cur)

    def run(self, lib, st=None):
        native.check(lib.wm_verify_step(C.byref(self.io), stream() if st is None else st), "wm_verify_step")

    def state(self):
        torch.cuda.synchronize()
        c = self.call
        return dict(tok=c.tok.cpu().numpy(), sums=c.sums.cpu().numpy().view(np.int32), done=c.done.cpu().numpy(),
                    n_done=int(c.n_done[0]), n_acc=self.n_acc.cpu().numpy())

    def offset_of(self, b, j):
        return (self.base_off + b * self.row_stride + j * self.pos_stride) % 8


def greedy_reference(lib, logits, tokens, rules, lists, cur, offset_of, done0, limit, sums0):
    """The same rows through real wm_greedy_step calls, one row and one position at a time, up to the first mismatch."""
    B, n_pos, _ = logits.shape
    tok, n_acc, n_done = tokens.copy(), np.zeros(B, dtype=np.int32), 0
    sums = torch.zeros(B, dtype=torch.float32, device="cuda") if sums0 is None else sums0.clone()
    done = torch.zeros(B, dtype=torch.int32, device="cuda") if done0 is None else done0.clone()
    for b in range(B):
        if tok[b, cur - 1] == EOT:
            continue
        for j in range(n_pos):
            rc = RefCall(logits[b, j][None], tok[b:b + 1, :cur + j], rules, lists if rules else None, offset=offset_of(b, j), tok_ld=TOK_LD,
                         done=done[b:b + 1], row_limit=None if limit is None else limit[b:b + 1], sums=sums[b:b + 1])
            rc.greedy(lib, 0.0)
            torch.cuda.synchronize()
            t, proposal = int(rc.tok[0, cur + j]), int(tok[b, cur + j])
            n_done += int(rc.n_done[0])
            tok[b, cur + j] = t
            n_acc[b] += 1
            if t == EOT or j == n_pos - 1 or t != proposal:
                break
    torch.cuda.synchronize()
    return dict(tok=tok, sums=sums.cpu().numpy().view(np.int32), done=done.cpu().numpy(), n_done=n_done, n_acc=n_acc)


def check_case(lib, lists, V, rules, rows, n_pos, cur, seed, pad=3, base_off=0, limit=None, sums0=None):
    """Build, verify, compare with the greedy reference and with the host rule.  Returns n_accept."""
    logits, tokens, elected = build_case(V, rules, lists, rows, n_pos, cur, seed)
    B = len(rows)
    done0 = torch.tensor([int(tokens[b, cur - 1] == EOT) for b in range(B)], dtype=torch.int32, device="cuda")
    limit_dev = None if limit is None else torch.tensor(limit, dtype=torch.int32, device="cuda")
    picks = expected_picks(rows, elected, tokens, rules, lists, logits, n_pos, cur, limit)
    want_acc = [0 if p is None else S.accept_length(p, list(tokens[b, cur:cur + n_pos - 1]), EOT) for b, p in enumerate(picks)]
    v = Verify(lib, logits, tokens, rules, lists, cur, pad=pad, base_off=base_off, done=done0.clone(), limit=limit_dev,
               sums=None if sums0 is None else sums0.clone())
    v.run(lib)
    got = v.state()
    ref = greedy_reference(lib, logits, tokens, rules, lists, cur, v.offset_of, done0, limit_dev, sums0)
    assert got["n_acc"].tolist() == want_acc == ref["n_acc"].tolist()
    assert np.array_equal(got["tok"], ref["tok"])
    assert np.array_equal(got["sums"], ref["sums"]), (got["sums"].view(np.float32), ref["sums"].view(np.float32))
    assert np.array_equal(got["done"], ref["done"]) and got["n_done"] == ref["n_done"]
    for b, p in enumerate(picks):                             # ... and the tokens are the ones the host rules elect
        if p is not None:
            assert got["tok"][b, cur:cur + want_acc[b]].tolist() == p[:want_acc[b]], b
            assert np.array_equal(got["tok"][b, cur + want_acc[b]:], tokens[b, cur + want_acc[b]:]), b      # later slots untouched
    return want_acc


def state_rows(B, n_pos, accept):
    """B rows cycling through the states of the timestamp rules; row b accepts accept(b) slots (a mismatch at accept - 1, none for n_pos)."""
    rows = []
    for b in range(B):
        hist, kinds = STATES[b % len(STATES)]
        a = accept(b)
        rows.append(dict(history=[IDS.sot, IDS.lang0, IDS.transcribe] + hist, kinds=kinds, mismatch_at=a - 1 if a < n_pos else None))
    return rows


@pytest.mark.parametrize("n_pos", [1, 2, 3, 4])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("V", [51865, 51866])
def test_every_accept_length_in_every_state_of_the_timestamp_rules(lib, lists, V, B, n_pos):
    """Accept lengths 1 .. n_pos (a mismatch at 0 among them), a different outcome per row, every state of the timestamp rules in
    `histories()` -- including proposals that are timestamps and change the rules of the next position -- n_vocab odd and even, a
    pos_stride larger than the row.  One row: every accept length in turn."""
    cur = SB + 3
    shifts = range(n_pos) if B == 1 else (0, 2)
    seen = set()
    for shift in shifts:
        rows = state_rows(B, n_pos, lambda b: (b + shift) % n_pos + 1)
        if B == 1:
            rows[0].update(history=[IDS.sot, IDS.lang0, IDS.transcribe] + STATES[shift][0], kinds=STATES[shift][1])
        seen |= set(check_case(lib, lists, V, 1, rows, n_pos, cur, seed=V + 10 * B + n_pos + shift))
    assert seen == set(range(1, n_pos + 1))


@pytest.mark.parametrize("V", [51865, 51866])
def test_eot_in_the_middle_a_done_row_row_limit_and_the_row_of_minus_infinity(lib, lists, V):
    """Five rows, four positions: EOT proposed and accepted at position 1 (later slots stay untouched, done and n_done are set); a row
    whose previous token is EOT (n_accept 0, nothing moves); row_limit reached at position 2 (EOT, nothing booked for it); a row of
    -inf at position 1 (EOT, the sum becomes -inf); a mismatch at 0.  The sums start from values of their own."""
    cur, n_pos = SB + 3, 4
    start = [IDS.sot, IDS.lang0, IDS.transcribe]
    rows = [dict(history=start + [300, 400, 500], kinds=("text", "eot", "text", "text")),
            dict(history=start + [300, 400, EOT], kinds=("text", "text", "text", "text")),
            dict(history=start + [300, 400, 500], kinds=("text", "text", "text", "text")),
            dict(history=start + [TB + 5, 300, 400], kinds=("text", "text", "text", "text"), inf_at=1),
            dict(history=start + [300, TB + 9, TB + 9], kinds=("text", "text", "ts", "ts"), mismatch_at=0)]
    limit = [100, 100, 3 + 2, 100, 100]
    sums0 = torch.tensor([-1.5, -2.25, -0.125, -7.0, 0.0], dtype=torch.float32, device="cuda")
    assert check_case(lib, lists, V, 1, rows, n_pos, cur, seed=7, limit=limit, sums0=sums0) == [2, 0, 3, 2, 1]


@pytest.mark.parametrize("rules", [1, 2])
def test_the_first_sampled_position(lib, lists, rules):
    """cur_len = sample_begin: SuppressBlank and max_initial_timestamp hold at position 0 only (a blank token and a late timestamp stand
    far above the elected token there), a timestamp accepted at 0 decides what position 1 may be.  Also without the timestamp rules."""
    start = [IDS.sot, IDS.lang0, IDS.transcribe]
    kinds = ("ts", "text", "text", "ts") if rules == 1 else ("text", "text", "text", "text")
    rows = [dict(history=start, kinds=kinds, mismatch_at=m) for m in (None, 0, 1, 2, None)]
    assert check_case(lib, lists, 51865, rules, rows, 4, SB, seed=40 + rules) == [4, 1, 2, 3, 4]


@pytest.mark.parametrize("rules", [0, 1, 2])
@pytest.mark.parametrize("base_off,pad", [(0, 3), (1, 4), (3, 11)])
def test_apply_rules_and_odd_aligned_bases(lib, lists, rules, base_off, pad):
    """apply_rules 0 / 1 / 2 with the logits base 0, 1 and 3 elements behind a 16-byte boundary and odd and even position strides: the
    scalar head of the scan takes every length."""
    rows = state_rows(5, 3, lambda b: b % 3 + 1)
    if rules != 1:
        for row in rows:
            row["kinds"] = ("text", "ts", "text")           # no timestamp rules: any order of classes is allowed
    assert check_case(lib, lists, 51865, rules, rows, 3, SB + 3, seed=90 + rules, pad=pad, base_off=base_off) == [1, 2, 3, 1, 2]


def test_capture_and_replay(lib, lists):
    """The two launches captured into a graph and replayed on fresh copies of the state give what the eager call gives."""
    rows = state_rows(5, 4, lambda b: b % 4 + 1)
    logits, tokens, _ = build_case(51865, 1, lists, rows, 4, SB + 3, seed=5)
    eager = Verify(lib, logits, tokens, 1, lists, SB + 3)
    eager.run(lib)
    want = eager.state()
    v = Verify(lib, logits, tokens, 1, lists, SB + 3)
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        v.run(lib, side.cuda_stream)                          # warm-up on the side stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            v.run(lib, torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        v.lg.copy_(torch.from_numpy(logits))
        v.call.tok.copy_(torch.from_numpy(tokens))
        v.call.sums.zero_(); v.call.done.zero_(); v.call.n_done.zero_(); v.n_acc.fill_(-7)
        torch.cuda.synchronize()
        graph.replay()
        got = v.state()
        assert want["n_acc"].tolist() == [1, 2, 3, 4, 1]
        for name in ("tok", "sums", "done", "n_acc"):
            assert np.array_equal(got[name], want[name]), name
        assert got["n_done"] == want["n_done"]


def test_refusals_launch_nothing(lib, lists):
    """rc 1, the message names the entry, nothing is written."""
    rows = state_rows(2, 3, lambda b: 3)
    logits, tokens, _ = build_case(51865, 1, lists, rows, 3, SB + 3, seed=6)
    counter = torch.tensor([SB + 2], dtype=torch.int32, device="cuda")
    seed_dev = torch.tensor([1, 2], dtype=torch.int32, device="cuda")
    bad = [dict(temperature=0.7), dict(n_past_dev=counter.data_ptr()), dict(seed_dev=seed_dev.data_ptr()), dict(n_pos=0), dict(n_pos=5),
           dict(n_pos=-1), dict(null="n_accept"), dict(null="workspace"), dict(null_g="logits"), dict(null_g="tokens"),
           dict(null_g="sum_logprobs"), dict(cur_len=0), dict(cur_len=TOK_LD - 2), dict(pos_stride=51864), dict(row_stride=2 * (51865 + 3) + 51864), dict(ws_off=4)]
    for case in bad:
        v = Verify(lib, logits, tokens, 1, lists, SB + 3)
        for name in ("temperature", "n_past_dev", "seed_dev", "cur_len"):
            if name in case:
                setattr(v.io.g, name, case[name])
        for name in ("n_pos", "pos_stride"):
            if name in case:
                setattr(v.io, name, case[name])
        if "row_stride" in case:                               # one element short of the three positions of a row (two rows)
            v.io.g.row_stride = case["row_stride"]
        if "ws_off" in case:
            v.io.workspace = v.ws.data_ptr() + case["ws_off"]
        if "null" in case:
            setattr(v.io, case["null"], None)
        if "null_g" in case:
            setattr(v.io.g, case["null_g"], None)
        rc = lib.wm_verify_step(C.byref(v.io), stream())
        got = v.state()
        assert rc == 1, case
        assert "wm_verify_step" in lib.wm_last_error().decode(), case
        assert np.array_equal(got["tok"], tokens) and not got["sums"].any() and not got["done"].any() and got["n_done"] == 0, case
        assert (got["n_acc"] == -7).all(), case
    assert lib.wm_verify_step(None, stream()) == 1
    ok = Verify(lib, logits, tokens, 1, lists, SB + 3)
    ok.io.g.cur_len = SB + 3
    ok.run(lib)
    assert ok.state()["n_acc"].tolist() == [3, 3]
