"""Hotwords and sequence bias on a real MI355X: wm_sequence_bias (csrc/bias.hip) through the C entry, bit for bit against the brute
force of tests/bias_refs.py -- whole buffers, guard elements included -- and the bias inside every device loop -- greedy, beam, long-form
-- against the literal loops, whose filter the CPU tests (tests/test_bias_cpu.py) hold to the same brute force.

The hotwords of the loop tests are made of tokens the stock model (seed 3, mel seed 41) samples anyway: picked on the CPU torch path,
where the default biases (3.0 / 1.5) change 18 to 20 of every row's 24 tokens."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import biasing as BI  # noqa: E402
import longform as LF  # noqa: E402
import native  # noqa: E402
import synthetic  # noqa: E402
import test_gpu_beam as BM  # noqa: E402  (helpers only)
import transcribe as T  # noqa: E402
from bias_refs import bias_batch  # noqa: E402
from decoding import DecodingOptions, WhisperDecoding  # noqa: E402
from encoding import WhisperEncoding  # noqa: E402
from oracle.whisper_oracle import Dims, synthetic_mel  # noqa: E402
from test_gpu_beam import engines  # noqa: E402,F401  (module fixture: the peaked fp16 / int8 engines and four clips)
from test_gpu_decode_loop import CASES as LOOP_CASES  # noqa: E402
from test_gpu_model import build_engine  # noqa: E402

DIMS = Dims(**synthetic.DIMS["micro-fullvocab"])
W = 2 * DIMS.n_audio_ctx
MODEL_SEED, MEL_SEED = 3, 41
SENTINEL = 0x7a5a                    # a finite fp16 pattern no case produces
BOUND = 512                          # WM_REPEAT_MAX_HISTORY
HOTWORDS = ((8952, 34168), (46939, 1294), (34532, 17886, 8952), (1000, 1001))


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return native.load_library()


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------ the kernel alone
FIRST, GUARD, LD, SAMPLE_BEGIN = 3, 64, 3 + BOUND, 3
SPECIAL = [0.0, -0.0, 5.96e-8, 65504.0, -65504.0, -np.inf, 65472.0, -65472.0, 1.0]


def alphabet_of(eot):
    return np.array([1, 2, 3, eot // 2, eot - 2, eot - 1])


def make_table(rng, n, eot, extra_hotwords=()):
    """A built table of exactly n items: the given hotwords, then sequences over a six-token alphabet (so that prefixes do occur in the
    histories) whose targets are alphabet tokens or any text token, biases of either sign."""
    alpha = alphabet_of(eot)
    seqs, seen = [], set()
    table = BI.build_table(hotwords=extra_hotwords or None, eot=eot)
    seen |= {(t, p) for t, _, p, _ in table.items}
    assert len(seen) <= n
    while len(seen) < n:
        k = int(rng.integers(0, 4))
        prefix = tuple(int(t) for t in rng.choice(alpha, size=k))
        target = int(rng.choice(alpha)) if rng.random() < 0.5 else int(rng.integers(0, eot))
        if (target, prefix) in seen:
            continue
        seen.add((target, prefix))
        seqs.append((prefix + (target,), float(np.float32(rng.choice([-1, 1]) * rng.uniform(0.25, 12)))))
    table = BI.build_table(hotwords=extra_hotwords or None, sequence_bias=tuple(seqs) or None, eot=eot)
    assert len(table) == n
    return table


def histories(rng, batch, m, eot, V, phrase32):
    """Row b by b % 4: 0 the alphabet at random, 1 ONE token throughout (every item of a phrase (a, a, a, a) matches at once), 2 the
    alphabet with a timestamp every fifth token (breaks phrases), 3 the 32-token phrase over and over."""
    alpha = alphabet_of(eot)
    H = np.zeros((batch, m), dtype=np.int64)
    for b in range(batch):
        kind = b % 4
        if kind == 0:
            H[b] = rng.choice(alpha, size=m)
        elif kind == 1:
            H[b] = alpha[0]
        elif kind == 2:
            H[b] = rng.choice(alpha, size=m)
            H[b, 4::5] = V - 2
        else:
            H[b] = np.resize(np.array(phrase32), m)
    return H


def run_kernel(lib, logits_buf, first, stride, batch, V, tokens, ld, cur_len, sample_begin, eot, dev_table, done=None, counter=False,
               capacity=None, pool_capacity=None, use_count=True, items_ptr=None, pool_ptr=None, sm=None):
    items, pool, count = dev_table
    io = native.WmBiasIO()
    io.logits, io.row_stride = logits_buf.data_ptr() + 2 * first, stride
    io.batch, io.n_vocab = batch, V
    io.tokens, io.tokens_ld = tokens.data_ptr(), ld
    keep = None
    if counter:
        keep = torch.tensor([cur_len - 1], dtype=torch.int32, device="cuda")
        io.cur_len, io.n_past_dev = 0, keep.data_ptr()
    else:
        io.cur_len = cur_len
    io.sample_begin, io.eot = sample_begin, eot
    io.done = done.data_ptr() if done is not None else None
    io.items = items.data_ptr() if items_ptr is None else items_ptr
    io.pool = pool.data_ptr() if pool_ptr is None else pool_ptr
    io.capacity = items.numel() // 4 if capacity is None else capacity
    io.pool_capacity = pool.numel() if pool_capacity is None else pool_capacity
    io.n_items_dev = count.data_ptr() if use_count else None
    rc = lib.wm_sequence_bias(C.byref(io), stream() if sm is None else sm)
    torch.cuda.synchronize()
    return rc


def upload(table, capacity=None, pool_capacity=None):
    """(items, pool, count) on the device: the table at the front of buffers of the given capacities (default: exactly the table's)."""
    n, n_pool = len(table), table.pool.size
    items = torch.zeros(4 * max(capacity or n, 1), dtype=torch.int32, device="cuda")
    pool = torch.zeros(max(pool_capacity or n_pool, 1), dtype=torch.int32, device="cuda")
    if n:
        items[:4 * n] = torch.from_numpy(table.packed.view(np.int32).reshape(-1).copy()).cuda()
    if n_pool:
        pool[:n_pool] = torch.from_numpy(table.pool.copy()).cuda()
    return items, pool, torch.tensor([n], dtype=torch.int32, device="cuda")


def kernel_case(rng, V, pad, batch, m, table, phrase32, special_tokens):
    """One case on the host: the buffer handed to the kernel (sentinels around the rows and in their padding), the buffer wanted, the
    token rows and the `done` flags."""
    eot = 1000 if V == 1024 else 50257
    stride = V + pad
    cur_len = SAMPLE_BEGIN + m
    H = histories(rng, batch, m, eot, V, phrase32)
    tokens = np.full((batch, LD), 1, dtype=np.int64)                  # alphabet token 1 everywhere else: before sample_begin, behind cur_len
    tokens[:, SAMPLE_BEGIN:cur_len] = H
    logits = (rng.standard_normal((batch, V)) * 4).astype(np.float16)
    for b in range(batch):                                            # zeros, a subnormal, values near +-65504, -inf on the targets
        for i, t in enumerate(special_tokens):
            logits[b, t] = np.float16(SPECIAL[(i + b) % len(SPECIAL)])
    done = (rng.random(batch) < 0.3).astype(np.int32) if batch > 1 else np.zeros(1, dtype=np.int32)
    want_rows = bias_batch(logits, tokens, SAMPLE_BEGIN, cur_len, eot, table.items, done=done)
    buf = np.full(FIRST + GUARD + batch * stride + GUARD, SENTINEL, dtype=np.uint16)
    want = buf.copy()
    for b in range(batch):
        lo = FIRST + GUARD + b * stride
        buf[lo:lo + V] = logits[b].view(np.uint16)
        want[lo:lo + V] = want_rows[b].view(np.uint16)
    changed = int((want != buf).sum())
    return buf, want, tokens.astype(np.int32), done, eot, cur_len, changed


def check_case(lib, V, pad, batch, m, table, dev_table, rng, phrase32, counter, **kw):
    alpha = alphabet_of(1000 if V == 1024 else 50257)
    buf, want, tokens, done, eot, cur_len, changed = kernel_case(rng, V, pad, batch, m, table, phrase32, list(alpha) + list(phrase32[:6]))
    dev = torch.from_numpy(buf.view(np.int16)).cuda()
    tok_dev = torch.from_numpy(tokens).cuda()
    rc = run_kernel(lib, dev, FIRST + GUARD, V + pad, batch, V, tok_dev, LD, cur_len, SAMPLE_BEGIN, eot, dev_table,
                    done=torch.from_numpy(done).cuda(), counter=counter, **kw)
    assert rc == 0, lib.wm_last_error().decode()
    got = dev.cpu().numpy().view(np.uint16)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (V, pad, batch, m, len(table), counter, bad[:8], got[bad[:8]], want[bad[:8]])
    assert np.array_equal(tok_dev.cpu().numpy(), tokens)
    return changed


LENGTHS = [0, 1, 31, 32, 511, 512]
SIZES = [1, 255, 256, 257, 4096]


@pytest.mark.parametrize("batch", [1, 3, 70])
@pytest.mark.parametrize("V,pad", [(1024, 0), (1024, 37), (51865, 11)])
def test_kernel_equals_the_brute_force_bit_for_bit(lib, V, pad, batch):
    """Sentinel guard bands in front of the logits, behind them and in every row's padding; rows at odd 2-byte offsets (stride V + pad,
    a first row 3 elements into the buffer); the start sequence and the slots behind cur_len hold an alphabet token that must not count;
    every history length through a host cur_len AND through the device counter; `done` rows untouched; the table sizes rotate over the
    cases (tests below pin each size); the tables hold a phrase of 32 tokens, a phrase of one, (a, a, a, a), two phrases that share a
    prefix and two that share a target."""
    rng = np.random.default_rng(V + 7 * pad + batch)
    eot = 1000 if V == 1024 else 50257
    alpha = alphabet_of(eot)
    a = int(alpha[0])
    phrase32 = tuple(int(t) for t in rng.permutation(eot - 10)[:32] + 4)
    hot = (phrase32, (int(alpha[1]),), (a, a, a, a), (int(alpha[2]), int(alpha[3]), int(alpha[4])), (int(alpha[2]), int(alpha[3]), int(alpha[5])),
           (int(alpha[4]), int(alpha[1]), int(alpha[5])))
    changed = 0
    for i, m in enumerate(LENGTHS):
        table = make_table(rng, max(SIZES[(i + batch) % len(SIZES)], 64), eot, hot)
        dev_table = upload(table)
        for counter in (False, True):
            changed += check_case(lib, V, pad, batch, m, table, dev_table, rng, phrase32, counter)
    assert changed > 6 * batch, "the cases exercise nothing"


@pytest.mark.parametrize("n", SIZES)
def test_table_sizes_at_the_workgroup_stride(lib, n):
    """1, 255, 256, 257 and 4096 items (256 threads stride over them), in buffers of exactly that capacity and in buffers of the largest
    capacity with the count read from the device word; without the word all `capacity` items count."""
    V, eot = 1024, 1000
    rng = np.random.default_rng(n)
    phrase32 = tuple(range(100, 132))
    table = make_table(rng, n, eot, ((1,),) if n == 1 else ((1, 1, 1, 1), (2, 3)))
    changed = 0
    for m in (0, 40):
        changed += check_case(lib, V, 5, 3, m, table, upload(table), rng, phrase32, counter=False)
        changed += check_case(lib, V, 5, 3, m, table, upload(table), rng, phrase32, counter=True, use_count=False)
        changed += check_case(lib, V, 5, 3, m, table, upload(table, BI.MAX_ITEMS, BI.MAX_POOL), rng, phrase32, counter=True)
    assert changed, "the cases exercise nothing"


def test_one_bias_not_four_and_shared_prefixes_and_targets(lib):
    V, eot, ld = 1024, 1000, 64
    a = 7
    table = BI.build_table(hotwords=((a, a, a, a), (20, 21, 22), (20, 21, 23), (30, 31, 22)), sequence_bias=(((40, 41), -6.0),), eot=eot)
    dev_table = upload(table)
    rows = [[a] * 9, [a], [], [5, 20, 21], [30, 31], [40], [20, 50400, 21]]
    tokens = torch.zeros((len(rows), ld), dtype=torch.int32, device="cuda")
    want = np.full((len(rows), V), 2.0, dtype=np.float16)
    want[:, [a, 20, 30]] = 3.5                                   # the start bias of every phrase, at every step
    want[0, a] = want[1, a] = 5.0                                # (a, a, a, a): the items of k = 3, 2, 1 and 0 match -- one bias of 3.0
    want[3, [22, 23]] = 5.0                                      # a shared prefix, two targets
    want[4, 22] = 5.0                                            # the same target through another prefix
    want[5, 41] = -4.0                                           # a negative sequence bias
    logits = torch.full((len(rows), V), 2.0, dtype=torch.float16, device="cuda")
    for b, r in enumerate(rows):                                 # rows of different lengths: a launch each
        tokens[b, 3:3 + len(r)] = torch.tensor(r, dtype=torch.int32)
        assert run_kernel(lib, logits, b * V, V, 1, V, tokens[b:b + 1], ld, 3 + len(r), 3, eot, dev_table) == 0
    got = logits.cpu().numpy()
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), np.nonzero(got != want)
    assert got[6, 21] == 2.0 and got[3, 21] == 2.0               # a timestamp between two words breaks the phrase; 21 follows 20 only directly


def test_kernel_refusals(lib):
    V, eot, ld = 1024, 1000, 700
    logits = torch.full((1, V), 1.0, dtype=torch.float16, device="cuda")
    tokens = torch.zeros((1, ld), dtype=torch.int32, device="cuda")
    table = BI.build_table(hotwords=((0,),), hotword_start_bias=0.0, eot=eot)       # (a bias of zero: the calls that are taken change nothing)
    dev_table = upload(table, 8, 8)
    big = torch.zeros(4 * 4100, dtype=torch.int32, device="cuda")

    def call(**kw):
        a = dict(logits_buf=logits, first=0, stride=V, batch=1, V=V, tokens=tokens, ld=ld, cur_len=10, sample_begin=3, eot=eot, dev_table=dev_table)
        a.update(kw)
        return run_kernel(lib, **a)

    before = logits.clone()
    assert call() == 0 and call(cur_len=3 + BOUND) == 0                                        # m = the bound: taken
    assert call(counter=True, ld=3 + BOUND) == 0                                               # a device counter: tokens_ld bounds m
    assert call(capacity=0, items_ptr=0, pool_ptr=0) == 0                                      # an empty table: taken, nothing launched
    for bad in (dict(cur_len=3 + BOUND + 1), dict(counter=True), dict(cur_len=2), dict(cur_len=ld + 1), dict(eot=V + 1), dict(eot=-1),
                dict(batch=0), dict(V=0), dict(sample_begin=-1), dict(sample_begin=ld + 1), dict(items_ptr=0), dict(pool_ptr=0),
                dict(capacity=BI.MAX_ITEMS + 1, dev_table=(big, dev_table[1], dev_table[2])), dict(capacity=-1),
                dict(pool_capacity=BI.MAX_POOL + 1), dict(pool_capacity=-1), dict(items_ptr=dev_table[0].data_ptr() + 4),
                dict(pool_ptr=dev_table[1].data_ptr() + 2), dict(batch=2, stride=V - 1)):
        assert call(**bad) == 1, bad
        assert "wm_sequence_bias" in lib.wm_last_error().decode(), bad
    io = native.WmBiasIO()
    assert lib.wm_sequence_bias(None, stream()) == 1 and "null" in lib.wm_last_error().decode()
    assert lib.wm_sequence_bias(C.byref(io), stream()) == 1 and "null" in lib.wm_last_error().decode()
    io.logits, io.batch, io.n_vocab = logits.data_ptr(), 1, V
    assert lib.wm_sequence_bias(C.byref(io), stream()) == 1 and "null" in lib.wm_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(logits.view(torch.int16), before.view(torch.int16))                     # refused: nothing was launched


def test_a_table_the_builder_did_not_make_stays_inside_its_arrays(lib):
    """Unsorted items, k outside [0, 31] and above the history, prefix offsets outside the pool, targets outside [0, eot), a count word
    above the capacity: such items are inert.  The guard elements, the tokens >= eot and every row's padding keep their bits, and the
    items that are well formed still apply (targets that occur once: the only unspecified thing on such a table is which item wins)."""
    V, eot, pad, batch, m = 1024, 1000, 9, 3, 20
    cap, pool_cap = 16, 8
    raw = [(5, 0, 0, 1.0), (-1, 0, 0, 9.0), (eot, 0, 0, 9.0), (V + 50, 0, 0, 9.0), (2 ** 31 - 1, 0, 0, 9.0), (6, -1, 0, 9.0), (7, 32, 0, 9.0),
           (8, 21, 0, 9.0), (9, 2, 7, 9.0), (10, 1, -1, 9.0), (11, 1, 2 ** 31 - 1, 9.0), (12, 31, 2 ** 31 - 20, 9.0), (3, 1, 0, 2.0),
           (-2 ** 31, -2 ** 31, -2 ** 31, 9.0), (4, 0, 8, -1.0), (13, 1, 8, 9.0)]
    packed = np.zeros(cap, dtype=BI.ITEM_DTYPE)
    for i, r in enumerate(raw):
        packed[i] = r
    items = torch.from_numpy(packed.view(np.int32).reshape(-1).copy()).cuda()
    pool = torch.full((pool_cap,), 2, dtype=torch.int32, device="cuda")                         # every prefix inside the pool reads 2s
    stride = V + pad
    buf = np.full(GUARD + batch * stride + GUARD, SENTINEL, dtype=np.uint16)
    one = np.float16(1.0).view(np.uint16)
    for b in range(batch):
        buf[GUARD + b * stride: GUARD + b * stride + V] = one
    want = buf.copy()
    for b in range(batch):
        lo = GUARD + b * stride
        want[lo + 5] = np.float16(2.0).view(np.uint16)             # (5, k = 0)
        want[lo + 3] = np.float16(3.0).view(np.uint16)             # (3, k = 1, prefix pool[0] = 2 = the last token of H)
        want[lo + 4] = np.float16(0.0).view(np.uint16)             # (4, k = 0, offset = pool_capacity: no token is read)
    tokens = torch.full((batch, LD), 2, dtype=torch.int32, device="cuda")
    for count in (len(raw), 2 ** 31 - 1, -5):
        dev = torch.from_numpy(buf.view(np.int16)).cuda()
        table = (items, pool, torch.tensor([count], dtype=torch.int32, device="cuda"))
        assert run_kernel(lib, dev, GUARD, stride, batch, V, tokens, LD, SAMPLE_BEGIN + m, SAMPLE_BEGIN, eot, table) == 0
        got = dev.cpu().numpy().view(np.uint16)
        assert np.array_equal(got, want if count > 0 else buf), (count, np.nonzero(got != want)[0][:8])


def test_a_replayed_launch_follows_a_table_rewritten_in_place(lib):
    V, eot, batch, m = 1024, 1000, 3, 12
    rng = np.random.default_rng(9)
    first, second = make_table(rng, 40, eot, ((1, 2, 3),)), make_table(rng, 300, eot, ((3, 2), (1,)))
    items, pool, count = upload(first, BI.MAX_ITEMS, BI.MAX_POOL)
    H = rng.choice(alphabet_of(eot), size=(batch, m))
    tokens = np.full((batch, LD), 1, dtype=np.int64)
    tokens[:, SAMPLE_BEGIN:SAMPLE_BEGIN + m] = H
    logits0 = (rng.standard_normal((batch, V)) * 4).astype(np.float16)
    tok_dev, src = torch.from_numpy(tokens.astype(np.int32)).cuda(), torch.from_numpy(logits0).cuda()
    logits = src.clone()
    counter = torch.tensor([SAMPLE_BEGIN + m - 1], dtype=torch.int32, device="cuda")
    io = native.WmBiasIO()
    io.logits, io.row_stride, io.batch, io.n_vocab = logits.data_ptr(), V, batch, V
    io.tokens, io.tokens_ld, io.n_past_dev, io.sample_begin, io.eot = tok_dev.data_ptr(), LD, counter.data_ptr(), SAMPLE_BEGIN, eot
    io.items, io.pool, io.n_items_dev, io.capacity, io.pool_capacity = items.data_ptr(), pool.data_ptr(), count.data_ptr(), BI.MAX_ITEMS, BI.MAX_POOL
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # issued eagerly once, then captured
        assert lib.wm_sequence_bias(C.byref(io), side.cuda_stream) == 0
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with native.CAPTURE_LOCK, torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        assert lib.wm_sequence_bias(C.byref(io), torch.cuda.current_stream().cuda_stream) == 0
    wants = [bias_batch(logits0, tokens, SAMPLE_BEGIN, SAMPLE_BEGIN + m, eot, t.items) for t in (first, second)]
    assert not np.array_equal(wants[0].view(np.uint16), wants[1].view(np.uint16))
    for table, want in ((first, wants[0]), (second, wants[1]), (first, wants[0])):
        new = upload(table, BI.MAX_ITEMS, BI.MAX_POOL)
        items.copy_(new[0]), pool.copy_(new[1]), count.copy_(new[2])                            # in place: the graph keeps its pointers
        logits.copy_(src)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(logits.cpu().numpy().view(np.uint16), want.view(np.uint16)), len(table)


# ------------------------------------------------------------------------------------------------------------ the engine loops
@pytest.fixture(scope="module")
def stock(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    eng = build_engine(str(tmp_path_factory.mktemp("bias_engines")), "micro-fullvocab", MODEL_SEED)
    enc = WhisperEncoding(eng)
    xa = enc.get_audio_features(synthetic_mel(3, W, DIMS.n_mels, MEL_SEED).cuda())
    base = WhisperDecoding(eng, options=DecodingOptions(sample_len=24, language="en"))
    t_off, _, _ = base.main_loop(xa)
    base._state.clear()
    return eng, enc, xa, t_off.cpu()


@pytest.mark.parametrize("repeat", [False, True])
def test_device_loop_equals_the_literal_loop_and_its_three_phases_agree(stock, repeat):
    """With the repetition controls on as well: penalty and bans, then the bias, then Whisper's rules -- in both loops."""
    eng, enc, xa, t_off = stock
    controls = dict(repetition_penalty=1.2, no_repeat_ngram_size=2) if repeat else {}
    dec = WhisperDecoding(eng, options=DecodingOptions(sample_len=24, language="en", hotwords=HOTWORDS, **controls))
    t_fast, lp_fast, nsp_fast = dec.main_loop(xa)
    assert set(dec._state[3]['graphs']) == LOOP_CASES["one_group"]["keys"]                  # the options change no graph key
    t_ref, lp_ref, nsp_ref = dec.main_loop_reference(xa)
    assert torch.equal(t_fast.cpu(), t_ref.cpu())
    assert torch.allclose(lp_fast.cpu(), lp_ref.cpu(), atol=2e-3)
    assert np.allclose(nsp_fast, nsp_ref, atol=1e-4)
    assert not torch.equal(t_off, t_fast.cpu()), "the bias changed nothing: the comparison shows nothing"
    runs = []
    for phase, use_graphs in (("eager + capture", True), ("replay", True), ("no graphs", False)):
        dec.use_graphs = use_graphs
        t, lp, _ = dec.main_loop(xa, ignore_eot=True)
        torch.cuda.synchronize()
        runs.append((phase, t.cpu(), lp.cpu(), [c.clone() for c in dec._state[3]['kv']]))
    _, t0, lp0, kv0 = runs[0]
    assert t0.shape == (3, dec.sample_begin + 24)
    for phase, t, lp, kv in runs[1:]:
        assert torch.equal(t, t0) and torch.equal(lp, lp0), phase
        for layer, (a, b) in enumerate(zip(kv, kv0)):
            assert torch.equal(a, b), (phase, layer)
    dec._state.clear()


def first_text(row, eot):
    return next(i for i, t in enumerate(row) if t < eot)


def test_forced_continuation_and_set_bias_under_replayed_graphs(stock):
    """sequence_bias = (((a, b), 1000),): b follows the first a -- deterministic by construction -- and nothing before it moves.  Then
    set_bias with a table of another length between calls: the SAME captured graphs are replayed and follow the new table."""
    eng, enc, xa, t_off = stock
    probe = WhisperDecoding(eng, options=DecodingOptions(sample_len=24, language="en"))
    eot, L0 = probe.tokenizer.eot, probe.sample_begin
    rows = [r[L0:].tolist() for r in t_off]
    a = rows[0][first_text(rows[0], eot)]
    barred = set(probe._get_suppress_tokens()) | set(probe.tokenizer.blank_tokens()) | {t for r in rows for t in r}
    b, c = [t for t in range(1000, 1100) if t not in barred][:2]

    def check(tokens, follow):
        """Every row that holds a: identical to the unbiased row up to and including the first a, then `follow`."""
        hit = 0
        for r, r_off in zip(tokens, rows):
            r = r[L0:].tolist()
            if a not in r_off or r_off.index(a) + len(follow) >= len(r_off):
                continue
            i = r_off.index(a)
            assert r[:i + 1] == r_off[:i + 1], (r, r_off)
            assert r[i + 1:i + 1 + len(follow)] == list(follow), (r, follow)
            assert r_off[i + 1] != follow[0]                      # (the unbiased run does not have it there: b and c were never sampled)
            hit += 1
        assert hit >= 1 and a in rows[0]

    dec = WhisperDecoding(eng, options=DecodingOptions(sample_len=24, language="en", sequence_bias=(((a, b), 1000.0),)))
    t1, _, _ = dec.main_loop(xa)                                  # eager + capture
    check(t1.cpu(), (b,))
    graphs = dict(dec._state[3]['graphs'])
    t2, _, _ = dec.main_loop(xa)                                  # replay
    assert torch.equal(t1.cpu(), t2.cpu())
    dec.set_bias(sequence_bias=(((a, c), 1000.0), ((a, c, b), 1000.0), ((c, b, b), 1000.0)))
    t3, lp3, nsp3 = dec.main_loop(xa)
    assert all(dec._state[3]['graphs'][k] is g for k, g in graphs.items()) and set(dec._state[3]['graphs']) == set(graphs)
    check(t3.cpu(), (c, b, b))
    t_ref, lp_ref, _ = dec.main_loop_reference(xa)                # the literal loop follows set_bias too
    assert torch.equal(t3.cpu(), t_ref.cpu()) and torch.allclose(lp3.cpu(), lp_ref.cpu(), atol=2e-3)
    dec.set_bias()                                                # an empty table: the launch stays, nothing is biased
    t4, _, _ = dec.main_loop(xa)
    assert torch.equal(t4.cpu(), t_off)
    dec.set_bias(hotwords=((a, b),), hotword_bias=1000.0, hotword_start_bias=0.0)
    t5, _, _ = dec.main_loop(xa)
    check(t5.cpu(), (b,))
    with pytest.raises(ValueError, match="built with"):
        probe.set_bias(hotwords=((a, b),))
    dec._state.clear()


@pytest.mark.parametrize("shared", [False, True])
def test_beam_loop_with_hotwords_equals_the_literal_loop(engines, shared):
    K = 3
    eng = engines["fp16"]
    enc = WhisperEncoding(eng)
    xa = enc.get_audio_features(engines["mel"][:3].cuda())
    plain = WhisperDecoding(eng, options=DecodingOptions(beam_size=K, sample_len=24))
    languages, _ = plain.detect_language(xa)
    t, lp, _ = plain.main_loop(xa)
    unbiased = BM.candidates(plain, t, lp)[0]
    plain._state.clear()
    # hotwords made of tokens the peaked model proposes (its unbiased candidates hold 6552, 34532, 43215 and 46939).  Its logits have a
    # standard deviation of 16: biases the size of the defaults would never show.  On the CPU torch path these change every candidate
    hot = [(34532, 6552), (6552, 34532, 43215)]
    opts = DecodingOptions(beam_size=K, sample_len=24, hotwords=tuple(hot), hotword_bias=48.0, hotword_start_bias=24.0)
    dec = WhisperDecoding(eng, options=opts, shared_cross_kv=shared)
    dec.detect_language(xa)
    out = []
    for _ in range(2):                                           # eager, then the replayed graphs
        t, lp, nsp = dec.main_loop(xa)
        out.append((BM.candidates(dec, t, lp), dec.post_process(t, lp, nsp, xa, languages), nsp))
    lit = dec if not shared else WhisperDecoding(eng, options=opts)
    if shared:
        lit.detect_language(xa)
    t, lp, nsp = lit.main_loop_reference(xa)
    ref = (BM.candidates(lit, t, lp), lit.post_process(t, lp, nsp, xa, languages), nsp)
    for got in out:
        BM.assert_same_candidates(got, ref)
    assert ref[0][0] != unbiased, "the hotwords changed no candidate: the comparison shows nothing"
    dec._state.clear()
    lit._state.clear()


def test_long_form_with_hotwords_equals_the_literal_schedule(stock):
    """transcribe_mel over two short files with hotwords on: the segments are those of longform.transcribe_reference replayed on the
    recorded decoder results, and every temperature-0 call again through the public path gives the same tokens."""
    eng, enc, _, _ = stock
    contents = [100, 300]
    mels = [synthetic_mel(1, c + W, DIMS.n_mels, 900 + i)[0].cuda().contiguous() for i, c in enumerate(contents)]
    dec = WhisperDecoding(eng, options=DecodingOptions(language="en", hotwords=HOTWORDS))
    dec.sample_len = 12
    calls = []
    real = dec._sequence_bias
    dec._sequence_bias = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    trace = []
    kw = dict(temperatures=(0.0, 0.4), compression_ratio_threshold=None, logprob_threshold=-1.0, no_speech_threshold=None)
    results = T.transcribe_mel(enc, dec, mels, contents, n_rows=2, trace=trace, **kw)
    assert calls and len(results) == 2 and all(r["segments"] for r in results)
    tk = dec.tokenizer
    recorded = {}
    for e in trace:
        for r, live, res in zip(e["rows"], e["live"], e["results"]):
            if live:
                recorded[(r[0], r[1], e["temperature"])] = res
    for f, c in enumerate(contents):
        want = LF.transcribe_reference(lambda seek, temperature, f=f: recorded[(f, seek, temperature)], c, window=W,
                                       timestamp_begin=tk.timestamp_begin, decode_text=tk.decode, **kw)
        assert results[f]["segments"] == want, f
    n_zero = 0
    for e in trace:
        if e["temperature"] != 0.0:
            continue
        n_zero += 1
        xa = enc.get_audio_features(e["windows"].cuda())
        if e["language_tokens"] is not None:
            dec.set_language_tokens(e["language_tokens"])
        tokens, sums, nsp = dec.main_loop(xa, row_limit=e["row_limit"])
        again = dec.post_process(tokens, sums, nsp, xa, e["languages"])
        for i, live in enumerate(e["live"]):
            assert again[i].tokens == (e["results"][i].tokens if live else []), (e["round"], i)
    assert n_zero >= 2
    dec._state.clear()


def test_defaults_never_reach_the_entry_and_the_partitioned_schedule_refuses(stock, monkeypatch):
    eng, enc, xa, t_off = stock
    lib = native.load_library()

    def boom(*a, **k):
        raise AssertionError("wm_sequence_bias called with the options off")
    monkeypatch.setattr(lib, "wm_sequence_bias", boom)
    xa2 = enc.get_audio_features(synthetic_mel(2, W, DIMS.n_mels, 41).cuda())
    for case in ("one_group", "beam"):
        dec = WhisperDecoding(eng, options=DecodingOptions(sample_len=6, language="en", **LOOP_CASES[case]["options"]))
        assert not dec.bias_on and dec._bias_dev is None
        for _ in range(2):
            dec.main_loop(xa2)
        assert set(dec._state[2 * dec.n_group]['graphs']) == LOOP_CASES[case]["keys"] and dec._bias_dev is None
        dec._state.clear()
    on = WhisperDecoding(eng, options=DecodingOptions(sample_len=6, language="en", hotwords=HOTWORDS))
    on.cu_partition = True
    with pytest.raises(ValueError, match="cu_partition"):
        on.main_loop(xa2)
    on.cu_partition = False
    with pytest.raises(AssertionError, match="options off"):       # (the patch does catch a call)
        on.main_loop(xa2)
    torch.cuda.synchronize()
    on._state.clear()
