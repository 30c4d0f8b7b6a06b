"""Cases and references for the token-step kernels at the edges of the allowed token ranges (csrc/greedy.hip, csrc/beam.hip,
csrc/truncate.hip over csrc/logit_rules.h)  --  TEST INFRASTRUCTURE, CPU only.  tests/test_rule_edges_cpu.py checks this module
against itself and the oracle; tests/test_gpu_rule_edges.py runs its cases through the kernels.

What the cases are about: the kernels reduce Whisper's rules to "suppress lists -> -inf, allowed = [lo_txt, hi_txt) U [lo_ts, hi_ts),
timestamps win if their mass beats the best text token", and scan a 2-byte-aligned row as a scalar head up to a 16-byte boundary,
an 8-wide body and a scalar tail.  A bound off by one, an element lost at a seam or a chunk sent down the wrong path moves one
token in or out of the allowed set -- which random logits notice about once in a thousand rows and by 1e-5 in the booked sum.  Here
every row PLANTS its winner (or a trap) on such a token.

EDGE TOKENS come from the oracle (oracle/decoding_rules.apply_filters, pinned to the reference's classes by the golden), never from
a restatement of the kernel's ranges: both sides of every transition of the allowed mask under empty suppress lists, the fixed
tokens 0, eot-1, eot, tb-1, tb, V-1, and the first and last finite token of each class under the full lists.

REFERENCES
  oracle_step      DR.apply_filters + DR.greedy_update (fp32, the reference's arithmetic) and a float64 log-softmax of the same
                   masked row: the token, and the value the GPU's booked sum is bounded against;
  range_eval       "lists -> -inf, two ranges, dominance, arg-max, log Z" in float64.  Used ONLY to judge whether the cases could
                   tell a kernel with a bound off by one (range mutants) or an element lost at a seam (seam mutants) from a right one.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import decoding_rules as DR

SAMPLE_BEGIN = 3
MAX_INITIAL = 50
SUM_TOL = 2e-4                 # the bound of tests/test_gpu_kernels.py::test_greedy_step_* on one step's booked log-probability
DOMINANCE_MIN = 0.05           # the project's near-tie threshold of the timestamp-dominance rule (tests/test_gpu_kernels.py, NpBeam)
WINNER_GAP_MIN = 4.0           # every planted winner leads the runner-up by at least this much
T_SAMPLE = 0.01                # the temperature of the sampled edge cases

VOCABS: Dict[str, DR.SpecialIds] = {
    "multilingual": DR.SpecialIds(50257),            # V = 51 865
    "gpt2": DR.SpecialIds(50256),                    # V = 51 864 (the .en models)
    "v3": DR.SpecialIds(50257, n_langs=100),         # V = 51 866 (large-v3)
}


def suppressed_specials(ids: DR.SpecialIds) -> List[int]:
    """The specials upstream's _get_suppress_tokens adds to every list, and <|notimestamps|> (SuppressTokens' companion when
    timestamps are on: the kernels take it from the list, the oracle's ApplyTimestampRules masks it itself)."""
    return [ids.sot, ids.translate, ids.transcribe, ids.sot_lm, ids.sot_prev, ids.no_speech, ids.no_timestamps]


def lists_for(name: str, golden_dir: Optional[str] = None) -> Tuple[List[int], List[int]]:
    """(suppress, blank) of a vocabulary: the golden's lists for the multilingual one, lists built from the ids for the others --
    the specials, a few dozen scattered text ids (the neighbours of the two ends of the text range among them, the ends themselves
    stay allowed: a suppressed end would make the bound beside it untestable) and blank = [220, eot]."""
    ids = VOCABS[name]
    if name == "multilingual":
        golden_dir = golden_dir or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        fix = np.load(os.path.join(golden_dir, "decoding_rules.npz"))
        return sorted(set(fix["suppress"].tolist() + [ids.no_timestamps])), fix["blank"].tolist()
    r = np.random.Generator(np.random.Philox(len(name)))
    text = set(r.choice(ids.n_base, size=40, replace=False).tolist()) | {1, 2, 9, ids.n_base - 2}
    return sorted(text | set(suppressed_specials(ids))), [220, ids.eot]


def rule_set(name: str, apply_rules: int, suppress: Sequence[int], blank: Sequence[int]) -> DR.RuleSet:
    return DR.RuleSet(VOCABS[name], SAMPLE_BEGIN, list(suppress), list(blank), MAX_INITIAL, timestamps=apply_rules == 1)


@dataclass(frozen=True)
class State:
    name: str
    hist: Tuple[int, ...]          # the sampled tokens so far
    apply_rules: int = 1


def states(ids: DR.SpecialIds) -> List[State]:
    tb = ids.timestamp_begin
    a, b = (tb + 3, 400, tb + 40), (tb + 3, 7, tb + 1500)
    hists = [
        ("first", ()), ("ts", (tb + 3,)), ("ts_txt", (tb + 3, 400)), ("ts_txt_ts", a), ("pair", a + (tb + 40,)),
        ("pair_txt", a + (tb + 40, 321)), ("ts0", (tb,)), ("ts_txt_last", b), ("last_pair", b + (tb + 1500,)),
        ("last_pair_txt", b + (tb + 1500, 9)), ("ts0_txt_txt", (tb, 5, 6)),
    ]
    return [State(n, h) for n, h in hists] + [State("lists_only", (tb + 3, 400), 2), State("plain", (400, 500), 0)]


def context(ids: DR.SpecialIds, st: State) -> np.ndarray:
    return np.array([ids.sot, ids.lang0, ids.transcribe] + list(st.hist), dtype=np.int64)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def oracle_filter(rows: np.ndarray, name: str, st: State, suppress, blank, dominance_out=None) -> np.ndarray:
    """DR.apply_filters on every row of `rows` [B, V] under the state's history (apply_rules = 0: nothing is filtered)."""
    if st.apply_rules == 0:
        if dominance_out is not None:
            dominance_out += [np.inf] * len(rows)
        return rows.astype(np.float32).copy()
    toks = np.repeat(context(VOCABS[name], st)[None], len(rows), axis=0)
    dom = []
    out = DR.apply_filters(rows, toks, rule_set(name, st.apply_rules, suppress, blank), dominance_out=dom)
    if dominance_out is not None:
        dominance_out += dom if dom else [np.inf] * len(rows)
    return out


def log_softmax_f64(masked: np.ndarray) -> np.ndarray:
    x = masked.astype(np.float64)
    m = x.max(axis=-1, keepdims=True)
    with np.errstate(divide="ignore"):
        return (x - m) - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def oracle_step(rows: np.ndarray, name: str, st: State, suppress, blank):
    """(token, fp32 sum of the oracle, float64 sum, dominance, masked rows) for one greedy step from sum_logprobs = 0."""
    ids = VOCABS[name]
    dom: list = []
    masked = oracle_filter(rows, name, st, suppress, blank, dom)
    sums = np.zeros(len(rows), dtype=np.float32)
    toks = np.repeat(context(ids, st)[None], len(rows), axis=0)
    out, _ = DR.greedy_update(toks, masked, sums, ids.eot)
    tok = out[:, -1].astype(np.int64)
    f64 = log_softmax_f64(masked)[np.arange(len(rows)), tok]
    return tok, sums, f64, np.array(dom), masked


def allowed_mask(name: str, st: State, suppress, blank) -> np.ndarray:
    """The allowed set BEFORE the dominance rule, read off the oracle: every text token at 40 and every timestamp at 0, so that the
    best text token beats the whole timestamp mass (log 1501 = 7.3) and the last rule masks nothing that the others left."""
    ids = VOCABS[name]
    x = np.zeros((1, ids.n_vocab), dtype=np.float32)
    x[0, :ids.timestamp_begin] = 40.0
    return np.isfinite(oracle_filter(x, name, st, suppress, blank)[0])


def class_ends(mask: np.ndarray, tb: int) -> List[Tuple[int, int]]:
    """(first, last) allowed token of the text class and of the timestamp class, where the class is not empty."""
    out = []
    for lo, hi in ((0, tb), (tb, len(mask))):
        idx = np.nonzero(mask[lo:hi])[0]
        if idx.size:
            out.append((lo + int(idx[0]), lo + int(idx[-1])))
    return out


def edge_tokens(name: str, st: State, suppress, blank) -> List[int]:
    ids = VOCABS[name]
    V, tb = ids.n_vocab, ids.timestamp_begin
    bare = allowed_mask(name, st, [], [])
    full = allowed_mask(name, st, suppress, blank)
    edges = {0, ids.eot - 1, ids.eot, tb - 1, tb, V - 1}
    for t in np.nonzero(bare[1:] != bare[:-1])[0].tolist():
        edges |= {t, t + 1}
    for first, last in class_ends(full, tb):
        edges |= {first, last}
    return sorted(edges)


# ---- planted rows --------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    kind: str                      # inside | outside | mass | tie | seam
    row: np.ndarray                # [V] fp32, every value fp16-exact
    planted: Tuple[int, ...]       # the tokens the case is about
    sample: bool = True            # also run at temperature T_SAMPLE (ties are for temperature 0 only)
    trap: Optional[int] = None     # outside: the disallowed token that carries 30


def base_row(V: int, seed: int = 11) -> np.ndarray:
    r = np.random.Generator(np.random.Philox(seed))
    return r.standard_normal(V).astype(np.float16).astype(np.float32)


def interior_token(full: np.ndarray, ends: Tuple[int, int], avoid: Sequence[int]) -> int:
    """An allowed token in the middle of the class whose first and last allowed tokens are `ends`, away from every edge."""
    lo, hi = ends
    idx = lo + np.nonzero(full[lo:hi + 1])[0]
    for t in idx[len(idx) // 2:].tolist() + idx[:len(idx) // 2][::-1].tolist():
        if all(abs(t - a) > 1 for a in avoid):
            return int(t)
    raise AssertionError("no interior token")


def planted_cases(name: str, st: State, suppress, blank, base: Optional[np.ndarray] = None) -> List[Case]:
    """The rows of one (vocabulary, state): see the module docstring.  The multiple-of-8 phase of a row does not enter: the GPU test
    replicates every case at all eight."""
    ids = VOCABS[name]
    V, tb = ids.n_vocab, ids.timestamp_begin
    base = base_row(V) if base is None else base
    full = allowed_mask(name, st, suppress, blank)
    edges = edge_tokens(name, st, suppress, blank)
    inner = interior_token(full, max(class_ends(full, tb), key=lambda e: e[1] - e[0]), edges)      # of the larger class
    cases: List[Case] = []
    for t in edges:
        x = base.copy()
        if full[t]:
            x[t] = 20.0
            cases.append(Case("inside", x, (t,)))
        else:
            x[t], x[inner] = 30.0, 12.0
            cases.append(Case("outside", x, (inner,), trap=t))
    for first, last in class_ends(full, tb):
        if first != last:
            x = base.copy()
            x[first], x[last] = 16.0, 15.5
            cases.append(Case("mass", x, (first, last)))
        if last - first >= 8:                          # exact ties inside one class (two classes at 20 would tie the dominance rule)
            inner = interior_token(full, (first, last), edges)
            if first < inner:                          # a class's first token and its interior: the first index wins
                x = base.copy()
                x[first] = x[inner] = 20.0
                cases.append(Case("tie", x, (first, inner), sample=False))
            if inner < last:                           # ... the interior and the class's last token
                x = base.copy()
                x[inner] = x[last] = 20.0
                cases.append(Case("tie", x, (inner, last), sample=False))
    # exact ties across the head/body seam of the row: (h - 1, h) is that seam in the replica whose head is h tokens long
    for h in range(1, 8):
        if full[h - 1] and full[h]:
            x = base.copy()
            x[h - 1] = x[h] = 20.0
            cases.append(Case("seam", x, (h - 1, h), sample=False))
    # ... and across the body/tail seam: with a head of h tokens the body ends at h + 8 * ((V - h) // 8)
    for h in range(8):
        e = h + 8 * ((V - h) // 8)
        if 0 < e < V and full[e - 1] and full[e]:
            x = base.copy()
            x[e - 1] = x[e] = 20.0
            cases.append(Case("seam", x, (e - 1, e), sample=False))
    return cases


# ---- the range evaluator and its mutants (adequacy of the cases, nothing else) ---------------------------------------------------
def true_ranges(name: str, st: State) -> Tuple[int, int, int, int]:
    """[lo_txt, hi_txt) U [lo_ts, hi_ts) as csrc/logit_rules.h states them.  test_rule_edges_cpu holds range_eval over these ranges
    to the oracle on every case, so a slip here cannot hide a slip there."""
    ids = VOCABS[name]
    V, tb, h = ids.n_vocab, ids.timestamp_begin, st.hist
    if st.apply_rules != 1:
        return 0, V, V, V
    lo_txt, hi_txt, lo_ts, hi_ts = 0, tb, tb, V
    last_ts = len(h) >= 1 and h[-1] >= tb
    pen_ts = len(h) < 2 or h[-2] >= tb
    if not h:
        hi_txt, hi_ts = 0, min(V, tb + MAX_INITIAL + 1)
    if last_ts:
        if pen_ts:
            lo_ts = V
        else:
            lo_txt = ids.eot
    stamps = [t for t in h if t >= tb]
    if stamps:
        lo_ts = max(lo_ts, stamps[-1] + (0 if last_ts and not pen_ts else 1))
    return lo_txt, hi_txt, lo_ts, hi_ts


def listed(name: str, st: State, suppress, blank) -> np.ndarray:
    """The tokens the lists write -inf into on this step."""
    m = np.zeros(VOCABS[name].n_vocab, dtype=bool)
    if st.apply_rules:
        m[list(suppress)] = True
        if not st.hist:
            m[list(blank)] = True
    return m


def range_classes(ranges, V: int, dead: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(allowed, is_text) of every token under the kernel's model: n < hi_txt is the text class."""
    lo_txt, hi_txt, lo_ts, hi_ts = ranges
    n = np.arange(V)
    is_text = n < hi_txt
    allowed = np.where(is_text, n >= lo_txt, (n >= lo_ts) & (n < hi_ts)) & ~dead
    return allowed, is_text


def range_eval(row: np.ndarray, ranges, ts_rules: bool, dead: np.ndarray) -> Tuple[int, float]:
    """(token, log-probability) of one row in float64; (-1, -inf) if nothing finite is allowed."""
    allowed, is_text = range_classes(ranges, len(row), dead)
    x = np.where(allowed, row.astype(np.float64), -np.inf)
    txt, ts = np.where(is_text, x, -np.inf), np.where(is_text, -np.inf, x)
    if ts_rules and np.isfinite(ts.max()):
        lse_ts = ts.max() + np.log(np.exp(ts - ts.max()).sum())
        if lse_ts > txt.max():
            x = ts
    if not np.isfinite(x.max()):
        return -1, -np.inf
    tok = int(np.argmax(x))
    return tok, float(x[tok] - (x.max() + np.log(np.exp(x - x.max()).sum())))


def range_mutants(ranges) -> List[Tuple[str, Tuple[int, int, int, int]]]:
    out = []
    for k, nm in enumerate(("lo_txt", "hi_txt", "lo_ts", "hi_ts")):
        for d in (-1, 1):
            m = list(ranges)
            m[k] += d
            out.append((f"{nm}{d:+d}", tuple(m)))
    return out


def mutant_is_equivalent(ranges, mutant, V: int, dead: np.ndarray) -> bool:
    """From the masks alone: the mutant allows the same tokens and puts every one of them in the same class."""
    a0, t0 = range_classes(ranges, V, dead)
    a1, t1 = range_classes(mutant, V, dead)
    return bool(np.array_equal(a0, a1) and np.array_equal(t0[a0], t1[a0]))


# ---- plain arg-max at the seams of the row walk ---------------------------------------------------------------------------------
ARGMAX_SIZES = (1, 5, 8, 9, 16, 17, 1031)


def walk_of(V: int, head: int) -> Tuple[int, int]:
    """(head length, number of 8-wide chunks) of a row whose 16-byte boundary lies `head` tokens in."""
    h = min(V, head)
    return h, (V - h) >> 3


def argmax_rows(V: int, head: int, seed: int = 0) -> np.ndarray:
    """Rows [n, V] for one (size, head length): the winner at 0, head - 1, head, V - 1, and exact ties across the head/body and
    the body/tail seam.  Base values N(0, 1), the planted ones at 9 (fp16-exact)."""
    h, nvec = walk_of(V, head)
    r = np.random.Generator(np.random.Philox(1000 * V + 8 * seed + head))
    singles = sorted({0, max(h - 1, 0), min(h, V - 1), V - 1})
    pairs = sorted({(a, b) for a, b in ((h - 1, h), (h + 8 * nvec - 1, h + 8 * nvec)) if 0 <= a and b < V})
    rows = []
    for planted in [(t,) for t in singles] + pairs:
        x = r.standard_normal(V).astype(np.float16).astype(np.float32)
        x[list(planted)] = 9.0
        rows.append(x)
    return np.stack(rows)


def seam_mutants(V: int, head: int) -> List[Tuple[str, int]]:
    """"One element skipped" at each seam of the walk, where that element exists."""
    h, nvec = walk_of(V, head)
    out = [("V-1", V - 1)]
    if h >= 1:
        out.append(("head-1", h - 1))
    if h < V:
        out.append(("head", h))
    if nvec >= 1:
        out.append(("body_end", h + 8 * nvec - 1))
    return out


def argmax_skipping(row: np.ndarray, skip: Optional[int] = None) -> int:
    x = row.astype(np.float64).copy()
    if skip is not None:
        x[skip] = -np.inf
    return int(np.argmax(x))


# ---- the sampler's noise --------------------------------------------------------------------------------------------------------
def _fmix32(x: np.ndarray) -> np.ndarray:
    M = np.uint64(0xffffffff)
    x = x.astype(np.uint64)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x85ebca6b)) & M
    x ^= x >> np.uint64(13); x = (x * np.uint64(0xc2b2ae35)) & M
    x ^= x >> np.uint64(16)
    return x


def noise_counts(seed: int, row: int, cur_len: int, V: int) -> np.ndarray:
    """The 24-bit integer k that csrc/sample_rng.h turns into u for every token of a row (fmix32 / gumbel_noise restated)."""
    M = np.uint64(0xffffffff)
    lo, hi = seed & 0xffffffff, seed >> 32
    key = _fmix32(np.array([(lo ^ ((row * 0x9e3779b1) & 0xffffffff)) & 0xffffffff], dtype=np.uint64))
    key = _fmix32((key ^ np.uint64(hi) ^ np.uint64((cur_len * 0x85ebca77) & 0xffffffff)) & M)[0]
    n = np.arange(V, dtype=np.uint64)
    h = _fmix32((key ^ ((n * np.uint64(0x27d4eb2f)) & M)) & M)
    h = _fmix32((h + ((np.uint64(0x9e3779b9) * n) & M)) & M)
    return (h >> np.uint64(8)).astype(np.int64)


def noise_u(k: np.ndarray) -> np.ndarray:
    """u of csrc/sample_rng.h from k, in the kernel's fp32 operations (the + 0.5f rounds to even above 2^23)."""
    f = np.asarray(k).astype(np.float32) + np.float32(0.5)
    return np.minimum(f, np.float32(16777215.0)) * np.float32(1.0 / 16777216.0)


def gumbel_range() -> Tuple[float, float]:
    """(smallest, largest) value of g = -log(-log u) over all 2^24 values of k: g is monotone in u and u in k."""
    u = noise_u(np.array([0, (1 << 24) - 1])).astype(np.float64)
    with np.errstate(divide="ignore"):
        g = -np.log(-np.log(u))
    return float(g[0]), float(g[1])


# A draw whose noise is the generator's largest: (seed, global row, cur_len, token) with k = 2^24 - 1, found by search over rows.
# Before the bound in sample_rng.h that k gave u = 1 and g = +inf: the token was drawn whatever its logit.
EXTREME_DRAW = dict(seed=0x5EEDED6E5, row=422, cur_len=5, token=2980)       # test_rule_edges_cpu verifies it


# ---- beam: planted rows and the contract for rows with too few proposals ---------------------------------------------------------
def beam_rows(name: str, st: State, suppress, blank, K: int, n_rows: int, r: np.random.Generator) -> np.ndarray:
    """Rows [n_rows, V] whose K + 1 best allowed tokens are planted inside-edge tokens at 20, 19.25, 18.5, ... -- the first and last
    finite token of each allowed class first, then the other inside edges, then interior tokens -- and whose disallowed edge tokens
    carry 30.  A row is led by text (timestamps interleaved below it: their mass stays under the best text token) or, where the
    timestamp class has K + 1 tokens, by timestamps (the text ends at 19.625 are then masked by the dominance rule)."""
    ids = VOCABS[name]
    V, tb = ids.n_vocab, ids.timestamp_begin
    full = allowed_mask(name, st, suppress, blank)
    edges = edge_tokens(name, st, suppress, blank)
    per_class = {}
    for first, last in class_ends(full, tb):
        own = [t for t in edges if full[t] and first <= t <= last and t not in (first, last)]
        idx = first + np.nonzero(full[first:last + 1])[0]
        pads = [int(t) for t in idx[len(idx) // 3: len(idx) // 3 + 3 * (K + 2): 3] if t not in edges]
        per_class["txt" if first < tb else "ts"] = list(dict.fromkeys([first, last] + own + pads))
    x = np.stack([base_row(V, seed=100 + b) for b in range(n_rows)])
    for b in range(n_rows):
        for t in edges:
            if not full[t]:
                x[b, t] = 30.0
        txt, ts = per_class.get("txt", []), per_class.get("ts", [])
        txt, ts = txt[b % max(len(txt), 1):] + txt[:b % max(len(txt), 1)], ts[b % max(len(ts), 1):] + ts[:b % max(len(ts), 1)]
        off = 0.0625 * int(r.integers(0, 8))
        ts_led = bool(ts) and (not txt or (len(ts) >= K + 1 and (b + int(r.integers(0, 2))) % 2 == 1))
        if ts_led:
            order = ts
            for t in txt[:2]:
                x[b, t] = 19.625 - off
        else:                                          # text on top, the two classes alternating below it
            order = [t for pair in zip(txt, ts + [None] * len(txt)) for t in pair if t is not None]
        for q, t in enumerate(order[:K + 3]):
            x[b, t] = 20.0 - 0.75 * q - off
    return x.astype(np.float16).astype(np.float32)


def scarce_beam_step(ref, logits: np.ndarray, cur: int, rules: DR.RuleSet, dominance_min: float = DOMINANCE_MIN) -> None:
    """One step of the state of tests/test_gpu_beam.NpBeam (`ref`, updated in place) under the WHOLE contract of csrc/beam.hip,
    rows with fewer than beam_size + 1 finite allowed logits included: a row proposes what it has (absent candidates sort last and
    the walk stops at the first one); a beam for which no live candidate is left ends -- it keeps its own history, takes EOT, its
    sum becomes -inf and its parent is its own row.  No row_limit, no ignore_eot.  Records the smallest gap between walked
    candidates in ref.min_gap like NpBeam.step."""
    K, MC, eot = ref.K, ref.MC, rules.ids.eot
    dom: list = []
    filtered = DR.apply_filters(logits, ref.tokens[:, :cur].astype(np.int64), rules, dominance_out=dom)
    with np.errstate(invalid="ignore"):
        lp = DR.log_softmax_f32(filtered)
    first = cur == rules.sample_begin
    old_tokens, old_sums = ref.tokens.copy(), ref.sums.copy()
    for a in range(ref.n_audio):
        r0 = a * K
        ref.parent[r0:r0 + K] = np.arange(r0, r0 + K)
        if ref.done[r0]:
            continue
        cands = []
        for j in range(1 if first else K):
            assert not np.isfinite(dom[r0 + j]) or abs(dom[r0 + j]) > dominance_min, "near-tie of the timestamp-dominance rule"
            idx = np.nonzero(np.isfinite(filtered[r0 + j]))[0]
            props = idx[np.lexsort((idx, -filtered[r0 + j, idx]))][:K + 1]
            cands += [(np.float32(old_sums[r0 + j] + lp[r0 + j, t]), j, int(t)) for t in props]
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        live, fin, walked = [], [], 0
        for c in cands:
            if len(live) == K:
                break
            walked += 1
            (fin if c[2] == eot else live).append(c)
        for c0, c1 in zip(cands[:walked], cands[1:walked + 1]):
            if not (c0[1] == c1[1] and filtered[r0 + c0[1], c0[2]] == filtered[r0 + c1[1], c1[2]]):
                ref.min_gap = min(ref.min_gap, float(c0[0] - c1[0]))
        for i in range(K):
            if i < len(live):
                s, j, t = live[i]
                ref.tokens[r0 + i, :cur] = old_tokens[r0 + j, :cur]
                ref.tokens[r0 + i, cur], ref.sums[r0 + i], ref.parent[r0 + i] = t, s, r0 + j
            else:
                ref.tokens[r0 + i, :cur] = old_tokens[r0 + i, :cur]
                ref.tokens[r0 + i, cur], ref.sums[r0 + i], ref.parent[r0 + i] = eot, -np.inf, r0 + i
                ref.events.add("ended")
        for s, j, t in fin:
            n = ref.fin_count[a]
            if n >= MC:
                break
            ref.fin_tokens[a, n, :cur] = old_tokens[r0 + j, :cur]
            ref.fin_tokens[a, n, cur] = eot
            ref.fin_scores[a, n], ref.fin_len[a, n] = s, cur + 1
            ref.fin_count[a] = n + 1
        if ref.fin_count[a] >= MC:
            ref.done[r0:r0 + K], ref.live_len[a] = 1, cur + 1
            ref.n_done += K
