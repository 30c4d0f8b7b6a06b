"""wm_forced_probs (csrc/forced_probs.hip): the probability a forced pass gives the token that follows, from fp16 logits.

    out[b][p] = exp(x[b][p][min(next[b][p], limit - 1)] - logsumexp_{v < limit} x[b][p][v])

Held to an fp64 numpy restatement on the same fp16 logits.  The bound is max(4 * e_torch, 2^-22), e_torch = the largest
|fp32 PyTorch expression - fp64| of the case -- the expression WhisperDecoding.word_timestamps(token_probs="torch") evaluates on
the GPU (an fp32 copy, gather, logsumexp, exp).  4 x is the project's convention for a reordering of fp32 sums; 2^-22 is two fp32
ulps at 1, for the cases in which PyTorch happens to be exact.  Rows whose logits below the limit are all -inf are NaN in
PyTorch and must be exactly 0 here; they take no part in e_torch.

Shapes: batch 3, n_pos 1 and 4, V in {7, 1003, 51865} with limit = V - 4 (V = 7: three logits, all in the scalar head or tail;
1003: less than one 16-byte piece per lane; 51865: Whisper's vocabulary, the four-loads-in-flight loop and its remainder), a row
stride larger than V, and a base pointer 1 and 3 elements into its buffer, so rows start at every 2-byte offset of a 16-byte line.
Values: N(0, 4); rows holding +-60000; rows with -inf entries; one row all -inf; `next` = 0, limit - 1, limit and V - 1 (the
clamp).  The output lies inside a buffer pre-filled with a sentinel, `next` and `out` have leading dimensions larger than n_pos.

Measured on MI355X (printed by the test): max |device - fp64| 5.1e-09 in every case with n_pos 1 and with V = 1003 / 51865 (the
PyTorch expression: 5.1e-09 .. 5.4e-09), 2.5e-08 .. 8.3e-08 at n_pos 4, V = 7, where probabilities lie near 1/2 (PyTorch: 1.9e-08 ..
5.5e-08); the bound was its floor, 2^-22 = 2.4e-07, everywhere.  Two runs were bit-identical.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_refs as KR  # noqa: E402
import native  # noqa: E402

BATCH = 3
GUARD = 64


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return native.load_library()


def make_case(n_pos, V, pad, offset, seed):
    """(buffer fp16 on the GPU, logits view [BATCH, n_pos, V] with strides, next int32 [BATCH, n_pos], all-(-inf) rows)"""
    rng = KR.philox(seed)
    limit = V - 4
    stride_p = V + pad
    stride_b = n_pos * stride_p + (5 if pad else 0)
    x = (2.0 * rng.standard_normal((BATCH, n_pos, V))).astype(np.float16)
    nxt = rng.integers(0, limit, size=(BATCH, n_pos)).astype(np.int32)
    dead = np.zeros((BATCH, n_pos), dtype=bool)
    # row (0, 0): +-60000 among the noise, the forced token is the +60000 one; row (1, 0): the same row, forced token elsewhere
    for b in (0, 1):
        x[b, 0, :limit:2] = -60000.0
        x[b, 0, limit // 2] = 60000.0
    nxt[0, 0] = limit // 2
    nxt[1, 0] = 0
    # row (2, 0): -inf everywhere below the limit except two entries (a probability near 1/2); finite values behind the limit
    x[2, 0, :limit] = -np.inf
    x[2, 0, 1] = 1.5
    x[2, 0, limit - 1] = 1.25
    nxt[2, 0] = limit - 1
    if n_pos > 1:
        x[0, 1, :limit] = -np.inf                       # all -inf below the limit (behind it: finite, must not be read)
        dead[0, 1] = True
        nxt[0, 1] = 2
        x[1, 1, ::3] = -np.inf                          # scattered -inf, one of them the forced token
        nxt[1, 1] = 0
        nxt[2, 1], nxt[0, 2], nxt[1, 2], nxt[2, 2] = 0, limit - 1, limit, V - 1          # the clamp: limit and V - 1 read limit - 1
        x[2, 3, limit:] = 60000.0                       # huge values behind the limit: not part of the sum
    else:
        nxt[1, 0] = V - 1                               # the clamp on the +-60000 row: reads x[limit - 1]
    total = offset + (BATCH - 1) * stride_b + (n_pos - 1) * stride_p + V
    buf = torch.full((total + 8,), 7.0, dtype=torch.float16, device="cuda")
    view = torch.as_strided(buf, (BATCH, n_pos, V), (stride_b, stride_p, 1), offset)
    view.copy_(torch.from_numpy(x).cuda())
    return buf, view, x, nxt, dead, limit, stride_b, stride_p


def reference64(x, nxt, limit):
    xs = x[:, :, :limit].astype(np.float64)
    m = xs.max(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        lse = m[..., 0] + np.log(np.exp(xs - m).sum(axis=-1))
        idx = np.minimum(nxt, limit - 1)
        out = np.exp(np.take_along_axis(xs, idx[..., None].astype(np.int64), axis=-1)[..., 0] - lse)
    return np.where(np.isneginf(m[..., 0]), 0.0, out)


def parent_expression(view, nxt_dev, limit):
    """decoding.py, token_probs="torch": fp32 on the GPU."""
    lf = view[:, :, :limit].float()
    nxt = nxt_dev.long().clamp(max=limit - 1)
    return (lf.gather(-1, nxt[..., None])[..., 0] - lf.logsumexp(dim=-1)).exp()


def run(lib, view, nxt, n_pos, V, limit, stride_b, stride_p):
    next_ld, out_ld = n_pos + 3, n_pos + 2
    nxt_buf = torch.full((BATCH, next_ld), 10 ** 9, dtype=torch.int32, device="cuda")
    nxt_buf[:, :n_pos] = torch.from_numpy(nxt).cuda()
    out_buf = torch.full((GUARD + BATCH * out_ld + GUARD,), KR.SENTINEL, dtype=torch.float32, device="cuda")
    out = out_buf[GUARD: GUARD + BATCH * out_ld]
    native.check(lib.wm_forced_probs(view.data_ptr(), BATCH, n_pos, V, stride_b, stride_p, limit, nxt_buf.data_ptr(), next_ld,
                                     out.data_ptr(), out_ld, torch.cuda.current_stream().cuda_stream), "wm_forced_probs")
    torch.cuda.synchronize()
    host = out_buf.cpu()
    assert (host[:GUARD] == KR.SENTINEL).all() and (host[GUARD + BATCH * out_ld:] == KR.SENTINEL).all(), "written outside the output"
    grid = host[GUARD: GUARD + BATCH * out_ld].view(BATCH, out_ld)
    assert (grid[:, n_pos:] == KR.SENTINEL).all(), "written between the rows of the output"
    return grid[:, :n_pos].clone(), nxt_buf


@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("pad", [0, 11])
@pytest.mark.parametrize("V", [7, 1003, 51865])
@pytest.mark.parametrize("n_pos", [1, 4])
def test_forced_probs_against_fp64(lib, n_pos, V, pad, offset):
    buf, view, x, nxt, dead, limit, stride_b, stride_p = make_case(n_pos, V, pad, offset, 100000 * n_pos + 10 * V + pad + offset)
    got, nxt_buf = run(lib, view, nxt, n_pos, V, limit, stride_b, stride_p)
    again, _ = run(lib, view, nxt, n_pos, V, limit, stride_b, stride_p)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "two runs differ"
    assert (buf.cpu()[:offset] == 7.0).all(), "the logits were written"
    ref = reference64(x, nxt, limit)
    parent = parent_expression(view, nxt_buf[:, :n_pos], limit).cpu().numpy().astype(np.float64)
    got = got.numpy().astype(np.float64)
    assert np.isfinite(got).all()
    assert (got[dead] == 0.0).all() and (ref[dead] == 0.0).all(), "an all -inf row must give exactly 0"
    assert np.isnan(parent[dead]).all() or not dead.any()            # (what the PyTorch expression makes of such a row)
    live = ~dead
    e_torch = float(np.abs(parent[live] - ref[live]).max())
    e_dev = float(np.abs(got[live] - ref[live]).max())
    bound = max(4 * e_torch, 2.0 ** -22)
    print(f"forced probs n_pos {n_pos} V {V} pad {pad} offset {offset}: max |device - fp64| = {e_dev:.3g}, "
          f"max |torch fp32 - fp64| = {e_torch:.3g}, bound = {bound:.3g}")
    assert e_dev <= bound, (e_dev, e_torch)
    # the rows built by hand say what they should: the +60000 entry has all the mass, its neighbours none
    assert got[0, 0] == 1.0 and (n_pos == 1 or got[1, 0] == 0.0)
    assert abs(got[2, 0] - 1.0 / (1.0 + np.exp(0.25))) <= 2.0 ** -22


def test_forced_probs_bad_arguments(lib):
    V, n_pos = 1003, 4
    x = torch.zeros((BATCH, n_pos, V), dtype=torch.float16, device="cuda")
    nxt = torch.zeros((BATCH, n_pos), dtype=torch.int32, device="cuda")
    out = torch.full((BATCH, n_pos), KR.SENTINEL, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(logits=x.data_ptr(), batch=BATCH, n_pos_=n_pos, V_=V, sb=n_pos * V, sp=V, limit=V - 4, nx=nxt.data_ptr(), nld=n_pos,
             o=out.data_ptr(), old=n_pos):
        return lib.wm_forced_probs(logits, batch, n_pos_, V_, sb, sp, limit, nx, nld, o, old, s)

    for bad in (dict(logits=None), dict(nx=None), dict(o=None), dict(batch=0), dict(n_pos_=0), dict(V_=0), dict(limit=0),
                dict(limit=V + 1), dict(sp=V - 1), dict(sb=n_pos * V - 1), dict(nld=n_pos - 1), dict(old=n_pos - 1),
                dict(logits=x.data_ptr() + 1), dict(o=out.data_ptr() + 2)):
        assert call(**bad) == 1, bad
        assert "wm_forced_probs" in lib.wm_last_error().decode(), bad
    torch.cuda.synchronize()
    assert (out == KR.SENTINEL).all(), "a refused call wrote"
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.allclose(out.cpu(), torch.full((BATCH, n_pos), 1.0 / (V - 4)), rtol=1e-6, atol=0)
