"""The open-end walk on a real MI355X (csrc/align.hip behind wm_dtw_open and wm_align_open): bit for bit
alignment.dtw_open_cpu's paths and end rows, the closed entries unchanged on the same inputs, and wm_align_open's matrix bit for
bit wm_align's."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import alignment as A  # noqa: E402
import native  # noqa: E402
import timing  # noqa: E402
from test_gpu_word_timestamps import dtw_inputs, run_dtw  # noqa: E402  (the closed walk's inputs and its runner)


def run_dtw_open(xs):
    """wm_dtw_open on a (ragged) batch of fp32 matrices -> [(text_indices, time_indices, end_row)] and the raw outputs."""
    lib = native.load_library()
    Bn = len(xs)
    R, Cc = max(max(x.shape[0] for x in xs), 1), max(max(x.shape[1] for x in xs), 1)
    ld = Cc + 3
    buf = torch.full((Bn, R, ld), 1e30, dtype=torch.float32)
    for b, x in enumerate(xs):
        buf[b, :x.shape[0], :x.shape[1]] = torch.from_numpy(x)
    buf = buf.cuda()
    n_rows = torch.tensor([x.shape[0] for x in xs], dtype=torch.int32).cuda()
    n_cols = torch.tensor([x.shape[1] for x in xs], dtype=torch.int32).cuda()
    path_ld = R + Cc
    pt = torch.full((Bn, path_ld), -7, dtype=torch.int32).cuda()
    pf = torch.full((Bn, path_ld), -7, dtype=torch.int32).cuda()
    pl = torch.full((Bn,), -7, dtype=torch.int32).cuda()
    er = torch.full((Bn + 1,), -7, dtype=torch.int32).cuda()
    ws = torch.empty(lib.wm_dtw_workspace_bytes(Bn, R, Cc), dtype=torch.uint8).cuda()
    native.check(lib.wm_dtw_open(buf.data_ptr(), ld, R * ld, Bn, n_rows.data_ptr(), n_cols.data_ptr(), R, Cc, pt.data_ptr(), pf.data_ptr(),
                                 path_ld, pl.data_ptr(), er.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream),
                 "wm_dtw_open")
    torch.cuda.synchronize()
    pt, pf, pl, er = pt.cpu().numpy(), pf.cpu().numpy(), pl.cpu().tolist(), er.cpu().tolist()
    assert er[Bn] == -7                                                            # nothing past end_row[batch - 1]
    return [(pt[b, :pl[b]], pf[b, :pl[b]], er[b]) for b in range(Bn)], (pt, pf, pl)


def band(N, M, k):
    x = np.ones((N, M), dtype=np.float32)
    for r in range(k):
        x[r, r * M // k: (r + 1) * M // k] = -1
    return x


def check_open(x, got, raw=None):
    ti, fi, end = A.dtw_open_cpu(x)
    gt, gf, gend = got
    assert gend == end and len(gt) == len(ti) and gt.tolist() == ti.tolist() and gf.tolist() == fi.tolist()
    if raw is not None:
        pt, pf, pl = raw
        assert (pt[0, pl[0]:] == -7).all() and (pf[0, pl[0]:] == -7).all()          # nothing past the path


def check_closed(x):
    (got,), _ = run_dtw([x])
    ti, fi = timing.dtw_cpu(x)
    assert got[0].tolist() == ti.tolist() and got[1].tolist() == fi.tolist()


@pytest.mark.parametrize("kind", ["random", "ties"])
@pytest.mark.parametrize("N,M", [(1, 1), (1, 7), (5, 1), (7, 40), (33, 100), (225, 1500), (447, 1500)])
def test_dtw_open_equals_dtw_open_cpu(kind, N, M):
    x = dtw_inputs(kind, N, M, 100 * N + M)
    (got,), raw = run_dtw_open([x])
    check_open(x, got, raw)
    check_closed(x)                                                                 # wm_dtw on the same input is still dtw_cpu


@pytest.mark.parametrize("N,M,k", [(12, 60, 1), (12, 60, 6), (12, 60, 12), (225, 1500, 1), (225, 1500, 100), (225, 1500, 225),
                                   (600, 700, 513)])
def test_dtw_open_planted_band(N, M, k):
    """A band of -1 over the first k rows: the walk ends in row k (k = 1, the middle, N); 600 rows take the 1024-thread form."""
    x = band(N, M, k)
    (got,), raw = run_dtw_open([x])
    assert got[2] == k
    check_open(x, got, raw)
    check_closed(x)


@pytest.mark.parametrize("kind", ["random", "ties"])
def test_dtw_open_ragged_batch_with_an_empty_row(kind):
    xs = [dtw_inputs(kind, n, m, 7 + n) for n, m in ((9, 61), (1, 5), (30, 17))]
    xs.insert(2, np.zeros((0, 11), dtype=np.float32))
    xs.append(band(20, 50, 8))
    got, (_, _, pl) = run_dtw_open(xs)
    for x, g in zip(xs, got):
        check_open(x, g)
    assert pl[2] == 0 and got[2][2] == 0                                            # no rows: no path, end_row 0
    closed, _ = run_dtw([x for x in xs if x.shape[0]])
    for x, (gt, gf) in zip([x for x in xs if x.shape[0]], closed):
        ti, fi = timing.dtw_cpu(x)
        assert gt.tolist() == ti.tolist() and gf.tolist() == fi.tolist()


def test_align_open_matrix_is_wm_aligns_and_its_walk_is_dtw_open_cpu():
    """The ragged three-head fixture of test_align_matrix_three_heads_ragged through wm_align and wm_align_open."""
    lib = native.load_library()
    Bn, n_layers, H, heads, cap, Tk, n_tokens, n_frames, n_prefix = 3, 2, 2, [0, 2, 3], 16, 100, [6, 16, 9], [100, 93, 3], 3
    g = torch.Generator().manual_seed(11)
    tape = (torch.randn(Bn, len(heads), cap, 64, generator=g) * 4.0).half().cuda()
    cross = [torch.randn(Bn, 2, H, Tk, 64, generator=g).half().cuda() for _ in range(n_layers)]
    nt, nf = torch.tensor(n_tokens, dtype=torch.int32).cuda(), torch.tensor(n_frames, dtype=torch.int32).cuda()
    ld, path_ld = Tk + 4, cap + Tk
    out = {}
    for name in ("closed", "open"):
        matrix = torch.full((Bn, cap, ld), 777.0, dtype=torch.float32).cuda()
        pt = torch.full((Bn, path_ld), -7, dtype=torch.int32).cuda()
        pf = torch.full((Bn, path_ld), -7, dtype=torch.int32).cuda()
        pl, er = torch.full((Bn,), -7, dtype=torch.int32).cuda(), torch.full((Bn,), -7, dtype=torch.int32).cuda()
        ws = torch.empty(lib.wm_align_workspace_bytes(Bn, len(heads), cap, Tk), dtype=torch.uint8).cuda()
        io = native.align_io(None, H, Tk, tape, cross, heads, nt, nf, n_prefix, 7, cap, matrix, ld, pt, pf, pl, ws)
        stream = torch.cuda.current_stream().cuda_stream
        rc = lib.wm_align(C.byref(io), stream) if name == "closed" else lib.wm_align_open(C.byref(io), er.data_ptr(), stream)
        torch.cuda.synchronize()
        assert rc == 0, lib.wm_last_error()
        out[name] = (matrix.cpu().numpy(), pt.cpu().numpy(), pf.cpu().numpy(), pl.cpu().tolist(), er.cpu().tolist())
    m_closed, m_open = out["closed"][0], out["open"][0]
    assert m_closed.tobytes() == m_open.tobytes()                                   # guards included
    _, pt, pf, pl, er = out["open"]
    for b in range(Bn):
        N, F = n_tokens[b] - n_prefix - 1, n_frames[b]
        ti, fi, end = A.dtw_open_cpu(-m_open[b, :N, :F])
        assert er[b] == end and pl[b] == len(ti) and pt[b, :pl[b]].tolist() == ti.tolist() and pf[b, :pl[b]].tolist() == fi.tolist()
        assert (pt[b, pl[b]:] == -7).all() and (pf[b, pl[b]:] == -7).all()
        ct, cf = timing.dtw_cpu(-m_closed[b, :N, :F])
        assert out["closed"][3][b] == len(ct) and out["closed"][1][b, :len(ct)].tolist() == ct.tolist()
    assert 1 <= min(er) and max(e - (n - n_prefix - 1) for e, n in zip(er, n_tokens)) <= 0
