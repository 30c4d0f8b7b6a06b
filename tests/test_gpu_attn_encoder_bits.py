"""Encoder attention (wm_attn_encoder), bit for bit against the kernel of the commit before the dead tail work and the LDS
exchanges were removed: tests/golden/attn_encoder_parent.npz holds that kernel's outputs (scripts/gen_attn_encoder_golden.py,
which also makes the inputs: seeded numpy PCG64, fp16, q / k pre-scaled as the QKV epilogue does).  Every assertion is byte
equality -- the change skips work whose contribution is exactly zero and exchanges maxima and sums over other wires; no rounding
moves.

Shapes (B = 2, H = 3: six heads, so the group of eight has padding items): the QB = 4 path with tails of 1, 16, 17, 44 and 63
keys (T = 257, 272, 273, 300, 383: either side of every 16-key block edge and of the 32-key chunk edge), without a tail (320),
with 32, 33 and 48 live queries in the last query tile (288, 289, 304); the QB = 2 path (100, 128); the real length once
(T = 1500); two shapes with eight key rows near the end times 8, one of them inside the tail tile, so that the rescale branch
fires in late tiles and in the tail; the persistent form on 8 workgroups (a child process: the lab knob is read once per
process), where t300_b3h5 has 32 items, four per workgroup."""
import hashlib
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_attn_encoder_golden", os.path.join(ROOT, "scripts", "gen_attn_encoder_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

gpu = pytest.mark.gpu
QB4 = [n for n, c in gen.CASES.items() if c[1] > 128]


@pytest.fixture(scope="module")
def golden():
    return np.load(gen.GOLDEN)


@pytest.fixture(scope="module")
def lib():
    import native
    return native.load_library()


_outs = {}


def plain(lib, name):
    """The plain launch form's output of a case, computed once."""
    if name not in _outs:
        import native
        import torch
        B, T, H, _ = gen.CASES[name]
        _outs[name] = gen.run_kernel(lib, native, torch, gen.make_qkv(name), B, T, H)
    return _outs[name]


def check_against_golden(golden, name, out):
    rows = gen.kept_rows(name)
    want = golden[name + "/rows"]
    got = out if rows is None else out[:, rows]
    diff = np.argwhere(got.view(np.uint16) != want.view(np.uint16))
    print(f"{name}: {len(diff)} of {got.size} stored values differ; output sha256 {gen.sha(out)[:16]}, golden {str(golden[name + '/out_sha256'])[:16]}")
    assert len(diff) == 0, f"{name}: first differences (clip, stored row, column): {diff[:8].tolist()}"
    assert gen.sha(out) == str(golden[name + "/out_sha256"]), f"{name}: the stored rows agree, the whole output does not"


@gpu
@pytest.mark.parametrize("name", list(gen.CASES))
def test_bits_of_parent_kernel(lib, golden, name):
    assert gen.sha(gen.make_qkv(name)) == str(golden[name + "/in_sha256"]), "the input generator moved, not the kernel"
    check_against_golden(golden, name, plain(lib, name))


@pytest.mark.parametrize("name", ["t273_late", "t300_late"])
def test_late_maxima_move_the_running_maximum(name):
    """(No GPU needed.)  The two `late` cases do what they are there for: in most rows the largest score sits in one of the boosted key rows, so the
    running maximum moves in late tiles and, for the row inside the tail tile, in the tail."""
    B, T, H, _ = gen.CASES[name]
    x = gen.make_qkv(name).astype(np.float32).reshape(B, T, 3, H, 64)
    s = np.einsum("qd,kd->qk", x[0, :, 0, 0], x[0, :, 1, 0])
    boosted = [T - b for b in gen.LATE_ROWS]
    arg = s.argmax(axis=1)
    assert np.isin(arg, boosted).mean() > 0.9
    assert (arg >= (T - 1) // 64 * 64).mean() > 0.05            # the tail tile's boosted row wins for its share of the queries


@gpu
def test_batch_independence(lib):
    """Clip 0 of a two-clip launch is byte-equal to the same clip launched alone."""
    import native
    import torch
    for name in ("t300", "t289", "t100"):
        B, T, H, _ = gen.CASES[name]
        qkv = gen.make_qkv(name)
        alone = gen.run_kernel(lib, native, torch, np.ascontiguousarray(qkv[:T]), 1, T, H)
        assert np.array_equal(alone[0].view(np.uint16), plain(lib, name)[0].view(np.uint16)), name


_CHILD = r"""
import os, sys
import numpy as np
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "eddie-wang-hackathon2023_amd"), os.path.join(sys.argv[1], "scripts")]
import native, torch
import gen_attn_encoder_golden as gen
lib = native.load_library()
for name in sys.argv[2:]:
    B, T, H, _ = gen.CASES[name]
    print(name, gen.sha(gen.run_kernel(lib, native, torch, gen.make_qkv(name), B, T, H)), flush=True)
buf = __import__("ctypes").create_string_buffer(4096)
lib.wm_lab_knobs(buf, 4096)
print("knobs", buf.value.decode(), flush=True)
"""


@gpu
@pytest.mark.parametrize("wgs", [8, 4])
def test_persistent_form(lib, golden, wgs):
    """8 workgroups walk over 16 (B = 2, H = 3), 32 (t300_b3h5) and 48 (T = 1500) items, 4 workgroups over twice as many each:
    byte-equal to the plain form and to the golden file, so a clip's result depends neither on the launch form nor on the
    grid size.  wm_attn_encoder has no max_wgs argument; the lab knob WM_ATTN_MAX_WGS reaches it and is read once per
    process, hence the child."""
    env = dict(os.environ, WM_LAB="1", WM_ATTN_MAX_WGS=str(wgs))
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT] + QB4, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = {}
    for l in r.stdout.splitlines():                       # only the child's own lines: the runtime may print warnings of its own
        key, _, val = l.partition(" ")
        if key in QB4 or key == "knobs":
            lines[key] = val.strip()
    assert f"WM_ATTN_MAX_WGS={wgs}" in lines["knobs"], "the persistent form was not reached: " + lines["knobs"]
    for name in QB4:
        assert lines[name] == str(golden[name + "/out_sha256"]), f"{name}: persistent form differs from the golden file"
        assert lines[name] == gen.sha(plain(lib, name)), f"{name}: persistent form differs from the plain form"
