"""Encoder attention kernel, builds against each other in ONE process: every library given on the command line is loaded twice
(copies under other names, so that each copy has its own state), once for the plain launch form and once for the budget form
(the lab knob WM_ATTN_MAX_WGS is read at a library's first launch: 2 x 96 workgroups, the 96-CU budget of the shared
encoder).  The arms then take turns, ROUNDS times: LAUNCHES launches each per turn (200: windows of 0.2 to 0.5 s), random data,
events around them.

    python scripts/attn_encoder_tail_ab.py name=path/to/lib.so [name=path ...]        (first name = the base of the ratios)

Shapes: large-v2 (H = 20, T = 1500), B = 128 and B = 72 (one launch of the 576-clip pass: 8 launches per layer) in the plain
form, B = 72 in the budget form.  Prints every turn's time, then mean and spread (max - min) per arm and the ratio to the base;
a SHA-256 of one output per arm shows that the builds agree bit for bit."""
import ctypes as C
import hashlib
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "eddie-wang-hackathon2023_amd")]
import native  # noqa: E402,F401  (runtime defaults before torch initialises HIP)
import torch  # noqa: E402

ROUNDS = int(os.environ.get("ROUNDS", "6"))
LAUNCHES = int(os.environ.get("LAUNCHES", "200"))
H, T = 20, 1500
vp, i32 = C.c_void_p, C.c_int
tmp = tempfile.mkdtemp()
s = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device="cuda").manual_seed(7)
qkv = (torch.randn(128 * T, 3 * H * 64, device="cuda", generator=g) * 0.5).half()
out = torch.empty(128 * T, H * 64, device="cuda", dtype=torch.float16)


def load(name, path, form):
    copy = os.path.join(tmp, f"{name}_{form}.so")
    shutil.copy(path, copy)
    lib = C.CDLL(copy)
    lib.wm_attn_encoder.argtypes = [vp, i32, i32, i32, i32, vp, i32, vp]
    return lib


def launch(lib, B):
    rc = lib.wm_attn_encoder(qkv.data_ptr(), 3 * H * 64, B, T, H, out.data_ptr(), H * 64, s)
    assert rc == 0, rc


names = [a.split("=")[0] for a in sys.argv[1:]]
paths = dict(a.split("=") for a in sys.argv[1:])
arms = {}                                     # (form, B, name) -> lib
os.environ.pop("WM_ATTN_MAX_WGS", None)
for n in names:
    lib = load(n, paths[n], "plain")
    launch(lib, 3)                            # first launch: the knob is read (absent)
    arms[("plain", 128, n)] = arms[("plain", 72, n)] = lib
os.environ["WM_LAB"], os.environ["WM_ATTN_MAX_WGS"] = "1", "192"
for n in names:
    lib = load(n, paths[n], "budget")
    launch(lib, 3)
    arms[("budget96", 72, n)] = lib
torch.cuda.synchronize()

times = {k: [] for k in arms}
hashes = {}
for k, lib in arms.items():
    out.zero_()
    launch(lib, k[1])
    torch.cuda.synchronize()
    hashes[k] = hashlib.sha256(out[:k[1] * T].cpu().numpy().tobytes()).hexdigest()[:16]
for r in range(ROUNDS):
    for k, lib in arms.items():
        for _ in range(3):
            launch(lib, k[1])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            launch(lib, k[1])
        e1.record()
        torch.cuda.synchronize()
        times[k].append(e0.elapsed_time(e1) / LAUNCHES)
        print(f"round {r} {k[0]:8s} B={k[1]:3d} {k[2]:8s} {times[k][-1]:8.4f} ms", flush=True)
shutil.rmtree(tmp, ignore_errors=True)              # (the copies stay mapped; only their names go)
print()
for form, B in (("plain", 128), ("plain", 72), ("budget96", 72)):
    base = sum(times[(form, B, names[0])]) / ROUNDS
    for n in names:
        t = times[(form, B, n)]
        mean = sum(t) / len(t)
        print(f"{form:8s} B={B:3d} {n:8s} mean {mean:8.4f} ms  spread {max(t) - min(t):7.4f}  min {min(t):8.4f}  "
              f"{4.0 * T * T * 64 * H * B / mean / 1e9:5.0f} TFLOP/s  vs {names[0]} {100 * (mean / base - 1):+6.2f} %  sha256 {hashes[(form, B, n)]}")
