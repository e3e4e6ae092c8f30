"""relu_frag (encoder_core.h) against the form it replaced, bit for bit, on the GPU.

block_stream2 derives the split-f16 operand fragments of relu(b) from those of b on the packed halves (v_pk_max_f16
on hi, lo cleared under hi's sign bit) where it used to apply relu4 and split again.  Every other test sees the
encoder through both of its users at once, so a wrong fragment would cancel there; this one builds
tests/c/relu_frag_check.hip, which writes the fragments of both forms for the same inputs, and compares the bits on
the values where the two could part: +-0, negatives that round to -0 in f16 (with a lo half that is not zero),
f16 subnormals, the neighbourhood of 65504 on both sides of the overflow to inf, +-inf, and a dense random sweep
over 2^-40 .. 2^17.  NaN inputs are left out: relu4 turns a NaN into 0 while relu_frag may leave a NaN lo half, and a
NaN only follows an operand overflow that the range guard has already reported for the voxel."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def edge_values():
    f16_tiny = 2.0 ** -24            # smallest f16 subnormal; |x| <= 2^-25 rounds hi to +-0
    v = [0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 3.14159, -3.14159]
    for k in range(-40, -22):        # hi = +-0 or the first subnormals, lo carries the value
        v += [2.0 ** k, -(2.0 ** k), 1.37 * 2.0 ** k, -1.37 * 2.0 ** k]
    v += [f16_tiny / 2, -f16_tiny / 2, np.nextafter(np.float32(f16_tiny / 2), np.float32(1)),
          -np.nextafter(np.float32(f16_tiny / 2), np.float32(1)), 1e-9, -1e-9, 1e-30, -1e-30, 1e-45, -1e-45]
    for k in range(-24, -13):        # f16 subnormals and the first normals
        v += [1.11 * 2.0 ** k, -1.11 * 2.0 ** k, 2.0 ** k, -(2.0 ** k)]
    for x in (65504.0, 65503.9, 65519.9, 65520.0, 65536.0, 7e4, 1e5, 3e38):   # last finite half, the tie to inf, beyond
        v += [x, -x]
    v += [np.inf, -np.inf]
    return np.array(v, np.float32)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(cc), "hipcc not found: the ROCm toolchain is required"
    out = str(tmp_path_factory.mktemp("relu_frag") / "librelu_frag_check.so")
    cmd = [cc, "-O3", "--offload-arch=gfx950", "-fPIC", "-shared", "-std=c++17", "-fno-gpu-rdc", "-Wno-unused-function",
           "-I", os.path.join(ROOT, "qbold_vi_amd", "csrc"), os.path.join(ROOT, "tests", "c", "relu_frag_check.hip"),
           "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(out)
    lib.relu_frag_check.restype = C.c_int
    lib.relu_frag_check.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def fragments(lib, x):
    """(ref, got) as uint16 [n, 2]: the (hi, lo) halves of every input value in both forms."""
    n = x.size
    assert n % 16 == 0
    x = np.ascontiguousarray(x, np.float32)
    ref, got = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    rc = lib.relu_frag_check(x.ctypes.data, n // 16, ref.ctypes.data, got.ctypes.data)
    assert rc == 0, f"HIP error {rc}"

    def halves(d):   # per lane: [k-step 2][hi 4 dwords | lo 4 dwords], a dword = the halves of two neighbouring values
        d = d.view(np.uint16).reshape(n // 16, 2, 2, 8)          # lane, k-step, part, value
        return np.stack([d[:, :, 0, :].reshape(-1), d[:, :, 1, :].reshape(-1)], -1)
    return halves(ref), halves(got)


def test_relu_frag_is_the_split_of_relu_bit_for_bit(checker):
    edge = edge_values()
    rng = np.random.default_rng(5)
    sweep = (rng.choice([-1.0, 1.0], 1 << 16) * 2.0 ** rng.uniform(-40, 17, 1 << 16)).astype(np.float32)
    x = np.concatenate([edge, sweep, rng.standard_normal(1 << 14).astype(np.float32)])
    x = np.concatenate([x, np.zeros(-x.size % 16, np.float32)])
    assert not np.isnan(x).any()
    ref, got = fragments(checker, x)
    # the reference form is what it claims to be: hi = f16(relu x) wherever that is finite
    with np.errstate(over="ignore"):
        want_hi = np.maximum(x, np.float32(0)).astype(np.float16).view(np.uint16)
    assert np.array_equal(ref[:, 0], want_hi)
    neg = np.signbit(x)
    assert (ref[neg] == 0).all()                       # relu of anything negative, -0 and -inf included: +0, +0
    assert int((ref[~neg & (x > 0) & (x < 2.0 ** -25), 1] != 0).sum()) > 10   # hi = +0 with a live lo half is covered
    bad = np.nonzero((ref != got).any(1))[0]
    print(f"{x.size} values, {int(neg.sum())} negative, mismatches: {bad.size}",
          [(float(x[i]), ref[i].tolist(), got[i].tolist()) for i in bad[:8]])
    assert bad.size == 0
