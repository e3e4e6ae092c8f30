"""Static checks on the device listing of the six 64-wide exact-f32 training GEMM kernels (train_kernels.hip: the
kernels built on the 16-voxel tile skeleton), cross-compiled for gfx950 without a GPU.  For each of their nine
instantiations: no scratch, the register count stays inside the occupancy step it sat in before the kernels were
written on the shared skeleton (128 VGPRs: four waves per SIMD, 168: three), and the static count of
v_mfma_f32_16x16x4 instructions is the one of the hand-written kernels -- a helper that unrolled differently, or
dropped a chain, would change it.

The counts before and after the skeleton are in MEASUREMENTS.md ("Training GEMMs on one tile skeleton")."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "qbold_vi_amd", "csrc", "train_kernels.hip")

# kernel-name substring -> (VGPRs of the hand-written kernel, its static v_mfma_f32_16x16x4 count)
KERNELS = {
    "xw64_kernelILb0ELb0EE": (100, 64),
    "xw64_kernelILb1ELb0EE": (108, 64),
    "xw64_kernelILb0ELb1EE": (108, 64),
    "xw64_kernelILb1ELb1EE": (124, 64),
    "xw64_fork_kernel": (112, 128),
    "xw64_heads_kernel": (120, 80),
    "xw64_gate_kernel": (128, 64),
    "xw64_dual_kernel": (144, 128),
    "gate_bwd_wg_kernel": (164, 64),
}


def occupancy_step(vgprs):
    """the register count up to which a kernel keeps the waves per SIMD it has at `vgprs` (512 / waves, in eights)"""
    assert vgprs <= 168
    return 128 if vgprs <= 128 else 168


def hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    cc = hipcc()
    if cc is None:
        pytest.fail("hipcc not found: the ROCm toolchain is required")
    out = str(tmp_path_factory.mktemp("train_gemm_listing") / "train_kernels.s")
    cmd = [cc, "-S", "--cuda-device-only", "-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-gpu-rdc",
           "-Wno-unused-function", SRC, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out) as f:
        return f.read().split("\n")


def kernel_body(lines, key):
    """(body lines, {resource: value}) of the one kernel whose mangled name holds `key`."""
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l) and key in l.split(":")[0]]
    assert len(starts) == 1, (key, len(starts))
    end = next(i for i in range(starts[0], len(lines)) if "s_endpgm" in lines[i])
    res = {}
    for l in lines[end:end + 400]:
        m = re.match(r"^; (TotalNumVgprs|NumVgprs|NumAgprs|ScratchSize): (\d+)", l)
        if m and m.group(1) not in res:
            res[m.group(1)] = int(m.group(2))
        if len(res) == 4:
            break
    return lines[starts[0]:end + 1], res


@pytest.mark.parametrize("key", list(KERNELS))
def test_gemm_kernel_resources(listing, key):
    before, mfma = KERNELS[key]
    body, res = kernel_body(listing, key)
    vgprs = res.get("TotalNumVgprs", res["NumVgprs"])
    got = sum(1 for l in body if l.split(";")[0].strip().startswith("v_mfma_f32_16x16x4"))
    print(f"{key}: {res}; v_mfma_f32_16x16x4: {got} (hand-written kernel: {before} VGPRs, {mfma})")
    assert res["ScratchSize"] == 0
    assert vgprs <= occupancy_step(before), (vgprs, before)
    assert got == mfma
