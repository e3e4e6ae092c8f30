"""Static checks on the device listing of the one-lane-per-voxel fused kernel (vi_fwd_kernel_vox, vi_kernels.hip),
cross-compiled for gfx950 without a GPU: its T = 11 and T = 24 instantiations (split-f16 encoder, the ones the default
contexts dispatch whole rounds of 64-voxel tiles to) keep the register budgets of their workgroup sizes -- 128 VGPRs at
1,024 threads, 168 at 768 -- and stay out of scratch.

The count of static vector instructions of the tile loop outside the encoder phase is printed beside the four-lane
kernel's under the same counter, and beside the 595 / 802 of tests/test_vi_fwd_listing.py, for the record; it is not a
bound.  The figures are per tile, and a tile is 64 voxels here and 16 there: the new kernel executes its per-voxel
part once for 64 voxels where the four-lane kernel executes it four times (loop bodies count once either way)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "qbold_vi_amd", "csrc", "vi_kernels.hip")

# <T, NL, SE, BF, BLK>
KERNELS = {
    11: "vi_fwd_kernel_voxILi11ELi2ELi2ELb0ELi1024EE",
    24: "vi_fwd_kernel_voxILi24ELi2ELi7ELb0ELi768EE",
}
FOUR_LANE_KERNELS = {
    11: "vi_fwd_kernelILi11ELi2ELi2ELb1ELb0ELb0ELb1ELb0ELi1024EE",
    24: "vi_fwd_kernelILi24ELi2ELi7ELb1ELb0ELb0ELb1ELb0ELi768EE",
}
VGPR_BUDGET = {11: 128, 24: 168}
FOUR_LANE_TAIL_VALU = {11: 595, 24: 802}


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
    out = str(tmp_path_factory.mktemp("vi_vox_listing") / "vi_kernels.s")
    cmd = [cc, "-S", "--cuda-device-only", "-O3", "-DQB_VI_PROBE", "--offload-arch=gfx950", "-std=c++17",
           "-fno-gpu-rdc", "-Wno-unused-function", SRC, "-o", out]
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


def opcode(line):
    t = line.split(";")[0].strip()
    if not t or t.startswith(".") or t.endswith(":"):
        return None
    return t.split()[0]


def tile_valu(body):
    """Static vector instructions (MFMAs apart) of the tile loop outside its encoder phase, whatever their trip count:
    everything between the barrier behind the LDS fill and the block reduction's barrier, less the stretch from the
    tile's first `s_setprio 3` (a tile, or a sub-tile, starts there) to the first `s_setprio 0` behind the last MFMA
    (the encoder phase ends there).  Unlike the four-lane test's counter this one does not depend on where the
    compiler puts the loop's back edge, so it reads both kernels."""
    ops = [opcode(l) for l in body]
    prio = lambda i: ops[i] == "s_setprio" and body[i].split(";")[0].split()[-1]
    barriers = [i for i, o in enumerate(ops) if o == "s_barrier"]
    assert len(barriers) >= 2, "expected the LDS-fill barrier and the block reduction's"
    first, last = barriers[0], barriers[-1]
    last_mfma = max(i for i, o in enumerate(ops) if o and o.startswith("v_mfma"))
    enc0 = next(i for i in range(first, len(body)) if prio(i) == "3")
    enc1 = next(i for i in range(last_mfma, len(body)) if prio(i) == "0")
    assert first < enc0 < enc1 < last
    valu = lambda a, b: sum(1 for o in ops[a:b] if o and o.startswith("v_") and not o.startswith("v_mfma"))
    return valu(first, enc0) + valu(enc1, last), valu(enc0, enc1)


@pytest.mark.parametrize("T", [11, 24])
def test_whole_voxel_kernel_resources(listing, T):
    body, res = kernel_body(listing, KERNELS[T])
    n, enc = tile_valu(body)
    n4, enc4 = tile_valu(kernel_body(listing, FOUR_LANE_KERNELS[T])[0])
    print(f"T={T}: {res}; static vector instructions outside / inside the encoder phase: {n} / {enc} per 64-voxel tile "
          f"(encoder phase: one rolled sub-tile, run four times); four-lane kernel, same counter: {n4} / {enc4} per "
          f"16-voxel tile (its own test's counter: {FOUR_LANE_TAIL_VALU[T]})")
    assert res["ScratchSize"] == 0
    assert res.get("TotalNumVgprs", res["NumVgprs"]) <= VGPR_BUDGET[T]
