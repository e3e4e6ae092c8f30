"""Static checks on the device listing of the fused encoder + ELBO kernels (vi_kernels.hip), cross-compiled for gfx950
without a GPU: the per-tau-table instantiations of both protocols keep their register budgets and stay out of
scratch, and the per-voxel part of the tile loop -- everything after the encoder phase -- holds no more vector
instructions than the figure recorded here.

That last figure is a guard for later work, not a result: the per-voxel part has not been changed since it was
recorded (MEASUREMENTS.md section 16 says why sharing it across the four lanes of a voxel was not built), so the
assertion holds with equality today and fails when something adds instructions behind the encoder.

The counter: inside one kernel, from the first `s_setprio 0` after the last MFMA (the encoder phase ends there, behind
gather_head) to the last branch back to the head of the tile loop before the block reduction's `s_barrier`, every
`v_*` instruction that is not an MFMA counts once, whatever its trip count.  Both ends are found by those landmarks
in the text of the listing: a change of the wave priorities or of the block reduction moves them, and the recorded
figure then has to be taken again with this counter on the commit before that change."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "qbold_vi_amd", "csrc", "vi_kernels.hip")

# <T, NL, SE, FAST, LITERAL, BF, GT, MIR, BLK> of the table kernels the default contexts dispatch to
KERNELS = {
    11: "vi_fwd_kernelILi11ELi2ELi2ELb1ELb0ELb0ELb1ELb0ELi1024EE",
    24: "vi_fwd_kernelILi24ELi2ELi7ELb1ELb0ELb0ELb1ELb0ELi768EE",
}
VGPR_BUDGET = {11: 128, 24: 168}
# this counter on the listing of commit a9948dc (the per-voxel part is the same code there and here)
PARENT_TAIL_VALU = {11: 595, 24: 802}


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
    out = str(tmp_path_factory.mktemp("vi_listing") / "vi_kernels.s")
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


def tail_valu(body):
    """Static vector instructions from the end of the encoder phase to the end of the tile loop."""
    ops = [opcode(l) for l in body]
    labels = {l.split(":")[0].strip(): i for i, l in enumerate(body) if re.match(r"^\.LBB\w+:", l)}
    last_mfma = max(i for i, o in enumerate(ops) if o and o.startswith("v_mfma"))
    start = next(i for i in range(last_mfma, len(body)) if ops[i] == "s_setprio" and body[i].split(";")[0].split()[-1] == "0")
    barrier = next(i for i in range(start, len(body)) if ops[i] == "s_barrier")
    back = [i for i in range(start, barrier) if ops[i] and ops[i].startswith("s_cbranch")
            and labels.get(body[i].split(";")[0].split()[-1], len(body)) < start]
    assert back, "no branch back to the head of the tile loop"
    n = sum(1 for o in ops[start:back[-1]] if o and o.startswith("v_") and not o.startswith("v_mfma"))
    return n


@pytest.mark.parametrize("T", [11, 24])
def test_table_kernel_resources_and_per_voxel_part(listing, T):
    body, res = kernel_body(listing, KERNELS[T])
    n = tail_valu(body)
    print(f"T={T}: {res}, vector instructions after the encoder phase: {n} (parent {PARENT_TAIL_VALU[T]})")
    assert res["ScratchSize"] == 0
    assert res.get("TotalNumVgprs", res["NumVgprs"]) <= VGPR_BUDGET[T]
    assert n <= PARENT_TAIL_VALU[T]
