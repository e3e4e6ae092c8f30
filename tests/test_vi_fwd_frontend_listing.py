"""Static checks on the device listings of the one-lane-per-voxel fused kernels after the per-lane front end
(first_operand) and the head hand-over by one transpose per tile (keep_head_tile, transpose_heads, encoder_core.h):
vi_fwd_kernel_vox_fold<11,2,2,false,1024> and <24,2,7,false,768> and their classic vi_fwd_kernel_vox siblings,
cross-compiled for gfx950 without a GPU with the fixtures and the counter of tests/test_vi_fwd_vox_listing.py.

  - no scratch, and the register budgets of the workgroup sizes: 128 VGPRs at 1,024 threads, 168 at 768;
  - the encoder-phase counter (tile_valu's second figure: static vector instructions from the first `s_setprio 3`
    behind the LDS fill to the first `s_setprio 0` behind the last MFMA) of the folded kernels at least 40 below what
    MEASUREMENTS 28 recorded: 765 at T = 11, 889 at T = 24.  A listing of the parent commit built the same way with
    this compiler gives the same 765 / 889; this tree gives 712 / 729.  (The classic siblings, for the record: 891 ->
    838 at T = 11; 1033 -> 920 at T = 24, L = 2, the one kernel that keeps gather_head because the slot form needs 12
    bytes of scratch there.)
  - no canonicalising `v_max_f32 vN, vN, vN` is left in the front end of the four changed kernels (the four-lane
    kernels keep theirs: 11 and 24, one per signal)."""
import re

import pytest

from test_vi_fwd_vox_listing import KERNELS, VGPR_BUDGET, kernel_body, listing, opcode, tile_valu  # noqa: F401

FOLD_KERNELS = {T: k.replace("vi_fwd_kernel_voxI", "vi_fwd_kernel_vox_foldI") for T, k in KERNELS.items()}
ENC_VALU_BEFORE = {11: 765, 24: 889}   # MEASUREMENTS 28; the parent commit's listing under this compiler gives the same


@pytest.mark.parametrize("T", [11, 24])
@pytest.mark.parametrize("names", [KERNELS, FOLD_KERNELS], ids=["classic", "fold"])
def test_resources(listing, names, T):
    body, res = kernel_body(listing, names[T])
    print(f"{names[T]}: {res}")
    assert res["ScratchSize"] == 0
    assert res.get("TotalNumVgprs", res["NumVgprs"]) <= VGPR_BUDGET[T]


@pytest.mark.parametrize("T", [11, 24])
def test_encoder_phase_counter(listing, T):
    outside, enc = tile_valu(kernel_body(listing, FOLD_KERNELS[T])[0])
    outside_c, enc_c = tile_valu(kernel_body(listing, KERNELS[T])[0])
    print(f"T={T}: static vector instructions outside / inside the encoder phase: folded {outside} / {enc} "
          f"(before: {ENC_VALU_BEFORE[T]} inside), classic {outside_c} / {enc_c}")
    assert enc <= ENC_VALU_BEFORE[T] - 40


@pytest.mark.parametrize("T", [11, 24])
@pytest.mark.parametrize("names", [KERNELS, FOLD_KERNELS], ids=["classic", "fold"])
def test_no_canonicalising_max_in_front_of_the_clamp(listing, names, T):
    """`v_max_f32 vN, vN, vN` quiets a loaded value in front of v_med3_f32; the clamp is one instruction now.  The whole
    kernel is searched: the sampling phase has none either."""
    body, _ = kernel_body(listing, names[T])
    canon = [l.strip() for l in body if opcode(l) and opcode(l).startswith("v_max_f32")
             and re.match(r"v_max_f32\w*\s+(v\d+), \1, \1\s*$", l.split(";")[0].strip())]
    med3 = sum(1 for l in body if (opcode(l) or "").startswith("v_med3_f32"))
    print(f"{names[T]}: {len(canon)} canonicalising v_max_f32, {med3} v_med3_f32")
    assert not canon
    assert med3 >= 9     # the spin echo and the eight signals of the lane's window
