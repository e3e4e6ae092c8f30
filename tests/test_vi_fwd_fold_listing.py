"""Static checks on the device listing of the fused kernels on the folded gate ops (vi_fwd_kernel_vox_fold,
vi_kernels.hip / vi_fwd_kernels.inc), cross-compiled for gfx950 without a GPU, with the counter of
tests/test_vi_fwd_vox_listing.py.

The fold removes the operand split of r (8 v_max3 of the range guard, 8 conversions, 8 packed scalings, 16 mixed FMAs =
40 per block), the sigmoid's multiply (16) and one instruction of the blend (16): 72 per block, 144 for the two blocks of
a 16-voxel sub-tile's encoder phase.  Held here: the folded forms of the two default instantiations stay out of scratch
and within the register budgets of their workgroup sizes (128 VGPRs at 1,024 threads, 168 at 768), and their encoder
phase issues at least 120 fewer static vector instructions than the classic form compiled from the same tree (the 24
below 144 are for what the compiler re-forms around the change)."""
import pytest

from test_vi_fwd_vox_listing import KERNELS, VGPR_BUDGET, kernel_body, listing, tile_valu  # noqa: F401

# <T, NL, SE, BF, BLK>
FOLD_KERNELS = {
    11: "vi_fwd_kernel_vox_foldILi11ELi2ELi2ELb0ELi1024EE",
    24: "vi_fwd_kernel_vox_foldILi24ELi2ELi7ELb0ELi768EE",
}
MIN_SAVED = 120


@pytest.mark.parametrize("T", [11, 24])
def test_folded_kernel_resources_and_encoder_phase(listing, T):
    body, res = kernel_body(listing, FOLD_KERNELS[T])
    out, enc = tile_valu(body)
    out0, enc0 = tile_valu(kernel_body(listing, KERNELS[T])[0])
    print(f"T={T}: folded {res}; static vector instructions outside / inside the encoder phase: {out} / {enc}; "
          f"classic form, same tree: {out0} / {enc0}; saved in the encoder phase: {enc0 - enc}")
    assert res["ScratchSize"] == 0
    assert res.get("TotalNumVgprs", res["NumVgprs"]) <= VGPR_BUDGET[T]
    assert enc0 - enc >= MIN_SAVED
