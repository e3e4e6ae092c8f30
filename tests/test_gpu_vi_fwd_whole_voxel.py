"""The one-lane-per-voxel fused kernel (vi_fwd_kernel_vox: 64-voxel wave tiles, a lane owns a voxel through the sampling
phase) against the four-lane kernel (vi_fwd_kernel: 16-voxel tiles, four lanes share a voxel's draws), through the two
kernel-selection bits of qbold_vi_fwd:

  QBOLD_KSEL_VI_FOUR_LANE    every voxel on the four-lane kernel
  QBOLD_KSEL_VI_WHOLE_TILES  every whole 64-voxel tile on the new kernel, the remainder on the four-lane one

The new kernel walks a voxel's four draw shares in the four-lane kernel's order and adds them in voxel_sum's order
(elbo_core.h), so posterior parameters and (nll, kl) are held to bitwise equality; only the three masked sums, which
are float accumulations whose order depends on the layout as it depends on the grid, get the 1e-6 the existing
fused-kernel test (test_gpu_vi_fwd_shared_prologue.py) holds sums to.  Weights and inputs are that test's make_case."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_gpu_vi_fwd_shared_prologue import dev, make_case  # noqa: E402

pytestmark = pytest.mark.gpu

FOUR_LANE = 16777216     # QBOLD_KSEL_VI_FOUR_LANE
WHOLE_TILES = 33554432   # QBOLD_KSEL_VI_WHOLE_TILES
N_SMALL = 64 * 3 + 21    # three whole 64-voxel tiles; the rest is one whole 16-voxel tile plus five voxels
Z_MAX = 4.8549           # QB_Z_MAX, qbold_dev.h
LOGIT_CLIP = 13.815509557963774   # QB_LOGIT_CLIP, elbo_core.h

_cases = {}


def small_case(params, T):
    """make_case cut to N_SMALL voxels, computed once per protocol and never modified (users copy what they change)."""
    if T not in _cases:
        ctx, orc, w, x, mask, prior, _ = make_case(params, T, seed=21)
        x, mask, prior = x[:N_SMALL].copy(), mask[:N_SMALL].copy(), prior[:N_SMALL].copy()
        mask[N_SMALL - 1], mask[N_SMALL - 2], mask[70] = 0.0, 1.0, 0.0   # zeros in the remainder and in a whole tile
        _cases[T] = (ctx, orc, w, x, mask, prior)
    return _cases[T]


def run(ctx, sel, *args, **kw):
    ctx.set_kernel_selection(sel)
    try:
        return ctx.vi_fwd(*args, **kw)
    finally:
        ctx.set_kernel_selection(0)


def assert_same(a, b, what):
    (sa, qa, nka), (sb, qb, nkb) = a, b
    assert torch.equal(qa, qb), what
    assert torch.equal(nka, nkb), what
    assert torch.allclose(sa, sb, rtol=1e-6, atol=1e-9), (what, sa, sb)
    assert float(sa[2]) == float(sb[2]), what


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("T", [11, 24])
def test_whole_tiles_match_four_lane_kernel(params, T, precision):
    """Full and short Philox calls and empty draw shares ((S, K) = (32, 70), (5, 9), (1, 0)), a mask with zeros and no
    mask, voxel0 = 0 and beyond 2^32, the split-f16 and the bf16 encoder."""
    from qbold_vi_amd.ops import EncoderWeights
    ctx, orc, w, x, mask, prior = small_case(params, T)
    ew = EncoderWeights(ctx, T, 60, 2, True, -3.0, precision=precision).set_from_arrays(w)
    xd, md, pd = dev(x), dev(mask), dev(prior)
    assert 0 < int((mask == 0).sum()) < N_SMALL
    for m in (md, None):
        for S, K in ((32, 70), (5, 9), (1, 0)):
            for v0 in (0, 12345678901):
                a = run(ctx, FOUR_LANE, ew, xd, m, pd, S, K, seed=4, voxel0=v0)
                b = run(ctx, WHOLE_TILES, ew, xd, m, pd, S, K, seed=4, voxel0=v0)
                assert bool(torch.isfinite(a[2]).all()) and bool(torch.isfinite(a[1]).all())
                assert_same(a, b, (T, precision, m is not None, S, K, v0))


@pytest.mark.parametrize("T", [11, 24])
def test_operand_range_status_per_voxel(params, T):
    """A voxel beyond the f16 operand range in sub-tile 2 of 64-voxel tile 1 (built as test_operand_range_status_reaches_nll
    builds it): its terms are NaN on both kernels, and every other voxel -- the same column of the tile's other three
    sub-tiles and the rest of its own sub-tile included -- is the same bits."""
    from qbold_vi_amd.ops import EncoderWeights
    ctx, orc, w, x, mask, prior = small_case(params, T)
    hot = 64 + 16 * 2 + 6
    x, mask = x.copy(), mask.copy()
    x[hot] = 1e8
    x[hot, ctx.se_idx] = 1e-2
    mask[hot] = 1.0
    xd, md, pd = dev(x), dev(mask), dev(prior)

    def scaled(sc):
        w2 = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in w.items()}
        for k in ("W0", "b0", "bc", "br1", "br2"):
            w2[k] = w[k] * sc
        w2["Wf"], w2["Ws"] = w["Wf"] / sc, w["Ws"] / sc
        return w2

    ew = tripped = None
    for sc in (1.0, 3.0, 10.0, 30.0, 100.0, 300.0, 1000.0, 3000.0, 10000.0):
        ew = EncoderWeights(ctx, T, 60, 2, True, -3.0).set_from_arrays(scaled(sc))
        tripped = torch.isnan(ctx.encoder_fwd(ew, xd, want=("out2",))[1]).any(1)
        if bool(tripped[hot]):
            break
    assert bool(tripped[hot]) and int(tripped.sum()) == 1, "no scale of the ladder trips the hot voxel alone"
    a = run(ctx, FOUR_LANE, ew, xd, md, pd, 6, 10, seed=7)
    b = run(ctx, WHOLE_TILES, ew, xd, md, pd, 6, 10, seed=7)
    keep = ~tripped
    for sums, q, nk in (a, b):
        assert bool(torch.isnan(nk[hot, 0]))
        assert not bool(torch.isfinite(sums[0]))
        assert bool(torch.isfinite(nk[keep]).all())
        assert float(sums[2]) == float(md.sum())
    assert torch.equal(a[1][keep], b[1][keep])
    assert torch.equal(a[2][keep], b[2][keep])
    for mate in (hot - 32, hot - 16, hot + 16, hot - 1, hot + 1):
        assert bool(keep[mate])


def reach_of(q, std, offdiag):
    """The reach kl_draws_fast tests against the logit clip, from posterior parameters [n, 5]; std / offdiag: the two
    transforms (numpy on the host, LogitMVN's on the device)."""
    e_so, e_sd, c = np.exp(std(q[:, 1])), np.exp(std(q[:, 3])), offdiag(q[:, 4])
    return np.maximum(np.abs(q[:, 0]) + Z_MAX * e_so, np.abs(q[:, 2]) + Z_MAX * (np.abs(c) + e_sd))


@pytest.mark.parametrize("T", [11, 24])
def test_mixed_kl_loops_within_a_tile(params, T):
    """The whitened KL loop is chosen per 16 voxels on both kernels (per wave there, per 16-lane row here).  The
    log-std head biases are raised by a value chosen on the host with the oracle's encoder so that, within one
    64-voxel tile, some 16-voxel groups lie entirely under the reach bound and others do not; the condition is then
    asserted on the device's own posterior parameters, and the two kernels must agree bit for bit."""
    from qbold_vi_amd.logit_mvn import LogitMVN
    from qbold_vi_amd.ops import EncoderWeights
    ctx, orc, w, x, mask, prior = small_case(params, T)
    q0 = np.asarray(orc.encoder_fwd(w, x)[1], np.float64)
    best = None
    for delta in np.arange(0.0, 3.0, 0.01):
        q = q0.copy()
        q[:, 1] += delta
        q[:, 3] += delta
        r = reach_of(q, lambda p: np.tanh(p) * 3.0 - 1.0, lambda p: np.tanh(p) * np.exp(-2.0))
        gmax = r[:192].reshape(3, 4, 16).max(2)            # [tile][group]: the group takes the whitened loop iff < clip
        for t in range(3):
            under = gmax[t] < LOGIT_CLIP
            margin = float(np.abs(np.log(gmax[t] / LOGIT_CLIP)).min())
            if 0 < int(under.sum()) < 4 and (best is None or margin > best[0]):
                best = (margin, float(delta), t)
    assert best is not None, "no bias shift mixes the KL loops within a tile"
    margin, delta, tile = best
    assert margin > 1e-3     # far beyond what float32 rounding of the encoder moves the reach by
    w2 = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in w.items()}
    w2["bf"][1] += np.float32(delta)
    w2["bf"][3] += np.float32(delta)
    ew = EncoderWeights(ctx, T, 60, 2, True, -3.0).set_from_arrays(w2)
    xd, md, pd = dev(x), dev(mask), dev(prior)
    a = run(ctx, FOUR_LANE, ew, xd, md, pd, 32, 70, seed=5)
    b = run(ctx, WHOLE_TILES, ew, xd, md, pd, 32, 70, seed=5)
    lm = LogitMVN(ctx)
    r = reach_of(b[1].cpu().numpy().astype(np.float64), lambda p: lm.transform_std(dev(p.astype(np.float32))).cpu().numpy().astype(np.float64),
                 lambda p: lm.transform_offdiag(dev(p.astype(np.float32))).cpu().numpy().astype(np.float64))
    under = r[64 * tile:64 * tile + 64].reshape(4, 16).max(1) < LOGIT_CLIP
    print(f"T={T}: bias shift {delta:.2f}, tile {tile}, groups under the reach bound: {under.tolist()}, margin {margin:.3e}")
    assert 0 < int(under.sum()) < 4
    assert bool(torch.isfinite(a[2]).all())
    assert_same(a, b, (T, delta))


@pytest.mark.parametrize("T", [11, 24])
def test_default_dispatch_two_ranges(params, T):
    """One balanced round of 64-voxel tiles on every wave of the device plus 16 * 3 + 5 voxels: the default dispatch
    runs the new kernel on the round and the four-lane kernel on the remainder, at its offsets, and adds the two
    launches' partial sums slot by slot.  The small case's rows, repeated; voxel0 keeps the draws apart."""
    from qbold_vi_amd.ops import EncoderWeights
    ctx, orc, w, x, mask, prior = small_case(params, T)
    waves = torch.cuda.get_device_properties(0).multi_processor_count * ((768 if T == 24 else 1024) // 64)
    n = 64 * waves + 16 * 3 + 5
    idx = np.arange(n) % N_SMALL
    xd, md, pd = dev(x[idx]), dev(mask[idx]), dev(prior[idx])
    ew = EncoderWeights(ctx, T, 60, 2, True, -3.0).set_from_arrays(w)
    a = run(ctx, FOUR_LANE, ew, xd, md, pd, 5, 9, seed=3, voxel0=77)
    b = run(ctx, 0, ew, xd, md, pd, 5, 9, seed=3, voxel0=77)
    b2 = run(ctx, 0, ew, xd, md, pd, 5, 9, seed=3, voxel0=77)
    assert bool(torch.isfinite(a[2]).all())
    assert_same(a, b, (T, n))
    assert torch.equal(b[0], b2[0])
