"""The one-lane-per-voxel fused kernels (vi_fwd_kernel_vox, vi_fwd_kernel_vox_fold) with the per-lane front end
(first_operand: a lane loads and normalises only the spin echo and the eight signals it feeds the first layer) and the
head hand-over by one transpose per tile (keep_head_tile, transpose_heads), against the four-lane kernels, which keep
normalise, dense_first and gather_head: the independent comparator.  Both changes move or skip work without changing
any arithmetic, so q and (nll, kl) -- nothing else is compared -- are held to bitwise equality (NaNs equal) between

  QBOLD_KSEL_VI_WHOLE_TILES  every whole 64-voxel tile on the changed kernels, the remainder on the four-lane ones
  QBOLD_KSEL_VI_FOUR_LANE    every voxel on the four-lane kernels

for (T, L) = (11, 2), (11, 1), (24, 2), the split-f16 encoder on the folded and on the classic image and the bf16
encoder, at N = 64 (one tile, every voxel distinct: a wrong transpose swaps rows), N = 229 (three whole tiles and a
ragged four-lane remainder) and N = 1; S = 4, K = 8.  The inputs hit both ends of the clamp (signals <= 0 and >= 1e9,
in the first and the last window of a row and at the spin echo itself) in every sub-tile of the first tile, and one
voxel carries a NaN signal: its nll is non-finite on both paths and every other voxel keeps its bits."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_gpu_vi_fwd_shared_prologue import PROTOCOLS, dev  # noqa: E402

pytestmark = pytest.mark.gpu

FOUR_LANE = 16777216     # QBOLD_KSEL_VI_FOUR_LANE
WHOLE_TILES = 33554432   # QBOLD_KSEL_VI_WHOLE_TILES
N_ALL = 64 * 3 + 37      # three whole tiles, two whole 16-voxel tiles and a ragged five
S, K = 4, 8
NAN_VOXEL = 62           # sub-tile 3 of the first tile

_inputs = {}
_weights = {}


def inputs(params, T):
    """Context, signals, mask and prior of a protocol: made once, never modified."""
    if T not in _inputs:
        from oracle.oracle import Oracle, synth_inputs
        from qbold_vi_amd.ops import Context
        p = dict(params, **PROTOCOLS[T][0])
        ctx = Context(p, full_model=True, include_blood=True)
        assert ctx.T == T
        x, _ = synth_inputs(N_ALL, p, seed=57, oracle=Oracle("f32", p))
        x = np.array(x, np.float32)
        assert len(np.unique(x, axis=0)) == N_ALL      # every voxel distinct
        se = ctx.se_idx
        edge = [t for t in (0, 1, T - 2, T - 1) if t != se]
        x[0, edge[0]], x[0, edge[-1]] = -1.0, 2e9      # row 0 alone is the N = 1 case: both clamp ends
        x[5, edge[0]], x[5, edge[2]] = 0.0, -3.0       # sub-tile 0: signals <= 0 in the first and the last window
        x[21, edge[1]], x[21, edge[3]] = 1e9, 3e9      # sub-tile 1: signals >= 1e9
        x[40, se] = -0.5                               # sub-tile 2: the spin echo itself below the clamp
        x[55, se] = 4e9                                # sub-tile 3: ... and above it
        x[NAN_VOXEL, T - 2] = np.nan
        x[64 + 16 + 3, edge[3]], x[200, edge[0]] = 5e9, -2.0    # a later tile and the four-lane remainder
        rng = np.random.default_rng(157)
        mask = (rng.uniform(size=N_ALL) > 0.3).astype(np.float32)
        mask[0], mask[70], mask[N_ALL - 1] = 1.0, 0.0, 0.0
        prior = (rng.standard_normal((N_ALL, 5)) * 0.3).astype(np.float32)
        _inputs[T] = (ctx, x, mask, prior)
    return _inputs[T]


def weights(T, L):
    if (T, L) not in _weights:
        from oracle.oracle import init_weights
        w = init_weights(T=T, U=60, L=L, channelwise_gating=True, seed=61 + L)
        rng = np.random.default_rng(161)
        for name in ("b0", "bc", "br1", "br2", "bg", "bf"):
            w[name] = (rng.standard_normal(w[name].shape) * 0.1).astype(np.float32)
        w["gate_offset"] = -3.0
        _weights[(T, L)] = w
    return _weights[(T, L)]


def run(ctx, sel, *args, **kw):
    ctx.set_kernel_selection(sel)
    try:
        return ctx.vi_fwd(*args, **kw)
    finally:
        ctx.set_kernel_selection(0)


def same_bits(a, b):
    """torch.equal with NaNs compared as equal."""
    na, nb = torch.isnan(a), torch.isnan(b)
    zero = torch.zeros_like(a)
    return torch.equal(na, nb) and torch.equal(torch.where(na, zero, a), torch.where(nb, zero, b))


@pytest.mark.parametrize("precision,fold_gate", [("f32", True), ("f32", False), ("bf16", True)])
@pytest.mark.parametrize("T,L", [(11, 2), (11, 1), (24, 2)])
def test_whole_tiles_same_bits_as_four_lane(params, T, L, precision, fold_gate):
    from qbold_vi_amd.ops import EncoderWeights
    ctx, x, mask, prior = inputs(params, T)
    ew = EncoderWeights(ctx, T, 60, L, True, -3.0, precision=precision).set_from_arrays(weights(T, L))
    for n in (64, N_ALL, 1):
        xd, md, pd = dev(x[:n]), dev(mask[:n]), dev(prior[:n])
        _, qa, nka = run(ctx, FOUR_LANE, ew, xd, md, pd, S, K, seed=9, fold_gate=fold_gate)
        _, qb, nkb = run(ctx, WHOLE_TILES, ew, xd, md, pd, S, K, seed=9, fold_gate=fold_gate)
        what = (T, L, precision, fold_gate, n)
        # untouched voxels are finite; the NaN signal reaches its voxel's nll on both paths
        plain = torch.as_tensor(np.isfinite(x[:n]).all(1) & (x[:n] > 0).all(1), device="cuda")
        assert bool(torch.isfinite(nka[plain]).all()) and bool(torch.isfinite(qa).all()), what
        if n > NAN_VOXEL:
            assert not bool(torch.isfinite(nka[NAN_VOXEL, 0])) and not bool(torch.isfinite(nkb[NAN_VOXEL, 0])), what
        bad_q = (~((qa == qb) | (torch.isnan(qa) & torch.isnan(qb)))).any(1).nonzero().flatten().tolist()
        bad_nk = (~((nka == nkb) | (torch.isnan(nka) & torch.isnan(nkb)))).any(1).nonzero().flatten().tolist()
        print(f"T={T} L={L} {precision} fold_gate={fold_gate} N={n}: voxels that differ in q {bad_q[:8]}, "
              f"in (nll, kl) {bad_nk[:8]}; non-finite nll at {(~torch.isfinite(nka[:, 0])).nonzero().flatten().tolist()}")
        assert same_bits(qa, qb), what
        assert same_bits(nka, nkb), what
