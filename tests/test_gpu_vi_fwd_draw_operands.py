"""The one-lane-per-voxel fused kernels whose likelihood draws read their wave-uniform operands from vector registers
(voxel_mc_sums<.., DREGS>, LikRegs, elbo_core.h / qbold_dev.h: the blood brackets of the evaluated taus, fwd_fast_sig's
constants, 0.8 and 0.04) against the four-lane kernels, which this change does not touch: the independent comparator.
Only the place an operand is read from moves, so q and (nll, kl) are held to bitwise equality (NaNs equal) between

  QBOLD_KSEL_VI_WHOLE_TILES  every whole 64-voxel tile on the one-lane-per-voxel kernels, the remainder on the four-lane ones
  QBOLD_KSEL_VI_FOUR_LANE    every voxel on the four-lane kernels

for (T, L) = (11, 2), (24, 2), (11, 1); the split-f16 encoder on the folded image, on the classic image (switched on at
(24, 2) and (11, 1), switched off at (11, 2), the one instance without the registers) and the bf16 encoder; draw counts
that reach every edge of both loops -- (S, K) = (32, 70): whole likelihood calls on all four shares and a short last KL
call; (5, 3): one short call in either stream and empty shares; (17, 9) -- at N = 64, 229 and 1, with a seed whose high
word is not zero and voxel0 = 2^32 - 32, so that the high word of the Philox counter changes inside the first tile.

One more case mixes the two KL loops in one wave.  It was written for registers of the whitened KL loop, which were
measured slower and are not in the library (MEASUREMENTS 34): the KL loops it runs are the parent's, and what it holds
for this change is that the likelihood registers leave a wave with both KL paths behind them as it was.  The head
biases belong to the network, not to a voxel, so log-std biases of +3 (bench.py's wide_posterior) would send every row
to the general loop; a smaller bias leaves some voxels' draws short of the logit clip (the whitened loop) and others
beyond it (the general loop).  A 64-voxel tile is assembled from both kinds so that rows 0 and 2 of the wave are whitened
and rows 1 and 3 hold voxels of the general loop; which voxel is which is decided from the four-lane kernel's own q with
kl_draws_fast's bound, well clear of the bound on either side, and checked again on the q the compared runs return."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_gpu_vi_fwd_frontend import FOUR_LANE, N_ALL, WHOLE_TILES, inputs, run, same_bits, weights  # noqa: E402
from test_gpu_vi_fwd_shared_prologue import dev  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = (0x5a17 << 32) | 9       # a non-zero high word: both key words count
VOXEL0 = (1 << 32) - 32         # voxel 32 of the first tile is the first with a non-zero high counter word
DRAWS = [(32, 70), (5, 3), (17, 9)]
Z_MAX, LOGIT_CLIP = 4.8549, 13.815509557963774   # QB_Z_MAX, QB_LOGIT_CLIP


def compare(ctx, ew, x, mask, prior, S, K, fold_gate, what):
    xd, md, pd = dev(x), dev(mask), dev(prior)
    _, qa, nka = run(ctx, FOUR_LANE, ew, xd, md, pd, S, K, seed=SEED, voxel0=VOXEL0, fold_gate=fold_gate)
    _, qb, nkb = run(ctx, WHOLE_TILES, ew, xd, md, pd, S, K, seed=SEED, voxel0=VOXEL0, fold_gate=fold_gate)
    bad_q = (~((qa == qb) | (torch.isnan(qa) & torch.isnan(qb)))).any(1).nonzero().flatten().tolist()
    bad_nk = (~((nka == nkb) | (torch.isnan(nka) & torch.isnan(nkb)))).any(1).nonzero().flatten().tolist()
    print(f"{what}: voxels that differ in q {bad_q[:8]}, in (nll, kl) {bad_nk[:8]}; "
          f"finite (nll, kl) rows {int(torch.isfinite(nka).all(1).sum())} of {len(x)}")
    assert int(torch.isfinite(nka).all(1).sum()) >= len(x) - 1, what    # the shared inputs hold one NaN signal
    assert same_bits(qa, qb), what
    assert same_bits(nka, nkb), what
    return qa


@pytest.mark.parametrize("precision,fold_gate", [("f32", True), ("f32", False), ("bf16", True)])
@pytest.mark.parametrize("T,L", [(11, 2), (24, 2), (11, 1)])
def test_draw_loops_same_bits_as_four_lane(params, T, L, precision, fold_gate):
    from qbold_vi_amd.ops import EncoderWeights
    ctx, x, mask, prior = inputs(params, T)
    ew = EncoderWeights(ctx, T, 60, L, True, -3.0, precision=precision).set_from_arrays(weights(T, L))
    for S, K in DRAWS:
        for n in (64, N_ALL, 1):
            compare(ctx, ew, x[:n], mask[:n], prior[:n], S, K, fold_gate,
                    f"T={T} L={L} {precision} fold_gate={fold_gate} S={S} K={K} N={n}")


def kl_reach(q):
    """kl_draws_fast's bound on the logits a voxel's draws can reach, from the raw posterior heads."""
    q = q.astype(np.float64)
    e_so, e_sd = np.exp(3.0 * np.tanh(q[:, 1]) - 1.0), np.exp(3.0 * np.tanh(q[:, 3]) - 1.0)
    c = np.tanh(q[:, 4]) * np.exp(-2.0)
    return np.maximum(np.abs(q[:, 0]) + Z_MAX * e_so, np.abs(q[:, 2]) + Z_MAX * (np.abs(c) + e_sd))


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_whitened_and_general_kl_rows_in_one_wave(params, precision):
    from qbold_vi_amd.ops import EncoderWeights
    T, L, S, K = 11, 2, 5, 70
    ctx, x, mask, prior = inputs(params, T)
    finite = np.isfinite(x).all(1)
    tile = None
    for bias in (0.6, 0.5, 0.7, 0.4, 0.8, 1.0, 0.2):
        w = {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in weights(T, L).items()}
        w["bf"][1] = w["bf"][3] = bias
        ew = EncoderWeights(ctx, T, 60, L, True, -3.0, precision=precision).set_from_arrays(w)
        _, q, _ = run(ctx, FOUR_LANE, ew, dev(x), dev(mask), dev(prior), 1, 4, seed=SEED, fold_gate=True)
        reach = kl_reach(q.cpu().numpy())
        narrow = np.nonzero(finite & (reach < 0.97 * LOGIT_CLIP))[0]
        wide = np.nonzero(finite & (reach > 1.03 * LOGIT_CLIP))[0]
        print(f"{precision} log-std bias {bias}: {len(narrow)} voxels on the whitened side of the bound, {len(wide)} beyond it")
        if len(narrow) >= 24 and len(wide) >= 5:
            # rows 0 and 2: whitened voxels only (the same sixteen inputs; their draws differ with the voxel index);
            # rows 1 and 3: every third lane a voxel of the general loop
            mixed = [wide[j % len(wide)] if j % 3 == 0 else narrow[16 + j % 8] for j in range(16)]
            tile = np.concatenate([narrow[:16], mixed, narrow[:16][::-1], mixed[::-1]])
            break
    assert tile is not None, "no head bias puts voxels on both sides of the KL bound"
    q = compare(ctx, ew, x[tile], mask[tile], prior[tile], S, K, True, f"mixed KL rows, {precision}")
    over = kl_reach(q.cpu().numpy()).reshape(4, 16) >= LOGIT_CLIP
    assert not over[0].any() and not over[2].any() and over[1].any() and over[3].any()
    assert not over[1].all() and not over[3].all()
