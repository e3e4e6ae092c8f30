"""The folded gate ops of the fused ELBO kernels (qbold_encoder_pack_gatefold), read back from the device: per block one
dense op in the layout of the weight image's ops,

  A[k-step s][m][part = hi, lo][lane][j] f16 = -log2(e) (Wr2 Wg)[in = unit(s, lane >> 4, j)][out = 16 m + (lane & 15)]
  bias[m][group][reg] f32                    = -log2(e) (br2 Wg + bg + gate_offset)[16 m + 4 group + reg]

against the same product in numpy float64, for a full-width and a narrow encoder (U = 60, U = 7), the channel-wise and
the shared gate (G = U, G = 1), one and two blocks, and 9-tap residual kernels (the centre tap is the one folded).

Bounds, from the number formats.  An element is the float64 product rounded once to float32 (2^-24 relative), then
split: hi = f16(v) leaves a residual of at most 2^-11 |v|, lo = f16(2^11 (v - hi)) leaves 2^-11 of that, 2^-22 |v|; lo
in the f16 subnormals (elements below ~6e-5) is spaced 2^-24, which is 2^-36 after the 2^-11 scale.  So
|hi + 2^-11 lo - v| <= 2^-21 |v| + 2^-36.  A bias is the float64 sum rounded once: one float32 ulp, 2^-23 relative,
allows for the last bits of the two float64 summation orders."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
OP = 4160   # floats per folded op: 4096 of fragments, 64 of bias


def frag_coords():
    """(in, out) unit of every half h = j + 8 lane + 512 part + 1024 m + 4096 s of an op's fragments, and its part."""
    h = np.arange(8192)
    j, lane, part, m, s = h & 7, (h >> 3) & 63, (h >> 9) & 1, (h >> 10) & 3, h >> 12
    return 16 * (2 * s + (j >> 2)) + 4 * (lane >> 4) + (j & 3), 16 * m + (lane & 15), part


@pytest.mark.parametrize("U,L,channelwise,taps,gate_offset", [
    (60, 2, True, 1, -3.0), (60, 2, False, 1, 0.0), (7, 1, True, 1, 0.0), (7, 2, False, 1, -3.0), (60, 1, True, 9, -3.0)])
def test_folded_gate_ops_match_float64_product(params, U, L, channelwise, taps, gate_offset):
    from qbold_vi_amd.init import init_encoder_weights
    from qbold_vi_amd.ops import Context, EncoderWeights
    ctx = Context(params, full_model=True, include_blood=True)
    w = init_encoder_weights(T=11, U=U, L=L, channelwise_gating=channelwise, seed=5, spatial_taps=taps)
    rng = np.random.default_rng(6)
    for name in ("br2", "bg"):
        w[name] = (rng.standard_normal(w[name].shape) * 0.3).astype(np.float32)
    ew = EncoderWeights(ctx, 11, U, L, channelwise, gate_offset, spatial_taps=taps).set_from_arrays(w)
    ew.gate_fold_ptr()
    torch.cuda.synchronize()
    fold = ew.gate_fold.cpu().numpy()
    assert fold.size == L * OP + 4 == int(ctx.lib.qbold_encoder_gatefold_floats(C.byref(ew.shape)))
    assert np.all(fold[L * OP:] == 0.0)          # the flag (no folded weight beyond the f16 range) and the padding
    fin, fout, part = frag_coords()
    worst_a = worst_b = 0.0
    for l in range(L):
        wr2 = w["Wr2"][l].astype(np.float64)
        if taps == 9:
            wr2 = wr2[1, 1]
        wg = w["Wg"][l].astype(np.float64)
        bg = w["bg"][l].astype(np.float64)
        if not channelwise:                      # one gate for all units
            wg, bg = np.repeat(wg, U, axis=1), np.repeat(bg, U)
        want = np.zeros((64, 64))
        want[:U, :U] = -LOG2E * (wr2 @ wg)
        want_b = np.zeros(64)
        want_b[:U] = -LOG2E * (w["br2"][l].astype(np.float64) @ wg + bg + gate_offset)
        op = fold[l * OP:(l + 1) * OP]
        halves = op[:4096].view(np.float16).astype(np.float64)
        hi, lo = halves[part == 0], halves[part == 1]
        i, o = fin[part == 0], fout[part == 0]
        assert np.array_equal(i, fin[part == 1]) and np.array_equal(o, fout[part == 1])
        got = np.zeros((64, 64))
        got[i, o] = hi + lo / 2048.0
        pad = (i >= U) | (o >= U)
        assert np.all(hi[pad] == 0.0) and np.all(lo[pad] == 0.0)
        err = np.abs(got - want)
        assert np.all(err <= 2.0 ** -21 * np.abs(want) + 2.0 ** -36), (l, float(err.max()))
        worst_a = max(worst_a, float((err / np.maximum(np.abs(want), 1e-3)).max()))
        # bias [m][group][reg] holds unit 16 m + 4 group + reg: the natural order
        got_b = op[4096:].astype(np.float64)
        assert np.all(got_b[U:] == 0.0)
        errb = np.abs(got_b - want_b)
        assert np.all(errb <= 2.0 ** -23 * np.abs(want_b)), (l, float(errb.max()))
        worst_b = max(worst_b, float((errb / np.maximum(np.abs(want_b), 1e-30)).max()))
    print(f"U={U} L={L} G={'U' if channelwise else 1} taps={taps}: fragments {worst_a:.2e} of max(|v|, 1e-3), "
          f"bias {worst_b:.2e} relative")
