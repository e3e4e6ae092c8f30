"""The float64 reference of the training backward (tests/_train_bwd_reference.py) against the C oracle: its forward
equals qbo_encoder_fwd / qbo_encoder_fwd_spatial, its VJP equals central differences of the float64 oracle (random
directions and single off-centre taps that reach crop borders), and the per-tensor comparison the GPU tests use
rejects planted kernel defects while it accepts a float32 evaluation of the same reference.  CPU only."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _train_bwd_reference as ref  # noqa: E402

EPS = ref.EPS   # the GPU tests' per-tensor tolerance (max |hip - ref| <= EPS max |ref|)


def weights(U, L, cw, seed, taps=9, gate_offset=-3.0):
    from oracle.oracle import init_weights
    w = init_weights(T=11, U=U, L=L, channelwise_gating=cw, seed=seed, taps=taps, resid_init_std=0.08)
    rng = np.random.default_rng(seed)
    for k in ("b0", "bc", "br1", "br2", "bg", "bf"):
        w[k] = (rng.standard_normal(w[k].shape) * 0.1).astype(np.float32)
    w["gate_offset"] = gate_offset
    return w


def crops(oracle, B, X, Y, Z, seed):
    from oracle.oracle import synth_inputs
    x, _ = synth_inputs(B * X * Y * Z, seed=seed, oracle=oracle)
    return x.reshape(B, X, Y, Z, 11).astype(np.float64)


@pytest.mark.parametrize("U,L,cw", [(60, 2, True), (20, 1, False), (33, 2, True)])
def test_forward_equals_oracle(oracle64, U, L, cw):
    w = weights(U, L, cw, seed=3)
    xv = crops(oracle64, 1, 1, 1, 40, seed=2).reshape(-1, 11)
    o1, o2, sg = oracle64.encoder_fwd(w, xv)
    q2, ls = ref.outputs(w, xv, se_idx=oracle64.se_idx)
    q1, _ = ref.outputs(w, xv, stream=1, se_idx=oracle64.se_idx)
    for got, want in ((q2, o2), (ls, np.log(sg)), (q1, o1)):
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    x = crops(oracle64, 3, 5, 4, 2, seed=4)
    o2, sg = oracle64.encoder_fwd_spatial(w, x)
    q2, ls = ref.outputs(w, x, se_idx=oracle64.se_idx)
    assert np.abs(q2 - o2).max() <= 1e-12 * np.abs(o2).max()
    assert np.abs(ls - np.log(sg)).max() <= 1e-12 * np.abs(np.log(sg)).max()
    # the neighbourhood matters (the crop forward is not the voxel-wise one)
    assert np.abs(q2.reshape(-1, 5) - ref.outputs(w, x.reshape(-1, 11), se_idx=oracle64.se_idx)[0]).max() > 1e-3


def _oracle_loss(oracle64, w, x, g_q, g_ls, stream, s):
    if x.ndim == 5:
        o2, sg = oracle64.encoder_fwd_spatial(w, x)
        q, ls = o2.reshape(-1, 5), np.log(sg).reshape(-1, 11)
    else:
        o1, o2, sg = oracle64.encoder_fwd(w, x)
        q, ls = (o1, None) if stream == 1 else (o2, np.log(sg))
    v = (q * g_q).sum()
    if ls is not None:
        v += (ls * g_ls).sum()
    return v / s


def _fd(oracle64, w, x, g_q, g_ls, stream, s, direction, h=1e-6):
    wp = {k: (np.asarray(w[k], np.float64) + h * direction[k]) if k in direction else w[k] for k in w}
    wm = {k: (np.asarray(w[k], np.float64) - h * direction[k]) if k in direction else w[k] for k in w}
    return (_oracle_loss(oracle64, wp, x, g_q, g_ls, stream, s) - _oracle_loss(oracle64, wm, x, g_q, g_ls, stream, s)) / (2 * h)


@pytest.mark.parametrize("case", ["voxel2", "voxel1", "crop"])
def test_vjp_equals_oracle_central_differences(oracle64, case):
    rng = np.random.default_rng(7)
    U, L = 20, 2
    w = weights(U, L, True, seed=5, taps=9)
    if case == "crop":   # 4 x 3 crops: every off-centre tap reaches a border of some voxel
        x = crops(oracle64, 2, 4, 3, 2, seed=6)
    else:
        x = crops(oracle64, 1, 1, 1, 30, seed=6).reshape(-1, 11)
    stream = 1 if case == "voxel1" else 2
    n = x.size // 11
    g_q = rng.standard_normal((n, 5))
    g_ls = None if stream == 1 else rng.standard_normal((n, 11))
    sums = [0.0, 0.0, 3.0]
    grads, _, _ = ref.vjp(w, x, g_q, g_ls, sums, stream=stream, se_idx=oracle64.se_idx)
    dirs = [{k: rng.standard_normal(np.shape(w[k])) for k in ref.NAMES} for _ in range(3)]
    if case == "crop":
        for (i, j) in ((0, 0), (2, 1), (1, 2), (0, 2)):   # single off-centre taps, one entry each
            for name in ("Wr1", "Wr2"):
                d = {k: np.zeros(np.shape(w[k])) for k in ref.NAMES}
                d[name][1, i, j, 3, 5] = 1.0
                dirs.append(d)
    for d in dirs:
        want = _fd(oracle64, w, x, g_q, g_ls, stream, sums[2], d)
        got = sum(float((grads[k] * d[k]).sum()) for k in ref.NAMES)
        assert abs(got - want) <= 1e-7 * max(abs(want), 1e-2 * max(abs(float(np.abs(grads[k]).max())) for k in grads)), \
            (got, want)


def _worst(got, want, bias_abs):
    return max(ref.error_ratios(got, want, bias_abs).values())


@pytest.mark.parametrize("U,L,geom", [(60, 2, (2, 9, 8, 4)), (20, 1, (3, 6, 5, 4))])
def test_comparison_has_teeth(oracle64, U, L, geom):
    """The GPU tests' per-tensor tolerance EPS rejects a backward whose 3x3 products see the deltas as an f16 high half
    only (a split that lost its lo half) and one that drops an off-centre tap at a crop border, each by at least 10x;
    it accepts the torch float32 evaluation of the same reference."""
    rng = np.random.default_rng(11)
    w = weights(U, L, True, seed=8)
    x = crops(oracle64, *geom, seed=9)
    n = x.size // 11
    g_q, g_ls = rng.standard_normal((n, 5)), rng.standard_normal((n, 11))
    sums = [0.0, 0.0, float(n)]
    want, pre, bias_abs = ref.vjp(w, x, g_q, g_ls, sums, se_idx=oracle64.se_idx)
    f32, _, _ = ref.vjp(w, x, g_q, g_ls, sums, se_idx=oracle64.se_idx, dtype=torch.float32)
    hi, _, _ = ref.vjp(w, x, g_q, g_ls, sums, se_idx=oracle64.se_idx, hi_only_deltas=True)
    drop, _, _ = ref.vjp(w, x, g_q, g_ls, sums, se_idx=oracle64.se_idx, drop_border_tap=True)
    assert _worst(f32, want, bias_abs) <= EPS / 4
    assert _worst(hi, want, bias_abs) >= 10 * EPS
    assert _worst(drop, want, bias_abs) >= 10 * EPS


def test_relu_screen_keeps_most_voxels(oracle64):
    """The screen that makes the GPU comparison immune to relu flips removes few voxels at the optimal.yaml shape."""
    w = weights(60, 2, True, seed=8)
    x = crops(oracle64, 2, 12, 10, 4, seed=9)
    n = x.size // 11
    _, pre, _ = ref.vjp(w, x, np.ones((n, 5)), np.ones((n, 11)), se_idx=oracle64.se_idx)
    keep = ref.keep_mask(ref.relu_sites_near_zero(pre), x.shape[:4])
    assert keep.mean() >= 0.8
    # the dilation is Chebyshev `reach` in x / y, within one batch element and z slice
    reach = np.full(x.shape[:4], -1)
    reach[1, 0, 0, 2] = 2
    reach[0, 5, 5, 1] = 0
    k = ref.keep_mask(reach.reshape(-1), x.shape[:4]).reshape(x.shape[:4])
    assert (~k).sum() == 10 and not k[1, :3, :3, 2].any() and not k[0, 5, 5, 1] and k[1, :, :, 1].all()
