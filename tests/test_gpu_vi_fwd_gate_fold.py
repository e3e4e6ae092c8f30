"""The fused ELBO kernels on the folded gate ops (qbold_vi_fwd_folded; ops.vi_fwd(fold_gate=True)) against the classic
entry (qbold_vi_fwd; fold_gate=False) and against the float64 oracle encoder.

A block's gate logits Wg r + bg + gate_offset, r = Wr2 relu(t) + br2, are (Wr2 Wg) relu(t) + (br2 Wg + bg +
gate_offset): the folded kernels take them from relu(t)'s fragments through the product matrix, which
qbold_encoder_pack_gatefold forms once.  Results move by the one float32 rounding of that product, so the two entries
are held to each other by the project's bounds for fused against layer-wise (MEASUREMENTS 2): q 2e-5, (nll, kl) 1e-4 of
1 + |.|, -ELBO 1e-4 relative.  Against the float64 oracle the folded q may be at most twice as far as the classic q is
in the same test (the factor two: one extra rounding; a CPU emulation of the split arithmetic gave a ratio of 1.0).

Every case: N = 213 under QBOLD_KSEL_VI_WHOLE_TILES -- three 64-voxel tiles on the one-lane-per-voxel kernel, one full
16-voxel tile and a ragged five on the four-lane kernel --, S = 5, K = 6, a mask with zeros.  The bf16 encoder has no
folded kernel (there the product's rounding is bf16's own, 1e-3 on q: not the same results); its cases run the same
comparisons through the entry's fallback."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_gpu_vi_fwd_shared_prologue import PROTOCOLS, dev  # noqa: E402

pytestmark = pytest.mark.gpu

FOUR_LANE = 16777216     # QBOLD_KSEL_VI_FOUR_LANE
WHOLE_TILES = 33554432   # QBOLD_KSEL_VI_WHOLE_TILES
N = 64 * 3 + 21
S, K = 5, 6

# T, L, channel-wise gate, gate_offset, precision, spatial_taps
CASES = [
    (11, 2, True, -3.0, "f32", 1),
    (11, 2, False, 0.0, "f32", 1),
    (11, 1, True, 0.0, "f32", 1),
    (11, 1, False, -3.0, "f32", 1),
    (24, 2, True, -3.0, "f32", 1),
    (24, 2, False, 0.0, "f32", 1),
    (11, 2, True, -3.0, "f32", 9),
    (11, 2, True, -3.0, "bf16", 1),
    (24, 2, False, 0.0, "bf16", 1),
    (11, 1, True, 0.0, "bf16", 1),
]

_inputs = {}
_weights = {}


def inputs(params, T):
    """Context, float64 oracle, signals, mask and prior of a protocol: made once, never modified."""
    if T not in _inputs:
        from oracle.oracle import Oracle, synth_inputs
        from qbold_vi_amd.ops import Context
        p = dict(params, **PROTOCOLS[T][0])
        ctx = Context(p, full_model=True, include_blood=True)
        orc = Oracle("f64", p)
        assert ctx.T == orc.T == T
        x, _ = synth_inputs(N, p, seed=31, oracle=Oracle("f32", p))
        rng = np.random.default_rng(131)
        mask = (rng.uniform(size=N) > 0.35).astype(np.float32)
        mask[N - 1], mask[N - 2], mask[70], mask[0] = 0.0, 1.0, 0.0, 1.0   # zeros in the remainder and in a whole tile
        prior = (rng.standard_normal((N, 5)) * 0.3).astype(np.float32)
        _inputs[T] = (ctx, orc, np.asarray(x, np.float32), mask, prior)
    return _inputs[T]


def weights(T, L, cw, gate_offset, taps):
    key = (T, L, cw, gate_offset, taps)
    if key not in _weights:
        from oracle.oracle import init_weights
        w = init_weights(T=T, U=60, L=L, channelwise_gating=cw, seed=41 + L, taps=taps)
        rng = np.random.default_rng(141)
        for name in ("b0", "bc", "br1", "br2", "bg", "bf"):
            w[name] = (rng.standard_normal(w[name].shape) * 0.1).astype(np.float32)
        w["gate_offset"] = gate_offset
        _weights[key] = w
    return _weights[key]


def run(ctx, sel, *args, **kw):
    ctx.set_kernel_selection(sel)
    try:
        return ctx.vi_fwd(*args, **kw)
    finally:
        ctx.set_kernel_selection(0)


def neg_elbo(sums):
    return float((sums[0] + sums[1]) / sums[2])


@pytest.mark.parametrize("T,L,cw,gate_offset,precision,taps", CASES)
def test_folded_against_classic_and_oracle(params, T, L, cw, gate_offset, precision, taps):
    from qbold_vi_amd.ops import EncoderWeights
    ctx, orc, x, mask, prior = inputs(params, T)
    w = weights(T, L, cw, gate_offset, taps)
    ew = EncoderWeights(ctx, T, 60, L, cw, gate_offset, spatial_taps=taps, precision=precision).set_from_arrays(w)
    xd, md, pd = dev(x), dev(mask), dev(prior)
    assert 0 < int((mask == 0).sum()) < N
    fold = run(ctx, WHOLE_TILES, ew, xd, md, pd, S, K, seed=4, fold_gate=True)
    classic = run(ctx, WHOLE_TILES, ew, xd, md, pd, S, K, seed=4, fold_gate=False)
    (sf, qf, nkf), (sc, qc, nkc) = fold, classic
    assert bool(torch.isfinite(nkf).all()) and bool(torch.isfinite(qf).all()) and bool(torch.isfinite(sf).all())
    dq = float((qf - qc).abs().max())
    dnk = float(((nkf - nkc).abs() / (1.0 + nkc.abs())).max())
    de = abs(neg_elbo(sf) / neg_elbo(sc) - 1.0)
    print(f"T={T} L={L} G={'U' if cw else 1} offset={gate_offset} {precision} taps={taps}: folded vs classic "
          f"max|dq|={dq:.3e} max|d(nll,kl)|/(1+|.|)={dnk:.3e} -ELBO rel {de:.3e} "
          f"bitwise={bool(torch.equal(qf, qc) and torch.equal(nkf, nkc))}")
    if precision == "f32":
        q64 = np.asarray(orc.encoder_fwd(w, x)[1], np.float64)
        ef = float(np.abs(qf.cpu().numpy().astype(np.float64) - q64).max())
        ec = float(np.abs(qc.cpu().numpy().astype(np.float64) - q64).max())
        print(f"    against the float64 oracle: folded max|dq|={ef:.3e}, classic {ec:.3e}, ratio {ef / ec:.2f}")
    assert dq <= 2e-5
    assert dnk <= 1e-4
    assert de <= 1e-4
    if precision == "f32":
        assert not torch.equal(qf, qc)      # the folded kernels did run
        assert ef <= 2.0 * ec
    # the same voxels through the four-lane kernel: the same bits
    four = run(ctx, FOUR_LANE, ew, xd, md, pd, S, K, seed=4, fold_gate=True)
    assert np.array_equal(four[1].cpu().numpy(), qf.cpu().numpy())
    assert np.array_equal(four[2].cpu().numpy(), nkf.cpu().numpy())
    assert float(four[0][2]) == float(sf[2]) == float(md.sum())
    # the sums are deterministic
    again = run(ctx, WHOLE_TILES, ew, xd, md, pd, S, K, seed=4, fold_gate=True)
    assert torch.equal(again[0], sf)


@pytest.mark.parametrize("T", [11, 24])
def test_activation_beyond_the_operand_range(params, T):
    """One voxel whose activations pass 65504 (the hot voxel of tests/test_gpu_vi_fwd_shared_prologue.py, in sub-tile 2
    of 64-voxel tile 1): NaN on both entries, and only there."""
    from qbold_vi_amd.ops import EncoderWeights
    ctx, orc, x, mask, prior = inputs(params, T)
    w = weights(T, 2, True, -3.0, 1)
    hot = 64 + 16 * 2 + 6
    x, mask = x.copy(), mask.copy()
    x[hot] = 1e8
    x[hot, ctx.se_idx] = 1e-2
    mask[hot] = 1.0
    xd, md, pd = dev(x), dev(mask), dev(prior)

    def scaled(sc):   # hidden activations scale with sc (the layers are positively homogeneous), the heads undo it
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
    for fold_gate in (True, False):
        for sel in (WHOLE_TILES, FOUR_LANE):
            sums, q, nk = run(ctx, sel, ew, xd, md, pd, S, K, seed=7, fold_gate=fold_gate)
            bad = torch.isnan(nk[:, 0])
            assert bool(bad[hot]) and int(bad.sum()) == 1, (fold_gate, sel, int(bad.sum()))
            assert bool(torch.isfinite(nk[~bad]).all())
            assert not bool(torch.isfinite(sums[0]))
            assert float(sums[2]) == float(md.sum())


def test_folded_weight_beyond_the_operand_range(params):
    """One row of Wr2 and the matching column of Wg at 300: every weight splits, the product 60 x 300 x 300 x log2(e)
    does not.  The fold buffer's own flag slot carries it: every voxel NaN on the folded entry, finite on the classic."""
    from qbold_vi_amd.ops import EncoderWeights
    ctx, orc, x, mask, prior = inputs(params, 11)
    w = weights(11, 2, True, -3.0, 1)
    w2 = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in w.items()}
    w2["Wr2"][1, 5, :] = 300.0
    w2["Wg"][1, :, 9] = 300.0
    assert 60 * 300.0 * 300.0 * 1.4426950408889634 > 65504.0
    ew = EncoderWeights(ctx, 11, 60, 2, True, -3.0).set_from_arrays(w2)
    xd, md, pd = dev(x), dev(mask), dev(prior)
    for sel in (WHOLE_TILES, FOUR_LANE):
        sums, q, nk = run(ctx, sel, ew, xd, md, pd, S, K, seed=7, fold_gate=True)
        assert bool(torch.isnan(nk[:, 0]).all()) and not bool(torch.isfinite(sums[0]))
        sums, q, nk = run(ctx, sel, ew, xd, md, pd, S, K, seed=7, fold_gate=False)
        assert bool(torch.isfinite(nk).all()) and bool(torch.isfinite(sums).all())
    flag = float(ew.gate_fold[2 * 4160])
    assert flag > 65504.0 and float(ew.packed[-4:].max()) == 0.0   # in the fold's flag slot, not in the image's


def test_off_grid_context_falls_back_to_the_classic_path(params):
    """tau_start = -0.017: no per-tau table, so no folded kernel -- qbold_vi_fwd_folded is qbold_vi_fwd, bit for bit."""
    from qbold_vi_amd import _lib
    from qbold_vi_amd.ops import Context, EncoderWeights, _ptr, _stream
    p = dict(params, tau_start="-0.017", tau_end="0.071", tau_step="0.008")
    ctx = Context(p, full_model=True, include_blood=True)
    assert ctx.T == 11
    _, _, x, mask, prior = inputs(params, 11)
    w = weights(11, 2, True, -3.0, 1)
    ew = EncoderWeights(ctx, 11, 60, 2, True, -3.0).set_from_arrays(w)
    xd, md, pd = dev(x), dev(mask), dev(prior)
    out = []
    for folded in (True, False):
        sums = torch.empty(3, dtype=torch.float64, device="cuda")
        q = torch.empty((N, 5), dtype=torch.float32, device="cuda")
        nk = torch.empty((N, 2), dtype=torch.float32, device="cuda")
        head = (ctx.handle, C.byref(ew.shape), ew.packed_ptr())
        tail = (_ptr(xd), _ptr(md), _ptr(pd), S, K, 4, 0, _ptr(q), _ptr(nk), _ptr(sums), _ptr(ctx._workspace()), N,
                _stream())
        if folded:
            _lib.check(ctx.lib.qbold_vi_fwd_folded(*head, ew.gate_fold_ptr(), *tail), "qbold_vi_fwd_folded")
        else:
            _lib.check(ctx.lib.qbold_vi_fwd(*head, *tail), "qbold_vi_fwd")
        out.append((sums, q, nk))
    (sa, qa, nka), (sb, qb, nkb) = out
    assert bool(torch.isfinite(nka).all())
    assert torch.equal(qa, qb) and torch.equal(nka, nkb) and torch.equal(sa, sb)
