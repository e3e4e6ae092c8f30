"""The fused encoder + ELBO kernel (qbold_vi_fwd) against the two-step path on the same heads: qbold_encoder_fwd, then
the stand-alone ELBO entry point (qbold_elbo_fwd) on the posterior parameters and sigmas it wrote.

The cases are the ones that a change to the per-voxel part of the fused kernel (what runs between the encoder and
the draw loops, and after them) can break without the oracle-level sums noticing: both protocols (T = 11 at 1,024
threads, T = 24 at 768), a batch that ends inside a 16-voxel tile, a mask with zeros, and a voxel whose activations
leave the f16 operand range, whose NaN status has to reach its nll and the sums.

Tolerances are those of the existing fused-against-unfused comparisons (tests/test_gpu_parity.py): rtol = atol = 1e-5
on (nll, kl) at T = 11 (test_vi_fwd_fused_matches_oracle), 1e-4 at T = 24 (test_24_tau_protocol); no existing test
establishes bitwise agreement between the two paths (the stand-alone kernel takes sigma, the fused one log sigma), so
none is asserted here.  The posterior parameters are held to the 2e-5 that the existing tests allow against the
oracle."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

PROTOCOLS = {
    11: ({}, 1e-5),
    24: (dict(tau_start="-0.028", tau_end="0.065", tau_step="0.004"), 1e-4),
}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def make_case(params, T, seed):
    from oracle.oracle import Oracle, init_weights, synth_inputs
    from qbold_vi_amd.ops import Context
    over, tol = PROTOCOLS[T]
    p = dict(params, **over)
    orc = Oracle("f32", p)
    ctx = Context(p, full_model=True, include_blood=True)
    assert ctx.T == orc.T == T
    w = init_weights(T=T, U=60, L=2, seed=seed)
    rng = np.random.default_rng(seed + 100)
    for name in ("b0", "bc", "br1", "br2", "bg", "bf"):
        w[name] = (rng.standard_normal(w[name].shape) * 0.1).astype(np.float32)
    w["gate_offset"] = -3.0
    n = 16 * 37 + 5                                     # the last tile holds five voxels
    x, _ = synth_inputs(n, p, seed=seed, oracle=orc)
    mask = (rng.uniform(size=n) > 0.35).astype(np.float32)
    mask[0], mask[n - 1], mask[n - 2] = 1.0, 0.0, 1.0   # zeros and ones inside the ragged tile too
    assert 0 < int((mask == 0).sum()) < n
    prior = orc.encoder_fwd(w, x)[0]
    return ctx, orc, w, x, mask, prior, tol


def two_step(ctx, ew, x, mask, prior, S, K, seed, voxel0=0):
    _, q, sigma = ctx.encoder_fwd(ew, x)
    sums, nk = ctx.elbo_fwd(x, mask, q, prior, sigma, S, K, seed=seed, voxel0=voxel0)
    return sums, q, nk


@pytest.mark.parametrize("T", [11, 24])
def test_fused_matches_encoder_then_elbo(params, T):
    """Ragged batch, mask with zeros, full Philox calls and short ones (S = 32 / K = 70 is the benchmark's shape: 18 KL
    calls over four lane groups, so the last trip is half empty; S = 5 / K = 9 leaves short calls in both loops)."""
    from qbold_vi_amd.ops import EncoderWeights
    ctx, orc, w, x, mask, prior, tol = make_case(params, T, seed=21)
    ew = EncoderWeights(ctx, T, 60, 2, True, -3.0).set_from_arrays(w)
    n = x.shape[0]
    xd, md, pd = dev(x), dev(mask), dev(prior)
    for S, K, seed, v0 in ((32, 70, 4, 0), (5, 9, 11, 12345678901)):
        sums, q, nk = ctx.vi_fwd(ew, xd, md, pd, S, K, seed=seed, voxel0=v0)
        sums2, q2, nk2 = two_step(ctx, ew, xd, md, pd, S, K, seed, v0)
        dq = float((q - q2).abs().max())
        dnk = float(((nk - nk2).abs() / (1.0 + nk2.abs())).max())
        print(f"T={T} S={S} K={K}: max|dq|={dq:.3e} bitwise q={bool(torch.equal(q, q2))} "
              f"max|d(nll,kl)|/(1+|.|)={dnk:.3e} bitwise={bool(torch.equal(nk, nk2))}")
        assert bool(torch.isfinite(nk).all()) and bool(torch.isfinite(q).all())
        assert dq < 2e-5
        assert torch.allclose(nk, nk2, rtol=tol, atol=tol), (S, K)
        # the three sums are the masked sums of the per-voxel outputs, zeros of the mask included
        want = torch.stack([(nk[:, 0].double() * md.double()).sum(), nk[:, 1].double()[md > 0].sum(), md.double().sum()])
        assert torch.allclose(sums, want, rtol=1e-6, atol=1e-9), (S, K)
        # ... and agree with the two-step sums as far as the per-voxel tolerance carries: tol (1 + |v|) per voxel
        room = tol * (n + nk2.double().abs().sum(0))
        assert abs(float(sums[0] - sums2[0])) <= float(room[0]) and abs(float(sums[1] - sums2[1])) <= float(room[1])
        assert float(sums[2]) == float(sums2[2]) == float(md.sum())
        # a voxel's outputs do not depend on where the batch ends: whole tiles only, and one voxel into the next tile
        for m in (n - 5, n - 4):
            _, qm, nkm = ctx.vi_fwd(ew, xd[:m], md[:m], pd[:m], S, K, seed=seed, voxel0=v0)
            assert torch.equal(qm, q[:m]) and torch.equal(nkm, nk[:m]), (S, K, m)
    # no mask at all is a mask of ones
    a, _, nka = ctx.vi_fwd(ew, xd, None, pd, 5, 9, seed=11)
    b, _, nkb = ctx.vi_fwd(ew, xd, torch.ones(n, device="cuda"), pd, 5, 9, seed=11)
    assert torch.equal(a, b) and torch.equal(nka, nkb)


@pytest.mark.parametrize("T", [11, 24])
def test_operand_range_status_reaches_nll(params, T):
    """One voxel whose normalised signal is ln(1e8 / 1e-2) = 23 at every tau but the spin echo -- some fifty times a
    tissue voxel's -- under weights scaled so that only its activations pass 65504: its nll is NaN on both paths (the
    stand-alone encoder poisons the heads, the fused kernel the per-draw constant), the masked nll sum carries the
    status, and every other voxel is untouched."""
    from qbold_vi_amd.ops import EncoderWeights
    ctx, orc, w, x, mask, prior, tol = make_case(params, T, seed=22)
    n, hot = x.shape[0], 16 * 11 + 6
    x = x.copy()
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

    # the smallest scale of the ladder at which the stand-alone encoder reports the hot voxel, and only it
    ew = tripped = None
    for sc in (1.0, 3.0, 10.0, 30.0, 100.0, 300.0, 1000.0, 3000.0, 10000.0):
        ew = EncoderWeights(ctx, T, 60, 2, True, -3.0).set_from_arrays(scaled(sc))
        tripped = torch.isnan(ctx.encoder_fwd(ew, xd, want=("out2",))[1]).any(1)
        print(f"T={T} scale {sc:g}: {int(tripped.sum())} voxels beyond the operand range, hot voxel: {bool(tripped[hot])}")
        if bool(tripped[hot]):
            break
    assert bool(tripped[hot]) and int(tripped.sum()) == 1, "no scale of the ladder trips the hot voxel alone"
    S, K, seed = 6, 10, 7
    sums, q, nk = ctx.vi_fwd(ew, xd, md, pd, S, K, seed=seed)
    sums2, q2, nk2 = two_step(ctx, ew, xd, md, pd, S, K, seed)
    assert bool(torch.isnan(nk[hot, 0])) and bool(torch.isnan(nk2[hot, 0]))
    assert not bool(torch.isfinite(sums[0])) and not bool(torch.isfinite(sums2[0]))
    assert float(sums[2]) == float(md.sum())
    keep = ~tripped
    # The whitened KL loop is chosen per wave (any lane whose posterior can reach the logit clip sends the wave's 16
    # voxels through the general loop), and the hot voxel's posterior is garbage on the fused path and NaN on the
    # two-step path: its fifteen tile mates may take different KL loops on the two paths.  Their kl is held to what
    # test_whitened_kl_draws_against_the_general_form allows between the two loops (2e-3 of 1 + |kl|), their nll and
    # everything outside that tile to the fused-against-unfused tolerance.
    mates = torch.zeros_like(keep)
    mates[16 * (hot // 16):16 * (hot // 16) + 16] = True
    mates &= keep
    far = keep & ~mates
    dnk = float(((nk[far] - nk2[far]).abs() / (1.0 + nk2[far].abs())).max())
    dnll = float(((nk[mates, 0] - nk2[mates, 0]).abs() / (1.0 + nk2[mates, 0].abs())).max())
    dkl = float(((nk[mates, 1] - nk2[mates, 1]).abs() / (1.0 + nk2[mates, 1].abs())).max())
    print(f"T={T}: other tiles max|d(nll,kl)|/(1+|.|)={dnk:.3e}; the hot voxel's tile: nll {dnll:.3e}, kl {dkl:.3e}")
    assert bool(torch.isfinite(nk[keep]).all())
    assert torch.allclose(nk[far], nk2[far], rtol=tol, atol=tol)
    assert torch.allclose(nk[mates, 0], nk2[mates, 0], rtol=tol, atol=tol)
    assert dkl < 2e-3
    assert float((q[keep] - q2[keep]).abs().max()) < 2e-5
