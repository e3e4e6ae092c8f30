"""Refinement of a volume under the TV smoothness prior (qbold_refine_posterior_spatial,
Context.refine_posterior_spatial, FineTuner.refine(smoothness_weight=...)): at w = 0 it is the per-voxel refinement
bit for bit; its TV gradient is qbold_smoothness's; twenty steps against the float64 Jacobi restatement
(tests/_refine_tv_reference.py); the structure of the coupling (batch elements, z slices, masked voxels); the joint
objective it lowers and what that buys on a noisy volume; argument errors and the Python surface."""
import ctypes as C
import os

import numpy as np
import pytest

from _refine_reference import padded_draws
from _refine_tv_reference import refine_tv_reference

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

REFINE_STREAM = 7


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _p24(params):
    return dict(params, tau_start="-0.028", tau_end="0.065", tau_step="0.004")


def _volume(o32, p, lead, seed, spread=0.3, keep=0.75, stripes=False):
    """Synthetic signals, heads of an untrained encoder (perturbed), a random mask, all shaped lead + (C,).
    stripes: heads 0 and 2 become diagonal stripes of 0, 0.6, 1.2 (plus noise of sd 0.05) about the encoder's mean
    head, so no two neighbours' means come close (no tie of the TV subgradient within a few steps)."""
    from oracle.oracle import init_weights, synth_inputs
    n = int(np.prod(lead))
    x, _ = synth_inputs(n, p, seed=seed, oracle=o32)
    w = init_weights(T=o32.T, U=60, L=2, seed=3)
    w["gate_offset"] = -3.0
    prior, q, sigma = o32.encoder_fwd(w, x)
    rng = np.random.default_rng(seed)
    q = (q + rng.normal(size=q.shape) * spread).astype(np.float32)
    mask = (rng.uniform(size=n) < keep).astype(np.float32)
    if stripes:
        xi, yi = np.meshgrid(np.arange(lead[1]), np.arange(lead[2]), indexing="ij")
        q = q.reshape(tuple(lead) + (5,))
        for ch, pat in ((0, (xi + 2 * yi) % 3), (2, (2 * xi + yi) % 3)):
            q[..., ch] = (np.float32(np.mean(q[..., ch])) + 0.6 * pat[None, :, :, None] +
                          0.05 * rng.standard_normal(tuple(lead)).astype(np.float32)) - 0.6
    r = lambda a: np.ascontiguousarray(a.reshape(tuple(lead) + a.shape[-1:]))   # noqa: E731
    return r(x), mask.reshape(lead), r(q), r(prior), r(sigma)


@pytest.fixture(scope="module")
def ctx(params):
    from qbold_vi_amd.ops import Context
    c = Context(params, full_model=True, include_blood=True)
    c.set_grad_node0(False)
    return c


def _flat(t, c):
    return t.reshape(-1, c)


# ---- 1. w = 0 is qbold_refine_posterior ---------------------------------------------------------------------------
IDENTITY_CASES = {
    "T11_se2": (None, {}),                                          # the <11, 2> instance
    "T11_three_image_norm": (None, dict(multi_image_normalisation=True)),   # the <11, -1> instance
    "T24": (_p24, {}),
}


@pytest.mark.parametrize("case", list(IDENTITY_CASES))
@pytest.mark.parametrize("explicit", [False, True])
def test_zero_weight_is_the_per_voxel_refinement_bitwise(params, case, explicit):
    from oracle.oracle import Oracle
    from qbold_vi_amd.ops import Context
    proto, sw = IDENTITY_CASES[case]
    p = proto(params) if proto else params
    c = Context(p, True, True, **sw)
    lead = (2, 19, 13, 4)
    x, m, q, prior, sigma = (dev(a) for a in _volume(Oracle("f32", p, **sw), p, lead, 11))
    n, T = int(np.prod(lead)), c.T
    for opt, steps, S in (("adam", 30, 2), ("sgd", 7, 5), ("adam", 1, 1)):
        Sp = padded_draws(S)
        z = torch.randn((n, steps, Sp, 2), device="cuda") if explicit else None
        kw = dict(steps=steps, S=S, lr=0.05, lr_final=0.01, optimizer=opt, z=z, seed=9, voxel0=321, want_loss=True)
        a, la = c.refine_posterior_spatial(x, m, q, prior, sigma, 0.0, **kw)
        b, lb = c.refine_posterior(_flat(x, T), m.reshape(-1), _flat(q, 5), _flat(prior, 5), _flat(sigma, T), **kw)
        assert _same_bits(_flat(a, 5), b), (case, opt, steps)
        assert _same_bits(_flat(la, 2), lb), (case, opt, steps)


# ---- 2. the TV gradient is qbold_smoothness's -----------------------------------------------------------------------
def test_tv_gradient_is_the_smoothness_kernels(ctx, params):
    from oracle.oracle import Oracle
    lead = (2, 19, 13, 4)
    x, m, q, prior, _ = (dev(a) for a in _volume(Oracle("f32", params), params, lead, 12, spread=1.0))
    sigma = torch.full_like(x, 0.5)   # a small likelihood gradient: the step is dominated by the TV term
    lr, w = 1e-2, 5.0
    z = torch.randn((int(np.prod(lead)), 1, 4, 2), device="cuda")
    kw = dict(steps=1, S=3, lr=lr, lr_final=lr, optimizer="sgd", z=z)
    q0 = ctx.refine_posterior_spatial(x, m, q, prior, sigma, 0.0, **kw)
    qw = ctx.refine_posterior_spatial(x, m, q, prior, sigma, w, **kw)
    g_q = torch.zeros((q.numel() // 5, 5), device="cuda")
    ctx.smoothness(q, m, weight=w, g_q=g_q)
    got = ((qw.double() - q0.double()) / (-lr)).reshape(-1, 5)
    qi = q.double().reshape(-1, 5)
    a0, aw = q0.double().reshape(-1, 5), qw.double().reshape(-1, 5)
    # w = 0 is the per-voxel kernel, w > 0 the per-step kernel: their likelihood gradients agree to rounding, and each
    # q_out is one fma of q - lr g, rounded once; a few ulps of q and of lr g, over lr
    ulp = (torch.maximum(a0.abs(), aw.abs()) + 4.0 * ((qi - a0).abs() + (qi - aw).abs())) * 2.0 ** -23
    err = torch.abs(got - g_q.double())
    print("max |g_q|", g_q.abs().max().item(), "max err", err.max().item(), "max err / tol",
          (err / (ulp / lr + 1e-12)).max().item())
    assert torch.all(err <= ulp / lr + 1e-12)
    assert g_q.abs().max().item() > 1.0
    dead = m.reshape(-1) <= 0
    assert _same_bits(_flat(qw, 5)[dead], _flat(q, 5)[dead])


# ---- 3. the whole loop against float64 -----------------------------------------------------------------------------
LOOP_CASES = {
    "T11_25x25x8": (None, {}, (1, 25, 25, 8)),
    "T11_2x19x13x4": (None, {}, (2, 19, 13, 4)),
    "T24": (_p24, {}, (1, 9, 7, 3)),
    "student_t": (None, dict(student_t_df=5.0), (1, 9, 7, 3)),
    "log_data": (None, dict(predict_log_data=True), (1, 9, 7, 3)),
    "three_image_norm": (None, dict(multi_image_normalisation=True), (1, 9, 7, 3)),
}


@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("case", list(LOOP_CASES))
def test_loop_matches_float64_jacobi(params, case, opt):
    """Twenty steps, w = 5, explicit normals, against the float64 Jacobi restatement.  The restatement records the
    smallest |sigmoid difference| over every live pair and step: above 1e-4 no float32 / float64 sign disagreement
    of the TV subgradient is possible, so the runs differ by float32 and the tissue table's gradient error only."""
    from oracle.oracle import Oracle
    from qbold_vi_amd.ops import Context
    proto, sw, lead = LOOP_CASES[case]
    p = proto(params) if proto else params
    c = Context(p, True, True, **sw)
    c.set_grad_node0(False)
    x, m, q, prior, sigma = _volume(Oracle("f32", p, **sw), p, lead, 13, spread=0.1, stripes=True)
    n, S, steps, w = int(np.prod(lead)), 2, 20, 5.0
    lr = 1e-4 if opt == "sgd" else 1e-3
    z = np.random.default_rng(4).standard_normal((n, steps, padded_draws(S), 2)).astype(np.float32)
    o64 = Oracle("f64", p, node0_zero=True, **sw)
    try:
        ref, gap = refine_tv_reference(o64, x, m, q, prior, sigma, z, S, w, lr=lr, lr_final=0.0, optimizer=opt)
    finally:
        o64.lib.qbo_set_node0_zero(0)
    got = c.refine_posterior_spatial(dev(x), dev(m), dev(q), dev(prior), dev(sigma), w, steps=steps, S=S, lr=lr,
                                     lr_final=0.0, optimizer=opt, z=dev(z)).cpu().numpy().astype(np.float64)
    live = m > 0
    diff = np.abs(got - ref)[live]
    moved = np.abs(ref - q)[live]
    print(case, opt, "min gap", gap, "moved max", moved.max(), "diff max", diff.max(), "p99", np.quantile(diff, 0.99))
    assert gap > 1e-4
    np.testing.assert_array_equal(got[~live], q[~live])
    assert diff.max() < 1e-5, (case, opt, diff.max())


# ---- 4. structure --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vol3(params):
    from oracle.oracle import Oracle
    return _volume(Oracle("f32", params), params, (3, 17, 15, 4), 14, spread=1.0)


def test_structure_is_bitwise(ctx, vol3):
    x, m, q, prior, sigma = vol3
    B, X, Y, Z = m.shape
    xyz = X * Y * Z
    kw = dict(steps=25, S=2, lr=0.05, seed=17, want_loss=True)
    args = [dev(a) for a in (x, m, q, prior, sigma)]
    o, lo = ctx.refine_posterior_spatial(*args, 5.0, voxel0=1000, **kw)
    o2, lo2 = ctx.refine_posterior_spatial(*args, 5.0, voxel0=1000, **kw)
    assert _same_bits(o, o2) and _same_bits(lo, lo2)
    # batch elements are independent: three calls with voxel0 offsets
    for b in range(B):
        ob, lb = ctx.refine_posterior_spatial(*(a[b:b + 1] for a in args), 5.0, voxel0=1000 + b * xyz, **kw)
        assert _same_bits(ob, o[b:b + 1]) and _same_bits(lb, lo[b:b + 1]), b
    # Philox equals explicit normals
    n, Sp = B * xyz, padded_draws(2)
    z = ctx.normals(n, 25 * Sp, stream_id=REFINE_STREAM, seed=17, voxel0=1000).reshape(n, 25, Sp, 2)
    oz, lz = ctx.refine_posterior_spatial(*args, 5.0, voxel0=1000, z=z, **kw)
    assert _same_bits(oz, o) and _same_bits(lz, lo)
    # the data of one z slice reaches no other slice
    xs = args[0].clone()
    xs[:, :, :, 1] *= 1.05
    os_ = ctx.refine_posterior_spatial(xs, *args[1:], 5.0, voxel0=1000, **kw)[0]
    others = [k for k in range(Z) if k != 1]
    assert _same_bits(os_[:, :, :, others], o[:, :, :, others])
    assert not torch.equal(os_[:, :, :, 1], o[:, :, :, 1])
    # masked voxels return q_in and their heads reach no other voxel
    dead = args[1] <= 0
    assert dead.any() and _same_bits(o[dead], args[2][dead])
    assert not torch.equal(o[~dead], args[2][~dead])
    qx = args[2].clone()
    vals = torch.tensor([1e30, -1e30, float("nan"), 40.0, -40.0], device="cuda")
    qx[dead] = vals[torch.arange(int(dead.sum()), device="cuda") % 5].unsqueeze(-1).expand(-1, 5)
    xx = args[0].clone()
    xx[dead] = float("nan")   # masked voxels' data is not read either
    ox = ctx.refine_posterior_spatial(xx, args[1], qx, args[3], args[4], 5.0, voxel0=1000, **kw)[0]
    assert _same_bits(ox[~dead], o[~dead]) and _same_bits(ox[dead], qx[dead])
    # a NaN mask is a masked voxel
    mn = args[1].clone()
    mn[dead] = float("nan")
    assert _same_bits(ctx.refine_posterior_spatial(args[0], mn, *args[2:], 5.0, voxel0=1000, **kw)[0], o)
    # w > 0 couples voxels within a slice
    o0 = ctx.refine_posterior_spatial(*args, 0.0, voxel0=1000, **kw)[0]
    assert not torch.equal(o0[~dead], o[~dead])


def test_in_place_through_the_c_abi(ctx, vol3):
    from qbold_vi_amd import _lib
    from qbold_vi_amd._lib import Geometry
    x, m, q, prior, sigma = (dev(a) for a in vol3)
    geom = Geometry(*m.shape)
    P = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    ws = torch.empty(int(ctx.lib.qbold_refine_spatial_workspace_bytes(ctx.handle, C.byref(geom))), dtype=torch.uint8,
                     device="cuda")
    assert ws.numel() == 88 * m.numel()
    for steps in (1, 2, 9):
        want = ctx.refine_posterior_spatial(x, m, q, prior, sigma, 5.0, steps=steps, S=1, lr=0.05, seed=3)
        qi = q.clone()
        cfg = _lib.RefineCfg(0, 0.05, 0.005, 0.9, 0.999, 1e-8)
        rc = ctx.lib.qbold_refine_posterior_spatial(ctx.handle, P(x), P(m), P(qi), P(prior), P(sigma), None,
                                                    C.byref(geom), C.c_float(5.0), steps, 1, C.byref(cfg), 3, 0,
                                                    P(qi), None, P(ws), None)
        assert rc == 0
        torch.cuda.synchronize()
        assert _same_bits(qi, want), steps


# ---- 5 and 6. the objective, and what it is for ---------------------------------------------------------------------
def _smooth_volume(ctx, lead, noise, seed):
    """make_synthetic_volumes-style: smooth OEF / DBV truth fields, an elliptic brain mask, Gaussian noise of sd
    `noise` relative to the normalising echo; a broad constant prior and sigma = noise."""
    B, X, Y, Z = lead
    rng = np.random.default_rng(seed)
    xx, yy = np.meshgrid(np.linspace(-1, 1, X), np.linspace(-1, 1, Y), indexing="ij")

    def field(lo, hi):
        f = np.zeros(lead)
        for _ in range(4):
            kx, ky, ph = rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0), rng.uniform(0, 2 * np.pi, size=(B, 1, 1, Z))
            f += np.sin(np.pi * (kx * xx + ky * yy))[None, :, :, None] * np.cos(ph) + \
                np.cos(np.pi * (kx * xx - ky * yy))[None, :, :, None] * np.sin(ph)
        f = (f - f.min()) / (f.max() - f.min())
        return lo + (hi - lo) * f
    oef, dbv = field(0.2, 0.6), field(0.01, 0.08)
    brain = ((xx / 0.85) ** 2 + (yy / 0.7) ** 2 < 1.0)[None, :, :, None] * np.ones(lead)
    y = dev(np.stack([oef, dbv], -1).reshape(-1, 2).astype(np.float32))
    s = ctx.signal_fwd(y)
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = s + noise * s[:, 2:3] * torch.randn(s.shape, device="cuda", generator=g)
    n = s.shape[0]
    prior = torch.tensor([-0.2, 0.3, -2.0, 0.3, 0.0], device="cuda").expand(n, 5).contiguous()
    sigma = torch.full((n, ctx.T), noise, device="cuda")
    r = lambda t: t.reshape(lead + (t.shape[-1],)).contiguous()   # noqa: E731
    return r(x), dev(brain.astype(np.float32)), r(prior), r(sigma), oef


def _objective(ctx, x, m, q, prior, sigma, w):
    """F(q) = sum over the mask of (nll + kl) at S = K = 256 (the same draws for every q) + w TV(q)."""
    T = ctx.T
    sums, _ = ctx.elbo_fwd(_flat(x, T), m.reshape(-1), _flat(q, 5), _flat(prior, 5), _flat(sigma, T), 256, 256,
                           seed=4242)
    tv = ctx.smoothness(q, m).item()
    return sums[0].item() + sums[1].item() + w * tv, tv


def test_lowers_the_joint_objective(ctx):
    lead, w = (2, 48, 48, 8), 5.0
    x, m, prior, sigma, _ = _smooth_volume(ctx, lead, 0.02, 5)
    g = torch.Generator(device="cuda").manual_seed(6)
    q_enc = (prior + 0.3 * torch.randn(prior.shape, device="cuda", generator=g)).contiguous()
    q0 = ctx.refine_posterior_spatial(x, m, q_enc, prior, sigma, 0.0)
    qw = ctx.refine_posterior_spatial(x, m, q_enc, prior, sigma, w)
    f_enc, tv_enc = _objective(ctx, x, m, q_enc, prior, sigma, w)
    f0, tv0 = _objective(ctx, x, m, q0, prior, sigma, w)
    fw, tvw = _objective(ctx, x, m, qw, prior, sigma, w)
    print("F encoder", f_enc, "F w=0", f0, "F w=5", fw, "TV", tv_enc, tv0, tvw)
    assert fw < f_enc and fw < f0
    assert tvw < tv0


@pytest.mark.parametrize("noise", [0.01, 0.03, 0.06])
def test_smoothness_lowers_the_oef_error_on_noisy_volumes(ctx, noise):
    """Posterior-mean OEF of the refined heads against the truth field over the mask, w = 5 against w = 0.  The
    improvement is required where per-voxel posteriors are wide (the two noisier levels); every level is printed."""
    lead = (2, 48, 48, 8)
    x, m, prior, sigma, oef = _smooth_volume(ctx, lead, noise, 7)
    q_enc = prior.clone()
    live = m.reshape(-1) > 0
    truth = dev(oef.reshape(-1).astype(np.float32))[live]
    rmse = {}
    for w in (0.0, 5.0):
        qw = ctx.refine_posterior_spatial(x, m, q_enc, prior, sigma, w)
        mean = ctx.posterior_moments(_flat(qw, 5), 512, seed=3, want_vars=False)[0][:, 0]
        rmse[w] = torch.sqrt(torch.mean((mean[live] - truth) ** 2)).item()
    print(f"noise {noise}: masked OEF RMSE w=0 {rmse[0.0]:.4f}, w=5 {rmse[5.0]:.4f}")
    if noise >= 0.03:
        assert rmse[5.0] < rmse[0.0]


# ---- 7. API ----------------------------------------------------------------------------------------------------------
def test_bad_arguments(ctx, params, vol3):
    from qbold_vi_amd import _lib
    from qbold_vi_amd._lib import Geometry
    from qbold_vi_amd.ops import Context
    x, m, q, prior, sigma = (dev(a[:1]) for a in vol3)
    good = Geometry(*m.shape)
    ws = torch.empty(88 * m.numel() + 16, dtype=torch.uint8, device="cuda")
    out = torch.empty_like(q)
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731

    def call(c=ctx, geom=good, w=5.0, steps=5, S=1, lr=0.05, opt=0, qq=q, o=out, wsp=P(ws)):
        cfg = _lib.RefineCfg(opt, lr, lr, 0.9, 0.999, 1e-8)
        return c.lib.qbold_refine_posterior_spatial(c.handle, P(x), P(m), P(qq), P(prior), P(sigma), None,
                                                    C.byref(geom) if geom is not None else None, C.c_float(w), steps,
                                                    S, C.byref(cfg), 1, 0, P(o), None, wsp, None)
    assert call() == _lib.QBOLD_OK
    torch.cuda.synchronize()
    for kw in (dict(steps=0), dict(S=0), dict(lr=0.0), dict(opt=2), dict(qq=None), dict(o=None),
               dict(w=-1.0), dict(w=float("nan")), dict(w=float("inf")), dict(geom=None),
               dict(geom=Geometry(0, 1, 1, 1)), dict(geom=Geometry(1, -2, 1, 1)),
               dict(geom=Geometry(1 << 30, 1 << 30, 1 << 30, 4)),   # N beyond int64
               dict(wsp=None), dict(wsp=C.c_void_p(ws.data_ptr() + 4)),
               dict(steps=(1 << 31) - 1, S=9)):
        assert call(**kw) == -1, kw
    assert ctx.lib.qbold_refine_spatial_workspace_bytes(ctx.handle, C.byref(good)) == 88 * m.numel()
    assert ctx.lib.qbold_refine_spatial_workspace_bytes(ctx.handle, C.byref(Geometry(0, 1, 1, 1))) == -1
    assert ctx.lib.qbold_refine_spatial_workspace_bytes(ctx.handle, None) == -1
    cl = Context(params, True, True)
    cl.set_tissue_mode("literal")
    assert call(c=cl) == -3
    c64 = Context(dict(params, tau_start="-0.015", tau_end="0.065", tau_step="0.00125"), True, True)
    assert call(c=c64) == -3
    with pytest.raises(ValueError, match="z must be"):
        ctx.refine_posterior_spatial(x, m, q, prior, sigma, 5.0, steps=5, z=torch.zeros((7, 5, 4, 2), device="cuda"))
    with pytest.raises(ValueError, match="expects x"):
        ctx.refine_posterior_spatial(_flat(x, 11), m, q, prior, sigma, 5.0)
    with pytest.raises(ValueError, match="mask"):
        ctx.refine_posterior_spatial(x, m[:, :3], q, prior, sigma, 5.0)


@pytest.fixture(scope="module")
def trainer(params):
    from qbold_vi_amd import EncoderTrainer
    return EncoderTrainer(system_params=params, no_units=60, use_layer_norm=False, dropout_rate=0.0,
                          no_intermediate_layers=2, initial_im_sigma=0.05, activation_type='relu',
                          multi_image_normalisation=False, channelwise_gating=True, infer_inv_gamma=False,
                          use_population_prior=False, use_mvg=True, predict_log_data=False)


def _fine_tuner(tr, params, model=None):
    from qbold_vi_amd import SignalGenerationLayer
    if model is None:
        model, _ = tr.create_encoder(gate_offset=-3.0, resid_init_std=0.05, no_ip_images=11)
    return model, tr.build_fine_tuner(model, SignalGenerationLayer(dict(params, simulate_noise='False'), True, True))


def test_fine_tuner_refine_with_smoothness(trainer, params):
    from oracle.oracle import Oracle, synth_inputs
    model, ft = _fine_tuner(trainer, params)
    lead = (2, 19, 13, 4)
    nv = int(np.prod(lead))
    x, _ = synth_inputs(nv, params, seed=8, oracle=Oracle("f32", params))
    x5 = dev(x).reshape(lead + (11,))
    m5 = dev((np.random.default_rng(8).uniform(size=nv) > 0.3).astype(np.float32)).reshape(lead + (1,))
    p5 = model(x5)[0]
    got = ft.refine(x5, m5, p5, steps=50, no_samples=2, seed=4, voxel0=7, smoothness_weight=5.0)
    assert got["q"].shape == lead + (5,) and got["loss"].shape == lead + (2,)
    _, q5, sg5 = model.predict(x5, want=("out2", "sigma"))
    want, loss = trainer.context.refine_posterior_spatial(x5, m5, q5, p5, sg5, 5.0, steps=50, S=2, lr=0.1,
                                                          lr_final=0.01, seed=4, voxel0=7, want_loss=True)
    assert _same_bits(got["q"], want) and _same_bits(got["loss"], loss)
    plain = ft.refine(x5, m5, p5, steps=50, no_samples=2, seed=4, voxel0=7)
    zero = ft.refine(x5, m5, p5, steps=50, no_samples=2, seed=4, voxel0=7, smoothness_weight=0.0)
    assert _same_bits(plain["q"], zero["q"]) and not torch.equal(plain["q"], got["q"])
    with pytest.raises(ValueError, match="image data"):
        ft.refine(x5.reshape(-1, 11), m5.reshape(-1), p5.reshape(-1, 5), steps=5, smoothness_weight=5.0)


def test_fine_tuner_refine_with_smoothness_refuses_the_diagonal_family(params):
    from qbold_vi_amd import EncoderTrainer
    tr = EncoderTrainer(system_params=params, no_units=30, use_mvg=False, use_population_prior=False,
                        activation_type='relu', predict_log_data=False)
    model, ft = _fine_tuner(tr, params)
    x5 = torch.ones((1, 4, 3, 1, 11), device="cuda")
    with pytest.raises(NotImplementedError, match="diagonal family"):
        ft.refine(x5, torch.ones((1, 4, 3, 1, 1), device="cuda"), torch.zeros((1, 4, 3, 1, 4), device="cuda"),
                  smoothness_weight=5.0)


def test_save_predictions_with_smoothness(trainer, params, tmp_path):
    from oracle.oracle import Oracle, synth_inputs
    model, ft = _fine_tuner(trainer, params)
    B, X, Y, Z = 2, 6, 5, 4
    x, _ = synth_inputs(B * X * Y * Z, params, seed=12, oracle=Oracle("f32", params))
    mask = (np.random.default_rng(1).uniform(size=(B * X * Y * Z, 1)) > 0.2).astype(np.float32)
    data = dev(np.concatenate([x, mask], -1)).reshape(B, X, Y, Z, 12)
    priors = model(data[..., :-1])[0]
    d0, d1 = tmp_path / "w0", tmp_path / "w5"
    os.makedirs(d0)
    os.makedirs(d1)
    maps0 = trainer.save_predictions(model, data, str(d0 / "sub"), fine_tuner_model=ft, priors=priors,
                                     refine_steps=100)
    _, ft1 = _fine_tuner(trainer, params, model)
    maps5 = trainer.save_predictions(model, data, str(d1 / "sub"), fine_tuner_model=ft1, priors=priors,
                                     refine_steps=100, refine_smoothness_weight=5.0)
    assert set(os.listdir(d0)) == set(os.listdir(d1))
    live = mask.reshape(B, X, Y, Z) > 0
    for k in ("oef_refined", "dbv_refined", "r2p_refined", "amortgap"):
        a, b = maps0[k].cpu().numpy(), maps5[k].cpu().numpy()
        assert b.shape == (B, X, Y, Z, 1) and np.all(np.isfinite(b))
        assert not np.array_equal(a[live], b[live]), k
