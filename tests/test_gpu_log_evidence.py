"""Importance-weighted evidence (qbold_log_evidence_fwd, Context.log_evidence, FineTuner.log_evidence): against a
float64 reference built from the oracle's primitives (tests/_iw_reference.py), the Philox stream, the bound's
identities, a known answer by quadrature, sharding / determinism, and the Python surface."""
import math

import numpy as np
import pytest

from _iw_reference import dw_coef, iw_reference, rel, rel1

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

IW_STREAM = 6


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def heads(o32, p, T, n, seed):
    from oracle.oracle import init_weights, synth_inputs
    x, _ = synth_inputs(n, p, seed=seed, oracle=o32)
    w = init_weights(T=T, U=60, L=2, seed=3)
    w["gate_offset"] = -3.0
    prior, q, sigma = o32.encoder_fwd(w, x)
    return x, q, prior, sigma


@pytest.fixture(scope="module")
def ctx(params):
    from qbold_vi_amd.ops import Context
    return Context(params, full_model=True, include_blood=True)


@pytest.fixture(scope="module")
def data11(params):
    from oracle.oracle import Oracle
    return heads(Oracle("f32", params), params, 11, 4096, 1)


def _p24(params):
    return dict(params, tau_start="-0.028", tau_end="0.065", tau_step="0.004")


def _p64(params):
    return dict(params, tau_start="-0.015", tau_end="0.065", tau_step="0.00125")


# name: (protocol, Context / Oracle loss switches, tissue mode, voxels, tolerance on log p^ and ELBO_same (rel1),
#        tolerance on ESS and is_means (rel))
CASES = {
    "table_T11": (None, {}, "table", 4096),
    "protocol_T24": (_p24, {}, "table", 1024),
    "protocol_T64": (_p64, {}, "table", 256),
    "literal": (None, {}, "literal", 512),
    "student_t": (None, dict(student_t_df=5.0), "table", 1024),
    "log_data": (None, dict(predict_log_data=True), "table", 1024),
    "three_image_norm": (None, dict(multi_image_normalisation=True), "table", 1024),
}


@pytest.mark.parametrize("case", list(CASES))
def test_matches_float64_reference_explicit_normals(params, case):
    from oracle.oracle import Oracle
    from qbold_vi_amd.ops import Context
    proto, sw, mode, n = CASES[case]
    p = proto(params) if proto else params
    o32 = Oracle("f32", p, **sw)
    o64 = Oracle("f64", p, node0_zero=True, **sw)   # node 0 of the Simpson sum rounds to 0 in float32 (the table's F)
    try:
        T = o32.T
        x, q, prior, sigma = heads(o32, p, T, n, 11)
        K = 64
        z = np.random.default_rng(5).standard_normal((n, K, 2)).astype(np.float32)
        ref = iw_reference(o64, x, q, prior, sigma, z, p)
    finally:
        o64.lib.qbo_set_node0_zero(0)
    c = Context(p, True, True, **sw)
    c.set_tissue_mode(mode)
    sums, out, means = c.log_evidence(dev(x), None, dev(q), dev(prior), dev(sigma), K, z=dev(z), want_means=True)
    out = out.cpu().numpy()
    means = means.cpu().numpy()
    errs = dict(log_p=rel1(out[:, 0], ref["log_p"]), elbo=rel1(out[:, 1], ref["elbo"]), ess=rel(out[:, 2], ref["ess"]),
                means=rel(means, ref["means"]))
    print(case, errs)
    assert errs["log_p"] < 1e-4 and errs["elbo"] < 1e-4, (case, errs)
    assert errs["ess"] < 1e-4 and errs["means"] < 1e-4, (case, errs)
    s = sums.cpu().numpy()
    assert s[2] == n


def test_philox_stream_equals_explicit_normals(ctx, data11):
    x, q, prior, sigma = (dev(a) for a in data11)
    n, K, seed, v0 = x.shape[0], 100, 77, 123457
    s1, o1, m1 = ctx.log_evidence(x, None, q, prior, sigma, K, seed=seed, voxel0=v0, want_means=True)
    z = ctx.normals(n, K, stream_id=IW_STREAM, seed=seed, voxel0=v0)
    s2, o2, m2 = ctx.log_evidence(x, None, q, prior, sigma, K, z=z, seed=seed, voxel0=v0, want_means=True)
    assert rel1(o1.cpu().numpy(), o2.cpu().numpy()) < 1e-6
    assert rel1(m1.cpu().numpy(), m2.cpu().numpy()) < 1e-6
    # another stream id gives other draws
    z5 = ctx.normals(n, K, stream_id=5, seed=seed, voxel0=v0)
    _, o5, _ = ctx.log_evidence(x, None, q, prior, sigma, K, z=z5)
    assert not torch.equal(o5, o1)


def test_identities(ctx, data11, oracle64):
    x, q, prior, sigma = data11
    n = x.shape[0]
    xd, qd, pd, sd = dev(x), dev(q), dev(prior), dev(sigma)
    # K = 1: one draw, log p^ = ELBO_same = log w of that draw, ESS = 1
    z = ctx.normals(n, 1, stream_id=IW_STREAM, seed=3)
    _, o1, _ = ctx.log_evidence(xd, None, qd, pd, sd, 1, seed=3)
    o1 = o1.cpu().numpy()
    assert np.array_equal(o1[:, 0], o1[:, 1]) and np.all(o1[:, 2] == 1.0)
    try:
        oracle64.lib.qbo_set_node0_zero(1)
        ref = iw_reference(oracle64, x[:512], q[:512], prior[:512], sigma[:512], z[:512].cpu().numpy())
    finally:
        oracle64.lib.qbo_set_node0_zero(0)
    assert rel1(o1[:512, 0], ref["lw"][:, 0]) < 1e-4
    # the bound, the ESS range, and the averaged bound rising with K (the K = 8 draws are the first of the K = 1024)
    means = {}
    for K in (8, 64, 1024):
        _, o, _ = ctx.log_evidence(xd, None, qd, pd, sd, K, seed=3)
        o = o.cpu().numpy().astype(np.float64)
        assert np.all(np.isfinite(o))
        assert np.all(o[:, 0] - o[:, 1] >= -1e-6 * (1.0 + np.abs(o[:, 1]))), K   # float32 rounding only
        assert np.all(o[:, 2] >= 1.0 - 1e-6) and np.all(o[:, 2] <= K * (1.0 + 1e-6)), K
        means[K] = o[:, 0].mean()
    assert means[8] < means[64] < means[1024], means


def _logit_mvn_logpdf(l, raw):
    """log N(l; mu, L L^T) in the logit plane for the 5 raw parameters (transform_std / transform_offdiag)."""
    so, sd = 3 * np.tanh(raw[1]) - 1, 3 * np.tanh(raw[3]) - 1
    c = np.tanh(raw[4]) * np.exp(-2.0)
    r0, r1 = l[..., 0] - raw[0], l[..., 1] - raw[2]
    w0 = r0 * np.exp(-so)
    w1 = (r1 - c * w0) * np.exp(-sd)
    return -np.log(2 * np.pi) - (so + sd) - 0.5 * (w0 * w0 + w1 * w1)


def _quadrature(o64, x, sigma, prior, grid):
    """log p(x) = log int p(x | y) N(y; mu_p, Sigma_p) dy on a float64 grid in the logit plane, and the grid
    posterior's logit mean / covariance and (OEF, DBV, R2') means."""
    def loglik(la, lb):
        A, B = np.meshgrid(la, lb, indexing="ij")
        lg = np.stack([A.ravel(), B.ravel()], -1)
        y = np.stack([1 / (1 + np.exp(-lg[:, 0])) * 0.8 + 0.04, 1 / (1 + np.exp(-lg[:, 1])) * 0.2 + 0.001], -1)
        m = lg.shape[0]
        nll = o64.nll(np.repeat(x[None], m, 0), np.ones(m), o64.signal_fwd(y), np.repeat(sigma[None], m, 0))
        return lg, y, -nll + _logit_mvn_logpdf(lg, prior)
    so, sd = np.exp(3 * np.tanh(prior[1]) - 1), np.exp(3 * np.tanh(prior[3]) - 1)
    la = np.linspace(prior[0] - 6 * so, prior[0] + 6 * so, 121)
    lb = np.linspace(prior[2] - 6 * sd, prior[2] + 6 * sd, 121)
    lg, _, lj = loglik(la, lb)
    keep = lj > lj.max() - 40.0
    lo, hi = lg[keep].min(0), lg[keep].max(0)
    pad = np.array([la[1] - la[0], lb[1] - lb[0]])
    lo, hi = lo - pad, hi + pad
    fa, fb = np.linspace(lo[0], hi[0], grid), np.linspace(lo[1], hi[1], grid)
    lg, y, lj = loglik(fa, fb)
    M = lj.max()
    w = np.exp(lj - M)
    Z = w.sum()
    logp = M + np.log(Z) + np.log((fa[1] - fa[0]) * (fb[1] - fb[0]))
    w = w / Z
    mu = (w[:, None] * lg).sum(0)
    d = lg - mu
    cov = (w[:, None, None] * d[:, :, None] * d[:, None, :]).sum(0)
    theta = np.stack([y[:, 0], y[:, 1], dw_coef(o64.params) * y[:, 0] * y[:, 1]], -1)
    return logp, mu, cov, (w[:, None] * theta).sum(0)


def test_known_answer_by_quadrature(ctx, params):
    """log p(x) and the posterior means of a handful of voxels by float64 quadrature; q = the family's closest member
    (the grid posterior's mean and Cholesky factor, clipped into transform_std / transform_offdiag range).  Catches a
    wrong constant, Jacobian or sign."""
    from oracle.oracle import Oracle, synth_inputs
    o32 = Oracle("f32", params)
    n = 6
    x, _ = synth_inputs(n, params, seed=21, oracle=o32)
    sigma = np.full((n, o32.T), 0.05, np.float32)
    prior = np.tile(np.array([-0.2, 0.3, -2.0, 0.3, 0.0], np.float32), (n, 1))
    o64 = Oracle("f64", params, node0_zero=True)
    try:
        quad = [_quadrature(o64, x[i].astype(np.float64), sigma[i].astype(np.float64), prior[i].astype(np.float64),
                            241) for i in range(n)]
    finally:
        o64.lib.qbo_set_node0_zero(0)
    q = np.zeros((n, 5), np.float32)
    for i, (_, mu, cov, _) in enumerate(quad):
        L = np.linalg.cholesky(cov)
        q[i] = [mu[0], np.arctanh(np.clip((np.log(L[0, 0]) + 1) / 3, -0.999, 0.999)), mu[1],
                np.arctanh(np.clip((np.log(L[1, 1]) + 1) / 3, -0.999, 0.999)),
                np.arctanh(np.clip(L[1, 0] / np.exp(-2.0), -0.99, 0.99))]
    K = 16384
    _, out, means = ctx.log_evidence(dev(x), None, dev(q), dev(prior), dev(sigma), K, seed=5, want_means=True)
    out, means = out.cpu().numpy().astype(np.float64), means.cpu().numpy().astype(np.float64)
    for i, (logp, _, _, pm) in enumerate(quad):
        band = 5.0 / np.sqrt(out[i, 2]) + 1e-3
        print(i, "quadrature", logp, "iw", out[i, 0], "ess", out[i, 2], "means", pm, means[i])
        assert abs(out[i, 0] - logp) < band, (i, out[i], logp)
        assert out[i, 1] <= out[i, 0]
        assert np.all(np.abs(means[i] - pm) < band * np.abs(pm)), (i, means[i], pm)


def _same_bits(a, b):
    """bitwise equality (NaN included)"""
    iv = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def test_sharding_determinism_and_sums(ctx, data11):
    x, q, prior, sigma = (a[:3001] for a in data11)
    n, K, seed, v0 = 3001, 48, 99, 5000
    mask = (np.random.default_rng(4).uniform(size=n) > 0.25).astype(np.float32)
    mask[mask > 0] = np.random.default_rng(6).uniform(0.5, 1.5, int((mask > 0).sum())).astype(np.float32)
    x = x.copy()
    x[mask == 0] = np.nan   # masked voxels must stay out of the sums whatever they hold
    args = [dev(x), dev(mask), dev(q), dev(prior), dev(sigma)]
    s, o, m = ctx.log_evidence(*args, K, seed=seed, voxel0=v0, want_means=True)
    s2, o2, m2 = ctx.log_evidence(*args, K, seed=seed, voxel0=v0, want_means=True)
    assert _same_bits(o, o2) and _same_bits(m, m2) and _same_bits(s, s2)
    h = 1500
    sa, oa, ma = ctx.log_evidence(*(a[:h] for a in args), K, seed=seed, voxel0=v0, want_means=True)
    sb, ob, mb = ctx.log_evidence(*(a[h:] for a in args), K, seed=seed, voxel0=v0 + h, want_means=True)
    assert _same_bits(o[:h], oa) and _same_bits(o[h:], ob)
    assert _same_bits(m[:h], ma) and _same_bits(m[h:], mb)
    on = o.cpu().numpy().astype(np.float64)
    live = mask > 0
    assert np.all(np.isfinite(on[live])) and np.all(np.isnan(on[~live, 0]))
    want = np.array([(mask[live] * -on[live, 0]).sum(), (mask[live] * -on[live, 1]).sum(), mask.astype(np.float64).sum()])
    got = s.cpu().numpy()
    assert np.all(np.abs(got - want) <= 1e-8 * np.abs(want)), (got, want)
    both = (sa + sb).cpu().numpy()
    assert np.all(np.abs(both - want) <= 1e-8 * np.abs(want))


def test_bad_arguments(ctx, data11):
    import ctypes as C
    from qbold_vi_amd import _lib
    x, q, prior, sigma = (dev(a[:64]) for a in data11)
    out = torch.empty((64, 3), device="cuda")
    sums = torch.empty(3, dtype=torch.float64, device="cuda")
    ws = ctx._workspace()
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731

    def call(K, o=out):
        return ctx.lib.qbold_log_evidence_fwd(ctx.handle, P(x), None, P(q), P(prior), P(sigma), None, int(K), 1, 0,
                                              P(o), None, P(sums), P(ws), 64, None)
    assert call(0) == -1 and call(-5) == -1 and call((1 << 30) + 1) == -1
    assert call(8, None) == -1
    assert call(8) == _lib.QBOLD_OK
    torch.cuda.synchronize()
    with pytest.raises(_lib.QboldError):
        ctx.log_evidence(x, None, q, prior, sigma, 0)


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


def _flat_check(tr, model, ft, x5, mask5, prior5, K, seed, sigma=None):
    got = ft.log_evidence(x5, mask5, prior5, no_samples=K, seed=seed, voxel0=7, want_means=True)
    lead = x5.shape[:-1]
    assert got["log_evidence"].shape == lead and got["elbo"].shape == lead and got["ess"].shape == lead
    assert got["is_means"].shape == lead + (3,)
    _, q5, sg5 = model.predict(x5, want=("out2", "sigma"))
    sg = sg5.reshape(-1, 11) if sigma is None else torch.full_like(sg5.reshape(-1, 11), sigma)
    sums, out, means = tr.context.log_evidence(x5.reshape(-1, 11), mask5.reshape(-1), q5.reshape(-1, 5),
                                               prior5.reshape(-1, 5), sg, K, seed=seed, voxel0=7, want_means=True)
    assert torch.equal(got["log_evidence"].reshape(-1), out[:, 0]) and torch.equal(got["ess"].reshape(-1), out[:, 2])
    assert torch.equal(got["elbo"].reshape(-1), out[:, 1]) and torch.equal(got["is_means"].reshape(-1, 3), means)
    assert torch.equal(got["sums"], sums)
    s = sums.cpu().numpy()
    assert abs(float(got["gap"]) - (s[1] - s[0]) / s[2]) < 1e-12 * abs(s[0] / s[2]) + 1e-12
    assert float(got["gap"]) >= 0.0
    return got


def test_fine_tuner_voxel_batch_and_crops(trainer, params):
    from oracle.oracle import Oracle, synth_inputs
    o32 = Oracle("f32", params)
    model, ft = _fine_tuner(trainer, params)
    n = 1000
    x, _ = synth_inputs(n, params, seed=3, oracle=o32)
    x5 = dev(x).reshape(n, 1, 1, 1, 11)
    mask5 = dev((np.random.default_rng(4).uniform(size=n) > 0.3).astype(np.float32)).reshape(n, 1, 1, 1, 1)
    out1 = model(x5)[0]
    _flat_check(trainer, model, ft, x5, mask5, out1, 32, 5)
    B, X, Y, Z = 2, 38, 25, 8
    xc, _ = synth_inputs(B * X * Y * Z, params, seed=8, oracle=o32)
    xc5 = dev(xc).reshape(B, X, Y, Z, 11)
    mc5 = dev((np.random.default_rng(9).uniform(size=B * X * Y * Z) > 0.2).astype(np.float32)).reshape(B, X, Y, Z, 1)
    pc5 = model(xc5)[0]
    _flat_check(trainer, model, ft, xc5, mc5, pc5, 16, 6)
    # homoscedastic noise: the fine tuner's one sigma instead of the encoder's sigma head
    from qbold_vi_amd import EncoderTrainer
    tr2 = EncoderTrainer(system_params=params, no_units=60, no_intermediate_layers=2, initial_im_sigma=0.07,
                         activation_type='relu', multi_image_normalisation=False, channelwise_gating=True,
                         use_population_prior=False, use_mvg=True, predict_log_data=False, heteroscedastic_noise=False)
    m2, ft2 = _fine_tuner(tr2, params)
    _flat_check(tr2, m2, ft2, x5, mask5, m2(x5)[0], 8, 5, sigma=math.exp(math.log(0.07)))


def test_fine_tuner_diagonal_family_is_refused(params):
    from qbold_vi_amd import EncoderTrainer
    tr = EncoderTrainer(system_params=params, no_units=30, use_mvg=False, use_population_prior=False,
                        activation_type='relu', predict_log_data=False)
    model, ft = _fine_tuner(tr, params)
    x5 = torch.ones((4, 1, 1, 1, 11), device="cuda")
    with pytest.raises(NotImplementedError, match="diagonal family"):
        ft.log_evidence(x5, torch.ones((4, 1, 1, 1, 1), device="cuda"), torch.zeros((4, 1, 1, 1, 4), device="cuda"))


def test_save_predictions_writes_the_evidence_maps(trainer, params, tmp_path):
    import os
    from oracle.oracle import Oracle, synth_inputs
    from qbold_vi_amd import nifti
    model, ft = _fine_tuner(trainer, params)
    B, X, Y, Z = 2, 6, 5, 4
    x, _ = synth_inputs(B * X * Y * Z, params, seed=12, oracle=Oracle("f32", params))
    mask = (np.random.default_rng(1).uniform(size=(B * X * Y * Z, 1)) > 0.2).astype(np.float32)
    data = dev(np.concatenate([x, mask], -1)).reshape(B, X, Y, Z, 12)
    priors = model(data[..., :-1])[0]
    d0, d1 = tmp_path / "plain", tmp_path / "iw"
    os.makedirs(d0)
    os.makedirs(d1)
    assert trainer.save_predictions(model, data, str(d0 / "sub"), fine_tuner_model=ft, priors=priors) is None
    maps = trainer.save_predictions(model, data, str(d1 / "sub"), fine_tuner_model=ft, priors=priors, iw_samples=32)
    extra = {"sub_logevidence.nii.gz", "sub_vigap.nii.gz", "sub_ess.nii.gz"}
    assert set(os.listdir(d1)) == set(os.listdir(d0)) | extra and not (set(os.listdir(d0)) & extra)
    live = mask.reshape(B, X, Y, Z) > 0
    for k in ("logevidence", "vigap", "ess"):
        v = maps[k].cpu().numpy()
        assert v.shape == (B, X, Y, Z, 1)
        img = nifti.load(str(d1 / f"sub_{k}.nii.gz"))[0]
        want = np.concatenate(np.split(v, B, axis=0), axis=-1)[0]
        np.testing.assert_array_equal(img, want)
        assert np.all(v[..., 0][~live] == 0.0)
    assert np.all(maps["vigap"].cpu().numpy() >= -1e-4) and np.all(maps["ess"].cpu().numpy()[..., 0][live] >= 1.0 - 1e-6)
