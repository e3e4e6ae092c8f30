"""Host-side checks of the per-voxel refinement: the float64 restatement of one refinement step that the GPU tests hold
qbold_refine_posterior to (tests/_refine_reference.py), the C ABI entry, and the argument checks of
Context.refine_posterior that raise before any launch.  No GPU needed."""
import numpy as np
import pytest

from _refine_reference import kl_closed_and_grad, padded_draws, refine_reference, step_grad, to_raw


def _inputs(o32, params, n, seed):
    from oracle.oracle import init_weights, synth_inputs
    x, _ = synth_inputs(n, params, seed=seed, oracle=o32)
    w = init_weights(T=o32.T, U=60, L=2, seed=3)
    w["gate_offset"] = -3.0
    prior, q, sigma = o32.encoder_fwd(w, x)
    q = (q + np.random.default_rng(seed).normal(size=q.shape) * 0.3).astype(np.float32)   # away from the prior
    prior[:, 4] = 0.0   # Oracle.kl_closed is the exact KL for a prior without off-diagonal term (see below)
    return x, q, prior, sigma


VARIANTS = {
    "gaussian": {},
    "student_t": dict(student_t_df=5.0),
    "log_data": dict(predict_log_data=True),
    "three_image_norm": dict(multi_image_normalisation=True),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_step_gradient_matches_finite_differences(params, variant):
    """The restatement (reparameterised NLL gradient + closed-form KL gradient, chained to the raw heads) against
    central differences of Oracle("f64").elbo's NLL over the same explicit normals plus Oracle.kl_closed."""
    from oracle.oracle import Oracle
    sw = VARIANTS[variant]
    o32 = Oracle("f32", params, **sw)
    o64 = Oracle("f64", params, node0_zero=True, **sw)
    try:
        n, S = 24, 3
        x, q, prior, sigma = _inputs(o32, params, n, 7)
        z = np.random.default_rng(1).standard_normal((n, S, 2))
        zk = np.zeros((n, 1, 2))
        q64 = q.astype(np.float64)

        def loss(qq):
            e = o64.elbo(x, np.ones(n), qq, prior, sigma, z, zk)
            return e["nll_v"] + o64.kl_closed(qq, prior)
        g = step_grad(o64, x, q64, prior, sigma, z)
        h = 1e-5
        for k in range(5):
            d = np.zeros_like(q64)
            d[:, k] = h
            fd = (loss(q64 + d) - loss(q64 - d)) / (2 * h)
            scale = np.abs(fd).max() + 1e-3
            assert np.max(np.abs(g[:, k] - fd)) / scale < 1e-6, (variant, k, np.max(np.abs(g[:, k] - fd)), scale)
    finally:
        o64.lib.qbo_set_node0_zero(0)


def test_closed_form_kl_is_the_expected_monte_carlo_kl(oracle64):
    """The refinement's KL is the exact one: the expectation of the library's Monte-Carlo KL (Oracle.kl_samples).
    With a prior whose off-diagonal head is 0 it is Oracle.kl_closed to rounding; with one that is not, Oracle.kl_closed
    (the reference's mvg_kl trace term, tr(L_p^-1 L_p^-T Sigma_q)) differs from it, and the Monte-Carlo mean sides
    with the exact KL."""
    rng = np.random.default_rng(3)
    q = rng.normal(size=(6, 5)) * 0.5
    p = rng.normal(size=(6, 5)) * 0.5
    p0 = p.copy()
    p0[:, 4] = 0.0
    kl, _ = kl_closed_and_grad(q, p0)
    np.testing.assert_allclose(kl, oracle64.kl_closed(q, p0), rtol=1e-12, atol=1e-12)
    p[:, 4] = 2.0   # c = tanh(2) e^-2
    kl, _ = kl_closed_and_grad(q, p)
    K = 200_000
    z = rng.standard_normal((6, K, 2))
    mc = oracle64.kl_samples(q, p, z)
    se = 5.0 * np.sqrt(np.var([oracle64.kl_samples(q, p, z[:, k:k + 1]) for k in range(0, 2000)], axis=0) / K)
    assert np.all(np.abs(mc - kl) < se + 1e-6), (mc, kl, se)
    assert np.any(np.abs(oracle64.kl_closed(q, p) - kl) > 20 * se)
    kl0, g0 = kl_closed_and_grad(p, p)
    np.testing.assert_allclose(kl0, 0.0, atol=1e-12)
    np.testing.assert_allclose(g0, 0.0, atol=1e-12)


def test_closed_form_kl_gradient_matches_finite_differences():
    rng = np.random.default_rng(5)
    q = rng.normal(size=(20, 5)) * 0.6
    p = rng.normal(size=(20, 5)) * 0.6
    _, g = kl_closed_and_grad(q, p)
    g = to_raw(q, g)
    h = 1e-6
    for k in range(5):
        d = np.zeros_like(q)
        d[:, k] = h
        fd = (kl_closed_and_grad(q + d, p)[0] - kl_closed_and_grad(q - d, p)[0]) / (2 * h)
        np.testing.assert_allclose(g[:, k], fd, rtol=1e-6, atol=1e-8)


def test_reference_loop_descends(params):
    """Twenty float64 SGD steps at a small rate lower each voxel's loss on fixed draws (a sanity check of the
    whole-loop restatement the GPU optimiser test compares against)."""
    from oracle.oracle import Oracle
    o32 = Oracle("f32", params)
    o64 = Oracle("f64", params, node0_zero=True)
    try:
        n, S, steps = 16, 2, 20
        x, q, prior, sigma = _inputs(o32, params, n, 9)
        z = np.zeros((n, steps, padded_draws(S), 2))
        z[:, :, :S] = np.random.default_rng(2).standard_normal((n, 1, S, 2))   # the same draws at every step

        def loss(qq):
            e = o64.elbo(x, np.ones(n), qq, prior, sigma, z[:, 0, :S], np.zeros((n, 1, 2)))
            return e["nll_v"] + o64.kl_closed(qq, prior)
        q1 = refine_reference(o64, x, q, prior, sigma, z, S, lr=2e-3, optimizer="sgd")
        assert np.all(loss(q1) < loss(q.astype(np.float64)))
    finally:
        o64.lib.qbo_set_node0_zero(0)


def test_abi_declares_the_entry_point():
    import os
    from qbold_vi_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "qbold_hip.h")) as f:
        hdr = f.read()
    assert "int qbold_refine_posterior(" in hdr and "qbold_refine_cfg;" in hdr
    assert "#define QBOLD_ABI_VERSION 5" in hdr
    assert "7 = the refinement draws of qbold_refine_posterior" in hdr
    _, args = _lib.SIGNATURES["qbold_refine_posterior"]
    assert len(args) == 16
    assert [f[0] for f in _lib.RefineCfg._fields_] == ["optimizer", "lr", "lr_final", "beta1", "beta2", "eps"]


@pytest.fixture(scope="module")
def host_ctx(params):
    from qbold_vi_amd.ops import Context
    return Context(params, host_only=True)


@pytest.mark.parametrize("kw,err", [
    (dict(steps=0), ValueError), (dict(S=0), ValueError), (dict(lr=0.0), ValueError), (dict(lr=-1.0), ValueError),
    (dict(lr_final=-0.1), ValueError), (dict(optimizer="rmsprop"), ValueError),
    (dict(steps=1 << 31, S=5), ValueError),
])
def test_context_refine_checks_arguments_before_launch(host_ctx, kw, err):
    torch = pytest.importorskip("torch")
    t = torch.zeros((4, 11))
    q = torch.zeros((4, 5))
    with pytest.raises(err):
        host_ctx.refine_posterior(t, None, q, q, t, **kw)


def test_context_refine_needs_device_tensors(host_ctx):
    torch = pytest.importorskip("torch")
    from qbold_vi_amd._lib import QboldError
    t = torch.zeros((4, 11))
    q = torch.zeros((4, 5))
    with pytest.raises(QboldError, match="no CPU fallback"):
        host_ctx.refine_posterior(t, None, q, q, t)


def test_fine_tuner_refine_rejects_the_diagonal_family_and_the_population_prior():
    from qbold_vi_amd.model import FineTuner

    class _Tr:
        _use_mvg = False
        _heteroscedastic_noise = True
        _use_population_prior = False
        _mog_components = 1
        _seed = 1

    ft = FineTuner(_Tr(), None, None)
    with pytest.raises(NotImplementedError, match="diagonal family"):
        ft.refine(None, None, None)
    _Tr._use_mvg = True
    _Tr._use_population_prior = True
    ft = FineTuner(_Tr(), None, None)
    with pytest.raises(NotImplementedError, match="population prior"):
        ft.refine(None, None, None)
