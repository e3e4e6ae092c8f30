"""Host-side checks of the float64 reference the GPU tests hold qbold_log_evidence_bwd to (tests/_iw_grad_reference.py):
its sigma gradient and its doubly-reparameterised head gradient against central differences of the oracle's own
numbers, and its K = 1 case against the stop-gradient ELBO gradient of the same draw.  No GPU needed."""
import numpy as np
import pytest

from _iw_grad_reference import frozen_log_weights, iw_grad_reference, neg_log_p
from _refine_reference import nll_grad, to_raw


@pytest.fixture(scope="module")
def inputs(params):
    from oracle.oracle import Oracle, init_weights, synth_inputs
    o32 = Oracle("f32", params)
    n = 6
    x, _ = synth_inputs(n, params, seed=5, oracle=o32)
    w = init_weights(T=11, U=60, L=2, seed=3)
    w["gate_offset"] = -3.0
    prior, q, sigma = o32.encoder_fwd(w, x)
    q = (q + np.random.default_rng(4).normal(size=q.shape) * 0.3).astype(np.float32)
    return tuple(np.asarray(a, np.float64) for a in (x, q, prior, sigma))


@pytest.fixture(scope="module")
def o64(params):
    from oracle.oracle import Oracle
    o = Oracle("f64", params, node0_zero=True)   # exact derivatives of the forward value (test_gpu_refine)
    yield o
    o.lib.qbo_set_node0_zero(0)


def test_sigma_gradient_is_the_derivative_of_log_p(o64, inputs):
    """g_log_sigma = d(-log p^_K) / d log sigma with eps fixed, per voxel and tau, by central differences."""
    x, q, prior, sigma = inputs
    n, K, T = x.shape[0], 5, x.shape[1]
    z = np.random.default_rng(6).standard_normal((n, K, 2))
    ref = iw_grad_reference(o64, x, q, prior, sigma, z)
    ls = np.log(sigma)
    h = 1e-6
    fd = np.empty((n, T))
    for t in range(T):
        d = np.zeros_like(ls)
        d[:, t] = h
        fd[:, t] = (neg_log_p(o64, x, q, prior, np.exp(ls + d), z) -
                    neg_log_p(o64, x, q, prior, np.exp(ls - d), z)) / (2 * h)
    scale = np.abs(fd).max()
    err = np.abs(ref["g_log_sigma"] - fd).max() / scale
    assert err < 1e-6, (err, scale)


def test_dreg_is_the_gradient_of_the_squared_weight_surrogate(o64, inputs):
    """g_q = -d/dq sum_k stop(w~_k^2) f_k(q), f_k = log w_k with log q's parameters frozen: the restated formula."""
    x, q, prior, sigma = inputs
    n, K = x.shape[0], 7
    z = np.random.default_rng(7).standard_normal((n, K, 2))
    ref = iw_grad_reference(o64, x, q, prior, sigma, z)
    w2 = ref["w"] ** 2
    h = 1e-5
    for k in range(5):
        d = np.zeros_like(q)
        d[:, k] = h
        fd = -((w2 * frozen_log_weights(o64, x, q + d, q, prior, sigma, z)).sum(1) -
               (w2 * frozen_log_weights(o64, x, q - d, q, prior, sigma, z)).sum(1)) / (2 * h)
        scale = np.abs(fd).max() + 1e-3
        err = np.abs(ref["g_q"][:, k] - fd).max() / scale
        assert err < 1e-5, (k, err, scale)


def test_k1_is_the_stop_gradient_elbo_gradient(o64, inputs):
    """At K = 1 (w~ = 1) DReG is the reference's gradient of nll + KL with q stop-gradient inside log q and the KL drawn
    at the likelihood's draw: _refine_reference.nll_grad plus the KL draw's gradient in elbo_bwd_kernel's whitened
    moment form (A0 + A1 z0 + A2 z1, B0 + B1 z0 + B2 z1)."""
    x, q, prior, sigma = inputs
    n = x.shape[0]
    z = np.random.default_rng(8).standard_normal((n, 1, 2))
    ref = iw_grad_reference(o64, x, q, prior, sigma, z)
    tq = [3.0 * np.tanh(q[:, 1]) - 1.0, 3.0 * np.tanh(q[:, 3]) - 1.0, np.tanh(q[:, 4]) * np.exp(-2.0)]
    tp = [3.0 * np.tanh(prior[:, 1]) - 1.0, 3.0 * np.tanh(prior[:, 3]) - 1.0, np.tanh(prior[:, 4]) * np.exp(-2.0)]
    e_so, e_sd = np.exp(tq[0]), np.exp(tq[1])
    qi_so, qi_sd, qi_bl = np.exp(-tq[0]), np.exp(-tq[1]), -np.exp(-tq[0] - tq[1]) * tq[2]
    pi_so, pi_sd, pi_bl = np.exp(-tp[0]), np.exp(-tp[1]), -np.exp(-tp[0] - tp[1]) * tp[2]
    dmo, dmd = q[:, 0] - prior[:, 0], q[:, 2] - prior[:, 2]
    d0, m00 = dmo * pi_so, e_so * pi_so
    d1 = dmd * pi_sd + dmo * pi_bl
    m10, m11 = tq[2] * pi_sd + e_so * pi_bl, e_sd * pi_sd
    A0, A1, A2 = d0 * pi_so + d1 * pi_bl, m00 * pi_so + m10 * pi_bl - qi_so, m11 * pi_bl - qi_bl
    B0, B1, B2 = d1 * pi_sd, m10 * pi_sd, m11 * pi_sd - qi_sd
    z0, z1 = z[:, 0, 0], z[:, 0, 1]
    ga, gb = A0 + A1 * z0 + A2 * z1, B0 + B1 * z0 + B2 * z1
    g_kl = np.stack([ga, ga * z0 * e_so, gb, gb * z1 * e_sd, gb * z0], -1)
    want = to_raw(q, nll_grad(o64, x, q, sigma, z) + g_kl)
    np.testing.assert_allclose(ref["g_q"], want, rtol=1e-10, atol=1e-10 * np.abs(want).max())
