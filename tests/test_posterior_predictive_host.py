"""Host-side checks of the posterior predictive checks: the float64 reference the GPU tests hold
qbold_posterior_predictive to (tests/_ppc_reference.py) against the oracle's NLL and scipy, the Rao-Blackwellised
p-value against simulated replicates, the C ABI entry, the sums helper and the argument checks.  No GPU needed."""
import os
import re

import numpy as np
import pytest

from _ppc_reference import chi2_sf, draws, ppc_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SWITCHES = {
    "gaussian": {},
    "student_t": dict(student_t_df=5.0),
    "log_data": dict(predict_log_data=True),
    "three_image_norm": dict(multi_image_normalisation=True),
}


def _inputs(o32, params, n, seed):
    from oracle.oracle import init_weights, synth_inputs
    x, _ = synth_inputs(n, params, seed=seed, oracle=o32)
    w = init_weights(T=11, U=60, L=2, seed=3)
    w["gate_offset"] = -3.0
    _, q, sigma = o32.encoder_fwd(w, x)
    return x, q, sigma


@pytest.mark.parametrize("case", list(SWITCHES))
def test_per_tau_log_density_sums_to_the_oracle_nll(params, case):
    from oracle.oracle import Oracle
    sw = SWITCHES[case]
    o32, o64 = Oracle("f32", params, **sw), Oracle("f64", params, **sw)
    n, L = 32, 8
    x, q, sigma = _inputs(o32, params, n, 5)
    z = np.random.default_rng(1).standard_normal((n, L, 2))
    _, _, _, lp = draws(o64, x, q, sigma, z)
    T = o64.T
    th = o64.reparam(np.repeat(q.astype(np.float64), L, axis=0), z.reshape(-1, 2))
    rep = lambda a: np.repeat(np.asarray(a, np.float64), L, axis=0)   # noqa: E731
    nll = o64.nll(rep(x), np.ones(n * L), o64.signal_fwd(th), rep(sigma)).reshape(n, L)
    assert T == 11
    np.testing.assert_allclose(lp.sum(-1), -nll, rtol=1e-12, atol=1e-10)


def test_chi2_tail_equals_scipy():
    from scipy.stats import chi2
    D = np.concatenate([np.linspace(0.0, 5.0, 51), np.linspace(5.0, 200.0, 196), [500.0, 1e4, 1e6]])
    for T in (1, 2, 7, 11, 24, 33, 64):
        got, want = chi2_sf(T, D), chi2.sf(D, T)
        assert np.all(np.isfinite(got)), T
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-300)


def test_rao_blackwellised_ppp_equals_simulated_replicates(oracle64, params):
    """ppp = mean_l P(D(y_rep, theta_l) >= D(y, theta_l)) with y_rep ~ N(yh_l, sigma^2): simulate the replicates."""
    from oracle.oracle import Oracle
    x, q, sigma = _inputs(Oracle("f32", params), params, 3, 9)
    # a misfit voxel (small ppp), a typical one, and one with its sigma doubled (ppp near 1)
    sigma = sigma.astype(np.float64).copy()
    sigma[0] *= 0.35
    sigma[2] *= 2.0
    x = x.astype(np.float64)
    L, R = 16, 8192
    z = np.random.default_rng(4).standard_normal((3, L, 2))
    ref = ppc_reference(oracle64, x, q, sigma, z)
    rng = np.random.default_rng(6)
    T = oracle64.T
    for i in range(3):
        yh = draws(oracle64, x[i:i + 1], q[i:i + 1], sigma[i:i + 1], z[i:i + 1])[1][0]   # [L, T]
        eps = rng.standard_normal((L, R, T))
        y_rep = yh[:, None, :] + sigma[i][None, None, :] * eps
        d_rep = (((y_rep - yh[:, None, :]) / sigma[i][None, None, :]) ** 2).sum(-1)   # [L, R]
        hit = d_rep >= ref["D"][i][:, None]
        brute = hit.mean()
        se = max(np.sqrt(hit.mean(1).var() / L + brute * (1 - brute) / (L * R)), 1.0 / (L * R))
        assert abs(brute - ref["out"][i, 0]) < 3.0 * se + 1e-12, (i, brute, ref["out"][i, 0], se)


def test_header_declares_the_entry():
    h = open(os.path.join(ROOT, "include", "qbold_hip.h")).read()
    assert re.search(r"int qbold_posterior_predictive\(const qbold_ctx\* ctx, const float\* x, const float\* mask,", h)
    assert re.search(r"#define QBOLD_PPC_OUT 6\b", h)
    assert re.search(r"#define QBOLD_ABI_VERSION 5\b", h)
    from qbold_vi_amd import _lib
    from qbold_vi_amd.ops import Context
    assert "qbold_posterior_predictive" in _lib.SIGNATURES and _lib.QBOLD_PPC_OUT == 6
    assert len(Context.PPC_COLUMNS) == 6


def test_ppc_from_sums():
    from qbold_vi_amd.distributed import ppc_from_sums
    elpd = np.array([-3.0, -5.0, 1.0])
    pw = np.array([0.5, 1.5, 0.25])
    ppp = np.array([0.2, 0.9, 0.01])
    m = np.array([1.0, 2.0, 0.5])
    sums = np.array([(m * elpd).sum(), (m * pw).sum(), (m * ppp).sum(), m.sum()])
    got = ppc_from_sums(sums)
    np.testing.assert_allclose(got, [(m * elpd).sum() / 3.5, (m * pw).sum() / 3.5, (m * ppp).sum() / 3.5])


@pytest.mark.parametrize("L", [1, 0, -3, (1 << 30) + 1])
def test_context_refuses_bad_draw_counts(params, L):
    import torch
    from qbold_vi_amd.ops import Context
    ctx = Context(params, True, True, host_only=True)
    with pytest.raises(ValueError):
        ctx.posterior_predictive(torch.ones(4, 11), None, torch.zeros(4, 5), torch.ones(4, 11), L=L)


def test_context_refuses_cpu_tensors(params):
    import torch
    from qbold_vi_amd.ops import Context
    ctx = Context(params, True, True, host_only=True)
    with pytest.raises(ValueError, match="cuda"):
        ctx.posterior_predictive(torch.ones(4, 11), None, torch.zeros(4, 5), torch.ones(4, 11))


def test_fine_tuner_refuses_the_diagonal_family():
    from qbold_vi_amd.model import FineTuner

    class _Tr:
        _use_mvg = False
        _heteroscedastic_noise = True
        _use_population_prior = False
        _mog_components = 1
        _seed = 1

    with pytest.raises(NotImplementedError, match="diagonal family"):
        FineTuner(_Tr(), None, None).posterior_predictive(None, None)
