"""Host-side checks of the exact posterior by quadrature: the float64 restatement of qbold_posterior_grid that the GPU
tests hold the kernel to (tests/_grid_reference.py) against closed forms and its own diagnostics, the C ABI entry, and
the argument checks of Context.posterior_grid and FineTuner.posterior_grid that raise before any launch.  No GPU
needed."""
import os
import re

import numpy as np
import pytest
from statistics import NormalDist

import _grid_reference as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ident = lambda u: u   # noqa: E731


def _gauss(mu, cov):
    P = np.linalg.inv(cov)
    c = -np.log(2 * np.pi) - 0.5 * np.log(np.linalg.det(cov))

    def logj(A, B):
        da, db = A - mu[0], B - mu[1]
        return c - 0.5 * (P[0, 0] * da * da + 2 * P[0, 1] * da * db + P[1, 1] * db * db)
    return logj


def test_correlated_gaussian_closed_form():
    """log Z = 0 (the density is normalised), means, sds, correlation exact to 1e-6 at the defaults; quantiles are
    those of a CDF linear within a cell, so they converge as h^2: within 1e-2 sd at fine = 64, 1e-3 sd at 256."""
    mu = np.array([0.3, -1.2])
    sa, sb, rho = 0.7, 0.4, 0.8
    cov = np.array([[sa * sa, rho * sa * sb], [rho * sa * sb, sb * sb]])
    logj = _gauss(mu, cov)
    box0 = np.array([mu[0] - 6 * 2 * sa, mu[0] + 6 * 2 * sa, mu[1] - 6 * 2 * sb, mu[1] + 6 * 2 * sb])
    out, box = gr.posterior_grid(logj, box0, ta=ident, tb=ident, dw=1.0)
    assert abs(out[0]) < 1e-6
    np.testing.assert_allclose(out[2:4], mu, atol=1e-6)
    np.testing.assert_allclose(out[4], mu[0] * mu[1] + rho * sa * sb, atol=1e-6)   # E[ab]
    np.testing.assert_allclose(out[5:7], [sa, sb], rtol=1e-6)
    var_ab = (sa * sb) ** 2 * (1 + rho ** 2) + mu[0] ** 2 * sb ** 2 + mu[1] ** 2 * sa ** 2 + \
        2 * mu[0] * mu[1] * rho * sa * sb
    np.testing.assert_allclose(out[7], np.sqrt(var_ab), rtol=1e-6)
    np.testing.assert_allclose(out[8], rho, atol=1e-6)
    z = np.array([NormalDist().inv_cdf(0.025), NormalDist().inv_cdf(0.975)])
    for n, tol in ((64, 1e-2), (256, 1e-3)):
        o, _ = gr.posterior_grid(logj, box0, fine=n, ta=ident, tb=ident)
        assert np.all(np.abs(o[9:11] - (mu[0] + sa * z)) < tol * sa), (n, o[9:11])
        assert np.all(np.abs(o[11:13] - (mu[1] + sb * z)) < tol * sb), (n, o[11:13])
    np.testing.assert_allclose(out[13:15], mu, atol=0.5 * (box[1] - box[0]) / 63 + 0.5 * (box[3] - box[2]) / 63)
    assert out[15] < 1e-12 and out[16] < 1e-6


def test_banana_converges_with_fine():
    """A banana-shaped density (a ~ N(0, 1), b | a ~ N(a^2 - 1, 0.1^2)): the moments converge as the fine grid
    grows, to the analytic ones."""
    def logj(A, B):
        r = (B - A * A + 1.0) / 0.1
        return -np.log(2 * np.pi * 0.1) - 0.5 * (A * A + r * r)
    box0 = np.array([-8.0, 8.0, -4.0, 30.0])
    errs = []
    for n in (32, 64, 128, 256):
        o, _ = gr.posterior_grid(logj, box0, coarse=64, fine=n, ta=ident, tb=ident)
        # log Z = 0, E[a] = 0, E[b] = 0, sd(a) = 1, sd(b) = sqrt(2 + 0.01)
        errs.append(max(abs(o[0]), abs(o[2]), abs(o[3]), abs(o[5] - 1), abs(o[6] - np.sqrt(2.01))))
    assert errs[-1] < 1e-4 and errs[-1] < 1e-4 * errs[0], errs
    assert all(e2 <= e1 * 1.01 + 1e-12 for e1, e2 in zip(errs, errs[1:])), errs


def test_diagnostics_grow_when_the_grid_is_too_coarse_or_too_small():
    mu, cov = np.array([0.0, 0.0]), np.array([[1.0, 0.95], [0.95, 1.0]])
    logj = _gauss(mu, cov)
    box0 = np.array([-12.0, 12.0, -12.0, 12.0])
    # quad_err compares with the 2h grid, so it is conservative: at rho = 0.95 the default 64-node grid's log Z is
    # exact to 1e-10 while its 32-node half is not
    good, _ = gr.posterior_grid(logj, box0, fine=256)
    coarse, _ = gr.posterior_grid(logj, box0, fine=16, locate_passes=1, cut=10.0)
    assert good[16] < 1e-6 and coarse[16] > 1e-4 and coarse[16] > 1e3 * good[16]
    assert abs(coarse[0]) > abs(good[0])
    small = np.array([-0.5, 0.5, -0.5, 0.5])   # span too small: the box truncates the posterior
    trunc, _ = gr.posterior_grid(logj, small)
    assert good[15] < 1e-12 and trunc[15] > 1e-2
    assert trunc[0] < -0.5


def test_oracle_voxel_reference_agrees_with_the_dense_one(oracle64, params):
    """One real voxel: the default grid against the 481^2 two-stage reference."""
    from oracle.oracle import Oracle, synth_inputs
    x, _ = synth_inputs(2, params, seed=21, oracle=Oracle("f32", params))
    sigma = np.full(11, 0.05)
    prior = np.array([-0.2, 0.3, -2.0, 0.3, 0.0])
    J = gr.VoxelJoint(oracle64, x[0], sigma, prior)
    out, _ = gr.voxel_reference(oracle64, x[0], sigma, prior, q=prior, gh=16)
    ref, _ = gr.dense(J, gr.start_box(prior))
    assert abs(out[0] - ref[0]) < 1e-3
    assert np.all(np.abs(out[2:5] / ref[2:5] - 1) < 1e-3)
    assert out[1] <= out[0]   # ELBO(q) <= log p(x)


def test_header_declares_the_entry():
    h = open(os.path.join(ROOT, "include", "qbold_hip.h")).read()
    assert re.search(r"int qbold_posterior_grid\(const qbold_ctx\* ctx, const float\* x, const float\* mask,", h)
    assert "} qbold_grid_cfg;" in h and re.search(r"#define QBOLD_GRID_OUT 17\b", h)
    assert re.search(r"#define QBOLD_ABI_VERSION 5\b", h)
    from qbold_vi_amd import _lib
    assert "qbold_posterior_grid" in _lib.SIGNATURES and _lib.QBOLD_GRID_OUT == 17


BAD = [dict(coarse=24 + 1), dict(coarse=8), dict(coarse=136), dict(fine=12), dict(fine=264), dict(fine=70),
       dict(locate=0), dict(locate=5), dict(gh=1), dict(gh=33), dict(gh=-1), dict(span=0.0), dict(span=-1.0),
       dict(cut=9.0), dict(cut=81.0), dict(levels=(0.0, 0.5)), dict(levels=(0.5, 0.5)), dict(levels=(0.1, 1.0)),
       dict(levels=(0.9, 0.1))]


@pytest.mark.parametrize("kw", BAD, ids=[str(k) for k in BAD])
def test_context_refuses_bad_arguments(params, kw):
    import torch
    from qbold_vi_amd.ops import Context
    ctx = Context(params, True, True, host_only=True)
    n = 4
    x, p, s = torch.ones(n, 11), torch.zeros(n, 5), torch.ones(n, 11)
    with pytest.raises(ValueError):
        ctx.posterior_grid(x, None, p, s, **kw)


def test_context_refuses_cpu_tensors(params):
    import torch
    from qbold_vi_amd.ops import Context
    ctx = Context(params, True, True, host_only=True)
    with pytest.raises(ValueError, match="cuda"):
        ctx.posterior_grid(torch.ones(4, 11), None, torch.zeros(4, 5), torch.ones(4, 11))


def test_fine_tuner_refuses_the_diagonal_family_and_the_population_prior():
    from qbold_vi_amd.model import FineTuner

    class _Tr:
        _use_mvg = False
        _heteroscedastic_noise = True
        _use_population_prior = False
        _mog_components = 1
        _seed = 1

    with pytest.raises(NotImplementedError, match="diagonal family"):
        FineTuner(_Tr(), None, None).posterior_grid(None, None, None)
    _Tr._use_mvg = True
    _Tr._use_population_prior = True
    with pytest.raises(NotImplementedError, match="population prior"):
        FineTuner(_Tr(), None, None).posterior_grid(None, None, None)
