"""The float64 restatement of qbold_laplace_posterior (tests/_laplace_reference.py) checked against itself and against
tests/_grid_reference.py on the CPU: the gradient against central differences of F, the Gauss-Newton matrix against
the finite-difference Hessian where it is exact, the heads' round trip and clamp rule, the log-joint's constants, the
conditions the GPU tests put on the seeded inputs (the float64 Levenberg-Marquardt converges on every voxel within half
of max_iter), and the argument checks that are raised before any launch."""
import math
import os
import re

import numpy as np
import pytest

import _grid_reference as gr
import _laplace_reference as lr
from test_gpu_forward_protocols import float64_oracle

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_PROTOCOLS = ("ref11", "odd33_3img", "off22", "two")


def _case(params, name):
    from oracle.oracle import Oracle
    p, sw = lr.setup(params, name)
    d = lr.inputs(Oracle("f32", p, **sw), name)
    return p, sw, d


@pytest.mark.parametrize("name", FD_PROTOCOLS)
def test_gradient_matches_central_differences_of_F(params, name):
    p, sw, d = _case(params, name)
    rows = np.arange(24)
    rng = np.random.default_rng(3)
    with float64_oracle(p, sw) as o64:
        m = lr.model_of(o64, d, sw, rows)
        u = d["u_true"][rows] + 0.3 * rng.standard_normal((24, 2))
        g = m.evaluate(u)["g"]
        h = 1e-5
        for k in range(2):
            e = np.zeros(2)
            e[k] = h
            fd = (m.F(u + e) - m.F(u - e)) / (2 * h)
            scale = np.abs(fd).max() + 1e-3
            err = np.max(np.abs(g[:, k] - fd)) / scale
            print(name, "coordinate", k, "scale", scale, "err", err)
            # central differences at h = 1e-5: h^2 F''' / 6 ~ 1e-10 F plus the rounding 1e-16 F / h ~ 1e-11 F
            assert err < 1e-6


@pytest.mark.parametrize("name", FD_PROTOCOLS)
def test_gauss_newton_is_the_hessian_on_noise_free_data_at_the_truth(params, name):
    """Noise-free float64 data and the prior centred on the truth: every residual row is 0 at the truth, where the
    second-order term sum r_t grad^2 r_t vanishes and J^T J is the Hessian of F."""
    p, sw, d = _case(params, name)
    n = 16
    with float64_oracle(p, sw) as o64:
        x = np.asarray(o64.signal_fwd(d["truth"][:n]), np.float64)
        prior = np.array(d["prior"][:n], np.float64)
        prior[:, 0], prior[:, 2] = d["u_true"][:n, 0], d["u_true"][:n, 1]
        m = lr.Model(o64, x, d["sigma"][:n], prior, multi=bool(sw))
        u = d["u_true"][:n]
        ev = m.evaluate(u)
        assert np.all(ev["F"] < 1e-20) and np.all(ev["dec"] < 1e-9)
        h = 1e-5
        H = np.zeros((n, 2, 2))
        for k in range(2):
            e = np.zeros(2)
            e[k] = h
            H[:, :, k] = (m.evaluate(u + e)["g"] - m.evaluate(u - e)["g"]) / (2 * h)
        scale = np.abs(ev["A"]).max(axis=(1, 2), keepdims=True)
        err = np.max(np.abs(H - ev["A"]) / scale)
        print(name, "max |H_fd - A| / max |A|", err)
        assert err < 1e-6


def test_heads_round_trip_unclamped_and_clamped():
    rng = np.random.default_rng(5)
    n = 200
    sd_a, sd_b = np.exp(rng.uniform(-5.0, 2.5, n)), np.exp(rng.uniform(-5.0, 2.5, n))
    corr = rng.uniform(-0.95, 0.95, n)
    corr[:60] *= 0.05                                          # |c| = |corr| sd_b < e^-2 for most of these
    sd_a[:60], sd_b[:60] = np.exp(rng.uniform(-3, 1.5, 60)), np.exp(rng.uniform(-3, 0.0, 60))
    Sigma = np.zeros((n, 2, 2))
    Sigma[:, 0, 0], Sigma[:, 1, 1] = sd_a ** 2, sd_b ** 2
    Sigma[:, 0, 1] = Sigma[:, 1, 0] = corr * sd_a * sd_b
    u = rng.standard_normal((n, 2))
    q, clamped = lr.heads_from(u, Sigma)
    assert 20 < clamped.sum() < n - 20
    mu, S2 = lr.heads_cov(q)
    assert np.array_equal(mu, u)
    ok = ~clamped
    # atanh then tanh near saturation: 1 - tanh^2 >= 2e-6 amplifies float64 rounding to ~1e-10 at the clamp
    assert np.max(np.abs(S2[ok] - Sigma[ok]) / np.abs(Sigma[ok]).max(axis=(1, 2), keepdims=True)) < 1e-8
    # the clamp rule: s_o, c clamped just inside their ranges; e^(2 s_d) = Sigma_bb - c^2 with the stored c
    s_lo, s_hi, c_max = 3 * -lr.TANH_MAX - 1, 3 * lr.TANH_MAX - 1, lr.TANH_MAX * math.exp(-2.0)
    so = np.clip(0.5 * np.log(Sigma[:, 0, 0]), s_lo, s_hi)
    c = np.clip(Sigma[:, 0, 1] / np.sqrt(Sigma[:, 0, 0]), -c_max, c_max)
    sd = np.clip(0.5 * np.log(Sigma[:, 1, 1] - c * c), s_lo, s_hi)
    np.testing.assert_allclose(S2[:, 0, 0], np.exp(2 * so), rtol=1e-8)
    np.testing.assert_allclose(S2[:, 0, 1], c * np.exp(so), rtol=1e-8, atol=1e-300)
    np.testing.assert_allclose(S2[:, 1, 1], c * c + np.exp(2 * sd), rtol=1e-8)
    # the marginal variance of b survives a clamped c (whenever s_d itself is in range)
    keeps = clamped & (sd > s_lo) & (sd < s_hi)
    assert keeps.sum() > 10
    np.testing.assert_allclose(S2[keeps, 1, 1], Sigma[keeps, 1, 1], rtol=1e-8)


@pytest.mark.parametrize("name", ("ref11", "odd33_3img"))
def test_log_joint_is_the_grids_up_to_the_stated_constants(params, name):
    p, sw, d = _case(params, name)
    rng = np.random.default_rng(2)
    with float64_oracle(p, sw) as o64:
        m = lr.model_of(o64, d, sw, np.arange(6))
        for i in range(6):
            J = gr.VoxelJoint(o64, d["x"][i], d["sigma"][i], d["prior"][i])
            u = d["u_true"][i] + rng.standard_normal((5, 2))
            got = m.log_joint(u, np.full(5, i))
            want = J(u[:, 0], u[:, 1])
            assert np.max(np.abs(got - want) / (np.abs(want) + 1.0)) < 1e-10, (i, got, want)


def test_fine_tuner_laplace_refuses_the_diagonal_family_and_the_population_prior():
    from qbold_vi_amd.model import FineTuner

    class _Tr:
        _use_mvg = False
        _heteroscedastic_noise = True
        _use_population_prior = False
        _mog_components = 1
        _seed = 1

    with pytest.raises(NotImplementedError, match="diagonal family"):
        FineTuner(_Tr(), None, None).laplace(None, None, None)
    _Tr._use_mvg = True
    _Tr._use_population_prior = True
    with pytest.raises(NotImplementedError, match="population prior"):
        FineTuner(_Tr(), None, None).laplace(None, None, None)


@pytest.mark.parametrize("name", lr.protocol_names())
def test_float64_lm_converges_on_every_seeded_voxel_within_half_of_max_iter(params, name):
    """A condition on the inputs and the reference alone: the GPU tests ask the kernel to converge on every voxel."""
    p, sw, d = _case(params, name)
    assert d["x"].shape[0] == lr.N_VOX == 333
    assert 0 < (~d["live"]).sum() < lr.N_VOX
    assert np.all((d["truth"][:, 0] >= 0.2) & (d["truth"][:, 0] <= 0.6))
    assert np.all((d["truth"][:, 1] >= 0.02) & (d["truth"][:, 1] <= 0.1))
    with float64_oracle(p, sw) as o64:
        m = lr.model_of(o64, d, sw)
        res = lr.lm(m, **lr.DEFAULTS)
        start = m.evaluate(m.mu)
    print(name, "iterations max", res["iterations"].max(), "mean", res["iterations"].mean(),
          "dec max", res["ev"]["dec"].max())
    assert res["converged"].all()
    assert res["iterations"].max() <= lr.DEFAULTS["max_iter"] // 2
    assert np.all(res["ev"]["dec"] < lr.DEFAULTS["tol"])
    assert np.all(res["ev"]["F"] <= start["F"])


def test_argument_checks_are_raised_before_any_launch(params):
    from qbold_vi_amd.ops import Context
    ctx = Context(params, True, True, host_only=True)
    x, p5, sg = torch.ones(4, 11), torch.zeros(4, 5), torch.ones(4, 11)
    for kw in (dict(max_iter=0), dict(tol=0.0), dict(tol=float("nan")), dict(lambda0=-1.0), dict(lambda0=float("inf")),
               dict(lambda_up=1.0), dict(lambda_down=0.5)):
        with pytest.raises(ValueError, match="laplace_posterior"):
            ctx.laplace_posterior(x, None, p5, sg, **kw)
    with pytest.raises(ValueError, match="cuda"):
        ctx.laplace_posterior(x, None, p5, sg)


def test_header_binding_and_build_list_agree():
    from qbold_vi_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "qbold_hip.h")).read()
    assert re.search(r"#define QBOLD_ABI_VERSION 5\b", hdr)       # additions only
    assert re.search(r"#define QBOLD_LAPLACE_OUT 15\b", hdr) and _lib.QBOLD_LAPLACE_OUT == 15 == lr.OUT_COLUMNS
    args = re.search(r"int qbold_laplace_posterior\((.*?)\);", hdr, re.S).group(1)
    assert len(args.split(",")) == len(_lib.SIGNATURES["qbold_laplace_posterior"][1]) == 11
    assert [n for n, _ in _lib.LaplaceCfg._fields_] == ["max_iter", "lambda0", "lambda_up", "lambda_down", "tol"]
    assert "laplace_kernels.hip" in build.SOURCES
    assert hasattr(_lib.load(), "qbold_laplace_posterior")
