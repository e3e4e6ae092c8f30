"""Host-side checks of the refinement under the TV smoothness prior: the float64 restatement the GPU tests hold
qbold_refine_posterior_spatial to (tests/_refine_tv_reference.py) against the CPU oracle's smoothness_loss, its
subgradient against central differences, its Jacobi loop at w = 0 against the per-voxel loop, the C ABI entry and
the argument checks that raise before any launch.  No GPU needed."""
import numpy as np
import pytest

from _refine_reference import padded_draws, refine_reference
from _refine_tv_reference import refine_tv_reference, tv_grad, tv_value


def _crop(rng, lead, keep=0.7):
    q = rng.normal(size=lead + (5,))
    mask = (rng.uniform(size=lead) < keep).astype(np.float64)
    return q, mask


@pytest.mark.parametrize("lead", [(2, 19, 13, 4), (1, 7, 9, 3), (3, 1, 6, 2), (1, 5, 1, 1)])
def test_tv_value_is_the_oracle_smoothness_sum(oracle64, lead):
    rng = np.random.default_rng(sum(lead))
    for keep in (1.0, 0.6):
        q, mask = _crop(rng, lead, keep)
        if mask.sum() == 0:
            mask.flat[0] = 1.0
        want = oracle64.smoothness_loss(q, mask) * mask.sum()
        np.testing.assert_allclose(tv_value(q, mask), want, rtol=1e-12, atol=1e-12)


def test_tv_subgradient_matches_central_differences():
    rng = np.random.default_rng(3)
    lead = (2, 9, 7, 3)
    q, mask = _crop(rng, lead)
    g, gap = tv_grad(q, mask, w=2.5)
    assert gap > 1e-4   # away from ties: |.| is smooth within h of q
    h = 1e-5
    assert not np.any(g[..., [1, 3, 4]])
    fd = np.zeros_like(q)
    for idx in np.ndindex(*lead):
        for ch in (0, 2):
            d = np.zeros_like(q)
            d[idx + (ch,)] = h
            fd[idx + (ch,)] = 2.5 * (tv_value(q + d, mask) - tv_value(q - d, mask)) / (2 * h)
    np.testing.assert_allclose(g, fd, rtol=1e-6, atol=1e-8)
    assert not np.any(g[mask == 0])   # masked voxels take no TV gradient


def test_tv_subgradient_sign_of_zero_is_zero():
    q = np.zeros((1, 3, 1, 1, 5))
    q[0, 2, 0, 0, 0] = 1.0
    g, gap = tv_grad(q, np.ones((1, 3, 1, 1)))
    assert gap == 0.0
    assert g[0, 0, 0, 0, 0] == 0.0 and g[0, 1, 0, 0, 0] < 0.0 and g[0, 2, 0, 0, 0] > 0.0
    assert not np.any(g[..., 2])


@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_jacobi_loop_at_zero_weight_is_the_per_voxel_loop(params, opt):
    from oracle.oracle import Oracle, init_weights, synth_inputs
    o32 = Oracle("f32", params)
    o64 = Oracle("f64", params, node0_zero=True)
    try:
        lead = (1, 4, 3, 2)
        n, S, steps = int(np.prod(lead)), 2, 4
        x, _ = synth_inputs(n, params, seed=5, oracle=o32)
        w = init_weights(T=o32.T, U=60, L=2, seed=3)
        w["gate_offset"] = -3.0
        prior, q, sigma = o32.encoder_fwd(w, x)
        z = np.random.default_rng(2).standard_normal((n, steps, padded_draws(S), 2))
        lr = 1e-2 if opt == "adam" else 1e-4
        want = refine_reference(o64, x, q, prior, sigma, z, S, lr=lr, lr_final=0.0, optimizer=opt)
        r = lambda a: a.reshape(lead + a.shape[-1:])   # noqa: E731
        got, _ = refine_tv_reference(o64, r(x), np.ones(lead), r(q), r(prior), r(sigma), z, S, 0.0, lr=lr,
                                     lr_final=0.0, optimizer=opt)
        np.testing.assert_allclose(got.reshape(-1, 5), want, rtol=1e-12, atol=1e-14)
        # a masked voxel keeps its heads; with w = 0 the others do not see it
        mask = np.ones(lead)
        mask[0, 1, 1, 0] = 0.0
        got_m, _ = refine_tv_reference(o64, r(x), mask, r(q), r(prior), r(sigma), z, S, 0.0, lr=lr, lr_final=0.0,
                                       optimizer=opt)
        np.testing.assert_array_equal(got_m[0, 1, 1, 0], q.reshape(lead + (5,))[0, 1, 1, 0])
        live = mask.reshape(-1) > 0
        np.testing.assert_allclose(got_m.reshape(-1, 5)[live], want[live], rtol=1e-12, atol=1e-14)
    finally:
        o64.lib.qbo_set_node0_zero(0)


def test_abi_declares_the_entry_point():
    import os
    from qbold_vi_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "qbold_hip.h")) as f:
        hdr = f.read()
    assert "int qbold_refine_posterior_spatial(" in hdr
    assert "int64_t qbold_refine_spatial_workspace_bytes(const qbold_ctx* ctx, const qbold_geometry* geom);" in hdr
    assert "#define QBOLD_ABI_VERSION 5" in hdr
    _, args = _lib.SIGNATURES["qbold_refine_posterior_spatial"]
    assert len(args) == 18
    _, args = _lib.SIGNATURES["qbold_refine_spatial_workspace_bytes"]
    assert len(args) == 2


@pytest.fixture(scope="module")
def host_ctx(params):
    from qbold_vi_amd.ops import Context
    return Context(params, host_only=True)


@pytest.mark.parametrize("kw,err", [
    (dict(steps=0), ValueError), (dict(S=0), ValueError), (dict(lr=0.0), ValueError),
    (dict(lr_final=-0.1), ValueError), (dict(optimizer="rmsprop"), ValueError),
    (dict(steps=1 << 31, S=5), ValueError), (dict(tv_weight=-1.0), ValueError),
    (dict(tv_weight=float("nan")), ValueError), (dict(tv_weight=float("inf")), ValueError),
])
def test_context_refine_spatial_checks_arguments_before_launch(host_ctx, kw, err):
    torch = pytest.importorskip("torch")
    t = torch.zeros((1, 2, 2, 1, 11))
    q = torch.zeros((1, 2, 2, 1, 5))
    kw = dict(dict(tv_weight=5.0), **kw)
    with pytest.raises(err):
        host_ctx.refine_posterior_spatial(t, None, q, q, t, **kw)


def test_context_refine_spatial_needs_device_tensors(host_ctx):
    torch = pytest.importorskip("torch")
    from qbold_vi_amd._lib import QboldError
    t = torch.zeros((1, 2, 2, 1, 11))
    q = torch.zeros((1, 2, 2, 1, 5))
    with pytest.raises(QboldError, match="no CPU fallback"):
        host_ctx.refine_posterior_spatial(t, None, q, q, t, 5.0)


def test_fine_tuner_refine_with_smoothness_rejects_the_diagonal_family():
    from qbold_vi_amd.model import FineTuner

    class _Tr:
        _use_mvg = False
        _heteroscedastic_noise = True
        _use_population_prior = False
        _mog_components = 1
        _seed = 1

    ft = FineTuner(_Tr(), None, None)
    with pytest.raises(NotImplementedError, match="diagonal family"):
        ft.refine(None, None, None, smoothness_weight=5.0)


def test_fine_tuner_refine_with_smoothness_needs_image_data():
    torch = pytest.importorskip("torch")
    from qbold_vi_amd.model import FineTuner

    class _Tr:
        _use_mvg = True
        _heteroscedastic_noise = True
        _use_population_prior = False
        _mog_components = 1
        _seed = 1

    ft = FineTuner(_Tr(), None, None)
    with pytest.raises(ValueError, match="image data"):
        ft.refine(torch.zeros((8, 11)), None, torch.zeros((8, 5)), smoothness_weight=5.0)
