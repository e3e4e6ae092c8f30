"""Gradient of the importance-weighted bound (qbold_log_evidence_bwd, Context.log_evidence_bwd) and fine-tuning on it
(iw_samples): the doubly-reparameterised head gradient and the sigma gradient against the float64 reference
(tests/_iw_grad_reference.py), the Philox stream, agreement with qbold_log_evidence_fwd, bitwise properties,
unbiasedness and variance at scale, an optimisation check, argument errors and the training surface."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from _iw_grad_reference import iw_grad_reference
from _iw_reference import rel1

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IW_STREAM = 6
ERR_UNSUPPORTED = -3   # QBOLD_ERR_UNSUPPORTED


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _p24(params):
    return dict(params, tau_start="-0.028", tau_end="0.065", tau_step="0.004")


def _p64(params):
    return dict(params, tau_start="-0.015", tau_end="0.065", tau_step="0.00125")


def _case(o32, p, n, seed, spread=0.3, wide=False):
    """x, q (encoder heads plus noise), prior, log_sigma: float32 arrays."""
    from oracle.oracle import init_weights, synth_inputs
    x, _ = synth_inputs(n, p, seed=seed, oracle=o32)
    w = init_weights(T=o32.T, U=60, L=2, seed=3)
    w["gate_offset"] = -3.0
    prior, q, sigma = o32.encoder_fwd(w, x)
    rng = np.random.default_rng(seed)
    q = q + rng.normal(size=q.shape) * spread
    if wide:   # means near the logit clip and wide spreads: some draws reach +-13.8155
        q[:, 0] += np.where(rng.uniform(size=n) < 0.5, -12.5, 12.5)
        q[:, 1] = 0.5
        q[:, 3] = 0.5
    return x, q.astype(np.float32), prior, np.log(sigma).astype(np.float32)


@pytest.fixture(scope="module")
def ctx(params):
    from qbold_vi_amd.ops import Context
    c = Context(params, full_model=True, include_blood=True)
    c.set_grad_node0(False)
    return c


@pytest.fixture(scope="module")
def data11(params):
    from oracle.oracle import Oracle
    return tuple(dev(a) for a in _case(Oracle("f32", params), params, 4096, 1))


# name: (protocol, loss switches, wide heads)
CASES = {
    "T11": (None, {}, False),
    "three_image_norm": (None, dict(multi_image_normalisation=True), False),
    "T24": (_p24, {}, False),
    "student_t": (None, dict(student_t_df=5.0), False),
    "log_data": (None, dict(predict_log_data=True), False),
    "wide_heads_clip": (None, {}, True),
}
SIZES = [(48, 1), (48, 7), (48, 32), (48, 40), (1024, 7)]   # K = 40: the four-lane mapping


@pytest.mark.parametrize("case", list(CASES))
def test_matches_float64_reference(params, case):
    """Explicit normals: g_q (DReG) and g_log_sigma against the float64 reference, max|d| / scale < 2e-3 per column
    (test_one_sgd_step_is_the_gradient's bound), for a partial wave at K = 1, 7, 32 (one lane per voxel) and 40 (four
    lanes), and 1,024 voxels at K = 7 (that size on the T = 11 case only, to keep the float64 side near
    test_gpu_log_evidence's)."""
    from oracle.oracle import Oracle
    from qbold_vi_amd.ops import Context
    proto, sw, wide = CASES[case]
    p = proto(params) if proto else params
    c = Context(p, True, True, **sw)
    c.set_grad_node0(False)
    o32 = Oracle("f32", p, **sw)
    o64 = Oracle("f64", p, node0_zero=True, **sw)
    try:
        worst = [0.0, 0.0]
        for n, K in (SIZES if case == "T11" else SIZES[:4]):
            x, q, prior, ls = _case(o32, p, n, 5 + K, wide=wide)
            z = np.random.default_rng(K).standard_normal((n, K, 2)).astype(np.float32)
            if wide:
                assert np.abs(np.stack([q[:, 0:1] + z[..., 0] * np.exp(3 * np.tanh(0.5) - 1)], -1)).max() > 13.82
            sums, gq, gls, out = c.log_evidence_bwd(dev(x), None, dev(q), dev(prior), dev(ls), K, z=dev(z),
                                                    want_out=True)
            ref = iw_grad_reference(o64, x, q, prior, np.exp(ls.astype(np.float64)), z)
            for name, got, want in (("g_q", gq, ref["g_q"]), ("g_log_sigma", gls, ref["g_log_sigma"])):
                got = got.cpu().numpy().astype(np.float64)
                for k in range(want.shape[1]):
                    scale = np.abs(want[:, k]).max() + 1e-3
                    err = np.abs(got[:, k] - want[:, k]).max() / scale
                    worst[name == "g_log_sigma"] = max(worst[name == "g_log_sigma"], err)
                    assert err < 2e-3, (case, n, K, name, k, err, scale)
            assert rel1(out[:, 0].cpu().numpy(), ref["log_p"]) < 1e-3, case
        print(f"{case}: max err / scale  g_q {worst[0]:.2e}  g_log_sigma {worst[1]:.2e}")
    finally:
        o64.lib.qbo_set_node0_zero(0)


@pytest.mark.parametrize("K", [1, 40])
@pytest.mark.parametrize("case", ["T11", "T24"])
def test_default_node0_policy_per_voxel(params, case, K):
    """The shipped gradient policy (a context whose grad_node0 nobody set: the J1 sum over all Simpson nodes,
    iw_bwd_kernels.hip's restatement of fwd_signal_grad) against the reference given the oracle's analytic Jacobian.
    Every entry of every voxel, |d| <= 2e-4 A with A the same sum in absolute values (tests/_elbo_bwd_reference.py), next
    to test_matches_float64_reference's column-max bound; against the reference of the other policy the per-voxel
    measure misses by more than 10 x at K = 1 (at K = 40 the squared weights concentrate on few draws)."""
    from _elbo_bwd_reference import analytic_jac
    from oracle.oracle import Oracle
    from qbold_vi_amd.ops import Context
    proto, sw, _ = CASES[case]
    p = proto(params) if proto else params
    c = Context(p, True, True, **sw)
    o32 = Oracle("f32", p, **sw)
    o64 = Oracle("f64", p, node0_zero=True, **sw)
    try:
        n = 48
        x, q, prior, ls = _case(o32, p, n, 5 + K)
        mask = np.where(np.arange(n) % 5 == 2, 0.0, np.where(np.arange(n) % 3 == 0, 0.5, 1.0)).astype(np.float32)
        z = np.random.default_rng(K).standard_normal((n, K, 2)).astype(np.float32)
        _, gq, gls, _ = c.log_evidence_bwd(dev(x), dev(mask), dev(q), dev(prior), dev(ls), K, z=dev(z))
        sigma = np.exp(ls.astype(np.float64))
        ref = iw_grad_reference(o64, x, q, prior, sigma, z, mask=mask, jac=analytic_jac)
        other = iw_grad_reference(o64, x, q, prior, sigma, z, mask=mask)
        worst = {}
        for name, got, want, A in (("g_q", gq, ref["g_q"], ref["A_q"]), ("g_log_sigma", gls, ref["g_log_sigma"], ref["A_ls"])):
            got = got.cpu().numpy().astype(np.float64)
            assert np.all(got[mask == 0] == 0.0)
            d = np.abs(got - want)
            worst[name] = float(np.max(d[mask > 0] / A[mask > 0]))
            for k in range(want.shape[1]):
                assert d[:, k].max() / (np.abs(want[:, k]).max() + 1e-3) < 2e-3, (case, K, name, k)
            if name == "g_q":
                apart = float(np.max(np.abs(got - other["g_q"])[mask > 0] / other["A_q"][mask > 0]))
        print(f"{case} K={K}: worst |d| / A  g_q {worst['g_q']:.2e}  g_log_sigma {worst['g_log_sigma']:.2e}; "
              f"against the other policy {apart:.2e}")
        assert worst["g_q"] <= 2e-4 and worst["g_log_sigma"] <= 2e-4, (case, K, worst)
        if K == 1:
            assert apart > 2e-3
    finally:
        o64.lib.qbo_set_node0_zero(0)


@pytest.mark.parametrize("K", [1, 7, 16, 40])
def test_philox_stream_equals_explicit_normals(ctx, data11, K):
    x, q, prior, ls = (a[:777] for a in data11)
    seed, v0 = 11, 12345
    a = ctx.log_evidence_bwd(x, None, q, prior, ls, K, seed=seed, voxel0=v0, want_out=True)
    z = ctx.normals(777, K, stream_id=IW_STREAM, seed=seed, voxel0=v0)
    b = ctx.log_evidence_bwd(x, None, q, prior, ls, K, z=z, seed=seed, voxel0=v0, want_out=True)
    for u, v in zip(a, b):
        assert _same_bits(u, v)


@pytest.mark.parametrize("K", [1, 16])
def test_out_and_sums_equal_log_evidence(params, data11, K):
    """out and sums against qbold_log_evidence_fwd at sigma = exp(log_sigma), the same seed and voxel0: the sums within
    1e-5 rel1, every voxel's (log p^, ELBO_same, ESS) within 1e-4.  The backward scores a draw with elbo_bwd_kernel's
    signal arithmetic, the forward with its own (per-tau table by default, QBOLD_KSEL_X_TABLE: the x-indexed one);
    where sigma is small the NLL amplifies their float32 differences, to 2.3e-5 rel1 in a voxel here."""
    from qbold_vi_amd.ops import Context
    x, q, prior, ls = data11
    mask = dev((np.random.default_rng(2).uniform(size=x.shape[0]) > 0.25).astype(np.float32))
    for ksel in (8, 0):
        c = Context(params, True, True)
        c.set_kernel_selection(ksel)
        s1, _, _, o1 = c.log_evidence_bwd(x, mask, q, prior, ls, K, seed=4, voxel0=9, want_out=True)
        s2, o2, _ = c.log_evidence(x, mask, q, prior, torch.exp(ls), K, seed=4, voxel0=9)
        a, b = o1.cpu().numpy(), o2.cpu().numpy()
        errs = [rel1(a[:, j], b[:, j]) for j in range(3)]
        es = rel1(s1.cpu().numpy(), s2.cpu().numpy())
        print(f"K={K} ksel={ksel}: out rel1 (log p^, ELBO, ESS) {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}; sums {es:.2e}")
        assert max(errs) < 1e-4 and es < 1e-5, (ksel, errs, es)
        assert float(s1[2]) == float(mask.sum())


@pytest.mark.parametrize("K", [1, 16, 40])
def test_bitwise_properties(ctx, data11, K):
    x, q, prior, ls = data11
    n = x.shape[0]
    args = (x, None, q, prior, ls, K)
    a = ctx.log_evidence_bwd(*args, seed=3, voxel0=100, want_out=True)
    b = ctx.log_evidence_bwd(*args, seed=3, voxel0=100, want_out=True)
    for u, v in zip(a, b):   # run to run
        assert _same_bits(u, v)
    h = 1234   # two shards against one call
    sa = ctx.log_evidence_bwd(*(t[:h] if t is not None else None for t in args[:5]), K, seed=3, voxel0=100,
                              want_out=True)
    sb = ctx.log_evidence_bwd(*(t[h:] if t is not None else None for t in args[:5]), K, seed=3, voxel0=100 + h,
                              want_out=True)
    for i in (1, 2, 3):
        assert _same_bits(torch.cat([sa[i], sb[i]]), a[i])
    # a voxel moved to another batch position (its explicit normals move with it)
    z = ctx.normals(n, K, stream_id=IW_STREAM, seed=3, voxel0=100)
    perm = torch.as_tensor(np.random.default_rng(1).permutation(n), device="cuda")
    p = ctx.log_evidence_bwd(x[perm], None, q[perm], prior[perm], ls[perm], K, z=z[perm], want_out=True)
    for i in (1, 2, 3):
        assert _same_bits(p[i], a[i][perm])
    # masked and NaN-mask voxels: exact zeros, nothing in the sums; m = 0.5 halves the gradients exactly
    m = np.ones(n, np.float32)
    m[::3] = 0.0
    m[1::7] = np.nan
    m[2::5] = 0.5
    sm, gqm, glm, _ = ctx.log_evidence_bwd(x, dev(m), q, prior, ls, K, seed=3, voxel0=100)
    out_ = torch.isnan(dev(m)) | (dev(m) <= 0)
    assert bool((gqm[out_] == 0).all()) and bool((glm[out_] == 0).all())
    assert not bool(torch.signbit(gqm[out_]).any())
    half = dev(m) == 0.5
    assert _same_bits(gqm[half], a[1][half] * 0.5) and _same_bits(glm[half], a[2][half] * 0.5)
    one = dev(m) == 1.0
    assert _same_bits(gqm[one], a[1][one]) and _same_bits(glm[one], a[2][one])
    inm = ~out_
    mm = dev(m)[inm].double()
    lp = a[3][inm, 0].double()
    assert float(sm[2]) == float(mm.sum())
    assert abs(float(sm[0]) + float((mm * lp).sum())) < 1e-9 * abs(float(sm[0]))


def test_unbiased_and_lower_variance_than_the_plain_iw_gradient(ctx, data11):
    """One voxel replicated 65,536 times at K = 16 (independent draws: keys use the global index).  Common random
    numbers: the per-replicate central differences of log_evidence in q and in log sigma are the plain IW (IWAE)
    gradient of -log p^_16 on the same draws.  Both estimators have the same mean (within 5 standard errors of the
    difference of the two means) and DReG's summed variance over the five heads is the smaller.  The step h keeps the float32
    rounding noise of the differences, measured from two arithmetics of log p^ on the same draws, below 1 % of their
    standard deviation."""
    R, K, h = 65536, 16, 5e-2
    x, q, prior, ls = (a[7:8] for a in data11)
    ls = torch.full_like(ls, math.log(0.02))   # a likelihood sharper than the prior: the weights matter
    # q near the posterior, as an encoder being fine-tuned is: the voxel's heads refined (refine_posterior); at the
    # raw noisy heads DReG's summed variance is the larger (printed, MEASUREMENTS.md section 14)
    q_raw = q.expand(R, -1).contiguous()
    q = ctx.refine_posterior(x, None, q, prior, torch.exp(ls), steps=400, S=4, lr=0.05)
    x, q, prior, ls = (a.expand(R, -1).contiguous() for a in (x, q, prior, ls))
    seed = 21
    _, gq, gls, out = ctx.log_evidence_bwd(x, None, q, prior, ls, K, seed=seed, want_out=True)
    sigma = torch.exp(ls)

    def lp(qq, ss):
        return ctx.log_evidence(x, None, qq, prior, ss, K, seed=seed)[1][:, 0].double()
    base = lp(q, sigma)
    noise = float((base - out[:, 0].double()).std())          # one evaluation's rounding noise
    fd_noise = math.sqrt(2.0) * noise / (2 * h)
    # sigma is the same in every replicate, so the float32 rounding of its terms in log p^ is common to all of them
    # and does not average out: a floor of a few ulps of log p^ over 2 h on the sigma components
    floor = 8.0 * float(np.spacing(np.float32(base.abs().max().item()))) / (2 * h)
    rows = []
    var_dreg = var_fd = 0.0
    for k in range(5):
        d = torch.zeros_like(q)
        d[:, k] = h
        fd = -(lp(q + d, sigma) - lp(q - d, sigma)) / (2 * h)
        g = gq[:, k].double()
        se = math.sqrt((float(g.var()) + float(fd.var())) / R)   # standard error of the difference of the means
        rows.append(("q", k, float(g.mean()), float(fd.mean()), se, float(g.var()), float(fd.var())))
        assert abs(float(g.mean() - fd.mean())) < 5 * se, rows[-1]
        assert fd_noise < 0.01 * float(fd.std()), (k, fd_noise, float(fd.std()))
        var_dreg += float(g.var())
        var_fd += float(fd.var())
    for t in range(ls.shape[1]):
        d = torch.zeros_like(ls)
        d[:, t] = h
        fd = -(lp(q, torch.exp(ls + d)) - lp(q, torch.exp(ls - d))) / (2 * h)
        g = gls[:, t].double()
        se = math.sqrt((float(g.var()) + float(fd.var())) / R)
        rows.append(("log_sigma", t, float(g.mean()), float(fd.mean()), se, floor))
        assert abs(float(g.mean() - fd.mean())) < 5 * se + floor, rows[-1]
    print(f"rounding noise of one log p^ {noise:.3e}; of a difference {fd_noise:.3e}")
    for r in rows:
        print(r)
    print(f"summed variance over the five heads: DReG {var_dreg:.4e}, plain IW (differences) {var_fd:.4e}")
    _, gq_raw, _, _ = ctx.log_evidence_bwd(x, None, q_raw, prior, ls, K, seed=seed)
    v_raw = sum(float(gq_raw[:, k].double().var()) for k in range(5))
    v_raw_fd = 0.0
    for k in range(5):
        d = torch.zeros_like(q_raw)
        d[:, k] = h
        v_raw_fd += float((-(lp(q_raw + d, sigma) - lp(q_raw - d, sigma)) / (2 * h)).var())
    print(f"at the unrefined heads: DReG {v_raw:.4e}, plain IW (differences) {v_raw_fd:.4e}")
    assert var_dreg < var_fd


def test_sgd_on_the_gradient_raises_the_bound(ctx, params):
    """4,096 synthetic voxels from noisy heads: 100 plain SGD steps on g_q with fresh seeds raise the mean log p^_16
    on a seed no step used."""
    from oracle.oracle import Oracle
    x, q, prior, ls = (dev(a) for a in _case(Oracle("f32", params), params, 4096, 1, spread=0.5))
    sigma = torch.exp(ls)

    def mean_lp(qq):
        s, _, _ = ctx.log_evidence(x, None, qq, prior, sigma, 16, seed=999)
        return float(-s[0] / s[2])
    before = mean_lp(q)
    qq = q.clone()
    for j in range(100):
        _, gq, _, _ = ctx.log_evidence_bwd(x, None, qq, prior, ls, 16, seed=1 + j)
        qq = qq - 2e-4 * gq
    after = mean_lp(qq)
    print(f"mean log p^_16: {before:.4f} -> {after:.4f}")
    assert bool(torch.isfinite(qq).all()) and after > before


def test_bad_arguments_and_unsupported(ctx, data11, params):
    from qbold_vi_amd import _lib
    from qbold_vi_amd.ops import Context
    x, q, prior, ls = (a[:64] for a in data11)
    gq = torch.empty((64, 5), device="cuda")
    gls = torch.empty((64, 11), device="cuda")
    sums = torch.empty(3, dtype=torch.float64, device="cuda")
    ws = ctx._workspace()
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731

    def call(c, K, g=gq, gl=gls, s=sums, xx=x, lsx=ls):
        return c.lib.qbold_log_evidence_bwd(c.handle, P(xx), None, P(q), P(prior), P(lsx), None, int(K), 1, 0, P(g),
                                            P(gl), None, P(s), P(c._workspace()), 64, None)
    assert call(ctx, 0) == -1 and call(ctx, -3) == -1 and call(ctx, (1 << 30) + 1) == -1
    assert call(ctx, 8, g=None) == -1 and call(ctx, 8, gl=None) == -1 and call(ctx, 8, s=None) == -1
    assert call(ctx, 8, xx=None) == -1
    assert call(ctx, 8) == _lib.QBOLD_OK
    torch.cuda.synchronize()
    with pytest.raises(_lib.QboldError):
        ctx.log_evidence_bwd(x, None, q, prior, ls, 0)
    c64 = Context(_p64(params), True, True)
    x64 = torch.ones((64, 64), device="cuda")
    assert c64.lib.qbold_log_evidence_bwd(c64.handle, P(x64), None, P(q), P(prior), P(x64), None, 4, 1, 0, P(gq),
                                          P(x64), None, P(sums), P(c64._workspace()), 64, None) == \
        ERR_UNSUPPORTED
    lit = Context(params, True, True)
    lit.set_tissue_mode("literal")
    assert call(lit, 4) == ERR_UNSUPPORTED
    del ws


# ---- training -----------------------------------------------------------------------------------------------------
def small_config(tmp, **over):
    from qbold_vi_amd.utils import load_arguments
    args = load_arguments(["train.py", os.path.join(ROOT, "configurations", "optimal.yaml")], entry="train")
    args.update(no_units=24, no_intermediate_layers=1, no_pt_epochs=10, no_ft_epochs=3,
                save_directory=str(tmp), synthetic_voxels=4096, mc_samples=1)
    args.update(over)
    return args


def test_voxel_fine_tuning_on_the_bound(tmp_path, monkeypatch):
    from qbold_vi_amd import training
    monkeypatch.chdir(ROOT)
    _, _, hist = training.train_model(small_config(tmp_path, iw_samples=8), pt_sample_size=200)
    ft = [h for h in hist if "val_elbo" in h]
    assert len(ft) == 3
    for h in ft:
        assert all(np.isfinite(v) for v in h.values() if isinstance(v, float))
        assert "val_log_evidence" in h and "iw_elbo_same" in h
    assert ft[-1]["loss"] < ft[0]["loss"]
    assert ft[-1]["iw_elbo_same"] >= ft[-1]["loss"] - 1e-6   # -ELBO_same >= -log p^ draw by draw (Jensen)


def test_iw_samples_zero_is_the_elbo_run_bit_for_bit(tmp_path, monkeypatch):
    from qbold_vi_amd import training
    monkeypatch.chdir(ROOT)
    cfg = small_config(tmp_path / "a", no_pt_epochs=2, no_ft_epochs=1)
    m1, _, h1 = training.train_model(cfg, pt_sample_size=100, max_ft_steps=20)
    m2, _, h2 = training.train_model(dict(small_config(tmp_path / "b", no_pt_epochs=2, no_ft_epochs=1), iw_samples=0),
                                     pt_sample_size=100, max_ft_steps=20)
    for k, v in m1.get_weights().items():
        np.testing.assert_array_equal(v, m2.get_weights()[k])
    assert [sorted(h) for h in h1] == [sorted(h) for h in h2]


def test_refused_configurations(tmp_path, monkeypatch):
    from qbold_vi_amd import training
    monkeypatch.chdir(ROOT)
    with pytest.raises(NotImplementedError, match="diagonal family"):
        training.train_model(small_config(tmp_path / "d", use_mvg=False, iw_samples=4, no_pt_epochs=1),
                             pt_sample_size=100)
    with pytest.raises(NotImplementedError):
        training.train_model(small_config(tmp_path / "p", use_population_prior=True, iw_samples=4, no_pt_epochs=1),
                             pt_sample_size=100)
    with pytest.raises(ValueError, match="mc_samples"):
        training.train_model(small_config(tmp_path / "m", mc_samples=2, iw_samples=4, no_pt_epochs=1),
                             pt_sample_size=100)


def test_crop_fine_tuning_on_the_bound(tmp_path, monkeypatch):
    from qbold_vi_amd import training
    from qbold_vi_amd.signals import SignalGenerationLayer
    monkeypatch.chdir(ROOT)
    params = training.get_params("config")
    layer = SignalGenerationLayer(dict(params, simulate_noise='True'), True, True)
    d = tmp_path / "data"
    os.makedirs(d)
    nx = ny = 12
    gx, gy = np.meshgrid(np.linspace(0, 1, nx), np.linspace(0, 1, ny), indexing="ij")
    for name in ("ASE_scan", "ASE_INF", "ASE_SUP", "hyperv_ase", "baseline_ase"):
        y = np.stack([np.broadcast_to(0.3 + 0.2 * gx[None, :, :, None], (2, nx, ny, 8)),
                      np.broadcast_to(0.02 + 0.03 * gy[None, :, :, None], (2, nx, ny, 8))], -1)
        sig = layer(torch.as_tensor(y.reshape(-1, 2), dtype=torch.float32, device="cuda")).cpu().numpy()
        vol = np.concatenate([sig * 100.0, np.ones((sig.shape[0], 2), np.float32)], -1).reshape(2, nx, ny, 8, 13)
        vol[:, 0, :, :, -2:] = 0.0
        np.save(d / f"{name}.npy", vol)
    cfg = small_config(tmp_path / "run", synthetic_voxels=0, d=str(d), no_ft_epochs=2, crop_size=8, iw_samples=8,
                       smoothness_weight=5.0)
    _, _, hist = training.train_model(cfg, pt_sample_size=200, max_ft_steps=30)
    ft = [h for h in hist if "val_elbo" in h]
    assert ft and all(np.isfinite(h["loss"]) and np.isfinite(h["val_log_evidence"]) for h in ft)
    assert "predictions_smoothness_metric" in ft[-1] and ft[-1]["val_smoothness"] > 0.0
    assert abs(ft[-1]["val_elbo_smooth"] - (ft[-1]["val_elbo"] + 5.0 * ft[-1]["val_smoothness"])) < 1e-9


def test_train_py_cli_iw_samples(tmp_path):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configurations", "optimal.yaml")))
    cfg.update(save_directory=str(tmp_path / "run"), no_pt_epochs=1, no_ft_epochs=1, no_units=16,
               no_intermediate_layers=1)
    ypath = tmp_path / "small.yaml"
    yaml.safe_dump(cfg, open(ypath, "w"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), str(ypath), "--synthetic_voxels", "4096",
                        "--iw_samples", "8"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    last = json.loads(r.stdout.strip().splitlines()[-1])
    assert np.isfinite(last["val_log_evidence"])
