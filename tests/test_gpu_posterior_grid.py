"""Exact posteriors by quadrature (qbold_posterior_grid, Context.posterior_grid, FineTuner.posterior_grid): against the
float64 restatement on the kernel's own box (tests/_grid_reference.py) in the seven IW configurations, a known answer
by dense quadrature, the truncation / resolution diagnostics, agreement with the IW evidence, the ELBO kernels and the
refinement, determinism and masks, and the Python surface."""
import numpy as np
import pytest

import _grid_reference as gr
from _iw_reference import dw_coef, rel, rel1

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PRIOR = np.array([-0.2, 0.3, -2.0, 0.3, 0.0], np.float32)


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


def _p24(params):
    return dict(params, tau_start="-0.028", tau_end="0.065", tau_step="0.004")


def _p64(params):
    return dict(params, tau_start="-0.015", tau_end="0.065", tau_step="0.00125")


CASES = {
    "table_T11": (None, {}, "table"),
    "protocol_T24": (_p24, {}, "table"),
    "protocol_T64": (_p64, {}, "table"),
    "literal": (None, {}, "literal"),
    "student_t": (None, dict(student_t_df=5.0), "table"),
    "log_data": (None, dict(predict_log_data=True), "table"),
    "three_image_norm": (None, dict(multi_image_normalisation=True), "table"),
}


def _node_step(box, n):
    return (box[1] - box[0]) / (n - 1), (box[3] - box[2]) / (n - 1)


@pytest.mark.parametrize("case", list(CASES))
def test_matches_float64_reference_on_the_kernels_box(params, case):
    from oracle.oracle import Oracle
    from qbold_vi_amd.ops import Context
    proto, sw, mode = CASES[case]
    p = proto(params) if proto else params
    o32 = Oracle("f32", p, **sw)
    n = 24
    x, q, prior, sigma = heads(o32, p, o32.T, n, 11)
    c = Context(p, True, True, **sw)
    c.set_tissue_mode(mode)
    sums, out, box = c.posterior_grid(dev(x), None, dev(prior), dev(sigma), q=dev(q), want_box=True)
    out, box = out.cpu().numpy().astype(np.float64), box.cpu().numpy().astype(np.float64)
    o64 = Oracle("f64", p, node0_zero=True, **sw)
    try:
        ref, own = [], []
        for i in range(n):
            r, _ = gr.voxel_reference(o64, x[i], sigma[i], prior[i], q=q[i], gh=16, fine_box=box[i],
                                      dw=dw_coef(p))
            ref.append(r)
            _, b = gr.voxel_reference(o64, x[i], sigma[i], prior[i], q=q[i], gh=0, dw=dw_coef(p))
            own.append(b)
    finally:
        o64.lib.qbo_set_node0_zero(0)
    ref, own = np.array(ref), np.array(own)
    errs = dict(log_p=rel1(out[:, 0], ref[:, 0]), elbo=rel1(out[:, 1], ref[:, 1]), means=rel(out[:, 2:5], ref[:, 2:5]),
                sds=rel(out[:, 5:8], ref[:, 5:8]), corr=float(np.max(np.abs(out[:, 8] - ref[:, 8]))),
                quant=float(np.max(np.abs(out[:, 9:13] - ref[:, 9:13]))))
    print(case, errs)
    assert errs["log_p"] < 2e-4 and errs["elbo"] < 2e-4, (case, errs)
    assert errs["means"] < 1e-4 and errs["sds"] < 1e-4, (case, errs)
    assert errs["corr"] < 1e-3 and errs["quant"] < 1e-4, (case, errs)
    for i in range(n):
        ha, hb = _node_step(box[i], 64)
        # one node in OEF / DBV units: the transforms' slopes are at most 0.8 / 4 and 0.2 / 4 per logit
        assert abs(out[i, 13] - ref[i, 13]) <= 0.2 * ha + 1e-6 and abs(out[i, 14] - ref[i, 14]) <= 0.05 * hb + 1e-6
        b0 = gr.start_box(prior[i], q[i])
        ca, cb = _node_step(b0, 32)
        assert np.all(np.abs(box[i, :2] - own[i, :2]) <= ca) and np.all(np.abs(box[i, 2:] - own[i, 2:]) <= cb), i
    assert sums.cpu().numpy()[2] == n


def _known_answer_data(params, sigmas, per=3):
    from oracle.oracle import Oracle, synth_inputs
    o32 = Oracle("f32", params)
    n = per * len(sigmas)
    x, _ = synth_inputs(n, params, seed=21, oracle=o32)
    sigma = np.repeat(np.asarray(sigmas, np.float32), per)[:, None] * np.ones((1, o32.T), np.float32)
    prior = np.tile(PRIOR, (n, 1))
    return x, sigma, prior


def test_known_answer_by_dense_quadrature(ctx, params, oracle64):
    """Defaults against the 481^2 two-stage float64 reference at sigma = 0.2, 0.05, 0.01, 0.003.  At sigma <= 0.01
    the posterior is a thin OEF-DBV ridge that 64 nodes a side can under-resolve: such voxels must say so (quad_err
    > 1e-4), and every voxel that does not must match.  At sigma >= 0.05 none may be flagged."""
    x, sigma, prior = _known_answer_data(params, (0.2, 0.05, 0.01, 0.003))
    _, out, _ = ctx.posterior_grid(dev(x), None, dev(prior), dev(sigma))
    out = out.cpu().numpy().astype(np.float64)
    dw = dw_coef(params)
    matched = 0
    try:
        oracle64.lib.qbo_set_node0_zero(1)
        for i in range(x.shape[0]):
            J = gr.VoxelJoint(oracle64, x[i], sigma[i], prior[i].astype(np.float64))
            ref, _ = gr.dense(J, gr.start_box(prior[i]), dw=dw)
            sd = ref[5:8]
            flagged = out[i, 16] > 1e-4 or out[i, 15] > 1e-4
            print(i, sigma[i, 0], "log_p", out[i, 0], ref[0], "means", out[i, 2:5], ref[2:5], "diag", out[i, 15:])
            if sigma[i, 0] >= 0.05:
                assert not flagged and out[i, 15] < 1e-6, i
            if flagged:
                continue
            matched += 1
            assert abs(out[i, 0] - ref[0]) < 1e-3, (i, out[i, 0], ref[0])
            assert np.all(np.abs(out[i, 2:5] / ref[2:5] - 1) < 1e-3), (i, out[i, 2:5], ref[2:5])
            assert np.all(np.abs(out[i, 5:8] / sd - 1) < 1e-2), (i, out[i, 5:8], sd)
            assert np.all(np.abs(out[i, 9:11] - ref[9:11]) < 0.02 * sd[0]), (i, out[i, 9:11], ref[9:11])
            assert np.all(np.abs(out[i, 11:13] - ref[11:13]) < 0.02 * sd[1]), (i, out[i, 11:13], ref[11:13])
    finally:
        oracle64.lib.qbo_set_node0_zero(0)
    assert matched >= 6


def test_diagnostics_flag_every_miss(ctx, params, oracle64):
    """Under-resolved (fine = 16, one locate pass, sigma = 0.003) and truncated (span = 0.5, a narrow prior far from
    the likelihood) runs: every voxel whose log_p misses the dense reference by more than 1e-3 nats is flagged."""
    x, sigma, prior = _known_answer_data(params, (0.003,), per=8)
    far = np.tile(np.array([2.5, -1.0, 1.0, -1.0, 0.0], np.float32), (x.shape[0], 1))
    runs = [(prior, dict(fine=16, locate=1)), (far, dict(span=0.5))]
    try:
        oracle64.lib.qbo_set_node0_zero(1)
        for pr, kw in runs:
            _, out, _ = ctx.posterior_grid(dev(x), None, dev(pr), dev(sigma), **kw)
            out = out.cpu().numpy().astype(np.float64)
            missed = 0
            for i in range(x.shape[0]):
                J = gr.VoxelJoint(oracle64, x[i], sigma[i], pr[i].astype(np.float64))
                ref, _ = gr.dense(J, gr.start_box(pr[i]))
                if abs(out[i, 0] - ref[0]) > 1e-3:
                    missed += 1
                    assert out[i, 16] > 1e-4 or out[i, 15] > 1e-4, (kw, i, out[i, 0], ref[0], out[i, 15:])
            print(kw, "missed", missed, "of", x.shape[0])
            assert missed > 0, kw   # the runs are meant to miss
    finally:
        oracle64.lib.qbo_set_node0_zero(0)


def test_agrees_with_the_iw_evidence_and_bounds_the_elbo(ctx, params):
    from oracle.oracle import Oracle
    _, sigma, prior = _known_answer_data(params, (0.2, 0.05), per=4)
    xs, q, _, _ = heads(Oracle("f32", params), params, 11, 8, 21)   # encoder heads
    x, q, sigma, prior = dev(xs), dev(q), dev(sigma), dev(prior)
    _, out, _ = ctx.posterior_grid(x, None, prior, sigma, q=q)
    # the IW estimate is held to its band with a proposal near the posterior (the encoder's untrained heads give an
    # ESS too small for 5 / sqrt(ESS) to bound the lower bound's bias)
    q_near = ctx.refine_posterior(x, None, q, prior, sigma, steps=2000, S=4, lr=0.1, lr_final=0.0)
    _, iw, means = ctx.log_evidence(x, None, q_near, prior, sigma, 16384, seed=5, want_means=True)
    out, iw, means = (t.cpu().numpy().astype(np.float64) for t in (out, iw, means))
    band = 5.0 / np.sqrt(iw[:, 2]) + 1e-3
    print("grid", out[:, 0], "iw", iw[:, 0], "ess", iw[:, 2])
    assert np.all(np.abs(iw[:, 0] - out[:, 0]) < band)
    assert np.all(np.abs(means - out[:, 2:5]) < band[:, None] * np.abs(out[:, 2:5]))
    assert np.all(out[:, 1] <= out[:, 0] + 1e-4)
    q_ref = ctx.refine_posterior(x, None, q, prior, sigma, steps=300)
    _, out_r, _ = ctx.posterior_grid(x, None, prior, sigma, q=q_ref)
    out_r = out_r.cpu().numpy().astype(np.float64)
    assert np.all(out_r[:, 1] <= out_r[:, 0] + 1e-4)
    assert np.all(out_r[:, 1] >= out[:, 1] - 1e-3)   # refinement raised the exact ELBO


def _mc_agrees(mc, exact):
    d = np.asarray(mc, np.float64) - np.asarray(exact, np.float64)
    se = d.std(ddof=1) / np.sqrt(d.size)
    print("mean diff", d.mean(), "se", se)
    assert abs(d.mean()) < 5.0 * se + 1e-4, (d.mean(), se)


def test_elbo_agrees_with_the_elbo_kernel_and_the_refinement(ctx, params):
    from oracle.oracle import Oracle
    o32 = Oracle("f32", params)
    n = 512
    x, q, prior, sigma = (dev(a) for a in heads(o32, params, 11, n, 4))
    _, out, _ = ctx.posterior_grid(x, None, prior, sigma, q=q)
    exact = out[:, 1].cpu().numpy()
    _, nll_kl = ctx.elbo_fwd(x, None, q, prior, sigma, 4096, 4096, seed=3)
    nk = nll_kl.cpu().numpy().astype(np.float64)
    _mc_agrees(-(nk[:, 0] + nk[:, 1]), exact)
    q_ref, loss = ctx.refine_posterior(x, None, q, prior, sigma, steps=200, want_loss=True)
    _, out_r, _ = ctx.posterior_grid(x, None, prior, sigma, q=q_ref)
    _mc_agrees(loss[:, 1].cpu().numpy(), -out_r[:, 1].cpu().numpy())


def _same_bits(a, b):
    iv = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def test_determinism_masks_and_sums(ctx, params):
    from oracle.oracle import Oracle
    o32 = Oracle("f32", params)
    n = 1001
    x, q, prior, sigma = heads(o32, params, 11, n, 9)
    mask = (np.random.default_rng(4).uniform(size=n) > 0.3).astype(np.float32)
    mask[mask > 0] = np.random.default_rng(6).uniform(0.5, 1.5, int((mask > 0).sum())).astype(np.float32)
    mask[7] = np.nan
    x = x.copy()
    x[mask == 0] = np.nan
    args = [dev(x), dev(mask), dev(prior), dev(sigma)]
    s1, o1, b1 = ctx.posterior_grid(*args, q=dev(q), want_box=True)
    s2, o2, b2 = ctx.posterior_grid(*args, q=dev(q), want_box=True)
    assert _same_bits(o1, o2) and _same_bits(s1, s2) and _same_bits(b1, b2)
    perm = np.random.default_rng(2).permutation(n)
    _, op, _ = ctx.posterior_grid(*(a[perm] for a in args), q=dev(q)[perm])
    assert _same_bits(op, o1[perm])
    _, one, _ = ctx.posterior_grid(*(a[5:6] for a in args), q=dev(q)[5:6])
    assert _same_bits(one, o1[5:6])
    on = o1.cpu().numpy().astype(np.float64)
    live = mask > 0
    assert np.all(np.isfinite(on[live])) and np.all(np.isnan(on[~live]))
    want = np.array([(mask[live] * -on[live, 0]).sum(), (mask[live] * -on[live, 1]).sum(),
                     mask[live].astype(np.float64).sum()])
    got = s1.cpu().numpy()
    assert np.all(np.abs(got - want) <= 1e-8 * np.abs(want)), (got, want)
    # without q: no ELBO column, second sum 0
    s0, o0, _ = ctx.posterior_grid(*args)
    assert np.all(np.isnan(o0.cpu().numpy()[:, 1])) and s0.cpu().numpy()[1] == 0.0


def test_bad_arguments_return_invalid(ctx, params):
    import ctypes as C
    from qbold_vi_amd import _lib
    n = 8
    x, p, s = (torch.ones((n, 11), device="cuda"), torch.zeros((n, 5), device="cuda"),
               torch.full((n, 11), 0.05, device="cuda"))
    out = torch.empty((n, 17), device="cuda")
    sums = torch.empty(3, dtype=torch.float64, device="cuda")
    ws = ctx._workspace()
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731

    def call(o=out, **kw):
        cfg = dict(coarse=32, fine=64, locate=2, gh=16, span=6.0, cut=40.0, level_lo=0.025, level_hi=0.975)
        cfg.update(kw)
        g = _lib.GridCfg(**cfg)
        return ctx.lib.qbold_posterior_grid(ctx.handle, P(x), None, P(p), P(s), None, C.byref(g), P(o), None,
                                            P(sums), P(ws), n, None)
    for kw in (dict(coarse=20), dict(coarse=136), dict(fine=8), dict(fine=264), dict(locate=0), dict(locate=5),
               dict(gh=1), dict(gh=33), dict(span=0.0), dict(cut=5.0), dict(cut=90.0), dict(level_lo=0.0),
               dict(level_lo=0.6, level_hi=0.4), dict(level_hi=1.0)):
        assert call(**kw) == -1, kw
    assert call(o=None) == -1
    assert call() == _lib.QBOLD_OK
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def trainer(params):
    from qbold_vi_amd import EncoderTrainer
    return EncoderTrainer(system_params=params, no_units=60, use_layer_norm=False, dropout_rate=0.0,
                          no_intermediate_layers=2, initial_im_sigma=0.05, activation_type='relu',
                          multi_image_normalisation=False, channelwise_gating=True, infer_inv_gamma=False,
                          use_population_prior=False, use_mvg=True, predict_log_data=False)


def _fine_tuner(tr, params):
    from qbold_vi_amd import SignalGenerationLayer
    model, _ = tr.create_encoder(gate_offset=-3.0, resid_init_std=0.05, no_ip_images=11)
    return model, tr.build_fine_tuner(model, SignalGenerationLayer(dict(params, simulate_noise='False'), True, True))


def test_fine_tuner_voxel_batch_and_crops(trainer, params):
    from oracle.oracle import Oracle, synth_inputs
    o32 = Oracle("f32", params)
    model, ft = _fine_tuner(trainer, params)
    for shape in ((300, 1, 1, 1), (2, 9, 7, 4)):
        nv = int(np.prod(shape))
        x, _ = synth_inputs(nv, params, seed=3, oracle=o32)
        x5 = dev(x).reshape(shape + (11,))
        m5 = dev((np.random.default_rng(4).uniform(size=nv) > 0.3).astype(np.float32)).reshape(shape + (1,))
        p5 = model(x5)[0]
        got = ft.posterior_grid(x5, m5, p5, fine=48)
        _, q5, sg5 = model.predict(x5, want=("out2", "sigma"))
        sums, out, _ = trainer.context.posterior_grid(x5.reshape(-1, 11), m5.reshape(-1), p5.reshape(-1, 5),
                                                      sg5.reshape(-1, 11), q=q5.reshape(-1, 5), fine=48)
        assert got["oef"].shape == shape and got["oef_ci"].shape == shape + (2,) and got["map"].shape == shape + (2,)
        assert torch.equal(got["log_evidence"].reshape(-1).nan_to_num(), out[:, 0].nan_to_num())
        assert torch.equal(got["dbv_ci"].reshape(-1, 2).nan_to_num(), out[:, 11:13].nan_to_num())
        assert torch.equal(got["sums"], sums)
        assert float(got["mean_gap"]) >= -1e-4
        live = m5.reshape(shape) > 0
        assert torch.all(got["gap"][live] >= -1e-4)


def test_save_predictions_writes_the_exact_maps(trainer, params, tmp_path):
    import os
    from oracle.oracle import Oracle, synth_inputs
    from qbold_vi_amd import nifti
    model, ft = _fine_tuner(trainer, params)
    B, X, Y, Z = 2, 5, 4, 3
    x, _ = synth_inputs(B * X * Y * Z, params, seed=12, oracle=Oracle("f32", params))
    mask = (np.random.default_rng(1).uniform(size=(B * X * Y * Z, 1)) > 0.2).astype(np.float32)
    data = dev(np.concatenate([x, mask], -1)).reshape(B, X, Y, Z, 12)
    priors = model(data[..., :-1])[0]
    d0, d1 = tmp_path / "plain", tmp_path / "grid"
    os.makedirs(d0)
    os.makedirs(d1)
    assert trainer.save_predictions(model, data, str(d0 / "sub"), fine_tuner_model=ft, priors=priors) is None
    maps = trainer.save_predictions(model, data, str(d1 / "sub"), fine_tuner_model=ft, priors=priors,
                                    posterior_grid=True)
    names = ("oef_exact", "dbv_exact", "r2p_exact", "oef_exact_sd", "dbv_exact_sd", "oef_ci_lo", "oef_ci_hi",
             "dbv_ci_lo", "dbv_ci_hi", "logevidence_exact", "vigap_exact", "gridedge")
    extra = {f"sub_{k}.nii.gz" for k in names}
    assert set(os.listdir(d1)) == set(os.listdir(d0)) | extra
    live = mask.reshape(B, X, Y, Z) > 0
    for k in names:
        v = maps[k].cpu().numpy()
        assert v.shape == (B, X, Y, Z, 1)
        img = nifti.load(str(d1 / f"sub_{k}.nii.gz"))[0]
        np.testing.assert_array_equal(img, np.concatenate(np.split(v, B, axis=0), axis=-1)[0])
        assert np.all(v[..., 0][~live] == 0.0) and np.all(np.isfinite(v))
    lo, hi, mean = (maps[k].cpu().numpy()[..., 0][live] for k in ("oef_ci_lo", "oef_ci_hi", "oef_exact"))
    assert np.all(lo <= mean) and np.all(mean <= hi)
    assert np.all(maps["vigap_exact"].cpu().numpy() >= -1e-4)
