"""qbold_fisher_information (fisher_kernel) and qbold_design_scores (design_kernel, design_sum_kernel) against the float64
restatement of tests/_design_reference.py on the cases of tests/_design_cases.py: 11 / 24 / 12 / 22 / 33 / 64 taus with
and without three-image normalisation, one tau, 40 and 257 points, per-voxel and shared sigma, 70 designs.

Bounds.  The data-only quantities are ill-conditioned by nature (a relative error eps of the entries of I moves det I
by eps kappa), so they are measured as _design_cases.measures states and held to 4 x the case's float32 floor
(_design_cases.FLOOR; the margin of 4 is test_gpu_elbo_bwd_reference's).  The quantities with the prior are
laplace_kernel's arithmetic at a given point and are held to test_gpu_laplace's SD_ERR bounds (9e-5 on the sds, 2e-6 on
the correlation); log det A to 4 x floor x kappa_A; a design's sums to the same bounds summed over the voxels."""
import ctypes as C

import numpy as np
import pytest

import _design_cases as cases
import _design_reference as dr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAMES = list(cases.CASES)
MARGIN = 4.0
SD_BOUND, CORR_BOUND = 9e-5, 2e-6                      # test_gpu_laplace.SD_ERR
LAPLACE_SD = {"oef_sd": 9e-5, "dbv_sd": 9e-5, "r2p_sd": 7e-5, "corr": 2e-6}
FISHER_DESIGNS = (None, 0, 1, 2, 3, 4)                 # weights None, then the first five rows of the case's designs
_CTX = {}


def dev(a):
    return torch.as_tensor(np.array(a, order="C"), device="cuda")   # a copy: the shared inputs are read-only


def same_bits(a, b):
    iv = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def setup(params, name):
    """The case, its context, its device tensors and the kernels' outputs on all its designs; made once."""
    if name not in _CTX:
        from qbold_vi_amd.ops import Context
        c = cases.build(params, name)
        ctx = Context(c.p, True, True, **c.sw)
        assert ctx.T == c.T
        t = {k: dev(getattr(c, k)) for k in ("theta", "sigma", "prior", "mask", "weights")}
        scores, pv = ctx.design_scores(t["theta"], t["sigma"], t["weights"], t["prior"], t["mask"], want_per_voxel=True)
        torch.cuda.synchronize()
        _CTX[name] = (c, ctx, t, scores, pv)
    return _CTX[name]


def fisher_rows(ctx, t, designs, prior=True, mask=True):
    """out [len(designs), N, 15] (numpy): one call per design (None: weights NULL)."""
    return np.stack([ctx.fisher_information(t["theta"], t["sigma"], None if b is None else t["weights"][b],
                                            t["prior"] if prior else None, t["mask"] if mask else None)["out"]
                     .cpu().numpy() for b in designs])


def as_reference(out):
    """The reference's dict from out [B, N, 15]."""
    o = out.astype(np.float64)
    I = np.empty(o.shape[:2] + (2, 2))
    I[..., 0, 0], I[..., 0, 1], I[..., 1, 0], I[..., 1, 1] = o[..., 0], o[..., 1], o[..., 1], o[..., 2]
    return dict(I=I, kappa=o[..., 3], log_det=o[..., 4], crlb=o[..., 5:9], bound=o[..., 9:13], log_det_A=o[..., 13],
                singular=(np.nan_to_num(o[..., 14]).astype(int) & 1) != 0)


def pick(ref, ref1, designs):
    """The reference's rows of `designs` (None: the unweighted call's)."""
    keys = ("I", "kappa", "log_det", "crlb", "singular", "A", "kappa_A", "log_det_A", "bound", "var")
    return {k: np.stack([ref1[k][0] if b is None else ref[k][b] for b in designs]) for k in keys}


@pytest.mark.parametrize("name", NAMES)
def test_fisher_information_matches_float64(params, name):
    c, ctx, t, _, _ = setup(params, name)
    out = fisher_rows(ctx, t, FISHER_DESIGNS)
    got, ref = as_reference(out), pick(c.ref, c.ref1, FISHER_DESIGNS)
    live = c.live
    assert np.all(np.isnan(out[:, ~live])), "masked-out voxels carry a NaN row"
    assert np.all(np.isfinite(out[:, live, 0:3])) and np.all(np.isfinite(out[:, live, 9:14]))
    assert np.array_equal(got["singular"][:, live], ref["singular"][:, live])
    assert np.array_equal(out[:, live, 14], ref["singular"][:, live].astype(np.float32))
    s = ref["singular"][:, live]
    o = out[:, live]
    assert np.all(np.isposinf(o[s][:, 3])) and np.all(np.isneginf(o[s][:, 4])) and np.all(np.isposinf(o[s][:, 5:8])) \
        and np.all(np.isnan(o[s][:, 8])) and np.all(np.isfinite(o[~s][:, 3:9]))
    m = cases.groups(cases.measures(got, ref, live))
    ratio = [g / f if f > 0 else (0.0 if g == 0 else np.inf) for g, f in zip(m, cases.FLOOR[name])]
    sd = float(np.max(np.abs(got["bound"][:, live, :3] / ref["bound"][:, live, :3] - 1.0)))
    corr = float(np.max(np.abs(got["bound"][:, live, 3] - ref["bound"][:, live, 3])))
    print(f"[design] {name}: I {m[0]:.3e} ({ratio[0]:.2f} floors)  det {m[1]:.3e} ({ratio[1]:.2f})  log det A "
          f"{m[2]:.3e} ({ratio[2]:.2f})  sds with prior {sd:.3e}  corr {corr:.3e}")
    assert max(ratio) <= MARGIN, (m, cases.FLOOR[name])
    assert sd <= SD_BOUND and corr <= CORR_BOUND


@pytest.mark.parametrize("name", NAMES)
def test_design_scores_match_float64(params, name):
    c, ctx, t, scores, pv = setup(params, name)
    live, m64 = c.live, c.mask.astype(np.float64)
    pvn, sc = pv.cpu().numpy().astype(np.float64), scores.cpu().numpy()
    assert pvn.shape == (cases.B_ALL, c.N, 4) and sc.shape == (cases.B_ALL, 5)
    assert np.all(np.isnan(pvn[:, ~live])) and np.all(np.isfinite(pvn[:, live])) and np.all(np.isfinite(sc))
    ref = c.ref
    b_ld = MARGIN * cases.FLOOR[name][2] * ref["kappa_A"]                  # [B, N]
    e_ld = np.abs(pvn[..., 0] - ref["log_det_A"])
    e_sd = np.abs(np.sqrt(pvn[..., 1:4]) / ref["bound"][..., :3] - 1.0)
    print(f"[design] {name} per voxel: log det A {np.max((e_ld / b_ld)[:, live]):.2f} bounds, sds "
          f"{np.max(e_sd[:, live]):.3e}")
    assert np.all(e_ld[:, live] <= b_ld[:, live]) and np.all(e_sd[:, live] <= SD_BOUND)
    # the sums per design: the per-voxel bounds, weighted and summed (a variance carries twice its sd's relative bound)
    want = dr.scores(ref, c.mask)
    bound = np.concatenate([(b_ld * m64)[:, live].sum(1, keepdims=True),
                            (2 * SD_BOUND * ref["var"] * m64[None, :, None])[:, live].sum(1)], -1)
    err = np.abs(sc[:, :4] - want[:, :4])
    print(f"[design] {name} sums: worst {np.max(err / bound):.3f} of the bound")
    assert np.all(err <= bound) and np.array_equal(sc[:, 4], want[:, 4])
    # the sums are the double sums of the per-voxel rows in tile order
    mine = np.zeros((cases.B_ALL, 4))
    for lo in range(0, c.N, 64):
        rows = np.arange(lo, min(lo + 64, c.N))
        rows = rows[live[rows]]
        mine += (pvn[:, rows] * m64[None, rows, None]).sum(1)
    assert np.max(np.abs(sc[:, :4] - mine) / np.abs(mine)) <= 1e-12


@pytest.mark.parametrize("name", ("t11_N257", "t33_multi_N40", "t64_multi_N257", "t12_N257"))
def test_bits(params, name):
    c, ctx, t, scores, pv = setup(params, name)
    args = (t["theta"], t["sigma"], t["weights"], t["prior"], t["mask"])
    # run to run
    s2, p2 = ctx.design_scores(*args, want_per_voxel=True)
    assert same_bits(s2, scores) and same_bits(p2, pv)
    # B = 1 and B = 5 are the first rows of the 70; another chunking of B is the same bits
    for B in (1, 5):
        sb, pb = ctx.design_scores(args[0], args[1], t["weights"][:B], args[3], args[4], want_per_voxel=True)
        assert same_bits(sb, scores[:B]) and same_bits(pb, pv[:B]), B
    per_design = ctx.lib.qbold_design_workspace_bytes(ctx.handle, c.N, 1)
    sc, pc = ctx.design_scores(*args, want_per_voxel=True, workspace_bytes=9 * per_design)
    assert same_bits(sc, scores) and same_bits(pc, pv)
    # a design in another slot of the batch
    perm = torch.as_tensor(np.random.default_rng(3).permutation(cases.B_ALL), device="cuda")
    sp, pp = ctx.design_scores(args[0], args[1], t["weights"][perm], args[3], args[4], want_per_voxel=True)
    assert same_bits(sp, scores[perm]) and same_bits(pp, pv[perm])
    # weights None is all ones; B = 1 is the fisher kernel's arithmetic
    f_none = ctx.fisher_information(t["theta"], t["sigma"], None, t["prior"], t["mask"])
    f_ones = ctx.fisher_information(t["theta"], t["sigma"], t["weights"][0], t["prior"], t["mask"])
    assert same_bits(f_none["out"], f_ones["out"])
    assert same_bits(pv[0, :, 0].contiguous(), f_none["log_det_bayes"].contiguous())
    lv = dev(c.live)
    for k, key in ((1, "oef_bound"), (2, "dbv_bound"), (3, "r2p_bound")):
        assert torch.max(torch.abs(torch.sqrt(pv[0, lv, k]) / f_none[key][lv] - 1.0)).item() <= 3e-7, key
    m = t["mask"].double()
    for k, col in ((0, f_none["log_det_bayes"]), (1, f_none["oef_bound"] ** 2)):
        want = (col.double()[lv] * m[lv]).sum().item()
        assert abs(scores[0, k].item() - want) <= 1e-6 * abs(want)
    if c.N == 257:
        # shards: the voxels' rows are the same bits, the sums add up
        cuts = ((0, 100), (100, 101), (101, 257))
        parts = []
        for lo, hi in cuts:
            sg = t["sigma"] if c.shared else t["sigma"][lo:hi]
            parts.append(ctx.design_scores(t["theta"][lo:hi], sg, t["weights"], t["prior"][lo:hi], t["mask"][lo:hi],
                                           want_per_voxel=True))
            fs = ctx.fisher_information(t["theta"][lo:hi], sg, t["weights"][1], t["prior"][lo:hi], t["mask"][lo:hi])
            fw = ctx.fisher_information(t["theta"], t["sigma"], t["weights"][1], t["prior"], t["mask"])
            assert same_bits(fs["out"], fw["out"][lo:hi])
        assert same_bits(torch.cat([p for _, p in parts], 1), pv)
        tot = sum(s for s, _ in parts)
        assert torch.max(torch.abs(tot - scores) / torch.abs(scores)).item() <= 1e-12


@pytest.mark.parametrize("name", ("t11_N257", "t22_multi_N257"))
def test_weights_are_averages(params, name):
    """Weights w on sigma are all ones on sigma / sqrt(w): both calls sit within the bound of the weighted reference."""
    c, ctx, t, _, _ = setup(params, name)
    w = c.weights[1]
    assert w.min() >= 1
    sg = np.broadcast_to(c.sigma.reshape(-1, c.T), (c.N, c.T)) / np.sqrt(w)[None, :]
    a = ctx.fisher_information(t["theta"], t["sigma"], t["weights"][1], t["prior"], t["mask"])["out"].cpu().numpy()
    b = ctx.fisher_information(t["theta"], dev(sg.astype(np.float32)), None, t["prior"], t["mask"])["out"].cpu().numpy()
    ref = pick(c.ref, c.ref1, (1,))
    for out in (a, b):
        m = cases.groups(cases.measures(as_reference(out[None]), ref, c.live))
        assert all(g <= MARGIN * f for g, f in zip(m, cases.FLOOR[name])), m
    live = c.live
    assert np.max(np.abs(a[live, 9:12] / b[live, 9:12] - 1.0)) <= 2 * SD_BOUND


@pytest.mark.parametrize("name", ("t11_N257", "t33_N257", "t24_multi_N257"))
def test_two_kernels_one_definition(params, name):
    """Noise-free data x = model(theta*), the Laplace fit u^ of it, and the information at theta(u^): columns 9-12 are
    qbold_laplace_posterior's columns 8-10 and 7, within 2 x test_gpu_laplace's SD_ERR.  The points 1e-4 from a range
    end are left out (rows 0-3): there theta(u^), handed over in float32, no longer determines the slopes of
    forward_transform to the bound."""
    c, ctx, t, _, _ = setup(params, name)
    x = np.asarray(c.o32.signal_fwd(c.theta), np.float32)
    sg = dev(np.ascontiguousarray(np.broadcast_to(c.sigma.reshape(-1, c.T), (c.N, c.T))))
    _, out = ctx.laplace_posterior(dev(x), None, t["prior"], sg)
    f = ctx.fisher_information(out[:, 2:4].contiguous(), sg, None, t["prior"], None)
    lo, fo = out.cpu().numpy().astype(np.float64), f["out"].cpu().numpy().astype(np.float64)
    ok = (lo[:, 14].astype(int) & 3) == 0   # converged and off the clip (bit 2, clamped heads, does not touch Sigma)
    ok[:4] = False
    assert ok.sum() >= 200
    errs = dict(oef_sd=np.max(np.abs(fo[ok, 9] / lo[ok, 8] - 1)), dbv_sd=np.max(np.abs(fo[ok, 10] / lo[ok, 9] - 1)),
                r2p_sd=np.max(np.abs(fo[ok, 11] / lo[ok, 10] - 1)), corr=np.max(np.abs(fo[ok, 12] - lo[ok, 7])))
    print(f"[design] {name} against laplace:", " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    assert all(v <= 2 * LAPLACE_SD[k] for k, v in errs.items()), errs


def test_out_of_range_points_and_no_prior(params):
    c, ctx, t, _, _ = setup(params, cases.DEFAULT_CASE)
    th = c.theta[:64].copy()
    th[5], th[6], th[7], th[9] = (0.04, 0.05), (0.9, 0.05), (0.3, 0.0005), (np.nan, 0.05)
    bad = [5, 6, 7, 9]
    f = ctx.fisher_information(dev(th), t["sigma"][:64], None, None, None)
    out = f["out"].cpu().numpy()
    assert np.all(np.isnan(out[bad, :14])) and np.all(out[bad, 14] == 2.0) and f["out_of_range"][bad].all()
    good = np.setdiff1d(np.arange(64), bad)
    assert np.all(np.isfinite(out[good, :9])) and np.all(np.isnan(out[good, 9:14])) and np.all(out[good, 14] == 0.0)
    # the other voxels' rows do not depend on them, nor on the prior
    whole = ctx.fisher_information(t["theta"][:64], t["sigma"][:64], None, t["prior"][:64], None)["out"]
    assert same_bits(f["out"][dev(good)][:, :9], whole[dev(good)][:, :9])


def test_errors_and_empty_calls(params):
    from qbold_vi_amd import _lib
    from qbold_vi_amd.ops import Context
    c, ctx, t, _, _ = setup(params, cases.DEFAULT_CASE)
    n, B, T = 64, 5, c.T
    th, sg, pr = t["theta"][:n].contiguous(), t["sigma"][:n].contiguous(), t["prior"][:n].contiguous()
    w = t["weights"][:B].contiguous()
    out = torch.empty((n, 15), device="cuda")
    sc = torch.empty((B, 5), dtype=torch.float64, device="cuda")
    ws = torch.empty(ctx.lib.qbold_design_workspace_bytes(ctx.handle, n, B) // 8, dtype=torch.float64, device="cuda")
    P = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None   # noqa: E731

    def fis(cx=ctx, th_=th, sg_=sg, rows=n, w_=None, out_=out, N=n):
        return cx.lib.qbold_fisher_information(cx.handle, P(th_), P(sg_), rows, P(w_), P(pr), None, P(out_), N, None)

    def des(cx=ctx, th_=th, sg_=sg, rows=n, w_=w, pr_=pr, sc_=sc, ws_=ws, N=n, B_=B):
        return cx.lib.qbold_design_scores(cx.handle, P(th_), P(sg_), rows, P(w_), P(pr_), None, P(sc_), None, P(ws_),
                                          N, B_, None)
    assert fis() == _lib.QBOLD_OK and des() == _lib.QBOLD_OK and fis(w_=w[1]) == _lib.QBOLD_OK
    torch.cuda.synchronize()
    assert fis(th_=None) == -1 and fis(sg_=None) == -1 and fis(out_=None) == -1 and fis(N=-1) == -1
    assert fis(rows=2) == -1 and fis(rows=0) == -1 and fis(rows=1) == _lib.QBOLD_OK
    for bad in (-1.0, float("nan"), float("inf")):
        wb = w[1].clone()
        wb[3] = bad
        assert fis(w_=wb) == -1, bad
    assert des(th_=None) == -1 and des(sg_=None) == -1 and des(w_=None) == -1 and des(pr_=None) == -1
    assert des(sc_=None) == -1 and des(ws_=None) == -1 and des(N=-1) == -1 and des(B_=-1) == -1 and des(rows=3) == -1
    with pytest.raises(ValueError):
        ctx.design_scores(th, sg, -w, pr)
    # configurations without a kernel: checked after the arguments
    lit = Context(c.p, True, True)
    lit.set_tissue_mode("literal")
    for cx in (lit, Context(c.p, True, True, student_t_df=4.0), Context(c.p, True, True, predict_log_data=True),
               Context(c.p, False, True)):
        assert fis(cx) == -3 and des(cx) == -3 and fis(cx, th_=None) == -1 and des(cx, w_=None) == -1
    # N = 0 and B = 0
    assert fis(N=0, rows=0) == _lib.QBOLD_OK and des(B_=0) == _lib.QBOLD_OK
    sc.fill_(7.0)
    assert des(N=0, rows=0) == _lib.QBOLD_OK
    torch.cuda.synchronize()
    assert torch.equal(sc, torch.zeros_like(sc))
    e = torch.empty((0, 2), device="cuda")
    f0 = ctx.fisher_information(e, t["sigma"][:0] if not c.shared else t["sigma"], None, None, None)
    assert f0["out"].shape == (0, 15)
    s0 = ctx.design_scores(e, t["sigma"][:0], w, t["prior"][:0])
    assert s0.shape == (B, 5) and torch.equal(s0, torch.zeros_like(s0))
    assert ctx.design_scores(th, sg, w[:0], pr).shape == (0, 5)


def test_fine_tuner_identifiability_voxel_batch_and_crops(params):
    """FineTuner.identifiability is Context.fisher_information at the heads' posterior means with the encoder's sigma,
    and the ratios are calculate_means' sds over the Bayesian bounds; voxel batches and crops."""
    from oracle.oracle import Oracle, synth_inputs
    from qbold_vi_amd import EncoderTrainer, SignalGenerationLayer
    tr = EncoderTrainer(system_params=params, no_units=60, use_layer_norm=False, dropout_rate=0.0,
                        no_intermediate_layers=2, initial_im_sigma=0.05, activation_type='relu',
                        multi_image_normalisation=False, channelwise_gating=True, infer_inv_gamma=False,
                        use_population_prior=False, use_mvg=True, predict_log_data=False)
    model, _ = tr.create_encoder(gate_offset=-3.0, resid_init_std=0.05, no_ip_images=11)
    ft = tr.build_fine_tuner(model, SignalGenerationLayer(dict(params, simulate_noise='False'), True, True))
    o32 = Oracle("f32", params)
    for lead, seed in (((300, 1, 1, 1), 3), ((2, 9, 7, 4), 8)):
        nv = int(np.prod(lead))
        x, _ = synth_inputs(nv, params, seed=seed, oracle=o32)
        x5 = dev(x).reshape(lead + (11,))
        m5 = dev((np.random.default_rng(seed).uniform(size=nv) > 0.3).astype(np.float32)).reshape(lead + (1,))
        p5 = model(x5)[0]
        _, q5, sg5 = model.predict(x5, want=("out2", "sigma"))
        got = ft.identifiability(x5, m5, p5)
        means, var = tr.calculate_means(q5.reshape(-1, 5), None, include_r2p=True, return_stds=True, no_samples=200)
        f = tr.context.fisher_information(means[:, :2].contiguous(), sg5.reshape(-1, 11), None, p5.reshape(-1, 5),
                                          m5.reshape(-1))
        live = m5.reshape(-1) > 0
        for k in ("oef_crlb", "dbv_crlb", "r2p_crlb", "corr", "kappa", "oef_bound", "dbv_bound", "r2p_bound"):
            assert got[k].shape == lead and same_bits(got[k].reshape(-1), f[k].contiguous()), k
            assert torch.isfinite(got[k].reshape(-1)[live]).all() and torch.isnan(got[k].reshape(-1)[~live]).all(), k
        for i, k in enumerate(("oef", "dbv", "r2p")):
            want = torch.sqrt(var[:, i]) / f[k + "_bound"]
            assert same_bits(got[k + "_ratio"].reshape(-1), want.contiguous()), k
            assert (got[k + "_ratio"].reshape(-1)[live] > 0).all()
        # the data alone bound no tighter than data and prior together; the ridge shows as |corr| near 1
        assert (got["oef_crlb"].reshape(-1)[live] >= got["oef_bound"].reshape(-1)[live]).all()
        assert got["corr"].reshape(-1)[live].abs().median().item() > 0.9


def test_protocol_search_is_a_local_optimum_and_reproducible(params):
    """scripts/design_protocol.py's search on 4,096 prior draws, the 11-tau grid and a budget of 22: the final
    D-criterion is no lower than the uniform allocation's and than every single-move neighbour's (both scored again
    here), and the allocation is the same run to run."""
    import importlib.util
    import os
    from qbold_vi_amd import training
    from qbold_vi_amd.ops import Context
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("design_protocol", os.path.join(root, "scripts", "design_protocol.py"))
    dp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dp)
    ctx = Context(params, True, True)
    n, budget = 4096, 22
    _, _, theta = training.synthetic_voxel_dataset(params, dict(full_model=True, use_blood=True), n, ctx.device, 1)
    theta = theta.contiguous()
    assert dr.in_range(theta.cpu().numpy()).all()
    sigma = torch.full((ctx.T,), 0.02, device=theta.device)
    prior = torch.tensor(dp.PRIOR_HEADS, device=theta.device).repeat(n, 1)
    for require_se in (False, True):
        w, d, d0, rounds = dp.search(ctx, theta, sigma, prior, budget, require_se)
        w2, d2, _, _ = dp.search(ctx, theta, sigma, prior, budget, require_se)
        assert np.array_equal(w, w2) and d == d2
        assert w.sum() == budget and (w >= 0).all() and (w == np.round(w)).all()
        uni = dp.uniform_allocation(ctx.T, budget)
        again = dp.d_criterion(ctx, theta, sigma, prior, np.stack([w, uni]))
        assert again[0] == d and again[1] == d0 and d >= d0
        nb = dp.neighbours(w, (ctx.se_idx,) if require_se else ())
        assert len(nb) > 0 and (dp.d_criterion(ctx, theta, sigma, prior, nb) <= d).all()
        print(f"[design] search (require_se={require_se}): {w.astype(int).tolist()} D {d:.5f} uniform {d0:.5f} "
              f"after {rounds} moves")
        if require_se:
            assert w[ctx.se_idx] >= 1


def test_save_predictions_writes_the_identifiability_maps(params, tmp_path):
    import gzip
    import os
    from oracle.oracle import Oracle, synth_inputs
    from qbold_vi_amd import EncoderTrainer, SignalGenerationLayer, nifti
    tr = EncoderTrainer(system_params=params, no_units=60, use_layer_norm=False, dropout_rate=0.0,
                        no_intermediate_layers=2, initial_im_sigma=0.05, activation_type='relu',
                        multi_image_normalisation=False, channelwise_gating=True, infer_inv_gamma=False,
                        use_population_prior=False, use_mvg=True, predict_log_data=False)
    model, _ = tr.create_encoder(gate_offset=-3.0, resid_init_std=0.05, no_ip_images=11)
    sig = lambda: SignalGenerationLayer(dict(params, simulate_noise='False'), True, True)   # noqa: E731
    B, X, Y, Z = 2, 6, 5, 4
    x, _ = synth_inputs(B * X * Y * Z, params, seed=12, oracle=Oracle("f32", params))
    mask = (np.random.default_rng(1).uniform(size=(B * X * Y * Z, 1)) > 0.2).astype(np.float32)
    data = dev(np.concatenate([x, mask], -1)).reshape(B, X, Y, Z, 12)
    priors = model(data[..., :-1])[0]
    d0, d1 = tmp_path / "plain", tmp_path / "ident"
    os.makedirs(d0)
    os.makedirs(d1)
    assert tr.save_predictions(model, data, str(d0 / "sub"), fine_tuner_model=tr.build_fine_tuner(model, sig()),
                               priors=priors) is None
    maps = tr.save_predictions(model, data, str(d1 / "sub"), fine_tuner_model=tr.build_fine_tuner(model, sig()),
                               priors=priors, identifiability=True)
    names = ("oef_crlb", "dbv_crlb", "r2p_crlb", "crlbcorr", "crlbkappa")
    extra = {f"sub_{k}.nii.gz" for k in names}
    plain = set(os.listdir(d0))
    assert set(os.listdir(d1)) == plain | extra and not (plain & extra)
    for f in plain:   # the earlier maps are unchanged (gzip stamps the time, so compare the content)
        with gzip.open(d0 / f, "rb") as a, gzip.open(d1 / f, "rb") as b:
            assert a.read() == b.read(), f
    live = mask.reshape(B, X, Y, Z) > 0
    for k in names:
        v = maps[k].cpu().numpy()
        assert v.shape == (B, X, Y, Z, 1) and np.all(np.isfinite(v)) and np.all(v[..., 0][~live] == 0.0), k
        img = nifti.load(str(d1 / f"sub_{k}.nii.gz"))[0]
        np.testing.assert_array_equal(img, np.concatenate(np.split(v, B, axis=0), axis=-1)[0])
    assert np.all(maps["oef_crlb"].cpu().numpy()[..., 0][live] > 0) and np.all(maps["crlbkappa"].cpu().numpy()[..., 0][live] >= 1)
    with pytest.raises(ValueError, match="fine tuner"):
        tr.save_predictions(model, data, str(d1 / "none"), identifiability=True)
