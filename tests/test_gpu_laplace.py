"""qbold_laplace_posterior (laplace_kernel) against the float64 restatement of tests/_laplace_reference.py on the
reference's 11 and 24 taus and on the protocol table of tests/test_gpu_forward_protocols.py (2 - 64 taus, left-heavy,
right-only, off-grid spin echo, T % 4 != 0, three-image normalisation), 333 voxels each: two full 128-thread blocks, a
partial one and a partial wave.  The iteration path is not pinned: every check is made at the kernel's own u^.

Bounds.  Stationarity: the kernel stops where its float32 decrement is below tol, and g's float32 rounding is ~1e-5 in
decrement units, so the float64 decrement at u^ is held to 2 tol.  Columns 2-4, 11, 12: DESIGN section 2's 1e-4 rel_1.
Columns 5-10 inherit A's condition number: 4 x the maximum measured over all protocols, rounded up to one digit
(MEASUREMENTS.md section 27 has both numbers), under the hard ceiling of 1e-2.  Heads: float32 rounding of the five
transforms and their inverses is ~5e-7 relative in the Cholesky factor (atanh's slope 1 / (1 - t^2) and tanh's slope
cancel), held to 1e-5."""
import ctypes as C
import gzip
import math
import os

import numpy as np
import pytest

import _laplace_reference as lr
import test_gpu_forward_protocols as fp
from _iw_reference import dw_coef, rel, rel1

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAMES = lr.protocol_names()
TOL = lr.DEFAULTS["tol"]
# columns 5-10 against float64 at the kernel's u^: (measured maximum over all protocols, bound = 4 x, one digit up)
SD_ERR = {"sd_a": (2.133e-5, 9e-5), "sd_b": (2.124e-5, 9e-5), "corr": (2.994e-7, 2e-6), "oef_sd": (2.136e-5, 9e-5),
          "dbv_sd": (2.123e-5, 9e-5), "r2p_sd": (1.643e-5, 7e-5)}
SD_CEILING = 1e-2
# |Laplace log p^ - grid log_p| - quad_err over the voxels with edge_mass < 1e-6: the Laplace approximation's own error
# on posteriors that are not Gaussian, not rounding (measured maximum, bound = 2 x, one digit up)
EVIDENCE_GAP = (0.2505, 0.6)
HEADS_TOL = 1e-5

dev, _same_bits = fp.dev, fp._same_bits
_CASES = {}


def case(params, name):
    """Inputs, context, the kernel's outputs at the defaults (prior start, NaN data in the masked voxels) and the
    float64 reference at the kernel's u^ for the live voxels; computed once per protocol."""
    if name not in _CASES:
        from oracle.oracle import Oracle
        from qbold_vi_amd.ops import Context
        p, sw = lr.setup(params, name)
        d = lr.inputs(Oracle("f32", p, **sw), name)
        ctx = Context(p, True, True, **sw)
        x = d["x"].copy()
        x[~d["live"]] = np.nan
        t = dict(x=dev(x), mask=dev(d["mask"]), prior=dev(d["prior"]), sigma=dev(d["sigma"]))
        q_out, out = ctx.laplace_posterior(t["x"], t["mask"], t["prior"], t["sigma"])
        torch.cuda.synchronize()
        qn, on = q_out.cpu().numpy(), out.cpu().numpy()
        live = np.nonzero(d["live"])[0]
        u_hat = on[live, 0:2].astype(np.float64)
        with fp.float64_oracle(p, sw) as o64:
            m = lr.model_of(o64, d, sw)
            ev = m.evaluate(u_hat, live)
            ref_out, ref_q = lr.outputs(m, u_hat, dw_coef(p), live, ev=ev)
            F0 = m.F(m.mu[live], live)
        _CASES[name] = dict(p=p, sw=sw, d=d, ctx=ctx, t=t, q_out=q_out, out=out, qn=qn, on=on, live=live, ev=ev,
                            ref_out=ref_out, ref_q=ref_q, F0=F0)
    return _CASES[name]


@pytest.mark.parametrize("name", NAMES)
def test_stationary_and_converged_and_monotone(params, name):
    c = case(params, name)
    on, live, ev = c["on"], c["live"], c["ev"]
    assert c["ctx"].T == c["d"]["x"].shape[1]
    flags = on[live, 14].astype(int)
    conv = (flags & 1) == 0
    dec = ev["dec"]
    print(f"[laplace] {name}: float64 decrement at u^ max {dec[conv].max():.3e} (tol {TOL:g}); iterations mean "
          f"{on[live, 13].mean():.2f} max {on[live, 13].max():.0f}; not converged {int((~conv).sum())}; "
          f"on clip {int(((flags >> 1) & 1).sum())}; clamped {int(((flags >> 2) & 1).sum())} of {live.size}")
    assert np.all(np.isfinite(on[live])) and np.all(np.isfinite(c["qn"]))
    assert np.all(dec[conv] <= 2 * TOL)
    assert conv.all(), np.nonzero(~conv)[0]
    assert np.all(on[live, 13] >= 0) and np.all(on[live, 13] <= lr.DEFAULTS["max_iter"])
    # monotone: F64(u^) <= F64(u0), u0 = the prior mean
    assert np.all(ev["F"] <= c["F0"])


@pytest.mark.parametrize("name", NAMES)
def test_outputs_match_float64_at_the_kernels_own_map(params, name):
    c = case(params, name)
    got, ref = c["on"][c["live"]].astype(np.float64), c["ref_out"]
    errs = dict(oef=rel1(got[:, 2], ref[:, 2]), dbv=rel1(got[:, 3], ref[:, 3]), r2p=rel1(got[:, 4], ref[:, 4]),
                chi2=rel1(got[:, 12], ref[:, 12]), log_p=rel1(got[:, 11], ref[:, 11]))
    sds = dict(sd_a=rel(got[:, 5], ref[:, 5]), sd_b=rel(got[:, 6], ref[:, 6]),
               corr=float(np.max(np.abs(got[:, 7] - ref[:, 7]))), oef_sd=rel(got[:, 8], ref[:, 8]),
               dbv_sd=rel(got[:, 9], ref[:, 9]), r2p_sd=rel(got[:, 10], ref[:, 10]))
    print(f"[laplace] {name}:", " ".join(f"{k}={v:.3e}" for k, v in {**errs, **sds}.items()))
    fails = [(k, v) for k, v in errs.items() if not v <= 1e-4]
    fails += [(k, v, SD_ERR[k][1]) for k, v in sds.items() if not v <= min(SD_ERR[k][1], SD_CEILING)]
    assert not fails, fails
    # columns 0-1 are the heads' means, bit for bit
    assert np.array_equal(c["on"][c["live"], 0], c["qn"][c["live"], 0])
    assert np.array_equal(c["on"][c["live"], 1], c["qn"][c["live"], 2])


@pytest.mark.parametrize("name", NAMES)
def test_known_answer_on_noise_free_data(params, name):
    """Noise-free data, the prior centred on the truth's logits, the start displaced by (+1.0, -0.8): the MAP is the
    truth.  chi2: DESIGN section 2's NLL bound, |chi2 / 2 - 0| <= 1e-4 (|0| + 1)."""
    from oracle.oracle import Oracle
    c = case(params, name)
    p, sw, ctx = c["p"], c["sw"], c["ctx"]
    d = lr.inputs(Oracle("f32", p, **sw), name, noise=False)
    prior = d["prior"].copy()
    prior[:, 0], prior[:, 2] = d["u_true"][:, 0], d["u_true"][:, 1]
    u0 = (prior[:, [0, 2]] + np.array([1.0, -0.8], np.float32)).astype(np.float32)
    q_out, out = ctx.laplace_posterior(dev(d["x"]), None, dev(prior), dev(d["sigma"]), u0=dev(u0))
    out = out.cpu().numpy().astype(np.float64)
    with fp.float64_oracle(p, sw) as o64:
        m = lr.Model(o64, d["x"], d["sigma"], prior, multi=bool(sw))
        ref, _ = lr.outputs(m, prior[:, [0, 2]].astype(np.float64), dw_coef(p))
    off = np.abs(out[:, 0:2] - prior[:, [0, 2]]) / ref[:, 5:7]
    print(f"[laplace] {name} known answer: |u^ - u_true| max {off.max():.3e} sds, chi2 max {out[:, 12].max():.3e}, "
          f"iterations max {out[:, 13].max():.0f}")
    assert np.all(out[:, 14].astype(int) & 1 == 0)
    assert np.all(off <= 5e-3)
    assert np.all(out[:, 12] <= 2e-4)


@pytest.mark.parametrize("name", ("ref11", "odd33"))
def test_global_optimum_and_evidence_against_the_grid(params, name):
    c = case(params, name)
    d, ctx, t = c["d"], c["ctx"], c["t"]
    rows = c["live"][:64]
    idx = dev(rows.astype(np.int64))
    _, grid, _ = ctx.posterior_grid(t["x"][idx], None, t["prior"][idx], t["sigma"][idx])
    grid = grid.cpu().numpy().astype(np.float64)
    node = np.stack([np.log((grid[:, 13] - 0.04) / (0.84 - grid[:, 13])),
                     np.log((grid[:, 14] - 0.001) / (0.201 - grid[:, 14]))], -1)
    with fp.float64_oracle(c["p"], c["sw"]) as o64:
        F_node = lr.model_of(o64, d, c["sw"]).F(node, rows)
    F_hat = c["ev"]["F"][:64]
    print(f"[laplace] {name} grid: F64(u^) - F64(argmax node) max {np.max(F_hat - F_node):.3e}")
    assert np.all(F_hat <= F_node + 1e-6 * np.abs(F_node))
    inside = grid[:, 15] < 1e-6
    gap = np.abs(c["on"][rows, 11] - grid[:, 0]) - grid[:, 16]
    print(f"[laplace] {name} grid: |log p^ - log_p| - quad_err max {gap[inside].max():.3e} over {int(inside.sum())} "
          f"voxels with edge_mass < 1e-6")
    assert inside.sum() >= 32
    assert np.all(gap[inside] <= EVIDENCE_GAP[1])


def test_heads_reproduce_the_map_and_the_covariance(params):
    n_clamped = n_plain = 0
    for name in NAMES:
        c = case(params, name)
        live = c["live"]
        on, qn = c["on"][live].astype(np.float64), c["qn"][live]
        Sigma = np.zeros((live.size, 2, 2))
        Sigma[:, 0, 0], Sigma[:, 1, 1] = on[:, 5] ** 2, on[:, 6] ** 2
        Sigma[:, 0, 1] = Sigma[:, 1, 0] = on[:, 7] * on[:, 5] * on[:, 6]
        want_q, want_clamped, t_raw = lr.heads_from(on[:, 0:2], Sigma, want_t=True)
        mu, S_got = lr.heads_cov(qn)
        _, S_want = lr.heads_cov(want_q)
        assert np.array_equal(mu, on[:, 0:2])
        # in Cholesky terms (sd_a, c, e^sd), each relative to its own size or to sd_b
        Lg, Lw = np.linalg.cholesky(S_got), np.linalg.cholesky(S_want)
        err = np.abs(Lg - Lw) / np.sqrt(S_want[:, 1, 1])[:, None, None]
        err[:, 0, 0] = np.abs(Lg[:, 0, 0] - Lw[:, 0, 0]) / Lw[:, 0, 0]
        flag = ((on[:, 14].astype(int) >> 2) & 1) == 1
        # the flag may differ from float64's only where a tanh lands within float32 rounding of the clamp
        edge = (np.abs(np.abs(t_raw) - lr.TANH_MAX) < 1e-5).any(1)
        print(f"[laplace] {name} heads: max error {err.max():.3e}; clamped {int(flag.sum())} of {live.size}")
        assert err.max() <= HEADS_TOL
        assert np.array_equal(flag[~edge], want_clamped[~edge])
        ok = ~flag
        # unclamped voxels: mvn(q_out) is (u^, Sigma) itself
        assert np.max(np.abs(S_got[ok] - Sigma[ok]) / np.sqrt(np.einsum("nii,njj->nij", Sigma[ok], Sigma[ok]))) <= 4 * HEADS_TOL
        # a clamped c keeps the marginal variance of b (whenever s_d is in range)
        keeps = flag & (np.abs(t_raw[:, 1]) < lr.TANH_MAX - 1e-5)
        if keeps.any():
            assert np.max(np.abs(S_got[keeps, 1, 1] / Sigma[keeps, 1, 1] - 1.0)) <= 4 * HEADS_TOL
        n_clamped += int(flag.sum())
        n_plain += int(ok.sum())
    assert n_clamped >= 20 and n_plain >= 20, (n_clamped, n_plain)


@pytest.mark.parametrize("name", ("odd33", "ref24", "off22_3img"))
def test_bits(params, name):
    c = case(params, name)
    ctx, t, d = c["ctx"], c["t"], c["d"]
    n, T = lr.N_VOX, ctx.T
    args = [t[k] for k in ("x", "mask", "prior", "sigma")]
    q2, o2 = ctx.laplace_posterior(*args)
    assert _same_bits(q2, c["q_out"]) and _same_bits(o2, c["out"])
    for h in (1, 17, 128, 200):
        qa, oa = ctx.laplace_posterior(*[a[:h] for a in args])
        qb, ob = ctx.laplace_posterior(*[a[h:] for a in args])
        assert _same_bits(torch.cat([qa, qb]), c["q_out"]) and _same_bits(torch.cat([oa, ob]), c["out"]), h
    e = [torch.empty((0, w), device="cuda") for w in (T, 5, T)]
    q0, o0 = ctx.laplace_posterior(e[0], torch.empty(0, device="cuda"), e[1], e[2])
    assert q0.shape == (0, 5) and o0.shape == (0, 15)
    # masked rows: NaN in out, the prior's row in q_out, bit for bit (their data are NaN)
    dead = dev(~d["live"])
    assert torch.isnan(c["out"][dead]).all()
    assert _same_bits(c["q_out"][dead], t["prior"][dead])
    # mask None evaluates every voxel: the live rows keep their bits whatever the mask weights are
    keep = np.array([5, 63, 64, 70, 200, 255, 256, 332])
    keep = keep[d["live"][keep]]
    assert keep.size >= 4
    # a voxel's row does not depend on its wave-mates: replace everybody else's data and prior
    rng = np.random.default_rng(8)
    x2 = (d["x"] * rng.uniform(0.7, 1.3, d["x"].shape)).astype(np.float32)
    p2 = (d["prior"] + rng.normal(size=d["prior"].shape) * 0.3).astype(np.float32)
    x2[keep], p2[keep] = d["x"][keep], d["prior"][keep]
    q3, o3 = ctx.laplace_posterior(dev(x2), None, dev(p2), t["sigma"])
    ki = dev(keep.astype(np.int64))
    assert _same_bits(q3[ki], c["q_out"][ki]) and _same_bits(o3[ki], c["out"][ki])
    others = np.setdiff1d(c["live"], keep)
    assert not torch.equal(o3[dev(others)], c["out"][dev(others)])
    assert torch.isfinite(o3[:, :13]).all()   # mask None: every voxel evaluated


def test_consumers_take_the_heads_at_33_taus(params):
    c = case(params, "odd33")
    ctx, t = c["ctx"], c["t"]
    x = dev(c["d"]["x"])   # finite data everywhere: the consumers below read masked rows of some buffers
    q = c["q_out"]
    sums_q, nk = ctx.elbo_fwd(x, t["mask"], q, t["prior"], t["sigma"], 32, 70, seed=3)
    sums_p, _ = ctx.elbo_fwd(x, t["mask"], t["prior"], t["prior"], t["sigma"], 32, 70, seed=3)
    live = dev(c["d"]["live"])
    assert torch.isfinite(nk[live]).all()
    sq, sp = sums_q.cpu().numpy(), sums_p.cpu().numpy()
    eq, ep = (sq[0] + sq[1]) / sq[2], (sp[0] + sp[1]) / sp[2]
    print(f"[laplace] odd33 consumers: mean -ELBO of the Laplace heads {eq:.4f}, of the prior as q {ep:.4f}")
    assert eq < ep
    lw, th = ctx.log_evidence_draws(x, t["mask"], q, t["prior"], t["sigma"], 64, seed=5, want_theta=True)
    po, pm, _ = ctx.psis(lw, th, t["mask"])
    assert torch.isfinite(po[live]).all() and torch.isfinite(pm[live]).all()
    print(f"[laplace] odd33 consumers: PSIS k^ median {po[live, 0].median().item():.3f} max {po[live, 0].max().item():.3f}")
    _, ev, _ = ctx.log_evidence(x, t["mask"], q, t["prior"], t["sigma"], 64, seed=5)
    assert torch.isfinite(ev[live]).all()
    _, grid, _ = ctx.posterior_grid(x[:48], t["mask"][:48], t["prior"][:48], t["sigma"][:48], q=q[:48])
    assert torch.isfinite(grid[live[:48]]).all()
    # the exact ELBO of the Laplace heads is below the exact evidence
    assert (grid[live[:48], 1] <= grid[live[:48], 0] + 1e-3).all()


def test_errors(params):
    from qbold_vi_amd import _lib
    from qbold_vi_amd.ops import Context
    c = case(params, "ref11")
    ctx, t = c["ctx"], c["t"]
    n = 64
    x, prior, sigma = t["x"][:n].contiguous(), t["prior"][:n].contiguous(), t["sigma"][:n].contiguous()
    q_out, out = torch.empty((n, 5), device="cuda"), torch.empty((n, 15), device="cuda")
    P = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None   # noqa: E731
    nan, inf = float("nan"), float("inf")

    def call(cx, max_iter=50, lambda0=1e-2, up=10.0, down=3.0, tol=1e-3, xx=x, pp=prior, ss=sigma, qq=q_out, oo=out,
             cfg=True, N=n):
        cf = _lib.LaplaceCfg(max_iter, lambda0, up, down, tol)
        return cx.lib.qbold_laplace_posterior(cx.handle, P(xx), None, P(pp), P(ss), None,
                                              C.byref(cf) if cfg else None, P(qq), P(oo), N, None)
    assert call(ctx) == _lib.QBOLD_OK
    torch.cuda.synchronize()
    assert call(ctx, max_iter=0) == -1 and call(ctx, max_iter=-3) == -1
    for bad in (0.0, -1.0, nan, inf):
        assert call(ctx, lambda0=bad) == -1 and call(ctx, tol=bad) == -1, bad
    assert call(ctx, up=1.0) == -1 and call(ctx, down=1.0) == -1 and call(ctx, up=0.5) == -1 and call(ctx, down=nan) == -1
    assert call(ctx, xx=None) == -1 and call(ctx, pp=None) == -1 and call(ctx, ss=None) == -1
    assert call(ctx, qq=None) == -1 and call(ctx, oo=None) == -1 and call(ctx, cfg=False) == -1 and call(ctx, N=-1) == -1
    # configurations without a kernel
    lit = Context(params, True, True)
    lit.set_tissue_mode("literal")
    assert call(lit) == -3
    assert call(Context(params, True, True, student_t_df=4.0)) == -3
    assert call(Context(params, True, True, predict_log_data=True)) == -3
    assert call(Context(params, False, True)) == -3
    # the refinement entry keeps refusing 64 taus
    c64 = Context(dict(params, tau_start="-0.015", tau_end="0.065", tau_step="0.00125"), True, True)
    assert c64.T == 64
    x64, s64 = torch.ones((n, 64), device="cuda"), torch.full((n, 64), 0.02, device="cuda")
    rcfg = _lib.RefineCfg(0, 0.05, 0.05, 0.9, 0.999, 1e-8)
    assert c64.lib.qbold_refine_posterior(c64.handle, P(x64), None, P(prior), P(prior), P(s64), None, 5, 1,
                                          C.byref(rcfg), 1, 0, P(q_out), None, n, None) == -3
    assert call(c64, xx=x64, ss=s64) == _lib.QBOLD_OK
    torch.cuda.synchronize()


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


def test_fine_tuner_laplace_voxel_batch_and_crops(trainer, params):
    from oracle.oracle import Oracle, synth_inputs
    o32 = Oracle("f32", params)
    model, ft = _fine_tuner(trainer, params)
    for lead, seed in (((500, 1, 1, 1), 3), ((2, 9, 7, 4), 8)):
        nv = int(np.prod(lead))
        x, _ = synth_inputs(nv, params, seed=seed, oracle=o32)
        x5 = dev(x).reshape(lead + (11,))
        m5 = dev((np.random.default_rng(seed).uniform(size=nv) > 0.3).astype(np.float32)).reshape(lead + (1,))
        p5 = model(x5)[0]
        _, q5, sg5 = model.predict(x5, want=("out2", "sigma"))
        for start in ("prior", "encoder"):
            got = ft.laplace(x5, m5, p5, start=start, max_iter=40)
            u0 = q5.reshape(-1, 5)[:, [0, 2]].contiguous() if start == "encoder" else None
            q_w, o_w = trainer.context.laplace_posterior(x5.reshape(-1, 11), m5.reshape(-1), p5.reshape(-1, 5),
                                                         sg5.reshape(-1, 11), u0=u0, max_iter=40)
            assert got["q"].shape == lead + (5,) and got["map"].shape == lead + (2,)
            assert _same_bits(got["q"].reshape(-1, 5), q_w)
            for key, col in (("oef", 2), ("dbv", 3), ("r2p", 4), ("corr", 7), ("oef_sd", 8), ("dbv_sd", 9),
                             ("r2p_sd", 10), ("log_evidence", 11), ("chi2", 12), ("iterations", 13)):
                assert got[key].shape == lead and _same_bits(got[key].reshape(-1), o_w[:, col].contiguous()), key
            assert _same_bits(got["map"].reshape(-1, 2), o_w[:, 0:2].contiguous())
            assert _same_bits(got["logit_sd"].reshape(-1, 2), o_w[:, 5:7].contiguous())
            live = m5.reshape(-1) > 0
            flags = torch.nan_to_num(o_w[:, 14]).int()
            assert torch.equal(got["converged"].reshape(-1), live & ((flags & 1) == 0))
            assert torch.equal(got["on_clip"].reshape(-1), (flags & 2) != 0)
            assert torch.equal(got["clamped"].reshape(-1), (flags & 4) != 0)
            assert got["converged"].reshape(-1)[live].float().mean().item() > 0.9
            assert not got["converged"].reshape(-1)[~live].any()
        # the heads go to the other entries unchanged
        e = ft.elbo(x5, m5, p5, no_samples=4, seed=2, q=got["q"])
        assert math.isfinite(float(e["elbo"]))
    with pytest.raises(ValueError, match="start"):
        ft.laplace(x5, m5, p5, start="map")


def test_save_predictions_writes_the_laplace_maps(trainer, params, tmp_path):
    from oracle.oracle import Oracle, synth_inputs
    from qbold_vi_amd import nifti
    model, ft = _fine_tuner(trainer, params)
    B, X, Y, Z = 2, 6, 5, 4
    x, _ = synth_inputs(B * X * Y * Z, params, seed=12, oracle=Oracle("f32", params))
    mask = (np.random.default_rng(1).uniform(size=(B * X * Y * Z, 1)) > 0.2).astype(np.float32)
    data = dev(np.concatenate([x, mask], -1)).reshape(B, X, Y, Z, 12)
    priors = model(data[..., :-1])[0]
    d0, d1 = tmp_path / "plain", tmp_path / "laplace"
    os.makedirs(d0)
    os.makedirs(d1)
    assert trainer.save_predictions(model, data, str(d0 / "sub"), fine_tuner_model=ft, priors=priors) is None
    _, ft1 = _fine_tuner(trainer, params, model)   # a fresh fine tuner: its sampling layer counts its calls
    maps = trainer.save_predictions(model, data, str(d1 / "sub"), fine_tuner_model=ft1, priors=priors, laplace=True)
    names = ("oef_laplace", "dbv_laplace", "r2p_laplace", "oefsd_laplace", "dbvsd_laplace", "logevidence_laplace",
             "chi2", "laplaceflags")
    extra = {f"sub_{k}.nii.gz" for k in names}
    plain = set(os.listdir(d0))
    assert set(os.listdir(d1)) == plain | extra and not (plain & extra)
    for f in plain:   # the earlier maps are unchanged, byte for byte (gzip stamps the time, so compare the content)
        with gzip.open(d0 / f, "rb") as a, gzip.open(d1 / f, "rb") as b:
            assert a.read() == b.read(), f
    live = mask.reshape(B, X, Y, Z) > 0
    for k in names:
        v = maps[k].cpu().numpy()
        assert v.shape == (B, X, Y, Z, 1) and np.all(np.isfinite(v)), k
        assert np.all(v[..., 0][~live] == 0.0), k
        img = nifti.load(str(d1 / f"sub_{k}.nii.gz"))[0]
        np.testing.assert_array_equal(img, np.concatenate(np.split(v, B, axis=0), axis=-1)[0])
    oef = maps["oef_laplace"].cpu().numpy()[..., 0][live]
    assert np.all((oef > 0.04) & (oef < 0.84))
    with pytest.raises(ValueError, match="fine tuner"):
        trainer.save_predictions(model, data, str(d1 / "none"), laplace=True)
