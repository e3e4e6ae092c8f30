"""Credible intervals from importance draws (qbold_draw_summary, Context.draw_summary, FineTuner.credible_intervals,
save_predictions(interval_samples=K)) against the float64 restatement of tests/_summary_reference.py.

Quantiles and interval ends are order statistics, so they are held to the reference without any tolerance on their
values: the kernel's float32 W_r lies within eps / 2 = (K + 32) 2^-24 of the float64 one, hence
q_ref(p - eps) <= kernel <= q_ref(p + eps), asserted with <= on float32-exact values, and where the two reference
values coincide (tests/test_summary_host.py holds the rows to how often they must) the kernel value is pinned exactly.
The interval is held the same way in its mass and its width."""
import ctypes as C
import gzip
import math
import os

import numpy as np
import pytest

import _summary_reference as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# NJ = 1 (K <= 64), 2 (<= 128), 4 (<= 256), 8 (<= 512) and 16 register slots: 4, 25, 64 | 65, 100 | 225 | 500 | 1000, 1024;
# 65: a slot with one live draw.  tests/test_summary_host.py holds the rows of exactly these K to their tightness limits.
KS = (4, 25, 64, 65, 100, 225, 500, 1000, 1024)
# Largest relative error of mean / sd / ESS / largest weight and absolute error of corr against float64 over the
# 9 x 240 rows, measured on the MI355X (MEASUREMENTS.md section 36); held to min(4 x measured, 1e-4).
MOMENT_MEASURED = 4.85e-7    # the ESS at K = 500
CORR_MEASURED = 2.07e-7      # at K = 4
CAP = 1e-4


def _bound(measured):
    return min(4.0 * measured, CAP)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def host(t):
    return None if t is None else t.cpu().numpy().astype(np.float64)


def _same_bits(a, b):
    """bitwise equality (NaN included)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


@pytest.fixture(scope="module")
def ctx(params):
    from qbold_vi_amd.ops import Context
    return Context(params, full_model=True, include_blood=True)


def summary(ctx, theta, lw=None, mask=None, **kw):
    kw.setdefault("probs", R.LEVELS)
    kw.setdefault("hpd_mass", R.MASS)
    kw.setdefault("want_corr", True)
    return ctx.draw_summary(dev(theta), None if lw is None else dev(lw), None if mask is None else dev(mask), **kw)


# ---- 1. rows against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_rows_match_float64_reference(ctx, K):
    r = R.reference(K)
    lw, theta = r["lw"], r["theta"]
    stats, quant, row_out, corr = (host(t) for t in summary(ctx, theta, lw))
    assert stats.shape == (240, 3, 4) and quant.shape == (240, 3, 5) and row_out.shape == (240, 2)
    assert corr.shape == (240, 3)
    # quantiles: the sandwich, and every value a draw of its column
    assert np.all(r["q_lo"] <= quant) and np.all(quant <= r["q_hi"])
    assert np.all((quant[:, None] == theta.astype(np.float64)[..., None]).any(1))
    pinned = float(np.mean(r["q_lo"] == r["q_hi"]))
    # the interval: its mass, its width between the reference widths at mass -+ eps, its ends draws of the column
    e = R.eps(K)
    lo, hi = stats[..., 2], stats[..., 3]
    th64 = theta.astype(np.float64)
    assert np.all((lo[:, None] == th64).any(1)) and np.all((hi[:, None] == th64).any(1)) and np.all(lo <= hi)
    inside = (th64 >= lo[:, None]) & (th64 <= hi[:, None])
    mass = (r["w"][..., None] * inside).sum(1)
    assert np.all(mass >= R.MASS - e), float(mass.min())
    width = hi - lo
    assert np.all(width <= r["hpd_hi"][..., 1] - r["hpd_hi"][..., 0])
    assert np.all(width >= r["hpd_lo"][..., 1] - r["hpd_lo"][..., 0])
    # moments
    errs = dict(mean=rel(stats[..., 0], r["mean"]), sd=rel(stats[..., 1], r["sd"]), ess=rel(row_out[:, 0], r["ess"]),
                wmax=rel(row_out[:, 1], r["wmax"]), corr=float(np.max(np.abs(corr - r["corr"]))))
    print(f"K={K} eps={e:.3e} pinned quantiles {pinned:.4f}", errs)
    assert max(errs[k] for k in ("mean", "sd", "ess", "wmax")) <= _bound(MOMENT_MEASURED), (K, errs)
    assert errs["corr"] <= _bound(CORR_MEASURED), (K, errs)


# ---- 2. edge rows ----------------------------------------------------------------------------------------------------
def test_edge_rows(ctx):
    K = 64
    r = R.reference(K)
    rng = np.random.default_rng(2)
    names = ("nan", "plus_inf", "all_minus_inf", "minus_inf", "one_weight", "column_nan", "ties", "masked", "plain",
             "zeros")
    ix = {k: i for i, k in enumerate(names)}
    lw = r["lw"][:len(names)].copy()
    theta = r["theta"][:len(names)].copy()
    lw[ix["nan"], 17] = np.nan
    lw[ix["plus_inf"], 5] = np.inf
    lw[ix["all_minus_inf"]] = -np.inf
    dead = np.array([3, 40, 63])
    lw[ix["minus_inf"], dead] = -np.inf
    theta[ix["minus_inf"], dead, 0] = [0.0, 1.0, 2.0]           # below, inside and above the live draws
    lw[ix["one_weight"]] = -np.inf
    lw[ix["one_weight"], 29] = -3.0
    theta[ix["column_nan"], 11, 1] = np.nan
    theta[ix["ties"]] = rng.choice(np.array([0.5, 0.75, 1.0, 1.25, 1.5], np.float32), (K, 3))
    # -0 and +0 are one value: ties by draw, and a returned zero is +0.  Column 0: zeros of both signs below the other
    # draws, so the low quantiles and the interval's lower end are zeros; column 1: every draw a zero
    zi = ix["zeros"]
    theta[zi, :40, 0] = np.where(np.arange(40) % 2 == 0, -0.0, 0.0).astype(np.float32)
    theta[zi, :, 1] = np.where(np.arange(K) % 3 == 0, 0.0, -0.0).astype(np.float32)
    lw[ix["masked"]] = np.nan                                    # poisoned: must not be read
    theta[ix["masked"]] = np.nan
    mask = np.ones(len(names), np.float32)
    mask[ix["masked"]] = 0.0
    stats, quant, row_out, corr = (host(t) for t in summary(ctx, theta, lw, mask))
    for k in ("nan", "plus_inf", "all_minus_inf", "masked"):
        i = ix[k]
        assert all(np.all(np.isnan(a[i])) for a in (stats, quant, row_out, corr)), k

    i = ix["minus_inf"]
    w = R.weights(lw[i])
    assert not np.isin(quant[i, 0], theta[i, dead, 0].astype(np.float64)).any()      # never a quantile
    assert not np.isin(stats[i, 0, 2:], theta[i, dead, 0].astype(np.float64)).any()
    R.check_sandwich(theta[i], w, quant[i], stats[i], R.LEVELS, R.MASS)

    i = ix["one_weight"]
    v = theta[i, 29].astype(np.float64)
    assert np.array_equal(quant[i], np.repeat(v[:, None], 5, 1))
    assert np.array_equal(stats[i, :, 0], v) and np.all(stats[i, :, 1] == 0.0)
    assert np.array_equal(stats[i, :, 2], v) and np.array_equal(stats[i, :, 3], v)
    assert np.all(np.isnan(corr[i])) and row_out[i, 0] == 1.0 and row_out[i, 1] == 1.0

    i = ix["column_nan"]
    w = R.weights(lw[i])
    assert np.all(np.isnan(stats[i, 1])) and np.all(np.isnan(quant[i, 1]))
    assert np.all(np.isnan(corr[i, [0, 2]])) and np.isfinite(corr[i, 1])             # pairs (0,1), (1,2); (0,2) stays
    keep = [0, 2]
    R.check_sandwich(theta[i][:, keep], w, quant[i, keep], stats[i, keep], R.LEVELS, R.MASS)
    m = R.moments(theta[i][:, keep], w)
    assert rel(stats[i, keep, 0], m["mean"]) < CAP and rel(stats[i, keep, 1], m["sd"]) < CAP
    assert abs(row_out[i, 0] - m["ess"]) < CAP * m["ess"] and abs(corr[i, 1] - m["corr"][0]) < CAP

    for k in ("ties", "plain", "zeros"):
        i = ix[k]
        R.check_sandwich(theta[i], R.weights(lw[i]), quant[i], stats[i], R.LEVELS, R.MASS)

    i = ix["zeros"]
    assert quant[i, 0, 0] == 0.0 and stats[i, 0, 2] == 0.0 and np.all(quant[i, 1] == 0.0)
    assert np.all(stats[i, 1] == 0.0) and np.all(np.isnan(corr[i, [0, 2]]))          # sd 0: no correlation with column 1
    zeros = np.concatenate([quant[i, 0, :1], stats[i, 0, 2:3], quant[i, 1], stats[i, 1]])
    assert not np.signbit(zeros).any()                                               # +0, whichever draw was met


def test_equal_weights(ctx):
    """log_w = None is an explicit constant row, bit for bit, and numpy's inverted_cdf of the column."""
    K = 100
    theta = R.reference(K)["theta"][:40]
    levels = (0.0251, 0.1003, 0.5009, 0.9751)                   # no multiple of 1 / K
    none = summary(ctx, theta, None, probs=levels)
    const = summary(ctx, theta, np.full((40, K), -7.25, np.float32), probs=levels)
    assert all(_same_bits(a, b) for a, b in zip(none, const))
    want = np.quantile(theta.astype(np.float64), levels, axis=1, method="inverted_cdf")   # [P, N, C]
    assert np.array_equal(host(none[1]), np.moveaxis(want, 0, -1))
    assert np.allclose(host(none[2]), [K, 1.0 / K], rtol=1e-5, atol=0)


# ---- 3. bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (25, 100, 225, 500, 1000))            # one K per register-slot count
def test_batch_position_and_requested_outputs_keep_the_bits(ctx, K):
    r = R.reference(K)
    lw, theta = r["lw"], r["theta"]
    full = summary(ctx, theta, lw)
    again = summary(ctx, theta, lw)
    assert all(_same_bits(a, b) for a, b in zip(full, again))
    perm = np.random.default_rng(4).permutation(240)
    moved = summary(ctx, theta[perm], lw[perm])
    back = torch.as_tensor(np.argsort(perm), device="cuda")
    assert all(_same_bits(m[back], f) for m, f in zip(moved, full))
    for a, b in ((0, 1), (7, 8), (0, 5), (233, 238), (239, 240)):       # N = 1 and N = 5: no multiple of a block's rows
        part = summary(ctx, theta[a:b], lw[a:b])
        assert all(_same_bits(p, f[a:b]) for p, f in zip(part, full)), (a, b)
    stats, quant, row_out, corr = summary(ctx, theta, lw, probs=(), want_corr=False)
    assert quant is None and corr is None and _same_bits(stats, full[0]) and _same_bits(row_out, full[2])
    stats, quant, row_out, corr = summary(ctx, theta, lw, probs=R.LEVELS[1:3], want_corr=False)
    assert _same_bits(stats, full[0]) and _same_bits(quant, full[1][..., 1:3].contiguous())
    # columns are summarised independently: another width gives the same columns
    th8 = np.concatenate([theta, theta[..., ::-1], theta[..., :2]], -1)
    s8, q8, r8, c8 = summary(ctx, th8, lw)
    assert s8.shape == (240, 8, 4) and c8.shape == (240, 28)
    assert _same_bits(s8[:, :3].contiguous(), full[0]) and _same_bits(q8[:, :3].contiguous(), full[1])
    assert _same_bits(r8, full[2]) and _same_bits(s8[:, 3].contiguous(), full[0][:, 2].contiguous())


# ---- 4. argument errors ------------------------------------------------------------------------------------------------
def test_bad_arguments(ctx):
    from qbold_vi_amd import _lib
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    N, K, Cc = 4, 64, 3
    lw = torch.zeros((N, K), device="cuda")
    th = torch.rand((N, K, 8), device="cuda")
    stats = torch.empty((N, 8, 4), device="cuda")
    quant = torch.empty((N, 8, 8), device="cuda")
    row_out = torch.empty((N, 2), device="cuda")
    good = (C.c_float * 8)(0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8)

    def call(K=K, Cc=Cc, levels=good, Pn=3, mass=0.95, th_=th, stats_=stats, quant_=quant, row_=row_out, n=N):
        return ctx.lib.qbold_draw_summary(ctx.handle, P(lw), P(th_), Cc, None, K, C.cast(levels, C.c_void_p), Pn, mass,
                                          P(stats_), P(quant_), P(row_), None, n, None)
    assert call() == _lib.QBOLD_OK and call(K=4) == _lib.QBOLD_OK and call(Cc=8, Pn=8) == _lib.QBOLD_OK
    assert call(Pn=0, quant_=None) == _lib.QBOLD_OK and call(n=0) == _lib.QBOLD_OK
    assert call(K=3) == -1 and call(K=1025) == -1 and call(Cc=0) == -1 and call(Cc=9) == -1
    assert call(Pn=-1) == -1 and call(Pn=9) == -1 and call(quant_=None) == -1 and call(n=-1) == -1
    assert call(levels=(C.c_float * 8)(0.1, 0.0, 0.3)) == -1 and call(levels=(C.c_float * 8)(0.1, 0.2, 1.0)) == -1
    assert call(levels=(C.c_float * 8)(float("nan"), 0.2, 0.3)) == -1
    assert call(mass=0.0) == -1 and call(mass=1.0) == -1 and call(mass=float("nan")) == -1
    assert call(th_=None) == -1 and call(stats_=None) == -1 and call(row_=None) == -1
    t3 = th[..., :3].contiguous()
    for kw in (dict(probs=(0.5, 1.0)), dict(probs=(0.0,)), dict(probs=tuple([0.5] * 9)), dict(hpd_mass=1.0),
               dict(hpd_mass=0.0), dict(log_w=lw[:, :63]), dict(mask=torch.ones(5, device="cuda"))):
        with pytest.raises(ValueError):
            ctx.draw_summary(t3, **kw)
    with pytest.raises(ValueError):
        ctx.draw_summary(t3[:, :3])
    with pytest.raises(ValueError):
        ctx.draw_summary(torch.rand((N, K, 9), device="cuda"))
    with pytest.raises(ValueError):
        ctx.draw_summary(t3[0])
    torch.cuda.synchronize()


# ---- 5. end to end -----------------------------------------------------------------------------------------------------
def _trainer(p):
    from qbold_vi_amd import EncoderTrainer
    return EncoderTrainer(system_params=p, no_units=60, use_layer_norm=False, dropout_rate=0.0,
                          no_intermediate_layers=2, initial_im_sigma=0.05, activation_type='relu',
                          multi_image_normalisation=False, channelwise_gating=True, infer_inv_gamma=False,
                          use_population_prior=False, use_mvg=True, predict_log_data=False)


def _fine_tuner(tr, p, T):
    from qbold_vi_amd import SignalGenerationLayer
    model, _ = tr.create_encoder(gate_offset=-3.0, resid_init_std=0.05, no_ip_images=T)
    return model, tr.build_fine_tuner(model, SignalGenerationLayer(dict(p, simulate_noise='False'), True, True))


@pytest.mark.parametrize("proto", ("ref11", "odd33"))
def test_credible_intervals_end_to_end(params, proto):
    """FineTuner.credible_intervals(psis=True, no_samples=256) on 204 synthetic voxels against the reference applied to
    the very rows log_evidence_draws + psis(want_weights=True) return for the same seed and chunking."""
    import _refine_anyt_cases as rc
    from oracle.oracle import Oracle, synth_inputs
    from qbold_vi_amd.ops import psis_khat_threshold
    p = params if proto == "ref11" else rc.fp.protocol(params, proto)
    tr = _trainer(p)
    T = tr.context.T
    assert T == {"ref11": 11, "odd33": 33}[proto]
    model, ft = _fine_tuner(tr, p, T)
    lead, K, chunk, seed, v0 = (2, 17, 3, 2), 256, 90, 5, 1000003
    n = int(np.prod(lead))
    x, _ = synth_inputs(n, p, seed=9, oracle=Oracle("f32", p))
    x5 = dev(x).reshape(lead + (T,))
    m5 = dev((np.random.default_rng(3).uniform(size=n) > 0.25).astype(np.float32)).reshape(lead + (1,))
    p5 = model(x5)[0]
    levels = (0.025, 0.5, 0.975)
    got = ft.credible_intervals(x5, m5, p5, no_samples=K, psis=True, seed=seed, voxel0=v0, psis_chunk=chunk)
    assert set(got) == {"mean", "sd", "quantiles", "hpd", "corr_oef_dbv", "ess", "khat", "khat_threshold", "probs"}
    assert got["mean"].shape == lead + (3,) and got["sd"].shape == lead + (3,) and got["hpd"].shape == lead + (3, 2)
    assert got["quantiles"].shape == lead + (3, 3) and got["ess"].shape == lead and got["khat"].shape == lead
    assert got["khat_threshold"] == psis_khat_threshold(K) and got["probs"] == levels
    # the rows behind it
    q, sg = ft._heads_and_sigma(x5)
    xf, mf, pf = x5.reshape(-1, T), m5.reshape(-1), p5.reshape(-1, 5).contiguous()
    live = mf.cpu().numpy() > 0
    quant = host(got["quantiles"]).reshape(n, 3, 3)
    stats = np.concatenate([host(got["mean"]).reshape(n, 3, 1), host(got["sd"]).reshape(n, 3, 1),
                            host(got["hpd"]).reshape(n, 3, 2)], -1)
    pinned = cases = 0
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        lw, th = tr.context.log_evidence_draws(xf[a:b], mf[a:b], q[a:b], pf[a:b], sg[a:b], K, seed=seed, voxel0=v0 + a,
                                               want_theta=True)
        po, _, wts = tr.context.psis(lw, None, mf[a:b], want_weights=True)
        st, _, ro, _ = tr.context.draw_summary(th, wts, mf[a:b], probs=levels)
        assert _same_bits(got["khat"].reshape(-1)[a:b], po[:, 0].contiguous())          # k^ and ess: those calls' bits
        assert _same_bits(got["ess"].reshape(-1)[a:b], ro[:, 0].contiguous())
        assert _same_bits(got["mean"].reshape(-1, 3)[a:b], st[..., 0].contiguous())
        th, wts = th.cpu().numpy(), wts.cpu().numpy()
        for i in range(a, b):
            if live[i]:
                pinned += R.check_sandwich(th[i - a], R.weights(wts[i - a]), quant[i], stats[i], levels, 0.95)
                cases += 9
    assert np.all(np.isnan(quant[~live])) and np.all(np.isnan(stats[~live]))
    assert np.all(np.isnan(host(got["ess"]).reshape(-1)[~live]))
    print(proto, "live voxels", int(live.sum()), "pinned quantile share", pinned / cases)
    assert pinned / cases >= 0.95                                                       # K = 225 - 256: the limit
    # the chunking does not enter, and the raw weights need no 25 draws
    whole = ft.credible_intervals(x5, m5, p5, no_samples=K, psis=True, seed=seed, voxel0=v0)
    assert all(_same_bits(whole[k], got[k]) for k in ("mean", "sd", "quantiles", "hpd", "corr_oef_dbv", "ess", "khat"))
    raw = ft.credible_intervals(x5, m5, p5, no_samples=8, psis=False, seed=seed, probs=(0.5,))
    assert "khat" not in raw and raw["quantiles"].shape == lead + (3, 1)
    assert torch.isfinite(raw["quantiles"].reshape(n, 3)[torch.as_tensor(live, device="cuda")]).all()
    with pytest.raises(ValueError):
        ft.credible_intervals(x5, m5, p5, no_samples=24, psis=True)
    with pytest.raises(ValueError):
        ft.credible_intervals(x5, m5, p5, no_samples=3, psis=False)


def test_column_0_is_the_draws_oef_in_ascending_order(ctx):
    """Equal weights on the draws of heads with a known (mu, s) for OEF: the p-quantile v of column 0 satisfies
    |Phi((logit v - mu) / s) - p| <= 6 sqrt(p (1 - p) / K), a binomial 6 sigma bound, at K = 1024 with a fixed seed."""
    K, n = 1024, 16
    mu, raw = -0.3, 0.2
    s = math.exp(math.tanh(raw) * 3.0 - 1.0)                     # transform_std, then exp: the sd of logit OEF
    q = torch.tensor([mu, raw, 0.4, -0.1, 0.3], device="cuda").repeat(n, 1)
    x = torch.ones((n, 11), device="cuda")
    sigma = torch.full((n, 11), 0.05, device="cuda")
    _, theta = ctx.log_evidence_draws(x, None, q, q, sigma, K, seed=13, voxel0=77, want_theta=True)
    levels = (0.025, 0.1, 0.5, 0.9, 0.975)
    _, quant, row_out, _ = ctx.draw_summary(theta, None, probs=levels)
    v = host(quant)[:, 0]                                        # [n, P]
    logit = np.log((v - 0.04) / 0.8) - np.log1p(-(v - 0.04) / 0.8)   # OEF = 0.04 + 0.8 sigmoid(logit)
    phi = 0.5 * (1.0 + np.vectorize(math.erf)((logit - mu) / (s * math.sqrt(2.0))))
    p = np.array(levels)
    dist = np.abs(phi - p) / np.sqrt(p * (1 - p) / K)
    print("largest distance in binomial sigmas", float(dist.max()))
    assert np.all(dist <= 6.0)
    assert np.all(np.diff(v, axis=1) > 0)


# ---- 6. save_predictions -----------------------------------------------------------------------------------------------
def test_save_predictions_writes_the_interval_maps(params, tmp_path):
    from oracle.oracle import Oracle, synth_inputs
    from qbold_vi_amd import SignalGenerationLayer, nifti
    tr = _trainer(params)
    model, ft = _fine_tuner(tr, params, 11)
    # one fresh fine tuner per call on the same encoder, so that both calls start from the same state
    ft2 = tr.build_fine_tuner(model, SignalGenerationLayer(dict(params, simulate_noise='False'), True, True))
    B, X, Y, Z = 2, 5, 4, 3
    x, _ = synth_inputs(B * X * Y * Z, params, seed=12, oracle=Oracle("f32", params))
    mask = (np.random.default_rng(1).uniform(size=(B * X * Y * Z, 1)) > 0.2).astype(np.float32)
    data = dev(np.concatenate([x, mask], -1)).reshape(B, X, Y, Z, 12)
    priors = model(data[..., :-1])[0]
    d0, d1 = tmp_path / "plain", tmp_path / "ci"
    os.makedirs(d0)
    os.makedirs(d1)
    m0 = tr.save_predictions(model, data, str(d0 / "sub"), fine_tuner_model=ft, priors=priors, interval_samples=None)
    m1 = tr.save_predictions(model, data, str(d1 / "sub"), fine_tuner_model=ft2, priors=priors, interval_samples=64)
    new = [f"{v}_is_{k}" for v in ("oef", "dbv", "r2p") for k in ("lo", "hi", "sd")] + ["oefdbv_is_corr"]
    extra = {f"sub_{k}.nii.gz" for k in new}
    assert len(extra) == 10 and m0 is None and set(m1) == set(new)
    assert set(os.listdir(d1)) == set(os.listdir(d0)) | extra and not (set(os.listdir(d0)) & extra)
    for f in os.listdir(d0):              # the parent's files: the same bytes (inside the gzip, whose header is dated)
        assert gzip.open(d0 / f, "rb").read() == gzip.open(d1 / f, "rb").read(), f
    live = mask.reshape(B, X, Y, Z) > 0
    for k in new:
        v = m1[k].cpu().numpy()
        assert v.shape == (B, X, Y, Z, 1) and np.all(np.isfinite(v[..., 0][live]))
        np.testing.assert_array_equal(nifti.load(str(d1 / f"sub_{k}.nii.gz"))[0],
                                      np.concatenate(np.split(v, B, axis=0), axis=-1)[0])
        assert np.all(v[..., 0][~live] == 0.0)
    for v in ("oef", "dbv", "r2p"):
        lo, hi = (m1[f"{v}_is_{k}"].cpu().numpy()[..., 0][live] for k in ("lo", "hi"))
        assert np.all(lo <= hi) and np.all(m1[f"{v}_is_sd"].cpu().numpy()[..., 0][live] >= 0.0)
    assert np.all(np.abs(m1["oefdbv_is_corr"].cpu().numpy()) <= 1.0 + 1e-5)
    with pytest.raises(ValueError):
        tr.save_predictions(model, data, str(d1 / "bad"), interval_samples=64)
