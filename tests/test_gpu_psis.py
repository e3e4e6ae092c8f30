"""Pareto-smoothed importance sampling per voxel (qbold_psis, qbold_log_evidence_draws, Context.psis,
Context.log_evidence_draws, FineTuner.log_evidence(psis=True), save_predictions(psis=True)): the Pareto fit on plain
rows against the float64 restatement of tests/_psis_reference.py, edge rows, bitwise structure, the per-draw rows
against tests/_iw_reference.log_weights, and the Python surface."""
import ctypes as C
import gzip
import math
import os

import numpy as np
import pytest

import _psis_reference as R
from _iw_reference import log_weights, rel, rel1

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

IW_STREAM = 6
KS = (25, 64, 100, 225, 1000, 1024)
# Largest |k^ - float64 k^| and |log w~ - float64 log w~| over the 6 x 240 rows below, measured on the MI355X
# (MEASUREMENTS.md section 18); the test holds both to min(4 x measured, 1e-3).
KHAT_MEASURED = 1.65e-5     # at K = 1000
LOGW_MEASURED = 8.38e-5     # at K = 1024
CAP = 1e-3


def _bound(measured):
    return CAP if measured is None else min(4.0 * measured, CAP)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _same_bits(a, b):
    """bitwise equality (NaN included)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _bits(t):
    return t.reshape(-1).view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@pytest.fixture(scope="module")
def ctx(params):
    from qbold_vi_amd.ops import Context
    return Context(params, full_model=True, include_blood=True)


_ROWS = {}


def rows_and_reference(K):
    """(rows float32 [240, K], theta float32 [240, K, 3], float64 reference), computed once per K."""
    if K not in _ROWS:
        lw = R.make_rows(K)
        theta = np.random.default_rng([11, K]).uniform(0.5, 1.5, (lw.shape[0], K, 3)).astype(np.float32)
        _ROWS[K] = (lw, theta, R.psis(lw, theta))
    return _ROWS[K]


# ---- 1. rows against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_rows_match_float64_reference(ctx, K):
    lw, theta, ref = rows_and_reference(K)
    assert lw.shape == (240, K) and np.all(np.isfinite(ref["out"]))          # every k^ finite: no row left out
    assert np.max(-ref["c"]) < 40.0                                           # far from the -c > 80 rule
    out, means, weights = ctx.psis(dev(lw), dev(theta), want_weights=True)
    out, means, weights = (t.cpu().numpy().astype(np.float64) for t in (out, means, weights))
    errs = dict(khat=float(np.max(np.abs(out[:, 0] - ref["out"][:, 0]))),
                logw=float(np.max(np.abs(weights - ref["weights"]))),
                log_p=rel1(out[:, 1], ref["out"][:, 1]), ess=rel(out[:, 2], ref["out"][:, 2]),
                means=rel(means, ref["means"]))
    print(f"K={K} M={R.tail_size(K)} khat in [{ref['out'][:, 0].min():.3f}, {ref['out'][:, 0].max():.3f}]", errs)
    assert np.array_equal(out[:, 3], ref["out"][:, 3])                       # the tail lengths, ties included
    assert errs["khat"] <= _bound(KHAT_MEASURED) and errs["logw"] <= _bound(LOGW_MEASURED), (K, errs)
    assert errs["log_p"] < 1e-4 and errs["ess"] < 1e-4 and errs["means"] < 1e-4, (K, errs)
    # the weights are normalised
    assert np.max(np.abs(np.exp(weights).sum(1) - 1.0)) < 1e-5


# ---- 2. edge rows ----------------------------------------------------------------------------------------------------
def test_edge_rows(ctx):
    K = 64
    M = R.tail_size(K)
    rng = np.random.default_rng(2)
    base = R.make_rows(K)[::40][:6].copy()
    rows = {}
    rows["nan"] = base[0].copy()
    rows["nan"][17] = np.nan
    rows["equal"] = np.full(K, -3.5, np.float32)
    top = np.linspace(-9.0, -5.0, K).astype(np.float32)
    top[rng.permutation(K)[:M + 1]] = -1.0
    rows["top_equal"] = top
    minf = base[1].copy()
    minf[[3, 40, 63]] = -np.inf
    rows["minus_inf"] = minf
    far = (rng.standard_normal(K) - 200.0).astype(np.float32)
    far[:8] = np.array([0.0, -0.5, -1.0, -2.0, -3.0, -4.0, -5.0, -6.0], np.float32)   # cutoff near -200: -c > 80
    rows["far_cutoff"] = far
    rows["masked"] = np.full(K, np.nan, np.float32)       # poisoned: must not be read
    rows["plain"] = base[2]
    names = list(rows)
    lw = np.stack([rows[k] for k in names])
    theta = rng.uniform(0.5, 1.5, (len(names), K, 2)).astype(np.float32)
    theta[names.index("masked")] = np.nan
    mask = np.ones(len(names), np.float32)
    mask[names.index("masked")] = 0.0
    out, means, weights = ctx.psis(dev(lw), dev(theta), dev(mask), want_weights=True)
    out, means, weights = (t.cpu().numpy().astype(np.float64) for t in (out, means, weights))
    got = {k: (out[i], means[i], weights[i]) for i, k in enumerate(names)}

    for k in ("nan", "masked"):
        o, m, w = got[k]
        assert np.all(np.isnan(o)) and np.all(np.isnan(m)) and np.all(np.isnan(w)), k

    o, m, w = got["equal"]
    assert o[0] == np.inf and o[3] == 0 and abs(o[1] + 3.5) < 1e-5 and abs(o[2] - K) < 1e-3 * K
    assert np.max(np.abs(w + math.log(K))) < 1e-5
    assert np.max(np.abs(m - theta[names.index("equal")].astype(np.float64).mean(0))) < 1e-5

    o, m, w = got["top_equal"]
    assert o[0] == np.inf and o[3] == 0

    def raw_normalised(row):
        x = row.astype(np.float64)
        mx = x.max()
        return x - (mx + math.log(np.exp(x - mx).sum()))

    o, m, w = got["far_cutoff"]
    ref = R.psis_row(far, theta[names.index("far_cutoff")])
    assert ref["khat"] == np.inf and -ref["c"] > 80 and ref["n"] > 4
    assert o[0] == np.inf and o[3] == ref["n"]
    assert np.max(np.abs(w - raw_normalised(far))) < 1e-5                      # unsmoothed, normalised
    assert abs(o[1] - ref["log_p"]) < 1e-4 * (1 + abs(ref["log_p"])) and abs(o[2] - ref["ess"]) < 1e-4 * ref["ess"]

    for k in ("minus_inf", "plain"):
        o, m, w = got[k]
        ref = R.psis_row(rows[k], theta[names.index(k)])
        assert np.isfinite(ref["khat"]) and o[3] == ref["n"], k
        assert abs(o[0] - ref["khat"]) <= CAP, (k, o[0], ref["khat"])
        fin = np.isfinite(ref["weights"])
        assert np.array_equal(np.isneginf(w), ~fin) and np.max(np.abs(w[fin] - ref["weights"][fin])) <= CAP, k
        assert abs(o[1] - ref["log_p"]) < 1e-4 * (1 + abs(ref["log_p"])) and abs(o[2] - ref["ess"]) < 1e-4 * ref["ess"]
        assert np.max(np.abs(m - ref["means"]) / np.abs(ref["means"])) < 1e-4, k
    assert (~np.isfinite(got["minus_inf"][2])).sum() == 3


# ---- 3. structure --------------------------------------------------------------------------------------------------
def test_batch_position_determinism_and_theta(ctx):
    K = 100
    lw, theta, _ = rows_and_reference(K)
    lw203 = np.concatenate([lw[:203 - 3], lw[:3]])[:203]
    th203 = np.concatenate([theta[:203 - 3], theta[:3]])[:203]
    mask = (np.random.default_rng(5).uniform(size=203) > 0.1).astype(np.float32)
    mask[[0, 4, 202]] = 1.0
    L, TH, MK = dev(lw203), dev(th203), dev(mask)
    full = ctx.psis(L, TH, MK, want_weights=True)
    again = ctx.psis(L, TH, MK, want_weights=True)
    assert all(_same_bits(a, b) for a, b in zip(full, again))
    assert torch.isfinite(full[0][MK > 0][:, 1:]).all()
    for a, b in ((0, 1), (0, 5), (4, 5), (7, 203), (198, 203), (202, 203)):     # N = 1, 5 and slices of 203
        part = ctx.psis(L[a:b], TH[a:b], MK[a:b], want_weights=True)
        assert all(_same_bits(p, f[a:b]) for p, f in zip(part, full)), (a, b)
    # theta NULL and theta of another width: the same out and weights
    o0, m0, w0 = ctx.psis(L, None, MK, want_weights=True)
    assert m0 is None and _same_bits(o0, full[0]) and _same_bits(w0, full[2])
    th8 = torch.cat([TH, TH * 2.0, TH[..., :2] + 1.0], -1).contiguous()
    o8, m8, _ = ctx.psis(L, th8, MK)
    assert m8.shape == (203, 8) and _same_bits(o8, full[0]) and _same_bits(m8[:, :3].contiguous(), full[1])
    live = torch.as_tensor(mask > 0, device="cuda")
    assert torch.allclose(m8[live][:, 3:6], 2.0 * full[1][live], rtol=1e-6, atol=0)


# ---- 4. the per-draw rows ------------------------------------------------------------------------------------------
def _p24(params):
    return dict(params, tau_start="-0.028", tau_end="0.065", tau_step="0.004")


def _p33(params):
    return dict(params, tau_start="-0.010", tau_end=str(-0.010 + 0.001 * 33 - 0.0005), tau_step="0.001")


DRAW_CASES = {
    "table_T11": (None, {}),
    "protocol_T24": (_p24, {}),
    "generic_T33": (_p33, {}),
    "student_t": (None, dict(student_t_df=5.0)),
    "three_image_norm": (None, dict(multi_image_normalisation=True)),
}


def _heads(o32, p, T, n, seed):
    from oracle.oracle import init_weights, synth_inputs
    x, _ = synth_inputs(n, p, seed=seed, oracle=o32)
    w = init_weights(T=T, U=60, L=2, seed=3)
    w["gate_offset"] = -3.0
    prior, q, sigma = o32.encoder_fwd(w, x)
    return x, q, prior, sigma


@pytest.mark.parametrize("case", list(DRAW_CASES))
def test_draws_match_float64_reference(params, case):
    from oracle.oracle import Oracle
    from qbold_vi_amd.ops import Context
    from _iw_reference import dw_coef
    proto, sw = DRAW_CASES[case]
    p = proto(params) if proto else params
    o32 = Oracle("f32", p, **sw)
    n = 48
    x, q, prior, sigma = _heads(o32, p, o32.T, n, 11)
    c = Context(p, True, True, **sw)
    assert c.T == {"protocol_T24": 24, "generic_T33": 33}.get(case, 11)
    xd, qd, pd, sd = dev(x), dev(q), dev(prior), dev(sigma)
    o64 = Oracle("f64", p, node0_zero=True, **sw)   # node 0 of the Simpson sum rounds to 0 in float32 (the table's F)
    try:
        for K in (25, 70):                            # 70: a short last Philox call; 25: rows not 16-byte aligned
            seed, v0 = 41 + K, 1000003
            z = c.normals(n, K, stream_id=IW_STREAM, seed=seed, voxel0=v0)
            lw_ref, y = log_weights(o64, x, q, prior, sigma, z.cpu().numpy())
            lw, th = c.log_evidence_draws(xd, None, qd, pd, sd, K, seed=seed, voxel0=v0, want_theta=True)
            lw2, th2 = c.log_evidence_draws(xd, None, qd, pd, sd, K, z=z, want_theta=True)
            assert _same_bits(lw, lw2) and _same_bits(th, th2)              # Philox = explicit normals, bit for bit
            only, none = c.log_evidence_draws(xd, None, qd, pd, sd, K, seed=seed, voxel0=v0)
            assert none is None and _same_bits(only, lw)
            th_ref = np.stack([y[..., 0], y[..., 1], dw_coef(p) * y[..., 0] * y[..., 1]], -1)
            errs = dict(lw=rel1(lw.cpu().numpy(), lw_ref), theta=rel(th.cpu().numpy(), th_ref))
            print(case, K, errs)
            assert errs["lw"] < 1e-4 and errs["theta"] < 1e-4, (case, K, errs)
            # the rows are what log_evidence reduces
            _, out, _ = c.log_evidence(xd, None, qd, pd, sd, K, seed=seed, voxel0=v0)
            lse = torch.logsumexp(lw.double(), 1) - math.log(K)
            assert rel1(lse.cpu().numpy(), out[:, 0].cpu().numpy()) < 1e-4
            # sharding by voxel0, and a mask: rows outside it are NaN and their data is not read
            h = 19
            a, ta = c.log_evidence_draws(xd[:h], None, qd[:h], pd[:h], sd[:h], K, seed=seed, voxel0=v0, want_theta=True)
            b, tb = c.log_evidence_draws(xd[h:], None, qd[h:], pd[h:], sd[h:], K, seed=seed, voxel0=v0 + h,
                                         want_theta=True)
            assert _same_bits(torch.cat([a, b]), lw) and _same_bits(torch.cat([ta, tb]), th)
            mask = np.ones(n, np.float32)
            mask[[0, 5, 17, 47]] = 0.0
            xm = x.copy()
            xm[mask == 0] = np.nan
            lm, tm = c.log_evidence_draws(dev(xm), dev(mask), qd, pd, sd, K, seed=seed, voxel0=v0, want_theta=True)
            dead = torch.as_tensor(mask == 0, device="cuda")
            assert torch.isnan(lm[dead]).all() and torch.isnan(tm[dead]).all()
            assert _same_bits(lm[~dead], lw[~dead]) and _same_bits(tm[~dead], th[~dead])
    finally:
        o64.lib.qbo_set_node0_zero(0)


# ---- 5. the surface ------------------------------------------------------------------------------------------------
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


PSIS_KEYS = ("khat", "log_evidence_psis", "ess_psis", "psis_means", "khat_threshold")


def test_fine_tuner_log_evidence_psis(trainer, params):
    from oracle.oracle import Oracle, synth_inputs
    from qbold_vi_amd.ops import psis_khat_threshold
    o32 = Oracle("f32", params)
    model, ft = _fine_tuner(trainer, params)
    K = 32
    for shape, seed in (((1000, 1, 1, 1), 3), ((2, 19, 13, 4), 8)):
        n = int(np.prod(shape))
        x, _ = synth_inputs(n, params, seed=seed, oracle=o32)
        x5 = dev(x).reshape(shape + (11,))
        m5 = dev((np.random.default_rng(seed + 1).uniform(size=n) > 0.3).astype(np.float32)).reshape(shape + (1,))
        p5 = model(x5)[0]
        plain = ft.log_evidence(x5, m5, p5, no_samples=K, seed=5, voxel0=7, want_means=True)
        assert not (set(PSIS_KEYS) & set(plain))
        got = ft.log_evidence(x5, m5, p5, no_samples=K, seed=5, voxel0=7, want_means=True, psis=True)
        assert set(got) == set(plain) | set(PSIS_KEYS)
        for k, v in plain.items():                                   # the earlier keys: the same bits
            if torch.is_tensor(v):
                assert v.dtype == got[k].dtype and torch.equal(_bits(v), _bits(got[k])), k
            else:
                assert float(v) == float(got[k]), k
        for k in ("khat", "log_evidence_psis", "ess_psis"):
            assert got[k].shape == shape, k
        assert got["psis_means"].shape == shape + (3,) and got["khat_threshold"] == psis_khat_threshold(K)
        live = m5[..., 0] > 0
        assert torch.isfinite(got["log_evidence_psis"][live]).all() and torch.isnan(got["khat"][~live]).all()
        assert (got["ess_psis"][live] >= 1.0 - 1e-5).all() and (got["ess_psis"][live] <= K * (1 + 1e-5)).all()
        none = live & torch.isinf(got["khat"])                       # no smoothing: the plain estimate
        if none.any():
            assert rel1(got["log_evidence_psis"][none].cpu().numpy(), got["log_evidence"][none].cpu().numpy()) < 1e-4
        print(shape, "khat quartiles", torch.quantile(got["khat"][live & torch.isfinite(got["khat"])],
                                                      torch.tensor([0.25, 0.5, 0.75], device="cuda")).tolist())
        chunked = ft.log_evidence(x5, m5, p5, no_samples=K, seed=5, voxel0=7, psis=True, psis_chunk=300)
        for k in PSIS_KEYS[:4]:
            assert _same_bits(chunked[k], got[k]), k
    with pytest.raises(ValueError):
        ft.log_evidence(x5, m5, p5, no_samples=24, psis=True)
    with pytest.raises(ValueError):
        ft.log_evidence(x5, m5, p5, no_samples=1025, psis=True)


def test_save_predictions_writes_the_psis_maps(trainer, params, tmp_path):
    from oracle.oracle import Oracle, synth_inputs
    from qbold_vi_amd import nifti
    from qbold_vi_amd import SignalGenerationLayer
    model, ft = _fine_tuner(trainer, params)
    # a fine tuner counts its sampled predictions (the `_residual` map's draw): one fresh fine tuner per call, on the
    # same encoder, so that both calls start from the same state
    ft2 = trainer.build_fine_tuner(model, SignalGenerationLayer(dict(params, simulate_noise='False'), True, True))
    B, X, Y, Z = 2, 6, 5, 4
    x, _ = synth_inputs(B * X * Y * Z, params, seed=12, oracle=Oracle("f32", params))
    mask = (np.random.default_rng(1).uniform(size=(B * X * Y * Z, 1)) > 0.2).astype(np.float32)
    data = dev(np.concatenate([x, mask], -1)).reshape(B, X, Y, Z, 12)
    priors = model(data[..., :-1])[0]
    d0, d1 = tmp_path / "iw", tmp_path / "psis"
    os.makedirs(d0)
    os.makedirs(d1)
    m0 = trainer.save_predictions(model, data, str(d0 / "sub"), fine_tuner_model=ft, priors=priors, iw_samples=64)
    m1 = trainer.save_predictions(model, data, str(d1 / "sub"), fine_tuner_model=ft2, priors=priors, iw_samples=64,
                                  psis=True)
    new = ("khat", "logevidence_psis", "ess_psis", "oef_psis", "dbv_psis", "r2p_psis")
    extra = {f"sub_{k}.nii.gz" for k in new}
    assert set(os.listdir(d1)) == set(os.listdir(d0)) | extra and not (set(os.listdir(d0)) & extra)
    for f in os.listdir(d0):              # every earlier file: the same bytes (inside the gzip, whose header is dated)
        assert gzip.open(d0 / f, "rb").read() == gzip.open(d1 / f, "rb").read(), f
    assert set(m1) == set(m0) | set(new)
    live = mask.reshape(B, X, Y, Z) > 0
    for k in new:
        v = m1[k].cpu().numpy()
        assert v.shape == (B, X, Y, Z, 1) and np.all(np.isfinite(v[..., 0][live]) | (k == "khat"))
        np.testing.assert_array_equal(nifti.load(str(d1 / f"sub_{k}.nii.gz"))[0],
                                      np.concatenate(np.split(v, B, axis=0), axis=-1)[0])
        assert np.all(v[..., 0][~live] == 0.0)
    oef = m1["oef_psis"].cpu().numpy()[..., 0][live]
    assert np.all(oef > 0.04) and np.all(oef < 0.84)


def test_bad_arguments(ctx, params):
    from qbold_vi_amd import _lib
    from qbold_vi_amd.ops import Context
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    lw = torch.zeros((4, 64), device="cuda")
    th = torch.zeros((4, 64, 9), device="cuda")
    out = torch.empty((4, 4), device="cuda")
    mn = torch.empty((4, 9), device="cuda")

    def psis(K=64, lw_=lw, th_=None, Cc=0, out_=out, mn_=None):
        return ctx.lib.qbold_psis(ctx.handle, P(lw_), P(th_), Cc, None, K, P(out_), P(mn_), None, 4, None)
    assert psis(24) == -1 and psis(1025) == -1 and psis(0) == -1
    assert psis(lw_=None) == -1 and psis(out_=None) == -1
    assert psis(th_=th, Cc=9) == -1 and psis(th_=th, Cc=0) == -1 and psis(mn_=mn) == -1
    assert psis(25) == _lib.QBOLD_OK and psis(th_=th, Cc=8, mn_=mn) == _lib.QBOLD_OK
    with pytest.raises(_lib.QboldError):
        ctx.psis(torch.zeros((4, 8), device="cuda"))

    x = torch.ones((4, 11), device="cuda")
    q = torch.zeros((4, 5), device="cuda")

    def draws(c, K=8, lw_=lw, x_=x):
        return c.lib.qbold_log_evidence_draws(c.handle, P(x_), None, P(q), P(q), P(x), None, K, 1, 0, P(lw_), None, 4,
                                              None)
    assert draws(ctx, 0) == -1 and draws(ctx, (1 << 30) + 1) == -1
    assert draws(ctx, lw_=None) == -1 and draws(ctx, x_=None) == -1
    assert draws(ctx) == _lib.QBOLD_OK
    lit = Context(params, True, True)
    lit.set_tissue_mode("literal")
    assert draws(lit) == -3
    p33 = _p33(params)
    st33 = Context(p33, True, True, student_t_df=5.0)                  # a generic tau count off the fast path
    x33 = torch.ones((4, 33), device="cuda")
    assert st33.lib.qbold_log_evidence_draws(st33.handle, P(x33), None, P(q), P(q), P(x33), None, 8, 1, 0, P(lw), None,
                                             4, None) == -3
    torch.cuda.synchronize()
