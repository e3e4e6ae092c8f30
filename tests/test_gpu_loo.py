"""PSIS leave-one-out cross-validation per voxel and per tau image (qbold_loo, Context.loo, FineTuner.loo,
save_predictions(loo_samples=K)) in two stages, as the entry is built:

  1. the rows (loglik, log_ratio) against the float64 reference of tests/_loo_reference.py, and row T against
     Context.log_evidence_draws;
  2. PSIS and the closing kernel against Context.psis on the RETURNED rows: k^ bit for bit, elpd_t / lppd_t and the
     first three columns against a float64 finalise over Context.psis' weights.

k^ is NOT held end to end against the float64 rows: a 1e-4 relative perturbation of the rows, which stage 1 permits,
moves k^_t by 0.5 at K = 25 (MEASUREMENTS.md section 24); the end-to-end distances are printed as measurements.
tests/test_loo_host.py holds, without a GPU, that every row of the reference is finite for these inputs."""
import ctypes as C
import os

import numpy as np
import pytest

import _loo_reference as R
from _loo_reference import rel1

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# Largest rel_1 distance of (elpd_t, lppd_t, elpd_loo, p_loo, lppd) to the float64 finalise over the cases below, measured
# on the MI355X (MEASUREMENTS.md section 24); the test holds them to min(4 x measured, 1e-5).
STAGE2_MEASURED = 1.99e-6   # p_loo, full64 at K = 100
STAGE2_CAP = 1e-5


def stage2_bound():
    return STAGE2_CAP if STAGE2_MEASURED is None else min(4.0 * STAGE2_MEASURED, STAGE2_CAP)


def dev(a):
    return torch.as_tensor(np.array(a, order="C"), device="cuda")   # a copy: the shared inputs are read-only


def _same_bits(a, b):
    """bitwise equality (NaN included)"""
    iv = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def same_result(a, b, keys=("out", "pointwise", "log_ratio", "loglik")):
    return all(_same_bits(a[k], b[k]) for k in keys)


def seed_of(K):
    return 41 + K


_RUNS = {}


def run_case(params, case, K):
    """The inputs on the device, the context, the stream's normals, one full call and the float64 rows: once per case."""
    from qbold_vi_amd.ops import Context
    key = (case, K)
    if key not in _RUNS:
        d = R.inputs(params, case)
        c = Context(d["p"], True, True, **d["sw"])
        assert c.T == d["T"]
        t = {k: dev(d[k]) for k in ("x", "q", "prior", "sigma")}
        z = c.normals(R.N_VOX, K, stream_id=R.IW_STREAM, seed=seed_of(K), voxel0=R.VOXEL0)
        got = c.loo(t["x"], None, t["q"], t["prior"], t["sigma"], K, seed=seed_of(K), voxel0=R.VOXEL0,
                    want_pointwise=True, want_rows=True)
        with R.float64_oracle(d["p"], d["sw"]) as o64:
            ref = R.rows(o64, d["x"], d["q"], d["prior"], d["sigma"], z.cpu().numpy())
        _RUNS[key] = dict(d=d, c=c, t=t, z=z, got=got, ref=ref)
    return _RUNS[key]


def call(r, K, sl=slice(None), mask=None, x=None, z=None, voxel0=None, **kw):
    t = r["t"]
    return r["c"].loo(t["x"][sl] if x is None else x, mask, t["q"][sl], t["prior"][sl], t["sigma"][sl], K, z=z,
                      seed=seed_of(K), voxel0=R.VOXEL0 if voxel0 is None else voxel0, want_pointwise=True,
                      want_rows=True, **kw)


# ---- stage 1: the rows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,K", R.CASE_KS)
def test_rows_match_float64_reference(params, case, K):
    r = run_case(params, case, K)
    got, ref, T = r["got"], r["ref"], r["d"]["T"]
    ll = got["loglik"].cpu().numpy().astype(np.float64)
    lr = got["log_ratio"].cpu().numpy().astype(np.float64)
    assert ll.shape == (R.N_VOX, T, K) and lr.shape == (R.N_VOX, T + 1, K)
    assert np.isfinite(ref["ll"]).all() and np.isfinite(ref["log_ratio"]).all()
    t = r["t"]
    lw, _ = r["c"].log_evidence_draws(t["x"], None, t["q"], t["prior"], t["sigma"], K, seed=seed_of(K), voxel0=R.VOXEL0)
    bound = 1e-4 * (np.abs(ref["lw"])[:, None, :] + np.abs(ref["ll"]) + 1.0)
    errs = dict(loglik=rel1(ll, ref["ll"]),
                log_ratio=float(np.max(np.abs(lr[:, :T] - ref["log_ratio"][:, :T]) / bound)) * 1e-4,
                row_T=rel1(lr[:, T], lw.cpu().numpy()), row_T_f64=rel1(lr[:, T], ref["lw"]))
    print("[loo rows]", case, K, " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    assert errs["loglik"] < 1e-4, errs
    assert errs["log_ratio"] <= 1e-4, errs
    assert errs["row_T"] < 2e-4, errs
    # the rows are written as defined: rho_t = log w - ll_t in float32, exactly
    g_lr, g_ll = got["log_ratio"], got["loglik"]
    assert _same_bits(g_lr[:, :T], g_lr[:, T:T + 1] - g_ll)


# ---- stage 2: PSIS and the closing kernel ----------------------------------------------------------------------------
@pytest.mark.parametrize("case,K", R.CASE_KS)
def test_psis_and_finalise(params, case, K):
    r = run_case(params, case, K)
    got, T, N = r["got"], r["d"]["T"], R.N_VOX
    po, _, w = r["c"].psis(got["log_ratio"].reshape(N * (T + 1), K), want_weights=True)
    kh = po[:, 0].reshape(N, T + 1)
    pw, out = got["pointwise"], got["out"]
    assert _same_bits(pw[..., 1], kh[:, :T]) and _same_bits(out[:, 5], kh[:, T])      # k^: bit for bit
    khn = kh.cpu().numpy()
    assert not np.isnan(khn).any()
    worst = np.argmax(khn[:, :T], axis=1)                                             # the first maximum, +inf included
    o = out.cpu().numpy()
    assert np.array_equal(o[:, 3], khn[np.arange(N), worst]) and np.array_equal(o[:, 4], worst.astype(np.float32))
    f = R.finalise(got["loglik"].cpu().numpy(), w.reshape(N, T + 1, K).cpu().numpy(), khn)
    pwn = pw.cpu().numpy()
    errs = dict(elpd_t=rel1(pwn[..., 0], f["pointwise"][..., 0]), lppd_t=rel1(pwn[..., 2], f["pointwise"][..., 2]),
                elpd_loo=rel1(o[:, 0], f["out"][:, 0]), p_loo=rel1(o[:, 1], f["out"][:, 1]),
                lppd=rel1(o[:, 2], f["out"][:, 2]))
    print("[loo stage 2]", case, K, f"khat_t in [{khn[:, :T].min():.3f}, {khn[:, :T].max():.3f}]",
          f"khat_max > 0.7: {int((o[:, 3] > 0.7).sum())}/{N}", " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    if K <= 256 and T <= 24:   # a measurement, not a bound: the whole definition in float64 from the float64 rows
        wr, kr = R.smooth(r["ref"]["log_ratio"])
        e = R.finalise(r["ref"]["ll"], wr, kr)
        fin = np.isfinite(kr[:, :T]) & np.isfinite(khn[:, :T])
        print("[loo end to end]", case, K, f"khat_t={np.max(np.abs(khn[:, :T] - kr[:, :T])[fin]):.3e}",
              f"elpd_t={rel1(pwn[..., 0], e['pointwise'][..., 0]):.3e}", f"elpd_loo={rel1(o[:, 0], e['out'][:, 0]):.3e}",
              f"p_loo={rel1(o[:, 1], e['out'][:, 1]):.3e}")
    assert max(errs.values()) <= stage2_bound(), errs
    # the sums: the float64 sums of the rows (mask NULL = ones)
    s = got["sums"].cpu().numpy()
    want = np.array([o[:, 0].astype(np.float64).sum(), o[:, 1].astype(np.float64).sum(), float((o[:, 3] > 0.7).sum()), N])
    assert np.max(np.abs(s - want) / (np.abs(want) + 1.0)) < 1e-8, (s, want)


# ---- determinism and edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,K", [("T11", 70), ("T11", 25), ("student_t", 100), ("off22", 100)])
def test_determinism(params, case, K):
    r = run_case(params, case, K)
    full, c = r["got"], r["c"]
    assert same_result(call(r, K), full) and _same_bits(call(r, K)["sums"], full["sums"])     # run to run
    assert same_result(call(r, K, z=r["z"]), full)                         # Philox = explicit normals, bit for bit
    h = 19                                                                 # two shards by voxel0
    a = call(r, K, slice(0, h))
    b = call(r, K, slice(h, None), voxel0=R.VOXEL0 + h)
    for k in ("out", "pointwise", "log_ratio", "loglik"):
        assert _same_bits(torch.cat([a[k], b[k]]), full[k]), k
    one = call(r, K, slice(5, 6), voxel0=R.VOXEL0 + 5)                     # N = 1
    for k in ("out", "pointwise", "log_ratio", "loglik"):
        assert _same_bits(one[k], full[k][5:6]), k
    # three chunks of 16 voxels under a small workspace cap
    cap = int(c.lib.qbold_loo_workspace_bytes(c.handle, K, 16))
    assert int(c.lib.qbold_loo_workspace_bytes(c.handle, K, 17)) > cap
    ch = call(r, K, max_workspace_bytes=cap)
    assert same_result(ch, full)
    s, sc = full["sums"].cpu().numpy(), ch["sums"].cpu().numpy()
    assert np.max(np.abs(s - sc) / (np.abs(s) + 1.0)) < 1e-14              # three float64 partial sums, another order
    # without the optional outputs: the same out
    t = r["t"]
    plain = c.loo(t["x"], None, t["q"], t["prior"], t["sigma"], K, seed=seed_of(K), voxel0=R.VOXEL0)
    assert plain["pointwise"] is None and plain["log_ratio"] is None and plain["loglik"] is None
    assert _same_bits(plain["out"], full["out"]) and _same_bits(plain["sums"], full["sums"])


@pytest.mark.parametrize("case,K", [("T11", 70), ("log_data", 100), ("left12", 100)])
def test_mask(params, case, K):
    """A quarter of the voxels masked, with NaN data there: NaN outputs and rows, the live voxels' bits unchanged, the
    sums = the float64 sums of the rows."""
    from test_gpu_forward_protocols import make_mask
    r = run_case(params, case, K)
    full = r["got"]
    mask = make_mask(R.N_VOX)
    dead = mask == 0
    assert 4 <= dead.sum() <= 20
    x = np.array(r["d"]["x"])
    x[dead] = np.nan
    got = call(r, K, mask=dev(mask), x=dev(x))
    dd = torch.as_tensor(dead, device="cuda")
    for k in ("out", "pointwise", "log_ratio", "loglik"):
        assert torch.isnan(got[k][dd]).all(), k
        assert _same_bits(got[k][~dd], full[k][~dd]), k
    o = got["out"].cpu().numpy().astype(np.float64)[~dead]
    m = mask.astype(np.float64)[~dead]
    want = np.array([(m * o[:, 0]).sum(), (m * o[:, 1]).sum(), (m * (o[:, 3] > 0.7)).sum(), m.sum()])
    s = got["sums"].cpu().numpy()
    assert np.all(np.isfinite(s)) and np.max(np.abs(s - want) / (np.abs(want) + 1.0)) < 1e-8, (s, want)


def test_empty_batch_and_bad_arguments(params):
    from qbold_vi_amd import _lib
    from qbold_vi_amd.ops import Context
    from test_gpu_psis import _p33
    K, n = 32, 4
    c = Context(params, True, True)
    e = lambda *s: torch.empty(s, device="cuda")   # noqa: E731
    res = c.loo(e(0, 11), None, e(0, 5), e(0, 5), e(0, 11), K)
    assert res["out"].shape == (0, 6) and res["sums"].cpu().tolist() == [0.0, 0.0, 0.0, 0.0]

    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    x = torch.ones((n, 11), device="cuda")
    q = torch.zeros((n, 5), device="cuda")
    out = e(n, 6)
    sums = torch.empty(4, dtype=torch.float64, device="cuda")
    ws = torch.empty(int(c.lib.qbold_loo_workspace_bytes(c.handle, 1024, n)), dtype=torch.uint8, device="cuda")
    good = dict(x=x, q=q, prior=q, sigma=x, out=out, sums=sums, ws=ws)

    def loo(ctx=c, K_=K, N=n, **kw):
        a = dict(good, **kw)
        return ctx.lib.qbold_loo(ctx.handle, P(a["x"]), None, P(a["q"]), P(a["prior"]), P(a["sigma"]), None, K_, 1, 0,
                                 P(a["out"]), None, None, None, P(a["sums"]), P(a["ws"]), N, None)
    assert loo() == _lib.QBOLD_OK and loo(K_=25) == _lib.QBOLD_OK and loo(K_=1024) == _lib.QBOLD_OK
    assert loo(K_=24) == -1 and loo(K_=1025) == -1 and loo(N=-1) == -1
    for k in good:
        assert loo(**{k: None}) == -1, k
    # N = 0: the inputs may be NULL, the sums are zeroed
    sums.fill_(7.0)
    assert loo(N=0, x=None, q=None, prior=None, sigma=None) == _lib.QBOLD_OK
    assert sums.cpu().tolist() == [0.0, 0.0, 0.0, 0.0]
    wb = c.lib.qbold_loo_workspace_bytes
    assert wb(c.handle, 24, 4) == -1 and wb(c.handle, 1025, 4) == -1 and wb(c.handle, 32, -1) == -1
    assert wb(None, 32, 4) == -1 and 0 < wb(c.handle, 32, 0) < wb(c.handle, 32, 4)
    per_voxel = 4 * 32 * (3 * 11 + 2) + 16 * 12                          # the header's bytes per voxel
    assert 0 <= wb(c.handle, 32, 1000) - wb(c.handle, 32, 0) - 1000 * per_voxel <= 4 * 256
    lit = Context(params, True, True)
    lit.set_tissue_mode("literal")
    assert loo(lit) == -3
    st33 = Context(_p33(params), True, True, student_t_df=5.0)          # a generic tau count off the fast path
    x33 = torch.ones((n, 33), device="cuda")
    assert loo(st33, x=x33, sigma=x33) == -3
    with pytest.raises(ValueError):
        c.loo(x, None, q, q, x, 24)
    torch.cuda.synchronize()


# ---- the surface -----------------------------------------------------------------------------------------------------
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


def test_fine_tuner_loo(trainer, params):
    from oracle.oracle import Oracle, synth_inputs
    o32 = Oracle("f32", params)
    model, ft = _fine_tuner(trainer, params)
    K = 32
    for shape, seed in (((70, 1, 1, 1), 3), ((2, 6, 5, 4), 8)):
        n = int(np.prod(shape))
        x, _ = synth_inputs(n, params, seed=seed, oracle=o32)
        x5 = dev(x).reshape(shape + (11,))
        m5 = dev((np.random.default_rng(seed + 1).uniform(size=n) > 0.3).astype(np.float32)).reshape(shape + (1,))
        p5 = model(x5)[0]
        got = ft.loo(x5, m5, p5, no_samples=K, seed=5, voxel0=7, want_pointwise=True)
        q, sg = ft._heads_and_sigma(x5)
        ref = trainer._ctx.loo(x5.reshape(n, 11), m5.reshape(n), q, p5.reshape(n, -1)[:, :5].contiguous(), sg, K,
                               seed=5, voxel0=7, want_pointwise=True)
        for i, k in enumerate(trainer._ctx.LOO_COLUMNS):
            assert got[k].shape == shape and _same_bits(got[k].reshape(n), ref["out"][:, i]), k
        for i, k in enumerate(("elpd_t", "khat_t", "lppd_t")):
            assert got[k].shape == shape + (11,) and _same_bits(got[k].reshape(n, 11), ref["pointwise"][..., i]), k
        assert _same_bits(got["sums"], ref["sums"])
        s = got["sums"].cpu().numpy()
        assert float(got["mean_elpd_loo"]) == s[0] / s[3] and float(got["mean_p_loo"]) == s[1] / s[3]
        live = m5[..., 0] > 0
        assert torch.isnan(got["elpd_loo"][~live]).all() and not torch.isnan(got["khat_max"][live]).any()
        other = ft.loo(x5, m5, p5, q=q.reshape(shape + (5,)) + 0.05, no_samples=K, seed=5, voxel0=7)
        assert not _same_bits(other["elpd_loo"], got["elpd_loo"])          # q: the heads evaluated instead
    with pytest.raises(ValueError):
        ft.loo(x5, m5, p5, no_samples=24)


def test_fine_tuner_loo_refuses_the_diagonal_family(params):
    from qbold_vi_amd import EncoderTrainer, SignalGenerationLayer
    tr = EncoderTrainer(system_params=params, no_units=60, use_layer_norm=False, dropout_rate=0.0,
                        no_intermediate_layers=2, initial_im_sigma=0.05, activation_type='relu',
                        multi_image_normalisation=False, channelwise_gating=True, infer_inv_gamma=False,
                        use_population_prior=False, use_mvg=False, predict_log_data=False)
    model, _ = tr.create_encoder(gate_offset=-3.0, resid_init_std=0.05, no_ip_images=11)
    ft = tr.build_fine_tuner(model, SignalGenerationLayer(dict(params, simulate_noise='False'), True, True))
    x5 = torch.ones((8, 1, 1, 1, 11), device="cuda")
    with pytest.raises(NotImplementedError, match="diagonal family"):
        ft.loo(x5, None, model(x5)[0], no_samples=32)


def test_save_predictions_writes_the_loo_maps(trainer, params, tmp_path):
    from oracle.oracle import Oracle, synth_inputs
    from qbold_vi_amd import SignalGenerationLayer, nifti
    model, ft = _fine_tuner(trainer, params)
    # one fresh fine tuner per call on the same encoder: a fine tuner counts its sampled predictions
    ft2 = trainer.build_fine_tuner(model, SignalGenerationLayer(dict(params, simulate_noise='False'), True, True))
    B, X, Y, Z = 2, 6, 5, 4
    x, _ = synth_inputs(B * X * Y * Z, params, seed=12, oracle=Oracle("f32", params))
    mask = (np.random.default_rng(1).uniform(size=(B * X * Y * Z, 1)) > 0.2).astype(np.float32)
    data = dev(np.concatenate([x, mask], -1)).reshape(B, X, Y, Z, 12)
    priors = model(data[..., :-1])[0]
    d0, d1 = tmp_path / "plain", tmp_path / "loo"
    os.makedirs(d0)
    os.makedirs(d1)
    m0 = trainer.save_predictions(model, data, str(d0 / "sub"), fine_tuner_model=ft, priors=priors)
    m1 = trainer.save_predictions(model, data, str(d1 / "sub"), fine_tuner_model=ft2, priors=priors, loo_samples=64)
    new = ("elpdloo", "ploo", "khatloo", "worsttau")
    extra = {f"sub_{k}.nii.gz" for k in new}
    assert set(os.listdir(d1)) == set(os.listdir(d0)) | extra and not (set(os.listdir(d0)) & extra)
    assert m0 is None and set(m1) == set(new)
    live = mask.reshape(B, X, Y, Z) > 0
    for k in new:
        v = m1[k].cpu().numpy()
        assert v.shape == (B, X, Y, Z, 1)
        assert np.all(np.isnan(v[..., 0][~live])) and not np.isnan(v[..., 0][live]).any(), k
        np.testing.assert_array_equal(nifti.load(str(d1 / f"sub_{k}.nii.gz"))[0],
                                      np.concatenate(np.split(v, B, axis=0), axis=-1)[0])
    wt = m1["worsttau"].cpu().numpy()[..., 0][live]
    assert np.all(wt == np.round(wt)) and wt.min() >= 0 and wt.max() <= 10
