"""Posterior calibration against a known truth (qbold_calibration, Context.calibration, calibration.summarise,
FineTuner.calibration, EncoderTrainer.calibration, scripts/calibrate.py): the six columns against the float64
restatement of tests/_calibration_reference.py, the Philox path against explicit normals and against the rows of
qbold_log_evidence_draws, bitwise structure, weights, the mask, the argument checks, the known answer (calibrated and
over-confident posteriors) and the Python surface."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _calibration_reference as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IW_STREAM = 6
# Largest |column - float64 column| over the voxels of tests 1 and 4 (columns 0 - 2) and, beyond the near-weight
# allowance, over the voxels of test 4 (weighted rank fractions), measured on the MI355X (MEASUREMENTS.md section 26);
# the tests hold both to min(4 x measured, 1e-4).  None would mean not measured yet: the cap alone.
CLOSED_MEASURED = 1.12e-5       # hpd at L = 64 of the weighted inputs (1.04e-5 at L = 1000 of test 1); PIT: 3.2e-6
WEIGHTED_MEASURED = 3.48e-7     # at L = 1000
CAP = 1e-4


def _bound(measured):
    return CAP if measured is None else min(4.0 * measured, CAP)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _same_bits(a, b):
    """bitwise equality (NaN included)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def ctx(params):
    from qbold_vi_amd.ops import Context
    return Context(params, full_model=True, include_blood=True)


# ---- 1. against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", R.L_CASES)
def test_columns_match_float64_reference(ctx, L):
    th, q, z, _, ref, near = R.comparison_case(L)
    out = ctx.calibration(dev(th), dev(q), L=L, z=dev(z)).cpu().numpy().astype(np.float64)
    assert out.shape == (R.N_CASE, 6) and np.isfinite(out).all()
    closed = np.abs(out[:, :3] - ref[:, :3]).max(0)
    steps = np.abs(2 * L * (out[:, 3:] - ref[:, 3:]))          # in half-draws: exact wherever near = 0
    print(f"L={L}: max |pit_oef, pit_dbv, hpd - ref| = {closed}, rank differences (half-draws) max {steps.max(0)}, "
          f"voxels with a near draw {(near > 0).sum(0)}, differing {(steps > 0).sum(0)}")
    assert np.all(steps <= 2 * near + 1e-3), np.argwhere(steps > 2 * near + 1e-3)[:10]   # 1e-3: float32's 2 L out
    assert closed.max() <= _bound(CLOSED_MEASURED), closed


# ---- 2. the Philox path ------------------------------------------------------------------------------------------------
def test_philox_draws_are_those_of_normals_and_of_log_evidence_draws(ctx, params):
    from oracle.oracle import Oracle, synth_inputs
    L, seed, v0 = 70, 9, 1000003                     # 70: a short last Philox call
    th, q, _, _, _, _ = R.comparison_case(255)
    N = R.N_CASE
    thd, qd = dev(th), dev(q)
    z = ctx.normals(N, L, stream_id=IW_STREAM, seed=seed, voxel0=v0)
    got = ctx.calibration(thd, qd, L=L, seed=seed, voxel0=v0)
    assert _same_bits(got, ctx.calibration(thd, qd, L=L, z=z))
    # the draws of log_evidence_draws for the same seed: ranks recomputed from its theta rows
    x, _ = synth_inputs(N, params, seed=3, oracle=Oracle("f32", params))
    sg = torch.full((N, 11), 0.02, device="cuda")
    _, theta = ctx.log_evidence_draws(dev(x), None, qd, qd, sg, L, seed=seed, voxel0=v0, want_theta=True)
    theta = theta.cpu().numpy().astype(np.float64)
    _, near = R.calibration(th, q, z.cpu().numpy())
    t64 = th.astype(np.float64)
    dw = theta[:, 0, 2] / (theta[:, 0, 0] * theta[:, 0, 1])          # R2' = dw_coef OEF DBV
    assert np.ptp(dw) < 1e-5 * dw.mean()
    for j, (d, t) in enumerate(((theta[:, :, 0], t64[:, 0]), (theta[:, :, 1], t64[:, 1]),
                                (theta[:, :, 2], dw.mean() * t64[:, 0] * t64[:, 1]))):
        rank = (2 * (d < t[:, None]).sum(1) + (d == t[:, None]).sum(1)) / (2.0 * L)
        # OEF and DBV are float32: towards the ends of their ranges one step of them spans more of the logit than the
        # near window does (at |logit| = 10 a step of OEF is 1.6e-3 in the logit), so the comparison in (OEF, DBV) stands
        # for the comparison of the logits in the middle of the range only (|logit| < 6: a step is below 3e-5)
        inside = np.ones(N, bool) if j == 2 else np.abs(R.truth_logits(th)[j]) < 6.0
        steps = np.abs(2 * L * (got[:, 3 + j].cpu().numpy() - rank))
        assert np.all(steps[inside] <= 2 * near[inside, j] + 1e-3), (j, np.argwhere(steps > 2 * near[:, j] + 1e-3)[:10])


# ---- 3. position independence ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", (False, True))
def test_batch_position_sharding_and_determinism(ctx, weighted):
    L, seed, v0, h = 64, 3, 5000, 101
    th, q, _, lw, _, _ = R.comparison_case(L, True)
    thd, qd, lwd = dev(th), dev(q), dev(lw) if weighted else None
    full = ctx.calibration(thd, qd, L=L, log_w=lwd, seed=seed, voxel0=v0)
    assert _same_bits(full, ctx.calibration(thd, qd, L=L, log_w=lwd, seed=seed, voxel0=v0))
    tail = ctx.calibration(thd[h:], qd[h:], L=L, log_w=None if lwd is None else lwd[h:], seed=seed, voxel0=v0 + h)
    assert _same_bits(tail, full[h:])
    assert not _same_bits(ctx.calibration(thd[h:], qd[h:], L=L, log_w=None if lwd is None else lwd[h:], seed=seed,
                                          voxel0=v0)[:, 3:], full[h:, 3:])       # other draws with another key


# ---- 4. weights ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", R.L_WEIGHTED)
def test_weighted_ranks_match_float64_reference(ctx, L):
    th, q, z, lw, ref, near = R.comparison_case(L, True)
    thd, qd, zd = dev(th), dev(q), dev(z)
    out = ctx.calibration(thd, qd, L=L, log_w=dev(lw), z=zd).cpu().numpy().astype(np.float64)
    assert np.isfinite(out).all()
    excess = np.abs(out[:, 3:] - ref[:, 3:]) - near
    print(f"L={L}: weighted rank fractions beyond the near-weight allowance: max {excess.max(0)}; "
          f"closed forms {np.abs(out[:, :3] - ref[:, :3]).max(0)}")
    assert excess.max() <= _bound(WEIGHTED_MEASURED), excess.max(0)
    assert np.abs(out[:, :3] - ref[:, :3]).max() <= _bound(CLOSED_MEASURED)
    # a constant row is the unweighted call; the scalar loads of a row that is not 16-byte aligned give the same bits
    plain = ctx.calibration(thd, qd, L=L, z=zd)
    flat = ctx.calibration(thd, qd, L=L, log_w=torch.full((R.N_CASE, L), -2.5, device="cuda"), z=zd)
    assert (flat - plain).abs().max().item() <= 1e-6
    pad = torch.empty(R.N_CASE * L + 1, device="cuda")
    pad[1:] = dev(lw).reshape(-1)
    zpad = torch.empty(R.N_CASE * L * 2 + 1, device="cuda")
    zpad[1:] = zd.reshape(-1)
    shifted = ctx.calibration(thd, qd, L=L, log_w=pad[1:].view(R.N_CASE, L), z=zpad[1:].view(R.N_CASE, L, 2))
    assert pad[1:].data_ptr() % 16 == 4 and _same_bits(shifted, dev(out.astype(np.float32)))


def test_psis_weights_and_unusable_rows(ctx, params):
    from oracle.oracle import Oracle, synth_inputs
    L, seed, v0 = 64, 4, 77
    th, q, _, _, _, _ = R.comparison_case(L, True)
    N = R.N_CASE
    thd, qd = dev(th), dev(q)
    x, _ = synth_inputs(N, params, seed=3, oracle=Oracle("f32", params))
    sg = torch.full((N, 11), 0.05, device="cuda")
    lw, _ = ctx.log_evidence_draws(dev(x), None, qd, qd, sg, L, seed=seed, voxel0=v0)
    po, _, wts = ctx.psis(lw, want_weights=True)
    plain = ctx.calibration(thd, qd, L=L, seed=seed, voxel0=v0)
    got = ctx.calibration(thd, qd, L=L, log_w=wts, seed=seed, voxel0=v0)           # accepted as they are
    ok = torch.isfinite(wts).any(1) & ~torch.isnan(wts).any(1)
    assert ok.float().mean().item() > 0.9 and _same_bits(got[:, :3], plain[:, :3])
    assert torch.isfinite(got[ok]).all() and torch.isnan(got[~ok][:, 3:]).all()
    assert got[ok][:, 3:].min().item() >= 0.0 and got[ok][:, 3:].max().item() <= 1.0 + 1e-6
    ok = ok.cpu().numpy()
    # the same draws under the weights, in float64
    z = ctx.normals(N, L, stream_id=IW_STREAM, seed=seed, voxel0=v0).cpu().numpy()
    ref, near = R.calibration(th, q, z, wts.cpu().numpy())
    excess = (np.abs(got[:, 3:].cpu().numpy() - ref[:, 3:]) - near)[ok]
    print(f"psis weights: beyond the near-weight allowance max {excess.max(0)}, khat median {po[:, 0].median().item():.2f}")
    assert excess.max() <= _bound(WEIGHTED_MEASURED)
    # raw log_w works as well: the weights are normalised inside
    raw = ctx.calibration(thd, qd, L=L, log_w=lw, seed=seed, voxel0=v0)
    ref, near = R.calibration(th, q, z, lw.cpu().numpy())
    fin = np.isfinite(ref[:, 3:]).all(1)
    assert fin.mean() > 0.9 and np.isnan(raw[:, 3:].cpu().numpy()[~fin]).all()
    excess = (np.abs(raw[:, 3:].cpu().numpy() - ref[:, 3:]) - near)[fin]
    print(f"raw log_w: beyond the near-weight allowance max {excess.max(0)}, usable rows {fin.sum()} / {N}")
    assert excess.max() <= _bound(WEIGHTED_MEASURED)
    # a NaN, a +inf, no finite entry: columns 3 - 5 are NaN, columns 0 - 2 untouched, the neighbours untouched
    bad = wts.clone()
    bad[5, 17] = float("nan")
    bad[64, 0] = float("inf")
    bad[299] = float("-inf")
    res = ctx.calibration(thd, qd, L=L, log_w=bad, seed=seed, voxel0=v0)
    rows = torch.zeros(N, dtype=torch.bool, device="cuda")
    rows[[5, 64, 299]] = True
    assert torch.isnan(res[rows][:, 3:]).all() and _same_bits(res[:, :3], got[:, :3])
    assert _same_bits(res[~rows], got[~rows])


# ---- 5. the mask ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", (False, True))
def test_mask(ctx, weighted):
    L = 25
    th, q, z, lw, _, _ = R.comparison_case(L, True)
    full = ctx.calibration(dev(th), dev(q), L=L, log_w=dev(lw) if weighted else None, z=dev(z))
    mask = np.ones(R.N_CASE, np.float32)
    mask[[0, 15, 16, 63, 64, 200]] = 0.0
    mask[[7, 299]] = -1.0
    mask[[100, 101]] = np.nan
    dead = ~(mask > 0)
    thp, qp, zp, lwp = th.copy(), q.copy(), z.copy(), lw.copy()
    thp[dead], qp[dead], zp[dead], lwp[dead] = np.nan, np.nan, np.nan, np.nan
    got = ctx.calibration(dev(thp), dev(qp), dev(mask), L=L, log_w=dev(lwp) if weighted else None, z=dev(zp))
    d = dev(dead)
    assert torch.isnan(got[d]).all() and _same_bits(got[~d], full[~d])


def test_nan_heads_and_truths_propagate(ctx):
    """A comparison with a NaN is false: the columns a NaN head or truth enters are NaN, never rank 0; the others stand."""
    L = 25
    th, q, z, _, ref, _ = R.comparison_case(L)
    th, q = th[:8].copy(), q[:8].copy()
    th[0, 0] = th[1, 1] = q[2, 0] = q[3, 1] = q[4, 2] = q[5, 3] = q[6, 4] = np.nan
    want, _ = R.calibration(th, q, z[:8])
    got = ctx.calibration(dev(th), dev(q), L=L, z=dev(z[:8])).cpu().numpy()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(want[:7]).any(1).all() and np.isfinite(want[7]).all()
    assert np.isnan(want[:, 3:]).sum() == 2 + 2 + 2 + 2 + 2 + 2 + 2
    fin = np.isfinite(want)
    assert np.abs(got[fin] - want[fin]).max() <= 1.0 / L + CAP      # the bounds proper are test 1's


# ---- 6. arguments --------------------------------------------------------------------------------------------------------
def test_arguments_and_every_context(ctx, params):
    from qbold_vi_amd import _lib
    from qbold_vi_amd.ops import Context
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    th = torch.full((4, 2), 0.1, device="cuda")
    q = torch.zeros((4, 5), device="cuda")
    out = torch.empty((4, 6), device="cuda")

    def cal(c=ctx, L=8, th_=th, q_=q, out_=out, N=4):
        return c.lib.qbold_calibration(c.handle, P(th_), None, P(q_), None, None, L, 1, 0, P(out_), N, None)
    assert cal(L=0) == -1 and cal(L=_lib.QBOLD_CAL_MAX_L + 1) == -1 and cal(out_=None) == -1
    assert cal(q_=None) == -1 and cal(th_=None) == -1 and cal(N=-1) == -1
    assert cal(N=0) == _lib.QBOLD_OK and cal(N=0, q_=None, th_=None) == _lib.QBOLD_OK and cal() == _lib.QBOLD_OK
    want = ctx.calibration(th, q, L=8)
    lit = Context(params, True, True)
    lit.set_tissue_mode("literal")
    p64 = dict(params, tau_start="-0.015", tau_end="0.065", tau_step="0.00125")
    c64 = Context(p64, True, True)
    assert c64.T == 64
    for c in (lit, c64):                                   # nothing of the forward model enters
        assert cal(c) == _lib.QBOLD_OK and _same_bits(c.calibration(th, q, L=8), want)
    with pytest.raises(ValueError):
        ctx.calibration(th, q, L=8, z=torch.zeros((4, 7, 2), device="cuda"))
    with pytest.raises(ValueError):
        ctx.calibration(th, q, L=8, log_w=torch.zeros((4, 9), device="cuda"))
    with pytest.raises(_lib.QboldError):
        ctx.calibration(th, q, L=0)
    torch.cuda.synchronize()


# ---- 7. the known answer -------------------------------------------------------------------------------------------------
def test_known_answer(ctx):
    """Truths drawn from q itself: every column uniform (chi2_15 below its 0.999 quantile 37.70) and 90 % intervals
    covering 0.90 +- 0.02; the same heads with truths from twice q's spread: chi2 > 1000, marginal 90 % coverage
    0.589 +- 0.02, HPD 90 % coverage 0.438 +- 0.02 (tests/_calibration_reference.check_known_answer; the host test
    holds the float64 reference to the same condition on the same numbers)."""
    from qbold_vi_amd.calibration import summarise
    summaries = {}
    for scale, (th, q, z) in R.known_answer_inputs().items():
        out = ctx.calibration(dev(th), dev(q), L=R.KNOWN_L, z=dev(z))
        assert torch.isfinite(out).all()
        summaries[scale] = summarise(out, R.KNOWN_L, bins=R.KNOWN_BINS)
    R.check_known_answer(summaries)


# ---- 8. the Python surface -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trainer(params):
    from qbold_vi_amd import EncoderTrainer
    return EncoderTrainer(system_params=params, no_units=24, use_layer_norm=False, dropout_rate=0.0,
                          no_intermediate_layers=2, initial_im_sigma=0.05, activation_type='relu',
                          multi_image_normalisation=False, channelwise_gating=True, infer_inv_gamma=False,
                          use_population_prior=False, use_mvg=True, predict_log_data=False)


def _hist_ok(summary, n):
    from qbold_vi_amd.calibration import COLUMNS
    for name in COLUMNS:
        st = summary["stats"][name]
        assert sum(st["hist"]) == n and np.isfinite([st["chi2"], st["p_value"], *st["coverage"]]).all(), (name, st)


def test_trainer_and_fine_tuner_calibration(trainer, params):
    from qbold_vi_amd import SignalGenerationLayer
    from qbold_vi_amd.training import synthetic_voxel_dataset
    n, L = 4096, 255
    model, _ = trainer.create_encoder(gate_offset=-3.0, resid_init_std=0.05, no_ip_images=11)
    res = trainer.calibration(model, n_voxels=n, no_samples=L, seed=2)
    assert res["out"].shape == (n, 6) and res["khat"] is None and torch.isfinite(res["out"]).all()
    s = res["summary"]
    assert s["n"] == n and s["dropped"] == 0 and not s["weighted"] and "reliable" not in s
    _hist_ok(s, n)
    assert len(s["z_mean"]) == 3 and np.isfinite(s["z_mean"]).all() and np.isfinite(s["z_rms"]).all()
    first = trainer.calibration(model, n_voxels=n, no_samples=L, seed=2, use_first_op=True)
    assert not _same_bits(first["out"], res["out"])                        # stream 1's heads are other heads
    # under the fine tuner's importance weights
    ft = trainer.build_fine_tuner(model, SignalGenerationLayer(dict(params, simulate_noise='False'), True, True))
    x, mask, y = synthetic_voxel_dataset(params, dict(uniform_prop=0.0, full_model=True, use_blood=True), n, "cuda", 2)
    prior = model.predict(x, want=("out1",))[0]
    same = trainer.calibration(model, n_voxels=n, no_samples=L, seed=2, fine_tuner=ft)
    assert _same_bits(same["out"], res["out"])
    ps = trainer.calibration(model, n_voxels=n, no_samples=L, seed=2, fine_tuner=ft, prior=prior, psis=True)
    assert ps["khat"].shape == (n,) and ps["summary"]["weighted"] and "z_rms" in ps["summary"]
    kept = int(torch.isfinite(ps["out"]).all(1).sum())
    assert ps["summary"]["n"] == kept and ps["summary"]["dropped"] == n - kept and kept > n // 2
    _hist_ok(ps["summary"], kept)
    rel = ps["summary"]["reliable"]
    live = torch.isfinite(ps["out"]).all(1)
    assert rel["n"] == int((live & (ps["khat"] < ps["summary"]["khat_threshold"])).sum())
    assert _same_bits(ps["out"][:, :3], res["out"][:, :3])
    # chunks pass their own voxel0: the result does not depend on the chunking; a mask drops voxels from the count
    m = mask.clone()
    m[::5] = 0.0
    got = ft.calibration(x, y, m, prior=prior, no_samples=64, psis=True, seed=5, voxel0=7)
    chunked = ft.calibration(x, y, m, prior=prior, no_samples=64, psis=True, seed=5, voxel0=7, psis_chunk=300)
    assert _same_bits(got["out"], chunked["out"]) and _same_bits(got["khat"], chunked["khat"])
    assert got["summary"] == chunked["summary"] and torch.isnan(got["out"][::5]).all()
    assert got["summary"]["n"] + got["summary"]["dropped"] == n and got["summary"]["dropped"] >= (n + 4) // 5
    lead = (n, 1, 1, 1)                                                       # any leading shape
    shaped = ft.calibration(x.reshape(lead + (11,)), y.reshape(lead + (2,)), m.reshape(lead),
                            prior=prior.reshape(lead + (5,)), no_samples=64, psis=True, seed=5, voxel0=7)
    assert shaped["out"].shape == lead + (6,) and shaped["khat"].shape == lead
    assert _same_bits(shaped["out"].reshape(-1, 6), got["out"])
    with pytest.raises(ValueError):
        ft.calibration(x, y, m, prior=prior, no_samples=1025, psis=True)
    with pytest.raises(ValueError):
        ft.calibration(x, y, m, no_samples=62)                               # 63 possible ranks do not split into 16 bins
    torch.cuda.synchronize()


def test_calibrate_script_writes_json(trainer, tmp_path):
    model, _ = trainer.create_encoder(gate_offset=-3.0, resid_init_std=0.05, no_ip_images=11)
    weights = str(tmp_path / "w.npz")
    model.save_weights(weights)
    cfg = tmp_path / "small.yaml"
    text = open(os.path.join(ROOT, "configurations", "optimal.yaml")).read()
    assert "no_units: 60" in text
    cfg.write_text(text.replace("no_units: 60", "no_units: 24"))
    out = str(tmp_path / "cal.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "calibrate.py"), str(cfg), "--weights", weights,
                        "--voxels", "2048", "--samples", "63", "--psis", "--out", out], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "rank_r2p" in r.stdout and "khat below threshold" in r.stdout
    with open(out) as f:
        got = json.load(f)
    assert got["voxels"] == 2048 and got["samples"] == 63 and got["psis"] is True
    assert got["summary"]["n"] + got["summary"]["dropped"] == 2048 and "reliable" in got["summary"]
