"""The run-time-T forward kernels (elbo_fwd_generic_kernel, iw_fwd_generic_kernel, iw_draws_generic_kernel,
ppc_generic_kernel, grid_generic_kernel) on tau protocols other than the three the suite was written around, each
against the float64 oracle per voxel: grids with more taus before the spin echo than after it (the left tail of the
mirrored loop), with no tau equal to 0 (the plain tau loop), with T % 4 != 0 and T < 4 (unequal LDS staging), with
fewer than 64 taus (idle lanes of the one-wave-per-voxel kernels), with three-image normalisation at a run-time T, and
with more voxels than one pass of the capped grid holds (the second trip of the tile loop).

The protocol table, the inputs and the host-side class of each protocol are checked without a GPU by
tests/test_forward_protocols_host.py, which imports them from here.

Not built: a comparison of the generic kernels with the specialised ones on a protocol of 11 taus.  Every forward
entry point dispatches on the tau count alone (`switch (T) case 11:`), so any 11-tau protocol takes a T = 11 kernel
and the forward has no selection bit that would route it elsewhere."""
import contextlib
import math

import numpy as np
import pytest

import _grid_reference as gr
from _iw_reference import dw_coef, iw_reference, log_weights, rel, rel1
from _ppc_reference import ppc_reference

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

IW_STREAM, PPC_STREAM = 6, 8
QB_TAB_SEG = 256                  # qbold_dev.h
LOGIT_CLIP = 13.815509557963774   # QB_LOGIT_CLIP
Z_MAX = 4.8549                    # QB_Z_MAX
N_VOX = 300                       # 300 % 32 != 0: a ragged last tile of the 32-voxel blocks

# name: (tau_start, tau_step, T, spin-echo index, tau = 0 at the spin echo in float32, three-image normalisation)
#   left12  mirrored; t = 9..11 paired with 7..5, t = 0..4 through the left-tail loop
#   right5  mirrored with no left side; the four lanes of a voxel stage 2 / 1 / 1 / 1 rows; small odd chi^2
#   two     T < 4: two lanes of a voxel stage nothing
#   odd33   mirrored, right-heavy; 33 of 64 lanes on in the PPC kernel; large odd chi^2
#   off22   tau[se] = -1 ms: the plain tau loop
#   full64  64 taus that do not take the config-3 kernels (spin echo at index 8, not 12): QB_MAX_T rows of LDS
PROTOCOLS = {
    "left12": (-0.016, 0.002, 12, 8, True, False),
    "right5": (0.0, 0.008, 5, 0, True, False),
    "two": (0.0, 0.01, 2, 0, True, False),
    "odd33": (-0.008, 0.002, 33, 4, True, False),
    "off22": (-0.017, 0.004, 22, 4, False, False),
    "full64": (-0.008, 0.001, 64, 8, True, False),
    "odd33_3img": (-0.008, 0.002, 33, 4, True, True),
    "off22_3img": (-0.017, 0.004, 22, 4, False, True),
}
GRID_PROTOCOLS = ("left12", "odd33", "off22", "odd33_3img")
# Seed of the synthetic voxels, per protocol: the smallest one from 11 (the seed of the tests this recipe comes from) at
# which the host-side conditions hold on the 300 voxels -- no voxel over the reach bound of the whitened KL, and the
# float32 oracle within the ELBO bounds of the float64 one in every run of ELBO_RUNS.  Both are properties of the
# inputs and the two oracles alone (tests/test_forward_protocols_host.py); no kernel was consulted.
INPUT_SEEDS = {"off22": 18, "full64": 13, "off22_3img": 12}


def protocol(params, name):
    start, step, T = PROTOCOLS[name][:3]
    return dict(params, tau_start=str(start), tau_end=str(start + step * T - step / 2), tau_step=str(step))


def switches(name):
    return dict(multi_image_normalisation=True) if PROTOCOLS[name][5] else {}


def takes_mirrored_loop(params, name):
    """The kernels' `mirrored`: one-image normalisation and fmaf(se, tauh_step, tauh0) == 0 in float32, with tauh0 /
    tauh_step as qbold_ctx_create forms them (tau_start and tau_step times the float32 inverse of the table step)."""
    f32 = np.float32
    start, step, T, se, _, multi = PROTOCOLS[name]
    ts, tstep = f32(start), f32(step)
    taus = np.array([ts + f32(i) * tstep for i in range(T)], f32)
    dwc = f32((4.0 / 3.0) * math.pi * float(params["gamma"]) * float(params["b0"]) * float(params["dchi"]) *
              float(params["hct"]))
    xmax = max(float(np.max(np.abs(taus))) * abs(float(dwc)), 1e-3)
    tab_inv_h = f32(1.0 / (xmax / QB_TAB_SEG))
    tauh0, tauh_step = f32(ts * tab_inv_h), f32(tstep * tab_inv_h)
    # the float32 product is exact in float64, and a float64 sum of two such numbers is 0 only when it is 0 exactly
    return (not multi) and float(f32(se)) * float(tauh_step) + float(tauh0) == 0.0


def heads(o32, p, T, n, seed):
    """test_gpu_log_evidence.heads()"""
    from oracle.oracle import init_weights, synth_inputs
    x, _ = synth_inputs(n, p, seed=seed, oracle=o32)
    w = init_weights(T=T, U=60, L=2, seed=3)
    w["gate_offset"] = -3.0
    prior, q, sigma = o32.encoder_fwd(w, x)
    return x, q, prior, sigma


def make_mask(n):
    """a quarter of the voxels out, the others weighted 0.5 .. 1.5"""
    mask = (np.random.default_rng(4).uniform(size=n) > 0.25).astype(np.float32)
    mask[mask > 0] = np.random.default_rng(6).uniform(0.5, 1.5, int((mask > 0).sum())).astype(np.float32)
    return mask


def kl_reach(q):
    """|mu| + QB_Z_MAX (|c| + e^s): while it stays below QB_LOGIT_CLIP for every voxel, every wave takes the whitened
    form of log q - log p, so a voxel's bits do not depend on the voxels that share its wave."""
    q = q.astype(np.float64)
    e_so, e_sd = np.exp(3.0 * np.tanh(q[:, 1]) - 1.0), np.exp(3.0 * np.tanh(q[:, 3]) - 1.0)
    c = np.tanh(q[:, 4]) * np.exp(-2.0)
    return np.maximum(np.abs(q[:, 0]) + Z_MAX * e_so, np.abs(q[:, 2]) + Z_MAX * (np.abs(c) + e_sd))


_INPUTS = {}


def inputs(params, name, n=N_VOX, seed=None):
    """dict(p, sw, x, q, prior, sigma, mask, live), computed once per (protocol, n) and never written to."""
    from oracle.oracle import Oracle
    seed = INPUT_SEEDS.get(name, 11) if seed is None else seed
    key = (name, n, seed)
    if key not in _INPUTS:
        p, sw = protocol(params, name), switches(name)
        o32 = Oracle("f32", p, **sw)
        x, q, prior, sigma = heads(o32, p, o32.T, n, seed)
        mask = make_mask(n)
        d = dict(p=p, sw=sw, x=x, q=q, prior=prior, sigma=sigma, mask=mask, live=mask > 0)
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _INPUTS[key] = d
    return _INPUTS[key]


@contextlib.contextmanager
def float64_oracle(p, sw):
    """node 0 of the Simpson sum rounds to 0 in float32 (the table's F); the flag is process-global in the C library"""
    from oracle.oracle import Oracle
    o64 = Oracle("f64", p, node0_zero=True, **sw)
    try:
        yield o64
    finally:
        o64.lib.qbo_set_node0_zero(0)


def elbo_reference(o, d, zs, zk, sl=slice(None)):
    """Oracle.elbo with K = 0 allowed (no KL draws: kl = 0, as the kernels and qbo_elbo have it)."""
    zs = np.asarray(zs)
    n, K = zs.shape[0], zk.shape[1]
    e = o.elbo(d["x"][sl], d["mask"][sl], d["q"][sl], d["prior"][sl], d["sigma"][sl], zs,
               zk if K else np.zeros((n, 1, 2), np.float32))
    if K == 0:
        kl_v = np.zeros_like(e["kl_v"])
        e = dict(e, kl_v=kl_v, kl=0.0, elbo=e["nll"])
    return e


def dev(a):
    return torch.as_tensor(np.array(a, order="C"), device="cuda")   # a copy: the shared inputs are read-only


def _same_bits(a, b):
    """bitwise equality (NaN included)"""
    iv = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def poisoned(d):
    """the data with NaN in the masked voxels: they must stay out of every sum and every other voxel's row"""
    x = d["x"].copy()
    x[~d["live"]] = np.nan
    return x


def context(d):
    from qbold_vi_amd.ops import Context
    return Context(d["p"], True, True, **d["sw"])


# The cases over the project's 1e-4 on the MI355X, each below the float32 oracle's own distance to the float64
# reference on the same inputs (tests/test_forward_protocols_host.py prints it): float32 accumulation of 33 / 64
# residuals of size 1 / sigma ~ 20, in voxels and draws whose 0.5 sum r^2 all but cancels T log sigma, so that rel_1
# is an absolute error of a sum of ~100.  Bound = 3 x the measured value (the convention of test_gpu_posterior_
# predictive.TOL); MEASUREMENTS.md section 19 has the table.  (case, column): (measured, float32 oracle)
ACCUMULATION_NOISE = {
    ("log_evidence full64 explicit K=64", "log_p"): (1.289e-4, 1.862e-4),
    ("log_evidence_draws odd33 K=27", "lw"): (1.058e-4, 1.330e-4),
    ("log_evidence_draws full64 K=27", "lw"): (1.591e-4, 3.498e-4),
    ("log_evidence_draws odd33_3img K=27", "lw"): (1.091e-4, 4.185e-4),
}


def _report(fails, what, errs, tols):
    """print every figure, collect the ones over their bound"""
    print("[forward protocols]", what, " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    for k, v in errs.items():
        tol = 3.0 * ACCUMULATION_NOISE[what, k][0] if (what, k) in ACCUMULATION_NOISE else tols[k]
        if not v <= tol:
            fails.append((what, k, v, tol))


@pytest.mark.parametrize("name", list(PROTOCOLS))
def test_protocol_is_what_the_table_says(params, name):
    _, _, T, se, zero_at_se, multi = PROTOCOLS[name]
    d = inputs(params, name)
    c = context(d)
    assert c.T == T and c.se_idx == se
    f32 = np.float32
    start, step = PROTOCOLS[name][:2]
    assert (f32(se) * f32(step) + f32(start) == 0) == zero_at_se
    assert takes_mirrored_loop(params, name) == (zero_at_se and not multi)
    assert float(c.taus[se]) == float(f32(se) * f32(step) + f32(start))
    assert 0 < (~d["live"]).sum() < N_VOX and np.all(kl_reach(d["q"]) < LOGIT_CLIP)


# ---- (a) ELBO forward ------------------------------------------------------------------------------------------------
# (S, K, explicit normals): S = 1 one lane of a voxel draws; S = 3, 5: S % 4 != 0; K = 0: no KL draws; S = 32: two
# Philox calls per lane
ELBO_RUNS = ((1, 70, False), (3, 7, False), (5, 0, False), (32, 70, False), (3, 7, True))


def elbo_tolerance(S, explicit):
    """per-voxel NLL / KL rel_1"""
    return 1e-4 if explicit else (2e-4 if S <= 5 else 5e-4)


@pytest.mark.parametrize("name", list(PROTOCOLS))
def test_elbo_forward_matches_float64_oracle(params, name):
    from oracle.oracle import Oracle
    d = inputs(params, name)
    c = context(d)
    o32 = Oracle("f32", d["p"], **d["sw"])
    n, v0 = N_VOX, 1000003
    x, mask, q, prior, sigma = (dev(d[k]) for k in ("x", "mask", "q", "prior", "sigma"))
    m64 = d["mask"].astype(np.float64)
    fails = []
    with float64_oracle(d["p"], d["sw"]) as o64:
        for S, K, explicit in ELBO_RUNS:
            seed = 100 + S
            if explicit:
                rng = np.random.default_rng(9)
                zs = rng.standard_normal((n, S, 2)).astype(np.float32)
                zk = rng.standard_normal((n, K, 2)).astype(np.float32)
                sums, nk = c.elbo_fwd(x, mask, q, prior, sigma, S, K, zs=dev(zs), zk=dev(zk))
            else:
                zs = o32.philox_normals(seed, 0, v0, n, S)
                zk = o32.philox_normals(seed, 1, v0, n, K)
                sums, nk = c.elbo_fwd(x, mask, q, prior, sigma, S, K, seed=seed, voxel0=v0)
            ref = elbo_reference(o64, d, zs, zk)
            sums, nk = sums.cpu().numpy(), nk.cpu().numpy().astype(np.float64)
            assert np.all(np.isfinite(nk))
            got = (sums[0] + sums[1]) / sums[2]
            rows = np.array([(m64 * nk[:, 0]).sum(), nk[d["live"], 1].sum(), m64.sum()])
            tol = elbo_tolerance(S, explicit)
            _report(fails, f"elbo {name} S={S} K={K} {'explicit' if explicit else 'philox'}",
                    dict(nll=rel1(nk[:, 0], ref["nll_v"]), kl=rel1(nk[:, 1], ref["kl_v"]),
                         elbo=abs(got - ref["elbo"]) / abs(ref["elbo"]),
                         sums=float(np.max(np.abs(sums - rows) / np.maximum(np.abs(rows), 1e-300)))),
                    dict(nll=tol, kl=tol, elbo=1e-4, sums=1e-8))
            if K == 0:
                assert np.all(nk[:, 1] == 0.0) and sums[1] == 0.0
    assert not fails, fails


@pytest.mark.parametrize("name", list(PROTOCOLS))
def test_elbo_forward_small_batches_and_voxel0(params, name):
    """N = 17 (one partial wave), N = 1, a batch that starts at voxel 100 of the stream, N = 0: the rows of the full
    batch bit for bit (no voxel here is over the reach bound of the whitened KL, so the form does not depend on the
    wave's other voxels), and zero sums for no voxels."""
    d = inputs(params, name)
    c = context(d)
    S, K, seed, v0 = 3, 7, 31, 77
    t = [dev(d[k]) for k in ("x", "mask", "q", "prior", "sigma")]
    s_all, nk = c.elbo_fwd(*t, S, K, seed=seed, voxel0=v0)
    parts = np.zeros(3)
    for lo, hi in ((0, 17), (17, 18), (18, 100), (100, N_VOX)):
        sp, nkp = c.elbo_fwd(*[a[lo:hi] for a in t], S, K, seed=seed, voxel0=v0 + lo)
        assert _same_bits(nkp, nk[lo:hi]), (name, lo, hi)
        parts += sp.cpu().numpy()
    want = s_all.cpu().numpy()
    assert np.all(np.abs(parts - want) <= 1e-8 * np.abs(want)), (parts, want)
    # the same voxels at voxel0 = 0 are other draws
    _, other = c.elbo_fwd(*[a[:17] for a in t], S, K, seed=seed, voxel0=0)
    assert not torch.equal(other, nk[:17])
    T = c.T
    e = [torch.empty((0, w), device="cuda") for w in (T, 5, 5, T)]
    s0, nk0 = c.elbo_fwd(e[0], torch.empty(0, device="cuda"), e[1], e[2], e[3], S, K)
    assert s0.cpu().tolist() == [0.0, 0.0, 0.0] and nk0.shape == (0, 2)


# ---- (b) importance-weighted evidence and its per-draw rows ---------------------------------------------------------
IW_TOL = dict(log_p=1e-4, elbo=1e-4, ess=1e-4, means=1e-4)   # test_gpu_log_evidence.py


def _iw_errors(out, means, ref, live):
    return dict(log_p=rel1(out[live, 0], ref["log_p"][live]), elbo=rel1(out[live, 1], ref["elbo"][live]),
                ess=rel(out[live, 2], ref["ess"][live]), means=rel(means[live], ref["means"][live]))


@pytest.mark.parametrize("name", list(PROTOCOLS))
def test_log_evidence_matches_float64_reference(params, name):
    d = inputs(params, name)
    c = context(d)
    n, v0, live = N_VOX, 1000003, d["live"]
    x, mask, q, prior, sigma = (dev(a) for a in (poisoned(d), d["mask"], d["q"], d["prior"], d["sigma"]))
    m64 = d["mask"].astype(np.float64)
    fails = []
    with float64_oracle(d["p"], d["sw"]) as o64:
        def check(what, K, normals, **kw):
            ref = iw_reference(o64, d["x"], d["q"], d["prior"], d["sigma"], normals, d["p"])
            sums, out, means = c.log_evidence(x, mask, q, prior, sigma, K, want_means=True, **kw)
            sums, out, means = (t.cpu().numpy().astype(np.float64) for t in (sums, out, means))
            assert np.all(np.isfinite(out[live])) and np.all(np.isfinite(means[live]))
            assert np.all(np.isnan(out[~live, 0]))   # their data are NaN: nothing of it may reach another row
            _report(fails, f"log_evidence {name} {what} K={K}", _iw_errors(out, means, ref, live), IW_TOL)
            want = np.array([(m64[live] * -out[live, 0]).sum(), (m64[live] * -out[live, 1]).sum(), m64.sum()])
            assert np.all(np.abs(sums - want) <= 1e-8 * np.abs(want)), (what, K, sums, want)
            return out

        z = np.random.default_rng(5).standard_normal((n, 64, 2)).astype(np.float32)
        check("explicit", 64, z, z=dev(z))
        for K in (1, 5, 27):   # one lane of four with a draw; a short Philox call; lanes with 8 / 8 / 8 / 3 draws
            seed = 40 + K
            z = c.normals(n, K, stream_id=IW_STREAM, seed=seed, voxel0=v0).cpu().numpy()
            out = check("philox", K, z, seed=seed, voxel0=v0)
            if K == 1:
                assert np.array_equal(out[live, 0], out[live, 1]) and np.all(out[live, 2] == 1.0)
        # the per-draw rows of that last run, K = 27 (iw_draws_generic_kernel), and what log_evidence made of them
        assert (K, seed, z.shape) == (27, 67, (n, 27, 2))
        lw_ref, y = log_weights(o64, d["x"], d["q"], d["prior"], d["sigma"], z)
        lw, th = c.log_evidence_draws(x, mask, q, prior, sigma, K, seed=seed, voxel0=v0, want_theta=True)
        dead = torch.as_tensor(~live, device="cuda")
        assert torch.isnan(lw[dead]).all() and torch.isnan(th[dead]).all()
        th_ref = np.stack([y[..., 0], y[..., 1], dw_coef(d["p"]) * y[..., 0] * y[..., 1]], -1)
        lse = (torch.logsumexp(lw.double(), 1) - math.log(K)).cpu().numpy()
        _report(fails, f"log_evidence_draws {name} K={K}",
                dict(lw=rel1(lw.cpu().numpy()[live], lw_ref[live]), theta=rel(th.cpu().numpy()[live], th_ref[live]),
                     reduced=rel1(lse[live], out[live, 0])), dict(lw=1e-4, theta=1e-4, reduced=1e-4))
    assert not fails, fails


# ---- (c) posterior predictive checks -------------------------------------------------------------------------------
def ppc_tolerances():
    import test_gpu_posterior_predictive as t
    return t.TOL, t._errors


@pytest.mark.parametrize("name", list(PROTOCOLS))
def test_posterior_predictive_matches_float64_reference(params, name):
    """At the encoder's sigma and at three times it: with the first the reference p-values of the long protocols are
    all but 0, with the second they spread over (0, 1) (tests/test_forward_protocols_host.py holds the inputs to
    that)."""
    TOL, errors = ppc_tolerances()
    d = inputs(params, name)
    c = context(d)
    n, v0, live = N_VOX, 1000003, d["live"]
    x, mask, q = (dev(a) for a in (poisoned(d), d["mask"], d["q"]))
    m64 = d["mask"].astype(np.float64)[live]
    fails = []
    with float64_oracle(d["p"], d["sw"]) as o64:
        for scale in (1.0, 3.0):
            sg = (d["sigma"] * np.float32(scale)).astype(np.float32)
            runs = [("explicit", 64, np.random.default_rng(5).standard_normal((n, 64, 2)).astype(np.float32), None),
                    ("philox", 6, None, 23)]
            for what, L, z, seed in runs:
                if z is None:
                    z = c.normals(n, L, stream_id=PPC_STREAM, seed=seed, voxel0=v0).cpu().numpy()
                    kw = dict(seed=seed, voxel0=v0)
                else:
                    kw = dict(z=dev(z))
                ref = ppc_reference(o64, d["x"], d["q"], sg, z)
                sums, out, curves = c.posterior_predictive(x, mask, q, dev(sg), L, want_curves=True, **kw)
                sums, out, curves = sums.cpu().numpy(), out.cpu().numpy(), curves.cpu().numpy()
                assert np.all(np.isnan(out[~live])) and np.all(np.isnan(curves[~live]))
                assert np.all(np.isfinite(out[live])) and np.all(np.isfinite(curves[live]))
                assert np.all((out[live, 0] >= 0) & (out[live, 0] <= 1))
                ref_live = dict(out=ref["out"][live], curves=ref["curves"][live])
                _report(fails, f"ppc {name} sigma x {scale:g} {what} L={L}", errors(out[live], curves[live], ref_live),
                        TOL)
                maz = rel(out[live, 5], ref["out"][live, 5])
                print("[forward protocols]", f"ppc {name} sigma x {scale:g} {what} L={L} max_abs_z={maz:.3e}")
                ol = out[live].astype(np.float64)
                want = np.array([(m64 * ol[:, 4]).sum(), (m64 * ol[:, 3]).sum(), (m64 * ol[:, 0]).sum(), m64.sum()])
                np.testing.assert_allclose(sums, want, rtol=1e-12)
    assert not fails, fails


# ---- (d) posterior grid ---------------------------------------------------------------------------------------------
def _node_step(box, n):
    return (box[1] - box[0]) / (n - 1), (box[3] - box[2]) / (n - 1)


@pytest.mark.parametrize("name", GRID_PROTOCOLS)
def test_posterior_grid_matches_float64_reference_on_the_kernels_box(params, name):
    """test_gpu_posterior_grid.test_matches_float64_reference_on_the_kernels_box, its bounds, 12 voxels."""
    d = inputs(params, name)
    c = context(d)
    n = 12
    x, q, prior, sigma = (d[k][:n] for k in ("x", "q", "prior", "sigma"))
    sums, out, box = c.posterior_grid(dev(x), None, dev(prior), dev(sigma), q=dev(q), want_box=True)
    out, box = out.cpu().numpy().astype(np.float64), box.cpu().numpy().astype(np.float64)
    with float64_oracle(d["p"], d["sw"]) as o64:
        ref, own = [], []
        for i in range(n):
            r, _ = gr.voxel_reference(o64, x[i], sigma[i], prior[i], q=q[i], gh=16, fine_box=box[i], dw=dw_coef(d["p"]))
            ref.append(r)
            _, b = gr.voxel_reference(o64, x[i], sigma[i], prior[i], q=q[i], gh=0, dw=dw_coef(d["p"]))
            own.append(b)
    ref, own = np.array(ref), np.array(own)
    fails = []
    _report(fails, f"grid {name}",
            dict(log_p=rel1(out[:, 0], ref[:, 0]), elbo=rel1(out[:, 1], ref[:, 1]), means=rel(out[:, 2:5], ref[:, 2:5]),
                 sds=rel(out[:, 5:8], ref[:, 5:8]), corr=float(np.max(np.abs(out[:, 8] - ref[:, 8]))),
                 quant=float(np.max(np.abs(out[:, 9:13] - ref[:, 9:13])))),
            dict(log_p=2e-4, elbo=2e-4, means=1e-4, sds=1e-4, corr=1e-3, quant=1e-4))
    assert not fails, fails
    for i in range(n):
        ha, hb = _node_step(box[i], 64)
        # one node in OEF / DBV units: the transforms' slopes are at most 0.8 / 4 and 0.2 / 4 per logit
        assert abs(out[i, 13] - ref[i, 13]) <= 0.2 * ha + 1e-6 and abs(out[i, 14] - ref[i, 14]) <= 0.05 * hb + 1e-6
        b0 = gr.start_box(prior[i], q[i])
        ca, cb = _node_step(b0, 32)
        assert np.all(np.abs(box[i, :2] - own[i, :2]) <= ca) and np.all(np.abs(box[i, 2:] - own[i, 2:]) <= cb), i
    assert sums.cpu().numpy()[2] == n


# ---- (e) more voxels than one pass of the capped grid ---------------------------------------------------------------
def big_n(num_cus):
    """One pass of the 32-voxel kernels holds 4 num_cus blocks = 128 num_cus voxels."""
    return 128 * num_cus + 37


def shards(n):
    """1,000 voxels, a multiple of 32 plus 5, the rest"""
    a = 1000
    b = a + 32 * (n // 64) + 5
    return (0, a), (a, b), (b, n)


@pytest.fixture(scope="module")
def big(params):
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = big_n(num_cus)
    d = inputs(params, "left12", n=n, seed=12)
    assert np.all(kl_reach(d["q"]) < LOGIT_CLIP)   # bit-equal shards need one form of log q - log p in every wave
    for lo, hi in shards(n):
        assert 0 < hi - lo <= 128 * num_cus
    sample = np.unique(np.concatenate([np.arange(0, n, 50), np.arange(n - 64, n)]))
    return d, context(d), n, sample[d["live"][sample]]


def test_second_pass_elbo(big):
    from oracle.oracle import Oracle
    d, c, n, _ = big
    S, K, seed, v0 = 1, 4, 19, 5000
    t = [dev(d[k]) for k in ("x", "mask", "q", "prior", "sigma")]
    sums, nk = c.elbo_fwd(*t, S, K, seed=seed, voxel0=v0)
    parts = np.zeros(3)
    for lo, hi in shards(n):
        sp, nkp = c.elbo_fwd(*[a[lo:hi] for a in t], S, K, seed=seed, voxel0=v0 + lo)
        assert _same_bits(nkp, nk[lo:hi]), (lo, hi)
        parts += sp.cpu().numpy()
    sums, nk = sums.cpu().numpy(), nk.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(parts - sums) <= 1e-8 * np.abs(sums)), (parts, sums)
    o32 = Oracle("f32", d["p"])
    with float64_oracle(d["p"], d["sw"]) as o64:
        ref = elbo_reference(o64, d, o32.philox_normals(seed, 0, v0, n, S), o32.philox_normals(seed, 1, v0, n, K))
    m64 = d["mask"].astype(np.float64)
    rows = np.array([(m64 * nk[:, 0]).sum(), nk[d["live"], 1].sum(), m64.sum()])
    fails = []
    _report(fails, f"second pass elbo left12 N={n}",
            dict(nll=rel1(nk[:, 0], ref["nll_v"]), kl=rel1(nk[:, 1], ref["kl_v"]),
                 elbo=abs((sums[0] + sums[1]) / sums[2] - ref["elbo"]) / abs(ref["elbo"]),
                 sums=float(np.max(np.abs(sums - rows) / np.abs(rows)))),
            dict(nll=elbo_tolerance(S, False), kl=elbo_tolerance(S, False), elbo=1e-4, sums=1e-8))
    assert not fails, fails


def test_second_pass_log_evidence(big):
    d, c, n, sample = big
    K, seed, v0 = 8, 21, 5000
    t = [dev(d[k]) for k in ("x", "mask", "q", "prior", "sigma")]
    sums, out, means = c.log_evidence(*t, K, seed=seed, voxel0=v0, want_means=True)
    lw, th = c.log_evidence_draws(*t, K, seed=seed, voxel0=v0, want_theta=True)
    parts = np.zeros(3)
    for lo, hi in shards(n):
        sp, op, mp = c.log_evidence(*[a[lo:hi] for a in t], K, seed=seed, voxel0=v0 + lo, want_means=True)
        assert _same_bits(op, out[lo:hi]) and _same_bits(mp, means[lo:hi]), (lo, hi)
        lp, tp = c.log_evidence_draws(*[a[lo:hi] for a in t], K, seed=seed, voxel0=v0 + lo, want_theta=True)
        assert _same_bits(lp, lw[lo:hi]) and _same_bits(tp, th[lo:hi]), (lo, hi)
        parts += sp.cpu().numpy()
    sums = sums.cpu().numpy()
    assert np.all(np.abs(parts - sums) <= 1e-8 * np.abs(sums)), (parts, sums)
    z = c.normals(n, K, stream_id=IW_STREAM, seed=seed, voxel0=v0)[dev(sample)].cpu().numpy()
    with float64_oracle(d["p"], d["sw"]) as o64:
        ref = iw_reference(o64, d["x"][sample], d["q"][sample], d["prior"][sample], d["sigma"][sample], z, d["p"])
    out, means, lw = (a.cpu().numpy().astype(np.float64)[sample] for a in (out, means, lw))
    fails = []
    errs = _iw_errors(out, means, ref, slice(None))
    errs["lw"] = rel1(lw, ref["lw"])
    _report(fails, f"second pass log_evidence left12 N={n} K={K} ({sample.size} voxels)", errs, dict(IW_TOL, lw=1e-4))
    assert not fails, fails


def test_second_pass_posterior_predictive(big):
    TOL, errors = ppc_tolerances()
    d, c, n, sample = big
    L, seed, v0 = 6, 25, 5000
    sg = (d["sigma"] * np.float32(3.0)).astype(np.float32)
    t = [dev(a) for a in (d["x"], d["mask"], d["q"], sg)]
    sums, out, curves = c.posterior_predictive(*t, L, seed=seed, voxel0=v0, want_curves=True)
    for lo, hi in shards(n):
        _, op, cp = c.posterior_predictive(*[a[lo:hi] for a in t], L, seed=seed, voxel0=v0 + lo, want_curves=True)
        assert _same_bits(op, out[lo:hi]) and _same_bits(cp, curves[lo:hi]), (lo, hi)
    z = c.normals(n, L, stream_id=PPC_STREAM, seed=seed, voxel0=v0)[dev(sample)].cpu().numpy()
    with float64_oracle(d["p"], d["sw"]) as o64:
        ref = ppc_reference(o64, d["x"][sample], d["q"][sample], sg[sample], z)
    out, curves = out.cpu().numpy(), curves.cpu().numpy()
    live = d["live"]
    assert np.all(np.isnan(out[~live])) and np.all(np.isfinite(out[live]))
    fails = []
    _report(fails, f"second pass ppc left12 N={n} L={L} ({sample.size} voxels)",
            errors(out[sample], curves[sample], ref), TOL)
    assert not fails, fails
    m64 = d["mask"].astype(np.float64)[live]
    ol = out[live].astype(np.float64)
    want = np.array([(m64 * ol[:, 4]).sum(), (m64 * ol[:, 3]).sum(), (m64 * ol[:, 0]).sum(), m64.sum()])
    np.testing.assert_allclose(sums.cpu().numpy(), want, rtol=1e-12)


def test_second_pass_posterior_grid(big):
    """The grid kernel holds 16 num_cus voxels in one pass: the full batch against its shards, bit for bit."""
    d, c, n, _ = big
    t = [dev(d[k]) for k in ("x", "mask", "prior", "sigma")]
    qd = dev(d["q"])
    sums, out, box = c.posterior_grid(*t, q=qd, want_box=True)
    parts = np.zeros(3)
    for lo, hi in shards(n):
        sp, op, bp = c.posterior_grid(*[a[lo:hi] for a in t], q=qd[lo:hi], want_box=True)
        assert _same_bits(op, out[lo:hi]) and _same_bits(bp, box[lo:hi]), (lo, hi)
        parts += sp.cpu().numpy()
    sums = sums.cpu().numpy()
    assert np.all(np.abs(parts - sums) <= 1e-8 * np.abs(sums)), (parts, sums)
    on = out.cpu().numpy()
    assert np.all(np.isnan(on[~d["live"]])) and np.all(np.isfinite(on[d["live"]]))
