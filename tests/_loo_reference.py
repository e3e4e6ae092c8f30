"""Float64 reference of PSIS leave-one-out cross-validation (qbold_loo, include/qbold_hip.h), composed from the
references the suite already has: _iw_reference.log_weights for log w, _ppc_reference.draws for the per-tau log density
and _psis_reference.psis_row for the smoothing of every row.  Also the inputs and the cases of tests/test_gpu_loo.py, so
that tests/test_loo_host.py can check without a GPU the condition the GPU tests rest on (every row finite in float64).
Test infrastructure (no GPU needed)."""
import contextlib
import math

import numpy as np

from _iw_reference import log_weights
from _ppc_reference import draws
from _psis_reference import psis_row

IW_STREAM = 6
N_VOX = 48          # a partial wave of the rows kernel's 16-voxel waves, 1.5 of its 32-voxel blocks
VOXEL0 = 1000003


def _p24(params):
    return dict(params, tau_start="-0.028", tau_end="0.065", tau_step="0.004")


def _protocol(name):
    def make(params):
        from test_gpu_forward_protocols import protocol
        return protocol(params, name)
    return make


# case: (protocol or None = the configuration's 11 taus, likelihood switches, the draw counts)
#   K = 25: rows not 16-byte aligned; 70: a short last Philox call; 1024: the PSIS kernel's 16 register slots
CASES = {
    "T11": (None, {}, (25, 70, 1024)),
    "T24": (_p24, {}, (100,)),
    "student_t": (None, dict(student_t_df=5.0), (100,)),
    "three_image": (None, dict(multi_image_normalisation=True), (100,)),
    "log_data": (None, dict(predict_log_data=True), (100,)),
    "left12": (_protocol("left12"), {}, (100,)),
    "off22": (_protocol("off22"), {}, (100,)),
    "two": (_protocol("two"), {}, (100,)),
    "full64": (_protocol("full64"), {}, (100,)),
}
CASE_KS = [(c, K) for c, (_, _, ks) in CASES.items() for K in ks]
# Seed of the synthetic voxels per case: the first one from 11 at which every row of the float64 reference is finite
# (tests/test_loo_host.py holds both halves of that sentence); a property of the inputs and the oracle alone.
INPUT_SEEDS = {}


def seed_of(case):
    return INPUT_SEEDS.get(case, 11)


def case_params(params, case):
    proto, sw, _ = CASES[case]
    return (proto(params) if proto else params), sw


def centred_heads(truth):
    """Raw heads [N, 5] of a posterior centred on the true (OEF, DBV): mu = logit of the unit-interval value, log sds
    log 0.3 and log 0.6 through the inverse of transform_std (s = 3 tanh(p) - 1), no correlation."""
    t = np.asarray(truth, np.float64)
    u0, u1 = (t[:, 0] - 0.04) / 0.8, (t[:, 1] - 0.001) / 0.2
    q = np.zeros((t.shape[0], 5))
    q[:, 0] = np.log(u0) - np.log1p(-u0)
    q[:, 1] = math.atanh((math.log(0.3) + 1.0) / 3.0)
    q[:, 2] = np.log(u1) - np.log1p(-u1)
    q[:, 3] = math.atanh((math.log(0.6) + 1.0) / 3.0)
    return q.astype(np.float32)


_INPUTS = {}


def inputs(params, case, seed=None, n=N_VOX):
    """dict(p, sw, T, x, q, prior, sigma), computed once per (case, seed) and never written to: the data and the true
    parameters of synth_inputs, heads centred on the truth, prior and sigma from the untrained encoder of
    test_gpu_psis._heads (its own heads give NaN rows in float64 and are not used)."""
    from oracle.oracle import Oracle, synth_inputs
    from test_gpu_psis import _heads
    seed = seed_of(case) if seed is None else seed
    key = (case, seed, n)
    if key not in _INPUTS:
        p, sw = case_params(params, case)
        o32 = Oracle("f32", p, **sw)
        x, _, prior, sigma = _heads(o32, p, o32.T, n, seed)
        x2, truth = synth_inputs(n, p, seed=seed, oracle=o32)
        assert np.array_equal(x, x2)
        d = dict(p=p, sw=sw, T=o32.T, x=x, q=centred_heads(truth), prior=np.asarray(prior, np.float32),
                 sigma=np.asarray(sigma, np.float32))
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


def rows(o, x, q, prior, sigma, z):
    """dict(lw [N, K], ll [N, T, K], log_ratio [N, T + 1, K], nll_check = max |sum_t ll + nll| relative) in `o`'s
    precision for explicit normals z [N, K, 2]."""
    lw, _ = log_weights(o, x, q, prior, sigma, z)
    _, _, _, lp = draws(o, x, q, sigma, z)            # [N, K, T]
    ll = np.ascontiguousarray(np.transpose(np.asarray(lp, np.float64), (0, 2, 1)))
    lw = np.asarray(lw, np.float64)
    rho = np.concatenate([lw[:, None, :] - ll, lw[:, None, :]], axis=1)
    return dict(lw=lw, ll=ll, log_ratio=rho)


def finalise(ll, weights, khat):
    """The closing stage in float64 from ll [N, T, K], the normalised smoothed log-weights of the T + 1 rows
    [N, T + 1, K] and their k^ [N, T + 1]: dict(out [N, 6], pointwise [N, T, 3])."""
    ll = np.asarray(ll, np.float64)
    w = np.asarray(weights, np.float64)
    khat = np.asarray(khat, np.float64)
    N, T, K = ll.shape
    m = ll.max(-1, keepdims=True)
    with np.errstate(all="ignore"):
        e = np.exp(ll - m)
        elpd_t = m[..., 0] + np.log((np.exp(w[:, :T]) * e).sum(-1))
        lppd_t = m[..., 0] + np.log((np.exp(w[:, T:T + 1]) * e).sum(-1))
    kt = khat[:, :T]
    worst = np.array([int(np.nonzero(np.isnan(r))[0][0]) if np.isnan(r).any() else int(np.argmax(r)) for r in kt])
    kmax = kt[np.arange(N), worst]
    elpd, lppd = elpd_t.sum(-1), lppd_t.sum(-1)
    out = np.stack([elpd, lppd - elpd, lppd, kmax, worst.astype(np.float64), khat[:, T]], -1)
    return dict(out=out, pointwise=np.stack([elpd_t, kt, lppd_t], -1))


def smooth(log_ratio):
    """psis_row on every row of log_ratio [N, T + 1, K]: (weights [N, T + 1, K], khat [N, T + 1])."""
    lr = np.asarray(log_ratio, np.float64)
    res = [[psis_row(r) for r in v] for v in lr]
    return (np.array([[r["weights"] for r in v] for v in res]), np.array([[r["khat"] for r in v] for v in res]))


def loo_reference(o, x, q, prior, sigma, z):
    """The whole definition in float64: rows() + dict(out, pointwise, weights, khat)."""
    r = rows(o, x, q, prior, sigma, z)
    w, kh = smooth(r["log_ratio"])
    return dict(r, weights=w, khat=kh, **finalise(r["ll"], w, kh))


def rel1(a, b):
    """max |a - b| / (|b| + 1)"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / (np.abs(b) + 1.0)))
