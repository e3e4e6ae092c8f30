"""The cases on which qbold_fisher_information and qbold_design_scores are held to tests/_design_reference.py: points,
sigma, priors, masks, designs and the float64 reference, built once per case and shared by test_design_host (the
float32 floor, the reference's own checks) and test_gpu_design (the kernels).  NumPy and the CPU oracle only."""
import contextlib

import numpy as np

import _design_reference as dr
from _elbo_bwd_cases import protocol

MULTI = dict(multi_image_normalisation=True)
SIGMA = 0.02
PRIOR = (0.0, 0.3, -1.0, 0.3, 0.0)
SEED = 23
B_ALL = 70           # the designs of a case; the first 1 and the first 5 are the smaller batches
EDGE = 1e-4          # the heads' saturating ends: this far from either end of the transforms' ranges

# name: (T, three-image normalisation, N, one sigma row shared by all voxels).  N = 40: a partial wave; N = 257: two
# 128-thread blocks plus one voxel (one 256-voxel tile plus one).  12 taus: the spin echo at index 10, every tau within
# 10 ms of it; 22: no tau equal to 0; 33: T % 4 != 0; T = 1: the exactly singular case, one row.
CASES = {
    "t11_N257": (11, False, 257, False), "t11_multi_N40": (11, True, 40, True),
    "t24_N40": (24, False, 40, True), "t24_multi_N257": (24, True, 257, False),
    "t12_N257": (12, False, 257, True), "t12_multi_N40": (12, True, 40, False),
    "t22_N40": (22, False, 40, False), "t22_multi_N257": (22, True, 257, True),
    "t33_N257": (33, False, 257, False), "t33_multi_N40": (33, True, 40, True),
    "t64_N40": (64, False, 40, True), "t64_multi_N257": (64, True, 257, False),
    "t1_N40": (1, False, 40, False),
}
DEFAULT_CASE = "t11_N257"

# The float32 floor per case, (entries of I, quantities derived from det I, log det A): the worst figures, in the measure
# of `measures` / `groups` below, of the same composition on the float32 oracle's primitives with float32 accumulation
# against float64 (test_design_host.test_float32_floor measures them again and holds these figures; nothing of the
# kernels enters).  The GPU test holds the kernels to 4 x these.  The entries' floor is set by the rows next to the spin
# echo, where d yhat_t is a difference of two nearly equal slopes, on the designs that put their weight there.
FLOOR = {
    "t11_N257": (4.374e-04, 8.173e-07, 4.809e-06),
    "t11_multi_N40": (6.188e-04, 2.485e-06, 1.408e-05),
    "t24_N40": (9.347e-05, 8.808e-07, 1.832e-05),
    "t24_multi_N257": (1.099e-04, 8.246e-07, 7.330e-06),
    "t12_N257": (1.206e-02, 1.096e-04, 2.181e-05),
    "t12_multi_N40": (5.949e-03, 4.902e-05, 1.222e-05),
    "t22_N40": (8.005e-05, 4.757e-07, 1.469e-05),
    "t22_multi_N257": (1.360e-04, 5.064e-07, 7.899e-06),
    "t33_N257": (9.019e-04, 1.525e-05, 1.674e-05),
    "t33_multi_N40": (6.420e-04, 2.440e-05, 2.209e-05),
    "t64_N40": (7.327e-05, 3.698e-07, 2.243e-05),
    "t64_multi_N257": (4.293e-05, 4.623e-07, 1.648e-05),
    "t1_N40": (1.459e-04, 0.000e+00, 5.425e-07),
}


def case_protocol(params, T):
    if T == 1:   # one tau, 0.5 ms before the spin echo (index 0)
        return dict(params, tau_start="-0.0005", tau_end="0.0004", tau_step="0.001")
    return protocol(params, T)


@contextlib.contextmanager
def float64_oracle(p, sw):
    """The f64 oracle with Simpson node 0 dropped from F (the float32 table's value); the flag is process-global in the
    C library and is put back."""
    from oracle.oracle import Oracle
    o64 = Oracle("f64", p, node0_zero=True, **sw)
    try:
        yield o64
    finally:
        o64.lib.qbo_set_node0_zero(0)


def designs(T, rng):
    """[B_ALL, T] weight rows: all ones, an integer allocation, a row with zeros, a single non-zero tau (the data part
    is then rank 1), a fractional row; then random integer allocations, every third with zeros."""
    w = np.ones((B_ALL, T), np.float32)
    w[1] = 1 + (np.arange(T) % 3)
    w[2] = (np.arange(T) % 2 == 0) * 2.0
    w[3] = 0.0
    w[3, T - 1] = 5.0
    w[4] = rng.uniform(0.25, 3.0, T)
    for b in range(5, B_ALL):
        w[b] = rng.integers(1, 5, T)
        if b % 3 == 0:
            w[b] *= rng.uniform(size=T) > 0.4
    return w


class Case:
    pass


_built = {}


def inputs(name):
    """The float32 arrays a case hands to the kernels (no oracle involved)."""
    T, multi, N, shared = CASES[name]
    rng = np.random.default_rng(SEED + T + 100 * multi)
    c = Case()
    c.name, c.T, c.multi, c.N, c.shared = name, T, multi, N, shared
    c.sw = dict(MULTI) if multi else {}
    theta = np.stack([rng.uniform(0.1, 0.75, N), rng.uniform(0.005, 0.15, N)], -1)
    theta[0:4, 0] = [dr.OEF_LO + EDGE, dr.OEF_HI - EDGE, 0.3, 0.5]
    theta[0:4, 1] = [0.03, 0.08, dr.DBV_LO + EDGE, dr.DBV_HI - EDGE]
    c.theta = theta.astype(np.float32)
    c.sigma = (SIGMA * rng.uniform(0.9, 1.1, (T,) if shared else (N, T))).astype(np.float32)
    prior = np.tile(np.array(PRIOR), (N, 1))
    prior[:, [0, 2]] += 0.3 * rng.standard_normal((N, 2))
    prior[:, [1, 3]] += 0.05 * rng.standard_normal((N, 2))
    prior[:, 4] += 0.2 * rng.standard_normal(N)
    c.prior = prior.astype(np.float32)
    c.mask = rng.choice(np.array([0.0, 0.5, 1.0, 1.0], np.float32), size=N)
    c.mask[:8] = [1.0, 1.0, 1.0, 1.0, 0.0, 0.5, 1.0, 0.0]
    c.live = c.mask > 0
    c.weights = designs(T, rng)
    for a in (c.theta, c.sigma, c.prior, c.mask, c.weights):
        a.setflags(write=False)
    return c


def build(params, name):
    """The case with its oracles and the float64 reference of all B_ALL designs (c.ref) and of the unweighted call
    (c.ref1: weights None).  Built once and kept; nothing in it may be modified."""
    if name in _built:
        return _built[name]
    from oracle.oracle import Oracle
    c = inputs(name)
    c.p = case_protocol(params, c.T)
    c.o32 = Oracle("f32", c.p, **c.sw)
    assert c.o32.T == c.T
    with float64_oracle(c.p, c.sw) as o64:
        c.ref = dr.reference(o64, c.theta, c.sigma, c.weights, c.prior, c.multi)
        c.ref1 = dr.reference(o64, c.theta, c.sigma, None, c.prior, c.multi)
    _built[name] = c
    return c


def measures(got, ref, live=None):
    """The worst figure of every quantity of `got` (the reference's dict, from a kernel or from the float32
    composition) against the float64 `ref`, over the voxels `live`, in the test's measure:
      I        |d| / (|I_aa| + 2 |I_ab| + |I_bb|): the entries to their absolute-sum scale
      the quantities derived from det I (kappa, log det I, the data-only sds and correlation): a relative error eps of
      the entries moves det I by eps kappa, so |d| / (scale kappa) with scale = the quantity itself (kappa, the sds) or
      1 (log det, the correlation); voxels the reference calls singular must be flagged and carry the fixed values
      log det A likewise by kappa_A.
    Returns dict(name: figure)."""
    sel = slice(None) if live is None else live
    out = {}
    I, Ir = np.asarray(got["I"], np.float64)[:, sel], ref["I"][:, sel]
    scale = np.abs(Ir[..., 0, 0]) + 2 * np.abs(Ir[..., 0, 1]) + np.abs(Ir[..., 1, 1])
    with np.errstate(all="ignore"):
        out["I"] = float(np.max(np.where(scale > 0, np.abs(I - Ir).max((-1, -2)) / scale,
                                         np.where(np.abs(I - Ir).max((-1, -2)) == 0, 0.0, np.inf))))
        ok = ~ref["singular"][:, sel]
        k = ref["kappa"][:, sel]

        def fig(g, r, sc):
            g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
            return float(np.max(np.where(ok, np.abs(g - r) / (sc * k), 0.0), initial=0.0))
        out["kappa"] = fig(got["kappa"][:, sel], k, k)
        out["log_det"] = fig(got["log_det"][:, sel], ref["log_det"][:, sel], 1.0)
        gc, rc = np.asarray(got["crlb"], np.float64)[:, sel], ref["crlb"][:, sel]
        for i, key in enumerate(("oef_crlb", "dbv_crlb", "r2p_crlb")):
            out[key] = fig(gc[..., i], rc[..., i], rc[..., i])
        out["corr"] = fig(gc[..., 3], rc[..., 3], 1.0)
        if "log_det_A" in got and "log_det_A" in ref:
            out["log_det_A"] = float(np.max(np.abs(np.asarray(got["log_det_A"], np.float64)[:, sel]
                                                   - ref["log_det_A"][:, sel]) / ref["kappa_A"][:, sel]))
    return out


DET_KEYS = ("kappa", "log_det", "oef_crlb", "dbv_crlb", "r2p_crlb", "corr")


def groups(m):
    """(the entries of I, the worst of the quantities derived from det I, log det A) of a `measures` dict: the three
    figures FLOOR records per case."""
    return m["I"], max(m[k] for k in DET_KEYS), m["log_det_A"]
