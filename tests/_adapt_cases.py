"""The case table of tests/test_adapt_host.py and tests/test_gpu_adapt.py: per case its inputs, the stream's normals, the
float64 reference run of tests/_adapt_reference.py and, on request, the float32 run (the floor), each built once and
shared.  The recorded floors live here; test_adapt_host.py holds them to what the float32 oracle gives, and nothing of
the kernel enters them.  Test infrastructure (no GPU needed)."""
import types

import numpy as np

import _adapt_reference as ar
import _laplace_reference as lr

N_VOX = 48   # 32 voxels per block: a full block and half a block
SHRINK = 4.0
VOXEL0 = 1000003


def make_mask(n=N_VOX):
    """0, 0.5 and 1 mixed (every fifth voxel out), one NaN"""
    i = np.arange(n)
    m = np.where(i % 5 == 3, 0.0, np.where(i % 2 == 1, 0.5, 1.0)).astype(np.float32)
    m[10] = np.nan
    return m


def _start_default(d, rng):
    """the prior's own heads on the even voxels, heads displaced by about a prior sd with other spreads on the odd"""
    q = d["prior"].copy()
    odd = np.arange(len(q)) % 2 == 1
    q[odd, 0] += rng.normal(0.0, 0.5, int(odd.sum())).astype(np.float32)
    q[odd, 2] += rng.normal(0.0, 0.5, int(odd.sum())).astype(np.float32)
    q[odd, 1] += rng.uniform(-0.3, 0.1, int(odd.sum())).astype(np.float32)
    q[odd, 3] += rng.uniform(-0.3, 0.1, int(odd.sum())).astype(np.float32)
    return q


def _start_reach(d, rng):
    """_start_default with six voxels over the reach bound of the whitened log q - log p (mean 10.5, sd 0.86 of the OEF
    or the DBV logit): |mu| + 4.8549 sd = 14.7 > 13.8155, while hardly a draw reaches the clip itself"""
    q = _start_default(d, rng)
    for k, v in enumerate((1, 6, 17, 30, 31, 44)):
        q[v, 0 if k % 2 == 0 else 2] = 10.5 if k % 4 < 2 else -10.5
        q[v, 1 if k % 2 == 0 else 3] = 0.29
    return q


def _start_clip(d, rng):
    """_elbo_bwd_cases.EDITS["kl_clip_binds"]'s heads: means within half a standard deviation of the clip in the OEF
    logit (voxels 0, 1 mod 4: + / -) or the DBV logit (2, 3 mod 4), log-std heads at raw 0.5 (sd 1.47)"""
    q = d["prior"].copy()
    q[:, [1, 3]] = 0.5
    i = np.arange(len(q))
    q[i % 4 == 0, 0], q[i % 4 == 1, 0] = 13.2, -13.2
    q[i % 4 == 2, 2], q[i % 4 == 3, 2] = 13.2, -13.2
    q[i % 8 == 0, 0], q[i % 8 == 6, 2] = 13.8, 13.8   # a hair inside the clip: an outward move lands on it
    return q


def _start_saturated(d, rng):
    """raw s_o, s_d, c heads at +-3, +-5, +-8 (voxel v: head (v // 6) % 3 at [3, -3, 5, -5, 8, -8][v % 6]; from voxel 36
    on all three at once)"""
    q = d["prior"].copy()
    vals = [3.0, -3.0, 5.0, -5.0, 8.0, -8.0]
    for v in range(len(q)):
        if v < 36:
            q[v, (1, 3, 4)[(v // 6) % 3]] = vals[v % 6]
        else:
            q[v, [1, 3, 4]] = vals[v % 6]
    return q


STARTS = dict(default=_start_default, reach=_start_reach, clip=_start_clip, saturated=_start_saturated)

# name: (protocol, rounds, K, start, seed of the draws)
#   (1, 8): two Philox calls, lane groups 2 and 3 of a voxel have no draws; (3, 20): five calls, lane group 0 wraps
CASES = {
    "ref11_R1_K8": ("ref11", 1, 8, "default", 3),
    "ref11_R3_K20": ("ref11", 3, 20, "default", 3),
    "ref11_R6_K64": ("ref11", 6, 64, "default", 3),
    "odd33_R3_K20": ("odd33", 3, 20, "default", 3),
    "odd33_R6_K64": ("odd33", 6, 64, "default", 3),
    "off22_3img_R3_K20": ("off22_3img", 3, 20, "default", 3),
    "full64_R6_K64": ("full64", 6, 64, "default", 3),
    "ref11_reach_R3_K20": ("ref11", 3, 20, "reach", 3),
    "ref11_clip_R3_K20": ("ref11", 3, 20, "clip", 3),
    "odd33_saturated_R3_K20": ("odd33", 3, 20, "saturated", 3),
}
PARITY = tuple(n for n, c in CASES.items() if c[3] == "default")
EDGES = ("ref11_clip_R3_K20", "odd33_saturated_R3_K20")
REACH = "ref11_reach_R3_K20"

ROUND0 = dict(log_p=1e-4, ess=1e-4, q=1e-4)   # test_gpu_log_evidence.py's bounds for the same arithmetic
FLOOR_FACTOR = 4.0                            # _elbo_bwd_cases.FLOOR_LS's precedent
# The float32 floors of the rounds after the first, per parity case: the worst distance over the live voxels and the
# rounds r >= 1 between the float32 run and the float64 run of tests/_adapt_reference.py, (log p^ rel_1, ESS relative,
# proposal_error of q_rounds).  Computed on the CPU; test_adapt_host.test_float32_floors holds the figures.
FLOORS = {
    "ref11_R3_K20": (1.12e-5, 1.38e-4, 3.14e-5),
    "ref11_R6_K64": (7.04e-6, 2.58e-4, 1.52e-4),
    "odd33_R3_K20": (1.47e-5, 2.57e-4, 7.98e-5),
    "odd33_R6_K64": (1.49e-5, 1.31e-3, 6.27e-4),
    "off22_3img_R3_K20": (2.09e-5, 1.31e-4, 2.81e-5),
    "full64_R6_K64": (3.28e-5, 3.53e-3, 2.03e-3),
}

_built = {}


def errors(got, ref, live=slice(None)):
    """per round [R]: (log_p rel_1, ess rel, proposal_error) of `got` against `ref` (dicts of log_p, ess, q_rounds)"""
    from _iw_reference import rel, rel1
    R = ref["log_p"].shape[1]
    e = np.zeros((R, 3))
    for r in range(R):
        e[r] = (rel1(got["log_p"][live, r], ref["log_p"][live, r]), rel(got["ess"][live, r], ref["ess"][live, r]),
                float(np.max(ar.proposal_error(got["q_rounds"][live, r], ref["q_rounds"][live, r]))))
    return e


def later_round_bounds(name):
    """(log_p, ess, q) bounds of the rounds r >= 1: 4 x the recorded floor, never below the round-0 bound"""
    f = FLOORS[name]
    return tuple(max(FLOOR_FACTOR * f[i], b) for i, b in enumerate((ROUND0["log_p"], ROUND0["ess"], ROUND0["q"])))


def build(params, name, want_f32=False):
    """The case: p, sw, R, K, seed, x, sigma, prior, q, mask, live [N_VOX], z [N_VOX, R K, 2] (the stream's normals),
    ref = the float64 run on the live voxels (rows in the order of np.nonzero(live)), f32 = the float32 run (want_f32)."""
    from oracle.oracle import Oracle
    from test_gpu_forward_protocols import float64_oracle
    if name not in _built:
        proto, R, K, start, seed = CASES[name]
        c = types.SimpleNamespace(name=name, R=R, K=K, seed=seed)
        c.p, c.sw = lr.setup(params, proto)
        c.o32 = Oracle("f32", c.p, **c.sw)
        d = lr.inputs(c.o32, proto, n=N_VOX)
        c.x, c.sigma, c.prior = d["x"], d["sigma"], d["prior"]
        c.q = STARTS[start](d, np.random.default_rng(21)).astype(np.float32)
        c.mask = make_mask()
        c.live = c.mask > 0
        c.rows = np.nonzero(c.live)[0]
        c.z = ar.normals(c.o32, seed, VOXEL0, N_VOX, R, K)
        with float64_oracle(c.p, c.sw) as o64:
            c.ref = ar.adapt(o64, c.x[c.rows], c.q[c.rows], c.prior[c.rows], c.sigma[c.rows], c.z[c.rows], R, K, SHRINK)
        c.f32 = None
        for a in (c.q, c.mask, c.z):
            a.setflags(write=False)
        _built[name] = c
    c = _built[name]
    if want_f32 and c.f32 is None:
        c.f32 = ar.adapt(c.o32, c.x[c.rows], c.q[c.rows], c.prior[c.rows], c.sigma[c.rows], c.z[c.rows], c.R, c.K,
                         SHRINK, f32=True)
    return c
