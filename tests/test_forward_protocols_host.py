"""Host-side conditions of tests/test_gpu_forward_protocols.py: its protocol table gives the tau count, spin-echo index
and class (tau = 0 at the spin echo or not) it lists, through the oracle and through a host-only context; the three
float64 references are finite on it; on its inputs the float32 oracle is within the project's bounds of the float64
one (so a kernel that misses a bound there is not missing it on float32 accumulation alone; the distances printed here
are what the GPU figures are read against); the reference p-values of the posterior predictive checks are not
degenerate; and the batches of its sharding checks are what their bit-equality needs.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import _grid_reference as gr
from _iw_reference import dw_coef, iw_reference, rel1
from _ppc_reference import ppc_reference
import test_gpu_forward_protocols as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(G.PROTOCOLS)


def test_noise_bounds_name_cases_of_the_table():
    assert all(what.split()[1] in G.PROTOCOLS for what, _ in G.ACCUMULATION_NOISE)


def test_table_rows_build_as_listed(params):
    from oracle.oracle import Oracle
    from qbold_vi_amd.ops import Context
    f32 = np.float32
    hdr = open(os.path.join(ROOT, "qbold_vi_amd", "csrc", "qbold_dev.h")).read()
    assert int(re.search(r"#define QB_TAB_SEG (\d+)", hdr).group(1)) == G.QB_TAB_SEG
    core = open(os.path.join(ROOT, "qbold_vi_amd", "csrc", "elbo_core.h")).read()
    assert float(re.search(r"#define QB_LOGIT_CLIP ([0-9.]+)f", core).group(1)) == G.LOGIT_CLIP
    assert float(re.search(r"#define QB_Z_MAX ([0-9.]+)f", hdr).group(1)) == G.Z_MAX
    for name, (start, step, T, se, zero_at_se, multi) in G.PROTOCOLS.items():
        p, sw = G.protocol(params, name), G.switches(name)
        o = Oracle("f64", p, **sw)
        assert (o.T, o.se_idx) == (T, se), name
        c = Context(p, True, True, host_only=True, **sw)
        assert (c.T, c.se_idx) == (T, se), name
        tau_se = f32(se) * f32(step) + f32(start)
        assert (tau_se == 0) == zero_at_se and float(c.taus[se]) == float(tau_se), name
        assert G.takes_mirrored_loop(params, name) == (zero_at_se and not multi), name
        if not zero_at_se:
            assert abs(float(tau_se) + 1e-3) < 1e-8, name   # off22: the spin-echo index lands on -1 ms
        assert T not in (11, 24) and not (T == 64 and se == 12), name   # none takes a specialised kernel
    # what the names promise
    left = {k: v[3] - (v[2] - 1 - v[3]) for k, v in G.PROTOCOLS.items()}   # taus before the spin echo without a partner
    assert left["left12"] == 5 and all(left[k] <= 0 for k in NAMES if k != "left12")
    assert [G.PROTOCOLS[k][2] % 4 for k in ("left12", "right5", "two", "odd33", "off22", "full64")] == [0, 1, 2, 1, 2, 0]
    assert set(G.GRID_PROTOCOLS) <= set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_float64_references_are_finite(params, name):
    d = G.inputs(params, name)
    n = 8
    x, q, prior, sigma = (d[k][:n] for k in ("x", "q", "prior", "sigma"))
    assert np.all(np.isfinite(x)) and np.all(sigma > 0)
    z = np.random.default_rng(5).standard_normal((n, 16, 2)).astype(np.float32)
    with G.float64_oracle(d["p"], d["sw"]) as o64:
        iw = iw_reference(o64, x, q, prior, sigma, z, d["p"])
        ppc = ppc_reference(o64, x, q, sigma, z)
        grid, box = gr.voxel_reference(o64, x[0], sigma[0], prior[0], q=q[0], gh=16, dw=dw_coef(d["p"]))
    assert all(np.all(np.isfinite(iw[k])) for k in ("log_p", "elbo", "ess", "means", "lw"))
    assert np.all(np.isfinite(ppc["out"])) and np.all(np.isfinite(ppc["curves"]))
    assert np.all(np.isfinite(grid)) and np.all(np.isfinite(box))


@pytest.mark.parametrize("name", NAMES)
def test_float32_oracle_is_within_the_bounds_on_these_inputs(params, name):
    """The ELBO runs of the GPU file (the Philox streams and the explicit normals it uses), float32 oracle against
    float64 oracle, at the bounds the kernels are held to; the K = 64 importance-weighted run is printed."""
    from oracle.oracle import Oracle
    d = G.inputs(params, name)
    o32 = Oracle("f32", d["p"], **d["sw"])
    n, v0 = G.N_VOX, 1000003
    fails = []
    with G.float64_oracle(d["p"], d["sw"]) as o64:
        for S, K, explicit in G.ELBO_RUNS:
            seed = 100 + S
            if explicit:
                rng = np.random.default_rng(9)
                zs = rng.standard_normal((n, S, 2)).astype(np.float32)
                zk = rng.standard_normal((n, K, 2)).astype(np.float32)
            else:
                zs, zk = o32.philox_normals(seed, 0, v0, n, S), o32.philox_normals(seed, 1, v0, n, K)
            a, b = G.elbo_reference(o32, d, zs, zk), G.elbo_reference(o64, d, zs, zk)
            tol = G.elbo_tolerance(S, explicit)
            G._report(fails, f"float32 oracle: elbo {name} S={S} K={K} {'explicit' if explicit else 'philox'}",
                      dict(nll=rel1(a["nll_v"], b["nll_v"]), kl=rel1(a["kl_v"], b["kl_v"]),
                           elbo=abs(a["elbo"] - b["elbo"]) / abs(b["elbo"])), dict(nll=tol, kl=tol, elbo=1e-4))
        z = np.random.default_rng(5).standard_normal((n, 64, 2)).astype(np.float32)
        args = (d["x"], d["q"], d["prior"], d["sigma"], z, d["p"])
        a, b = iw_reference(o32, *args), iw_reference(o64, *args)
        # The importance-weighted columns of the float32 oracle, for the comparison with the kernels' figures: printed,
        # not gated (log p^ and the same-draw ELBO carry the per-draw NLL's noise, ESS and the means an absolute error
        # of log w undamped; on the 33- and 64-tau rows the float32 oracle is at 1 - 2.5e-4 there).
        seen = {}
        errs = G._iw_errors(np.stack([a["log_p"], a["elbo"], a["ess"]], -1), a["means"], b, slice(None))
        seen[f"log_evidence {name} explicit K=64"] = dict(errs, lw=rel1(a["lw"], b["lw"]))
        # the per-draw rows of the K = 27 run, on the oracle's statement of stream 6
        z = o32.philox_normals(67, G.IW_STREAM, v0, n, 27)
        args = (d["x"], d["q"], d["prior"], d["sigma"], z, d["p"])
        seen[f"log_evidence_draws {name} K=27"] = dict(lw=rel1(iw_reference(o32, *args)["lw"],
                                                               iw_reference(o64, *args)["lw"]))
    for what, errs in seen.items():
        G._report([], "float32 oracle: " + what, errs, dict(G.IW_TOL, lw=1e-4))
    assert not fails, fails
    # the cases the GPU file bounds at 3 x their measured value: the float32 oracle's distance recorded beside them is
    # the one computed here, and the kernel's is within twice it
    for (what, col), (measured, oracle32) in G.ACCUMULATION_NOISE.items():
        if what in seen:
            assert abs(seen[what][col] / oracle32 - 1.0) < 0.01, (what, col, seen[what][col], oracle32)
            assert 1e-4 < measured <= 2.0 * seen[what][col], (what, col, measured, seen[what][col])


def _ppp_share(ref):
    p = ref["out"][:, 0]
    return float(np.mean((p >= 0.01) & (p <= 0.99)))


@pytest.mark.parametrize("name", NAMES)
def test_reference_p_values_are_not_degenerate(params, name):
    """At the encoder's sigma or at three times it, a quarter of the voxels or more have a reference ppp in
    [0.01, 0.99]: the chi^2 tail of the kernel is compared where it is neither 0 nor 1.  Also printed: the float32
    oracle's distance to the float64 reference in every column the GPU test bounds."""
    from oracle.oracle import Oracle
    import test_gpu_posterior_predictive as ppc_tests
    d = G.inputs(params, name)
    o32 = Oracle("f32", d["p"], **d["sw"])
    z = np.random.default_rng(5).standard_normal((G.N_VOX, 64, 2)).astype(np.float32)
    share = {}
    with G.float64_oracle(d["p"], d["sw"]) as o64:
        for scale in (1.0, 3.0):
            sg = (d["sigma"] * np.float32(scale)).astype(np.float32)
            ref = ppc_reference(o64, d["x"], d["q"], sg, z)
            share[scale] = _ppp_share(ref)
            r32 = ppc_reference(o32, d["x"], d["q"], sg, z)
            errs = ppc_tests._errors(r32["out"], r32["curves"], ref)
            q = np.quantile(ref["out"][:, 0], (0.05, 0.5, 0.95))
            print("[forward protocols]", f"float32 oracle: ppc {name} sigma x {scale:g}",
                  " ".join(f"{k}={v:.3e}" for k, v in errs.items()),
                  f"| reference ppp 5/50/95 % = {q[0]:.3g}/{q[1]:.3g}/{q[2]:.3g}, share in [0.01, 0.99] = {share[scale]:.2f}")
    assert max(share.values()) >= 0.25, (name, share)


def test_batches_of_the_sharding_checks(params):
    """Bit-equal shards need every wave on the whitened form of log q - log p (decided per wave: one voxel over the
    reach bound changes its neighbours' rounding), shards within one pass of the capped grid, and a job past it."""
    for name in NAMES:
        d = G.inputs(params, name)
        assert 0 < (~d["live"]).sum() < G.N_VOX, name
        assert np.all(G.kl_reach(d["q"]) < G.LOGIT_CLIP), name
    for num_cus in (256, 304):   # MI355X; a part with more compute units
        n = G.big_n(num_cus)
        assert n > 128 * num_cus and n % 32
        sh = G.shards(n)
        assert sh[0] == (0, 1000) and (sh[1][1] - sh[1][0]) % 32 == 5 and sh[2][1] == n
        assert all(0 < hi - lo <= 128 * num_cus for lo, hi in sh)
        assert [a[1] for a in sh[:-1]] == [b[0] for b in sh[1:]]
    d = G.inputs(params, "left12", n=G.big_n(256), seed=12)
    assert np.all(G.kl_reach(d["q"]) < G.LOGIT_CLIP)
    assert 0 < (~d["live"]).sum() < d["live"].size
