"""tests/_pretrain_loss_reference.py held on the CPU: its values against the float64 oracle's functions, its gradients
against five-point central differences of those functions (base and saturated heads), the same formulas in float32
NumPy against it (the floor of test_gpu_pretrain_loss_reference's bounds), and planted defects that the bounds must
tell apart."""
import numpy as np
import pytest

import _pretrain_loss_cases as cases
import _pretrain_loss_reference as R

BOUND_Q, BOUND_V = cases.BOUND_Q, cases.BOUND_V
VAL_TOL = 1e-11      # reference value against the oracle's, of A_v (both float64; different order of operations)
FD_TOL = 1e-6        # reference gradient against five-point differences, of A_q
H, H_SAT, SAT = 2e-4, 2e-2, 2.5
# Steps of the differences.  H: the sharpest curvature is the inverse-gamma term's b / (e^(2 s_d) + raw4^2), which turns
# over a raw4 of e^s_d = 0.02.  H_SAT, for a head at |raw| >= SAT: there tanh and the sigmoid are exponentials of the
# head (f^(5) / f' = 16, truncation h^4 16 / 30 = 9e-8 of the slope), and the slope (3 sech^2(8) = 1.4e-6) is so small
# against the value that the rounding of a difference over H (1e-16 |v| / H) would drown it.


def five_point(fn, q, k):
    """d fn / d q[:, k] per voxel (fn maps [N, 5] float64 heads to [N] values, voxels independent)."""
    h = np.where(np.abs(q[:, k]) >= SAT, H_SAT, H)
    d = np.zeros_like(q)
    d[:, k] = h
    return (-fn(q + 2 * d) + 8.0 * fn(q + d) - 8.0 * fn(q - d) + fn(q - 2 * d)) / (12.0 * h)


def fd_gradient(fn, q):
    q = np.asarray(q, np.float64)
    return np.stack([five_point(fn, q, k) for k in range(5)], -1)


def oracle_synth(o, y, q, a, b):
    """synthetic_data_loss one voxel at a time: the mean over one voxel is that voxel's loss."""
    y3 = np.zeros((len(q), 3))
    y3[:, :2] = np.asarray(y, np.float64)[:, :2]
    return np.array([o.synthetic_data_loss(y3[i:i + 1], q[i:i + 1], a, b) for i in range(len(q))])


def oracle_value(o, c):
    """q [N, 5] float64 -> the case's per-voxel value from the float64 oracle's own functions."""
    if c.kernel == "synth_loss":
        if c.a * c.b > 0:
            return lambda q: oracle_synth(o, c.y, q, c.a, c.b)
        off = R.LOG_2PI if c.diagonal else 0.0
        return lambda q: o.logit_mvn_nlogp(c.y[:, :2].astype(np.float64), q) - off
    if c.kernel == "hyper_prior":
        # the inverse-gamma part of synthetic_data_loss is T(s_o) + T(s_d) at a zero fifth head: with both log-std
        # heads set to the same raw value it is 2 T of that head
        y0 = np.full((c.N, 2), [0.3, 0.05])

        def term(q, col, a, b):
            qq = np.zeros_like(q)
            qq[:, 1] = qq[:, 3] = q[:, col]
            return 0.5 * (oracle_synth(o, y0, qq, a, b) - oracle_synth(o, y0, qq, 0.0, 0.0))
        return lambda q: term(q, 1, c.ig[0], c.ig[1]) + term(q, 3, c.ig[2], c.ig[3])
    if c.kernel == "r2p_loss":
        def nll(q):
            m, v = o.moments(q, c.z.astype(np.float64))
            return 0.5 * np.log(v[:, 2]) + 0.5 * (c.y[:, 2].astype(np.float64) - m[:, 2]) ** 2 / v[:, 2]
        return nll
    if c.kernel == "kl_diag":
        return lambda q: o.kl_diag(q, c.prior.astype(np.float64))
    return lambda q: o.kl_mog(q, c.comps.astype(np.float64), c.z.astype(np.float64))


def exact_reference(c):
    """The reference with the decimal constants the float64 oracle computes with."""
    kw = dict(f32_constants=False)
    if c.kernel == "synth_loss":
        return R.synth_loss(c.y, c.q, c.a, c.b, diagonal=c.diagonal, **kw)
    if c.kernel == "hyper_prior":
        return R.hyper_prior(c.q, c.ig, **kw)
    if c.kernel == "r2p_loss":
        return R.r2p_loss(c.y[:, 2], c.q, c.z, c.dw, **kw)
    if c.kernel == "kl_diag":
        with np.errstate(invalid="ignore"):
            return R.kl_diag(c.q, c.prior, **kw)
    return R.kl_mog(c.q, c.comps, c.z, **kw)


SMALL = [(k, n) for k in cases.CASES for n in cases.CASES[k] if not n.startswith("big")]


@pytest.mark.parametrize("kernel,name", SMALL)
def test_reference_equals_the_oracle_and_its_differences(params, oracle64, kernel, name):
    """Per voxel, the reference's value equals the float64 oracle's (synthetic_data_loss one voxel at a time,
    logit_mvn_nlogp, kl_diag, kl_mog, moments for the R2' mean and variance) to 1e-11 of A_v, and every entry of its
    gradient equals five-point differences of that oracle function to 1e-6 of A_q plus the differences' own rounding --
    on base and on saturated heads."""
    c = cases.build(params, kernel, name)
    ref = exact_reference(c)
    fn = oracle_value(oracle64, c)
    q64 = c.q.astype(np.float64)
    ok = ~np.isnan(ref["v"])           # kl_diag: NaN heads in masked-out voxels
    if not ok.all():
        q64 = np.where(ok[:, None], q64, 0.0)
    rv = R.worst(fn(q64)[ok], ref["v"][ok], ref["A_v"][ok])
    out = f"{kernel} {name}: value against the oracle {rv:.2e} of A_v"
    assert rv < VAL_TOL, out
    if kernel != "kl_mog":
        g = fd_gradient(fn, q64)
        if kernel == "synth_loss" and c.diagonal:
            assert R.worst(g[:, 4], ref["g4_kernel"], ref["A4_kernel"]) < FD_TOL
            g[:, 4] = 0.0              # the trainer zeroes the column
        dead = ref["A_q"] == 0         # entries the value does not depend on: differences of equal values
        assert np.all(ref["g_q"][dead] == 0)
        g[dead] = 0.0
        # the differences' own rounding: (18 / 12) |v| 2^-52 / h, taken as 4 A_v 2^-52 / h -- at |raw| = 8 the slope is
        # 1e-6 (log-std heads) to 1e-9 (the fifth head, exp(-2) sech^2(8)) of the value and this allowance, not FD_TOL,
        # is what limits the check there
        h = np.where(np.abs(q64) >= SAT, H_SAT, H)
        err = np.abs(g - ref["g_q"])[ok]
        allowed = (FD_TOL * ref["A_q"] + 4.0 * np.finfo(np.float64).eps * ref["A_v"][:, None] / h)[ok]
        rq = R.worst(g[ok], ref["g_q"][ok], ref["A_q"][ok])
        out += f", gradient against five-point differences {rq:.2e} of A_q (worst err / allowed {np.max(err / allowed):.2f})"
        assert np.all(err <= allowed), out
    print(out)


def test_diagonal_value_is_logit_gaussian_nlogp(params, oracle64):
    """The diagonal family's value (fifth column 0, log 2 pi subtracted) is the oracle's logit_gaussian_nlogp wherever
    y_true is off the clip (that oracle function states model.py:406-421, which has no clip)."""
    for name in ("diagonal_base_N257_ld3", "diagonal_saturated_N40_ld2"):
        c = cases.build(params, "synth_loss", name)
        ref = R.synth_loss(c.y, c.q, diagonal=True, f32_constants=False)
        u = R.unit_interval(c.y, f32_constants=False)
        inner = np.all((u > 1e-6) & (u < 1.0 - 1e-6), axis=1)
        assert inner.sum() > c.N // 2
        want = oracle64.logit_gaussian_nlogp(c.y[:, :2].astype(np.float64), c.q.astype(np.float64))
        assert R.worst(want[inner], ref["v"][inner], ref["A_v"][inner]) < VAL_TOL
        assert np.all(ref["g_q"][:, 4] == 0) and np.abs(ref["g4_kernel"]).max() > 0


def test_hyper_prior_sums(params):
    """The four sums are the float64 sums of log v and 1 / v over the voxels."""
    c = cases.build(params, "hyper_prior", "saturated_N257")
    s = 3.0 * np.tanh(c.q[:, [1, 3]].astype(np.float64)) - 1.0
    want = [(2 * s[:, 0]).sum(), np.exp(-2 * s[:, 0]).sum(), (2 * s[:, 1]).sum(), np.exp(-2 * s[:, 1]).sum()]
    assert np.allclose(c.ref["sums"], want, rtol=1e-13, atol=0)


ALL = [(k, n) for k in cases.CASES for n in cases.CASES[k]]


def test_float32_floor(params):
    """The reference's own formulas in float32 NumPy (sech^2 form) against float64, on every case of the GPU test: what
    float32 alone does under the A measure.  Gradients: within a quarter of BOUND_Q, except the cases recorded in
    cases.FLOOR_Q, whose recorded floor is above a quarter of the bound and not above what is measured here.
    Values: printed, and within the bound itself -- for synth_loss (7e-6 -- 1.4e-5 against 2e-5) the floor is the rounding
    of x = (y - min) / range where 1 - x is 1e-3 (6e-5 in log(1 - x), against |log(1 - x)| = 6.9 in A_v), and for
    r2p_loss with two draws (4e-5 -- 1.1e-4 against 2e-4) the rounding of r_k - mean at var = 1e-5 mean^2."""
    floors = {}
    for kernel, name in ALL:
        c = cases.build(params, kernel, name)
        f32 = cases.evaluate(c, np.float32)
        rv, rq = cases.worst_ratios(c, f32["v"], f32.get("g_q"))
        floors[(kernel, name)] = (rv, rq)
        print(f"{kernel:12s} {name:32s} N {c.N:7d}  float32 floor: value {rv:.2e} of A_v   gradient {rq:.2e} of A_q")
    for (kernel, name), (rv, rq) in floors.items():
        assert rv < BOUND_V[kernel], (kernel, name, rv)
        if (kernel, name) in cases.FLOOR_Q:
            assert BOUND_Q / 4 < cases.FLOOR_Q[(kernel, name)] <= 1.02 * rq, (kernel, name, rq)
        else:
            assert rq < BOUND_Q / 4, (kernel, name, rq)
    for k, v in cases.FLOOR_Q.items():
        assert k in floors, k


def miss(c, defect):
    """By how many bounds the worst gradient entry of the float32 evaluation with a planted defect misses."""
    d = cases.evaluate(c, np.float32, defect)
    return cases.worst_ratios(c, d["v"], d["g_q"])[1] / cases.bound_q(c.kernel, c.name)


def test_teeth(params):
    """Planted defects, each evaluated in float32 NumPy, miss the GPU test's bound by at least 10 x on some entry of
    some case:
      (a) 1 - th^2 with th recovered from the float32 s, on the saturated cases of all four kernels;
      (b) g1 of synth_loss without w1 r0 i_bl;
      (c) the inverse-gamma g4 without 2 raw4 d / d x_d;
      (d) the R2' term with the unbiased variance;
      (e) kl_diag with exp where expm1 belongs (the -1 lost), at s_q - s_p = 1e-4 where the slope should be 2e-4;
      (f) the R2' sigmoid slope as (x - min) (1 - (x - min) / range), which is what r2p_loss_bwd_kernel had."""
    b = lambda k, n: cases.build(params, k, n)
    table = {}
    for kernel, name in (("synth_loss", "saturated_N40_ld3_off"), ("hyper_prior", "saturated_N40"),
                         ("r2p_loss", "saturated_N40_ld5_n10"), ("kl_diag", "saturated_base_N257")):
        table[f"(a) 1 - th^2, {kernel}"] = miss(b(kernel, name), "one_minus_th2")
    table["(b) g1 without w1 r0 i_bl"] = max(miss(b("synth_loss", n), "no_w1_r0_ibl")
                                             for n in ("base_N257_ld3_ig3", "saturated_N40_ld3_off"))
    table["(c) g4 without 2 raw4 d / d x_d"] = miss(b("synth_loss", "base_N257_ld3_ig3"), "no_raw4_in_ig")
    table["(d) unbiased variance"] = min(miss(b("r2p_loss", n), "unbiased_var")
                                         for n in ("base_N40_ld3_n10", "base_N40_ld3_n2"))
    c = b("kl_diag", "base_base_N40")
    d = cases.evaluate(c, np.float32, "exp_for_expm1")
    table["(e) exp for expm1 at d = 1e-4"] = R.worst(d["g_q"][36:40], c.ref["g_q"][36:40], c.ref["A_q"][36:40]) / BOUND_Q
    table["(f) sigmoid slope by difference"] = max(miss(b("r2p_loss", n), "slope_by_difference")
                                                   for n in ("saturated_N40_ld5_n10", "saturated_N40_ld5_n2_philox"))
    for k, v in table.items():
        print(f"{k:40s} misses by {v:9.1f} bounds")
    assert len(table) == 9 and min(table.values()) >= 10.0, table
    # ... and the base cases do not see (a): the gap the suite had
    for kernel, name in (("synth_loss", "base_N257_ld3_ig3"), ("hyper_prior", "base_N257"),
                         ("r2p_loss", "base_N40_ld3_n10"), ("kl_diag", "base_base_N40")):
        assert miss(b(kernel, name), "one_minus_th2") < 0.25
