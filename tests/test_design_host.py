"""The float64 reference of the information entries (tests/_design_reference.py) held to independent computations, the
float32 floor of every case of tests/test_gpu_design.py, and the header's text.  No GPU."""
import os
import re

import numpy as np
import pytest

import _design_cases as cases
import _design_reference as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(cases.CASES))
def test_float32_floor(params, name):
    """The same composition on the float32 oracle's primitives with float32 accumulation, against float64, in the GPU
    test's measure: the recorded floor of the case is the one measured here (to 2 %), so the GPU test's bound of
    4 x FLOOR comes from float32 alone."""
    c = cases.build(params, name)
    f32 = dr.reference(c.o32, c.theta, c.sigma, c.weights, c.prior, c.multi, dtype=np.float32)
    m = cases.measures(f32, c.ref)
    worst = cases.groups(m)
    print(f'    "{name}": ({worst[0]:.3e}, {worst[1]:.3e}, {worst[2]:.3e}),   #',
          " ".join(f"{k}={v:.2e}" for k, v in m.items()))
    flagged = np.array_equal(f32["singular"], c.ref["singular"])
    assert flagged, "float32 and float64 disagree on which informations are singular"
    assert name in cases.FLOOR
    for got, kept in zip(worst, cases.FLOOR[name]):
        assert 0.98 * kept <= got <= 1.02 * kept, (name, worst, cases.FLOOR[name])


@pytest.mark.parametrize("name", ("t11_N257", "t12_multi_N40", "t22_N40", "t33_multi_N40"))
def test_rows_are_the_laplace_models_and_the_slope_of_yhat(params, name):
    """I + Lambda at unit weights is _laplace_reference.Model.evaluate's A at the points' logits, and the rows are the
    central differences of yhat on the logit plane."""
    c = cases.build(params, name)
    with cases.float64_oracle(c.p, c.sw) as o64:
        u = dr.logits(c.theta)
        A = dr.model_of(o64, c.theta, c.sigma, c.prior, c.multi).evaluate(u)["A"]
        j, d, _ = dr.rows(o64, c.theta, c.multi)
        win = slice(o64.se_idx - 1, o64.se_idx + 2) if c.multi else slice(o64.se_idx, o64.se_idx + 1)

        def yhat(uu):
            s = 1.0 / (1.0 + np.exp(-uu))
            sig = np.asarray(o64.signal_fwd(np.stack([0.8 * s[:, 0] + 0.04, 0.2 * s[:, 1] + 0.001], -1)), np.float64)
            return sig / (sig[:, win].mean(1, keepdims=True) + 1e-3)
        h = 1e-4   # the oracle's Bessel sums are smooth to ~1e-13 only: a smaller step differentiates their noise
        fd = np.stack([(yhat(u + h * e) - yhat(u - h * e)) / (2 * h) for e in (np.array([1.0, 0]), np.array([0, 1.0]))],
                      -1)
    assert np.max(np.abs(A - c.ref1["A"][0]) / np.abs(A).max((1, 2), keepdims=True)) <= 1e-12
    # 1e-13 of noise in yhat over 2 h is 5e-10 of slope: it counts against the rows of the points 1e-4 from a range end
    # (slopes ~1e-5), so the scale carries an absolute 1e-3
    scale = np.abs(j).max(1, keepdims=True) + 1e-3
    assert np.max(np.abs(fd - j) / scale) <= 1e-6, np.max(np.abs(fd - j) / scale)
    # I against the central differences, to the absolute-sum scale
    sg = np.broadcast_to(c.sigma.astype(np.float64).reshape(-1, c.T), (c.N, c.T))
    I_fd = np.einsum("ntk,ntl->nkl", fd / sg[:, :, None], fd / sg[:, :, None])
    I = c.ref1["I"][0]
    assert np.max(np.abs(I_fd - I).max((1, 2)) / np.abs(I).sum((1, 2))) <= 1e-5


def test_bounds_against_numpy_inverse_and_scores_against_a_loop(params):
    c = cases.build(params, cases.DEFAULT_CASE)
    r = c.ref
    Sigma = np.linalg.inv(r["A"])
    assert np.allclose(r["bound"][..., 0], r["d"][:, 0] * np.sqrt(Sigma[..., 0, 0]), rtol=1e-10)
    assert np.allclose(r["bound"][..., 1], r["d"][:, 1] * np.sqrt(Sigma[..., 1, 1]), rtol=1e-10)
    assert np.allclose(r["bound"][..., 2], np.sqrt(np.einsum("ni,bnij,nj->bn", r["gr2"], Sigma, r["gr2"])), rtol=1e-9)
    assert np.allclose(r["bound"][..., 3], Sigma[..., 0, 1] / np.sqrt(Sigma[..., 0, 0] * Sigma[..., 1, 1]), rtol=1e-9,
                       atol=1e-12)
    assert np.allclose(r["log_det_A"], np.log(np.linalg.det(r["A"])), rtol=1e-12)
    ok = ~r["singular"]
    Ci = np.linalg.inv(r["I"][ok])
    assert np.allclose(r["crlb"][ok][:, 0], np.broadcast_to(r["d"][:, 0], ok.shape)[ok] * np.sqrt(Ci[:, 0, 0]), rtol=1e-8)
    # design 3 has one non-zero tau: its data part is rank 1, with the prior it is fine
    assert r["singular"][3].all() and np.all(np.isfinite(r["log_det_A"][3])) and not r["singular"][0].any()
    # the weights are averages: w on sigma is ones on sigma / sqrt(w) (zeros aside)
    with cases.float64_oracle(c.p, c.sw) as o64:
        w = c.weights[1].astype(np.float64)
        alt = dr.reference(o64, c.theta, c.sigma.astype(np.float64) / np.sqrt(w), None, c.prior, c.multi)
    assert np.allclose(alt["I"][0], r["I"][1], rtol=1e-12)
    got = dr.scores(r, c.mask)
    want = np.zeros((cases.B_ALL, 5))
    for b in range(cases.B_ALL):
        for n in range(c.N):
            if c.mask[n] > 0:
                want[b, 0] += c.mask[n] * r["log_det_A"][b, n]
                want[b, 1:4] += c.mask[n] * r["var"][b, n]
                want[b, 4] += c.mask[n]
    assert np.allclose(got, want, rtol=1e-13)


def test_t1_is_exactly_singular(params):
    c = cases.build(params, "t1_N40")
    assert c.ref["singular"].all() and c.ref1["singular"].all()
    assert np.all(np.isneginf(c.ref1["log_det"])) and np.all(np.isposinf(c.ref1["crlb"][..., :3]))
    assert np.all(np.isnan(c.ref1["crlb"][..., 3])) and np.all(np.isfinite(c.ref1["bound"]))


def test_cases_cover_what_they_claim(params):
    Ts = {v[0] for v in cases.CASES.values()}
    assert Ts == {1, 11, 12, 22, 24, 33, 64}
    for T in Ts - {1}:
        assert {v[1] for v in cases.CASES.values() if v[0] == T} == {False, True}
    assert {v[2] for v in cases.CASES.values()} == {40, 257}
    assert {v[3] for v in cases.CASES.values()} == {False, True}
    from oracle.oracle import Oracle
    o = Oracle("f32", cases.case_protocol(params, 12))
    assert o.T == 12 and o.se_idx == 10 and np.max(np.abs(o.taus)) <= 0.0101
    o = Oracle("f32", cases.case_protocol(params, 22))
    assert o.T == 22 and np.min(np.abs(o.taus)) > 5e-4
    c = cases.inputs(cases.DEFAULT_CASE)
    assert dr.in_range(c.theta).all()
    assert abs(float(c.theta[0, 0]) - 0.0401) < 1e-6 and abs(float(c.theta[3, 1]) - 0.2009) < 1e-6
    assert set(np.unique(c.mask)) == {0.0, 0.5, 1.0}
    w = c.weights
    assert (w[0] == 1).all() and (w[3] > 0).sum() == 1 and (w[2] == 0).any() and (w[1] == np.round(w[1])).all()


def test_header_declares_the_entries_at_abi_5():
    hdr = open(os.path.join(ROOT, "include", "qbold_hip.h")).read()
    assert re.search(r"#define QBOLD_ABI_VERSION 5\b", hdr)
    assert re.search(r"#define QBOLD_FISHER_OUT 15\b", hdr) and re.search(r"#define QBOLD_DESIGN_OUT 5\b", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("qbold_fisher_information", "qbold_design_workspace_bytes", "qbold_design_scores"):
        assert re.search(r"\b" + name + r"\s*\(", code), name
    from qbold_vi_amd import _lib
    assert _lib.QBOLD_FISHER_OUT == 15 and _lib.QBOLD_DESIGN_OUT == 5
    for name in ("qbold_fisher_information", "qbold_design_workspace_bytes", "qbold_design_scores"):
        assert name in _lib.SIGNATURES
