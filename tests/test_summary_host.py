"""The float64 reference of qbold_draw_summary (tests/_summary_reference.py) against numpy and against its own
definitions, and the condition on the comparison's rows: the sandwich between the levels p -+ eps must pin the kernel's
value in nearly every case, or it would hide a failure.  No GPU."""
import os
import re

import numpy as np
import pytest

import _summary_reference as R

# K -> the least share of (row, column, level) cases with q_ref(p - eps) == q_ref(p + eps), for every K of the GPU
# comparison (tests/test_gpu_summary.py runs exactly these).  A level is loose when a W_r falls within eps of it, about
# 2 eps K = K^2 / 2^22 of the cases: 1e-5 - 0.012 up to K = 225 (limit 0.95), 0.24 at K >= 1000 (limit 0.8), and 0.06
# at K = 500, where 0.9 leaves the same factor of about one and a half on the expected loose share.
TIGHT_LIMITS = {4: 0.95, 25: 0.95, 64: 0.95, 65: 0.95, 100: 0.95, 225: 0.95, 500: 0.9, 1000: 0.8, 1024: 0.8}
# ... and of (row, column) cases in which hpd_ref(mass - eps) and hpd_ref(mass + eps) are the same pair.  The pair moves
# when a W_r falls within eps of the mass of the best pair or of a rival of nearly its width, a few times as often as a
# level is loose: 0.95 up to K = 225, 0.75 at K = 500 and one half at K >= 1000 leave room for a factor of two to four
# on K^2 / 2^22 and still fail on rows that pin nothing.
HPD_TIGHT_LIMITS = {4: 0.95, 25: 0.95, 64: 0.95, 65: 0.95, 100: 0.95, 225: 0.95, 500: 0.75, 1000: 0.5, 1024: 0.5}
KS = tuple(sorted(TIGHT_LIMITS))


@pytest.mark.parametrize("K", (8, 25, 100, 1000))
def test_equal_weights_are_numpys_inverted_cdf(K):
    rng = np.random.default_rng(K)
    theta = rng.uniform(0.5, 1.5, K).astype(np.float32).astype(np.float64)
    w = np.full(K, 1.0 / K)
    for p in (0.0251, 0.1003, 0.3337, 0.5009, 0.7493, 0.9751):      # no multiple of 1 / K: no W_r sits on a level
        assert abs(p * K - round(p * K)) > 1e-3
        assert R.q_ref(theta, w, p) == np.quantile(theta, p, method="inverted_cdf")
    assert np.array_equal(R.weights(np.full(K, -3.0)), w)


def test_hpd_collapses_on_a_dominant_weight():
    K = 50
    rng = np.random.default_rng(1)
    theta = rng.uniform(0.5, 1.5, K)
    lw = rng.standard_normal(K)
    lw[17] += 12.0
    w = R.weights(lw)
    assert w[17] > 0.96
    assert R.hpd_ref(theta, w, 0.95) == (theta[17], theta[17])
    assert R.q_ref(theta, w, 0.5) == theta[17]


def test_hpd_rule_on_a_small_row():
    theta = np.array([0.0, 1.0, 1.5, 4.0, 4.2])
    w = np.array([0.1, 0.3, 0.3, 0.2, 0.1])
    assert R.hpd_ref(theta, w, 0.55) == (1.0, 1.5)                  # 0.6 in a width of 0.5
    assert R.hpd_ref(theta, w, 0.65) == (0.0, 1.5)                  # [0, 1.5] = 0.7 beats [1, 4] = 0.8 in width
    assert R.hpd_ref(theta, np.full(5, 0.2), 0.35) == (4.0, 4.2)    # two draws each: the closest pair
    assert R.hpd_ref(np.array([0.0, 1.0, 2.0, 3.0]), np.full(4, 0.25), 0.45) == (0.0, 1.0)   # ties: the smallest a
    assert R.q_ref(theta, w, 0.1 - 1e-9) == 0.0 and R.q_ref(theta, w, 0.1 + 1e-9) == 1.0
    assert R.q_ref(theta, w, 1.0 - 1e-12) == 4.2


def test_outputs_are_invariant_under_a_permutation_of_the_draws():
    K = 100
    lw, theta = R.make_rows(K)
    rng = np.random.default_rng(3)
    for i in (0, 1, 100, 239):
        perm = rng.permutation(K)
        w, th = R.weights(lw[i]), theta[i].astype(np.float64)
        th[::7, 1] = th[0, 1]                                        # ties
        wp, tp = R.weights(lw[i][perm]), th[perm]
        for c in range(3):
            for p in R.LEVELS:
                assert R.q_ref(th[:, c], w, p) == R.q_ref(tp[:, c], wp, p)
            assert R.hpd_ref(th[:, c], w, R.MASS) == R.hpd_ref(tp[:, c], wp, R.MASS)
        a, b = R.moments(th, w), R.moments(tp, wp)
        for k in a:
            assert np.allclose(a[k], b[k], rtol=1e-12, atol=0), k


@pytest.mark.parametrize("K", KS)
def test_the_sandwich_is_tight_on_the_comparison_rows(K):
    r = R.reference(K)
    assert r["lw"].shape == (240, K) and r["theta"].shape == (240, K, 3)
    assert np.all(r["q_lo"] <= r["q_hi"])
    tight = float(np.mean(r["q_lo"] == r["q_hi"]))
    hpd = float(np.mean(np.all(r["hpd_lo"] == r["hpd_hi"], -1)))
    print(f"K={K} eps={R.eps(K):.3e} tight quantiles {tight:.4f} tight hpd {hpd:.4f} "
          f"ess in [{r['ess'].min():.1f}, {r['ess'].max():.1f}]")
    assert tight >= TIGHT_LIMITS[K], (K, tight)
    assert hpd >= HPD_TIGHT_LIMITS[K], (K, hpd)
    wa = (r["hpd_lo"][..., 1] - r["hpd_lo"][..., 0]), (r["hpd_hi"][..., 1] - r["hpd_hi"][..., 0])
    assert np.all(wa[0] <= wa[1])                                    # a larger mass never has a shorter interval


def test_c_abi_declares_the_entry():
    from qbold_vi_amd import _lib
    from qbold_vi_amd.build import SOURCES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "qbold_hip.h")).read()
    assert "int qbold_draw_summary(" in hdr
    for name, value in (("MIN_K", 4), ("MAX_K", 1024), ("MAX_C", 8), ("MAX_P", 8)):
        assert re.search(rf"#define QBOLD_SUMMARY_{name} {value}\b", hdr)
        assert getattr(_lib, "QBOLD_SUMMARY_" + name) == value
    assert re.search(r"#define QBOLD_ABI_VERSION 5\b", hdr)       # additions only
    res, args = _lib.SIGNATURES["qbold_draw_summary"]
    assert len(args) == 15
    proto = re.search(r"int qbold_draw_summary\((.*?)\);", hdr, re.S).group(1)
    assert len(proto.split(",")) == 15
    assert "summary_kernels.hip" in SOURCES
