"""Host-side checks of the float64 reference the GPU tests hold qbold_psis to (tests/_psis_reference.py), the C ABI
entries and the threshold helper.  No GPU needed."""
import math
import os
import re

import numpy as np
import pytest

import _psis_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (25, 64, 100, 225, 1000, 1024)


def test_tail_sizes():
    assert [R.tail_size(K) for K in KS] == [5, 13, 20, 45, 95, 96]
    assert max(R.tail_size(K) for K in range(25, 1025)) == 96      # the kernel's tail buffers


@pytest.mark.parametrize("K", KS)
def test_literal_and_expm1_forms_agree(K):
    """The kernel's fit scale y = expm1(x - c) against the paper's exp(x) - exp(c): k^ is invariant to the factor."""
    rows = R.make_rows(K)
    a, b = R.psis(rows), R.psis(rows, form="expm1")
    assert np.all(np.isfinite(a["out"])) and np.all(np.isfinite(b["out"]))
    assert np.array_equal(a["out"][:, 3], b["out"][:, 3])
    assert np.max(np.abs(a["out"][:, :3] - b["out"][:, :3]) / (1.0 + np.abs(a["out"][:, :3]))) < 1e-10
    assert np.max(np.abs(a["weights"] - b["weights"])) < 1e-10


def test_generator_covers_the_regimes():
    """What the GPU comparison relies on: finite k^ on both sides of every threshold, cutoffs far from the -c > 80
    rule, and rows with duplicated float32 values (the tie rule)."""
    kh, c, dup, rows = [], [], 0, 0
    for K in KS:
        lw = R.make_rows(K)
        ref = R.psis(lw)
        kh.append(ref["out"][:, 0])
        c.append(ref["c"])
        dup += sum(len(np.unique(r)) < K for r in lw)
        rows += lw.shape[0]
    kh, c = np.concatenate(kh), np.concatenate(c)
    assert rows == 6 * 240 and np.all(np.isfinite(kh))
    assert kh.min() < -0.3 and kh.max() > 3.5
    assert 0.4 < np.mean(kh > 0.7) < 0.55
    assert np.max(-c) < 40.0
    assert 0.05 < dup / rows < 0.2


def test_khat_is_invariant_to_shift_and_permutation():
    rng = np.random.default_rng(3)
    lw = R.make_rows(100)[::7].astype(np.float64)
    ref = R.psis(lw)
    sh = R.psis(lw + 123.25)       # exact in float64 for these values' exponents: x is unchanged
    assert np.allclose(sh["out"][:, 0], ref["out"][:, 0], rtol=0, atol=1e-9)
    assert np.allclose(sh["out"][:, 1], ref["out"][:, 1] + 123.25, rtol=0, atol=1e-9)
    perm = rng.permutation(lw.shape[1])
    pm = R.psis(lw[:, perm])
    assert np.array_equal(pm["out"][:, 3], ref["out"][:, 3])
    assert np.allclose(pm["out"][:, :3], ref["out"][:, :3], rtol=1e-12, atol=1e-12)
    assert np.allclose(pm["weights"], ref["weights"][:, perm], rtol=0, atol=1e-12)
    # the tie rule: equal tail values take their ranks in draw order, so a permutation moves the smoothed values
    # between the tied draws and nothing else -- the sorted weights, and so every estimate, stay
    row = lw[0].copy()
    top = np.argsort(row)[-3:]
    row[top[0]] = row[top[1]]
    a, b = R.psis_row(row), R.psis_row(row[perm])
    assert a["n"] == b["n"] and abs(a["khat"] - b["khat"]) < 1e-12
    assert np.allclose(np.sort(a["weights"]), np.sort(b["weights"]), rtol=0, atol=1e-12)
    lo, hi = sorted((top[0], top[1]))
    assert a["weights"][lo] < a["weights"][hi]      # the earlier draw has the lower rank


@pytest.mark.parametrize("k", [0.0, 0.5, 1.0])
def test_exact_generalised_pareto_rows(k):
    """Weights that are the exact GPD(k) quantiles at the K mid-point levels (no sampling error), in a scrambled order:
    the part of a GPD above any cutoff is a GPD of the same shape."""
    K = 1000
    l1 = np.log1p(-(np.arange(1, K + 1) - 0.5) / K)
    w = -l1 if k == 0.0 else np.expm1(-k * l1) / k
    r = R.psis_row(np.log(w)[np.random.default_rng(7).permutation(K)])
    print(k, r["khat"], r["n"])
    assert r["n"] == R.tail_size(K) and abs(r["khat"] - k) < 0.25, r["khat"]


def test_all_equal_row():
    r = R.psis_row(np.full(64, -3.5))
    assert r["n"] == 0 and r["khat"] == float("inf")
    assert np.allclose(r["weights"], -math.log(64), rtol=0, atol=1e-15)
    assert abs(r["log_p"] + 3.5) < 1e-14 and abs(r["ess"] - 64) < 1e-10
    # the top M + 1 values equal: every tail candidate ties with the cutoff
    lw = np.linspace(-9.0, -5.0, 64)
    lw[-14:] = -1.0
    assert R.psis_row(lw)["n"] == 0
    assert np.isnan(R.psis_row(np.r_[np.nan, np.zeros(30)])["khat"])


def test_threshold_helper():
    from qbold_vi_amd.ops import psis_khat_threshold
    assert psis_khat_threshold(100) == 0.5 and psis_khat_threshold(10 ** 4) == 0.7
    assert psis_khat_threshold(2154) < 0.7 and psis_khat_threshold(2155) == 0.7      # 10^(1 / 0.3) = 2154.4
    assert abs(psis_khat_threshold(25) - (1 - 1 / math.log10(25))) < 1e-15
    assert abs(psis_khat_threshold(1000) - 2.0 / 3.0) < 1e-15
    for K in KS:
        assert psis_khat_threshold(K) == R.khat_threshold(K)
    with pytest.raises(ValueError):
        psis_khat_threshold(1)


def test_c_abi_declares_the_entries():
    from qbold_vi_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "qbold_hip.h")).read()
    assert "int qbold_psis(" in hdr and "int qbold_log_evidence_draws(" in hdr
    assert re.search(r"#define QBOLD_PSIS_MIN_K 25\b", hdr) and re.search(r"#define QBOLD_PSIS_MAX_K 1024\b", hdr)
    assert re.search(r"#define QBOLD_ABI_VERSION 5\b", hdr)       # additions only
    assert (_lib.QBOLD_PSIS_MIN_K, _lib.QBOLD_PSIS_MAX_K, _lib.QBOLD_PSIS_MAX_C) == (25, 1024, 8)
    res, args = _lib.SIGNATURES["qbold_psis"]
    assert len(args) == 11
    res, args = _lib.SIGNATURES["qbold_log_evidence_draws"]
    assert len(args) == 14
