"""Host-side checks of the posterior calibration feature: the C ABI declaration, the float64 restatement of
qbold_calibration that the GPU tests hold the kernel to (tests/_calibration_reference.py) against a sort, scipy's normal
and chi-square CDFs, calibration.summarise on hand-made inputs, the argument checks that raise before any launch, and
the known-answer condition of the GPU test on the reference alone, and the compiler's report on
calibration_kernels.hip (no scratch, no LDS).  No GPU needed."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _calibration_reference as R

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_and_the_abi_is_still_5():
    from qbold_vi_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "qbold_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+qbold_calibration\s*\(", code)
    assert re.search(r"#define\s+QBOLD_CAL_OUT\s+6\b", code) and _lib.QBOLD_CAL_OUT == 6
    assert re.search(r"#define\s+QBOLD_CAL_MAX_L\s+\(1\s*<<\s*20\)", code) and _lib.QBOLD_CAL_MAX_L == 1 << 20
    assert re.search(r"#define\s+QBOLD_ABI_VERSION\s+5\b", code)
    args = re.search(r"qbold_calibration\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    assert len(args.split(",")) == len(_lib.SIGNATURES["qbold_calibration"][1]) == 12
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "qbold_calibration")
    assert _lib.load().qbold_abi_version() == 5


def test_reference_ranks_equal_a_sort():
    for L in (1, 2, 25, 255):
        th, q, z, _, out, _ = R.comparison_case(L)
        np.testing.assert_array_equal(out[:, 3:], R.brute_force_ranks(th, q, z))
    # ties count half: a draw placed exactly on the truth
    q = np.zeros((1, 5), np.float32)
    th = R.truths_from(q, np.zeros((1, 2)))                 # the posterior's centre
    a_t, _ = R.truth_logits(th)
    mu_o, s_o, *_ = R.transformed_heads(q)
    z = np.array([[[-1.0, 0.0], [(a_t[0] - mu_o[0]) / math.exp(s_o[0]), 0.0], [2.0, 0.0]]])
    out, _ = R.calibration(th, q, z)
    assert out[0, 3] == (2 * 1 + 1) / 6.0


def test_reference_closed_forms_equal_scipy():
    stats = pytest.importorskip("scipy.stats")
    th, q, z, _, out, _ = R.comparison_case(25)
    mu_o, s_o, mu_d, s_d, c = R.transformed_heads(q)
    a_t, b_t = R.truth_logits(th)
    np.testing.assert_allclose(out[:, 0], stats.norm.cdf(a_t, mu_o, np.exp(s_o)), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(out[:, 1], stats.norm.cdf(b_t, mu_d, np.sqrt(c * c + np.exp(2 * s_d))), rtol=1e-12,
                               atol=1e-300)
    # d^2 from the covariance itself: Sigma = L L^T, L = [[e^so, 0], [c, e^sd]]
    d2 = np.empty(len(q))
    for i in range(len(q)):
        Lq = np.array([[math.exp(s_o[i]), 0.0], [c[i], math.exp(s_d[i])]])
        r = np.array([a_t[i] - mu_o[i], b_t[i] - mu_d[i]])
        d2[i] = r @ np.linalg.solve(Lq @ Lq.T, r)
    np.testing.assert_allclose(out[:, 2], stats.chi2.cdf(d2, 2), rtol=1e-9, atol=1e-300)


def test_comparison_inputs_are_what_the_gpu_test_assumes():
    """Finite everywhere; ranks reach 0 and 1 and the clamp is reached; per statistic at most a quarter of the voxels has
    a draw within the gap of the truth (at L = 1000; the largest count there is 10)."""
    for L in R.L_CASES:
        th, q, z, _, out, near = R.comparison_case(L)
        assert np.isfinite(out).all() and out.shape == (R.N_CASE, 6)
        assert (out[:, 3:] == 0.0).any() and (out[:, 3:] == 1.0).any()
        assert np.all((near > 0).mean(0) <= 0.25), (L, (near > 0).mean(0))
        a_t, b_t = R.truth_logits(th)
        clip = math.log(1e-6) - math.log1p(-1e-6)
        assert (a_t == clip).sum() >= 10 and (b_t == clip).sum() >= 10
        assert (np.abs(a_t + clip) < 1e-9).sum() >= 10 and (np.abs(b_t + clip) < 1e-9).sum() >= 10
    for L in R.L_WEIGHTED:
        _, _, _, lw, out, near = R.comparison_case(L, True)
        assert np.isfinite(out).all() and np.isneginf(lw).any() and near.max() < 1.0


def test_reference_row_rules():
    th, q, z, lw, out, _ = R.comparison_case(25, True)
    lw = lw[:4].copy()
    lw[0, 3] = np.nan
    lw[1, 7] = np.inf
    lw[2] = -np.inf
    got, _ = R.calibration(th[:4], q[:4], z[:4], lw)
    assert np.isnan(got[:3, 3:]).all() and np.isfinite(got[3]).all()
    np.testing.assert_array_equal(got[:, :3], out[:4, :3])
    flat, _ = R.calibration(th[:4], q[:4], z[:4], np.full((4, 25), -3.5))      # a constant row: the unweighted ranks
    plain, _ = R.calibration(th[:4], q[:4], z[:4])
    np.testing.assert_allclose(flat, plain, rtol=0, atol=1e-15)
    thn = th[:4].copy()
    thn[0, 0] = np.nan
    got, _ = R.calibration(thn, q[:4], z[:4])
    assert np.isnan(got[0, [0, 2, 3, 5]]).all() and np.isfinite(got[0, [1, 4]]).all()


def _uniform_out(n, L):
    """n rows whose six columns are evenly spread: column value (i + 1/2) / n, ranks i (L + 1) // n."""
    u = (np.arange(n) + 0.5) / n
    r = (np.arange(n) * (L + 1)) // n
    return np.stack([u, u, u, r / L, r / L, r / L], 1)


def test_summarise_on_hand_made_inputs():
    from qbold_vi_amd.calibration import COLUMNS, summarise
    L, bins, n = 15, 4, 32
    out = _uniform_out(n, L)
    s = summarise(torch.as_tensor(out, dtype=torch.float32), L, bins=bins)
    assert s["n"] == n and s["dropped"] == 0 and s["levels"] == [0.5, 0.8, 0.9, 0.95] and not s["weighted"]
    for name in COLUMNS:
        st = s["stats"][name]
        assert st["hist"] == [8, 8, 8, 8] and st["chi2"] == 0.0 and st["p_value"] == 1.0
    # PIT at level 0.5: |u - 1/2| <= 1/4 holds for the 16 central values of (i + 1/2) / 32; hpd <= 0.5: the lower 16
    assert s["stats"]["pit_oef"]["coverage"][0] == 0.5 and s["stats"]["hpd"]["coverage"][0] == 0.5
    assert s["stats"]["pit_oef"]["coverage_se"][0] == math.sqrt(0.25 / n)
    # ranks: u = (r + 1/2) / 16 with every r in {0 .. 15} twice; |u - 1/2| <= 0.4 keeps r = 2 .. 13: 24 of 32
    assert s["stats"]["rank_oef"]["coverage"][1] == 24 / 32

    # a lopsided sample: everything in the lowest bin but for one row in the highest; NaN rows are dropped and counted
    out = np.full((10, 6), 0.01)
    out[:, 3:] = 0.0
    out[9] = [0.99, 0.99, 0.99, 1.0, 1.0, 1.0]
    out = np.concatenate([out, np.full((3, 6), np.nan)])
    out[11, :3] = 0.5                                     # NaN in the rank columns only: dropped as well
    s = summarise(torch.as_tensor(out, dtype=torch.float32), L, bins=bins, levels=(0.9,))
    assert s["n"] == 10 and s["dropped"] == 3
    want = ((9 - 2.5) ** 2 + 2 * 2.5 ** 2 + (1 - 2.5) ** 2) / 2.5
    stats = pytest.importorskip("scipy.stats")
    for name in COLUMNS:
        st = s["stats"][name]
        assert st["hist"] == [9, 0, 0, 1] and abs(st["chi2"] - want) < 1e-12
        assert abs(st["p_value"] - stats.chi2.sf(want, bins - 1)) < 1e-12
        assert st["coverage"] == [0.9 if name == "hpd" else 0.0]

    # weighted ranks are binned like a PIT and need no divisibility; unweighted ones do
    s = summarise(torch.as_tensor(_uniform_out(n, 16), dtype=torch.float32), 16, bins=bins, weighted=True)
    assert s["stats"]["rank_dbv"]["hist"][0] >= 7 and sum(s["stats"]["rank_dbv"]["hist"]) == n
    with pytest.raises(ValueError, match=r"\(L \+ 1\) % bins"):
        summarise(torch.zeros((4, 6)), 16, bins=bins)
    # the highest rank falls in the last bin
    top = np.ones((5, 6))
    s = summarise(torch.as_tensor(top, dtype=torch.float32), 255, bins=16)
    assert all(st["hist"] == [0] * 15 + [5] for st in s["stats"].values())
    # the table restricted to reliable k^
    khat = torch.tensor([0.1] * 16 + [0.9] * 16)
    s = summarise(torch.as_tensor(_uniform_out(n, 31), dtype=torch.float32), 31, bins=bins, weighted=True, khat=khat)
    from qbold_vi_amd.ops import psis_khat_threshold
    assert s["khat_threshold"] == psis_khat_threshold(31) and s["reliable"]["n"] == 16
    assert s["reliable"]["stats"]["pit_oef"]["hist"] == [8, 8, 0, 0]
    import json
    json.loads(json.dumps(s))


def test_fine_tuner_calibration_refuses_the_diagonal_family_and_checks_its_arguments():
    from qbold_vi_amd.model import FineTuner

    class _Tr:
        _use_mvg = False
        _heteroscedastic_noise = True
        _use_population_prior = False
        _mog_components = 1
        _seed = 1

    with pytest.raises(NotImplementedError, match="diagonal family"):
        FineTuner(_Tr(), None, None).calibration(None, None)
    _Tr._use_mvg = True
    with pytest.raises(ValueError, match="25 <= no_samples <= 1024"):
        FineTuner(_Tr(), None, None).calibration(None, None, prior=0, no_samples=24, psis=True)
    with pytest.raises(ValueError, match="needs the prior"):
        FineTuner(_Tr(), None, None).calibration(None, None, psis=True)
    _Tr._use_population_prior = True
    with pytest.raises(NotImplementedError, match="population prior"):
        FineTuner(_Tr(), None, None).calibration(None, None)


def test_known_answer_holds_for_the_reference_alone():
    """The statistical condition of test_gpu_calibration.test_known_answer on the float64 reference: calibrated truths
    give uniform columns (chi2 below the 0.999 quantile) and nominal coverage, truths from twice the spread do not."""
    from qbold_vi_amd.calibration import summarise
    summaries = {}
    for scale, (th, q, z) in R.known_answer_inputs().items():
        out, _ = R.calibration(th, q, z)
        assert np.isfinite(out).all()
        summaries[scale] = summarise(torch.as_tensor(out), R.KNOWN_L, bins=R.KNOWN_BINS)
    R.check_known_answer(summaries)


def test_calibration_kernels_use_no_scratch_and_no_lds(tmp_path):
    cc = next((c for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    if cc is None:
        pytest.fail("hipcc not found: the ROCm toolchain is required")
    out = str(tmp_path / "calibration_kernels.s")
    src = os.path.join(ROOT, "qbold_vi_amd", "csrc", "calibration_kernels.hip")
    r = subprocess.run([cc, "-S", "--cuda-device-only", "-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-gpu-rdc",
                        "-Wno-unused-function", src, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = open(out).read().split("\n")
    seen = {}
    for key in ("calibration_kernelILb0ELb0E", "calibration_kernelILb0ELb1E", "calibration_kernelILb1ELb0E",
                "calibration_kernelILb1ELb1E"):
        starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l) and key in l.split(":")[0]]
        assert len(starts) == 1, (key, len(starts))
        end = next(i for i in range(starts[0], len(lines)) if "s_endpgm" in lines[i])
        res = {}
        for l in lines[end:end + 400]:
            m = re.match(r"^; (NumVgprs|ScratchSize|LDSByteSize): (\d+)", l)
            if m and m.group(1) not in res:
                res[m.group(1)] = int(m.group(2))
        seen[key] = res
        assert res["ScratchSize"] == 0 and res["LDSByteSize"] == 0, (key, res)
    print(seen)
