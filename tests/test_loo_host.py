"""Host-side checks of PSIS leave-one-out cross-validation (qbold_loo): the C ABI entry, the float64 reference the GPU
tests hold it to (tests/_loo_reference.py), the condition those tests rest on -- every row of the reference finite for
their inputs -- and the compiler's report on loo_kernels.hip (no scratch).  No GPU needed."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _loo_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "qbold_vi_amd", "csrc", "loo_kernels.hip")


def host_normals(d, K, n=R.N_VOX):
    """the Philox stream of the importance draws from the float32 oracle (the GPU tests take qbold_normals')"""
    from oracle.oracle import Oracle
    return Oracle("f32", d["p"], **d["sw"]).philox_normals(41 + K, R.IW_STREAM, R.VOXEL0, n, K)


def reference_rows(params, case, K, seed=None):
    d = R.inputs(params, case, seed)
    with R.float64_oracle(d["p"], d["sw"]) as o64:
        return d, R.rows(o64, d["x"], d["q"], d["prior"], d["sigma"], host_normals(d, K))


def test_c_abi_declares_the_entry():
    from qbold_vi_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "qbold_hip.h")).read()
    assert "int qbold_loo(" in hdr and "int64_t qbold_loo_workspace_bytes(" in hdr
    assert re.search(r"#define QBOLD_LOO_OUT 6\b", hdr) and _lib.QBOLD_LOO_OUT == 6
    assert re.search(r"#define QBOLD_ABI_VERSION 5\b", hdr)       # additions only
    assert len(_lib.SIGNATURES["qbold_loo"][1]) == 18 and len(_lib.SIGNATURES["qbold_loo_workspace_bytes"][1]) == 3
    assert "loo_kernels.hip" in build.SOURCES
    from qbold_vi_amd.ops import Context
    assert Context.LOO_COLUMNS == ("elpd_loo", "p_loo", "lppd", "khat_max", "worst_tau", "khat_full")


@pytest.mark.parametrize("case,K", R.CASE_KS)
def test_reference_rows_are_finite_and_sum_to_the_nll(params, case, K):
    """What the GPU tests rest on: for their inputs every row of the float64 reference is finite; and the per-tau log
    densities of _ppc_reference add up to the -nll inside _iw_reference's log w."""
    from _iw_reference import log_weights
    d, r = reference_rows(params, case, K)
    assert r["ll"].shape == (R.N_VOX, d["T"], K) and r["log_ratio"].shape == (R.N_VOX, d["T"] + 1, K)
    assert np.isfinite(r["ll"]).all() and np.isfinite(r["log_ratio"]).all()
    # sum_t ll = -nll: log w + (log q - log p) recovered with a prior equal to q (log q - log p = 0)
    with R.float64_oracle(d["p"], d["sw"]) as o64:
        minus_nll, _ = log_weights(o64, d["x"], d["q"], d["q"], d["sigma"], host_normals(d, K))
    err = R.rel1(r["ll"].sum(1), minus_nll)
    print(case, K, "sum_t ll against -nll:", err)
    assert err < 1e-12


@pytest.mark.parametrize("case", list(R.CASES))
def test_input_seed_is_the_first_from_11(params, case):
    """INPUT_SEEDS: the first seed from 11 with finite rows (every smaller one fails, this one holds)."""
    K = R.CASES[case][2][0]
    for seed in range(11, R.seed_of(case)):
        _, r = reference_rows(params, case, K, seed)
        assert not (np.isfinite(r["ll"]).all() and np.isfinite(r["log_ratio"]).all()), (case, seed)
    _, r = reference_rows(params, case, K, R.seed_of(case))
    assert np.isfinite(r["log_ratio"]).all()


def test_an_uninformative_image_adds_nothing_to_p_loo(params):
    """sigma_t = 1e6 at one tau: its log density is the same for every draw, so leaving the image out changes no weight
    -- elpd_t = lppd_t there and the image adds 0 to p_loo."""
    K, t0 = 100, 7
    d = R.inputs(params, "T11")
    sigma = d["sigma"].copy()
    sigma[:, t0] = 1e6
    n = 12
    z = host_normals(d, K)[:n]
    with R.float64_oracle(d["p"], d["sw"]) as o64:
        ref = R.loo_reference(o64, d["x"][:n], d["q"][:n], d["prior"][:n], sigma[:n], z)
    pw = ref["pointwise"]
    assert np.isfinite(pw[..., [0, 2]]).all()
    assert np.max(np.abs(pw[:, t0, 0] - pw[:, t0, 2])) < 1e-9
    assert np.max(np.abs(ref["khat"][:, t0] - ref["khat"][:, -1])) < 1e-6   # the full-data row, shifted
    others = np.delete(np.arange(d["T"]), t0)
    p_loo = ref["out"][:, 1]
    assert np.max(np.abs(p_loo - (pw[:, others, 2] - pw[:, others, 0]).sum(-1))) < 1e-9
    assert np.allclose(ref["out"][:, 0], pw[..., 0].sum(-1)) and np.allclose(ref["out"][:, 2], pw[..., 2].sum(-1))


def test_finalise_columns():
    """khat_max / worst_tau: +inf wins, the lowest index among equals, and khat_full is row T's."""
    rng = np.random.default_rng(0)
    N, T, K = 3, 4, 30
    ll = rng.standard_normal((N, T, K))
    w = np.full((N, T + 1, K), -np.log(K))
    kh = np.array([[0.1, 0.9, 0.9, 0.2, 0.5], [np.inf, 0.3, np.inf, 0.1, -0.2], [-0.4, -0.1, -0.3, -0.1, 2.0]])
    f = R.finalise(ll, w, kh)
    assert f["out"][:, 3].tolist() == [0.9, np.inf, -0.1] and f["out"][:, 4].tolist() == [1.0, 0.0, 1.0]
    assert f["out"][:, 5].tolist() == [0.5, -0.2, 2.0]
    # equal weights in every row: elpd_t = lppd_t = log mean exp ll
    lme = np.log(np.exp(ll).mean(-1))
    assert np.allclose(f["pointwise"][..., 0], lme) and np.allclose(f["pointwise"][..., 2], lme)
    assert np.max(np.abs(f["out"][:, 1])) < 1e-12


# ---- the compiler's report ---------------------------------------------------------------------------------------------
def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_loo_kernels_use_no_scratch(tmp_path):
    cc = _hipcc()
    if cc is None:
        pytest.fail("hipcc not found: the ROCm toolchain is required")
    out = str(tmp_path / "loo_kernels.s")
    cmd = [cc, "-S", "--cuda-device-only", "-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-gpu-rdc",
           "-Wno-unused-function", SRC, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = open(out).read().split("\n")
    seen = {}
    for key in ("loo_rows_kernelILb1E", "loo_rows_kernelILb0E", "loo_finalise_kernel", "loo_reduce4_kernel"):
        starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l) and key in l.split(":")[0]]
        assert len(starts) == 1, (key, len(starts))
        end = next(i for i in range(starts[0], len(lines)) if "s_endpgm" in lines[i])
        res = {}
        for l in lines[end:end + 400]:
            m = re.match(r"^; (NumVgprs|ScratchSize|LDSByteSize): (\d+)", l)
            if m and m.group(1) not in res:
                res[m.group(1)] = int(m.group(2))
        seen[key] = res
        assert res["ScratchSize"] == 0, (key, res)
    print(seen)
