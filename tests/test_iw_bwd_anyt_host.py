"""Host-side checks of the importance-weighted backward on any tau grid (qbold_log_evidence_bwd_anyt,
Context.log_evidence_bwd(kernel=...)): the C ABI carries the entry with qbold_log_evidence_bwd's argument list, the
kernel and the entry are in the build, Context chooses between the two entries as the refinements do, and the float64
reference the GPU tests compare against (tests/_iw_grad_reference.py) agrees with central differences of the float64
oracle on every protocol of tests/test_gpu_forward_protocols.py -- the precondition of tests/test_gpu_iw_grad_anyt.py,
whose inputs it shares.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import _refine_anyt_cases as rc
import test_gpu_forward_protocols as fp
from _iw_grad_reference import frozen_log_weights, iw_grad_reference, neg_log_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "qbold_log_evidence_bwd"
N_CASE, N_LIVE, K = 48, 6, 7   # the GPU file's 48 voxels; six of its live ones here


def test_abi_declares_the_entry():
    from qbold_vi_amd import _lib
    with open(os.path.join(ROOT, "include", "qbold_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"#define QBOLD_ABI_VERSION 5\b", hdr)       # additions only
    assert f"int {ENTRY}_anyt(" in hdr and f"int {ENTRY}(" in hdr
    res, args = _lib.SIGNATURES[ENTRY + "_anyt"]
    old_res, old_args = _lib.SIGNATURES[ENTRY]
    assert len(args) == 17 and res is old_res and list(args) == list(old_args)
    # the declaration's own argument list is the existing entry's, name for name
    decl = {n: re.search(r"int " + n + r"\(([^;]*)\);", hdr).group(1).split() for n in (ENTRY, ENTRY + "_anyt")}
    assert decl[ENTRY] == decl[ENTRY + "_anyt"]
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert ENTRY + "_anyt" in f.read()


def test_the_kernel_is_in_the_build():
    """the run-time-T kernel is HIP in a translation unit of the build, beside the entry that launches it"""
    from qbold_vi_amd import build
    text = ""
    for src in build.SOURCES:
        with open(os.path.join(build.CSRC, src)) as f:
            text += f.read()
    assert re.search(r"__global__[^;{]*\biw_bwd_generic_kernel\(", text)
    assert re.search(r'extern "C" int ' + ENTRY + r"_anyt\(", text)
    assert re.search(r"hipLaunchKernelGGL\(kern\b", text) and "iw_bwd_generic_kernel<1>" in text


def test_dispatch_keeps_the_specialised_entry_at_11_and_24_taus(params):
    """kernel="auto": the existing entry at the reference's 11 / 24 taus (its bits are pinned by the existing tests),
    the any-T one elsewhere; kernel="generic": the any-T one everywhere"""
    from qbold_vi_amd.ops import Context
    import _laplace_reference as lr
    for name, T in (("ref11", 11), ("ref24", 24), ("odd33", 33), ("full64", 64), ("two", 2)):
        c = Context(lr.setup(params, name)[0], host_only=True)
        assert c.T == T
        assert c._log_evidence_bwd_entry("auto") == (ENTRY if T in (11, 24) else ENTRY + "_anyt")
        assert c._log_evidence_bwd_entry("generic") == ENTRY + "_anyt"


@pytest.fixture(scope="module")
def host33(params):
    from qbold_vi_amd.ops import Context
    c = Context(fp.protocol(params, "odd33"), host_only=True)
    assert c.T == 33
    return c


def test_unknown_kernel_raises_before_any_launch(host33):
    torch = pytest.importorskip("torch")
    t, q = torch.zeros((4, 33)), torch.zeros((4, 5))
    for bad in ("fast", "specialised", None):
        with pytest.raises(ValueError, match="kernel must be"):
            host33.log_evidence_bwd(t, None, q, q, t, 4, kernel=bad)


def test_cpu_tensors_have_no_fallback(host33):
    torch = pytest.importorskip("torch")
    from qbold_vi_amd._lib import QboldError
    t, q = torch.zeros((4, 33)), torch.zeros((4, 5))
    for kernel in ("auto", "generic"):
        with pytest.raises(QboldError, match="no CPU fallback"):
            host33.log_evidence_bwd(t, None, q, q, t, 4, kernel=kernel)


# ---- the float64 reference on every protocol: test_iw_grad_host.py's two central-difference checks, its bounds -------
_LIVE = {}


def live_inputs(params, name):
    """(case dict, x, q, prior, sigma as float64) of the first six live voxels of the GPU file's 48"""
    if name not in _LIVE:
        d = rc.case(params, name, N_CASE)
        idx = np.flatnonzero(d["live"])[:N_LIVE]
        assert idx.size == N_LIVE
        _LIVE[name] = (d,) + tuple(np.asarray(d[k][idx], np.float64) for k in ("x", "q", "prior", "sigma"))
    return _LIVE[name]


@pytest.mark.parametrize("name", list(fp.PROTOCOLS))
def test_sigma_gradient_is_the_derivative_of_log_p(params, name):
    """g_log_sigma = d(-log p^_K) / d log sigma with eps fixed, per voxel and tau, by central differences: < 1e-6"""
    d, x, q, prior, sigma = live_inputs(params, name)
    T = x.shape[1]
    z = np.random.default_rng(6).standard_normal((N_LIVE, K, 2))
    with rc.float64_oracle(d) as o64:
        ref = iw_grad_reference(o64, x, q, prior, sigma, z)
        ls = np.log(sigma)
        h = 1e-6
        fd = np.empty((N_LIVE, T))
        for t in range(T):
            dd = np.zeros_like(ls)
            dd[:, t] = h
            fd[:, t] = (neg_log_p(o64, x, q, prior, np.exp(ls + dd), z) -
                        neg_log_p(o64, x, q, prior, np.exp(ls - dd), z)) / (2 * h)
    scale = np.abs(fd).max()
    err = np.abs(ref["g_log_sigma"] - fd).max() / scale
    print(name, "sigma: ref-vs-fd", err, "scale", scale)
    assert err < 1e-6, (name, err, scale)


@pytest.mark.parametrize("name", list(fp.PROTOCOLS))
def test_dreg_is_the_gradient_of_the_squared_weight_surrogate(params, name):
    """g_q = -d/dq sum_k stop(w~_k^2) f_k(q), f_k = log w_k with log q's parameters frozen: < 1e-5 per column"""
    d, x, q, prior, sigma = live_inputs(params, name)
    z = np.random.default_rng(7).standard_normal((N_LIVE, K, 2))
    with rc.float64_oracle(d) as o64:
        ref = iw_grad_reference(o64, x, q, prior, sigma, z)
        w2 = ref["w"] ** 2
        h = 1e-5
        for k in range(5):
            dd = np.zeros_like(q)
            dd[:, k] = h
            fd = -((w2 * frozen_log_weights(o64, x, q + dd, q, prior, sigma, z)).sum(1) -
                   (w2 * frozen_log_weights(o64, x, q - dd, q, prior, sigma, z)).sum(1)) / (2 * h)
            scale = np.abs(fd).max() + 1e-3
            err = np.abs(ref["g_q"][:, k] - fd).max() / scale
            print(name, "DReG column", k, "ref-vs-fd", err, "scale", scale)
            assert err < 1e-5, (name, k, err, scale)
