"""Host-side checks of the refinement on any tau grid (qbold_refine_posterior_anyt,
qbold_refine_posterior_spatial_anyt): the C ABI carries the two entries, Context's argument checks raise before any
launch on a 33-tau host context, and the float64 restatement the GPU tests compare against
(tests/_refine_reference.py) agrees with central differences of the float64 oracle's NLL + exact KL on every protocol
of the table -- the precondition of tests/test_gpu_refine_anyt.py, whose cases it shares.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import _refine_anyt_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_the_two_entries():
    from qbold_vi_amd import _lib
    with open(os.path.join(ROOT, "include", "qbold_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"#define QBOLD_ABI_VERSION 5\b", hdr)       # additions only
    for name, nargs in (("qbold_refine_posterior", 16), ("qbold_refine_posterior_spatial", 18)):
        assert f"int {name}_anyt(" in hdr
        res, args = _lib.SIGNATURES[name + "_anyt"]
        old_res, old_args = _lib.SIGNATURES[name]
        assert len(args) == nargs and res is old_res and list(args) == list(old_args)   # the existing argument lists
    assert "which are unchanged" in hdr and "Traffic per voxel" in hdr
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    assert "qbold_refine_posterior_anyt" in doc and "qbold_refine_posterior_spatial_anyt" in doc


def test_the_kernels_are_in_the_build():
    """the two run-time-T kernels are HIP in a translation unit of the build, beside the entries that launch them"""
    from qbold_vi_amd import build
    text = ""
    for src in build.SOURCES:
        if src.startswith("refine"):
            with open(os.path.join(build.CSRC, src)) as f:
                text += f.read()
    for name in ("refine_generic_kernel", "refine_tv_step_generic_kernel"):
        assert re.search(r"__global__[^;{]*\b" + name + r"\(", text), name
    for name in ("qbold_refine_posterior_anyt", "qbold_refine_posterior_spatial_anyt"):
        assert re.search(r'extern "C" int ' + name + r"\(", text), name


@pytest.fixture(scope="module")
def host33(params):
    from qbold_vi_amd.ops import Context
    import test_gpu_forward_protocols as fp
    c = Context(fp.protocol(params, "odd33"), host_only=True)
    assert c.T == 33
    return c


@pytest.mark.parametrize("kw,err", [
    (dict(steps=0), ValueError), (dict(S=0), ValueError), (dict(lr=0.0), ValueError), (dict(lr=-1.0), ValueError),
    (dict(lr_final=-0.1), ValueError), (dict(optimizer="rmsprop"), ValueError),
    (dict(steps=1 << 31, S=5), ValueError), (dict(kernel="fast"), ValueError),
])
def test_context_checks_arguments_before_launch_at_33_taus(host33, kw, err):
    torch = pytest.importorskip("torch")
    t = torch.zeros((4, 33))
    q = torch.zeros((4, 5))
    with pytest.raises(err):
        host33.refine_posterior(t, None, q, q, t, **kw)
    t5, q5 = t.reshape(1, 2, 2, 1, 33), q.reshape(1, 2, 2, 1, 5)
    with pytest.raises(err):
        host33.refine_posterior_spatial(t5, None, q5, q5, t5, 5.0, **kw)


def test_context_needs_device_tensors_and_the_grids_columns(host33):
    torch = pytest.importorskip("torch")
    from qbold_vi_amd._lib import QboldError
    t = torch.zeros((4, 33))
    q = torch.zeros((4, 5))
    for kernel in ("auto", "generic"):
        with pytest.raises(QboldError, match="no CPU fallback"):
            host33.refine_posterior(t, None, q, q, t, kernel=kernel)
    with pytest.raises(ValueError, match="tv_weight"):
        host33.refine_posterior_spatial(t.reshape(1, 2, 2, 1, 33), None, q.reshape(1, 2, 2, 1, 5),
                                        q.reshape(1, 2, 2, 1, 5), t.reshape(1, 2, 2, 1, 33), -1.0)


def test_dispatch_keeps_the_specialised_entries_at_11_and_24_taus(params):
    """kernel="auto": the existing entries at the reference's 11 / 24 taus (their bits are pinned by the existing
    tests), the any-T ones elsewhere; kernel="generic": the any-T ones everywhere"""
    from qbold_vi_amd.ops import Context
    import _laplace_reference as lr
    for name, T in (("ref11", 11), ("ref24", 24), ("odd33", 33), ("full64", 64), ("two", 2)):
        c = Context(lr.setup(params, name)[0], host_only=True)
        assert c.T == T
        for base in ("qbold_refine_posterior", "qbold_refine_posterior_spatial"):
            assert c._refine_entry("refine", "auto", base) == (base if T in (11, 24) else base + "_anyt")
            assert c._refine_entry("refine", "generic", base) == base + "_anyt"


@pytest.mark.parametrize("name", rc.GRAD_CASES)
def test_reference_gradient_matches_finite_differences(params, name):
    """step_grad against central differences of Oracle("f64").elbo's NLL over the same explicit normals plus the exact
    KL, per head, on the 48 voxels and 3 draws of the GPU test, below the existing tests' 1e-6 of the column's scale."""
    g = rc.gradient_reference(params, name)
    assert g["ref"].shape == (48, 5) and np.all(np.isfinite(g["fd"]))
    for k in range(5):
        err = np.max(np.abs(g["ref"][:, k] - g["fd"][:, k])) / rc.fd_scale(g["fd"], k)
        print(name, k, "scale", rc.fd_scale(g["fd"], k), "ref-vs-fd", err)
        assert err < rc.FD_PRECONDITION, (name, k, err)
