"""The cases of the any-T refinement tests (tests/test_refine_anyt_host.py, tests/test_gpu_refine_anyt.py): the
protocol table -- the reference's 11 and 24 taus plus tests/test_gpu_forward_protocols.py's (2 - 64 taus, off-grid spin
echo, T % 4 != 0, three-image normalisation) -- the seeded inputs (that file's synthetic voxels and untrained-encoder
heads, the heads perturbed by N(0, 0.3^2) so that they stand away from the prior), and the central differences of the
float64 oracle's NLL + exact KL that the one-step gradients are held to.  Computed once per case and shared; never
written to.  Test infrastructure (no GPU needed)."""
import contextlib

import numpy as np

import _laplace_reference as lr
import test_gpu_forward_protocols as fp
from _refine_reference import kl_closed_and_grad, padded_draws, step_grad

PROTOCOLS = lr.protocol_names()          # ref11, ref24, then fp.PROTOCOLS
# likelihood switches on top of a protocol's own: name -> (protocol, switches)
SWITCHED = {
    "odd33_student_t": ("odd33", dict(student_t_df=5.0)),
    "odd33_log_data": ("odd33", dict(predict_log_data=True)),
}
GRAD_CASES = PROTOCOLS + tuple(SWITCHED)
FD_PRECONDITION = 1e-6                   # the reference against the finite differences (tests/test_gpu_refine.py)
_CASES = {}
_GRADS = {}


def case(params, name, n):
    """dict(p, sw, x, q, prior, sigma, mask, live) of a case name: q = the encoder heads + N(0, 0.3^2)."""
    key = (name, n)
    if key not in _CASES:
        from oracle.oracle import Oracle
        proto, extra = SWITCHED.get(name, (name, {}))
        if proto in fp.PROTOCOLS and not extra:
            d = dict(fp.inputs(params, proto, n))
        else:
            p, sw = lr.setup(params, proto)
            sw = dict(sw, **extra)
            o32 = Oracle("f32", p, **sw)
            x, q, prior, sigma = fp.heads(o32, p, o32.T, n, fp.INPUT_SEEDS.get(proto, 11))
            mask = fp.make_mask(n)
            d = dict(p=p, sw=sw, x=x, q=q, prior=prior, sigma=sigma, mask=mask, live=mask > 0)
        d["q"] = (d["q"] + np.random.default_rng(5).normal(size=d["q"].shape) * 0.3).astype(np.float32)
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CASES[key] = d
    return _CASES[key]


@contextlib.contextmanager
def float64_oracle(d):
    with fp.float64_oracle(d["p"], d["sw"]) as o64:
        yield o64


def one_step_normals(n, S):
    """z [n, 1, Sp, 2] float32 of one step, draws S .. Sp - 1 zero"""
    z = np.zeros((n, 1, padded_draws(S), 2), np.float32)
    z[:, 0, :S] = np.random.default_rng(8).standard_normal((n, S, 2))
    return z


def gradient_reference(params, name, n=48, S=3):
    """dict(d, z, ref [n, 5], fd [n, 5]): step_grad and the central differences (h = 1e-5 on the raw heads) of
    Oracle("f64").elbo's NLL over the same explicit normals plus the exact closed-form KL, at the case's heads."""
    key = (name, n, S)
    if key not in _GRADS:
        d = case(params, name, n)
        z = one_step_normals(n, S)
        zs = z[:, 0, :S].astype(np.float64)
        q64 = d["q"].astype(np.float64)
        with float64_oracle(d) as o64:
            def loss(qq):
                e = o64.elbo(d["x"], np.ones(n), qq, d["prior"], d["sigma"], zs, np.zeros((n, 1, 2)))
                return e["nll_v"] + kl_closed_and_grad(qq, d["prior"])[0]
            ref = step_grad(o64, d["x"], q64, d["prior"], d["sigma"], zs)
            fd = np.zeros_like(q64)
            h = 1e-5
            for k in range(5):
                dd = np.zeros_like(q64)
                dd[:, k] = h
                fd[:, k] = (loss(q64 + dd) - loss(q64 - dd)) / (2 * h)
        ref.setflags(write=False)
        fd.setflags(write=False)
        _GRADS[key] = dict(d=d, z=z, ref=ref, fd=fd)
    return _GRADS[key]


def fd_scale(fd, k):
    """the column's scale of tests/test_gpu_refine.py::test_one_sgd_step_is_the_gradient"""
    return np.abs(fd[:, k]).max() + 1e-3
