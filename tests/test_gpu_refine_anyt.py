"""Refinement on any tau grid (qbold_refine_posterior_anyt, qbold_refine_posterior_spatial_anyt and the Python surface
that chooses between them and the kernels specialised for 11 / 24 taus): the gradient of one step and twenty steps of
either optimiser against the float64 restatements (tests/_refine_reference.py, tests/_refine_tv_reference.py) on the
protocol table of tests/_refine_anyt_cases.py, the Philox stream, bitwise structure, errors through the C ABI, the
dispatch, the TV-coupled volume, and FineTuner.refine / save_predictions at 33 taus.  The cases, the float64 finite
differences and their precondition are shared with tests/test_refine_anyt_host.py.

Bounds are the existing refine tests' (tests/test_gpu_refine.py, tests/test_gpu_refine_tv.py).  The learning rates of
the twenty-step runs are lower than those tests': at 33 / 64 taus the likelihood gradient is larger, and the float64
loop must move the heads by about 0.1 at the most for the bounds' premise (two runs that differ by float32 and the
tissue table's gradient error only) to hold -- SGD 1e-5, Adam 1e-2 per voxel; SGD 1e-5, Adam 1e-3 on the volume."""
import ctypes as C
import os

import numpy as np
import pytest

import _refine_anyt_cases as rc
import test_gpu_forward_protocols as fp
from _refine_reference import padded_draws, refine_reference
from _refine_tv_reference import refine_tv_reference

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

REFINE_STREAM = 7
N_VOX = 333   # two full 128-thread blocks, a partial one, and a partial wave
dev = fp.dev
_same_bits = fp._same_bits


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _context(d, node0=False):
    """a context of the case's protocol and switches; node0 False: exact derivatives of the forward value, as the
    float64 finite differences take them (tests/test_gpu_refine.py)"""
    from qbold_vi_amd.ops import Context
    c = Context(d["p"], True, True, **d["sw"])
    if not node0:
        c.set_grad_node0(False)
    return c


def _p64(params):
    return dict(params, tau_start="-0.015", tau_end="0.065", tau_step="0.00125")


# ---- 1. one SGD step is the gradient ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.GRAD_CASES)
def test_one_sgd_step_is_the_gradient(params, name):
    """SGD, one step, explicit normals, 48 voxels (a partial wave), S = 3, through kernel="generic": (q_in - q_out) / lr
    against the float64 finite differences at 2e-3 of the column's scale, the reference within 1e-6 of them."""
    g = rc.gradient_reference(params, name)
    d, z, fd, ref = g["d"], g["z"], g["fd"], g["ref"]
    c = _context(d)
    lr = 1e-2
    q_out = c.refine_posterior(dev(d["x"]), None, dev(d["q"]), dev(d["prior"]), dev(d["sigma"]), steps=1, S=3, lr=lr,
                               optimizer="sgd", z=dev(z), kernel="generic")
    got = (d["q"].astype(np.float64) - q_out.cpu().numpy().astype(np.float64)) / lr
    assert np.all(np.isfinite(got))
    for k in range(5):
        scale = rc.fd_scale(fd, k)
        assert np.max(np.abs(ref[:, k] - fd[:, k])) / scale < rc.FD_PRECONDITION, (name, k)
        err = np.max(np.abs(got[:, k] - fd[:, k])) / scale
        print(name, k, "scale", scale, "err", err)
        assert err < 2e-3, (name, k, err, scale)


# ---- 2. twenty steps against the float64 loop ------------------------------------------------------------------------
_LOOP_Z = {}


def _loop_normals(steps, S):
    key = (steps, S)
    if key not in _LOOP_Z:
        z = np.random.default_rng(4).standard_normal((N_VOX, steps, padded_draws(S), 2)).astype(np.float32)
        z.setflags(write=False)
        _LOOP_Z[key] = z
    return _LOOP_Z[key]


@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("name", rc.PROTOCOLS)
def test_twenty_steps_match_float64_loop(params, name, opt):
    """333 voxels, S = 2, lr_final = 0, explicit normals.  SGD (lr 1e-5) within 2e-3 of the distance travelled;
    Adam (lr 1e-2) within 2 lr per step for every coordinate and within 2e-2 of the column's travel for 99 % of them
    (tests/test_gpu_refine.py::test_optimiser_matches_float64_loop states why Adam needs the two-part bound)."""
    d = rc.case(params, name, N_VOX)
    S, steps = 2, 20
    lr = 1e-5 if opt == "sgd" else 1e-2
    z = _loop_normals(steps, S)
    with rc.float64_oracle(d) as o64:
        ref = refine_reference(o64, d["x"], d["q"], d["prior"], d["sigma"], z, S, lr=lr, lr_final=0.0, optimizer=opt)
    c = _context(d)
    got = c.refine_posterior(dev(d["x"]), None, dev(d["q"]), dev(d["prior"]), dev(d["sigma"]), steps=steps, S=S, lr=lr,
                             lr_final=0.0, optimizer=opt, z=dev(z), kernel="generic").cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got))
    moved = np.abs(ref - d["q"])
    diff = np.abs(got - ref)
    print(name, opt, "moved max", moved.max(), "diff max", diff.max(), "p99", np.quantile(diff, 0.99),
          "rel", diff.max() / moved.max())
    assert moved.max() < 0.2   # the premise of the bounds (module docstring)
    if opt == "sgd":
        assert diff.max() < 2e-3 * moved.max() + 1e-5
    else:
        assert diff.max() < 2.0 * lr * steps
        assert np.quantile(diff / (moved.max(axis=0) + 1e-6), 0.99) < 2e-2


# ---- 3. the Philox stream --------------------------------------------------------------------------------------------
def test_philox_stream_equals_explicit_normals(params):
    d = rc.case(params, "odd33", N_VOX)
    c = _context(d, node0=True)
    x, q, prior, sigma = (dev(d[k]) for k in ("x", "q", "prior", "sigma"))
    S, steps, seed, v0 = 3, 6, 77, 123457
    Sp = padded_draws(S)
    a, la = c.refine_posterior(x, None, q, prior, sigma, steps=steps, S=S, seed=seed, voxel0=v0, want_loss=True)
    z = c.normals(N_VOX, steps * Sp, stream_id=REFINE_STREAM, seed=seed, voxel0=v0).reshape(N_VOX, steps, Sp, 2)
    b, lb = c.refine_posterior(x, None, q, prior, sigma, steps=steps, S=S, z=z, seed=seed, voxel0=v0, want_loss=True)
    assert _same_bits(a, b) and _same_bits(la, lb)
    assert torch.isfinite(a).all() and torch.isfinite(la).all()
    z6 = c.normals(N_VOX, steps * Sp, stream_id=6, seed=seed, voxel0=v0).reshape(N_VOX, steps, Sp, 2)
    c6 = c.refine_posterior(x, None, q, prior, sigma, steps=steps, S=S, z=z6, seed=seed, voxel0=v0)
    assert not torch.equal(c6, a)


# ---- 4. bitwise structure --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["full64", "two"])
def test_bitwise_structure(params, name):
    from qbold_vi_amd import _lib
    d = rc.case(params, name, N_VOX)
    c = _context(d, node0=True)
    n, seed, v0 = N_VOX, 99, 5000
    dead_np = ~d["live"]
    q = d["q"].copy()
    q[np.flatnonzero(dead_np)[:5]] = np.nan      # masked voxels' heads are copied, not read
    args = [dev(fp.poisoned(d)), dev(d["mask"]), dev(q), dev(d["prior"]), dev(d["sigma"])]
    kw = dict(steps=30, S=2, lr=0.05, lr_final=0.05, seed=seed, want_loss=True)
    o, lo = c.refine_posterior(*args, voxel0=v0, **kw)
    o2, lo2 = c.refine_posterior(*args, voxel0=v0, **kw)
    assert _same_bits(o, o2) and _same_bits(lo, lo2)
    h = 150   # not a multiple of the block: every voxel of the second shard changes its lane and its block
    oa, la = c.refine_posterior(*(a[:h] for a in args), voxel0=v0, **kw)
    ob, lb = c.refine_posterior(*(a[h:] for a in args), voxel0=v0 + h, **kw)
    assert _same_bits(o[:h], oa) and _same_bits(o[h:], ob) and _same_bits(lo[:h], la) and _same_bits(lo[h:], lb)
    dead = torch.as_tensor(dead_np, device="cuda")
    assert dead.sum().item() > n // 8
    assert _same_bits(o[dead], args[2][dead]) and torch.all(lo[dead] == 0.0)
    live = ~dead
    assert torch.isfinite(o[live]).all() and not torch.equal(o[live], args[2][live])
    # in place (q_out aliasing q_in) through the C ABI
    qi = args[2].clone()
    cfg = _lib.RefineCfg(0, 0.05, 0.05, 0.9, 0.999, 1e-8)
    rc_ = c.lib.qbold_refine_posterior_anyt(c.handle, P(args[0]), P(args[1]), P(qi), P(args[3]), P(args[4]), None, 30,
                                            2, C.byref(cfg), seed, v0, P(qi), None, n, None)
    assert rc_ == 0
    torch.cuda.synchronize()
    assert _same_bits(qi, o)
    # a NaN voxel inside the mask: NaN heads for that voxel, every other voxel's bits as before
    i = int(np.flatnonzero(d["live"])[3])
    xn = args[0].clone()
    xn[i] = float("nan")
    on = c.refine_posterior(xn, *args[1:], voxel0=v0, **kw)[0]
    assert torch.isnan(on[i]).all()
    others = torch.ones(n, dtype=torch.bool, device="cuda")
    others[i] = False
    assert _same_bits(on[others], o[others])


# ---- 5. errors through the C ABI -------------------------------------------------------------------------------------
def test_bad_arguments(params):
    from qbold_vi_amd import _lib
    from qbold_vi_amd._lib import Geometry
    from qbold_vi_amd.ops import Context
    n = 64
    d = rc.case(params, "ref11", n)
    ctx = Context(params, True, True)
    x, q, prior, sigma = (dev(d[k]) for k in ("x", "q", "prior", "sigma"))
    out = torch.empty((n, 5), device="cuda")

    def call(c, steps=5, S=1, lr=0.05, o=out, opt=0, qq=q, xx=x, ss=sigma, entry="qbold_refine_posterior_anyt"):
        cfg = _lib.RefineCfg(opt, lr, lr, 0.9, 0.999, 1e-8)
        return getattr(c.lib, entry)(c.handle, P(xx), None, P(qq), P(prior), P(ss), None, steps, S, C.byref(cfg), 1,
                                     0, P(o), None, n, None)
    # every invalid case of tests/test_gpu_refine.py::test_bad_arguments
    assert call(ctx, steps=0) == -1 and call(ctx, S=0) == -1 and call(ctx, lr=0.0) == -1 and call(ctx, lr=-1.0) == -1
    assert call(ctx, o=None) == -1 and call(ctx, qq=None) == -1 and call(ctx, opt=2) == -1
    assert call(ctx, steps=(1 << 31) - 1, S=9) == -1
    assert call(ctx) == _lib.QBOLD_OK
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    # configurations without a kernel: the literal tissue integral, no full model
    cl = Context(params, True, True)
    cl.set_tissue_mode("literal")
    assert call(cl) == -3
    assert call(Context(params, False, True)) == -3
    # 64 taus with 64-column buffers: the new entry runs, the old one keeps refusing
    c64 = Context(_p64(params), True, True)
    assert c64.T == 64
    x64, s64 = torch.ones((n, 64), device="cuda"), torch.full((n, 64), 0.02, device="cuda")
    assert call(c64, xx=x64, ss=s64) == _lib.QBOLD_OK
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert call(c64, xx=x64, ss=s64, entry="qbold_refine_posterior") == -3

    # the spatial entry: every invalid case of tests/test_gpu_refine_tv.py::test_bad_arguments
    lead = (1, 4, 4, 4)
    good = Geometry(*lead)
    m = torch.ones(lead, device="cuda")
    ws = torch.empty(88 * n + 16, dtype=torch.uint8, device="cuda")
    assert ctx.lib.qbold_refine_spatial_workspace_bytes(ctx.handle, C.byref(good)) == 88 * n

    def call5(c=ctx, geom=good, w=5.0, steps=5, S=1, lr=0.05, opt=0, qq=q, o=out, wsp=P(ws), xx=x, ss=sigma,
              entry="qbold_refine_posterior_spatial_anyt"):
        cfg = _lib.RefineCfg(opt, lr, lr, 0.9, 0.999, 1e-8)
        return getattr(c.lib, entry)(c.handle, P(xx), P(m), P(qq), P(prior), P(ss), None,
                                     C.byref(geom) if geom is not None else None, C.c_float(w), steps, S,
                                     C.byref(cfg), 1, 0, P(o), None, wsp, None)
    assert call5() == _lib.QBOLD_OK
    torch.cuda.synchronize()
    for kw in (dict(steps=0), dict(S=0), dict(lr=0.0), dict(opt=2), dict(qq=None), dict(o=None),
               dict(w=-1.0), dict(w=float("nan")), dict(w=float("inf")), dict(geom=None),
               dict(geom=Geometry(0, 1, 1, 1)), dict(geom=Geometry(1, -2, 1, 1)),
               dict(geom=Geometry(1 << 30, 1 << 30, 1 << 30, 4)),   # N beyond int64
               dict(wsp=None), dict(wsp=C.c_void_p(ws.data_ptr() + 4)),
               dict(steps=(1 << 31) - 1, S=9)):
        assert call5(**kw) == -1, kw
    assert call5(c=cl) == -3
    assert call5(c=Context(params, False, True)) == -3
    assert call5(c=c64, xx=x64, ss=s64) == _lib.QBOLD_OK
    assert call5(c=c64, xx=x64, ss=s64, w=0.0) == _lib.QBOLD_OK
    torch.cuda.synchronize()
    assert call5(c=c64, xx=x64, ss=s64, entry="qbold_refine_posterior_spatial") == -3


# ---- 6. the Python dispatch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ref11", "ref24"])
def test_dispatch_keeps_the_specialised_kernels_bits(params, name):
    """Context.refine_posterior without kernel= at the reference's 11 / 24 taus is the existing entry, bit for bit;
    kernel="generic" runs the run-time-T kernel there: the same draws, agreeing to rounding, not to the bit."""
    from qbold_vi_amd import _lib
    d = rc.case(params, name, N_VOX)
    c = _context(d, node0=True)
    x, m, q, prior, sigma = (dev(d[k]) for k in ("x", "mask", "q", "prior", "sigma"))
    steps, S, seed, v0 = 10, 2, 5, 1000
    a = c.refine_posterior(x, m, q, prior, sigma, steps=steps, S=S, lr=0.05, lr_final=0.005, seed=seed, voxel0=v0)
    want = torch.empty_like(a)
    cfg = _lib.RefineCfg(0, 0.05, 0.005, 0.9, 0.999, 1e-8)
    assert c.lib.qbold_refine_posterior(c.handle, P(x), P(m), P(q), P(prior), P(sigma), None, steps, S, C.byref(cfg),
                                        seed, v0, P(want), None, N_VOX, None) == 0
    torch.cuda.synchronize()
    assert _same_bits(a, want)
    # one SGD step at lr = 1 (q_in - q_out is the gradient to float32 rounding) on the same Philox draws: the two
    # kernels' gradients within the project's gradient bound, 2e-3 of the column's scale, of each other (each is held
    # to that bound against float64, which alone would allow twice as much)
    kw = dict(steps=1, S=S, lr=1.0, lr_final=1.0, optimizer="sgd", seed=seed, voxel0=v0)
    s0 = c.refine_posterior(x, m, q, prior, sigma, **kw)
    s1 = c.refine_posterior(x, m, q, prior, sigma, kernel="generic", **kw)
    g0, g1 = (q - s0).double(), (q - s1).double()
    err = ((g0 - g1).abs().max(0).values / (g0.abs().max(0).values + 1e-3)).max().item()
    print(name, "specialised vs generic, one SGD step: max column error", err, "bit-equal", _same_bits(s0, s1))
    assert err < 2e-3
    dead = m <= 0
    assert _same_bits(s1[dead], q[dead])


def test_dispatch_reaches_the_any_t_kernels(params):
    """On a 33-tau protocol Context.refine_posterior and refine_posterior_spatial run (the specialised entries refuse
    it), and give the bits of the direct calls of the new entries."""
    from qbold_vi_amd import _lib
    d = rc.case(params, "odd33", N_VOX)
    c = _context(d, node0=True)
    x, m, q, prior, sigma = (dev(d[k]) for k in ("x", "mask", "q", "prior", "sigma"))
    a = c.refine_posterior(x, m, q, prior, sigma, steps=10, S=1, lr=0.05, lr_final=0.005, seed=5)
    want = torch.empty_like(a)
    cfg = _lib.RefineCfg(0, 0.05, 0.005, 0.9, 0.999, 1e-8)
    assert c.lib.qbold_refine_posterior(c.handle, P(x), P(m), P(q), P(prior), P(sigma), None, 10, 1, C.byref(cfg),
                                        5, 0, P(want), None, N_VOX, None) == -3
    assert c.lib.qbold_refine_posterior_anyt(c.handle, P(x), P(m), P(q), P(prior), P(sigma), None, 10, 1,
                                             C.byref(cfg), 5, 0, P(want), None, N_VOX, None) == 0
    torch.cuda.synchronize()
    assert _same_bits(a, want) and torch.isfinite(a).all()
    assert _same_bits(a, c.refine_posterior(x, m, q, prior, sigma, steps=10, S=1, lr=0.05, lr_final=0.005, seed=5,
                                            kernel="generic"))
    lead = (1, 37, 9, 1)
    r5 = lambda t: t.reshape(lead + t.shape[1:])   # noqa: E731
    b = c.refine_posterior_spatial(r5(x), r5(m), r5(q), r5(prior), r5(sigma), 5.0, steps=10, S=1, lr=0.05, seed=5)
    assert b.shape == lead + (5,) and torch.isfinite(b).all() and not torch.equal(b.reshape(-1, 5), a)


# ---- 7. the volume under the TV prior --------------------------------------------------------------------------------
SPATIAL = ("odd33", "off22_3img", "full64")
_VOLUMES = {}


def _spatial_case(params, name):
    """test_gpu_refine_tv's striped volume (1, 9, 7, 3) on the protocol, and twenty steps' normals"""
    if name not in _VOLUMES:
        from oracle.oracle import Oracle
        from test_gpu_refine_tv import _volume
        p, sw = fp.protocol(params, name), fp.switches(name)
        lead = (1, 9, 7, 3)
        vol = _volume(Oracle("f32", p, **sw), p, lead, 13, spread=0.1, stripes=True)
        n, S, steps = int(np.prod(lead)), 2, 20
        z = np.random.default_rng(4).standard_normal((n, steps, padded_draws(S), 2)).astype(np.float32)
        for a in vol + (z,):
            a.setflags(write=False)
        _VOLUMES[name] = dict(p=p, sw=sw, vol=vol, z=z, S=S, steps=steps)
    return _VOLUMES[name]


@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("name", SPATIAL)
def test_volume_matches_float64_jacobi(params, name, opt):
    """Twenty Jacobi steps, w = 5, explicit normals, against the float64 restatement: while its smallest |sigmoid
    difference| over every live pair and step stays above 1e-4 no sign of the TV subgradient can differ, and the runs
    differ by float32 and the tissue table's gradient error only (tests/test_gpu_refine_tv.py's bound, 1e-5)."""
    s = _spatial_case(params, name)
    x, m, q, prior, sigma = s["vol"]
    w = 5.0
    lr = 1e-5 if opt == "sgd" else 1e-3
    with fp.float64_oracle(s["p"], s["sw"]) as o64:
        ref, gap = refine_tv_reference(o64, x, m, q, prior, sigma, s["z"], s["S"], w, lr=lr, lr_final=0.0,
                                       optimizer=opt)
    c = _context(s)
    got = c.refine_posterior_spatial(dev(x), dev(m), dev(q), dev(prior), dev(sigma), w, steps=s["steps"], S=s["S"],
                                     lr=lr, lr_final=0.0, optimizer=opt, z=dev(s["z"]),
                                     kernel="generic").cpu().numpy().astype(np.float64)
    live = m > 0
    diff = np.abs(got - ref)[live]
    moved = np.abs(ref - q)[live]
    print(name, opt, "min gap", gap, "moved max", moved.max(), "diff max", diff.max(), "p99", np.quantile(diff, 0.99))
    assert gap > 1e-4
    np.testing.assert_array_equal(got[~live], q[~live])
    assert diff.max() < 1e-5, (name, opt, diff.max())


@pytest.mark.parametrize("name", SPATIAL)
def test_zero_weight_is_the_per_voxel_entry_bitwise(params, name):
    s = _spatial_case(params, name)
    c = _context(s, node0=True)
    x, m, q, prior, sigma = (dev(a) for a in s["vol"])
    T = c.T
    for opt, steps, S, z in (("adam", 20, 2, dev(s["z"])), ("sgd", 7, 5, None), ("adam", 1, 1, None)):
        kw = dict(steps=steps, S=S, lr=0.05, lr_final=0.01, optimizer=opt, z=z, seed=9, voxel0=321, want_loss=True,
                  kernel="generic")
        a, la = c.refine_posterior_spatial(x, m, q, prior, sigma, 0.0, **kw)
        b, lb = c.refine_posterior(x.reshape(-1, T), m.reshape(-1), q.reshape(-1, 5), prior.reshape(-1, 5),
                                   sigma.reshape(-1, T), **kw)
        assert _same_bits(a.reshape(-1, 5), b) and _same_bits(la.reshape(-1, 2), lb), (name, opt, steps)


def test_tv_gradient_is_the_smoothness_kernels(params):
    """The TV part of one SGD step of the step kernel (w = 5 minus w = 0) is ctx.smoothness's gradient, under the ulp
    bound of tests/test_gpu_refine_tv.py::test_tv_gradient_is_the_smoothness_kernels."""
    from oracle.oracle import Oracle
    from test_gpu_refine_tv import _volume
    p, sw = fp.protocol(params, "odd33"), fp.switches("odd33")
    c = _context(dict(p=p, sw=sw))
    lead = (2, 9, 7, 3)
    x, m, q, prior, _ = (dev(a) for a in _volume(Oracle("f32", p, **sw), p, lead, 12, spread=1.0))
    sigma = torch.full_like(x, 0.5)   # a small likelihood gradient: the step is dominated by the TV term
    lr, w = 1e-2, 5.0
    z = torch.randn((int(np.prod(lead)), 1, 4, 2), device="cuda")
    kw = dict(steps=1, S=3, lr=lr, lr_final=lr, optimizer="sgd", z=z)
    q0 = c.refine_posterior_spatial(x, m, q, prior, sigma, 0.0, **kw)
    qw = c.refine_posterior_spatial(x, m, q, prior, sigma, w, **kw)
    g_q = torch.zeros((q.numel() // 5, 5), device="cuda")
    c.smoothness(q, m, weight=w, g_q=g_q)
    got = ((qw.double() - q0.double()) / (-lr)).reshape(-1, 5)
    qi = q.double().reshape(-1, 5)
    a0, aw = q0.double().reshape(-1, 5), qw.double().reshape(-1, 5)
    ulp = (torch.maximum(a0.abs(), aw.abs()) + 4.0 * ((qi - a0).abs() + (qi - aw).abs())) * 2.0 ** -23
    err = torch.abs(got - g_q.double())
    print("max |g_q|", g_q.abs().max().item(), "max err", err.max().item(), "max err / tol",
          (err / (ulp / lr + 1e-12)).max().item())
    assert torch.all(err <= ulp / lr + 1e-12)
    assert g_q.abs().max().item() > 1.0
    dead = m.reshape(-1) <= 0
    assert _same_bits(qw.reshape(-1, 5)[dead], q.reshape(-1, 5)[dead])


# ---- 8. the surface at 33 taus ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def surface33(params):
    from qbold_vi_amd import EncoderTrainer, SignalGenerationLayer
    p = fp.protocol(params, "odd33")
    tr = EncoderTrainer(system_params=p, no_units=60, use_layer_norm=False, dropout_rate=0.0,
                        no_intermediate_layers=2, initial_im_sigma=0.05, activation_type='relu',
                        multi_image_normalisation=False, channelwise_gating=True, infer_inv_gamma=False,
                        use_population_prior=False, use_mvg=True, predict_log_data=False)
    model, _ = tr.create_encoder(gate_offset=-3.0, resid_init_std=0.05, no_ip_images=33)

    def fine_tuner():
        return tr.build_fine_tuner(model, SignalGenerationLayer(dict(p, simulate_noise='False'), True, True))
    return p, tr, model, fine_tuner


def test_fine_tuner_refine_at_33_taus(params, surface33):
    from oracle.oracle import Oracle, synth_inputs
    p, tr, model, fine_tuner = surface33
    assert tr.context.T == 33
    ft = fine_tuner()
    o32 = Oracle("f32", p)
    for lead, seed in (((300, 1, 1, 1), 3), ((2, 9, 7, 3), 8)):
        nv = int(np.prod(lead))
        x, _ = synth_inputs(nv, p, seed=seed, oracle=o32)
        x5 = dev(x).reshape(lead + (33,))
        m5 = dev((np.random.default_rng(seed).uniform(size=nv) > 0.3).astype(np.float32)).reshape(lead + (1,))
        p5 = model(x5)[0]
        got = ft.refine(x5, m5, p5, steps=50, no_samples=2, seed=4, voxel0=7)
        assert got["q"].shape == lead + (5,) and got["loss"].shape == lead + (2,)
        _, q5, sg5 = model.predict(x5, want=("out2", "sigma"))
        want, loss = tr.context.refine_posterior(x5.reshape(-1, 33), m5.reshape(-1), q5.reshape(-1, 5),
                                                 p5.reshape(-1, 5), sg5.reshape(-1, 33), steps=50, S=2, lr=0.1,
                                                 lr_final=0.01, seed=4, voxel0=7, want_loss=True)
        assert _same_bits(got["q"].reshape(-1, 5), want) and _same_bits(got["loss"].reshape(-1, 2), loss)
        live = m5.reshape(-1) > 0
        assert torch.isfinite(want).all()
        print(lead, "mean loss", loss[live, 0].mean().item(), "->", loss[live, 1].mean().item())
        assert loss[live, 1].mean() < loss[live, 0].mean()
        # Laplace heads -> refine -> PSIS check
        lap = ft.laplace(x5, m5, p5)
        r2 = ft.refine(x5, m5, p5, steps=20, no_samples=2, seed=4, q=lap["q"])
        assert r2["q"].shape == lead + (5,) and torch.isfinite(r2["q"]).all()
        assert not torch.equal(r2["q"].reshape(-1, 5)[live], lap["q"].reshape(-1, 5)[live])
        assert _same_bits(r2["q"].reshape(-1, 5)[~live], lap["q"].reshape(-1, 5)[~live])
        le = ft.log_evidence(x5, m5, p5, no_samples=64, seed=2, q=r2["q"], psis=True)
        assert torch.isfinite(le["log_evidence"].reshape(-1)[live]).all()
        assert torch.isfinite(le["log_evidence_psis"].reshape(-1)[live]).all()
        assert not torch.isnan(le["khat"].reshape(-1)[live]).any()
        e0 = ft.elbo(x5, m5, p5, no_samples=4, seed=2, q=q5)
        e1 = ft.elbo(x5, m5, p5, no_samples=4, seed=2, q=got["q"])
        assert e1["elbo"] < e0["elbo"]
        if len(lead) == 4 and lead[1] > 1:   # the crop: under the TV prior as well
            tv = ft.refine(x5, m5, p5, steps=20, no_samples=1, seed=4, smoothness_weight=5.0)
            assert tv["q"].shape == lead + (5,) and torch.isfinite(tv["q"]).all()


def test_save_predictions_writes_the_refined_maps_at_33_taus(params, surface33, tmp_path):
    from oracle.oracle import Oracle, synth_inputs
    from qbold_vi_amd import nifti
    p, tr, model, fine_tuner = surface33
    B, X, Y, Z = 2, 6, 5, 4
    x, _ = synth_inputs(B * X * Y * Z, p, seed=12, oracle=Oracle("f32", p))
    mask = (np.random.default_rng(1).uniform(size=(B * X * Y * Z, 1)) > 0.2).astype(np.float32)
    data = dev(np.concatenate([x, mask], -1)).reshape(B, X, Y, Z, 34)
    priors = model(data[..., :-1])[0]
    live = mask.reshape(B, X, Y, Z) > 0
    names = ("oef_refined", "dbv_refined", "r2p_refined", "amortgap")
    for sub, kw in (("w0", {}), ("w5", dict(refine_smoothness_weight=5.0))):
        out = tmp_path / sub
        os.makedirs(out)
        maps = tr.save_predictions(model, data, str(out / "sub"), fine_tuner_model=fine_tuner(), priors=priors,
                                   refine_steps=20, **kw)
        assert {f"sub_{k}.nii.gz" for k in names} <= set(os.listdir(out))
        for k in names:
            v = maps[k].cpu().numpy()
            assert v.shape == (B, X, Y, Z, 1) and np.all(np.isfinite(v)), k
            img = nifti.load(str(out / f"sub_{k}.nii.gz"))[0]
            np.testing.assert_array_equal(img, np.concatenate(np.split(v, B, axis=0), axis=-1)[0])
        gap = maps["amortgap"].cpu().numpy()[..., 0]
        assert np.all(gap[~live] == 0.0)
        print(sub, "amortisation gap over the mask", gap[live].mean())
