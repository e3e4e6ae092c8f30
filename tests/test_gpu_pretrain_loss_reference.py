"""qbold_synth_loss_bwd, qbold_hyper_prior_bwd, qbold_r2p_loss_bwd, qbold_kl_diag and qbold_kl_mog, every voxel and
every entry, against the analytic float64 reference of tests/_pretrain_loss_reference.py under the cancellation-aware
measure defined there: head gradients |hip - ref| <= 2e-4 A_q (test_gpu_elbo_bwd_reference's BOUND_Q; 4 x the float32
floor for the cases of cases.FLOOR_Q), values |hip - ref| <= 2e-5 A_v (2e-4 for the R2' term), and the entry points'
contracts.  Cases: tests/_pretrain_loss_cases.py; figures: MEASUREMENTS.md section 25."""
import numpy as np
import pytest

import _pretrain_loss_cases as cases
import _pretrain_loss_reference as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BOUND_V = cases.BOUND_V
FILL_G, FILL_V, SCALE = 1.5, 2.0, 0.25     # what the caller's buffers hold before an accumulating launch; a scale
#                                            that is a power of two, so that scale * g is g's bits with another exponent
ULP = 2.0 ** -24
STATS_RES = 2.0 ** -24                      # 1 / kStatsFixed: the resolution of hyper_prior_kernel's fixed-point sums


def dev(a):
    return torch.as_tensor(np.array(a, order="C"), device="cuda")   # a copy: the cases' arrays are read-only


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def ctx(params):
    from qbold_vi_amd.ops import Context
    return Context(params, True, True)


@pytest.fixture(scope="module")
def num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def synth_loss_bwd(ctx, y, q, a, b, scale, g_q, loss_v):
    """qbold_synth_loss_bwd on the caller's buffers (the library's own wrapper fixes scale = 1 / N)."""
    from qbold_vi_amd import _lib
    from qbold_vi_amd.ops import _ptr, _stream
    _lib.check(ctx.lib.qbold_synth_loss_bwd(ctx.handle, _ptr(y), int(y.shape[1]), _ptr(q), _ptr(g_q), _ptr(loss_v),
                                            float(scale), float(a), float(b), q.shape[0], _stream()),
               "qbold_synth_loss_bwd")


def kl_diag(ctx, q, prior, mask, kl_v, g_q):
    """qbold_kl_diag on the caller's buffers -> sums (the library's own wrapper allocates kl_v)."""
    from qbold_vi_amd import _lib
    from qbold_vi_amd.ops import _ptr, _stream
    sums = torch.full((3,), -1.0, dtype=torch.float64, device="cuda")
    _lib.check(ctx.lib.qbold_kl_diag(ctx.handle, _ptr(q), _ptr(prior), _ptr(mask), _ptr(kl_v), _ptr(g_q), _ptr(sums),
                                     _ptr(ctx._workspace()), q.shape[0], _stream()), "qbold_kl_diag")
    return sums


def launch(ctx, c, accumulate=False):
    """One launch of the case's kernel -> dict of host arrays (float32 as the kernel wrote them): v, g_q and the
    kernel's sums.  accumulate = False: the plain result (scale 1; output buffers that the kernel adds to start at 0,
    buffers that it writes start at NaN).  accumulate = True: scale = SCALE and the buffers pre-filled with FILL_G /
    FILL_V."""
    N = c.N
    scale = SCALE if accumulate else 1.0
    full = lambda shape, val: torch.full(shape, val, dtype=torch.float32, device="cuda")
    out = {}
    if c.kernel == "synth_loss":
        g, v = full((N, 5), FILL_G if accumulate else np.nan), full((N,), FILL_V if accumulate else np.nan)
        synth_loss_bwd(ctx, dev(c.y), dev(c.q), c.a, c.b, scale, g, v)
    elif c.kernel == "hyper_prior":
        g, v = full((N, 5), FILL_G if accumulate else 0.0), full((N,), FILL_V if accumulate else 0.0)
        out["sums"] = host(ctx.hyper_prior_bwd(dev(c.q), c.ig, scale=scale, g_q=g, loss_v=v))
    elif c.kernel == "r2p_loss":
        g, v = full((N, 5), FILL_G if accumulate else 0.0), full((N,), FILL_V if accumulate else 0.0)
        kw = dict(seed=c.seed, voxel0=cases.VOXEL0) if c.philox else dict(z=dev(c.z))
        ctx.r2p_loss_bwd(dev(c.y), dev(c.q), c.n, scale=scale, g_q=g, loss_v=v, **kw)
    elif c.kernel == "kl_diag":
        g, v = full((N, 5), FILL_G if accumulate else 0.0), full((N,), np.nan if not accumulate else FILL_V)
        out["sums"] = host(kl_diag(ctx, dev(c.q), dev(c.prior), dev(c.mask), v, g))
    else:
        g = None
        kw = dict(seed=c.seed, voxel0=cases.VOXEL0) if c.philox else dict(z=dev(c.z))
        v = ctx.kl_mog(dev(c.q), dev(c.comps), **kw)
    torch.cuda.synchronize()
    out["v"] = host(v)
    if g is not None:
        out["g_q"] = host(g)
    return out


_runs = {}


def run(ctx, params, num_cus, kernel, name):
    """(case, plain launch), one launch per (kernel, case)."""
    c = cases.build(params, kernel, name, num_cus)
    if (kernel, name) not in _runs:
        _runs[(kernel, name)] = launch(ctx, c)
    return c, _runs[(kernel, name)]


def entries_over(got, want, A, bound):
    """[] or [count, voxel, entry, got, want, A] of the worst entry with |got - want| > bound A."""
    got = np.asarray(got, np.float64)
    r = R.ratio(got, want, A)
    bad = ~(r <= bound)
    if not bad.any():
        return []
    i = np.unravel_index(np.argmax(np.where(bad, r, -1.0)), r.shape)
    return [int(bad.sum())] + [int(k) for k in i] + [got[i], want[i], A[i]]


ALL = [(k, n) for k in cases.CASES for n in cases.CASES[k]]
WITH_GRADIENT = [(k, n) for k, n in ALL if k != "kl_mog"]


@pytest.mark.parametrize("kernel,name", WITH_GRADIENT)
def test_head_gradients_per_voxel(params, ctx, num_cus, kernel, name):
    """Every entry of g_q of every voxel, |hip - ref| <= 2e-4 A_q (cases.FLOOR_Q: 4 x the case's float32 floor).  The
    only voxels not compared are kl_diag's masked-out ones, whose gradient test_kl_diag_contract holds to be untouched.
    The diagonal family's use of synth_loss_bwd (fifth column 0): column 4 of the kernel's result is held to what the
    reference gives for c = 0, and with the trainer's own two lines applied (column 4 zeroed) the rest is held to the
    diagonal reference."""
    c, got = run(ctx, params, num_cus, kernel, name)
    bound = cases.bound_q(kernel, name)
    g = got["g_q"].astype(np.float64)
    failed = []
    if kernel == "synth_loss" and c.diagonal:
        r4 = R.worst(g[:, 4], c.ref["g4_kernel"], c.ref["A4_kernel"])
        print(f"{kernel} {name}: column 4 at c = 0, worst |d| / A {r4:.2e}")
        failed += entries_over(g[:, 4], c.ref["g4_kernel"], c.ref["A4_kernel"], bound)
        g[:, 4] = 0.0     # training.py: gq[:, 4] = 0.0
    sel = cases.compared(c)
    rq = R.worst(g[sel], c.ref["g_q"][sel], c.ref["A_q"][sel])
    print(f"{kernel} {name}: N {c.N}, heads, worst |d| / A_q {rq:.2e} (bound {bound:.1e})")
    failed += entries_over(g[sel], c.ref["g_q"][sel], c.ref["A_q"][sel], bound)
    assert not failed, failed


@pytest.mark.parametrize("kernel,name", ALL)
def test_values_per_voxel(params, ctx, num_cus, kernel, name):
    """Every voxel's value, |hip - ref| <= 2e-5 A_v (r2p_loss: 2e-4), masked-out voxels of kl_diag included (kl_v is
    written for every voxel; a voxel with NaN heads holds NaN).  The diagonal family's value is the kernel's minus the
    log 2 pi the trainer subtracts."""
    c, got = run(ctx, params, num_cus, kernel, name)
    v = got["v"].astype(np.float64)
    if kernel == "synth_loss" and c.diagonal:
        v = v - 1.8378770664093453     # training.py: lv = lv - 1.8378770664093453
    nan = np.isnan(c.ref["v"])
    assert np.array_equal(np.isnan(v), nan)
    rv = R.worst(v[~nan], c.ref["v"][~nan], c.ref["A_v"][~nan])
    print(f"{kernel} {name}: N {c.N}, values, worst |d| / A_v {rv:.2e} (bound {BOUND_V[kernel]:.0e})")
    over = entries_over(v[~nan], c.ref["v"][~nan], c.ref["A_v"][~nan], BOUND_V[kernel])
    assert not over, over


@pytest.mark.parametrize("name", list(cases.CASES["hyper_prior"]))
def test_hyper_prior_sums(params, ctx, num_cus, name):
    """The four sums against the float64 sums.  From the code: every thread adds its float32 terms (log v = 2 s, 1 / v =
    exp(-log v)) in double, the block's double sum is turned into fixed point with kStatsFixed = 2^24 by llrint and added
    as an integer.  The bound is twice the resolution 2^-24 of that accumulation plus N float32 roundings of a term,
    N 2^-24 max |term|.  (Each block's llrint is off by at most half a resolution; past four blocks those halves are
    covered by the second part, there being at least 256 voxels a block and max |term| >= 1 in every case -- asserted.)"""
    c, got = run(ctx, params, num_cus, "hyper_prior", name)
    lv = c.ref["log_v"]
    terms = np.stack([lv[:, 0], np.exp(-lv[:, 0]), lv[:, 1], np.exp(-lv[:, 1])], -1)
    assert np.all(np.abs(terms).max(0) >= 1.0)
    bound = 2.0 * STATS_RES + c.N * ULP * np.abs(terms).max(0)
    err = np.abs(got["sums"] - c.ref["sums"])
    print(f"hyper_prior {name}: N {c.N}, sums |d| / bound {err / bound}")
    assert np.all(err <= bound), (err, bound)


def accumulated(plain, fill, scale):
    """fill + scale * plain in float64, and the float32 roundings between it and what the kernel may hold: of the term
    (the plain launch rounded it; scaling by a power of two is exact) and of the sum (a fused multiply-add rounds the
    sum only)."""
    want = fill + scale * plain.astype(np.float64)
    return want, 1.01 * ULP * (np.abs(want) + scale * np.abs(plain))


@pytest.mark.parametrize("kernel,name", [("synth_loss", "saturated_N257_ld5_ig3"), ("hyper_prior", "saturated_N257"),
                                         ("r2p_loss", "saturated_N257_ld3_n10_philox"),
                                         ("r2p_loss", "saturated_N40_ld5_n10")])
def test_scale_and_accumulation(params, ctx, num_cus, kernel, name):
    """qbold_synth_loss_bwd WRITES scale * g and the value over whatever the buffers held: with scale = 1 / 4 and
    buffers pre-filled, g is the plain launch's times 1 / 4 bit for bit and the value is the plain launch's.
    qbold_hyper_prior_bwd and qbold_r2p_loss_bwd ADD scale * gradient and the value to buffers pre-filled with a
    non-zero constant: fill + scale * plain to the float32 rounding of that sum."""
    c, plain = run(ctx, params, num_cus, kernel, name)
    acc = launch(ctx, c, accumulate=True)
    if kernel == "synth_loss":
        assert np.array_equal(acc["g_q"], np.float32(SCALE) * plain["g_q"])
        assert np.array_equal(acc["v"], plain["v"])
        return
    for key, fill, scale in (("g_q", FILL_G, SCALE), ("v", FILL_V, 1.0)):
        want, tol = accumulated(plain[key], fill, scale)
        assert np.all(np.abs(acc[key] - want) <= tol), (key, np.abs(acc[key] - want).max())
    if kernel == "hyper_prior":
        assert np.array_equal(acc["sums"], plain["sums"])


@pytest.mark.parametrize("name", list(cases.CASES["kl_diag"]))
def test_kl_diag_contract(params, ctx, num_cus, name):
    """qbold_kl_diag adds d kl / d q to g_q: pre-filled buffers hold fill + gradient where mask > 0, are bit-for-bit
    untouched where mask = 0 and in column 4 everywhere; kl_v is written for every voxel; sums = (0, sum over mask > 0
    of kl, sum of the mask) with fractional masks, NaN heads in masked-out voxels staying out of sums[1]."""
    c, plain = run(ctx, params, num_cus, "kl_diag", name)
    acc = launch(ctx, c, accumulate=True)
    on = c.mask > 0
    assert (~on).any() and (c.mask == 0.5).any()
    assert np.all(acc["g_q"][~on] == np.float32(FILL_G)) and np.all(acc["g_q"][:, 4] == np.float32(FILL_G))
    assert np.all(plain["g_q"][~on] == 0.0) and np.all(plain["g_q"][:, 4] == 0.0)
    want, tol = accumulated(plain["g_q"][on][:, :4], FILL_G, 1.0)
    assert np.all(np.abs(acc["g_q"][on][:, :4] - want) <= tol)
    # kl_v is written (not added to) for every voxel, masked-out ones included
    assert np.array_equal(acc["v"], plain["v"], equal_nan=True)
    assert np.isnan(plain["v"][c.nan_voxels]).all() and np.isnan(plain["v"]).sum() == len(c.nan_voxels)
    sums = plain["sums"]
    assert sums[0] == 0.0 and sums[2] == c.mask.astype(np.float64).sum()
    want_kl, scale_kl = c.ref["v"][on].sum(), c.ref["A_v"][on].sum()
    print(f"kl_diag {name}: sums[1] |d| / sum A_v {abs(sums[1] - want_kl) / scale_kl:.2e}")
    assert np.isfinite(sums[1]) and abs(sums[1] - want_kl) <= BOUND_V["kl_diag"] * scale_kl
    assert np.array_equal(acc["sums"], sums)


@pytest.mark.parametrize("name", ["saturated_N40_ld5_n10", "saturated_N257_ld3_n10_philox", "base_N40_ld3_n2"])
def test_r2p_loss_without_gradient(params, ctx, num_cus, name):
    """want_grad = False returns the same values, bit for bit, as the launch with the gradient."""
    c, plain = run(ctx, params, num_cus, "r2p_loss", name)
    kw = dict(seed=c.seed, voxel0=cases.VOXEL0) if c.philox else dict(z=dev(c.z))
    v, g = ctx.r2p_loss_bwd(dev(c.y), dev(c.q), c.n, want_grad=False, **kw)
    assert g is None and np.array_equal(host(v), plain["v"])


def test_r2p_philox_stream_is_the_oracles(params, ctx, num_cus):
    """The kernel's own stream 3 at voxel0 = 1000 against explicit normals from oracle.philox_normals: the draws are
    float32 roundings apart (the device's log2 / sin / cos against libm's), so the two launches agree to the bound of
    the reference comparison."""
    c, plain = run(ctx, params, num_cus, "r2p_loss", "saturated_N257_ld3_n10_philox")
    v, g = ctx.r2p_loss_bwd(dev(c.y), dev(c.q), c.n, z=dev(c.z))
    rv, rq = cases.worst_ratios(c, host(v), host(g))
    print(f"explicit oracle normals: values {rv:.2e} of A_v, heads {rq:.2e} of A_q")
    assert rv <= BOUND_V["r2p_loss"] and rq <= cases.BOUND_Q


def test_kl_mog_rejects_too_many_components(params, ctx):
    """M = 16 (kMaxMog) runs (a case of test_values_per_voxel); M = 17 is the invalid-argument error."""
    from qbold_vi_amd._lib import QboldError
    c = cases.build(params, "kl_mog", "saturated_N40_M16")
    comps = np.concatenate([c.comps, c.comps[:1]])
    with pytest.raises(QboldError, match="status -1"):
        ctx.kl_mog(dev(c.q), dev(comps), z=dev(c.z))


@pytest.mark.parametrize("kernel,name", ALL)
def test_two_launches_are_bitwise_equal(params, ctx, num_cus, kernel, name):
    c, first = run(ctx, params, num_cus, kernel, name)
    second = launch(ctx, c)
    assert set(first) == set(second)
    for key in first:
        assert np.array_equal(first[key], second[key], equal_nan=True), key
