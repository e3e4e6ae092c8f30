"""qbold_elbo_bwd's head gradients, every entry of every voxel, against the analytic float64 gradient of
tests/_elbo_bwd_reference.py under the cancellation-aware measure defined there: |hip - ref| <= 2e-4 A_q for the heads
(the bound test_signal_bwd_matches_oracle_jacobian puts on the Jacobian they are linear in) and <= 1e-4 A_ls for log
sigma (DESIGN section 2's per-voxel NLL bound), under the shipped node-0 policy (a context nobody touched) and under
set_grad_node0(False).  Cases: tests/_elbo_bwd_cases.py; figures: MEASUREMENTS.md section 23."""
import numpy as np
import pytest

import _elbo_bwd_cases as cases
from _elbo_bwd_reference import elbo_bwd_reference

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BOUND_Q, BOUND_LS = 2e-4, 1e-4

FLOOR_LS = cases.FLOOR_LS   # log-sigma bounds set at 4 x the float32 floor of the literal reference, see there


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def rel1(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


@pytest.fixture(scope="module")
def context(params):
    """Context of a case under a node-0 policy.  node0_grad = True is the library's default: that context is constructed
    and its policy never set."""
    from qbold_vi_amd.ops import Context
    made = {}

    def get(c, node0_grad):
        key = (c.T, tuple(sorted(c.variant.items())), c.ksel, node0_grad)
        if key not in made:
            ctx = Context(c.p, True, True, **c.variant)
            if not node0_grad:
                ctx.set_grad_node0(False)
            if c.ksel:
                ctx.set_kernel_selection(c.ksel)
            made[key] = ctx
        return made[key]
    return get


_runs = {}


def run(context, c, node0_grad):
    """(sums, g_q, g_log_sigma, nll_kl) of a case under a policy as float64 arrays; one launch per (case, policy)."""
    key = (c.name, node0_grad)
    if key not in _runs:
        sums, gq, gls, nk = context(c, node0_grad).elbo_bwd(dev(c.x), dev(c.mask), dev(c.q), dev(c.prior), dev(c.ls),
                                                            c.S, c.K, seed=c.seed)
        _runs[key] = (sums.cpu().numpy(), gq.cpu().numpy().astype(np.float64), gls.cpu().numpy().astype(np.float64),
                      nk.cpu().numpy().astype(np.float64))
    return _runs[key]


def check_case_inputs(c):
    """What a case claims about the KL form its voxels take, asserted on the host from the Philox draws."""
    over = cases.kl_reach(c.q) >= cases.LOGIT_CLIP
    at_clip = cases.draws_at_clip(c.q, c.zk)
    if c.edit == "kl_under":
        assert not over.any()
    elif c.edit == "kl_one_over":
        assert over.sum() == 1
    elif c.edit == "kl_over_no_clip":
        assert over.all() and at_clip.sum() == 0
    elif c.edit == "kl_clip_binds":
        assert over.all() and at_clip.min() >= 5, at_clip   # both logits, both signs
    assert set(np.unique(c.mask[:16])) == {0.0, 0.5, 1.0}


def entries_over(got, want, A, bound):
    """[] or [count, voxel, entry, got, want, A] of the worst entry with |got - want| > bound A (A = 0: any difference)."""
    d = np.abs(got - want)
    bad = ~(d <= bound * A)
    if not bad.any():
        return []
    v, k = np.unravel_index(np.argmax(np.where(bad, d / np.maximum(A, 1e-300), -1.0)), d.shape)
    return [int(bad.sum()), int(v), int(k), got[v, k], want[v, k], A[v, k]]


@pytest.mark.parametrize("name", list(cases.CASES))
def test_head_gradients_per_voxel(params, context, name):
    """Every entry of g_q of every voxel, |hip - ref| <= 2e-4 A_q, under both node-0 policies; masked-out voxels are
    exact zeros."""
    c = cases.build(params, name)
    check_case_inputs(c)
    failed = []
    for node0_grad in (True, False):
        _, gq, gls, _ = run(context, c, node0_grad)
        ref = c.ref[node0_grad]
        rq, _ = cases.worst_ratio(gq, gls, ref)
        print(f"{name} node0_grad={node0_grad}: heads, worst |d| / A_q {rq:.2e} (bound {BOUND_Q:.0e})")
        assert np.all(gq[c.mask == 0] == 0.0)
        over = entries_over(gq, ref["g_q"], ref["A_q"], BOUND_Q)
        if over:
            failed.append([node0_grad] + over)
    assert not failed, failed


@pytest.mark.parametrize("name", list(cases.CASES))
def test_log_sigma_gradients_per_voxel(params, context, name):
    """Every entry of g_log_sigma of every voxel, |hip - ref| <= 1e-4 A_ls (cases.FLOOR_LS: 4 x the case's float32
    floor), under both node-0 policies, which must not move it; masked-out voxels are exact zeros.  The rows at
    log sigma = -11 hold the kernels to the residual at the normalising image, where y and yhat are both within 1e-3 of
    1 (elbo_bwd_kernel's d_se; MEASUREMENTS.md section 23)."""
    c = cases.build(params, name)
    bound = 4.0 * FLOOR_LS[name] if name in FLOOR_LS else BOUND_LS
    failed = []
    got = {}
    for node0_grad in (True, False):
        _, gq, gls, _ = run(context, c, node0_grad)
        got[node0_grad] = gls
        ref = c.ref[node0_grad]
        _, rl = cases.worst_ratio(gq, gls, ref)
        print(f"{name} node0_grad={node0_grad}: log sigma, worst |d| / A_ls {rl:.2e} (bound {bound:.1e})")
        assert np.all(gls[c.mask == 0] == 0.0)
        over = entries_over(gls, ref["g_log_sigma"], ref["A_ls"], bound)
        if over:
            failed.append([node0_grad] + over)
    assert np.array_equal(got[True], got[False])
    assert not failed, failed


@pytest.mark.parametrize("name", list(cases.CASES))
def test_values_per_voxel(params, context, name):
    """The backward's own (nll, kl) rows and sums at their existing bounds: per voxel 2e-4 rel_1 on the Philox stream
    (DESIGN section 2), against the float64 oracle on the same draws; -ELBO within 1e-4; sum(mask) exact."""
    c = cases.build(params, name)
    sums, _, _, nk = run(context, c, True)
    ref = c.ref[True]
    inm = c.mask > 0
    e_nll = rel1(nk[inm, 0], ref["nll_v"][inm])
    e_kl = rel1(nk[inm, 1], ref["kl_v"][inm])
    want = ((c.mask * ref["nll_v"]).sum() + ref["kl_v"][inm].sum()) / c.mask.sum()
    got = (sums[0] + sums[1]) / sums[2]
    print(f"{name}: nll_v rel1 {e_nll:.2e}  kl_v rel1 {e_kl:.2e}  -ELBO rel {abs(got - want) / abs(want):.2e}")
    assert e_nll < 2e-4 and e_kl < 2e-4
    assert abs(got - want) < 1e-4 * abs(want)
    assert sums[2] == c.mask.sum()


def test_the_comparison_tells_the_policies_apart(params, context):
    """The default case's gradients under the shipped policy against the reference of the OTHER policy miss the bound by
    more than 10 x: the measure sees a node-0 term that is wrong or missing."""
    c = cases.build(params, cases.DEFAULT_CASE)
    for node0_grad in (True, False):
        _, gq, gls, _ = run(context, c, node0_grad)
        rq, _ = cases.worst_ratio(gq, gls, c.ref[not node0_grad])
        print(f"node0_grad={node0_grad} against the other policy's reference: {rq:.2e}")
        assert rq > 10 * BOUND_Q


@pytest.mark.parametrize("S", [3, 1])
def test_tile_stride(params, context, S):
    """N = N0 + 40 with N0 the voxels one pass of the grid covers (4 x CUs blocks of 256 lanes: 65,536 voxels at four
    lanes per voxel, S = 3, and 262,144 at one, S = 1, on the MI355X's 256 CUs), K = 2: the last 40 voxels land in the
    second iteration of block 0's tile loop.  One call equals, bit for bit, the two calls on [0, N0) and [N0, N) with
    voxel0 set (every voxel under the reach bound, so the per-wave choice of the KL form cannot differ), and the tail
    is held to the float64 reference."""
    K, seed = 2, 11
    c = cases.build(params, "t11_S3_K3_N257")
    ctx = context(c, True)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    N0 = 4 * n_cu * (256 // (4 if S > 2 else 1))   # qb::elbo_grid blocks of kBlock / LPV voxels
    N = N0 + 40
    idx = np.arange(N) % c.N
    q = cases.under_reach(c.q)[idx]
    x, mask, prior, ls = c.x[idx], c.mask[idx], c.prior[idx], c.ls[idx]
    t = [dev(a) for a in (x, mask, q, prior, ls)]
    s_all, gq, gl, nk = ctx.elbo_bwd(*t, S, K, seed=seed)
    parts = np.zeros(3)
    for lo, hi in ((0, N0), (N0, N)):
        sp, gqp, glp, nkp = ctx.elbo_bwd(*[a[lo:hi] for a in t], S, K, seed=seed, voxel0=lo)
        assert torch.equal(gqp, gq[lo:hi]) and torch.equal(glp, gl[lo:hi]) and torch.equal(nkp, nk[lo:hi]), (S, lo)
        parts += sp.cpu().numpy()
    assert np.allclose(parts, s_all.cpu().numpy(), rtol=1e-6, atol=0)
    zs = c.o32.philox_normals(seed, cases.STREAM_LIK, N0, 40, S).astype(np.float64)
    zk = c.o32.philox_normals(seed, cases.STREAM_KL, N0, 40, K).astype(np.float64)
    ref = elbo_bwd_reference(c.o64, x[N0:], mask[N0:], q[N0:], prior[N0:], np.exp(ls[N0:].astype(np.float64)), zs, zk,
                             True)
    rq, rl = cases.worst_ratio(gq[N0:].cpu().numpy(), gl[N0:].cpu().numpy(), ref)
    print(f"S={S} N={N}: tail worst |d| / A  heads {rq:.2e}  log sigma {rl:.2e}")
    assert rq <= BOUND_Q and rl <= BOUND_LS
