"""tests/_elbo_bwd_reference.py held on the CPU: against central differences of the float64 oracle's loss, at a clip
that binds, under both node-0 policies, against the same composition on float32 primitives (the floor of
test_gpu_elbo_bwd_reference's bounds), and against seven mutated references that the bounds must tell apart."""
import numpy as np
import pytest

import _elbo_bwd_cases as cases
from _elbo_bwd_reference import analytic_jac, draw_mean, elbo_bwd_reference, raw_chain
from _iw_grad_reference import LOGIT_CLIP, kl_u_grad, logits
from _refine_reference import signal_jac_fd

BOUND_Q, BOUND_LS = 2e-4, 1e-4    # test_gpu_elbo_bwd_reference's
FD_TOL = 1e-7


def kl_stopgrad(o, q_sample, q_logq, prior, zk):
    """mean_k [log q_sg(y_k) - log p(y_k)], y_k = reparam(q_sample, z_k) (test_gpu_grad.kl_stopgrad)."""
    acc = 0.0
    for k in range(zk.shape[1]):
        y = o.reparam(q_sample, zk[:, k])
        acc = acc + o.logit_mvn_nlogp(y, prior) - o.logit_mvn_nlogp(y, q_logq)
    return acc / zk.shape[1]


def fd_gradients(o64, x, mask, q, prior, ls, zs, zk, h=1e-5, kl=kl_stopgrad):
    """Central differences of the float64 loss m nll_v + [m > 0] kl in every head and every log-sigma column."""
    q64, ls = np.asarray(q, np.float64), np.asarray(ls, np.float64)
    o64.lib.qbo_set_node0_zero(1)
    try:
        def loss(qq, lss):
            e = o64.elbo(x, mask, qq, prior, np.exp(lss), zs, zk)
            return e["nll_v"] * mask + np.where(mask > 0, kl(o64, qq, q64, prior, zk), 0.0)
        gq, gl = np.zeros_like(q64), np.zeros_like(ls)
        for k in range(5):
            d = np.zeros_like(q64)
            d[:, k] = h
            gq[:, k] = (loss(q64 + d, ls) - loss(q64 - d, ls)) / (2 * h)
        for t in range(ls.shape[1]):
            d = np.zeros_like(ls)
            d[:, t] = h
            gl[:, t] = (loss(q64, ls + d) - loss(q64, ls - d)) / (2 * h)
    finally:
        o64.lib.qbo_set_node0_zero(0)
    return gq, gl


def small_case(params, T, variant, n=48, S=3, K=7, seed=11, edit="kl_under"):
    """48 voxels, S = 3, K = 7 on the Philox streams; kl_under keeps every draw off the clip."""
    p, o32, o64 = cases.oracles(params, T, variant)
    x, mask, q, prior, ls = cases.inputs(o32, T, n)
    q, ls = cases.EDITS[edit](q, ls, None)
    zs = o32.philox_normals(seed, 0, 0, n, S).astype(np.float64)
    zk = o32.philox_normals(seed, 1, 0, n, K).astype(np.float64)
    return o32, o64, x, mask, q, prior, ls, zs, zk


@pytest.mark.parametrize("variant", [{}, dict(student_t_df=2.0, multi_image_normalisation=True),
                                     dict(predict_log_data=True)], ids=["gaussian", "student2_multi", "log_data"])
@pytest.mark.parametrize("T", [11, 24, 12])
def test_reference_is_the_derivative_of_the_value(params, T, variant):
    """node0_grad = False: every head and every log-sigma column of every voxel equals central differences (h = 1e-5) of
    the float64 oracle's loss to 1e-7 of A (heads 7e-11 -- 8e-10, log sigma 2e-10 -- 3e-8 here: the differences' own
    truncation and rounding)."""
    o32, o64, x, mask, q, prior, ls, zs, zk = small_case(params, T, variant)
    assert cases.draws_at_clip(q, zk).sum() == 0
    ref = elbo_bwd_reference(o64, x, mask, q, prior, np.exp(ls.astype(np.float64)), zs, zk, False)
    gq, gl = fd_gradients(o64, x, mask, q, prior, ls, zs, zk)
    rq, rl = cases.worst_ratio(gq, gl, ref)
    print(f"T={T} {variant}: reference against central differences, worst |d| / A  heads {rq:.2e}  log sigma {rl:.2e}")
    assert rq < FD_TOL and rl < FD_TOL
    assert np.all(ref["g_q"][mask == 0] == 0) and np.all(ref["g_log_sigma"][mask == 0] == 0)
    # the value the reference reports is the oracle's
    e = o64.elbo(x, mask, q, prior, np.exp(ls.astype(np.float64)), zs, zk)
    assert np.allclose(ref["kl_v"], e["kl_v"], rtol=1e-12)


def kl_part(o64, x, mask, q, prior, sigma, zs, zk, node0_grad=False):
    """(whole reference, its KL part, its likelihood part): the likelihood part is the reference at K = 0."""
    full = elbo_bwd_reference(o64, x, mask, q, prior, sigma, zs, zk, node0_grad)
    lik = elbo_bwd_reference(o64, x, mask, q, prior, sigma, zs, np.zeros((len(q), 0, 2)), node0_grad)
    return full, full["g_q"] - lik["g_q"], lik


def test_a_clip_that_binds_passes_gradient(params):
    """Draws beyond the clip in both logits and both signs: the KL part equals Sigma_p^-1 (u - mu_p) - Sigma_q^-1
    (u - mu_q) at the clipped u, written out draw by draw with explicit covariances and d u / d theta of the UNCLIPPED
    sample (tfp clip_by_value_preserve_gradient); central differences of the value, which see the clip's zero slope,
    differ from it by more than 1e-2 of A."""
    o32, o64, x, mask, q, prior, ls, zs, zk = small_case(params, 11, {}, K=70, edit="kl_clip_binds")
    assert cases.draws_at_clip(q, zk).min() >= 5
    sigma = np.exp(ls.astype(np.float64))
    full, gk, _ = kl_part(o64, x, mask, q, prior, sigma, zs, zk)
    q64, p64 = q.astype(np.float64), prior.astype(np.float64)
    want = np.zeros((len(q), 5))

    def gauss(h):
        so, sd = 3.0 * np.tanh(h[1]) - 1.0, 3.0 * np.tanh(h[3]) - 1.0
        L = np.array([[np.exp(so), 0.0], [np.tanh(h[4]) * np.exp(-2.0), np.exp(sd)]])
        return np.array([h[0], h[2]]), L

    for v in range(len(q)):
        if mask[v] <= 0:
            continue
        (mq, Lq), (mp, Lp) = gauss(q64[v]), gauss(p64[v])
        for z in zk[v]:
            u = np.clip(mq + Lq @ z, -LOGIT_CLIP, LOGIT_CLIP)
            gu = np.linalg.solve(Lp @ Lp.T, u - mp) - np.linalg.solve(Lq @ Lq.T, u - mq)
            # d u / d (mu_o, raw s_o, mu_d, raw s_d, raw c), rows u_0, u_1
            J = np.array([[1.0, z[0] * Lq[0, 0] * 3.0 / np.cosh(q64[v, 1]) ** 2, 0.0, 0.0, 0.0],
                          [0.0, 0.0, 1.0, z[1] * Lq[1, 1] * 3.0 / np.cosh(q64[v, 3]) ** 2,
                           z[0] * np.exp(-2.0) / np.cosh(q64[v, 4]) ** 2]])
            want[v] += gu @ J / zk.shape[1]
    err = np.abs(gk - want)
    assert np.all(err <= 1e-10 * full["A_q"])
    gq, gl = fd_gradients(o64, x, mask, q, prior, ls, zs, zk)
    rq, rl = cases.worst_ratio(gq, gl, full)
    print(f"clip binds: central differences against the reference, heads {rq:.2e}, log sigma {rl:.2e}")
    assert rq > 1e-2 and rl < FD_TOL


def node0_jacobian_term(o, y):
    """Node 0's share of d signal / d OEF [V, T], written out: -DBV dF_0(x_t) (x_t / OEF) (1 - bw) e^(-DBV F(x_t)) e^(-TE
    R2t), x_t = tau_t dw OEF, with dF_0 = (the J1 sum over all nodes, qbo_tissue_dF) - (the slope of F with node 0
    flat, by central differences of qbo_tissue_F)."""
    p = {k: float(v) for k, v in o.params.items()}
    y = np.asarray(y, np.float64)
    oef, dbv = y[:, 0:1], y[:, 1:2]
    dw_coef = (4.0 / 3.0) * np.pi * p["gamma"] * p["b0"] * p["dchi"] * p["hct"]
    x = o.taus[None, :].astype(np.float64) * dw_coef * oef
    h = 1e-6 * np.maximum(np.abs(x), 1e-3)
    dF0 = o.tissue_dF(x) - (o.tissue_F(x + h) - o.tissue_F(x - h)) / (2.0 * h)
    m_bld = 1.0 - (2.0 - np.exp(-(p["tr"] - p["ti"]) / p["t1b"])) * np.exp(-p["ti"] / p["t1b"])
    tw = 1.0 - m_bld * 0.775 * dbv
    return -dbv * dF0 * (x / oef) * tw * np.exp(-dbv * o.tissue_F(x)) * np.exp(-p["te"] * p["r2t"])


def test_the_two_node0_policies(params):
    """On the default case the shipped policy (the J1 sum over all nodes) moves some voxel's head gradient by at least
    5e-3 of A_q; and it is exactly the derivative of the value plus node 0's slope term, restated in NumPy."""
    c = cases.build(params, cases.DEFAULT_CASE)
    rq, rl = cases.worst_ratio(c.ref[False]["g_q"], c.ref[False]["g_log_sigma"], c.ref[True])
    print(f"default case: the two policies differ by {rq:.2e} of A_q")
    assert rq >= 5e-3 and rl == 0.0
    y = np.stack([np.linspace(0.05, 0.8, 40), np.linspace(0.003, 0.19, 40)[::-1]], -1)
    o = c.o64
    o.lib.qbo_set_node0_zero(1)
    try:
        ja, jf, term = analytic_jac(o, y), signal_jac_fd(o, y), node0_jacobian_term(o, y)
    finally:
        o.lib.qbo_set_node0_zero(0)
    scale = np.abs(ja).max(axis=(0, 1))
    assert np.abs(term).max() > 1e-3 * scale[0]
    assert np.abs(ja[..., 0] - (jf[..., 0] + term)).max() < 1e-8 * scale[0]
    assert np.abs(ja[..., 1] - jf[..., 1]).max() < 1e-8 * scale[1]
    # ... and through the whole composition (the gradient is linear in the Jacobian)
    import _elbo_bwd_reference as R
    keep = R.analytic_jac
    R.analytic_jac = lambda oo, yy: signal_jac_fd(oo, yy) + np.stack(
        [node0_jacobian_term(oo, np.asarray(yy, np.float64).reshape(-1, 2)), np.zeros((np.asarray(yy).size // 2, oo.T))], -1)
    try:
        alt = elbo_bwd_reference(o, c.x, c.mask, c.q, c.prior, c.sigma, c.zs, c.zk, True)
    finally:
        R.analytic_jac = keep
    rq, rl = cases.worst_ratio(alt["g_q"], alt["g_log_sigma"], c.ref[True])
    print(f"value's derivative + node-0 term against the analytic policy: {rq:.2e}")
    assert rq < FD_TOL


def test_float32_floor(params):
    """The same composition on the float32 oracle's primitives with the analytic Jacobian, against float64, on every
    case of the GPU test: what float32 noise of the literal reference alone does under the A measure.  The heads' floor
    stays under a quarter of their bound everywhere; for log sigma a case bounded at 4 x its floor (cases.FLOOR_LS)
    carries a recorded floor that is above a quarter of the bound and not above the one measured here."""
    worst = {}
    for name in cases.CASES:
        c = cases.build(params, name)
        f32 = elbo_bwd_reference(c.o32, c.x, c.mask, c.q, c.prior, c.sigma, c.zs, c.zk, True)
        worst[name] = cases.worst_ratio(f32["g_q"], f32["g_log_sigma"], c.ref[True])
        print(f"{name:32s} float32 floor: heads {worst[name][0]:.2e}  log sigma {worst[name][1]:.2e}")
    assert max(w[0] for w in worst.values()) < BOUND_Q / 4
    for name, floor in cases.FLOOR_LS.items():
        assert BOUND_LS / 4 < floor <= 1.02 * worst[name][1], (name, floor, worst[name][1])


# ---- teeth ----------------------------------------------------------------------------------------------------------
def misses(gq, gl, ref):
    """By how many bounds the worst entry of (gq, gl) misses ref."""
    rq, rl = cases.worst_ratio(gq, gl, ref)
    return max(rq / BOUND_Q, rl / BOUND_LS)


def test_teeth(params):
    """Seven references with one thing wrong each miss the true one by at least 10 x the GPU test's bound on some entry."""
    c = cases.build(params, cases.DEFAULT_CASE)           # T = 11, S = 3, K = 3, N = 257
    ref = c.ref[True]
    inm = (c.mask > 0).astype(np.float64)[:, None]
    table = {}
    # 1. the node-0 policy swapped
    table["node-0 policy swapped"] = misses(c.ref[False]["g_q"], c.ref[False]["g_log_sigma"], ref)
    # 2. log q's own parameters differentiated: the KL part by central differences of the whole kl_samples
    full, gk, lik = kl_part(c.o64, c.x, c.mask, c.q, c.prior, c.sigma, c.zs, c.zk, True)
    q64 = c.q.astype(np.float64)
    g_all = np.zeros_like(q64)
    for k in range(5):
        d = np.zeros_like(q64)
        d[:, k] = 1e-5
        g_all[:, k] = (c.o64.kl_samples(q64 + d, c.prior, c.zk) - c.o64.kl_samples(q64 - d, c.prior, c.zk)) / 2e-5
    table["stop-gradient dropped"] = misses(lik["g_q"] + inm * g_all, ref["g_log_sigma"], ref)
    # 4. draws weighted 1 / (4 ceil(S / 4)) instead of 1 / S
    w = c.S / (4.0 * ((c.S + 3) // 4))
    table["1 / Sp for 1 / S"] = misses(gk + w * lik["g_q"], w * ref["g_log_sigma"], ref)
    # 6. one tau's g_log_sigma contribution dropped (the last draw's, at the last tau)
    gl = ref["g_log_sigma"].copy()
    gl[:, -1] *= (c.S - 1.0) / c.S
    table["one tau's log-sigma term dropped"] = misses(ref["g_q"], gl, ref)
    # 7. [m > 0] replaced by m on the KL part (shows at m = 0.5)
    assert (c.mask == 0.5).any()
    table["m for [m > 0]"] = misses(lik["g_q"] + c.mask[:, None] * gk, ref["g_log_sigma"], ref)
    # 3. the clip blocking gradient, where it binds
    cb = cases.build(params, "kl_clip_binds_S1")
    rb = cb.ref[True]
    gu = kl_u_grad(cb.q, cb.prior, cb.zk)
    inside = (np.abs(logits(cb.q, cb.zk)) < LOGIT_CLIP).astype(np.float64)
    delta = (draw_mean(cb.q, cb.zk, gu * inside) - draw_mean(cb.q, cb.zk, gu)) * raw_chain(cb.q)
    table["clip blocks gradient"] = misses(rb["g_q"] + (cb.mask > 0)[:, None] * delta, rb["g_log_sigma"], rb)
    # 5. the last Philox call's short count ignored: K = 70 summed as 72 draws
    c70 = cases.build(params, "t11_S1_K70_N257")
    r70 = c70.ref[True]
    z72 = c70.o32.philox_normals(c70.seed, cases.STREAM_KL, 0, c70.N, 72).astype(np.float64)
    assert np.array_equal(z72[:, :70], c70.zk)
    extra = draw_mean(c70.q, z72[:, 70:], kl_u_grad(c70.q, c70.prior, z72[:, 70:])) * (2.0 / 70.0) * raw_chain(c70.q)
    table["K = 70 summed as 72"] = misses(r70["g_q"] + (c70.mask > 0)[:, None] * extra, r70["g_log_sigma"], r70)
    for k, v in table.items():
        print(f"{k:36s} misses by {v:8.1f} bounds")
    assert len(table) == 7 and min(table.values()) >= 10.0, table
