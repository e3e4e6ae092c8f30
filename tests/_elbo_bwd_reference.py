"""Float64 reference of the ELBO head gradients (qbold_elbo_bwd: g_q [N, 5], g_log_sigma [N, T]) as a closed
expression, composed from the pinned pieces: _iw_grad_reference.nll_parts (the per-draw likelihood gradient through
forward_transform, the signal model and the normalisation), kl_u_grad (the per-draw gradient of log q - log p through
the sample, q's own parameters held, the clip passing gradient) and chain_u (draws -> logit-space parameters), then
the raw-head chain with sech^2 taken directly.  Test infrastructure (CPU only, no torch).

    g_q  = chain( m mean_s d nll_s / du  (+)  [m > 0] mean_k d (log q - log p)_k / du )
    g_ls = m mean_s (1 - dr_s r_s)

The signal Jacobian is the policy under test (qbold_ctx_set_grad_node0):
    node0_grad = False  central differences of the value with Simpson node 0 flat (what float32 computes): the exact
                        derivative of the loss value;
    node0_grad = True   the oracle's analytic signal_jac, the J1 sum over ALL nodes, over that same value: the library's
                        default and TensorFlow's gradient.

The measure.  An entry is compared as |got - ref| <= bound * A, where A is the SAME sum as the entry with every
per-draw, per-tau term in absolute value, so that an entry which is small because its terms cancel is held to the size
of the terms and not to the size of what is left:
    likelihood, per draw and logit (nll_parts, scales=True), with a_t = w_r (|yt_t| + |yp_t|) / sigma_t^2 |d yp / d v|_t
    (w_r = 1, Student-t: (df + 1) / (df + r^2); the residual enters as (|yt| + |yp|) / sigma, not |yt - yp| / sigma):
        A_u = [ sum_t a_t / np |J_t|  +  (sum_t a_t |pred_t|) / np^2  sum_t w_t |J_t| ]  range s (1 - s)
        (the direct half and the normalisation half of d nll / d pred, each in absolute value);
    KL, per draw (kl_u_grad, scales=True):  A_u = |L_p^-T w_p| + |L_q^-T w_q|;
    both through chain_u with |z| in place of z, weighted m / S and [m > 0] / K, times |d head / d raw|:  A_q [N, 5];
    log sigma:  A_ls = m mean_s (1 + |dr_s r_s|)  [N, T].
A masked-out voxel has A = 0 and its gradients are exact zeros."""
import numpy as np

from _iw_grad_reference import chain_u, kl_u_grad, nll_parts
from _refine_reference import E2, signal_jac_fd


def analytic_jac(o, y):
    """The oracle's closed-form signal Jacobian [V, T, 2]: the J1 Simpson sum over all 129 nodes."""
    return o.signal_jac(y)


def raw_chain(q):
    """d (mu_o, s_o, mu_d, s_d, c) / d raw heads [N, 5]: transform_std / transform_offdiag with sech^2 = 1 / cosh^2
    (no 1 - tanh^2: nothing to cancel as a head saturates)."""
    q = np.asarray(q, np.float64)
    f = np.ones_like(q)
    f[:, 1] = 3.0 / np.cosh(q[:, 1]) ** 2
    f[:, 3] = 3.0 / np.cosh(q[:, 3]) ** 2
    f[:, 4] = E2 / np.cosh(q[:, 4]) ** 2
    return f


def draw_mean(q, z, gu):
    """mean over the draws of chain_u; no draws (K = 0): zeros."""
    n = np.asarray(z).shape[1]
    return chain_u(q, z, gu) / n if n else np.zeros((np.asarray(q).shape[0], 5))


def elbo_bwd_reference(o, x, mask, q, prior, sigma, zs, zk, node0_grad):
    """dict(g_q [N, 5], g_log_sigma [N, T], A_q, A_ls, nll_v [N], kl_v [N]) for likelihood normals zs [N, S, 2] and KL
    normals zk [N, K, 2] (K may be 0); o: the oracle whose primitives are used, Oracle("f64", ..., node0_zero=True) for
    the reference proper.  The node-0 policy of o's C library is switched on for the call and back to 0 after it."""
    q = np.asarray(q, np.float64)
    zs, zk = np.asarray(zs, np.float64), np.asarray(zk, np.float64)
    N = q.shape[0]
    m = np.asarray(mask, np.float64).reshape(N)
    inm = (m > 0).astype(np.float64)
    o.lib.qbo_set_node0_zero(1)
    try:
        gn_u, gn_ls, an_u, an_ls = nll_parts(o, x, q, sigma, zs, jac=analytic_jac if node0_grad else signal_jac_fd,
                                             scales=True)
        e = o.elbo(x, m, q, prior, sigma, zs, zk) if zk.shape[1] else o.elbo(x, m, q, prior, sigma, zs,
                                                                             np.zeros((N, 1, 2)))
    finally:
        o.lib.qbo_set_node0_zero(0)
    gk_u, ak_u = kl_u_grad(q, prior, zk, scales=True) if zk.shape[1] else (np.zeros((N, 0, 2)),) * 2
    f = raw_chain(q)
    g = m[:, None] * draw_mean(q, zs, gn_u) + inm[:, None] * draw_mean(q, zk, gk_u)
    A = m[:, None] * draw_mean(q, np.abs(zs), an_u) + inm[:, None] * draw_mean(q, np.abs(zk), ak_u)
    kl_v = np.asarray(e["kl_v"], np.float64) if zk.shape[1] else np.zeros(N)
    return dict(g_q=g * f, g_log_sigma=m[:, None] * gn_ls.mean(1), A_q=np.abs(A) * f,
                A_ls=m[:, None] * an_ls.mean(1), nll_v=np.asarray(e["nll_v"], np.float64), kl_v=kl_v)
