"""Float64 reference of the importance-weighted bound's head gradients (qbold_log_evidence_bwd), built from the CPU
oracle's primitives: _iw_reference.log_weights for the per-draw log w, _refine_reference's signal Jacobian by central
differences for d nll / du, the clipped-logit residuals of the two logit-space Gaussians for d (log q - log p) / du with
q held inside log q, and the raw-head chain.  Test infrastructure (no GPU needed)."""
import numpy as np

from _iw_reference import log_weights
from _refine_reference import DBV_RANGE, MIN_DBV, MIN_OEF, OEF_RANGE, _transformed, signal_jac_fd, to_raw

LOGIT_CLIP = np.log((1.0 - 1e-6) / 1e-6)   # model.py:393-396


def _chol_inv(p):
    """exp(s_o), exp(s_d), c and L^-1 = [[i_so, 0], [i_bl, i_sd]] of heads p [N, 5] (float64)."""
    so, sd, c = _transformed(p)
    i_so, i_sd = np.exp(-so), np.exp(-sd)
    return np.exp(so), np.exp(sd), c, i_so, i_sd, -np.exp(-so - sd) * c


def logits(q, z):
    """u = mu + L eps [N, K, 2] of heads q [N, 5] and normals z [N, K, 2]."""
    q = np.asarray(q, np.float64)
    z = np.asarray(z, np.float64)
    e_so, e_sd, c, *_ = _chol_inv(q)
    a = q[:, 0:1] + z[..., 0] * e_so[:, None]
    b = q[:, 2:3] + z[..., 0] * c[:, None] + z[..., 1] * e_sd[:, None]
    return np.stack([a, b], -1)


def nll_parts(o, x, q, sigma, z, jac=signal_jac_fd, scales=False):
    """Per draw: d nll / du [N, K, 2] (through forward_transform, the signal model and the normalisation) and
    d nll / d log sigma [N, K, T] (the NLL of fine_tune_loss_fn restated as in _refine_reference.nll_grad).
    jac(o, y) -> [V, T, 2] is the signal Jacobian (default: central differences of the value).  scales: also the
    cancellation-aware sizes of the two, the same sums with every per-tau term in absolute value and the residual
    entering as (|yt| + |yp|) / sigma (tests/_elbo_bwd_reference.py states the measure)."""
    u = logits(q, z)
    N, K = u.shape[:2]
    T = o.T
    sa, sb = 1.0 / (1.0 + np.exp(-u[..., 0])), 1.0 / (1.0 + np.exp(-u[..., 1]))
    y = np.stack([sa * OEF_RANGE + MIN_OEF, sb * DBV_RANGE + MIN_DBV], -1).reshape(-1, 2)
    pred = np.asarray(o.signal_fwd(y), np.float64).reshape(N, K, T)
    jac = np.asarray(jac(o, y), np.float64).reshape(N, K, T, 2)
    cfg = o.cfg
    se = cfg.se_idx
    w = np.zeros(T)
    if cfg.multi_image_normalisation:
        w[se - 1:se + 2] = 1.0 / 3.0
    else:
        w[se] = 1.0
    xx = np.asarray(x, np.float64)
    yt = xx / ((xx * w).sum(-1, keepdims=True) + 1e-3)
    npred = (pred * w).sum(-1, keepdims=True) + 1e-3
    v = pred / npred
    if cfg.predict_log_data:
        yt, yp, dyp = np.log(yt), np.log(v), 1.0 / v
    else:
        yp, dyp = v, np.ones_like(v)
    s = np.asarray(sigma, np.float64)[:, None, :]
    r = (yt[:, None, :] - yp) / s
    if cfg.use_student_t:
        df = cfg.student_t_df
        dr = (df + 1.0) * r / (df + r * r)
    else:
        dr = r
    gv = -dr / s * dyp
    gpred = gv / npred - (gv * pred).sum(-1, keepdims=True) / npred ** 2 * w
    ga = (gpred * jac[..., 0]).sum(-1) * OEF_RANGE * sa * (1.0 - sa)
    gb = (gpred * jac[..., 1]).sum(-1) * DBV_RANGE * sb * (1.0 - sb)
    if not scales:
        return np.stack([ga, gb], -1), 1.0 - dr * r
    wr = dr / np.where(r == 0.0, 1.0, r) if cfg.use_student_t else 1.0     # d nll / dr = wr r
    av = wr * (np.abs(yt[:, None, :]) + np.abs(yp)) / s / s * np.abs(dyp)
    a1 = (av * np.abs(pred)).sum(-1, keepdims=True) / npred ** 2
    au = [((av / np.abs(npred) * np.abs(jac[..., k])).sum(-1) + a1[..., 0] * (w * np.abs(jac[..., k])).sum(-1)) * f
          for k, f in ((0, OEF_RANGE * sa * (1.0 - sa)), (1, DBV_RANGE * sb * (1.0 - sb)))]
    return np.stack([ga, gb], -1), 1.0 - dr * r, np.stack(au, -1), 1.0 + np.abs(dr * r)


def kl_u_grad(q, prior, z, scales=False):
    """d (log q(u) - log p(u)) / du [N, K, 2] per draw with q held inside log q: L_p^-T w_p - L_q^-T w_q of the
    clipped logits (the clip passes gradient, model.py:395), as elbo_bwd_kernel's general KL loop.
    scales: also |L_p^-T w_p| + |L_q^-T w_q|, the size of the two terms before they cancel."""
    u = np.clip(logits(q, z), -LOGIT_CLIP, LOGIT_CLIP)
    g = a = 0.0
    for heads, sign in ((prior, 1.0), (q, -1.0)):
        h = np.asarray(heads, np.float64)
        _, _, _, i_so, i_sd, i_bl = _chol_inv(h)
        r0, r1 = u[..., 0] - h[:, 0:1], u[..., 1] - h[:, 2:3]
        w0, w1 = r0 * i_so[:, None], r1 * i_sd[:, None] + r0 * i_bl[:, None]
        t = np.stack([w0 * i_so[:, None] + w1 * i_bl[:, None], w1 * i_sd[:, None]], -1)
        g = g + sign * t
        a = a + np.abs(t)
    return (g, a) if scales else g


def chain_u(q, z, gu):
    """sum over the draws of gu [N, K, 2] du_k / d(mu_o, s_o, mu_d, s_d, c) -> [N, 5] (before the raw chain)."""
    e_so, e_sd, *_ = _chol_inv(np.asarray(q, np.float64))
    z = np.asarray(z, np.float64)
    ga, gb = gu[..., 0], gu[..., 1]
    return np.stack([ga.sum(1), (ga * z[..., 0]).sum(1) * e_so, gb.sum(1), (gb * z[..., 1]).sum(1) * e_sd,
                     (gb * z[..., 0]).sum(1)], -1)


def softmax(lw):
    e = np.exp(lw - lw.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def iw_grad_reference(o, x, q, prior, sigma, z, mask=None, jac=signal_jac_fd):
    """dict(g_q [N, 5] (DReG, raw heads), g_log_sigma [N, T], log_p, lw [N, K], w [N, K] normalised weights, A_q, A_ls),
    the outputs of qbold_log_evidence_bwd for explicit normals z [N, K, 2] (unnormalised by sum(mask); mask None = 1).
    jac: the signal Jacobian, as nll_parts.  A_q [N, 5], A_ls [N, T]: the same sums with every per-draw term in absolute
    value (nll_parts' and kl_u_grad's scales), the per-voxel measure of tests/_elbo_bwd_reference.py."""
    q = np.asarray(q, np.float64)
    N, K = np.asarray(z).shape[:2]
    m = np.ones(N) if mask is None else np.where(np.asarray(mask, np.float64) > 0, np.asarray(mask, np.float64), 0.0)
    lw, _ = log_weights(o, x, q, prior, sigma, z)
    w = softmax(lw)
    gn_u, gn_ls, an_u, an_ls = nll_parts(o, x, q, sigma, z, jac=jac, scales=True)
    gk_u, ak_u = kl_u_grad(q, prior, z, scales=True)
    h = gn_u + gk_u                                 # -(d log w / du) with q held
    g_q = to_raw(q, chain_u(q, z, (w ** 2)[..., None] * h)) * m[:, None]
    g_ls = (w[..., None] * gn_ls).sum(1) * m[:, None]
    A_q = np.abs(to_raw(q, chain_u(q, np.abs(z), (w ** 2)[..., None] * (an_u + ak_u)))) * m[:, None]
    A_ls = (w[..., None] * an_ls).sum(1) * m[:, None]
    M = lw.max(1)
    log_p = M + np.log(np.exp(lw - M[:, None]).sum(1)) - np.log(K)
    return dict(g_q=g_q, g_log_sigma=g_ls, log_p=log_p, lw=lw, w=w, A_q=A_q, A_ls=A_ls)


def frozen_log_weights(o, x, q, q_frozen, prior, sigma, z):
    """log w_k [N, K] with the draws u_k(q) but log q evaluated with the parameters q_frozen: the f_k whose
    stop(w~^2)-weighted gradient is DReG's."""
    z = np.asarray(z, np.float64)
    N, K = z.shape[:2]
    T = o.T

    def rep(a, c):
        return np.repeat(np.asarray(a, np.float64).reshape(N, c), K, axis=0)

    y = o.reparam(rep(q, 5), z.reshape(-1, 2))
    nll = o.nll(rep(x, T), np.ones(N * K), o.signal_fwd(y), rep(sigma, T)).reshape(N, K)
    log_q = -o.logit_mvn_nlogp(y, rep(q_frozen, 5)).reshape(N, K)
    log_p = -o.logit_mvn_nlogp(y, rep(prior, 5)).reshape(N, K)
    return -nll - (log_q - log_p)


def neg_log_p(o, x, q, prior, sigma, z):
    """-log p^_K [N] for explicit normals: the per-voxel loss."""
    lw, _ = log_weights(o, x, q, prior, sigma, z)
    M = lw.max(1)
    return -(M + np.log(np.exp(lw - M[:, None]).sum(1)) - np.log(lw.shape[1]))
