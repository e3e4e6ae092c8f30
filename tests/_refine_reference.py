"""Float64 reference of the per-voxel refinement (qbold_refine_posterior), built from the CPU oracle's primitives:
reparam -> signal_fwd (and its central differences for the signal Jacobian) for the reparameterised NLL gradient
(the NLL of fine_tune_loss_fn restated in NumPy, Gaussian or Student-t, linear or log data, one- or three-image normalisation), the closed-form KL(q || prior)
of the two logit-space Gaussians and its gradient, both chained to the raw heads through transform_std /
transform_offdiag, then SGD or bias-corrected Adam on a cosine learning rate.  Test infrastructure (no GPU needed)."""
import numpy as np

OEF_RANGE, MIN_OEF = 0.8, 0.04     # forward_transform
DBV_RANGE, MIN_DBV = 0.2, 0.001
E2 = np.exp(-2.0)                  # transform_offdiag's factor


def padded_draws(S):
    """Sp = 4 ceil(S / 4): a step's slot in the draw stream."""
    return 4 * ((S + 3) // 4)


def _transformed(q):
    so, sd = 3.0 * np.tanh(q[:, 1]) - 1.0, 3.0 * np.tanh(q[:, 3]) - 1.0
    return so, sd, np.tanh(q[:, 4]) * E2


def signal_jac_fd(o, y, h=1e-6):
    """d signal / d(OEF, DBV) [V, T, 2] by central differences of the float64 signal model (relative step h)."""
    y = np.asarray(y, np.float64)
    cols = []
    for k in range(2):
        d = np.zeros_like(y)
        d[:, k] = h * y[:, k]
        cols.append((np.asarray(o.signal_fwd(y + d), np.float64) - np.asarray(o.signal_fwd(y - d), np.float64)) /
                    (2.0 * d[:, k:k + 1]))
    return np.stack(cols, -1)


def nll_grad(o, x, q, sigma, z, jac=None, scales=False):
    """Mean over the S draws of d nll(x | reparam(q, z_s)) / d(mu_o, s_o, mu_d, s_d, c) [N, 5] (logit-space parameters,
    before the raw chain); z [N, S, 2].  jac(o, y) -> [V, T, 2]: the signal Jacobian (None: signal_jac_fd).  scales:
    also the same mean with every per-tau, per-draw term in absolute value and the residual entering as
    (|yt| + |yp|) / sigma (the per-voxel measure of tests/_elbo_bwd_reference.py)."""
    q = np.asarray(q, np.float64)
    z = np.asarray(z, np.float64)
    N, S = z.shape[:2]
    T = o.T
    so, sd, c = _transformed(q)
    z0, z1 = z[..., 0], z[..., 1]
    a = q[:, 0:1] + z0 * np.exp(so)[:, None]
    b = q[:, 2:3] + z0 * c[:, None] + z1 * np.exp(sd)[:, None]
    sa, sb = 1.0 / (1.0 + np.exp(-a)), 1.0 / (1.0 + np.exp(-b))
    y = np.stack([sa * OEF_RANGE + MIN_OEF, sb * DBV_RANGE + MIN_DBV], -1).reshape(-1, 2)
    pred = np.asarray(o.signal_fwd(y), np.float64).reshape(N, S, T)
    jac = np.asarray((jac or signal_jac_fd)(o, y), np.float64).reshape(N, S, T, 2)
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
    u = pred / npred
    if cfg.predict_log_data:
        yt, yp, dyp = np.log(yt), np.log(u), 1.0 / u
    else:
        yp, dyp = u, np.ones_like(u)
    s = np.asarray(sigma, np.float64)[:, None, :]
    r = (yt[:, None, :] - yp) / s
    if cfg.use_student_t:
        df = cfg.student_t_df
        dr = (df + 1.0) * r / (df + r * r)
    else:
        dr = r
    gu = -dr / s * dyp                                          # d nll / d u_t
    gpred = gu / npred - (gu * pred).sum(-1, keepdims=True) / npred ** 2 * w
    g_oef = (gpred * jac[..., 0]).sum(-1)
    g_dbv = (gpred * jac[..., 1]).sum(-1)
    ga = g_oef * OEF_RANGE * sa * (1.0 - sa)
    gb = g_dbv * DBV_RANGE * sb * (1.0 - sb)
    g = np.stack([ga, ga * z0 * np.exp(so)[:, None], gb, gb * z1 * np.exp(sd)[:, None], gb * z0], -1)
    if not scales:
        return g.mean(1)
    wr = dr / np.where(r == 0.0, 1.0, r) if cfg.use_student_t else 1.0     # d nll / dr = wr r
    av = wr * (np.abs(yt[:, None, :]) + np.abs(yp)) / s / s * np.abs(dyp)
    a1 = (av * np.abs(pred)).sum(-1, keepdims=True) / npred ** 2
    aa, ab = [((av / np.abs(npred) * np.abs(jac[..., k])).sum(-1) + a1[..., 0] * (w * np.abs(jac[..., k])).sum(-1)) * f
              for k, f in ((0, OEF_RANGE * sa * (1.0 - sa)), (1, DBV_RANGE * sb * (1.0 - sb)))]
    a0, a1z = np.abs(z0), np.abs(z1)
    A = np.stack([aa, aa * a0 * np.exp(so)[:, None], ab, ab * a1z * np.exp(sd)[:, None], ab * a0], -1)
    return g.mean(1), A.mean(1)


def kl_closed_and_grad(q, prior):
    """The exact KL(q || prior) [N] of the two logit-space Gaussians -- the expectation of the Monte-Carlo KL
    (Oracle.kl_samples) -- and its gradient with respect to (mu_o, s_o, mu_d, s_d, c) of q.  Oracle.kl_closed (mvg_kl,
    model.py:612-652) is the same number when the prior's off-diagonal head is 0; otherwise its trace term
    tr(L_p^-1 L_p^-T Sigma_q) is not tr(Sigma_p^-1 Sigma_q) and it differs (test_refine_host)."""
    q = np.asarray(q, np.float64)
    p = np.asarray(prior, np.float64)
    qso, qsd, qc = _transformed(q)
    pso, psd, pc = _transformed(p)
    # L_p^-1 = [[i_so, 0], [i_bl, i_sd]]
    i_so, i_sd = np.exp(-pso), np.exp(-psd)
    i_bl = -np.exp(-pso - psd) * pc
    d0 = (q[:, 0] - p[:, 0]) * i_so
    d1 = (q[:, 2] - p[:, 2]) * i_sd + (q[:, 0] - p[:, 0]) * i_bl
    m00, m10, m11 = np.exp(qso) * i_so, qc * i_sd + np.exp(qso) * i_bl, np.exp(qsd) * i_sd
    kl = 0.5 * (m00 ** 2 + m10 ** 2 + m11 ** 2 + d0 ** 2 + d1 ** 2) - (qso + qsd) + (pso + psd) - 1.0
    g = np.stack([d0 * i_so + d1 * i_bl, m00 ** 2 + m10 * np.exp(qso) * i_bl - 1.0, d1 * i_sd, m11 ** 2 - 1.0,
                  m10 * i_sd], -1)
    return kl, g


def to_raw(q, g):
    """Chain a gradient with respect to (mu_o, s_o, mu_d, s_d, c) to the raw heads."""
    q = np.asarray(q, np.float64)
    out = np.array(g, np.float64, copy=True)
    out[:, 1] *= 3.0 * (1.0 - np.tanh(q[:, 1]) ** 2)
    out[:, 3] *= 3.0 * (1.0 - np.tanh(q[:, 3]) ** 2)
    out[:, 4] *= E2 * (1.0 - np.tanh(q[:, 4]) ** 2)
    return out


def step_grad(o, x, q, prior, sigma, z, jac=None, scales=False):
    """d/d raw heads of mean_s nll(x | reparam(q, z_s)) + KL(q || prior) [N, 5]: one refinement step's gradient.
    jac: the signal Jacobian, as nll_grad.  scales: also A [N, 5], nll_grad's absolute sums plus |d KL| through the
    same chain."""
    _, gk = kl_closed_and_grad(q, prior)
    if not scales:
        return to_raw(q, nll_grad(o, x, q, sigma, z, jac=jac) + gk)
    gn, an = nll_grad(o, x, q, sigma, z, jac=jac, scales=True)
    return to_raw(q, gn + gk), np.abs(to_raw(q, an + np.abs(gk)))


def cosine_lr(j, steps, lr, lr_final):
    return lr_final + 0.5 * (lr - lr_final) * (1.0 + np.cos(np.pi * j / steps))


def refine_reference(o, x, q, prior, sigma, z, S, lr, lr_final=None, optimizer="adam", betas=(0.9, 0.999),
                     eps=1e-8):
    """The whole loop in float64; z [N, steps, Sp, 2] as the kernel takes it (draws S .. Sp - 1 of a step unused)."""
    z = np.asarray(z, np.float64)
    steps = z.shape[1]
    lr_final = lr if lr_final is None else lr_final
    qv = np.array(q, np.float64, copy=True)
    m1 = np.zeros_like(qv)
    m2 = np.zeros_like(qv)
    b1, b2 = betas
    for j in range(steps):
        g = step_grad(o, x, qv, prior, sigma, z[:, j, :S])
        lr_j = cosine_lr(j, steps, lr, lr_final)
        if optimizer == "adam":
            m1 = b1 * m1 + (1.0 - b1) * g
            m2 = b2 * m2 + (1.0 - b2) * g * g
            qv = qv - lr_j * (m1 / (1.0 - b1 ** (j + 1))) / (np.sqrt(m2 / (1.0 - b2 ** (j + 1))) + eps)
        else:
            qv = qv - lr_j * g
    return qv
