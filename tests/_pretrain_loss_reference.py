"""Analytic reference of the pre-training loss terms and of the diagonal-family KL, value and head gradient per voxel:
qbold_synth_loss_bwd (synth_loss), qbold_hyper_prior_bwd (hyper_prior), qbold_r2p_loss_bwd (r2p_loss), qbold_kl_diag
(kl_diag) and qbold_kl_mog (kl_mog, value only).  NumPy only, CPU.  Each function returns a dict of arrays: the
per-voxel value `v`, `g_q` [N, 5] = d v / d raw heads, and the scales `A_v` [N], `A_q` [N, 5].

dt = np.float64 is the reference: inputs are the float32 data cast to float64, the raw-head slopes are sech^2 =
1 / cosh^2 taken directly.  dt = np.float32 is the same formulas evaluated in float32 (sech^2 as 4 e / (e + 1)^2):
the floor of the bounds, and the carrier of the planted defects of test_pretrain_loss_host (`defect`).

The measure.  An entry is compared as |got - ref| <= bound * A, where A is the same expression as the entry with
every term in absolute value (for g_q times |d head / d raw|), so that an entry which is small because its terms
cancel is held to the size of the terms:
    synth_loss  r0 = logit(x0) - mu_o enters as |log x0| + |log(1 - x0)| + |mu_o|, likewise r1; w0, w1 are built from
                those; 1 - w0^2 - w1 r0 i_bl enters as 1 + w0^2 + |w1| |r0| |i_bl|; the inverse-gamma slope
                (a + 1) / x - b / x^2 as (a + 1) / x + b / x^2;
    hyper_prior 2 (a + 1) - 2 b / v as 2 (a + 1) + 2 b / v;
    r2p_loss    d nll / d r_k = -dy / (n var) + (1 - dy^2 / var) (r_k - mean) / (n var) enters as
                |dy| / (n var) + (1 + dy^2 / var) |r_k - mean| / (n var), and the sums over the draws are sums of
                absolute values (dy = y - mean and r_k - mean are taken as terms: the cases keep var >= 1e-6 mean^2);
    kl_diag     expm1(2 d) = exp(2 d) - 1 enters as exp(2 d) + 1, d = s_q - s_p as |s_q| + |s_p|.

Constants that the kernels and TensorFlow hold in float32 enter as those float32 values (f32_constants = True): the
comparison then measures arithmetic and not the rounding of a constant.  f32_constants = False takes the decimal
constants, which is what the float64 oracle computes with."""
import math

import numpy as np

LOG_2PI = math.log(2.0 * math.pi)


def constants(f32_constants=True):
    """min_oef, min_dbv, eps, 1 - eps, exp(-2): as float32 values (what the kernels and TensorFlow hold) or exact."""
    if f32_constants:
        f = np.float32
        return dict(min_oef=float(f(0.04)), min_dbv=float(f(0.001)), eps=float(f(1e-6)),
                    one_eps=float(f(1.0) - f(1e-6)), e2=float(f(math.exp(-2.0))))
    return dict(min_oef=0.04, min_dbv=0.001, eps=1e-6, one_eps=1.0 - 1e-6, e2=math.exp(-2.0))


def dw_coef(params):
    """calculate_dw's coefficient (signals.py:144) from the protocol constants, as the oracle forms it."""
    p = {k: float(params[k]) for k in ("gamma", "b0", "dchi", "hct")}
    return (4.0 / 3.0) * math.pi * p["gamma"] * p["b0"] * p["dchi"] * p["hct"]


def sech2(p, dt):
    """d tanh / d raw.  float64: 1 / cosh^2.  float32: 4 e / (e + 1)^2 with e = exp(2 p) capped (qb::sech2f_)."""
    if dt == np.float64:
        return 1.0 / np.cosh(p) ** 2
    with np.errstate(over="ignore"):
        e = np.exp(dt(2.0) * p)
    r = dt(1.0) / (e + dt(1.0))
    return dt(4.0) * (np.minimum(e, dt(1e30)) * r) * r


def heads(q, dt, k, defect=None):
    """(s_o, s_d, c, f [N, 5]): transform_std / transform_offdiag of the raw heads and d head / d raw.
    defect "one_minus_th2": the slopes as 1 - th^2 with th recovered from the rounded s and c."""
    q = np.asarray(q, dt)
    s_o, s_d = dt(3.0) * np.tanh(q[:, 1]) - dt(1.0), dt(3.0) * np.tanh(q[:, 3]) - dt(1.0)
    c = np.tanh(q[:, 4]) * dt(k["e2"])
    f = np.ones(q.shape, dt)
    if defect == "one_minus_th2":
        th1, th3 = (s_o + dt(1.0)) * dt(1.0 / 3.0), (s_d + dt(1.0)) * dt(1.0 / 3.0)
        th4 = c * dt(1.0 / k["e2"])
        f[:, 1], f[:, 3] = dt(3.0) * (dt(1.0) - th1 * th1), dt(3.0) * (dt(1.0) - th3 * th3)
        f[:, 4] = dt(k["e2"]) * (dt(1.0) - th4 * th4)
    else:
        f[:, 1], f[:, 3] = dt(3.0) * sech2(q[:, 1], dt), dt(3.0) * sech2(q[:, 3], dt)
        f[:, 4] = dt(k["e2"]) * sech2(q[:, 4], dt)
    return s_o, s_d, c, f


def observation(y, dt, k):
    """make_obs: clipped unit-interval values of the true (OEF, DBV) -> (l0, l1, jac, |l0| scale, |l1| scale, |jac|
    scale).  The divisions by the ranges are the kernels' multiplications by 1.25 and 5."""
    y = np.asarray(y, dt)
    x0 = np.clip((y[:, 0] - dt(k["min_oef"])) * dt(1.25), dt(k["eps"]), dt(k["one_eps"]))
    x1 = np.clip((y[:, 1] - dt(k["min_dbv"])) * dt(5.0), dt(k["eps"]), dt(k["one_eps"]))
    a0, b0, a1, b1 = np.log(x0), np.log(dt(1.0) - x0), np.log(x1), np.log(dt(1.0) - x1)
    return (a0 - b0, a1 - b1, (a0 + b0) + (a1 + b1), np.abs(a0) + np.abs(b0), np.abs(a1) + np.abs(b1),
            np.abs(a0) + np.abs(b0) + np.abs(a1) + np.abs(b1))


def unit_interval(y, f32_constants=True):
    """x = (y - min) / range before the clip, float64 [N, 2] (what the cases assert about y_true)."""
    k = constants(f32_constants)
    y = np.asarray(y, np.float64)
    return np.stack([(y[:, 0] - k["min_oef"]) * 1.25, (y[:, 1] - k["min_dbv"]) * 5.0], -1)


def synth_loss(y_true, q, a=0.0, b=0.0, diagonal=False, dt=np.float64, defect=None, f32_constants=True):
    """synthetic_data_loss per voxel (model.py:449-514, use_mvg branch) as nlogp_bwd_kernel states it, with the
    inverse-gamma prior on the marginal variances when a b > 0 (x_d = exp(2 s_d) + RAW fifth parameter squared,
    model.py:499).  y_true [N, >= 2] (columns 0, 1), q [N, 5].
    diagonal = True: the diagonal family's use (fifth column 0): v is logit_gaussian_log_prob's (no log 2 pi), column 4
    of g_q is forced to 0 as the trainer does, and g4_kernel / A4_kernel carry what the kernel itself returns there.
    defect: "one_minus_th2", "no_w1_r0_ibl" (g1 without w1 r0 i_bl), "no_raw4_in_ig" (g4 without 2 raw4 d / d x_d)."""
    k = constants(f32_constants)
    q = np.asarray(q, dt)
    if diagonal:
        assert np.all(q[:, 4] == 0)
    s_o, s_d, c, f = heads(q, dt, k, defect)
    l0, l1, jac, l0a, l1a, jaca = observation(np.asarray(y_true)[:, :2], dt, k)
    i_so, i_sd = np.exp(-s_o), np.exp(-s_d)
    i_bl = -np.exp(-s_o - s_d) * c
    r0, r1 = l0 - q[:, 0], l1 - q[:, 2]
    r0a, r1a = l0a + np.abs(q[:, 0]), l1a + np.abs(q[:, 2])
    w0, w1 = r0 * i_so, r1 * i_sd + r0 * i_bl
    w0a, w1a = r0a * i_so, r1a * i_sd + r0a * np.abs(i_bl)
    v = dt(LOG_2PI) + (s_o + s_d) + dt(0.5) * (w0 * w0 + w1 * w1) + jac
    A_v = dt(LOG_2PI) + np.abs(s_o) + np.abs(s_d) + dt(0.5) * (w0a * w0a + w1a * w1a) + jaca
    g, A = np.zeros(q.shape, dt), np.zeros(q.shape, dt)
    g[:, 0], A[:, 0] = -(w0 * i_so + w1 * i_bl), w0a * i_so + w1a * np.abs(i_bl)
    g[:, 1] = dt(1.0) - w0 * w0 - (dt(0.0) if defect == "no_w1_r0_ibl" else w1 * r0 * i_bl)
    A[:, 1] = dt(1.0) + w0a * w0a + w1a * r0a * np.abs(i_bl)
    g[:, 2], A[:, 2] = -(w1 * i_sd), w1a * i_sd
    g[:, 3], A[:, 3] = dt(1.0) - w1 * w1, dt(1.0) + w1a * w1a
    g[:, 4], A[:, 4] = -(w1 * r0 * i_so * i_sd), w1a * r0a * i_so * i_sd
    g4_direct, A4_direct = np.zeros(len(q), dt), np.zeros(len(q), dt)
    if a * b > 0.0:   # model.py:492
        ia, ib = dt(a), dt(b)
        c0 = dt(math.lgamma(a) - a * math.log(b))
        x_o, e_d = np.exp(dt(2.0) * s_o), np.exp(dt(2.0) * s_d)
        x_d = e_d + q[:, 4] * q[:, 4]
        v = v + (dt(2.0) * c0 + (ia + dt(1.0)) * (dt(2.0) * s_o + np.log(x_d)) + ib / x_o + ib / x_d)
        A_v = A_v + (dt(2.0) * abs(c0) + (ia + dt(1.0)) * (dt(2.0) * np.abs(s_o) + np.abs(np.log(x_d))) + ib / x_o
                     + ib / x_d)
        d_o, d_d = (ia + dt(1.0)) / x_o - ib / (x_o * x_o), (ia + dt(1.0)) / x_d - ib / (x_d * x_d)
        d_oa, d_da = (ia + dt(1.0)) / x_o + ib / (x_o * x_o), (ia + dt(1.0)) / x_d + ib / (x_d * x_d)
        g[:, 1], A[:, 1] = g[:, 1] + d_o * dt(2.0) * x_o, A[:, 1] + d_oa * dt(2.0) * x_o
        g[:, 3], A[:, 3] = g[:, 3] + d_d * dt(2.0) * e_d, A[:, 3] + d_da * dt(2.0) * e_d
        if defect != "no_raw4_in_ig":
            g4_direct = d_d * dt(2.0) * q[:, 4]      # x_d holds the raw head: no transform_offdiag slope
        A4_direct = d_da * dt(2.0) * np.abs(q[:, 4])
    g, A = g * f, A * f
    g[:, 4], A[:, 4] = g[:, 4] + g4_direct, A[:, 4] + A4_direct
    out = dict(v=v, g_q=g, A_v=A_v, A_q=A)
    if diagonal:
        out.update(g4_kernel=g[:, 4].copy(), A4_kernel=A[:, 4].copy(), v=v - dt(LOG_2PI))
        g[:, 4] = 0.0
        A[:, 4] = 0.0
    return out


def hyper_prior(q, ig, dt=np.float64, defect=None, f32_constants=True):
    """The learned inverse-gamma hyper-prior (hyper_prior_kernel): per voxel sum over (OEF, DBV) of
    lgamma(a) - a log b + (a + 1) log v + b / v, v = exp(2 s); d / d raw for columns 1 and 3; sums = (sum log v_o,
    sum 1 / v_o, sum log v_d, sum 1 / v_d) in float64.  ig = (a_o, b_o, a_d, b_d)."""
    k = constants(f32_constants)
    q = np.asarray(q, dt)
    s_o, s_d, _, f = heads(q, dt, k, defect)
    v, A_v = np.zeros(len(q), dt), np.zeros(len(q), dt)
    g, A = np.zeros(q.shape, dt), np.zeros(q.shape, dt)
    sums = []
    for col, s, a, b in ((1, s_o, ig[0], ig[1]), (3, s_d, ig[2], ig[3])):
        c0 = dt(math.lgamma(a) - a * math.log(b))
        lv = dt(2.0) * s
        iv = np.exp(-lv)
        v = v + (c0 + (dt(a) + dt(1.0)) * lv + dt(b) * iv)
        A_v = A_v + (abs(c0) + (dt(a) + dt(1.0)) * np.abs(lv) + dt(b) * iv)
        g[:, col] = (dt(2.0) * (dt(a) + dt(1.0)) - dt(2.0) * dt(b) * iv) * f[:, col]
        A[:, col] = (dt(2.0) * (dt(a) + dt(1.0)) + dt(2.0) * dt(b) * iv) * f[:, col]
        sums += [lv.astype(np.float64).sum(), iv.astype(np.float64).sum()]
    return dict(v=v, g_q=g, A_v=A_v, A_q=A, sums=np.array(sums), log_v=np.stack([2.0 * s_o, 2.0 * s_d], -1))


def r2p_draws(q, z, dw, dt=np.float64, f32_constants=True):
    """r_k = dw(OEF_k) DBV_k [N, n] of the reparameterised draws (ReparamTrickLayer, forward_transform -- a plain
    sigmoid, no clip -- and calculate_r2p), with OEF_k, DBV_k and their slopes in the logits."""
    k = constants(f32_constants)
    q, z = np.asarray(q, dt), np.asarray(z, dt)
    s_o, s_d, c, _ = heads(q, dt, k)
    a = q[:, 0:1] + z[..., 0] * np.exp(s_o)[:, None]
    b = q[:, 2:3] + z[..., 0] * c[:, None] + z[..., 1] * np.exp(s_d)[:, None]
    with np.errstate(over="ignore"):
        ea, eb = np.exp(-a), np.exp(-b)
    sa, sb = dt(1.0) / (dt(1.0) + ea), dt(1.0) / (dt(1.0) + eb)
    oef, dbv = sa * dt(0.8) + dt(k["min_oef"]), sb * dt(0.2) + dt(k["min_dbv"])
    # d OEF / d a = range sigmoid(a) sigmoid(-a) with sigmoid(-a) = sigmoid(a) e^-a: nothing cancels at the upper end
    # of the range, where (x - min) (1 - (x - min) / range) keeps only the rounding of x
    d_oef = dt(0.8) * sa * (sa * np.minimum(ea, dt(1e30)))
    d_dbv = dt(0.2) * sb * (sb * np.minimum(eb, dt(1e30)))
    return (dt(dw) * oef) * dbv, oef, dbv, d_oef, d_dbv


def r2p_loss(y_r2p, q, z, dw, dt=np.float64, defect=None, f32_constants=True):
    """The R2' term (r2p_loss_bwd_kernel's comment): n draws, mean and BIASED variance of r_k, v = 0.5 log var +
    0.5 (y - mean)^2 / var, and its gradient through calculate_r2p, forward_transform, the reparameterisation and the
    head transforms.  y_r2p [N] true R2', z [N, n, 2], dw from dw_coef(params).  Also mean, var.
    defect: "one_minus_th2", "unbiased_var" (the variance divided by n - 1), "slope_by_difference"."""
    k = constants(f32_constants)
    q, z, y = np.asarray(q, dt), np.asarray(z, dt), np.asarray(y_r2p, dt)
    n = z.shape[1]
    s_o, s_d, c, f = heads(q, dt, k, defect)
    e_so, e_sd = np.exp(s_o), np.exp(s_d)
    r, oef, dbv, d_oef, d_dbv = r2p_draws(q, z, dw, dt, f32_constants)
    if defect == "slope_by_difference":   # (x - min) (1 - (x - min) / range), as the kernel had it
        uo, ud = oef - dt(k["min_oef"]), dbv - dt(k["min_dbv"])
        d_oef, d_dbv = uo * (dt(1.0) - uo * dt(1.25)), ud * (dt(1.0) - ud * dt(5.0))
    inv_n = dt(1.0) / dt(n)
    mean = r.sum(1) * inv_n
    dev = r - mean[:, None]
    var = (dev * dev).sum(1) * (dt(1.0) / dt(n - 1) if defect == "unbiased_var" else inv_n)
    iv, dy = dt(1.0) / var, y - mean
    v = dt(0.5) * np.log(var) + dt(0.5) * dy * dy * iv
    A_v = dt(0.5) * np.abs(np.log(var)) + dt(0.5) * dy * dy * iv
    gr = (-dy * iv * inv_n)[:, None] + ((dt(1.0) - dy * dy * iv) * iv * inv_n)[:, None] * dev
    gra = (np.abs(dy) * iv * inv_n)[:, None] + ((dt(1.0) + dy * dy * iv) * iv * inv_n)[:, None] * np.abs(dev)
    da = dt(dw) * dbv * d_oef     # d r / d logit a (positive)
    db = dt(dw) * oef * d_dbv
    g, A = np.zeros(q.shape, dt), np.zeros(q.shape, dt)
    for w, out in ((gr, g), (gra, A)):
        z0, z1 = (z[..., 0], z[..., 1]) if out is g else (np.abs(z[..., 0]), np.abs(z[..., 1]))
        out[:, 0] = (w * da).sum(1)
        out[:, 1] = (w * da * z0).sum(1) * e_so
        out[:, 2] = (w * db).sum(1)
        out[:, 3] = (w * db * z1).sum(1) * e_sd
        out[:, 4] = (w * db * z0).sum(1)
    return dict(v=v, g_q=g * f, A_v=A_v, A_q=A * f, mean=mean, var=var)


def kl_diag(q, prior, dt=np.float64, defect=None, f32_constants=True):
    """kl_loss of the diagonal family (model.py:686-716): per dimension 0.5 ((mu_q - mu_p) / sigma_p)^2 +
    0.5 expm1(2 (s_q - s_p)) - (s_q - s_p); d / d raw q for columns 0 - 3 (column 4: 0).
    defect: "one_minus_th2", "exp_for_expm1" (exp where expm1 belongs)."""
    k = constants(f32_constants)
    q, p = np.asarray(q, dt), np.asarray(prior, dt)
    sq = heads(q, dt, k, defect)
    sp = heads(p, dt, k)
    f = sq[3]
    v, A_v = np.zeros(len(q), dt), np.zeros(len(q), dt)
    g, A = np.zeros(q.shape, dt), np.zeros(q.shape, dt)
    for dim in range(2):
        s_q, s_p = sq[dim], sp[dim]
        ip = np.exp(-s_p)
        d = s_q - s_p
        ro = (q[:, 2 * dim] - p[:, 2 * dim]) * ip
        roa = (np.abs(q[:, 2 * dim]) + np.abs(p[:, 2 * dim])) * ip
        em = np.exp(dt(2.0) * d) if defect == "exp_for_expm1" else np.expm1(dt(2.0) * d)
        ema = np.exp(dt(2.0) * d) + dt(1.0)
        v = v + (dt(0.5) * ro * ro + dt(0.5) * em - d)
        A_v = A_v + (dt(0.5) * roa * roa + dt(0.5) * ema + np.abs(s_q) + np.abs(s_p))
        g[:, 2 * dim], A[:, 2 * dim] = ro * ip, roa * ip
        g[:, 2 * dim + 1], A[:, 2 * dim + 1] = em * f[:, 2 * dim + 1], ema * f[:, 2 * dim + 1]
    return dict(v=v, g_q=g, A_v=A_v, A_q=A, d=np.stack([sq[0] - sp[0], sq[1] - sp[1]], -1))


def kl_mog(q, comps, z, dt=np.float64, f32_constants=True):
    """kl_loss against a mixture-of-Gaussians population prior (model.py:666-685), value only: one reparameterised
    draw per dimension, minus q's entropy, plus the mean of the components' Gaussian NLLs.  comps [M, 4], z [N, 2]."""
    k = constants(f32_constants)
    q, z = np.asarray(q, dt), np.asarray(z, dt)
    comps5 = np.concatenate([np.asarray(comps, dt), np.zeros((len(comps), 1), dt)], -1)
    s_o, s_d, _, _ = heads(q, dt, k)
    c_o, c_d, _, _ = heads(comps5, dt, k)
    M = len(comps5)
    v, A_v = -(s_o + s_d), np.abs(s_o) + np.abs(s_d)
    for col, s, cs, zz in ((0, s_o, c_o, z[:, 0]), (2, s_d, c_d, z[:, 1])):
        x = q[:, col] + zz * np.exp(s)
        xa = np.abs(q[:, col]) + np.abs(zz) * np.exp(s)
        for c in range(M):
            r = (x - comps5[c, col]) * np.exp(-cs[c])
            ra = (xa + np.abs(comps5[c, col])) * np.exp(-cs[c])
            v = v + (cs[c] + dt(0.5) * r * r) / dt(M)
            A_v = A_v + (np.abs(cs[c]) + dt(0.5) * ra * ra) / dt(M)
    return dict(v=v, A_v=A_v)


def ratio(got, want, A):
    """|got - want| / A entry by entry (A = 0: 0 where got == want, else inf); NaN in got counts as inf."""
    got, want, A = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(A, np.float64)
    d = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(A > 0, d / A, np.where(d == 0, 0.0, np.inf))
    return np.where(np.isnan(r), np.inf, r)


def worst(got, want, A):
    return float(ratio(got, want, A).max())
