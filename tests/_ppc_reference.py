"""Float64 reference of the posterior predictive checks (qbold_posterior_predictive), built from the CPU oracle's
primitives: reparam -> signal_fwd for each draw's prediction, the likelihood's normalisation restated in numpy
(se_norm, log data), then per-tau residuals and log densities -> every column and curve.  Test infrastructure (no GPU
needed)."""
import math

import numpy as np


def _cfg(o):
    c = o.cfg
    return dict(se=int(c.se_idx), multi=bool(c.multi_image_normalisation), log=bool(c.predict_log_data),
                t=bool(c.use_student_t), df=float(c.student_t_df))


def normalise(o, v):
    """model.py:541-549 in float64: v / (v[se] (or the mean of v[se-1..se+1]) + 1e-3), logged with predict_log."""
    c = _cfg(o)
    v = np.asarray(v, np.float64)
    se = c["se"]
    nt = v[..., se - 1:se + 2].mean(-1, keepdims=True) if c["multi"] else v[..., se:se + 1]
    y = v / (nt + 1e-3)
    return np.log(y) if c["log"] else y


def log_density(o, r, sigma):
    """log p(y_t | theta) per tau from r = (y - yh) / sigma: the terms of the oracle's nll_one, negated."""
    c = _cfg(o)
    if c["t"]:
        df = c["df"]
        const = math.lgamma(0.5 * (df + 1.0)) - math.lgamma(0.5 * df) - 0.5 * math.log(df) - 0.5 * math.log(math.pi)
        return const - np.log(sigma) - 0.5 * (df + 1.0) * np.log1p(r * r / df)
    return -np.log(sigma) - 0.5 * math.log(2.0 * math.pi) - 0.5 * r * r


def chi2_sf(T, D):
    """Q(T / 2, D / 2) by the finite series the kernel uses (integer or half-integer shape), float64."""
    h = 0.5 * np.asarray(D, np.float64)
    e = np.exp(-h)
    if T % 2:
        rh = np.sqrt(h)
        acc = np.array([math.erfc(v) for v in rh.ravel()]).reshape(h.shape)
        term = e * rh * 2.0 / math.sqrt(math.pi)
        n, j0 = (T - 1) // 2, 1.5
    else:
        acc = np.zeros_like(h)
        term = e
        n, j0 = T // 2, 1.0
    for j in range(n):
        acc = acc + term
        term = term * h / (j + j0)
    return np.minimum(acc, 1.0)


def draws(o, x, q, sigma, z):
    """y [N, T], yh [N, L, T], r [N, L, T], lp [N, L, T] for explicit normals z [N, L, 2]."""
    z = np.asarray(z, np.float64)
    N, L = z.shape[0], z.shape[1]
    T = o.T
    qs = np.repeat(np.asarray(q, np.float64).reshape(N, 5), L, axis=0)
    th = o.reparam(qs, z.reshape(-1, 2))
    yh = normalise(o, o.signal_fwd(th)).reshape(N, L, T)
    y = normalise(o, np.asarray(x, np.float64).reshape(N, T))
    sg = np.asarray(sigma, np.float64).reshape(N, 1, T)
    r = (y[:, None, :] - yh) / sg
    return y, yh, r, log_density(o, r, sg)


def ppc_reference(o, x, q, sigma, z):
    """dict(out [N, 6] in the kernel's column order, curves [N, T, 3], D [N, L], lp [N, L, T])."""
    c = _cfg(o)
    y, yh, r, lp = draws(o, x, q, sigma, z)
    N, L, T = yh.shape
    D = (r * r).sum(-1)
    ppp = np.full(N, np.nan) if c["t"] else chi2_sf(T, D).mean(1)
    M = lp.max(1, keepdims=True)
    lppd = (M[:, 0] + np.log(np.exp(lp - M).mean(1))).sum(-1)
    pw = lp.var(1, ddof=1).sum(-1)
    v = (c["df"] / (c["df"] - 2.0) if c["df"] > 2.0 else np.inf) if c["t"] else 1.0
    mu = yh.mean(1)
    sd = np.sqrt(yh.var(1, ddof=1) + v * np.asarray(sigma, np.float64).reshape(N, T) ** 2)
    zt = (y - mu) / sd
    out = np.stack([ppp, D.mean(1), lppd, pw, lppd - pw, np.abs(zt).max(-1)], -1)
    return dict(out=out, curves=np.stack([mu, sd, zt], -1), D=D, lp=lp)


def rel1(a, b):
    """max |a - b| / (|b| + 1)"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / (np.abs(b) + 1.0)))


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))
