"""Float64 reference of the importance-weighted evidence (qbold_log_evidence_fwd), built from the CPU oracle's
primitives: reparam -> signal_fwd -> nll (mask 1) for the likelihood of each draw, logit_mvn_nlogp under q and under
the prior for log q - log p of the SAME draw, then a float64 logsumexp.  Test infrastructure (no GPU needed)."""
import numpy as np


def dw_coef(params):
    """calculate_dw's factor (signals.py:142-147): dw = (4/3) pi gamma b0 dchi hct OEF."""
    p = {k: float(params[k]) for k in ("gamma", "b0", "dchi", "hct")}
    return (4.0 / 3.0) * np.pi * p["gamma"] * p["b0"] * p["dchi"] * p["hct"]


def log_weights(o, x, q, prior, sigma, z):
    """log w [N, K] and the draws (OEF, DBV) [N, K, 2] for explicit normals z [N, K, 2]; `o` is an Oracle."""
    z = np.asarray(z, np.float64)
    N, K = z.shape[0], z.shape[1]
    T = o.T

    def rep(a, c):
        return np.repeat(np.asarray(a, np.float64).reshape(N, c), K, axis=0)

    qs = rep(q, 5)
    y = o.reparam(qs, z.reshape(-1, 2))
    nll = o.nll(rep(x, T), np.ones(N * K), o.signal_fwd(y), rep(sigma, T)).reshape(N, K)
    log_q = -o.logit_mvn_nlogp(y, qs).reshape(N, K)
    log_p = -o.logit_mvn_nlogp(y, rep(prior, 5)).reshape(N, K)
    return -nll - (log_q - log_p), np.asarray(y, np.float64).reshape(N, K, 2)


def iw_reference(o, x, q, prior, sigma, z, params=None):
    """dict(log_p, elbo, ess, means [N, 3] = self-normalised (OEF, DBV, R2'), lw [N, K])."""
    lw, y = log_weights(o, x, q, prior, sigma, z)
    K = lw.shape[1]
    M = lw.max(1, keepdims=True)
    w = np.exp(lw - M)
    s1 = w.sum(1)
    theta = np.stack([y[..., 0], y[..., 1], dw_coef(params or o.params) * y[..., 0] * y[..., 1]], -1)
    return dict(log_p=M[:, 0] + np.log(s1) - np.log(K), elbo=lw.mean(1), ess=s1 ** 2 / (w ** 2).sum(1),
                means=(w[..., None] * theta).sum(1) / s1[:, None], lw=lw)


def rel1(a, b):
    """max |a - b| / (|b| + 1)"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / (np.abs(b) + 1.0)))


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))
