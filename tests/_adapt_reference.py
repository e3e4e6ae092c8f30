"""Float64 restatement of qbold_adapt_posterior (qbold_vi_amd/csrc/adapt_kernels.hip states the algorithm in its head):
adaptive importance sampling per voxel by moment matching, built on tests/_iw_reference.log_weights for the log-weights
of a round (the oracle's clip semantics included) and on the clamp rule of tests/_laplace_reference.heads_from
(test_adapt_host.py holds clamp_rule below to it).  f32=True runs the same composition on a float32 Oracle with
float32 update arithmetic: its distance to the float64 run is the float32 floor of the GPU test's later-round bounds.
Vectorised over voxels; every voxel passed in is evaluated (callers select the live ones).  Test infrastructure (no GPU
needed)."""
import math

import numpy as np

import _laplace_reference as lr
from _iw_reference import log_weights

STREAM_ADAPT = 9
CLIP = lr.CLIP
TANH_MAX = lr.TANH_MAX
E2, EM2 = math.exp(2.0), math.exp(-2.0)
DEFAULTS = dict(R=6, K=64, shrink=4.0)


def normals(o32, seed, voxel0, N, R, K):
    """The draws of the Philox path, [N, R K, 2]: draw r K + k of stream 9."""
    return o32.philox_normals(seed, STREAM_ADAPT, voxel0, N, R * K)


def clamp_rule(s_o, s_d, c, dt=np.float64):
    """(t_so, t_sd, t_c, clamped) of the Cholesky terms (log e_so, log e_sd, c) under laplace_kernel's clamp rule: each
    tanh value clamped to +-TANH_MAX, e^(2 s_d) re-formed as Sigma_bb - c^2 with the kept c where c was clamped."""
    s_o, s_d, c = (np.asarray(a, dt) for a in (s_o, s_d, c))
    tmax, third, one = dt(TANH_MAX), dt(1.0 / 3.0), dt(1.0)
    t_so_raw = (s_o + one) * third
    t_c_raw = c * dt(E2)
    t_so, t_c = np.clip(t_so_raw, -tmax, tmax), np.clip(t_c_raw, -tmax, tmax)
    cc = t_c * dt(EM2)
    with np.errstate(all="ignore"):
        kept = dt(0.5) * np.log(c * c + np.exp(dt(2.0) * s_d) - cc * cc)
    sd_kept = np.where(t_c != t_c_raw, kept, s_d).astype(dt)
    t_sd_raw = (sd_kept + one) * third
    t_sd = np.clip(t_sd_raw, -tmax, tmax)
    clamped = (t_so != t_so_raw) | (t_c != t_c_raw) | (t_sd != t_sd_raw)
    return t_so.astype(dt), t_sd.astype(dt), t_c.astype(dt), clamped


def heads_of(mu, t, dt=np.float64):
    """raw heads [n, 5] of means mu [n, 2] and tanh values t [n, 3] = (t_so, t_sd, t_c)"""
    with np.errstate(all="ignore"):
        a = np.arctanh(t.astype(dt))
    return np.stack([mu[:, 0], a[:, 0], mu[:, 1], a[:, 1], a[:, 2]], -1).astype(dt)


def round_stats(lw, z, dt=np.float64):
    """dict(log_p, ess, ok, m [n, 2], C [n, 3] = (c00, c01, c11)) of log-weights lw [n, K] and normals z [n, K, 2]"""
    lw, z = np.asarray(lw, dt), np.asarray(z, dt)
    K = lw.shape[1]
    with np.errstate(all="ignore"):
        M = lw.max(1, keepdims=True)
        w = np.exp(lw - M)
        s1, s2 = w.sum(1), (w * w).sum(1)
        ok = np.isfinite(s1) & (s1 > 0)
        log_p = M[:, 0] + np.log(s1) - dt(math.log(K))
        ess = np.where(ok, s1 * s1 / s2, np.nan).astype(dt)
        m = (w[:, :, None] * z).sum(1) / s1[:, None]
        c00 = (w * z[:, :, 0] * z[:, :, 0]).sum(1) / s1 - m[:, 0] * m[:, 0]
        c01 = (w * z[:, :, 0] * z[:, :, 1]).sum(1) / s1 - m[:, 0] * m[:, 1]
        c11 = (w * z[:, :, 1] * z[:, :, 1]).sum(1) / s1 - m[:, 1] * m[:, 1]
    return dict(log_p=log_p.astype(dt), ess=ess, ok=ok, m=m.astype(dt), C=np.stack([c00, c01, c11], -1).astype(dt))


def update(mu, t, st, shrink, dt=np.float64):
    """One moment-matching update of the proposals (mu [n, 2], t [n, 3]) from round statistics st.  Returns
    (mu', t', done [n] bool, on_clip [n], clamped [n]); rows that are not done keep their proposal."""
    one = dt(1.0)
    s_o, s_d = dt(3.0) * t[:, 0] - one, dt(3.0) * t[:, 1] - one
    c = t[:, 2] * dt(EM2)
    e_so, e_sd = np.exp(s_o), np.exp(s_d)
    m0, m1 = st["m"][:, 0], st["m"][:, 1]
    with np.errstate(all="ignore"):
        lam = st["ess"] / (st["ess"] + dt(shrink))
        om = one - lam
        lo = lam * om
        B00 = om + lam * st["C"][:, 0] + lo * m0 * m0
        B01 = lam * st["C"][:, 1] + lo * m0 * m1
        B11 = om + lam * st["C"][:, 2] + lo * m1 * m1
        g00 = np.sqrt(B00)
        g10 = B01 / g00
        g11 = np.sqrt(B11 - g10 * g10)
        mu_o = mu[:, 0] + lam * (e_so * m0)
        mu_d = mu[:, 1] + lam * (c * m0 + e_sd * m1)
        ns_o, ns_d = s_o + np.log(g00), s_d + np.log(g11)
        nc = c * g00 + e_sd * g10
        done = st["ok"] & np.isfinite(g00) & (g00 > 0) & np.isfinite(g11) & (g11 > 0) & np.isfinite(mu_o) & \
            np.isfinite(mu_d) & np.isfinite(nc)
        clip = dt(CLIP)
        mu_o, mu_d = np.clip(mu_o, -clip, clip), np.clip(mu_d, -clip, clip)
        on_clip = done & ((np.abs(mu_o) >= clip) | (np.abs(mu_d) >= clip))
        t_so, t_sd, t_c, clamped = clamp_rule(ns_o, ns_d, nc, dt)
    mu2 = np.where(done[:, None], np.stack([mu_o, mu_d], -1), mu).astype(dt)
    t2 = np.where(done[:, None], np.stack([t_so, t_sd, t_c], -1), t).astype(dt)
    return mu2, t2, done, on_clip, done & clamped


def adapt(o, x, q, prior, sigma, z, R=6, K=64, shrink=4.0, f32=False):
    """The algorithm on the voxels given: `o` an Oracle (float64, or float32 with f32=True), q [n, 5] the starting
    heads, z [n, R K, 2] the normals.  dict(q_out [n, 5], log_p [n, R], ess [n, R], best [n], flags [n],
    q_rounds [n, R, 5])."""
    dt = np.float32 if f32 else np.float64
    q = np.asarray(q)
    n = q.shape[0]
    z = np.asarray(z).reshape(n, R, K, 2)
    mu = q[:, [0, 2]].astype(dt)
    t = np.tanh(q[:, [1, 3, 4]].astype(dt)).astype(dt)
    log_p, ess = np.full((n, R), np.nan, dt), np.full((n, R), np.nan, dt)
    q_rounds = np.zeros((n, R, 5), dt)
    best, best_ess = np.zeros(n, int), np.full(n, -np.inf)
    q_out = q.astype(dt).copy()
    flags = np.zeros(n, int)
    for r in range(R):
        heads = q.astype(dt) if r == 0 else heads_of(mu, t, dt)   # round 0: the given heads themselves
        q_rounds[:, r] = heads
        lw, _ = log_weights(o, x, heads, prior, sigma, z[:, r])
        st = round_stats(lw, z[:, r], dt)
        log_p[:, r], ess[:, r] = st["log_p"], st["ess"]
        with np.errstate(invalid="ignore"):
            better = st["ok"] & (st["ess"] > best_ess)   # strict: ties go to the earliest round
        best[better], best_ess[better] = r, st["ess"][better]
        q_out[better] = heads[better]
        if r + 1 < R:
            mu, t, done, on_clip, clamped = update(mu, t, st, shrink, dt)
            flags |= np.where(done, 0, 1) | np.where(on_clip, 2, 0) | np.where(clamped, 4, 0)
        else:
            flags |= np.where(st["ok"], 0, 1)
    return dict(q_out=q_out, log_p=log_p, ess=ess, best=best, flags=flags, q_rounds=q_rounds)


def fresh_ess(o, x, q, prior, sigma, z):
    """ESS [n] of a fresh evaluation of the heads q on normals z [n, K, 2]"""
    lw, _ = log_weights(o, x, q, prior, sigma, z)
    return round_stats(lw, z)["ess"]


def chol_terms(q):
    """(mu [n, 2], (e_so, c, e_sd) [n, 3]) of raw heads in float64"""
    q = np.asarray(q, np.float64)
    return q[:, [0, 2]], np.stack([np.exp(3.0 * np.tanh(q[:, 1]) - 1.0), np.tanh(q[:, 4]) * EM2,
                                   np.exp(3.0 * np.tanh(q[:, 3]) - 1.0)], -1)


def proposal_error(got, want):
    """How far heads `got` are from heads `want`, per voxel [n]: the largest of the means' distances in units of the
    wanted marginal sds and the Cholesky terms' distances relative to e_so (its own size) and to the wanted sd of b
    (c and e_sd) -- the measure test_gpu_laplace.test_heads_reproduce_the_map_and_the_covariance takes."""
    mg, Lg = chol_terms(got)
    mw, Lw = chol_terms(want)
    sd_b = np.sqrt(Lw[:, 1] ** 2 + Lw[:, 2] ** 2)
    e = np.stack([np.abs(mg[:, 0] - mw[:, 0]) / Lw[:, 0], np.abs(mg[:, 1] - mw[:, 1]) / sd_b,
                  np.abs(Lg[:, 0] - Lw[:, 0]) / Lw[:, 0], np.abs(Lg[:, 1] - Lw[:, 1]) / sd_b,
                  np.abs(Lg[:, 2] - Lw[:, 2]) / sd_b], -1)
    return e.max(1)


def near_tie(ess, rel=1e-3):
    """[n] bool: the two largest ESS_r of a voxel differ by no more than `rel` relative (a voxel with one round never)"""
    e = np.sort(np.nan_to_num(np.asarray(ess, np.float64), nan=-np.inf), axis=1)
    if e.shape[1] < 2:
        return np.zeros(e.shape[0], bool)
    with np.errstate(invalid="ignore"):
        return ~(e[:, -1] - e[:, -2] > rel * np.abs(e[:, -1]))
