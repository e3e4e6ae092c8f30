"""Float64 restatement of qbold_fisher_information and qbold_design_scores (include/qbold_hip.h states the definitions):
the rows j_t of the normalised signal on the logit plane from the CPU oracle's primitives (signal_fwd and the analytic
signal_jac, Simpson node 0's slope taken out as tests/_laplace_reference.Model takes it out), the data information
I = sum_t w_t j_t j_t^T, the prior precision, A = I + Lambda and everything the two entries derive from them.  With
dtype=np.float32 and the float32 oracle the same composition in float32 arithmetic: the floor of the GPU test.
Vectorised over designs and voxels.  Test infrastructure (no GPU needed)."""
import numpy as np

import _grid_reference as gr
from _laplace_reference import Model, _node0_slope

SINGULAR = 2.0 ** -20       # flag bit 0: det I <= SINGULAR (I_aa I_bb + I_ab^2)
OEF_LO, OEF_HI, DBV_LO, DBV_HI = 0.04, 0.84, 0.001, 0.201


def in_range(theta):
    th = np.asarray(theta, np.float64)
    return (th[:, 0] > OEF_LO) & (th[:, 0] < OEF_HI) & (th[:, 1] > DBV_LO) & (th[:, 1] < DBV_HI)


def logits(theta):
    th = np.asarray(theta, np.float64)
    return np.stack([np.log((th[:, 0] - OEF_LO) / (OEF_HI - th[:, 0])),
                     np.log((th[:, 1] - DBV_LO) / (DBV_HI - th[:, 1]))], -1)


def model_of(o, theta, sigma, prior, multi):
    """_laplace_reference.Model at unit data: its constants, its window and (through evaluate) its A."""
    n = len(theta)
    sg = np.broadcast_to(np.asarray(sigma, np.float64).reshape(-1, o.T), (n, o.T))
    pr = np.zeros((n, 5)) if prior is None else prior
    return Model(o, np.ones((n, o.T)), sg, pr, multi=multi, node0_zero=True)


def rows(o, theta, multi, dtype=np.float64):
    """(j [n, T, 2] = d yhat_t / d (a, b) at unit sigma, slopes d [n, 2] of forward_transform, R2' gradient [n, 2]) at
    theta [n, 2] = (OEF, DBV): Model.evaluate's jl, restated for points given as theta and for either precision."""
    f = dtype
    th = np.asarray(theta, f)
    m = model_of(o, th, np.ones(o.T), None, multi)
    dw, taus = f(m.dw_coef), np.asarray(m.taus, f)
    s = np.asarray(o.signal_fwd(th), f)
    ds = np.array(o.signal_jac(th), f)
    xs = taus[None, :] * (dw * th[:, 0:1])
    tissue = np.exp(-th[:, 1:2] * np.asarray(o.tissue_F(xs), f)) * f(m.e_te_r2t)
    node0 = np.asarray(_node0_slope(xs.astype(np.float64)), f)
    ds[:, :, 0] += (f(1.0) - f(m.m_bld_nb) * th[:, 1:2]) * th[:, 1:2] * node0 * (taus[None, :] * dw) * tissue
    np1 = s[:, m.win].mean(1, dtype=f) + f(1e-3)
    dn = ds[:, m.win, :].mean(1, dtype=f)
    yh = s / np1[:, None]
    jt = (ds - yh[:, :, None] * dn[:, None, :]) / np1[:, None, None]
    # forward_transform's slopes at theta: 0.8 s (1 - s), s = (OEF - 0.04) / 0.8; the range ends enter in float64
    t64 = th.astype(np.float64)
    d = np.stack([(t64[:, 0] - OEF_LO) * (OEF_HI - t64[:, 0]) / 0.8,
                  (t64[:, 1] - DBV_LO) * (DBV_HI - t64[:, 1]) / 0.2], -1).astype(f)
    gr2 = np.stack([dw * th[:, 1] * d[:, 0], dw * th[:, 0] * d[:, 1]], -1)
    return (jt * d[:, None, :]).astype(f), d, gr2


def _det(M):
    return M[..., 0, 0] * M[..., 1, 1] - M[..., 0, 1] * M[..., 0, 1]


def _spread(M):
    return M[..., 0, 0] * M[..., 1, 1] + M[..., 0, 1] * M[..., 0, 1]


def _bounds(M, det, d, gr2):
    """sd of OEF, DBV, R2' (delta method) and the OEF-DBV correlation of M^-1: [..., 4]"""
    with np.errstate(all="ignore"):
        v_aa, v_bb, v_ab = M[..., 1, 1] / det, M[..., 0, 0] / det, -M[..., 0, 1] / det
        var_r = gr2[:, 0] ** 2 * v_aa + 2 * gr2[:, 0] * gr2[:, 1] * v_ab + gr2[:, 1] ** 2 * v_bb
        return np.stack([d[:, 0] * np.sqrt(v_aa), d[:, 1] * np.sqrt(v_bb), np.sqrt(np.maximum(var_r, 0)),
                         -M[..., 0, 1] / np.sqrt(M[..., 0, 0] * M[..., 1, 1])], -1)


def precision(prior, dtype=np.float64):
    """Lambda [n, 2, 2] = L_p^-T L_p^-1 of raw heads: in float64 through _grid_reference.mvn; in float32 the transforms
    of the heads, L_p^-1 = ((e^-so, 0), (-c e^(-so - sd), e^-sd)) and the products are float32 operations, as the rest of
    the floor's composition."""
    if dtype == np.float64:
        Li = np.array([np.linalg.inv(gr.mvn(p)[1]) for p in np.asarray(prior, np.float64)]).reshape(-1, 2, 2)
        return np.einsum("nji,njk->nik", Li, Li)
    f = dtype
    p = np.asarray(prior, f)
    s_o, s_d = f(3.0) * np.tanh(p[:, 1]) - f(1.0), f(3.0) * np.tanh(p[:, 3]) - f(1.0)
    c = np.tanh(p[:, 4]) * f(np.exp(-2.0))
    i_so, i_sd, i_bl = np.exp(-s_o), np.exp(-s_d), -c * np.exp(-s_o - s_d)
    lam = np.empty((len(p), 2, 2), f)
    lam[:, 0, 0], lam[:, 1, 1] = i_so * i_so + i_bl * i_bl, i_sd * i_sd
    lam[:, 0, 1] = lam[:, 1, 0] = i_bl * i_sd
    return lam


def reference(o, theta, sigma, weights, prior, multi, dtype=np.float64):
    """Per design b and voxel n, at theta [N, 2], sigma [N, T] or [T], weights [B, T] (None: one design of ones), prior
    [N, 5] or None: dict(I [B, N, 2, 2], kappa, log_det, singular [B, N], crlb [B, N, 4] (sds of OEF, DBV, R2', corr),
    and with a prior A, kappa_A, log_det_A, bound [B, N, 4], var [B, N, 3])."""
    f = dtype
    j, d, gr2 = rows(o, theta, multi, f)
    n, T = j.shape[:2]
    sg = np.broadcast_to(np.asarray(sigma, f).reshape(-1, T), (n, T))
    js = j / sg[:, :, None]
    w = np.ones((1, T), f) if weights is None else np.asarray(weights, f).reshape(-1, T)
    P = np.stack([js[:, :, 0] * js[:, :, 0], js[:, :, 0] * js[:, :, 1], js[:, :, 1] * js[:, :, 1]], -1)   # [n, T, 3]
    S = np.zeros((w.shape[0], n, 3), f)
    for t in range(T):   # tau order, in the working precision
        S = S + w[:, None, t:t + 1] * P[None, :, t, :]
    I = np.empty(S.shape[:2] + (2, 2), f)
    I[..., 0, 0], I[..., 0, 1], I[..., 1, 0], I[..., 1, 1] = S[..., 0], S[..., 1], S[..., 1], S[..., 2]
    out = dict(I=I, d=d, gr2=gr2)
    with np.errstate(all="ignore"):
        det, spread = _det(I), _spread(I)
        out["singular"] = ~(det > f(SINGULAR) * spread)
        out["kappa"] = np.where(out["singular"], np.inf, spread / det)
        out["log_det"] = np.where(out["singular"], -np.inf, np.log(np.where(out["singular"], 1.0, det)))
        crlb = _bounds(I, det, d, gr2)
        crlb[out["singular"]] = [np.inf, np.inf, np.inf, np.nan]
        out["crlb"] = crlb
    if prior is not None:
        A = I + precision(prior, f)[None]
        detA = _det(A)
        out.update(A=A, kappa_A=_spread(A) / detA, log_det_A=np.log(detA), bound=_bounds(A, detA, d, gr2))
        out["var"] = out["bound"][..., :3] ** 2
    return out


def scores(ref, mask):
    """[B, 5]: the masked sums of log det A and the three variances over the voxels, and of the mask, by a plain loop
    order-free in float64 (math.fsum-exact is not needed at 1e-12)."""
    m = np.ones(ref["A"].shape[1]) if mask is None else np.asarray(mask, np.float64)
    live = m > 0
    vals = np.concatenate([ref["log_det_A"][..., None], ref["var"]], -1).astype(np.float64)      # [B, N, 4]
    s = (vals[:, live, :] * m[None, live, None]).sum(1)
    return np.concatenate([s, np.full((s.shape[0], 1), m[live].sum())], -1)
