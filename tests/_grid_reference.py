"""Float64 restatement of qbold_posterior_grid (include/qbold_hip.h states the definition): start box, locate passes,
fine pass and the seventeen per-voxel outputs, parameterised by a log-joint callable J(A, B) on meshgrid arrays of
logits; a dense two-stage reference in the style of tests/test_gpu_log_evidence.py's _quadrature; and the log-joint of
one voxel built from the CPU oracle's primitives (o64.signal_fwd, o64.nll).  Test infrastructure (no GPU needed)."""
import numpy as np

CLIP = 13.815509557963774   # QB_LOGIT_CLIP: logit((1 - 1e-6)), model.py:393-396


def oef_of(a):
    return 1.0 / (1.0 + np.exp(-a)) * 0.8 + 0.04


def dbv_of(b):
    return 1.0 / (1.0 + np.exp(-b)) * 0.2 + 0.001


def mvn(raw):
    """(mu [2], L [2, 2]) of the logit-space Gaussian of five raw heads (transform_std / transform_offdiag)."""
    raw = np.asarray(raw, np.float64)
    so, sd = np.exp(3 * np.tanh(raw[1]) - 1), np.exp(3 * np.tanh(raw[3]) - 1)
    c = np.tanh(raw[4]) * np.exp(-2.0)
    return np.array([raw[0], raw[2]]), np.array([[so, 0.0], [c, sd]])


def mvn_logpdf(A, B, raw):
    mu, L = mvn(raw)
    w0 = (A - mu[0]) / L[0, 0]
    w1 = (B - mu[1] - L[1, 0] * w0) / L[1, 1]
    return -np.log(2 * np.pi) - np.log(L[0, 0] * L[1, 1]) - 0.5 * (w0 * w0 + w1 * w1)


def kl_closed(q, p):
    """KL(q || p) of two logit-space Gaussians given by raw heads."""
    mq, Lq = mvn(q)
    mp, Lp = mvn(p)
    Mw = np.linalg.solve(Lp, Lq)
    d = np.linalg.solve(Lp, mq - mp)
    return 0.5 * ((Mw ** 2).sum() + (d ** 2).sum()) - np.log(np.diag(Mw).prod()) - 1.0


def start_box(prior, q=None, span=6.0, clip=CLIP):
    def one(raw):
        mu, L = mvn(raw)
        s = np.sqrt((L ** 2).sum(1))
        return np.array([mu[0] - span * s[0], mu[0] + span * s[0], mu[1] - span * s[1], mu[1] + span * s[1]])
    b = one(prior)
    if q is not None:
        bq = one(q)
        b = np.array([min(b[0], bq[0]), max(b[1], bq[1]), min(b[2], bq[2]), max(b[3], bq[3])])
    return np.clip(b, -clip, clip)


def _grid(logj, box, n):
    a, b = np.linspace(box[0], box[1], n), np.linspace(box[2], box[3], n)
    A, B = np.meshgrid(a, b, indexing="ij")
    J = np.asarray(logj(A, B), np.float64)
    return a, b, np.where(np.isnan(J), -np.inf, J)


def locate(logj, box, n, cut):
    """One locate pass: the kept rows' and columns' range widened by one step, intersected with box."""
    a, b, J = _grid(logj, box, n)
    M = J.max()
    rows = np.nonzero(J.max(1) > M - cut)[0]
    cols = np.nonzero(J.max(0) > M - cut)[0]
    ha, hb = a[1] - a[0], b[1] - b[0]
    return np.array([max(box[0], a[rows[0]] - ha), min(box[1], a[rows[-1]] + ha),
                     max(box[2], b[cols[0]] - hb), min(box[3], b[cols[-1]] + hb)])


def cell_quantile(mass, nodes, h, p):
    """Quantile at level p of node masses spread uniformly over their cells (CDF linear within a cell)."""
    c = np.cumsum(mass)
    t = p * c[-1]
    i = int(np.argmax((c >= t) & (mass > 0)))
    frac = np.clip((t - (c[i] - mass[i])) / mass[i], 0.0, 1.0)
    return nodes[i] - 0.5 * h + h * frac


def fine_pass(logj, box, n, levels=(0.025, 0.975), ta=oef_of, tb=dbv_of, dw=1.0):
    """The fine pass's outputs (columns 0, 2-16 of out; elbo_q is added by the caller) as a dict."""
    a, b, J = _grid(logj, box, n)
    ha, hb = a[1] - a[0], b[1] - b[0]
    M = J.max()
    w = np.exp(J - M)
    Z = w.sum()
    P = w / Z
    o, d = ta(a)[:, None], tb(b)[None, :]
    r = dw * o * d
    eo, ed, er = (P * o).sum(), (P * d).sum(), (P * r).sum()
    vo, vd, vr = (P * (o - eo) ** 2).sum(), (P * (d - ed) ** 2).sum(), (P * (r - er) ** 2).sum()
    cov = (P * (o - eo) * (d - ed)).sum()
    qa = [cell_quantile(w.sum(1), a, ha, p) for p in levels]
    qb = [cell_quantile(w.sum(0), b, hb, p) for p in levels]
    i, j = np.unravel_index(int(np.argmax(J)), J.shape)
    ring = np.zeros_like(w, bool)
    ring[0, :] = ring[-1, :] = ring[:, 0] = ring[:, -1] = True
    out = np.full(17, np.nan)
    out[0] = M + np.log(Z) + np.log(ha * hb)
    out[2:5] = eo, ed, er
    out[5:8] = np.sqrt(vo), np.sqrt(vd), np.sqrt(vr)
    out[8] = cov / np.sqrt(vo * vd)
    out[9:11] = ta(np.array(qa))
    out[11:13] = tb(np.array(qb))
    out[13:15] = ta(a[i]), tb(b[j])
    out[15] = w[ring].sum() / Z
    out[16] = abs(np.log(Z) - np.log(4.0 * w[::2, ::2].sum()))
    return out, np.array([ha, hb])


def posterior_grid(logj, box0, coarse=32, fine=64, locate_passes=2, cut=40.0, levels=(0.025, 0.975), ta=oef_of,
                   tb=dbv_of, dw=1.0, fine_box=None):
    """(out [17] with elbo_q NaN, the fine box [4]); fine_box given: skip the locate passes and use it."""
    box = np.asarray(box0, np.float64)
    if fine_box is None:
        for _ in range(locate_passes):
            box = locate(logj, box, coarse, cut)
    else:
        box = np.asarray(fine_box, np.float64)
    out, _ = fine_pass(logj, box, fine, levels, ta, tb, dw)
    return out, box


def dense(logj, box0, n=481, coarse=161, cut=40.0, levels=(0.025, 0.975), ta=oef_of, tb=dbv_of, dw=1.0):
    """The dense two-stage reference (one coarse pass over box0, one fine n x n pass)."""
    return posterior_grid(logj, box0, coarse, n, 1, cut, levels, ta, tb, dw)


class VoxelJoint:
    """log p(x | u) and the log-joint of one voxel from the oracle's primitives; u clipped at +-CLIP."""

    def __init__(self, o64, x, sigma, prior):
        self.o, self.x, self.sigma, self.prior = o64, np.asarray(x, np.float64), np.asarray(sigma, np.float64), prior

    def loglik(self, A, B):
        A, B = np.clip(A, -CLIP, CLIP), np.clip(B, -CLIP, CLIP)
        y = np.stack([oef_of(A).ravel(), dbv_of(B).ravel()], -1)
        m = y.shape[0]
        nll = self.o.nll(np.repeat(self.x[None], m, 0), np.ones(m), self.o.signal_fwd(y),
                         np.repeat(self.sigma[None], m, 0))
        return -np.asarray(nll, np.float64).reshape(A.shape)

    def __call__(self, A, B):
        return self.loglik(A, B) + mvn_logpdf(A, B, self.prior)

    def elbo(self, q, gh=16):
        """E_q[log p(x | u)] by the gh x gh product Gauss-Hermite rule, minus the closed-form KL(q || prior)."""
        t, w = np.polynomial.hermite.hermgauss(gh)
        mu, L = mvn(q)
        T0, T1 = np.meshgrid(np.sqrt(2) * t, np.sqrt(2) * t, indexing="ij")
        A = mu[0] + L[0, 0] * T0
        B = mu[1] + L[1, 0] * T0 + L[1, 1] * T1
        W = np.outer(w, w) / np.pi
        return float((W * self.loglik(A, B)).sum()) - kl_closed(q, self.prior)


def voxel_reference(o64, x, sigma, prior, q=None, gh=16, fine_box=None, dw=1.0, **kw):
    """out [17] and the fine box of one voxel (kw: coarse, fine, locate_passes, cut, levels, span)."""
    span = kw.pop("span", 6.0)
    J = VoxelJoint(o64, x, sigma, prior)
    out, box = posterior_grid(J, start_box(prior, q, span), fine_box=fine_box, dw=dw, **kw)
    if q is not None and gh > 0:
        out[1] = J.elbo(q, gh)
    return out, box
