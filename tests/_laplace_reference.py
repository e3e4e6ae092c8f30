"""Float64 restatement of qbold_laplace_posterior (include/qbold_hip.h states the definition): F, g = J^T r, A = J^T J and
the Newton decrement at points of the logit plane, built from the CPU oracle's primitives (signal_fwd and the analytic
signal_jac) and tests/_grid_reference.py (mvn, VoxelJoint); Sigma, the Laplace evidence, the delta-method sds and the
clamped raw heads from (u^, A); a Levenberg-Marquardt loop with the header's schedule; and the seeded synthetic voxels
of the tests.  Vectorised over voxels.  Test infrastructure (no GPU needed)."""
import math

import numpy as np

import _grid_reference as gr

CLIP = gr.CLIP
LAM_MIN, LAM_MAX = 1e-7, 1e7      # the bracket of lambda
TANH_MAX = 1.0 - 1e-6             # the heads' clamp
BAND_EPS = 2.0 ** -22             # the tie rule's band
GAIN_MIN = 0.25                   # the gain rule: an accepted step below this gain ratio raises lambda
DEFAULTS = dict(max_iter=50, lambda0=1e-2, lambda_up=10.0, lambda_down=3.0, tol=1e-3)
OUT_COLUMNS = 15


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _node0_slope(x):
    """Simpson node 0's term of dF/dx (qbold_oracle.c, qbo_tissue_dF): h/3 pre_0 1.5 u_0 J1(1.5 x u_0) / (3 u_0^2) at
    u_0 = 1e-5, with J1(z) = z / 2 (1 - z^2 / 8) (z < 1e-3: the next term is below 1e-13 relative)."""
    u0 = 1e-5
    h3 = ((1.0 - u0) / 128.0) / 3.0
    z = 1.5 * x * u0
    return h3 * (2.0 + u0) * math.sqrt(1.0 - u0) * 1.5 * u0 * (0.5 * z * (1.0 - z * z / 8.0)) / (3.0 * u0 * u0)


class Model:
    """The least-squares model of N voxels: data x [N, T], sigma [N, T], prior heads [N, 5]; `o64` an f64 Oracle of the
    protocol (full model with blood), multi the normalisation window.
    node0_zero: the oracle runs with Simpson node 0 dropped from F (the value the float32 table holds, as in every GPU
    test).  qbo_signal_jac keeps that node's slope -- the training gradients restate TF's autodiff, which has it -- so
    its OEF column is not the derivative of the signal that signal_fwd returns; the node's term is taken out here, and
    test_laplace_host.py holds the result to central differences of F."""

    def __init__(self, o64, x, sigma, prior, multi=False, node0_zero=True):
        self.o = o64
        assert o64.phys.full_model and o64.phys.include_blood
        self.node0_zero = node0_zero
        P = {k: float(v) for k, v in o64.params.items()}
        self.dw_coef = (4.0 / 3.0) * math.pi * P["gamma"] * P["b0"] * P["dchi"] * P["hct"]
        self.e_te_r2t = math.exp(-P["te"] * P["r2t"])
        # m_bld nb, signals.py:102-107
        self.m_bld_nb = (1.0 - (2.0 - math.exp(-(P["tr"] - P["ti"]) / P["t1b"])) * math.exp(-P["ti"] / P["t1b"])) * 0.775
        self.taus = np.asarray(o64.taus, np.float64)
        self.x = np.asarray(x, np.float64)
        self.sigma = np.asarray(sigma, np.float64)
        self.prior = np.asarray(prior, np.float64)
        self.N, self.T = self.x.shape
        se = o64.se_idx
        self.win = slice(se - 1, se + 2) if multi else slice(se, se + 1)
        self.y = self.x / (self.x[:, self.win].mean(1, keepdims=True) + 1e-3)
        mv = [gr.mvn(p) for p in self.prior]
        self.mu = np.array([m for m, _ in mv]).reshape(self.N, 2)
        self.Linv = np.array([np.linalg.inv(L) for _, L in mv]).reshape(self.N, 2, 2)
        self.log_det_Lp = np.array([math.log(L[0, 0] * L[1, 1]) for _, L in mv])
        # -F = J + const: J the log-joint of _grid_reference.VoxelJoint
        self.const = -np.log(self.sigma).sum(1) - 0.5 * self.T * math.log(2 * math.pi) - math.log(2 * math.pi) - \
            self.log_det_Lp

    def evaluate(self, u, rows=None):
        """dict(F, chi2, band [n], g [n, 2], A [n, 2, 2], dec [n]) at logits u [n, 2] of the voxels `rows` (all)."""
        rows = np.arange(self.N) if rows is None else np.asarray(rows)
        u = np.clip(np.asarray(u, np.float64).reshape(-1, 2), -CLIP, CLIP)
        sa, sb = _sig(u[:, 0]), _sig(u[:, 1])
        th = np.stack([0.8 * sa + 0.04, 0.2 * sb + 0.001], -1)
        s = np.asarray(self.o.signal_fwd(th), np.float64)
        ds = np.array(self.o.signal_jac(th), np.float64)                  # [n, T, 2]
        if self.node0_zero:
            xs = self.taus[None, :] * (self.dw_coef * th[:, 0:1])
            tissue = np.exp(-th[:, 1:2] * np.asarray(self.o.tissue_F(xs), np.float64)) * self.e_te_r2t
            ds[:, :, 0] += (1.0 - self.m_bld_nb * th[:, 1:2]) * th[:, 1:2] * _node0_slope(xs) * \
                (self.taus[None, :] * self.dw_coef) * tissue
        np1 = s[:, self.win].mean(1) + 1e-3
        dn = ds[:, self.win, :].mean(1)                                   # [n, 2]
        yh = s / np1[:, None]
        inv_s = 1.0 / self.sigma[rows]
        r = (self.y[rows] - yh) * inv_s
        jt = (ds - yh[:, :, None] * dn[:, None, :]) / np1[:, None, None] * inv_s[:, :, None]   # d yh / d theta / sigma
        d = np.stack([0.8 * sa * (1 - sa), 0.2 * sb * (1 - sb)], -1)
        jl = jt * d[:, None, :]                                           # with respect to the logits; d r = -jl
        Li = self.Linv[rows]
        w = np.einsum("nij,nj->ni", Li, u - self.mu[rows])
        chi2 = (r * r).sum(1)
        F = 0.5 * (chi2 + (w * w).sum(1))
        g = -np.einsum("nt,ntk->nk", r, jl) + np.einsum("nji,nj->ni", Li, w)
        A = np.einsum("ntk,ntl->nkl", jl, jl) + np.einsum("nji,njk->nik", Li, Li)
        with np.errstate(all="ignore"):
            dec = np.sqrt(np.einsum("ni,ni->n", g, np.linalg.solve(A, g[:, :, None])[:, :, 0]))
        band = BAND_EPS * ((np.abs(r) * yh * inv_s).sum(1) + F)
        return dict(F=F, chi2=chi2, band=band, g=g, A=A, dec=dec)

    def F(self, u, rows=None):
        return self.evaluate(u, rows)["F"]

    def log_joint(self, u, rows=None):
        rows = np.arange(self.N) if rows is None else np.asarray(rows)
        return -self.F(u, rows) + self.const[rows]


def heads_from(u, Sigma, want_t=False):
    """(raw heads [n, 5], clamped [n] bool) of N(u, Sigma) under the header's clamp rule; want_t: also the three
    tanh values (s_o, s_d, c) before the clamp [n, 3]."""
    u, Sigma = np.asarray(u, np.float64), np.asarray(Sigma, np.float64)
    t_so = (0.5 * np.log(Sigma[:, 0, 0]) + 1.0) / 3.0
    c = Sigma[:, 0, 1] / np.sqrt(Sigma[:, 0, 0])
    t_c = c * math.exp(2.0)
    tc_so, tc_c = np.clip(t_so, -TANH_MAX, TANH_MAX), np.clip(t_c, -TANH_MAX, TANH_MAX)
    cc = tc_c * math.exp(-2.0)
    t_sd = (0.5 * np.log(Sigma[:, 1, 1] - cc * cc) + 1.0) / 3.0
    tc_sd = np.clip(t_sd, -TANH_MAX, TANH_MAX)
    clamped = (tc_so != t_so) | (tc_c != t_c) | (tc_sd != t_sd)
    q = np.stack([u[:, 0], np.arctanh(tc_so), u[:, 1], np.arctanh(tc_sd), np.arctanh(tc_c)], -1)
    return (q, clamped, np.stack([t_so, t_sd, t_c], -1)) if want_t else (q, clamped)


def heads_cov(q):
    """(mu [n, 2], Sigma [n, 2, 2]) of raw heads through _grid_reference.mvn."""
    mv = [gr.mvn(row) for row in np.asarray(q, np.float64)]
    return np.array([m for m, _ in mv]), np.array([L @ L.T for _, L in mv])


def outputs(model, u, dw, rows=None, ev=None):
    """out [n, 15] (iterations and flags' bit 0 left 0) and the raw heads [n, 5] at logits u; Sigma = A^-1 there."""
    ev = model.evaluate(u, rows) if ev is None else ev
    rows = np.arange(model.N) if rows is None else np.asarray(rows)
    u = np.clip(np.asarray(u, np.float64).reshape(-1, 2), -CLIP, CLIP)
    A = ev["A"]
    Sigma = np.linalg.inv(A)
    sa, sb = _sig(u[:, 0]), _sig(u[:, 1])
    oef, dbv = 0.8 * sa + 0.04, 0.2 * sb + 0.001
    da, db = 0.8 * sa * (1 - sa), 0.2 * sb * (1 - sb)
    out = np.zeros((u.shape[0], OUT_COLUMNS))
    out[:, 0:2] = u
    out[:, 2], out[:, 3], out[:, 4] = oef, dbv, dw * oef * dbv
    out[:, 5], out[:, 6] = np.sqrt(Sigma[:, 0, 0]), np.sqrt(Sigma[:, 1, 1])
    out[:, 7] = Sigma[:, 0, 1] / (out[:, 5] * out[:, 6])
    out[:, 8], out[:, 9] = da * out[:, 5], db * out[:, 6]
    gr2 = np.stack([dw * dbv * da, dw * oef * db], -1)
    out[:, 10] = np.sqrt(np.einsum("ni,nij,nj->n", gr2, Sigma, gr2))
    out[:, 11] = -ev["F"] + model.const[rows] + math.log(2 * math.pi) - 0.5 * np.log(np.linalg.det(A))
    out[:, 12] = ev["chi2"]
    q, clamped = heads_from(u, Sigma)
    on_clip = (np.abs(u) >= CLIP).any(1)
    out[:, 14] = 2.0 * on_clip + 4.0 * clamped
    return out, q


def lm(model, u0=None, max_iter=50, lambda0=1e-2, lambda_up=10.0, lambda_down=3.0, tol=1e-3):
    """The header's schedule in float64: dict(u [N, 2], iterations [N], converged [N], ev = evaluate(u))."""
    N = model.N
    u = np.clip(model.mu.copy() if u0 is None else np.asarray(u0, np.float64).reshape(N, 2), -CLIP, CLIP)
    cur = model.evaluate(u)
    lam = np.full(N, float(lambda0))
    conv = cur["dec"] < tol
    act = ~conv & np.isfinite(cur["F"])
    iters = np.zeros(N, int)
    for _ in range(int(max_iter)):
        if not act.any():
            break
        idx = np.nonzero(act)[0]
        A, g = cur["A"][idx], cur["g"][idx]
        M = A.copy()
        M[:, 0, 0] *= 1.0 + lam[idx]
        M[:, 1, 1] *= 1.0 + lam[idx]
        ut = np.clip(u[idx] - np.linalg.solve(M, g[:, :, None])[:, :, 0], -CLIP, CLIP)
        ev = model.evaluate(ut, idx)
        iters[idx] += 1
        bd = np.maximum(cur["band"][idx], ev["band"])
        dl = ut - u[idx]
        dF = cur["F"][idx] - ev["F"]
        with np.errstate(invalid="ignore", divide="ignore"):
            # inside the band the reduction is the trapezoid rule on the two gradients (the tie rule)
            dF = np.where(np.abs(dF) <= bd, -0.5 * np.einsum("ni,ni->n", g + ev["g"], dl), dF)
            better = dF > 0.0
            # the quadratic model's reduction along the step actually taken (after the clip): the gain rule
            pred = -np.einsum("ni,ni->n", g, dl) - 0.5 * np.einsum("ni,nij,nj->n", dl, A, dl)
            poor = better & ~(dF >= GAIN_MIN * pred)
        acc, rej = idx[better], idx[~better]
        shrink, grow = idx[better & ~poor], idx[~better | poor]
        u[acc] = ut[better]
        for k in cur:
            cur[k][acc] = ev[k][better]
        lam[shrink] = np.maximum(lam[shrink] * (1.0 / lambda_down), LAM_MIN)
        lam[grow] = np.minimum(lam[grow] * lambda_up, LAM_MAX)
        done = acc[cur["dec"][acc] < tol]
        conv[done] = True
        act[done] = False
    return dict(u=u, iterations=iters, converged=conv, ev=cur)


# ---- protocols: the reference's 11 and 24 taus plus the table of tests/test_gpu_forward_protocols.py -----------------
def protocol_names():
    import test_gpu_forward_protocols as fp
    return ("ref11", "ref24") + tuple(fp.PROTOCOLS)


def setup(params, name):
    """(system parameters, loss switches) of a protocol name."""
    import test_gpu_forward_protocols as fp
    if name == "ref11":
        return dict(params), {}
    if name == "ref24":
        return dict(params, tau_start="-0.028", tau_end="0.065", tau_step="0.004"), {}
    return fp.protocol(params, name), fp.switches(name)


def model_of(o64, d, sw, rows=None):
    rows = slice(None) if rows is None else rows
    return Model(o64, d["x"][rows], d["sigma"][rows], d["prior"][rows], multi=bool(sw))


# ---- the seeded synthetic voxels of the tests ------------------------------------------------------------------------
N_VOX = 333          # two full 128-thread blocks, a partial one, and a partial wave
SIGMA = 0.02
_INPUTS = {}


def inputs(o32, name, n=N_VOX, seed=7, noise=True):
    """dict(x, sigma, prior, mask, live, truth [n, 2], u_true [n, 2]) for the protocol of the f32 Oracle `o32` (name keys
    the cache): truths OEF 0.2 - 0.6, DBV 0.02 - 0.1, noise of sd
    SIGMA on the spin-echo-normalised signal, sigma = SIGMA (+-10 % per tau), priors centred within a prior sd of the
    truth with spread heads, a quarter of the voxels masked out.  Computed once and never written to."""
    key = (name, n, seed, noise)
    if key not in _INPUTS:
        rng = np.random.default_rng(seed)
        T = o32.T
        truth = np.stack([rng.uniform(0.2, 0.6, n), rng.uniform(0.02, 0.1, n)], -1)
        s = np.asarray(o32.signal_fwd(truth.astype(np.float32)), np.float64)
        if noise:
            s = s + SIGMA * s[:, o32.se_idx:o32.se_idx + 1] * rng.standard_normal((n, T))
        x = s.astype(np.float32)
        sigma = (SIGMA * rng.uniform(0.9, 1.1, (n, T))).astype(np.float32)
        u_true = np.stack([np.log((truth[:, 0] - 0.04) / (0.84 - truth[:, 0])),
                           np.log((truth[:, 1] - 0.001) / (0.201 - truth[:, 1]))], -1)
        prior = np.zeros((n, 5), np.float32)
        prior[:, 0] = u_true[:, 0] + 0.4 * rng.standard_normal(n)
        prior[:, 2] = u_true[:, 1] + 0.4 * rng.standard_normal(n)
        prior[:, 1] = rng.uniform(0.05, 0.25, n)      # s_o = 3 tanh - 1 in (-0.85, -0.27): prior sd 0.43 - 0.77 logits
        prior[:, 3] = rng.uniform(0.05, 0.25, n)
        prior[:, 4] = rng.uniform(-0.5, 0.5, n)
        from test_gpu_forward_protocols import make_mask
        mask = make_mask(n)
        d = dict(x=x, sigma=sigma, prior=prior, mask=mask, live=mask > 0, truth=truth, u_true=u_true)
        for a in d.values():
            a.setflags(write=False)
        _INPUTS[key] = d
    return _INPUTS[key]
