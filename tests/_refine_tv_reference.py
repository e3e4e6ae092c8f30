"""Float64 reference of the refinement of a volume under the TV smoothness prior (qbold_refine_posterior_spatial):
the TV term of smoothness_loss (model.py:726-754) on the sigmoids of heads 0 and 2 over x- and y-adjacent pairs inside
the mask, its subgradient (sign(0) = 0), and the Jacobi loop -- every voxel's gradient at the step-j heads of all
voxels, then each voxel's own Adam or SGD update -- on top of tests/_refine_reference.py's per-voxel step gradient.
Test infrastructure (no GPU needed)."""
import numpy as np

from _refine_reference import cosine_lr, step_grad


def _sig(u):
    return 1.0 / (1.0 + np.exp(-u))


def _edges(mask):
    """(axis, live pair mask [B, X', Y', Z]) for the x (axis 1) and y (axis 2) neighbour pairs with both masks > 0."""
    live = np.asarray(mask) > 0
    return [(1, live[:, 1:] & live[:, :-1]), (2, live[:, :, 1:] & live[:, :, :-1])]


def _diff(p, axis):
    return np.diff(p, axis=axis)   # p[n + 1] - p[n] along the axis


def tv_value(q5, mask):
    """TV(q) = sum over live x / y pairs of |sig(q0_v) - sig(q0_n)| + |sig(q2_v) - sig(q2_n)| (Oracle.smoothness_loss
    times sum(mask))."""
    q5 = np.asarray(q5, np.float64)
    tot = 0.0
    for ch in (0, 2):
        p = _sig(q5[..., ch])
        for axis, live in _edges(mask):
            tot += np.abs(_diff(p, axis))[live].sum()
    return tot


def tv_grad(q5, mask, w=1.0):
    """w d TV / d q [B, X, Y, Z, 5] with sign(0) = 0 (tf.abs' gradient), and the smallest |difference| over live pairs
    (inf without any)."""
    q5 = np.asarray(q5, np.float64)
    g = np.zeros_like(q5)
    gap = np.inf
    for ch in (0, 2):
        p = _sig(q5[..., ch])
        acc = np.zeros_like(p)
        for axis, live in _edges(mask):
            d = _diff(p, axis)
            if live.any():
                gap = min(gap, np.abs(d[live]).min())
            s = np.where(live, np.sign(d), 0.0)   # d TV / d p[n + 1] = +s, d TV / d p[n] = -s
            pad_hi = [(0, 0)] * 4
            pad_lo = [(0, 0)] * 4
            pad_hi[axis] = (1, 0)
            pad_lo[axis] = (0, 1)
            acc += np.pad(s, pad_hi) - np.pad(s, pad_lo)
        g[..., ch] = w * acc * p * (1.0 - p)
    return g, gap


def refine_tv_reference(o, x5, mask, q5, prior5, sigma5, z, S, w, lr, lr_final=None, optimizer="adam",
                        betas=(0.9, 0.999), eps=1e-8):
    """The Jacobi loop in float64.  x5, sigma5 [B, X, Y, Z, T], q5, prior5 [B, X, Y, Z, 5], mask [B, X, Y, Z],
    z [N, steps, Sp, 2] as the kernel takes it.  Voxels with mask <= 0 keep q.  Returns (q [B, X, Y, Z, 5], the
    smallest |sigmoid difference| over all live pairs and steps)."""
    z = np.asarray(z, np.float64)
    steps = z.shape[1]
    lead = np.asarray(q5).shape[:4]
    lr_final = lr if lr_final is None else lr_final
    live = (np.asarray(mask) > 0).reshape(-1)
    x = np.asarray(x5).reshape(-1, np.asarray(x5).shape[-1])[live]
    sg = np.asarray(sigma5).reshape(-1, np.asarray(sigma5).shape[-1])[live]
    pr = np.asarray(prior5).reshape(-1, 5)[live]
    zl = z[live]
    qv = np.array(q5, np.float64, copy=True).reshape(-1, 5)
    m1 = np.zeros((live.sum(), 5))
    m2 = np.zeros_like(m1)
    b1, b2 = betas
    gap = np.inf
    for j in range(steps):
        gt, gj = tv_grad(qv.reshape(lead + (5,)), mask, w)
        gap = min(gap, gj)
        g = step_grad(o, x, qv[live], pr, sg, zl[:, j, :S]) + gt.reshape(-1, 5)[live]
        lr_j = cosine_lr(j, steps, lr, lr_final)
        if optimizer == "adam":
            m1 = b1 * m1 + (1.0 - b1) * g
            m2 = b2 * m2 + (1.0 - b2) * g * g
            qv[live] -= lr_j * (m1 / (1.0 - b1 ** (j + 1))) / (np.sqrt(m2 / (1.0 - b2 ** (j + 1))) + eps)
        else:
            qv[live] -= lr_j * g
    return qv.reshape(lead + (5,)), gap
