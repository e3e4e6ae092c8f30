"""Float64 restatement of qbold_draw_summary's definitions (include/qbold_hip.h): normalised weights, two-pass moments,
quantiles by the inverse weighted ECDF, the shortest interval of a given mass, ESS, the largest weight and the weighted
correlations; plus the rows of the GPU comparison and the probability-level bound the float32 kernel is held to.  Test
infrastructure (no GPU needed)."""
import numpy as np

LEVELS = (0.025, 0.25, 0.5, 0.75, 0.975)     # the five levels of the comparison
MASS = 0.95


def eps(K):
    """(K + 32) 2^-23: a float32 prefix sum of K normalised weights has at most K - 1 roundings of at most 2^-24 each,
    and the 32 covers expf and the normalisation, so any summation order keeps each W_r within eps / 2 of its float64
    value; a comparison of W_r (or of a difference of two) with a level then decides as float64 would at a level within
    eps."""
    return (K + 32) * 2.0 ** -23


def weights(lw):
    """w~ [K] in float64"""
    lw = np.asarray(lw, np.float64)
    e = np.exp(lw - lw.max())
    return e / e.sum()


def _sorted(theta, w):
    theta = np.asarray(theta, np.float64)
    o = np.argsort(theta, kind="stable")      # ascending, equal values by ascending draw
    return theta[o], np.cumsum(np.asarray(w, np.float64)[o])


def q_ref(theta, w, p):
    """theta_(r*), r* = min{r : W_r >= p}, clamped to K - 1."""
    ts, W = _sorted(theta, w)
    return ts[min(int(np.searchsorted(W, p, side="left")), ts.shape[0] - 1)]


def hpd_ref(theta, w, mass):
    """(lo, hi) of the shortest [theta_(a), theta_(b)] with W_b - W_{a-1} >= mass (tested as W_b >= W_{a-1} + mass); for
    each a the smallest feasible b; width ties to the smallest a; an a without a feasible b is skipped."""
    ts, W = _sorted(theta, w)
    K = ts.shape[0]
    prev = np.concatenate([[0.0], W[:-1]])
    b = np.searchsorted(W, prev + mass, side="left")
    ok = b < K
    if not ok.any():
        return ts[0], ts[-1]
    a = np.nonzero(ok)[0]
    width = ts[b[ok]] - ts[a]
    i = int(np.argmin(width))                 # the first of equal widths: the smallest a
    return ts[a[i]], ts[b[ok][i]]


def mass_between(theta, w, lo, hi):
    theta = np.asarray(theta, np.float64)
    return float(np.asarray(w, np.float64)[(theta >= lo) & (theta <= hi)].sum())


def moments(theta, w):
    """theta [K, C] -> dict(mean [C], sd [C], corr [C (C - 1) / 2] in the order (0,1), (0,2), ..., ess, wmax)."""
    theta = np.asarray(theta, np.float64)
    w = np.asarray(w, np.float64)
    mean = (w[:, None] * theta).sum(0)
    d = theta - mean
    sd = np.sqrt((w[:, None] * d * d).sum(0))
    C = theta.shape[1]
    with np.errstate(all="ignore"):
        corr = np.array([(w * d[:, i] * d[:, j]).sum() / (sd[i] * sd[j]) if sd[i] > 0 and sd[j] > 0 else np.nan
                         for i in range(C) for j in range(i + 1, C)], np.float64)
    return dict(mean=mean, sd=sd, corr=corr, ess=1.0 / (w * w).sum(), wmax=w.max())


def make_rows(K, rows=240, seed=0):
    """(log_w float32 [240, K], theta float32 [240, K, 3]): Gaussian log-weights of scale 0.3 / 1 / 2.5 (a third of the
    rows each), every second row with a Pareto tail (shape 1) on top; theta uniform(0.5, 1.5) rounded to float32."""
    rng = np.random.default_rng([seed, K, 77])
    scale = np.repeat(np.array([0.3, 1.0, 2.5]), rows // 3)[:, None]
    lw = scale * rng.standard_normal((rows, K))
    tail = -np.log(rng.uniform(size=(rows, K)))
    tail[0::2] = 0.0
    lw = lw + tail - 40.0
    theta = rng.uniform(0.5, 1.5, (rows, K, 3))
    return lw.astype(np.float32), theta.astype(np.float32)


_REF = {}


def reference(K, levels=LEVELS, mass=MASS):
    """The float64 reference of make_rows(K), computed once per K: dict(lw, theta, w [N, K], q_lo / q_hi [N, C, P] =
    q_ref at p -+ eps, hpd_lo / hpd_hi [N, C, 2] = hpd_ref at mass -+ eps (as (lo, hi)), mean, sd [N, C], corr [N, 3],
    ess, wmax [N])."""
    key = (K, tuple(levels), mass)
    if key in _REF:
        return _REF[key]
    lw, theta = make_rows(K)
    N, _, C = theta.shape
    e = eps(K)
    r = dict(lw=lw, theta=theta, w=np.stack([weights(row) for row in lw]),
             q_lo=np.empty((N, C, len(levels))), q_hi=np.empty((N, C, len(levels))),
             hpd_lo=np.empty((N, C, 2)), hpd_hi=np.empty((N, C, 2)), mean=np.empty((N, C)), sd=np.empty((N, C)),
             corr=np.empty((N, C * (C - 1) // 2)), ess=np.empty(N), wmax=np.empty(N))
    for i in range(N):
        w = r["w"][i]
        m = moments(theta[i], w)
        r["mean"][i], r["sd"][i], r["corr"][i], r["ess"][i], r["wmax"][i] = m["mean"], m["sd"], m["corr"], m["ess"], \
            m["wmax"]
        for c in range(C):
            ts, W = _sorted(theta[i, :, c], w)
            for j, p in enumerate(levels):
                r["q_lo"][i, c, j] = ts[min(int(np.searchsorted(W, p - e, side="left")), K - 1)]
                r["q_hi"][i, c, j] = ts[min(int(np.searchsorted(W, p + e, side="left")), K - 1)]
            r["hpd_lo"][i, c] = hpd_ref(theta[i, :, c], w, mass - e)
            r["hpd_hi"][i, c] = hpd_ref(theta[i, :, c], w, mass + e)
    _REF[key] = r
    return r


def check_sandwich(theta, w, quant, stats, levels, mass, K=None):
    """The kernel's quantiles [C, P] and (lo, hi) = stats[:, 2:4] of ONE row against the float64 rule at the levels
    p -+ eps and the masses mass -+ eps.  theta [K, C] float32, w [K] float64 normalised.  Returns the number of
    (column, level) cases in which the two reference quantiles coincide (the kernel value is then pinned exactly)."""
    K = theta.shape[0] if K is None else K
    e = eps(K)
    pinned = 0
    for c in range(theta.shape[1]):
        col = theta[:, c].astype(np.float64)
        for j, p in enumerate(levels):
            lo, hi = q_ref(col, w, p - e), q_ref(col, w, p + e)
            v = float(quant[c, j])
            assert lo <= v <= hi, (c, p, lo, v, hi)
            assert v in col
            pinned += lo == hi
        lo, hi = float(stats[c, 2]), float(stats[c, 3])
        assert lo in col and hi in col and lo <= hi, (c, lo, hi)
        assert mass_between(col, w, lo, hi) >= mass - e, (c, mass_between(col, w, lo, hi))
        a, b = hpd_ref(col, w, mass + e)
        assert hi - lo <= b - a, (c, hi - lo, b - a)
        a, b = hpd_ref(col, w, mass - e)
        assert hi - lo >= b - a, (c, hi - lo, b - a)
    return pinned
