"""Float64 restatement of Pareto-smoothed importance sampling (Vehtari, Simpson, Gelman, Yao, Gabry, JMLR 2024) as
qbold_psis defines it (include/qbold_hip.h), in the paper's literal form: the tail y = exp(x) - exp(c), a stable argsort,
a strict `>` against the cutoff.  form="expm1" switches the fit scale to the kernel's y = expm1(x - c).  No third-party
PSIS package is used.  Test infrastructure (no GPU needed)."""
import math

import numpy as np


def tail_size(K):
    """M = ceil(min(K / 5, 3 sqrt K))"""
    return int(math.ceil(min(K / 5.0, 3.0 * math.sqrt(K))))


def khat_threshold(K):
    return min(1.0 - 1.0 / math.log10(K), 0.7)


def gpd_fit(y):
    """Zhang & Stephens' estimate for ascending y > 0: (k^ with the paper's prior, k, sigma)."""
    n = y.shape[0]
    m = 30 + int(math.floor(math.sqrt(n)))
    j = np.arange(1, m + 1, dtype=np.float64)
    q = int(math.floor(n / 4.0 + 0.5))
    b = 1.0 / y[-1] + (1.0 - np.sqrt(m / (j - 0.5))) / (3.0 * y[q - 1])
    kj = np.log1p(-b[:, None] * y[None, :]).mean(1)
    L = n * (np.log(-b / kj) - kj - 1.0)
    Lm = L.max()
    w = np.exp(L - Lm)
    w = w / w.sum()           # softmax as a log-sum-exp: the literal exp(L_j - L_i) overflows
    bhat = float((w * b).sum())
    k = float(np.log1p(-bhat * y).mean())
    sigma = -k / bhat
    return (n * k + 5.0) / (n + 10.0), k, sigma


def psis_row(lw, theta=None, form="literal"):
    """One row: dict(khat, log_p, ess, n, weights [K] = normalised log w~, means [C] or None, c)."""
    lw = np.asarray(lw, np.float64)
    K = lw.shape[0]
    nan = float("nan")
    if np.isnan(lw).any() or not np.isfinite(lw.max()):
        return dict(khat=nan, log_p=nan, ess=nan, n=nan, weights=np.full(K, nan),
                    means=None if theta is None else np.full(np.asarray(theta).shape[1], nan), c=nan)
    mx = lw.max()
    x = lw - mx
    M = tail_size(K)
    c = np.sort(x)[K - 1 - M]                    # the (M + 1)-th largest
    tail = np.nonzero(x > c)[0]                  # strictly above: ties at the cutoff shorten the tail
    n = tail.shape[0]
    xs = x.copy()
    khat = float("inf")
    with np.errstate(all="ignore"):
        if n > 4 and not (-c > 80.0):
            order = tail[np.argsort(x[tail], kind="stable")]   # ascending, equal values by ascending draw
            xt = x[order]
            if form == "literal":
                scale = math.exp(c)
                y = np.exp(xt) - scale
            else:
                scale = 1.0
                y = np.expm1(xt - c)
            kh, k, sigma = gpd_fit(y)
            if np.isfinite(kh) and np.isfinite(sigma):
                khat = kh
                p = (np.arange(1, n + 1) - 0.5) / n
                l1 = np.log1p(-p)
                qy = -sigma * l1 if k == 0.0 else sigma * np.expm1(-k * l1) / k
                sm = np.log(scale + qy) if form == "literal" else c + np.log1p(qy)
                xs[order] = np.minimum(sm, 0.0)
        m2 = xs.max()
        lse = m2 + math.log(np.exp(xs - m2).sum())
        lwn = xs - lse
        w = np.exp(lwn)
        means = None
        if theta is not None:
            means = (w[:, None] * np.asarray(theta, np.float64)).sum(0)
        return dict(khat=khat, log_p=mx + lse - math.log(K), ess=1.0 / (w * w).sum(), n=float(n), weights=lwn,
                    means=means, c=float(c))


def psis(log_w, theta=None, form="literal"):
    """Rows [N, K] -> dict of stacked results: out [N, 4] = (khat, log_p, ess, n), weights [N, K], means [N, C], c [N]."""
    log_w = np.asarray(log_w)
    rows = [psis_row(log_w[i], None if theta is None else theta[i], form) for i in range(log_w.shape[0])]
    return dict(out=np.array([[r["khat"], r["log_p"], r["ess"], r["n"]] for r in rows], np.float64),
                weights=np.stack([r["weights"] for r in rows]),
                means=None if theta is None else np.stack([r["means"] for r in rows]),
                c=np.array([r["c"] for r in rows]))


TAIL_SHAPES = (-0.3, 0.0, 0.3, 0.6, 0.9, 1.3)


def make_rows(K, rows_per_shape=40, seed=0):
    """The rows of the GPU comparison, float32 [6 * rows_per_shape, K]: generalised-Pareto weights of shape k in
    TAIL_SHAPES plus 0.05, raised to a power from U(0.5, 3), with log-normal jitter of sd 0.3, centred at -40."""
    out = []
    for s, k in enumerate(TAIL_SHAPES):
        rng = np.random.default_rng([seed, K, s])
        for _ in range(rows_per_shape):
            l1 = np.log1p(-rng.uniform(size=K))
            g = -l1 if k == 0.0 else np.expm1(-k * l1) / k          # GPD(k, 1) quantiles
            lw = rng.uniform(0.5, 3.0) * np.log(g + 0.05) + 0.3 * rng.standard_normal(K)
            out.append(lw - lw.mean() - 40.0)
    return np.asarray(out, np.float32)
