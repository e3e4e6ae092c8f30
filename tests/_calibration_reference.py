"""Float64 NumPy restatement of qbold_calibration (include/qbold_hip.h) and the inputs the calibration tests share.

calibration() returns the six columns and, per rank statistic, `near`: how many draws (or, with weights, how much
normalised weight) lie so close to the truth that a float32 evaluation of the draw may legitimately put it on the other
side.  A test holds the kernel's rank to the reference's within that per-voxel allowance, so no voxel is left out of the
comparison and every voxel without such a draw is compared exactly.
"""
import functools
import math

import numpy as np

GAP = 1e-4   # relative closeness of a draw to the truth that counts as `near`


def transformed_heads(q):
    """Raw heads [N, 5] -> (mu_o, s_o, mu_d, s_d, c): transform_std = 3 tanh - 1, transform_offdiag = e^-2 tanh."""
    q = np.asarray(q, np.float64)
    return q[:, 0], 3.0 * np.tanh(q[:, 1]) - 1.0, q[:, 2], 3.0 * np.tanh(q[:, 3]) - 1.0, np.tanh(q[:, 4]) * math.exp(-2.0)


def unit_clip(x):
    """clamp to [1e-6, 1 - 1e-6] that keeps a NaN"""
    return np.where(x < 1e-6, 1e-6, np.where(x > 1.0 - 1e-6, 1.0 - 1e-6, x))


def truth_logits(theta):
    """(a*, b*): the logits of the clamped unit-interval values of (OEF, DBV)."""
    theta = np.asarray(theta, np.float64)
    x0, x1 = unit_clip((theta[:, 0] - 0.04) / 0.8), unit_clip((theta[:, 1] - 0.001) / 0.2)
    return np.log(x0) - np.log1p(-x0), np.log(x1) - np.log1p(-x1)


def forward_transform(a, b):
    return 0.8 / (1.0 + np.exp(-a)) + 0.04, 0.2 / (1.0 + np.exp(-b)) + 0.001


def norm_cdf(w):
    return 0.5 * np.vectorize(math.erfc)(-np.asarray(w, np.float64) / math.sqrt(2.0))


def draws(q, z):
    """The logit draws a, b [N, L] of the heads q at the normals z [N, L, 2]."""
    mu_o, s_o, mu_d, s_d, c = transformed_heads(q)
    z = np.asarray(z, np.float64)
    a = mu_o[:, None] + z[:, :, 0] * np.exp(s_o)[:, None]
    b = mu_d[:, None] + z[:, :, 0] * c[:, None] + z[:, :, 1] * np.exp(s_d)[:, None]
    return a, b


def normalised_weights(log_w):
    """w~ [N, L] and the rows that cannot be used (a NaN, a +inf, or no finite entry)."""
    lw = np.asarray(log_w, np.float64)
    bad = np.isnan(lw).any(1) | np.isposinf(lw).any(1) | ~np.isfinite(lw).any(1)
    safe = np.where(bad[:, None], 0.0, lw)
    w = np.exp(safe - safe.max(1, keepdims=True))
    return w / w.sum(1, keepdims=True), bad


def calibration(theta_true, q, z, log_w=None, gap=GAP):
    """out [N, 6] (float64) and near [N, 3] of qbold_calibration at explicit normals z [N, L, 2]."""
    theta = np.asarray(theta_true, np.float64)
    mu_o, s_o, mu_d, s_d, c = transformed_heads(q)
    a_t, b_t = truth_logits(theta)
    N, L = np.asarray(z).shape[:2]
    out = np.full((N, 6), np.nan)
    w0 = (a_t - mu_o) * np.exp(-s_o)
    w1 = (b_t - mu_d) * np.exp(-s_d) - (a_t - mu_o) * c * np.exp(-s_o - s_d)
    out[:, 0] = norm_cdf(w0)
    out[:, 1] = norm_cdf((b_t - mu_d) / np.sqrt(c * c + np.exp(2.0 * s_d)))
    out[:, 2] = -np.expm1(-0.5 * (w0 * w0 + w1 * w1))
    a, b = draws(q, z)
    oef, dbv = forward_transform(a, b)
    if log_w is None:
        w, bad = np.full((N, L), 1.0 / L), np.zeros(N, bool)
    else:
        w, bad = normalised_weights(log_w)
    near = np.zeros((N, 3), np.int64 if log_w is None else np.float64)
    stats = ((a, a_t, np.maximum(1.0, np.abs(a_t))), (b, b_t, np.maximum(1.0, np.abs(b_t))),
             (oef * dbv, theta[:, 0] * theta[:, 1], np.abs(theta[:, 0] * theta[:, 1])))
    for j, (d, t, scale) in enumerate(stats):
        below, ties = d < t[:, None], d == t[:, None]
        if log_w is None:
            out[:, 3 + j] = (2 * below.sum(1) + ties.sum(1)) / (2.0 * L)
        else:
            out[:, 3 + j] = (w * below).sum(1) + 0.5 * (w * ties).sum(1)
        close = np.abs(d - t[:, None]) <= gap * scale[:, None]
        near[:, j] = close.sum(1) if log_w is None else (w * close).sum(1)
        lost = bad | np.isnan(t) | np.isnan(d).any(1)   # a comparison with a NaN is false: it must not look like a rank
        out[lost, 3 + j] = np.nan
    return out, near


def brute_force_ranks(theta_true, q, z):
    """The unweighted rank fractions by sorting: the position of the truth among the sorted draws, ties at half."""
    a, b = draws(q, z)
    oef, dbv = forward_transform(a, b)
    a_t, b_t = truth_logits(theta_true)
    th = np.asarray(theta_true, np.float64)
    N, L = a.shape
    r = np.empty((N, 3))
    for j, (d, t) in enumerate(((a, a_t), (b, b_t), (oef * dbv, th[:, 0] * th[:, 1]))):
        s = np.sort(d, 1)
        for i in range(N):
            lo, hi = np.searchsorted(s[i], t[i], "left"), np.searchsorted(s[i], t[i], "right")
            r[i, j] = (lo + hi) / (2.0 * L)
    return r


def truths_from(q, zt):
    """(OEF, DBV) float32 of the logit-space point mu + L_q zt under the heads q."""
    mu_o, s_o, mu_d, s_d, c = transformed_heads(q)
    oef, dbv = forward_transform(mu_o + zt[:, 0] * np.exp(s_o), mu_d + zt[:, 0] * c + zt[:, 1] * np.exp(s_d))
    return np.stack([oef, dbv], 1).astype(np.float32)


# ---- the inputs of the comparison against the kernel (tests 1 and 4 of tests/test_gpu_calibration.py) ------------------
N_CASE = 300          # a tail in every tiling: not a multiple of 16 or 64
L_CASES = (1, 2, 25, 255, 1000)
L_WEIGHTED = (25, 64, 1000)


@functools.lru_cache(maxsize=None)
def comparison_case(L, weighted=False):
    """(theta_true, q, z, log_w or None, out, near): heads over the whole range of the transforms; truths 100 from q, 100
    at three times q's spread (ranks 0 and L), 100 from q of which 10 each sit at OEF 0.04, OEF 0.84, DBV 0.001, DBV
    0.201 (the clamp).  Weighted: log_w = 3 N(0, 1) with a few -inf."""
    rng = np.random.default_rng(1000 + L)
    N = N_CASE
    q = np.stack([rng.uniform(-2, 2, N), rng.uniform(-1.5, 1.5, N), rng.uniform(-3, 1, N), rng.uniform(-1.5, 1.5, N),
                  rng.uniform(-2, 2, N)], 1).astype(np.float32)
    zt = rng.standard_normal((N, 2))
    zt[100:200] *= 3.0
    th = truths_from(q, zt)
    th[200:210, 0], th[210:220, 0] = 0.04, 0.84
    th[220:230, 1], th[230:240, 1] = 0.001, 0.201
    z = rng.standard_normal((N, L, 2)).astype(np.float32)
    lw = None
    if weighted:
        lw = (3.0 * rng.standard_normal((N, L))).astype(np.float32)
        lw[rng.uniform(size=(N, L)) < 0.02] = -np.inf
        lw[:, 0] = np.where(np.isfinite(lw).any(1), lw[:, 0], 0.0)   # every row keeps a finite entry
    out, near = calibration(th, q, z, lw)
    return th, q, z, lw, out, near


# ---- the known answer (test 7): truths drawn from q itself, and from twice its spread ------------------------------------
KNOWN_N, KNOWN_L, KNOWN_BINS = 20000, 255, 16


@functools.lru_cache(maxsize=None)
def known_answer_inputs():
    """{scale: (theta_true, q, z)} for scale 1 (calibrated) and 2 (over-confident), all from default_rng(5)."""
    rng = np.random.default_rng(5)
    N, L = KNOWN_N, KNOWN_L
    q = np.stack([rng.uniform(-1.5, 1.5, N), rng.uniform(-1, 0.3, N), rng.uniform(-2.5, 0.5, N), rng.uniform(-1, 0.3, N),
                  rng.uniform(-2, 2, N)], 1).astype(np.float32)
    cases = {}
    for scale in (1.0, 2.0):
        th = truths_from(q, rng.standard_normal((N, 2)) * scale)
        cases[scale] = (th, q, rng.standard_normal((N, L, 2)).astype(np.float32))
    return cases


def check_known_answer(summaries):
    """The statistical condition of the known-answer test on {scale: calibration.summarise(...)}.  15 degrees of freedom:
    37.70 is the 0.999 quantile of chi2_15.  Twice the spread: a central interval of nominal 90 % covers
    2 Phi(1.645 / 2) - 1 = 0.589, the 90 % highest-density ellipse 1 - exp(-4.605 / 8) = 0.438."""
    from qbold_vi_amd.calibration import COLUMNS
    i90 = summaries[1.0]["levels"].index(0.9)
    for name in COLUMNS:
        good, over = summaries[1.0]["stats"][name], summaries[2.0]["stats"][name]
        print(f"{name}: chi2 {good['chi2']:.2f} cov90 {good['coverage'][i90]:.4f} | over-confident chi2 "
              f"{over['chi2']:.0f} cov90 {over['coverage'][i90]:.4f}")
        assert sum(good["hist"]) == KNOWN_N and sum(over["hist"]) == KNOWN_N
        assert good["chi2"] < 37.70, (name, good["chi2"])
        assert abs(good["coverage"][i90] - 0.90) <= 0.02, (name, good["coverage"][i90])
        assert over["chi2"] > 1000.0, (name, over["chi2"])
        want = 0.438 if name == "hpd" else 0.589
        assert abs(over["coverage"][i90] - want) <= 0.02, (name, over["coverage"][i90])
