"""Posterior calibration summaries (simulation-based calibration: Talts et al. 2018; Sailynoja et al. 2022).

Context.calibration (qbold_calibration) places a known truth in each voxel's posterior: out [N, 6] = (pit_oef, pit_dbv,
hpd, rank fractions of OEF, DBV, R2'), every column Uniform(0, 1) over voxels exactly when the posterior's intervals
cover as often as they claim.  summarise() turns those columns into what one reads: a histogram per statistic, its
chi-square distance from uniform, and the coverage of the central intervals (of the highest-density regions for hpd) at
a few levels.  Torch only, on CPU or GPU tensors; nothing here touches the kernels.
"""
import math

import torch

COLUMNS = ("pit_oef", "pit_dbv", "hpd", "rank_oef", "rank_dbv", "rank_r2p")


def _table(out, L, bins, levels, weighted):
    n = int(out.shape[0])
    stats = {}
    for j, name in enumerate(COLUMNS):
        u = out[:, j]
        if j >= 3 and not weighted:
            # (2 #less + #equal) / (2 L) -> r = floor(#less + #equal / 2) in {0 .. L}; the quarter absorbs the float32
            # division's rounding (below 0.07 at L = 2^20) without reaching the next half
            r = torch.floor(u * L + 0.25).clamp_(0, L).long()
            idx = r * bins // (L + 1)
            u = (r.double() + 0.5) / (L + 1)
        else:
            idx = torch.floor(u * bins).long().clamp_(0, bins - 1)
        h = torch.bincount(idx, minlength=bins).double()
        if n > 0:
            e = n / bins
            chi2 = float(((h - e) ** 2 / e).sum())
            p = float(torch.special.gammaincc(torch.tensor((bins - 1) / 2.0, dtype=torch.float64),
                                              torch.tensor(chi2 / 2.0, dtype=torch.float64)))
        else:
            chi2, p = float("nan"), float("nan")
        cov, se = [], []
        for lev in levels:
            inside = (u <= lev) if name == "hpd" else ((u - 0.5).abs() <= lev / 2.0)
            cov.append(float(inside.double().mean()) if n > 0 else float("nan"))
            se.append(math.sqrt(lev * (1.0 - lev) / n) if n > 0 else float("nan"))   # under the nominal level
        stats[name] = dict(hist=[int(v) for v in h.tolist()], chi2=chi2, p_value=p, coverage=cov, coverage_se=se)
    return dict(n=n, stats=stats)


def summarise(out, L, bins=16, levels=(0.5, 0.8, 0.9, 0.95), weighted=False, khat=None):
    """Histograms, uniformity chi-square and interval coverage of Context.calibration's out [..., 6] at L draws.

    Rows with a NaN (voxels outside the mask, rows of unusable weights) are dropped and counted.  Per statistic
    (COLUMNS):
      hist         `bins` counts.  Unweighted ranks r = floor(out L) in {0 .. L} go to bin r bins // (L + 1), which needs
                   (L + 1) % bins == 0 (ValueError otherwise: unequal bins are not uniform under calibration); PIT, hpd
                   and weighted ranks (weighted=True: log_w was given) to bin min(floor(u bins), bins - 1).
      chi2         sum (h - n / bins)^2 / (n / bins), and p_value = gammaincc((bins - 1) / 2, chi2 / 2)
      coverage     per level l the fraction with |u - 1/2| <= l / 2 (u = (r + 1/2) / (L + 1) for unweighted ranks), for
                   hpd the fraction with hpd <= l; coverage_se = sqrt(l (1 - l) / n), the binomial standard error of a
                   calibrated posterior.
    khat [...] (the Pareto k^ of each voxel's weights): adds `reliable`, the same table over the voxels with
    khat < ops.psis_khat_threshold(L), and `khat_threshold`.
    Returns dict(n, dropped, L, bins, levels, weighted, stats[, khat_threshold, reliable = dict(n, stats)]); plain
    Python numbers, so json.dump takes it as it is."""
    L, bins = int(L), int(bins)
    if L < 1 or bins < 2:
        raise ValueError("summarise: need L >= 1 and bins >= 2")
    if not weighted and (L + 1) % bins != 0:
        raise ValueError(f"summarise: the {L + 1} possible ranks of L = {L} draws do not split into {bins} equal bins; "
                         "choose L with (L + 1) % bins == 0")
    levels = [float(v) for v in levels]
    out = torch.as_tensor(out).reshape(-1, len(COLUMNS)).double()
    keep = ~torch.isnan(out).any(1)
    res = dict(dropped=int((~keep).sum()), L=L, bins=bins, levels=levels, weighted=bool(weighted))
    res.update(_table(out[keep], L, bins, levels, weighted))
    if khat is not None:
        from .ops import psis_khat_threshold
        thr = psis_khat_threshold(L)
        k = torch.as_tensor(khat).reshape(-1).to(out.device)
        if k.numel() != out.shape[0]:
            raise ValueError("summarise: khat must hold one value per row of out")
        res["khat_threshold"] = thr
        res["reliable"] = _table(out[keep & (k < thr)], L, bins, levels, weighted)
    return res


def format_table(summary):
    """The coverage table of a summary as text: one row per statistic, one column per level."""
    lines = []
    for title, tab in (("all voxels", summary), ("khat below threshold", summary.get("reliable"))):
        if tab is None:
            continue
        lines.append(f"{title}: n = {tab['n']}")
        lines.append(f"  {'statistic':<10}{'chi2':>10}{'p':>10}" + "".join(f"{100 * lev:>9.0f}%" for lev in summary["levels"]))
        for name in COLUMNS:
            s = tab["stats"][name]
            lines.append(f"  {name:<10}{s['chi2']:>10.1f}{s['p_value']:>10.3g}" + "".join(f"{c:>10.3f}" for c in s["coverage"]))
    return "\n".join(lines)
