#!/usr/bin/env python3
"""Times qbold_draw_summary (HIP events on the launch stream, warm-up, median of repeats) on 262,144 rows of the
importance draws, C = 3, P = 3, K = 64 / 256 / 1024, beside what a user composes in torch for the quantiles alone on
the same device and rows (softmax + sort + gather + cumsum + searchsorted per column) and beside qbold_psis on the same
rows; then the three launches of FineTuner.credible_intervals (log_evidence_draws, psis with weights, draw_summary) on
1 M voxels at 11 taus and K = 256 in that method's chunks.  Prints one JSON object (ms).  MEASUREMENTS.md section 36."""
import configparser
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from qbold_vi_amd.init import init_encoder_weights  # noqa: E402
from qbold_vi_amd.ops import Context, EncoderWeights  # noqa: E402

LEVELS = (0.025, 0.5, 0.975)


def timed(fn, warmup=2, repeats=7):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def torch_quantiles(lw, theta, levels):
    """The composition: the weighted inverse-ECDF quantiles of every column, [N, C, P]."""
    w = torch.softmax(lw, 1)
    p = torch.tensor(levels, device=lw.device).expand(lw.shape[0], len(levels)).contiguous()
    out = []
    for c in range(theta.shape[2]):
        vals, idx = torch.sort(theta[..., c], dim=1, stable=True)
        W = torch.cumsum(torch.gather(w, 1, idx), 1)
        r = torch.searchsorted(W, p).clamp_(max=lw.shape[1] - 1)
        out.append(torch.gather(vals, 1, r))
    return torch.stack(out, 1)


def main():
    cfg = configparser.ConfigParser()
    cfg.read(os.path.join(ROOT, "config"))
    ctx = Context(dict(cfg["DEFAULT"]), True, True)
    T, n, nq = ctx.T, 1 << 20, 1 << 18
    w = init_encoder_weights(T=T, U=60, L=2, channelwise_gating=True, resid_init_std=0.05, seed=1, spatial_taps=9)
    ew = EncoderWeights(ctx, T, 60, 2, True, -3.0, spatial_taps=9).set_from_arrays(w)
    g = torch.Generator(device="cuda").manual_seed(0)
    y = torch.stack([torch.rand(n, generator=g, device="cuda") * 0.7 + 0.08,
                     torch.rand(n, generator=g, device="cuda") * 0.1 + 0.005], -1)
    x = ctx.signal_fwd(y)
    prior, q, sg = ctx.encoder_fwd(ew, x)
    mask = torch.ones(n, device="cuda")
    res = {}
    for K in (64, 256, 1024):
        lw, th = ctx.log_evidence_draws(x[:nq], mask[:nq], q[:nq], prior[:nq], sg[:nq], K, seed=1, want_theta=True)
        res[f"draw_summary(K={K},262144)"] = timed(lambda: ctx.draw_summary(th, lw, probs=LEVELS))
        res[f"draw_summary+corr(K={K},262144)"] = timed(lambda: ctx.draw_summary(th, lw, probs=LEVELS, want_corr=True))
        res[f"torch_quantiles(K={K},262144)"] = timed(lambda: torch_quantiles(lw, th, LEVELS))
        res[f"psis(K={K},262144)"] = timed(lambda: ctx.psis(lw, None, None))
        # the two compute the same quantiles wherever no W_r lies within float32 rounding of a level
        same = (ctx.draw_summary(th, lw, probs=LEVELS)[1] == torch_quantiles(lw, th, LEVELS)).float().mean().item()
        res[f"equal_quantile_share(K={K})"] = round(same, 6)
        del lw, th
    # credible_intervals' launches on 1 M voxels, K = 256, in its chunks of 65,535 voxels
    K = 256
    chunk = max((256 << 20) // (16 * K) - 1, 1)
    spans = [(a, min(a + chunk, n)) for a in range(0, n, chunk)]

    def draws():
        return [ctx.log_evidence_draws(x[a:b], mask[a:b], q[a:b], prior[a:b], sg[a:b], K, seed=1, voxel0=a,
                                       want_theta=True) for a, b in spans]
    rows = draws()

    def smooth():
        return [ctx.psis(lw, None, mask[a:b], want_weights=True)[2] for (lw, _), (a, b) in zip(rows, spans)]
    wts = smooth()

    def summarise():
        for (_, th), wt, (a, b) in zip(rows, wts, spans):
            ctx.draw_summary(th, wt, mask[a:b], probs=LEVELS, want_corr=True)

    def whole():
        for a, b in spans:
            lw, th = ctx.log_evidence_draws(x[a:b], mask[a:b], q[a:b], prior[a:b], sg[a:b], K, seed=1, voxel0=a,
                                            want_theta=True)
            wt = ctx.psis(lw, None, mask[a:b], want_weights=True)[2]
            ctx.draw_summary(th, wt, mask[a:b], probs=LEVELS, want_corr=True)
    res["credible_intervals(K=256,1M): log_evidence_draws"] = timed(draws)
    res["credible_intervals(K=256,1M): psis(want_weights)"] = timed(smooth)
    res["credible_intervals(K=256,1M): draw_summary"] = timed(summarise)
    res["credible_intervals(K=256,1M): the three launches per chunk"] = timed(whole)
    res["chunks"] = len(spans)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
