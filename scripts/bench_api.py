#!/usr/bin/env python3
"""Times every data-path entry point of the C ABI on 1 M voxels (HIP events on the launch stream) and
prints one JSON object: ms per call and the algorithmic GB/s each call moves.  Arguments: name substrings to time
only the matching calls (default: all).  The headline number is
bench.py's; this table backs the per-kernel rows of DESIGN.md."""
import configparser
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from qbold_vi_amd.init import init_encoder_weights  # noqa: E402
from qbold_vi_amd.ops import Context, EncoderWeights, TrainState  # noqa: E402


def only_names():
    return [a for a in sys.argv[1:] if not a.startswith("-")]   # name substrings: time only the matching calls


def main():
    cfg = configparser.ConfigParser()
    cfg.read(os.path.join(ROOT, "config"))
    params = dict(cfg["DEFAULT"])
    ctx = Context(params, True, True)
    T, n = ctx.T, 1 << 20
    w = init_encoder_weights(T=T, U=60, L=2, channelwise_gating=True, resid_init_std=0.05, seed=1, spatial_taps=9)
    ew = EncoderWeights(ctx, T, 60, 2, True, -3.0, spatial_taps=9).set_from_arrays(w)
    st = TrainState(ctx, ew)
    g = torch.Generator(device="cuda").manual_seed(0)
    y = torch.stack([torch.rand(n, generator=g, device="cuda") * 0.7 + 0.08,
                     torch.rand(n, generator=g, device="cuda") * 0.1 + 0.005], -1)
    x = ctx.signal_fwd(y)
    o1, q, sg = ctx.encoder_fwd(ew, x)
    ls = torch.log(sg)
    mask = torch.ones(n, device="cuda")
    z = ctx.normals(n, 1).reshape(n, 2)
    gs = torch.randn(n, T, device="cuda")
    y3 = torch.cat([y, y[:, :1]], -1).contiguous()
    B, X, Y, Z = 64, 32, 32, 16   # 1 M voxels as crops
    q5, m5 = q.reshape(B, X, Y, Z, 5), mask.reshape(B, X, Y, Z)
    x5 = x.reshape(B, X, Y, Z, T)
    gq0 = torch.zeros(n, 5, device="cuda")

    def fwd_train():
        st.forward(x, 2)

    def bwd_train():
        st.backward(2, gq0, gs, None)

    st.forward(x, 2)
    # per-voxel refinement at T = 11 and T = 24 (the same heads; a fixed sigma at T = 24), and the composed loop it
    # replaces: per step qbold_elbo_bwd(S, K = 70) and qbold_adamw_step on the N x 5 heads with weight decay 0
    ctx24 = Context(dict(params, tau_start="-0.028", tau_end="0.065", tau_step="0.004"), True, True)
    x24 = ctx24.signal_fwd(y)
    sg24 = torch.full((n, ctx24.T), 0.05, device="cuda")

    def composed(c, xx, lsx, steps, S):
        from qbold_vi_amd.ops import _ptr, _stream
        qq = q.clone()
        m1, m2 = torch.zeros_like(qq), torch.zeros_like(qq)
        for j in range(steps):
            _, gq, _, _ = c.elbo_bwd(xx, mask, qq, o1, lsx, S, 70, seed=1 + j)
            c.lib.qbold_adamw_step(c.handle, _ptr(qq), _ptr(gq), _ptr(m1), _ptr(m2), 5 * n, 0.05, 0.9, 0.999, 1e-8,
                                   0.0, j + 1, _stream())
        return qq

    def rbytes(TT):   # x, sigma, q, prior, mask in; q out
        return 4 * (2 * TT + 10) + 4 + 20

    # refinement under the TV prior (w = 5, optimal.yaml's smoothness_weight) on 1 M voxels as a 16 x 128 x 64 x 8
    # volume and on make_synthetic_volumes.py's 4 x 96 x 96 x 8, and the loop a user composes for it today: per step
    # qbold_elbo_bwd(S, K = 70) + qbold_smoothness(weight = w, g_q) + qbold_adamw_step on the N x 5 heads
    def volume(B, X, Y, Z):
        nv = B * X * Y * Z
        r = lambda t: t[:nv].reshape(B, X, Y, Z, t.shape[-1])   # noqa: E731
        return r(x), mask[:nv].reshape(B, X, Y, Z), r(q), r(o1), r(sg), r(ls)
    vol1m, vol96 = volume(16, 128, 64, 8), volume(4, 96, 96, 8)

    def spatial(v, steps, S, w=5.0):
        xx, mm, qq, pp, ss, _ = v
        return ctx.refine_posterior_spatial(xx, mm, qq, pp, ss, w, steps=steps, S=S)

    def composed_tv(v, steps, S, w=5.0):
        from qbold_vi_amd.ops import _ptr, _stream
        xx, mm, qv, pp, _, lsx = v
        nv = mm.numel()
        qq = qv.clone()
        m1, m2 = torch.zeros_like(qq), torch.zeros_like(qq)
        for j in range(steps):
            _, gq, _, _ = ctx.elbo_bwd(xx.reshape(nv, T), mm.reshape(nv), qq.reshape(nv, 5), pp.reshape(nv, 5),
                                       lsx.reshape(nv, T), S, 70, seed=1 + j)
            ctx.smoothness(qq, mm, weight=w, g_q=gq)
            ctx.lib.qbold_adamw_step(ctx.handle, _ptr(qq), _ptr(gq), _ptr(m1), _ptr(m2), 5 * nv, 0.05, 0.9, 0.999,
                                     1e-8, 0.0, j + 1, _stream())
        return qq

    def sbytes(TT):   # per step: x, sigma, heads, moments, loss, prior, mask, neighbours' heads 0, 2 and masks in; 68 out
        return 4 * (2 * TT + 21) + 68
    # PSIS diagnostics on 262,144 voxels (at 1 M voxels the per-draw rows of K = 256 take 4 GiB): the row dump, the
    # Pareto fit on ready rows, both, and log_evidence on the same voxels and draws beside them
    nq = 1 << 18
    xq, mq, qq_, pq, sq = x[:nq], mask[:nq], q[:nq], o1[:nq], sg[:nq]
    rows = {}

    def ready(K):   # the rows of K draws, dumped once
        if K not in rows:
            rows[K] = ctx.log_evidence_draws(xq, mq, qq_, pq, sq, K, seed=1, want_theta=True)
        return rows[K]

    def draws_psis(K):
        lw, th = ctx.log_evidence_draws(xq, mq, qq_, pq, sq, K, seed=1, want_theta=True)
        return ctx.psis(lw, th, mq)

    def psis_rows(K):
        f = nq / n    # the table's GB/s are per n voxels
        return {
            f"log_evidence(K={K},262144)": (lambda: ctx.log_evidence(xq, mq, qq_, pq, sq, K, seed=1, want_means=True),
                                            (8 * T + 64) * f),
            f"log_evidence_draws(K={K},262144)": (lambda: ctx.log_evidence_draws(xq, mq, qq_, pq, sq, K, seed=1,
                                                                                 want_theta=True),
                                                  (8 * T + 44 + 16 * K) * f),
            f"psis(K={K},262144)": (lambda: ctx.psis(*ready(K), mq), (16 * K + 32) * f),
            f"log_evidence_draws+psis(K={K},262144)": (lambda: draws_psis(K), (8 * T + 76 + 32 * K) * f),
            # log_w, theta and mask in; stats (48 B), three quantiles per column (36 B) and row_out (8 B) out
            # (scripts/bench_summary.py has the torch composition beside it, without a mask: 16 K + 92)
            f"draw_summary(K={K},262144)": (lambda: ctx.draw_summary(*ready(K)[::-1], mq), (16 * K + 4 + 92) * f),
        }
    # calibration against a known truth at L = 255 draws: the kernel regenerates the draws (28 bytes in, 24 out per voxel,
    # 4 L more with weights), and beside it the path it replaces: the rows of log_evidence_draws (16 L bytes per voxel
    # through HBM) compared in torch
    cal_rows = {}

    def cal_lw(L):   # the log-weights of L draws, dumped once
        if L not in cal_rows:
            cal_rows[L] = ctx.log_evidence_draws(x, mask, q, o1, sg, L, seed=1)[0]
        return cal_rows[L]

    def composed_ranks(L):
        _, th = ctx.log_evidence_draws(x, mask, q, o1, sg, L, seed=1, want_theta=True)
        d = torch.stack([th[..., 0], th[..., 1], th[..., 0] * th[..., 1]], -1)
        t = torch.stack([y[:, 0], y[:, 1], y[:, 0] * y[:, 1]], -1)[:, None, :]
        return (2 * (d < t).sum(1) + (d == t).sum(1)).float() / (2 * L)
    calls = {
        # name: (callable, algorithmic bytes per voxel)
        "calibration(L=255)": (lambda: ctx.calibration(y, q, mask, L=255, seed=1), 28 + 24),
        "calibration(L=255,log_w)": (lambda: ctx.calibration(y, q, mask, L=255, log_w=cal_lw(255), seed=1),
                                     28 + 24 + 4 * 255),
        "log_evidence_draws+torch_ranks(L=255)": (lambda: composed_ranks(255), 8 * T + 44 + 2 * 16 * 255),
        "signal_fwd": (lambda: ctx.signal_fwd(y), 8 + 4 * T),
        "signal_bwd": (lambda: ctx.signal_bwd(y, gs), 8 + 4 * T + 8),
        "signal_fwd_ex(hct)": (lambda: ctx.signal_fwd_ex(y, mask * 0.34), 12 + 4 * T),
        "normalise": (lambda: ctx.normalise(x), 8 * T),
        "encoder_fwd(stream 1)": (lambda: ctx.encoder_fwd(ew, x, want=("out1",)), 4 * T + 20),
        "encoder_fwd(stream 2 + sigma)": (lambda: ctx.encoder_fwd(ew, x, want=("out2", "sigma")), 8 * T + 20),
        "reparam": (lambda: ctx.reparam(q, z), 20 + 8 + 8),
        "logit_mvn_nlogp": (lambda: ctx.logit_mvn_nlogp(y, q), 8 + 20 + 4),
        "posterior_moments(20 draws)": (lambda: ctx.posterior_moments(q, 20, seed=1), 20 + 24),
        "posterior_moments(200 draws)": (lambda: ctx.posterior_moments(q, 200, seed=1), 20 + 24),
        "kl_fwd(K=70)": (lambda: ctx.kl_fwd(q, o1, K=70, seed=1), 44),
        "kl_closed": (lambda: ctx.kl_closed(q, o1), 44),
        "kl_diag(+grad)": (lambda: ctx.kl_diag(q, o1, mask, g_q=gq0), 44 + 40),
        "elbo_fwd(S=32,K=70)": (lambda: ctx.elbo_fwd(x, mask, q, o1, sg, 32, 70, seed=1), 8 * T + 52),
        "elbo_bwd(S=1,K=70)": (lambda: ctx.elbo_bwd(x, mask, q, o1, ls, 1, 70, seed=1), 12 * T + 72),
        # gradient of the importance-weighted bound (DReG) against the ELBO backward; bytes: x, log sigma, q, prior,
        # mask in, g_q, g_log_sigma out
        "elbo_bwd(S=8,K=8)": (lambda: ctx.elbo_bwd(x, mask, q, o1, ls, 8, 8, seed=1), 12 * T + 72),
        "log_evidence_bwd(T=11,K=1)": (lambda: ctx.log_evidence_bwd(x, mask, q, o1, ls, 1, seed=1), 12 * T + 64),
        "log_evidence_bwd(T=11,K=8)": (lambda: ctx.log_evidence_bwd(x, mask, q, o1, ls, 8, seed=1), 12 * T + 64),
        "log_evidence_bwd(T=11,K=32)": (lambda: ctx.log_evidence_bwd(x, mask, q, o1, ls, 32, seed=1), 12 * T + 64),
        "elbo_bwd(T=24,S=1,K=70)": (lambda: ctx24.elbo_bwd(x24, mask, q, o1, torch.log(sg24), 1, 70, seed=1),
                                    12 * 24 + 72),
        "log_evidence_bwd(T=24,K=1)": (lambda: ctx24.log_evidence_bwd(x24, mask, q, o1, torch.log(sg24), 1, seed=1),
                                       12 * 24 + 64),
        "log_evidence_bwd(T=24,K=8)": (lambda: ctx24.log_evidence_bwd(x24, mask, q, o1, torch.log(sg24), 8, seed=1),
                                       12 * 24 + 64),
        "log_evidence_bwd(T=24,K=32)": (lambda: ctx24.log_evidence_bwd(x24, mask, q, o1, torch.log(sg24), 32,
                                                                       seed=1), 12 * 24 + 64),
        # importance-weighted evidence against the ELBO kernel on the same draws' forward-model work (S = K = K_iw)
        "log_evidence(K=64)": (lambda: ctx.log_evidence(x, mask, q, o1, sg, 64, seed=1), 8 * T + 52),
        "elbo_fwd(S=64,K=64)": (lambda: ctx.elbo_fwd(x, mask, q, o1, sg, 64, 64, seed=1), 8 * T + 52),
        "log_evidence(K=1024)": (lambda: ctx.log_evidence(x, mask, q, o1, sg, 1024, seed=1), 8 * T + 52),
        "elbo_fwd(S=1024,K=1024)": (lambda: ctx.elbo_fwd(x, mask, q, o1, sg, 1024, 1024, seed=1), 8 * T + 52),
        "refine_posterior(T=11,steps=200,S=1)": (lambda: ctx.refine_posterior(x, mask, q, o1, sg, 200, 1), rbytes(T)),
        "refine_posterior(T=11,steps=100,S=4)": (lambda: ctx.refine_posterior(x, mask, q, o1, sg, 100, 4), rbytes(T)),
        "refine_posterior(T=24,steps=200,S=1)": (lambda: ctx24.refine_posterior(x24, mask, q, o1, sg24, 200, 1),
                                                 rbytes(24)),
        "refine_posterior(T=24,steps=100,S=4)": (lambda: ctx24.refine_posterior(x24, mask, q, o1, sg24, 100, 4),
                                                 rbytes(24)),
        "composed_loop(T=11,steps=200,S=1,K=70)": (lambda: composed(ctx, x, ls, 200, 1), 0),
        "composed_loop(T=11,steps=100,S=4,K=70)": (lambda: composed(ctx, x, ls, 100, 4), 0),
        "composed_loop(T=24,steps=200,S=1,K=70)": (lambda: composed(ctx24, x24, torch.log(sg24), 200, 1), 0),
        "composed_loop(T=24,steps=100,S=4,K=70)": (lambda: composed(ctx24, x24, torch.log(sg24), 100, 4), 0),
        "refine_posterior_spatial(T=11,steps=200,S=1,w=5,16x128x64x8)": (lambda: spatial(vol1m, 200, 1),
                                                                         200 * sbytes(T)),
        "refine_posterior_spatial(T=11,steps=200,S=1,w=0,16x128x64x8)": (lambda: spatial(vol1m, 200, 1, 0.0),
                                                                         200 * sbytes(T)),
        "composed_loop_tv(T=11,steps=200,S=1,K=70,w=5,16x128x64x8)": (lambda: composed_tv(vol1m, 200, 1), 0),
        "refine_posterior_spatial(T=11,steps=200,S=1,w=5,4x96x96x8)": (lambda: spatial(vol96, 200, 1),
                                                                       200 * sbytes(T) * 294912 / n),
        "refine_posterior(T=11,steps=200,S=1,4x96x96x8)": (
            lambda: ctx.refine_posterior(vol96[0].reshape(-1, T), vol96[1].reshape(-1), vol96[2].reshape(-1, 5),
                                         vol96[3].reshape(-1, 5), vol96[4].reshape(-1, T), 200, 1),
            rbytes(T) * 294912 / n),
        "composed_loop_tv(T=11,steps=200,S=1,K=70,w=5,4x96x96x8)": (lambda: composed_tv(vol96, 200, 1), 0),
        "posterior_grid(defaults)": (lambda: ctx.posterior_grid(x, mask, o1, sg, q=q), 8 * T + 48 + 68),
        "posterior_grid(q=None,gh=0)": (lambda: ctx.posterior_grid(x, mask, o1, sg, gh=0), 8 * T + 28 + 68),
        "log_evidence(K=256)": (lambda: ctx.log_evidence(x, mask, q, o1, sg, 256, seed=1), 8 * T + 52),
        "posterior_predictive(L=256)": (lambda: ctx.posterior_predictive(x, mask, q, sg, 256), 8 * T + 24 + 24),
        "posterior_predictive(L=256,curves)": (lambda: ctx.posterior_predictive(x, mask, q, sg, 256, want_curves=True),
                                               8 * T + 24 + 24 + 12 * T),
        # PSIS leave-one-out: inputs and out, plus the rows through the three stages (rows kernel: 4 K (2 T + 1) out and
        # 4 K T read back; qbold_psis: 4 K (T + 1) in and out; closing kernel: 4 K (2 T + 1) in); 1 GiB workspace chunks
        "loo(K=100)": (lambda: ctx.loo(x, mask, q, o1, sg, 100, seed=1), 8 * T + 68 + 4 * 100 * (7 * T + 4)),
        "vi_fwd(S=32,K=70)": (lambda: ctx.vi_fwd(ew, x, mask, o1, 32, 70, seed=1), 4 * T + 52),
        "synth_loss_bwd": (lambda: st.synth_loss_bwd(y3, o1), 12 + 20 + 24),
        "wls_fit": (lambda: ctx.wls_fit(x), 4 * T + 12),
        "smoothness(+grad)": (lambda: ctx.smoothness(q5, m5, weight=5.0, g_q=gq0), 24 + 40),
        "encoder_train_fwd(stream 2)": (fwd_train, None),
        "encoder_train_bwd(stream 2)": (bwd_train, None),
        "encoder_spatial_fwd(3x3x1)": (lambda: st.forward_spatial(x5), None),
        "adamw_step(146k params)": (lambda: st.adamw(1e-3, 1e-4), None),
    }
    calls.update(psis_rows(64))
    calls.update(psis_rows(256))
    # Laplace posteriors (Levenberg-Marquardt MAP + curvature) at the defaults from the prior mean, on noisy synthetic
    # voxels (noise sd 0.02 of the spin-echo image, sigma = 0.02, one prior for all: OEF 0.4, DBV 0.03, sd 0.6 logits),
    # beside the only other route to a MAP and a covariance on every T, posterior_grid at its defaults on the same
    # voxels.  Bytes: x, sigma, prior, mask in; q_out, out (and the grid's out) back.
    lap_info = {}

    def laplace_rows(name, p):
        c = Context(p, True, True)
        xs = c.signal_fwd(y)
        xs = xs + 0.02 * xs[:, c.se_idx:c.se_idx + 1] * torch.randn(xs.shape, generator=g, device="cuda")
        sgs = torch.full((n, c.T), 0.02, device="cuda")
        pl = torch.tensor([-0.2007, 0.1634, -1.7750, 0.1634, 0.0], device="cuda").repeat(n, 1)

        def lap():
            q_l, o_l = c.laplace_posterior(xs, mask, pl, sgs)
            lap_info[f"laplace(T={name})"] = o_l
            return q_l
        return {f"laplace(T={name})": (lap, 8 * c.T + 24 + 20 + 60),
                f"posterior_grid(T={name},q=None)": (lambda: c.posterior_grid(xs, mask, pl, sgs), 8 * c.T + 24 + 68)}
    if not only_names() or any("laplace" in o or "posterior_grid(T=" in o for o in only_names()):
        calls.update(laplace_rows("11", params))
        calls.update(laplace_rows("24", dict(params, tau_start="-0.028", tau_end="0.065", tau_step="0.004")))
        calls.update(laplace_rows("33", dict(params, tau_start="-0.008", tau_end="0.057", tau_step="0.002")))
        calls.update(laplace_rows("64", dict(params, tau_start="-0.008", tau_end="0.0555", tau_step="0.001")))
    # refinement on any tau grid (the run-time-T kernels): 33 and 64 taus (the Laplace rows' protocols) as the T = 24
    # rows above have it -- the T = 11 encoder's heads, sigma = 0.05 -- beside the composed loop on the same protocol,
    # and kernel="generic" at 11 / 24 taus beside the specialised kernels' rows above
    def refine_anyt_rows(name, p):
        c = Context(p, True, True)
        xs = c.signal_fwd(y)
        sgs = torch.full((n, c.T), 0.05, device="cuda")
        lss = torch.log(sgs)
        return {
            f"refine_posterior(T={name},steps=200,S=1)": (lambda: c.refine_posterior(xs, mask, q, o1, sgs, 200, 1),
                                                          rbytes(c.T)),
            f"refine_posterior(T={name},steps=100,S=4)": (lambda: c.refine_posterior(xs, mask, q, o1, sgs, 100, 4),
                                                          rbytes(c.T)),
            f"composed_loop(T={name},steps=200,S=1,K=70)": (lambda: composed(c, xs, lss, 200, 1), 0),
            f"refine_posterior_spatial(T={name},steps=200,S=1,w=5,16x128x64x8)": (
                lambda: c.refine_posterior_spatial(xs.reshape(16, 128, 64, 8, c.T), vol1m[1], vol1m[2], vol1m[3],
                                                   sgs.reshape(16, 128, 64, 8, c.T), 5.0, steps=200, S=1),
                200 * sbytes(c.T)),
        }
    if not only_names() or any("T=33" in o or "T=64" in o or "generic" in o for o in only_names()):
        calls.update(refine_anyt_rows("33", dict(params, tau_start="-0.008", tau_end="0.057", tau_step="0.002")))
        calls.update(refine_anyt_rows("64", dict(params, tau_start="-0.008", tau_end="0.0555", tau_step="0.001")))
        calls.update({
            "refine_posterior(T=11,steps=200,S=1,generic)": (
                lambda: ctx.refine_posterior(x, mask, q, o1, sg, 200, 1, kernel="generic"), rbytes(T)),
            "refine_posterior(T=11,steps=100,S=4,generic)": (
                lambda: ctx.refine_posterior(x, mask, q, o1, sg, 100, 4, kernel="generic"), rbytes(T)),
            "refine_posterior(T=24,steps=200,S=1,generic)": (
                lambda: ctx24.refine_posterior(x24, mask, q, o1, sg24, 200, 1, kernel="generic"), rbytes(24)),
            "refine_posterior(T=24,steps=100,S=4,generic)": (
                lambda: ctx24.refine_posterior(x24, mask, q, o1, sg24, 100, 4, kernel="generic"), rbytes(24)),
            "refine_posterior_spatial(T=11,steps=200,S=1,w=5,16x128x64x8,generic)": (
                lambda: ctx.refine_posterior_spatial(*vol1m[:5], 5.0, steps=200, S=1, kernel="generic"),
                200 * sbytes(T)),
        })
    # head gradients of the importance-weighted bound on any tau grid (iw_bwd_generic_kernel): 33 and 64 taus (the
    # Laplace rows' protocols, the T = 11 encoder's heads, sigma = 0.05) at K = 8 / 32 (one lane per voxel) and 64
    # (four), and kernel="generic" at 11 / 24 taus beside the specialised kernels' log_evidence_bwd rows above
    def iw_bwd_anyt_rows(name, p):
        c = Context(p, True, True)
        xs = c.signal_fwd(y)
        lss = torch.log(torch.full((n, c.T), 0.05, device="cuda"))
        return {f"log_evidence_bwd(T={name},K={K})": (
            lambda K=K: c.log_evidence_bwd(xs, mask, q, o1, lss, K, seed=1), 12 * c.T + 64) for K in (8, 32, 64)}
    if not only_names() or any("log_evidence_bwd" in o or "generic" in o for o in only_names()):
        calls.update(iw_bwd_anyt_rows("33", dict(params, tau_start="-0.008", tau_end="0.057", tau_step="0.002")))
        calls.update(iw_bwd_anyt_rows("64", dict(params, tau_start="-0.008", tau_end="0.0555", tau_step="0.001")))
        for K in (8, 32):
            calls[f"log_evidence_bwd(T=11,K={K},generic)"] = (
                lambda K=K: ctx.log_evidence_bwd(x, mask, q, o1, ls, K, seed=1, kernel="generic"), 12 * T + 64)
            calls[f"log_evidence_bwd(T=24,K={K},generic)"] = (
                lambda K=K: ctx24.log_evidence_bwd(x24, mask, q, o1, torch.log(sg24), K, seed=1, kernel="generic"),
                12 * 24 + 64)
    only = only_names()
    out = {}
    for name, (fn, bpv) in calls.items():
        if only and not any(o in name for o in only):
            continue
        import time
        t0 = time.perf_counter()   # clock ramp: ~20 ms of load before an idle MI355X runs at sustained clocks
        while time.perf_counter() - t0 < 0.1:
            fn()
            torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 10
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        out[name] = {"ms": round(ms, 4)}
        if bpv:
            out[name]["algorithmic_GBps"] = round(bpv * n / ms / 1e6, 1)
        if name in lap_info:   # what the timed call did: iterations per voxel, the share that converged
            o_l = lap_info[name]
            out[name]["mean_iterations"] = round(o_l[:, 13].mean().item(), 3)
            out[name]["max_iterations"] = int(o_l[:, 13].max().item())
            out[name]["converged"] = round(((o_l[:, 14].int() & 1) == 0).float().mean().item(), 6)
    print(json.dumps({"voxels": n, "T": T, "calls": out}, indent=1))


if __name__ == "__main__":
    main()
