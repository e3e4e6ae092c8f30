// iw_bwd_kernels.hip -- gradient of the importance-weighted bound (Burda et al. 2016) with respect to the encoder's head
// outputs, for fine-tuning on it: the backward of qbold_log_evidence_fwd (iw_kernels.hip), on the same draws.
//
// Per voxel, K normals eps_k (explicit, or Philox stream 6: exactly qbold_log_evidence_fwd's draws), u_k = mu + L eps_k,
//   log w_k = -nll(x | u_k; sigma) - (log q(u_k) - log p(u_k)),   w~_k = softmax_k(log w),   l = -(logsumexp log w - log K)
// and the outputs, unnormalised by sum(m) as qbold_elbo_bwd's are:
//   g_log_sigma[t] = m sum_k w~_k d nll_k / d log sigma_t                              (the exact gradient for fixed eps)
//   g_q            = m sum_k w~_k^2 (d nll_k / du + d (log q - log p)_k / du |q held) du_k / dq_raw
// -- the second the doubly-reparameterised gradient (DReG, Tucker et al. 2019) of the bound for the inference network's
// outputs: q is held inside log q, as in the reference's ELBO (model.py:596), and the squared normalised weights replace
// the plain IWAE weights, whose gradient signal-to-noise falls with K (Rainforth et al. 2018).  At K = 1 it is
// qbold_elbo_bwd's gradient of m nll + KL with the KL drawn at the likelihood's draw.
//
// Per draw, the likelihood-gradient passes 1 and 2 of elbo_bwd_kernel (its signal slopes are signal_grad.h's;
// Gaussian or Student-t, linear or log data, either normalisation) and the KL draw's value and gradient: the whitened
// form of iw_kernels.hip where the logit clip does not bind, elbo_bwd_kernel's general clipped-logit form (the clip
// passes gradient) where it does.  The check is made per draw, so explicit normals equal to the Philox stream's give
// the same bits, and a voxel's bits do not depend on its wave's other voxels.
//
// The draws fold into a streaming log-sum-exp (IwAcc's): relative to a running max M, sum e^{lw-M} and sum e^{2(lw-M)},
// the five DReG sums under e^{2(lw-M)} (the u-gradient and its products with eps for the three entries of L) and the T
// sigma sums under e^{lw-M}; a new max rescales them all.  One pass over the draws (a two-pass form would run every
// draw's likelihood twice).  The chain to the raw heads runs once per voxel.
//
// Lane mapping by K, as elbo_bwd_kernel's by S: one lane per voxel up to K = 32 (the four-lane mapping repeats the
// voxel's loads and preparation four times and leaves lanes idle at small K), four lanes splitting the Philox calls
// (call g -> draws 4 g .. 4 g + 3, lane group g & 3) for larger K, their partial accumulators merged in a fixed order.  Draws
// are keyed by (seed, voxel0 + v, draw), never by lane; fixed-order double sums, no atomics: a voxel's outputs are the
// same bits at any batch position, under any sharding by voxel0 and run to run.
//
// iw_bwd_kernel<T, SE, LPV> is specialised for the reference's 11 / 24 taus (qbold_log_evidence_bwd);
// iw_bwd_generic_kernel<LPV>, further down, reads T and the spin-echo index at run time (qbold_log_evidence_bwd_anyt).
#include <cmath>

#include "elbo_core.h"
#include "qbold_ctx.h"
#include "signal_grad.h"

// K <= QB_IW_BWD_LPV1_MAX_K: one lane per voxel; larger K: four.  Measured on 1 M voxels (MEASUREMENTS.md section 14):
// one lane is 3.3x faster at K = 1, 2.2x (T = 11) / 2.1x (T = 24) at K = 8 and 8 % / 6 % at K = 32; beyond 32 the
// four-lane mapping, the forward's, keeps small batches busy.
#ifndef QB_IW_BWD_LPV1_MAX_K
#define QB_IW_BWD_LPV1_MAX_K 32
#endif

namespace qb {
int elbo_grid(const qbold_ctx* ctx);   // elbo_kernels.hip
bool elbo_fast_path(const qbold_ctx* ctx);
}

namespace {

constexpr int kBlock = 256;

// The whitened log q - log p of iw_kernels.hip (make_iw_kl): d + M z is a draw's residual under the prior.
struct IwKl {
    float d0, d1, m00, m10, m11;
    float cst;   // (s_o + s_d)_p - (s_o + s_d)_q
};
__device__ __forceinline__ IwKl make_iw_kl(const qb::LogitMvn& q, const qb::LogitMvn& p) {
    IwKl k;
    const float dmu_o = q.mu_o - p.mu_o, dmu_d = q.mu_d - p.mu_d;
    k.d0 = dmu_o * p.i_so;
    k.m00 = q.e_so * p.i_so;
    k.d1 = fmaf(dmu_d, p.i_sd, dmu_o * p.i_bl);
    k.m10 = fmaf(q.c, p.i_sd, q.e_so * p.i_bl);
    k.m11 = q.e_sd * p.i_sd;
    k.cst = (p.s_o + p.s_d) - (q.s_o + q.s_d);
    return k;
}

// One lane's streaming accumulators, relative to the running max M of its draws' log w.
template <int T>
struct IwGradAcc {
    float M, s1, s2, slw;
    float h[5];    // sum e^{2(lw-M)} (ha, ha z0, hb, hb z1, hb z0): the loss gradient in u and its products with eps
    float gs[T];   // sum e^{lw-M} d nll / d log sigma_t
    __device__ __forceinline__ void init() {
        M = -INFINITY;
        s1 = s2 = slw = 0.0f;
#pragma unroll
        for (int i = 0; i < 5; ++i) h[i] = 0.0f;
#pragma unroll
        for (int t = 0; t < T; ++t) gs[t] = 0.0f;
    }
};

// One draw: log w, folded into acc with its sigma and DReG terms.  m: the voxel's mask (log data: 0 scores nothing).
template <int T, int SE>
__device__ __forceinline__ void iw_bwd_draw(const qb::FwdLds* L, const QbDev& c, const qb::VoxelLik<T>& lik, float m,
                                            const qb::LogitMvn& qm, const qb::LogitMvn& pm, const IwKl& kl,
                                            float z0, float z1, IwGradAcc<T>& acc) {
    float a, b;
    qb::reparam_logits(qm, z0, z1, a, b);
    // log q - log p of the draw and its gradient in u, q held inside log q
    float dswr, ka, kb;
    if (fmaxf(fabsf(a), fabsf(b)) > QB_LOGIT_CLIP) {   // the clip binds: elbo_bwd_kernel's general KL loop
        const float l0 = qb::clampf_(a, -QB_LOGIT_CLIP, QB_LOGIT_CLIP);
        const float l1 = qb::clampf_(b, -QB_LOGIT_CLIP, QB_LOGIT_CLIP);
        const float rq0 = l0 - qm.mu_o, rq1 = l1 - qm.mu_d;
        const float rp0 = l0 - pm.mu_o, rp1 = l1 - pm.mu_d;
        const float wq0 = rq0 * qm.i_so, wq1 = fmaf(rq1, qm.i_sd, rq0 * qm.i_bl);
        const float wp0 = rp0 * pm.i_so, wp1 = fmaf(rp1, pm.i_sd, rp0 * pm.i_bl);
        dswr = fmaf(wp0, wp0, wp1 * wp1) - fmaf(wq0, wq0, wq1 * wq1);   // kl_swr_diff
        ka = (wp0 * pm.i_so + wp1 * pm.i_bl) - (wq0 * qm.i_so + wq1 * qm.i_bl);
        kb = wp1 * pm.i_sd - wq1 * qm.i_sd;
    } else {   // whitened: the residual under q is z itself, under the prior w = d + M z
        const float w0 = fmaf(kl.m00, z0, kl.d0);
        const float w1 = fmaf(kl.m11, z1, fmaf(kl.m10, z0, kl.d1));
        dswr = fmaf(w0, w0, w1 * w1) - fmaf(z0, z0, z1 * z1);          // iw_dswr
        ka = (w0 * pm.i_so + w1 * pm.i_bl) - (z0 * qm.i_so + z1 * qm.i_bl);
        kb = w1 * pm.i_sd - z1 * qm.i_sd;
    }
    const float sa = qb::sigmoidf_(a), sb = qb::sigmoidf_(b);
    const float oef = sa * QB_OEF_RANGE + QB_MIN_OEF;
    const float dbv = sb * QB_DBV_RANGE + QB_MIN_DBV;
    const qb::FwdFast fv = qb::fwd_fast(c, oef, dbv);
    // pass 1 of elbo_bwd_kernel: signals, residuals, NLL, d nll / d yhat, d nll / d log sigma
    float sig[T];
#pragma unroll
    for (int t = 0; t < T; ++t) sig[t] = qb::fwd_signal_fast(L, c, fv, t);
    const float inv_np = qb::rcpf_(qb::se_norm<T, SE>(c, sig));
    float sq = 0.0f, a1 = 0.0f;
    float gy[T], dls[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        float yp = sig[t] * inv_np, dyp = 1.0f;
        if (c.predict_log) {                      // model.py:547-549
            dyp = m > 0.0f ? qb::rcpf_(yp) : 0.0f;
            yp = m > 0.0f ? __logf(yp) : 0.0f;
        }
        const float r = (lik.yt[t] - yp) * lik.inv_s[t];
        float dr = r;
        if (c.use_student_t) {                    // model.py:557-559
            const float w = (c.st_df + 1.0f) * qb::rcpf_(fmaf(r, r, c.st_df));
            sq += (c.st_df + 1.0f) * log1pf(r * r * qb::rcpf_(c.st_df)) - 2.0f * c.st_const;
            dr = w * r;
        } else {
            sq = fmaf(r, r, sq);
        }
        dls[t] = 1.0f - dr * r;                   // d/d log sigma_t of log sigma_t + nll_t(r)
        gy[t] = -dr * lik.inv_s[t] * dyp;
        a1 = fmaf(gy[t], sig[t], a1);
    }
    a1 *= inv_np * inv_np;
    const float lw = -fmaf(0.5f, sq, lik.log_s_sum) - fmaf(0.5f, dswr, kl.cst);
    // the streaming log-sum-exp: rescale what is there to the new max, add this draw
    const float mn = fmaxf(acc.M, lw);
    const float r1 = qb::exp2f_((acc.M - mn) * QB_LOG2E);   // 0 on the lane's first draw
    const float e1 = qb::exp2f_((lw - mn) * QB_LOG2E);
    const float r2 = r1 * r1, e2 = e1 * e1;
    acc.M = mn;
    acc.s1 = fmaf(acc.s1, r1, e1);
    acc.s2 = fmaf(acc.s2, r2, e2);
    acc.slw += lw;
#pragma unroll
    for (int t = 0; t < T; ++t) acc.gs[t] = fmaf(acc.gs[t], r1, e1 * dls[t]);
    // pass 2 of elbo_bwd_kernel: chain through the normalisation and the forward model
    float g_oef = 0.0f, g_dbv = 0.0f;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        float gs = gy[t] * inv_np;
        if (SE >= 0) {
            if (t == SE) gs -= a1;
        } else if (c.multi_norm) {
            if (t >= c.se_idx - 1 && t <= c.se_idx + 1) gs -= a1 * (1.0f / 3.0f);
        } else if (t == c.se_idx) {
            gs -= a1;
        }
        const qb::FwdGrad fg = qb::fwd_signal_grad(L, c, fv, oef, dbv, t);
        g_oef = fmaf(gs, fg.ds_doef, g_oef);
        g_dbv = fmaf(gs, fg.ds_ddbv, g_dbv);
    }
    // -d log w / du with q held: the NLL's gradient through forward_transform plus the KL draw's
    const float ha = fmaf(g_oef * QB_OEF_RANGE, sa * (1.0f - sa), ka);
    const float hb = fmaf(g_dbv * QB_DBV_RANGE, sb * (1.0f - sb), kb);
    const float wa = e2 * ha, wb = e2 * hb;
    acc.h[0] = fmaf(acc.h[0], r2, wa);
    acc.h[1] = fmaf(acc.h[1], r2, wa * z0);
    acc.h[2] = fmaf(acc.h[2], r2, wb);
    acc.h[3] = fmaf(acc.h[3], r2, wb * z1);
    acc.h[4] = fmaf(acc.h[4], r2, wb * z0);
}

// Fixed-order double sums (iw_kernels.hip's): wave, block, then reduce_partials_kernel over the blocks.
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ void block_partials_d(double* red, double a, double b, double m,
                                                 double* __restrict__ partials) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    a = wave_sum_d(a);
    b = wave_sum_d(b);
    m = wave_sum_d(m);
    if (lane == 0) {
        red[3 * wave + 0] = a;
        red[3 * wave + 1] = b;
        red[3 * wave + 2] = m;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double s = 0.0;
        for (int w = 0; w < nw; ++w) s += red[3 * w + threadIdx.x];
        partials[3 * blockIdx.x + threadIdx.x] = s;
    }
}

// LPV lanes per voxel (1 or 4, see the head of the file).  Lane `part` of a voxel takes Philox calls part, part + LPV,
// ...; explicit normals z [N][K][2] are read at the same draw indices.
template <int T, int SE, int LPV>
__global__ __launch_bounds__(kBlock) void iw_bwd_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* __restrict__ q, const float* __restrict__ prior, const float* __restrict__ log_sigma,
    const float* __restrict__ z, int K, uint64_t seed, int64_t voxel0, float* __restrict__ g_q,
    float* __restrict__ g_ls, float* __restrict__ out, double* __restrict__ partials, int64_t N) {
    __shared__ qb::FwdLds L;
    __shared__ double red[3 * (kBlock / 64)];
    qb::fwd_lds_fill(&L, g_tab, false);
    __syncthreads();

    constexpr int kVoxPerBlock = kBlock / LPV, kVoxPerWave = 64 / LPV;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int part = LPV == 1 ? 0 : lane >> 4;
    auto voxel_sum = [](float v) { return LPV == 1 ? v : qb::voxel_sum(v); };
    double s_lp = 0.0, s_el = 0.0, s_m = 0.0;
    const int64_t ntile = (N + kVoxPerBlock - 1) / kVoxPerBlock;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t v = tile * kVoxPerBlock + wave * kVoxPerWave + (LPV == 1 ? lane : lane & 15);
        if (v >= N) continue;
        const float m = mask ? mask[v] : 1.0f;
        const bool in = m > 0.0f;   // false for m <= 0 and NaN
        if (!in && !out) {          // nothing to score: zero gradients (the voxel's lanes take this branch together)
            if (part == 0) {
#pragma unroll
                for (int i = 0; i < 5; ++i) g_q[v * 5 + i] = 0.0f;
            }
            if (part == (LPV == 1 ? 0 : 1)) {
#pragma unroll
                for (int t = 0; t < T; ++t) g_ls[v * T + t] = 0.0f;
            }
            continue;
        }
        float xv[T], lsv[T], qv[5], pv[5];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            xv[t] = x[v * T + t];
            lsv[t] = log_sigma[v * T + t];
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            qv[i] = q[v * 5 + i];
            pv[i] = prior[v * 5 + i];
        }
        qb::VoxelLik<T> lik;
        qb::prepare_lik<T, SE, true>(c, xv, lsv, m, lik);
        const qb::LogitMvn qm = qb::make_mvn(qv), pm = qb::make_mvn(pv);
        const IwKl kl = make_iw_kl(qm, pm);
        const uint64_t vox = (uint64_t)(voxel0 + v);
        const float* zv = z ? z + v * (int64_t)K * 2 : nullptr;
        IwGradAcc<T> acc;
        acc.init();
#pragma unroll 1
        for (int g = part; 4 * g < K; g += LPV) {
            const int cnt = K - 4 * g < 4 ? K - 4 * g : 4;
            qb::DrawQuad dq;
            if (!zv) dq.load(seed, vox, (uint32_t)g, qb::STREAM_IW);
#pragma unroll 1
            for (int d = 0; d < cnt; ++d) {
                float z0, z1;
                if (zv) {
                    z0 = zv[2 * (4 * g + d)];
                    z1 = zv[2 * (4 * g + d) + 1];
                } else {
                    dq.next(z0, z1);
                }
                iw_bwd_draw<T, SE>(&L, c, lik, m, qm, pm, kl, z0, z1, acc);
            }
        }
        // merge the voxel's lanes in a fixed order (LPV = 4): common max, rescaled sums
        float Mx = acc.M;
        if (LPV > 1) {
            Mx = fmaxf(Mx, __shfl_xor(Mx, 16, 64));
            Mx = fmaxf(Mx, __shfl_xor(Mx, 32, 64));   // finite: lane group 0 holds draw 0
        }
        const float f1 = LPV == 1 ? 1.0f : qb::exp2f_((acc.M - Mx) * QB_LOG2E);   // 0 for a lane without draws
        const float f2 = f1 * f1;
        const float s1 = voxel_sum(acc.s1 * f1), s2 = voxel_sum(acc.s2 * f2), slw = voxel_sum(acc.slw);
        float h[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) h[i] = voxel_sum(acc.h[i] * f2);
        const float inv1 = 1.0f / s1;
        const float inv2 = inv1 * inv1;
        if (part == 0) {
            // transform_std / transform_offdiag (model.py:288-294): s = 3 tanh(raw) - 1, c = tanh(raw) e^-2
            const float wq = m * inv2;   // a voxel outside the mask writes exact zeros (its draws may be NaN)
            g_q[v * 5 + 0] = in ? wq * h[0] : 0.0f;
            g_q[v * 5 + 1] = in ? wq * (h[1] * qm.e_so) * 3.0f * qb::sech2f_(qv[1]) : 0.0f;
            g_q[v * 5 + 2] = in ? wq * h[2] : 0.0f;
            g_q[v * 5 + 3] = in ? wq * (h[3] * qm.e_sd) * 3.0f * qb::sech2f_(qv[3]) : 0.0f;
            g_q[v * 5 + 4] = in ? wq * h[4] * 0.1353352832366127f * qb::sech2f_(qv[4]) : 0.0f;
            const float lp = Mx + (logf(s1) - logf((float)K));
            const float el = slw / (float)K;
            if (out) {
                out[3 * v + 0] = lp;
                out[3 * v + 1] = el;
                out[3 * v + 2] = (s1 * s1) / s2;
            }
            if (in) {
                s_lp += (double)m * -(double)lp;
                s_el += (double)m * -(double)el;
                s_m += (double)m;
            }
        }
        float gsum[T];
#pragma unroll
        for (int t = 0; t < T; ++t) gsum[t] = voxel_sum(acc.gs[t] * f1);
        if (part == (LPV == 1 ? 0 : 1)) {
            const float ws = m * inv1;
#pragma unroll
            for (int t = 0; t < T; ++t) g_ls[v * T + t] = in ? ws * gsum[t] : 0.0f;
        }
    }
    block_partials_d(red, s_lp, s_el, s_m, partials);
}

// ---- any number of taus (1 <= T <= QB_MAX_T) ------------------------------------------------------------------------
// The same function as iw_bwd_kernel with T and the spin-echo index read at run time, for elbo_fast_path
// configurations (full model, table mode, Gaussian likelihood, linear data; either normalisation; the spin echo on or
// off the grid).  Same Philox words, same draw-to-lane dealing for either LPV, the same streaming log-sum-exp and the
// same fixed-order merge; the likelihood gradient is regrouped as in elbo_bwd_generic_kernel / refine_kernels.hip's
// gen_draw_nll_grad, so the outputs differ from iw_bwd_kernel's by rounding.
//
// The shape is refine_generic_kernel's / laplace_kernel's: 128 threads, FwdLds plus per-thread rows [t][thread] in
// dynamic LDS (signal_grad.h's VoxColumns), blood_B read from LDS, no barrier once the table is filled.  Four rows'
// worth: the normalised data yt, 1 / sigma, and one row of pairs (gs, dl) = (the sigma sums, the last draw's
// d nll / d log sigma) -- sizeof(FwdLds) + 2,048 T bytes per block (T = 11: 28 KiB, T = 64: 134 KiB, one block per CU
// from T = 38).
//
// Per draw: the one or three window images give np; then ONE pass over t gathers sum r^2, sum gy sig, sum gy ds/doef,
// sum gy ds/ddbv and the window's slopes (T + 1 or T + 3 table lookups, no sig[T] / gy[T]) and leaves dl[t] in LDS.  The
// sigma sums are what the ELBO backward does not have: gs[t] <- gs[t] r1 + e1 dl[t] needs the draw's log w, which
// exists only after that pass.  So a draw's row waits in LDS with its two factors (IwGenAcc::pr1, pe1) and is folded
// into gs by the NEXT draw's pass, which reads and writes the pair at t anyway (one 8-byte read, one 8-byte write);
// the row of the lane's last draw is folded where the sums are read out.  The fmafs per t are iw_bwd_kernel's, in its
// order.  No second loop over t, no table lookups or exponentials for the sums.
//
// Traffic per voxel, read from the code: reads 4T (x) + 4T (log sigma) + 20 (q) + 20 (prior) + 4 (mask) (+ 8K with
// explicit normals), writes 4T (g_log_sigma) + 20 (g_q) (+ 12 with out): 12T + 64 (+ 12) B, 844 B at T = 64, the reads
// repeated by each of a voxel's four lanes at LPV = 4.  Far from the memory roof; whether vector issue or the LDS pipe
// sets its time has not been profiled (MEASUREMENTS.md section 31).
constexpr int kGenBlock = 128;
constexpr int kGenRows = 4;   // yt, 1 / sigma, and the float2 row (gs, dl)
static_assert(sizeof(qb::FwdLds) + sizeof(float) * kGenRows * QB_MAX_T * kGenBlock <= 160 * 1024,
              "iw_bwd_generic_kernel: table + rows exceed the LDS");
static_assert(sizeof(qb::FwdLds) % sizeof(float2) == 0, "iw_bwd_generic_kernel: the (gs, dl) row is read as float2");

// One lane's streaming accumulators without the sigma sums, which live in the lane's LDS column
struct IwGenAcc {
    float M, s1, s2, slw;
    float h[5];
    float pr1, pe1;   // the waiting row's factors: gs <- gs pr1 + pe1 dl (0, 0 before the lane's first draw)
    __device__ __forceinline__ float fold(float2 p) const { return fmaf(p.x, pr1, pe1 * p.y); }
};

// iw_bwd_draw at a run-time T.  sd: this thread's column of (gs, dl) pairs (stride kGenBlock); n0: node 0's slope per
// u^2.
__device__ __forceinline__ void iw_bwd_gen_draw(const QbDev& c, const qb::VoxColumns& vx, float2* sd, float n0,
                                                float log_s_sum, const qb::LogitMvn& qm, const qb::LogitMvn& pm,
                                                const IwKl& kl, float z0, float z1, IwGenAcc& acc) {
    float a, b;
    qb::reparam_logits(qm, z0, z1, a, b);
    // log q - log p of the draw and its gradient in u, q held inside log q: iw_bwd_draw's two forms, statement for
    // statement (that function's text is frozen with its bits, so the block is repeated here instead of shared)
    float dswr, ka, kb;
    if (fmaxf(fabsf(a), fabsf(b)) > QB_LOGIT_CLIP) {
        const float l0 = qb::clampf_(a, -QB_LOGIT_CLIP, QB_LOGIT_CLIP);
        const float l1 = qb::clampf_(b, -QB_LOGIT_CLIP, QB_LOGIT_CLIP);
        const float rq0 = l0 - qm.mu_o, rq1 = l1 - qm.mu_d;
        const float rp0 = l0 - pm.mu_o, rp1 = l1 - pm.mu_d;
        const float wq0 = rq0 * qm.i_so, wq1 = fmaf(rq1, qm.i_sd, rq0 * qm.i_bl);
        const float wp0 = rp0 * pm.i_so, wp1 = fmaf(rp1, pm.i_sd, rp0 * pm.i_bl);
        dswr = fmaf(wp0, wp0, wp1 * wp1) - fmaf(wq0, wq0, wq1 * wq1);
        ka = (wp0 * pm.i_so + wp1 * pm.i_bl) - (wq0 * qm.i_so + wq1 * qm.i_bl);
        kb = wp1 * pm.i_sd - wq1 * qm.i_sd;
    } else {
        const float w0 = fmaf(kl.m00, z0, kl.d0);
        const float w1 = fmaf(kl.m11, z1, fmaf(kl.m10, z0, kl.d1));
        dswr = fmaf(w0, w0, w1 * w1) - fmaf(z0, z0, z1 * z1);
        ka = (w0 * pm.i_so + w1 * pm.i_bl) - (z0 * qm.i_so + z1 * qm.i_bl);
        kb = w1 * pm.i_sd - z1 * qm.i_sd;
    }
    const float sa = qb::sigmoidf_(a), sb = qb::sigmoidf_(b);
    const float oef = sa * QB_OEF_RANGE + QB_MIN_OEF;
    const float dbv = sb * QB_DBV_RANGE + QB_MIN_DBV;
    const qb::FwdFast fv = qb::fwd_fast(c, oef, dbv);
    // se_norm on the prediction
    float np_ = qb::sig_eval(vx.L, fv, vx.se).s;
    if (c.multi_norm) np_ = (qb::sig_eval(vx.L, fv, vx.se - 1).s + np_ + qb::sig_eval(vx.L, fv, vx.se + 1).s) / 3.0f;
    const float inv_np = qb::rcpf_(np_ + 1e-3f);
    const qb::SlopeFactors kf = qb::slope_factors(c, fv, oef, dbv, vx.dbw);
    // the one pass over t (see the head of this section)
    float sq = 0.0f, a1 = 0.0f, go = 0.0f, gd = 0.0f, wo = 0.0f, wd = 0.0f;
    for (int t = 0; t < vx.T; ++t) {
        const qb::SigEval sg = qb::sig_eval(vx.L, fv, t);
        const float inv_s = vx.is[t * kGenBlock];
        const float r = (vx.yt[t * kGenBlock] - sg.s * inv_np) * inv_s;
        sq = fmaf(r, r, sq);
        // the waiting row into the sums; this draw's d/d log sigma_t of log sigma_t + r^2 / 2 takes its place
        sd[t * kGenBlock] = make_float2(acc.fold(sd[t * kGenBlock]), 1.0f - r * r);
        const float gy = -r * inv_s;              // d nll / d (sig_t / np)
        a1 = fmaf(gy, sg.s, a1);
        // the cubic's slope plus node 0's slope in x, as fwd_signal_grad keeps it
        const float dFu = sg.dFu() + n0 * sg.u * sg.u;
        const float ds_doef = sg.ds_doef(kf, dFu);
        const float ds_ddbv = sg.ds_ddbv(kf);
        go = fmaf(gy, ds_doef, go);
        gd = fmaf(gy, ds_ddbv, gd);
        if (t >= vx.w_lo && t <= vx.w_hi) {       // wave-uniform
            wo += ds_doef;
            wd += ds_ddbv;
        }
    }
    a1 *= inv_np * inv_np * vx.w_se;              // yhat_t = sig_t / (norm + 1e-3)
    const float g_oef = fmaf(go, inv_np, -a1 * wo), g_dbv = fmaf(gd, inv_np, -a1 * wd);
    const float lw = -fmaf(0.5f, sq, log_s_sum) - fmaf(0.5f, dswr, kl.cst);
    // the streaming log-sum-exp: rescale what is there to the new max, add this draw
    const float mn = fmaxf(acc.M, lw);
    const float r1 = qb::exp2f_((acc.M - mn) * QB_LOG2E);   // 0 on the lane's first draw
    const float e1 = qb::exp2f_((lw - mn) * QB_LOG2E);
    const float r2 = r1 * r1, e2 = e1 * e1;
    acc.M = mn;
    acc.s1 = fmaf(acc.s1, r1, e1);
    acc.s2 = fmaf(acc.s2, r2, e2);
    acc.slw += lw;
    acc.pr1 = r1;   // this draw's row now waits with its factors
    acc.pe1 = e1;
    // -d log w / du with q held: the NLL's gradient through forward_transform plus the KL draw's
    const float ha = fmaf(g_oef * QB_OEF_RANGE, sa * (1.0f - sa), ka);
    const float hb = fmaf(g_dbv * QB_DBV_RANGE, sb * (1.0f - sb), kb);
    const float wa = e2 * ha, wb = e2 * hb;
    acc.h[0] = fmaf(acc.h[0], r2, wa);
    acc.h[1] = fmaf(acc.h[1], r2, wa * z0);
    acc.h[2] = fmaf(acc.h[2], r2, wb);
    acc.h[3] = fmaf(acc.h[3], r2, wb * z1);
    acc.h[4] = fmaf(acc.h[4], r2, wb * z0);
}

template <int LPV>
__global__ __launch_bounds__(kGenBlock) void iw_bwd_generic_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* __restrict__ q, const float* __restrict__ prior, const float* __restrict__ log_sigma,
    const float* __restrict__ z, int K, uint64_t seed, int64_t voxel0, float* __restrict__ g_q,
    float* __restrict__ g_ls, float* __restrict__ out, double* __restrict__ partials, int64_t N) {
    extern __shared__ __align__(16) unsigned char smem[];
    qb::FwdLds* L = reinterpret_cast<qb::FwdLds*>(smem);
    __shared__ double red[3 * (kGenBlock / 64)];
    qb::fwd_lds_fill(L, g_tab, false);
    if (threadIdx.x < QB_MAX_T) L->blood_B[threadIdx.x] = c.blood_B[threadIdx.x];
    __syncthreads();
    // no barrier inside the loop: a thread reads and writes its own column of the rows only
    const qb::VoxColumns vx = qb::vox_columns<kGenBlock>(c, smem);
    const int T = vx.T, se = vx.se;
    float2* sd = reinterpret_cast<float2*>(smem + sizeof(qb::FwdLds) + sizeof(float) * 2 * T * kGenBlock) + threadIdx.x;
    const float n0 = c.dF_node0 / (c.tab_inv_h * c.tab_inv_h);   // node 0's slope per u^2

    constexpr int kVoxPerBlock = kGenBlock / LPV, kVoxPerWave = 64 / LPV;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int part = LPV == 1 ? 0 : lane >> 4;
    auto voxel_sum = [](float v) { return LPV == 1 ? v : qb::voxel_sum(v); };
    double s_lp = 0.0, s_el = 0.0, s_m = 0.0;
    const int64_t ntile = (N + kVoxPerBlock - 1) / kVoxPerBlock;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t v = tile * kVoxPerBlock + wave * kVoxPerWave + (LPV == 1 ? lane : lane & 15);
        if (v >= N) continue;
        const float m = mask ? mask[v] : 1.0f;
        const bool in = m > 0.0f;   // false for m <= 0 and NaN
        float* gv = g_ls + v * T;
        if (!in && !out) {          // nothing to score: zero gradients (the voxel's lanes take this branch together)
            if (part == 0) {
#pragma unroll
                for (int i = 0; i < 5; ++i) g_q[v * 5 + i] = 0.0f;
            }
            if (part == (LPV == 1 ? 0 : 1)) {
                for (int t = 0; t < T; ++t) gv[t] = 0.0f;
            }
            continue;
        }
        const float* xv = x + v * T;
        const float* lv = log_sigma + v * T;
        float qv[5], pv[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            qv[i] = q[v * 5 + i];
            pv[i] = prior[v * 5 + i];
        }
        // prepare_lik<T, SE, true> into the thread's columns: se_norm on the data, yt = x / norm, 1 / sigma
        const float nt = c.multi_norm ? (xv[se - 1] + xv[se] + xv[se + 1]) / 3.0f + 1e-3f : xv[se] + 1e-3f;
        const float inv_nt = qb::rcpf_(nt);
        float ls = 0.0f;
        for (int t = 0; t < T; ++t) {
            const float l = lv[t];
            vx.yt[t * kGenBlock] = xv[t] * inv_nt;
            vx.is[t * kGenBlock] = qb::exp2f_(-QB_LOG2E * l);
            sd[t * kGenBlock] = make_float2(0.0f, 0.0f);
            ls += l;
        }
        const float log_s_sum = ls + (float)T * 0.9189385332046727f;   // log sqrt(2 pi)
        const qb::LogitMvn qm = qb::make_mvn(qv), pm = qb::make_mvn(pv);
        const IwKl kl = make_iw_kl(qm, pm);
        const uint64_t vox = (uint64_t)(voxel0 + v);
        const float* zv = z ? z + v * (int64_t)K * 2 : nullptr;
        IwGenAcc acc;
        acc.M = -INFINITY;
        acc.s1 = acc.s2 = acc.slw = acc.pr1 = acc.pe1 = 0.0f;
#pragma unroll
        for (int i = 0; i < 5; ++i) acc.h[i] = 0.0f;
#pragma unroll 1
        for (int g = part; 4 * g < K; g += LPV) {
            const int cnt = K - 4 * g < 4 ? K - 4 * g : 4;
            qb::DrawQuad dq;
            if (!zv) dq.load(seed, vox, (uint32_t)g, qb::STREAM_IW);
#pragma unroll 1
            for (int d = 0; d < cnt; ++d) {
                float z0, z1;
                if (zv) {
                    z0 = zv[2 * (4 * g + d)];
                    z1 = zv[2 * (4 * g + d) + 1];
                } else {
                    dq.next(z0, z1);
                }
                iw_bwd_gen_draw(c, vx, sd, n0, log_s_sum, qm, pm, kl, z0, z1, acc);
            }
        }
        // merge the voxel's lanes in iw_bwd_kernel's fixed order (LPV = 4): common max, rescaled sums
        float Mx = acc.M;
        if (LPV > 1) {
            Mx = fmaxf(Mx, __shfl_xor(Mx, 16, 64));
            Mx = fmaxf(Mx, __shfl_xor(Mx, 32, 64));   // finite: lane group 0 holds draw 0
        }
        const float f1 = LPV == 1 ? 1.0f : qb::exp2f_((acc.M - Mx) * QB_LOG2E);   // 0 for a lane without draws
        const float f2 = f1 * f1;
        const float s1 = voxel_sum(acc.s1 * f1), s2 = voxel_sum(acc.s2 * f2), slw = voxel_sum(acc.slw);
        float h[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) h[i] = voxel_sum(acc.h[i] * f2);
        const float inv1 = 1.0f / s1;
        const float inv2 = inv1 * inv1;
        if (part == 0) {
            // transform_std / transform_offdiag (model.py:288-294), as in iw_bwd_kernel
            const float wq = m * inv2;   // a voxel outside the mask writes exact zeros (its draws may be NaN)
            g_q[v * 5 + 0] = in ? wq * h[0] : 0.0f;
            g_q[v * 5 + 1] = in ? wq * (h[1] * qm.e_so) * 3.0f * qb::sech2f_(qv[1]) : 0.0f;
            g_q[v * 5 + 2] = in ? wq * h[2] : 0.0f;
            g_q[v * 5 + 3] = in ? wq * (h[3] * qm.e_sd) * 3.0f * qb::sech2f_(qv[3]) : 0.0f;
            g_q[v * 5 + 4] = in ? wq * h[4] * 0.1353352832366127f * qb::sech2f_(qv[4]) : 0.0f;
            const float lp = Mx + (logf(s1) - logf((float)K));
            const float el = slw / (float)K;
            if (out) {
                out[3 * v + 0] = lp;
                out[3 * v + 1] = el;
                out[3 * v + 2] = (s1 * s1) / s2;
            }
            if (in) {
                s_lp += (double)m * -(double)lp;
                s_el += (double)m * -(double)el;
                s_m += (double)m;
            }
        }
        const float ws = m * inv1;
        for (int t = 0; t < T; ++t) {
            const float gt = voxel_sum(acc.fold(sd[t * kGenBlock]) * f1);   // with the lane's last row folded in
            if ((t & (LPV - 1)) == part) gv[t] = in ? ws * gt : 0.0f;   // the voxel's lanes share the stores
        }
    }
    block_partials_d(red, s_lp, s_el, s_m, partials);
}

}  // namespace

extern "C" int qbold_log_evidence_bwd_anyt(const qbold_ctx* ctx, const float* x, const float* mask, const float* q,
                                           const float* prior, const float* log_sigma, const float* z, int K,
                                           uint64_t seed, int64_t voxel0, float* g_q, float* g_log_sigma, float* out,
                                           double* sums, void* workspace, int64_t N, void* stream) {
    QB_NEED_DEVICE(ctx);
    QB_REQUIRE(N >= 0 && K >= 1 && K <= QBOLD_IW_MAX_K,
               "qbold_log_evidence_bwd_anyt: need N >= 0 and 1 <= K <= QBOLD_IW_MAX_K");
    QB_REQUIRE(sums && workspace, "qbold_log_evidence_bwd_anyt: null sums/workspace");
    QB_REQUIRE(N == 0 || (x && q && prior && log_sigma && g_q && g_log_sigma),
               "qbold_log_evidence_bwd_anyt: null buffer");
    if (!ctx->dev.full_model) {
        qb::set_error("qbold_log_evidence_bwd_anyt: gradients are built for the full signal model only");
        return QBOLD_ERR_UNSUPPORTED;
    }
    if (ctx->dev.tissue_mode != QBOLD_TISSUE_TABLE) {
        qb::set_error("qbold_log_evidence_bwd_anyt: the run-time-T kernel reads the tissue table; the literal tissue "
                      "mode is not built");
        return QBOLD_ERR_UNSUPPORTED;
    }
    if (!qb::elbo_fast_path(ctx)) {
        qb::set_error("qbold_log_evidence_bwd_anyt: the run-time-T kernel is built for the Gaussian likelihood on "
                      "linear data; Student-t / log-data contexts take qbold_log_evidence_bwd at T = 11 or 24");
        return QBOLD_ERR_UNSUPPORTED;
    }
    const int T = ctx->dev.T;
    QB_REQUIRE(T >= 1 && T <= QB_MAX_T, "qbold_log_evidence_bwd_anyt: need 1 <= T <= 64");
    hipStream_t s = (hipStream_t)stream;
    double* partials = reinterpret_cast<double*>(workspace);
    const int lpv = K <= QB_IW_BWD_LPV1_MAX_K ? 1 : QB_LANES_PER_VOXEL;
    const int vpb = kGenBlock / lpv;
    const int64_t ntile = (N + vpb - 1) / vpb;
    // the workspace holds 3 doubles per block of elbo_grid blocks
    const int grid = (int)(ntile < qb::elbo_grid(ctx) ? (ntile > 0 ? ntile : 1) : qb::elbo_grid(ctx));
    const size_t smem = sizeof(qb::FwdLds) + sizeof(float) * kGenRows * (size_t)T * kGenBlock;
    auto kern = lpv == 1 ? iw_bwd_generic_kernel<1> : iw_bwd_generic_kernel<QB_LANES_PER_VOXEL>;
    if (smem > 64 * 1024)   // per instantiation: the attribute belongs to the function that is launched
        QB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)smem));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kGenBlock), smem, s, ctx->dev, ctx->d_tab, x, mask, q, prior, log_sigma,
                       z, K, seed, voxel0, g_q, g_log_sigma, out, partials, N);
    QB_HIP(hipGetLastError());
    hipLaunchKernelGGL(qb::reduce_partials_kernel, dim3(1), dim3(192), 0, s, partials, grid, sums);
    QB_HIP(hipGetLastError());
    return QBOLD_OK;
}

extern "C" int qbold_log_evidence_bwd(const qbold_ctx* ctx, const float* x, const float* mask, const float* q,
                                      const float* prior, const float* log_sigma, const float* z, int K,
                                      uint64_t seed, int64_t voxel0, float* g_q, float* g_log_sigma, float* out,
                                      double* sums, void* workspace, int64_t N, void* stream) {
    QB_NEED_DEVICE(ctx);
    QB_REQUIRE(N >= 0 && K >= 1 && K <= QBOLD_IW_MAX_K,
               "qbold_log_evidence_bwd: need N >= 0 and 1 <= K <= QBOLD_IW_MAX_K");
    QB_REQUIRE(sums && workspace, "qbold_log_evidence_bwd: null sums/workspace");
    QB_REQUIRE(N == 0 || (x && q && prior && log_sigma && g_q && g_log_sigma),
               "qbold_log_evidence_bwd: null buffer");
    if (!(ctx->dev.full_model && ctx->dev.tissue_mode == QBOLD_TISSUE_TABLE)) {
        qb::set_error("qbold_log_evidence_bwd: gradients are built for the full signal model in table mode "
                      "(qbold_elbo_bwd's configurations)");
        return QBOLD_ERR_UNSUPPORTED;
    }
    if (ctx->dev.T != 11 && ctx->dev.T != 24) {
        qb::set_error("qbold_log_evidence_bwd: kernels are built for T = 11 or 24 taus");
        return QBOLD_ERR_UNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    double* partials = reinterpret_cast<double*>(workspace);
    const int lpv = K <= QB_IW_BWD_LPV1_MAX_K ? 1 : QB_LANES_PER_VOXEL;
    const int vpb = kBlock / lpv;
    const int64_t ntile = (N + vpb - 1) / vpb;
    const int grid = (int)(ntile < qb::elbo_grid(ctx) ? (ntile > 0 ? ntile : 1) : qb::elbo_grid(ctx));
#define QB_LAUNCH_IWB(TT, SEC)                                                                                       \
    do {                                                                                                             \
        if (lpv == 1)                                                                                                \
            hipLaunchKernelGGL((iw_bwd_kernel<TT, SEC, 1>), dim3(grid), dim3(kBlock), 0, s, ctx->dev, ctx->d_tab, x,  \
                               mask, q, prior, log_sigma, z, K, seed, voxel0, g_q, g_log_sigma, out, partials, N);   \
        else                                                                                                         \
            hipLaunchKernelGGL((iw_bwd_kernel<TT, SEC, QB_LANES_PER_VOXEL>), dim3(grid), dim3(kBlock), 0, s,         \
                               ctx->dev, ctx->d_tab, x, mask, q, prior, log_sigma, z, K, seed, voxel0, g_q,          \
                               g_log_sigma, out, partials, N);                                                       \
    } while (0)
    if (ctx->dev.T == 24) {
        QB_LAUNCH_IWB(24, -1);
    } else if (ctx->dev.se_idx == 2 && !ctx->dev.multi_norm) {
        QB_LAUNCH_IWB(11, 2);
    } else {
        QB_LAUNCH_IWB(11, -1);
    }
#undef QB_LAUNCH_IWB
    QB_HIP(hipGetLastError());
    hipLaunchKernelGGL(qb::reduce_partials_kernel, dim3(1), dim3(192), 0, s, partials, grid, sums);
    QB_HIP(hipGetLastError());
    return QBOLD_OK;
}
