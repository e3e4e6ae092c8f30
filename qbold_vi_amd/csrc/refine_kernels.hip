// refine_kernels.hip -- semi-amortised inference (Kim et al. 2018; Cremer et al. 2018, "Inference suboptimality"):
// starting from given encoder heads, each voxel runs its own few hundred gradient steps on its own objective
//   L(q) = E_q[nll(x | y)] + KL(q || prior),   y = reparameterised draw of q, sigma held fixed, no TV term,
// and returns the refined heads in the encoder's raw parameterisation, so every consumer of encoder heads
// (calculate_means, qbold_elbo_fwd, qbold_log_evidence_fwd, save_predictions) takes them unchanged.
//
// One lane per voxel (elbo_bwd_kernel's LPV = 1 mapping): x[T], sigma[T], q[5], prior[5] are loaded once and
// prepare_lik runs once; the parameters and the Adam moments m[5], v[5] stay in registers for all steps; q_out[5]
// (and the optional loss[2]) are written once.  HBM traffic is 4 (2 T + 10 + 1) bytes in and 20 (+ 8) out per voxel,
// whatever the number of steps.
//
// Per step: S reparameterised draws give d(mean NLL)/d(logit-space parameters) through passes 1 and 2 of
// elbo_bwd_kernel (restated here: signal, residuals, d nll / d yhat, the chain through the normalisation, the forward
// model and forward_transform; no log sigma gradient).  The KL enters by its exact gradient in closed form -- the
// expectation of the ELBO kernels' Monte-Carlo KL gradient while the logit clip does not bind -- then everything is
// chained to the raw heads through transform_std / transform_offdiag as at the end of elbo_bwd_kernel, and Adam (with
// bias correction) or SGD takes the step at a cosine-scheduled rate lr_j = lr_final + (lr - lr_final)(1 + cos(pi j /
// steps)) / 2.
//
// Draws: Philox stream 7; step j's draw d is draw j Sp + d of the voxel's stream (Sp = 4 ceil(S / 4): a Philox call
// never straddles two steps), i.e. exactly qbold_normals(seed, 7, voxel0, steps Sp) keyed by the global voxel, or the
// same layout [N][steps][Sp][2] given explicitly.  Both sources feed one code path, so they agree bit for bit.
#include <cmath>

#include "elbo_core.h"
#include "qbold_ctx.h"

namespace qb {
int elbo_grid(const qbold_ctx* ctx);   // elbo_kernels.hip
}

namespace {

// The Philox stream of the refinement draws: 0 - 3 are qbold_dev.h's, 4 kl_mog's, 5 the dropout masks', 6 the
// importance draws'.
constexpr uint32_t kStreamRefine = 7u;

constexpr int kBlock = 256;   // one voxel per lane

struct RefineArgs {
    int steps, S, Sp, adam;
    float lr, lr_final, beta1, beta2, eps;
};

struct FwdGrad {
    float s, ds_doef, ds_ddbv;
};

// signal and its partials at tau index t (full model, table mode): elbo_bwd_kernels.hip's fwd_signal_grad
__device__ __forceinline__ FwdGrad fwd_signal_grad(const qb::FwdLds* L, const QbDev& c,
                                                   const qb::FwdFast& v, float oef, float dbv, int t) {
    const float us = fmaf((float)t, v.ub, v.ua);
    const float u = fabsf(us);
    const int i = min((int)u, QB_TAB_SEG - 1);
    const float f = u - (float)i;
    const float4 k = L->tab[i];
    const float F = fmaf(fmaf(fmaf(k.w, f, k.z), f, k.y), f, k.x);
    const float ax = u * (1.0f / c.tab_inv_h);
    const float dF = fmaf(fmaf(3.0f * k.w, f, 2.0f * k.z), f, k.y) * c.tab_inv_h + c.dF_node0 * ax;
    const float e1 = qb::exp2f_(v.nd * F);
    const float e2 = qb::exp2f_(v.ng * c.blood_B[t]);
    const float tissue = v.tissue_w * e1, blood = v.blood_w * e2;
    FwdGrad g;
    g.s = tissue + blood;
    const float inv_oef = qb::rcpf_(oef);
    g.ds_doef = -dbv * dF * ax * inv_oef * tissue +
                (2.0f * QB_LN2) * v.ng * c.blood_B[t] * inv_oef * blood;
    const float dbw = c.include_blood ? c.m_bld_nb : 1.0f;
    g.ds_ddbv = -F * tissue - dbw * c.e_te_r2t * e1 + (c.include_blood ? dbw * c.e_r2b_te * e2 : 0.0f);
    return g;
}

// One draw's NLL and its gradient with respect to the logit-space sample parameters (mu_o, s_o, mu_d, s_d, c),
// ADDED to g[5]: passes 1 and 2 of elbo_bwd_kernel.
template <int T, int SE>
__device__ __forceinline__ float draw_nll_grad(const qb::FwdLds* L, const QbDev& c, const qb::VoxelLik<T>& lik,
                                               const qb::LogitMvn& qm, float z0, float z1, float (&g)[5]) {
    float a, b;
    qb::reparam_logits(qm, z0, z1, a, b);
    const float sa = qb::sigmoidf_(a), sb = qb::sigmoidf_(b);
    const float oef = sa * QB_OEF_RANGE + QB_MIN_OEF;
    const float dbv = sb * QB_DBV_RANGE + QB_MIN_DBV;
    const qb::FwdFast fv = qb::fwd_fast(c, oef, dbv);
    // pass 1: signals, residuals, NLL, d nll / d yhat
    float sig[T];
#pragma unroll
    for (int t = 0; t < T; ++t) sig[t] = qb::fwd_signal_fast(L, c, fv, t);
    const float inv_np = qb::rcpf_(qb::se_norm<T, SE>(c, sig));
    float acc = 0.0f, a1 = 0.0f;
    float gy[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        float yp = sig[t] * inv_np, dyp = 1.0f;
        if (c.predict_log) {                      // model.py:547-549 (only voxels with m > 0 are refined)
            dyp = qb::rcpf_(yp);
            yp = __logf(yp);
        }
        const float r = (lik.yt[t] - yp) * lik.inv_s[t];
        float dr = r;
        if (c.use_student_t) {                    // model.py:557-559
            const float w = (c.st_df + 1.0f) * qb::rcpf_(fmaf(r, r, c.st_df));
            acc += (c.st_df + 1.0f) * log1pf(r * r * qb::rcpf_(c.st_df)) - 2.0f * c.st_const;
            dr = w * r;
        } else {
            acc = fmaf(r, r, acc);
        }
        gy[t] = -dr * lik.inv_s[t] * dyp;
        a1 = fmaf(gy[t], sig[t], a1);
    }
    a1 *= inv_np * inv_np;
    // pass 2: chain through the normalisation and the forward model
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
        const FwdGrad fg = fwd_signal_grad(L, c, fv, oef, dbv, t);
        g_oef = fmaf(gs, fg.ds_doef, g_oef);
        g_dbv = fmaf(gs, fg.ds_ddbv, g_dbv);
    }
    const float ga = g_oef * QB_OEF_RANGE * sa * (1.0f - sa);   // forward_transform
    const float gb = g_dbv * QB_DBV_RANGE * sb * (1.0f - sb);
    g[0] += ga;
    g[1] = fmaf(ga, z0 * qm.e_so, g[1]);
    g[2] += gb;
    g[4] = fmaf(gb, z0, g[4]);
    g[3] = fmaf(gb, z1 * qm.e_sd, g[3]);
    return fmaf(0.5f, acc, lik.log_s_sum);
}

// KL(q || p) of two Gaussians in logit space in whitened form, M = L_p^-1 L_q, d = L_p^-1 (mu_q - mu_p):
//   KL = (|M|_F^2 + |d|^2) / 2 - log det M - 1,   log det M = (s_o + s_d)_q - (s_o + s_d)_p
// -- the expectation of the Monte-Carlo KL of the ELBO kernels; qbold_kl_closed (model.py:612-652) gives the same
// number when the prior's off-diagonal term is 0, its trace term being tr(L_p^-1 L_p^-T Sigma_q) -- and ADDS its
// gradient with respect to (mu_o, s_o, mu_d, s_d, c) of q.
__device__ __forceinline__ float kl_closed_grad(const qb::LogitMvn& q, const qb::LogitMvn& p, float (&g)[5]) {
    const float dmu_o = q.mu_o - p.mu_o, dmu_d = q.mu_d - p.mu_d;
    const float d0 = dmu_o * p.i_so, d1 = fmaf(dmu_d, p.i_sd, dmu_o * p.i_bl);
    const float m00 = q.e_so * p.i_so, m10 = fmaf(q.c, p.i_sd, q.e_so * p.i_bl), m11 = q.e_sd * p.i_sd;
    g[0] += fmaf(d0, p.i_so, d1 * p.i_bl);
    g[1] += fmaf(m00, m00, fmaf(m10, q.e_so * p.i_bl, -1.0f));
    g[2] += d1 * p.i_sd;
    g[3] += fmaf(m11, m11, -1.0f);
    g[4] += m10 * p.i_sd;
    const float sq = fmaf(m00, m00, fmaf(m10, m10, fmaf(m11, m11, fmaf(d0, d0, d1 * d1))));
    return fmaf(0.5f, sq, (p.s_o + p.s_d) - (q.s_o + q.s_d) - 1.0f);
}

template <int T, int SE>
__global__ __launch_bounds__(kBlock) void refine_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* q_in, const float* __restrict__ prior, const float* __restrict__ sigma,
    const float* __restrict__ z, RefineArgs ra, uint64_t seed, int64_t voxel0, float* q_out,
    float* __restrict__ loss, int64_t N) {
    __shared__ qb::FwdLds L;
    qb::fwd_lds_fill(&L, g_tab, false);
    __syncthreads();

    const int steps = ra.steps, S = ra.S, Sp = ra.Sp;
    const int tail = (steps + 9) / 10;   // the last ceil(steps / 10) steps make loss[1]
    const float inv_S = 1.0f / (float)S;
    for (int64_t v = blockIdx.x * (int64_t)kBlock + threadIdx.x; v < N; v += (int64_t)gridDim.x * kBlock) {
        float qv[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) qv[i] = q_in[v * 5 + i];
        const float m = mask ? mask[v] : 1.0f;
        if (!(m > 0.0f)) {   // masked voxel: q copied through bit for bit
#pragma unroll
            for (int i = 0; i < 5; ++i) q_out[v * 5 + i] = qv[i];
            if (loss) {
                loss[2 * v + 0] = 0.0f;
                loss[2 * v + 1] = 0.0f;
            }
            continue;
        }
        float xv[T], sv[T], pv[5];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            xv[t] = x[v * T + t];
            sv[t] = sigma[v * T + t];
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) pv[i] = prior[v * 5 + i];
        qb::VoxelLik<T> lik;
        qb::prepare_lik<T, SE, false>(c, xv, sv, 1.0f, lik);
        const qb::LogitMvn pm = qb::make_mvn(pv);
        const uint64_t vox = (uint64_t)(voxel0 + v);
        const float* zv = z ? z + v * (int64_t)steps * Sp * 2 : nullptr;

        float m1[5], m2[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) m1[i] = m2[i] = 0.0f;
        float b1t = 1.0f, b2t = 1.0f;   // beta^t of the bias correction
        float loss0 = 0.0f, loss_tail = 0.0f;
#pragma unroll 1
        for (int j = 0; j < steps; ++j) {
            const qb::LogitMvn qm = qb::make_mvn(qv);
            float g[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            float nll = 0.0f;
#pragma unroll 1
            for (int k = 0; 4 * k < S; ++k) {
                const int cnt = S - 4 * k < 4 ? S - 4 * k : 4;
                qb::DrawQuad dq;
                if (!zv) dq.load(seed, vox, (uint32_t)(j * (Sp >> 2) + k), kStreamRefine);
#pragma unroll 1
                for (int d = 0; d < cnt; ++d) {
                    float z0, z1;
                    if (zv) {
                        const int64_t i = (int64_t)j * Sp + 4 * k + d;
                        z0 = zv[2 * i];
                        z1 = zv[2 * i + 1];
                    } else {
                        dq.next(z0, z1);
                    }
                    nll += draw_nll_grad<T, SE>(&L, c, lik, qm, z0, z1, g);
                }
            }
#pragma unroll
            for (int i = 0; i < 5; ++i) g[i] *= inv_S;
            const float kl = kl_closed_grad(qm, pm, g);
            const float lj = fmaf(nll, inv_S, kl);   // this step's Monte-Carlo -ELBO at the step's q
            if (j == 0) loss0 = lj;
            if (j >= steps - tail) loss_tail += lj;
            // transform_std / transform_offdiag (model.py:288-294): s = 3 tanh(raw) - 1, c = tanh(raw) e^-2
            g[1] *= 3.0f * qb::sech2f_(qv[1]);
            g[3] *= 3.0f * qb::sech2f_(qv[3]);
            g[4] *= 0.1353352832366127f * qb::sech2f_(qv[4]);
            const float lr = fmaf(0.5f * (ra.lr - ra.lr_final), 1.0f + cosf((float)M_PI * ((float)j / (float)steps)),
                                  ra.lr_final);
            if (ra.adam) {
                b1t *= ra.beta1;
                b2t *= ra.beta2;
                const float c1 = 1.0f / (1.0f - b1t), c2 = 1.0f / (1.0f - b2t);
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    m1[i] = fmaf(ra.beta1, m1[i], (1.0f - ra.beta1) * g[i]);
                    m2[i] = fmaf(ra.beta2, m2[i], (1.0f - ra.beta2) * (g[i] * g[i]));
                    qv[i] -= lr * (m1[i] * c1) / (sqrtf(m2[i] * c2) + ra.eps);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 5; ++i) qv[i] = fmaf(-lr, g[i], qv[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) q_out[v * 5 + i] = qv[i];
        if (loss) {
            loss[2 * v + 0] = loss0;
            loss[2 * v + 1] = loss_tail / (float)tail;
        }
    }
}

}  // namespace

extern "C" int qbold_refine_posterior(const qbold_ctx* ctx, const float* x, const float* mask, const float* q_in,
                                      const float* prior, const float* sigma, const float* z, int steps, int S,
                                      const qbold_refine_cfg* cfg, uint64_t seed, int64_t voxel0, float* q_out,
                                      float* loss, int64_t N, void* stream) {
    QB_NEED_DEVICE(ctx);
    QB_REQUIRE(cfg, "qbold_refine_posterior: null cfg");
    QB_REQUIRE(N >= 0 && steps >= 1 && S >= 1, "qbold_refine_posterior: need N >= 0, steps >= 1, S >= 1");
    const int64_t Sp = 4 * (((int64_t)S + 3) / 4);
    QB_REQUIRE((int64_t)steps * Sp / 4 < ((int64_t)1 << 32),
               "qbold_refine_posterior: steps * Sp / 4 must fit the 32-bit Philox call word");
    QB_REQUIRE(cfg->optimizer == 0 || cfg->optimizer == 1, "qbold_refine_posterior: optimizer must be 0 (Adam) or 1 (SGD)");
    QB_REQUIRE(cfg->lr > 0.0f && cfg->lr_final >= 0.0f, "qbold_refine_posterior: need lr > 0 and lr_final >= 0");
    QB_REQUIRE(cfg->optimizer == 1 || (cfg->beta1 >= 0.0f && cfg->beta1 < 1.0f && cfg->beta2 >= 0.0f &&
                                       cfg->beta2 < 1.0f && cfg->eps > 0.0f),
               "qbold_refine_posterior: Adam needs 0 <= beta1, beta2 < 1 and eps > 0");
    QB_REQUIRE(N == 0 || (x && q_in && prior && sigma && q_out), "qbold_refine_posterior: null buffer");
    if (!(ctx->dev.full_model && ctx->dev.tissue_mode == QBOLD_TISSUE_TABLE)) {
        qb::set_error("qbold_refine_posterior: built for the full signal model in table mode "
                      "(Gaussian or Student-t likelihood, linear or log data, either normalisation)");
        return QBOLD_ERR_UNSUPPORTED;
    }
    if (ctx->dev.T != 11 && ctx->dev.T != 24) {
        qb::set_error("qbold_refine_posterior: kernels are built for T = 11 or 24 taus");
        return QBOLD_ERR_UNSUPPORTED;
    }
    if (N == 0) return QBOLD_OK;
    hipStream_t s = (hipStream_t)stream;
    const RefineArgs ra{steps, S, (int)Sp, cfg->optimizer == 0 ? 1 : 0, cfg->lr, cfg->lr_final,
                        cfg->beta1, cfg->beta2, cfg->eps};
    const int64_t ntile = (N + kBlock - 1) / kBlock;
    const int grid = (int)(ntile < qb::elbo_grid(ctx) ? ntile : qb::elbo_grid(ctx));
#define QB_LAUNCH_REFINE(TT, SEC)                                                                                   \
    hipLaunchKernelGGL((refine_kernel<TT, SEC>), dim3(grid), dim3(kBlock), 0, s, ctx->dev, ctx->d_tab, x, mask,   \
                       q_in, prior, sigma, z, ra, seed, voxel0, q_out, loss, N)
    if (ctx->dev.T == 24) {
        QB_LAUNCH_REFINE(24, -1);
    } else if (ctx->dev.se_idx == 2 && !ctx->dev.multi_norm) {
        QB_LAUNCH_REFINE(11, 2);
    } else {
        QB_LAUNCH_REFINE(11, -1);
    }
#undef QB_LAUNCH_REFINE
    QB_HIP(hipGetLastError());
    return QBOLD_OK;
}

// ---- Refinement of a volume under the TV smoothness prior (qbold_refine_posterior_spatial) ----------------------
// Full-batch Adam / SGD on F(q) = sum_v (E_q_v[nll] + KL(q_v || p_v)) + w TV(q), TV = qbold_smoothness's tv_sum.
// Jacobi steps: step j's gradient of every voxel is taken at the step-j heads of all voxels, so the TV term couples
// a voxel to its four in-plane neighbours' step-j means.  One launch per step (the grid is the barrier between
// steps); the heads ping-pong between two workspace buffers, the Adam moments and the loss accumulators live in the
// workspace.  Per voxel and step: 4 (2 T + 21) B in (x, sigma, heads, moments, loss, prior, mask, the neighbours'
// heads 0 and 2 and masks), 68 B out.  The per-voxel arithmetic is refine_kernel's step, expression for expression;
// the compiler schedules the inlined likelihood differently in the two kernels, so they agree to rounding, not to the
// bit.  w = 0 couples nothing: the entry runs qbold_refine_posterior itself, which gives its bits exactly.
namespace {

constexpr int kStateFloats = 12;   // workspace state per voxel: m1[5], m2[5], loss0, loss_tail

struct TvStep {
    int j;             // this launch's step
    float b1p, b2p;    // beta1^j, beta2^j: refine_kernel's running products before step j, accumulated in float32
    float w;           // TV weight, > 0
    qbold_geometry gm;
    int last;          // j == steps - 1: write q_dst from q_in for masked voxels and the loss
};

__device__ __forceinline__ float tv_sigmoid(float u) { return 1.0f / (1.0f + expf(-u)); }   // smoothness_kernel's

template <int T, int SE>
__global__ __launch_bounds__(kBlock) void refine_tv_step_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* q_in, const float* __restrict__ q_src, const float* __restrict__ prior,
    const float* __restrict__ sigma, const float* __restrict__ z, RefineArgs ra, TvStep st, uint64_t seed,
    int64_t voxel0, float* q_dst, float4* __restrict__ state, float* __restrict__ loss, int64_t N) {
    __shared__ qb::FwdLds L;
    qb::fwd_lds_fill(&L, g_tab, false);
    __syncthreads();

    const int steps = ra.steps, S = ra.S, Sp = ra.Sp, j = st.j;
    const int tail = (steps + 9) / 10;
    const float inv_S = 1.0f / (float)S;
    const int64_t yz = (int64_t)st.gm.Y * st.gm.Z;
    for (int64_t v = blockIdx.x * (int64_t)kBlock + threadIdx.x; v < N; v += (int64_t)gridDim.x * kBlock) {
        const float m = mask ? mask[v] : 1.0f;
        if (!(m > 0.0f)) {   // masked voxel: q_in copied through bit for bit at the last step, never read by others
            if (st.last) {
#pragma unroll
                for (int i = 0; i < 5; ++i) q_dst[v * 5 + i] = q_in[v * 5 + i];
                if (loss) {
                    loss[2 * v + 0] = 0.0f;
                    loss[2 * v + 1] = 0.0f;
                }
            }
            continue;
        }
        float qv[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) qv[i] = q_src[v * 5 + i];
        float xv[T], sv[T], pv[5];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            xv[t] = x[v * T + t];
            sv[t] = sigma[v * T + t];
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) pv[i] = prior[v * 5 + i];
        qb::VoxelLik<T> lik;
        qb::prepare_lik<T, SE, false>(c, xv, sv, 1.0f, lik);
        const qb::LogitMvn pm = qb::make_mvn(pv);
        const uint64_t vox = (uint64_t)(voxel0 + v);
        const float* zv = z ? z + v * (int64_t)steps * Sp * 2 : nullptr;

        float m1[5], m2[5], loss0 = 0.0f, loss_tail = 0.0f;
#pragma unroll
        for (int i = 0; i < 5; ++i) m1[i] = m2[i] = 0.0f;
        if (j > 0) {
            const float4 s0 = state[3 * v], s1 = state[3 * v + 1], s2 = state[3 * v + 2];
            if (ra.adam) {
                m1[0] = s0.x; m1[1] = s0.y; m1[2] = s0.z; m1[3] = s0.w; m1[4] = s1.x;
                m2[0] = s1.y; m2[1] = s1.z; m2[2] = s1.w; m2[3] = s2.x; m2[4] = s2.y;
            }
            loss0 = s2.z;
            loss_tail = s2.w;
        }

        // refine_kernel's step j
        const qb::LogitMvn qm = qb::make_mvn(qv);
        float g[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        float nll = 0.0f;
#pragma unroll 1
        for (int k = 0; 4 * k < S; ++k) {
            const int cnt = S - 4 * k < 4 ? S - 4 * k : 4;
            qb::DrawQuad dq;
            if (!zv) dq.load(seed, vox, (uint32_t)(j * (Sp >> 2) + k), kStreamRefine);
#pragma unroll 1
            for (int d = 0; d < cnt; ++d) {
                float z0, z1;
                if (zv) {
                    const int64_t i = (int64_t)j * Sp + 4 * k + d;
                    z0 = zv[2 * i];
                    z1 = zv[2 * i + 1];
                } else {
                    dq.next(z0, z1);
                }
                nll += draw_nll_grad<T, SE>(&L, c, lik, qm, z0, z1, g);
            }
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) g[i] *= inv_S;
        const float kl = kl_closed_grad(qm, pm, g);
        const float lj = fmaf(nll, inv_S, kl);
        if (j == 0) loss0 = lj;
        if (j >= steps - tail) loss_tail += lj;
        {   // w d TV / d (mu_o, mu_d) at the step-j heads: smoothness_kernel's subgradient
            const int xi = (int)((v / yz) % st.gm.X), yi = (int)((v / st.gm.Z) % st.gm.Y);
            const float so = tv_sigmoid(qv[0]), sd = tv_sigmoid(qv[2]);
            const int64_t off[4] = {yz, (int64_t)st.gm.Z, -yz, -(int64_t)st.gm.Z};
            const bool inside[4] = {xi + 1 < st.gm.X, yi + 1 < st.gm.Y, xi > 0, yi > 0};
            float go = 0.0f, gd = 0.0f;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                if (!inside[n]) continue;
                const int64_t u = v + off[n];
                if (!(mask ? mask[u] > 0.0f : true)) continue;
                const float dO = so - tv_sigmoid(q_src[5 * u]), dD = sd - tv_sigmoid(q_src[5 * u + 2]);
                go += (dO > 0.0f) - (dO < 0.0f);
                gd += (dD > 0.0f) - (dD < 0.0f);
            }
            g[0] += st.w * go * so * (1.0f - so);
            g[2] += st.w * gd * sd * (1.0f - sd);
        }
        g[1] *= 3.0f * qb::sech2f_(qv[1]);
        g[3] *= 3.0f * qb::sech2f_(qv[3]);
        g[4] *= 0.1353352832366127f * qb::sech2f_(qv[4]);
        const float lr = fmaf(0.5f * (ra.lr - ra.lr_final), 1.0f + cosf((float)M_PI * ((float)j / (float)steps)),
                              ra.lr_final);
        if (ra.adam) {
            // refine_kernel's expressions (the compiler may fuse the product into 1 - b: it must fuse it alike)
            const float b1t = st.b1p * ra.beta1, b2t = st.b2p * ra.beta2;
            const float c1 = 1.0f / (1.0f - b1t), c2 = 1.0f / (1.0f - b2t);
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                m1[i] = fmaf(ra.beta1, m1[i], (1.0f - ra.beta1) * g[i]);
                m2[i] = fmaf(ra.beta2, m2[i], (1.0f - ra.beta2) * (g[i] * g[i]));
                qv[i] -= lr * (m1[i] * c1) / (sqrtf(m2[i] * c2) + ra.eps);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 5; ++i) qv[i] = fmaf(-lr, g[i], qv[i]);
        }

#pragma unroll
        for (int i = 0; i < 5; ++i) q_dst[v * 5 + i] = qv[i];
        if (st.last) {
            if (loss) {
                loss[2 * v + 0] = loss0;
                loss[2 * v + 1] = loss_tail / (float)tail;
            }
        } else {
            state[3 * v] = make_float4(m1[0], m1[1], m1[2], m1[3]);
            state[3 * v + 1] = make_float4(m1[4], m2[0], m2[1], m2[2]);
            state[3 * v + 2] = make_float4(m2[3], m2[4], loss0, loss_tail);
        }
    }
}

// voxels of a geometry, or -1 when it is not a positive one or the workspace size would not fit int64
int64_t tv_voxels(const qbold_geometry* g) {
    if (!g || g->B <= 0 || g->X <= 0 || g->Y <= 0 || g->Z <= 0) return -1;
    int64_t n = 1;
    for (const int32_t d : {g->B, g->X, g->Y, g->Z}) {
        if (__builtin_mul_overflow(n, (int64_t)d, &n)) return -1;
    }
    int64_t b;
    if (__builtin_mul_overflow(n, (int64_t)(sizeof(float) * (kStateFloats + 10)), &b)) return -1;
    return n;
}

}  // namespace

extern "C" int64_t qbold_refine_spatial_workspace_bytes(const qbold_ctx* ctx, const qbold_geometry* geom) {
    const int64_t N = tv_voxels(geom);
    if (!ctx || N < 0) return QBOLD_ERR_INVALID;
    return N * (int64_t)sizeof(float) * (kStateFloats + 10);
}

extern "C" int qbold_refine_posterior_spatial(const qbold_ctx* ctx, const float* x, const float* mask,
                                              const float* q_in, const float* prior, const float* sigma,
                                              const float* z, const qbold_geometry* geom, float tv_weight, int steps,
                                              int S, const qbold_refine_cfg* cfg, uint64_t seed, int64_t voxel0,
                                              float* q_out, float* loss, void* workspace, void* stream) {
    QB_NEED_DEVICE(ctx);
    QB_REQUIRE(cfg, "qbold_refine_posterior_spatial: null cfg");
    QB_REQUIRE(steps >= 1 && S >= 1, "qbold_refine_posterior_spatial: need steps >= 1, S >= 1");
    const int64_t N = tv_voxels(geom);
    QB_REQUIRE(N >= 0, "qbold_refine_posterior_spatial: need a geometry with B, X, Y, Z >= 1 whose voxel count "
                       "and workspace fit int64");
    QB_REQUIRE(std::isfinite(tv_weight) && tv_weight >= 0.0f,
               "qbold_refine_posterior_spatial: tv_weight must be finite and >= 0");
    const int64_t Sp = 4 * (((int64_t)S + 3) / 4);
    QB_REQUIRE((int64_t)steps * Sp / 4 < ((int64_t)1 << 32),
               "qbold_refine_posterior_spatial: steps * Sp / 4 must fit the 32-bit Philox call word");
    QB_REQUIRE(cfg->optimizer == 0 || cfg->optimizer == 1,
               "qbold_refine_posterior_spatial: optimizer must be 0 (Adam) or 1 (SGD)");
    QB_REQUIRE(cfg->lr > 0.0f && cfg->lr_final >= 0.0f, "qbold_refine_posterior_spatial: need lr > 0 and lr_final >= 0");
    QB_REQUIRE(cfg->optimizer == 1 || (cfg->beta1 >= 0.0f && cfg->beta1 < 1.0f && cfg->beta2 >= 0.0f &&
                                       cfg->beta2 < 1.0f && cfg->eps > 0.0f),
               "qbold_refine_posterior_spatial: Adam needs 0 <= beta1, beta2 < 1 and eps > 0");
    QB_REQUIRE(x && q_in && prior && sigma && q_out, "qbold_refine_posterior_spatial: null buffer");
    QB_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0,
               "qbold_refine_posterior_spatial: need a 16-byte aligned workspace of "
               "qbold_refine_spatial_workspace_bytes() bytes");
    if (!(ctx->dev.full_model && ctx->dev.tissue_mode == QBOLD_TISSUE_TABLE)) {
        qb::set_error("qbold_refine_posterior_spatial: built for the full signal model in table mode "
                      "(Gaussian or Student-t likelihood, linear or log data, either normalisation)");
        return QBOLD_ERR_UNSUPPORTED;
    }
    if (ctx->dev.T != 11 && ctx->dev.T != 24) {
        qb::set_error("qbold_refine_posterior_spatial: kernels are built for T = 11 or 24 taus");
        return QBOLD_ERR_UNSUPPORTED;
    }
    // no coupling: the per-voxel refinement, one launch with the state in registers (its bits by construction)
    if (tv_weight == 0.0f)
        return qbold_refine_posterior(ctx, x, mask, q_in, prior, sigma, z, steps, S, cfg, seed, voxel0, q_out, loss,
                                      N, stream);
    hipStream_t s = (hipStream_t)stream;
    const RefineArgs ra{steps, S, (int)Sp, cfg->optimizer == 0 ? 1 : 0, cfg->lr, cfg->lr_final,
                        cfg->beta1, cfg->beta2, cfg->eps};
    // workspace: state [N][12] (16-byte rows of float4), then the two head buffers [N][5]
    float4* state = (float4*)workspace;
    float* heads[2] = {(float*)workspace + N * kStateFloats, (float*)workspace + N * (kStateFloats + 5)};
    const int64_t ntile = (N + kBlock - 1) / kBlock;
    const int64_t cap = 8 * (int64_t)qb::elbo_grid(ctx);
    const int grid = (int)(ntile < cap ? ntile : cap);
    TvStep st{0, 1.0f, 1.0f, tv_weight, *geom, 0};
    for (int j = 0; j < steps; ++j) {
        st.j = j;
        st.last = j == steps - 1;
        const float* src = j == 0 ? q_in : heads[(j - 1) & 1];
        // the last step writes q_out, except a single step, which reads q_in (q_out may alias it) and is copied
        float* dst = st.last && steps > 1 ? q_out : heads[j & 1];
#define QB_LAUNCH_REFINE_TV(TT, SEC)                                                                                \
    hipLaunchKernelGGL((refine_tv_step_kernel<TT, SEC>), dim3(grid), dim3(kBlock), 0, s, ctx->dev, ctx->d_tab, x,  \
                       mask, q_in, src, prior, sigma, z, ra, st, seed, voxel0, dst, state, loss, N)
        if (ctx->dev.T == 24) {
            QB_LAUNCH_REFINE_TV(24, -1);
        } else if (ctx->dev.se_idx == 2 && !ctx->dev.multi_norm) {
            QB_LAUNCH_REFINE_TV(11, 2);
        } else {
            QB_LAUNCH_REFINE_TV(11, -1);
        }
#undef QB_LAUNCH_REFINE_TV
        QB_HIP(hipGetLastError());
        st.b1p *= cfg->beta1;   // refine_kernel's running products, rounded to float32 after every step
        st.b2p *= cfg->beta2;
    }
    if (steps == 1) QB_HIP(hipMemcpyAsync(q_out, heads[0], N * 5 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return QBOLD_OK;
}
