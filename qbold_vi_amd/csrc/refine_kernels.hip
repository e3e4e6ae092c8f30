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

// ---- the argument checks the four entries share (what: the entry's name, for the message) ------------------------
#define QB_REFINE_REQUIRE(cond, msg)                        \
    do {                                                    \
        if (!(cond)) {                                      \
            qb::set_error(std::string(what) + ": " + msg);  \
            return QBOLD_ERR_INVALID;                       \
        }                                                   \
    } while (0)

// steps, S, the Philox call word and the optimiser's settings; *Sp = 4 ceil(S / 4)
int refine_check_cfg(const char* what, const qbold_refine_cfg* cfg, int steps, int S, int64_t* Sp) {
    *Sp = 4 * (((int64_t)S + 3) / 4);
    QB_REFINE_REQUIRE((int64_t)steps * *Sp / 4 < ((int64_t)1 << 32),
                      "steps * Sp / 4 must fit the 32-bit Philox call word");
    QB_REFINE_REQUIRE(cfg->optimizer == 0 || cfg->optimizer == 1, "optimizer must be 0 (Adam) or 1 (SGD)");
    QB_REFINE_REQUIRE(cfg->lr > 0.0f && cfg->lr_final >= 0.0f, "need lr > 0 and lr_final >= 0");
    QB_REFINE_REQUIRE(cfg->optimizer == 1 || (cfg->beta1 >= 0.0f && cfg->beta1 < 1.0f && cfg->beta2 >= 0.0f &&
                                              cfg->beta2 < 1.0f && cfg->eps > 0.0f),
                      "Adam needs 0 <= beta1, beta2 < 1 and eps > 0");
    return QBOLD_OK;
}

// the configurations with a kernel: the full model in table mode; any_t: every 1 <= T <= QB_MAX_T, else T = 11 / 24
int refine_check_mode(const char* what, const qbold_ctx* ctx, bool any_t) {
    if (!(ctx->dev.full_model && ctx->dev.tissue_mode == QBOLD_TISSUE_TABLE)) {
        qb::set_error(std::string(what) + ": built for the full signal model in table mode "
                      "(Gaussian or Student-t likelihood, linear or log data, either normalisation)");
        return QBOLD_ERR_UNSUPPORTED;
    }
    if (any_t) {
        QB_REFINE_REQUIRE(ctx->dev.T >= 1 && ctx->dev.T <= QB_MAX_T, "need 1 <= T <= 64");
    } else if (ctx->dev.T != 11 && ctx->dev.T != 24) {
        qb::set_error(std::string(what) + ": kernels are built for T = 11 or 24 taus");
        return QBOLD_ERR_UNSUPPORTED;
    }
    return QBOLD_OK;
}

// every check of the per-voxel entries
int refine_check_voxels(const char* what, const qbold_ctx* ctx, const float* x, const float* q_in, const float* prior,
                        const float* sigma, int steps, int S, const qbold_refine_cfg* cfg, const float* q_out,
                        int64_t N, bool any_t, int64_t* Sp) {
    QB_NEED_DEVICE(ctx);
    QB_REFINE_REQUIRE(cfg, "null cfg");
    QB_REFINE_REQUIRE(N >= 0 && steps >= 1 && S >= 1, "need N >= 0, steps >= 1, S >= 1");
    if (const int rc = refine_check_cfg(what, cfg, steps, S, Sp)) return rc;
    QB_REFINE_REQUIRE(N == 0 || (x && q_in && prior && sigma && q_out), "null buffer");
    return refine_check_mode(what, ctx, any_t);
}

}  // namespace

extern "C" int qbold_refine_posterior(const qbold_ctx* ctx, const float* x, const float* mask, const float* q_in,
                                      const float* prior, const float* sigma, const float* z, int steps, int S,
                                      const qbold_refine_cfg* cfg, uint64_t seed, int64_t voxel0, float* q_out,
                                      float* loss, int64_t N, void* stream) {
    int64_t Sp;
    if (const int rc = refine_check_voxels("qbold_refine_posterior", ctx, x, q_in, prior, sigma, steps, S, cfg, q_out,
                                           N, false, &Sp))
        return rc;
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

// every check of the spatial entries; *N = the geometry's voxels
int refine_check_volume(const char* what, const qbold_ctx* ctx, const float* x, const float* q_in, const float* prior,
                        const float* sigma, const qbold_geometry* geom, float tv_weight, int steps, int S,
                        const qbold_refine_cfg* cfg, const float* q_out, const void* workspace, bool any_t,
                        int64_t* Sp, int64_t* N) {
    QB_NEED_DEVICE(ctx);
    QB_REFINE_REQUIRE(cfg, "null cfg");
    QB_REFINE_REQUIRE(steps >= 1 && S >= 1, "need steps >= 1, S >= 1");
    *N = tv_voxels(geom);
    QB_REFINE_REQUIRE(*N >= 0, "need a geometry with B, X, Y, Z >= 1 whose voxel count and workspace fit int64");
    QB_REFINE_REQUIRE(std::isfinite(tv_weight) && tv_weight >= 0.0f, "tv_weight must be finite and >= 0");
    if (const int rc = refine_check_cfg(what, cfg, steps, S, Sp)) return rc;
    QB_REFINE_REQUIRE(x && q_in && prior && sigma && q_out, "null buffer");
    QB_REFINE_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0,
                      "need a 16-byte aligned workspace of qbold_refine_spatial_workspace_bytes() bytes");
    return refine_check_mode(what, ctx, any_t);
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
    int64_t Sp, N;
    if (const int rc = refine_check_volume("qbold_refine_posterior_spatial", ctx, x, q_in, prior, sigma, geom,
                                           tv_weight, steps, S, cfg, q_out, workspace, false, &Sp, &N))
        return rc;
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

// ---- any number of taus (1 <= T <= QB_MAX_T): qbold_refine_posterior_anyt, qbold_refine_posterior_spatial_anyt ------
// refine_kernel's and refine_tv_step_kernel's functions with T and the spin-echo index read at run time.  The kernels
// above are frozen with their bits (T = 11 / 24 keep them); what is not tied to a compile-time T is shared with them
// (kl_closed_grad, RefineArgs, TvStep, tv_sigmoid, the stream, the workspace layout), and the two kernels here share
// one per-voxel step (gen_step_grad, refine_update) and one TV subgradient (tv_subgrad).
//
// Shape: laplace_kernel's and elbo_bwd_generic_kernel<1>'s.  128 threads, one lane per voxel; the voxel's normalised
// (optionally log) data and 1 / sigma live in dynamic LDS as rows [t][thread] beside FwdLds: 8 T bytes per thread,
// sizeof(FwdLds) + 1,024 T bytes per block (T = 11: 16.8 KiB, T = 33: 38.8 KiB, T = 64: 69.8 KiB, above the 64 KiB
// default and taken by the hipFuncSetAttribute opt-in; two blocks per CU there, one wave per SIMD).  A thread touches
// only its own column, so a wave's access at a fixed t is 64 consecutive floats (conflict-free) and no barrier follows
// the table fill; blood_B is read from LDS (t is a run-time index).  Heads, the prior's LogitMvn, the Adam moments and
// the loss accumulators stay in registers across all steps of refine_generic_kernel.
//
// Per draw: elbo_bwd_generic_kernel's regrouping.  With gy_t = d nll / d yhat_t and yhat_t = sig_t / np,
//     g_oef = (1 / np) sum_t gy_t ds_t/doef - w a1 sum_window ds_t/doef,   a1 = (1 / np^2) sum_t gy_t sig_t,  w = 1 or 1/3,
// so the 1 or 3 window images give np first, then ONE pass over t gathers sum gy sig, sum gy ds/doef, sum gy ds/ddbv
// and the window's slopes: T + 1 (T + 3) table lookups per draw, no sig[T] / gy[T] arrays.  The likelihood switches
// (Student-t, log data, three-image normalisation) are wave-uniform branches on QbDev, as in draw_nll_grad.
//
// No scratch, no atomics, no cross-lane operation, no workspace (per-voxel kernel): a voxel's bits depend on its own
// inputs and its global index only -- not on the batch, its position in it, or the sharding.
namespace {

constexpr int kGenBlock = 128;
static_assert(sizeof(qb::FwdLds) % 16 == 0, "the data rows start 16-byte aligned behind FwdLds");
static_assert(sizeof(qb::FwdLds) + sizeof(float) * 2 * QB_MAX_T * kGenBlock <= 160 * 1024,
              "refine_generic_kernel: table + rows exceed the LDS");

// what a thread keeps of its voxel's likelihood side and of the protocol
struct GenVox {
    const qb::FwdLds* L;
    float* yt;   // this thread's column: yt[t * kGenBlock], is[t * kGenBlock]
    float* is;
    int T, se, w_lo, w_hi;
    float w_se, dbw, n0;
    float log_s_sum;   // per voxel (gen_load)
};

__device__ __forceinline__ GenVox gen_vox(const QbDev& c, unsigned char* smem) {
    GenVox vx;
    vx.L = reinterpret_cast<const qb::FwdLds*>(smem);
    vx.T = c.T;
    vx.se = c.se_idx;
    vx.yt = reinterpret_cast<float*>(smem + sizeof(qb::FwdLds)) + threadIdx.x;
    vx.is = vx.yt + vx.T * kGenBlock;
    // normalisation window (model.py:541-545) and the weight of each of its images
    vx.w_lo = c.multi_norm ? vx.se - 1 : vx.se;
    vx.w_hi = c.multi_norm ? vx.se + 1 : vx.se;
    vx.w_se = c.multi_norm ? 1.0f / 3.0f : 1.0f;
    vx.dbw = c.include_blood ? c.m_bld_nb : 1.0f;
    vx.n0 = c.dF_node0 / (c.tab_inv_h * c.tab_inv_h);   // node 0's slope per u^2
    vx.log_s_sum = 0.0f;
    return vx;
}

// prepare_lik<T, SE, false> of a live voxel into the thread's column
__device__ __forceinline__ void gen_load(const QbDev& c, GenVox& vx, const float* __restrict__ xv,
                                         const float* __restrict__ sv) {
    const int se = vx.se;
    const float nt = c.multi_norm ? (xv[se - 1] + xv[se] + xv[se + 1]) / 3.0f + 1e-3f : xv[se] + 1e-3f;
    const float inv_nt = qb::rcpf_(nt);
    float ls = 0.0f;
    for (int t = 0; t < vx.T; ++t) {
        float y = xv[t] * inv_nt;
        if (c.predict_log) y = __logf(y);   // model.py:548
        const float s = sv[t];
        vx.yt[t * kGenBlock] = y;
        vx.is[t * kGenBlock] = qb::rcpf_(s);
        ls += QB_LN2 * qb::log2f_(s);
    }
    vx.log_s_sum = c.use_student_t ? ls : ls + (float)vx.T * 0.9189385332046727f;   // log sqrt(2 pi)
}

struct GenSig {
    float s, tissue, blood, F, e1, e2, u, f, B;
    float4 k;
};
// fwd_signal_fast, keeping what the slopes need; blood_B from LDS.  The segment index is clamped: forward_transform
// bounds OEF by 0.84 and the table spans OEF <= 1, so the clamp never binds for finite heads and keeps a NaN or
// infinite head inside the table.
__device__ __forceinline__ GenSig gen_signal(const qb::FwdLds* L, const qb::FwdFast& v, int t) {
    GenSig g;
    g.u = fabsf(fmaf((float)t, v.ub, v.ua));
    const int i = min(max((int)g.u, 0), QB_TAB_SEG - 1);
    g.f = __builtin_amdgcn_fractf(g.u);
    g.k = L->tab[i];
    g.F = fmaf(fmaf(fmaf(g.k.w, g.f, g.k.z), g.f, g.k.y), g.f, g.k.x);
    g.e1 = qb::exp2f_(v.nd * g.F);
    g.B = L->blood_B[t];
    g.e2 = qb::exp2f_(v.ng * g.B);
    g.tissue = v.tissue_w * g.e1;
    g.blood = v.blood_w * g.e2;
    g.s = g.tissue + g.blood;
    return g;
}

// draw_nll_grad at a run-time T: one draw's NLL, and its gradient with respect to (mu_o, s_o, mu_d, s_d, c) ADDED to g
__device__ __forceinline__ float gen_draw_nll_grad(const QbDev& c, const GenVox& vx, const qb::LogitMvn& qm, float z0,
                                                   float z1, float (&g)[5]) {
    float a, b;
    qb::reparam_logits(qm, z0, z1, a, b);
    const float sa = qb::sigmoidf_(a), sb = qb::sigmoidf_(b);
    const float oef = sa * QB_OEF_RANGE + QB_MIN_OEF;
    const float dbv = sb * QB_DBV_RANGE + QB_MIN_DBV;
    const qb::FwdFast fv = qb::fwd_fast(c, oef, dbv);
    const float inv_oef = qb::rcpf_(oef);
    // se_norm on the prediction
    float np_ = gen_signal(vx.L, fv, vx.se).s;
    if (c.multi_norm) np_ = (gen_signal(vx.L, fv, vx.se - 1).s + np_ + gen_signal(vx.L, fv, vx.se + 1).s) / 3.0f;
    const float inv_np = qb::rcpf_(np_ + 1e-3f);
    // per-draw factors of the slopes (fwd_signal_grad): tissue exp(-dbv F(x)), x proportional to oef; blood
    // exp(-g B), g proportional to oef^2
    const float ko = -dbv * inv_oef, kb = (2.0f * QB_LN2) * fv.ng * inv_oef;
    const float kd1 = vx.dbw * c.e_te_r2t, kd2 = c.include_blood ? vx.dbw * c.e_r2b_te : 0.0f;
    const float df1 = c.st_df + 1.0f, inv_df = qb::rcpf_(c.st_df);
    float acc = 0.0f, a1 = 0.0f, go = 0.0f, gd = 0.0f, wo = 0.0f, wd = 0.0f;
    for (int t = 0; t < vx.T; ++t) {
        const GenSig sg = gen_signal(vx.L, fv, t);
        const float inv_s = vx.is[t * kGenBlock];
        float yp = sg.s * inv_np, dyp = 1.0f;
        if (c.predict_log) {                      // model.py:547-549 (only voxels with m > 0 are refined)
            dyp = qb::rcpf_(yp);
            yp = __logf(yp);
        }
        const float r = (vx.yt[t * kGenBlock] - yp) * inv_s;
        float dr = r;
        if (c.use_student_t) {                    // model.py:557-559
            const float w = df1 * qb::rcpf_(fmaf(r, r, c.st_df));
            acc += df1 * log1pf(r * r * inv_df) - 2.0f * c.st_const;
            dr = w * r;
        } else {
            acc = fmaf(r, r, acc);
        }
        const float gy = -dr * inv_s * dyp;       // d nll / d (sig_t / np)
        a1 = fmaf(gy, sg.s, a1);
        // |x| dF/dx at x = u / tab_inv_h (the cubic's slope in u, plus node 0's slope in x): d|x| / d oef = |x| / oef
        const float dFu = fmaf(fmaf(3.0f * sg.k.w, sg.f, 2.0f * sg.k.z), sg.f, sg.k.y) * sg.u + vx.n0 * sg.u * sg.u;
        const float ds_doef = fmaf(ko * dFu, sg.tissue, kb * sg.B * sg.blood);
        const float ds_ddbv = fmaf(kd2, sg.e2, -fmaf(sg.F, sg.tissue, kd1 * sg.e1));
        go = fmaf(gy, ds_doef, go);
        gd = fmaf(gy, ds_ddbv, gd);
        if (t >= vx.w_lo && t <= vx.w_hi) {       // wave-uniform
            wo += ds_doef;
            wd += ds_ddbv;
        }
    }
    a1 *= inv_np * inv_np * vx.w_se;              // yhat_t = sig_t / (norm + 1e-3)
    const float g_oef = fmaf(go, inv_np, -a1 * wo), g_dbv = fmaf(gd, inv_np, -a1 * wd);
    const float ga = g_oef * QB_OEF_RANGE * sa * (1.0f - sa);   // forward_transform
    const float gb = g_dbv * QB_DBV_RANGE * sb * (1.0f - sb);
    g[0] += ga;
    g[1] = fmaf(ga, z0 * qm.e_so, g[1]);
    g[2] += gb;
    g[4] = fmaf(gb, z0, g[4]);
    g[3] = fmaf(gb, z1 * qm.e_sd, g[3]);
    return fmaf(0.5f, acc, vx.log_s_sum);
}

// Step j's Monte-Carlo -ELBO at the heads qm and its gradient g with respect to (mu_o, s_o, mu_d, s_d, c):
// refine_kernel's draw loop (the same Philox words, or the same rows of z) and the closed-form KL
__device__ __forceinline__ float gen_step_grad(const QbDev& c, const GenVox& vx, const qb::LogitMvn& qm,
                                               const qb::LogitMvn& pm, const float* __restrict__ zv, uint64_t seed,
                                               uint64_t vox, int j, const RefineArgs& ra, float (&g)[5]) {
    const int S = ra.S, Sp = ra.Sp;
#pragma unroll
    for (int i = 0; i < 5; ++i) g[i] = 0.0f;
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
            nll += gen_draw_nll_grad(c, vx, qm, z0, z1, g);
        }
    }
    const float inv_S = 1.0f / (float)S;
#pragma unroll
    for (int i = 0; i < 5; ++i) g[i] *= inv_S;
    const float kl = kl_closed_grad(qm, pm, g);
    return fmaf(nll, inv_S, kl);
}

// The chain to the raw heads (transform_std / transform_offdiag, model.py:288-294: s = 3 tanh(raw) - 1,
// c = tanh(raw) e^-2), the cosine rate of step j and the Adam (b1t, b2t = beta^(j + 1)) or SGD update: refine_kernel's
// expressions
__device__ __forceinline__ void refine_update(const RefineArgs& ra, int j, float b1t, float b2t, float (&qv)[5],
                                              float (&m1)[5], float (&m2)[5], float (&g)[5]) {
    g[1] *= 3.0f * qb::sech2f_(qv[1]);
    g[3] *= 3.0f * qb::sech2f_(qv[3]);
    g[4] *= 0.1353352832366127f * qb::sech2f_(qv[4]);
    const float lr = fmaf(0.5f * (ra.lr - ra.lr_final), 1.0f + cosf((float)M_PI * ((float)j / (float)ra.steps)),
                          ra.lr_final);
    if (ra.adam) {
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

// w d TV / d (mu_o, mu_d) of voxel v at the step's heads q_src, ADDED to g[0] and g[2]: refine_tv_step_kernel's
// (smoothness_kernel's) subgradient
__device__ __forceinline__ void tv_subgrad(const TvStep& st, const float* __restrict__ mask,
                                           const float* __restrict__ q_src, int64_t v, const float (&qv)[5],
                                           float (&g)[5]) {
    const int64_t yz = (int64_t)st.gm.Y * st.gm.Z;
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

__global__ __launch_bounds__(kGenBlock) void refine_generic_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* q_in, const float* __restrict__ prior, const float* __restrict__ sigma,
    const float* __restrict__ z, RefineArgs ra, uint64_t seed, int64_t voxel0, float* q_out,
    float* __restrict__ loss, int64_t N) {
    extern __shared__ __align__(16) unsigned char smem[];
    qb::FwdLds* L = reinterpret_cast<qb::FwdLds*>(smem);
    qb::fwd_lds_fill(L, g_tab, false);
    if (threadIdx.x < QB_MAX_T) L->blood_B[threadIdx.x] = c.blood_B[threadIdx.x];
    __syncthreads();
    GenVox vx = gen_vox(c, smem);

    const int steps = ra.steps, T = vx.T;
    const int tail = (steps + 9) / 10;   // the last ceil(steps / 10) steps make loss[1]
    const int64_t ntile = (N + kGenBlock - 1) / kGenBlock;
    // no barrier inside the loop: a thread reads and writes its own column only
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t v = tile * kGenBlock + threadIdx.x;
        if (v >= N) continue;
        float qv[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) qv[i] = q_in[v * 5 + i];
        const float m = mask ? mask[v] : 1.0f;
        if (!(m > 0.0f)) {   // masked voxel: q copied through bit for bit, its data never read
#pragma unroll
            for (int i = 0; i < 5; ++i) q_out[v * 5 + i] = qv[i];
            if (loss) {
                loss[2 * v + 0] = 0.0f;
                loss[2 * v + 1] = 0.0f;
            }
            continue;
        }
        gen_load(c, vx, x + v * T, sigma + v * T);
        float pv[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) pv[i] = prior[v * 5 + i];
        const qb::LogitMvn pm = qb::make_mvn(pv);
        const uint64_t vox = (uint64_t)(voxel0 + v);
        const float* zv = z ? z + v * (int64_t)steps * ra.Sp * 2 : nullptr;

        float m1[5], m2[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) m1[i] = m2[i] = 0.0f;
        float b1t = 1.0f, b2t = 1.0f;   // beta^t of the bias correction
        float loss0 = 0.0f, loss_tail = 0.0f;
#pragma unroll 1
        for (int j = 0; j < steps; ++j) {
            const qb::LogitMvn qm = qb::make_mvn(qv);
            float g[5];
            const float lj = gen_step_grad(c, vx, qm, pm, zv, seed, vox, j, ra, g);
            if (j == 0) loss0 = lj;
            if (j >= steps - tail) loss_tail += lj;
            b1t *= ra.beta1;
            b2t *= ra.beta2;
            refine_update(ra, j, b1t, b2t, qv, m1, m2, g);
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) q_out[v * 5 + i] = qv[i];
        if (loss) {
            loss[2 * v + 0] = loss0;
            loss[2 * v + 1] = loss_tail / (float)tail;
        }
    }
}

// refine_tv_step_kernel's Jacobi step j at a run-time T: the same workspace (state [N][12], two head buffers), the
// same launch-per-step protocol of the entry below
__global__ __launch_bounds__(kGenBlock) void refine_tv_step_generic_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* q_in, const float* __restrict__ q_src, const float* __restrict__ prior,
    const float* __restrict__ sigma, const float* __restrict__ z, RefineArgs ra, TvStep st, uint64_t seed,
    int64_t voxel0, float* q_dst, float4* __restrict__ state, float* __restrict__ loss, int64_t N) {
    extern __shared__ __align__(16) unsigned char smem[];
    qb::FwdLds* L = reinterpret_cast<qb::FwdLds*>(smem);
    qb::fwd_lds_fill(L, g_tab, false);
    if (threadIdx.x < QB_MAX_T) L->blood_B[threadIdx.x] = c.blood_B[threadIdx.x];
    __syncthreads();
    GenVox vx = gen_vox(c, smem);

    const int steps = ra.steps, T = vx.T, j = st.j;
    const int tail = (steps + 9) / 10;
    const int64_t ntile = (N + kGenBlock - 1) / kGenBlock;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t v = tile * kGenBlock + threadIdx.x;
        if (v >= N) continue;
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
        float qv[5], pv[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            qv[i] = q_src[v * 5 + i];
            pv[i] = prior[v * 5 + i];
        }
        gen_load(c, vx, x + v * T, sigma + v * T);
        const qb::LogitMvn pm = qb::make_mvn(pv);
        const uint64_t vox = (uint64_t)(voxel0 + v);
        const float* zv = z ? z + v * (int64_t)steps * ra.Sp * 2 : nullptr;

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

        const qb::LogitMvn qm = qb::make_mvn(qv);
        float g[5];
        const float lj = gen_step_grad(c, vx, qm, pm, zv, seed, vox, j, ra, g);
        if (j == 0) loss0 = lj;
        if (j >= steps - tail) loss_tail += lj;
        tv_subgrad(st, mask, q_src, v, qv, g);
        refine_update(ra, j, st.b1p * ra.beta1, st.b2p * ra.beta2, qv, m1, m2, g);

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

// dynamic LDS of a block at T taus, taken by the opt-in above the 64 KiB default
template <typename K>
int gen_lds_bytes(K kernel, int T, size_t* smem) {
    *smem = sizeof(qb::FwdLds) + sizeof(float) * 2 * (size_t)T * kGenBlock;
    if (*smem > 64 * 1024)
        QB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)*smem));
    return QBOLD_OK;
}

}  // namespace

extern "C" int qbold_refine_posterior_anyt(const qbold_ctx* ctx, const float* x, const float* mask,
                                           const float* q_in, const float* prior, const float* sigma, const float* z,
                                           int steps, int S, const qbold_refine_cfg* cfg, uint64_t seed,
                                           int64_t voxel0, float* q_out, float* loss, int64_t N, void* stream) {
    int64_t Sp;
    if (const int rc = refine_check_voxels("qbold_refine_posterior_anyt", ctx, x, q_in, prior, sigma, steps, S, cfg,
                                           q_out, N, true, &Sp))
        return rc;
    if (N == 0) return QBOLD_OK;
    hipStream_t s = (hipStream_t)stream;
    const RefineArgs ra{steps, S, (int)Sp, cfg->optimizer == 0 ? 1 : 0, cfg->lr, cfg->lr_final,
                        cfg->beta1, cfg->beta2, cfg->eps};
    const int64_t ntile = (N + kGenBlock - 1) / kGenBlock;
    const int cap = 2 * qb::elbo_grid(ctx);   // 128-thread blocks: twice the 256-thread kernels' cap
    const int grid = (int)(ntile < cap ? ntile : cap);
    size_t smem;
    if (const int rc = gen_lds_bytes(refine_generic_kernel, ctx->dev.T, &smem)) return rc;
    hipLaunchKernelGGL(refine_generic_kernel, dim3(grid), dim3(kGenBlock), smem, s, ctx->dev, ctx->d_tab, x, mask, q_in,
                       prior, sigma, z, ra, seed, voxel0, q_out, loss, N);
    QB_HIP(hipGetLastError());
    return QBOLD_OK;
}

extern "C" int qbold_refine_posterior_spatial_anyt(const qbold_ctx* ctx, const float* x, const float* mask,
                                                   const float* q_in, const float* prior, const float* sigma,
                                                   const float* z, const qbold_geometry* geom, float tv_weight,
                                                   int steps, int S, const qbold_refine_cfg* cfg, uint64_t seed,
                                                   int64_t voxel0, float* q_out, float* loss, void* workspace,
                                                   void* stream) {
    int64_t Sp, N;
    if (const int rc = refine_check_volume("qbold_refine_posterior_spatial_anyt", ctx, x, q_in, prior, sigma, geom,
                                           tv_weight, steps, S, cfg, q_out, workspace, true, &Sp, &N))
        return rc;
    // no coupling: the per-voxel refinement, one launch with the state in registers (its bits by construction)
    if (tv_weight == 0.0f)
        return qbold_refine_posterior_anyt(ctx, x, mask, q_in, prior, sigma, z, steps, S, cfg, seed, voxel0, q_out,
                                           loss, N, stream);
    hipStream_t s = (hipStream_t)stream;
    const RefineArgs ra{steps, S, (int)Sp, cfg->optimizer == 0 ? 1 : 0, cfg->lr, cfg->lr_final,
                        cfg->beta1, cfg->beta2, cfg->eps};
    // workspace: qbold_refine_posterior_spatial's -- state [N][12] (16-byte rows of float4), then two head buffers [N][5]
    float4* state = (float4*)workspace;
    float* heads[2] = {(float*)workspace + N * kStateFloats, (float*)workspace + N * (kStateFloats + 5)};
    const int64_t ntile = (N + kGenBlock - 1) / kGenBlock;
    const int64_t cap = 16 * (int64_t)qb::elbo_grid(ctx);   // that entry's cap in voxels
    const int grid = (int)(ntile < cap ? ntile : cap);
    size_t smem;
    if (const int rc = gen_lds_bytes(refine_tv_step_generic_kernel, ctx->dev.T, &smem)) return rc;
    TvStep st{0, 1.0f, 1.0f, tv_weight, *geom, 0};
    for (int j = 0; j < steps; ++j) {
        st.j = j;
        st.last = j == steps - 1;
        const float* src = j == 0 ? q_in : heads[(j - 1) & 1];
        // the last step writes q_out, except a single step, which reads q_in (q_out may alias it) and is copied
        float* dst = st.last && steps > 1 ? q_out : heads[j & 1];
        hipLaunchKernelGGL(refine_tv_step_generic_kernel, dim3(grid), dim3(kGenBlock), smem, s, ctx->dev, ctx->d_tab, x,
                           mask, q_in, src, prior, sigma, z, ra, st, seed, voxel0, dst, state, loss, N);
        QB_HIP(hipGetLastError());
        st.b1p *= cfg->beta1;   // refine_generic_kernel's running products, rounded to float32 after every step
        st.b2p *= cfg->beta2;
    }
    if (steps == 1) QB_HIP(hipMemcpyAsync(q_out, heads[0], N * 5 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return QBOLD_OK;
}
