// laplace_kernels.hip -- per-voxel Laplace posteriors of the fine-tuning model: the MAP of the log-joint on the logit
// plane by Levenberg-Marquardt and the Gauss-Newton (Fisher) curvature there, on any tau grid (1 <= T <= QB_MAX_T).
// include/qbold_hip.h, qbold_laplace_posterior, states the definition (model, schedule, outputs) that the float64
// reference of the tests restates; this file is its float32 form.
//
// Shape: the any-T refinement kernels' (refine_kernels.hip), with which this file shares the signal-with-slopes
// evaluation and the per-thread LDS columns (signal_grad.h: sig_eval, slope_factors, VoxColumns) -- without node 0's
// slope, see lap_signal.  128 threads, one lane per voxel; the voxel's normalised data and 1 / sigma live in dynamic LDS
// as rows [t][thread] beside FwdLds (8 T bytes per thread: 16.8 KiB per block at T = 11, 69.8 KiB at T = 64, two blocks
// per CU).  A thread owns its column of every row, so a wave's access at a fixed t is 64 consecutive floats and no
// barrier is needed after the table fill.
//
// One evaluation = one pass over t that gathers F, g = J^T r and A = J^T J together.  The 1 or 3 images of the
// normalisation window are evaluated first, value AND slopes, so that the pass forms each row of the Jacobian directly,
//     d yhat_t / d theta = (d s_t / d theta - yhat_t d n / d theta) / (n + 1e-3),   n = mean of the window's signals,
// and squares it into A without the cancellation a regrouped sum of products would bring into the curvature; neither
// sig[t] nor a per-tau gradient is stored.  That is T + 1 (T + 3) value-and-slope evaluations per trial point.  The
// 2 x 2 solves are in registers.
//
// The iteration loop's trip count is wave-uniform (while any lane is active, at most max_iter trials); converged,
// masked and out-of-range lanes are frozen by predication, so a voxel's bits do not depend on its wave-mates, the
// batch position or the sharding.  No random stream, no atomics, no sums, no workspace.
#include <cmath>

#include "elbo_core.h"
#include "qbold_ctx.h"
#include "signal_grad.h"

namespace qb {
bool elbo_fast_path(const qbold_ctx* ctx);   // elbo_kernels.hip
int elbo_grid(const qbold_ctx* ctx);
}  // namespace qb

namespace {

constexpr int kLapBlock = 128;
static_assert(sizeof(qb::FwdLds) % 16 == 0, "the data rows start 16-byte aligned behind FwdLds");
static_assert(sizeof(qb::FwdLds) + sizeof(float) * 2 * QB_MAX_T * kLapBlock <= 160 * 1024,
              "laplace_kernel: table + rows exceed the LDS");

constexpr float kLamMin = 1e-7f, kLamMax = 1e7f;   // the bracket of lambda (qbold_hip.h)
constexpr float kTanhMax = 0.999999f;              // the heads' clamp: |tanh(raw)| <= 1 - 1e-6 (qbold_hip.h)
constexpr float kBandEps = 2.384185791015625e-7f;  // 2^-22: two float32 roundings (qbold_hip.h, the tie rule)
constexpr float kGainMin = 0.25f;                  // the gain rule (qbold_hip.h)
constexpr float kHalfLog2Pi = 0.9189385332046727f;

struct LapArgs {
    int max_iter;
    float lambda0, lambda_up, inv_lambda_down, tol;
};

// signal and its partials with respect to (OEF, DBV) at tau index t.  The table's F drops Simpson node 0 (as the float32
// reference's value does) and the slope here drops it too (SigEval::dFu alone, no n0 u^2 term), so that g is the
// gradient of the F that the acceptance test compares -- unlike the training and refinement gradients, which restate
// TF's autodiff and keep that node's slope (QbDev::dF_node0).
struct LapSig {
    float s, ds_doef, ds_ddbv;
};
struct LapPoint {
    qb::FwdFast fv;
    qb::SlopeFactors k;
};
__device__ __forceinline__ LapSig lap_signal(const qb::FwdLds* L, const LapPoint& p, int t) {
    const qb::SigEval e = qb::sig_eval(L, p.fv, t);
    LapSig g;
    g.s = e.s;
    g.ds_doef = e.ds_doef(p.k, e.dFu());
    g.ds_ddbv = e.ds_ddbv(p.k);
    return g;
}

// F, chi2, the rounding band of F, g and A (with respect to the logits) at one point
struct LapEval {
    float F, chi2, band, ga, gb, aaa, aab, abb;
};

__device__ __forceinline__ LapEval lap_eval(const QbDev& c, const qb::VoxColumns& vx, const qb::LogitMvn& pm, float a,
                                            float b) {
    const float sa = qb::sigmoidf_(a), sb = qb::sigmoidf_(b);
    const float oef = sa * QB_OEF_RANGE + QB_MIN_OEF;
    const float dbv = sb * QB_DBV_RANGE + QB_MIN_DBV;
    LapPoint p;
    p.fv = qb::fwd_fast(c, oef, dbv);
    p.k = qb::slope_factors(c, p.fv, oef, dbv, vx.dbw);
    // the normaliser n and its slopes over the window (1 or 3 images, wave-uniform)
    float ns = 0.0f, no = 0.0f, nd = 0.0f;
    for (int t = vx.w_lo; t <= vx.w_hi; ++t) {
        const LapSig g = lap_signal(vx.L, p, t);
        ns += g.s;
        no += g.ds_doef;
        nd += g.ds_ddbv;
    }
    ns *= vx.w_se;
    no *= vx.w_se;
    nd *= vx.w_se;
    const float inv_np = qb::rcpf_(ns + 1e-3f);
    float chi2 = 0.0f, band = 0.0f, so = 0.0f, sd = 0.0f, soo = 0.0f, sod = 0.0f, sdd = 0.0f;
    for (int t = 0; t < vx.T; ++t) {
        const LapSig g = lap_signal(vx.L, p, t);
        const float inv_s = vx.is[t * kLapBlock];
        const float yp = g.s * inv_np;
        const float r = (vx.yt[t * kLapBlock] - yp) * inv_s;
        const float ws = inv_np * inv_s;
        const float jo = fmaf(-yp, no, g.ds_doef) * ws;   // d yhat_t / d oef / sigma_t = -d r_t / d oef
        const float jd = fmaf(-yp, nd, g.ds_ddbv) * ws;
        chi2 = fmaf(r, r, chi2);
        band = fmaf(fabsf(r) * yp, inv_s, band);
        so = fmaf(r, jo, so);
        sd = fmaf(r, jd, sd);
        soo = fmaf(jo, jo, soo);
        sod = fmaf(jo, jd, sod);
        sdd = fmaf(jd, jd, sdd);
    }
    // forward_transform's slopes, then the prior rows w = L_p^-1 (u - mu_p)
    const float da = QB_OEF_RANGE * sa * (1.0f - sa), db = QB_DBV_RANGE * sb * (1.0f - sb);
    const float w0 = (a - pm.mu_o) * pm.i_so;
    const float w1 = fmaf(b - pm.mu_d, pm.i_sd, (a - pm.mu_o) * pm.i_bl);
    LapEval e;
    e.chi2 = chi2;
    e.F = 0.5f * (chi2 + fmaf(w0, w0, w1 * w1));
    e.band = kBandEps * (band + e.F);
    e.ga = fmaf(-da, so, fmaf(w0, pm.i_so, w1 * pm.i_bl));
    e.gb = fmaf(-db, sd, w1 * pm.i_sd);
    e.aaa = fmaf(da * da, soo, fmaf(pm.i_so, pm.i_so, pm.i_bl * pm.i_bl));
    e.aab = fmaf(da * db, sod, pm.i_bl * pm.i_sd);
    e.abb = fmaf(db * db, sdd, pm.i_sd * pm.i_sd);
    return e;
}

// det of the symmetric 2 x 2 matrix with the product's rounding error recovered (Kahan)
__device__ __forceinline__ float det2(float aaa, float aab, float abb) {
    const float w = aab * aab;
    const float e = fmaf(-aab, aab, w);
    return fmaf(aaa, abb, -w) + e;
}

// Newton decrement sqrt(g^T A^-1 g) through the Cholesky factor of A
__device__ __forceinline__ float lap_decrement(const LapEval& e) {
    const float y1sq = e.ga * e.ga / e.aaa;
    const float l22sq = det2(e.aaa, e.aab, e.abb) / e.aaa;
    const float y2 = fmaf(-e.aab / e.aaa, e.ga, e.gb);
    return sqrtf(y1sq + y2 * y2 / l22sq);
}

__device__ __forceinline__ float atanhf_(float t) { return 0.5f * (log1pf(t) - log1pf(-t)); }

__global__ __launch_bounds__(kLapBlock) void laplace_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* __restrict__ prior, const float* __restrict__ sigma, const float* __restrict__ u0, LapArgs la,
    float* __restrict__ q_out, float* __restrict__ out, int64_t N) {
    extern __shared__ __align__(16) unsigned char smem[];
    qb::FwdLds* L = reinterpret_cast<qb::FwdLds*>(smem);
    const int T = c.T, se = c.se_idx;
    // this thread's column of the two rows, set up ahead of the table fill: through vox_columns (after the fill, as the
    // refinement kernels have it, or here) the kernel comes out with one to four more address additions
    float* yt = reinterpret_cast<float*>(smem + sizeof(qb::FwdLds)) + threadIdx.x;
    float* is = yt + T * kLapBlock;
    qb::fwd_lds_fill(L, g_tab, false);
    if (threadIdx.x < QB_MAX_T) L->blood_B[threadIdx.x] = c.blood_B[threadIdx.x];
    __syncthreads();

    qb::VoxColumns vx;
    qb::vox_window(c, vx);
    vx.L = L;
    vx.yt = yt;
    vx.is = is;

    const int64_t ntile = (N + kLapBlock - 1) / kLapBlock;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t v = tile * kLapBlock + threadIdx.x;
        const bool in = v < N;
        const float m = in ? (mask ? mask[v] : 1.0f) : 0.0f;
        const bool live = m > 0.0f;   // false for NaN
        float pv[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) pv[i] = in ? prior[v * 5 + i] : 0.0f;
        const qb::LogitMvn pm = qb::make_mvn(pv);
        // the data normalised by the spin-echo image (the mean of three) + 1e-3, 1 / sigma, sum log sigma; lanes that
        // evaluate nothing hold zeros
        float ls = 0.0f;
        if (live) {
            const float* xv = x + v * T;
            const float* sv = sigma + v * T;
            const float nt = c.multi_norm ? (xv[se - 1] + xv[se] + xv[se + 1]) / 3.0f + 1e-3f : xv[se] + 1e-3f;
            const float inv_nt = qb::rcpf_(nt);
            for (int t = 0; t < T; ++t) {
                const float s = sv[t];
                yt[t * kLapBlock] = xv[t] * inv_nt;
                is[t * kLapBlock] = qb::rcpf_(s);
                ls += logf(s);
            }
        } else {
            for (int t = 0; t < T; ++t) {
                yt[t * kLapBlock] = 0.0f;
                is[t * kLapBlock] = 0.0f;
            }
        }

        // ---- Levenberg-Marquardt (qbold_hip.h states the schedule) ----
        // state at the last accepted point; before the start point is accepted F = inf so that any finite F wins
        float ua = 0.0f, ub = 0.0f, F = INFINITY, band = 0.0f, dec = INFINITY, chi2 = 0.0f;
        float ga = 0.0f, gb = 0.0f, aaa = 1.0f, aab = 0.0f, abb = 1.0f;
        float lam = la.lambda0;
        int iters = 0;
        bool act = live, conv = false;
        float ta = live ? (u0 ? u0[v * 2 + 0] : pm.mu_o) : 0.0f;
        float tb = live ? (u0 ? u0[v * 2 + 1] : pm.mu_d) : 0.0f;
        ta = qb::clampf_(ta, -QB_LOGIT_CLIP, QB_LOGIT_CLIP);
        tb = qb::clampf_(tb, -QB_LOGIT_CLIP, QB_LOGIT_CLIP);
        // trial 0 is the start point itself; trials 1 .. max_iter are the iterations
        for (int k = 0; k <= la.max_iter && __any(act); ++k) {
            const LapEval e = lap_eval(c, vx, pm, ta, tb);
            const float dt = lap_decrement(e);
            if (act) {
                if (k > 0) ++iters;
                const float bd = fmaxf(band, e.band);
                const float du_a = ta - ua, du_b = tb - ub;   // the step actually taken (after the clip)
                float dF = F - e.F;
                // the tie rule: inside the band float32 cannot order the two values of F; the reduction is then the
                // trapezoid rule on the two gradients, which keep their digits there
                if (fabsf(dF) <= bd) dF = -0.5f * fmaf(ga + e.ga, du_a, (gb + e.gb) * du_b);
                if (dF > 0.0f) {   // false for NaN
                    // the gain rule: the quadratic model's reduction along the step
                    const float pred = -fmaf(ga, du_a, gb * du_b) -
                                       0.5f * fmaf(aaa * du_a, du_a, fmaf(2.0f * aab * du_a, du_b, abb * du_b * du_b));
                    const bool good = dF >= kGainMin * pred;
                    ua = ta;
                    ub = tb;
                    F = e.F;
                    band = e.band;
                    chi2 = e.chi2;
                    dec = dt;
                    ga = e.ga;
                    gb = e.gb;
                    aaa = e.aaa;
                    aab = e.aab;
                    abb = e.abb;
                    if (k > 0) lam = good ? fmaxf(lam * la.inv_lambda_down, kLamMin) : fminf(lam * la.lambda_up, kLamMax);
                    if (dec < la.tol) {
                        act = false;
                        conv = true;
                    }
                } else {
                    lam = fminf(lam * la.lambda_up, kLamMax);
                }
            }
            // the next trial: delta = -(A + lambda diag A)^-1 g, u' = clip(u + delta)
            const float maa = fmaf(lam, aaa, aaa), mbb = fmaf(lam, abb, abb);
            const float inv_det = 1.0f / det2(maa, aab, mbb);
            ta = qb::clampf_(ua - (mbb * ga - aab * gb) * inv_det, -QB_LOGIT_CLIP, QB_LOGIT_CLIP);
            tb = qb::clampf_(ub - (maa * gb - aab * ga) * inv_det, -QB_LOGIT_CLIP, QB_LOGIT_CLIP);
        }

        if (!in) continue;
        float* ov = out + v * QBOLD_LAPLACE_OUT;
        float* qv = q_out + v * 5;
        if (!live) {
#pragma unroll
            for (int i = 0; i < QBOLD_LAPLACE_OUT; ++i) ov[i] = NAN;
#pragma unroll
            for (int i = 0; i < 5; ++i) qv[i] = pv[i];
            continue;
        }
        // ---- outputs at the last accepted point ----
        const float sa = qb::sigmoidf_(ua), sb = qb::sigmoidf_(ub);
        const float oef = sa * QB_OEF_RANGE + QB_MIN_OEF, dbv = sb * QB_DBV_RANGE + QB_MIN_DBV;
        const float da = QB_OEF_RANGE * sa * (1.0f - sa), db = QB_DBV_RANGE * sb * (1.0f - sb);
        const float det = det2(aaa, aab, abb);
        const float v_aa = abb / det, v_bb = aaa / det, v_ab = -aab / det;   // Sigma = A^-1
        const float sd_a = sqrtf(v_aa), sd_b = sqrtf(v_bb);
        const float corr = -aab / sqrtf(aaa * abb);
        // delta method: R2' = dw OEF DBV, gradient (dw DBV dOEF/da, dw OEF dDBV/db)
        const float ra = c.dw_coef * dbv * da, rb = c.dw_coef * oef * db;
        const float r2p_var = fmaf(ra * ra, v_aa, fmaf(2.0f * ra * rb, v_ab, rb * rb * v_bb));
        // raw heads: Sigma = L L^T, L = ((e^so, 0), (c, e^sd)), through the inverses of transform_std / transform_offdiag
        int flags = conv ? 0 : 1;
        if (fabsf(ua) >= QB_LOGIT_CLIP || fabsf(ub) >= QB_LOGIT_CLIP) flags |= 2;
        bool clamped = false;
        auto clamp_t = [&](float t) {
            const float tc = qb::clampf_(t, -kTanhMax, kTanhMax);
            if (!(tc == t)) clamped = true;
            return tc;
        };
        const float t_so = clamp_t((0.5f * logf(v_aa) + 1.0f) * (1.0f / 3.0f));
        const float c_raw = v_ab / sd_a;                                   // Sigma_ab / e^so
        const float t_c = clamp_t(c_raw * 7.38905609893065f);              // c e^2
        const float cc = t_c * 0.1353352832366127f;
        // the marginal variance of b survives a clamped c: e^(2 sd) = Sigma_bb - c^2 with the c that is stored
        const float t_sd = clamp_t((0.5f * logf(fmaf(-cc, cc, v_bb)) + 1.0f) * (1.0f / 3.0f));
        if (clamped) flags |= 4;
        qv[0] = ua;
        qv[1] = atanhf_(t_so);
        qv[2] = ub;
        qv[3] = atanhf_(t_sd);
        qv[4] = atanhf_(t_c);
        ov[0] = ua;
        ov[1] = ub;
        ov[2] = oef;
        ov[3] = dbv;
        ov[4] = c.dw_coef * oef * dbv;
        ov[5] = sd_a;
        ov[6] = sd_b;
        ov[7] = corr;
        ov[8] = da * sd_a;
        ov[9] = db * sd_b;
        ov[10] = sqrtf(fmaxf(r2p_var, 0.0f));
        // log p^ = J(u^) + log 2 pi - 0.5 log det A,  J = -F - sum log sigma - (T / 2) log 2 pi - log 2 pi - log det L_p
        ov[11] = -F - ls - (float)T * kHalfLog2Pi - (pm.s_o + pm.s_d) - 0.5f * logf(det);
        ov[12] = chi2;
        ov[13] = (float)iters;
        ov[14] = (float)flags;
    }
}

}  // namespace

extern "C" int qbold_laplace_posterior(const qbold_ctx* ctx, const float* x, const float* mask, const float* prior,
                                       const float* sigma, const float* u0, const qbold_laplace_cfg* cfg,
                                       float* q_out, float* out, int64_t N, void* stream) {
    QB_NEED_DEVICE(ctx);
    QB_REQUIRE(cfg, "qbold_laplace_posterior: null cfg");
    QB_REQUIRE(N >= 0, "qbold_laplace_posterior: need N >= 0");
    QB_REQUIRE(cfg->max_iter >= 1, "qbold_laplace_posterior: need max_iter >= 1");
    QB_REQUIRE(cfg->lambda0 > 0.0f && cfg->lambda0 < INFINITY, "qbold_laplace_posterior: lambda0 must be positive and finite");
    QB_REQUIRE(cfg->tol > 0.0f && cfg->tol < INFINITY, "qbold_laplace_posterior: tol must be positive and finite");
    QB_REQUIRE(cfg->lambda_up > 1.0f && cfg->lambda_up < INFINITY && cfg->lambda_down > 1.0f && cfg->lambda_down < INFINITY,
               "qbold_laplace_posterior: need finite lambda_up > 1 and lambda_down > 1");
    QB_REQUIRE(q_out && out, "qbold_laplace_posterior: null q_out/out");
    QB_REQUIRE(N == 0 || (x && prior && sigma), "qbold_laplace_posterior: null input buffer");
    if (!qb::elbo_fast_path(ctx)) {
        qb::set_error("qbold_laplace_posterior: built for the full signal model in table mode with the Gaussian "
                      "likelihood on linear data (either normalisation)");
        return QBOLD_ERR_UNSUPPORTED;
    }
    const int T = ctx->dev.T;
    QB_REQUIRE(T >= 1 && T <= QB_MAX_T, "qbold_laplace_posterior: need 1 <= T <= 64");
    if (N == 0) return QBOLD_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t ntile = (N + kLapBlock - 1) / kLapBlock;
    const int cap = 2 * qb::elbo_grid(ctx);   // 128-thread blocks: twice the 256-thread kernels' cap
    const int grid = (int)(ntile < cap ? ntile : cap);
    const size_t smem = sizeof(qb::FwdLds) + sizeof(float) * 2 * (size_t)T * kLapBlock;
    if (smem > 64 * 1024)
        QB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(laplace_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    const LapArgs la{cfg->max_iter, cfg->lambda0, cfg->lambda_up, 1.0f / cfg->lambda_down, cfg->tol};
    hipLaunchKernelGGL(laplace_kernel, dim3(grid), dim3(kLapBlock), smem, s, ctx->dev, ctx->d_tab, x, mask, prior, sigma,
                       u0, la, q_out, out, N);
    QB_HIP(hipGetLastError());
    return QBOLD_OK;
}
