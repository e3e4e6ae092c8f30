// ppc_kernels.hip -- posterior predictive checks of the fine-tuning model on given encoder heads (model checking, not
// inference: Gelman, Meng & Stern 1996; Watanabe 2010; Vehtari, Gelman & Gabry 2017).  Per voxel, L draws theta_l ~ q
// (explicit normals or Philox stream 8), and for EACH draw and tau, in the likelihood's own space (data normalised by
// se_norm, logged when predict_log), the prediction yh_{l,t}, the residual r_{l,t} = (y_t - yh_{l,t}) / sigma_t and the
// per-tau log density log p(y_t | theta_l) (the per-tau term of sample_nll).  Folded per tau into
//   sum (yh - yh_0), sum (yh - yh_0)^2           (shifted by draw 0's prediction: mean / variance of the prediction)
//   sum (lp - lp_0), sum (lp - lp_0)^2           (shifted by draw 0's log density: the WAIC variance term)
//   running max of lp and sum e^{lp - max}       (lppd's streaming log-sum-exp, one exponential per draw and tau)
// and per draw D_l = sum_t r^2 into mean_l D_l and mean_l Q_{chi2_T}(D_l) (the Rao-Blackwellised posterior predictive
// p-value: under the Gaussian likelihood D(y_rep, theta) ~ chi2_T exactly).  The columns are qbold_hip.h's.
//
// Per-tau outputs need each tau's own residual, so sample_sq_fast's merged mirror pairs cannot be used; sample_nll's
// sharing of the tissue factor between taus that mirror exactly can, and is.
//
// Lane mapping (the choice and its reason):
//   T = 11 / 24 (ppc_kernel): one lane per voxel, as refine_kernel.  The data, the inverse sigmas and the eight
//     per-tau accumulators stay in registers (10 T + the draw's prediction); a voxel's draws run in order in one lane,
//     so no merge is needed and the results are the same bits whatever the batch.  Splitting the draws over lanes would
//     multiply the 8 T accumulators by the lane count for the merge and buy nothing at 1 M voxels, where one lane per
//     voxel already fills the machine.
//   Any other T <= 64 (ppc_generic_kernel, fast path only, as iw_fwd_generic_kernel): one wave per voxel, lanes over
//     taus (the grid kernel's layout for columns): 8 T accumulators per lane would be ~500 registers at T = 64.  The
//     spin-echo normalisers are uniform readlanes, D_l a wave reduction read back from lane 0.
// Masked sums in doubles in fixed orders (block, then one reducing block): no atomics, bitwise reproducible.
#include <cmath>

#include "elbo_core.h"
#include "qbold_ctx.h"

namespace qb {
bool elbo_fast_path(const qbold_ctx* ctx);   // elbo_kernels.hip
int elbo_grid(const qbold_ctx* ctx);
}  // namespace qb

namespace {

// qbold_normals(seed, STREAM_PPC, voxel0, L) reproduces the in-kernel predictive draws exactly.
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

// One tau's accumulators over the draws; draw 0 sets the shifts.
struct TauAcc {
    float yh0, se, se2;   // draw 0's prediction, sums of (yh - yh0) and (yh - yh0)^2
    float lp0, sd, sd2;   // draw 0's log density (without its per-tau constant), sums of (lp - lp0), (lp - lp0)^2
    float m, s;           // running max of lp and sum e^{lp - m}
    __device__ __forceinline__ void first(float yh, float lp) {
        yh0 = yh;
        lp0 = lp;
        m = lp;
        se = se2 = sd = sd2 = 0.0f;
        s = 1.0f;
    }
    __device__ __forceinline__ void add(float yh, float lp) {
        const float de = yh - yh0, dd = lp - lp0;
        se += de;
        se2 = fmaf(de, de, se2);
        sd += dd;
        sd2 = fmaf(dd, dd, sd2);
        // one exponential: the smaller of (lp, m) relative to the larger
        const float d = lp - m;
        const float e = qb::exp2f_(-fabsf(d) * QB_LOG2E);
        s = d > 0.0f ? fmaf(s, e, 1.0f) : s + e;
        m = fmaxf(m, lp);
    }
};

// log p(y_t | theta) up to its per-tau constant, from r^2: -r^2 / 2 (Gaussian) or -(df + 1) / 2 log1p(r^2 / df)
template <bool LINEAR>
__device__ __forceinline__ float lp_core(const QbDev& c, float r2) {
    if (!LINEAR && c.use_student_t) return -0.5f * (c.st_df + 1.0f) * log1pf(r2 / c.st_df);
    return -0.5f * r2;
}
// the per-tau constant: -log sigma - log sqrt(2 pi), or the Student-t log-normaliser - log sigma
template <bool LINEAR>
__device__ __forceinline__ float lp_const(const QbDev& c, float sigma) {
    if (!LINEAR && c.use_student_t) return c.st_const - logf(sigma);
    return -logf(sigma) - 0.9189385332046727f;
}
// variance of the likelihood's noise in units of sigma^2: 1, or df / (df - 2) (+inf for df <= 2)
template <bool LINEAR>
__device__ __forceinline__ float noise_var(const QbDev& c) {
    if (!LINEAR && c.use_student_t) return c.st_df > 2.0f ? c.st_df / (c.st_df - 2.0f) : INFINITY;
    return 1.0f;
}

// Q(T / 2, D / 2), the chi2_T upper tail, by its finite series: for even T  e^{-h} sum_{j < T/2} h^j / j!, for odd T
// erfc(sqrt h) + e^{-h} sum_{j < (T-1)/2} h^{j+1/2} / Gamma(j + 3/2) (h = D / 2).  The terms run forward from e^{-h}
// (each one a Poisson-like mass <= 1), so a large D underflows to 0 and nothing overflows; NaN stays NaN.
__device__ __forceinline__ float chi2_sf(int T, float D) {
    const float h = 0.5f * D;
    if (h > 1.0e4f) return 0.0f;   // Q(32, 1e4) = 0 in float32; keeps sqrt(inf) * 0 out
    const float e = __expf(-h);
    float acc, term;
    int n;
    float j0;
    if (T & 1) {
        const float rh = sqrtf(h);
        acc = erfcf(rh);
        term = e * rh * 1.1283791670955126f;   // 2 / sqrt(pi)
        n = (T - 1) >> 1;
        j0 = 1.5f;
    } else {
        acc = 0.0f;
        term = e;
        n = T >> 1;
        j0 = 1.0f;
    }
    for (int j = 0; j < n; ++j) {
        acc += term;
        term *= h / ((float)j + j0);
    }
    return fminf(acc, 1.0f);
}

struct PpcTau {   // one tau's closing values
    float mu, sd, z, lppd, pw;
};
template <bool LINEAR>
__device__ __forceinline__ PpcTau ppc_close(const QbDev& c, const TauAcc& a, float y, float sigma, int L) {
    PpcTau o;
    const float inv_l = 1.0f / (float)L, inv_l1 = 1.0f / (float)(L - 1);
    o.mu = fmaf(a.se, inv_l, a.yh0);
    const float var = fmaxf(fmaf(-a.se, a.se * inv_l, a.se2) * inv_l1, 0.0f);
    o.sd = sqrtf(fmaf(noise_var<LINEAR>(c), sigma * sigma, var));
    o.z = (y - o.mu) / o.sd;
    o.lppd = a.m + (logf(a.s) - logf((float)L)) + lp_const<LINEAR>(c, sigma);
    o.pw = fmaxf(fmaf(-a.sd, a.sd * inv_l, a.sd2) * inv_l1, 0.0f);
    return o;
}

// Masked sums as doubles (wave, block, grid: fixed orders): sum [m > 0] m elpd_waic, m p_waic, m ppp, m.
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ void block_partials4(double* red, const double (&a)[4], double* __restrict__ partials) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double s = wave_sum_d(a[k]);
        if (lane == 0) red[4 * wave + k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double s = 0.0;
        for (int w = 0; w < kWaves; ++w) s += red[4 * w + threadIdx.x];
        partials[4 * blockIdx.x + threadIdx.x] = s;
    }
}
__global__ __launch_bounds__(256) void reduce4_kernel(const double* __restrict__ partials, int nblocks,
                                                      double* __restrict__ sums) {
    __shared__ double sh[256];
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double a = 0.0;
    for (int b = lane; b < nblocks; b += 64) a += partials[4 * b + k];
    sh[threadIdx.x] = a;
    __syncthreads();
    if (lane == 0) {
        double t = 0.0;
        for (int i = 0; i < 64; ++i) t += sh[64 * k + i];
        sums[k] = t;
    }
}

__device__ __forceinline__ void store_out(float* __restrict__ o, float ppp, float dbar, float lppd, float pw,
                                          float maz) {
    o[0] = ppp;
    o[1] = dbar;
    o[2] = lppd;
    o[3] = pw;
    o[4] = lppd - pw;
    o[5] = maz;
}

// The normalised prediction of one draw (sample_nll's forward model and normalisation, each tau kept).
template <int T, int SE, bool FAST, bool LITERAL>
__device__ __forceinline__ void predict(const qb::FwdLds* L, const QbDev& c, float oef, float dbv, float (&yh)[T]) {
    float s[T];
    if constexpr (FAST) {
        const qb::FwdFast fv = qb::fwd_fast(c, oef, dbv);
#pragma unroll
        for (int t = 0; t < T; ++t) s[t] = qb::fwd_signal_fast(L, c, fv, t);
    } else {
        const qb::FwdVox fv = qb::fwd_vox(c, oef, dbv);
        if constexpr (SE >= 0) {   // a pair of taus that mirror exactly shares one tissue factor (sample_nll)
            float tis[T];
#pragma unroll
            for (int t = T - 1; t >= 0; --t) {
                const int m = (t < SE && 2 * SE - t < T) ? 2 * SE - t : 0;
                const bool mirrored = t < SE && 2 * SE - t < T && c.full_model && c.taus[m] == -c.taus[t];
                if (mirrored) tis[t] = tis[m];
                else tis[t] = qb::fwd_tissue<LITERAL>(L, c, fv, t);
                s[t] = qb::fwd_mix(c, fv, tis[t], t);
            }
        } else {
#pragma unroll
            for (int t = 0; t < T; ++t) s[t] = qb::fwd_signal<LITERAL>(L, c, fv, t);
        }
    }
    const float inv_np = 1.0f / qb::se_norm<T, SE>(c, s);
#pragma unroll
    for (int t = 0; t < T; ++t) {
        yh[t] = s[t] * inv_np;
        if (!FAST && c.predict_log) yh[t] = __logf(yh[t]);
    }
}

// T = 11 / 24: one lane per voxel.  FAST: the optimal.yaml configuration (Gaussian, linear data, table mode), the
// x-indexed table per tau; otherwise sample_nll's forward model with every likelihood switch read at run time.
template <int T, int SE, bool FAST, bool LITERAL>
__global__ __launch_bounds__(kBlock) void ppc_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* __restrict__ q, const float* __restrict__ sigma, const float* __restrict__ z, int L, uint64_t seed,
    int64_t voxel0, float* __restrict__ out, float* __restrict__ curves, double* __restrict__ partials, int64_t N) {
    __shared__ qb::FwdLds lds;
    __shared__ double red[4 * kWaves];
    qb::fwd_lds_fill(&lds, g_tab, LITERAL);
    __syncthreads();

    double acc_d[4] = {0.0, 0.0, 0.0, 0.0};
    const int64_t ntile = (N + kBlock - 1) / kBlock;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t v = tile * kBlock + threadIdx.x;
        if (v >= N) continue;
        const float m = mask ? mask[v] : 1.0f;
        if (!(m > 0.0f)) {   // mask <= 0 or NaN: NaN rows, nothing in the sums
            store_out(out + 6 * v, NAN, NAN, NAN, NAN, NAN);
            if (curves)
                for (int i = 0; i < 3 * T; ++i) curves[v * 3 * T + i] = NAN;
            continue;
        }
        float y[T], is[T];
        {
            float xv[T];
#pragma unroll
            for (int t = 0; t < T; ++t) xv[t] = x[v * T + t];
            const float inv_nt = qb::rcpf_(qb::se_norm<T, SE>(c, xv));
#pragma unroll
            for (int t = 0; t < T; ++t) {
                y[t] = xv[t] * inv_nt;
                if (!FAST && c.predict_log) y[t] = __logf(y[t]);
                is[t] = qb::rcpf_(sigma[v * T + t]);
            }
        }
        float qv[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) qv[i] = q[v * 5 + i];
        const qb::LogitMvn qm = qb::make_mvn(qv);
        const float* zv = z ? z + v * (int64_t)L * 2 : nullptr;
        const uint64_t vox = (uint64_t)(voxel0 + v);
        const bool gauss = FAST || !c.use_student_t;
        TauAcc acc[T];
        float dsum = 0.0f, psum = 0.0f;
        qb::DrawQuad dq;
#pragma unroll 1
        for (int l = 0; l < L; ++l) {
            float z0, z1;
            if (zv) {
                z0 = zv[2 * l];
                z1 = zv[2 * l + 1];
            } else {
                if ((l & 3) == 0) dq.load(seed, vox, (uint32_t)(l >> 2), qb::STREAM_PPC);
                dq.next(z0, z1);
            }
            float a, b, oef, dbv;
            qb::reparam_logits(qm, z0, z1, a, b);
            qb::forward_transform(a, b, oef, dbv);
            float yh[T];
            predict<T, SE, FAST, LITERAL>(&lds, c, oef, dbv, yh);
            float D = 0.0f;
            if (l == 0) {
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const float r = (y[t] - yh[t]) * is[t], r2 = r * r;
                    D += r2;
                    acc[t].first(yh[t], lp_core<FAST>(c, r2));
                }
            } else {
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const float r = (y[t] - yh[t]) * is[t], r2 = r * r;
                    D += r2;
                    acc[t].add(yh[t], lp_core<FAST>(c, r2));
                }
            }
            dsum += D;
            if (gauss) psum += chi2_sf(T, D);
        }
        float lppd = 0.0f, pw = 0.0f, maz = 0.0f;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const PpcTau o = ppc_close<FAST>(c, acc[t], y[t], sigma[v * T + t], L);
            lppd += o.lppd;
            pw += o.pw;
            maz = fmaxf(maz, fabsf(o.z));
            if (curves) {
                curves[(v * T + t) * 3 + 0] = o.mu;
                curves[(v * T + t) * 3 + 1] = o.sd;
                curves[(v * T + t) * 3 + 2] = o.z;
            }
        }
        const float ppp = gauss ? psum / (float)L : NAN;
        store_out(out + 6 * v, ppp, dsum / (float)L, lppd, pw, maz);
        acc_d[0] += (double)m * (double)(lppd - pw);
        acc_d[1] += (double)m * (double)pw;
        acc_d[2] += (double)m * (double)ppp;
        acc_d[3] += (double)m;
    }
    block_partials4(red, acc_d, partials);
}

__device__ __forceinline__ float readlane_f(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// Any other T <= 64 (fast path only): one wave per voxel, lane t owns tau t.
__global__ __launch_bounds__(kBlock) void ppc_generic_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* __restrict__ q, const float* __restrict__ sigma, const float* __restrict__ z, int L, uint64_t seed,
    int64_t voxel0, float* __restrict__ out, float* __restrict__ curves, double* __restrict__ partials, int64_t N) {
    __shared__ qb::FwdLds lds;
    __shared__ double red[4 * kWaves];
    qb::fwd_lds_fill(&lds, g_tab, false);
    __syncthreads();

    const int T = c.T, se = c.se_idx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool on = lane < T;
    const int t = on ? lane : T - 1;   // lanes past T mirror the last tau and add nothing
    double acc_d[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t v = (int64_t)blockIdx.x * kWaves + wave; v < N; v += (int64_t)gridDim.x * kWaves) {
        const float m = mask ? mask[v] : 1.0f;
        if (!(m > 0.0f)) {
            if (lane < 6) out[6 * v + lane] = NAN;
            if (curves && on) {
                curves[(v * T + t) * 3 + 0] = NAN;
                curves[(v * T + t) * 3 + 1] = NAN;
                curves[(v * T + t) * 3 + 2] = NAN;
            }
            continue;
        }
        const float xv = x[v * T + t], sg = sigma[v * T + t];
        const float nt = c.multi_norm
                             ? (readlane_f(xv, se - 1) + readlane_f(xv, se) + readlane_f(xv, se + 1)) / 3.0f + 1e-3f
                             : readlane_f(xv, se) + 1e-3f;
        const float y = xv * qb::rcpf_(nt), is = qb::rcpf_(sg);
        float qv[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) qv[i] = q[v * 5 + i];
        const qb::LogitMvn qm = qb::make_mvn(qv);
        const float* zv = z ? z + v * (int64_t)L * 2 : nullptr;
        const uint64_t vox = (uint64_t)(voxel0 + v);
        TauAcc acc;
        float dsum = 0.0f, psum = 0.0f;
        qb::DrawQuad dq;
        for (int l = 0; l < L; ++l) {
            float z0, z1;
            if (zv) {
                z0 = zv[2 * l];
                z1 = zv[2 * l + 1];
            } else {
                if ((l & 3) == 0) dq.load(seed, vox, (uint32_t)(l >> 2), qb::STREAM_PPC);
                dq.next(z0, z1);
            }
            float a, b, oef, dbv;
            qb::reparam_logits(qm, z0, z1, a, b);
            qb::forward_transform(a, b, oef, dbv);
            const qb::FwdFast fv = qb::fwd_fast(c, oef, dbv);
            const float st = qb::fwd_signal_fast(&lds, c, fv, t);
            const float np_ = c.multi_norm
                                  ? (readlane_f(st, se - 1) + readlane_f(st, se) + readlane_f(st, se + 1)) / 3.0f
                                  : readlane_f(st, se);
            const float yh = st * qb::rcpf_(np_ + 1e-3f);
            const float r = (y - yh) * is, r2 = r * r;
            const float D = readlane_f(qb::wave_sum(on ? r2 : 0.0f), 0);
            if (l == 0) acc.first(yh, -0.5f * r2);
            else acc.add(yh, -0.5f * r2);
            dsum += D;
            psum += chi2_sf(T, D);
        }
        const PpcTau o = ppc_close<true>(c, acc, y, sg, L);
        if (curves && on) {
            curves[(v * T + t) * 3 + 0] = o.mu;
            curves[(v * T + t) * 3 + 1] = o.sd;
            curves[(v * T + t) * 3 + 2] = o.z;
        }
        const float lppd = readlane_f(qb::wave_sum(on ? o.lppd : 0.0f), 0);
        const float pw = readlane_f(qb::wave_sum(on ? o.pw : 0.0f), 0);
        float maz = on ? fabsf(o.z) : 0.0f;
#pragma unroll
        for (int k = 32; k > 0; k >>= 1) maz = fmaxf(maz, __shfl_xor(maz, k, 64));
        maz = readlane_f(maz, 0);
        const float ppp = psum / (float)L;
        if (lane == 0) {
            store_out(out + 6 * v, ppp, dsum / (float)L, lppd, pw, maz);
            acc_d[0] += (double)m * (double)(lppd - pw);
            acc_d[1] += (double)m * (double)pw;
            acc_d[2] += (double)m * (double)ppp;
            acc_d[3] += (double)m;
        }
    }
    block_partials4(red, acc_d, partials);
}

}  // namespace

extern "C" int qbold_posterior_predictive(const qbold_ctx* ctx, const float* x, const float* mask, const float* q,
                                          const float* sigma, const float* z, int L, uint64_t seed, int64_t voxel0,
                                          float* out, float* curves, double* sums, void* workspace, int64_t N,
                                          void* stream) {
    QB_NEED_DEVICE(ctx);
    QB_REQUIRE(N >= 0 && L >= 2 && L <= (1 << 30), "qbold_posterior_predictive: need N >= 0 and 2 <= L <= 2^30");
    QB_REQUIRE(out && sums && workspace, "qbold_posterior_predictive: null out/sums/workspace");
    QB_REQUIRE(N == 0 || (x && q && sigma), "qbold_posterior_predictive: null input buffer");
    hipStream_t s = (hipStream_t)stream;
    double* partials = reinterpret_cast<double*>(workspace);
    // qbold_elbo_workspace_bytes holds 3 doubles per block of elbo_grid: 4 per block here
    const int max_grid = 3 * qb::elbo_grid(ctx) / 4;
    const bool lit = ctx->dev.tissue_mode == QBOLD_TISSUE_LITERAL;
    const bool fast = qb::elbo_fast_path(ctx);
    const int T = ctx->dev.T;
    const int64_t work = (T == 11 || T == 24) ? (N + kBlock - 1) / kBlock : (N + kWaves - 1) / kWaves;
    const int grid = (int)(work < max_grid ? (work > 0 ? work : 1) : max_grid);
#define QB_LAUNCH_PPC(TT, SE, FAST, LIT)                                                                           \
    hipLaunchKernelGGL((ppc_kernel<TT, SE, FAST, LIT>), dim3(grid), dim3(kBlock), 0, s, ctx->dev, ctx->d_tab, x,  \
                       mask, q, sigma, z, L, seed, voxel0, out, curves, partials, N)
#define QB_PPC_T(TT, SE)                                                                                           \
    do {                                                                                                           \
        const bool se_c = ctx->dev.se_idx == SE && !ctx->dev.multi_norm;                                           \
        if (fast && se_c) QB_LAUNCH_PPC(TT, SE, true, false);                                                      \
        else if (fast) QB_LAUNCH_PPC(TT, -1, true, false);                                                         \
        else if (lit && se_c) QB_LAUNCH_PPC(TT, SE, false, true);                                                  \
        else if (lit) QB_LAUNCH_PPC(TT, -1, false, true);                                                          \
        else if (se_c) QB_LAUNCH_PPC(TT, SE, false, false);                                                        \
        else QB_LAUNCH_PPC(TT, -1, false, false);                                                                  \
    } while (0)
    // the configurations of qbold_log_evidence_fwd: every likelihood switch at T = 11 / 24, the fast path otherwise
    switch (T) {
        case 11: QB_PPC_T(11, 2); break;
        case 24: QB_PPC_T(24, 7); break;
        default:
            if (!fast) {
                qb::set_error("qbold_posterior_predictive: for T other than 11 / 24 only the optimal.yaml "
                              "configuration (table mode, Gaussian likelihood, linear data) is built");
                return QBOLD_ERR_UNSUPPORTED;
            }
            hipLaunchKernelGGL(ppc_generic_kernel, dim3(grid), dim3(kBlock), 0, s, ctx->dev, ctx->d_tab, x, mask, q,
                               sigma, z, L, seed, voxel0, out, curves, partials, N);
    }
#undef QB_PPC_T
#undef QB_LAUNCH_PPC
    QB_HIP(hipGetLastError());
    hipLaunchKernelGGL(reduce4_kernel, dim3(1), dim3(256), 0, s, partials, grid, sums);
    QB_HIP(hipGetLastError());
    return QBOLD_OK;
}
