// iw_kernels.hip -- importance-weighted evidence of the fine-tuning model (Burda et al. 2016), evaluation only, on
// given encoder heads (like qbold_elbo_fwd).  Per voxel, K draws z_k ~ q (explicit or from Philox stream 6) and for
// EACH draw
//   log w_k = -nll(x | y_k) - (log q(y_k) - log p(y_k))          y_k = reparameterised z_k, the same draw in both terms
// folded into a streaming log-sum-exp: a running max and, relative to it, sum e^{log w}, sum e^{2 log w} and the three
// weighted sums of theta_k = (OEF, DBV, R2').  Out per voxel:
//   log p^ = logsumexp_k log w_k - log K,   ELBO_same = mean_k log w_k,   ESS = (sum w)^2 / sum w^2,
//   E_post[theta] = sum w theta / sum w  (self-normalised)
//
// The current ELBO kernels cannot supply this: they average the NLL over the draws of stream 0 and the KL over
// other draws of stream 1, and a sum of two means is no logsumexp of per-draw joint weights.
//
// Lane mapping, per-voxel likelihood preparation, per-draw NLL and table / LDS setup are those of the ELBO kernels
// (elbo_core.h, elbo_kernels.hip): a wave owns 16 voxels, the four lanes l, l + 16, l + 32, l + 48 of a voxel split
// its draws by Philox call (call g -> draws 4 g .. 4 g + 3, lane group g & 3), and a fixed-order combine of the four
// lanes' partial log-sum-exps closes the voxel: no atomics, bitwise reproducible, independent of the sharding.
// log q - log p of a draw is the whitened form of kl_draws_fast per draw,
//   0.5 (swr_p - swr_q) + (s_o + s_d)_p - (s_o + s_d)_q,   swr_q = |z|^2, swr_p = |d + M z|^2,
// wherever the clip of the logits (model.py:393-396) does not bind -- there it is exact -- and the clipped-logit form
// (kl_swr_diff) of the ELBO kernels' general KL loop for a draw where it does.  For Philox draws the choice is made per
// wave as kl_draws_fast makes it (QB_Z_MAX bounds the normals); explicit normals are checked draw by draw.
#include <cmath>

#include "elbo_core.h"
#include "qbold_ctx.h"

namespace qb {
bool elbo_fast_path(const qbold_ctx* ctx);   // elbo_kernels.hip
int elbo_grid(const qbold_ctx* ctx);
}  // namespace qb

namespace {

// qbold_normals(seed, STREAM_IW, voxel0, K) reproduces the in-kernel importance draws exactly.
constexpr int kBlock = 256;                                  // 4 waves
constexpr int kVoxPerBlock = kBlock / QB_LANES_PER_VOXEL;    // 16 voxels per wave, 4 lanes each

template <int T, int SE, bool GT>
struct IwLds { using type = qb::FwdLds; };
template <int T, int SE>
struct IwLds<T, SE, true> { using type = qb::GtLds<T, SE>; };

// One lane's streaming log-sum-exp over its share of a voxel's draws; everything relative to the running max m.
struct IwAcc {
    float m, s1, s2, so, sd, sr, slw;
    __device__ __forceinline__ void init() {
        m = -INFINITY;
        s1 = s2 = so = sd = sr = slw = 0.0f;
    }
    __device__ __forceinline__ void add(float lw, float oef, float dbv, float r2p) {
        const float mn = fmaxf(m, lw);
        const float a = qb::exp2f_((m - mn) * QB_LOG2E);    // rescale of what is there (0 on the first draw)
        const float b = qb::exp2f_((lw - mn) * QB_LOG2E);   // this draw's weight
        s1 = fmaf(s1, a, b);
        s2 = fmaf(s2, a * a, b * b);
        so = fmaf(so, a, b * oef);
        sd = fmaf(sd, a, b * dbv);
        sr = fmaf(sr, a, b * r2p);
        slw += lw;
        m = mn;
    }
};

// log q - log p of a draw in the whitened form (see the head of the file): d + M z is the draw's residual under the
// prior, z its residual under q itself.
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

__device__ __forceinline__ float iw_dswr(const IwKl& k, float z0, float z1) {   // swr_p - swr_q of one draw
    const float w0 = fmaf(k.m00, z0, k.d0);
    const float w1 = fmaf(k.m11, z1, fmaf(k.m10, z0, k.d1));
    return fmaf(w0, w0, w1 * w1) - fmaf(z0, z0, z1 * z1);
}

// This lane's draws: Philox calls part, part + 4, ... -> draws 4 g .. 4 g + 3, the last call possibly short
// (voxel_mc_sums' walk).  zv: explicit normals [K][2] of the voxel or nullptr.
__device__ __forceinline__ int iw_lane_draws(int K, int part) {
    const int calls = K > 4 * part ? (K - 4 * part + 15) / 16 : 0;
    const int last = calls > 0 ? K - 4 * (part + 4 * (calls - 1)) : 0;
    return calls > 0 ? 4 * (calls - 1) + (last < 4 ? last : 4) : 0;
}

// The per-draw loop of the register kernel.  WHITEN: no logit of the wave's draws can reach the clip (Philox draws,
// iw_whiten), so the whitened log q - log p is exact for all of them; otherwise each draw whose logits do reach it takes
// kl_swr_diff, the clipped-logit form (explicit normals are unbounded) -- so explicit normals equal to the Philox
// stream's give the same numbers bit for bit.
template <int T, int SE, bool FAST, bool LITERAL, bool MIR, bool WHITEN, class LDS>
__device__ __forceinline__ void iw_draws(const LDS* L, const QbDev& c, const qb::VoxelLik<T>& lik,
                                         const qb::LogitMvn& q, const qb::LogitMvn& p, const IwKl& kl, int K,
                                         const float* __restrict__ zv, uint64_t seed, uint64_t vox, int part,
                                         IwAcc& acc) {
    const int n = iw_lane_draws(K, part);
    qb::DrawQuad dq;
    uint32_t g = (uint32_t)part;
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
        float z0, z1;
        if (zv) {
            const int draw = 4 * (part + 4 * (i >> 2)) + (i & 3);
            z0 = zv[2 * draw];
            z1 = zv[2 * draw + 1];
        } else {
            if ((i & 3) == 0) {
                dq.load(seed, vox, g, qb::STREAM_IW);
                g += QB_LANES_PER_VOXEL;
            }
            dq.next(z0, z1);
        }
        float a, b, oef, dbv, nll;
        qb::reparam_logits(q, z0, z1, a, b);
        if constexpr (FAST && qb::IsGtLds<LDS>::value) {
            const float sa = qb::sigmoidf_(a), sb = qb::sigmoidf_(b);
            nll = fmaf(0.5f, qb::sample_sq_fast<T, SE>(L, c, lik, sa, sb), lik.log_s_sum);
            oef = fmaf(sa, QB_OEF_RANGE, QB_MIN_OEF);
            dbv = fmaf(sb, QB_DBV_RANGE, QB_MIN_DBV);
        } else {
            qb::forward_transform(a, b, oef, dbv);
            if constexpr (FAST) nll = fmaf(0.5f, qb::sample_sq_fast<T, SE, MIR>(L, c, lik, oef, dbv), lik.log_s_sum);
            else nll = qb::sample_nll<T, SE, LITERAL>(L, c, lik, oef, dbv);
        }
        float dswr = iw_dswr(kl, z0, z1);   // swr_p - swr_q
        if (!WHITEN && fmaxf(fabsf(a), fabsf(b)) > QB_LOGIT_CLIP) dswr = qb::kl_swr_diff(q, p, z0, z1);
        acc.add(-nll - fmaf(0.5f, dswr, kl.cst), oef, dbv, (c.dw_coef * oef) * dbv);
    }
}

// Per-wave choice of the log q - log p form, as kl_draws_fast makes it: Philox draws are bounded by QB_Z_MAX, so the
// whitened form is exact while |mu| + QB_Z_MAX (|c| + e^s) stays below the logit clip for every voxel of the wave.
__device__ __forceinline__ bool iw_whiten(const qb::LogitMvn& q, const float* zv) {
    const float reach = fmaxf(fabsf(q.mu_o) + QB_Z_MAX * q.e_so, fabsf(q.mu_d) + QB_Z_MAX * (fabsf(q.c) + q.e_sd));
    return zv == nullptr && __all(reach < QB_LOGIT_CLIP);
}

// The four lanes of a voxel merged in a fixed order (max, then rescaled sums over the lane groups 16 apart) and the
// voxel's results.  Every lane of the voxel ends with the same values.
struct IwOut {
    float log_p, elbo, ess, mo, md, mr;
};
__device__ __forceinline__ IwOut iw_finish(IwAcc a, int K) {
    float M = fmaxf(a.m, __shfl_xor(a.m, 16, 64));
    M = fmaxf(M, __shfl_xor(M, 32, 64));   // finite: lane group 0 holds draw 0
    const float f = qb::exp2f_((a.m - M) * QB_LOG2E);   // 0 for a lane without draws (m = -inf)
    const float s1 = qb::voxel_sum(a.s1 * f), s2 = qb::voxel_sum(a.s2 * (f * f));
    const float so = qb::voxel_sum(a.so * f), sd = qb::voxel_sum(a.sd * f), sr = qb::voxel_sum(a.sr * f);
    const float slw = qb::voxel_sum(a.slw);
    IwOut o;
    o.log_p = M + (logf(s1) - logf((float)K));
    o.elbo = slw / (float)K;
    o.ess = (s1 * s1) / s2;
    const float inv = 1.0f / s1;
    o.mo = so * inv;
    o.md = sd * inv;
    o.mr = sr * inv;
    return o;
}

// Masked sums as doubles all the way (wave, block, grid: fixed orders), so that they equal the float64 sum of the
// per-voxel outputs: sum [m > 0] m (-log p^), sum [m > 0] m (-ELBO_same), sum m.
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

__device__ __forceinline__ void iw_store(const IwOut& o, int64_t v, float m, float* __restrict__ out,
                                         float* __restrict__ is_means, double& s_lp, double& s_el, double& s_m) {
    out[3 * v + 0] = o.log_p;
    out[3 * v + 1] = o.elbo;
    out[3 * v + 2] = o.ess;
    if (is_means) {
        is_means[3 * v + 0] = o.mo;
        is_means[3 * v + 1] = o.md;
        is_means[3 * v + 2] = o.mr;
    }
    if (m > 0.0f) {
        s_lp += (double)m * -(double)o.log_p;
        s_el += (double)m * -(double)o.elbo;
    }
    s_m += (double)m;
}

// T = 11 / 24: the data in registers, as elbo_fwd_kernel (the same template switches and the same dispatch).
template <int T, int SE, bool FAST, bool LITERAL, bool GT = false, bool MIR = false>
__global__ __launch_bounds__(kBlock) void iw_fwd_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* __restrict__ q, const float* __restrict__ prior, const float* __restrict__ sigma,
    const float* __restrict__ z, int K, uint64_t seed, int64_t voxel0, float* __restrict__ out,
    float* __restrict__ is_means, double* __restrict__ partials, int64_t N) {
    static_assert(!GT || (FAST && SE >= 0 && qb::gtab_segs(T) > 0), "GT needs the fast path with a compile-time spin echo");
    static_assert(!MIR || (FAST && SE >= 0), "merged mirror pairs: fast path with a compile-time spin echo");
    constexpr bool kMir = GT || MIR;
    using Lds = typename IwLds<T, SE, GT>::type;
    __shared__ Lds L;
    __shared__ double red[3 * (kBlock / 64)];
    if constexpr (qb::IsGtLds<Lds>::value) {
        qb::gt_lds_fill(&L, g_tab, c);
    } else {
        qb::fwd_lds_fill(&L, g_tab, true);
        if (threadIdx.x < QB_MAX_T) L.blood_B[threadIdx.x] = c.blood_B[threadIdx.x];
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int part = lane >> 4;
    double s_lp = 0.0, s_el = 0.0, s_m = 0.0;
    const int64_t ntile = (N + kVoxPerBlock - 1) / kVoxPerBlock;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t v = tile * kVoxPerBlock + wave * QB_VOX_PER_WAVE + (lane & 15);
        if (v < N) {
            float xv[T], sv[T], qv[5], pv[5];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                xv[t] = x[v * T + t];
                sv[t] = sigma[v * T + t];
            }
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                qv[i] = q[v * 5 + i];
                pv[i] = prior[v * 5 + i];
            }
            const float m = mask ? mask[v] : 1.0f;
            qb::VoxelLik<T> lik;
            qb::prepare_lik<T, SE, false, (FAST && SE >= 0), FAST, kMir>(c, xv, sv, m, lik);
            const qb::LogitMvn qm = qb::make_mvn(qv), pm = qb::make_mvn(pv);
            const IwKl kl = make_iw_kl(qm, pm);
            const float* zv = z ? z + v * (int64_t)K * 2 : nullptr;
            IwAcc acc;
            acc.init();
            const uint64_t vox = (uint64_t)(voxel0 + v);
            __builtin_amdgcn_s_setprio(QB_PRIO_LIK);
            if (iw_whiten(qm, zv))
                iw_draws<T, SE, FAST, LITERAL, kMir, true>(&L, c, lik, qm, pm, kl, K, zv, seed, vox, part, acc);
            else
                iw_draws<T, SE, FAST, LITERAL, kMir, false>(&L, c, lik, qm, pm, kl, K, zv, seed, vox, part, acc);
            __builtin_amdgcn_s_setprio(QB_PRIO_AFTER);
            // the four lanes of a voxel are active together (v depends on lane & 15 only)
            const IwOut o = iw_finish(acc, K);
            if (part == 0) iw_store(o, v, m, out, is_means, s_lp, s_el, s_m);
        }
    }
    block_partials_d(red, s_lp, s_el, s_m, partials);
}

// Any other tau count (fast path only, as elbo_fwd_generic_kernel): the normalised data and inverse sigmas in LDS
// ([t][voxel]), a run-time tau loop, mirrored pairs evaluated once when tau = 0 at the spin echo.
constexpr int kGenBlock = 128;
constexpr int kGenVox = kGenBlock / QB_LANES_PER_VOXEL;

// 0.5 sum_t r_t^2 of one draw (elbo_fwd_generic_kernel's likelihood arithmetic)
__device__ __forceinline__ float generic_half_sq(const qb::FwdLds* L, const QbDev& c, const qb::FwdFast& fv,
                                                 const float* yt, const float* is, int vl, int T, int se,
                                                 bool mirrored) {
    float acc = 0.0f;
    if (mirrored) {
        const float s_se = fmaf(fv.tissue_w, 1.0f, fv.blood_w * qb::exp2f_(fv.ng * L->blood_B[se]));
        const float inv_np = qb::rcpf_(s_se + 1e-3f);
        const float lt = qb::log2f_(fv.tissue_w * inv_np), lb = qb::log2f_(fv.blood_w * inv_np);
        auto signal = [&](int t) {
            const float u = fabsf(fmaf((float)t, fv.ub, fv.ua));
            const float4 kk = L->tab[(int)u];
            const float f = __builtin_amdgcn_fractf(u);
            const float F = fmaf(fmaf(fmaf(kk.w, f, kk.z), f, kk.y), f, kk.x);
            return qb::exp2f_(fmaf(fv.nd, F, lt)) + qb::exp2f_(fmaf(fv.ng, L->blood_B[t], lb));
        };
        auto residual = [&](int t, float yh) {
            const float r = (yt[t * kGenVox + vl] - yh) * is[t * kGenVox + vl];
            acc = fmaf(r, r, acc);
        };
        residual(se, s_se * inv_np);
        for (int t = se + 1; t < T; ++t) {
            const float yh = signal(t);
            residual(t, yh);
            if (2 * se - t >= 0) residual(2 * se - t, yh);
        }
        for (int t = 0; t < 2 * se - (T - 1); ++t) residual(t, signal(t));   // no partner on the grid
        return 0.5f * acc;
    }
    float np_ = qb::fwd_signal_fast(L, c, fv, se);
    if (c.multi_norm)
        np_ = (np_ + qb::fwd_signal_fast(L, c, fv, se - 1) + qb::fwd_signal_fast(L, c, fv, se + 1)) / 3.0f;
    const float inv_np = qb::rcpf_(np_ + 1e-3f);
    for (int t = 0; t < T; ++t) {
        const float st = qb::fwd_signal_fast(L, c, fv, t);
        const float r = fmaf(-st, inv_np, yt[t * kGenVox + vl]) * is[t * kGenVox + vl];
        acc = fmaf(r, r, acc);
    }
    return 0.5f * acc;
}

__global__ __launch_bounds__(kGenBlock) void iw_fwd_generic_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* __restrict__ q, const float* __restrict__ prior, const float* __restrict__ sigma,
    const float* __restrict__ z, int K, uint64_t seed, int64_t voxel0, float* __restrict__ out,
    float* __restrict__ is_means, double* __restrict__ partials, int64_t N) {
    extern __shared__ __align__(16) unsigned char smem[];
    qb::FwdLds* L = reinterpret_cast<qb::FwdLds*>(smem);
    float* yt = reinterpret_cast<float*>(smem + sizeof(qb::FwdLds));   // [T][kGenVox]
    float* is = yt + QB_MAX_T * kGenVox;                                // [T][kGenVox]
    __shared__ double red[3 * (kGenBlock / 64)];
    qb::fwd_lds_fill(L, g_tab, false);
    if (threadIdx.x < QB_MAX_T) L->blood_B[threadIdx.x] = c.blood_B[threadIdx.x];
    __syncthreads();

    const int T = c.T, se = c.se_idx;
    const bool mirrored = !c.multi_norm && fmaf((float)se, c.tauh_step, c.tauh0) == 0.0f;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int part = lane >> 4;
    const int vl = wave * QB_VOX_PER_WAVE + (lane & 15);
    double s_lp = 0.0, s_el = 0.0, s_m = 0.0;
    const int64_t ntile = (N + kGenVox - 1) / kGenVox;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t v = tile * kGenVox + vl;
        const bool live = v < N;
        const int64_t vc = live ? v : N - 1;
        const float* xv = x + vc * T;
        const float* sv = sigma + vc * T;
        const float nt = c.multi_norm ? (xv[se - 1] + xv[se] + xv[se + 1]) / 3.0f + 1e-3f : xv[se] + 1e-3f;
        const float inv_nt = qb::rcpf_(nt);
        float ls = 0.0f;
        __syncthreads();   // previous tile's readers are done
        for (int t = part; t < T; t += QB_LANES_PER_VOXEL) {
            yt[t * kGenVox + vl] = xv[t] * inv_nt;
            is[t * kGenVox + vl] = qb::rcpf_(sv[t]);
            ls += QB_LN2 * qb::log2f_(sv[t]);
        }
        const float log_s_sum = qb::voxel_sum(ls) + (float)T * 0.9189385332046727f;
        __syncthreads();
        if (live) {
            float qv[5], pv[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                qv[i] = q[v * 5 + i];
                pv[i] = prior[v * 5 + i];
            }
            const float m = mask ? mask[v] : 1.0f;
            const qb::LogitMvn qm = qb::make_mvn(qv), pm = qb::make_mvn(pv);
            const IwKl kl = make_iw_kl(qm, pm);
            const float* zv = z ? z + v * (int64_t)K * 2 : nullptr;
            const bool whiten = iw_whiten(qm, zv);
            const uint64_t vox = (uint64_t)(voxel0 + v);
            IwAcc acc;
            acc.init();
            const int n = iw_lane_draws(K, part);
            qb::DrawQuad dq;
            uint32_t g = (uint32_t)part;
            for (int i = 0; i < n; ++i) {
                float z0, z1;
                if (zv) {
                    const int draw = 4 * (part + 4 * (i >> 2)) + (i & 3);
                    z0 = zv[2 * draw];
                    z1 = zv[2 * draw + 1];
                } else {
                    if ((i & 3) == 0) {
                        dq.load(seed, vox, g, qb::STREAM_IW);
                        g += QB_LANES_PER_VOXEL;
                    }
                    dq.next(z0, z1);
                }
                float a, b, oef, dbv;
                qb::reparam_logits(qm, z0, z1, a, b);
                qb::forward_transform(a, b, oef, dbv);
                const qb::FwdFast fv = qb::fwd_fast(c, oef, dbv);
                const float nll = generic_half_sq(L, c, fv, yt, is, vl, T, se, mirrored) + log_s_sum;
                float dswr = iw_dswr(kl, z0, z1);
                if (!whiten && fmaxf(fabsf(a), fabsf(b)) > QB_LOGIT_CLIP) dswr = qb::kl_swr_diff(qm, pm, z0, z1);
                acc.add(-nll - fmaf(0.5f, dswr, kl.cst), oef, dbv, (c.dw_coef * oef) * dbv);
            }
            const IwOut o = iw_finish(acc, K);
            if (part == 0) iw_store(o, v, m, out, is_means, s_lp, s_el, s_m);
        }
    }
    block_partials_d(red, s_lp, s_el, s_m, partials);
}

}  // namespace

extern "C" int qbold_log_evidence_fwd(const qbold_ctx* ctx, const float* x, const float* mask, const float* q,
                                      const float* prior, const float* sigma, const float* z, int K, uint64_t seed,
                                      int64_t voxel0, float* out, float* is_means, double* sums, void* workspace,
                                      int64_t N, void* stream) {
    QB_NEED_DEVICE(ctx);
    QB_REQUIRE(N >= 0 && K >= 1 && K <= QBOLD_IW_MAX_K,
               "qbold_log_evidence_fwd: need N >= 0 and 1 <= K <= QBOLD_IW_MAX_K");
    QB_REQUIRE(out && sums && workspace, "qbold_log_evidence_fwd: null out/sums/workspace");
    QB_REQUIRE(N == 0 || (x && q && prior && sigma), "qbold_log_evidence_fwd: null input buffer");
    hipStream_t s = (hipStream_t)stream;
    double* partials = reinterpret_cast<double*>(workspace);
    const int64_t ntile = (N + kVoxPerBlock - 1) / kVoxPerBlock;
    int grid = (int)(ntile < qb::elbo_grid(ctx) ? (ntile > 0 ? ntile : 1) : qb::elbo_grid(ctx));
    const bool lit = ctx->dev.tissue_mode == QBOLD_TISSUE_LITERAL;
    const bool fast = qb::elbo_fast_path(ctx);
    const bool gt = ctx->gtab_ok && !(ctx->kernel_sel & 8) && qb::gtab_segs(ctx->dev.T) > 0;
#define QB_LAUNCH_IW(TT, SE, FAST, LIT)                                                                            \
    hipLaunchKernelGGL((iw_fwd_kernel<TT, SE, FAST, LIT>), dim3(grid), dim3(kBlock), 0, s, ctx->dev, ctx->d_tab, x, \
                       mask, q, prior, sigma, z, K, seed, voxel0, out, is_means, partials, N)
#define QB_LAUNCH_IW_MIR(TT, SE)                                                                                    \
    hipLaunchKernelGGL((iw_fwd_kernel<TT, SE, true, false, false, true>), dim3(grid), dim3(kBlock), 0, s, ctx->dev, \
                       ctx->d_tab, x, mask, q, prior, sigma, z, K, seed, voxel0, out, is_means, partials, N)
#define QB_LAUNCH_IW_GT(TT, SE)                                                                                     \
    hipLaunchKernelGGL((iw_fwd_kernel<TT, SE, true, false, (qb::gtab_segs(TT) > 0)>), dim3(grid), dim3(kBlock), 0, \
                       s, ctx->dev, ctx->d_gtab, x, mask, q, prior, sigma, z, K, seed, voxel0, out, is_means,       \
                       partials, N)
    // the dispatch of qbold_elbo_fwd (elbo_kernels.hip, elbo_fwd_launch) for the register kernels
    switch (ctx->dev.T) {
        case 11:
            if (fast && ctx->dev.se_idx == 2 && !ctx->dev.multi_norm && gt) QB_LAUNCH_IW_GT(11, 2);
            else if (fast && ctx->dev.se_idx == 2 && !ctx->dev.multi_norm && ctx->grid_mirrors) QB_LAUNCH_IW_MIR(11, 2);
            else if (fast && ctx->dev.se_idx == 2 && !ctx->dev.multi_norm) QB_LAUNCH_IW(11, 2, true, false);
            else if (fast) QB_LAUNCH_IW(11, -1, true, false);
            else if (lit && ctx->dev.se_idx == 2 && !ctx->dev.multi_norm) QB_LAUNCH_IW(11, 2, false, true);
            else if (lit) QB_LAUNCH_IW(11, -1, false, true);
            else QB_LAUNCH_IW(11, -1, false, false);
            break;
        case 24:
            if (fast && ctx->dev.se_idx == 7 && !ctx->dev.multi_norm && gt) QB_LAUNCH_IW_GT(24, 7);
            else if (fast && ctx->dev.se_idx == 7 && !ctx->dev.multi_norm && ctx->grid_mirrors) QB_LAUNCH_IW_MIR(24, 7);
            else if (fast && ctx->dev.se_idx == 7 && !ctx->dev.multi_norm) QB_LAUNCH_IW(24, 7, true, false);
            else if (fast) QB_LAUNCH_IW(24, -1, true, false);
            else if (lit && ctx->dev.se_idx == 7 && !ctx->dev.multi_norm) QB_LAUNCH_IW(24, 7, false, true);
            else if (lit) QB_LAUNCH_IW(24, -1, false, true);
            else QB_LAUNCH_IW(24, -1, false, false);
            break;
        default: {
            if (!fast) {
                qb::set_error("qbold_log_evidence_fwd: for T other than 11 / 24 only the optimal.yaml "
                              "configuration (table mode, Gaussian likelihood, linear data) is built");
                return QBOLD_ERR_UNSUPPORTED;
            }
            const int64_t gtile = (N + kGenVox - 1) / kGenVox;
            grid = (int)(gtile < qb::elbo_grid(ctx) ? (gtile > 0 ? gtile : 1) : qb::elbo_grid(ctx));
            const size_t smem = sizeof(qb::FwdLds) + sizeof(float) * 2 * QB_MAX_T * kGenVox;
            hipLaunchKernelGGL(iw_fwd_generic_kernel, dim3(grid), dim3(kGenBlock), smem, s, ctx->dev, ctx->d_tab, x,
                               mask, q, prior, sigma, z, K, seed, voxel0, out, is_means, partials, N);
        }
    }
#undef QB_LAUNCH_IW
#undef QB_LAUNCH_IW_MIR
#undef QB_LAUNCH_IW_GT
    QB_HIP(hipGetLastError());
    hipLaunchKernelGGL(qb::reduce_partials_kernel, dim3(1), dim3(192), 0, s, partials, grid, sums);
    QB_HIP(hipGetLastError());
    return QBOLD_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// qbold_log_evidence_draws: the same draws, unreduced.  The kernels above with a storing sink in place of the streaming
// log-sum-exp: same lane mapping (lane group g owns draws 4 g .. 4 g + 3 of a Philox call), per-draw arithmetic restated
// from iw_draws / iw_fwd_generic_kernel, each draw's log w and (OEF, DBV, R2') kept until its call is complete and then
// stored as one 16-byte piece of the log_w row and three of the theta row (element stores when K is no multiple of 4,
// where rows are not 16-byte aligned, and for a short last call).  Voxels with mask <= 0 (or NaN) are not read; their
// rows are NaN.  The kernels above are untouched.
namespace {

struct IwRowSink {
    float* __restrict__ lw;   // this voxel's log_w row [K]
    float* __restrict__ th;   // this voxel's theta row [K][3] or nullptr
    bool vec;                 // rows 16-byte aligned
    float l[4], t[12];        // the call's draws so far, the newest last
    __device__ __forceinline__ void push(float lwk, float oef, float dbv, float r2p) {
#pragma unroll
        for (int i = 0; i < 3; ++i) l[i] = l[i + 1];
#pragma unroll
        for (int i = 0; i < 9; ++i) t[i] = t[i + 3];
        l[3] = lwk;
        t[9] = oef;
        t[10] = dbv;
        t[11] = r2p;
    }
    // the call's first draw d0 (a multiple of 4) and how many it had: they sit in the last cnt slots
    __device__ __forceinline__ void flush(int d0, int cnt) {
        if (cnt == 4 && vec) {
            *reinterpret_cast<float4*>(lw + d0) = make_float4(l[0], l[1], l[2], l[3]);
            if (th) {
                float4* p = reinterpret_cast<float4*>(th + 3 * d0);
                p[0] = make_float4(t[0], t[1], t[2], t[3]);
                p[1] = make_float4(t[4], t[5], t[6], t[7]);
                p[2] = make_float4(t[8], t[9], t[10], t[11]);
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int d = d0 + i - (4 - cnt);
            if (i >= 4 - cnt) {
                lw[d] = l[i];
                if (th) {
                    th[3 * d + 0] = t[3 * i + 0];
                    th[3 * d + 1] = t[3 * i + 1];
                    th[3 * d + 2] = t[3 * i + 2];
                }
            }
        }
    }
};

// NaN rows of a voxel outside the mask, its four lanes taking the draws they own
__device__ __forceinline__ void iw_nan_rows(int K, int part, float* __restrict__ lw, float* __restrict__ th) {
    const float nan = __uint_as_float(0x7fc00000u);
    for (int g = part; 4 * g < K; g += QB_LANES_PER_VOXEL)
        for (int d = 4 * g; d < 4 * g + 4 && d < K; ++d) {
            lw[d] = nan;
            if (th) th[3 * d + 0] = th[3 * d + 1] = th[3 * d + 2] = nan;
        }
}

// iw_draws with the sink
template <int T, int SE, bool FAST, bool MIR, bool WHITEN, class LDS>
__device__ __forceinline__ void iw_draws_to_rows(const LDS* L, const QbDev& c, const qb::VoxelLik<T>& lik,
                                               const qb::LogitMvn& q, const qb::LogitMvn& p, const IwKl& kl, int K,
                                               const float* __restrict__ zv, uint64_t seed, uint64_t vox, int part,
                                               IwRowSink& sink) {
    const int n = iw_lane_draws(K, part);
    qb::DrawQuad dq;
    uint32_t g = (uint32_t)part;
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
        float z0, z1;
        if (zv) {
            const int draw = 4 * (part + 4 * (i >> 2)) + (i & 3);
            z0 = zv[2 * draw];
            z1 = zv[2 * draw + 1];
        } else {
            if ((i & 3) == 0) {
                dq.load(seed, vox, g, qb::STREAM_IW);
                g += QB_LANES_PER_VOXEL;
            }
            dq.next(z0, z1);
        }
        float a, b, oef, dbv, nll;
        qb::reparam_logits(q, z0, z1, a, b);
        if constexpr (FAST && qb::IsGtLds<LDS>::value) {
            const float sa = qb::sigmoidf_(a), sb = qb::sigmoidf_(b);
            nll = fmaf(0.5f, qb::sample_sq_fast<T, SE>(L, c, lik, sa, sb), lik.log_s_sum);
            oef = fmaf(sa, QB_OEF_RANGE, QB_MIN_OEF);
            dbv = fmaf(sb, QB_DBV_RANGE, QB_MIN_DBV);
        } else {
            qb::forward_transform(a, b, oef, dbv);
            if constexpr (FAST) nll = fmaf(0.5f, qb::sample_sq_fast<T, SE, MIR>(L, c, lik, oef, dbv), lik.log_s_sum);
            else nll = qb::sample_nll<T, SE, false>(L, c, lik, oef, dbv);
        }
        float dswr = iw_dswr(kl, z0, z1);   // swr_p - swr_q
        if (!WHITEN && fmaxf(fabsf(a), fabsf(b)) > QB_LOGIT_CLIP) dswr = qb::kl_swr_diff(q, p, z0, z1);
        sink.push(-nll - fmaf(0.5f, dswr, kl.cst), oef, dbv, (c.dw_coef * oef) * dbv);
        if ((i & 3) == 3 || i == n - 1) sink.flush(4 * (part + 4 * (i >> 2)), (i & 3) + 1);
    }
}

// T = 11 / 24: iw_fwd_kernel's template switches and dispatch (table mode only)
template <int T, int SE, bool FAST, bool GT = false, bool MIR = false>
__global__ __launch_bounds__(kBlock) void iw_draws_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* __restrict__ q, const float* __restrict__ prior, const float* __restrict__ sigma,
    const float* __restrict__ z, int K, uint64_t seed, int64_t voxel0, float* __restrict__ log_w,
    float* __restrict__ theta, bool vec, int64_t N) {
    static_assert(!GT || (FAST && SE >= 0 && qb::gtab_segs(T) > 0), "GT needs the fast path with a compile-time spin echo");
    static_assert(!MIR || (FAST && SE >= 0), "merged mirror pairs: fast path with a compile-time spin echo");
    constexpr bool kMir = GT || MIR;
    using Lds = typename IwLds<T, SE, GT>::type;
    __shared__ Lds L;
    if constexpr (qb::IsGtLds<Lds>::value) {
        qb::gt_lds_fill(&L, g_tab, c);
    } else {
        qb::fwd_lds_fill(&L, g_tab, true);
        if (threadIdx.x < QB_MAX_T) L.blood_B[threadIdx.x] = c.blood_B[threadIdx.x];
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int part = lane >> 4;
    const int64_t ntile = (N + kVoxPerBlock - 1) / kVoxPerBlock;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t v = tile * kVoxPerBlock + wave * QB_VOX_PER_WAVE + (lane & 15);
        if (v >= N) continue;
        IwRowSink sink = {};
        sink.lw = log_w + v * K;
        sink.th = theta ? theta + v * K * 3 : nullptr;
        sink.vec = vec;
        const float m = mask ? mask[v] : 1.0f;
        if (!(m > 0.0f)) {
            iw_nan_rows(K, part, sink.lw, sink.th);
            continue;
        }
        float xv[T], sv[T], qv[5], pv[5];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            xv[t] = x[v * T + t];
            sv[t] = sigma[v * T + t];
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            qv[i] = q[v * 5 + i];
            pv[i] = prior[v * 5 + i];
        }
        qb::VoxelLik<T> lik;
        qb::prepare_lik<T, SE, false, (FAST && SE >= 0), FAST, kMir>(c, xv, sv, m, lik);
        const qb::LogitMvn qm = qb::make_mvn(qv), pm = qb::make_mvn(pv);
        const IwKl kl = make_iw_kl(qm, pm);
        const float* zv = z ? z + v * (int64_t)K * 2 : nullptr;
        const uint64_t vox = (uint64_t)(voxel0 + v);
        // the choice is per wave over its voxels inside the mask; a draw that the whitened form covers has the same
        // bits in both loops, so a voxel's rows do not depend on its neighbours
        if (iw_whiten(qm, zv))
            iw_draws_to_rows<T, SE, FAST, kMir, true>(&L, c, lik, qm, pm, kl, K, zv, seed, vox, part, sink);
        else
            iw_draws_to_rows<T, SE, FAST, kMir, false>(&L, c, lik, qm, pm, kl, K, zv, seed, vox, part, sink);
    }
}

// Any other tau count: iw_fwd_generic_kernel with the sink
__global__ __launch_bounds__(kGenBlock) void iw_draws_generic_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* __restrict__ q, const float* __restrict__ prior, const float* __restrict__ sigma,
    const float* __restrict__ z, int K, uint64_t seed, int64_t voxel0, float* __restrict__ log_w,
    float* __restrict__ theta, bool vec, int64_t N) {
    extern __shared__ __align__(16) unsigned char smem[];
    qb::FwdLds* L = reinterpret_cast<qb::FwdLds*>(smem);
    float* yt = reinterpret_cast<float*>(smem + sizeof(qb::FwdLds));   // [T][kGenVox]
    float* is = yt + QB_MAX_T * kGenVox;                                // [T][kGenVox]
    qb::fwd_lds_fill(L, g_tab, false);
    if (threadIdx.x < QB_MAX_T) L->blood_B[threadIdx.x] = c.blood_B[threadIdx.x];
    __syncthreads();

    const int T = c.T, se = c.se_idx;
    const bool mirrored = !c.multi_norm && fmaf((float)se, c.tauh_step, c.tauh0) == 0.0f;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int part = lane >> 4;
    const int vl = wave * QB_VOX_PER_WAVE + (lane & 15);
    const int64_t ntile = (N + kGenVox - 1) / kGenVox;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t v = tile * kGenVox + vl;
        const bool inb = v < N;
        const float m = inb ? (mask ? mask[v] : 1.0f) : 0.0f;
        const bool live = m > 0.0f;
        const int64_t vc = inb ? v : N - 1;
        const float* xv = x + vc * T;
        const float* sv = sigma + vc * T;
        float ls = 0.0f;
        __syncthreads();   // previous tile's readers are done
        if (live) {
            const float nt = c.multi_norm ? (xv[se - 1] + xv[se] + xv[se + 1]) / 3.0f + 1e-3f : xv[se] + 1e-3f;
            const float inv_nt = qb::rcpf_(nt);
            for (int t = part; t < T; t += QB_LANES_PER_VOXEL) {
                yt[t * kGenVox + vl] = xv[t] * inv_nt;
                is[t * kGenVox + vl] = qb::rcpf_(sv[t]);
                ls += QB_LN2 * qb::log2f_(sv[t]);
            }
        }
        const float log_s_sum = qb::voxel_sum(ls) + (float)T * 0.9189385332046727f;
        __syncthreads();
        if (inb && !live) iw_nan_rows(K, part, log_w + v * K, theta ? theta + v * K * 3 : nullptr);
        if (live) {
            float qv[5], pv[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                qv[i] = q[v * 5 + i];
                pv[i] = prior[v * 5 + i];
            }
            const qb::LogitMvn qm = qb::make_mvn(qv), pm = qb::make_mvn(pv);
            const IwKl kl = make_iw_kl(qm, pm);
            const float* zv = z ? z + v * (int64_t)K * 2 : nullptr;
            const bool whiten = iw_whiten(qm, zv);
            const uint64_t vox = (uint64_t)(voxel0 + v);
            IwRowSink sink = {};
            sink.lw = log_w + v * K;
            sink.th = theta ? theta + v * K * 3 : nullptr;
            sink.vec = vec;
            const int n = iw_lane_draws(K, part);
            qb::DrawQuad dq;
            uint32_t g = (uint32_t)part;
            for (int i = 0; i < n; ++i) {
                float z0, z1;
                if (zv) {
                    const int draw = 4 * (part + 4 * (i >> 2)) + (i & 3);
                    z0 = zv[2 * draw];
                    z1 = zv[2 * draw + 1];
                } else {
                    if ((i & 3) == 0) {
                        dq.load(seed, vox, g, qb::STREAM_IW);
                        g += QB_LANES_PER_VOXEL;
                    }
                    dq.next(z0, z1);
                }
                float a, b, oef, dbv;
                qb::reparam_logits(qm, z0, z1, a, b);
                qb::forward_transform(a, b, oef, dbv);
                const qb::FwdFast fv = qb::fwd_fast(c, oef, dbv);
                const float nll = generic_half_sq(L, c, fv, yt, is, vl, T, se, mirrored) + log_s_sum;
                float dswr = iw_dswr(kl, z0, z1);
                if (!whiten && fmaxf(fabsf(a), fabsf(b)) > QB_LOGIT_CLIP) dswr = qb::kl_swr_diff(qm, pm, z0, z1);
                sink.push(-nll - fmaf(0.5f, dswr, kl.cst), oef, dbv, (c.dw_coef * oef) * dbv);
                if ((i & 3) == 3 || i == n - 1) sink.flush(4 * (part + 4 * (i >> 2)), (i & 3) + 1);
            }
        }
    }
}

}  // namespace

extern "C" int qbold_log_evidence_draws(const qbold_ctx* ctx, const float* x, const float* mask, const float* q,
                                        const float* prior, const float* sigma, const float* z, int K, uint64_t seed,
                                        int64_t voxel0, float* log_w, float* theta, int64_t N, void* stream) {
    QB_NEED_DEVICE(ctx);
    QB_REQUIRE(N >= 0 && K >= 1 && K <= QBOLD_IW_MAX_K,
               "qbold_log_evidence_draws: need N >= 0 and 1 <= K <= QBOLD_IW_MAX_K");
    QB_REQUIRE(log_w, "qbold_log_evidence_draws: null log_w");
    QB_REQUIRE(N == 0 || (x && q && prior && sigma), "qbold_log_evidence_draws: null input buffer");
    hipStream_t s = (hipStream_t)stream;
    const bool fast = qb::elbo_fast_path(ctx);
    if (ctx->dev.tissue_mode == QBOLD_TISSUE_LITERAL || (!fast && ctx->dev.T != 11 && ctx->dev.T != 24)) {
        qb::set_error("qbold_log_evidence_draws: built for table mode; for T other than 11 / 24 only the optimal.yaml "
                      "configuration (Gaussian likelihood, linear data)");
        return QBOLD_ERR_UNSUPPORTED;
    }
    if (N == 0) return QBOLD_OK;
    const bool vec = (K & 3) == 0 && (reinterpret_cast<uintptr_t>(log_w) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(theta) & 15) == 0;
    const int64_t ntile = (N + kVoxPerBlock - 1) / kVoxPerBlock;
    int grid = (int)(ntile < qb::elbo_grid(ctx) ? ntile : qb::elbo_grid(ctx));
    const bool gt = ctx->gtab_ok && !(ctx->kernel_sel & 8) && qb::gtab_segs(ctx->dev.T) > 0;
#define QB_LAUNCH_DRAWS(TT, SE, FAST, GT, MIR, TAB)                                                                   \
    hipLaunchKernelGGL((iw_draws_kernel<TT, SE, FAST, GT, MIR>), dim3(grid), dim3(kBlock), 0, s, ctx->dev, TAB, x,    \
                       mask, q, prior, sigma, z, K, seed, voxel0, log_w, theta, vec, N)
    // the dispatch of qbold_log_evidence_fwd, table mode
    switch (ctx->dev.T) {
        case 11:
            if (fast && ctx->dev.se_idx == 2 && !ctx->dev.multi_norm && gt)
                QB_LAUNCH_DRAWS(11, 2, true, (qb::gtab_segs(11) > 0), false, ctx->d_gtab);
            else if (fast && ctx->dev.se_idx == 2 && !ctx->dev.multi_norm && ctx->grid_mirrors)
                QB_LAUNCH_DRAWS(11, 2, true, false, true, ctx->d_tab);
            else if (fast && ctx->dev.se_idx == 2 && !ctx->dev.multi_norm) QB_LAUNCH_DRAWS(11, 2, true, false, false, ctx->d_tab);
            else if (fast) QB_LAUNCH_DRAWS(11, -1, true, false, false, ctx->d_tab);
            else QB_LAUNCH_DRAWS(11, -1, false, false, false, ctx->d_tab);
            break;
        case 24:
            if (fast && ctx->dev.se_idx == 7 && !ctx->dev.multi_norm && gt)
                QB_LAUNCH_DRAWS(24, 7, true, (qb::gtab_segs(24) > 0), false, ctx->d_gtab);
            else if (fast && ctx->dev.se_idx == 7 && !ctx->dev.multi_norm && ctx->grid_mirrors)
                QB_LAUNCH_DRAWS(24, 7, true, false, true, ctx->d_tab);
            else if (fast && ctx->dev.se_idx == 7 && !ctx->dev.multi_norm) QB_LAUNCH_DRAWS(24, 7, true, false, false, ctx->d_tab);
            else if (fast) QB_LAUNCH_DRAWS(24, -1, true, false, false, ctx->d_tab);
            else QB_LAUNCH_DRAWS(24, -1, false, false, false, ctx->d_tab);
            break;
        default: {
            const int64_t gtile = (N + kGenVox - 1) / kGenVox;
            grid = (int)(gtile < qb::elbo_grid(ctx) ? gtile : qb::elbo_grid(ctx));
            const size_t smem = sizeof(qb::FwdLds) + sizeof(float) * 2 * QB_MAX_T * kGenVox;
            hipLaunchKernelGGL(iw_draws_generic_kernel, dim3(grid), dim3(kGenBlock), smem, s, ctx->dev, ctx->d_tab, x,
                               mask, q, prior, sigma, z, K, seed, voxel0, log_w, theta, vec, N);
        }
    }
#undef QB_LAUNCH_DRAWS
    QB_HIP(hipGetLastError());
    return QBOLD_OK;
}
