// adapt_kernels.hip -- adaptive importance sampling per voxel by moment matching (Paananen, Piironen, Buerkner & Vehtari
// 2021, "Implicitly adaptive importance sampling"; the population Monte Carlo family): draw from q, weight the draws,
// replace q's mean and covariance by the weighted ones, repeat -- the forward-KL (mass covering) projection that a
// proposal wants.  One launch runs all rounds, because round r + 1's proposal depends on round r's weights.
//
// The algorithm (qbold_adapt_posterior; tests/_adapt_reference.py restates it in float64).  Per voxel with mask > 0, the
// proposal q_0 is the given heads; rounds r = 0 .. R - 1 of K draws each (K a multiple of 4).
//   Draws.  z_k of round r is draw r K + k of the voxel's Philox stream STREAM_ADAPT = 9 (qbold_normals(seed, 9, voxel0 +
//     i, R K) reproduces them), or row r K + k of explicit normals z [N][R K][2].  A round is K / 4 whole Philox calls;
//     round r's call g is call r K / 4 + g of the stream and goes to lane group g & 3.
//   Weight.  log w_k = -nll(x | y_k) - (log q_r(y_k) - log p(y_k)), y_k the reparameterised draw: qbold_log_evidence_fwd's
//     log-weight under the round's proposal.  log q - log p is the whitened form 0.5 (|d + M z|^2 - |z|^2) + const where
//     the clip of the logits at +-13.8155 cannot bind, and the clipped-logit form (kl_swr_diff) for a draw where it does.
//     The form is chosen PER VOXEL and per round from the round's own reach bound |mu| + QB_Z_MAX (|c| + e^s) (explicit
//     normals: draw by draw), never per wave, so a voxel's bits do not depend on its neighbours.
//   Statistics.  log p^_r = logsumexp_k log w_k - log K, ESS_r = (sum w)^2 / sum w^2, by the streaming log-sum-exp and
//     the fixed-order four-lane merge of iw_kernels.hip (IwAcc / iw_finish).
//   Weighted moments, in z-space, where they are O(1) (in logit space sum w u u^T - m m^T cancels in float32 once
//     |mu| ~ 13 and sd ~ e^-4): m_z = sum w~ z, C_z = sum w~ z z^T - m_z m_z^T, from five running sums (w z0, w z1, w z0^2,
//     w z0 z1, w z1^2) carried through the same rescaling as sum w.
//   Update: to the moments of the mixture (1 - lambda) q_r + lambda (weighted sample), lambda = ESS_r / (ESS_r + shrink):
//       B = (1 - lambda) I + lambda C_z + lambda (1 - lambda) m_z m_z^T,   G = chol(B) (lower; B is positive definite),
//       mu <- mu + lambda L m_z,   L <- L G,   L = ((e^s_o, 0), (c, e^s_d)).
//   The next proposal is carried as (mu, the tanh-domain values of s_o, s_d, c) after laplace_kernel's clamp rule: every
//     tanh value clamped to |tanh| <= 1 - 1e-6 (flag bit 4), e^(2 s_d) re-formed as Sigma_bb - c^2 with the c that is kept
//     when c was clamped (the marginal variance of the DBV logit survives), the means clamped to +-QB_LOGIT_CLIP (flag
//     bit 2 when one reaches it).  Every round's proposal is thus a member of the family; LogitMvn is built directly from
//     those values, and atanh happens only where heads are written.  Round 0's proposal is the given heads themselves
//     (make_mvn, unclamped), and its row of q_rounds / q_out is the given row bit for bit.
//   Non-finite weights.  A round whose sum w is 0 or not finite (or whose update would not be finite) leaves the proposal
//     unchanged and sets flag bit 1; its ESS is NaN and never the largest.
//   Returned: the proposal of the round with the largest ESS_r, the earliest one on ties -- R evaluations, R - 1 updates,
//     so a good starting q cannot be made worse on the draws that were seen.
//   Outputs.  q_out [N][5] raw heads; out [N][2 R + 2] = (log p^_r, ESS_r) per round, the returned round's index, the
//     flags (1 a round skipped, 2 a mean on the clip, 4 a spread head clamped; as floats); q_rounds [N][R][5] (nullable)
//     every round's proposal as raw heads.  Voxels with mask <= 0 or NaN are not read: q_out is the given row, out and
//     q_rounds rows are NaN.
//
// Shape: iw_fwd_generic_kernel's.  128 threads, 32 voxels per block, four lanes per voxel; normalised data and 1 / sigma
// as [t][voxel] rows in dynamic LDS beside FwdLds (filled once per voxel tile, reused by all R rounds), blood_B from LDS;
// per draw generic_half_sq's arithmetic with its merged mirror pairs when tau = 0 sits at the spin echo.  Per lane in
// registers: the proposal, its IwKl, the running sums and the best round so far.  After each merge the four lanes of a
// voxel hold the same proposal (voxel_sum is symmetric), so no LDS exchange is needed; R and K are wave uniform.  No
// atomics, no workspace, no masked sums.
//
// IwKl / make_iw_kl / iw_dswr and generic_half_sq are restated from iw_kernels.hip (as loo_kernels.hip and
// calibration_kernels.hip restate them): that file's generated code is pinned bit for bit by the log-evidence, PSIS and
// LOO tests, and moving its helpers into a header would re-inline them there.
#include <cmath>

#include "elbo_core.h"
#include "qbold_ctx.h"

namespace qb {
bool elbo_fast_path(const qbold_ctx* ctx);   // elbo_kernels.hip
int elbo_grid(const qbold_ctx* ctx);
}  // namespace qb

namespace {

constexpr int kAdBlock = 128;
constexpr int kAdVox = kAdBlock / QB_LANES_PER_VOXEL;   // 32 voxels per block, 16 per wave
constexpr float kTanhMax = 0.999999f;                   // laplace_kernel's clamp of the heads
constexpr float kE2 = 7.38905609893065f, kEm2 = 0.1353352832366127f;
constexpr float kHalfLog2Pi = 0.9189385332046727f;

// a proposal as it is carried between rounds
struct AdProp {
    float mu_o, mu_d, t_so, t_sd, t_c;   // means and tanh-domain values
};

// make_mvn from the tanh values
__device__ __forceinline__ qb::LogitMvn ad_mvn(const AdProp& p) {
    qb::LogitMvn m;
    m.mu_o = p.mu_o;
    m.mu_d = p.mu_d;
    m.s_o = p.t_so * 3.0f - 1.0f;
    m.s_d = p.t_sd * 3.0f - 1.0f;
    m.c = p.t_c * kEm2;
    m.e_so = __expf(m.s_o);
    m.e_sd = __expf(m.s_d);
    m.i_so = __expf(-m.s_o);
    m.i_sd = __expf(-m.s_d);
    m.i_bl = __expf(-m.s_o - m.s_d) * m.c * -1.0f;
    return m;
}

__device__ __forceinline__ float ad_atanh(float t) { return 0.5f * (log1pf(t) - log1pf(-t)); }

__device__ __forceinline__ void ad_write_heads(const AdProp& p, float* __restrict__ dst) {
    dst[0] = p.mu_o;
    dst[1] = ad_atanh(p.t_so);
    dst[2] = p.mu_d;
    dst[3] = ad_atanh(p.t_sd);
    dst[4] = ad_atanh(p.t_c);
}

// iw_kernels.hip: log q - log p of a draw in the whitened form
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

// iw_kernels.hip, generic_half_sq: 0.5 sum_t r_t^2 of one draw
__device__ __forceinline__ float ad_half_sq(const qb::FwdLds* L, const QbDev& c, const qb::FwdFast& fv, const float* yt,
                                            const float* is, int vl, int T, int se, bool mirrored) {
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
            const float r = (yt[t * kAdVox + vl] - yh) * is[t * kAdVox + vl];
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
        const float r = fmaf(-st, inv_np, yt[t * kAdVox + vl]) * is[t * kAdVox + vl];
        acc = fmaf(r, r, acc);
    }
    return 0.5f * acc;
}

// One lane's share of a round: IwAcc's streaming log-sum-exp (m, s1, s2: the same arithmetic) and, through the same
// rescaling, the five weighted sums of the normals.
struct AdAcc {
    float m, s1, s2, a0, a1, b00, b01, b11;
    __device__ __forceinline__ void init() {
        m = -INFINITY;
        s1 = s2 = a0 = a1 = b00 = b01 = b11 = 0.0f;
    }
    __device__ __forceinline__ void add(float lw, float z0, float z1) {
        const float mn = fmaxf(m, lw);
        const float a = qb::exp2f_((m - mn) * QB_LOG2E);    // rescale of what is there (0 on the first draw)
        const float b = qb::exp2f_((lw - mn) * QB_LOG2E);   // this draw's weight
        const float bz0 = b * z0, bz1 = b * z1;
        s1 = fmaf(s1, a, b);
        s2 = fmaf(s2, a * a, b * b);
        a0 = fmaf(a0, a, bz0);
        a1 = fmaf(a1, a, bz1);
        b00 = fmaf(b00, a, bz0 * z0);
        b01 = fmaf(b01, a, bz0 * z1);
        b11 = fmaf(b11, a, bz1 * z1);
        m = mn;
    }
};

// iw_finish's merge of the four lanes of a voxel; every lane ends with the same values
struct AdRound {
    float log_p, ess, s1, m0, m1, c00, c01, c11;
};
__device__ __forceinline__ AdRound ad_finish(const AdAcc& a, int K) {
    float M = fmaxf(a.m, __shfl_xor(a.m, 16, 64));
    M = fmaxf(M, __shfl_xor(M, 32, 64));
    const float f = qb::exp2f_((a.m - M) * QB_LOG2E);   // 0 for a lane without draws (m = -inf)
    const float s1 = qb::voxel_sum(a.s1 * f), s2 = qb::voxel_sum(a.s2 * (f * f));
    const float a0 = qb::voxel_sum(a.a0 * f), a1 = qb::voxel_sum(a.a1 * f);
    const float b00 = qb::voxel_sum(a.b00 * f), b01 = qb::voxel_sum(a.b01 * f), b11 = qb::voxel_sum(a.b11 * f);
    AdRound o;
    o.log_p = M + (logf(s1) - logf((float)K));
    o.ess = (s1 * s1) / s2;
    o.s1 = s1;
    const float inv = 1.0f / s1;
    o.m0 = a0 * inv;
    o.m1 = a1 * inv;
    o.c00 = fmaf(-o.m0, o.m0, b00 * inv);
    o.c01 = fmaf(-o.m0, o.m1, b01 * inv);
    o.c11 = fmaf(-o.m1, o.m1, b11 * inv);
    return o;
}

// The update (head of the file).  Returns false, with the proposal untouched, when the result would not be finite.
__device__ __forceinline__ bool ad_update(AdProp& p, const qb::LogitMvn& q, const AdRound& r, float shrink, int& flags) {
    const float lam = r.ess / (r.ess + shrink);
    const float om = 1.0f - lam, lo = lam * om;
    const float B00 = om + fmaf(lam, r.c00, lo * (r.m0 * r.m0));
    const float B01 = fmaf(lam, r.c01, lo * (r.m0 * r.m1));
    const float B11 = om + fmaf(lam, r.c11, lo * (r.m1 * r.m1));
    const float g00 = sqrtf(B00);
    const float g10 = B01 / g00;
    const float g11 = sqrtf(fmaf(-g10, g10, B11));
    if (!(g00 > 0.0f && g00 < INFINITY && g11 > 0.0f && g11 < INFINITY)) return false;
    float mu_o = fmaf(lam, q.e_so * r.m0, q.mu_o);
    float mu_d = fmaf(lam, fmaf(q.c, r.m0, q.e_sd * r.m1), q.mu_d);
    const float s_o = q.s_o + logf(g00);
    const float s_d = q.s_d + logf(g11);
    const float c = fmaf(q.c, g00, q.e_sd * g10);
    if (!(fabsf(mu_o) < INFINITY && fabsf(mu_d) < INFINITY && fabsf(c) < INFINITY)) return false;
    mu_o = qb::clampf_(mu_o, -QB_LOGIT_CLIP, QB_LOGIT_CLIP);
    mu_d = qb::clampf_(mu_d, -QB_LOGIT_CLIP, QB_LOGIT_CLIP);
    if (fabsf(mu_o) >= QB_LOGIT_CLIP || fabsf(mu_d) >= QB_LOGIT_CLIP) flags |= 2;
    bool clamped = false;
    auto clamp_t = [&](float t) {
        const float tc = qb::clampf_(t, -kTanhMax, kTanhMax);
        if (!(tc == t)) clamped = true;
        return tc;
    };
    const float t_so = clamp_t((s_o + 1.0f) * (1.0f / 3.0f));
    const float tc_raw = c * kE2;
    const float t_c = clamp_t(tc_raw);
    float sd_kept = s_d;
    if (!(t_c == tc_raw)) {   // the marginal variance of b survives a clamped c
        const float cc = t_c * kEm2;
        const float e2 = __expf(2.0f * s_d);
        sd_kept = 0.5f * logf(fmaf(c, c, e2) - cc * cc);
    }
    const float t_sd = clamp_t((sd_kept + 1.0f) * (1.0f / 3.0f));
    if (clamped) flags |= 4;
    p.mu_o = mu_o;
    p.mu_d = mu_d;
    p.t_so = t_so;
    p.t_sd = t_sd;
    p.t_c = t_c;
    return true;
}

struct AdArgs {
    int R, K;
    float shrink;
};

__global__ __launch_bounds__(kAdBlock) void adapt_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* __restrict__ q, const float* __restrict__ prior, const float* __restrict__ sigma,
    const float* __restrict__ z, AdArgs aa, uint64_t seed, int64_t voxel0, float* __restrict__ q_out,
    float* __restrict__ out, float* __restrict__ q_rounds, int64_t N) {
    extern __shared__ __align__(16) unsigned char smem[];
    qb::FwdLds* L = reinterpret_cast<qb::FwdLds*>(smem);
    float* yt = reinterpret_cast<float*>(smem + sizeof(qb::FwdLds));   // [T][kAdVox]
    float* is = yt + QB_MAX_T * kAdVox;                                 // [T][kAdVox]
    qb::fwd_lds_fill(L, g_tab, false);
    if (threadIdx.x < QB_MAX_T) L->blood_B[threadIdx.x] = c.blood_B[threadIdx.x];
    __syncthreads();

    const int T = c.T, se = c.se_idx;
    const int R = aa.R, K = aa.K;
    const int calls = K >> 2;                 // Philox calls per round
    const int ncol = 2 * R + 2;
    const bool mirrored = !c.multi_norm && fmaf((float)se, c.tauh_step, c.tauh0) == 0.0f;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int part = lane >> 4;
    const int vl = wave * QB_VOX_PER_WAVE + (lane & 15);
    const float nan = __uint_as_float(0x7fc00000u);
    const int64_t ntile = (N + kAdVox - 1) / kAdVox;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t v = tile * kAdVox + vl;
        const bool inb = v < N;
        const float m = inb ? (mask ? mask[v] : 1.0f) : 0.0f;
        const bool live = m > 0.0f;   // false for NaN
        float ls = 0.0f;
        __syncthreads();   // previous tile's readers are done
        if (live) {
            const float* xv = x + v * T;
            const float* sv = sigma + v * T;
            const float nt = c.multi_norm ? (xv[se - 1] + xv[se] + xv[se + 1]) / 3.0f + 1e-3f : xv[se] + 1e-3f;
            const float inv_nt = qb::rcpf_(nt);
            for (int t = part; t < T; t += QB_LANES_PER_VOXEL) {
                yt[t * kAdVox + vl] = xv[t] * inv_nt;
                is[t * kAdVox + vl] = qb::rcpf_(sv[t]);
                ls += QB_LN2 * qb::log2f_(sv[t]);
            }
        }
        const float log_s_sum = qb::voxel_sum(ls) + (float)T * kHalfLog2Pi;
        __syncthreads();
        if (inb && !live && part == 0) {
#pragma unroll
            for (int i = 0; i < 5; ++i) q_out[v * 5 + i] = q[v * 5 + i];
            for (int i = 0; i < ncol; ++i) out[v * ncol + i] = nan;
            if (q_rounds)
                for (int i = 0; i < 5 * R; ++i) q_rounds[v * 5 * R + i] = nan;
        }
        if (live) {
            float qv[5], pv[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                qv[i] = q[v * 5 + i];
                pv[i] = prior[v * 5 + i];
            }
            const qb::LogitMvn pm = qb::make_mvn(pv);
            qb::LogitMvn qm = qb::make_mvn(qv);
            AdProp prop;   // round 0: the given heads (their tanh values as make_mvn forms them)
            prop.mu_o = qv[0];
            prop.mu_d = qv[2];
            prop.t_so = qb::tanhf_(qv[1]);
            prop.t_sd = qb::tanhf_(qv[3]);
            prop.t_c = qb::tanhf_(qv[4]);
            AdProp best = prop;
            float best_ess = -INFINITY;
            int best_r = 0, flags = 0;
            const float* zv = z ? z + v * (int64_t)R * K * 2 : nullptr;
            const uint64_t vox = (uint64_t)(voxel0 + v);
            float* ov = out + v * ncol;
            float* qr = q_rounds ? q_rounds + v * 5 * R : nullptr;
            for (int r = 0; r < R; ++r) {
                if (r > 0) qm = ad_mvn(prop);
                if (qr && part == 0) {
                    if (r == 0) {
#pragma unroll
                        for (int i = 0; i < 5; ++i) qr[i] = qv[i];
                    } else {
                        ad_write_heads(prop, qr + 5 * r);
                    }
                }
                const IwKl kl = make_iw_kl(qm, pm);
                const float reach = fmaxf(fabsf(qm.mu_o) + QB_Z_MAX * qm.e_so,
                                          fabsf(qm.mu_d) + QB_Z_MAX * (fabsf(qm.c) + qm.e_sd));
                const bool whiten = zv == nullptr && reach < QB_LOGIT_CLIP;   // this voxel's own bound
                AdAcc acc;
                acc.init();
                qb::DrawQuad dq;
                for (int g = part; g < calls; g += QB_LANES_PER_VOXEL) {
                    if (!zv) dq.load(seed, vox, (uint32_t)(r * calls + g), qb::STREAM_ADAPT);
#pragma unroll 1
                    for (int i = 0; i < 4; ++i) {
                        float z0, z1;
                        if (zv) {
                            const int64_t draw = (int64_t)r * K + 4 * g + i;
                            z0 = zv[2 * draw];
                            z1 = zv[2 * draw + 1];
                        } else {
                            dq.next(z0, z1);
                        }
                        float a, b, oef, dbv;
                        qb::reparam_logits(qm, z0, z1, a, b);
                        qb::forward_transform(a, b, oef, dbv);
                        const qb::FwdFast fv = qb::fwd_fast(c, oef, dbv);
                        const float nll = ad_half_sq(L, c, fv, yt, is, vl, T, se, mirrored) + log_s_sum;
                        float dswr = iw_dswr(kl, z0, z1);
                        if (!whiten && fmaxf(fabsf(a), fabsf(b)) > QB_LOGIT_CLIP) dswr = qb::kl_swr_diff(qm, pm, z0, z1);
                        acc.add(-nll - fmaf(0.5f, dswr, kl.cst), z0, z1);
                    }
                }
                // the four lanes of a voxel are active together (v depends on lane & 15 only)
                const AdRound ro = ad_finish(acc, K);
                const bool ok = ro.s1 > 0.0f && ro.s1 < INFINITY;   // false for NaN
                if (part == 0) {
                    ov[2 * r + 0] = ro.log_p;
                    ov[2 * r + 1] = ok ? ro.ess : nan;
                }
                if (ok && ro.ess > best_ess) {
                    best_ess = ro.ess;
                    best_r = r;
                    best = prop;
                }
                if (r + 1 < R) {
                    if (!(ok && ad_update(prop, qm, ro, aa.shrink, flags))) flags |= 1;
                } else if (!ok) {
                    flags |= 1;
                }
            }
            if (part == 0) {
                if (best_r == 0) {
#pragma unroll
                    for (int i = 0; i < 5; ++i) q_out[v * 5 + i] = qv[i];
                } else {
                    ad_write_heads(best, q_out + v * 5);
                }
                ov[2 * R + 0] = (float)best_r;
                ov[2 * R + 1] = (float)flags;
            }
        }
    }
}

}  // namespace

extern "C" int qbold_adapt_posterior(const qbold_ctx* ctx, const float* x, const float* mask, const float* q,
                                     const float* prior, const float* sigma, const float* z,
                                     const qbold_adapt_cfg* cfg, uint64_t seed, int64_t voxel0, float* q_out, float* out,
                                     float* q_rounds, int64_t N, void* stream) {
    QB_NEED_DEVICE(ctx);
    QB_REQUIRE(cfg, "qbold_adapt_posterior: null cfg");
    QB_REQUIRE(N >= 0, "qbold_adapt_posterior: need N >= 0");
    QB_REQUIRE(cfg->rounds >= 1 && cfg->rounds <= QBOLD_ADAPT_MAX_ROUNDS, "qbold_adapt_posterior: need 1 <= rounds <= 16");
    QB_REQUIRE(cfg->K >= QBOLD_ADAPT_MIN_K && cfg->K <= QBOLD_ADAPT_MAX_K && cfg->K % 4 == 0,
               "qbold_adapt_posterior: K must be a multiple of 4 in [8, 1024]");
    QB_REQUIRE(cfg->shrink > 0.0f && cfg->shrink < INFINITY, "qbold_adapt_posterior: shrink must be positive and finite");
    QB_REQUIRE(q_out && out, "qbold_adapt_posterior: null q_out/out");
    QB_REQUIRE(N == 0 || (x && q && prior && sigma), "qbold_adapt_posterior: null input buffer");
    if (!qb::elbo_fast_path(ctx)) {
        qb::set_error("qbold_adapt_posterior: built for the full signal model in table mode with the Gaussian "
                      "likelihood on linear data (either normalisation)");
        return QBOLD_ERR_UNSUPPORTED;
    }
    const int T = ctx->dev.T;
    QB_REQUIRE(T >= 1 && T <= QB_MAX_T, "qbold_adapt_posterior: need 1 <= T <= 64");
    if (N == 0) return QBOLD_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t ntile = (N + kAdVox - 1) / kAdVox;
    const int grid = (int)(ntile < qb::elbo_grid(ctx) ? ntile : qb::elbo_grid(ctx));
    const size_t smem = sizeof(qb::FwdLds) + sizeof(float) * 2 * QB_MAX_T * kAdVox;
    const AdArgs aa{cfg->rounds, cfg->K, cfg->shrink};
    hipLaunchKernelGGL(adapt_kernel, dim3(grid), dim3(kAdBlock), smem, s, ctx->dev, ctx->d_tab, x, mask, q, prior, sigma,
                       z, aa, seed, voxel0, q_out, out, q_rounds, N);
    QB_HIP(hipGetLastError());
    return QBOLD_OK;
}
