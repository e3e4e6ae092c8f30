// calibration_kernels.hip -- qbold_calibration: where a KNOWN (OEF, DBV) falls in a voxel's posterior q (simulation-based
// calibration, Talts et al. 2018; Sailynoja et al. 2022).  Per voxel, from the raw heads of the use_mvg family and the
// truth: the two marginal PIT values and the level of the smallest highest-density ellipse of q that holds the truth
// (closed forms in logit space), and the rank of the truth among L reparameterised draws for OEF, DBV and R2' -- the
// draws of qbold_log_evidence_draws (explicit z, or Philox stream 6 keyed (seed, voxel0 + i)), optionally weighted by a
// row of log-weights of those same draws (qbold_psis' `weights`), which turns the rank into the importance-corrected
// posterior's CDF at the truth.  The specification is the comment at the declaration in include/qbold_hip.h.
//
// Lane mapping of iw_draws_kernel (iw_kernels.hip): a wave owns 16 voxels, the four lanes l, l + 16, l + 32, l + 48 of a
// voxel split its draws by Philox call (call g -> draws 4 g .. 4 g + 3, lane group g & 3) and read the pieces of the z
// and log_w rows that belong to those draws; integer counts (unweighted) or float sums (weighted) close over the four
// lanes with two __shfl_xor steps in a fixed order: no atomics, no LDS, the same bits at any batch position.  The
// weighted form walks the voxel's log_w row twice: the maximum (and the NaN / +inf check), then the sums relative to it.
#include <cmath>
#include <type_traits>

#include "elbo_core.h"
#include "qbold_ctx.h"

namespace {

constexpr int kBlock = 256;                                  // 4 waves
constexpr int kVoxPerBlock = kBlock / QB_LANES_PER_VOXEL;    // 16 voxels per wave, 4 lanes each

// The truth's logit as make_obs forms it (model.py:393-398: the unit-interval value clamped to [1e-6, 1 - 1e-6]), with
// two differences that matter for a rank: 1 - x is formed from the upper end of the range, (hi - t) / range, not as
// 1 - x, so that it does not cancel for a truth at the upper clamp (make_obs: log(1 - x) off by 1.3e-2 there), and the
// ends of the range carry their float32 remainders (lo = lo_h + lo_l), so that x keeps its leading digits at the lower
// one.  Both differences t - lo_h and hi_h - t are exact within a factor of two of the end (Sterbenz).  A NaN truth
// stays NaN (fminf / fmaxf would turn it into a clamp bound).
__device__ __forceinline__ float cal_unit(float x) {
    return x < 1e-6f ? 1e-6f : (x > 1.0f - 1e-6f ? 1.0f - 1e-6f : x);
}
template <int WHICH>
__device__ __forceinline__ float cal_truth_logit(float t) {
    constexpr double lo = WHICH == 0 ? 0.04 : 0.001, hi = WHICH == 0 ? 0.84 : 0.201;
    constexpr float inv_range = WHICH == 0 ? 1.25f : 5.0f;
    constexpr float lo_h = (float)lo, lo_l = (float)(lo - (double)lo_h);
    constexpr float hi_h = (float)hi, hi_l = (float)(hi - (double)hi_h);
    const float x = cal_unit(((t - lo_h) - lo_l) * inv_range);
    const float y = cal_unit(((hi_h - t) + hi_l) * inv_range);
    return __logf(x) - __logf(y);
}

// Phi(w), the standard normal CDF
__device__ __forceinline__ float cal_phi(float w) { return 0.5f * erfcf(-0.70710678118654752f * w); }

// the four log-weights of Philox call g of a voxel's row; the entries beyond L come out as -inf (a zero weight)
__device__ __forceinline__ void cal_load_lw(const float* __restrict__ lwv, int g, int L, bool vec, float l[4]) {
    if (vec) {   // L is a multiple of 4: every call is whole
        const float4 t = *reinterpret_cast<const float4*>(lwv + 4 * g);
        l[0] = t.x; l[1] = t.y; l[2] = t.z; l[3] = t.w;
        return;
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) l[d] = 4 * g + d < L ? lwv[4 * g + d] : -INFINITY;
}
// the explicit normals of the cnt draws of call g: exactly 2 L floats of the row are ever read
__device__ __forceinline__ void cal_load_z(const float* __restrict__ zv, int g, int cnt, bool vec, float zq[8]) {
    if (vec && cnt == 4) {
        const float4 a = *reinterpret_cast<const float4*>(zv + 8 * g);
        const float4 b = *reinterpret_cast<const float4*>(zv + 8 * g + 4);
        zq[0] = a.x; zq[1] = a.y; zq[2] = a.z; zq[3] = a.w;
        zq[4] = b.x; zq[5] = b.y; zq[6] = b.z; zq[7] = b.w;
        return;
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        zq[2 * d] = d < cnt ? zv[8 * g + 2 * d] : 0.0f;
        zq[2 * d + 1] = d < cnt ? zv[8 * g + 2 * d + 1] : 0.0f;
    }
}

__device__ __forceinline__ int voxel_sum_i(int v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// One lane's share of a voxel's draws against the truth: per statistic (logit OEF, logit DBV, OEF DBV) what lies below
// it and what ties with it -- counts, or sums of weights relative to the row's maximum.
template <bool WEIGHTED>
struct CalAcc {
    using T = typename std::conditional<WEIGHTED, float, int>::type;
    T lt[3], eq[3];
    float sw;
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < 3; ++j) lt[j] = eq[j] = (T)0;
        sw = 0.0f;
    }
    __device__ __forceinline__ void add(int j, float d, float t, float w) {
        if constexpr (WEIGHTED) {
            lt[j] += d < t ? w : 0.0f;
            eq[j] += d == t ? w : 0.0f;
        } else {
            lt[j] += d < t ? 1 : 0;
            eq[j] += d == t ? 1 : 0;
        }
    }
};

template <bool WEIGHTED, bool EXPLICIT>
__global__ __launch_bounds__(kBlock) void calibration_kernel(
    const float* __restrict__ theta_true, const float* __restrict__ mask, const float* __restrict__ q,
    const float* __restrict__ log_w, const float* __restrict__ z, int L, bool zvec, bool wvec, uint64_t seed,
    int64_t voxel0, float* __restrict__ out, int64_t N) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int part = lane >> 4;
    const float nan = __uint_as_float(0x7fc00000u);
    const int64_t ntile = (N + kVoxPerBlock - 1) / kVoxPerBlock;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        // the four lanes of a voxel take every branch below together (v depends on lane & 15 only)
        const int64_t v = tile * kVoxPerBlock + wave * QB_VOX_PER_WAVE + (lane & 15);
        if (v >= N) continue;
        const float m = mask ? mask[v] : 1.0f;
        if (!(m > 0.0f)) {   // outside the mask: nothing of the voxel is read
            if (part == 0) {
#pragma unroll
                for (int i = 0; i < QBOLD_CAL_OUT; ++i) out[QBOLD_CAL_OUT * v + i] = nan;
            }
            continue;
        }
        float qv[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) qv[i] = q[v * 5 + i];
        const qb::LogitMvn qm = qb::make_mvn(qv);
        const float t_o = theta_true[2 * v], t_d = theta_true[2 * v + 1];
        const float a_t = cal_truth_logit<0>(t_o), b_t = cal_truth_logit<1>(t_d);
        const float r_t = t_o * t_d;   // dw_coef > 0 cancels from both sides of the R2' comparison

        // the row's maximum, and whether the row can be used at all
        float M = 0.0f;
        bool bad = false;
        const float* lwv = nullptr;
        if constexpr (WEIGHTED) {
            lwv = log_w + v * (int64_t)L;
            M = -INFINITY;
            int nbad = 0;
            for (int g = part; 4 * g < L; g += QB_LANES_PER_VOXEL) {
                float l[4];
                cal_load_lw(lwv, g, L, wvec, l);
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    nbad += l[d] < INFINITY ? 0 : 1;   // NaN or +inf
                    M = fmaxf(M, l[d]);
                }
            }
            M = fmaxf(M, __shfl_xor(M, 16, 64));
            M = fmaxf(M, __shfl_xor(M, 32, 64));
            bad = voxel_sum_i(nbad) != 0 || M == -INFINITY;   // ... or no finite entry
        }

        CalAcc<WEIGHTED> acc;
        acc.init();
        const float* zv = EXPLICIT ? z + v * (int64_t)L * 2 : nullptr;
        const uint64_t vox = (uint64_t)(voxel0 + v);
#pragma unroll 1
        for (int g = part; 4 * g < L; g += QB_LANES_PER_VOXEL) {
            const int cnt = L - 4 * g < 4 ? L - 4 * g : 4;
            float zq[8], l[4];
            qb::DrawQuad dq;
            if constexpr (EXPLICIT) cal_load_z(zv, g, cnt, zvec, zq);
            else dq.load(seed, vox, (uint32_t)g, qb::STREAM_IW);
            if constexpr (WEIGHTED) cal_load_lw(lwv, g, L, wvec, l);
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                float z0, z1;
                if constexpr (EXPLICIT) {
                    z0 = zq[2 * d];
                    z1 = zq[2 * d + 1];
                } else {
                    dq.next(z0, z1);
                }
                if (d < cnt) {
                    float a, b, oef, dbv, w = 1.0f;
                    qb::reparam_logits(qm, z0, z1, a, b);
                    qb::forward_transform(a, b, oef, dbv);
                    if constexpr (WEIGHTED) {
                        w = qb::exp2f_((l[d] - M) * QB_LOG2E);   // -inf: a zero weight
                        acc.sw += w;
                    }
                    acc.add(0, a, a_t, w);   // the sigmoid is monotone: ranks of OEF and DBV are ranks of the logits
                    acc.add(1, b, b_t, w);
                    acc.add(2, oef * dbv, r_t, w);
                }
            }
        }

        float rank[3];
        if constexpr (WEIGHTED) {
            const float inv = 1.0f / qb::voxel_sum(acc.sw);
#pragma unroll
            for (int j = 0; j < 3; ++j)
                rank[j] = bad ? nan : fmaf(0.5f, qb::voxel_sum(acc.eq[j]), qb::voxel_sum(acc.lt[j])) * inv;
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                rank[j] = (float)(2 * voxel_sum_i(acc.lt[j]) + voxel_sum_i(acc.eq[j])) / (float)(2 * L);
        }
        if (part == 0) {
            const float r0 = a_t - qm.mu_o, r1 = b_t - qm.mu_d;
            const float w0 = r0 * qm.i_so;
            const float w1 = fmaf(r1, qm.i_sd, r0 * qm.i_bl);   // L_q^-1 (u* - mu), model.py:423-441
            // a comparison with a NaN is false: a NaN head or truth must not come out as rank 0
            const bool nan_o = a_t != a_t || qm.mu_o != qm.mu_o || qm.e_so != qm.e_so;
            const bool nan_d = b_t != b_t || qm.mu_d != qm.mu_d || qm.e_sd != qm.e_sd || qm.c != qm.c;
            float* o = out + QBOLD_CAL_OUT * v;
            o[0] = cal_phi(w0);
            o[1] = cal_phi(r1 / sqrtf(fmaf(qm.c, qm.c, qm.e_sd * qm.e_sd)));
            o[2] = -expm1f(-0.5f * fmaf(w0, w0, w1 * w1));
            o[3] = nan_o ? nan : rank[0];
            o[4] = nan_d ? nan : rank[1];
            o[5] = (nan_o || nan_d || r_t != r_t) ? nan : rank[2];
        }
    }
}

}  // namespace

extern "C" int qbold_calibration(const qbold_ctx* ctx, const float* theta_true, const float* mask, const float* q,
                                 const float* log_w, const float* z, int L, uint64_t seed, int64_t voxel0, float* out,
                                 int64_t N, void* stream) {
    QB_NEED_DEVICE(ctx);
    QB_REQUIRE(N >= 0 && L >= 1 && L <= QBOLD_CAL_MAX_L, "qbold_calibration: need N >= 0 and 1 <= L <= QBOLD_CAL_MAX_L");
    QB_REQUIRE(out, "qbold_calibration: null out");
    QB_REQUIRE(N == 0 || (theta_true && q), "qbold_calibration: null theta_true / q");
    if (N == 0) return QBOLD_OK;
    // rows of z start at 8 v L bytes and rows of log_w at 4 v L bytes: 16-byte pieces only where every row is aligned
    const bool zvec = (L & 1) == 0 && (reinterpret_cast<uintptr_t>(z) & 15) == 0;
    const bool wvec = (L & 3) == 0 && (reinterpret_cast<uintptr_t>(log_w) & 15) == 0;
    const int64_t ntile = (N + kVoxPerBlock - 1) / kVoxPerBlock, cap = (int64_t)ctx->num_cus * 8;
    const int grid = (int)(ntile < cap ? ntile : cap);
#define QB_LAUNCH_CAL(W, E)                                                                                        \
    hipLaunchKernelGGL((calibration_kernel<W, E>), dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, theta_true,   \
                       mask, q, log_w, z, L, zvec, wvec, seed, voxel0, out, N)
    if (log_w && z) QB_LAUNCH_CAL(true, true);
    else if (log_w) QB_LAUNCH_CAL(true, false);
    else if (z) QB_LAUNCH_CAL(false, true);
    else QB_LAUNCH_CAL(false, false);
#undef QB_LAUNCH_CAL
    QB_HIP(hipGetLastError());
    return QBOLD_OK;
}
