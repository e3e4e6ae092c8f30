// psis_kernels.hip -- Pareto-smoothed importance sampling (Vehtari, Simpson, Gelman, Yao, Gabry, JMLR 2024) of N
// independent rows of K log-weights: the tail-shape estimate k^ of each row, its smoothed normalised weights, and the
// estimates they give (log p^, ESS, weighted means).  Nothing of the qBOLD model enters; qbold_log_evidence_draws
// (iw_kernels.hip) supplies the rows of the importance draws.
//
// One wave per row, four waves (rows) per block, each with its own LDS slice; lane l holds the draws l, l + 64, ... (at
// most 16).  Per row:
//   1. max, NaN check; the row's values as order-preserving 32-bit keys in registers.
//   2. cutoff = the (M + 1)-th largest value, M = ceil(min(K / 5, 3 sqrt K)) <= 96, by a 32-step bisection on the key
//      bits: a step counts the keys >= the candidate with one ballot per register slot, so no sort of the row.
//   3. tail = the n <= M entries strictly above the cutoff, compacted into LDS in draw order (ballot prefix), then
//      ordered by a rank count over (value, position): equal values keep their draw order (a stable order).
//      Selection and order work on the RAW float32 log-weights, whose order is exact; only then y = expm1(lw - cutoff).
//   4. Zhang & Stephens' fit of the generalised Pareto: its m = 30 + floor(sqrt n) <= 39 candidates one per lane, each
//      looping over the tail in LDS (a broadcast read); the softmax over the candidates' profile likelihoods as a
//      log-sum-exp over the wave.
//   5. the tail replaced by the fitted quantiles, truncated at the largest raw weight, scattered into the row in LDS;
//      the row's log-sum-exp and the weighted sums.
// Every sum is a per-lane loop in draw order followed by one fixed wave reduction: no atomics, so a row's results
// do not depend on where in the batch it stands.  The fit's arithmetic is float32 (expm1f / logf / expf of the device
// library, IEEE division, log1p as log1p_ratio below); MEASUREMENTS.md section 18 holds its measured
// distance to float64.
#include <cmath>

#include "qbold_ctx.h"

namespace {

constexpr int kWaves = 4;
constexpr int kBlock = 64 * kWaves;
constexpr int kSlots = QBOLD_PSIS_MAX_K / 64;   // register slots per lane
constexpr int kMaxTail = 96;                    // ceil(3 sqrt(1024)): the largest M
static_assert(kSlots == 16, "a lane holds at most 16 draws");

struct PsisLds {                // 5,632 bytes per wave
    float row[QBOLD_PSIS_MAX_K];   // x = lw - max, the tail then overwritten by its smoothed values
    float tv[kMaxTail];            // the tail's raw log-weights in draw order
    int ti[kMaxTail];              // ... and their draws
    float sy[kMaxTail];            // y = expm1(lw - cutoff), ascending
    int si[kMaxTail];              // the draw of each rank
};

// Wave reductions in registers (DPP), every lane getting the result: an inclusive scan along each row of 16 lanes
// (row_shr 1, 2, 4, 8; lanes without a source take the identity), row 0's total into row 1 and row 2's into row 3
// (row_bcast:15), rows 0 - 1's total into rows 2 - 3 (row_bcast:31), lane 63 read back.  One fixed order.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_take(float identity, float v) {
    return __uint_as_float(__builtin_amdgcn_update_dpp(__float_as_uint(identity), __float_as_uint(v), CTRL, ROW_MASK,
                                                       0xf, false));
}
__device__ __forceinline__ float lane63(float v) {
    return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), 63));
}
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp_take<0x111, 0xf>(0.0f, v);
    v += dpp_take<0x112, 0xf>(0.0f, v);
    v += dpp_take<0x114, 0xf>(0.0f, v);
    v += dpp_take<0x118, 0xf>(0.0f, v);
    v += dpp_take<0x142, 0xa>(0.0f, v);
    v += dpp_take<0x143, 0xc>(0.0f, v);
    return lane63(v);
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp_take<0x111, 0xf>(-INFINITY, v));
    v = fmaxf(v, dpp_take<0x112, 0xf>(-INFINITY, v));
    v = fmaxf(v, dpp_take<0x114, 0xf>(-INFINITY, v));
    v = fmaxf(v, dpp_take<0x118, 0xf>(-INFINITY, v));
    v = fmaxf(v, dpp_take<0x142, 0xa>(-INFINITY, v));
    v = fmaxf(v, dpp_take<0x143, 0xc>(-INFINITY, v));
    return lane63(v);
}
// LDS written by some lanes of a wave and read by others: order the wave's accesses
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// float -> unsigned key of the same order (no NaN, -0 canonicalised by the caller); 0 lies below every key
__device__ __forceinline__ uint32_t order_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
    return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
}

// The kernel's log1p(x): log(u) x / (u - 1) with u = fl(1 + x), in which the rounding of u cancels (u - 1 is exact for
// u in [1/2, 2] and within one rounding elsewhere) -- a few ulps, at a third of log1pf's 120 instructions, and the
// candidates' loop, where the kernel spends its time, is n of them per lane
__device__ __forceinline__ float log1p_ratio(float x) {
    const float u = 1.0f + x;
    const float d = u - 1.0f;
    return d == 0.0f ? x : logf(u) * (x / d);
}

__device__ __forceinline__ void nan_row(int64_t row, int K, int C, int lane, float* __restrict__ out,
                                        float* __restrict__ means, float* __restrict__ weights) {
    const float nan = __uint_as_float(0x7fc00000u);
    if (lane < 4) out[4 * row + lane] = nan;
    if (means && lane < C) means[row * C + lane] = nan;
    if (weights)
        for (int k = lane; k < K; k += 64) weights[row * K + k] = nan;
}

// NJ: the register slots of a lane, ceil(K / 64) rounded up to a power of two (the host picks the instantiation), so
// that the slot loops unroll without guards and a short row does not pay for the registers of a long one
template <int NJ>
__global__ __launch_bounds__(kBlock) void psis_kernel(const float* __restrict__ log_w, const float* __restrict__ theta,
                                                      int C, const float* __restrict__ mask, int K, int M,
                                                      float* __restrict__ out, float* __restrict__ means,
                                                      float* __restrict__ weights, int64_t N) {
    __shared__ PsisLds lds[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    PsisLds& S = lds[wave];
    const uint64_t below = (1ull << lane) - 1ull;
    for (int64_t row = (int64_t)blockIdx.x * kWaves + wave; row < N; row += (int64_t)gridDim.x * kWaves) {
        if (mask && !(mask[row] > 0.0f)) {   // not read
            nan_row(row, K, C, lane, out, means, weights);
            continue;
        }
        const float* lw = log_w + row * K;
        // 1. the row, its max, NaN check
        float v[NJ];
        float mx = -INFINITY;
        bool bad = false;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            v[j] = -INFINITY;
            const int k = lane + 64 * j;
            if (k < K) {
                v[j] = lw[k] + 0.0f;   // -0 -> +0: one key per value
                bad = bad || (v[j] != v[j]);
            }
            mx = fmaxf(mx, v[j]);
        }
        mx = wave_max(mx);
        if (__any(bad) || !(fabsf(mx) < INFINITY)) {   // a NaN, a +inf, or no finite weight at all
            nan_row(row, K, C, lane, out, means, weights);
            continue;
        }
        uint32_t key[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) key[j] = (lane + 64 * j < K) ? order_key(v[j]) : 0u;
        // 2. the (M + 1)-th largest key: the largest t with #{key >= t} >= M + 1, bit by bit
        uint32_t ck = 0u;
#pragma unroll 1
        for (int b = 31; b >= 0; --b) {
            const uint32_t t = ck | (1u << b);
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                cnt += __popcll(__ballot(key[j] >= t));
            if (cnt > M) ck = t;
        }
        const float c_lw = key_value(ck);
        const float cx = c_lw - mx;   // the cutoff on the x scale, <= 0 (-inf when the cutoff is a zero weight)
        // 3. x into LDS; the tail (strictly above the cutoff) compacted in draw order
        wave_lds_sync();              // the previous row's readers are done
        int n = 0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = lane + 64 * j;
            const bool in = key[j] > ck;
            const uint64_t bal = __ballot(in);
            const int pos = n + __popcll(bal & below);
            if (k < K) S.row[k] = v[j] - mx;
            if (in && pos < kMaxTail) {
                S.tv[pos] = v[j];
                S.ti[pos] = k;
            }
            n += __popcll(bal);
        }
        // n <= M <= kMaxTail: at least M + 1 keys are >= ck, so at most M lie above it
        float khat = INFINITY;
        if (n > 4 && !(-cx > 80.0f)) {
            wave_lds_sync();
            // order by (value, position in draw order): rank = the number of entries before this one
            const int e0 = lane, e1 = lane + 64;
            const float x0 = e0 < n ? S.tv[e0] : 0.0f, x1 = e1 < n ? S.tv[e1] : 0.0f;
            int r0 = 0, r1 = 0;
            for (int s = 0; s < n; ++s) {
                const float xs = S.tv[s];
                r0 += (xs < x0 || (xs == x0 && s < e0)) ? 1 : 0;
                r1 += (xs < x1 || (xs == x1 && s < e1)) ? 1 : 0;
            }
            if (e0 < n) {
                S.sy[r0] = expm1f(x0 - c_lw);
                S.si[r0] = S.ti[e0];
            }
            if (e1 < n) {
                S.sy[r1] = expm1f(x1 - c_lw);
                S.si[r1] = S.ti[e1];
            }
            wave_lds_sync();
            // 4. the fit: candidate j = lane + 1 of m
            int sq = (int)sqrtf((float)n);
            while (sq * sq > n) --sq;
            while ((sq + 1) * (sq + 1) <= n) ++sq;
            const int m = 30 + sq;
            const float fn = (float)n;
            const float yn = S.sy[n - 1], yq = S.sy[(n + 2) / 4 - 1];   // q = floor(n / 4 + 1 / 2)
            const bool cand = lane < m;
            const float fj = (float)(cand ? lane + 1 : m) - 0.5f;
            const float b = 1.0f / yn + (1.0f - sqrtf((float)m / fj)) / (3.0f * yq);
            float ks = 0.0f;
#pragma unroll 4
            for (int r = 0; r < n; ++r) ks += log1p_ratio(-b * S.sy[r]);   // the sum stays in rank order
            const float kj = ks / fn;
            const float L = cand ? fn * (logf(-b / kj) - kj - 1.0f) : -INFINITY;
            const float Lmax = wave_max(L);
            const float e = cand ? expf(L - Lmax) : 0.0f;   // NaN from a non-finite candidate reaches bhat
            const float bhat = wave_sum(e * b) / wave_sum(e);
            float kp = 0.0f;
            if (e0 < n) kp += log1p_ratio(-bhat * S.sy[e0]);
            if (e1 < n) kp += log1p_ratio(-bhat * S.sy[e1]);
            const float k = wave_sum(kp) / fn;
            const float sigma = -k / bhat;
            const float kreg = (fn * k + 5.0f) / (fn + 10.0f);
            if (fabsf(kreg) < INFINITY && fabsf(sigma) < INFINITY) {
                khat = kreg;
                // 5. the fitted quantiles at p_r = (r - 1/2) / n, r = 1 .. n, back on the x scale, truncated at 0
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int r = lane + 64 * h;
                    if (r < n) {
                        const float l1 = log1p_ratio(-((float)r + 0.5f) / fn);
                        const float qy = k == 0.0f ? -sigma * l1 : sigma * expm1f(-k * l1) / k;
                        S.row[S.si[r]] = fminf(cx + log1p_ratio(qy), 0.0f);
                    }
                }
            }
        }
        wave_lds_sync();
        // the smoothed row: log-sum-exp, ESS, weighted means, normalised log-weights
        float m2 = -INFINITY;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            v[j] = -INFINITY;
            const int k = lane + 64 * j;
            if (k < K) v[j] = S.row[k];
            m2 = fmaxf(m2, v[j]);
        }
        m2 = wave_max(m2);
        float s1 = 0.0f;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            s1 += expf(v[j] - m2);
        const float lse = m2 + logf(wave_sum(s1));
        float s2 = 0.0f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = lane + 64 * j;
            const float lwn = v[j] - lse;
            if (weights && k < K) weights[row * K + k] = lwn;
            v[j] = expf(lwn);   // the normalised weight from here on; 0 in the padding
            s2 = fmaf(v[j], v[j], s2);
        }
        s2 = wave_sum(s2);
        if (lane == 0) {
            float4 o;
            o.x = khat;
            o.y = mx + lse - logf((float)K);
            o.z = 1.0f / s2;
            o.w = (float)n;
            out[4 * row + 0] = o.x;
            out[4 * row + 1] = o.y;
            out[4 * row + 2] = o.z;
            out[4 * row + 3] = o.w;
        }
        if (means) {
            const float* th = theta + row * K * C;
            for (int c = 0; c < C; ++c) {
                float sm = 0.0f;
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int k = lane + 64 * j;
                    if (k < K) sm = fmaf(v[j], th[(int64_t)k * C + c], sm);
                }
                sm = wave_sum(sm);
                if (lane == 0) means[row * C + c] = sm;
            }
        }
    }
}

}  // namespace

extern "C" int qbold_psis(const qbold_ctx* ctx, const float* log_w, const float* theta, int C, const float* mask,
                          int K, float* out, float* means, float* weights, int64_t N, void* stream) {
    QB_NEED_DEVICE(ctx);
    QB_REQUIRE(N >= 0 && K >= QBOLD_PSIS_MIN_K && K <= QBOLD_PSIS_MAX_K,
               "qbold_psis: need N >= 0 and QBOLD_PSIS_MIN_K <= K <= QBOLD_PSIS_MAX_K");
    QB_REQUIRE(out && (N == 0 || log_w), "qbold_psis: null log_w/out");
    QB_REQUIRE(!theta || (C >= 1 && C <= QBOLD_PSIS_MAX_C), "qbold_psis: theta needs 1 <= C <= QBOLD_PSIS_MAX_C");
    QB_REQUIRE(!means || theta, "qbold_psis: means needs theta");
    if (N == 0) return QBOLD_OK;
    const double tail = std::fmin((double)K / 5.0, 3.0 * std::sqrt((double)K));
    const int M = (int)std::ceil(tail);
    const int64_t blocks = (N + kWaves - 1) / kWaves, cap = (int64_t)ctx->num_cus * 8;
    const int grid = (int)(blocks < cap ? blocks : cap);
#define QB_LAUNCH_PSIS(NJ)                                                                                          \
    hipLaunchKernelGGL(psis_kernel<NJ>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, log_w, theta, theta ? C : 0, \
                       mask, K, M, out, means, weights, N)
    if (K <= 64) QB_LAUNCH_PSIS(1);
    else if (K <= 128) QB_LAUNCH_PSIS(2);
    else if (K <= 256) QB_LAUNCH_PSIS(4);
    else if (K <= 512) QB_LAUNCH_PSIS(8);
    else QB_LAUNCH_PSIS(kSlots);
#undef QB_LAUNCH_PSIS
    QB_HIP(hipGetLastError());
    return QBOLD_OK;
}
