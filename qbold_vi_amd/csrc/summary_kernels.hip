// summary_kernels.hip -- summaries of N independent rows of K weighted draws (qbold_draw_summary): per column the
// weighted mean and sd, weighted quantiles by the inverse ECDF, the highest-density interval, and per row the ESS, the
// largest weight and the weighted correlations.  Nothing of the qBOLD model enters; qbold_log_evidence_draws
// (iw_kernels.hip) and qbold_psis supply the rows.  include/qbold_hip.h holds the definitions.
//
// psis_kernel's shape: one wave per row, four waves (rows) per block, each with its own LDS slice, a grid-stride loop
// over the rows, NJ register slots per lane picked by K on the host.  Per row:
//   1. the weights once: max, NaN check, expf, the normaliser, ESS, the largest weight; w~ into LDS by draw.
//   2. per column (a run-time loop): the moments from the draws as loaded (lane l holds the draws l, l + 64, ...), then
//      a bitonic sort of the wave's n = 64 NJ elements on the 64-bit key (order_key(theta) : draw).  All keys differ, so
//      the network yields the order of the definition.  Position p = NJ lane + slot: strides below NJ are
//      compare-exchanges in registers, larger ones go across lanes by __shfl_xor; after it a lane holds NJ consecutive
//      ranks.  Padding slots and draws of weight 0 carry the maximal key word: they end up behind the L live draws and
//      no search below looks at them.
//   3. w~ gathered by draw from LDS, a sequential prefix per lane plus an exclusive wave scan = W_r; theta_(r) and W_r
//      into LDS.
//   4. a quantile = theta_(min(#{r < L : W_r < p}, L - 1)), one ballot per slot.
//   5. the interval: a lane takes the starts a of its NJ ranks and binary-searches W in LDS for b(a) (W_b >= W_{a-1} +
//      mass, compared in float64 where that sum is exact); the width is the float64 difference, exact as well; the
//      lane's best, a wave minimum of the width, and the lowest lane that holds it (= the smallest a).
// Every sum is a per-lane loop in a fixed order followed by one fixed DPP reduction or scan: no atomics, so a row's
// results do not depend on where in the batch it stands.  The float32 W_r need not be monotone to the last bit across
// lanes (the scan and the per-lane prefixes round differently); each stays within its error bound, which is all the
// count in 4 and the search in 5 need.
#include <cmath>

#include "qbold_ctx.h"

namespace {

constexpr int kWaves = 4;
constexpr int kBlock = 64 * kWaves;
constexpr int kMaxC = QBOLD_SUMMARY_MAX_C;
constexpr int kMaxP = QBOLD_SUMMARY_MAX_P;
constexpr uint32_t kDeadKey = 0xffffffffu;   // above order_key of every non-NaN float

template <int NJ>
struct SummaryLds {          // 12 NJ * 64 + 64 bytes per wave: 12,352 at NJ = 16
    float w[64 * NJ];        // w~ by draw, 0 in the padding
    float W[64 * NJ];        // W_r by rank
    float sv[64 * NJ];       // theta_(r) by rank
    float mean[kMaxC], sd[kMaxC];
};

struct Levels {
    float p[kMaxP];
};

// Wave reductions in registers (DPP), as in psis_kernels.hip: an inclusive scan along each row of 16 lanes (row_shr 1,
// 2, 4, 8; lanes without a source take the identity), row 0's total into row 1 and row 2's into row 3 (row_bcast:15),
// rows 0 - 1's total into rows 2 - 3 (row_bcast:31): every lane then holds the inclusive scan, lane 63 the total.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_take(float identity, float v) {
    return __uint_as_float(__builtin_amdgcn_update_dpp(__float_as_uint(identity), __float_as_uint(v), CTRL, ROW_MASK,
                                                       0xf, false));
}
__device__ __forceinline__ float lane63(float v) {
    return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), 63));
}
__device__ __forceinline__ float wave_scan(float v) {
    v += dpp_take<0x111, 0xf>(0.0f, v);
    v += dpp_take<0x112, 0xf>(0.0f, v);
    v += dpp_take<0x114, 0xf>(0.0f, v);
    v += dpp_take<0x118, 0xf>(0.0f, v);
    v += dpp_take<0x142, 0xa>(0.0f, v);
    v += dpp_take<0x143, 0xc>(0.0f, v);
    return v;
}
__device__ __forceinline__ float wave_sum(float v) { return lane63(wave_scan(v)); }
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
// float -> unsigned key of the same order (no NaN, -0 canonicalised by the caller)
__device__ __forceinline__ uint32_t order_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
    return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
}

__device__ __forceinline__ void nan_fill(float* __restrict__ p, int n, int lane) {
    const float nan = __uint_as_float(0x7fc00000u);
    for (int i = lane; i < n; i += 64) p[i] = nan;
}

// ascending bitonic sort of the wave's 64 NJ keys; position p = NJ lane + slot
template <int NJ>
__device__ __forceinline__ void wave_sort(uint64_t (&key)[NJ], int lane) {
    constexpr int n = 64 * NJ;
#pragma unroll 1
    for (int k = 2; k <= n; k <<= 1) {
#pragma unroll 1
        for (int j = k >> 1; j >= NJ; j >>= 1) {   // across lanes: the partner holds position p ^ j
            const int lm = j / NJ;
            const bool asc = ((lane * NJ) & k) == 0;
            const bool keep_min = ((lane & lm) == 0) == asc;
#pragma unroll
            for (int s = 0; s < NJ; ++s) {
                const uint64_t o = __shfl_xor((unsigned long long)key[s], lm);
                const bool o_less = o < key[s];
                key[s] = (o_less == keep_min) ? o : key[s];
            }
        }
#pragma unroll
        for (int j = NJ >> 1; j >= 1; j >>= 1) {   // within the lane's registers
            if (j <= (k >> 1)) {
#pragma unroll
                for (int s = 0; s < NJ; ++s) {
                    if ((s & j) == 0) {
                        const bool asc = ((lane * NJ + s) & k) == 0;
                        const uint64_t a = key[s], b = key[s | j];
                        const bool swap = (a > b) == asc;
                        key[s] = swap ? b : a;
                        key[s | j] = swap ? a : b;
                    }
                }
            }
        }
    }
}

template <int NJ>
__global__ __launch_bounds__(kBlock) void draw_summary_kernel(const float* __restrict__ log_w,
                                                              const float* __restrict__ theta, int C,
                                                              const float* __restrict__ mask, int K, Levels lv, int P,
                                                              float hpd_mass, float* __restrict__ stats,
                                                              float* __restrict__ quant, float* __restrict__ row_out,
                                                              float* __restrict__ corr, int64_t N) {
    constexpr int n = 64 * NJ;
    constexpr int kSteps = 6 + (NJ == 1 ? 0 : NJ == 2 ? 1 : NJ == 4 ? 2 : NJ == 8 ? 3 : 4);   // log2 n
    __shared__ SummaryLds<NJ> lds[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    SummaryLds<NJ>& S = lds[wave];
    const float nan = __uint_as_float(0x7fc00000u);
    const int pairs = C * (C - 1) / 2;
    for (int64_t row = (int64_t)blockIdx.x * kWaves + wave; row < N; row += (int64_t)gridDim.x * kWaves) {
        float* st = stats + row * C * 4;
        float* qo = quant ? quant + row * C * P : nullptr;
        float* co = corr ? corr + row * pairs : nullptr;
        // 1. the weights
        float wv[NJ];
        float mx = -INFINITY;
        bool bad = mask && !(mask[row] > 0.0f);   // not read
        if (!bad) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int k = lane + 64 * j;
                wv[j] = -INFINITY;
                if (k < K) {
                    wv[j] = log_w ? log_w[row * K + k] : 0.0f;
                    bad = bad || (wv[j] != wv[j]);
                }
                mx = fmaxf(mx, wv[j]);
            }
            mx = wave_max(mx);
        }
        if (__any(bad) || !(fabsf(mx) < INFINITY)) {   // masked; a NaN, a +inf, or no finite weight at all
            nan_fill(st, 4 * C, lane);
            if (qo) nan_fill(qo, C * P, lane);
            if (co) nan_fill(co, pairs, lane);
            if (lane < 2) row_out[2 * row + lane] = nan;
            continue;
        }
        float s1 = 0.0f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            wv[j] = expf(wv[j] - mx);   // 0 in the padding
            s1 += wv[j];
        }
        s1 = wave_sum(s1);
        float s2 = 0.0f, wmax = 0.0f;
        int L = 0;   // the draws with a positive weight
        wave_lds_sync();   // the previous row's readers are done
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            wv[j] = wv[j] / s1;
            s2 = fmaf(wv[j], wv[j], s2);
            wmax = fmaxf(wmax, wv[j]);
            L += __popcll(__ballot(wv[j] > 0.0f));
            S.w[lane + 64 * j] = wv[j];
        }
        s2 = wave_sum(s2);
        wmax = wave_max(wmax);
        if (lane == 0) {
            row_out[2 * row + 0] = 1.0f / s2;
            row_out[2 * row + 1] = wmax;
        }
        const float* th = theta + row * K * C;
        // 2. the columns
#pragma unroll 1
        for (int c = 0; c < C; ++c) {
            float tv[NJ];
            bool tbad = false;
            float sm = 0.0f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int k = lane + 64 * j;
                tv[j] = 0.0f;
                if (k < K) {
                    tv[j] = th[(int64_t)k * C + c] + 0.0f;   // -0 -> +0: one key per value
                    tbad = tbad || (tv[j] != tv[j]);
                }
                sm = fmaf(wv[j], tv[j], sm);
            }
            if (__any(tbad)) {
                if (lane < 4) st[4 * c + lane] = nan;
                if (qo && lane < P) qo[c * P + lane] = nan;
                if (lane == 0) S.mean[c] = S.sd[c] = nan;
                continue;
            }
            const float mean = wave_sum(sm);
            float sv = 0.0f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const float d = tv[j] - mean;
                sv = fmaf(wv[j] * d, d, sv);
            }
            const float sd = sqrtf(wave_sum(sv));
            uint64_t key[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const uint32_t k = (uint32_t)(lane + 64 * j);
                key[j] = ((uint64_t)(wv[j] > 0.0f ? order_key(tv[j]) : kDeadKey) << 32) | k;
            }
            wave_sort<NJ>(key, lane);
            // 3. W_r: rank r = NJ lane + j
            wave_lds_sync();   // the previous column's readers of W and sv are done
            float cw[NJ];
            float run = 0.0f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                run += S.w[(uint32_t)key[j]];
                cw[j] = run;
            }
            const float incl = wave_scan(run);
            float excl = __shfl_up(incl, 1);
            if (lane == 0) excl = 0.0f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                cw[j] = excl + cw[j];
                S.W[NJ * lane + j] = cw[j];
                S.sv[NJ * lane + j] = key_value((uint32_t)(key[j] >> 32));
            }
            wave_lds_sync();
            // 4. the quantiles
            float qv = 0.0f;
#pragma unroll
            for (int i = 0; i < kMaxP; ++i) {
                if (i < P) {
                    int cnt = 0;
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
                        cnt += __popcll(__ballot(NJ * lane + j < L && cw[j] < lv.p[i]));
                    const float v = S.sv[min(cnt, L - 1)];
                    if (lane == i) qv = v;
                }
            }
            if (qo && lane < P) qo[c * P + lane] = qv;
            // 5. the interval
            int lo[NJ], hi[NJ];
            double target[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int a = NJ * lane + j;
                const float wprev = j > 0 ? cw[j - 1] : excl;   // W_{a-1}; 0 at a = 0
                target[j] = (double)wprev + (double)hpd_mass;
                lo[j] = a;
                hi[j] = L - 1;
            }
#pragma unroll 1
            for (int it = 0; it < kSteps; ++it) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    if (lo[j] < hi[j]) {
                        const int mid = (lo[j] + hi[j]) >> 1;
                        if ((double)S.W[mid] >= target[j]) hi[j] = mid;
                        else lo[j] = mid + 1;
                    }
                }
            }
            double best = INFINITY;
            int ba = 0, bb = L - 1;   // no feasible pair at all: the live range
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int a = NJ * lane + j, b = lo[j];
                if (a < L && (double)S.W[b] >= target[j]) {
                    const double width = (double)S.sv[b] - (double)S.sv[a];
                    if (width < best) {
                        best = width;
                        ba = a;
                        bb = b;
                    }
                }
            }
            double wmin = best;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) wmin = fmin(wmin, __shfl_xor(wmin, m));
            const uint64_t holders = __ballot(best == wmin);   // every lane when no pair is feasible
            const int src = __ffsll((unsigned long long)holders) - 1;
            ba = __shfl(ba, src);
            bb = __shfl(bb, src);
            if (lane == 0) {
                st[4 * c + 0] = mean;
                st[4 * c + 1] = sd;
                st[4 * c + 2] = S.sv[ba];
                st[4 * c + 3] = S.sv[bb];
                S.mean[c] = mean;
                S.sd[c] = sd;
            }
        }
        if (co) {
            wave_lds_sync();   // mean and sd of every column
            int pr = 0;
#pragma unroll 1
            for (int c1 = 0; c1 < C; ++c1) {
#pragma unroll 1
                for (int c2 = c1 + 1; c2 < C; ++c2, ++pr) {
                    const float m1 = S.mean[c1], m2 = S.mean[c2], d1 = S.sd[c1], d2 = S.sd[c2];
                    float r = nan;
                    if (d1 > 0.0f && d2 > 0.0f) {   // false for the NaN of a column with a NaN
                        float cv = 0.0f;
#pragma unroll
                        for (int j = 0; j < NJ; ++j) {
                            const int k = lane + 64 * j;
                            if (k < K) cv = fmaf(wv[j] * (th[(int64_t)k * C + c1] - m1), th[(int64_t)k * C + c2] - m2, cv);
                        }
                        r = wave_sum(cv) / (d1 * d2);
                    }
                    if (lane == 0) co[pr] = r;
                }
            }
        }
    }
}

}  // namespace

extern "C" int qbold_draw_summary(const qbold_ctx* ctx, const float* log_w, const float* theta, int C,
                                  const float* mask, int K, const float* probs_host, int P, float hpd_mass,
                                  float* stats, float* quant, float* row_out, float* corr, int64_t N, void* stream) {
    QB_NEED_DEVICE(ctx);
    QB_REQUIRE(N >= 0 && K >= QBOLD_SUMMARY_MIN_K && K <= QBOLD_SUMMARY_MAX_K,
               "qbold_draw_summary: need N >= 0 and QBOLD_SUMMARY_MIN_K <= K <= QBOLD_SUMMARY_MAX_K");
    QB_REQUIRE(C >= 1 && C <= QBOLD_SUMMARY_MAX_C, "qbold_draw_summary: need 1 <= C <= QBOLD_SUMMARY_MAX_C");
    QB_REQUIRE(P >= 0 && P <= QBOLD_SUMMARY_MAX_P, "qbold_draw_summary: need 0 <= P <= QBOLD_SUMMARY_MAX_P");
    QB_REQUIRE(P == 0 || (probs_host && quant), "qbold_draw_summary: P > 0 needs probs_host and quant");
    QB_REQUIRE(theta && stats && row_out, "qbold_draw_summary: null theta/stats/row_out");
    QB_REQUIRE(hpd_mass > 0.0f && hpd_mass < 1.0f, "qbold_draw_summary: hpd_mass must lie strictly inside (0, 1)");
    Levels lv = {};
    for (int i = 0; i < P; ++i) {
        QB_REQUIRE(probs_host[i] > 0.0f && probs_host[i] < 1.0f,
                   "qbold_draw_summary: every level must lie strictly inside (0, 1)");
        lv.p[i] = probs_host[i];
    }
    if (N == 0) return QBOLD_OK;
    if (P == 0) quant = nullptr;
    const int64_t blocks = (N + kWaves - 1) / kWaves, cap = (int64_t)ctx->num_cus * 8;
    const int grid = (int)(blocks < cap ? blocks : cap);
#define QB_LAUNCH_SUMMARY(NJ)                                                                                       \
    hipLaunchKernelGGL(draw_summary_kernel<NJ>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, log_w, theta, C,  \
                       mask, K, lv, P, hpd_mass, stats, quant, row_out, corr, N)
    if (K <= 64) QB_LAUNCH_SUMMARY(1);
    else if (K <= 128) QB_LAUNCH_SUMMARY(2);
    else if (K <= 256) QB_LAUNCH_SUMMARY(4);
    else if (K <= 512) QB_LAUNCH_SUMMARY(8);
    else QB_LAUNCH_SUMMARY(16);
#undef QB_LAUNCH_SUMMARY
    QB_HIP(hipGetLastError());
    return QBOLD_OK;
}
