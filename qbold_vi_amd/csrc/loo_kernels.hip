// loo_kernels.hip -- Pareto-smoothed importance-sampling leave-one-out cross-validation per voxel and per tau image
// (Vehtari, Gelman & Gabry 2017; for draws from a variational posterior Yao et al. 2018, Magnusson et al. 2019).
// The contract is qbold_loo's in include/qbold_hip.h.  Three stages on one stream:
//
//   1. loo_rows_kernel: per voxel the K draws of qbold_log_evidence_draws (explicit normals or Philox stream 6) and for
//      each draw the per-tau log density ll_{t,k} (ppc_kernels.hip's term, restated), log w_k = sum_t ll_{t,k} -
//      (log q - log p) (iw_kernels.hip's whitened / clipped form, restated: those files are untouched) and the rows
//      rho_{t,k} = log w_k - ll_{t,k}, row T = log w_k.
//   2. qbold_psis itself on the N (T + 1) rows, weights output on: nothing of the PSIS arithmetic is restated here.
//   3. loo_finalise_kernel: per voxel, over its T + 1 smoothed rows, elpd_t, lppd_t, the k^ columns and the masked sums.
//
// Rows kernel, lane mapping (the choice and its reason): a wave owns 16 voxels, the four lanes l, l + 16, l + 32, l + 48
// of a voxel split its TAUS (t = part, part + 4, ...), not its draws: a lane that owned draws would hold four draws x T
// log densities until a Philox call completes (256 VGPRs at T = 64).  All four lanes walk every draw (reparameterisation,
// fwd_fast and the spin-echo normaliser are computed four times over: 1 - 3 of the T signals), each scores its <= 16
// taus, four draws (one Philox call) at a time, and the voxel sum of the four partial sums is -nll.  The tau loop runs
// at run time (one kernel for every T <= 64, no mirrored-pair merge: each tau needs its own term); the normalised data,
// 1 / sigma and the per-tau constant sit in LDS rows [t][voxel], each slot written and read by one lane only, so the
// kernel has no barrier after the table fill.  A call's four log densities of a tau go out as one 16-byte piece of the
// loglik row (element stores when K is no multiple of 4 or for a short last call); once log w of the call is known the
// lane reads its own pieces back (same thread, program order) and writes the rho pieces.
//   Traffic per voxel: reads 4 (2 T + 11) bytes of inputs (+ 8 K of explicit normals); writes 4 T K (loglik) +
//     4 (T + 1) K (log_ratio) and reads the 4 T K of loglik back once.
//     Stage 2 reads 4 (T + 1) K and writes 4 (T + 1) K + 16 (T + 1); stage 3 reads 4 (2 T + 1) K + 16 (T + 1).
//   LDS per block (128 threads, 32 voxels): sizeof(FwdLds) = 5,936 + 3 x 64 x 32 x 4 = 30,512 bytes.
//   Compiler report (scripts/dev/so_resources.py, gfx950): loo_rows_kernel<true> 130 VGPRs, <false> 164 (three waves
//     per SIMD either way), loo_finalise_kernel 70, loo_reduce4_kernel 22; every kernel of this file has 0 bytes of
//     scratch, which tests/test_loo_host.py holds.
// Every sum is a fixed-order loop followed by a fixed butterfly; no atomics: a voxel's outputs are the same bits at any
// batch position, under any sharding by voxel0 and from run to run.
#include <cmath>
#include <type_traits>

#include "elbo_core.h"
#include "qbold_ctx.h"

namespace qb {
bool elbo_fast_path(const qbold_ctx* ctx);   // elbo_kernels.hip
int elbo_grid(const qbold_ctx* ctx);
}  // namespace qb

namespace {

constexpr int kRowsBlock = 128;
constexpr int kRowsVox = kRowsBlock / QB_LANES_PER_VOXEL;   // 32 voxels per block
constexpr int kFinWaves = 4;
constexpr int kFinBlock = 64 * kFinWaves;

// log q - log p of a draw in the whitened form (iw_kernels.hip, IwKl / iw_dswr, restated)
struct LooKl {
    float d0, d1, m00, m10, m11;
    float cst;   // (s_o + s_d)_p - (s_o + s_d)_q
};
__device__ __forceinline__ LooKl make_loo_kl(const qb::LogitMvn& q, const qb::LogitMvn& p) {
    LooKl k;
    const float dmu_o = q.mu_o - p.mu_o, dmu_d = q.mu_d - p.mu_d;
    k.d0 = dmu_o * p.i_so;
    k.m00 = q.e_so * p.i_so;
    k.d1 = fmaf(dmu_d, p.i_sd, dmu_o * p.i_bl);
    k.m10 = fmaf(q.c, p.i_sd, q.e_so * p.i_bl);
    k.m11 = q.e_sd * p.i_sd;
    k.cst = (p.s_o + p.s_d) - (q.s_o + q.s_d);
    return k;
}
__device__ __forceinline__ float loo_dswr(const LooKl& k, float z0, float z1) {   // swr_p - swr_q of one draw
    const float w0 = fmaf(k.m00, z0, k.d0);
    const float w1 = fmaf(k.m11, z1, fmaf(k.m10, z0, k.d1));
    return fmaf(w0, w0, w1 * w1) - fmaf(z0, z0, z1 * z1);
}

// the pieces of a row: draws d0 .. d0 + 3 of which cnt exist
__device__ __forceinline__ void store4(float* row, int d0, int cnt, bool vec, const float (&a)[4]) {
    if (vec && cnt == 4) {
        *reinterpret_cast<float4*>(row + d0) = make_float4(a[0], a[1], a[2], a[3]);
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < cnt) row[d0 + i] = a[i];
}
__device__ __forceinline__ void load4(const float* row, int d0, int cnt, bool vec, float (&a)[4]) {
    if (vec && cnt == 4) {
        const float4 v = *reinterpret_cast<const float4*>(row + d0);
        a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = i < cnt ? row[d0 + i] : 0.0f;
}

// One draw, the part that does not depend on tau: the forward model's per-draw factors, the reciprocal of the
// prediction's normaliser and log q - log p.
template <bool FAST>
struct LooDraw {
    typename std::conditional<FAST, qb::FwdFast, qb::FwdVox>::type fv;
    float inv_np, kl;
};

template <bool FAST>
__device__ __forceinline__ float loo_signal(const qb::FwdLds* L, const QbDev& c, const LooDraw<FAST>& d, int t) {
    if constexpr (FAST) return qb::fwd_signal_fast(L, c, d.fv, t);
    else return qb::fwd_signal<false>(L, c, d.fv, t);
}

// FAST: qbold_log_evidence_draws' generic configuration (full model from the table, Gaussian likelihood on linear data),
// its arithmetic per tau (iw_kernels.hip, generic_half_sq's plain loop).  Otherwise sample_nll's forward model and
// normalisation with every likelihood switch read at run time (T = 11 / 24, the host's dispatch).
template <bool FAST>
__global__ __launch_bounds__(kRowsBlock) void loo_rows_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* __restrict__ q, const float* __restrict__ prior, const float* __restrict__ sigma,
    const float* __restrict__ z, int K, uint64_t seed, int64_t voxel0, float* log_ratio, float* loglik, bool vec,
    int64_t N) {
    extern __shared__ __align__(16) unsigned char smem[];
    qb::FwdLds* L = reinterpret_cast<qb::FwdLds*>(smem);
    float* yt = reinterpret_cast<float*>(smem + sizeof(qb::FwdLds));   // [T][kRowsVox] normalised (logged) data
    float* is = yt + QB_MAX_T * kRowsVox;                               // [T][kRowsVox] 1 / sigma
    float* lc = is + QB_MAX_T * kRowsVox;                               // [T][kRowsVox] the per-tau constant
    qb::fwd_lds_fill(L, g_tab, !FAST);
    __syncthreads();

    const int T = c.T, se = c.se_idx;
    const bool student = !FAST && c.use_student_t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int part = lane >> 4;
    const int vl = wave * QB_VOX_PER_WAVE + (lane & 15);
    const float nan = __uint_as_float(0x7fc00000u);
    const int64_t ntile = (N + kRowsVox - 1) / kRowsVox;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t v = tile * kRowsVox + vl;
        if (v >= N) continue;   // the four lanes of a voxel share v: they stay together in every branch below
        float* ll_rows = loglik + v * T * (int64_t)K;
        float* lr_rows = log_ratio + v * (T + 1) * (int64_t)K;
        const float m = mask ? mask[v] : 1.0f;
        if (!(m > 0.0f)) {   // mask <= 0 or NaN: not read, NaN rows
            for (int t = part; t < T; t += QB_LANES_PER_VOXEL)
                for (int k = 0; k < K; ++k) {
                    ll_rows[(int64_t)t * K + k] = nan;
                    lr_rows[(int64_t)t * K + k] = nan;
                }
            if (part == 0)
                for (int k = 0; k < K; ++k) lr_rows[(int64_t)T * K + k] = nan;
            continue;
        }
        // the likelihood side of the voxel: this lane's taus into its own LDS slots (model.py:541-549)
        const float* xv = x + v * T;
        const float* sv = sigma + v * T;
        {
            const float nt = c.multi_norm ? (xv[se - 1] + xv[se] + xv[se + 1]) / 3.0f + 1e-3f : xv[se] + 1e-3f;
            const float inv_nt = qb::rcpf_(nt);
            for (int t = part; t < T; t += QB_LANES_PER_VOXEL) {
                float y = xv[t] * inv_nt;
                if (!FAST && c.predict_log) y = __logf(y);
                const float sg = sv[t];
                yt[t * kRowsVox + vl] = y;
                is[t * kRowsVox + vl] = qb::rcpf_(sg);
                lc[t * kRowsVox + vl] = student ? c.st_const - logf(sg) : -logf(sg) - 0.9189385332046727f;
            }
        }
        float qv[5], pv[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            qv[i] = q[v * 5 + i];
            pv[i] = prior[v * 5 + i];
        }
        const qb::LogitMvn qm = qb::make_mvn(qv), pm = qb::make_mvn(pv);
        const LooKl kl = make_loo_kl(qm, pm);
        const float* zv = z ? z + v * (int64_t)K * 2 : nullptr;
        const uint64_t vox = (uint64_t)(voxel0 + v);
        const int calls = (K + 3) >> 2;
#pragma unroll 1
        for (int g = 0; g < calls; ++g) {
            const int d0 = 4 * g;
            const int cnt = K - d0 < 4 ? K - d0 : 4;
            // the call's four draws (a short last call repeats draw K - 1 of explicit normals; its extra values are
            // never stored)
            LooDraw<FAST> dr[4];
            qb::DrawQuad dq;
            if (!zv) dq.load(seed, vox, (uint32_t)g, qb::STREAM_IW);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float z0, z1;
                if (zv) {
                    const int d = d0 + i < K ? d0 + i : K - 1;
                    z0 = zv[2 * d];
                    z1 = zv[2 * d + 1];
                } else {
                    dq.next(z0, z1);
                }
                float a, b, oef, dbv;
                qb::reparam_logits(qm, z0, z1, a, b);
                qb::forward_transform(a, b, oef, dbv);
                if constexpr (FAST) {
                    dr[i].fv = qb::fwd_fast(c, oef, dbv);
                    float np_ = qb::fwd_signal_fast(L, c, dr[i].fv, se);
                    if (c.multi_norm)
                        np_ = (np_ + qb::fwd_signal_fast(L, c, dr[i].fv, se - 1) +
                               qb::fwd_signal_fast(L, c, dr[i].fv, se + 1)) / 3.0f;
                    dr[i].inv_np = qb::rcpf_(np_ + 1e-3f);
                } else {
                    dr[i].fv = qb::fwd_vox(c, oef, dbv);
                    const float sb = qb::fwd_signal<false>(L, c, dr[i].fv, se);
                    float np_ = sb + 1e-3f;
                    if (c.multi_norm)
                        np_ = (qb::fwd_signal<false>(L, c, dr[i].fv, se - 1) + sb +
                               qb::fwd_signal<false>(L, c, dr[i].fv, se + 1)) / 3.0f + 1e-3f;
                    dr[i].inv_np = 1.0f / np_;
                }
                // the whitened log q - log p wherever the clip of the logits does not bind (there it is exact), the
                // clipped-logit form for a draw where it does: per draw, so a voxel's rows do not depend on its wave
                float dswr = loo_dswr(kl, z0, z1);
                if (fmaxf(fabsf(a), fabsf(b)) > QB_LOGIT_CLIP) dswr = qb::kl_swr_diff(qm, pm, z0, z1);
                dr[i].kl = fmaf(0.5f, dswr, kl.cst);
            }
            // this lane's taus: the per-tau log density of the four draws
            float part_sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
            for (int t = part; t < T; t += QB_LANES_PER_VOXEL) {
                const float y = yt[t * kRowsVox + vl], isv = is[t * kRowsVox + vl], lcv = lc[t * kRowsVox + vl];
                float ll[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float st = loo_signal<FAST>(L, c, dr[i], t);
                    float r;
                    if constexpr (FAST) {
                        r = fmaf(-st, dr[i].inv_np, y) * isv;
                    } else {
                        float yp = st * dr[i].inv_np;
                        if (c.predict_log) yp = __logf(yp);
                        r = (y - yp) * isv;
                    }
                    const float r2 = r * r;
                    const float core = student ? -0.5f * (c.st_df + 1.0f) * log1pf(r2 / c.st_df) : -0.5f * r2;
                    ll[i] = core + lcv;
                    part_sum[i] += ll[i];
                }
                store4(ll_rows + (int64_t)t * K, d0, cnt, vec, ll);
            }
            // log w = sum_t ll - (log q - log p): the same bits in the voxel's four lanes (the butterfly is symmetric)
            float lw[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) lw[i] = qb::voxel_sum(part_sum[i]) - dr[i].kl;
#pragma unroll 1
            for (int t = part; t < T; t += QB_LANES_PER_VOXEL) {
                float ll[4], rho[4];
                load4(ll_rows + (int64_t)t * K, d0, cnt, vec, ll);   // this lane's own stores
#pragma unroll
                for (int i = 0; i < 4; ++i) rho[i] = lw[i] - ll[i];
                store4(lr_rows + (int64_t)t * K, d0, cnt, vec, rho);
            }
            if (part == 0) store4(lr_rows + (int64_t)T * K, d0, cnt, vec, lw);
        }
    }
}

// ---- stage 3 ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum_f(float v) {   // a symmetric butterfly: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// One wave per voxel, lanes over the draws.  psis_out [N (T + 1)][4] and weights [N (T + 1)][K] are qbold_psis' outputs
// for the rows of log_ratio.  The sums over the taus run in doubles (p_loo is the small difference of two of them);
// the masked sums as ppc_kernels.hip's (block partials, then one reducing block).
__global__ __launch_bounds__(kFinBlock) void loo_finalise_kernel(
    const float* __restrict__ mask, const float* __restrict__ loglik, const float* __restrict__ weights,
    const float* __restrict__ psis_out, int T, int K, float* __restrict__ out, float* __restrict__ pointwise,
    double* __restrict__ partials, int64_t N) {
    __shared__ double red[4 * kFinWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float nan = __uint_as_float(0x7fc00000u);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};   // lane 0 of each wave
    for (int64_t v = (int64_t)blockIdx.x * kFinWaves + wave; v < N; v += (int64_t)gridDim.x * kFinWaves) {
        const float m = mask ? mask[v] : 1.0f;
        if (!(m > 0.0f)) {
            if (lane < QBOLD_LOO_OUT) out[QBOLD_LOO_OUT * v + lane] = nan;
            if (pointwise)
                for (int i = lane; i < 3 * T; i += 64) pointwise[v * 3 * T + i] = nan;
            continue;
        }
        const int64_t r0 = v * (T + 1);
        const float* wT = weights + (r0 + T) * K;
        double elpd = 0.0, lppd = 0.0;
        float kmax = 0.0f;
        int kidx = 0;
        for (int t = 0; t < T; ++t) {
            const float* ll = loglik + (v * T + t) * K;
            const float* wt = weights + (r0 + t) * K;
            float mt = -INFINITY;
            for (int k = lane; k < K; k += 64) mt = fmaxf(mt, ll[k]);
            mt = wave_max_f(mt);
            float se = 0.0f, sl = 0.0f;
            for (int k = lane; k < K; k += 64) {
                const float d = ll[k] - mt;
                se += expf(wt[k] + d);
                sl += expf(wT[k] + d);
            }
            const float e_t = mt + logf(wave_sum_f(se)), l_t = mt + logf(wave_sum_f(sl));
            const float kh = psis_out[4 * (r0 + t)];
            elpd += (double)e_t;
            lppd += (double)l_t;
            // the largest k^, the lowest tau attaining it; +inf beats every finite value and a NaN (a NaN row) beats all
            if (t == 0 || kh > kmax || (kh != kh && kmax == kmax)) {
                kmax = kh;
                kidx = t;
            }
            if (pointwise && lane == 0) {
                float* pw = pointwise + (v * T + t) * 3;
                pw[0] = e_t;
                pw[1] = kh;
                pw[2] = l_t;
            }
        }
        if (lane == 0) {
            const float e = (float)elpd, p = (float)(lppd - elpd);
            float* o = out + QBOLD_LOO_OUT * v;
            o[0] = e;
            o[1] = p;
            o[2] = (float)lppd;
            o[3] = kmax;
            o[4] = (float)kidx;
            o[5] = psis_out[4 * (r0 + T)];
            acc[0] += (double)m * (double)e;
            acc[1] += (double)m * (double)p;
            acc[2] += kmax > 0.7f ? (double)m : 0.0;
            acc[3] += (double)m;
        }
    }
    // lane 0 of each wave holds the wave's partial; the block's in wave order
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) red[4 * wave + k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double s = 0.0;
        for (int w = 0; w < kFinWaves; ++w) s += red[4 * w + threadIdx.x];
        partials[4 * blockIdx.x + threadIdx.x] = s;
    }
}

// ppc_kernels.hip's reduce4_kernel, restated: four columns of block partials in a fixed order
__global__ __launch_bounds__(256) void loo_reduce4_kernel(const double* __restrict__ partials, int nblocks,
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

// the workspace: [block partials][psis out][weights][log_ratio][loglik], each section on a 256-byte boundary
struct LooWorkspace {
    int64_t partials, psis_out, weights, log_ratio, loglik, total;
};
int64_t round256(int64_t b) { return (b + 255) & ~(int64_t)255; }
int fin_grid_cap(const qbold_ctx* ctx) { return ctx->num_cus * 8; }
LooWorkspace loo_workspace(const qbold_ctx* ctx, int K, int64_t N) {
    const int64_t T = ctx->dev.T, rows = N * (T + 1);
    LooWorkspace w;
    w.partials = 0;
    w.psis_out = w.partials + round256((int64_t)sizeof(double) * 4 * fin_grid_cap(ctx));
    w.weights = w.psis_out + round256(rows * 16);
    w.log_ratio = w.weights + round256(rows * K * 4);
    w.loglik = w.log_ratio + round256(rows * K * 4);
    w.total = w.loglik + round256(N * T * K * 4);
    return w;
}

}  // namespace

extern "C" int64_t qbold_loo_workspace_bytes(const qbold_ctx* ctx, int K, int64_t N) {
    if (!ctx || N < 0 || K < QBOLD_PSIS_MIN_K || K > QBOLD_PSIS_MAX_K) return QBOLD_ERR_INVALID;
    return loo_workspace(ctx, K, N).total;
}

extern "C" int qbold_loo(const qbold_ctx* ctx, const float* x, const float* mask, const float* q, const float* prior,
                         const float* sigma, const float* z, int K, uint64_t seed, int64_t voxel0, float* out,
                         float* pointwise, float* log_ratio, float* loglik, double* sums, void* workspace, int64_t N,
                         void* stream) {
    QB_NEED_DEVICE(ctx);
    QB_REQUIRE(N >= 0 && K >= QBOLD_PSIS_MIN_K && K <= QBOLD_PSIS_MAX_K,
               "qbold_loo: need N >= 0 and QBOLD_PSIS_MIN_K <= K <= QBOLD_PSIS_MAX_K");
    QB_REQUIRE(out && sums && workspace, "qbold_loo: null out/sums/workspace");
    QB_REQUIRE(N == 0 || (x && q && prior && sigma), "qbold_loo: null input buffer");
    hipStream_t s = (hipStream_t)stream;
    const int T = ctx->dev.T;
    const bool fast = qb::elbo_fast_path(ctx);
    if (ctx->dev.tissue_mode == QBOLD_TISSUE_LITERAL || (!fast && T != 11 && T != 24)) {
        qb::set_error("qbold_loo: built for table mode; for T other than 11 / 24 only the optimal.yaml configuration "
                      "(Gaussian likelihood, linear data)");
        return QBOLD_ERR_UNSUPPORTED;
    }
    if (N == 0) {
        QB_HIP(hipMemsetAsync(sums, 0, 4 * sizeof(double), s));
        return QBOLD_OK;
    }
    const LooWorkspace w = loo_workspace(ctx, K, N);
    unsigned char* base = reinterpret_cast<unsigned char*>(workspace);
    double* partials = reinterpret_cast<double*>(base + w.partials);
    float* psis_out = reinterpret_cast<float*>(base + w.psis_out);
    float* weights = reinterpret_cast<float*>(base + w.weights);
    // the caller's row buffers, when given, are where the rows are written: what the caller sees is what PSIS read
    float* lr = log_ratio ? log_ratio : reinterpret_cast<float*>(base + w.log_ratio);
    float* ll = loglik ? loglik : reinterpret_cast<float*>(base + w.loglik);
    const bool vec = (K & 3) == 0 && (reinterpret_cast<uintptr_t>(lr) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(ll) & 15) == 0;

    const int64_t rtile = (N + kRowsVox - 1) / kRowsVox;
    const int rgrid = (int)(rtile < qb::elbo_grid(ctx) ? rtile : qb::elbo_grid(ctx));
    const size_t smem = sizeof(qb::FwdLds) + sizeof(float) * 3 * QB_MAX_T * kRowsVox;
    if (fast)
        hipLaunchKernelGGL(loo_rows_kernel<true>, dim3(rgrid), dim3(kRowsBlock), smem, s, ctx->dev, ctx->d_tab, x, mask,
                           q, prior, sigma, z, K, seed, voxel0, lr, ll, vec, N);
    else
        hipLaunchKernelGGL(loo_rows_kernel<false>, dim3(rgrid), dim3(kRowsBlock), smem, s, ctx->dev, ctx->d_tab, x, mask,
                           q, prior, sigma, z, K, seed, voxel0, lr, ll, vec, N);
    QB_HIP(hipGetLastError());

    // every row through qbold_psis as that entry defines it; the rows of a voxel outside the mask are NaN rows
    const int rc = qbold_psis(ctx, lr, nullptr, 0, nullptr, K, psis_out, nullptr, weights, N * (T + 1), stream);
    if (rc != QBOLD_OK) return rc;

    const int64_t fblocks = (N + kFinWaves - 1) / kFinWaves;
    const int fgrid = (int)(fblocks < fin_grid_cap(ctx) ? fblocks : fin_grid_cap(ctx));
    hipLaunchKernelGGL(loo_finalise_kernel, dim3(fgrid), dim3(kFinBlock), 0, s, mask, ll, weights, psis_out, T, K, out,
                       pointwise, partials, N);
    QB_HIP(hipGetLastError());
    hipLaunchKernelGGL(loo_reduce4_kernel, dim3(1), dim3(256), 0, s, partials, fgrid, sums);
    QB_HIP(hipGetLastError());
    return QBOLD_OK;
}
