// design_kernels.hip -- Fisher information of the fine-tuning likelihood at given points (OEF, DBV), the Cramer-Rao
// bounds that follow from it, and the scores of many tau-protocol designs (per-tau numbers of averages) at once, on any
// tau grid (1 <= T <= QB_MAX_T).  include/qbold_hip.h, qbold_fisher_information and qbold_design_scores, states the
// definitions that tests/_design_reference.py restates in float64; this file is their float32 form.
//
// The rows are laplace_kernel's (laplace_kernels.hip): j_t = (d yhat_t / da, d yhat_t / db) / sigma_t from
// signal_grad.h's sig_eval / slope_factors, the table's own F without Simpson node 0's slope, the one or three images
// of the normalisation window evaluated first.  Both kernels here form them through the same two functions (row_setup,
// row_at), square them ONCE per tau into p_t = (jo^2, jo jd, jd^2) and weight the squares, I = sum_t w_t p_t in tau
// order by one FMA each, so that qbold_design_scores' per-voxel values are qbold_fisher_information's to the bit.
//
// fisher_kernel: laplace_kernel's shape -- 128 threads, one lane per voxel, FwdLds in LDS, one pass over t for the three
// sums.  One pass reads each 1 / sigma once, so sigma is read where it is used and no [t][thread] column is staged.
//
// design_kernel<TP>: one lane per voxel, a wave per fixed 64-voxel tile, four waves (256 consecutive voxels) per block.
// The 3 T squares of a lane live in REGISTERS (TP = T rounded up to 16, the tail zero), filled by one unrolled pass.
// Per-thread LDS columns ([t][thread], 12 T bytes per thread) would be 96 KiB per 128 threads at T = 64: two waves per
// CU and an LDS read per FMA.  In registers the tile's state is 192 VGPRs at T = 64 (one wave per SIMD there, two up to T = 32), and
// the only LDS traffic of the inner loop is the weights.  The designs come in chunks of 16: the block stages the
// chunk's weight rows in LDS, zero-padded to TP; every wave reads them at wave-uniform addresses (broadcast
// ds_read_b128, no bank conflicts, a VGPR operand for the FMAs) and runs four designs abreast, 12 independent FMA
// chains over t.  Each design closes with the 2 x 2 arithmetic of close2x2 per lane.
// Sums.  The four values of 16 designs go to a per-wave staging image in LDS (rows padded to 65 floats: the transposed
// read below is conflict-free); lane (design d, value k) then adds its row over the tile's 64 voxels in lane order, in
// double, each value times its voxel's mask weight.  The block adds its four waves' partials in wave order and writes
// one double per (256-voxel tile, design, value) to the workspace; design_sum_kernel adds the tiles in tile order.
// Tiles are fixed by the voxel index, never by the launch grid: the sums are the same bits at any grid and run to run.
// No atomics, no random stream.
#include <cmath>

#include "elbo_core.h"
#include "qbold_ctx.h"
#include "signal_grad.h"

namespace qb {
bool elbo_fast_path(const qbold_ctx* ctx);   // elbo_kernels.hip
int elbo_grid(const qbold_ctx* ctx);
}  // namespace qb

namespace {

// The two kernels promise each other's bits, so nothing written in this file is left to the compiler's choice between a
// fused and an unfused multiply-add: every FMA below is an explicit fmaf.
#pragma clang fp contract(off)

constexpr int kFisBlock = 128;
constexpr int kDesBlock = 256, kDesWaves = kDesBlock / 64;
constexpr int kChunk = 16;                 // designs per staged chunk
constexpr int kStageRow = 65;              // floats per staging row: 64 voxels + 1 of padding
constexpr float kSingular = 9.5367431640625e-7f;   // 2^-20 (qbold_hip.h, flag bit 0)

// forward_transform's range ends with the part float32 drops of them, so that OEF - 0.04 keeps its digits 1e-4 from
// the end (0.04f alone is 8.9e-10 off: 9e-6 of that distance)
constexpr float kOefLo = 0.04f, kOefLoR = (float)(0.04 - (double)0.04f);
constexpr float kOefHi = 0.84f, kOefHiR = (float)(0.84 - (double)0.84f);
constexpr float kDbvLo = 0.001f, kDbvLoR = (float)(0.001 - (double)0.001f);
constexpr float kDbvHi = 0.201f, kDbvHiR = (float)(0.201 - (double)0.201f);
static_assert(kOefLo == QB_MIN_OEF && kDbvLo == QB_MIN_DBV, "forward_transform's ranges");

// a point (OEF, DBV): the slopes of forward_transform there, d OEF / da = 0.8 s (1 - s) with s = (OEF - 0.04) / 0.8, and
// of R2' = dw OEF DBV; ok = inside the transforms' open ranges
struct Point {
    float oef, dbv, da, db, ra, rb;
    bool ok;
};
__device__ __forceinline__ Point make_point(const QbDev& c, float oef, float dbv) {
    Point p;
    p.oef = oef;
    p.dbv = dbv;
    const float xo = (oef - kOefLo) - kOefLoR, yo = (kOefHi - oef) + kOefHiR;
    const float xd = (dbv - kDbvLo) - kDbvLoR, yd = (kDbvHi - dbv) + kDbvHiR;
    p.ok = xo > 0.0f && yo > 0.0f && xd > 0.0f && yd > 0.0f;   // false for NaN
    p.da = xo * yo * (1.0f / QB_OEF_RANGE);
    p.db = xd * yd * (1.0f / QB_DBV_RANGE);
    p.ra = c.dw_coef * dbv * p.da;
    p.rb = c.dw_coef * oef * p.db;
    return p;
}

// what the rows of one point share: the signal's factors, the normaliser's slopes over the window and 1 / (n + 1e-3)
struct RowSetup {
    qb::FwdFast fv;
    qb::SlopeFactors k;
    float no, nd, inv_np;
};
struct Sig {
    float s, ds_doef, ds_ddbv;
};
// laplace_kernels.hip's lap_signal: the table's own slope (SigEval::dFu alone, no node 0 term)
__device__ __forceinline__ Sig signal_at(const qb::FwdLds* L, const RowSetup& r, int t) {
    const qb::SigEval e = qb::sig_eval(L, r.fv, t);
    Sig g;
    g.s = e.tissue + e.blood;   // sig_eval's s, the sum formed here (unfused in both kernels)
    g.ds_doef = e.ds_doef(r.k, e.dFu());
    g.ds_ddbv = e.ds_ddbv(r.k);
    return g;
}
__device__ __forceinline__ RowSetup row_setup(const QbDev& c, const qb::VoxColumns& vx, float oef, float dbv) {
    RowSetup r;
    r.fv = qb::fwd_fast(c, oef, dbv);
    r.k = qb::slope_factors(c, r.fv, oef, dbv, vx.dbw);
    float ns = 0.0f, no = 0.0f, nd = 0.0f;
    for (int t = vx.w_lo; t <= vx.w_hi; ++t) {
        const Sig g = signal_at(vx.L, r, t);
        ns += g.s;
        no += g.ds_doef;
        nd += g.ds_ddbv;
    }
    r.no = no * vx.w_se;
    r.nd = nd * vx.w_se;
    r.inv_np = qb::rcpf_(ns * vx.w_se + 1e-3f);
    return r;
}
// the squares of row t: (d yhat_t / d OEF / sigma_t)^2, the mixed product, (d yhat_t / d DBV / sigma_t)^2
struct Squares {
    float oo, od, dd;
};
__device__ __forceinline__ Squares row_at(const qb::FwdLds* L, const RowSetup& r, int t, float inv_s) {
    const Sig g = signal_at(L, r, t);
    const float yp = g.s * r.inv_np;
    const float ws = r.inv_np * inv_s;
    const float jo = fmaf(-yp, r.no, g.ds_doef) * ws;
    const float jd = fmaf(-yp, r.nd, g.ds_ddbv) * ws;
    Squares q;
    q.oo = jo * jo;
    q.od = jo * jd;
    q.dd = jd * jd;
    return q;
}

// det of the symmetric 2 x 2 matrix with the product's rounding error recovered (Kahan), as laplace_kernel has it
__device__ __forceinline__ float det2(float aaa, float aab, float abb) {
    const float w = aab * aab;
    const float e = fmaf(-aab, aab, w);
    return fmaf(aaa, abb, -w) + e;
}

// log det and, through Sigma = M^-1, the delta-method variances of OEF, DBV and R2' (laplace_kernel's columns 8 - 10,
// squared) of a symmetric 2 x 2 information matrix M on the logit plane
struct Closed {
    float log_det, var_oef, var_dbv, var_r2p;
};
__device__ __forceinline__ Closed close2x2(const Point& p, float maa, float mab, float mbb, float det) {
    const float inv = qb::rcpf_(det);
    const float v_aa = mbb * inv, v_bb = maa * inv, v_ab = -mab * inv;
    Closed o;
    o.log_det = logf(det);
    o.var_oef = p.da * p.da * v_aa;
    o.var_dbv = p.db * p.db * v_bb;
    o.var_r2p = fmaxf(fmaf(p.ra * p.ra, v_aa, fmaf(2.0f * p.ra * p.rb, v_ab, p.rb * p.rb * v_bb)), 0.0f);
    return o;
}

// the prior precision Lambda = L_p^-T L_p^-1 of raw heads, as laplace_kernel adds it to its curvature
struct Precision {
    float aa, ab, bb;
};
__device__ __forceinline__ Precision prior_precision(const float pv[5]) {
    const qb::LogitMvn pm = qb::make_mvn(pv);
    Precision l;
    l.aa = fmaf(pm.i_so, pm.i_so, pm.i_bl * pm.i_bl);
    l.ab = pm.i_bl * pm.i_sd;
    l.bb = pm.i_sd * pm.i_sd;
    return l;
}

__global__ __launch_bounds__(kFisBlock) void fisher_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ theta, const float* __restrict__ sigma,
    int sigma_shared, const float* __restrict__ weights, const float* __restrict__ prior,
    const float* __restrict__ mask, float* __restrict__ out, int64_t N) {
    extern __shared__ __align__(16) unsigned char smem[];
    qb::FwdLds* L = reinterpret_cast<qb::FwdLds*>(smem);
    qb::fwd_lds_fill(L, g_tab, false);
    if (threadIdx.x < QB_MAX_T) L->blood_B[threadIdx.x] = c.blood_B[threadIdx.x];
    __syncthreads();
    qb::VoxColumns vx;
    qb::vox_window(c, vx);
    vx.L = L;
    vx.yt = vx.is = nullptr;
    const int T = c.T;

    const int64_t ntile = (N + kFisBlock - 1) / kFisBlock;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t v = tile * kFisBlock + threadIdx.x;
        if (v >= N) continue;
        float* ov = out + v * QBOLD_FISHER_OUT;
        const float m = mask ? mask[v] : 1.0f;
        if (!(m > 0.0f)) {   // masked out (or NaN)
#pragma unroll
            for (int i = 0; i < QBOLD_FISHER_OUT; ++i) ov[i] = NAN;
            continue;
        }
        const Point p = make_point(c, theta[v * 2 + 0], theta[v * 2 + 1]);
        if (!p.ok) {
#pragma unroll
            for (int i = 0; i < QBOLD_FISHER_OUT - 1; ++i) ov[i] = NAN;
            ov[QBOLD_FISHER_OUT - 1] = 2.0f;
            continue;
        }
        const RowSetup r = row_setup(c, vx, p.oef, p.dbv);
        const float* sv = sigma + (sigma_shared ? 0 : v * T);
        float soo = 0.0f, sod = 0.0f, sdd = 0.0f;
        for (int t = 0; t < T; ++t) {
            const Squares q = row_at(L, r, t, qb::rcpf_(sv[t]));
            const float w = weights ? weights[t] : 1.0f;
            soo = fmaf(w, q.oo, soo);
            sod = fmaf(w, q.od, sod);
            sdd = fmaf(w, q.dd, sdd);
        }
        // the data information on the logit plane
        const float iaa = p.da * p.da * soo, iab = p.da * p.db * sod, ibb = p.db * p.db * sdd;
        const float det = det2(iaa, iab, ibb);
        const float spread = fmaf(iaa, ibb, iab * iab);
        const bool singular = !(det > kSingular * spread);
        ov[0] = iaa;
        ov[1] = iab;
        ov[2] = ibb;
        if (singular) {
            ov[3] = INFINITY;
            ov[4] = -INFINITY;
            ov[5] = ov[6] = ov[7] = INFINITY;
            ov[8] = NAN;
        } else {
            const Closed d = close2x2(p, iaa, iab, ibb, det);
            ov[3] = spread / det;
            ov[4] = d.log_det;
            ov[5] = sqrtf(d.var_oef);
            ov[6] = sqrtf(d.var_dbv);
            ov[7] = sqrtf(d.var_r2p);
            ov[8] = -iab / sqrtf(iaa * ibb);
        }
        if (prior) {
            float pv[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) pv[i] = prior[v * 5 + i];
            const Precision l = prior_precision(pv);
            const float aaa = fmaf(p.da * p.da, soo, l.aa), aab = fmaf(p.da * p.db, sod, l.ab),
                        abb = fmaf(p.db * p.db, sdd, l.bb);
            const Closed d = close2x2(p, aaa, aab, abb, det2(aaa, aab, abb));
            ov[9] = sqrtf(d.var_oef);
            ov[10] = sqrtf(d.var_dbv);
            ov[11] = sqrtf(d.var_r2p);
            ov[12] = -aab / sqrtf(aaa * abb);
            ov[13] = d.log_det;
        } else {
            ov[9] = ov[10] = ov[11] = ov[12] = ov[13] = NAN;
        }
        ov[14] = singular ? 1.0f : 0.0f;
    }
}

// LDS image of design_kernel behind FwdLds
template <int TP>
struct DesignLds {
    float wts[kChunk * TP];                              // [design][t], zero beyond B and beyond T
    float mk[kDesWaves][64];                             // mask weight of each voxel of the wave's tile, 0 = out
    float stage[kDesWaves][kChunk * 4][kStageRow];       // [design][value][voxel]
    double part[kDesWaves][64];                          // the waves' partial sums of one chunk
};
static_assert(sizeof(qb::FwdLds) % 16 == 0, "the weights start 16-byte aligned behind FwdLds");
static_assert(sizeof(qb::FwdLds) + sizeof(DesignLds<QB_MAX_T>) <= 80 * 1024, "design_kernel: two blocks per CU");

template <int TP>
__global__ __launch_bounds__(kDesBlock) void design_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ theta, const float* __restrict__ sigma,
    int sigma_shared, const float* __restrict__ weights, const float* __restrict__ prior,
    const float* __restrict__ mask, float* __restrict__ per_voxel, double* __restrict__ ws, int64_t N, int64_t B) {
    extern __shared__ __align__(16) unsigned char smem[];
    qb::FwdLds* L = reinterpret_cast<qb::FwdLds*>(smem);
    DesignLds<TP>* D = reinterpret_cast<DesignLds<TP>*>(smem + sizeof(qb::FwdLds));
    qb::fwd_lds_fill(L, g_tab, false);
    if (threadIdx.x < QB_MAX_T) L->blood_B[threadIdx.x] = c.blood_B[threadIdx.x];
    __syncthreads();
    qb::VoxColumns vx;
    qb::vox_window(c, vx);
    vx.L = L;
    vx.yt = vx.is = nullptr;
    const int T = c.T;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;

    const int64_t nblk = (N + kDesBlock - 1) / kDesBlock;   // 256-voxel tiles; a wave's tile is 64 voxels of one
    double* wsm = ws + nblk * B * 4;                        // behind the partials: the tiles' mask sums
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t v = blk * kDesBlock + threadIdx.x;
        const bool in = v < N;
        const bool wave_in = blk * kDesBlock + wave * 64 < N;   // wave-uniform: the wave's tile holds a voxel
        const float m = in ? (mask ? mask[v] : 1.0f) : 0.0f;
        const bool live = m > 0.0f;   // false for NaN
        Point p = make_point(c, live ? theta[v * 2 + 0] : 0.4f, live ? theta[v * 2 + 1] : 0.05f);
        float pv[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) pv[i] = live ? prior[v * 5 + i] : 0.0f;
        const Precision l = prior_precision(pv);
        const float daa = p.da * p.da, dab = p.da * p.db, dbb = p.db * p.db;
        // the squares of this voxel's rows, in registers; a point outside the ranges poisons its values (and the sums)
        float poo[TP], pod[TP], pdd[TP];
        {
            const RowSetup r = row_setup(c, vx, p.oef, p.dbv);
            const float* sv = sigma + ((sigma_shared || !live) ? 0 : v * T);
            const float bad = p.ok ? 0.0f : NAN;
#pragma unroll
            for (int t = 0; t < TP; ++t) {
                poo[t] = pod[t] = pdd[t] = 0.0f;
                if (t < T) {
                    const Squares q = row_at(L, r, t, qb::rcpf_(sv[t]));
                    poo[t] = q.oo + bad;
                    pod[t] = q.od + bad;
                    pdd[t] = q.dd + bad;
                }
            }
        }
        D->mk[wave][lane] = live ? m : 0.0f;

        for (int64_t b0 = 0; b0 < B; b0 += kChunk) {
            __syncthreads();   // the previous chunk's weights, staging image and partials have been read
            for (int i = threadIdx.x; i < kChunk * TP; i += kDesBlock) {
                const int d = i / TP, t = i % TP;
                D->wts[i] = (b0 + d < B && t < T) ? weights[(b0 + d) * T + t] : 0.0f;
            }
            __syncthreads();
            if (wave_in) {
                for (int g = 0; g < kChunk; g += 4) {
                    float acc[4][3];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 0.0f;
#pragma unroll
                    for (int t = 0; t < TP; t += 4) {
                        float4 w[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) w[j] = *reinterpret_cast<const float4*>(&D->wts[(g + j) * TP + t]);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float wj[4] = {w[j].x, w[j].y, w[j].z, w[j].w};
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                acc[j][0] = fmaf(wj[u], poo[t + u], acc[j][0]);
                                acc[j][1] = fmaf(wj[u], pod[t + u], acc[j][1]);
                                acc[j][2] = fmaf(wj[u], pdd[t + u], acc[j][2]);
                            }
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float aaa = fmaf(daa, acc[j][0], l.aa), aab = fmaf(dab, acc[j][1], l.ab),
                                    abb = fmaf(dbb, acc[j][2], l.bb);
                        const Closed d = close2x2(p, aaa, aab, abb, det2(aaa, aab, abb));
                        const int row = (g + j) * 4;
                        D->stage[wave][row + 0][lane] = live ? d.log_det : 0.0f;
                        D->stage[wave][row + 1][lane] = live ? d.var_oef : 0.0f;
                        D->stage[wave][row + 2][lane] = live ? d.var_dbv : 0.0f;
                        D->stage[wave][row + 3][lane] = live ? d.var_r2p : 0.0f;
                        const int64_t b = b0 + g + j;
                        if (per_voxel && in && b < B)
                            *reinterpret_cast<float4*>(per_voxel + (b * N + v) * 4) =
                                live ? make_float4(d.log_det, d.var_oef, d.var_dbv, d.var_r2p)
                                     : make_float4(NAN, NAN, NAN, NAN);
                    }
                }
            }
            __syncthreads();   // the staging image is complete
            // lane (design lane / 4, value lane % 4) adds its row over the tile's voxels in lane order
            double s = 0.0;
            if (wave_in) {
                const float* row = D->stage[wave][lane];
                for (int u = 0; u < 64; ++u) s = fma((double)row[u], (double)D->mk[wave][u], s);
            }
            D->part[wave][lane] = s;
            __syncthreads();
            if (wave == 0) {
                double tot = D->part[0][lane];
#pragma unroll
                for (int k = 1; k < kDesWaves; ++k) tot += D->part[k][lane];
                const int64_t b = b0 + (lane >> 2);
                if (b < B) ws[(blk * B + b) * 4 + (lane & 3)] = tot;
            }
        }
        __syncthreads();   // mk is complete (B = 0 runs no chunk)
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int k = 0; k < kDesWaves; ++k)
                for (int u = 0; u < 64; ++u) s += (double)D->mk[k][u];
            wsm[blk] = s;
        }
        __syncthreads();   // before the next tile overwrites mk
    }
}

// scores[b] = the sums of the 256-voxel tiles' partials in tile order; one thread per (design, value)
__global__ __launch_bounds__(256) void design_sum_kernel(const double* __restrict__ ws, double* __restrict__ scores,
                                                         int64_t nblk, int64_t B) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B * 4) return;
    const double* wsm = ws + nblk * B * 4;
    double s = 0.0, sm = 0.0;
    for (int64_t blk = 0; blk < nblk; ++blk) {
        s += ws[blk * B * 4 + i];
        sm += wsm[blk];
    }
    const int64_t b = i >> 2;
    const int k = (int)(i & 3);
    scores[b * QBOLD_DESIGN_OUT + k] = s;
    if (k == 0) scores[b * QBOLD_DESIGN_OUT + 4] = sm;
}

int unsupported(const char* what) {
    qb::set_error(std::string(what) + ": built for the full signal model in table mode with the Gaussian likelihood on "
                                      "linear data (either normalisation)");
    return QBOLD_ERR_UNSUPPORTED;
}

template <int TP>
int launch_design(const qbold_ctx* ctx, const float* theta, const float* sigma, int shared, const float* weights,
                  const float* prior, const float* mask, float* per_voxel, double* ws, int64_t N, int64_t B,
                  hipStream_t s) {
    const int64_t nblk = (N + kDesBlock - 1) / kDesBlock;
    const int cap = 2 * ctx->num_cus;   // two blocks per CU are resident
    const int grid = (int)(nblk < cap ? nblk : cap);
    const size_t smem = sizeof(qb::FwdLds) + sizeof(DesignLds<TP>);
    if (smem > 64 * 1024)
        QB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(design_kernel<TP>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(design_kernel<TP>, dim3(grid), dim3(kDesBlock), smem, s, ctx->dev, ctx->d_tab, theta, sigma,
                       shared, weights, prior, mask, per_voxel, ws, N, B);
    QB_HIP(hipGetLastError());
    return QBOLD_OK;
}

}  // namespace

extern "C" int qbold_fisher_information(const qbold_ctx* ctx, const float* theta, const float* sigma,
                                        int64_t sigma_rows, const float* weights, const float* prior,
                                        const float* mask, float* out, int64_t N, void* stream) {
    QB_NEED_DEVICE(ctx);
    QB_REQUIRE(N >= 0, "qbold_fisher_information: need N >= 0");
    QB_REQUIRE(out, "qbold_fisher_information: null out");
    QB_REQUIRE(N == 0 || (theta && sigma), "qbold_fisher_information: null input buffer");
    QB_REQUIRE(sigma_rows == 1 || sigma_rows == N, "qbold_fisher_information: sigma_rows must be 1 or N");
    hipStream_t s = (hipStream_t)stream;
    const int T = ctx->dev.T;
    if (weights && T >= 1 && T <= QB_MAX_T) {
        // the one place an entry waits for its stream: the T weights are read back to be checked
        float hw[QB_MAX_T];
        QB_HIP(hipMemcpyAsync(hw, weights, sizeof(float) * T, hipMemcpyDeviceToHost, s));
        QB_HIP(hipStreamSynchronize(s));
        for (int t = 0; t < T; ++t)
            QB_REQUIRE(hw[t] >= 0.0f && hw[t] < INFINITY, "qbold_fisher_information: weights must be finite and >= 0");
    }
    if (!qb::elbo_fast_path(ctx)) return unsupported("qbold_fisher_information");
    QB_REQUIRE(T >= 1 && T <= QB_MAX_T, "qbold_fisher_information: need 1 <= T <= 64");
    if (N == 0) return QBOLD_OK;
    const int64_t ntile = (N + kFisBlock - 1) / kFisBlock;
    const int cap = 2 * qb::elbo_grid(ctx);
    const int grid = (int)(ntile < cap ? ntile : cap);
    hipLaunchKernelGGL(fisher_kernel, dim3(grid), dim3(kFisBlock), sizeof(qb::FwdLds), s, ctx->dev, ctx->d_tab, theta,
                       sigma, sigma_rows == 1 ? 1 : 0, weights, prior, mask, out, N);
    QB_HIP(hipGetLastError());
    return QBOLD_OK;
}

extern "C" int64_t qbold_design_workspace_bytes(const qbold_ctx* ctx, int64_t N, int64_t B) {
    if (!ctx || N < 0 || B < 0) return QBOLD_ERR_INVALID;
    const int64_t nblk = (N + kDesBlock - 1) / kDesBlock;
    if (B > 0 && nblk > (INT64_MAX / 64) / B) return QBOLD_ERR_INVALID;
    const int64_t bytes = (int64_t)sizeof(double) * (nblk * B * 4 + nblk);
    return bytes > 8 ? bytes : 8;
}

extern "C" int qbold_design_scores(const qbold_ctx* ctx, const float* theta, const float* sigma, int64_t sigma_rows,
                                   const float* weights, const float* prior, const float* mask, double* scores,
                                   float* per_voxel, void* workspace, int64_t N, int64_t B, void* stream) {
    QB_NEED_DEVICE(ctx);
    QB_REQUIRE(N >= 0 && B >= 0, "qbold_design_scores: need N >= 0 and B >= 0");
    QB_REQUIRE(B == 0 || (scores && workspace), "qbold_design_scores: null scores / workspace");
    QB_REQUIRE(N == 0 || B == 0 || (theta && sigma && weights && prior), "qbold_design_scores: null input buffer");
    QB_REQUIRE(sigma_rows == 1 || sigma_rows == N, "qbold_design_scores: sigma_rows must be 1 or N");
    QB_REQUIRE(qbold_design_workspace_bytes(ctx, N, B) > 0, "qbold_design_scores: N B beyond int64");
    QB_REQUIRE(B == 0 || (reinterpret_cast<uintptr_t>(workspace) % 8 == 0 &&
                          (!per_voxel || reinterpret_cast<uintptr_t>(per_voxel) % 16 == 0)),
               "qbold_design_scores: workspace must be 8-byte and per_voxel 16-byte aligned");
    if (!qb::elbo_fast_path(ctx)) return unsupported("qbold_design_scores");
    const int T = ctx->dev.T;
    QB_REQUIRE(T >= 1 && T <= QB_MAX_T, "qbold_design_scores: need 1 <= T <= 64");
    if (B == 0) return QBOLD_OK;
    hipStream_t s = (hipStream_t)stream;
    double* ws = static_cast<double*>(workspace);
    const int shared = sigma_rows == 1 ? 1 : 0;
    int rc = QBOLD_OK;
    if (N > 0) {
        if (T <= 16) rc = launch_design<16>(ctx, theta, sigma, shared, weights, prior, mask, per_voxel, ws, N, B, s);
        else if (T <= 32) rc = launch_design<32>(ctx, theta, sigma, shared, weights, prior, mask, per_voxel, ws, N, B, s);
        else if (T <= 48) rc = launch_design<48>(ctx, theta, sigma, shared, weights, prior, mask, per_voxel, ws, N, B, s);
        else rc = launch_design<64>(ctx, theta, sigma, shared, weights, prior, mask, per_voxel, ws, N, B, s);
        if (rc != QBOLD_OK) return rc;
    }
    const int64_t nblk = (N + kDesBlock - 1) / kDesBlock;
    hipLaunchKernelGGL(design_sum_kernel, dim3((unsigned)((B * 4 + 255) / 256)), dim3(256), 0, s, ws, scores, nblk, B);
    QB_HIP(hipGetLastError());
    return QBOLD_OK;
}
