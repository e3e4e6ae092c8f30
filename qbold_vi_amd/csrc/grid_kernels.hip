// grid_kernels.hip -- exact per-voxel posteriors of the fine-tuning model by quadrature on the logit plane.  The
// latent space is two-dimensional (u = (a, b), the logits of OEF and DBV; sigma fixed), so the posterior is a 2-D
// integral of the log-joint
//   J(u) = -nll(x | OEF(clip a), DBV(clip b); sigma) + log N(u; mu_p, Sigma_p)
// (the sigmoid Jacobians cancel), evaluated on equal-weight grids: `locate` coarse passes shrink a start box to where
// J is within `cut` of its maximum, one fine pass integrates (include/qbold_hip.h, qbold_posterior_grid, states the
// definition the float64 reference of the tests restates).
//
// One wave per voxel.  Lanes run over the grid's columns (DBV) and a loop runs over its rows (OEF): a 16- or
// 32-column grid puts 4 or 2 rows side by side, a wider one takes ceil(n / 64) steps per row.  Per node: one
// likelihood evaluation (the ELBO / IW kernels' per-draw code, elbo_core.h: per-tau table, merged mirror pairs,
// literal Simpson, the general likelihood, or the generic kernel's tau loop for other T), the prior's whitened
// quadratic form and two exponentials.  Nothing is stored per node:
//   * locate pass: per-row maxima in LDS (one float per row), per-column maxima in registers;
//   * fine pass: a running maximum M of J; per lane and column, relative to M, sum w, sum w dOEF, sum w dOEF^2
//     (dOEF = OEF - OEF_ref, OEF_ref at the last locate pass's maximum, so that float32 does not cancel), the even-row
//     sum (Z_2h) and the outer ring's sum; per row, its own maximum and its sum relative to it (LDS), so that no
//     shift has to be known in advance and a sharp peak the coarse passes missed cannot overflow.  OEF depends on
//     the row only and DBV on the column only, so every moment -- R2' = dw OEF DBV included -- follows from those
//     column sums; the marginals are the row sums and column sums, their quantiles a wave prefix scan.
// Reductions are xor butterflies and fixed-order scans: a voxel's outputs do not depend on the batch it is in, and
// the masked sums are doubles in a fixed order (iw_kernels.hip's), so there are no atomics.
#include <cmath>

#include "elbo_core.h"
#include "qbold_ctx.h"

namespace qb {
bool elbo_fast_path(const qbold_ctx* ctx);   // elbo_kernels.hip
int elbo_grid(const qbold_ctx* ctx);
}  // namespace qb

namespace {

constexpr int kBlock = 256;                 // 4 waves, one voxel each
constexpr int kWaves = kBlock / QB_WAVE;
constexpr int kMaxN = 256;                  // the largest grid side (fine)
constexpr int kMaxChunks = kMaxN / QB_WAVE;
constexpr int kMaxGh = 32;
constexpr float kLog2Pi = 1.8378770664093453f;

// Gauss-Hermite rule, nodes t_k and weights w_k / sqrt(pi) (sum 1), computed on the host in double.
struct GhRule {
    int n;
    float t[kMaxGh], w[kMaxGh];
};

struct GridArgs {
    int coarse, fine, locate;
    float span, cut, level_lo, level_hi;
};

// ---- wave reductions (xor butterflies: every lane ends with the same value, the same bits) ----
__device__ __forceinline__ float seg_max(float v, int width) {
    for (int o = 1; o < width; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float seg_sum(float v, int width) {
    for (int o = 1; o < width; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_sum(float v) { return seg_sum(v, 64); }
__device__ __forceinline__ float wave_max(float v) { return seg_max(v, 64); }
// (J, row-major index) of the larger J; a tie goes to the lower index
__device__ __forceinline__ void wave_argmax(float& j, int& idx) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float j2 = __shfl_xor(j, o, 64);
        const int i2 = __shfl_xor(idx, o, 64);
        if (j2 > j || (j2 == j && i2 < idx)) {
            j = j2;
            idx = i2;
        }
    }
}
// LDS written by some lanes of a wave and read by others: order the wave's accesses
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ float exp_(float v) { return qb::exp2f_(v * QB_LOG2E); }

// The lane geometry of one pass over an n x n grid: R rows side by side (n = 16, 32), or one row in `nch` steps.
struct Geo {
    int n, R, width, nch, steps;
    __device__ __forceinline__ explicit Geo(int n_) : n(n_) {
        R = (n <= 32 && 64 % n == 0) ? 64 / n : 1;
        width = R > 1 ? n : 64;
        nch = R > 1 ? 1 : (n + 63) / 64;
        steps = R > 1 ? n / R : n * nch;
    }
    // node of this lane at step s: row, column, column chunk (this lane's register slot), validity
    __device__ __forceinline__ void at(int s, int lane, int& row, int& col, int& k, bool& ok) const {
        if (R > 1) {
            row = s * R + lane / n;
            col = lane % n;
            k = 0;
        } else {
            row = s / nch;
            k = s % nch;
            col = k * 64 + lane;
        }
        ok = col < n;
    }
};

// log N(u; prior) in whitened form (make_mvn's parameters)
__device__ __forceinline__ float prior_logpdf(const qb::LogitMvn& p, float a, float b) {
    const float w0 = (a - p.mu_o) * p.i_so;
    const float w1 = fmaf(b - p.mu_d, p.i_sd, (a - p.mu_o) * p.i_bl);
    return fmaf(-0.5f, fmaf(w0, w0, w1 * w1), -(p.s_o + p.s_d) - kLog2Pi);
}

struct Box {
    float a0, a1, b0, b1;
};

// One locate pass over box `bx`: per-row maxima (LDS), per-column maxima (registers), then the kept range widened by
// one step and intersected with bx.  Also the pass's argmax node (the reference point of the fine pass).
template <class Eval>
__device__ __forceinline__ Box locate_pass(const Eval& ev, const qb::LogitMvn& pm, const Box& bx, int n, float cut,
                                           float* rmax, float& ref_a, float& ref_b) {
    const int lane = threadIdx.x & 63;
    const Geo g(n);
    const float ha = (bx.a1 - bx.a0) / (float)(n - 1), hb = (bx.b1 - bx.b0) / (float)(n - 1);
    float cmax[kMaxChunks];
#pragma unroll
    for (int k = 0; k < kMaxChunks; ++k) cmax[k] = -INFINITY;
    float best = -INFINITY, rm = -INFINITY;
    int bidx = 0x7fffffff;
#pragma unroll 1
    for (int s = 0; s < g.steps; ++s) {
        int row, col, k;
        bool ok;
        g.at(s, lane, row, col, k, ok);
        const float a = fmaf((float)row, ha, bx.a0), b = fmaf((float)col, hb, bx.b0);
        float J = ev.log_lik(a, b) + prior_logpdf(pm, a, b);
        J = (ok && J == J) ? J : -INFINITY;
        if (J > best) {
            best = J;
            bidx = row * n + col;
        }
#pragma unroll
        for (int kk = 0; kk < kMaxChunks; ++kk)
            if (kk == k) cmax[kk] = fmaxf(cmax[kk], J);
        const float sm = seg_max(J, g.width);
        rm = (g.R > 1 || k == 0) ? sm : fmaxf(rm, sm);
        if ((g.R > 1 ? col == 0 : lane == 0) && (g.R > 1 || k == g.nch - 1)) rmax[row] = rm;
    }
    wave_lds_sync();
    wave_argmax(best, bidx);
    const float M = best;
    Box nb = bx;
    if (!(M > -INFINITY)) return nb;
    ref_a = fmaf((float)(bidx / n), ha, bx.a0);
    ref_b = fmaf((float)(bidx % n), hb, bx.b0);
    const float thr = M - cut;
    int r0 = n, r1 = -1, c0 = n, c1 = -1;
#pragma unroll
    for (int m = 0; m < kMaxChunks; ++m) {
        if (64 * m >= n) break;
        const int i = 64 * m + lane;
        const uint64_t rb = __ballot(i < n && rmax[i < n ? i : 0] > thr);
        // columns: R > 1 folds the side-by-side rows first
        float cm = cmax[m];
        if (g.R > 1)
            for (int o = n; o < 64; o <<= 1) cm = fmaxf(cm, __shfl_xor(cm, o, 64));
        const uint64_t cb = __ballot(i < n && cm > thr);
        if (rb) {
            r0 = min(r0, 64 * m + (int)__builtin_ctzll(rb));
            r1 = max(r1, 64 * m + 63 - (int)__builtin_clzll(rb));
        }
        if (cb) {
            c0 = min(c0, 64 * m + (int)__builtin_ctzll(cb));
            c1 = max(c1, 64 * m + 63 - (int)__builtin_clzll(cb));
        }
    }
    wave_lds_sync();   // rmax is rewritten by the next pass
    nb.a0 = fmaxf(bx.a0, fmaf((float)(r0 - 1), ha, bx.a0));
    nb.a1 = fminf(bx.a1, fmaf((float)(r1 + 1), ha, bx.a0));
    nb.b0 = fmaxf(bx.b0, fmaf((float)(c0 - 1), hb, bx.b0));
    nb.b1 = fminf(bx.b1, fmaf((float)(c1 + 1), hb, bx.b0));
    return nb;
}

// Quantiles at levels p0 < p1 of a marginal held as masses m[k] at index 64 k + lane (n of them, nodes x0 + i h):
// each node's mass spread uniformly over its cell [x_i - h/2, x_i + h/2], so the CDF is linear within a cell.
__device__ __forceinline__ void marginal_quantiles(const float (&m)[kMaxChunks], int n, float x0, float h, float p0,
                                                   float p1, float& q0, float& q1) {
    const int lane = threadIdx.x & 63;
    float cinc[kMaxChunks];
    float carry = 0.0f;
#pragma unroll
    for (int k = 0; k < kMaxChunks; ++k) {
        float v = m[k];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float u = __shfl_up(v, o, 64);
            if (lane >= o) v += u;
        }
        cinc[k] = v + carry;
        carry = __shfl(cinc[k], 63, 64);
    }
    const float total = carry;
    float qs[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const float t = (e == 0 ? p0 : p1) * total;
        int first = n - 1;
        float cexc = 0.0f, mi = 0.0f;
#pragma unroll
        for (int k = kMaxChunks - 1; k >= 0; --k) {
            const uint64_t bal = __ballot(64 * k + lane < n && cinc[k] >= t && m[k] > 0.0f);
            if (bal) {
                const int l = (int)__builtin_ctzll(bal);
                first = 64 * k + l;
                mi = __shfl(m[k], l, 64);
                cexc = __shfl(cinc[k], l, 64) - mi;
            }
        }
        const float fr = mi > 0.0f ? fminf(fmaxf((t - cexc) / mi, 0.0f), 1.0f) : 0.5f;
        qs[e] = fmaf((float)first - 0.5f + fr, h, x0);
    }
    q0 = qs[0];
    q1 = qs[1];
}

struct GridOut {
    float v[QBOLD_GRID_OUT];
    Box box;
};

// E_q[nll] by the gh x gh product Gauss-Hermite rule in q's whitened coordinates, u = mu_q + L_q sqrt(2) t
template <class Eval>
__device__ __forceinline__ float gh_expected_nll(const Eval& ev, const qb::LogitMvn& qm, const GhRule& gh) {
    const int lane = threadIdx.x & 63;
    const int nn = gh.n * gh.n;
    float acc = 0.0f;
#pragma unroll 1
    for (int base = 0; base < nn; base += 64) {
        const int i = base + lane;
        if (i < nn) {
            const int k = i / gh.n, l = i - k * gh.n;
            const float t0 = 1.4142135623730951f * gh.t[k], t1 = 1.4142135623730951f * gh.t[l];
            float a, b;
            qb::reparam_logits(qm, t0, t1, a, b);
            a = qb::clampf_(a, -QB_LOGIT_CLIP, QB_LOGIT_CLIP);
            b = qb::clampf_(b, -QB_LOGIT_CLIP, QB_LOGIT_CLIP);
            acc = fmaf(gh.w[k] * gh.w[l], -ev.log_lik(a, b), acc);
        }
    }
    return wave_sum(acc);
}

// KL(q || p) of two logit-space Gaussians, closed form (refine_kernels.hip's kl_closed_grad without the gradient)
__device__ __forceinline__ float kl_closed(const qb::LogitMvn& q, const qb::LogitMvn& p) {
    const float dmu_o = q.mu_o - p.mu_o, dmu_d = q.mu_d - p.mu_d;
    const float d0 = dmu_o * p.i_so, d1 = fmaf(dmu_d, p.i_sd, dmu_o * p.i_bl);
    const float m00 = q.e_so * p.i_so, m10 = fmaf(q.c, p.i_sd, q.e_so * p.i_bl), m11 = q.e_sd * p.i_sd;
    const float sq = fmaf(m00, m00, fmaf(m10, m10, fmaf(m11, m11, fmaf(d0, d0, d1 * d1))));
    return fmaf(0.5f, sq, (p.s_o + p.s_d) - (q.s_o + q.s_d) - 1.0f);
}

__device__ __forceinline__ void grow_box(Box& b, const qb::LogitMvn& m, float span) {
    const float sa = m.e_so, sb = sqrtf(fmaf(m.c, m.c, m.e_sd * m.e_sd));
    b.a0 = fminf(b.a0, fmaf(-span, sa, m.mu_o));
    b.a1 = fmaxf(b.a1, fmaf(span, sa, m.mu_o));
    b.b0 = fminf(b.b0, fmaf(-span, sb, m.mu_d));
    b.b1 = fmaxf(b.b1, fmaf(span, sb, m.mu_d));
}

__device__ __forceinline__ float oef_of(float a) { return fmaf(qb::sigmoidf_(a), QB_OEF_RANGE, QB_MIN_OEF); }
__device__ __forceinline__ float dbv_of(float b) { return fmaf(qb::sigmoidf_(b), QB_DBV_RANGE, QB_MIN_DBV); }

// Everything of one voxel (all lanes of the wave; every lane ends with the same GridOut).
template <class Eval>
__device__ __forceinline__ void grid_voxel(const Eval& ev, const QbDev& c, const qb::LogitMvn& pm,
                                           const qb::LogitMvn& qm, bool has_q, const GridArgs& ga, const GhRule& gh,
                                           float* rmax, float* rsum, GridOut& o) {
    const int lane = threadIdx.x & 63;
    // 1. the start box
    Box bx{INFINITY, -INFINITY, INFINITY, -INFINITY};
    grow_box(bx, pm, ga.span);
    if (has_q) grow_box(bx, qm, ga.span);
    bx.a0 = qb::clampf_(bx.a0, -QB_LOGIT_CLIP, QB_LOGIT_CLIP);
    bx.a1 = qb::clampf_(bx.a1, -QB_LOGIT_CLIP, QB_LOGIT_CLIP);
    bx.b0 = qb::clampf_(bx.b0, -QB_LOGIT_CLIP, QB_LOGIT_CLIP);
    bx.b1 = qb::clampf_(bx.b1, -QB_LOGIT_CLIP, QB_LOGIT_CLIP);
    // 2. locate passes
    float ref_a = 0.5f * (bx.a0 + bx.a1), ref_b = 0.5f * (bx.b0 + bx.b1);
#pragma unroll 1
    for (int p = 0; p < ga.locate; ++p) bx = locate_pass(ev, pm, bx, ga.coarse, ga.cut, rmax, ref_a, ref_b);
    // 3. the fine pass
    const int n = ga.fine;
    const Geo g(n);
    const float ha = (bx.a1 - bx.a0) / (float)(n - 1), hb = (bx.b1 - bx.b0) / (float)(n - 1);
    const float o_ref = oef_of(ref_a), d_ref = dbv_of(ref_b);
    float s0[kMaxChunks], s1[kMaxChunks], s2[kMaxChunks], se[kMaxChunks], sr[kMaxChunks];
#pragma unroll
    for (int k = 0; k < kMaxChunks; ++k) s0[k] = s1[k] = s2[k] = se[k] = sr[k] = 0.0f;
    float M = -INFINITY, rm = -INFINITY, rs = 0.0f, best = -INFINITY;
    int bidx = 0x7fffffff;
#pragma unroll 1
    for (int s = 0; s < g.steps; ++s) {
        int row, col, k;
        bool ok;
        g.at(s, lane, row, col, k, ok);
        const float a = fmaf((float)row, ha, bx.a0), b = fmaf((float)col, hb, bx.b0);
        float J = ev.log_lik(a, b) + prior_logpdf(pm, a, b);
        J = (ok && J == J) ? J : -INFINITY;
        if (J > best) {
            best = J;
            bidx = row * n + col;
        }
        // the running maximum over everything so far; the column sums follow it
        const float sm = seg_max(J, g.width);
        const float stepmax = g.R > 1 ? wave_max(sm) : sm;
        if (stepmax > M) {
            const float sc = exp_(M - stepmax);
#pragma unroll
            for (int kk = 0; kk < kMaxChunks; ++kk) {
                s0[kk] *= sc;
                s1[kk] *= sc;
                s2[kk] *= sc;
                se[kk] *= sc;
                sr[kk] *= sc;
            }
            M = stepmax;
        }
        // this row's own maximum and its sum relative to it
        const float rm_new = (g.R > 1 || k == 0) ? sm : fmaxf(rm, sm);
        const float rm_s = rm_new > -INFINITY ? rm_new : 0.0f;
        const float wr = exp_(J - rm_s);
        const float part = seg_sum(wr, g.width);
        rs = (g.R > 1 || k == 0) ? part : fmaf(rs, exp_((rm > -INFINITY ? rm : rm_s) - rm_s), part);
        rm = rm_new;
        if ((g.R > 1 ? col == 0 : lane == 0) && (g.R > 1 || k == g.nch - 1)) {
            rmax[row] = rm;
            rsum[row] = rs;
        }
        const float w = exp_(J - M);   // M is finite once any J is; J = -inf gives 0
        const float dO = oef_of(a) - o_ref;
        const float wd = w * dO;
        const bool even = (row & 1) == 0;
        const bool ring = row == 0 || row == n - 1 || col == 0 || col == n - 1;
#pragma unroll
        for (int kk = 0; kk < kMaxChunks; ++kk)
            if (kk == k) {
                s0[kk] += w;
                s1[kk] += wd;
                s2[kk] = fmaf(wd, dO, s2[kk]);
                if (even) se[kk] += w;
                if (ring) sr[kk] += w;
            }
    }
    wave_lds_sync();
    wave_argmax(best, bidx);
    // 4. the per-voxel results
    float Z = 0.0f, S1 = 0.0f, S2 = 0.0f, Ed = 0.0f, Edd = 0.0f, Eod = 0.0f, Eg = 0.0f, Egg = 0.0f, Se = 0.0f, Sr = 0.0f;
    float cm[kMaxChunks];   // the DBV marginal: column sums at column 64 k + lane
    const float dw = c.dw_coef;
#pragma unroll
    for (int k = 0; k < kMaxChunks; ++k) {
        const int col = g.R > 1 ? lane % n : 64 * k + lane;
        const bool ok = g.R > 1 ? k == 0 : col < n;
        const float dbv = dbv_of(fmaf((float)col, hb, bx.b0));
        const float dd = dbv - d_ref;
        const float a0 = ok ? s0[k] : 0.0f, a1 = ok ? s1[k] : 0.0f, a2 = ok ? s2[k] : 0.0f;
        Z += a0;
        S1 += a1;
        S2 += a2;
        Ed = fmaf(a0, dd, Ed);
        Edd = fmaf(a0 * dd, dd, Edd);
        Eod = fmaf(a1, dd, Eod);
        // R2' - R2'_ref = dw (dOEF DBV + OEF_ref dDBV)
        Eg = fmaf(a1, dbv, fmaf(a0 * o_ref, dd, Eg));
        Egg = fmaf(a2 * dbv, dbv, fmaf(2.0f * a1 * dbv, o_ref * dd, fmaf(a0 * (o_ref * dd), o_ref * dd, Egg)));
        if (ok && (col & 1) == 0) Se += se[k];
        if (ok) Sr += sr[k];
        float cs = a0;
        if (g.R > 1)
            for (int off = n; off < 64; off <<= 1) cs += __shfl_xor(cs, off, 64);
        cm[k] = (g.R > 1 ? (k == 0 && lane < n) : ok) ? cs : 0.0f;
    }
    Z = wave_sum(Z);
    S1 = wave_sum(S1);
    S2 = wave_sum(S2);
    Ed = wave_sum(Ed);
    Edd = wave_sum(Edd);
    Eod = wave_sum(Eod);
    Eg = wave_sum(Eg);
    Egg = wave_sum(Egg);
    Se = wave_sum(Se);
    Sr = wave_sum(Sr);
    const float iZ = 1.0f / Z;
    const float eo = S1 * iZ, ed = Ed * iZ, eg = Eg * iZ;
    const float vo = fmaxf(fmaf(S2, iZ, -eo * eo), 0.0f), vd = fmaxf(fmaf(Edd, iZ, -ed * ed), 0.0f);
    const float vg = fmaxf(fmaf(Egg, iZ, -eg * eg), 0.0f);
    const float cov = fmaf(Eod, iZ, -eo * ed);
    const float logZ = M + logf(Z);
    o.v[0] = logZ + (logf(ha) + logf(hb));
    o.v[2] = o_ref + eo;
    o.v[3] = d_ref + ed;
    o.v[4] = dw * fmaf(o_ref, d_ref, eg);
    o.v[5] = sqrtf(vo);
    o.v[6] = sqrtf(vd);
    o.v[7] = fabsf(dw) * sqrtf(vg);
    o.v[8] = cov / (sqrtf(vo) * sqrtf(vd));
    // the OEF marginal: the rows' sums, each relative to its own maximum
    float rmass[kMaxChunks];
#pragma unroll
    for (int k = 0; k < kMaxChunks; ++k) {
        const int i = 64 * k + lane;
        rmass[k] = i < n ? rsum[i] * exp_(rmax[i] > -INFINITY ? rmax[i] - M : -INFINITY) : 0.0f;
    }
    wave_lds_sync();   // rmax / rsum are rewritten by the next voxel
    float qa0, qa1, qb0, qb1;
    marginal_quantiles(rmass, n, bx.a0, ha, ga.level_lo, ga.level_hi, qa0, qa1);
    marginal_quantiles(cm, n, bx.b0, hb, ga.level_lo, ga.level_hi, qb0, qb1);
    o.v[9] = oef_of(qa0);
    o.v[10] = oef_of(qa1);
    o.v[11] = dbv_of(qb0);
    o.v[12] = dbv_of(qb1);
    o.v[13] = oef_of(fmaf((float)(bidx / n), ha, bx.a0));
    o.v[14] = dbv_of(fmaf((float)(bidx % n), hb, bx.b0));
    o.v[15] = Sr * iZ;
    o.v[16] = fabsf(logf(Z) - logf(4.0f * Se));
    o.v[1] = NAN;
    if (has_q && gh.n > 0) o.v[1] = -gh_expected_nll(ev, qm, gh) - kl_closed(qm, pm);
    o.box = bx;
}

// ---- node evaluators: log p(x | u) at logits (a, b) inside the clip ----

// T = 11 / 24 with the data in registers: the IW kernel's per-draw likelihood (iw_draws)
template <int T, int SE, bool FAST, bool LITERAL, bool MIR, class LDS>
struct RegEval {
    const LDS* L;
    const QbDev* c;
    const qb::VoxelLik<T>* lik;
    __device__ __forceinline__ float log_lik(float a, float b) const {
        if constexpr (FAST && qb::IsGtLds<LDS>::value) {
            return -fmaf(0.5f, qb::sample_sq_fast<T, SE>(L, *c, *lik, qb::sigmoidf_(a), qb::sigmoidf_(b)),
                         lik->log_s_sum);
        } else {
            float oef, dbv;
            qb::forward_transform(a, b, oef, dbv);
            if constexpr (FAST) return -fmaf(0.5f, qb::sample_sq_fast<T, SE, MIR>(L, *c, *lik, oef, dbv), lik->log_s_sum);
            else return -qb::sample_nll<T, SE, LITERAL>(L, *c, *lik, oef, dbv);
        }
    }
};

template <int T, int SE, bool GT>
struct GridLds { using type = qb::FwdLds; };
template <int T, int SE>
struct GridLds<T, SE, true> { using type = qb::GtLds<T, SE>; };

__device__ __forceinline__ void store_voxel(const GridOut& o, bool live, int64_t v, float m, float* __restrict__ out,
                                            float* __restrict__ box, double& s_lp, double& s_el, double& s_m) {
    const int lane = threadIdx.x & 63;
    if (lane < QBOLD_GRID_OUT) {
        float val = NAN;
#pragma unroll
        for (int i = 0; i < QBOLD_GRID_OUT; ++i)
            if (i == lane) val = o.v[i];
        out[v * QBOLD_GRID_OUT + lane] = live ? val : NAN;
    }
    if (box && lane < 4) {
        const float bv = lane == 0 ? o.box.a0 : lane == 1 ? o.box.a1 : lane == 2 ? o.box.b0 : o.box.b1;
        box[v * 4 + lane] = live ? bv : NAN;
    }
    if (live && lane == 0) {
        s_lp += (double)m * -(double)o.v[0];
        if (o.v[1] == o.v[1]) s_el += (double)m * -(double)o.v[1];
        s_m += (double)m;
    }
}

// Masked sums in doubles, fixed order (iw_kernels.hip's block_partials_d)
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ void block_partials_d(double* red, double a, double b, double m,
                                                 double* __restrict__ partials) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
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
        for (int w = 0; w < kWaves; ++w) s += red[3 * w + threadIdx.x];
        partials[3 * blockIdx.x + threadIdx.x] = s;
    }
}

template <int T, int SE, bool FAST, bool LITERAL, bool GT = false, bool MIR = false>
__global__ __launch_bounds__(kBlock) void grid_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* __restrict__ prior, const float* __restrict__ sigma, const float* __restrict__ q, GridArgs ga,
    GhRule gh, float* __restrict__ out, float* __restrict__ box, double* __restrict__ partials, int64_t N) {
    static_assert(!GT || (FAST && SE >= 0 && qb::gtab_segs(T) > 0), "GT needs the fast path with a compile-time spin echo");
    static_assert(!MIR || (FAST && SE >= 0), "merged mirror pairs: fast path with a compile-time spin echo");
    constexpr bool kMir = GT || MIR;
    using Lds = typename GridLds<T, SE, GT>::type;
    __shared__ Lds L;
    __shared__ float rows[kWaves][2][kMaxN];
    __shared__ double red[3 * kWaves];
    if constexpr (qb::IsGtLds<Lds>::value) {
        qb::gt_lds_fill(&L, g_tab, c);
    } else {
        qb::fwd_lds_fill(&L, g_tab, true);
        if (threadIdx.x < QB_MAX_T) L.blood_B[threadIdx.x] = c.blood_B[threadIdx.x];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    double s_lp = 0.0, s_el = 0.0, s_m = 0.0;
    for (int64_t v = (int64_t)blockIdx.x * kWaves + wave; v < N; v += (int64_t)gridDim.x * kWaves) {
        const float m = mask ? mask[v] : 1.0f;
        const bool live = m > 0.0f;
        GridOut o;
        if (live) {
            float xv[T], sv[T], pv[5], qv[5];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                xv[t] = x[v * T + t];
                sv[t] = sigma[v * T + t];
            }
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                pv[i] = prior[v * 5 + i];
                qv[i] = q ? q[v * 5 + i] : 0.0f;
            }
            qb::VoxelLik<T> lik;
            qb::prepare_lik<T, SE, false, (FAST && SE >= 0), FAST, kMir>(c, xv, sv, m, lik);
            const qb::LogitMvn pm = qb::make_mvn(pv), qm = qb::make_mvn(qv);
            const RegEval<T, SE, FAST, LITERAL, kMir, Lds> ev{&L, &c, &lik};
            grid_voxel(ev, c, pm, qm, q != nullptr, ga, gh, rows[wave][0], rows[wave][1], o);
        }
        store_voxel(o, live, v, m, out, box, s_lp, s_el, s_m);
    }
    block_partials_d(red, s_lp, s_el, s_m, partials);
}

// Any other tau count (table mode, Gaussian likelihood, linear data, as iw_fwd_generic_kernel): the normalised data
// and inverse sigmas of the wave's voxel in LDS, a run-time tau loop, mirrored pairs evaluated once when tau = 0 at
// the spin echo.  0.5 sum_t r_t^2 is iw_kernels.hip's generic_half_sq with one voxel per wave.
struct GenEval {
    const qb::FwdLds* L;
    const QbDev* c;
    const float* yt;   // [T]
    const float* is;   // [T]
    float log_s_sum;
    int T, se;
    bool mirrored;
    __device__ __forceinline__ float log_lik(float a, float b) const {
        float oef, dbv;
        qb::forward_transform(a, b, oef, dbv);
        const qb::FwdFast fv = qb::fwd_fast(*c, oef, dbv);
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
                const float r = (yt[t] - yh) * is[t];
                acc = fmaf(r, r, acc);
            };
            residual(se, s_se * inv_np);
            for (int t = se + 1; t < T; ++t) {
                const float yh = signal(t);
                residual(t, yh);
                if (2 * se - t >= 0) residual(2 * se - t, yh);
            }
            for (int t = 0; t < 2 * se - (T - 1); ++t) residual(t, signal(t));
        } else {
            float np_ = qb::fwd_signal_fast(L, *c, fv, se);
            if (c->multi_norm)
                np_ = (np_ + qb::fwd_signal_fast(L, *c, fv, se - 1) + qb::fwd_signal_fast(L, *c, fv, se + 1)) / 3.0f;
            const float inv_np = qb::rcpf_(np_ + 1e-3f);
            for (int t = 0; t < T; ++t) {
                const float st = qb::fwd_signal_fast(L, *c, fv, t);
                const float r = fmaf(-st, inv_np, yt[t]) * is[t];
                acc = fmaf(r, r, acc);
            }
        }
        return -fmaf(0.5f, acc, log_s_sum);
    }
};

__global__ __launch_bounds__(kBlock) void grid_generic_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* __restrict__ prior, const float* __restrict__ sigma, const float* __restrict__ q, GridArgs ga,
    GhRule gh, float* __restrict__ out, float* __restrict__ box, double* __restrict__ partials, int64_t N) {
    __shared__ qb::FwdLds L;
    __shared__ float rows[kWaves][2][kMaxN];
    __shared__ float yts[kWaves][2][QB_MAX_T];
    __shared__ double red[3 * kWaves];
    qb::fwd_lds_fill(&L, g_tab, false);
    if (threadIdx.x < QB_MAX_T) L.blood_B[threadIdx.x] = c.blood_B[threadIdx.x];
    __syncthreads();
    const int T = c.T, se = c.se_idx;
    const bool mirrored = !c.multi_norm && fmaf((float)se, c.tauh_step, c.tauh0) == 0.0f;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* yt = yts[wave][0];
    float* is = yts[wave][1];
    double s_lp = 0.0, s_el = 0.0, s_m = 0.0;
    for (int64_t v = (int64_t)blockIdx.x * kWaves + wave; v < N; v += (int64_t)gridDim.x * kWaves) {
        const float m = mask ? mask[v] : 1.0f;
        const bool live = m > 0.0f;
        GridOut o;
        if (live) {
            const float* xv = x + v * T;
            const float* sv = sigma + v * T;
            const float nt = c.multi_norm ? (xv[se - 1] + xv[se] + xv[se + 1]) / 3.0f + 1e-3f : xv[se] + 1e-3f;
            const float inv_nt = qb::rcpf_(nt);
            float ls = 0.0f;
            if (lane < T) {
                yt[lane] = xv[lane] * inv_nt;
                is[lane] = qb::rcpf_(sv[lane]);
                ls = QB_LN2 * qb::log2f_(sv[lane]);
            }
            wave_lds_sync();
            const float log_s_sum = wave_sum(ls) + (float)T * 0.9189385332046727f;
            float pv[5], qv[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                pv[i] = prior[v * 5 + i];
                qv[i] = q ? q[v * 5 + i] : 0.0f;
            }
            const qb::LogitMvn pm = qb::make_mvn(pv), qm = qb::make_mvn(qv);
            const GenEval ev{&L, &c, yt, is, log_s_sum, T, se, mirrored};
            grid_voxel(ev, c, pm, qm, q != nullptr, ga, gh, rows[wave][0], rows[wave][1], o);
            wave_lds_sync();   // yt / is are rewritten by the next voxel
        }
        store_voxel(o, live, v, m, out, box, s_lp, s_el, s_m);
    }
    block_partials_d(red, s_lp, s_el, s_m, partials);
}

// Gauss-Hermite nodes and weights (weight e^{-t^2}) by Newton on the orthonormal Hermite recurrence, in double;
// weights divided by sqrt(pi) so that they sum to 1.
void gauss_hermite(int n, GhRule& r) {
    r.n = n;
    const double pim4 = 0.7511255444649425;   // pi^{-1/4}
    const int m = (n + 1) / 2;
    double z = 0.0;
    for (int i = 0; i < m; ++i) {
        if (i == 0) z = std::sqrt(2.0 * n + 1.0) - 1.85575 * std::pow(2.0 * n + 1.0, -0.16667);
        else if (i == 1) z -= 1.14 * std::pow((double)n, 0.426) / z;
        else if (i == 2) z = 1.86 * z - 0.86 * r.t[0];
        else if (i == 3) z = 1.91 * z - 0.91 * r.t[1];
        else z = 2.0 * z - r.t[i - 2];
        double pp = 0.0;
        for (int it = 0; it < 100; ++it) {
            double p1 = pim4, p2 = 0.0;
            for (int j = 1; j <= n; ++j) {
                const double p3 = p2;
                p2 = p1;
                p1 = z * std::sqrt(2.0 / j) * p2 - std::sqrt((j - 1.0) / j) * p3;
            }
            pp = std::sqrt(2.0 * n) * p2;
            const double z1 = z;
            z = z1 - p1 / pp;
            if (std::fabs(z - z1) <= 1e-15 * std::fmax(1.0, std::fabs(z))) {
                // one more pass for the derivative at the converged node
                p1 = pim4;
                p2 = 0.0;
                for (int j = 1; j <= n; ++j) {
                    const double p3 = p2;
                    p2 = p1;
                    p1 = z * std::sqrt(2.0 / j) * p2 - std::sqrt((j - 1.0) / j) * p3;
                }
                pp = std::sqrt(2.0 * n) * p2;
                break;
            }
        }
        const double w = 2.0 / (pp * pp) / 1.7724538509055159;   // / sqrt(pi)
        r.t[i] = (float)z;   // kept as float: the recurrence above reads the previous nodes
        r.t[n - 1 - i] = (float)-z;
        r.w[i] = r.w[n - 1 - i] = (float)w;
    }
}

}  // namespace

extern "C" int qbold_posterior_grid(const qbold_ctx* ctx, const float* x, const float* mask, const float* prior,
                                    const float* sigma, const float* q, const qbold_grid_cfg* cfg, float* out,
                                    float* box, double* sums, void* workspace, int64_t N, void* stream) {
    QB_NEED_DEVICE(ctx);
    QB_REQUIRE(cfg, "qbold_posterior_grid: null cfg");
    QB_REQUIRE(N >= 0, "qbold_posterior_grid: need N >= 0");
    QB_REQUIRE(cfg->coarse % 8 == 0 && cfg->coarse >= 16 && cfg->coarse <= 128,
               "qbold_posterior_grid: coarse must be a multiple of 8 in [16, 128]");
    QB_REQUIRE(cfg->fine % 8 == 0 && cfg->fine >= 16 && cfg->fine <= kMaxN,
               "qbold_posterior_grid: fine must be a multiple of 8 in [16, 256]");
    QB_REQUIRE(cfg->locate >= 1 && cfg->locate <= 4, "qbold_posterior_grid: locate must be in [1, 4]");
    QB_REQUIRE(cfg->gh == 0 || (cfg->gh >= 2 && cfg->gh <= kMaxGh), "qbold_posterior_grid: gh must be 0 or in [2, 32]");
    QB_REQUIRE(cfg->span > 0.0f && cfg->span < INFINITY, "qbold_posterior_grid: need span > 0");
    QB_REQUIRE(cfg->cut >= 10.0f && cfg->cut <= 80.0f, "qbold_posterior_grid: cut must be in [10, 80]");
    QB_REQUIRE(cfg->level_lo > 0.0f && cfg->level_lo < cfg->level_hi && cfg->level_hi < 1.0f,
               "qbold_posterior_grid: need 0 < level_lo < level_hi < 1");
    QB_REQUIRE(out && sums && workspace, "qbold_posterior_grid: null out/sums/workspace");
    QB_REQUIRE(N == 0 || (x && prior && sigma), "qbold_posterior_grid: null input buffer");
    const bool lit = ctx->dev.tissue_mode == QBOLD_TISSUE_LITERAL;
    const bool fast = qb::elbo_fast_path(ctx);
    const int T = ctx->dev.T;
    if (T != 11 && T != 24 && !fast) {
        qb::set_error("qbold_posterior_grid: for T other than 11 / 24 only the optimal.yaml configuration (table "
                      "mode, Gaussian likelihood, linear data) is built");
        return QBOLD_ERR_UNSUPPORTED;
    }
    GridArgs ga{cfg->coarse, cfg->fine, cfg->locate, cfg->span, cfg->cut, cfg->level_lo, cfg->level_hi};
    GhRule gh{};
    if (q && cfg->gh > 0) gauss_hermite(cfg->gh, gh);
    hipStream_t s = (hipStream_t)stream;
    double* partials = reinterpret_cast<double*>(workspace);
    const int64_t nblk = (N + kWaves - 1) / kWaves;
    const int grid = (int)(nblk < qb::elbo_grid(ctx) ? (nblk > 0 ? nblk : 1) : qb::elbo_grid(ctx));
    const bool gt = ctx->gtab_ok && !(ctx->kernel_sel & 8) && qb::gtab_segs(T) > 0;
#define QB_GRID_ARGS ctx->dev, ctx->d_tab, x, mask, prior, sigma, q, ga, gh, out, box, partials, N
#define QB_LAUNCH_GRID(TT, SE, FAST, LIT) \
    hipLaunchKernelGGL((grid_kernel<TT, SE, FAST, LIT>), dim3(grid), dim3(kBlock), 0, s, QB_GRID_ARGS)
#define QB_LAUNCH_GRID_MIR(TT, SE) \
    hipLaunchKernelGGL((grid_kernel<TT, SE, true, false, false, true>), dim3(grid), dim3(kBlock), 0, s, QB_GRID_ARGS)
#define QB_LAUNCH_GRID_GT(TT, SE)                                                                                    \
    hipLaunchKernelGGL((grid_kernel<TT, SE, true, false, (qb::gtab_segs(TT) > 0)>), dim3(grid), dim3(kBlock), 0, s, \
                       ctx->dev, ctx->d_gtab, x, mask, prior, sigma, q, ga, gh, out, box, partials, N)
    // the dispatch of qbold_log_evidence_fwd (iw_kernels.hip)
    switch (T) {
        case 11:
            if (fast && ctx->dev.se_idx == 2 && !ctx->dev.multi_norm && gt) QB_LAUNCH_GRID_GT(11, 2);
            else if (fast && ctx->dev.se_idx == 2 && !ctx->dev.multi_norm && ctx->grid_mirrors) QB_LAUNCH_GRID_MIR(11, 2);
            else if (fast && ctx->dev.se_idx == 2 && !ctx->dev.multi_norm) QB_LAUNCH_GRID(11, 2, true, false);
            else if (fast) QB_LAUNCH_GRID(11, -1, true, false);
            else if (lit && ctx->dev.se_idx == 2 && !ctx->dev.multi_norm) QB_LAUNCH_GRID(11, 2, false, true);
            else if (lit) QB_LAUNCH_GRID(11, -1, false, true);
            else QB_LAUNCH_GRID(11, -1, false, false);
            break;
        case 24:
            if (fast && ctx->dev.se_idx == 7 && !ctx->dev.multi_norm && gt) QB_LAUNCH_GRID_GT(24, 7);
            else if (fast && ctx->dev.se_idx == 7 && !ctx->dev.multi_norm && ctx->grid_mirrors) QB_LAUNCH_GRID_MIR(24, 7);
            else if (fast && ctx->dev.se_idx == 7 && !ctx->dev.multi_norm) QB_LAUNCH_GRID(24, 7, true, false);
            else if (fast) QB_LAUNCH_GRID(24, -1, true, false);
            else if (lit && ctx->dev.se_idx == 7 && !ctx->dev.multi_norm) QB_LAUNCH_GRID(24, 7, false, true);
            else if (lit) QB_LAUNCH_GRID(24, -1, false, true);
            else QB_LAUNCH_GRID(24, -1, false, false);
            break;
        default:
            hipLaunchKernelGGL(grid_generic_kernel, dim3(grid), dim3(kBlock), 0, s, QB_GRID_ARGS);
    }
#undef QB_LAUNCH_GRID
#undef QB_LAUNCH_GRID_MIR
#undef QB_LAUNCH_GRID_GT
#undef QB_GRID_ARGS
    QB_HIP(hipGetLastError());
    hipLaunchKernelGGL(qb::reduce_partials_kernel, dim3(1), dim3(192), 0, s, partials, grid, sums);
    QB_HIP(hipGetLastError());
    return QBOLD_OK;
}
