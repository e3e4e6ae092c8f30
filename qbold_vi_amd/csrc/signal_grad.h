// signal_grad.h -- the forward signal of the full model in table mode TOGETHER WITH its slopes in (OEF, DBV): the one
// copy of the device code that the gradient kernels share.
//   * fwd_signal_grad: compile-time-T kernels (blood_B from QbDev, the index unrolled): elbo_bwd_kernel, the
//     importance-weighted backward (iw_bwd_kernels.hip) and the refinement kernels specialised for 11 / 24 taus.
//   * sig_eval / SigEval / slope_factors: run-time-T kernels, one lane per voxel (blood_B from LDS, the segment index
//     clamped): the any-T refinement kernels and laplace_kernel.
//   * VoxColumns / vox_window / vox_columns: those kernels' per-thread [t][thread] LDS columns and normalisation window.
// elbo_bwd_generic_kernel keeps a signal evaluation of its own (elbo_bwd_kernels.hip says how it differs).
#pragma once
#include "elbo_core.h"

namespace qb {

struct FwdGrad {
    float s, ds_doef, ds_ddbv;
};

// signal and its partials at tau index t (full model, table mode)
__device__ __forceinline__ FwdGrad fwd_signal_grad(const FwdLds* L, const QbDev& c, const FwdFast& v, float oef,
                                                   float dbv, int t) {
    const float us = fmaf((float)t, v.ub, v.ua);  // signed table coordinate
    const float u = fabsf(us);
    const int i = min((int)u, QB_TAB_SEG - 1);
    const float f = u - (float)i;
    const float4 k = L->tab[i];
    const float F = fmaf(fmaf(fmaf(k.w, f, k.z), f, k.y), f, k.x);
    // dF/dx at |x| (x = u / tab_inv_h), plus node 0's slope; d|x|/doef = |x| / oef
    const float ax = u * (1.0f / c.tab_inv_h);
    const float dF = fmaf(fmaf(3.0f * k.w, f, 2.0f * k.z), f, k.y) * c.tab_inv_h + c.dF_node0 * ax;
    const float e1 = exp2f_(v.nd * F);
    const float e2 = exp2f_(v.ng * c.blood_B[t]);
    const float tissue = v.tissue_w * e1, blood = v.blood_w * e2;
    FwdGrad g;
    g.s = tissue + blood;
    const float inv_oef = rcpf_(oef);
    // tissue: exp(-dbv F(x)), x proportional to oef;  blood: exp(-g B), g proportional to oef^2
    g.ds_doef = -dbv * dF * ax * inv_oef * tissue +
                (2.0f * QB_LN2) * v.ng * c.blood_B[t] * inv_oef * blood;
    // weights: tissue_w = (1 - bw) C1, blood_w = bw C2, bw = m_bld_nb dbv (or dbv without blood)
    const float dbw = c.include_blood ? c.m_bld_nb : 1.0f;
    g.ds_ddbv = -F * tissue - dbw * c.e_te_r2t * e1 + (c.include_blood ? dbw * c.e_r2b_te * e2 : 0.0f);
    return g;
}

// ---- run-time T ------------------------------------------------------------------------------------------------------
// The factors of the slopes that depend on the point (OEF, DBV) only, not on tau: tissue exp(-dbv F(x)), x
// proportional to oef; blood exp(-g B), g proportional to oef^2; weights tissue_w = (1 - bw) C1, blood_w = bw C2,
// bw = dbw dbv
struct SlopeFactors {
    float ko, kb, kd1, kd2;
};
__device__ __forceinline__ SlopeFactors slope_factors(const QbDev& c, const FwdFast& fv, float oef, float dbv,
                                                      float dbw) {
    const float inv_oef = rcpf_(oef);
    SlopeFactors p;
    p.ko = -dbv * inv_oef;
    p.kb = (2.0f * QB_LN2) * fv.ng * inv_oef;
    p.kd1 = dbw * c.e_te_r2t;
    p.kd2 = c.include_blood ? dbw * c.e_r2b_te : 0.0f;
    return p;
}

// fwd_signal_fast at tau index t, keeping what the slopes need; blood_B from LDS (t is a run-time index)
struct SigEval {
    float s, tissue, blood, F, e1, e2, u, f, B;
    float4 k;
    // |x| dF/dx at x = u / tab_inv_h, the cubic's own slope in u: d|x| / d oef = |x| / oef.  The table's F drops
    // Simpson node 0 and so does this slope; a caller that wants the node's slope (QbDev::dF_node0, as the training
    // gradients have it) adds n0 u^2 itself -- the Laplace kernel must not, and adding it there with n0 = 0 would
    // cost instructions and could flip the sign of a zero.
    __device__ __forceinline__ float dFu() const { return fmaf(fmaf(3.0f * k.w, f, 2.0f * k.z), f, k.y) * u; }
    __device__ __forceinline__ float ds_doef(const SlopeFactors& p, float dfu) const {
        return fmaf(p.ko * dfu, tissue, p.kb * B * blood);
    }
    __device__ __forceinline__ float ds_ddbv(const SlopeFactors& p) const {
        return fmaf(p.kd2, e2, -fmaf(F, tissue, p.kd1 * e1));
    }
};
// The segment index is clamped: forward_transform bounds OEF by 0.84 and the table spans OEF <= 1, so the clamp never
// binds for a finite point and keeps a NaN or infinite one inside the table.
__device__ __forceinline__ SigEval sig_eval(const FwdLds* L, const FwdFast& v, int t) {
    SigEval g;
    g.u = fabsf(fmaf((float)t, v.ub, v.ua));
    const int i = min(max((int)g.u, 0), QB_TAB_SEG - 1);
    g.f = __builtin_amdgcn_fractf(g.u);
    g.k = L->tab[i];
    g.F = fmaf(fmaf(fmaf(g.k.w, g.f, g.k.z), g.f, g.k.y), g.f, g.k.x);
    g.e1 = exp2f_(v.nd * g.F);
    g.B = L->blood_B[t];
    g.e2 = exp2f_(v.ng * g.B);
    g.tissue = v.tissue_w * g.e1;
    g.blood = v.blood_w * g.e2;
    g.s = g.tissue + g.blood;
    return g;
}

// What a thread of a BLOCK-thread, one-lane-per-voxel kernel keeps of the protocol and of its voxel's likelihood side:
// the normalised data and 1 / sigma live in dynamic LDS behind FwdLds as rows [t][thread], 8 T bytes per thread.  A
// thread touches only its own column, so a wave's access at a fixed t is 64 consecutive floats (conflict-free) and no
// barrier follows the table fill.
struct VoxColumns {
    const FwdLds* L;
    float* yt;   // this thread's column: yt[t * BLOCK], is[t * BLOCK]
    float* is;
    int T, se, w_lo, w_hi;
    float w_se, dbw;
};
// normalisation window (model.py:541-545), the weight of each of its images, and the blood weight's slope in DBV
__device__ __forceinline__ void vox_window(const QbDev& c, VoxColumns& vx) {
    vx.T = c.T;
    vx.se = c.se_idx;
    vx.w_lo = c.multi_norm ? vx.se - 1 : vx.se;
    vx.w_hi = c.multi_norm ? vx.se + 1 : vx.se;
    vx.w_se = c.multi_norm ? 1.0f / 3.0f : 1.0f;
    vx.dbw = c.include_blood ? c.m_bld_nb : 1.0f;
}
template <int BLOCK>
__device__ __forceinline__ VoxColumns vox_columns(const QbDev& c, unsigned char* smem) {
    VoxColumns vx;
    vox_window(c, vx);
    vx.L = reinterpret_cast<const FwdLds*>(smem);
    vx.yt = reinterpret_cast<float*>(smem + sizeof(FwdLds)) + threadIdx.x;
    vx.is = vx.yt + vx.T * BLOCK;
    return vx;
}

}  // namespace qb
