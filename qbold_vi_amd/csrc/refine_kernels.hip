// refine_kernels.hip -- semi-amortised inference (Kim et al. 2018; Cremer et al. 2018, "Inference suboptimality"):
// starting from given encoder heads, each voxel runs its own few hundred gradient steps on its own objective
//   L(q) = E_q[nll(x | y)] + KL(q || prior),   y = reparameterised draw of q, sigma held fixed,
// optionally coupled to its in-plane neighbours by a TV smoothness prior, and returns the refined heads in the
// encoder's raw parameterisation, so every consumer of encoder heads (calculate_means, qbold_elbo_fwd,
// qbold_log_evidence_fwd, save_predictions) takes them unchanged.
//
// Four kernels = (how a voxel's likelihood side is held) x (who owns the step loop):
//   compile-time T   T = 11 / 24: x, sigma through prepare_lik into registers, 256 threads, FwdLds static; per draw
//   (SpecVox)        passes 1 and 2 of elbo_bwd_kernel (draw_nll_grad, with sig[T] and gy[T] arrays).
//   run-time T       1 <= T <= QB_MAX_T: the normalised data and 1 / sigma in the thread's LDS columns (signal_grad.h,
//   (GenVox)         VoxColumns), 128 threads; per draw ONE regrouped pass over t (gen_draw_nll_grad).  It gives the
//                    compile-time-T gradient to rounding, not to the bit, so T = 11 / 24 keep their kernels.
//   per voxel        one launch; heads, Adam moments and loss accumulators in registers for all steps
//                    (refine_kernel<T, SE>, refine_generic_kernel).
//   TV step          one Jacobi step of a volume under the TV prior per launch, the state in the workspace
//                    (refine_tv_step_kernel<T, SE>, refine_tv_step_generic_kernel).
// What a step is made of exists once -- the draw source (DrawSource) and the draw loop over it (draws_nll_grad,
// templated on the voxel type whose draw() is the per-draw function), the closed-form KL (kl_closed_grad), the chain to
// the raw heads with the cosine rate and the Adam / SGD update (refine_update), the TV subgradient (tv_subgrad), the
// masked-voxel pass-through, the state load / store and the loss bookkeeping -- and three of the four kernels call it.
// refine_kernel<T, SE> spells the same step out: called from there the shared pieces give the same bits but cost up to
// 1 % of its time at 11 taus (the kernel says what was measured).  The compile-time-T TV kernel scales the gradient
// and adds the KL inline (three lines), because inside a function one of its multiply-add pairs becomes an fma.  Every
// sharing step was held to "no arithmetic instruction more or less in any kernel" against the parent's listing.  On
// the host each pair of entries shares its checks (refine_check_voxels / refine_check_volume, which also build the
// kernels' RefineArgs); the per-voxel entries then launch once, the spatial entries run one step loop
// (refine_run_volume).
//
// Per step: S reparameterised draws give d(mean NLL)/d(logit-space parameters): signal, residuals, d nll / d yhat, the
// chain through the normalisation, the forward model (signal_grad.h) and forward_transform; no log sigma gradient.
// The KL enters by its exact gradient in closed form -- the expectation of the ELBO kernels' Monte-Carlo KL gradient
// while the logit clip does not bind -- then everything is chained to the raw heads through transform_std /
// transform_offdiag as at the end of elbo_bwd_kernel, and Adam (with bias correction) or SGD takes the step at a
// cosine-scheduled rate lr_j = lr_final + (lr - lr_final)(1 + cos(pi j / steps)) / 2.
//
// Draws: Philox stream STREAM_REFINE (7); step j's draw d is draw j Sp + d of the voxel's stream (Sp = 4 ceil(S / 4):
// a Philox call never straddles two steps), i.e. exactly qbold_normals(seed, 7, voxel0, steps Sp) keyed by the global
// voxel, or the same layout [N][steps][Sp][2] given explicitly.  Both sources feed one code path, so they agree bit
// for bit.
//
// HBM traffic of the per-voxel kernels: 4 (2 T + 10 + 1) bytes in and 20 (+ 8 with the loss) out per voxel, whatever
// the number of steps.  No scratch, no atomics, no cross-lane operation: a voxel's bits depend on its own inputs
// (under TV: and its neighbours' heads) and its global index only -- not on the batch, its position in it, or the
// sharding.
#include <cmath>

#include "elbo_core.h"
#include "qbold_ctx.h"
#include "signal_grad.h"

namespace qb {
int elbo_grid(const qbold_ctx* ctx);   // elbo_kernels.hip
}

namespace {

constexpr int kBlock = 256;        // compile-time-T kernels: one voxel per lane
constexpr int kGenBlock = 128;     // run-time-T kernels: one voxel per lane, 8 T bytes of LDS each
constexpr int kStateFloats = 12;   // workspace state per voxel of the TV kernels: m1[5], m2[5], loss0, loss_tail
static_assert(sizeof(qb::FwdLds) % 16 == 0, "the data rows start 16-byte aligned behind FwdLds");
static_assert(sizeof(qb::FwdLds) + sizeof(float) * 2 * QB_MAX_T * kGenBlock <= 160 * 1024,
              "run-time-T kernels: table + rows exceed the LDS");

struct RefineArgs {
    int steps, S, Sp, adam;
    float lr, lr_final, beta1, beta2, eps;
};

struct TvStep {
    int j;             // this launch's step
    float b1p, b2p;    // beta1^j, beta2^j: the per-voxel kernels' running products before step j, accumulated in float32
    float w;           // TV weight, > 0
    qbold_geometry gm;
    int last;          // j == steps - 1: write q_dst from q_in for masked voxels and the loss
};

// ---- what a step is made of: shared by the four kernels ------------------------------------------------------------
// The normals of a step's draws, four at a time: Philox call `quad` of the voxel's stream (step j's call k is quad
// j Sp / 4 + k, draws 4 quad .. 4 quad + 3), or the same draws' rows of the voxel's explicit normals zv
struct DrawSource {
    const float* zv;
    qb::DrawQuad dq;
    __device__ __forceinline__ DrawSource(const float* __restrict__ z, uint64_t seed, uint64_t vox, int quad) : zv(z) {
        if (!zv) dq.load(seed, vox, (uint32_t)quad, qb::STREAM_REFINE);
    }
    __device__ __forceinline__ void next(int64_t i, float& z0, float& z1) {   // draw i, in order
        if (zv) {
            z0 = zv[2 * i];
            z1 = zv[2 * i + 1];
        } else {
            dq.next(z0, z1);
        }
    }
};

// Step j's S draws: the sum of their NLLs, their gradients ADDED to g
template <class V>
__device__ __forceinline__ float draws_nll_grad(const QbDev& c, const V& vx, const qb::LogitMvn& qm,
                                                const float* __restrict__ zv, uint64_t seed, uint64_t vox, int j,
                                                const RefineArgs& ra, float (&g)[5]) {
    const int S = ra.S, Sp = ra.Sp;
    float nll = 0.0f;
#pragma unroll 1
    for (int k = 0; 4 * k < S; ++k) {
        const int cnt = S - 4 * k < 4 ? S - 4 * k : 4;
        DrawSource ds(zv, seed, vox, j * (Sp >> 2) + k);
#pragma unroll 1
        for (int d = 0; d < cnt; ++d) {
            float z0, z1;
            ds.next(4 * ((int64_t)j * (Sp >> 2) + k) + d, z0, z1);
            nll += vx.draw(c, qm, z0, z1, g);
        }
    }
    return nll;
}

// KL(q || p) of two Gaussians in logit space in whitened form, M = L_p^-1 L_q, d = L_p^-1 (mu_q - mu_p):
//   KL = (|M|_F^2 + |d|^2) / 2 - log det M - 1,   log det M = (s_o + s_d)_q - (s_o + s_d)_p
// -- the expectation of the Monte-Carlo KL of the ELBO kernels; qbold_kl_closed (model.py:612-652) gives the same
// number when the prior's off-diagonal term is 0, its trace term being tr(L_p^-1 L_p^-T Sigma_q) -- and ADDS its
// gradient with respect to (mu_o, s_o, mu_d, s_d, c) of q.
__device__ __forceinline__ float kl_closed_grad(const qb::LogitMvn& q, const qb::LogitMvn& p, float (&g)[5]) {
    const float dmu_o = q.mu_o - p.mu_o, dmu_d = q.mu_d - p.mu_d;
    const float d0 = dmu_o * p.i_so, d1 = fmaf(dmu_d, p.i_sd, dmu_o * p.i_bl);
    const float m00 = q.e_so * p.i_so, m10 = fmaf(q.c, p.i_sd, q.e_so * p.i_bl), m11 = q.e_sd * p.i_sd;
    g[0] += fmaf(d0, p.i_so, d1 * p.i_bl);
    g[1] += fmaf(m00, m00, fmaf(m10, q.e_so * p.i_bl, -1.0f));
    g[2] += d1 * p.i_sd;
    g[3] += fmaf(m11, m11, -1.0f);
    g[4] += m10 * p.i_sd;
    const float sq = fmaf(m00, m00, fmaf(m10, m10, fmaf(m11, m11, fmaf(d0, d0, d1 * d1))));
    return fmaf(0.5f, sq, (p.s_o + p.s_d) - (q.s_o + q.s_d) - 1.0f);
}

__device__ __forceinline__ float tv_sigmoid(float u) { return 1.0f / (1.0f + expf(-u)); }   // smoothness_kernel's

// The chain to the raw heads (transform_std / transform_offdiag, model.py:288-294: s = 3 tanh(raw) - 1,
// c = tanh(raw) e^-2), the cosine rate of step j and the Adam (b1t, b2t = beta^(j + 1), the bias correction's
// products) or SGD update
__device__ __forceinline__ void refine_update(const RefineArgs& ra, int j, float b1t, float b2t, float (&qv)[5],
                                              float (&m1)[5], float (&m2)[5], float (&g)[5]) {
    g[1] *= 3.0f * qb::sech2f_(qv[1]);
    g[3] *= 3.0f * qb::sech2f_(qv[3]);
    g[4] *= 0.1353352832366127f * qb::sech2f_(qv[4]);
    const float lr = fmaf(0.5f * (ra.lr - ra.lr_final), 1.0f + cosf((float)M_PI * ((float)j / (float)ra.steps)),
                          ra.lr_final);
    if (ra.adam) {
        const float c1 = 1.0f / (1.0f - b1t), c2 = 1.0f / (1.0f - b2t);
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            m1[i] = fmaf(ra.beta1, m1[i], (1.0f - ra.beta1) * g[i]);
            m2[i] = fmaf(ra.beta2, m2[i], (1.0f - ra.beta2) * (g[i] * g[i]));
            qv[i] -= lr * (m1[i] * c1) / (sqrtf(m2[i] * c2) + ra.eps);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 5; ++i) qv[i] = fmaf(-lr, g[i], qv[i]);
    }
}

// w d TV / d (mu_o, mu_d) of voxel v at the step's heads q_src, ADDED to g[0] and g[2]: smoothness_kernel's
// subgradient over the four in-plane neighbours inside the mask
__device__ __forceinline__ void tv_subgrad(const TvStep& st, const float* __restrict__ mask,
                                           const float* __restrict__ q_src, int64_t v, const float (&qv)[5],
                                           float (&g)[5]) {
    const int64_t yz = (int64_t)st.gm.Y * st.gm.Z;
    const int xi = (int)((v / yz) % st.gm.X), yi = (int)((v / st.gm.Z) % st.gm.Y);
    const float so = tv_sigmoid(qv[0]), sd = tv_sigmoid(qv[2]);
    const int64_t off[4] = {yz, (int64_t)st.gm.Z, -yz, -(int64_t)st.gm.Z};
    const bool inside[4] = {xi + 1 < st.gm.X, yi + 1 < st.gm.Y, xi > 0, yi > 0};
    float go = 0.0f, gd = 0.0f;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        if (!inside[n]) continue;
        const int64_t u = v + off[n];
        if (!(mask ? mask[u] > 0.0f : true)) continue;
        const float dO = so - tv_sigmoid(q_src[5 * u]), dD = sd - tv_sigmoid(q_src[5 * u + 2]);
        go += (dO > 0.0f) - (dO < 0.0f);
        gd += (dD > 0.0f) - (dD < 0.0f);
    }
    g[0] += st.w * go * so * (1.0f - so);
    g[2] += st.w * gd * sd * (1.0f - sd);
}

// a masked voxel: the heads q5[0 .. 4] copied through bit for bit, zero loss; its data is never read
__device__ __forceinline__ void store_masked(const float* q5, float* q_to, float* __restrict__ loss, int64_t v) {
#pragma unroll
    for (int i = 0; i < 5; ++i) q_to[v * 5 + i] = q5[i];
    if (loss) {
        loss[2 * v + 0] = 0.0f;
        loss[2 * v + 1] = 0.0f;
    }
}

// loss[0] = the -ELBO estimate at step 0, loss[1] = its mean over the last ceil(steps / 10) steps
__device__ __forceinline__ int loss_tail_steps(int steps) { return (steps + 9) / 10; }
__device__ __forceinline__ void loss_add(float lj, int j, int steps, int tail, float& loss0, float& loss_tail) {
    if (j == 0) loss0 = lj;
    if (j >= steps - tail) loss_tail += lj;
}
__device__ __forceinline__ void loss_store(float* __restrict__ loss, int64_t v, float loss0, float loss_tail, int tail) {
    if (loss) {
        loss[2 * v + 0] = loss0;
        loss[2 * v + 1] = loss_tail / (float)tail;
    }
}

// the TV kernels' state of voxel v between two launches: three float4 (the moments only under Adam)
__device__ __forceinline__ void state_load(const float4* __restrict__ state, int64_t v, int adam, float (&m1)[5],
                                           float (&m2)[5], float& loss0, float& loss_tail) {
    const float4 s0 = state[3 * v], s1 = state[3 * v + 1], s2 = state[3 * v + 2];
    if (adam) {
        m1[0] = s0.x; m1[1] = s0.y; m1[2] = s0.z; m1[3] = s0.w; m1[4] = s1.x;
        m2[0] = s1.y; m2[1] = s1.z; m2[2] = s1.w; m2[3] = s2.x; m2[4] = s2.y;
    }
    loss0 = s2.z;
    loss_tail = s2.w;
}
__device__ __forceinline__ void state_store(float4* __restrict__ state, int64_t v, const float (&m1)[5],
                                            const float (&m2)[5], float loss0, float loss_tail) {
    state[3 * v] = make_float4(m1[0], m1[1], m1[2], m1[3]);
    state[3 * v + 1] = make_float4(m1[4], m2[0], m2[1], m2[2]);
    state[3 * v + 2] = make_float4(m2[3], m2[4], loss0, loss_tail);
}

// ---- T at compile time (11 / 24 taus) --------------------------------------------------------------------------------
// One draw's NLL and its gradient with respect to the logit-space sample parameters (mu_o, s_o, mu_d, s_d, c),
// ADDED to g[5]: passes 1 and 2 of elbo_bwd_kernel.
template <int T, int SE>
__device__ __forceinline__ float draw_nll_grad(const qb::FwdLds* L, const QbDev& c, const qb::VoxelLik<T>& lik,
                                               const qb::LogitMvn& qm, float z0, float z1, float (&g)[5]) {
    float a, b;
    qb::reparam_logits(qm, z0, z1, a, b);
    const float sa = qb::sigmoidf_(a), sb = qb::sigmoidf_(b);
    const float oef = sa * QB_OEF_RANGE + QB_MIN_OEF;
    const float dbv = sb * QB_DBV_RANGE + QB_MIN_DBV;
    const qb::FwdFast fv = qb::fwd_fast(c, oef, dbv);
    // pass 1: signals, residuals, NLL, d nll / d yhat
    float sig[T];
#pragma unroll
    for (int t = 0; t < T; ++t) sig[t] = qb::fwd_signal_fast(L, c, fv, t);
    const float inv_np = qb::rcpf_(qb::se_norm<T, SE>(c, sig));
    float acc = 0.0f, a1 = 0.0f;
    float gy[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        float yp = sig[t] * inv_np, dyp = 1.0f;
        if (c.predict_log) {                      // model.py:547-549 (only voxels with m > 0 are refined)
            dyp = qb::rcpf_(yp);
            yp = __logf(yp);
        }
        const float r = (lik.yt[t] - yp) * lik.inv_s[t];
        float dr = r;
        if (c.use_student_t) {                    // model.py:557-559
            const float w = (c.st_df + 1.0f) * qb::rcpf_(fmaf(r, r, c.st_df));
            acc += (c.st_df + 1.0f) * log1pf(r * r * qb::rcpf_(c.st_df)) - 2.0f * c.st_const;
            dr = w * r;
        } else {
            acc = fmaf(r, r, acc);
        }
        gy[t] = -dr * lik.inv_s[t] * dyp;
        a1 = fmaf(gy[t], sig[t], a1);
    }
    a1 *= inv_np * inv_np;
    // pass 2: chain through the normalisation and the forward model
    float g_oef = 0.0f, g_dbv = 0.0f;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        float gs = gy[t] * inv_np;
        if (SE >= 0) {
            if (t == SE) gs -= a1;
        } else if (c.multi_norm) {
            if (t >= c.se_idx - 1 && t <= c.se_idx + 1) gs -= a1 * (1.0f / 3.0f);
        } else if (t == c.se_idx) {
            gs -= a1;
        }
        const qb::FwdGrad fg = qb::fwd_signal_grad(L, c, fv, oef, dbv, t);
        g_oef = fmaf(gs, fg.ds_doef, g_oef);
        g_dbv = fmaf(gs, fg.ds_ddbv, g_dbv);
    }
    const float ga = g_oef * QB_OEF_RANGE * sa * (1.0f - sa);   // forward_transform
    const float gb = g_dbv * QB_DBV_RANGE * sb * (1.0f - sb);
    g[0] += ga;
    g[1] = fmaf(ga, z0 * qm.e_so, g[1]);
    g[2] += gb;
    g[4] = fmaf(gb, z0, g[4]);
    g[3] = fmaf(gb, z1 * qm.e_sd, g[3]);
    return fmaf(0.5f, acc, lik.log_s_sum);
}

// the likelihood side of a voxel at a compile-time T, as draws_nll_grad takes it
template <int T, int SE>
struct SpecVox {
    const qb::FwdLds* L;
    const qb::VoxelLik<T>& lik;
    __device__ __forceinline__ float draw(const QbDev& c, const qb::LogitMvn& qm, float z0, float z1,
                                          float (&g)[5]) const {
        return draw_nll_grad<T, SE>(L, c, lik, qm, z0, z1, g);
    }
};

// Per-voxel refinement: all steps of a voxel in one thread.  This kernel alone spells its step out instead of calling
// the shared pieces (DrawSource / draws_nll_grad, loss_add, refine_update, store_masked, loss_store): they are the same
// expressions and give the same bits, but called from here they cost time at 11 taus -- 200 steps, S = 1, 1 M voxels:
// 6.71 ms as written, 6.79 ms with refine_update and the small helpers, 6.73 ms with the draw source as well
// (MEASUREMENTS.md section 30) -- and the listing of each instance below is the one before the step was shared.
template <int T, int SE>
__global__ __launch_bounds__(kBlock) void refine_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* q_in, const float* __restrict__ prior, const float* __restrict__ sigma,
    const float* __restrict__ z, RefineArgs ra, uint64_t seed, int64_t voxel0, float* q_out,
    float* __restrict__ loss, int64_t N) {
    __shared__ qb::FwdLds L;
    qb::fwd_lds_fill(&L, g_tab, false);
    __syncthreads();

    const int steps = ra.steps, S = ra.S, Sp = ra.Sp;
    const int tail = (steps + 9) / 10;   // the last ceil(steps / 10) steps make loss[1]
    const float inv_S = 1.0f / (float)S;
    for (int64_t v = blockIdx.x * (int64_t)kBlock + threadIdx.x; v < N; v += (int64_t)gridDim.x * kBlock) {
        float qv[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) qv[i] = q_in[v * 5 + i];
        const float m = mask ? mask[v] : 1.0f;
        if (!(m > 0.0f)) {   // masked voxel: q copied through bit for bit (store_masked, spelled out)
#pragma unroll
            for (int i = 0; i < 5; ++i) q_out[v * 5 + i] = qv[i];
            if (loss) {
                loss[2 * v + 0] = 0.0f;
                loss[2 * v + 1] = 0.0f;
            }
            continue;
        }
        float xv[T], sv[T], pv[5];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            xv[t] = x[v * T + t];
            sv[t] = sigma[v * T + t];
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) pv[i] = prior[v * 5 + i];
        qb::VoxelLik<T> lik;
        qb::prepare_lik<T, SE, false>(c, xv, sv, 1.0f, lik);
        const qb::LogitMvn pm = qb::make_mvn(pv);
        const uint64_t vox = (uint64_t)(voxel0 + v);
        const float* zv = z ? z + v * (int64_t)steps * Sp * 2 : nullptr;

        float m1[5], m2[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) m1[i] = m2[i] = 0.0f;
        float b1t = 1.0f, b2t = 1.0f;   // beta^t of the bias correction
        float loss0 = 0.0f, loss_tail = 0.0f;
#pragma unroll 1
        for (int j = 0; j < steps; ++j) {
            const qb::LogitMvn qm = qb::make_mvn(qv);
            float g[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            float nll = 0.0f;
#pragma unroll 1
            for (int k = 0; 4 * k < S; ++k) {
                const int cnt = S - 4 * k < 4 ? S - 4 * k : 4;
                qb::DrawQuad dq;
                if (!zv) dq.load(seed, vox, (uint32_t)(j * (Sp >> 2) + k), qb::STREAM_REFINE);
#pragma unroll 1
                for (int d = 0; d < cnt; ++d) {
                    float z0, z1;
                    if (zv) {
                        const int64_t i = (int64_t)j * Sp + 4 * k + d;
                        z0 = zv[2 * i];
                        z1 = zv[2 * i + 1];
                    } else {
                        dq.next(z0, z1);
                    }
                    nll += draw_nll_grad<T, SE>(&L, c, lik, qm, z0, z1, g);
                }
            }
#pragma unroll
            for (int i = 0; i < 5; ++i) g[i] *= inv_S;
            const float kl = kl_closed_grad(qm, pm, g);
            const float lj = fmaf(nll, inv_S, kl);   // this step's Monte-Carlo -ELBO at the step's q
            if (j == 0) loss0 = lj;
            if (j >= steps - tail) loss_tail += lj;
            // transform_std / transform_offdiag (model.py:288-294): s = 3 tanh(raw) - 1, c = tanh(raw) e^-2
            g[1] *= 3.0f * qb::sech2f_(qv[1]);
            g[3] *= 3.0f * qb::sech2f_(qv[3]);
            g[4] *= 0.1353352832366127f * qb::sech2f_(qv[4]);
            const float lr = fmaf(0.5f * (ra.lr - ra.lr_final), 1.0f + cosf((float)M_PI * ((float)j / (float)steps)),
                                  ra.lr_final);
            if (ra.adam) {
                b1t *= ra.beta1;
                b2t *= ra.beta2;
                const float c1 = 1.0f / (1.0f - b1t), c2 = 1.0f / (1.0f - b2t);
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    m1[i] = fmaf(ra.beta1, m1[i], (1.0f - ra.beta1) * g[i]);
                    m2[i] = fmaf(ra.beta2, m2[i], (1.0f - ra.beta2) * (g[i] * g[i]));
                    qv[i] -= lr * (m1[i] * c1) / (sqrtf(m2[i] * c2) + ra.eps);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 5; ++i) qv[i] = fmaf(-lr, g[i], qv[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) q_out[v * 5 + i] = qv[i];
        if (loss) {
            loss[2 * v + 0] = loss0;
            loss[2 * v + 1] = loss_tail / (float)tail;
        }
    }
}

// Jacobi step st.j of a volume under the TV prior: every voxel's gradient is taken at the step-j heads q_src of all
// voxels, so the TV term couples a voxel to its four in-plane neighbours' step-j means.  The per-voxel arithmetic is
// refine_kernel's step, expression for expression; the compiler schedules the inlined likelihood differently in the two
// kernels, so they agree to rounding, not to the bit.
template <int T, int SE>
__global__ __launch_bounds__(kBlock) void refine_tv_step_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* q_in, const float* __restrict__ q_src, const float* __restrict__ prior,
    const float* __restrict__ sigma, const float* __restrict__ z, RefineArgs ra, TvStep st, uint64_t seed,
    int64_t voxel0, float* q_dst, float4* __restrict__ state, float* __restrict__ loss, int64_t N) {
    __shared__ qb::FwdLds L;
    qb::fwd_lds_fill(&L, g_tab, false);
    __syncthreads();

    const int steps = ra.steps, S = ra.S, Sp = ra.Sp, j = st.j;
    const int tail = loss_tail_steps(steps);
    const float inv_S = 1.0f / (float)S;
    for (int64_t v = blockIdx.x * (int64_t)kBlock + threadIdx.x; v < N; v += (int64_t)gridDim.x * kBlock) {
        const float m = mask ? mask[v] : 1.0f;
        if (!(m > 0.0f)) {   // masked voxel: q_in copied through bit for bit at the last step, never read by others
            if (st.last) store_masked(q_in + v * 5, q_dst, loss, v);
            continue;
        }
        float qv[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) qv[i] = q_src[v * 5 + i];
        float xv[T], sv[T], pv[5];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            xv[t] = x[v * T + t];
            sv[t] = sigma[v * T + t];
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) pv[i] = prior[v * 5 + i];
        qb::VoxelLik<T> lik;
        qb::prepare_lik<T, SE, false>(c, xv, sv, 1.0f, lik);
        const SpecVox<T, SE> spv{&L, lik};
        const qb::LogitMvn pm = qb::make_mvn(pv);
        const uint64_t vox = (uint64_t)(voxel0 + v);
        const float* zv = z ? z + v * (int64_t)steps * Sp * 2 : nullptr;

        float m1[5], m2[5], loss0 = 0.0f, loss_tail = 0.0f;
#pragma unroll
        for (int i = 0; i < 5; ++i) m1[i] = m2[i] = 0.0f;
        if (j > 0) state_load(state, v, ra.adam, m1, m2, loss0, loss_tail);

        // refine_kernel's step j (its scaling and KL inline, as there)
        const qb::LogitMvn qm = qb::make_mvn(qv);
        float g[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        const float nll = draws_nll_grad(c, spv, qm, zv, seed, vox, j, ra, g);
#pragma unroll
        for (int i = 0; i < 5; ++i) g[i] *= inv_S;
        const float kl = kl_closed_grad(qm, pm, g);
        const float lj = fmaf(nll, inv_S, kl);
        loss_add(lj, j, steps, tail, loss0, loss_tail);
        tv_subgrad(st, mask, q_src, v, qv, g);
        refine_update(ra, j, st.b1p * ra.beta1, st.b2p * ra.beta2, qv, m1, m2, g);

#pragma unroll
        for (int i = 0; i < 5; ++i) q_dst[v * 5 + i] = qv[i];
        if (st.last)
            loss_store(loss, v, loss0, loss_tail, tail);
        else
            state_store(state, v, m1, m2, loss0, loss_tail);
    }
}

// ---- T at run time (1 <= T <= QB_MAX_T) ------------------------------------------------------------------------------
// Shape: laplace_kernel's.  LDS per block: sizeof(FwdLds) + 1,024 T bytes (T = 11: 16.8 KiB, T = 33: 38.8 KiB, T = 64:
// 69.8 KiB, above the 64 KiB default and taken by the hipFuncSetAttribute opt-in; two blocks per CU there, one wave
// per SIMD).  A thread touches only its own column, so no barrier follows the table fill; blood_B is read from LDS (t
// is a run-time index).
//
// Per draw: with gy_t = d nll / d yhat_t and yhat_t = sig_t / np,
//     g_oef = (1 / np) sum_t gy_t ds_t/doef - w a1 sum_window ds_t/doef,   a1 = (1 / np^2) sum_t gy_t sig_t,  w = 1 or 1/3,
// so the 1 or 3 window images give np first, then ONE pass over t gathers sum gy sig, sum gy ds/doef, sum gy ds/ddbv
// and the window's slopes: T + 1 (T + 3) table lookups per draw, no sig[T] / gy[T] arrays.  The likelihood switches
// (Student-t, log data, three-image normalisation) are wave-uniform branches on QbDev, as in draw_nll_grad.
// what a thread keeps of its voxel's likelihood side and of the protocol: the LDS columns of signal_grad.h and
// two numbers of its own
struct GenVox : qb::VoxColumns {
    float n0;          // node 0's slope per u^2 (QbDev::dF_node0: the training gradients' slope keeps that node)
    float log_s_sum;   // per voxel (gen_load)
    __device__ __forceinline__ float draw(const QbDev& c, const qb::LogitMvn& qm, float z0, float z1,
                                          float (&g)[5]) const;
};

__device__ __forceinline__ GenVox gen_vox(const QbDev& c, unsigned char* smem) {
    GenVox vx;
    static_cast<qb::VoxColumns&>(vx) = qb::vox_columns<kGenBlock>(c, smem);
    vx.n0 = c.dF_node0 / (c.tab_inv_h * c.tab_inv_h);
    vx.log_s_sum = 0.0f;
    return vx;
}

// prepare_lik<T, SE, false> of a live voxel into the thread's column
__device__ __forceinline__ void gen_load(const QbDev& c, GenVox& vx, const float* __restrict__ xv,
                                         const float* __restrict__ sv) {
    const int se = vx.se;
    const float nt = c.multi_norm ? (xv[se - 1] + xv[se] + xv[se + 1]) / 3.0f + 1e-3f : xv[se] + 1e-3f;
    const float inv_nt = qb::rcpf_(nt);
    float ls = 0.0f;
    for (int t = 0; t < vx.T; ++t) {
        float y = xv[t] * inv_nt;
        if (c.predict_log) y = __logf(y);   // model.py:548
        const float s = sv[t];
        vx.yt[t * kGenBlock] = y;
        vx.is[t * kGenBlock] = qb::rcpf_(s);
        ls += QB_LN2 * qb::log2f_(s);
    }
    vx.log_s_sum = c.use_student_t ? ls : ls + (float)vx.T * 0.9189385332046727f;   // log sqrt(2 pi)
}

// draw_nll_grad at a run-time T: one draw's NLL, and its gradient with respect to (mu_o, s_o, mu_d, s_d, c) ADDED to g
__device__ __forceinline__ float gen_draw_nll_grad(const QbDev& c, const GenVox& vx, const qb::LogitMvn& qm, float z0,
                                                   float z1, float (&g)[5]) {
    float a, b;
    qb::reparam_logits(qm, z0, z1, a, b);
    const float sa = qb::sigmoidf_(a), sb = qb::sigmoidf_(b);
    const float oef = sa * QB_OEF_RANGE + QB_MIN_OEF;
    const float dbv = sb * QB_DBV_RANGE + QB_MIN_DBV;
    const qb::FwdFast fv = qb::fwd_fast(c, oef, dbv);
    // se_norm on the prediction
    float np_ = qb::sig_eval(vx.L, fv, vx.se).s;
    if (c.multi_norm) np_ = (qb::sig_eval(vx.L, fv, vx.se - 1).s + np_ + qb::sig_eval(vx.L, fv, vx.se + 1).s) / 3.0f;
    const float inv_np = qb::rcpf_(np_ + 1e-3f);
    const qb::SlopeFactors kf = qb::slope_factors(c, fv, oef, dbv, vx.dbw);
    const float df1 = c.st_df + 1.0f, inv_df = qb::rcpf_(c.st_df);
    float acc = 0.0f, a1 = 0.0f, go = 0.0f, gd = 0.0f, wo = 0.0f, wd = 0.0f;
    for (int t = 0; t < vx.T; ++t) {
        const qb::SigEval sg = qb::sig_eval(vx.L, fv, t);
        const float inv_s = vx.is[t * kGenBlock];
        float yp = sg.s * inv_np, dyp = 1.0f;
        if (c.predict_log) {                      // model.py:547-549 (only voxels with m > 0 are refined)
            dyp = qb::rcpf_(yp);
            yp = __logf(yp);
        }
        const float r = (vx.yt[t * kGenBlock] - yp) * inv_s;
        float dr = r;
        if (c.use_student_t) {                    // model.py:557-559
            const float w = df1 * qb::rcpf_(fmaf(r, r, c.st_df));
            acc += df1 * log1pf(r * r * inv_df) - 2.0f * c.st_const;
            dr = w * r;
        } else {
            acc = fmaf(r, r, acc);
        }
        const float gy = -dr * inv_s * dyp;       // d nll / d (sig_t / np)
        a1 = fmaf(gy, sg.s, a1);
        // the cubic's slope plus node 0's slope in x (kept here, as in fwd_signal_grad; the Laplace kernel drops it)
        const float dFu = sg.dFu() + vx.n0 * sg.u * sg.u;
        const float ds_doef = sg.ds_doef(kf, dFu);
        const float ds_ddbv = sg.ds_ddbv(kf);
        go = fmaf(gy, ds_doef, go);
        gd = fmaf(gy, ds_ddbv, gd);
        if (t >= vx.w_lo && t <= vx.w_hi) {       // wave-uniform
            wo += ds_doef;
            wd += ds_ddbv;
        }
    }
    a1 *= inv_np * inv_np * vx.w_se;              // yhat_t = sig_t / (norm + 1e-3)
    const float g_oef = fmaf(go, inv_np, -a1 * wo), g_dbv = fmaf(gd, inv_np, -a1 * wd);
    const float ga = g_oef * QB_OEF_RANGE * sa * (1.0f - sa);   // forward_transform
    const float gb = g_dbv * QB_DBV_RANGE * sb * (1.0f - sb);
    g[0] += ga;
    g[1] = fmaf(ga, z0 * qm.e_so, g[1]);
    g[2] += gb;
    g[4] = fmaf(gb, z0, g[4]);
    g[3] = fmaf(gb, z1 * qm.e_sd, g[3]);
    return fmaf(0.5f, acc, vx.log_s_sum);
}
__device__ __forceinline__ float GenVox::draw(const QbDev& c, const qb::LogitMvn& qm, float z0, float z1,
                                              float (&g)[5]) const {
    return gen_draw_nll_grad(c, *this, qm, z0, z1, g);
}

// Step j's Monte-Carlo -ELBO at the heads qm and its gradient g with respect to (mu_o, s_o, mu_d, s_d, c): the draws
// (the same Philox words, or the same rows of z, as at a compile-time T), their mean and the closed-form KL
__device__ __forceinline__ float gen_step_grad(const QbDev& c, const GenVox& vx, const qb::LogitMvn& qm,
                                               const qb::LogitMvn& pm, const float* __restrict__ zv, uint64_t seed,
                                               uint64_t vox, int j, const RefineArgs& ra, float (&g)[5]) {
#pragma unroll
    for (int i = 0; i < 5; ++i) g[i] = 0.0f;
    const float nll = draws_nll_grad(c, vx, qm, zv, seed, vox, j, ra, g);
    const float inv_S = 1.0f / (float)ra.S;
#pragma unroll
    for (int i = 0; i < 5; ++i) g[i] *= inv_S;
    const float kl = kl_closed_grad(qm, pm, g);
    return fmaf(nll, inv_S, kl);
}

__global__ __launch_bounds__(kGenBlock) void refine_generic_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* q_in, const float* __restrict__ prior, const float* __restrict__ sigma,
    const float* __restrict__ z, RefineArgs ra, uint64_t seed, int64_t voxel0, float* q_out,
    float* __restrict__ loss, int64_t N) {
    extern __shared__ __align__(16) unsigned char smem[];
    qb::FwdLds* L = reinterpret_cast<qb::FwdLds*>(smem);
    qb::fwd_lds_fill(L, g_tab, false);
    if (threadIdx.x < QB_MAX_T) L->blood_B[threadIdx.x] = c.blood_B[threadIdx.x];
    __syncthreads();
    GenVox vx = gen_vox(c, smem);

    const int steps = ra.steps, T = vx.T;
    const int tail = loss_tail_steps(steps);
    const int64_t ntile = (N + kGenBlock - 1) / kGenBlock;
    // no barrier inside the loop: a thread reads and writes its own column only
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t v = tile * kGenBlock + threadIdx.x;
        if (v >= N) continue;
        float qv[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) qv[i] = q_in[v * 5 + i];
        const float m = mask ? mask[v] : 1.0f;
        if (!(m > 0.0f)) {
            store_masked(qv, q_out, loss, v);
            continue;
        }
        gen_load(c, vx, x + v * T, sigma + v * T);
        float pv[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) pv[i] = prior[v * 5 + i];
        const qb::LogitMvn pm = qb::make_mvn(pv);
        const uint64_t vox = (uint64_t)(voxel0 + v);
        const float* zv = z ? z + v * (int64_t)steps * ra.Sp * 2 : nullptr;

        float m1[5], m2[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) m1[i] = m2[i] = 0.0f;
        float b1t = 1.0f, b2t = 1.0f;   // beta^t of the bias correction
        float loss0 = 0.0f, loss_tail = 0.0f;
#pragma unroll 1
        for (int j = 0; j < steps; ++j) {
            const qb::LogitMvn qm = qb::make_mvn(qv);
            float g[5];
            const float lj = gen_step_grad(c, vx, qm, pm, zv, seed, vox, j, ra, g);
            loss_add(lj, j, steps, tail, loss0, loss_tail);
            b1t *= ra.beta1;
            b2t *= ra.beta2;
            refine_update(ra, j, b1t, b2t, qv, m1, m2, g);
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) q_out[v * 5 + i] = qv[i];
        loss_store(loss, v, loss0, loss_tail, tail);
    }
}

// refine_tv_step_kernel's Jacobi step j at a run-time T: the same workspace and launch-per-step protocol
__global__ __launch_bounds__(kGenBlock) void refine_tv_step_generic_kernel(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ x, const float* __restrict__ mask,
    const float* q_in, const float* __restrict__ q_src, const float* __restrict__ prior,
    const float* __restrict__ sigma, const float* __restrict__ z, RefineArgs ra, TvStep st, uint64_t seed,
    int64_t voxel0, float* q_dst, float4* __restrict__ state, float* __restrict__ loss, int64_t N) {
    extern __shared__ __align__(16) unsigned char smem[];
    qb::FwdLds* L = reinterpret_cast<qb::FwdLds*>(smem);
    qb::fwd_lds_fill(L, g_tab, false);
    if (threadIdx.x < QB_MAX_T) L->blood_B[threadIdx.x] = c.blood_B[threadIdx.x];
    __syncthreads();
    GenVox vx = gen_vox(c, smem);

    const int steps = ra.steps, T = vx.T, j = st.j;
    const int tail = loss_tail_steps(steps);
    const int64_t ntile = (N + kGenBlock - 1) / kGenBlock;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t v = tile * kGenBlock + threadIdx.x;
        if (v >= N) continue;
        const float m = mask ? mask[v] : 1.0f;
        if (!(m > 0.0f)) {   // masked voxel: q_in copied through bit for bit at the last step, never read by others
            if (st.last) store_masked(q_in + v * 5, q_dst, loss, v);
            continue;
        }
        float qv[5], pv[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            qv[i] = q_src[v * 5 + i];
            pv[i] = prior[v * 5 + i];
        }
        gen_load(c, vx, x + v * T, sigma + v * T);
        const qb::LogitMvn pm = qb::make_mvn(pv);
        const uint64_t vox = (uint64_t)(voxel0 + v);
        const float* zv = z ? z + v * (int64_t)steps * ra.Sp * 2 : nullptr;

        float m1[5], m2[5], loss0 = 0.0f, loss_tail = 0.0f;
#pragma unroll
        for (int i = 0; i < 5; ++i) m1[i] = m2[i] = 0.0f;
        if (j > 0) state_load(state, v, ra.adam, m1, m2, loss0, loss_tail);

        const qb::LogitMvn qm = qb::make_mvn(qv);
        float g[5];
        const float lj = gen_step_grad(c, vx, qm, pm, zv, seed, vox, j, ra, g);
        loss_add(lj, j, steps, tail, loss0, loss_tail);
        tv_subgrad(st, mask, q_src, v, qv, g);
        refine_update(ra, j, st.b1p * ra.beta1, st.b2p * ra.beta2, qv, m1, m2, g);

#pragma unroll
        for (int i = 0; i < 5; ++i) q_dst[v * 5 + i] = qv[i];
        if (st.last)
            loss_store(loss, v, loss0, loss_tail, tail);
        else
            state_store(state, v, m1, m2, loss0, loss_tail);
    }
}

// ---- host: the argument checks the four entries share (what: the entry's name, for the message) ---------------------
#define QB_REFINE_REQUIRE(cond, msg)                        \
    do {                                                    \
        if (!(cond)) {                                      \
            qb::set_error(std::string(what) + ": " + msg);  \
            return QBOLD_ERR_INVALID;                       \
        }                                                   \
    } while (0)

// steps, S, the Philox call word and the optimiser's settings; *ra = the kernels' arguments, Sp = 4 ceil(S / 4)
int refine_check_cfg(const char* what, const qbold_refine_cfg* cfg, int steps, int S, RefineArgs* ra) {
    const int64_t Sp = 4 * (((int64_t)S + 3) / 4);
    QB_REFINE_REQUIRE((int64_t)steps * Sp / 4 < ((int64_t)1 << 32),
                      "steps * Sp / 4 must fit the 32-bit Philox call word");
    QB_REFINE_REQUIRE(cfg->optimizer == 0 || cfg->optimizer == 1, "optimizer must be 0 (Adam) or 1 (SGD)");
    QB_REFINE_REQUIRE(cfg->lr > 0.0f && cfg->lr_final >= 0.0f, "need lr > 0 and lr_final >= 0");
    QB_REFINE_REQUIRE(cfg->optimizer == 1 || (cfg->beta1 >= 0.0f && cfg->beta1 < 1.0f && cfg->beta2 >= 0.0f &&
                                              cfg->beta2 < 1.0f && cfg->eps > 0.0f),
                      "Adam needs 0 <= beta1, beta2 < 1 and eps > 0");
    *ra = RefineArgs{steps, S, (int)Sp, cfg->optimizer == 0 ? 1 : 0, cfg->lr, cfg->lr_final,
                     cfg->beta1, cfg->beta2, cfg->eps};
    return QBOLD_OK;
}

// the configurations with a kernel: the full model in table mode; any_t: every 1 <= T <= QB_MAX_T, else T = 11 / 24
int refine_check_mode(const char* what, const qbold_ctx* ctx, bool any_t) {
    if (!(ctx->dev.full_model && ctx->dev.tissue_mode == QBOLD_TISSUE_TABLE)) {
        qb::set_error(std::string(what) + ": built for the full signal model in table mode "
                      "(Gaussian or Student-t likelihood, linear or log data, either normalisation)");
        return QBOLD_ERR_UNSUPPORTED;
    }
    if (any_t) {
        QB_REFINE_REQUIRE(ctx->dev.T >= 1 && ctx->dev.T <= QB_MAX_T, "need 1 <= T <= 64");
    } else if (ctx->dev.T != 11 && ctx->dev.T != 24) {
        qb::set_error(std::string(what) + ": kernels are built for T = 11 or 24 taus");
        return QBOLD_ERR_UNSUPPORTED;
    }
    return QBOLD_OK;
}

// every check of the per-voxel entries
int refine_check_voxels(const char* what, const qbold_ctx* ctx, const float* x, const float* q_in, const float* prior,
                        const float* sigma, int steps, int S, const qbold_refine_cfg* cfg, const float* q_out,
                        int64_t N, bool any_t, RefineArgs* ra) {
    QB_NEED_DEVICE(ctx);
    QB_REFINE_REQUIRE(cfg, "null cfg");
    QB_REFINE_REQUIRE(N >= 0 && steps >= 1 && S >= 1, "need N >= 0, steps >= 1, S >= 1");
    if (const int rc = refine_check_cfg(what, cfg, steps, S, ra)) return rc;
    QB_REFINE_REQUIRE(N == 0 || (x && q_in && prior && sigma && q_out), "null buffer");
    return refine_check_mode(what, ctx, any_t);
}

// voxels of a geometry, or -1 when it is not a positive one or the workspace size would not fit int64
int64_t tv_voxels(const qbold_geometry* g) {
    if (!g || g->B <= 0 || g->X <= 0 || g->Y <= 0 || g->Z <= 0) return -1;
    int64_t n = 1;
    for (const int32_t d : {g->B, g->X, g->Y, g->Z}) {
        if (__builtin_mul_overflow(n, (int64_t)d, &n)) return -1;
    }
    int64_t b;
    if (__builtin_mul_overflow(n, (int64_t)(sizeof(float) * (kStateFloats + 10)), &b)) return -1;
    return n;
}

// every check of the spatial entries; *N = the geometry's voxels
int refine_check_volume(const char* what, const qbold_ctx* ctx, const float* x, const float* q_in, const float* prior,
                        const float* sigma, const qbold_geometry* geom, float tv_weight, int steps, int S,
                        const qbold_refine_cfg* cfg, const float* q_out, const void* workspace, bool any_t,
                        RefineArgs* ra, int64_t* N) {
    QB_NEED_DEVICE(ctx);
    QB_REFINE_REQUIRE(cfg, "null cfg");
    QB_REFINE_REQUIRE(steps >= 1 && S >= 1, "need steps >= 1, S >= 1");
    *N = tv_voxels(geom);
    QB_REFINE_REQUIRE(*N >= 0, "need a geometry with B, X, Y, Z >= 1 whose voxel count and workspace fit int64");
    QB_REFINE_REQUIRE(std::isfinite(tv_weight) && tv_weight >= 0.0f, "tv_weight must be finite and >= 0");
    if (const int rc = refine_check_cfg(what, cfg, steps, S, ra)) return rc;
    QB_REFINE_REQUIRE(x && q_in && prior && sigma && q_out, "null buffer");
    QB_REFINE_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0,
                      "need a 16-byte aligned workspace of qbold_refine_spatial_workspace_bytes() bytes");
    return refine_check_mode(what, ctx, any_t);
}

// ---- host: the launches -------------------------------------------------------------------------------------------------
// blocks of `block` voxels, at most `cap` of them
int refine_grid(int64_t N, int block, int64_t cap) {
    const int64_t ntile = (N + block - 1) / block;
    return (int)(ntile < cap ? ntile : cap);
}

// dynamic LDS of a run-time-T block at T taus, taken by the opt-in above the 64 KiB default
template <typename K>
int gen_lds_bytes(K kernel, int T, size_t* smem) {
    *smem = sizeof(qb::FwdLds) + sizeof(float) * 2 * (size_t)T * kGenBlock;
    if (*smem > 64 * 1024)
        QB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)*smem));
    return QBOLD_OK;
}

// The per-voxel entries are one launch on refine_grid blocks each, written out in the entry.  The spatial entries:
// full-batch Adam / SGD on F(q) = sum_v (E_q_v[nll] + KL(q_v || p_v)) + w TV(q), TV = qbold_smoothness's tv_sum, by
// Jacobi steps.  One launch per step (the grid is the barrier between steps);
// launch(grid, st, src, dst, state) starts the chosen kernel on step st.j.  Workspace: state [N][12] (16-byte rows of
// float4), then the two head buffers [N][5] that the heads ping-pong between.  Per voxel and step: 4 (2 T + 21) B in
// (x, sigma, heads, moments, loss, prior, mask, the neighbours' heads 0 and 2 and masks), 68 B out.  The per-voxel
// arithmetic is the per-voxel kernels' step, expression for expression; the compiler schedules the inlined likelihood
// differently in the two kernels, so they agree to rounding, not to the bit (w = 0 couples nothing: the entries run the
// per-voxel entry itself, which gives its bits exactly).
template <typename Launch>
int refine_run_volume(const qbold_refine_cfg* cfg, const qbold_geometry* geom, float tv_weight, int steps, int64_t N,
                      int block, int64_t cap, const float* q_in, float* q_out, void* workspace, hipStream_t s,
                      Launch launch) {
    float4* state = (float4*)workspace;
    float* heads[2] = {(float*)workspace + N * kStateFloats, (float*)workspace + N * (kStateFloats + 5)};
    const int grid = refine_grid(N, block, cap);
    TvStep st{0, 1.0f, 1.0f, tv_weight, *geom, 0};
    for (int j = 0; j < steps; ++j) {
        st.j = j;
        st.last = j == steps - 1;
        const float* src = j == 0 ? q_in : heads[(j - 1) & 1];
        // the last step writes q_out, except a single step, which reads q_in (q_out may alias it) and is copied
        float* dst = st.last && steps > 1 ? q_out : heads[j & 1];
        launch(grid, st, src, dst, state);
        QB_HIP(hipGetLastError());
        st.b1p *= cfg->beta1;   // the per-voxel kernels' running products, rounded to float32 after every step
        st.b2p *= cfg->beta2;
    }
    if (steps == 1) QB_HIP(hipMemcpyAsync(q_out, heads[0], N * 5 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return QBOLD_OK;
}

// the compile-time-T instance of a context: T = 24, T = 11 normalised by image 2 alone, T = 11 otherwise
#define QB_DISPATCH_SPEC(ctx, LAUNCH)                                  \
    do {                                                               \
        if ((ctx)->dev.T == 24) {                                      \
            LAUNCH(24, -1);                                            \
        } else if ((ctx)->dev.se_idx == 2 && !(ctx)->dev.multi_norm) { \
            LAUNCH(11, 2);                                             \
        } else {                                                       \
            LAUNCH(11, -1);                                            \
        }                                                              \
    } while (0)

// The launches that QB_DISPATCH_SPEC instantiates.  They name what is in scope where they are used, spelled exactly so:
// the entry's parameters (ctx, x, mask, q_in, prior, sigma, z, seed, voxel0, q_out, loss) and its locals ra, s, N,
// grid; QB_LAUNCH_REFINE_TV also the parameters st, src, dst, state of refine_run_volume's callable.
#define QB_LAUNCH_REFINE(TT, SEC)                                                                                 \
    hipLaunchKernelGGL((refine_kernel<TT, SEC>), dim3(grid), dim3(kBlock), 0, s, ctx->dev, ctx->d_tab, x, mask,   \
                       q_in, prior, sigma, z, ra, seed, voxel0, q_out, loss, N)
#define QB_LAUNCH_REFINE_TV(TT, SEC)                                                                                \
    hipLaunchKernelGGL((refine_tv_step_kernel<TT, SEC>), dim3(grid), dim3(kBlock), 0, s, ctx->dev, ctx->d_tab, x,  \
                       mask, q_in, src, prior, sigma, z, ra, st, seed, voxel0, dst, state, loss, N)

}  // namespace

extern "C" int qbold_refine_posterior(const qbold_ctx* ctx, const float* x, const float* mask, const float* q_in,
                                      const float* prior, const float* sigma, const float* z, int steps, int S,
                                      const qbold_refine_cfg* cfg, uint64_t seed, int64_t voxel0, float* q_out,
                                      float* loss, int64_t N, void* stream) {
    RefineArgs ra;
    if (const int rc = refine_check_voxels("qbold_refine_posterior", ctx, x, q_in, prior, sigma, steps, S, cfg, q_out,
                                           N, false, &ra))
        return rc;
    if (N == 0) return QBOLD_OK;
    hipStream_t s = (hipStream_t)stream;
    const int grid = refine_grid(N, kBlock, qb::elbo_grid(ctx));
    QB_DISPATCH_SPEC(ctx, QB_LAUNCH_REFINE);
    QB_HIP(hipGetLastError());
    return QBOLD_OK;
}

extern "C" int qbold_refine_posterior_anyt(const qbold_ctx* ctx, const float* x, const float* mask,
                                           const float* q_in, const float* prior, const float* sigma, const float* z,
                                           int steps, int S, const qbold_refine_cfg* cfg, uint64_t seed,
                                           int64_t voxel0, float* q_out, float* loss, int64_t N, void* stream) {
    RefineArgs ra;
    if (const int rc = refine_check_voxels("qbold_refine_posterior_anyt", ctx, x, q_in, prior, sigma, steps, S, cfg,
                                           q_out, N, true, &ra))
        return rc;
    if (N == 0) return QBOLD_OK;
    hipStream_t s = (hipStream_t)stream;
    size_t smem;
    if (const int rc = gen_lds_bytes(refine_generic_kernel, ctx->dev.T, &smem)) return rc;
    // 128-thread blocks: twice the 256-thread kernels' cap
    const int grid = refine_grid(N, kGenBlock, 2 * (int64_t)qb::elbo_grid(ctx));
    hipLaunchKernelGGL(refine_generic_kernel, dim3(grid), dim3(kGenBlock), smem, s, ctx->dev, ctx->d_tab, x, mask, q_in,
                       prior, sigma, z, ra, seed, voxel0, q_out, loss, N);
    QB_HIP(hipGetLastError());
    return QBOLD_OK;
}

extern "C" int64_t qbold_refine_spatial_workspace_bytes(const qbold_ctx* ctx, const qbold_geometry* geom) {
    const int64_t N = tv_voxels(geom);
    if (!ctx || N < 0) return QBOLD_ERR_INVALID;
    return N * (int64_t)sizeof(float) * (kStateFloats + 10);
}

extern "C" int qbold_refine_posterior_spatial(const qbold_ctx* ctx, const float* x, const float* mask,
                                              const float* q_in, const float* prior, const float* sigma,
                                              const float* z, const qbold_geometry* geom, float tv_weight, int steps,
                                              int S, const qbold_refine_cfg* cfg, uint64_t seed, int64_t voxel0,
                                              float* q_out, float* loss, void* workspace, void* stream) {
    RefineArgs ra;
    int64_t N;
    if (const int rc = refine_check_volume("qbold_refine_posterior_spatial", ctx, x, q_in, prior, sigma, geom,
                                           tv_weight, steps, S, cfg, q_out, workspace, false, &ra, &N))
        return rc;
    // no coupling: the per-voxel refinement, one launch with the state in registers (its bits by construction)
    if (tv_weight == 0.0f)
        return qbold_refine_posterior(ctx, x, mask, q_in, prior, sigma, z, steps, S, cfg, seed, voxel0, q_out, loss,
                                      N, stream);
    hipStream_t s = (hipStream_t)stream;
    return refine_run_volume(cfg, geom, tv_weight, steps, N, kBlock, 8 * (int64_t)qb::elbo_grid(ctx), q_in, q_out,
                             workspace, s,
                             [&](int grid, const TvStep& st, const float* src, float* dst, float4* state) {
                                 QB_DISPATCH_SPEC(ctx, QB_LAUNCH_REFINE_TV);
                             });
}

extern "C" int qbold_refine_posterior_spatial_anyt(const qbold_ctx* ctx, const float* x, const float* mask,
                                                   const float* q_in, const float* prior, const float* sigma,
                                                   const float* z, const qbold_geometry* geom, float tv_weight,
                                                   int steps, int S, const qbold_refine_cfg* cfg, uint64_t seed,
                                                   int64_t voxel0, float* q_out, float* loss, void* workspace,
                                                   void* stream) {
    RefineArgs ra;
    int64_t N;
    if (const int rc = refine_check_volume("qbold_refine_posterior_spatial_anyt", ctx, x, q_in, prior, sigma, geom,
                                           tv_weight, steps, S, cfg, q_out, workspace, true, &ra, &N))
        return rc;
    if (tv_weight == 0.0f)   // as above
        return qbold_refine_posterior_anyt(ctx, x, mask, q_in, prior, sigma, z, steps, S, cfg, seed, voxel0, q_out,
                                           loss, N, stream);
    hipStream_t s = (hipStream_t)stream;
    size_t smem;
    if (const int rc = gen_lds_bytes(refine_tv_step_generic_kernel, ctx->dev.T, &smem)) return rc;
    // the specialised entry's cap in voxels
    return refine_run_volume(cfg, geom, tv_weight, steps, N, kGenBlock, 16 * (int64_t)qb::elbo_grid(ctx), q_in, q_out,
                             workspace, s,
                             [&](int grid, const TvStep& st, const float* src, float* dst, float4* state) {
                                 hipLaunchKernelGGL(refine_tv_step_generic_kernel, dim3(grid), dim3(kGenBlock), smem, s,
                                                    ctx->dev, ctx->d_tab, x, mask, q_in, src, prior, sigma, z, ra, st,
                                                    seed, voxel0, dst, state, loss, N);
                             });
}
