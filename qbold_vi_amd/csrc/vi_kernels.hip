// vi_kernels.hip -- the whole voxel-ELBO hot path behind one entry point (qbold_vi_fwd).
//
// Narrow encoders (U <= 64, T = 11 or 24: BASELINE configs 1, 2, 4, 5) -- one launch, vi_fwd_kernel.  Per
// 16-voxel wave tile: load x -> normalise -> encoder stream 2 on the f16 matrix cores (encoder_core.h: operands
// split into two f16 halves, three v_mfma_f32_16x16x32_f16 passes hi.hi + hi.lo + lo.hi with f32 accumulation,
// float32-grade products; QBOLD_ENC_BF16: operands rounded to bf16, one pass) -> posterior parameters and log
// sigma stay in registers -> S reparameterised draws through the forward model + K-draw Monte-Carlo KL on the
// vector pipe (elbo_core.h) -> per-voxel (nll, kl), posterior parameters and the three masked sums.  This is the
// reference's full_model([data, mask]) + fine_tune_loss_fn + kl_loss (model.py:239-286, 527-568, 654-665)
// evaluated for (N,1,1,1,T) voxel batches, with ELBO = nll + kl as train.py:351.
//
// HBM traffic per voxel (T = 11): read x 44 + mask 4 + prior 20, write q 20 + (nll, kl) 8 = 96 B; the weight
// image (~145 KB of split-f16 fragments), the F(x) table (4 KB) and constants are LDS / SGPR resident.  Work per
// voxel at S = 32, K = 70: 60.8 kFLOP of encoder products (x 3 passes on the matrix pipe) and ~30 kFLOP of
// sampling: compute-bound by the vector pipe's issue rate (MEASUREMENTS.md 4.4), ~900 flop/B against a machine balance
// of ~20 flop/B.
//
// One 1024-thread workgroup per CU (the weight image takes ~145 KB of the 160 KB LDS), 128 VGPRs, so four waves
// share each SIMD: while some are in their sampling phase others own the SIMD's matrix pipe, and the LDS-table /
// transcendental latencies of the sampling phase are covered by thread-level parallelism.
//
// An activation or weight outside the f16 operand range (|v| > 65504) cannot be split: the pack kernel records
// it in the image's flag slot, the encoder tracks the largest activation it split, and the voxel's terms come
// out NaN -- never a silent clamp (include/qbold_hip.h, operand range; ops.vi_fwd(range_check=True) falls back to
// the exact-f32 layer-wise path).
//
// Two layouts of the sampling phase.  vi_fwd_kernel: 16-voxel wave tiles, the four lanes l, l + 16, l + 32, l + 48
// share voxel l & 15 and split its draws by Philox call -- everything that is per voxel, not per draw (prepare_lik,
// make_mvn, the KL's moment assembly, the divisions) is issued four times for one result, and 18 KL calls take five
// lock-step trips.  vi_fwd_kernel_vox (per-tau-table fast path, T = 11 / 24): 64-voxel wave tiles -- four encoder
// phases on 16-voxel sub-tiles, each exactly vi_fwd_kernel's, then ONE sampling phase in which a lane owns a voxel
// and walks its four draw shares itself, in the four-lane order (voxel_mc_sums<.., 1>, elbo_core.h): the per-voxel
// part runs once per voxel and every per-voxel output is the same bits.  The sub-tile loop stays rolled (unrolled it
// is ~40 KB of code against a 64 KB instruction cache).  Two stretches of a sub-tile differ from vi_fwd_kernel's, in
// what is issued and not in any value (encoder_core.h).  The front end: a lane loads and normalises the spin echo and
// the eight signals of its voxel that it feeds the first layer (first_operand), not all T of them to pick eight, or
// none, afterwards; the clamp is one v_med3_f32.  The head hand-over: the head accumulators of sub-tile s stay as they
// are in register slot s (a scalar branch around four moves), and one in-place transpose of (slot, lane group) per
// tile -- 16 v_permlane*_swap at T = 11 -- hands lane (g, i) the rows of voxel 16 g + i, where gather_head broadcast
// every sub-tile's rows to all four groups and a select per row threw three copies away.  (The classic split-f16
// image at T = 24, L = 2 keeps gather_head: the slots do not fit its registers, vi_fwd_kernels.inc.)  qbold_vi_fwd
// sends whole balanced rounds of 64-voxel tiles (64 voxels on every wave of the device) to vi_fwd_kernel_vox and the
// remainder to vi_fwd_kernel, which keeps normalise, dense_first and gather_head.  Where the registers allow (every
// instance but the classic split-f16 image at T = 11, L = 2) the likelihood draws of vi_fwd_kernel_vox read their
// wave-uniform operands -- the blood brackets, fwd_fast_sig's constants -- from vector registers filled once per tile
// (LikRegs, qbold_dev.h).
//
// The folded gate image (qbold_vi_fwd_folded; ops.vi_fwd's default).  A block's gate logits, Wg r + bg + gate_offset
// with r = Wr2 relu(t) + br2, are affine in relu(t): (Wr2 Wg) relu(t) + (br2 Wg + bg + gate_offset).  The weights do
// not change between calls, so qbold_encoder_pack_gatefold forms that product once (float64, one rounding, times
// -log2(e)) as one more dense op per block, and vi_fwd_kernel_fold / vi_fwd_kernel_vox_fold -- the same text as the two
// kernels above, vi_fwd_kernels.inc -- stage it in the image's gate slots (same LDS footprint, same single barrier).
// A block then takes r and the logits from ONE set of fragments: no operand split of r (40 vector instructions per
// block and sub-tile), no multiply in the sigmoid, a three-instruction blend (32 more), and the gate MFMAs no longer
// wait for the Wr2 product.  Built for the per-tau-table fast path with the split-f16 encoder, both layouts together;
// everything else (the bf16 encoder included: there the product's rounding would be bf16's own), and qbold_vi_fwd
// itself, runs the classic image.  The range guard starts from the larger of the two flag slots.
//
// Wide encoders (U = 256, T <= 16 or 49..64: BASELINE config 3) -- two launches: the one-launch encoder of
// wide_fused_kernels.hip writes q and log sigma into the caller's workspace (qbold_vi_workspace_bytes), the
// compile-time-T ELBO kernel of elbo_kernels.hip reads them back.
#include "elbo_core.h"
// Wave priorities (s_setprio): a wave starts a tile (signal loads, normalisation) at 3, runs its encoder
// phase at 2 (3 inside the MFMA chains), its likelihood draws at 1, its KL draws at 3 and the tile's tail
// at 0 (elbo_core.h).  The four waves of a SIMD are in different phases most of the time; preferring the
// one that feeds the matrix pipe, and the one about to finish, keeps the matrix pipe busy while the
// others fill the VALU: 0.610 -> 0.572 ms per 1 M voxels.
#ifndef QB_PRIO_TILE_START
#define QB_PRIO_TILE_START 3
#endif
#define QB_ENC_BASE_PRIO 2
#include "encoder_core.h"
#include "qbold_ctx.h"

namespace qb {
int check_encoder_shape(const qbold_ctx* ctx, const qbold_encoder_shape* s);
bool elbo_fast_path(const qbold_ctx* ctx);
bool elbo_logsigma_path(const qbold_ctx* ctx);
int elbo_fwd_launch(const qbold_ctx* ctx, const float* x, const float* mask, const float* q, const float* prior,
                    const float* sigma, bool sigma_is_log, const float* zs, const float* zk, int S, int K,
                    uint64_t seed, int64_t voxel0, float* nll_kl, double* sums, void* workspace, int64_t N,
                    hipStream_t s);
bool wide_fused_supported(const qbold_encoder_shape* s);
int wide_fused_fwd(const qbold_ctx* ctx, const qbold_encoder_shape* shape, const float* packed, const float* x,
                   float* out_q, float* out_log_sigma, int64_t N, hipStream_t s);
}

namespace {

using qb::EncLayout;
using qb::f32x4;

constexpr int kBlock = 1024;
// threads per workgroup of the 24-tau instantiations: with 1,024 (128 VGPRs) that protocol's 34 data registers leave the
// kernel ~35 registers short around its sampling phase (140 bytes of scratch per lane, re-read every tile: 4.5 x the
// algorithmic HBM bytes); 768 threads get 168 VGPRs and three waves per SIMD
#ifndef QB_VI_BLOCK_24
#define QB_VI_BLOCK_24 768
#endif

template <int T, int SE, bool GT>
struct ViLds { using type = qb::FwdLds; };
template <int T, int SE>
struct ViLds<T, SE, true> { using type = qb::GtLds<T, SE>; };
constexpr size_t kLdsLimit = 160 * 1024;   // gfx950: LDS per workgroup

// The two kernel templates live in vi_fwd_kernels.inc and are compiled from that one text twice: as vi_fwd_kernel /
// vi_fwd_kernel_vox on the classic image, and as vi_fwd_kernel_fold / vi_fwd_kernel_vox_fold with one more argument,
// the folded gate ops of qbold_encoder_pack_gatefold (header of the .inc).  Two names rather than a template
// parameter: the classic kernels keep their symbols and, token for token the same source, their listings.
#define QB_VI_FOLD 0
#include "vi_fwd_kernels.inc"
#undef QB_VI_FOLD
#define QB_VI_FOLD 1
#include "vi_fwd_kernels.inc"
#undef QB_VI_FOLD

}  // namespace

namespace {
// Wide encoders (BASELINE config 3): the path is two launches -- the one-launch encoder of
// wide_fused_kernels.hip, then the ELBO kernel reading the heads (q, log sigma) back from the workspace.
// Workspace: [per-workgroup partials][log sigma N T floats][q N 5 floats (used when q_out is NULL)].
inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }
bool wide_vi_path(const qbold_ctx* ctx, const qbold_encoder_shape* shape) {
    return qb::wide_fused_supported(shape) && ctx && shape->T == ctx->dev.T && qb::elbo_logsigma_path(ctx);
}
// the shapes vi_fwd_kernel_vox is instantiated for (each with the split-f16 and the bf16 encoder)
bool vox_kernel_built(int T, int L) {
#ifdef QB_VI_PROBE
    return (T == 11 || T == 24) && L == 2;
#else
    return (T == 11 || T == 24) && (L == 1 || L == 2);
#endif
}
}  // namespace

extern "C" int64_t qbold_vi_workspace_bytes(const qbold_ctx* ctx, const qbold_encoder_shape* shape, int64_t N) {
    if (!ctx || !shape || N < 0) return QBOLD_ERR_INVALID;
    const int64_t part = align256(qbold_elbo_workspace_bytes(ctx));
    if (!wide_vi_path(ctx, shape)) return part;
    return part + align256(N * (int64_t)shape->T * 4) + align256(N * 5 * 4);
}

namespace {
// qbold_vi_fwd (gate_fold = NULL) and qbold_vi_fwd_folded.  The folded gate ops are used where the FOLD kernels are
// built: the per-tau-table fast path of the narrow shapes, on both layouts of the sampling phase together (per-voxel
// outputs do not depend on which kernel took a voxel); everywhere else gate_fold is ignored.
int vi_fwd_run(const qbold_ctx* ctx, const qbold_encoder_shape* shape, const float* packed, const float* gate_fold,
               const float* x, const float* mask, const float* prior, int S, int K, uint64_t seed, int64_t voxel0,
               float* q_out, float* nll_kl, double* sums, void* workspace, int64_t N, void* stream) {
    QB_NEED_DEVICE(ctx);
    QB_RELU_ONLY(shape, "qbold_vi_fwd");
    if (wide_vi_path(ctx, shape)) {
        QB_REQUIRE(N >= 0 && S >= 1 && K >= 0, "qbold_vi_fwd: need N >= 0, S >= 1, K >= 0");
        QB_REQUIRE(sums && workspace, "qbold_vi_fwd: null sums/workspace");
        QB_REQUIRE(N == 0 || (packed && x && prior), "qbold_vi_fwd: null input buffer");
        QB_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 256 == 0 && reinterpret_cast<uintptr_t>(packed) % 16 == 0 &&
                       reinterpret_cast<uintptr_t>(x) % 16 == 0,
                   "qbold_vi_fwd: wide shapes need a 256-byte aligned workspace of qbold_vi_workspace_bytes() and "
                   "16-byte aligned packed / x");
        char* w = reinterpret_cast<char*>(workspace);
        float* ls = reinterpret_cast<float*>(w + align256(qbold_elbo_workspace_bytes(ctx)));
        float* qbuf = q_out ? q_out : reinterpret_cast<float*>(reinterpret_cast<char*>(ls) + align256(N * (int64_t)shape->T * 4));
        if (N > 0) {
            const int rc = qb::wide_fused_fwd(ctx, shape, packed, x, qbuf, ls, N, (hipStream_t)stream);
            if (rc) return rc;
        }
        return qb::elbo_fwd_launch(ctx, x, mask, qbuf, prior, ls, true, nullptr, nullptr, S, K, seed, voxel0, nll_kl,
                                   sums, workspace, N, (hipStream_t)stream);
    }
    int rc = qb::check_encoder_shape(ctx, shape);
    if (rc) return rc;
    QB_REQUIRE(N >= 0 && S >= 1 && K >= 0, "qbold_vi_fwd: need N >= 0, S >= 1, K >= 0");
    QB_REQUIRE(sums && workspace, "qbold_vi_fwd: null sums/workspace");
    QB_REQUIRE(N == 0 || (packed && x && prior), "qbold_vi_fwd: null input buffer");
    hipStream_t s = (hipStream_t)stream;
    double* partials = reinterpret_cast<double*>(workspace);
    const int blk = shape->T == 24 ? QB_VI_BLOCK_24 : kBlock, waves = blk / 64;
    const bool lit = ctx->dev.tissue_mode == QBOLD_TISSUE_LITERAL;
    const bool bf = shape->precision == QBOLD_ENC_BF16;
    const bool fast = qb::elbo_fast_path(ctx);
    // The batch in two ranges.  [0, n_vox): whole balanced rounds of 64-voxel wave tiles (64 voxels on each of the
    // device's num_cus x waves waves) go to the one-lane-per-voxel kernel; what is left -- less than one round, which
    // that kernel's four times coarser tiles would quantise four times worse -- goes to the four-lane kernel, as a
    // launch of its own on the offset pointers, and costs what it always did.  The per-voxel outputs do not depend on
    // which kernel took a voxel (elbo_core.h); the three sums depend on it as they depend on the grid.
    // QBOLD_KSEL_VI_FOUR_LANE keeps every voxel on the four-lane kernel, QBOLD_KSEL_VI_WHOLE_TILES sends every whole
    // 64-voxel tile to the new one whatever N is.
    const bool vox_kernel = !(ctx->kernel_sel & QBOLD_KSEL_VI_FOUR_LANE) && vox_kernel_built(shape->T, shape->L) && fast &&
                            qb::gtab_segs(shape->T) > 0 && ctx->dev.se_idx == (shape->T == 24 ? 7 : 2) &&
                            !ctx->dev.multi_norm && !(ctx->kernel_sel & (4 | 8)) && ctx->gtab_ok;
    // the folded gate ops: wherever the per-tau-table kernels run (the condition of QB_DISPATCH_VI's first branch)
    // (split-f16 only: rounded to bf16 the product matrix is another arithmetic than qbold_encoder_fwd's bf16 mode,
    // 1e-3 apart on q -- MEASUREMENTS.md 28 -- so QBOLD_ENC_BF16 keeps the two-step form)
    const bool fold = gate_fold && !bf && vox_kernel_built(shape->T, shape->L) && fast && qb::gtab_segs(shape->T) > 0 &&
                      ctx->dev.se_idx == (shape->T == 24 ? 7 : 2) && !ctx->dev.multi_norm &&
                      !(ctx->kernel_sel & (4 | 8)) && ctx->gtab_ok;
    QB_REQUIRE(!fold || reinterpret_cast<uintptr_t>(gate_fold) % 16 == 0,
               "qbold_vi_fwd_folded: gate_fold must be 16-byte aligned");
    const int64_t round = (ctx->kernel_sel & QBOLD_KSEL_VI_WHOLE_TILES) ? 64 : 64 * (int64_t)ctx->num_cus * waves;
    const int64_t n_vox = vox_kernel ? N / round * round : 0;
    // the reduced-precision encoder is built for the table-mode fast path (the bench / training
    // configuration); the literal and generic paths exist to reproduce float32 semantics
    QB_REQUIRE(!bf || fast, "qbold_vi_fwd: QBOLD_ENC_BF16 needs the table-mode Gaussian fast path");
#define QB_LAUNCH_VI(TT, NL, SE, FAST, LIT) QB_LAUNCH_VI_GT(TT, NL, SE, FAST, LIT, false, false)
#define QB_LAUNCH_VI_GT(TT, NL, SE, FAST, LIT, GT, MIR)                                              \
    do {                                                                                          \
        using LdsT = typename ViLds<TT, SE, GT>::type;                                             \
        constexpr size_t smem = sizeof(float) * qb::make_enc_layout(TT, 64, NL).total + sizeof(LdsT) + \
                                sizeof(double) * 3 * (kBlock / 64);                                \
        static_assert(smem <= kLdsLimit, "weight image + sampling table exceed the LDS");          \
        const float4* tab = qb::IsGtLds<LdsT>::value ? ctx->d_gtab : ctx->d_tab;                    \
        constexpr int BLKT = TT == 24 ? QB_VI_BLOCK_24 : kBlock;                                   \
        auto k = vi_fwd_kernel<TT, NL, SE, FAST, LIT, false, GT, MIR, BLKT>;                       \
        if constexpr (FAST) { if (bf) k = vi_fwd_kernel<TT, NL, SE, FAST, LIT, true, GT, MIR, BLKT>; }   \
        QB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k),                              \
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));       \
        hipLaunchKernelGGL(k, dim3(grid), dim3(BLKT), smem, s, ctx->dev, tab, packed,              \
                           x, mask, prior, S, K, seed, voxel0, q_out, out, partials, N);          \
    } while (0)
#define QB_LAUNCH_VI_FOLD(TT, NL, SEC)                                                             \
    do {                                                                                          \
        constexpr size_t smem = sizeof(float) * qb::make_enc_layout(TT, 64, NL).total +            \
                                sizeof(qb::GtLds<TT, SEC>) + sizeof(double) * 3 * (kBlock / 64);   \
        static_assert(smem <= kLdsLimit, "weight image + sampling table exceed the LDS");          \
        constexpr int BLKT = TT == 24 ? QB_VI_BLOCK_24 : kBlock;                                   \
        auto k = vi_fwd_kernel_fold<TT, NL, SEC, true, false, false, true, false, BLKT>;           \
        QB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k),                              \
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));       \
        hipLaunchKernelGGL(k, dim3(grid), dim3(BLKT), smem, s, ctx->dev, ctx->d_gtab, packed,      \
                           gate_fold, x, mask, prior, S, K, seed, voxel0, q_out, out, partials, N); \
    } while (0)
    // SEC: the protocol's spin-echo index (tau = 0), folded at compile time when the context agrees
#define QB_DISPATCH_VI(TT, NL, SEC)                                              \
    do {                                                                          \
        if (qb::gtab_segs(TT) > 0 && fast && ctx->dev.se_idx == SEC && !ctx->dev.multi_norm && !(ctx->kernel_sel & 4) && ctx->gtab_ok && !(ctx->kernel_sel & 8)) QB_LAUNCH_VI_GT(TT, NL, SEC, true, false, (qb::gtab_segs(TT) > 0), false);   \
        else if (fast && ctx->dev.se_idx == SEC && !ctx->dev.multi_norm && !(ctx->kernel_sel & 4) && ctx->grid_mirrors) QB_LAUNCH_VI_GT(TT, NL, SEC, true, false, false, true);   \
        else if (fast && ctx->dev.se_idx == SEC && !ctx->dev.multi_norm && !(ctx->kernel_sel & 4)) QB_LAUNCH_VI(TT, NL, SEC, true, false);   \
        else if (fast) QB_LAUNCH_VI(TT, NL, -1, true, false);                     \
        else if (lit && ctx->dev.se_idx == SEC && !ctx->dev.multi_norm) QB_LAUNCH_VI(TT, NL, SEC, false, true);   \
        else if (lit) QB_LAUNCH_VI(TT, NL, -1, false, true);                      \
        else QB_LAUNCH_VI(TT, NL, -1, false, false);                              \
    } while (0)
    // the four-lane kernels over one range of the batch; grid: the workgroups launched = the partial-sum slots written
    auto four_lane = [&](const float* x, const float* mask, const float* prior, int64_t voxel0, float* q_out,
                         float2* out, int64_t N, int& grid) -> int {
        const int64_t ntile = (N + 15) / 16;
        const int64_t nblk = (ntile + waves - 1) / waves;
        grid = (int)(nblk < ctx->num_cus ? (nblk > 0 ? nblk : 1) : ctx->num_cus);
        if (fold) {
            if (shape->T == 11 && shape->L == 2) QB_LAUNCH_VI_FOLD(11, 2, 2);
#ifndef QB_VI_PROBE
            else if (shape->T == 11 && shape->L == 1) QB_LAUNCH_VI_FOLD(11, 1, 2);
            else if (shape->T == 24 && shape->L == 1) QB_LAUNCH_VI_FOLD(24, 1, 7);
#endif
            else QB_LAUNCH_VI_FOLD(24, 2, 7);
            QB_HIP(hipGetLastError());
            return QBOLD_OK;
        }
#ifdef QB_VI_PROBE  // scripts/dev/resources.sh: compile the optimal.yaml depth only (register / scratch reports in seconds)
        if (shape->T == 11 && shape->L == 2) QB_DISPATCH_VI(11, 2, 2);
        else if (shape->T == 24 && shape->L == 2) QB_DISPATCH_VI(24, 2, 7);
#else
        if (shape->T == 11 && shape->L == 1) QB_DISPATCH_VI(11, 1, 2);
        else if (shape->T == 11 && shape->L == 2) QB_DISPATCH_VI(11, 2, 2);
        else if (shape->T == 24 && shape->L == 1) QB_DISPATCH_VI(24, 1, 7);
        else if (shape->T == 24 && shape->L == 2) QB_DISPATCH_VI(24, 2, 7);
#endif
        else {
            qb::set_error("qbold_vi_fwd: kernels are built for T = 11 or 24 taus, L = 1 or 2");
            return QBOLD_ERR_UNSUPPORTED;
        }
        QB_HIP(hipGetLastError());
        return QBOLD_OK;
    };
#define QB_LAUNCH_VOX(TT, NL, SEC)                                                                     \
    do {                                                                                              \
        constexpr size_t smem = sizeof(float) * qb::make_enc_layout(TT, 64, NL).total +                \
                                sizeof(qb::GtLds<TT, SEC>) + sizeof(double) * 3 * (kBlock / 64);       \
        static_assert(smem <= kLdsLimit, "weight image + sampling table exceed the LDS");              \
        constexpr int BLKT = TT == 24 ? QB_VI_BLOCK_24 : kBlock;                                       \
        auto k = bf ? vi_fwd_kernel_vox<TT, NL, SEC, true, BLKT> : vi_fwd_kernel_vox<TT, NL, SEC, false, BLKT>; \
        QB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k),                                  \
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));           \
        hipLaunchKernelGGL(k, dim3(vgrid), dim3(BLKT), smem, s, ctx->dev, ctx->d_gtab, packed, x, mask, \
                           prior, S, K, seed, voxel0, q_out, out, partials, n_vox, grid);             \
    } while (0)
#define QB_LAUNCH_VOX_FOLD(TT, NL, SEC)                                                                \
    do {                                                                                              \
        constexpr size_t smem = sizeof(float) * qb::make_enc_layout(TT, 64, NL).total +                \
                                sizeof(qb::GtLds<TT, SEC>) + sizeof(double) * 3 * (kBlock / 64);       \
        static_assert(smem <= kLdsLimit, "weight image + sampling table exceed the LDS");              \
        constexpr int BLKT = TT == 24 ? QB_VI_BLOCK_24 : kBlock;                                       \
        auto k = vi_fwd_kernel_vox_fold<TT, NL, SEC, false, BLKT>;                                     \
        QB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k),                                  \
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));           \
        hipLaunchKernelGGL(k, dim3(vgrid), dim3(BLKT), smem, s, ctx->dev, ctx->d_gtab, packed, gate_fold, x, mask, \
                           prior, S, K, seed, voxel0, q_out, out, partials, n_vox, grid);             \
    } while (0)
    float2* out = reinterpret_cast<float2*>(nll_kl);
    int grid = 0;   // partial-sum slots holding a value
    if (n_vox < N || N == 0) {
        rc = four_lane(x + n_vox * shape->T, mask ? mask + n_vox : nullptr, prior + n_vox * 5, voxel0 + n_vox,
                       q_out ? q_out + n_vox * 5 : nullptr, out ? out + n_vox : nullptr, N - n_vox, grid);
        if (rc) return rc;
    }
    if (n_vox > 0) {
        // second on the stream: its first `grid` workgroups add to the slots the remainder's launch wrote (one writer
        // per slot, in stream order: deterministic), so the workspace holds one slot per workgroup as before
        const int64_t nblk = (n_vox / 64 + waves - 1) / waves;
        const int vgrid = (int)(nblk < ctx->num_cus ? nblk : ctx->num_cus);
        if (fold) {
            if (shape->T == 11 && shape->L == 2) QB_LAUNCH_VOX_FOLD(11, 2, 2);
#ifndef QB_VI_PROBE
            else if (shape->T == 11 && shape->L == 1) QB_LAUNCH_VOX_FOLD(11, 1, 2);
            else if (shape->T == 24 && shape->L == 1) QB_LAUNCH_VOX_FOLD(24, 1, 7);
#endif
            else QB_LAUNCH_VOX_FOLD(24, 2, 7);
        }
        else if (shape->T == 11 && shape->L == 2) QB_LAUNCH_VOX(11, 2, 2);
#ifndef QB_VI_PROBE
        else if (shape->T == 11 && shape->L == 1) QB_LAUNCH_VOX(11, 1, 2);
        else if (shape->T == 24 && shape->L == 1) QB_LAUNCH_VOX(24, 1, 7);
#endif
        else QB_LAUNCH_VOX(24, 2, 7);
        QB_HIP(hipGetLastError());
        grid = vgrid > grid ? vgrid : grid;
    }
#undef QB_LAUNCH_VOX
#undef QB_LAUNCH_VOX_FOLD
#undef QB_LAUNCH_VI_FOLD
#undef QB_DISPATCH_VI
#undef QB_LAUNCH_VI
#undef QB_LAUNCH_VI_GT
    hipLaunchKernelGGL(qb::reduce_partials_kernel, dim3(1), dim3(192), 0, s, partials, grid, sums);
    QB_HIP(hipGetLastError());
    return QBOLD_OK;
}
}  // namespace

extern "C" int qbold_vi_fwd(const qbold_ctx* ctx, const qbold_encoder_shape* shape,
                            const float* packed, const float* x, const float* mask,
                            const float* prior, int S, int K, uint64_t seed, int64_t voxel0,
                            float* q_out, float* nll_kl, double* sums, void* workspace, int64_t N,
                            void* stream) {
    return vi_fwd_run(ctx, shape, packed, nullptr, x, mask, prior, S, K, seed, voxel0, q_out, nll_kl, sums, workspace,
                      N, stream);
}

extern "C" int qbold_vi_fwd_folded(const qbold_ctx* ctx, const qbold_encoder_shape* shape,
                                   const float* packed, const float* gate_fold, const float* x, const float* mask,
                                   const float* prior, int S, int K, uint64_t seed, int64_t voxel0,
                                   float* q_out, float* nll_kl, double* sums, void* workspace, int64_t N,
                                   void* stream) {
    QB_REQUIRE(gate_fold, "qbold_vi_fwd_folded: null gate_fold (qbold_encoder_pack_gatefold fills it)");
    return vi_fwd_run(ctx, shape, packed, gate_fold, x, mask, prior, S, K, seed, voxel0, q_out, nll_kl, sums,
                      workspace, N, stream);
}
