/*
 * qbold_hip.h -- C ABI of libqbold_hip.so: the MI355X (gfx950) implementation of the qBOLD-VI
 * voxel-wise amortised-VI hot path.
 *
 * The reference (wearepal/qBOLD-VI) has no FFI/plugin interface: the path sits behind Python
 * classes used as Keras layers / loss callables.  Each entry point below names the reference
 * interface (file:line, relative to the reference repository root) whose arithmetic it replaces;
 * the Python host mirror in qbold_vi_amd/ keeps the reference's class and method names and calls
 * these functions through ctypes (see INTEGRATION.md for the binding a maintainer would add).
 *
 * Conventions
 *   - every buffer is a caller-owned DEVICE pointer (float32, row-major, channel-last) unless
 *     a parameter is documented as host; nothing is allocated per call;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all work is
 *     asynchronous on that stream, and the library never synchronises the device;
 *   - return value: 0 on success, a negative qbold_status otherwise; functions never throw;
 *   - a context is bound to one device, immutable after creation and re-entrant.
 *
 * Tensor conventions (as the reference): posterior/prior parameters are
 * [mu_oef, raw_s_oef, mu_dbv, raw_s_dbv, raw_c] (model.py:26-31,380-383); (OEF,DBV) pairs are
 * interleaved [V][2] (signals.py:75-77); signals are [V][T] with T = number of taus.
 */
#ifndef QBOLD_HIP_H
#define QBOLD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QBOLD_MAX_T 64
#define QBOLD_ABI_VERSION 5

typedef enum {
    QBOLD_OK = 0,
    QBOLD_ERR_INVALID = -1,     /* bad argument (null pointer, size, unsupported shape) */
    QBOLD_ERR_HIP = -2,         /* a HIP runtime call failed; see qbold_last_error() */
    QBOLD_ERR_UNSUPPORTED = -3, /* configuration outside what the kernels were built for */
    QBOLD_ERR_NO_DEVICE = -4
} qbold_status;

/* System constants: INI `config` [DEFAULT] (config:1-38) as parsed by
 * SignalGenerationLayer.__init__ (signals.py:18-53). */
typedef struct {
    double gamma, b0, dchi, te, r2t, tr, ti, t1b, hct;
    double tau_start, tau_end, tau_step; /* tf.range(...) grid, signals.py:34-35 */
    int32_t full_model;                  /* signals.py:192: Simpson/Bessel tissue model or log-linear */
    int32_t include_blood;               /* signals.py:100 */
} qbold_consts;

/* Likelihood / normalisation switches of EncoderTrainer.__init__ (model.py:54-95). */
typedef struct {
    int32_t multi_image_normalisation; /* model.py:102-106, 540-545 */
    int32_t predict_log_data;          /* model.py:547-549 */
    int32_t use_student_t;             /* model.py:557: student_t_df is not None and < 50 */
    double student_t_df;
} qbold_loss_cfg;

/* How the tissue integral F(x) of signals.py:159-185 is evaluated. */
typedef enum {
    QBOLD_TISSUE_TABLE = 0,   /* cubic-Hermite table of the reference's float32 Simpson-129 sum */
    QBOLD_TISSUE_LITERAL = 1  /* the 129-node Simpson sum with Cephes j0f, per (voxel, tau) */
} qbold_tissue_mode;

/* Arithmetic of the fused voxel-wise encoder kernels (qbold_encoder_fwd, qbold_vi_fwd, qbold_encoder_wide_fwd,
 * qbold_encoder_fused_fwd).
 *
 * QBOLD_ENC_F32 operand range.  Every weight and activation x enters the matrix cores as hi = f16(x) plus a lo half
 * carrying the next 11 bits; products hi.hi + hi.lo + lo.hi accumulate in float32 (the lo.lo term, <= 2^-22
 * relative, is dropped).  Consequences the float32 reference does not share:
 *   - |x| > 65504 (the largest f16): hi overflows to inf.  The heads then come out non-finite and, because
 *     nll * mask is NaN for a NaN nll whatever the mask, so do the three sums: NON-FINITE SUMS ARE THE STATUS
 *     CHANNEL for this condition (the library never clamps silently).  The exact-float32 layer-wise path
 *     (qbold_encoder_train_fwd + qbold_elbo_fwd) has no such limit; the Python mirror's
 *     Context.vi_fwd(range_check=True) / FineTuner.elbo fall back to it.
 *   - 6.1e-5 <= |x| <= 65504: 22 significant bits (relative error <= ~7e-7 per product).
 *   - |x| < 6.1e-5: both halves are f16 subnormals, absolute resolution 2^-35 = 2.9e-11 (LDS-resident kernels,
 *     lo scaled by 2^11) or 2^-25 = 3e-8 for activations in qbold_encoder_fused_fwd (unscaled lo; its weights
 *     are pre-scaled per dense op by a power of two, so their lo halves stay normal) -- absolute errors far
 *     below float32 rounding of an O(1) layer output, but the RELATIVE precision of tiny operands degrades.
 *   tests/test_gpu_parity.py::test_split_operand_range drives all three regimes against the oracle. */
typedef enum {
    QBOLD_ENC_F32 = 0,  /* float32-grade: operands split into two f16 halves, three MFMAs per tile */
    QBOLD_ENC_BF16 = 1  /* operands rounded to bfloat16, float32 accumulate (BASELINE config 5:
                           "bf16 forward / fp32 ELBO accum"); sampling and ELBO stay float32 */
} qbold_encoder_precision;

typedef enum {
    QBOLD_ACT_RELU = 0, /* 'relu': both of the reference's configuration files */
    QBOLD_ACT_GELU = 1  /* 'gelu' (Keras: exact, 0.5 x (1 + erf(x / sqrt 2))): the class default of EncoderTrainer */
} qbold_activation;

/* Voxel-wise encoder geometry (model.py:122-223; 3x3x1 convolutions act through their centre
 * tap on (N,1,1,1,T) voxel batches). */
typedef struct {
    int32_t T;                  /* no_ip_images */
    int32_t U;                  /* no_units */
    int32_t L;                  /* no_intermediate_layers */
    int32_t channelwise_gating; /* model.py:160-162 */
    float gate_offset;          /* model.py:169 */
    int32_t spatial_taps;       /* 1: Wr1/Wr2 hold the centre tap [U][U] only (voxel batches);
                                   9: full 3x3x1 kernels [3][3][U][U] in Keras order (model.py:152-157) */
    int32_t precision;          /* qbold_encoder_precision; the packed image (qbold_encoder_pack) and the
                                   kernels that read it must be given the same value */
    int32_t activation;         /* qbold_activation: EncoderTrainer's activation_type (model.py:60, 115-120, 151, 155).
                                   QBOLD_ACT_GELU runs on the layer-wise entry points (qbold_encoder_train_fwd / _bwd,
                                   qbold_encoder_spatial_fwd / _bwd: general kernels, pre-activations recomputed in the
                                   backward); the fused / wide entry points return QBOLD_ERR_UNSUPPORTED for it (ABI v4) */
    int32_t layer_norm;         /* EncoderTrainer's use_layer_norm (model.py:133-140): tfa GroupNormalization(groups = 1,
                                   axis = -1) in front of both activations of a block's residual path -- mean and biased
                                   variance over ALL positions and channels of one batch element (a voxel of a voxel batch,
                                   a whole crop of a crop batch), epsilon 1e-3, per-channel gamma / beta: 4 U more
                                   parameters per block behind the heads (qbold_encoder_num_params).  Layer-wise entry
                                   points only, like gelu (ABI v5) */
    float dropout_rate;         /* EncoderTrainer's dropout_rate: keras Dropout in front of each GroupNormalization (or
                                   activation).  Active in the TRAINING forward / backward when dropout_seed != 0: an
                                   element is dropped iff its 16-bit uniform of the library's Philox stream 5, keyed
                                   (dropout_seed; row, normalizer, column), is below rate 2^16; kept ones scale by
                                   1 / (1 - rate).  Inference (dropout_seed = 0) is the identity, as in Keras */
    uint64_t dropout_seed;      /* per-step seed, the same for a step's forward and backward; 0 = inference */
} qbold_encoder_shape;

/* Image-crop geometry of a [B][X][Y][Z][C] batch (train.py:17-72): voxel v = ((b X + x) Y + y) Z + z.
 * The 3x3x1 'same' convolutions couple (x, y) neighbours within one b and z. */
typedef struct {
    int32_t B, X, Y, Z;
} qbold_geometry;

typedef struct qbold_ctx qbold_ctx;

int qbold_abi_version(void);
const char* qbold_last_error(void);

/* ---- context ----------------------------------------------------------------------------- */
/* Replaces SignalGenerationLayer.__init__ (signals.py:18-53) + EncoderTrainer.__init__'s
 * se_idx (model.py:95).  Builds the tau grid, the folded float32 constants and the F(x) table
 * and uploads them to `device`. */
int qbold_ctx_create(const qbold_consts* consts, const qbold_loss_cfg* loss, int device,
                     qbold_ctx** out);
void qbold_ctx_destroy(qbold_ctx* ctx);
int qbold_ctx_num_taus(const qbold_ctx* ctx);
int qbold_ctx_se_idx(const qbold_ctx* ctx);
/* host_out: HOST float[T] */
int qbold_ctx_taus(const qbold_ctx* ctx, float* host_out);
int qbold_ctx_set_tissue_mode(qbold_ctx* ctx, int mode);
int qbold_ctx_tissue_mode(const qbold_ctx* ctx);
/* Gradient of the tissue integral: 1 (default) = TensorFlow's autodiff value, the J1-kernel
 * Simpson sum over all 129 nodes; 0 = the exact derivative of the float32 forward value, in which
 * node 0 is flat.  They differ by 1.95e-3 * x. */
int qbold_ctx_set_grad_node0(qbold_ctx* ctx, int on);
/* Which of several EQUIVALENT kernels an entry point dispatches to (default 0 = the fastest form of each).  Every bit
 * selects an older / simpler kernel that computes the same result; the tests use them to hold the fused kernels to
 * the layer-wise ones.  No bit skips work (the work-skipping hooks of the timing experiments exist only in
 * -DQBOLD_ABLATION builds, scripts/dev/build_ablation.sh). */
#define QBOLD_KSEL_RUNTIME_SE_IDX 4          /* ELBO kernels: run-time instead of compile-time spin-echo index */
#define QBOLD_KSEL_X_TABLE 8                 /* ELBO kernels: x-indexed F table per (draw, tau) instead of the per-tau OEF-indexed one */
#define QBOLD_KSEL_CONV_PER_TAP 256          /* 3x3x1 convolution as nine gathered GEMM launches */
#define QBOLD_KSEL_GENERAL_GEMM 512          /* layer GEMMs on the general xw_kernel */
#define QBOLD_KSEL_SEPARATE_GATE 2048        /* gate blend as its own launch; layer-wise backward: gate backward and the gating conv's backward-data product as two */
#define QBOLD_KSEL_SEPARATE_BWD_DATA 4096    /* a block's two backward-data GEMMs as two launches */
#define QBOLD_KSEL_SEPARATE_FORK 8192        /* skip / t of a block as two GEMMs */
#define QBOLD_KSEL_PER_HEAD_BWD 16384        /* one backward pass per head */
#define QBOLD_KSEL_PER_HEAD_FWD 32768        /* one forward GEMM per head */
#define QBOLD_KSEL_CONV_EXACT_F32 65536      /* 3x3x1 convolution on the f32-input MFMA */
#define QBOLD_KSEL_LAYERWISE_BWD 131072      /* voxel batches: layer-wise backward instead of the one-launch block kernels */
#define QBOLD_KSEL_BLOCK_BWD_SPLIT_DW 262144 /* block backward with separate weight-gradient launches */
#define QBOLD_KSEL_DW_EXACT_F32 524288      /* 3x3x1 weight gradients as exact f32 products instead of bf16 pieces */
#define QBOLD_KSEL_HEADS_BWD_LAYERWISE 1048576 /* heads' backward as delta tensor + GEMM + weight-gradient pass */
#define QBOLD_KSEL_SLAB_SUMS_SEPARATE 2097152 /* crop backward: every weight-gradient slab sum as its own launch instead of the queued ones */
#define QBOLD_KSEL_DW_BF16_PIECES 4194304     /* layer-wise weight gradients on three bfloat16 pieces per operand instead of two f16 halves */
#define QBOLD_KSEL_ELBO_BWD_GENERIC 8388608   /* qbold_elbo_bwd at T = 11 / 24: the run-time-T kernel of every other protocol (Gaussian likelihood on linear data; Student-t / log-data contexts keep the specialised kernels) */
#define QBOLD_KSEL_VI_FOUR_LANE 16777216      /* qbold_vi_fwd: every voxel on the kernel with four lanes per voxel (16-voxel wave tiles) instead of whole balanced rounds of 64-voxel tiles on the one-lane-per-voxel kernel */
#define QBOLD_KSEL_VI_WHOLE_TILES 33554432   /* qbold_vi_fwd: every whole 64-voxel tile on the one-lane-per-voxel kernel whatever N is (default: whole rounds of num_cus x waves tiles only), the remainder on the four-lane kernel: per-voxel outputs are the same bits either way */
#define QBOLD_KSEL_ALL (4 | 8 | 256 | 512 | 2048 | 4096 | 8192 | 16384 | 32768 | 65536 | 131072 | 262144 | 524288 | 1048576 | 2097152 | 4194304 | 8388608 | 16777216 | 33554432)
int qbold_ctx_set_kernel_selection(qbold_ctx* ctx, int mask);
/* Host-side evaluation of the uploaded table (for tests): F(x) and dF/dx, HOST arrays. */
int qbold_ctx_table_eval(const qbold_ctx* ctx, const float* host_x, float* host_F, float* host_dF,
                         int64_t n);

/* ---- forward signal model ------------------------------------------------------------------ */
/* SignalGenerationLayer.call without noise/misalignment (signals.py:55-114,137-138):
 * oef_dbv [V][2] -> signal [V][T]. */
int qbold_signal_fwd(const qbold_ctx* ctx, const float* oef_dbv, float* signal, int64_t V,
                     void* stream);
/* The same with the options configurations/optimal.yaml disables (signals.py:64-96).  hct [V]:
 * per-voxel haematocrit (variable_hct, :64-70) or NULL for the config's value.  Misalignment
 * (:80-96) with its random draws made by the caller: images t > from_index[v] are computed from
 * alt_oef_dbv[v] (the perturbed, clipped pair); from_index[v] >= T-1 leaves voxel v aligned.  Both
 * NULL: no misalignment. */
int qbold_signal_fwd_ex(const qbold_ctx* ctx, const float* oef_dbv, const float* hct,
                        const float* alt_oef_dbv, const int32_t* from_index, float* signal, int64_t V,
                        void* stream);
/* Vector-Jacobian product of the above: grad_signal [V][T] -> grad_oef_dbv [V][2]
 * (what tf.GradientTape yields through signals.py:55-114). */
int qbold_signal_bwd(const qbold_ctx* ctx, const float* oef_dbv, const float* grad_signal,
                     float* grad_oef_dbv, int64_t V, void* stream);

/* ---- encoder ------------------------------------------------------------------------------- */
/* Number of floats of the canonical (Keras-orientation, [in][out]) weight blob:
 * W0[T][U] b0[U] { Wc[U][U] bc[U] Wr1[taps][U][U] br1[U] Wr2[taps][U][U] br2[U] Wg[U][G] bg[G] } x L
 * Wf[U][5] bf[5] Ws[U][T] bs[T]   (model.py:181,144,152,156,164,196,211-214); taps = spatial_taps. */
int64_t qbold_encoder_num_params(const qbold_encoder_shape* shape);
/* Size in floats of the device workspace holding the MFMA-ordered copy of the weights. */
int64_t qbold_encoder_packed_floats(const qbold_encoder_shape* shape);
/* Re-order the canonical blob into the LDS image the kernels stage (call after every update). */
int qbold_encoder_pack(const qbold_ctx* ctx, const qbold_encoder_shape* shape,
                       const float* weights, float* packed, void* stream);
/* The folded gate ops qbold_vi_fwd_folded reads beside the image (U <= 64 shapes): per block one dense op in the
 * layout of the image's ops -- 4096 floats of A fragments [k-step][m][hi, lo][lane][8 halves], 64 floats of bias
 * [m][group][reg] -- holding  A = -log2(e) (Wr2 Wg)  and  bias = -log2(e) (br2 Wg + bg + gate_offset)  (centre tap
 * of Wr2 when spatial_taps == 9; a shared gate broadcast to all units; rows >= U zero).  The product is formed in
 * float64, rounded once to float32 and split into f16 halves like every weight (whatever shape->precision says: the
 * folded kernels are built for the split-f16 encoder only).  Behind the L ops: one flag
 * float (0, or the largest folded weight beyond the f16 operand range) and padding to a multiple of 4 floats.
 * qbold_encoder_gatefold_floats: the buffer's size in floats.  Pack after every weight update, as the image. */
int64_t qbold_encoder_gatefold_floats(const qbold_encoder_shape* shape);
int qbold_encoder_pack_gatefold(const qbold_ctx* ctx, const qbold_encoder_shape* shape,
                                const float* weights, float* fold, void* stream);
/* create_encoder forward, voxel-wise (model.py:97-113 normalise_data, :122-223):
 * x [N][T] -> out1 [N][5] (stream 1), out2 [N][5] (stream 2), sigma [N][T]; any may be NULL. */
int qbold_encoder_fwd(const qbold_ctx* ctx, const qbold_encoder_shape* shape, const float* packed,
                      const float* x, float* out1, float* out2, float* sigma, int64_t N,
                      void* stream);

/* The same encoder for widths beyond the LDS-resident kernels (BASELINE config 3: 64 taus,
 * no_units 256): one weight-streaming split-f16 MFMA GEMM per layer over activations in HBM, with
 * bias / relu / gate / head fused into the epilogues.  Built for U = 128 or 256, L <= 8, T <= 64,
 * channel-wise gating, QBOLD_ENC_F32.  *_packed_floats / *_workspace_floats return the sizes (in
 * floats) of the image and of the caller-owned activation workspace for N voxels, or a negative
 * qbold_status.  stream_sel = 1: out_q = stream-1 parameters (model.py:199), out_log_sigma unused;
 * 2: out_q = stream-2 parameters (:208), out_log_sigma [N][T] = log of the sigma head (:211-214). */
int64_t qbold_encoder_wide_packed_floats(const qbold_encoder_shape* shape);
int64_t qbold_encoder_wide_workspace_floats(const qbold_encoder_shape* shape, int64_t N);
int qbold_encoder_wide_pack(const qbold_ctx* ctx, const qbold_encoder_shape* shape, const float* weights,
                            float* packed, void* stream);
int qbold_encoder_wide_fwd(const qbold_ctx* ctx, const qbold_encoder_shape* shape, const float* packed,
                           const float* x, int stream_sel, float* workspace, float* out_q,
                           float* out_log_sigma, int64_t N, void* stream);

/* The stream-2 encoder of the same wide shapes in ONE launch, activations resident in registers from the
 * first layer to the heads (HBM sees x once and the heads once; create_encoder, model.py:122-223).  Built for
 * U = 256, L = 1 or 2, T <= 16 or 49 <= T <= 64, channel-wise gating, QBOLD_ENC_F32; *_packed_floats returns
 * the image size in floats or a negative qbold_status for other shapes.  x [N][T] -> out_q [N][5] (model.py:208),
 * out_log_sigma [N][T] (the sigma head before its exp, :211-214).  packed, and x / out_log_sigma when T is a
 * multiple of 4, must be 16-byte aligned. */
int64_t qbold_encoder_fused_packed_floats(const qbold_encoder_shape* shape);
int qbold_encoder_fused_pack(const qbold_ctx* ctx, const qbold_encoder_shape* shape, const float* weights,
                             float* packed, void* stream);
int qbold_encoder_fused_fwd(const qbold_ctx* ctx, const qbold_encoder_shape* shape, const float* packed,
                            const float* x, float* out_q, float* out_log_sigma, int64_t N, void* stream);

/* ---- logit-Normal pieces -------------------------------------------------------------------- */
/* ReparamTrickLayer.call + forward_transform (model.py:15-50, 299-305): q [N][5], z [N][2] ->
 * oef_dbv [N][2]. */
int qbold_reparam(const qbold_ctx* ctx, const float* q, const float* z, float* oef_dbv, int64_t N,
                  void* stream);
/* logit_gaussian_mvg_log_prob (model.py:376-400 = logit_mvn.py:46-70): NEGATIVE log-density of
 * y [N][2] under params [N][5] -> out [N]. */
int qbold_logit_mvn_nlogp(const qbold_ctx* ctx, const float* y, const float* params, float* out,
                          int64_t N, void* stream);
/* kl_loss against a mixture-of-Gaussians population prior (use_mvg = False, use_population_prior = True,
 * mog_components = M > 1; model.py:666-685): q [N][5] (columns 0-3), comps DEVICE [M][4] raw parameters (M <= 16),
 * z = explicit normals [N][2] (OEF draw, DBV draw) or NULL for the in-kernel Philox stream -> kl [N] (unmasked). */
int qbold_kl_mog(const qbold_ctx* ctx, const float* q, const float* comps, int M, const float* z, uint64_t seed,
                 int64_t voxel0, float* kl, int64_t N, void* stream);
/* EncoderTrainer.squared_whitened_residual (model.py:423-441) = LogitMVN.squared_whitened_residual
 * (logit_mvn.py:20-38), a static method there and context-free here: obs, mean [N][2]; oef_log_std, dbv_log_std,
 * oef_dbv_cov [N] (already transformed) -> out [N] = || L^-1 (obs - mean) ||^2. */
int qbold_squared_whitened_residual(const float* obs, const float* mean, const float* oef_log_std,
                                    const float* dbv_log_std, const float* oef_dbv_cov, float* out, int64_t N,
                                    void* stream);
/* calculate_means(include_r2p=True, return_stds=True) (model.py:318-343): q [N][5] ->
 * means [N][3], vars [N][3] over n_samples reparameterised draws.  z = explicit normals
 * [N][n_samples][2] or NULL for the in-kernel Philox stream (seed, global voxel = voxel0+i). */
int qbold_posterior_moments(const qbold_ctx* ctx, const float* q, const float* z, int n_samples,
                            uint64_t seed, int64_t voxel0, float* means, float* vars, int64_t N,
                            void* stream);

/* EncoderTrainer.normalise_data (model.py:97-113): x [N][T] -> log(clip(x)/clip(x)[se]) [N][T]. */
int qbold_normalise(const qbold_ctx* ctx, const float* x, float* out, int64_t N, void* stream);

/* loglinear.fit_wls (loglinear.py:68-105): the log-linear comparator.  Per voxel a weighted
 * least-squares line ln S = c - R2' tau over the taus > tau_min (reference: 0.016) with weights
 * 1/tau, in closed form; DBV = c - ln S(tau = 0), OEF = R2' / (DBV gamma 4/3 pi dchi hct B0);
 * clipped to [0.01,0.8], [0.002,0.25], [1e-2,100].  signals [N][T] -> out [N][3] = (OEF, DBV, R2').
 * The taus are rounded to 7 decimals in float32 as the reference does (:126-127); fails with
 * QBOLD_ERR_ARG when no tau equals 0 or fewer than two taus exceed tau_min. */
int qbold_wls_fit(const qbold_ctx* ctx, const float* signals, double tau_min, float* out, int64_t N,
                  void* stream);

/* Element-wise parameter transforms of EncoderTrainer / LogitMVN (model.py:288-316 =
 * logit_mvn.py:72-100).  The FORWARD/BACKWARDS ops act on interleaved (OEF, DBV) pairs. */
typedef enum {
    QBOLD_TRANSFORM_STD = 0,            /* tanh(x)*3 - 1                     model.py:288-290 */
    QBOLD_TRANSFORM_OFFDIAG = 1,        /* tanh(x)*exp(-2)                   model.py:292-294 */
    QBOLD_INV_TRANSFORM_STD = 2,        /* atanh((x+1)/3)                    model.py:296-297 */
    QBOLD_FORWARD_TRANSFORM = 3,        /* sigmoid * range + min             model.py:299-305 */
    QBOLD_BACKWARDS_TRANSFORM = 4,      /* (y - min) / range                 model.py:307-311 */
    QBOLD_BACKWARDS_TRANSFORM_LOGIT = 5,/* ... followed by logit             model.py:312-314 */
    QBOLD_EXP = 6                       /* exp(x): sigma from the sigma head, model.py:214 */
} qbold_transform_op;
int qbold_transform(const qbold_ctx* ctx, int op, const float* in, float* out, int64_t n,
                    void* stream);

/* fine_tune_loss_fn(return_mean=False) before the mask multiply (model.py:527-563): data x [N][T],
 * mask [N] or NULL, predicted signals pred [N*S][T] and sigma [N*S][T] (row j belongs to voxel
 * j % N, the reference's S-fold batch tiling, model.py:529) -> nll [N*S]. */
int qbold_nll_fwd(const qbold_ctx* ctx, const float* x, const float* mask, const float* pred,
                  const float* sigma, float* nll, int64_t N, int S, void* stream);

/* mvg_kl_samples (model.py:592-610) per voxel: q, prior [N][5]; zk explicit normals [N][K][2] or
 * NULL for the Philox KL stream (seed, voxel0 + i) -> kl [N]. */
int qbold_kl_fwd(const qbold_ctx* ctx, const float* q, const float* prior, const float* zk, int K,
                 uint64_t seed, int64_t voxel0, float* kl, int64_t N, void* stream);
/* mvg_kl closed form, use_population_prior = False (model.py:612-652) -> kl [N]. */
int qbold_kl_closed(const qbold_ctx* ctx, const float* q, const float* prior, float* kl, int64_t N,
                    void* stream);
/* kl_loss of the DIAGONAL family (use_mvg = False, use_population_prior = False; model.py:686-721):
 * tfp LogitNormal.kl_divergence per dimension, closed form.  q, prior [N][5] (columns 0-3 used).
 * kl_v [N] or NULL; g_q [N][5] or NULL: [m_v > 0] d kl_v / d q is ADDED to columns 0-3 (analytic
 * KL: no stop-gradient); sums: DEVICE double[3] = (0, sum [m > 0] kl, sum m); workspace as
 * qbold_elbo_fwd. */
int qbold_kl_diag(const qbold_ctx* ctx, const float* q, const float* prior, const float* mask, float* kl_v,
                  float* g_q, double* sums, void* workspace, int64_t N, void* stream);

/* The counter-based normal stream the fused kernels consume: z [N][n][2] for global voxels
 * voxel0 .. voxel0+N-1; stream_id 0 = likelihood draws, 1 = KL draws, 2 = moments, 3 = noise, 6 = the importance
 * draws of qbold_log_evidence_fwd, 7 = the refinement draws of qbold_refine_posterior, 8 = the predictive draws of
 * qbold_posterior_predictive (4 is qbold_kl_mog's, 5 the dropout masks').
 * Replaces tf.random.normal at model.py:25 with a reproducible, sharding-invariant generator
 * (Random123 Philox4x32-7, four draws per call: draw i = word i & 3 of call i >> 2 keyed (voxel, call, stream_id; seed);
 * Box-Muller on the word's low sixteen bits (radius, u1 = (lo + 0.5) 2^-16, so |z| <= 4.8549) and top 23 bits (angle,
 * (w >> 9) 2^-23 revolutions).  The definition is this library's; oracle/qbold_oracle.c restates it. */
int qbold_normals(const qbold_ctx* ctx, uint64_t seed, uint32_t stream_id, int64_t voxel0, int n,
                  float* z, int64_t N, void* stream);

/* Noise model of SignalGenerationLayer.call (signals.py:116-128), in place on signal [V][T]:
 * std[v][t] = mean_v(signal[.][t]) / (U(snr_lo, snr_hi)[v] * norm_snr[t]).  norm_snr: HOST [T]. */
int64_t qbold_noise_workspace_bytes(const qbold_ctx* ctx);
int qbold_signal_add_noise(const qbold_ctx* ctx, float* signal, const float* norm_snr_host,
                           float snr_lo, float snr_hi, uint64_t seed, int64_t voxel0,
                           void* workspace, int64_t V, void* stream);

/* ---- ELBO ----------------------------------------------------------------------------------- */
/* Size in bytes of the scratch the ELBO / fused kernels need for their per-workgroup partials. */
int64_t qbold_elbo_workspace_bytes(const qbold_ctx* ctx);

/* One voxel-ELBO evaluation given the encoder outputs: build_fine_tuner's sampling + forward
 * model (model.py:245-248,273), fine_tune_loss_fn (model.py:527-568), kl_loss -> mvg_kl_samples
 * (model.py:654-665, 592-610), masked sums as train.py:351.
 *   x [N][T], mask [N] (NULL = ones), q / prior [N][5], sigma [N][T]
 *   zs [N][S][2], zk [N][K][2] explicit normals, or NULL for the in-kernel Philox4x32-7 stream (qbold_normals)
 *   keyed (seed; global voxel voxel0+i; draw) -- identical for any sharding of the voxels
 *   nll_kl [N][2] per-voxel (nll averaged over S, kl) or NULL
 *   sums: DEVICE double[3] = (sum_v m*nll, sum_v [m>0] kl, sum_v m), overwritten
 *   workspace: qbold_elbo_workspace_bytes() bytes */
int qbold_elbo_fwd(const qbold_ctx* ctx, const float* x, const float* mask, const float* q,
                   const float* prior, const float* sigma, const float* zs, const float* zk, int S,
                   int K, uint64_t seed, int64_t voxel0, float* nll_kl, double* sums,
                   void* workspace, int64_t N, void* stream);

/* The same with the sigma head handed over BEFORE its exp (log_sigma [N][T], model.py:211-214), as the one-launch
 * wide encoder (qbold_encoder_fused_fwd) writes it; Philox stream only.  Built for the 64-tau protocol whose
 * tau = 0 image is index 12 (BASELINE config 3; table mode, Gaussian likelihood, one-image normalisation):
 * QBOLD_ERR_UNSUPPORTED otherwise. */
int qbold_elbo_fwd_logsigma(const qbold_ctx* ctx, const float* x, const float* mask, const float* q,
                            const float* prior, const float* log_sigma, int S, int K, uint64_t seed, int64_t voxel0,
                            float* nll_kl, double* sums, void* workspace, int64_t N, void* stream);

/* The whole hot path in one launch: encoder stream 2 (model.py:122-223) -> S reparameterised
 * samples -> forward model -> NLL, K-sample KL against `prior`, masked sums.  q_out [N][5]
 * receives the posterior parameters (NULL to skip); other arguments as qbold_elbo_fwd. */
/* Wide shapes (qbold_encoder_fused_packed_floats(shape) > 0 on the 64-tau protocol, BASELINE config 3) run as
 * two launches -- the one-launch encoder, then the ELBO kernel on its heads: `packed` is then the image of
 * qbold_encoder_fused_pack and `workspace` must hold qbold_vi_workspace_bytes(ctx, shape, N) bytes, 256-byte
 * aligned (for the LDS-resident shapes that is qbold_elbo_workspace_bytes()). */
int64_t qbold_vi_workspace_bytes(const qbold_ctx* ctx, const qbold_encoder_shape* shape, int64_t N);
int qbold_vi_fwd(const qbold_ctx* ctx, const qbold_encoder_shape* shape, const float* packed,
                 const float* x, const float* mask, const float* prior, int S, int K, uint64_t seed,
                 int64_t voxel0, float* q_out, float* nll_kl, double* sums, void* workspace,
                 int64_t N, void* stream);
/* qbold_vi_fwd with the gate logits of the gated residual blocks taken from relu(t) through the product matrix:
 * gl = Wg r + bg + gate_offset with r = Wr2 relu(t) + br2 is gl = (Wr2 Wg) relu(t) + (br2 Wg + bg + gate_offset), so
 * the kernels read `gate_fold` (qbold_encoder_pack_gatefold: that product, formed once per weight update) beside
 * `packed` and split no second operand per block.  Same contract, same operand-range rule (a folded weight beyond
 * 65504 poisons every voxel, as a weight of the image does); outputs agree with qbold_vi_fwd's to float32 rounding of
 * the product, not bit for bit.  The folded kernels are built for the per-tau-table fast path (T = 11 or 24, L <= 2,
 * table mode, Gaussian likelihood, the protocol's own spin echo, one-image normalisation) with the split-f16 encoder;
 * on every other shape or context, and for QBOLD_ENC_BF16 (rounded to bf16 the product matrix would be another
 * arithmetic than qbold_encoder_fwd's, 1e-3 apart on q), this IS qbold_vi_fwd on `packed` and `gate_fold` is not read
 * (it must still be non-NULL).  gate_fold: 16-byte aligned. */
int qbold_vi_fwd_folded(const qbold_ctx* ctx, const qbold_encoder_shape* shape, const float* packed,
                        const float* gate_fold, const float* x, const float* mask, const float* prior, int S, int K,
                        uint64_t seed, int64_t voxel0, float* q_out, float* nll_kl, double* sums, void* workspace,
                        int64_t N, void* stream);

/* Importance-weighted evidence (Burda et al. 2016) of the fine-tuning model (model.py:239-286, 527-568, 592-610):
 * per voxel K draws z_k ~ q, log w_k = -nll(x|z_k) - log q(z_k) + log prior(z_k) on the SAME draw.
 *   out [N][3] = (log p^ = logsumexp log w - log K, mean_k log w (the same-draw ELBO), ESS = (sum w)^2 / sum w^2)
 *   is_means [N][3] or NULL: self-normalised posterior means of (OEF, DBV, R2') (calculate_means' columns)
 *   z: explicit normals [N][K][2] or NULL for the Philox stream 6 (seed, voxel0 + i): qbold_normals(seed, 6, ...)
 *   sums: DEVICE double[3] = (sum_{m>0} m (-log p^), sum_{m>0} m (-ELBO_same), sum m), overwritten
 *   workspace: qbold_elbo_workspace_bytes() bytes; x, mask, q, prior, sigma, stream as qbold_elbo_fwd.
 * The use_mvg = True family: configurations qbold_elbo_fwd accepts; QBOLD_ERR_UNSUPPORTED otherwise.
 * QBOLD_ERR_INVALID for K < 1, K > QBOLD_IW_MAX_K (2 K must index the explicit normals with 32 bits) or NULL out. */
#define QBOLD_IW_MAX_K (1 << 30)
int qbold_log_evidence_fwd(const qbold_ctx* ctx, const float* x, const float* mask, const float* q,
                           const float* prior, const float* sigma, const float* z, int K, uint64_t seed,
                           int64_t voxel0, float* out, float* is_means, double* sums, void* workspace,
                           int64_t N, void* stream);

/* Gradient of the importance-weighted bound above with respect to the encoder's head outputs, for fine-tuning the encoder
 * on it (this package's addition; the reference trains on the ELBO only).  Per voxel the K draws of
 * qbold_log_evidence_fwd (explicit z [N][K][2], or the Philox stream 6 keyed (seed, voxel0 + i): the same draws for the
 * same seed), u_k = mu + L eps_k, log w_k as there, w~_k = softmax_k(log w), loss l_v = -(logsumexp_k log w_k - log K).
 *   log_sigma [N][T]: the sigma head BEFORE exp, as qbold_elbo_bwd takes it
 *   g_log_sigma [N][T] = m_v sum_k w~_k d nll_k / d log sigma_t   (the exact gradient of l_v for fixed eps)
 *   g_q [N][5] = m_v sum_k w~_k^2 (d nll_k / du + d (log q - log p)_k / du, q held inside log q) du_k / dq_raw: the
 *     doubly-reparameterised gradient (DReG, Tucker et al. 2019), chained to the raw heads as qbold_elbo_bwd chains
 *     its own, clipped draws included.  At K = 1 and m in {0, 1} it is qbold_elbo_bwd's gradient of m nll + KL with
 *     the KL drawn at the likelihood's draw.
 *   Both UNNORMALISED by sum(m), like qbold_elbo_bwd's; voxels with mask <= 0 (or NaN) get exact zeros and add nothing
 *   to the sums; mask NULL = ones.
 *   out [N][3] or NULL: qbold_log_evidence_fwd's columns (log p^, ELBO_same, ESS)
 *   sums: DEVICE double[3] = (sum_{m>0} m (-log p^), sum_{m>0} m (-ELBO_same), sum_{m>0} m), overwritten: [2] is the
 *     normaliser qbold_encoder_train_bwd / qbold_encoder_spatial_bwd read
 *   workspace: qbold_elbo_workspace_bytes() bytes.
 * Fixed-order sums, no atomics: a voxel's outputs are the same bits at any batch position, under any sharding by voxel0
 * and run to run.  Full signal model in table mode, T = 11 or 24 with every likelihood switch (every other protocol:
 * qbold_log_evidence_bwd_anyt below), the use_mvg = True family;
 * QBOLD_ERR_UNSUPPORTED otherwise.  QBOLD_ERR_INVALID for K < 1, K > QBOLD_IW_MAX_K or a NULL required buffer. */
int qbold_log_evidence_bwd(const qbold_ctx* ctx, const float* x, const float* mask, const float* q,
                           const float* prior, const float* log_sigma, const float* z, int K, uint64_t seed,
                           int64_t voxel0, float* g_q, float* g_log_sigma, float* out, double* sums,
                           void* workspace, int64_t N, void* stream);

/* qbold_log_evidence_bwd on any tau grid, 1 <= T <= 64 (run-time-T kernel: the voxel's normalised data, 1 / sigma and
 * its T sigma sums in LDS, the streaming log-sum-exp and the five DReG sums in registers).  Arguments, draws (Philox
 * stream 6 or z: draw k is draw k of qbold_log_evidence_fwd), the lane mapping by K, outputs, masked voxels, sums,
 * workspace, the bitwise properties and the QBOLD_ERR_INVALID cases are those of qbold_log_evidence_bwd, which is
 * unchanged: it keeps its T = 11 / 24 kernels, their bits, and QBOLD_ERR_UNSUPPORTED for every other T.
 *   This entry takes T = 11 and 24 too and runs the run-time-T kernel there: the same function on the same draws,
 *   the likelihood-gradient sums regrouped (one pass over the taus per draw), so it agrees with the specialised
 *   kernels to rounding, not to the bit.
 *   Configurations: those of the any-T forward and of qbold_elbo_bwd at these T -- full signal model, table mode,
 *   Gaussian likelihood on linear data, either normalisation, the spin echo on or off the grid.
 *   Traffic per voxel: 4 (2 T + 10 + 1) B in (+ 8 K B of z when given), 4 (T + 5) B out (+ 12 with out); with K > 32
 *   the four lanes of a voxel repeat the reads.
 * QBOLD_ERR_UNSUPPORTED for a context without the full signal model, for the literal tissue mode, and for the
 * Student-t likelihood or log data (qbold_log_evidence_bwd has those at T = 11 / 24). */
int qbold_log_evidence_bwd_anyt(const qbold_ctx* ctx, const float* x, const float* mask, const float* q,
                                const float* prior, const float* log_sigma, const float* z, int K, uint64_t seed,
                                int64_t voxel0, float* g_q, float* g_log_sigma, float* out, double* sums,
                                void* workspace, int64_t N, void* stream);

/* The per-draw rows behind qbold_log_evidence_fwd, unreduced (this package's addition): the K draws of that entry
 * (explicit z [N][K][2], or the Philox stream 6 keyed (seed, voxel0 + i): draw k of this call is draw k there) and per
 * draw
 *   log_w [N][K] = -nll - (log q - log p), the value qbold_log_evidence_fwd folds into its log-sum-exp
 *   theta [N][K][3] or NULL: (OEF, DBV, R2') of the draw.
 * No sums, no workspace.  Voxels with mask <= 0 (or NaN) are not read and their rows are filled with NaN; mask NULL =
 * ones.  A voxel's rows are the same bits at any batch position and under any sharding by voxel0.
 * Table mode: T = 11 / 24 with every likelihood switch (Student-t, log data, three-image normalisation), every other
 * T <= 64 on the configuration of qbold_log_evidence_fwd's generic kernel (Gaussian likelihood, linear data); the
 * literal tissue mode and anything else: QBOLD_ERR_UNSUPPORTED.  QBOLD_ERR_INVALID for K < 1, K > QBOLD_IW_MAX_K, a
 * NULL log_w or a NULL input buffer.  x, q, prior, sigma, stream as qbold_log_evidence_fwd. */
int qbold_log_evidence_draws(const qbold_ctx* ctx, const float* x, const float* mask, const float* q,
                             const float* prior, const float* sigma, const float* z, int K, uint64_t seed,
                             int64_t voxel0, float* log_w, float* theta, int64_t N, void* stream);

/* Pareto-smoothed importance sampling (Vehtari, Simpson, Gelman, Yao, Gabry, JMLR 2024) of N independent rows of K
 * log-weights (this package's addition; nothing of the qBOLD model enters).
 *   log_w [N][K]: any finite values; -inf is a zero weight; a NaN (or +inf, or no finite value) anywhere in a row makes
 *     that row's outputs NaN.
 *   theta [N][K][C] or NULL, 1 <= C <= QBOLD_PSIS_MAX_C: per-draw quantities to average.
 *   mask [N] or NULL (= ones): rows with mask <= 0 (or NaN) are not read; their outputs are NaN.
 * Per row, with x = log_w - max:  M = ceil(min(K / 5, 3 sqrt K));  the cutoff c = the (M + 1)-th largest x;  the tail =
 * the n entries strictly greater than c (ties at the cutoff shorten it), ascending, equal values by ascending draw;
 * y_r = expm1(x_r - c) (the paper's exp(x) - exp(c) up to the factor exp(c), to which the fit's k is invariant);
 * Zhang & Stephens' fit: m = 30 + floor(sqrt n) candidates b_j = 1 / y_n + (1 - sqrt(m / (j - 1/2))) / (3 y_q),
 * q = floor(n / 4 + 1/2), k_j = mean_r log1p(-b_j y_r), L_j = n (log(-b_j / k_j) - k_j - 1), b^ = sum_j softmax(L)_j b_j,
 * k = mean_r log1p(-b^ y_r), sigma = -k / b^, k^ = (n k + 5) / (n + 10);  the tail entry of rank r becomes
 * c + log1p(sigma expm1(-k log1p(-p_r)) / k), p_r = (r - 1/2) / n (k = 0: -sigma log1p(-p_r)), truncated at 0, the
 * largest raw weight; then the row is normalised by its log-sum-exp.  k^ = +inf and the weights stay unsmoothed (but
 * normalised) when n <= 4, when -c > 80 (beyond float32's exp), or when the fit is not finite.
 *   out [N][4] = (k^, log p^_PSIS = max + logsumexp(smoothed x) - log K, ESS_PSIS = 1 / sum w~^2, n)
 *   means [N][C] or NULL (needs theta): sum_k w~_k theta_k
 *   weights [N][K] or NULL: log w~, normalised.
 * k^ below min(1 - 1 / log10 K, 0.7) marks a reliable estimate.  Fixed-order sums, no atomics: a row's outputs are the
 * same bits at any position in the batch.  QBOLD_ERR_INVALID for K outside [QBOLD_PSIS_MIN_K, QBOLD_PSIS_MAX_K] (a
 * row fits a wave, 16 draws per lane; at 25 the tail has its five points), C outside its range, means without theta,
 * or a NULL log_w / out. */
#define QBOLD_PSIS_MIN_K 25
#define QBOLD_PSIS_MAX_K 1024
#define QBOLD_PSIS_MAX_C 8
int qbold_psis(const qbold_ctx* ctx, const float* log_w, const float* theta, int C, const float* mask, int K,
               float* out, float* means, float* weights, int64_t N, void* stream);

/* Summaries of N independent rows of K weighted draws: moments, weighted quantiles, the highest-density interval and
 * correlations (this package's addition; like qbold_psis, nothing of the qBOLD model enters).
 *   log_w [N][K], or NULL for equal weights (the intervals of q's own draws): -inf is a zero weight; a NaN, a +inf or
 *     no finite value in a row makes every output of the row NaN (qbold_psis's rule).  Raw log_w and qbold_psis'
 *     normalised `weights` are both valid inputs.
 *   theta [N][K][C], 1 <= C <= QBOLD_SUMMARY_MAX_C: a NaN in a column makes that column's outputs NaN; the other
 *     columns and row_out are unaffected.
 *   mask [N] or NULL (= ones): rows with mask <= 0 (or NaN) are not read; their outputs are NaN.
 *   K in [QBOLD_SUMMARY_MIN_K, QBOLD_SUMMARY_MAX_K];  P in [0, QBOLD_SUMMARY_MAX_P] levels probs_host[P], read from the
 *     host, each strictly inside (0, 1);  hpd_mass strictly inside (0, 1).
 * Definitions, per row and column:
 *   w~_k = exp(lw_k - max) / sum_j exp(lw_j - max).
 *   mean = sum w~ theta.
 *   sd = sqrt(sum w~ (theta - mean)^2), computed in two passes with no Bessel correction.
 *   Sort the column ascending.  Equal values are ordered by ascending draw.  W_r is the inclusive cumulative sum of w~
 *   in that order.
 *   Quantile at level p = theta_(r*), with r* = min{r : W_r >= p}; r* is clamped to K - 1.  This is the inverse
 *   weighted ECDF (numpy's `inverted_cdf`).  It does not interpolate, so the result is always one of the draws.
 *   HPD = the shortest [theta_(a), theta_(b)] with W_b - W_{a-1} >= hpd_mass.  For each a, b(a) is the smallest feasible
 *   b.  Width ties go to the smallest a.  An a with no feasible b is skipped.
 *   row_out [N][2] = (ESS = 1 / sum w~^2, max_k w~_k).
 *   corr [N][C (C - 1) / 2], or NULL.  It holds the weighted Pearson correlations in the pair order (0,1), (0,2), ...,
 *   (C-2,C-1).  An entry is NaN where an sd is 0.
 *   stats [N][C][4] = (mean, sd, hpd_lo, hpd_hi).
 *   quant [N][C][P], or NULL when P = 0.
 * The kernel works in float32: W_r is within (K + 32) 2^-24 of its exact value, so a quantile lies between the exact
 * rule's values at levels p -+ (K + 32) 2^-23, and the interval likewise in its mass.  Draws whose float32 weight is 0
 * are ordered after every other draw: they change no value above (if hpd_mass is so close to 1 that rounding leaves no
 * feasible pair, the interval is the range of the draws with a positive weight).  Widths are compared as exact
 * float64 differences.  Fixed-order sums, no atomics: a row's outputs are the same bits at any position in the batch
 * and whether or not quant / corr are requested.
 * QBOLD_ERR_INVALID for K, C or P out of range, a level or a mass outside (0, 1), quant NULL while P > 0, N < 0, or a
 * NULL theta, stats or row_out. */
#define QBOLD_SUMMARY_MIN_K 4
#define QBOLD_SUMMARY_MAX_K 1024
#define QBOLD_SUMMARY_MAX_C 8
#define QBOLD_SUMMARY_MAX_P 8
int qbold_draw_summary(const qbold_ctx* ctx, const float* log_w, const float* theta, int C, const float* mask, int K,
                       const float* probs_host, int P, float hpd_mass, float* stats, float* quant, float* row_out,
                       float* corr, int64_t N, void* stream);

/* Semi-amortised inference (Kim et al. 2018; Cremer et al. 2018): refine each voxel's posterior, starting from given
 * encoder heads, by `steps` gradient steps on that voxel's own objective
 *   E_q[nll(x | y)] + KL(q || prior)   (exact closed-form KL of the logit-space Gaussians, sigma fixed, no TV term)
 * -- what a Python loop of qbold_elbo_bwd + qbold_adamw_step on the N x 5 heads would do, in one launch with the
 * voxel's data, heads and optimiser state in registers.  This package's addition; the reference has no counterpart.
 *   q_in, q_out [N][5]: raw heads (the encoder's parameterisation, transform_std / transform_offdiag); q_out may alias
 *     q_in.  Voxels with mask <= 0 (or NaN) get q_in copied bit for bit; mask NULL refines every voxel.
 *   sigma [N][T]: the exponentiated sigma, as qbold_elbo_fwd takes it.
 *   Per step j: S reparameterised likelihood draws; the gradient of their mean NLL plus the exact gradient of the
 *     closed-form KL (the expectation of the Monte-Carlo KL gradient while the logit clip does not bind), then Adam
 *     (bias-corrected) or SGD at lr_j = lr_final + (lr - lr_final)(1 + cos(pi j / steps)) / 2.
 *   z: explicit normals [N][steps][Sp][2], Sp = 4 ceil(S / 4) (draws S .. Sp - 1 of a step unused), or NULL for the
 *     Philox stream 7 keyed by the global voxel: step j's draw d is draw j Sp + d of qbold_normals(seed, 7, voxel0,
 *     steps Sp), so results do not depend on the sharding.
 *   loss [N][2] or NULL: the Monte-Carlo -ELBO (mean NLL of the step's draws + closed-form KL) at step 0 and its mean
 *     over the last ceil(steps / 10) steps; 0 for masked voxels.
 * Full signal model in table mode, T = 11 or 24; QBOLD_ERR_UNSUPPORTED otherwise.
 * QBOLD_ERR_INVALID for steps < 1, S < 1, steps Sp / 4 >= 2^32 (the Philox call word), lr <= 0, lr_final < 0, Adam
 * betas outside [0, 1) or eps <= 0, an optimizer other than 0 / 1, or a NULL required buffer. */
typedef struct {
    int optimizer; /* 0 Adam, 1 SGD */
    float lr, lr_final, beta1, beta2, eps;
} qbold_refine_cfg;
int qbold_refine_posterior(const qbold_ctx* ctx, const float* x, const float* mask, const float* q_in,
                           const float* prior, const float* sigma, const float* z, int steps, int S,
                           const qbold_refine_cfg* cfg, uint64_t seed, int64_t voxel0,
                           float* q_out, float* loss, int64_t N, void* stream);

/* The same refinement of a volume under the TV smoothness prior of the fine-tuning loss (model.py:726-754; this
 * package's addition).  The volume is in qbold_smoothness's layout: geom {B, X, Y, Z}, voxel
 * v = ((b X + x) Y + y) Z + z, N = B X Y Z.  The steps minimise the joint objective
 *   F(q) = sum_{v: m_v > 0} (E_q_v[nll(x_v | .)] + KL(q_v || p_v)) + tv_weight TV(q),
 *   TV(q) = sum over x- and y-adjacent pairs (v, n) with m_v > 0 and m_n > 0 of
 *           |sigmoid(q_v[0]) - sigmoid(q_n[0])| + |sigmoid(q_v[2]) - sigmoid(q_n[2])|
 * -- the first sum qbold_refine_posterior's, TV qbold_smoothness's tv_sum (no z term, as in the reference); F / sum(mask)
 * is the reference's fine-tuning loss with kl weight 1 and the closed-form KL when tv_weight = smoothness_weight.  The
 * subgradient of |d| is sign(d), sign(0) = 0.
 *   Jacobi steps: at step j every voxel's gradient is taken at the step-j heads of all voxels (its own draws and KL at
 *   its own heads, the TV subgradient against its neighbours' step-j means), then every voxel takes its own Adam / SGD
 *   update: full-batch Adam / SGD on F, independent of how voxels map to lanes or launches.
 *   Draws, z, the cosine schedule, cfg, loss [N][2] (the -ELBO part only), the configurations and the error codes are
 *   qbold_refine_posterior's.  tv_weight = 0 couples nothing and runs qbold_refine_posterior itself (its bits, one
 *   launch, the workspace unused); tv_weight > 0 runs one launch per step, whose per-voxel part agrees with
 *   qbold_refine_posterior's arithmetic to rounding.
 *   Voxels with mask <= 0 (or NaN) get q_in copied bit for bit and never enter a TV edge; mask NULL = all voxels in.
 *   q_out may alias q_in.  voxel0: the global index of the volume's first voxel (the Philox key).  TV never couples
 *   batch elements or z slices, so sharding by whole batch elements (voxel0 = b0 X Y Z) gives the same bits.
 *   workspace: qbold_refine_spatial_workspace_bytes() bytes (88 per voxel), 16-byte aligned, not kept between calls.
 * All work on `stream`.  QBOLD_ERR_INVALID also for a non-finite or negative tv_weight, a bad geometry,
 * a voxel count (or workspace size) beyond int64, or a NULL or misaligned workspace. */
int64_t qbold_refine_spatial_workspace_bytes(const qbold_ctx* ctx, const qbold_geometry* geom);
int qbold_refine_posterior_spatial(const qbold_ctx* ctx, const float* x, const float* mask, const float* q_in,
                                   const float* prior, const float* sigma, const float* z,
                                   const qbold_geometry* geom, float tv_weight, int steps, int S,
                                   const qbold_refine_cfg* cfg, uint64_t seed, int64_t voxel0,
                                   float* q_out, float* loss, void* workspace, void* stream);

/* The two refinements on any tau grid, 1 <= T <= 64 (run-time-T kernels: the voxel's normalised data and 1 / sigma in
 * LDS, heads and optimiser state in registers).  Arguments, draws (Philox stream 7 or z), schedule, optimisers, loss,
 * masked voxels, aliasing, the 88-byte-per-voxel workspace (qbold_refine_spatial_workspace_bytes) and the
 * QBOLD_ERR_INVALID cases are those of qbold_refine_posterior / qbold_refine_posterior_spatial, which are unchanged:
 * they keep their T = 11 / 24 kernels, their bits, and QBOLD_ERR_UNSUPPORTED for every other T.
 *   These entries take T = 11 and 24 too and run the run-time-T kernels there: the same function on the same draws,
 *   the gradient sums regrouped (one pass over the taus per draw), so they agree with the specialised kernels to
 *   rounding, not to the bit.  qbold_refine_posterior_spatial_anyt with tv_weight = 0 runs
 *   qbold_refine_posterior_anyt itself (its bits).
 *   Traffic per voxel: per-voxel entry 4 (2 T + 10 + 1) B in and 20 (+ 8 with loss) B out whatever the number of
 *   steps (+ 8 Sp B of z per step when given); spatial entry, per step, 4 (2 T + 21) B in and 68 B out, as
 *   qbold_refine_posterior_spatial.
 * QBOLD_ERR_UNSUPPORTED only for the literal tissue mode or a context without the full signal model. */
int qbold_refine_posterior_anyt(const qbold_ctx* ctx, const float* x, const float* mask, const float* q_in,
                                const float* prior, const float* sigma, const float* z, int steps, int S,
                                const qbold_refine_cfg* cfg, uint64_t seed, int64_t voxel0,
                                float* q_out, float* loss, int64_t N, void* stream);
int qbold_refine_posterior_spatial_anyt(const qbold_ctx* ctx, const float* x, const float* mask, const float* q_in,
                                        const float* prior, const float* sigma, const float* z,
                                        const qbold_geometry* geom, float tv_weight, int steps, int S,
                                        const qbold_refine_cfg* cfg, uint64_t seed, int64_t voxel0,
                                        float* q_out, float* loss, void* workspace, void* stream);

/* Exact per-voxel posteriors of the fine-tuning model by quadrature on the logit plane (this package's addition; the
 * reference has no counterpart).  With sigma fixed the latent space is u = (a, b), the logits of (OEF, DBV), and
 *   J(u) = -nll(x | OEF(clip a), DBV(clip b); sigma) + log N(u; mu_p, Sigma_p)
 * is the log-joint (nll: qbold_elbo_fwd's per-draw NLL with every likelihood switch; clip at +-13.8155, the logit
 * clip of model.py:393-396; N: the prior's logit-space Gaussian, make_mvn of prior[5]); the sigmoid Jacobians cancel,
 * so its integral over u is the log p(x) that qbold_log_evidence_fwd converges to.
 *   1. Start box B0: a in mu_a +- span sd_a, b in mu_b +- span sd_b (Sigma_p's marginal sds); with q, the bounding box
 *      of that box and q's; intersected with [-clip, clip]^2.
 *   2. locate passes k = 1 .. locate: coarse x coarse nodes at linspace points over B_{k-1} (endpoints included);
 *      M = max J; keep the rows whose maximum J exceeds M - cut, and the columns likewise; B_k = the range of the kept
 *      rows and columns widened by one node step on each side, intersected with B_{k-1}.
 *   3. fine pass: fine x fine linspace nodes over B_locate, steps h_a, h_b, equal weights w_ij = exp(J_ij - M_f).
 *   4. out [N][QBOLD_GRID_OUT]:
 *      0 log_p = M_f + log sum w + log(h_a h_b)
 *      1 elbo_q = E_q[-nll] - KL(q || prior): E_q by the gh x gh product Gauss-Hermite rule in q's whitened
 *        coordinates (u = mu_q + L_q sqrt(2) t), the KL in closed form (qbold_refine_posterior's); NaN when q is NULL
 *        or gh = 0
 *      2-4 posterior means of OEF, DBV, R2' = dw_coef OEF DBV;  5-7 their posterior sds;  8 corr(OEF, DBV)
 *      9-10 OEF quantiles at level_lo, level_hi; 11-12 DBV quantiles: of the logit marginals (row sums, column sums),
 *        each node's mass spread uniformly over its cell [u_i - h/2, u_i + h/2] (the CDF linear within a cell),
 *        mapped through forward_transform (monotone)
 *      13-14 OEF, DBV at the fine grid's argmax node (a tie goes to the lowest row-major index)
 *      15 edge_mass = the mass on the fine grid's outer ring / sum w (large: the box truncated the posterior)
 *      16 quad_err = |log Z_h - log Z_2h|, Z_2h = 4 h_a h_b sum over even i, even j of w_ij (large: under-resolved)
 *   box [N][4] or NULL: (a_lo, a_hi, b_lo, b_hi) of the fine pass.
 *   Voxels with mask <= 0 (or NaN) are not evaluated: NaN rows, nothing in the sums; mask NULL evaluates every voxel.
 *   sums: DEVICE double[3] = (sum_{m>0} m (-log_p), sum_{m>0} m (-elbo_q) (0 without q), sum_{m>0} m), overwritten
 *     (qbold_log_evidence_fwd's layout).  No random stream, no atomics: a voxel's outputs are the same bits in any
 *     batch at any position.
 *   workspace: qbold_elbo_workspace_bytes() bytes; x, mask, prior, sigma, q (heads [N][5]), stream as qbold_elbo_fwd.
 * Defaults: coarse 32, fine 64, locate 2, gh 16, span 6, cut 40, levels 0.025 / 0.975.  Configurations
 * qbold_log_evidence_fwd accepts; QBOLD_ERR_UNSUPPORTED otherwise.  QBOLD_ERR_INVALID for coarse not a multiple of 8
 * in [16, 128], fine not a multiple of 8 in [16, 256], locate outside [1, 4], gh not 0 or in [2, 32], span <= 0, cut
 * outside [10, 80], levels not 0 < level_lo < level_hi < 1, or a NULL required buffer. */
typedef struct {
    int coarse, fine, locate, gh;
    float span, cut, level_lo, level_hi;
} qbold_grid_cfg;
#define QBOLD_GRID_OUT 17
int qbold_posterior_grid(const qbold_ctx* ctx, const float* x, const float* mask, const float* prior,
                         const float* sigma, const float* q, const qbold_grid_cfg* cfg, float* out, float* box,
                         double* sums, void* workspace, int64_t N, void* stream);

/* Per-voxel Laplace posteriors of the fine-tuning model on any tau grid (this package's addition; the reference has no
 * counterpart): the MAP of qbold_posterior_grid's log-joint by Levenberg-Marquardt on the logit plane -- the classical
 * per-voxel non-linear least-squares fit, with the prior as two more residual rows -- and the Gauss-Newton (Fisher)
 * curvature there, returned as numbers and as five raw heads that every entry taking q accepts.  No encoder is involved.
 *   Model (qbold_posterior_grid's): u = (a, b), the logits of (OEF, DBV), kept within +-13.8155; sigma fixed.
 *     F(u) = 1/2 (sum_t r_t^2 + |w|^2),  r_t = (y_t - yh_t(u)) / sigma_t,  w = L_p^-1 (u - mu_p)
 *     y, yh: data and prediction, each divided by its own spin-echo image (the mean of three with multi-image
 *     normalisation) + 1e-3, as qbold_elbo_bwd forms them; (mu_p, L_p) = make_mvn of prior[5].  So
 *     -F = J - (-sum_t log sigma_t - (T/2) log 2 pi - log 2 pi - log det L_p), J the grid entry's log-joint.
 *   A = J^T J, the 2 x 2 Gauss-Newton matrix over the T + 2 residual rows (positive definite through the prior rows),
 *   g = J^T r, dec(u) = sqrt(g^T A^-1 g): the Newton decrement, the distance to the stationary point in posterior sds.
 *   J is the derivative of the r that is evaluated: the tissue table drops Simpson node 0 from F (as the reference's
 *   float32 value does) and J takes the table's own slope, without that node's -- unlike qbold_elbo_bwd, which restates
 *   the reference's autodiff gradient and keeps it (qbold_ctx_set_grad_node0 has no effect here).
 *   Schedule.  Start u_0 = clip(u0 row), or clip(mu_p) when u0 is NULL; lambda = lambda0.  The start point is evaluated
 *   and accepted (iterations = 0; a voxel with dec(u_0) < tol stops there).  Then at most max_iter iterations, each one
 *   evaluation of (F, g, A) at the trial point
 *       u' = clip(u + delta),  delta = -(A + lambda diag A)^-1 g   (A, g at the last accepted point u):
 *     with dF = F(u) - F(u'), except that when |F(u) - F(u')| <= band
 *         dF = -1/2 (g(u) + g(u'))^T (u' - u)   [the tie rule: the trapezoid rule on the two gradients, exact for a
 *         quadratic F], band = max(band(u), band(u')), band(v) = 2^-22 (sum_t |r_t| yh_t / sigma_t + F) at v: what
 *         two float32 roundings of every yh_t move F by, to first order.  Within it float32 cannot order the two
 *         values of F, while the gradients keep their digits.
 *     dF > 0: accepted, u <- u'.  The voxel has converged and stops when dec(u) < tol.  Then [the gain rule]
 *         lambda <- max(lambda * (1 / lambda_down), 1e-7) when dF >= 0.25 pred, pred = -g^T d - 1/2 d^T A d the
 *         quadratic model's reduction along the step d = u' - u actually taken; lambda <- min(lambda * lambda_up, 1e7)
 *         otherwise: the step is kept but the damping raised.  Gauss-Newton leaves out the residuals' curvature; on a
 *         weakly determined voxel its full step overshoots about twofold along the soft direction, F still falls a
 *         little every time, and without this rule lambda only shrinks while the iterates zig-zag across the valley
 *         past max_iter (MEASUREMENTS.md section 27).
 *     otherwise (a non-finite F(u') included): rejected, lambda <- min(lambda * lambda_up, 1e7).
 *     Deviations from the plain accept-if-lower schedule: the tie rule, the gain rule, the bracket [1e-7, 1e7] of
 *     lambda, and the division by lambda_down as a multiplication by its float32 reciprocal.
 *   Defaults: max_iter 50, lambda0 1e-2, lambda_up 10, lambda_down 3, tol 1e-3.
 *   u0 [N][2] or NULL.  sigma [N][T]: the exponentiated sigma, as qbold_elbo_fwd takes it.
 *   out [N][QBOLD_LAPLACE_OUT], everything at the last accepted point u^, Sigma = A^-1 there:
 *      0-1  a^, b^
 *      2-4  OEF, DBV, R2' = dw_coef OEF DBV at u^
 *      5-7  sd_a, sd_b, corr of Sigma
 *      8-10 delta-method sds of OEF, DBV, R2' (the transforms' slopes at u^ through Sigma)
 *      11   log p^ = J(u^) + log 2 pi - 1/2 log det A: the Laplace evidence, comparable with qbold_posterior_grid's log_p
 *      12   chi2 = sum_t r_t^2 at u^
 *      13   iterations used (trial points after the start point)
 *      14   flags, as a float: bit 0 = not converged within max_iter, bit 1 = a coordinate of u^ sits on the clip,
 *           bit 2 = heads clamped
 *   q_out [N][5]: raw heads whose make_mvn is (u^, the Cholesky factor of Sigma): e^(2 s_o) = Sigma_aa,
 *     c = Sigma_ab / e^(s_o), e^(2 s_d) = Sigma_bb - c^2, through the inverses of transform_std / transform_offdiag.  Those
 *     reach s in (-4, 2) and |c| < e^-2 only; each tanh is clamped to |tanh(raw)| <= 1 - 1e-6, i.e. s to
 *     [-4 + 3e-6, 2 - 3e-6] and |c| to (1 - 1e-6) e^-2, and e^(2 s_d) is formed with the c that is stored, so that the
 *     marginal variance of b survives a clamped c.  Any clamp sets bit 2; out keeps the unclamped Sigma.
 *   Voxels with mask <= 0 (or NaN) are not evaluated: a NaN row in out, the prior row copied bit for bit to q_out; mask
 *   NULL evaluates every voxel.  No random stream, no atomics, no sums, no workspace: a voxel's outputs are the same
 *   bits in any batch at any position, whatever shares its wave.  One run-time-T kernel serves every 1 <= T <= 64.
 * Full signal model in table mode, Gaussian likelihood on linear data, either normalisation, any spin-echo index;
 * QBOLD_ERR_UNSUPPORTED otherwise (literal tissue mode, Student-t, log data, no full model).  QBOLD_ERR_INVALID for
 * max_iter < 1, a non-positive or non-finite lambda0 or tol, lambda_up <= 1 or lambda_down <= 1 (or non-finite), N < 0
 * or a NULL required buffer (cfg, q_out, out; x, prior, sigma when N > 0); these are checked first. */
typedef struct {
    int max_iter;
    float lambda0, lambda_up, lambda_down, tol;
} qbold_laplace_cfg;
#define QBOLD_LAPLACE_OUT 15
int qbold_laplace_posterior(const qbold_ctx* ctx, const float* x, const float* mask, const float* prior,
                            const float* sigma, const float* u0, const qbold_laplace_cfg* cfg,
                            float* q_out, float* out, int64_t N, void* stream);

/* Adaptive importance sampling per voxel by moment matching (this package's addition; Paananen, Piironen, Buerkner &
 * Vehtari 2021 and the population Monte Carlo family): `rounds` rounds of K draws from the current proposal, each
 * weighted as qbold_log_evidence_fwd weights them, after each of which the proposal's mean and covariance move to the
 * weighted ones (shrunk by lambda = ESS / (ESS + shrink)); the proposal of the round with the largest ESS comes back as
 * raw heads that every entry taking q accepts.  qbold_vi_amd/csrc/adapt_kernels.hip states the algorithm in full in its
 * head; tests/_adapt_reference.py restates it in float64.
 *   q [N][5]: the starting heads (the encoder's, qbold_laplace_posterior's, or the prior's own row).  z [N][rounds K][2]
 *   explicit normals or NULL: draw r K + k of qbold_normals(seed, 9, voxel0 + i, rounds K) (Philox stream 9).
 *   q_out [N][5]; out [N][2 rounds + 2] = (log p^_r, ESS_r) per round, the returned round's index, flags (bit 0 a round
 *   skipped for non-finite weights, bit 1 a mean reached the logit clip, bit 2 a spread head was clamped -- bits 1 and 2
 *   as qbold_laplace_posterior's); q_rounds [N][rounds][5] or NULL: every round's proposal as raw heads (row 0 and a
 *   returned round 0 are the given heads bit for bit).  Voxels with mask <= 0 (or NaN) are not read: q_out is q's row,
 *   out and q_rounds rows are NaN.  No atomics, no workspace, no sums: a voxel's outputs are the same bits in any batch
 *   at any position (with voxel0 following it).  One run-time-T kernel serves every 1 <= T <= 64.
 * Full signal model in table mode, Gaussian likelihood on linear data, either normalisation, any spin-echo index;
 * QBOLD_ERR_UNSUPPORTED otherwise.  QBOLD_ERR_INVALID for rounds outside 1 .. 16, K outside 8 .. 1024 or no multiple of
 * 4, a shrink that is not positive and finite, N < 0 or a NULL required buffer (cfg, q_out, out; x, q, prior, sigma
 * when N > 0); these are checked first.  N = 0 returns QBOLD_OK without a launch. */
typedef struct { int rounds; int K; float shrink; } qbold_adapt_cfg;
#define QBOLD_ADAPT_MAX_ROUNDS 16
#define QBOLD_ADAPT_MIN_K 8
#define QBOLD_ADAPT_MAX_K 1024
int qbold_adapt_posterior(const qbold_ctx* ctx, const float* x, const float* mask, const float* q, const float* prior,
                          const float* sigma, const float* z /* nullable */, const qbold_adapt_cfg* cfg, uint64_t seed,
                          int64_t voxel0, float* q_out, float* out, float* q_rounds /* nullable */, int64_t N,
                          void* stream);

/* Fisher information of the likelihood the library fits with, at given points, and the Cramer-Rao bounds that follow
 * (this package's addition): how well a tau protocol can determine OEF and DBV in a voxel at all, apart from any fit.
 *   A point is theta = (OEF, DBV) with logits (a, b) through forward_transform.  yhat_t(theta) = s_t / (mean of s over
 *   the normalisation window + 1e-3) is the prediction the likelihood scores, sigma_t its per-tau standard deviation,
 *   w_t >= 0 the per-tau weights: the number of averages of tau t, so that the variance is sigma_t^2 / w_t; w_t = 0
 *   drops the tau.  Rows j_t = (d yhat_t / da, d yhat_t / db) / sigma_t, formed exactly as qbold_laplace_posterior
 *   forms its Jacobian rows (the table's own F without Simpson node 0's slope, the window's one or three images first).
 *     I(theta; w) = sum_t w_t j_t j_t^T      the data information, 2 x 2 on the logit plane
 *     Lambda = L_p^-T L_p^-1                 the prior precision, (mu_p, L_p) = make_mvn of prior[5]
 *     A = I + Lambda, Sigma = A^-1           the Bayesian information and its bound
 *   This is the information of independent noise sigma_t on the NORMALISED data: the normaliser's own noise is ignored,
 *   as the likelihood ignores it.  Under one-image normalisation the spin-echo row is therefore ~ 0 although that image
 *   must be acquired; the library does not account for that (scripts/design_protocol.py --require-se does).
 *   theta [N][2]; sigma [sigma_rows][T], sigma_rows = N (per voxel) or 1 (one row shared by all voxels); weights [T] or
 *   NULL = all ones (the same bits); prior [N][5] or NULL; mask [N] or NULL = ones.
 *   out [N][QBOLD_FISHER_OUT]:
 *      0-2  I_aa, I_ab, I_bb
 *      3    kappa = (I_aa I_bb + I_ab^2) / det I, the conditioning of the data information
 *      4    log det I
 *      5-8  the data-only Cramer-Rao bound I^-1: sd of OEF, DBV, R2' = dw_coef OEF DBV (delta method through the
 *           transforms' slopes, as qbold_laplace_posterior's columns 8-10), and the OEF-DBV correlation of I^-1
 *      9-12 the same four from Sigma = (I + Lambda)^-1; NaN when prior is NULL
 *      13   log det A; NaN when prior is NULL
 *      14   flags, as a float: bit 0 = the data information is singular to float32, det I <= 2^-20 (I_aa I_bb + I_ab^2):
 *           column 3 is then +inf and columns 4-8 are -inf, +inf, +inf, +inf, NaN (columns 9-13 stand, A is positive
 *           definite through the prior); bit 1 = theta outside the transforms' open ranges (0.04, 0.84) x (0.001,
 *           0.201), or NaN: columns 0-13 are NaN and this column is 2
 *   Voxels with mask <= 0 (or NaN) get a NaN row, flags included.  No random stream, no atomics, no sums, no workspace:
 *   a voxel's row is the same bits in any batch at any position.  One run-time-T kernel serves every 1 <= T <= 64.
 * Configurations: qbold_laplace_posterior's; QBOLD_ERR_UNSUPPORTED otherwise.  QBOLD_ERR_INVALID for a NULL out (theta,
 * sigma when N > 0), sigma_rows not in {1, N}, N < 0 and a negative or non-finite weight; these are checked first.
 * The weights are checked on the host: when given, this entry reads T floats back and WAITS for `stream` (the one
 * exception to the rule at the top). */
#define QBOLD_FISHER_OUT 15
int qbold_fisher_information(const qbold_ctx* ctx, const float* theta, const float* sigma, int64_t sigma_rows,
                             const float* weights /* nullable */, const float* prior /* nullable */,
                             const float* mask /* nullable */, float* out, int64_t N, void* stream);

/* Scores of B designs of the tau protocol at once (this package's addition): a design is a row of per-tau weights w_b
 * on the context's tau grid, as above.  For every design the masked sums over the voxels of
 *      0    log det A_b, A_b = I(theta; w_b) + Lambda: summed over draws theta of a prior this is the Bayesian
 *           D-criterion E_theta log det(I + Lambda) (Chaloner & Verdinelli 1995)
 *      1-3  the variances of OEF, DBV and R2' from Sigma_b = A_b^-1 by the delta method (the squares of
 *           qbold_fisher_information's columns 9-11)
 *      4    sum of the mask weights
 *   scores: DEVICE double [B][QBOLD_DESIGN_OUT] = sum over voxels with m > 0 of m times the value (column 4: of m).
 *   per_voxel [B][N][4] or NULL (16-byte aligned): the four values per design and voxel, unweighted; NaN where
 *     mask <= 0 (or NaN).  A voxel's values are qbold_fisher_information's arithmetic to the bit (column 13; the
 *     variances before their square root).
 *   weights [B][T]: finite and >= 0 (NOT checked here: the buffer is the caller's on the device; a negative weight can
 *     make A indefinite and a NaN weight makes that design's scores NaN).  prior [N][5] is REQUIRED: A is then positive
 *     definite whatever the design, no design or voxel is dropped and no threshold decides anything.  A theta outside
 *     the transforms' open ranges makes its values, and every sum it enters, NaN.
 *   workspace: qbold_design_workspace_bytes(ctx, N, B) bytes, 8-byte aligned, not kept between calls; a caller with
 *     less memory scores the designs in several calls (a design's sums do not depend on its batch).
 *   Sums: partials belong to fixed 256-voxel tiles (four 64-voxel wave tiles, each added in voxel order, in double)
 *   and are added in tile order: the same bits run to run, at any launch grid, in any slot of any batch of designs.
 *   theta, sigma, sigma_rows, mask, the supported configurations and QBOLD_ERR_UNSUPPORTED as above.
 * QBOLD_ERR_INVALID for N < 0, B < 0, a NULL required buffer (scores, workspace when B > 0; theta, sigma, weights,
 * prior when N > 0 and B > 0), sigma_rows not in {1, N}, a misaligned workspace or per_voxel.  N = 0 returns zero sums,
 * B = 0 writes nothing. */
#define QBOLD_DESIGN_OUT 5
int64_t qbold_design_workspace_bytes(const qbold_ctx* ctx, int64_t N, int64_t B);
int qbold_design_scores(const qbold_ctx* ctx, const float* theta, const float* sigma, int64_t sigma_rows,
                        const float* weights, const float* prior, const float* mask /* nullable */, double* scores,
                        float* per_voxel /* nullable */, void* workspace, int64_t N, int64_t B, void* stream);

/* Posterior predictive checks of the fine-tuning model per voxel (this package's addition; the reference has no
 * counterpart): Gelman, Meng & Stern 1996 for the p-value, Watanabe 2010 / Vehtari, Gelman & Gabry 2017 for lppd and
 * WAIC.  theta_l, l = 0 .. L-1: the reparameterised draws of q (heads [N][5], the use_mvg = True family), from explicit
 * normals z [N][L][2] or, z NULL, draw l of qbold_normals(seed, 8, voxel0 + i, L) for voxel i (Philox stream 8).
 * Everything lives in the likelihood's own space, the one qbold_elbo_fwd scores: y_t the data normalised by the
 * spin-echo image (the mean of three with multi-image normalisation) + 1e-3, logged when predict_log; yh_{l,t} draw l's
 * prediction normalised the same way; r_{l,t} = (y_t - yh_{l,t}) / sigma_t; log p(y_t | theta_l) the per-tau term of
 * the NLL (Gaussian or Student-t).  No prior is involved.
 *   out [N][QBOLD_PPC_OUT]:
 *     0 ppp       = mean_l Q_{chi2_T}(D_l), D_l = sum_t r_{l,t}^2: the posterior predictive p-value of the chi2
 *                   discrepancy, Rao-Blackwellised (under the Gaussian likelihood D(y_rep, theta) ~ chi2_T exactly, so
 *                   no replicate noise is drawn); Q by its finite series.  NaN under Student-t.
 *     1 dbar      = mean_l D_l
 *     2 lppd      = sum_t log mean_l p(y_t | theta_l)   (streaming log-sum-exp per tau, relative to a running max)
 *     3 p_waic    = sum_t var_l log p(y_t | theta_l)    (denominator L - 1, from sums shifted by draw 0's value)
 *     4 elpd_waic = lppd - p_waic
 *     5 max_abs_z = max_t |z_t|
 *   curves [N][T][3] or NULL: (mu_t, sd_t, z_t) with mu_t = mean_l yh_{l,t}, sd_t = sqrt(var_l yh_{l,t} + v sigma_t^2)
 *     (v = 1 for the Gaussian, df / (df - 2) for Student-t, +inf for df <= 2), z_t = (y_t - mu_t) / sd_t: the fitted
 *     curve with its predictive band.
 *   Rows with mask <= 0 (or NaN) are NaN in out and curves and add nothing to the sums; mask NULL evaluates every voxel.
 *   sums: DEVICE double[4] = (sum m elpd_waic, sum m p_waic, sum m ppp, sum m) over the voxels with m > 0, overwritten
 *     (fixed-order reductions, no atomics: a voxel's outputs are the same bits at any batch position).
 *   workspace: qbold_elbo_workspace_bytes() bytes; x, mask, sigma (exponentiated), stream as qbold_elbo_fwd.
 * The observed r at the spin-echo image is ~0 by construction (the data are normalised by it), while chi2_T counts a
 * degree of freedom there: ppp is skewed upward on well-specified voxels and flags fewer, never more (at T = 11,
 * sigma = 0.01, q at the true parameters: 3.5 % below 0.05, 0.64 % below 0.01; MEASUREMENTS.md section 12).
 * Configurations qbold_log_evidence_fwd accepts; QBOLD_ERR_UNSUPPORTED otherwise.  QBOLD_ERR_INVALID for L < 2,
 * L > 2^30 or a NULL out / sums / workspace. */
#define QBOLD_PPC_OUT 6
int qbold_posterior_predictive(const qbold_ctx* ctx, const float* x, const float* mask, const float* q,
                               const float* sigma, const float* z, int L, uint64_t seed, int64_t voxel0,
                               float* out, float* curves, double* sums, void* workspace, int64_t N, void* stream);

/* Pareto-smoothed importance-sampling leave-one-out cross-validation per voxel and per tau image (this package's
 * addition; Vehtari, Gelman & Gabry 2017; with draws from a variational posterior Yao et al. 2018, Magnusson et al.
 * 2019).  For a voxel with heads q, prior, exponentiated sigma and K draws theta_k ~ q -- the draws of
 * qbold_log_evidence_draws: explicit z [N][K][2], or the Philox stream 6 keyed (seed, voxel0 + i), draw k here is draw
 * k there --
 *   log w_k   = qbold_log_evidence_draws' value, -nll - (log q - log p) on the draw
 *   ll_{t,k}  = log p(y_t | theta_k), qbold_posterior_predictive's per-tau term (Gaussian or Student-t, in the
 *               likelihood's own normalised or logged space); sum_t ll_{t,k} = -nll_k
 *   row t < T : rho_{t,k} = log w_k - ll_{t,k}, the log-ratio of the posterior without image t;  row T: log w_k.
 * Every row goes through qbold_psis as that entry defines it (tail rule, ties, the k^ = +inf cases, NaN rows): row t
 * gives the normalised smoothed weights w~^(t), row T gives w~.  With m_t = max_k ll_{t,k}
 *   elpd_t = m_t + log sum_k w~^(t)_k exp(ll_{t,k} - m_t),     lppd_t = m_t + log sum_k w~_k exp(ll_{t,k} - m_t)
 *   out [N][QBOLD_LOO_OUT]:
 *     0 elpd_loo  = sum_t elpd_t
 *     1 p_loo     = lppd - elpd_loo
 *     2 lppd      = sum_t lppd_t
 *     3 khat_max  = max_t k^_t (+inf beats every finite value; a NaN k^, from a NaN row, beats all)
 *     4 the lowest tau index attaining it, as a float
 *     5 khat_full = row T's k^
 *   pointwise [N][T][3] or NULL: (elpd_t, k^_t, lppd_t)
 *   log_ratio [N][T + 1][K] or NULL: the rows above;  loglik [N][T][K] or NULL: ll.  When given, they are where the rows
 *     are written: the caller sees exactly what the PSIS stage read.
 *   Voxels with mask <= 0 (or NaN) are not read; their outputs and rows are NaN and they add nothing to the sums; mask
 *     NULL = ones.
 *   sums: DEVICE double[4] = (sum m elpd_loo, sum m p_loo, sum m [khat_max > 0.7], sum m) over the voxels with m > 0,
 *     overwritten; accumulated in doubles in a fixed order, no atomics.
 *   workspace: qbold_loo_workspace_bytes(ctx, K, N) bytes, 16-byte aligned, caller-owned: per voxel
 *     4 K (3 T + 2) + 16 (T + 1) bytes (loglik, log_ratio, the smoothed weights of the T + 1 rows, qbold_psis' out), each
 *     of the four sections rounded up to 256 bytes, plus 32 bytes per block of the reduction (8 blocks per compute
 *     unit).  The size does not depend on whether log_ratio / loglik are given.
 * A high k^_t says that image t alone dominates the voxel's fit -- the signature of a corrupted tau image; elpd_loo
 * compares forward-model variants.  A voxel's outputs are the same bits at any batch position, under any sharding by
 * voxel0 and from run to run.  Configurations qbold_log_evidence_draws accepts (table mode; T = 11 / 24 with every
 * likelihood switch; every other T <= 64 with the Gaussian likelihood on linear data); QBOLD_ERR_UNSUPPORTED otherwise.
 * QBOLD_ERR_INVALID for K outside [QBOLD_PSIS_MIN_K, QBOLD_PSIS_MAX_K], N < 0, a NULL out / sums / workspace, or a NULL
 * input buffer when N > 0; N = 0 succeeds with zero sums.  qbold_loo_workspace_bytes returns QBOLD_ERR_INVALID for a
 * NULL context, K outside that range or N < 0.  x, q, prior, sigma, stream as qbold_log_evidence_fwd. */
#define QBOLD_LOO_OUT 6
int64_t qbold_loo_workspace_bytes(const qbold_ctx* ctx, int K, int64_t N);
int qbold_loo(const qbold_ctx* ctx, const float* x, const float* mask, const float* q, const float* prior,
              const float* sigma, const float* z, int K, uint64_t seed, int64_t voxel0, float* out, float* pointwise,
              float* log_ratio, float* loglik, double* sums, void* workspace, int64_t N, void* stream);

/* Posterior calibration against a KNOWN truth (this package's addition; simulation-based calibration, Talts et al. 2018;
 * Sailynoja et al. 2022): where the true (OEF, DBV) of a simulated voxel falls in the posterior q the encoder returned
 * for it.  Over many voxels every column below is Uniform(0, 1) exactly when the intervals of q cover as often as they
 * claim.  Nothing of the forward model enters: no table, no tau grid, so the entry runs on every context.
 *   theta_true [N][2]: the known (OEF, DBV).
 *   q [N][5]: raw heads of the use_mvg family, (mu_o, s_o, mu_d, s_d, c) = the transforms of model.py:288-294.
 *   mask [N] or NULL (= ones): voxels with mask <= 0 (or NaN) are not read; their six outputs are NaN.
 *   z: explicit normals [N][L][2] (exactly 2 L floats per voxel are read), or NULL for the Philox stream 6 keyed
 *     (seed, voxel0 + i): draw k is draw k of qbold_normals(seed, 6, voxel0, L), which is draw k of
 *     qbold_log_evidence_draws -- so a row of weights of that entry's draws lines up with the draws here.
 *   log_w [N][L] or NULL: log-weights of the same draws, normalised or not -- qbold_psis' `weights`, or the raw log_w of
 *     qbold_log_evidence_draws.  -inf is a zero weight; a NaN or +inf anywhere in a row, or no finite entry, makes
 *     columns 3 - 5 of that voxel NaN and leaves columns 0 - 2 as they are.
 * Per voxel: (a*, b*) = the truth's logits, logit(clamp((OEF - 0.04) / 0.8, 1e-6, 1 - 1e-6)) and the same with
 * (DBV - 0.001) / 0.2 (model.py:393-398; 1 - x is formed as (0.84 - OEF) / 0.8, which does not cancel at the upper
 * clamp);  draw k: a_k = mu_o + z0 e^{s_o}, b_k = mu_d + z0 c + z1 e^{s_d} (model.py:25-31), (OEF_k, DBV_k) =
 * forward_transform(a_k, b_k) (model.py:299-305).
 *   out [N][QBOLD_CAL_OUT]:
 *     0 pit_oef = Phi((a* - mu_o) e^{-s_o})
 *     1 pit_dbv = Phi((b* - mu_d) / sqrt(c^2 + e^{2 s_d}))
 *     2 hpd     = -expm1(-d^2 / 2), d^2 = || L_q^-1 (u* - mu) ||^2: the level of the smallest highest-density ellipse of
 *                 q that contains the truth
 *     3 rank fraction of OEF: a_k against a* (the sigmoid is monotone)
 *     4 rank fraction of DBV: b_k against b*
 *     5 rank fraction of R2': OEF_k DBV_k against OEF* DBV* of the given truth (dw_coef > 0 cancels)
 *   The rank fraction of a statistic d, without log_w: float(2 #{d_k < d*} + #{d_k == d*}) / float(2 L) -- integer
 *   counts, one rounding; with log_w: sum_k w~_k ([d_k < d*] + [d_k == d*] / 2), w~ = exp(log_w - max) / sum exp(log_w -
 *   max), float32 sums in a fixed order.
 * Non-finite heads or truths propagate (a NaN one gives NaN, never rank 0); nothing is clamped but the unit-interval
 * value above.  No sums, no workspace, no atomics: a voxel's outputs are the same bits at any batch position, under any
 * sharding by voxel0 and from run to run.  QBOLD_ERR_INVALID for L < 1, L > QBOLD_CAL_MAX_L, N < 0, a NULL out, or a
 * NULL theta_true / q when N > 0; N = 0 succeeds. */
#define QBOLD_CAL_OUT 6
#define QBOLD_CAL_MAX_L (1 << 20)
int qbold_calibration(const qbold_ctx* ctx, const float* theta_true, const float* mask, const float* q,
                      const float* log_w, const float* z, int L, uint64_t seed, int64_t voxel0, float* out,
                      int64_t N, void* stream);

/* ---- gradients (training) ------------------------------------------------------------------- */
/* Adjoint of qbold_elbo_fwd with respect to the encoder's head outputs: what TensorFlow autodiff
 * yields through build_fine_tuner's sampling + fine_tune_loss_fn + kl_loss (model.py:239-286,
 * 527-568, 592-610; q is stop-gradient inside log q, model.py:596).
 *   log_sigma [N][T] (the sigma head BEFORE exp, model.py:211-214)
 *   g_q [N][5], g_log_sigma [N][T]:  m_v * d nll_v/d. + [m_v > 0] * d kl_v/d.   (NOT divided by
 *   sum(m): the caller scales the weight gradient once)
 *   nll_kl, sums, workspace: as qbold_elbo_fwd (same Philox stream -> same loss values).
 * Built for the full signal model in table mode.  T = 11 or 24: Gaussian or Student-t likelihood, linear or log
 * data, one- or three-image normalisation (the switches of qbold_loss_cfg).  Every other 1 <= T <= 64, with or
 * without a tau equal to 0: the configurations qbold_elbo_fwd runs there (Gaussian likelihood on linear data, one-
 * or three-image normalisation, any spin-echo index), same Philox words and the same fixed-order sums, so the
 * outputs are the same bits under any sharding by voxel0 and run to run; Student-t or log data at such a T return
 * QBOLD_ERR_UNSUPPORTED.  QBOLD_KSEL_ELBO_BWD_GENERIC runs T = 11 / 24 on that kernel too. */
int qbold_elbo_bwd(const qbold_ctx* ctx, const float* x, const float* mask, const float* q,
                   const float* prior, const float* log_sigma, int S, int K, uint64_t seed,
                   int64_t voxel0, float* g_q, float* g_log_sigma, float* nll_kl, double* sums,
                   void* workspace, int64_t N, void* stream);

/* Encoder training (TensorFlow autodiff through create_encoder, model.py:122-223, in the Keras fit
 * loops train.py:285-376 / :379-427).  `weights` is the canonical blob; `workspace` holds
 * qbold_train_workspace_floats(shape, N) floats (saved activations + scratch).
 *   stream_sel 1: pre-training stream (out_q = output 0, model.py:199), 2: fine-tuning stream
 *   (out_q = second_net, out_log_sigma = sigma head before exp, model.py:208-214). */
int64_t qbold_train_workspace_floats(const qbold_encoder_shape* shape, int64_t N);
int qbold_encoder_train_fwd(const qbold_ctx* ctx, const qbold_encoder_shape* shape, const float* weights,
                            const float* x, int stream_sel, float* workspace, float* out_q,
                            float* out_log_sigma, int64_t N, void* stream);
/* stream_sel = 2 of the call above in ONE launch for the shapes of the LDS-resident kernels (U <= 64, L <= 2,
 * T = 11 or 24, channel-wise gating, QBOLD_ENC_F32; 0 < N < 2^23): `packed` is the image of
 * qbold_encoder_pack; the workspace receives the same saved tensors, so qbold_encoder_train_bwd follows
 * unchanged.  save_all = 2 saves every tensor; 1 leaves out the two per block (skip, gate logits) and 0 the four
 * per block (also t, r) that qbold_encoder_train_bwd recomputes -- pass 2 - qbold_encoder_train_bwd_recomputes(ctx,
 * shape, N), or 2.  Products are the float32-grade split-f16 ones of qbold_encoder_fwd (operand range above: heads
 * come out NaN beyond it), not the exact-f32 GEMMs of qbold_encoder_train_fwd. */
int qbold_encoder_train_fwd_fused(const qbold_ctx* ctx, const qbold_encoder_shape* shape, const float* packed,
                                  const float* x, int save_all, float* workspace, float* out_q,
                                  float* out_log_sigma, int64_t N, void* stream);
/* What qbold_encoder_train_bwd (stream 2, voxel batch) recomputes from each gated block's input instead of
 * reading it: 0 nothing (the layer-wise backward), 1 skip and the gate logits (one launch per block for the data
 * side), 2 also t and r (the same launch accumulates the block's weight gradients). */
int qbold_encoder_train_bwd_recomputes(const qbold_ctx* ctx, const qbold_encoder_shape* shape, int64_t N);
/* The same on image crops: geom->B*X*Y*Z voxels, stream 2 with its 3x3x1 'same' convolutions
 * (shape->spatial_taps must be 9).  geom = NULL is the voxel-batch call above.  For U % 4 == 0 the convolutions run on
 * split-f16 operands: an input activation beyond 65504 (or a NaN one) makes the output row of every voxel whose 3x3
 * neighbourhood reads it NaN, and the relus of the later layers keep the NaN, so the affected voxels' q and log sigma
 * come out NaN -- never a clamped number; other voxels and other batch elements are unaffected.  (A weight beyond
 * 65504 has no such guard here: keep the convolution kernels inside f16's range.) */
int qbold_encoder_spatial_fwd(const qbold_ctx* ctx, const qbold_encoder_shape* shape, const float* weights,
                              const float* x, const qbold_geometry* geom, float* workspace, float* out_q,
                              float* out_log_sigma, void* stream);
int qbold_encoder_spatial_bwd(const qbold_ctx* ctx, const qbold_encoder_shape* shape, const float* weights,
                              const qbold_geometry* geom, float* workspace, const float* g_q,
                              const float* g_log_sigma, const double* sums, float* grad, void* stream);
/* smoothness_loss (model.py:726-754) on crops: q [V][5], mask [V].  tv_sum: DEVICE double[1] =
 * sum |dx| + sum |dy| (divide by sum(mask)); if g_q is not NULL, weight * d tv_sum / d q is ADDED to
 * g_q [V][5] (unnormalised, like qbold_elbo_bwd's output). */
int qbold_smoothness(const qbold_ctx* ctx, const float* q, const float* mask, const qbold_geometry* geom,
                     float weight, float* g_q, double* tv_sum, void* stream);
/* g_q [N][5], g_log_sigma [N][T] (stream 2; may be NULL): gradients of the loss with respect to
 * the head outputs.  sums: DEVICE double[3] whose [2] is sum(mask) -- the head gradients are
 * divided by it (NULL: already normalised).  grad: canonical layout, overwritten.
 * When qbold_encoder_train_bwd_recomputes(...) is 2 the backward RECOMPUTES each block (skip, t, r, gate logits) with
 * the split-f16 products of qbold_encoder_train_fwd_fused and takes its relu masks from that recomputation: it is the
 * adjoint of THAT forward.  After the exact-f32 layer-wise qbold_encoder_train_fwd the masks can differ for
 * activations within ~1e-6 of zero (where the relu's derivative is a convention anyway); callers that need the adjoint
 * of the layer-wise forward bit for bit select QBOLD_KSEL_LAYERWISE_BWD.
 * Operand range of the layer-wise backward (crops, and voxel batches under QBOLD_KSEL_LAYERWISE_BWD): the 3x3x1
 * backward-data products and the weight gradients run on split-f16 operands.  Deltas are NOT bound by f16's range:
 * the backward-data products keep a running power-of-two scale per voxel and the weight-gradient kernels one per wave,
 * each following the largest |delta| seen (accumulators rescaled, exact; a scale starts at 2^126, so deltas from
 * about 2^-112 up to 1e30 keep float32-grade precision), with or without `sums` -- tested against a float64 VJP for
 * head gradients 2^k g, |k| <= 60, and per-voxel magnitudes from 1e-9 to 1e6 in one batch.  Activations are taken as
 * they are: the forwards' limit applies (an activation beyond 65504 makes the affected heads NaN, never a clamped
 * number: qbold_encoder_spatial_fwd above), and an activation below 2^-14 in magnitude
 * keeps an absolute 2^-25 in the weight gradients.  QBOLD_KSEL_DW_BF16_PIECES (three bfloat16 pieces per operand, no
 * range at all) and QBOLD_KSEL_DW_EXACT_F32 select the other forms. */
int qbold_encoder_train_bwd(const qbold_ctx* ctx, const qbold_encoder_shape* shape, const float* weights,
                            int stream_sel, float* workspace, const float* g_q, const float* g_log_sigma,
                            const double* sums, float* grad, int64_t N, void* stream);
/* synthetic_data_loss (model.py:449-514; use_mvg, no r2p term) per voxel and its gradient: y_true
 * rows of ld_y floats (OEF, DBV first), q [N][5] -> loss_v [N] (may be NULL), g_q [N][5] =
 * scale * d loss_v / d q.  inv_gamma_alpha * inv_gamma_beta > 0 adds the inverse-gamma prior on the
 * two marginal variances (:492-507: - log IG(exp(s_o)^2) - log IG(exp(s_d)^2 + q[4]^2)). */
int qbold_synth_loss_bwd(const qbold_ctx* ctx, const float* y_true, int ld_y, const float* q, float* g_q,
                         float* loss_v, float scale, double inv_gamma_alpha, double inv_gamma_beta,
                         int64_t N, void* stream);
/* The learned inverse-gamma hyper-prior of synthetic_data_loss (infer_inv_gamma with the diagonal family,
 * model.py:201-205, 454-455, 493-507): ig_host = HOST double[4] (alpha_oef, beta_oef, alpha_dbv, beta_dbv), the
 * exp-activated VariableLayer values.  Per voxel - log IG(exp(2 s_o); a_o, b_o) - log IG(exp(2 s_d); a_d, b_d) is
 * ADDED to loss_v [N], scale * its gradient to g_q [N][5] (columns 1, 3); stats: DEVICE double[4] = sum log v_o,
 * sum 1 / v_o, sum log v_d, sum 1 / v_d -- what the gradient with respect to the four hyper-parameters needs
 * (d / d a = digamma(a) - log b + mean log v, d / d b = - a / b + mean 1 / v).  Any of g_q / loss_v / stats may be
 * NULL.  Call after qbold_synth_loss_bwd. */
int qbold_hyper_prior_bwd(const qbold_ctx* ctx, const float* q, const double* ig_host, float scale, float* g_q,
                          float* loss_v, double* stats, int64_t N, void* stream);
/* The R2' term of synthetic_data_loss (use_r2p_loss, model.py:475-490): n_samples (reference: 10)
 * reparameterised draws of (OEF, DBV) from q [N][5], r = dw(OEF) DBV (calculate_r2p :524-525), a normal
 * fitted by the draws' mean and biased std, gaussian_nll (:403-404) of the true R2' y_true[:, 2] under it.
 * ADDS the per-voxel value to loss_v [N] and scale * d / d q to g_q [N][5] (either may be NULL): call it
 * after qbold_synth_loss_bwd.  z = explicit normals [N][n_samples][2] or NULL for the in-kernel Philox
 * stream (seed, global voxel = voxel0 + i). */
int qbold_r2p_loss_bwd(const qbold_ctx* ctx, const float* y_true, int ld_y, const float* q, const float* z,
                       int n_samples, uint64_t seed, int64_t voxel0, float scale, float* g_q, float* loss_v,
                       int64_t N, void* stream);
/* One tfa.optimizers.AdamW step (train.py:308-310, 382-385) on a flat blob: decoupled decay
 * var -= weight_decay * var, Keras Adam moments and bias correction at step t >= 1, eps 1e-7. */
int qbold_adamw_step(const qbold_ctx* ctx, float* params, const float* grads, float* m, float* v,
                     int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay,
                     int64_t t, void* stream);

#ifdef __cplusplus
}
#endif
#endif
