// vi_fwd_kernels.inc -- the two fused kernel templates of vi_kernels.hip (its header comment describes them), which
// includes this text twice.
//   QB_VI_FOLD 0: vi_fwd_kernel, vi_fwd_kernel_vox -- the classic weight image (qbold_vi_fwd).
//   QB_VI_FOLD 1: vi_fwd_kernel_fold, vi_fwd_kernel_vox_fold -- one more argument, gate_fold: the folded gate ops of
//     qbold_encoder_pack_gatefold.  The LDS image is the classic one with each block's gate slot filled from gate_fold
//     and the flag slot holding the larger of the two flags (copy_to_lds_fold, encoder_core.h: same footprint, the one
//     barrier), and the blocks take their gate logits from relu(t)'s fragments (block_stream2<.., FOLD>).  Instantiated
//     for the per-tau-table fast path only (GT), the path both layouts of the sampling phase share.
// The four-lane kernels run normalise, dense_first and gather_head; the one-lane-per-voxel kernels run first_operand,
// keep_head_tile and transpose_heads (encoder_core.h) to the same bits, and are tested against the four-lane ones.
#if QB_VI_FOLD
#define QB_VI_KERNEL(name) name##_fold
#define QB_VI_GATE_FOLD_ARG const float* __restrict__ gate_fold,
#define QB_VI_COPY_IMAGE(BLK) qb::copy_to_lds_fold<BLK, e.flag, e.blk0, NL>(lds_w, packed, gate_fold, e.total / 4)
#else
#define QB_VI_KERNEL(name) name
#define QB_VI_GATE_FOLD_ARG
#define QB_VI_COPY_IMAGE(BLK) qb::copy_to_lds<BLK>(lds_w, packed, e.total / 4)
#endif

// GT: the sampling fast path reads the per-tau OEF-indexed table (GtLds) instead of the x-indexed one (FwdLds);
// requires FAST and a compile-time spin-echo index.
// MIR: the protocol mirrors about the spin echo (qbold_ctx::grid_mirrors): mirrored tau pairs are evaluated once and
// scored as one merged data point (elbo_core.h, prepare_lik); GT implies it.
template <int T, int NL, int SE, bool FAST, bool LITERAL, bool BF, bool GT = false, bool MIR = false, int BLK = kBlock>
__global__ __launch_bounds__(BLK) void QB_VI_KERNEL(vi_fwd_kernel)(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ packed, QB_VI_GATE_FOLD_ARG
    const float* __restrict__ x, const float* __restrict__ mask, const float* __restrict__ prior,
    int S, int K, uint64_t seed, int64_t voxel0, float* __restrict__ q_out,
    float2* __restrict__ nll_kl, double* __restrict__ partials, int64_t N) {
    // compile-time weight-image layout: every LDS offset below folds into an instruction immediate
    constexpr EncLayout e = qb::make_enc_layout(T, 64, NL);
    // the sampling phase's table: per-tau OEF-indexed rows (GtLds) on the fast path with a compile-time spin-echo
    // index, the x-indexed table + literal nodes (FwdLds) otherwise; g_tab points at the matching device table
    static_assert(!GT || (FAST && SE >= 0 && qb::gtab_segs(T) > 0), "GT needs the fast path with a compile-time spin echo");
    static_assert(!MIR || (FAST && SE >= 0), "merged mirror pairs: fast path with a compile-time spin echo");
    static_assert(!QB_VI_FOLD || GT, "the folded gate ops: built for the per-tau-table fast path");
    constexpr bool kMir = GT || MIR;
    using Lds = typename ViLds<T, SE, GT>::type;
    extern __shared__ __align__(16) unsigned char smem[];
    float* lds_w = reinterpret_cast<float*>(smem);
    Lds* L = reinterpret_cast<Lds*>(smem + sizeof(float) * e.total);
    double* red = reinterpret_cast<double*>(smem + sizeof(float) * e.total + sizeof(Lds));
    constexpr int kWaves = BLK / 64;
    QB_VI_COPY_IMAGE(BLK);
    if constexpr (qb::IsGtLds<Lds>::value) {
        qb::gt_lds_fill(L, g_tab, c);
    } else {
        qb::fwd_lds_fill(L, g_tab, true);
        if (threadIdx.x < QB_MAX_T) L->blood_B[threadIdx.x] = c.blood_B[threadIdx.x];
    }
    __syncthreads();

    constexpr int HT = (5 + T + 15) / 16;
    const int lane0 = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float s_nll = 0.0f, s_kl = 0.0f, s_m = 0.0f;
    const int64_t ntile = (N + 15) / 16;
    for (int64_t tile = (int64_t)blockIdx.x * kWaves + wave; tile < ntile;
         tile += (int64_t)gridDim.x * kWaves) {
        // The lane index is made opaque once per tile: everything derived from it (the encoder's LDS fragment
        // addresses, the voxel's row pointers) is then recomputed per tile -- a handful of vector instructions --
        // instead of being hoisted out of the tile loop as 20-70 loop-invariant registers that the sampling phase
        // (which needs none of them) has to spill and reload around itself.
        int lane = lane0;
        asm volatile("" : "+v"(lane));
        const int g = lane >> 4, i = lane & 15;
        const int64_t v = tile * 16 + i;
        const int64_t vc = v < N ? v : N - 1;
        float o[5 + T];
        // largest activation this lane split (operand range guard, encoder_core.h); starts from the image's flag
        // slot: 0, or the largest weight the pack kernel could not split
        float amax = lds_w[e.flag];
        {
            __builtin_amdgcn_s_setprio(QB_PRIO_TILE_START);
            float xv[T], nv[T];
#pragma unroll
            for (int t = 0; t < T; ++t) xv[t] = x[vc * T + t];
            qb::normalise<T, SE>(c, xv, nv);
            __builtin_amdgcn_s_setprio(2);
            f32x4 b[4];
            qb::dense_first<T, BF>(lds_w + e.first_A, lds_w + e.first_b, nv, b, lane);
            if (!QB_ABLATE(c, 1) && qb_phase_fence()) {
                // block 0 reads dense_first's output, which its relu4 left non-negative
                qb::block_stream2<BF, true, QB_VI_FOLD>(lds_w + e.blk0, b, lane, &amax);
#pragma unroll
                for (int l = 1; l < NL; ++l) qb::block_stream2<BF, false, QB_VI_FOLD>(lds_w + e.blk0 + l * e.blk_stride, b, lane, &amax);
            }
            f32x4 hd[HT];
            qb::dense_head<HT, BF>(lds_w + e.head_A, lds_w + e.head_b, b, hd, lane, &amax);
            qb::gather_head<5 + T, HT>(hd, o);
            __builtin_amdgcn_s_setprio(0);
        }
        if (v < N && !QB_ABLATE(c, 2) && qb_phase_fence()) {
            // x is read again (an L1/L2 hit) rather than held in 11 VGPRs across the encoder; the
            // empty asm keeps the compiler from merging the two reads
            const float* xr = x + v * T;
            asm volatile("" : "+v"(xr));
            float xv[T], sv[T], qv[5];
#pragma unroll
            for (int t = 0; t < T; ++t) xv[t] = xr[t];
#pragma unroll
            for (int k = 0; k < 5; ++k) qv[k] = o[k];
#pragma unroll
            for (int t = 0; t < T; ++t) sv[t] = o[5 + t];  // log sigma; sigma = exp(.), model.py:214
            // the mask: the likelihood needs it only on log data (model.py:548); the sums read it again after the draws
            // (a second load through an opaque pointer) instead of carrying it through the loops
            qb::VoxelLik<T> lik;
            qb::prepare_lik<T, SE, true, (FAST && SE >= 0), FAST, kMir>(c, xv, sv, FAST ? 1.0f : (mask ? mask[v] : 1.0f), lik);
            const qb::LogitMvn qm = qb::make_mvn(qv);
            // posterior parameters leave before the draws (lane group 1), so that they do not live through them
            if (g == 1 && q_out) {
#pragma unroll
                for (int k = 0; k < 5; ++k) q_out[v * 5 + k] = qv[k];
            }
            // an activation beyond the f16 operand range: this voxel's terms become NaN (never a silent clamp) -- through
            // the per-draw constant, which every draw's NLL adds
            if (!BF && qb::split_overflowed(amax)) lik.log_s_sum = __builtin_nanf("");
            float nll_part, kl_part;
            qb::voxel_mc_sums<T, SE, FAST, LITERAL, kMir>(L, c, lik, qm, prior + v * 5, S, K, nullptr, nullptr, seed,
                                                    (uint64_t)(voxel0 + v), g, nll_part, kl_part);
            const float nll = qb::voxel_sum(nll_part) / (float)S;
            const float kl = K > 0 ? qb::voxel_sum(kl_part) / (float)K : 0.0f;
            if (g == 0) {
                const float* mp = mask;
                asm volatile("" : "+v"(mp));
                const float m = mp ? mp[v] : 1.0f;
                if (nll_kl) nll_kl[v] = make_float2(nll, kl);
                s_nll += nll * m;              // model.py:564
                s_kl += m > 0.0f ? kl : 0.0f;  // model.py:661
                s_m += m;
            }
        }
    }
    qb::block_partials(red, s_nll, s_kl, s_m, partials);
}

// The same tile loop with one lane per voxel through the sampling phase (header comment).  Per 64-voxel tile the encoder
// phase runs four times, on the 16-voxel sub-tiles s = 0 .. 3, with vi_fwd_kernel's arithmetic: the first layer's
// operand comes from the nine signals the lane feeds it (first_operand), and the head accumulators of sub-tile s are
// kept in register slot s; one transpose of (slot, lane group) behind the loop (transpose_heads) then leaves lane
// (g, i) with the heads of voxel 64 tile + 16 g + i = 64 tile + lane.  The sampling phase then runs once,
// voxel_mc_sums<.., 1> walking the four draw shares in vi_fwd_kernel's order (elbo_core.h): every per-voxel output is
// the same bits whichever kernel took the voxel.  Built for the per-tau-table fast path only (GT in vi_fwd_kernel's
// terms).  add_blocks: workgroups below it add their partial sums to what the slot holds (the four-lane launch over
// the batch's remainder wrote it earlier on the stream) instead of overwriting it.
template <int T, int NL, int SE, bool BF, int BLK = kBlock>
__global__ __launch_bounds__(BLK) void QB_VI_KERNEL(vi_fwd_kernel_vox)(
    QbDev c, const float4* __restrict__ g_tab, const float* __restrict__ packed, QB_VI_GATE_FOLD_ARG
    const float* __restrict__ x, const float* __restrict__ mask, const float* __restrict__ prior,
    int S, int K, uint64_t seed, int64_t voxel0, float* __restrict__ q_out,
    float2* __restrict__ nll_kl, double* __restrict__ partials, int64_t N, int add_blocks) {
    constexpr EncLayout e = qb::make_enc_layout(T, 64, NL);
    static_assert(SE >= 0 && qb::gtab_segs(T) > 0, "built for the per-tau table with a compile-time spin echo");
    using Lds = qb::GtLds<T, SE>;
    extern __shared__ __align__(16) unsigned char smem[];
    float* lds_w = reinterpret_cast<float*>(smem);
    Lds* L = reinterpret_cast<Lds*>(smem + sizeof(float) * e.total);
    double* red = reinterpret_cast<double*>(smem + sizeof(float) * e.total + sizeof(Lds));
    constexpr int kWaves = BLK / 64;
    QB_VI_COPY_IMAGE(BLK);
    qb::gt_lds_fill(L, g_tab, c);
    __syncthreads();

    constexpr int HT = (5 + T + 15) / 16;
    // The head hand-over keeps the accumulators in slots and transposes once per tile (keep_head_tile, transpose_heads)
    // everywhere but on the classic split-f16 image at two head tiles: there 32 slot registers, where o[] holds 29, on
    // top of the classic block's peak do not fit the 168 registers of the 768-thread workgroup (12 bytes of scratch
    // at T = 24, L = 2), and that kernel keeps gather_head and a select per row.
    constexpr bool kSlots = HT == 1 || BF || QB_VI_FOLD;
    // The likelihood draws read their wave-uniform operands from vector registers (voxel_mc_sums<.., DREGS>, elbo_core.h:
    // 18 registers at T = 11, 26 at T = 24) in every instance that keeps its register budget without scratch with them.
    // Eleven of the twelve do (MEASUREMENTS.md 34 lists them); the classic split-f16 image at T = 11, L = 2 takes 12
    // bytes of scratch and keeps SGPR and literal operands.
    constexpr bool kDrawRegs = BF || QB_VI_FOLD || !(T == 11 && NL == 2);
    // Nothing per lane lives across the tile loop but the thread index: the encoder phases hold the finished sub-tiles'
    // head rows on top of their own peak, and every further loop-carried vector register would be spilled around them.
    // The wave index is read as a scalar (the tile counter and its bounds stay on the scalar unit), and the three
    // running sums are wave-uniform, added up across the wave once per tile.
    const int lane0 = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float s_nll = 0.0f, s_kl = 0.0f, s_m = 0.0f;
    auto uniform = [](float v) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v))); };
    const int64_t ntile = (N + 63) / 64;
    for (int64_t tile = (int64_t)blockIdx.x * kWaves + wave; tile < ntile;
         tile += (int64_t)gridDim.x * kWaves) {
        // slot s: the head accumulators of sub-tile s, each written in its own trip of the loop below (the empty asm
        // defines it without an instruction); o: the head rows of this lane's voxel
        float hs[4][HT][4], o[5 + T];
#pragma unroll
        for (int k = 0; k < 16 * HT; ++k) asm volatile("" : "=v"(hs[k / (4 * HT)][(k / 4) % HT][k % 4]));
        if constexpr (!kSlots) {
#pragma unroll
            for (int k = 0; k < 5 + T; ++k) o[k] = 0.0f;
        }
        // operand range guard: bit l = the voxel of lane l had an activation beyond the split's range in any of the four
        // lane groups that encoded it (a wave-uniform mask: it costs no vector register across the encoder phases)
        unsigned long long hot = 0;
#pragma unroll 1
        for (int s = 0; s < 4; ++s) {
            // the lane index is made opaque per sub-tile, as vi_fwd_kernel makes it per tile: what derives from it (the
            // encoder's LDS fragment addresses) is formed again for each sub-tile instead of living through all four
            int lane = lane0;
            asm volatile("" : "+v"(lane));
            const int i = lane & 15;
            const int64_t ve = tile * 64 + 16 * s + i;
            const int64_t vc = ve < N ? ve : N - 1;
            float amax = lds_w[e.flag];
            __builtin_amdgcn_s_setprio(QB_PRIO_TILE_START);
            // the first layer's operand from the nine signals this lane feeds it (first_operand, encoder_core.h)
            qb::f16x8 fhi, flo;
            qb::first_operand<T, SE, BF>(x + vc * T, lane, fhi, flo);
            __builtin_amdgcn_s_setprio(2);
            f32x4 b[4];
            qb::dense_first_frag<BF>(lds_w + e.first_A, lds_w + e.first_b, fhi, flo, b, lane);
            if (!QB_ABLATE(c, 1) && qb_phase_fence()) {
                qb::block_stream2<BF, true, QB_VI_FOLD>(lds_w + e.blk0, b, lane, &amax);
#pragma unroll
                for (int l = 1; l < NL; ++l) qb::block_stream2<BF, false, QB_VI_FOLD>(lds_w + e.blk0 + l * e.blk_stride, b, lane, &amax);
            }
            f32x4 hd[HT];
            qb::dense_head<HT, BF>(lds_w + e.head_A, lds_w + e.head_b, b, hd, lane, &amax);
            if constexpr (kSlots) {
                // the head accumulators go to slot s as they are (s is wave-uniform: a scalar branch around four moves)
#pragma unroll
                for (int m = 0; m < HT; ++m) qb::keep_head_tile<BF>(s, hs[0][m], hs[1][m], hs[2][m], hs[3][m], hd[m]);
            } else {
                // gather_head hands every group a copy; the lanes of group s keep theirs, a select per row
                float os[5 + T];
                qb::gather_head<5 + T, HT>(hd, os);
#pragma unroll
                for (int k = 0; k < 5 + T; ++k) o[k] = (lane >> 4) == s ? os[k] : o[k];
            }
            if constexpr (!BF) {
                unsigned long long over = __ballot(qb::split_overflowed(amax));
                over |= over >> 32;
                over |= over >> 16;
                hot |= (over & 0xffffull) << (16 * s);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        if constexpr (kSlots) {
            // one transpose per tile: lane (g, i) takes the head rows of voxel 64 tile + 16 g + i
            qb::transpose_heads<HT>(hs);
#pragma unroll
            for (int k = 0; k < 5 + T; ++k) o[k] = qb::head_row<HT>(hs, k);
        }
        int lane = lane0;
        asm volatile("" : "+v"(lane));
        const int64_t v = tile * 64 + lane;
        float t_nll = 0.0f, t_kl = 0.0f, t_m = 0.0f;   // this lane's terms of the three masked sums
        if (v < N && !QB_ABLATE(c, 2) && qb_phase_fence()) {
            const float* xr = x + v * T;   // read again rather than held across the encoder phases (vi_fwd_kernel)
            asm volatile("" : "+v"(xr));
            float xv[T], sv[T], qv[5];
#pragma unroll
            for (int t = 0; t < T; ++t) xv[t] = xr[t];
#pragma unroll
            for (int k = 0; k < 5; ++k) qv[k] = o[k];
#pragma unroll
            for (int t = 0; t < T; ++t) sv[t] = o[5 + t];
            qb::VoxelLik<T> lik;
            qb::prepare_lik<T, SE, true, true, true, true>(c, xv, sv, 1.0f, lik);
            const qb::LogitMvn qm = qb::make_mvn(qv);
            if (q_out) {
#pragma unroll
                for (int k = 0; k < 5; ++k) q_out[v * 5 + k] = qv[k];
            }
            if (!BF && ((hot >> lane) & 1)) lik.log_s_sum = __builtin_nanf("");
            float nll_sum, kl_sum;
            qb::voxel_mc_sums<T, SE, true, false, true, 1, kDrawRegs>(L, c, lik, qm, prior + v * 5, S, K, nullptr, nullptr,
                                                                      seed, (uint64_t)(voxel0 + v), 0, nll_sum, kl_sum);
            int Sd = S, Kd = K;   // opaque: (float)S and (float)K are formed here, not carried through the tile loop
            asm volatile("" : "+s"(Sd), "+s"(Kd));
            const float nll = nll_sum / (float)Sd;
            const float kl = Kd > 0 ? kl_sum / (float)Kd : 0.0f;
            // the voxel index is formed again for the outputs rather than carried through the draw loops
            int lane_out = lane0;
            asm volatile("" : "+v"(lane_out));
            const int64_t vo = tile * 64 + lane_out;
            const float* mp = mask;
            asm volatile("" : "+v"(mp));
            const float m = mp ? mp[vo] : 1.0f;
            if (nll_kl) nll_kl[vo] = make_float2(nll, kl);
            t_nll = nll * m;              // model.py:564
            t_kl = m > 0.0f ? kl : 0.0f;  // model.py:661
            t_m = m;
        }
        s_nll = uniform(s_nll + qb::wave_sum(t_nll));
        s_kl = uniform(s_kl + qb::wave_sum(t_kl));
        s_m = uniform(s_m + qb::wave_sum(t_m));
    }
    const bool first = (threadIdx.x & 63) == 0;   // the wave's sums enter the block reduction once
    qb::block_partials(red, first ? s_nll : 0.0f, first ? s_kl : 0.0f, first ? s_m : 0.0f, partials,
                       (int)blockIdx.x < add_blocks);
}

#undef QB_VI_KERNEL
#undef QB_VI_GATE_FOLD_ARG
#undef QB_VI_COPY_IMAGE
