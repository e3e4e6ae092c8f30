"""Each fused form of the 64-wide exact-f32 training GEMM (train_kernels.hip, the kernels on the 16-voxel tile
skeleton) against the separate launches it replaced, which the selection bits of include/qbold_hip.h bring back:

    xw64_kernel (four instantiations)  vs  xw_kernel                            QBOLD_KSEL_GENERAL_GEMM       512
    xw64_gate_kernel                   vs  GEMM + gate_fwd_kernel               QBOLD_KSEL_SEPARATE_GATE     2048
    gate_bwd_wg_kernel                 vs  gate_bwd_kernel + GEMM               QBOLD_KSEL_SEPARATE_GATE     2048
    xw64_dual_kernel                   vs  masked GEMM + accumulating GEMM      QBOLD_KSEL_SEPARATE_BWD_DATA 4096
    xw64_fork_kernel                   vs  two GEMMs                            QBOLD_KSEL_SEPARATE_FORK     8192
    xw64_heads_kernel                  vs  one GEMM per head                    QBOLD_KSEL_PER_HEAD_FWD     32768

The same weights, batch and head gradients run forward and backward under a selection s0 and under s0 | bit; q, log
sigma and the flat gradient are compared.  Voxel batches take the layer-wise forward (TrainState.fused_forward =
False: the one-launch forward does not reach these kernels).

Pairs that run the same products in the same order (BITWISE) must agree bit for bit.  The others differ in the last
bits -- the dual kernel adds its second chain onto the masked accumulator where two launches add a finished product to
a stored value; the fused gate backward evaluates the gate with another sigmoid form -- so both sides are held to the
float64 VJP of _train_bwd_reference.py within its EPS (relu-site screen included) and to the float64 forward within
the 2e-5 of test_gpu_grad.py's layer-wise forward, and may differ from each other by no more than each differs from
the reference.  Which pairs are bitwise was decided by a run of this file before the kernels moved onto the shared
skeleton; the measured differences are in MEASUREMENTS.md ("Training GEMMs on one tile skeleton")."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _train_bwd_reference as ref  # noqa: E402
from test_gpu_train_bwd_reference import LAYERWISE, Path, check, signals, weights  # noqa: E402

GENERAL_GEMM, SEPARATE_GATE, SEPARATE_BWD_DATA, SEPARATE_FORK, PER_HEAD_FWD = 512, 2048, 4096, 8192, 32768
FWD_TOL = 2e-5       # test_gpu_grad.py, the layer-wise forward against the oracle
TAU24 = dict(tau_start="-0.028", tau_end="0.065", tau_step="0.004")   # T = 24, spin echo at index 7

# bit: (s0 on voxel batches, s0 on crops or None where the bit changes nothing there)
BITS = {
    GENERAL_GEMM: (LAYERWISE, LAYERWISE),
    SEPARATE_GATE: (0, 0),
    SEPARATE_BWD_DATA: (LAYERWISE, None),
    SEPARATE_FORK: (0, None),
    PER_HEAD_FWD: (0, 0),
}
# (U, L, channel-wise, batch): voxel batches [N] and crops [B, X, Y, Z]
VOXELS = {
    "u60-n1000": (60, 2, True, (1000,)),
    "u33-n777": (33, 1, True, (777,)),      # ragged column tail, kdim % 4 != 0, three float4 per row
    "u20-shared-n333": (20, 2, False, (333,)),   # G = 1: the gate is not fused, nothing may change
    "u64-n501": (64, 1, True, (501,)),
    "u60-n1": (60, 2, True, (1,)),          # the v < N and tile < ntile clamps of the prefetch
    "u60-n17": (60, 2, True, (17,)),
    "u60-two-rounds": (60, 2, True, None),  # 4 num_cus 64 + 83 voxels: some waves take a second tile, others prefetch past the end
}
CROPS = {
    "crop-u60": (60, 2, True, (3, 12, 11, 4)),
    "crop-u64": (64, 1, True, (3, 1, 9, 8)),
}
SEED = 3    # of the signals: the relu-site screen keeps at least 96 % of the voxels of every shape here (seen on the CPU)
# (bit, on crops) whose two sides agree bit for bit: all but the gate's bit on crops (gate_bwd_wg_kernel) and the dual
# kernel's.  Bit 2048 on voxel batches reaches xw64_gate_kernel only (selection 0 takes the block backward).
BITWISE = {(GENERAL_GEMM, False), (GENERAL_GEMM, True), (SEPARATE_GATE, False), (SEPARATE_FORK, False),
           (PER_HEAD_FWD, False), (PER_HEAD_FWD, True)}


def cases():
    out = []
    for bit, (s_vox, s_crop) in BITS.items():
        out += [(bit, s_vox, name, 11) for name in VOXELS]
        if s_crop is not None:
            out += [(bit, s_crop, name, 11) for name in CROPS]
    # the heads kernel's two layouts: 16 columns (T = 11, every case above) and 29 columns in four tiles (T = 24)
    out.append((PER_HEAD_FWD, 0, "u60-n777-t24", 24))
    out.append((PER_HEAD_FWD, 0, "u60-n777", 11))
    return out


def shape_of(name):
    if name.startswith("u60-n777"):
        return 60, 2, True, (777,)
    U, L, cw, shape = (CROPS if name in CROPS else VOXELS)[name]
    if shape is None:
        shape = (4 * torch.cuda.get_device_properties(0).multi_processor_count * 64 + 83,)
    return U, L, cw, shape


class PathT(Path):
    """Path on a tau protocol of T points with the spin echo at index se."""

    def __init__(self, params, sel, w, x, T, se):
        from qbold_vi_amd.ops import Context, EncoderWeights, TrainState
        self.ctx = Context(params, full_model=True, include_blood=True)
        self.ctx.set_kernel_selection(sel)
        U, L, cw = w["W0"].shape[1], w["Wc"].shape[0], w["Wg"].shape[2] > 1
        self.ew = EncoderWeights(self.ctx, T, U, L, cw, w["gate_offset"], spatial_taps=9).set_from_arrays(w)
        self.st = TrainState(self.ctx, self.ew)
        self.w, self.x, self.stream, self.L, self.se = w, x, 2, L, se
        self.crops = x.ndim == 5
        self.n = x.size // T

    def reference(self, g_q, g_ls):
        grads, pre, babs = ref.vjp(self.w, self.x, g_q, g_ls, None, stream=2, se_idx=self.se)
        return grads, ref.relu_sites_near_zero(pre), babs


def inputs(params, name, T):
    """(params of the protocol, weights, batch, spin-echo index) of one shape"""
    from oracle.oracle import Oracle, init_weights, synth_inputs
    U, L, cw, shape = shape_of(name)
    if T == 11:
        return params, weights(U, L, cw), signals(Oracle("f32", params), shape, SEED), 2
    p = dict(params, **TAU24)
    w = init_weights(T=T, U=U, L=L, channelwise_gating=cw, seed=4, taps=9, resid_init_std=0.08)
    rng = np.random.default_rng(4)
    for k in ("b0", "bc", "br1", "br2", "bg", "bf"):
        w[k] = (rng.standard_normal(w[k].shape) * 0.1).astype(np.float32)
    w["gate_offset"] = -3.0
    x, _ = synth_inputs(int(np.prod(shape)), p, seed=SEED, oracle=Oracle("f32", p))
    return p, w, x.reshape(*shape, T), 7


def run_pair(params, bit, s0, name, T):
    """Forward and backward under s0 and s0 | bit.  Returns the two paths, the head gradients and, per side,
    (q, log sigma, flat gradient) as float64 arrays."""
    p, w, x, se = inputs(params, name, T)
    rng = np.random.default_rng(1)
    n = x.size // T
    g_q, g_ls = rng.standard_normal((n, 5)), rng.standard_normal((n, T))
    paths, sides = [], []
    for sel in (s0, s0 | bit):
        path = PathT(p, sel, w, x, T, se)
        path.st.fused_forward = False
        q, ls = path.forward()
        q, ls = q.double().cpu().numpy(), ls.double().cpu().numpy()
        paths.append(path)
        sides.append((q, ls, path.grad(g_q, g_ls)))
    return paths, (g_q, g_ls), sides


def between(p, a, b, want, babs):
    """The largest |a - b| of a weight tensor over the denominator error_ratios() gives that tensor against `want`."""
    A, B = p.arrays(a), p.arrays(b)
    out = 0.0
    for name, l, r in ref.per_tensor(want, p.L):
        den = float(np.abs(r).max())
        if name in babs:
            den = max(den, float(np.max(babs[name] if l is None else babs[name][l])))
        d = float(np.abs((A[name] if l is None else A[name][l]) - (B[name] if l is None else B[name][l])).max())
        assert den > 0 or d == 0.0, (name, l)
        if den > 0:
            out = max(out, d / den)
    return out


def against_reference(paths, g, sides, what):
    """Both sides within EPS of the float64 VJP (head gradients screened) and FWD_TOL of the float64 forward, and no
    further from each other than each is from the reference.  Returns the measured figures."""
    p0, p1 = paths
    g_q, g_ls, want, babs = p0.screened(*g)
    ga, gb = p0.grad(g_q, g_ls), p1.grad(g_q, g_ls)
    ra, rb = check(p0, ga, want, babs, 1.0, what + ("s0",)), check(p1, gb, want, babs, 1.0, what + ("s0|bit",))
    rab = between(p0, ga, gb, want, babs)
    q64, ls64 = ref.outputs(p0.w, p0.x, stream=2, se_idx=p0.se)
    q64, ls64 = q64.reshape(-1, 5), ls64.reshape(q64.size // 5, -1)
    (qa, lsa, _), (qb, lsb, _) = sides
    fa = max(np.abs(qa - q64).max(), np.abs(lsa - ls64).max())
    fb = max(np.abs(qb - q64).max(), np.abs(lsb - ls64).max())
    fab = max(np.abs(qa - qb).max(), np.abs(lsa - lsb).max())
    fig = dict(grad_s0=ra, grad_bit=rb, grad_between=rab, fwd_s0=float(fa), fwd_bit=float(fb), fwd_between=float(fab))
    print(what, {k: f"{v:.2e}" for k, v in fig.items()})
    assert fa <= FWD_TOL and fb <= FWD_TOL, (what, fa, fb)
    assert fab <= min(fa, fb), (what, fab, fa, fb)
    assert rab <= min(ra, rb), (what, rab, ra, rb)
    return fig


@pytest.mark.parametrize("bit,s0,name,T", cases(), ids=lambda v: str(v))
def test_fused_variant_against_its_separate_launches(params, bit, s0, name, T):
    paths, g, sides = run_pair(params, bit, s0, name, T)
    (qa, lsa, ga), (qb, lsb, gb) = sides
    assert np.all(np.isfinite(ga)) and np.all(np.isfinite(gb))
    same = np.array_equal(qa, qb) and np.array_equal(lsa, lsb) and np.array_equal(ga, gb)
    print((bit, s0, name, T), "bit for bit" if same else "differs")
    if (bit, name in CROPS) in BITWISE:
        assert np.array_equal(qa, qb) and np.array_equal(lsa, lsb), (bit, name, "forward")
        assert np.array_equal(ga, gb), (bit, name, "gradient", float(np.abs(ga - gb).max()))
    else:
        against_reference(paths, g, sides, (bit, s0, name, T))
