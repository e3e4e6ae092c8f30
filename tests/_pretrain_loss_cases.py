"""The cases on which qbold_synth_loss_bwd, qbold_hyper_prior_bwd, qbold_r2p_loss_bwd, qbold_kl_diag and qbold_kl_mog
are held to tests/_pretrain_loss_reference.py: inputs (float32, as the kernels read them) and the float64 reference,
built once per case and shared by test_pretrain_loss_host (the reference itself, the float32 floor, the planted
defects) and test_gpu_pretrain_loss_reference (the kernels).  NumPy and the CPU oracle only; nothing built here may be
modified afterwards."""
import numpy as np

import _pretrain_loss_reference as R
from _elbo_bwd_cases import _saturated

BOUND_Q = 2e-4                      # test_gpu_elbo_bwd_reference's bound for head gradients
BOUND_V = dict(synth_loss=2e-5, hyper_prior=2e-5, kl_diag=2e-5, kl_mog=2e-5, r2p_loss=2e-4)
HYPER = (20.0, 2.5, 15.0, 3.0)
STREAM_R2P, STREAM_MOG = 3, 4       # qb::STREAM_R2P, kl_mog_kernel's stream
VOXEL0 = 1000
MI355X_CUS = 256                    # the host tests size the grid-stride cases for this many compute units
N_SAT = 32                          # voxels of the saturated block

# Cases whose gradient bound is 4 x their float32 floor instead of BOUND_Q: (kernel, case) -> floor, the worst
# |f32 - f64| / A_q of the reference's own formulas in float32 NumPy (test_pretrain_loss_host.test_float32_floor holds
# the figure; nothing of the kernels enters it).
# r2p_loss with two draws on the narrow posteriors of the saturated block: var = 1.4e-5 -- 1.9e-5 of mean^2 (voxels 24,
# 30), so the float32 rounding of each r_k (6e-8 of the mean) is 1.5e-5 of r_k - mean, which A takes as a term; with
# ten or seven draws on the same heads the floor is 8e-6 -- 3e-5.
FLOOR_Q = {("r2p_loss", "saturated_N40_ld5_n2_philox"): 6.8e-5}


def base_heads(n, seed):
    """0.5 N(0, 1) raw heads [n, 5], as the existing tests of these kernels draw them."""
    return (np.random.default_rng(seed).normal(size=(n, 5)) * 0.5).astype(np.float32)


def saturated_heads(n, seed):
    """base heads whose first 32 voxels are _elbo_bwd_cases._saturated's block: raw s_o / s_d / c heads at +-3, +-5,
    +-8 one at a time (voxels 0 .. 17) and all three together (18 .. 23), and narrow posteriors (raw log-std heads
    -1) whose mu heads put OEF (24 .. 27) or DBV (28 .. 31) within 1e-4 of either end of their ranges."""
    q, _ = _saturated(base_heads(n, seed), None, None)
    q = q.astype(np.float32)
    check_saturated(q[:N_SAT])
    return q


def check_saturated(b):
    """What saturated_heads claims about the block, asserted."""
    vals = [3.0, -3.0, 5.0, -5.0, 8.0, -8.0]
    for v in range(18):
        assert b[v, (1, 3, 4)[v // 6]] == vals[v % 6]
    for v in range(18, 24):
        assert list(b[v, [1, 3, 4]]) == [vals[v - 18]] * 3
    sig = lambda a: 1.0 / (1.0 + np.exp(-a.astype(np.float64)))
    oef, dbv = sig(b[24:28, 0]) * 0.8, sig(b[28:32, 2]) * 0.2
    assert np.all(np.minimum(oef, 0.8 - oef) <= 1.0001e-4) and np.all(np.minimum(dbv, 0.2 - dbv) <= 1.0001e-4)
    assert (oef < 0.4).any() and (oef > 0.4).any() and (dbv < 0.1).any() and (dbv > 0.1).any()
    assert np.all(b[24:32, [1, 3]] == -1.0)


def heads(kind, n, seed):
    """'base', 'saturated', or 'tail': base heads with the saturated block tiled over the last 256 voxels (what the
    second trip of a grid-stride loop sees when N is the grid's threads + 257)."""
    if kind == "base":
        return base_heads(n, seed)
    if kind == "saturated":
        return saturated_heads(n, seed)
    assert kind == "tail" and n > 256 + N_SAT
    q = base_heads(n, seed)
    q[-256:] = np.tile(saturated_heads(64, seed + 1)[:N_SAT], (8, 1))
    check_saturated(q[-N_SAT:])
    return q


def y_true(n, ld, seed):
    """[n, ld] true (OEF, DBV, R2', filler ...): x = (y - min) / range interior, in [1e-3, 1 - 1e-3] (two voxels in ten
    within 1e-5 of those two limits), except voxels 4, 5, 6, 7 mod 10, which sit on the four clipped ends (OEF 0.0 and
    0.9, DBV 0.0 and 0.25, where make_obs clamps x to 1e-6 / 1 - 1e-6); true R2' uniform in 1 .. 8; columns past the
    third hold 1e30 (never read)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(1.01e-3, 1.0 - 1.01e-3, size=(n, 2))
    i = np.arange(n)
    x[i % 10 == 8] = 1.0e-3 + 1e-5
    x[i % 10 == 9] = 1.0 - 1.0e-3 - 1e-5
    y = np.full((n, max(ld, 3)), 1e30, np.float32)
    y[:, 0] = (0.04 + 0.8 * x[:, 0]).astype(np.float32)
    y[:, 1] = (0.001 + 0.2 * x[:, 1]).astype(np.float32)
    y[i % 10 == 4, 0], y[i % 10 == 5, 0] = 0.0, 0.9
    y[i % 10 == 6, 1], y[i % 10 == 7, 1] = 0.0, 0.25
    y[:, 2] = rng.uniform(1.0, 8.0, n).astype(np.float32)
    y = np.ascontiguousarray(y[:, :ld])
    u = R.unit_interval(y)
    clipped = np.zeros(n, bool)
    for k, col, lo in ((4, 0, True), (5, 0, False), (6, 1, True), (7, 1, False)):
        sel = i % 10 == k
        clipped |= sel
        assert sel.any() and np.all(u[sel, col] < 1e-6 if lo else u[sel, col] > 1.0 - 1e-6)
    inner = u[~clipped]
    assert np.all(inner >= 1e-3) and np.all(inner <= 1.0 - 1e-3)
    assert np.abs(inner - 1e-3).min() < 2e-5 and np.abs(inner - (1.0 - 1e-3)).min() < 2e-5
    if ld >= 3:
        assert y[:, 2].min() >= 1.0 and y[:, 2].max() <= 8.0
    return y


def grid_stride_n(kernel, num_cus):
    """block * blocks-of-the-launch + 257: every case of this size sends the first 257 threads of the grid round their
    grid-stride loop a second time.  nlogp_bwd / hyper_prior / kl_mog: 256 x 8 CUs; r2p_loss_bwd: 128 x 8 CUs; kl_diag:
    256 x qb::elbo_grid = 4 CUs."""
    return {"synth_loss": 256 * 8, "hyper_prior": 256 * 8, "kl_mog": 256 * 8, "r2p_loss": 128 * 8,
            "kl_diag": 256 * 4}[kernel] * num_cus + 257


BIG = "big"
# kernel -> name -> spec.  N = BIG: grid_stride_n.
CASES = {
    # (heads, N, ld_y, (a, b), diagonal): (2, 0) switches the prior off (model.py:492)
    "synth_loss": {
        "base_N40_ld2_off": ("base", 40, 2, (2.0, 0.0), False),
        "base_N257_ld3_ig3": ("base", 257, 3, (3.0, 0.15), False),
        "base_N40_ld5_ig2": ("base", 40, 5, (2.0, 0.5), False),
        "saturated_N40_ld3_off": ("saturated", 40, 3, (0.0, 0.0), False),
        "saturated_N257_ld5_ig3": ("saturated", 257, 5, (3.0, 0.15), False),
        "saturated_N40_ld2_ig2": ("saturated", 40, 2, (2.0, 0.5), False),
        "diagonal_base_N257_ld3": ("base", 257, 3, (0.0, 0.0), True),
        "diagonal_saturated_N40_ld2": ("saturated", 40, 2, (0.0, 0.0), True),
        "big_tail_ld3_ig3": ("tail", BIG, 3, (3.0, 0.15), False),
    },
    # (heads, N)
    "hyper_prior": {
        "base_N40": ("base", 40),
        "base_N257": ("base", 257),
        "saturated_N40": ("saturated", 40),
        "saturated_N257": ("saturated", 257),
        "big_tail": ("tail", BIG),
    },
    # (heads, N, ld_y, n draws, philox): philox = the kernel's stream 3 at voxel0 = 1000, else explicit normals
    "r2p_loss": {
        "base_N40_ld3_n10": ("base", 40, 3, 10, False),
        "base_N257_ld5_n7_philox": ("base", 257, 5, 7, True),
        "base_N40_ld3_n2": ("base", 40, 3, 2, False),
        "saturated_N40_ld5_n10": ("saturated", 40, 5, 10, False),
        "saturated_N257_ld3_n10_philox": ("saturated", 257, 3, 10, True),
        "saturated_N40_ld3_n7": ("saturated", 40, 3, 7, False),
        "saturated_N40_ld5_n2_philox": ("saturated", 40, 5, 2, True),
        "big_tail_ld3_n10_philox": ("tail", BIG, 3, 10, True),
    },
    # (q heads, prior heads, N)
    "kl_diag": {
        "base_base_N40": ("base", "base", 40),
        "saturated_base_N257": ("saturated", "base", 257),
        "base_saturated_N40": ("base", "saturated", 40),
        "saturated_saturated_N257": ("saturated", "saturated", 257),
        "big_tail_tail": ("tail", "tail", BIG),
    },
    # (heads, N, M, philox): philox = the kernel's stream 4 at voxel0 = 1000
    "kl_mog": {
        "base_N40_M1": ("base", 40, 1, False),
        "saturated_N257_M3_philox": ("saturated", 257, 3, True),
        "saturated_N40_M16": ("saturated", 40, 16, False),
        "big_tail_M16_philox": ("tail", BIG, 16, True),
    },
}
SEED = 7
_SEEDS = {k: 100 * (i + 1) for i, k in enumerate(CASES)}


class Case:
    pass


_built = {}


def _philox(params, stream, n, k, seed=SEED):
    from oracle.oracle import Oracle
    return Oracle("f32", params).philox_normals(seed, stream, VOXEL0, n, k)


def _prior_heads(kind, n, seed):
    """Prior heads drawn independently of q; a saturated prior carries the block shifted by one voxel, so that against
    a saturated q the difference of the log-std heads reaches +-6 (s = 2 at raw 8 against s = -4 at raw -8)."""
    p = heads(kind, n, seed)
    if kind == "saturated":
        p[:N_SAT] = np.roll(p[:N_SAT], -1, axis=0)
    elif kind == "tail":
        p[-256:] = np.roll(p[-256:], -1, axis=0)
    return p


def build(params, kernel, name, num_cus=MI355X_CUS):
    """The case's inputs and its float64 reference c.ref, built once per (kernel, name, num_cus) and kept."""
    key = (kernel, name, num_cus)
    if key in _built:
        return _built[key]
    spec = CASES[kernel][name]
    c = Case()
    c.kernel, c.name, c.spec, c.seed = kernel, name, spec, SEED
    seed = _SEEDS[kernel] + list(CASES[kernel]).index(name)
    N = spec[1] if kernel != "kl_diag" else spec[2]
    c.N = N = grid_stride_n(kernel, num_cus) if N == BIG else N
    c.q = heads(spec[0], N, seed)
    if kernel == "synth_loss":
        _, _, c.ld, (c.a, c.b), c.diagonal = spec
        c.y = y_true(N, c.ld, seed + 50)
        if c.diagonal:
            c.q[:, 4] = 0.0
        c.ref = R.synth_loss(c.y, c.q, c.a, c.b, diagonal=c.diagonal)
    elif kernel == "hyper_prior":
        c.ig = HYPER
        c.ref = R.hyper_prior(c.q, c.ig)
    elif kernel == "r2p_loss":
        _, _, c.ld, c.n, c.philox = spec
        c.y = y_true(N, c.ld, seed + 50)
        c.dw = R.dw_coef(params)
        # no voxel is excluded from any comparison, so every voxel's draws must have spread: the seed of the draws
        # moves (deterministically) until the float64 variance of every voxel is at least 1e-6 of its squared mean
        for shift in range(64):
            c.seed = SEED + shift
            c.z = (_philox(params, STREAM_R2P, N, c.n, c.seed) if c.philox else
                   np.random.default_rng(seed + 70 + shift).normal(size=(N, c.n, 2)).astype(np.float32))
            c.ref = R.r2p_loss(c.y[:, 2], c.q, c.z, c.dw)
            rel = c.ref["var"] / c.ref["mean"] ** 2
            if rel.min() >= 1e-6:
                break
        assert rel.min() >= 1e-6, (name, int(np.argmin(rel)), float(rel.min()))
    elif kernel == "kl_diag":
        c.prior = _prior_heads(spec[1], N, seed + 30)
        rng = np.random.default_rng(seed + 60)
        c.mask = rng.choice(np.array([0.0, 0.5, 1.0, 1.0], np.float32), size=N)
        c.mask[:N_SAT] = np.where(np.arange(N_SAT) % 2 == 0, 1.0, 0.5)   # the saturated block is compared whole
        c.mask[-256:] = np.where(c.mask[-256:] == 0, 0.5, c.mask[-256:]) if N > 257 else c.mask[-256:]
        c.mask[32:36] = [0.0, 1.0, 0.5, 0.0]
        assert set(np.unique(c.mask)) == {0.0, 0.5, 1.0}
        if name == "base_base_N40":
            # voxels 36 .. 39: s_q - s_p = 1e-4 in both dimensions, where expm1(2 d) is 2e-4
            c.mask[36:40] = 1.0
            s = 3.0 * np.tanh(c.q[36:40, [1, 3]].astype(np.float64)) - 1.0
            c.prior[36:40, [1, 3]] = np.arctanh((s - 1e-4 + 1.0) / 3.0).astype(np.float32)
        # NaN heads in masked-out voxels only
        c.nan_voxels = np.flatnonzero(c.mask == 0)[:2]
        assert len(c.nan_voxels) == 2
        c.q[c.nan_voxels[0]] = np.nan
        c.prior[c.nan_voxels[1], 1] = np.nan
        assert np.all(c.mask[np.isnan(c.q).any(1) | np.isnan(c.prior).any(1)] == 0)
        with np.errstate(invalid="ignore"):
            c.ref = R.kl_diag(c.q, c.prior)
        d = c.ref["d"][c.mask > 0]
        if spec[0] != "base" and spec[1] != "base":
            assert d.max() >= 5.9 and d.min() <= -5.9, (d.min(), d.max())
        if name == "base_base_N40":
            assert np.all(np.abs(c.ref["d"][36:40] - 1e-4) < 2e-5), c.ref["d"][36:40]
    elif kernel == "kl_mog":
        _, _, c.M, c.philox = spec
        rng = np.random.default_rng(seed + 80)
        c.comps = (rng.normal(size=(c.M, 4)) * np.array([1.0, 0.5, 1.0, 0.5])).astype(np.float32)
        c.z = (_philox(params, STREAM_MOG, N, 1)[:, 0] if c.philox else
               rng.normal(size=(N, 2)).astype(np.float32))
        c.ref = R.kl_mog(c.q, c.comps, c.z)
    for a in vars(c).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    for a in c.ref.values():
        a.setflags(write=False)
    _built[key] = c
    return c


def evaluate(c, dt, defect=None):
    """The reference's formulas on the case's inputs in precision dt, with an optional planted defect."""
    with np.errstate(invalid="ignore"):
        if c.kernel == "synth_loss":
            return R.synth_loss(c.y, c.q, c.a, c.b, diagonal=c.diagonal, dt=dt, defect=defect)
        if c.kernel == "hyper_prior":
            return R.hyper_prior(c.q, c.ig, dt=dt, defect=defect)
        if c.kernel == "r2p_loss":
            return R.r2p_loss(c.y[:, 2], c.q, c.z, c.dw, dt=dt, defect=defect)
        if c.kernel == "kl_diag":
            return R.kl_diag(c.q, c.prior, dt=dt, defect=defect)
        return R.kl_mog(c.q, c.comps, c.z, dt=dt)


def compared(c):
    """The voxels whose gradient is compared: all of them, except kl_diag's masked-out ones (asserted untouched)."""
    return c.mask > 0 if c.kernel == "kl_diag" else np.ones(c.N, bool)


def worst_ratios(c, got_v, got_g):
    """(worst |d| / A_v, worst |d| / A_q) of a result against the case's reference; got_g None: values only."""
    sel = compared(c)
    finite = ~np.isnan(c.ref["v"])
    rv = R.worst(np.asarray(got_v)[finite], c.ref["v"][finite], c.ref["A_v"][finite])
    rq = R.worst(np.asarray(got_g)[sel], c.ref["g_q"][sel], c.ref["A_q"][sel]) if got_g is not None else 0.0
    return rv, rq


def bound_q(kernel, name):
    return 4.0 * FLOOR_Q[(kernel, name)] if (kernel, name) in FLOOR_Q else BOUND_Q
