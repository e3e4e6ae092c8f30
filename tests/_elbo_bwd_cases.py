"""The cases on which qbold_elbo_bwd's head gradients are held to tests/_elbo_bwd_reference.py: inputs, draws and the
float64 reference of either node-0 policy, built once per case and shared by test_elbo_bwd_host (the float32 floor)
and test_gpu_elbo_bwd_reference (the kernels).  NumPy and the CPU oracle only."""
import numpy as np

from _elbo_bwd_reference import elbo_bwd_reference

LOGIT_CLIP = 13.815509557963774   # QB_LOGIT_CLIP
Z_MAX = 4.8549                    # QB_Z_MAX
KSEL_GENERIC = 8388608            # QBOLD_KSEL_ELBO_BWD_GENERIC
STREAM_LIK, STREAM_KL = 0, 1


def protocol(params, T):
    """The tau grids of test_gpu_elbo_bwd_protocols: the reference's 11 and 24, 12 / 33 taus on a 1 ms grid, 22 taus with
    no tau equal to 0, BASELINE config 3's 64."""
    if T == 11:
        return dict(params)
    if T == 24:
        return dict(params, tau_start="-0.028", tau_end="0.065", tau_step="0.004")
    if T == 22:
        return dict(params, tau_start="-0.017", tau_end="0.071", tau_step="0.004")
    if T == 64:
        return dict(params, tau_start="-0.015", tau_end="0.065", tau_step="0.00125")
    return dict(params, tau_start="-0.010", tau_end=str(-0.010 + 0.001 * T - 0.0005), tau_step="0.001")


def spread(q):
    """e^s_o, e^s_d, c of raw heads q (float64)."""
    q = np.asarray(q, np.float64)
    return np.exp(3.0 * np.tanh(q[:, 1]) - 1.0), np.exp(3.0 * np.tanh(q[:, 3]) - 1.0), np.tanh(q[:, 4]) * np.exp(-2.0)


def kl_reach(q):
    """The kernels' bound on a voxel's logits, |mu| + QB_Z_MAX (|c| + e^s): below QB_LOGIT_CLIP the clip cannot bind and
    the KL takes the five-moment form."""
    q = np.asarray(q, np.float64)
    e_so, e_sd, c = spread(q)
    return np.maximum(np.abs(q[:, 0]) + Z_MAX * e_so, np.abs(q[:, 2]) + Z_MAX * (np.abs(c) + e_sd))


def draws_at_clip(q, zk):
    """Per logit and sign, how many of the KL draws u = mu + L z lie beyond the clip: [[a < -C, a > C], [b < -C, b > C]]."""
    q = np.asarray(q, np.float64)
    e_so, e_sd, c = spread(q)
    a = q[:, 0:1] + e_so[:, None] * zk[..., 0]
    b = q[:, 2:3] + c[:, None] * zk[..., 0] + e_sd[:, None] * zk[..., 1]
    return np.array([[(u < -LOGIT_CLIP).sum(), (u > LOGIT_CLIP).sum()] for u in (a, b)])


def under_reach(q):
    """Heads pulled in until no voxel's reach can pass the clip: |mu| <= 4, raw log-std heads <= 0.3."""
    q = q.copy()
    q[:, [0, 2]] = np.clip(q[:, [0, 2]], -4.0, 4.0)
    q[:, [1, 3]] = np.minimum(q[:, [1, 3]], 0.3)
    assert kl_reach(q).max() < LOGIT_CLIP - 1.0
    return q


# ---- how a case changes the encoder's heads and sigma (q, log sigma float32 in, out) ---------------------------------
def _kl_under(q, ls, rng):
    return under_reach(q), ls


def _kl_one_over(q, ls, rng):
    """Voxel 17 alone over the reach bound (OEF logit mean 13, sd 0.88): at one lane per voxel the whole first wave of
    a specialised kernel takes the general loop, at four lanes voxels 16 .. 31."""
    q = under_reach(q)
    q[17, 0], q[17, 1] = 13.0, 0.3
    over = kl_reach(q) >= LOGIT_CLIP
    assert over.sum() == 1 and over[17]
    return q, ls


def _kl_over_no_clip(q, ls, rng):
    """Every voxel 4.2 posterior standard deviations inside the clip in the OEF logit, either sign: over the reach
    bound (4.8549 sd), and no draw of the cases' streams reaches the clip (asserted where the draws are known)."""
    q = under_reach(q)
    e_so = spread(q)[0]
    q[:, 0] = (np.where(np.arange(len(q)) % 2 == 0, 1.0, -1.0) * (LOGIT_CLIP - 4.2 * e_so)).astype(np.float32)
    assert kl_reach(q).min() >= LOGIT_CLIP
    return q, ls


def _kl_clip_binds(q, ls, rng):
    """Means within half a standard deviation of the clip, in the OEF logit (voxels 0, 1 mod 4: + / -) or the DBV logit
    (2, 3 mod 4), log-std heads at raw 0.5 (sd 1.47): about a third of a voxel's draws are clipped."""
    q = under_reach(q)
    q[:, [1, 3]] = 0.5
    i = np.arange(len(q))
    q[i % 4 == 0, 0], q[i % 4 == 1, 0] = 13.2, -13.2
    q[i % 4 == 2, 2], q[i % 4 == 3, 2] = 13.2, -13.2
    return q, ls


def _saturated(q, ls, rng):
    """Raw s_o, s_d, c heads at +-3, +-5, +-8 (voxels 0 .. 17: head j = v // 6 at [3, -3, 5, -5, 8, -8][v % 6]; voxels
    18 .. 23: all three heads at once), and mu heads that put OEF (voxels 24 .. 27) or DBV (28 .. 31) within 1e-4 of
    either end of their ranges."""
    q = under_reach(q)
    vals = [3.0, -3.0, 5.0, -5.0, 8.0, -8.0]
    for v in range(18):
        q[v, (1, 3, 4)[v // 6]] = vals[v % 6]
    for v in range(18, 24):
        q[v, [1, 3, 4]] = vals[v - 18]
    # sigmoid(a) range = 1e-4 (5e-5) from an end of the range: a = -+ log(range / 1e-4 - 1)
    a_o, a_o2 = np.log(0.8 / 1e-4 - 1.0), np.log(0.8 / 5e-5 - 1.0)
    a_d, a_d2 = np.log(0.2 / 1e-4 - 1.0), np.log(0.2 / 5e-5 - 1.0)
    q[24:28, 0] = [a_o, -a_o, a_o2, -a_o2]
    q[28:32, 2] = [a_d, -a_d, a_d2, -a_d2]
    q[24:32, [1, 3]] = -1.0   # narrow posteriors: every draw stays near the end of the range
    return q, ls


def _sigma_low(q, ls, rng):
    ls = ls.copy()
    ls[:] = -11.0
    return q, ls


def _sigma_high(q, ls, rng):
    ls = ls.copy()
    ls[:] = 12.0
    return q, ls


def _sigma_mixed(q, ls, rng):
    """Each voxel's log sigma row mixes -11 and +12 (alternating taus, the phase alternating by voxel); every fourth
    voxel keeps the encoder's row."""
    ls = ls.copy()
    T = ls.shape[1]
    for v in range(len(ls)):
        if v % 4 != 3:
            ls[v] = np.where((np.arange(T) + v) % 2 == 0, -11.0, 12.0)
    return q, ls


EDITS = dict(kl_under=_kl_under, kl_one_over=_kl_one_over, kl_over_no_clip=_kl_over_no_clip,
             kl_clip_binds=_kl_clip_binds, saturated=_saturated, sigma_low=_sigma_low, sigma_high=_sigma_high,
             sigma_mixed=_sigma_mixed)

MULTI = dict(multi_image_normalisation=True)
# name: (T, context / oracle switches, kernel selection, N, S, K, edit)
CASES = {}


def _add(name, T, variant, ksel, N, S, K, edit=None):
    assert name not in CASES
    CASES[name] = (T, variant, ksel, N, S, K, edit)


# elbo_bwd_kernel<11, 2>, <11, -1> (three-image normalisation), <24, -1>: S in {1, 2} one lane per voxel, {3, 5, 9} four
# (5: two lane groups idle and a short second Philox call; 9: lane group 0 wraps); K = 70: 18 calls, the last of two
# draws; N = 40: a partial wave, 257: one block plus one voxel (four blocks plus one at four lanes).
SK_SPEC = [(1, 70, 257), (2, 0, 40), (3, 3, 257), (5, 1, 40), (9, 70, 40)]
for _tag, _T, _var in (("t11", 11, {}), ("t11_multi", 11, MULTI), ("t24", 24, {})):
    for _S, _K, _N in SK_SPEC:
        _add(f"{_tag}_S{_S}_K{_K}_N{_N}", _T, _var, 0, _N, _S, _K)
# likelihood switches at T = 11
for _tag, _var in (("student2", dict(student_t_df=2.0)), ("student5", dict(student_t_df=5.0)),
                   ("logdata", dict(predict_log_data=True)),
                   ("student5_log_multi", dict(student_t_df=5.0, predict_log_data=True, multi_image_normalisation=True))):
    for _S in (1, 3):
        _add(f"{_tag}_S{_S}", 11, _var, 0, 40, _S, 3)
# the two KL forms in the specialised kernels (N = 64: one full wave at one lane per voxel)
_add("kl_under_S1", 11, {}, 0, 64, 1, 7, "kl_under")
_add("kl_one_over_S1", 11, {}, 0, 64, 1, 7, "kl_one_over")
_add("kl_one_over_S3", 11, {}, 0, 64, 3, 7, "kl_one_over")
_add("kl_over_no_clip_S1", 11, {}, 0, 64, 1, 70, "kl_over_no_clip")
_add("kl_clip_binds_S1", 11, {}, 0, 64, 1, 70, "kl_clip_binds")
_add("kl_clip_binds_S3_t24", 24, {}, 0, 40, 3, 70, "kl_clip_binds")
# elbo_bwd_generic_kernel<1> / <4>: the KL form is per voxel at T other than 11 / 24
SK_GEN = [(1, 70, 257), (5, 3, 40)]
for _tag, _T, _var, _ksel in (("g12", 12, {}, 0), ("g33", 33, {}, 0), ("g64", 64, {}, 0), ("g22", 22, {}, 0),
                              ("g22_multi", 22, MULTI, 0), ("g11_ksel", 11, {}, KSEL_GENERIC),
                              ("g24_ksel", 24, {}, KSEL_GENERIC)):
    for _S, _K, _N in SK_GEN:
        _add(f"{_tag}_S{_S}_K{_K}_N{_N}", _T, _var, _ksel, _N, _S, _K)
_add("g12_S2_K0", 12, {}, 0, 40, 2, 0)
_add("g33_S9_K1", 33, {}, 0, 40, 9, 1)
_add("g33_kl_one_over_S1", 33, {}, 0, 64, 1, 7, "kl_one_over")
_add("g33_kl_clip_binds_S3", 33, {}, 0, 40, 3, 70, "kl_clip_binds")
_add("g11_ksel_kl_one_over_S1", 11, {}, KSEL_GENERIC, 64, 1, 7, "kl_one_over")
# edges
_add("saturated_S1", 11, {}, 0, 40, 1, 7, "saturated")
_add("saturated_S3_t24", 24, {}, 0, 40, 3, 7, "saturated")
_add("saturated_g12_S1", 12, {}, 0, 40, 1, 7, "saturated")
_add("saturated_g33_S3", 33, {}, 0, 40, 3, 7, "saturated")
_add("sigma_low_S1", 11, {}, 0, 40, 1, 3, "sigma_low")
_add("sigma_high_S3", 11, {}, 0, 40, 3, 3, "sigma_high")
_add("sigma_mixed_S1", 11, {}, 0, 40, 1, 3, "sigma_mixed")
_add("sigma_mixed_g12_S3", 12, {}, 0, 40, 3, 3, "sigma_mixed")

DEFAULT_CASE = "t11_S3_K3_N257"
# Cases whose log-sigma bound is 4 x their float32 floor instead of 1e-4 (test_gpu_elbo_bwd_reference): name -> floor,
# the worst |f32 - f64| / A_ls of the same composition on the float32 oracle's primitives, computed on the CPU
# (test_elbo_bwd_host.test_float32_floor holds the figure; nothing of the kernel enters it).  On the 12-tau protocol
# every tau lies within 10 ms of the spin echo, so every yt_t - yp_t is a difference of numbers near 1; at
# sigma = e^-11 it is multiplied by 6e4 while A_ls = 1 + r^2 is the size of what is left, and the floor passes a quarter
# of the bound.  Everywhere else the floor is 8e-6 - 2.5e-4 and the kernels are held to 1e-4.
FLOOR_LS = {"sigma_mixed_g12_S3": 2.85e-3}
SEED = 11

_oracles = {}
_inputs = {}
_built = {}


def oracles(params, T, variant):
    """(Oracle f32, Oracle f64) of a protocol and loss configuration, made once."""
    from oracle.oracle import Oracle
    key = (T, tuple(sorted(variant.items())))
    if key not in _oracles:
        p = protocol(params, T)
        _oracles[key] = (p, Oracle("f32", p, **variant), Oracle("f64", p, **variant))
    return _oracles[key]


def inputs(o32, T, n, seed=5):
    """x, mask (values 0, 0.5 and 1 mixed within every 16 voxels), q (encoder heads plus noise), prior, log sigma:
    float32 arrays, as test_gpu_elbo_bwd_protocols._case."""
    from oracle.oracle import init_weights, synth_inputs
    key = (T, n, seed)
    if key not in _inputs:
        w = init_weights(T=T, U=60, L=2, seed=seed)
        w["gate_offset"] = -3.0
        x, _ = synth_inputs(n, seed=seed, oracle=o32)
        prior, q, sigma = o32.encoder_fwd(w, x)
        rng = np.random.default_rng(seed)
        q = (q + rng.normal(size=q.shape) * 0.3).astype(np.float32)
        mask = rng.choice(np.array([0.0, 0.5, 1.0, 1.0], np.float32), size=n)
        mask[:4] = [1.0, 0.0, 0.5, 1.0]
        _inputs[key] = (x.astype(np.float32), mask, q, prior.astype(np.float32),
                        np.log(sigma.astype(np.float64)).astype(np.float32))
    return tuple(a.copy() for a in _inputs[key])


class Case:
    pass


def build(params, name):
    """The case's inputs (float32, as the kernel reads them), its Philox draws and the float64 reference of both
    policies: c.ref[node0_grad].  Built once and kept; nothing in it may be modified."""
    if name in _built:
        return _built[name]
    T, variant, ksel, N, S, K, edit = CASES[name]
    c = Case()
    c.name, c.T, c.variant, c.ksel, c.N, c.S, c.K, c.edit, c.seed = name, T, variant, ksel, N, S, K, edit, SEED
    c.p, c.o32, c.o64 = oracles(params, T, variant)
    x, mask, q, prior, ls = inputs(c.o32, T, N)
    if edit:
        q, ls = EDITS[edit](q, ls, np.random.default_rng(3))
        q, ls = q.astype(np.float32), ls.astype(np.float32)
    c.x, c.mask, c.q, c.prior, c.ls = x, mask, q, prior, ls
    c.zs = c.o32.philox_normals(c.seed, STREAM_LIK, 0, N, S).astype(np.float64)
    c.zk = c.o32.philox_normals(c.seed, STREAM_KL, 0, N, K).astype(np.float64) if K else np.zeros((N, 0, 2))
    c.sigma = np.exp(ls.astype(np.float64))
    c.ref = {g: elbo_bwd_reference(c.o64, x, mask, q, prior, c.sigma, c.zs, c.zk, g) for g in (True, False)}
    _built[name] = c
    return c


def worst_ratio(got_q, got_ls, ref):
    """max over voxels and entries of |got - ref| / A for the heads and for log sigma (entries with A = 0 -- masked-out
    voxels -- must be exact zeros and count as 0 or inf)."""
    out = []
    for got, want, A in ((got_q, ref["g_q"], ref["A_q"]), (got_ls, ref["g_log_sigma"], ref["A_ls"])):
        d = np.abs(np.asarray(got, np.float64) - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(A > 0, d / A, np.where(d == 0, 0.0, np.inf))
        out.append(float(r.max()))
    return tuple(out)
