"""The float64 reference of the training backward (tests/_train_bwd_reference.py) against the C oracle: its forward
equals qbo_encoder_fwd / qbo_encoder_fwd_spatial, its VJP equals central differences of the float64 oracle (random
directions and single off-centre taps that reach crop borders), and the per-tensor comparison the GPU tests use
rejects planted kernel defects while it accepts a float32 evaluation of the same reference.  The same for its
normalizer mode (use_layer_norm, dropout_rate): forward and VJP against the oracle's restatement, the planted defects
detach_var and stale_mask, the relu bands of the GPU file's layer-norm crop cases, and the oracle's exported dropout
keep factors.  CPU only."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _train_bwd_reference as ref  # noqa: E402

EPS = ref.EPS   # the GPU tests' per-tensor tolerance (max |hip - ref| <= EPS max |ref|)


def weights(U, L, cw, seed, taps=9, gate_offset=-3.0):
    from oracle.oracle import init_weights
    w = init_weights(T=11, U=U, L=L, channelwise_gating=cw, seed=seed, taps=taps, resid_init_std=0.08)
    rng = np.random.default_rng(seed)
    for k in ("b0", "bc", "br1", "br2", "bg", "bf"):
        w[k] = (rng.standard_normal(w[k].shape) * 0.1).astype(np.float32)
    w["gate_offset"] = gate_offset
    return w


def crops(oracle, B, X, Y, Z, seed):
    from oracle.oracle import synth_inputs
    x, _ = synth_inputs(B * X * Y * Z, seed=seed, oracle=oracle)
    return x.reshape(B, X, Y, Z, 11).astype(np.float64)


@pytest.mark.parametrize("U,L,cw", [(60, 2, True), (20, 1, False), (33, 2, True)])
def test_forward_equals_oracle(oracle64, U, L, cw):
    w = weights(U, L, cw, seed=3)
    xv = crops(oracle64, 1, 1, 1, 40, seed=2).reshape(-1, 11)
    o1, o2, sg = oracle64.encoder_fwd(w, xv)
    q2, ls = ref.outputs(w, xv, se_idx=oracle64.se_idx)
    q1, _ = ref.outputs(w, xv, stream=1, se_idx=oracle64.se_idx)
    for got, want in ((q2, o2), (ls, np.log(sg)), (q1, o1)):
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    x = crops(oracle64, 3, 5, 4, 2, seed=4)
    o2, sg = oracle64.encoder_fwd_spatial(w, x)
    q2, ls = ref.outputs(w, x, se_idx=oracle64.se_idx)
    assert np.abs(q2 - o2).max() <= 1e-12 * np.abs(o2).max()
    assert np.abs(ls - np.log(sg)).max() <= 1e-12 * np.abs(np.log(sg)).max()
    # the neighbourhood matters (the crop forward is not the voxel-wise one)
    assert np.abs(q2.reshape(-1, 5) - ref.outputs(w, x.reshape(-1, 11), se_idx=oracle64.se_idx)[0]).max() > 1e-3


def _oracle_loss(oracle64, w, x, g_q, g_ls, stream, s):
    if x.ndim == 5:
        o2, sg = oracle64.encoder_fwd_spatial(w, x)
        q, ls = o2.reshape(-1, 5), np.log(sg).reshape(-1, 11)
    else:
        o1, o2, sg = oracle64.encoder_fwd(w, x)
        q, ls = (o1, None) if stream == 1 else (o2, np.log(sg))
    v = (q * g_q).sum()
    if ls is not None:
        v += (ls * g_ls).sum()
    return v / s


def _fd(oracle64, w, x, g_q, g_ls, stream, s, direction, h=1e-6):
    wp = {k: (np.asarray(w[k], np.float64) + h * direction[k]) if k in direction else w[k] for k in w}
    wm = {k: (np.asarray(w[k], np.float64) - h * direction[k]) if k in direction else w[k] for k in w}
    return (_oracle_loss(oracle64, wp, x, g_q, g_ls, stream, s) - _oracle_loss(oracle64, wm, x, g_q, g_ls, stream, s)) / (2 * h)


@pytest.mark.parametrize("case", ["voxel2", "voxel1", "crop"])
def test_vjp_equals_oracle_central_differences(oracle64, case):
    rng = np.random.default_rng(7)
    U, L = 20, 2
    w = weights(U, L, True, seed=5, taps=9)
    if case == "crop":   # 4 x 3 crops: every off-centre tap reaches a border of some voxel
        x = crops(oracle64, 2, 4, 3, 2, seed=6)
    else:
        x = crops(oracle64, 1, 1, 1, 30, seed=6).reshape(-1, 11)
    stream = 1 if case == "voxel1" else 2
    n = x.size // 11
    g_q = rng.standard_normal((n, 5))
    g_ls = None if stream == 1 else rng.standard_normal((n, 11))
    sums = [0.0, 0.0, 3.0]
    grads, _, _ = ref.vjp(w, x, g_q, g_ls, sums, stream=stream, se_idx=oracle64.se_idx)
    dirs = [{k: rng.standard_normal(np.shape(w[k])) for k in ref.NAMES} for _ in range(3)]
    if case == "crop":
        for (i, j) in ((0, 0), (2, 1), (1, 2), (0, 2)):   # single off-centre taps, one entry each
            for name in ("Wr1", "Wr2"):
                d = {k: np.zeros(np.shape(w[k])) for k in ref.NAMES}
                d[name][1, i, j, 3, 5] = 1.0
                dirs.append(d)
    for d in dirs:
        want = _fd(oracle64, w, x, g_q, g_ls, stream, sums[2], d)
        got = sum(float((grads[k] * d[k]).sum()) for k in ref.NAMES)
        assert abs(got - want) <= 1e-7 * max(abs(want), 1e-2 * max(abs(float(np.abs(grads[k]).max())) for k in grads)), \
            (got, want)


def _worst(got, want, bias_abs):
    return max(ref.error_ratios(got, want, bias_abs).values())


@pytest.mark.parametrize("U,L,geom", [(60, 2, (2, 9, 8, 4)), (20, 1, (3, 6, 5, 4))])
def test_comparison_has_teeth(oracle64, U, L, geom):
    """The GPU tests' per-tensor tolerance EPS rejects a backward whose 3x3 products see the deltas as an f16 high half
    only (a split that lost its lo half) and one that drops an off-centre tap at a crop border, each by at least 10x;
    it accepts the torch float32 evaluation of the same reference."""
    rng = np.random.default_rng(11)
    w = weights(U, L, True, seed=8)
    x = crops(oracle64, *geom, seed=9)
    n = x.size // 11
    g_q, g_ls = rng.standard_normal((n, 5)), rng.standard_normal((n, 11))
    sums = [0.0, 0.0, float(n)]
    want, pre, bias_abs = ref.vjp(w, x, g_q, g_ls, sums, se_idx=oracle64.se_idx)
    f32, _, _ = ref.vjp(w, x, g_q, g_ls, sums, se_idx=oracle64.se_idx, dtype=torch.float32)
    hi, _, _ = ref.vjp(w, x, g_q, g_ls, sums, se_idx=oracle64.se_idx, hi_only_deltas=True)
    drop, _, _ = ref.vjp(w, x, g_q, g_ls, sums, se_idx=oracle64.se_idx, drop_border_tap=True)
    assert _worst(f32, want, bias_abs) <= EPS / 4
    assert _worst(hi, want, bias_abs) >= 10 * EPS
    assert _worst(drop, want, bias_abs) >= 10 * EPS


def test_relu_screen_keeps_most_voxels(oracle64):
    """The screen that makes the GPU comparison immune to relu flips removes few voxels at the optimal.yaml shape."""
    w = weights(60, 2, True, seed=8)
    x = crops(oracle64, 2, 12, 10, 4, seed=9)
    n = x.size // 11
    _, pre, _ = ref.vjp(w, x, np.ones((n, 5)), np.ones((n, 11)), se_idx=oracle64.se_idx)
    keep = ref.keep_mask(ref.relu_sites_near_zero(pre), x.shape[:4])
    assert keep.mean() >= 0.8
    # the dilation is Chebyshev `reach` in x / y, within one batch element and z slice
    reach = np.full(x.shape[:4], -1)
    reach[1, 0, 0, 2] = 2
    reach[0, 5, 5, 1] = 0
    k = ref.keep_mask(reach.reshape(-1), x.shape[:4]).reshape(x.shape[:4])
    assert (~k).sum() == 10 and not k[1, :3, :3, 2].any() and not k[0, 5, 5, 1] and k[1, :, :, 1].all()


# ---- normalizer mode: use_layer_norm and dropout_rate ------------------------------------------------------------------
SEED = ref.FIRST_STEP_SEED


def _with_activation(oracle, act):
    oracle.lib.qbo_set_activation_gelu(1 if act == "gelu" else 0)


def _norm_inputs(oracle64, geom, U, L, with_ln, rate, wseed=5, xseed=4):
    w, ln = ref.norm_weights(U, L, True, wseed)
    x = crops(oracle64, *geom, seed=xseed)
    n = x.size // 11
    return w, (ln if with_ln else None), x, ref.drop_factors(oracle64, rate, SEED, L, n, U)


@pytest.mark.parametrize("act", ["relu", "gelu"])
@pytest.mark.parametrize("with_ln,rate", [(True, 0.0), (False, 0.3), (True, 0.25)])
@pytest.mark.parametrize("geom", [(3, 5, 4, 2), (37, 1, 1, 1)])
def test_normalizer_forward_equals_oracle(oracle64, geom, with_ln, rate, act):
    """The reference forward with ln, with drop and with both equals qbo_encoder_fwd_spatial under the same
    GroupNormalization parameters and (rate, seed) to 1e-12; on an (N,1,1,1) batch the voxel-shaped call equals the
    crop-shaped one (group = one voxel, centre tap)."""
    w, ln, x, drop = _norm_inputs(oracle64, geom, 20, 2, with_ln, rate)
    _with_activation(oracle64, act)
    try:
        o2, sg = oracle64.encoder_fwd_spatial(w, x, ln=ln, dropout_rate=rate, dropout_seed=SEED if rate > 0 else 0)
        plain, _ = oracle64.encoder_fwd_spatial(w, x)
    finally:
        _with_activation(oracle64, "relu")
    q, ls = ref.outputs(w, x, act=act, se_idx=oracle64.se_idx, ln=ln, drop=drop)
    assert np.abs(q - o2).max() <= 1e-12 * np.abs(o2).max()
    assert np.abs(ls - np.log(sg)).max() <= 1e-12 * np.abs(np.log(sg)).max()
    assert np.abs(plain - o2).max() > 1e-3          # the normalizer does something
    if geom[1:] == (1, 1, 1):
        qv, lsv = ref.outputs(w, x.reshape(-1, 11), act=act, se_idx=oracle64.se_idx, ln=ln, drop=drop)
        assert np.abs(qv - q.reshape(-1, 5)).max() <= 1e-13 * np.abs(q).max()
        assert np.abs(lsv - ls.reshape(-1, 11)).max() <= 1e-13 * np.abs(ls).max()


def _norm_fd(oracle64, w, ln, x, rate, act, g_q, g_ls, s, d, dln, h=1e-6):
    def loss(sign):
        ww = {k: (np.asarray(w[k], np.float64) + sign * h * d[k]) if k in d else w[k] for k in w}
        lln = np.asarray(ln, np.float64) + sign * h * dln
        _with_activation(oracle64, act)
        try:
            o2, sg = oracle64.encoder_fwd_spatial(ww, x, ln=lln, dropout_rate=rate, dropout_seed=SEED if rate > 0 else 0)
        finally:
            _with_activation(oracle64, "relu")
        return ((o2.reshape(-1, 5) * g_q).sum() + (np.log(sg).reshape(-1, 11) * g_ls).sum()) / s
    return (loss(1.0) - loss(-1.0)) / (2 * h)


@pytest.mark.parametrize("geom,act,rate", [((2, 4, 3, 2), "relu", 0.0), ((2, 4, 3, 2), "gelu", 0.2),
                                           ((30, 1, 1, 1), "relu", 0.3)])
def test_normalizer_vjp_equals_oracle_central_differences(oracle64, geom, act, rate):
    """The VJP in normalizer mode against central differences of the float64 oracle (the file's 1e-7 criterion): random
    directions over every tensor and ln, GroupNormalization-only directions, single entries of one gamma and one
    beta."""
    rng = np.random.default_rng(7)
    U, L = 20, 2
    w, ln, x, drop = _norm_inputs(oracle64, geom, U, L, True, rate)
    n = x.size // 11
    g_q, g_ls = rng.standard_normal((n, 5)), rng.standard_normal((n, 11))
    sums = [0.0, 0.0, 3.0]
    grads, _, _ = ref.vjp(w, x, g_q, g_ls, sums, act=act, se_idx=oracle64.se_idx, ln=ln, drop=drop)
    zero = {k: np.zeros(np.shape(w[k])) for k in ref.NAMES}
    dirs = [({k: rng.standard_normal(np.shape(w[k])) for k in ref.NAMES}, rng.standard_normal(ln.shape))
            for _ in range(3)]
    dirs += [(zero, rng.standard_normal(ln.shape)) for _ in range(2)]           # GroupNormalization only
    for (l, row, c) in ((1, 0, 3), (0, 2, 17), (0, 1, 5), (1, 3, 0)):            # one gamma / one beta entry
        dln = np.zeros(ln.shape)
        dln[l, row, c] = 1.0
        dirs.append((zero, dln))
    scale = max(float(np.abs(g).max()) for g in grads.values())
    for d, dln in dirs:
        want = _norm_fd(oracle64, w, ln, x, rate, act, g_q, g_ls, sums[2], d, dln)
        got = sum(float((grads[k] * d[k]).sum()) for k in ref.NAMES) + float((grads["ln"] * dln).sum())
        assert abs(got - want) <= 1e-7 * max(abs(want), 1e-2 * scale), (got, want)


@pytest.mark.parametrize("geom,act,rate", [((2, 9, 8, 4), "gelu", 0.0), ((300, 1, 1, 1), "relu", 0.25)])
def test_normalizer_comparison_has_teeth(oracle64, geom, act, rate):
    """At EPS the per-tensor comparison (with the bias and GroupNormalization-row bounds in place) rejects an LN
    backward without its variance term and a backward under the next step's dropout mask, each by at least 10x on
    some tensor; the torch float32 evaluation of the same reference stays within EPS / 4.  One LN crop case, one
    LN + dropout voxel case (voxel-shaped call)."""
    rng = np.random.default_rng(11)
    U, L = 60, 2
    w, ln, x, drop = _norm_inputs(oracle64, geom, U, L, True, rate)
    if geom[1:] == (1, 1, 1):
        x = x.reshape(-1, 11)
    n = x.size // 11
    g_q, g_ls = rng.standard_normal((n, 5)), rng.standard_normal((n, 11))
    sums = [0.0, 0.0, float(n)]
    kw = dict(act=act, se_idx=oracle64.se_idx, ln=ln, drop=drop)
    want, _, babs = ref.vjp(w, x, g_q, g_ls, sums, **kw)
    assert "ln" in babs and babs["ln"].shape == ln.shape and (babs["ln"].max(-1) > 0).all()
    f32, _, _ = ref.vjp(w, x, g_q, g_ls, sums, dtype=torch.float32, **kw)
    worst32 = _worst(f32, want, babs)
    print(f"{geom} {act} rate {rate}: float32 evaluation {worst32:.2e}")
    assert worst32 <= EPS / 4
    det, _, _ = ref.vjp(w, x, g_q, g_ls, sums, detach_var=True, **kw)
    print(f"  detach_var {_worst(det, want, babs):.2e}")
    assert _worst(det, want, babs) >= 10 * EPS
    if rate > 0:
        stale = ref.drop_factors(oracle64, rate, SEED + 1, L, n, U)
        assert not np.array_equal(stale, drop)
        st, _, _ = ref.vjp(w, x, g_q, g_ls, sums, stale_mask=stale, **kw)
        print(f"  stale_mask {_worst(st, want, babs):.2e}")
        assert _worst(st, want, babs) >= 10 * EPS
        same, _, _ = ref.vjp(w, x, g_q, g_ls, sums, stale_mask=drop, **kw)   # the planted path itself is exact
        assert _worst(same, want, babs) <= 1e-12


def test_error_ratios_hold_every_group_norm_row():
    """error_ratios reports gamma1, beta1, gamma2, beta2 of every block separately, and a tensor the reference leaves
    identically zero must come out exactly zero."""
    rng = np.random.default_rng(3)
    w, ln = ref.norm_weights(8, 2, True, 1)
    want = {k: rng.standard_normal(np.shape(w[k])) for k in ref.NAMES}
    want["ln"] = rng.standard_normal(ln.shape)
    got = {k: v.copy() for k, v in want.items()}
    got["ln"][1, 3, 2] += 1e-3 * np.abs(want["ln"][1, 3]).max()
    r = ref.error_ratios(got, want)
    assert len([k for k in r if k[0].startswith("ln:")]) == 8
    assert abs(r[("ln:beta2", 1)] - 1e-3) < 1e-9 and max(v for k, v in r.items() if k != ("ln:beta2", 1)) == 0.0
    want["ln"][:] = 0.0
    assert ref.error_ratios(want, want)[("ln:gamma1", 0)] == 0.0
    got["ln"][:] = 0.0
    got["ln"][0, 0, 0] = 1e-30
    assert ref.error_ratios(got, want)[("ln:gamma1", 0)] == np.inf


@pytest.mark.parametrize("name", [k for k, c in ref.NORM_CASES.items()
                                  if c[2] == "relu" and c[3] and len(c[0]) == 4 and int(np.prod(c[0][1:])) > 1])
def test_relu_layer_norm_crop_cases_have_an_empty_band(oracle32, oracle64, name):
    """A relu + layer-norm crop case of the GPU file cannot be screened (the group sums carry every voxel's delta to
    every site of its crop): at its hard-coded seeds the float64 forward has no relu site within 1e-5 rms of zero."""
    _, _, act, _, rate, U, L, _, _, _ = ref.NORM_CASES[name]
    w, ln, x = ref.norm_case(name, oracle32)
    n = x.size // 11
    drop = ref.drop_factors(oracle64, rate, SEED, L, n, U)
    _, pre, _ = ref.vjp(w, x, np.ones((n, 5)), np.ones((n, 11)), act=act, se_idx=oracle64.se_idx, ln=ln, drop=drop)
    assert {"z0", "zc0", "v10", "v20"} <= set(pre)
    assert ref.band_is_empty(pre)


def test_relu_band_finds_a_planted_site(oracle32, oracle64):
    """The band check has teeth: a beta moved so that one normalizer output lands at 1e-7 rms is found."""
    w, ln, x = ref.norm_case("c-ln-drop-relu", oracle32)
    n = x.size // 11
    _, pre, _ = ref.vjp(w, x, np.ones((n, 5)), np.ones((n, 11)), se_idx=oracle64.se_idx, ln=ln)
    z, _, rms = pre["v21"]
    ln = ln.astype(np.float64)
    ln[1, 3, 7] -= z[2, 3, 1, 0, 7] - 1e-7 * rms
    _, pre, _ = ref.vjp(w, x, np.ones((n, 5)), np.ones((n, 11)), se_idx=oracle64.se_idx, ln=ln)
    assert not ref.band_is_empty(pre)
    reach = ref.relu_sites_near_zero(pre).reshape(x.shape[:4])
    assert reach[2, 3, 1, 0] == 1      # one convolution (conv2 of block 1) behind the site


@pytest.mark.parametrize("rate", [0.1, 0.25, 0.5])
def test_oracle_dropout_factors(oracle64, oracle32, rate):
    """Oracle.dropout_factors: values in {0, keep_scale}; the share of zeros over 200 x 256 factors within 4 binomial
    sigma of lrint(rate 65536) / 65536; layers differ; rows (row0 = 7, rows - 7) are those of (row0 = 0, rows) shifted;
    and they are the factors the oracle's forward applies."""
    rows, U = 200, 256
    p = float(np.rint(np.float32(rate) * np.float32(65536.0))) / 65536.0
    f = oracle64.dropout_factors(rate, SEED, 0, rows, U)
    assert f.shape == (rows, U)
    assert np.all((f == 0.0) | (f == 1.0 / (1.0 - p)))
    share = float((f == 0.0).mean())
    assert abs(share - p) <= 4.0 * np.sqrt(p * (1.0 - p) / (rows * U)), (share, p)
    assert not np.array_equal(f, oracle64.dropout_factors(rate, SEED, 1, rows, U))
    assert not np.array_equal(f, oracle64.dropout_factors(rate, SEED + 1, 0, rows, U))
    assert np.array_equal(f[7:], oracle64.dropout_factors(rate, SEED, 0, rows - 7, U, row0=7))
    assert np.array_equal(f[:, :65], oracle64.dropout_factors(rate, SEED, 0, rows, 65))        # columns do not depend on U
    assert np.array_equal(f.astype(np.float32), oracle32.dropout_factors(rate, SEED, 0, rows, U))
    assert np.all(oracle64.dropout_factors(0.0, SEED, 0, 3, 8) == 1.0)          # rate 0 or seed 0: the identity
    assert np.all(oracle64.dropout_factors(rate, 0, 0, 3, 8) == 1.0)
