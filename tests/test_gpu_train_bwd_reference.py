"""The training backward (qbold_encoder_train_bwd, qbold_encoder_spatial_bwd) against the float64 VJP of
tests/_train_bwd_reference.py, per weight tensor: max |hip - ref| <= EPS max |ref| (bias tensors: over the larger of
that and max sum_v |delta|), with the head gradients of voxels near a relu site within 1e-5 rms of zero set to zero
(a float32 forward may take the other side there).  Every path of the backward, head gradients scaled by 2^k from
2^-60 to 2^60 with and without a `sums` normaliser, per-voxel magnitudes over fifteen decades, impulses on crop
borders, and the ELBO's own head gradients of an outlier voxel under a small sigma (beyond f16's range).

Worst ratios measured on an MI355X are in MEASUREMENTS.md ("Training backward against a float64 VJP")."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _train_bwd_reference as ref  # noqa: E402

EPS = ref.EPS
LAYERWISE, BF16, EXACT_DW, EXACT_CONV = 131072, 4194304, 524288, 65536
KS = (-60, -40, -20, -8, 0, 8, 16, 17, 20, 24, 40, 60)
SUMS = (None, 1.1e5, 3e9)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def weights(U, L, cw, seed=4, gate_offset=-3.0):
    from oracle.oracle import init_weights
    w = init_weights(T=11, U=U, L=L, channelwise_gating=cw, seed=seed, taps=9, resid_init_std=0.08)
    rng = np.random.default_rng(seed)
    for k in ("b0", "bc", "br1", "br2", "bg", "bf"):
        w[k] = (rng.standard_normal(w[k].shape) * 0.1).astype(np.float32)
    w["gate_offset"] = gate_offset
    return w


def signals(oracle32, shape, seed):
    from oracle.oracle import synth_inputs
    x, _ = synth_inputs(int(np.prod(shape)), seed=seed, oracle=oracle32)
    return x.reshape(*shape, 11)


class Path:
    """One backward path: a context with a kernel selection, the weights, a batch (voxels [N, 11] or crops
    [B, X, Y, Z, 11]) and the stream; optionally the activation, GroupNormalization parameters ln [L, 4, U]
    (use_layer_norm) and a dropout rate, whose keep factors at the state's step come from `oracle`."""

    act, ln, drop, seed = "relu", None, None, 0   # a plain relu path (a subclass with a constructor of its own keeps these)

    def __init__(self, params, sel, w, x, stream=2, activation="relu", ln=None, dropout_rate=0.0, oracle=None):
        from qbold_vi_amd.ops import Context, EncoderWeights, TrainState
        self.ctx = Context(params, full_model=True, include_blood=True)
        self.ctx.set_kernel_selection(sel)
        U, L, cw = w["W0"].shape[1], w["Wc"].shape[0], w["Wg"].shape[2] > 1
        self.ew = EncoderWeights(self.ctx, 11, U, L, cw, w["gate_offset"], spatial_taps=9, activation=activation,
                                 layer_norm=ln is not None, dropout_rate=dropout_rate)
        self.ew.set_from_arrays(w if ln is None else dict(w, ln=ln))
        self.st = TrainState(self.ctx, self.ew)
        self.w, self.x, self.stream, self.L = w, x, stream, L
        self.crops = x.ndim == 5
        self.n = x.size // 11
        self.act, self.ln = activation, ln
        if dropout_rate > 0.0:   # one forward draws the step's mask; every backward here runs at the same step
            self.forward()
            self.seed = int(self.ew.shape.dropout_seed)
            assert self.seed != 0
            self.drop = ref.drop_factors(oracle, dropout_rate, self.seed, L, self.n, U)

    def forward(self, x=None):
        x = self.x if x is None else x
        if self.crops:
            return self.st.forward_spatial(dev(x))
        return self.st.forward(dev(x), self.stream)

    def grad(self, g_q, g_ls, sums=None):
        self.forward()
        assert int(self.ew.shape.dropout_seed) == self.seed
        s = None if sums is None else dev(np.array([0.0, 0.0, sums], np.float64))
        gq, gls = dev(g_q.astype(np.float32)), None if g_ls is None else dev(g_ls.astype(np.float32))
        if self.crops:
            g = self.st.backward_spatial(gq, gls, s)
        else:
            g = self.st.backward(self.stream, gq, gls, s)
        torch.cuda.synchronize()
        return g.double().cpu().numpy()

    def arrays(self, flat):
        return ref.to_arrays(flat, self.ew._slices())

    def reference(self, g_q, g_ls):
        """float64 VJP (no normaliser), the relu screen's reach per voxel and the bias bounds"""
        grads, pre, babs = ref.vjp(self.w, self.x, g_q, g_ls, None, stream=self.stream, se_idx=2, act=self.act,
                                   ln=self.ln, drop=self.drop)
        return grads, ref.relu_sites_near_zero(pre), babs

    def screened(self, g_q, g_ls, min_keep=0.8):
        """head gradients with the voxels in reach of a near-zero relu site zeroed, and the reference VJP"""
        _, reach, _ = self.reference(g_q, g_ls)
        keep = ref.keep_mask(reach, self.x.shape[:4] if self.crops else None)
        assert keep.mean() >= min_keep, keep.mean()
        g_q = g_q * keep[:, None]
        g_ls = None if g_ls is None else g_ls * keep[:, None]
        grads, _, babs = self.reference(g_q, g_ls)
        return g_q, g_ls, grads, babs


def check(p, flat, want, babs, f=1.0, what=""):
    """Every entry finite, every tensor within EPS of f x want; returns the worst ratio."""
    assert np.all(np.isfinite(flat)), (what, int((~np.isfinite(flat)).sum()))
    r = ref.error_ratios(p.arrays(flat), ref.scaled(want, f), ref.scaled(babs, abs(f)))
    worst = max(r, key=r.get)
    assert r[worst] <= EPS, (what, worst, r[worst])
    return r[worst]


def heads(rng, n, stream):
    return rng.standard_normal((n, 5)), None if stream == 1 else rng.standard_normal((n, 11))


# (selection, U, L, channel-wise, batch, stream): every family at optimal.yaml's training shape and an odd one
PATHS = {
    "voxel-block": (0, 60, 2, True, (1000,), 2),
    "voxel-block-odd": (0, 33, 1, True, (777,), 2),
    "voxel-layerwise": (LAYERWISE, 60, 2, True, (1000,), 2),
    "voxel-layerwise-odd": (LAYERWISE, 20, 2, False, (333,), 2),
    "voxel-layerwise-bf16": (LAYERWISE | BF16, 60, 2, True, (1000,), 2),
    "voxel-layerwise-exact": (LAYERWISE | EXACT_DW, 60, 2, True, (1000,), 2),
    "voxel-stream1": (0, 60, 2, True, (1000,), 1),
    "voxel-stream1-odd": (0, 64, 1, False, (501,), 1),
    "crop": (0, 60, 2, True, (3, 12, 11, 4), 2),
    "crop-odd": (0, 64, 1, True, (3, 1, 9, 8), 2),
    "crop-bf16": (BF16, 60, 2, True, (3, 12, 11, 4), 2),
    "crop-exact": (EXACT_CONV | EXACT_DW, 60, 2, True, (3, 12, 11, 4), 2),
    "crop-ninetap-z": (0, 60, 2, True, (3, 10, 9, 3), 2),
    "crop-ninetap-u": (0, 33, 1, False, (4, 9, 1, 4), 2),
}
# selections whose every step is exact float32 or scaled by powers of two found from the data (conv9h_kernel's
# backward-data form): scaling the head gradients by 2^k scales the gradient bit for bit
EXACT = ("voxel-layerwise-exact", "crop-exact", "crop-ninetap-z", "crop-ninetap-u")


def make_path(params, oracle32, name, seed=3):
    sel, U, L, cw, shape, stream = PATHS[name]
    return Path(params, sel, weights(U, L, cw), signals(oracle32, shape, seed), stream)


@pytest.mark.parametrize("name", list(PATHS))
def test_scale_sweep(params, oracle32, name):
    """Head gradients 2^k g0, k from -60 to 60, with sums[2] in {none, 1.1e5, 3e9}: every entry finite and every tensor
    within EPS of 2^k / sums[2] x the float64 VJP of g0; the exact-f32 selections scale bit for bit.

    Worst ratios measured on an MI355X: voxel-block 7.1e-7, voxel-block-odd 6.4e-7, voxel-layerwise 6.9e-7,
    voxel-layerwise-odd 1.5e-6, voxel-layerwise-bf16 7.4e-7, voxel-layerwise-exact 9.1e-7, voxel-stream1 3.1e-7,
    voxel-stream1-odd 3.6e-7, crop 5.6e-7, crop-odd 3.8e-7, crop-bf16 6.2e-7, crop-exact 9.8e-7, crop-ninetap-z 5.8e-7,
    crop-ninetap-u 1.2e-6 (MEASUREMENTS.md, section 15)."""
    p = make_path(params, oracle32, name)
    rng = np.random.default_rng(1)
    g_q, g_ls = heads(rng, p.n, p.stream)
    g_q, g_ls, want, babs = p.screened(g_q, g_ls)
    if name == "voxel-block" or name == "voxel-block-odd":
        import ctypes as C
        assert p.ctx.lib.qbold_encoder_train_bwd_recomputes(p.ctx.handle, C.byref(p.ew.shape), p.n) == 2
    base = {s: p.grad(g_q, g_ls, s) for s in SUMS}
    worst = 0.0
    for k in KS:
        f = 2.0 ** k
        for s in SUMS:
            got = base[s] if k == 0 else p.grad(g_q * f, None if g_ls is None else g_ls * f, s)
            worst = max(worst, check(p, got, want, babs, f / (1.0 if s is None else s), (name, k, s)))
            if name in EXACT:
                assert np.array_equal(got, base[s] * f), (name, k, s)
    print(f"{name}: worst ratio {worst:.2e}")


@pytest.mark.parametrize("name", ["crop", "crop-bf16", "crop-exact", "crop-ninetap-z", "voxel-layerwise", "voxel-block"])
def test_mixed_magnitudes(params, oracle32, name):
    """Per-voxel head-gradient magnitudes log-uniform over 1e-9 .. 1e6, and one outlier voxel at 1e6 in an O(1) batch."""
    p = make_path(params, oracle32, name)
    rng = np.random.default_rng(2)
    g_q, g_ls = heads(rng, p.n, p.stream)
    g_q, g_ls, _, _ = p.screened(g_q, g_ls)
    mag = np.exp(rng.uniform(np.log(1e-9), np.log(1e6), (p.n, 1)))
    out = np.ones((p.n, 1))
    out[p.n // 3] = 1e6
    for m in (mag, out):
        want, _, babs = ref.vjp(p.w, p.x, g_q * m, g_ls * m, None, se_idx=2)
        for s in (None, 3e9):
            check(p, p.grad(g_q * m, g_ls * m, s), want, babs, 1.0 / (1.0 if s is None else s), (name, s))


@pytest.mark.parametrize("name", ["crop", "crop-bf16", "crop-exact", "crop-odd"])
def test_impulses_on_crop_borders(params, oracle32, name):
    """A single non-zero head-gradient voxel at every corner and edge of a crop and on both sides of the boundary
    between two batch elements: the tap geometry and the flip of the backward-data products."""
    p = make_path(params, oracle32, name)
    B, X, Y, Z = p.x.shape[:4]
    rng = np.random.default_rng(4)
    g_q0, g_ls0 = heads(rng, p.n, 2)
    _, reach, _ = p.reference(g_q0, g_ls0)
    keep = ref.keep_mask(reach, (B, X, Y, Z)).reshape(B, X, Y, Z)
    spots = set()
    for b in range(B):
        for x in sorted({0, X // 2, X - 1}):
            for y in sorted({0, Y // 2, Y - 1}):
                spots.add((b, x, y, Z - 1 if b % 2 else 0))
    tested = 0
    for spot in sorted(spots):
        if not keep[spot]:
            continue
        v = np.ravel_multi_index(spot, (B, X, Y, Z))
        g_q, g_ls = np.zeros_like(g_q0), np.zeros_like(g_ls0)
        g_q[v], g_ls[v] = g_q0[v], g_ls0[v]
        want, _, babs = ref.vjp(p.w, p.x, g_q, g_ls, None, se_idx=2)
        check(p, p.grad(g_q, g_ls, None), want, babs, 1.0, (name, spot))
        tested += 1
    assert tested >= 0.8 * len(spots)


@pytest.mark.parametrize("name", ["crop", "crop-exact"])
def test_real_gradients_of_an_outlier_under_small_sigma(params, oracle32, name):
    """elbo_bwd's head gradients on a crop batch with one outlier voxel and the log sigma head biased to e^-11: max
    |g_ls| passes 2^22, so the deltas that reach the 3x3 backward-data products (the heads' and the gate's factors are
    ~1e-2 here) pass f16's 65504 too, and the gradient still matches the float64 VJP of the same head gradients."""
    p = make_path(params, oracle32, name)
    p.w = dict(p.w, bs=np.full(11, -11.0, np.float32))
    p.ew.set_from_arrays(p.w)
    x = p.x.reshape(-1, 11).copy()
    x[p.n // 2] *= 1.3      # the outlier: a signal 30 % off the model
    p.x = x.reshape(p.x.shape)
    n = p.n
    mask = np.ones(n, np.float32)
    prior = np.tile(np.array([[-0.5, -1.0, -2.5, -1.0, 0.0]], np.float32), (n, 1))
    q, ls = p.forward()
    sums, gq, gls, _ = p.ctx.elbo_bwd(dev(x), dev(mask), q, dev(prior), ls, 1, 8, seed=5)
    torch.cuda.synchronize()
    g_q, g_ls, s = gq.double().cpu().numpy(), gls.double().cpu().numpy(), sums.cpu().numpy()
    assert np.abs(g_ls).max() > 2.0 ** 22
    _, reach, _ = p.reference(g_q, g_ls)
    keep = ref.keep_mask(reach, p.x.shape[:4])
    assert keep[n // 2] and keep.mean() >= 0.8
    g_q, g_ls = g_q * keep[:, None], g_ls * keep[:, None]
    want, _, babs = ref.vjp(p.w, p.x, g_q, g_ls, None, se_idx=2)
    check(p, p.grad(g_q, g_ls, float(s[2])), want, babs, 1.0 / float(s[2]), name)


@pytest.mark.parametrize("names", [("crop", "crop-bf16", "crop-exact"),
                                   ("voxel-block", "voxel-layerwise", "voxel-layerwise-bf16", "voxel-layerwise-exact")])
def test_selections_take_their_own_kernels(params, oracle32, names):
    """The same weights, batch and head gradients under each selection: the gradients differ bit for bit between every
    pair (as test_gpu_spatial.py's nine-tap comparison asserts), so a dispatch change that routed several selections to
    one kernel would be noticed -- while each is within EPS of the float64 VJP (test_scale_sweep)."""
    grads = []
    for name in names:
        p = make_path(params, oracle32, name)
        g_q, g_ls = heads(np.random.default_rng(1), p.n, p.stream)
        grads.append(p.grad(g_q, g_ls, 1.1e5))
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            assert not np.array_equal(grads[a], grads[b]), (names[a], names[b])


@pytest.mark.parametrize("kind", ["crop", "voxel"])
def test_training_forward_operand_range(params, oracle32, oracle64, kind):
    """Block-0 activations of one batch element pushed past 65504 come out NaN in q and log sigma, never as finite
    numbers; the other elements stay finite and match the oracle, and activations just below 65504 keep float32
    parity -- the training forwards' guard of the split-f16 operands, as test_split_operand_range for inference.  The
    large activation comes from the data (a weight beyond 65504 would be out of range for every voxel)."""
    from qbold_vi_amd.ops import Context, EncoderWeights, TrainState
    ctx = Context(params, full_model=True, include_blood=True)
    B, X, Y, Z, bad, w00 = 3, 6, 5, 4, 1, 8192.0
    for target, poisoned in ((7e4, True), (6e4, False)):
        # block 0's unit 0 = w00 log(x_0 / x_2): target on element `bad`, exactly 0 elsewhere
        x = signals(oracle32, (B, X, Y, Z), seed=5).astype(np.float32)
        x[..., 0] = x[..., 2]
        x[bad, ..., 0] = x[bad, ..., 2] * np.float32(np.exp(target / w00))
        w = weights(60, 2, True)
        w["W0"][:, 0] = 0.0
        w["W0"][0, 0] = w00
        w["b0"][0] = 0.0
        # what unit 0 feeds stays moderate (~6), so the later layers' activations stay inside f16's range too
        w["Wc"][0, 0, :] *= 1e-3
        w["Wr1"][0, :, :, 0, :] *= 1e-3
        ew = EncoderWeights(ctx, 11, 60, 2, True, -3.0, spatial_taps=9).set_from_arrays(w)
        st = TrainState(ctx, ew)
        if kind == "crop":
            q, ls = st.forward_spatial(dev(x))
            o2, sg = oracle64.encoder_fwd_spatial(w, x)
        else:
            q, ls = st.forward(dev(x.reshape(-1, 11)), 2)
            _, o2, sg = oracle64.encoder_fwd(w, x.reshape(-1, 11))
        q = q.cpu().numpy().reshape(B, X, Y, Z, 5)
        ls = ls.cpu().numpy().reshape(B, X, Y, Z, 11)
        o2, lsw = o2.reshape(B, X, Y, Z, 5), np.log(sg).reshape(B, X, Y, Z, 11)
        for b in range(B):
            if b == bad and poisoned:
                assert np.all(np.isnan(q[b])) and np.all(np.isnan(ls[b])), (kind, int(np.isfinite(q[b]).sum()))
                continue
            assert np.all(np.isfinite(q[b])) and np.all(np.isfinite(ls[b])), ("finite", kind, target, b)
            assert np.abs(q[b] - o2[b]).max() <= 1e-4 * max(np.abs(o2[b]).max(), 1.0), ("q", kind, target, b)
            assert np.abs(ls[b] - lsw[b]).max() <= 1e-4 * max(np.abs(lsw[b]).max(), 1.0), ("ls", kind, target, b)


def test_fixed_point_sums_propagate_nan(params):
    """qbold_smoothness's TV sum and qbold_hyper_prior_bwd's four inverse-gamma statistics are 64-bit fixed-point sums:
    a NaN in q comes out NaN (not finite garbage); finite inputs give the same bits run to run and match a float64
    sum (the non-finite flag leaves every finite partial's integer as it was)."""
    from qbold_vi_amd.ops import Context
    ctx = Context(params, full_model=True, include_blood=True)
    rng = np.random.default_rng(3)
    B, X, Y, Z = 2, 6, 5, 3
    q = rng.normal(size=(B, X, Y, Z, 5)).astype(np.float32)
    mask = np.ones((B, X, Y, Z), np.float32)
    tv = float(ctx.smoothness(dev(q), dev(mask)))
    assert np.isfinite(tv)
    assert tv == float(ctx.smoothness(dev(q), dev(mask)))
    qn = q.copy()
    qn[1, 2, 3, 1, 0] = np.nan
    assert np.isnan(float(ctx.smoothness(dev(qn), dev(mask))))
    ig = (3.0, 2.0, 2.5, 0.5)
    qv = q.reshape(-1, 5)
    stats = ctx.hyper_prior_bwd(dev(qv), ig).cpu().numpy()
    assert np.all(np.isfinite(stats))
    v = np.exp(2.0 * (3.0 * np.tanh(qv[:, [1, 3]].astype(np.float64)) - 1.0))
    want = np.array([np.log(v[:, 0]).sum(), (1 / v[:, 0]).sum(), np.log(v[:, 1]).sum(), (1 / v[:, 1]).sum()])
    assert np.allclose(stats, want, rtol=1e-5, atol=1e-3)
    qn = qv.copy()
    qn[7, 1] = np.nan
    qn[9, 3] = np.nan
    stats = ctx.hyper_prior_bwd(dev(qn), ig).cpu().numpy()
    assert np.all(np.isnan(stats))
