"""qbold_elbo_bwd on protocols other than the reference's two: elbo_bwd_generic_kernel (any 1 <= T <= 64) against
central differences of the float64 oracle, against the generic forward, against the specialised T = 11 / 24 kernels
under QBOLD_KSEL_ELBO_BWD_GENERIC, under sharding, and through the fine-tuning loop."""
import configparser
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KSEL_ELBO_BWD_GENERIC = 8388608   # QBOLD_KSEL_ELBO_BWD_GENERIC
LOGIT_CLIP = 13.815509557963774   # QB_LOGIT_CLIP
Z_MAX = 4.8549                    # QB_Z_MAX


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def protocol(params, T):
    """tau grids of the tests: 12 / 33 taus after test_one_launch_wide_encoder_on_partly_filled_tau_tiles, 22 taus
    with no tau equal to 0 (the spin-echo index lands on -1 ms), BASELINE config 3's 64, the reference's 11 and 24."""
    if T == 11:
        return dict(params)
    if T == 24:
        return dict(params, tau_start="-0.028", tau_end="0.065", tau_step="0.004")
    if T == 22:
        return dict(params, tau_start="-0.017", tau_end="0.071", tau_step="0.004")
    if T == 64:
        return dict(params, tau_start="-0.015", tau_end="0.065", tau_step="0.00125")
    return dict(params, tau_start="-0.010", tau_end=str(-0.010 + 0.001 * T - 0.0005), tau_step="0.001")


class _Setup:
    def __init__(self, params, T, **variant):
        from oracle.oracle import Oracle
        from qbold_vi_amd.ops import Context
        self.p = protocol(params, T)
        self.ctx = Context(self.p, True, True, **variant)
        self.ctx.set_grad_node0(False)   # gradients as exact derivatives of the forward value, as test_gpu_grad's ctx
        self.o32 = Oracle("f32", self.p, **variant)
        self.o64 = Oracle("f64", self.p, node0_zero=True, **variant)
        assert self.ctx.T == self.o32.T == self.o64.T == T


@pytest.fixture(scope="module")
def setup(params):
    from oracle.oracle import Oracle
    cache = {}

    def get(T, **variant):
        key = (T, tuple(sorted(variant.items())))
        if key not in cache:
            cache[key] = _Setup(params, T, **variant)
        return cache[key]
    yield get
    Oracle("f64", params).lib.qbo_set_node0_zero(0)   # the policy is process-global in the C library


def kl_stopgrad(o, q_sample, q_logq, prior, zk):
    """mean_k [log q_sg(y_k) - log p(y_k)], y_k = reparam(q_sample, z_k): the q-parameters inside
    log q are stop-gradient in the reference (model.py:596), so finite differences must vary the
    sampling parameters only."""
    K = zk.shape[1]
    acc = 0.0
    for k in range(K):
        y = o.reparam(q_sample, zk[:, k])
        acc = acc + o.logit_mvn_nlogp(y, prior) - o.logit_mvn_nlogp(y, q_logq)
    return acc / K


_cases = {}


def _case(o32, T, n, seed):
    """test_gpu_grad._case at T taus; computed once per (T, n, seed) and handed out as copies."""
    from oracle.oracle import init_weights, synth_inputs
    key = (T, n, seed)
    if key not in _cases:
        w = init_weights(T=T, U=60, L=2, seed=seed)
        w["gate_offset"] = -3.0
        x, _ = synth_inputs(n, seed=seed, oracle=o32)
        prior, q, sigma = o32.encoder_fwd(w, x)
        rng = np.random.default_rng(seed)
        q = (q + rng.normal(size=q.shape) * 0.3).astype(np.float32)   # posterior away from the prior
        mask = (rng.uniform(size=n) > 0.25).astype(np.float32)
        _cases[key] = (x, mask, q, prior, sigma)
    return tuple(a.copy() for a in _cases[key])


def rel1(a, b):
    return np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))


def kl_reach(q):
    """The kernels' bound on a voxel's logits, |mu| + QB_Z_MAX (|c| + e^s): below QB_LOGIT_CLIP the clip cannot bind and
    the KL takes the whitened five-moment form."""
    q = q.astype(np.float64)
    e_so, e_sd = np.exp(3.0 * np.tanh(q[:, 1]) - 1.0), np.exp(3.0 * np.tanh(q[:, 3]) - 1.0)
    c = np.tanh(q[:, 4]) * np.exp(-2.0)
    return np.maximum(np.abs(q[:, 0]) + Z_MAX * e_so, np.abs(q[:, 2]) + Z_MAX * (np.abs(c) + e_sd))


@pytest.mark.parametrize("T,S,K,multi", [(T, S, K, False) for T in (12, 33, 22, 64) for S, K in ((1, 70), (3, 7))] +
                         [(22, 1, 70, True)])
def test_generic_head_gradients_vs_oracle_fd(setup, T, S, K, multi):
    """All five heads and log sigma at t in {0, se, se + 1, T - 1} against central differences (h = 1e-4) of the
    float64 oracle, test_elbo_head_gradients_vs_oracle_fd's method and bound; S = 1: one lane per voxel, S = 3: four.
    40 voxels: a partial wave in either mapping."""
    s = setup(T, multi_image_normalisation=True) if multi else setup(T)
    ctx, o32, o64 = s.ctx, s.o32, s.o64
    n, seed = 40, 11
    x, mask, q, prior, sigma = _case(o32, T, n, 5)
    assert 0 < (mask == 0).sum() < n
    ls = np.log(sigma.astype(np.float64))
    zs = o32.philox_normals(seed, 0, 0, n, S)
    zk = o32.philox_normals(seed, 1, 0, n, K)
    q64 = q.astype(np.float64)

    def loss_v(qq, lss):
        e = o64.elbo(x, mask, qq, prior, np.exp(lss), zs, zk)
        return e["nll_v"] * mask + np.where(mask > 0, kl_stopgrad(o64, qq, q64, prior, zk), 0.0)

    sums, gq, gls, nk = ctx.elbo_bwd(dev(x), dev(mask), dev(q), dev(prior), dev(ls.astype(np.float32)), S, K, seed=seed)
    gq, gls = gq.cpu().numpy(), gls.cpu().numpy()
    want = o32.elbo(x, mask, q, prior, sigma, zs, zk)
    got = (sums[0] + sums[1]).item() / sums[2].item()
    print(f"T={T} S={S} K={K} multi={multi}: elbo {got:.6f} oracle {want['elbo']:.6f}")
    assert abs(got - want["elbo"]) < 1e-4 * abs(want["elbo"])
    h = 1e-4
    for k in range(5):
        d = np.zeros_like(q64)
        d[:, k] = h
        fd = (loss_v(q64 + d, ls) - loss_v(q64 - d, ls)) / (2 * h)
        scale = np.abs(fd).max() + 1e-3
        err = np.max(np.abs(gq[:, k] - fd)) / scale
        print(f"  head {k}: {err:.2e}")
        assert err < 2e-3, (k, err, scale)
    se = ctx.se_idx
    for t in (0, se, se + 1, T - 1):
        d = np.zeros_like(ls)
        d[:, t] = h
        fd = (loss_v(q64, ls + d) - loss_v(q64, ls - d)) / (2 * h)
        scale = np.abs(fd).max() + 1e-3
        err = np.max(np.abs(gls[:, t] - fd)) / scale
        print(f"  log sigma {t}: {err:.2e}")
        assert err < 2e-3, (t, err, scale)
    # masked-out voxels carry no gradient
    assert np.abs(gq[mask == 0]).max() == 0.0 and np.abs(gls[mask == 0]).max() == 0.0


@pytest.mark.parametrize("T", [33, 64])
def test_backward_value_is_the_forward_value(setup, T):
    """The per-voxel (nll, kl) rows of the backward against Context.elbo_fwd on the same seed: the same Philox words,
    so DESIGN section 2's stream bound at S = 1 (2e-4 rel_1) holds between the two kernels."""
    s = setup(T)
    n, S, K, seed = 40, 1, 70, 17
    x, mask, q, prior, sigma = _case(s.o32, T, n, 5)
    ls = np.log(sigma.astype(np.float64)).astype(np.float32)
    _, _, _, nk = s.ctx.elbo_bwd(dev(x), dev(mask), dev(q), dev(prior), dev(ls), S, K, seed=seed)
    _, want = s.ctx.elbo_fwd(dev(x), dev(mask), dev(q), dev(prior), dev(np.exp(ls)), S, K, seed=seed)
    err = rel1(nk.cpu().numpy().astype(np.float64), want.cpu().numpy().astype(np.float64))
    print(f"T={T}: backward nll_kl against forward, rel1 {err:.2e}")
    assert err < 2e-4


@pytest.mark.parametrize("clip_bound", [False, True])
def test_generic_kl_only_gradient_is_exact(setup, clip_bound):
    """Likelihood switched off numerically (sigma = e^12), T = 33, S = 2, K = 40: the KL's gradient alone, with
    test_elbo_gradient_kl_only_is_exact's bound.  clip_bound: |mu_oef| pushed out to 4.2 posterior standard deviations
    below the logit clip, so that reach = |mu| + 4.8549 e^s crosses QB_LOGIT_CLIP (the clipped general loop runs) while
    no draw of this stream reaches the clip itself (the clip passes gradient, a finite difference would not)."""
    T = 33
    s = setup(T)
    n, S, K, seed = 32, 2, 40, 3
    x, mask, q, prior, sigma = _case(s.o32, T, n, 7)
    mask[:] = 1.0
    ls = np.full((n, T), 12.0)
    zk = s.o32.philox_normals(seed, 1, 0, n, K)
    e_so = np.exp(3.0 * np.tanh(q[:, 1].astype(np.float64)) - 1.0)
    e_sd = np.exp(3.0 * np.tanh(q[:, 3].astype(np.float64)) - 1.0)
    c = np.tanh(q[:, 4].astype(np.float64)) * np.exp(-2.0)
    if clip_bound:
        sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        q[:, 0] = (sign * (LOGIT_CLIP - 4.2 * e_so)).astype(np.float32)
    reach = kl_reach(q)
    if clip_bound:
        assert np.all(reach >= LOGIT_CLIP)
        a = q[:, 0:1].astype(np.float64) + e_so[:, None] * zk[:, :, 0]
        b = q[:, 2:3].astype(np.float64) + c[:, None] * zk[:, :, 0] + e_sd[:, None] * zk[:, :, 1]
        assert max(np.abs(a).max(), np.abs(b).max()) < LOGIT_CLIP - 1e-3   # the bound is crossed, the clip is not
    else:
        assert np.all(reach < LOGIT_CLIP)
    q64 = q.astype(np.float64)

    def loss_v(qq):
        return kl_stopgrad(s.o64, qq, q64, prior, zk)

    _, gq, _, _ = s.ctx.elbo_bwd(dev(x), dev(mask), dev(q), dev(prior), dev(ls.astype(np.float32)), S, K, seed=seed)
    gq = gq.cpu().numpy()
    for k in range(5):
        d = np.zeros_like(q64)
        d[:, k] = 1e-5
        fd = (loss_v(q64 + d) - loss_v(q64 - d)) / 2e-5
        err = np.max(np.abs(gq[:, k] - fd))
        print(f"clip_bound={clip_bound} head {k}: {err:.2e} of {np.abs(fd).max():.3e}")
        assert err < 2e-4 * (np.abs(fd).max() + 1.0), k


# d = max |g_gen - g_spec| / (max |g_spec| + 1e-3): the two kernels differ in the order of the gradient sums only, a few
# float32 roundings of the largest term (above 2.5e-5 something else would differ).  The bound is four times the value
# measured on the MI355X and never looser than 1e-4; None = not measured yet (MEASUREMENTS.md section 17), which leaves
# the cap.
GENERIC_VS_SPECIALISED_MEASURED = None
GENERIC_VS_SPECIALISED_BOUND = 1e-4 if GENERIC_VS_SPECIALISED_MEASURED is None else min(4 * GENERIC_VS_SPECIALISED_MEASURED, 1e-4)


@pytest.mark.parametrize("S,K", [(1, 70), (4, 10)])
@pytest.mark.parametrize("T", [11, 24])
def test_generic_kernel_against_the_specialised_one(params, T, S, K):
    """QBOLD_KSEL_ELBO_BWD_GENERIC routes T = 11 / 24 through elbo_bwd_generic_kernel: the same draws on the same
    lanes, the same value arithmetic and -- at these two T -- the specialised kernels' per-wave choice of the KL form
    (the T = 11 inputs hold voxels over the reach bound, so both forms run), so the sums agree to 1e-8; the gradients
    are summed in another order."""
    from oracle.oracle import Oracle
    from qbold_vi_amd.ops import Context
    p = protocol(params, T)
    spec, gen = Context(p, True, True), Context(p, True, True)
    gen.set_kernel_selection(KSEL_ELBO_BWD_GENERIC)
    n, seed = 300, 23
    x, mask, q, prior, sigma = _case(Oracle("f32", p), T, n, 9)
    ls = np.log(sigma.astype(np.float64)).astype(np.float32)
    args = (dev(x), dev(mask), dev(q), dev(prior), dev(ls), S, K)
    s0, gq0, gl0, nk0 = spec.elbo_bwd(*args, seed=seed)
    s1, gq1, gl1, nk1 = gen.elbo_bwd(*args, seed=seed)
    s0, s1 = s0.cpu().numpy(), s1.cpu().numpy()
    ds = np.max(np.abs(s1 - s0) / np.abs(s0))
    dv = rel1(nk1.cpu().numpy().astype(np.float64), nk0.cpu().numpy().astype(np.float64))
    d = 0.0
    for g1, g0 in ((gq1, gq0), (gl1, gl0)):
        g1, g0 = g1.cpu().numpy().astype(np.float64), g0.cpu().numpy().astype(np.float64)
        d = max(d, np.max(np.abs(g1 - g0)) / (np.abs(g0).max() + 1e-3))
    print(f"T={T} S={S} K={K}: sums rel {ds:.2e}, nll_kl rel1 {dv:.2e}, gradients d = {d:.3e}")
    assert ds < 1e-8
    assert d < GENERIC_VS_SPECIALISED_BOUND


def test_generic_sharding_raggedness_reproducibility(setup, params):
    """T = 33, N = 333: one call equals three calls on [0, 100) / [100, 101) / [101, 333) with voxel0 set, bit for bit;
    two identical calls are bit-equal; N = 0 returns zero sums; Student-t at T = 33 is QBOLD_ERR_UNSUPPORTED.
    A few of the voxels are over the reach bound of the whitened KL (checked here): the form a voxel takes must be
    its own, not that of the voxels that share its wave, which the shards regroup."""
    from qbold_vi_amd._lib import QboldError
    from qbold_vi_amd.ops import Context
    T = 33
    s = setup(T)
    n, seed = 333, 29
    x, mask, q, prior, sigma = _case(s.o32, T, n, 13)
    ls = np.log(sigma.astype(np.float64)).astype(np.float32)
    over = kl_reach(q) >= LOGIT_CLIP
    assert 0 < over.sum() < 10 and over[101:].any()   # mixed waves, and the shards move their boundaries
    for S, K in ((1, 70), (3, 7)):
        t = [dev(a) for a in (x, mask, q, prior, ls)]
        s_all, gq, gl, nk = s.ctx.elbo_bwd(*t, S, K, seed=seed)
        s_again, gq2, gl2, nk2 = s.ctx.elbo_bwd(*t, S, K, seed=seed)
        assert torch.equal(gq, gq2) and torch.equal(gl, gl2) and torch.equal(nk, nk2) and torch.equal(s_all, s_again)
        parts = np.zeros(3)
        for lo, hi in ((0, 100), (100, 101), (101, 333)):
            sp, gqp, glp, nkp = s.ctx.elbo_bwd(*[a[lo:hi] for a in t], S, K, seed=seed, voxel0=lo)
            assert torch.equal(gqp, gq[lo:hi]) and torch.equal(glp, gl[lo:hi]) and torch.equal(nkp, nk[lo:hi]), (S, lo)
            parts += sp.cpu().numpy()
        assert np.allclose(parts, s_all.cpu().numpy(), rtol=1e-6, atol=0)
    e = [torch.empty((0, w), device="cuda") for w in (T, 5, 5, T)]
    s0, gq0, gl0, _ = s.ctx.elbo_bwd(e[0], torch.empty(0, device="cuda"), e[1], e[2], e[3], 1, 70)
    assert s0.cpu().tolist() == [0.0, 0.0, 0.0] and gq0.shape == (0, 5) and gl0.shape == (0, T)
    ct = Context(s.p, True, True, student_t_df=2)
    with pytest.raises(QboldError, match=r"status -3: qbold_elbo_bwd: for T other than 11 / 24 only"):
        ct.elbo_bwd(dev(x), dev(mask), dev(q), dev(prior), dev(ls), 1, 70)


def test_finetune_weight_gradient_directional_at_12_taus(setup):
    """test_finetune_weight_gradient_directional at T = 12, U = 24, L = 1: d/dw of the masked-mean negative ELBO through
    encoder stream 2 + sampling along random directions, against the float64 oracle; that test's tolerance."""
    from oracle.oracle import WEIGHT_NAMES, init_weights, synth_inputs
    from qbold_vi_amd.ops import EncoderWeights, TrainState
    T, U, L, cw = 12, 24, 1, False
    s = setup(T)
    ctx, o32, o64 = s.ctx, s.o32, s.o64
    w = init_weights(T=T, U=U, L=L, channelwise_gating=cw, seed=3)
    rng = np.random.default_rng(3)
    for k in ("b0", "bc", "br1", "br2", "bg", "bf"):
        w[k] = (rng.standard_normal(w[k].shape) * 0.1).astype(np.float32)
    w["gate_offset"] = -1.0
    ew = EncoderWeights(ctx, T, U, L, cw, -1.0).set_from_arrays(w)
    n, S, K, seed = 256, 2, 6, 21
    x, _ = synth_inputs(n, seed=6, oracle=o32)
    rng = np.random.default_rng(1)
    mask = (rng.uniform(size=n) > 0.2).astype(np.float32)
    prior = o32.encoder_fwd(w, x)[0]
    st = TrainState(ctx, ew)
    q2, ls = st.forward(dev(x), 2)
    sums, gq, gls, _ = ctx.elbo_bwd(dev(x), dev(mask), q2, dev(prior), ls, S, K, seed=seed)
    grad = st.backward(2, gq, gls, sums).cpu().numpy().astype(np.float64)
    zs = o32.philox_normals(seed, 0, 0, n, S)
    zk = o32.philox_normals(seed, 1, 0, n, K)
    q_fixed = o64.encoder_fwd(w, x)[1]

    def perturbed(direction, eps):
        out = dict(w)
        for k, d in direction.items():
            out[k] = w[k].astype(np.float64) + eps * d
        return out

    def loss(ww):
        _, qq, sg = o64.encoder_fwd(ww, x)
        e = o64.elbo(x, mask, qq, prior, sg, zs, zk)
        kl = kl_stopgrad(o64, qq, q_fixed, prior, zk)
        return ((e["nll_v"] * mask).sum() + np.where(mask > 0, kl, 0).sum()) / mask.sum()

    for trial in range(4):
        direction = {k: rng.standard_normal(w[k].shape) for k in WEIGHT_NAMES}
        if trial == 1:   # sigma head only
            for k in WEIGHT_NAMES:
                if k not in ("Ws", "bs"):
                    direction[k] *= 0
        if trial == 2:   # residual branch only
            for k in WEIGHT_NAMES:
                if k not in ("Wr1", "br1", "Wr2", "br2", "Wg", "bg"):
                    direction[k] *= 0
        dflat = EncoderWeights(ctx, T, U, L, cw, -1.0).set_from_arrays(
            {k: direction[k].astype(np.float32) for k in WEIGHT_NAMES}).flat.cpu().numpy().astype(np.float64)
        eps = 2e-6
        fd = (loss(perturbed(direction, eps)) - loss(perturbed(direction, -eps))) / (2 * eps)
        got = float(grad @ dflat)
        print(f"trial {trial}: got {got:.6f} fd {fd:.6f}")
        assert abs(got - fd) < 1e-2 * (abs(fd) + 0.05), (trial, got, fd)


def test_train_model_on_a_20_tau_protocol(tmp_path, monkeypatch):
    """Both phases of training.train_model on a protocol of 20 taus (-16 .. 60 ms in 4 ms steps) read from an INI
    `config` in the working directory; tau_weighted = False because the reference defines its per-tau SNR profile for
    11 / 24 taus only."""
    from qbold_vi_amd import training
    from qbold_vi_amd.utils import load_arguments
    ini = configparser.ConfigParser()
    ini.read(os.path.join(ROOT, "config"))
    for k, v in dict(tau_start="-0.016", tau_end="0.064", tau_step="0.004", tau_weighted="False").items():
        ini["DEFAULT"][k] = v
    with open(tmp_path / "config", "w") as f:
        ini.write(f)
    monkeypatch.chdir(tmp_path)   # the INI `config` is read from the CWD, as in the reference
    cfg = load_arguments(["train.py", os.path.join(ROOT, "configurations", "optimal.yaml")], entry="train")
    cfg.update(no_units=24, no_intermediate_layers=1, no_pt_epochs=20, no_ft_epochs=3,
               save_directory=str(tmp_path / "run"), synthetic_voxels=20000, mc_samples=2)
    model, trainer, hist = training.train_model(cfg, pt_sample_size=200)
    assert trainer.context.T == 20
    pt = [h for h in hist if "val_oef_metric" in h]
    ft = [h for h in hist if "val_elbo" in h]
    assert len(pt) == 20 and len(ft) == 3
    assert all(np.isfinite(h["loss"]) for h in hist)
    for h in ft:
        for k in ("val_nll", "val_elbo", "val_elbo_smooth", "val_smoothness", "val_smoothness_scaled", "val_kl"):
            assert k in h and np.isfinite(h[k]), (k, h)
        assert abs(h["val_elbo"] - (h["val_nll"] + h["val_kl"])) < 1e-9
    print("fine-tuning losses", [h["loss"] for h in ft])
    assert ft[-1]["loss"] < ft[0]["loss"]
