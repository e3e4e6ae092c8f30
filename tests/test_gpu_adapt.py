"""qbold_adapt_posterior (adapt_kernel) against the float64 restatement of tests/_adapt_reference.py on the cases of
tests/_adapt_cases.py: 48 voxels (a full 32-voxel block and half a block), masks mixing 0, 0.5, 1 and one NaN, the
reference's 11 taus (mirrored pairs), odd33 (T % 4 != 0), off22_3img (off-grid spin echo, three-image normalisation) and
64 taus, (rounds, K) = (1, 8), (3, 20), (6, 64).

Bounds.  Round 0 is qbold_log_evidence_fwd's arithmetic and is held to its bounds (test_gpu_log_evidence.py): log p^
1e-4 rel_1, ESS 1e-4 relative.  From round 1 on the proposal itself carries the rounding of the rounds before it, so log
p^, ESS and the proposals are held to 4 x their float32 floor (tests/test_adapt_host.test_float32_floors computes it from
the float32 oracle; nothing of the kernel enters it), never below the round-0 bound.  MEASUREMENTS.md section 32 has the
floors and the measured worst ratios."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import _adapt_cases as ac
import _adapt_reference as ar
import _laplace_reference as lr
import test_gpu_forward_protocols as fp
from _iw_reference import rel, rel1

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

dev, _same_bits = fp.dev, fp._same_bits
_RUNS = {}


def run(params, name):
    """The case, its context, device inputs (NaN data in the masked voxels) and the kernel's outputs; once per case."""
    if name not in _RUNS:
        from qbold_vi_amd.ops import Context
        c = ac.build(params, name)
        ctx = Context(c.p, True, True, **c.sw)
        x = c.x.copy()
        x[~c.live] = np.nan
        t = dict(x=dev(x), mask=dev(c.mask), q=dev(c.q), prior=dev(c.prior), sigma=dev(c.sigma))
        kw = dict(rounds=c.R, K=c.K, shrink=ac.SHRINK, seed=c.seed, voxel0=ac.VOXEL0)
        q_out, out, q_rounds = ctx.adapt_posterior(*t.values(), want_rounds=True, **kw)
        torch.cuda.synchronize()
        _RUNS[name] = dict(c=c, ctx=ctx, t=t, kw=kw, q_out=q_out, out=out, q_rounds=q_rounds)
    return _RUNS[name]


def _got(r):
    c = r["c"]
    on = r["out"].cpu().numpy().astype(np.float64)[c.rows]
    return dict(log_p=on[:, 0:2 * c.R:2], ess=on[:, 1:2 * c.R:2], best=on[:, 2 * c.R].astype(int),
                flags=on[:, 2 * c.R + 1].astype(int), q_rounds=r["q_rounds"].cpu().numpy().astype(np.float64)[c.rows],
                q_out=r["q_out"].cpu().numpy().astype(np.float64)[c.rows])


def _check_rows(r):
    """what holds for every case: masked rows, finite live rows, q_out = the row of q_rounds that out names (bits)"""
    c = r["c"]
    dead, live = dev(~c.live), dev(c.live)
    assert r["out"].shape == (ac.N_VOX, 2 * c.R + 2) and r["q_rounds"].shape == (ac.N_VOX, c.R, 5)
    assert torch.isnan(r["out"][dead]).all() and torch.isnan(r["q_rounds"][dead]).all()
    assert _same_bits(r["q_out"][dead], r["t"]["q"][dead])
    assert torch.isfinite(r["out"][live]).all() and torch.isfinite(r["q_rounds"][live]).all()
    assert torch.isfinite(r["q_out"]).all()
    best = r["out"][live, 2 * c.R].long()
    assert ((best >= 0) & (best < c.R)).all()
    named = r["q_rounds"][live][torch.arange(best.numel(), device="cuda"), best]
    assert _same_bits(r["q_out"][live], named)
    # round 0's proposal is the given heads, bit for bit
    assert _same_bits(r["q_rounds"][live][:, 0], r["t"]["q"][live])
    # the returned round has the largest ESS, the earliest on ties
    ess = r["out"][live][:, 1:2 * c.R:2]
    first = (ess == ess.max(1, keepdim=True).values).float().argmax(1)
    assert torch.equal(best, first)


@pytest.mark.parametrize("name", ac.PARITY)
def test_matches_float64_reference_round_by_round(params, name):
    r = run(params, name)
    c = r["c"]
    _check_rows(r)
    got, ref = _got(r), c.ref
    e = ac.errors(got, ref)
    b0 = (ac.ROUND0["log_p"], ac.ROUND0["ess"], ac.ROUND0["q"])
    fails = []
    print(f"[adapt] {name} round 0: log_p {e[0, 0]:.3e} ess {e[0, 1]:.3e} q {e[0, 2]:.3e} (bounds {b0})")
    fails += [(0, k, v, b) for k, v, b in zip(("log_p", "ess", "q"), e[0], b0) if not v <= b]
    if c.R > 1:
        bl = ac.later_round_bounds(name)
        floor = ac.FLOORS[name]
        worst = e[1:].max(0)
        print(f"[adapt] {name} rounds 1..{c.R - 1}: log_p {worst[0]:.3e} ess {worst[1]:.3e} q {worst[2]:.3e}; floors "
              f"{floor}; ratios to the floor {tuple(round(float(w / f), 2) for w, f in zip(worst, floor))}; bounds {bl}")
        for rr in range(1, c.R):
            fails += [(rr, k, v, b) for k, v, b in zip(("log_p", "ess", "q"), e[rr], bl) if not v <= b]
    assert not fails, fails
    # the returned round and heads, away from near ties of the reference's ESS
    clear = ~ar.near_tie(ref["ess"])
    assert clear.mean() >= 0.95
    assert np.array_equal(got["best"][clear], ref["best"][clear])
    qb = ac.ROUND0["q"] if c.R == 1 else ac.later_round_bounds(name)[2]
    eq = ar.proposal_error(got["q_out"][clear], ref["q_out"][clear])
    print(f"[adapt] {name} q_out: {eq.max():.3e} on {int(clear.sum())} of {clear.size} voxels; flags "
          f"{np.bincount(got['flags'], minlength=8)} (reference {np.bincount(ref['flags'], minlength=8)})")
    assert eq.max() <= qb
    assert np.all(got["flags"] & 1 == 0)


@pytest.mark.parametrize("name", ("ref11_R1_K8", "ref11_R3_K20", "odd33_R6_K64", ac.REACH))
def test_explicit_normals_equal_to_the_stream_give_the_same_bits(params, name):
    r = run(params, name)
    c, ctx, t, kw = r["c"], r["ctx"], r["t"], r["kw"]
    z = ctx.normals(ac.N_VOX, c.R * c.K, stream_id=ar.STREAM_ADAPT, seed=c.seed, voxel0=ac.VOXEL0)
    # the oracle's restatement of the stream (the reference's draws) is the kernel's
    assert np.max(np.abs(z.cpu().numpy() - c.z)) <= 1e-5
    q2, o2, r2 = ctx.adapt_posterior(*t.values(), z=z, want_rounds=True, **dict(kw, seed=999, voxel0=5))
    assert _same_bits(q2, r["q_out"]) and _same_bits(o2, r["out"]) and _same_bits(r2, r["q_rounds"])
    # other draws are another answer
    q3, o3 = ctx.adapt_posterior(*t.values(), **dict(kw, seed=c.seed + 1))
    assert not torch.equal(torch.nan_to_num(o3), torch.nan_to_num(r["out"]))


@pytest.mark.parametrize("name", (ac.REACH, "full64_R6_K64", "off22_3img_R3_K20"))
def test_reproducible_and_independent_of_the_sharding(params, name):
    r = run(params, name)
    c, ctx, t, kw = r["c"], r["ctx"], r["t"], r["kw"]
    if name == ac.REACH:   # voxels over the reach bound of the whitened form sit in both shards
        over = fp.kl_reach(c.q) >= fp.LOGIT_CLIP
        assert (over & c.live)[:ac.N_VOX // 3].any() and (over & c.live)[ac.N_VOX // 3:].any()
    args = list(t.values())
    q2, o2, r2 = ctx.adapt_posterior(*args, want_rounds=True, **kw)
    assert _same_bits(q2, r["q_out"]) and _same_bits(o2, r["out"]) and _same_bits(r2, r["q_rounds"])
    for h in (1, ac.N_VOX // 3, 32, 47):
        qa, oa, ra = ctx.adapt_posterior(*[a[:h] for a in args], want_rounds=True, **kw)
        qb, ob, rb = ctx.adapt_posterior(*[a[h:] for a in args], want_rounds=True, **dict(kw, voxel0=ac.VOXEL0 + h))
        assert _same_bits(torch.cat([qa, qb]), r["q_out"]), h
        assert _same_bits(torch.cat([oa, ob]), r["out"]), h
        assert _same_bits(torch.cat([ra, rb]), r["q_rounds"]), h
    # without q_rounds the other outputs keep their bits; mask None evaluates every voxel and keeps the live rows' bits
    q4, o4 = ctx.adapt_posterior(*args, **kw)
    assert _same_bits(q4, r["q_out"]) and _same_bits(o4, r["out"])
    q5, o5 = ctx.adapt_posterior(dev(c.x), None, *args[2:], **kw)
    live = dev(c.live)
    assert _same_bits(q5[live], r["q_out"][live]) and _same_bits(o5[live], r["out"][live])
    assert torch.isfinite(o5).all()


@pytest.mark.parametrize("name", ac.EDGES + (ac.REACH,))
def test_clip_and_clamp_edges(params, name):
    r = run(params, name)
    c = r["c"]
    _check_rows(r)
    got, ref = _got(r), c.ref
    e = ac.errors(got, ref)
    print(f"[adapt] {name}: per round (log_p, ess, q) against float64\n{e}\n  flags {np.bincount(got['flags'], minlength=8)}"
          f" (reference {np.bincount(ref['flags'], minlength=8)})")
    assert np.all(got["flags"] & 1 == 0)
    for bit in (2, 4):   # set where the reference sets them
        want = (ref["flags"] & bit) != 0
        assert np.all((got["flags"][want] & bit) != 0), (bit, np.nonzero(want & ((got["flags"] & bit) == 0))[0])
    if name == "ref11_clip_R3_K20":
        assert (ref["flags"] & 2).any()
    if name == "odd33_saturated_R3_K20":
        assert (ref["flags"] & 4).any()
    # every proposal is a member of the family: means inside the clip, raw spread heads finite
    qr = got["q_rounds"]
    assert np.all(np.abs(qr[:, 1:, [0, 2]]) <= fp.LOGIT_CLIP + 1e-6)
    assert np.all(np.abs(np.tanh(qr[:, 1:, [1, 3, 4]])) <= 1.0 - 0.99e-6)


def test_bad_arguments_and_unsupported_contexts(params):
    from qbold_vi_amd import _lib
    from qbold_vi_amd.ops import Context
    r = run(params, "ref11_R3_K20")
    ctx, t = r["ctx"], r["t"]
    n = 32
    x, q, prior, sigma = (t[k][:n].contiguous() for k in ("x", "q", "prior", "sigma"))
    x = torch.nan_to_num(x, nan=1.0)
    q_out, out = torch.empty((n, 5), device="cuda"), torch.empty((n, 2 * 16 + 2), device="cuda")
    P = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None   # noqa: E731
    nan, inf = float("nan"), float("inf")

    def call(cx, rounds=3, K=20, shrink=4.0, xx=x, qq=q, pp=prior, ss=sigma, qo=q_out, oo=out, cfg=True, N=n):
        cf = _lib.AdaptCfg(rounds, K, shrink)
        return cx.lib.qbold_adapt_posterior(cx.handle, P(xx), None, P(qq), P(pp), P(ss), None,
                                            C.byref(cf) if cfg else None, 1, 0, P(qo), P(oo), None, N, None)
    assert call(ctx) == _lib.QBOLD_OK
    torch.cuda.synchronize()
    for bad in (0, -1, 17):
        assert call(ctx, rounds=bad) == -1, bad
    for bad in (0, 4, 7, 22, 1028, 2048, -8):
        assert call(ctx, K=bad) == -1, bad
    for bad in (0.0, -1.0, nan, inf):
        assert call(ctx, shrink=bad) == -1, bad
    assert call(ctx, rounds=16, K=8) == _lib.QBOLD_OK and call(ctx, rounds=1, K=1024) == _lib.QBOLD_OK
    assert call(ctx, xx=None) == -1 and call(ctx, qq=None) == -1 and call(ctx, pp=None) == -1 and call(ctx, ss=None) == -1
    assert call(ctx, qo=None) == -1 and call(ctx, oo=None) == -1 and call(ctx, cfg=False) == -1 and call(ctx, N=-1) == -1
    assert call(ctx, N=0) == _lib.QBOLD_OK and call(ctx, N=0, xx=None, qq=None, pp=None, ss=None) == _lib.QBOLD_OK
    e = [torch.empty((0, w), device="cuda") for w in (11, 5, 5, 11)]
    q0, o0, r0 = ctx.adapt_posterior(e[0], torch.empty(0, device="cuda"), e[1], e[2], e[3], rounds=2, K=8,
                                     want_rounds=True)
    assert q0.shape == (0, 5) and o0.shape == (0, 6) and r0.shape == (0, 2, 5)
    with pytest.raises(ValueError, match="z must be"):
        ctx.adapt_posterior(x, None, q, prior, sigma, rounds=2, K=8, z=torch.zeros((n, 8, 2), device="cuda"))
    # configurations without a kernel
    lit = Context(params, True, True)
    lit.set_tissue_mode("literal")
    assert call(lit) == -3
    assert call(Context(params, True, True, student_t_df=4.0)) == -3
    assert call(Context(params, True, True, predict_log_data=True)) == -3
    assert call(Context(params, False, True)) == -3
    torch.cuda.synchronize()


def test_closing_the_loop_on_2048_voxels(params):
    """Start = the prior's own heads, 6 rounds of 64 draws.  Under the returned heads a fresh 256-draw evaluation
    (another stream, another seed) has a higher mean ESS, a lower median Pareto k^ and a smaller total distance of
    log p^ to posterior_grid's exact log p(x) than under the starting heads: inequalities between two runs of
    existing entry points."""
    from oracle.oracle import Oracle
    from qbold_vi_amd.ops import Context
    n = 2048
    d = lr.inputs(Oracle("f32", params), "ref11", n=n)
    ctx = Context(params, True, True)
    x, prior, sigma = dev(d["x"]), dev(d["prior"]), dev(d["sigma"])
    q_out, out = ctx.adapt_posterior(x, None, prior, prior, sigma, rounds=6, K=64, shrink=4.0, seed=5)
    assert torch.isfinite(out).all() and torch.isfinite(q_out).all()
    series = out[:, 1:12:2].mean(0).cpu().numpy()
    _, grid, _ = ctx.posterior_grid(x, None, prior, sigma)
    exact = grid[:, 0].double()
    inside = grid[:, 15] < 1e-6

    def evaluate(q):
        _, ev, _ = ctx.log_evidence(x, None, q, prior, sigma, 256, seed=77)
        lw, _ = ctx.log_evidence_draws(x, None, q, prior, sigma, 256, seed=77)
        po, _, _ = ctx.psis(lw)
        return (ev[:, 2].double().mean().item(), po[:, 0].double().median().item(),
                (ev[:, 0].double() - exact)[inside].abs().sum().item(), (po[:, 0] > 0.7).float().mean().item())
    before, after = evaluate(prior), evaluate(q_out)
    print(f"[adapt] closing the loop, {n} voxels at 11 taus: mean ESS of 64 per round {np.round(series, 2)}; fresh "
          f"256-draw mean ESS {before[0]:.2f} -> {after[0]:.2f}; median k^ {before[1]:.3f} -> {after[1]:.3f}; "
          f"share of k^ > 0.7 {before[3]:.3f} -> {after[3]:.3f}; sum |log p^ - log p(x)| over {int(inside.sum())} voxels "
          f"{before[2]:.2f} -> {after[2]:.2f}")
    assert inside.sum() >= n // 2
    assert after[0] > before[0]
    assert after[1] < before[1]
    assert after[2] < before[2]


@pytest.fixture(scope="module")
def trainer(params):
    from qbold_vi_amd import EncoderTrainer
    return EncoderTrainer(system_params=params, no_units=60, use_layer_norm=False, dropout_rate=0.0,
                          no_intermediate_layers=2, initial_im_sigma=0.05, activation_type='relu',
                          multi_image_normalisation=False, channelwise_gating=True, infer_inv_gamma=False,
                          use_population_prior=False, use_mvg=True, predict_log_data=False)


def _fine_tuner(tr, params, model=None):
    from qbold_vi_amd import SignalGenerationLayer
    if model is None:
        model, _ = tr.create_encoder(gate_offset=-3.0, resid_init_std=0.05, no_ip_images=11)
    return model, tr.build_fine_tuner(model, SignalGenerationLayer(dict(params, simulate_noise='False'), True, True))


def test_fine_tuner_adapt(trainer, params):
    from oracle.oracle import Oracle, synth_inputs
    model, ft = _fine_tuner(trainer, params)
    lead = (2, 6, 5, 4)
    nv = int(np.prod(lead))
    x, _ = synth_inputs(nv, params, seed=8, oracle=Oracle("f32", params))
    x5 = dev(x).reshape(lead + (11,))
    m5 = dev((np.random.default_rng(8).uniform(size=nv) > 0.3).astype(np.float32)).reshape(lead + (1,))
    p5 = model(x5)[0]
    _, q5, sg5 = model.predict(x5, want=("out2", "sigma"))
    flat = (x5.reshape(-1, 11), m5.reshape(-1), None, p5.reshape(-1, 5), sg5.reshape(-1, 11))
    live = m5.reshape(-1) > 0
    for start, q0 in ((None, q5.reshape(-1, 5)), ("prior", p5.reshape(-1, 5)), (q5 + 0.01, (q5 + 0.01).reshape(-1, 5))):
        got = ft.adapt(x5, m5, p5, q=start, rounds=3, no_samples=16, seed=4, voxel0=9)
        q_w, o_w = trainer.context.adapt_posterior(flat[0], flat[1], q0.contiguous(), flat[3], flat[4], rounds=3, K=16,
                                                   seed=4, voxel0=9)
        assert got["q"].shape == lead + (5,) and _same_bits(got["q"].reshape(-1, 5), q_w)
        assert got["log_evidence"].shape == lead + (3,) and got["ess"].shape == lead + (3,)
        assert _same_bits(got["log_evidence"].reshape(-1, 3), o_w[:, 0:6:2].contiguous())
        assert _same_bits(got["ess"].reshape(-1, 3), o_w[:, 1:6:2].contiguous())
        assert got["best"].shape == lead and got["flags"].shape == lead
        assert torch.equal(got["best"].reshape(-1)[live], o_w[live, 6].to(torch.int32))
        assert torch.equal(got["flags"].reshape(-1)[live], o_w[live, 7].to(torch.int32))
        assert (got["best"].reshape(-1)[~live] == -1).all() and (got["flags"].reshape(-1)[~live] == 0).all()
        assert torch.isfinite(got["ess"].reshape(-1, 3)[live]).all()
    # the heads go to the entries that take q
    q = got["q"]
    assert np.isfinite(float(ft.elbo(x5, m5, p5, no_samples=4, seed=2, q=q)["elbo"]))
    iw = ft.log_evidence(x5, m5, p5, no_samples=32, seed=2, q=q, psis=True)
    assert torch.isfinite(iw["log_evidence"].reshape(-1)[live]).all()
    # qbold_psis answers k^ = +inf where a tail of 32 draws has no finite Pareto fit, NaN only for a row it cannot read
    assert not torch.isnan(iw["khat"].reshape(-1)[live]).any()
    assert torch.isfinite(ft.posterior_grid(x5, m5, p5, q=q)["elbo"].reshape(-1)[live]).all()
    assert torch.isfinite(ft.posterior_predictive(x5, m5, q=q, no_samples=16)["ppp"].reshape(-1)[live]).all()
    assert torch.isfinite(trainer.calculate_means(q, None)).all()
    with pytest.raises(ValueError, match="adapt"):
        ft.adapt(x5, m5, p5, q="encoder")
    with pytest.raises(ValueError, match="adapt_posterior"):
        ft.adapt(x5, m5, p5, no_samples=10)


def test_save_predictions_writes_the_adapt_maps(trainer, params, tmp_path):
    from oracle.oracle import Oracle, synth_inputs
    from qbold_vi_amd import nifti
    model, ft = _fine_tuner(trainer, params)
    B, X, Y, Z = 2, 6, 5, 4
    x, _ = synth_inputs(B * X * Y * Z, params, seed=12, oracle=Oracle("f32", params))
    mask = (np.random.default_rng(1).uniform(size=(B * X * Y * Z, 1)) > 0.2).astype(np.float32)
    data = dev(np.concatenate([x, mask], -1)).reshape(B, X, Y, Z, 12)
    priors = model(data[..., :-1])[0]
    d0, d1, d2 = tmp_path / "plain", tmp_path / "adapt", tmp_path / "adapt_iw"
    for d in (d0, d1, d2):
        os.makedirs(d)
    assert trainer.save_predictions(model, data, str(d0 / "sub"), fine_tuner_model=ft, priors=priors,
                                    adapt_rounds=None) is None
    _, ft1 = _fine_tuner(trainer, params, model)   # a fresh fine tuner: its sampling layer counts its calls
    maps = trainer.save_predictions(model, data, str(d1 / "sub"), fine_tuner_model=ft1, priors=priors, adapt_rounds=3)
    names = ("oef_adapt", "dbv_adapt", "r2p_adapt", "ess_adapt")
    extra = {f"sub_{k}.nii.gz" for k in names}
    plain = set(os.listdir(d0))
    assert set(os.listdir(d1)) == plain | extra and not (plain & extra)
    for f in plain:   # the earlier maps are unchanged, byte for byte (gzip stamps the time, so compare the content)
        with gzip.open(d0 / f, "rb") as a, gzip.open(d1 / f, "rb") as b:
            assert a.read() == b.read(), f
    live = mask.reshape(B, X, Y, Z) > 0
    assert set(maps) == set(names)
    for k in names:
        v = maps[k].cpu().numpy()
        assert v.shape == (B, X, Y, Z, 1) and np.all(np.isfinite(v)), k
        assert np.all(v[..., 0][~live] == 0.0), k
        img = nifti.load(str(d1 / f"sub_{k}.nii.gz"))[0]
        np.testing.assert_array_equal(img, np.concatenate(np.split(v, B, axis=0), axis=-1)[0])
    oef = maps["oef_adapt"].cpu().numpy()[..., 0][live]
    ess = maps["ess_adapt"].cpu().numpy()[..., 0][live]
    assert np.all((oef > 0.04) & (oef < 0.84)) and np.all((ess > 0.0) & (ess <= 1.0 + 1e-6))
    # with iw_samples and psis the importance maps are taken under the adapted heads
    _, ft2 = _fine_tuner(trainer, params, model)
    both = trainer.save_predictions(model, data, str(d2 / "sub"), fine_tuner_model=ft2, priors=priors, adapt_rounds=3,
                                    iw_samples=32, psis=True)
    ad = ft2.adapt(data[..., :-1], data[..., -1:], priors, rounds=3, seed=trainer._seed + 61)
    assert _same_bits(both["oef_adapt"], maps["oef_adapt"])
    iw = ft2.log_evidence(data[..., :-1], data[..., -1:], priors, no_samples=32, seed=trainer._seed + 31, psis=True,
                          q=ad["q"])
    lv = dev(live)
    assert _same_bits(both["khat"][..., 0][lv], iw["khat"][lv])
    assert {"khat", "logevidence", "ess", "ess_adapt"} <= set(both)
    with pytest.raises(ValueError, match="fine tuner"):
        trainer.save_predictions(model, data, str(d1 / "none"), adapt_rounds=3)
