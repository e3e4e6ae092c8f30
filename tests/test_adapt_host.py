"""qbold_adapt_posterior without a GPU: the header, the binding and the build list; the argument checks that are raised
before any launch; the float64 restatement of tests/_adapt_reference.py against itself (the fixed point of the update,
the clamp rule against tests/_laplace_reference.heads_from, the properties the adaptation is for); the conditions the
GPU test puts on its cases (near ties under the cap, voxels over the reach bound present); and the float32 floors that
the GPU test's later-round bounds rest on."""
import math
import os
import re

import numpy as np
import pytest

import _adapt_cases as ac
import _adapt_reference as ar
import _laplace_reference as lr
from test_gpu_forward_protocols import LOGIT_CLIP, float64_oracle, kl_reach

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_binding_and_build_list_agree():
    from qbold_vi_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "qbold_hip.h")).read()
    assert re.search(r"#define QBOLD_ABI_VERSION 5\b", hdr)       # additions only
    assert re.search(r"typedef struct \{ int rounds; int K; float shrink; \} qbold_adapt_cfg;", hdr)
    args = re.search(r"int qbold_adapt_posterior\((.*?)\);", hdr, re.S).group(1)
    assert len(args.split(",")) == len(_lib.SIGNATURES["qbold_adapt_posterior"][1]) == 15
    assert [n for n, _ in _lib.AdaptCfg._fields_] == ["rounds", "K", "shrink"]
    for k in ("MAX_ROUNDS", "MIN_K", "MAX_K"):
        v = int(re.search(rf"#define QBOLD_ADAPT_{k} (\d+)", hdr).group(1))
        assert v == getattr(_lib, f"QBOLD_ADAPT_{k}") == dict(MAX_ROUNDS=16, MIN_K=8, MAX_K=1024)[k]
    dev_h = open(os.path.join(ROOT, "qbold_vi_amd", "csrc", "qbold_dev.h")).read()
    assert re.search(r"STREAM_ADAPT = 9,", dev_h) and ar.STREAM_ADAPT == 9
    assert "adapt_kernels.hip" in build.SOURCES
    assert hasattr(_lib.load(), "qbold_adapt_posterior")


def test_argument_checks_are_raised_before_any_launch(params):
    from qbold_vi_amd.ops import Context, QboldError
    ctx = Context(params, True, True, host_only=True)
    x, h5, sg = torch.ones(4, 11), torch.zeros(4, 5), torch.ones(4, 11)
    for kw in (dict(rounds=0), dict(rounds=17), dict(K=4), dict(K=1028), dict(K=22), dict(shrink=0.0),
               dict(shrink=-1.0), dict(shrink=float("nan")), dict(shrink=float("inf"))):
        with pytest.raises(ValueError, match="adapt_posterior"):
            ctx.adapt_posterior(x, None, h5, h5, sg, **kw)
    with pytest.raises(QboldError, match="no CPU fallback"):
        ctx.adapt_posterior(x, None, h5, h5, sg)


def test_fine_tuner_adapt_refuses_the_diagonal_family_and_the_population_prior():
    from qbold_vi_amd.model import FineTuner

    class _Tr:
        _use_mvg = False
        _heteroscedastic_noise = True
        _use_population_prior = False
        _mog_components = 1
        _seed = 1

    with pytest.raises(NotImplementedError, match="diagonal family"):
        FineTuner(_Tr(), None, None).adapt(None, None, None)
    _Tr._use_mvg = True
    _Tr._use_population_prior = True
    with pytest.raises(NotImplementedError, match="population prior"):
        FineTuner(_Tr(), None, None).adapt(None, None, None)


def test_the_proposal_does_not_move_when_the_weighted_moments_are_its_own():
    """Equal weights on a symmetric design: m_z = 0 and C_z = I by construction, so B = I, G = I and the update is the
    identity on every member of the family (heads inside the clamps)."""
    r2 = math.sqrt(2.0)
    design = np.array([[r2, 0.0], [-r2, 0.0], [0.0, r2], [0.0, -r2]] * 4)           # K = 16
    n = 12
    rng = np.random.default_rng(1)
    z = np.repeat(design[None], n, 0)
    st = ar.round_stats(np.full((n, 16), -37.5), z)
    assert np.allclose(st["m"], 0.0, atol=1e-15) and np.allclose(st["C"], [1.0, 0.0, 1.0], atol=1e-15)
    assert np.allclose(st["ess"], 16.0) and np.allclose(st["log_p"], -37.5)
    mu = rng.normal(0.0, 3.0, (n, 2))
    t = rng.uniform(-0.5, 0.9, (n, 3))    # halving e_so below stays inside the clamp
    mu2, t2, done, on_clip, clamped = ar.update(mu, t, st, 4.0)
    assert done.all() and not on_clip.any() and not clamped.any()
    assert np.max(np.abs(mu2 - mu)) <= 1e-15 and np.max(np.abs(t2 - t)) <= 1e-15
    # and a shifted, scaled design moves it to exactly that mean and factor as shrink -> 0
    zs = 0.5 * z + np.array([0.3, -0.2])
    st = ar.round_stats(np.zeros((n, 16)), zs)
    mu3, t3, *_ = ar.update(mu, t, st, 1e-12)
    e_so, e_sd, c = np.exp(3 * t[:, 0] - 1), np.exp(3 * t[:, 1] - 1), t[:, 2] * ar.EM2
    assert np.allclose(mu3[:, 0], mu[:, 0] + e_so * 0.3, rtol=1e-9)
    assert np.allclose(mu3[:, 1], mu[:, 1] + c * 0.3 + e_sd * -0.2, rtol=1e-9)
    assert np.allclose(np.exp(3 * t3[:, 0] - 1), 0.5 * e_so, rtol=1e-9)


def test_clamp_rule_is_laplace_heads_from():
    rng = np.random.default_rng(5)
    n = 300
    s_o, s_d = rng.uniform(-5.0, 2.5, n), rng.uniform(-5.0, 2.5, n)
    c = rng.uniform(-0.3, 0.3, n)
    Sigma = np.zeros((n, 2, 2))
    Sigma[:, 0, 0] = np.exp(2 * s_o)
    Sigma[:, 0, 1] = Sigma[:, 1, 0] = c * np.exp(s_o)
    Sigma[:, 1, 1] = c * c + np.exp(2 * s_d)
    q, clamped, t_raw = lr.heads_from(np.zeros((n, 2)), Sigma, want_t=True)
    t_so, t_sd, t_c, cl = ar.clamp_rule(s_o, s_d, c)
    assert 30 < cl.sum() < n - 30
    # a tanh value within float64 rounding of the clamp may be flagged by one and not the other
    edge = (np.abs(np.abs(t_raw) - lr.TANH_MAX) < 1e-12).any(1)
    assert np.array_equal(cl[~edge], clamped[~edge])
    want = np.tanh(q[:, [1, 3, 4]])
    assert np.max(np.abs(np.stack([t_so, t_sd, t_c], -1) - want)) < 1e-10


def test_adaptation_raises_the_ess_from_the_prior(params):
    """The float64 reference alone: _laplace_reference.inputs("ref11", n=64), start = the prior's heads, 6 rounds of 64
    draws, shrink 4."""
    from oracle.oracle import Oracle
    p, sw = lr.setup(params, "ref11")
    o32 = Oracle("f32", p, **sw)
    d = lr.inputs(o32, "ref11", n=64)
    rows = np.nonzero(d["live"])[0]
    x, sg, pr = d["x"][rows], d["sigma"][rows], d["prior"][rows]
    z = ar.normals(o32, 5, 0, 64, 6, 64)[rows]
    zf = o32.philox_normals(77, 6, 0, 64, 256)[rows]    # an unused seed, another stream
    with float64_oracle(p, sw) as o64:
        res = ar.adapt(o64, x, pr, pr, sg, z, 6, 64, 4.0)
        before = ar.fresh_ess(o64, x, pr, pr, sg, zf)
        after = ar.fresh_ess(o64, x, res["q_out"], pr, sg, zf)
    series = res["ess"].mean(0)
    print(f"[adapt] ref11 from the prior, {rows.size} voxels: mean ESS of 64 per round {np.round(series, 2)}; fresh "
          f"256-draw ESS before {before.mean():.2f} after {after.mean():.2f}; improved {np.mean(after > before):.2f}")
    assert np.all(np.isfinite(res["ess"])) and np.all(res["flags"] & 1 == 0)
    assert series[-1] > series[0]
    assert after.mean() > before.mean()
    # the returned round is the one with the largest ESS, the earliest on ties
    assert np.array_equal(res["best"], np.argmax(res["ess"], 1))
    assert np.array_equal(res["q_out"], res["q_rounds"][np.arange(rows.size), res["best"]])


@pytest.mark.parametrize("name", list(ac.CASES))
def test_case_conditions(params, name):
    """Conditions on the inputs and the float64 reference alone."""
    c = ac.build(params, name)
    assert c.x.shape[0] == c.q.shape[0] == ac.N_VOX
    m = c.mask
    assert np.isnan(m).sum() == 1 and (m == 0).sum() > 0 and (m == 0.5).sum() > 0 and (m == 1).sum() > 0
    assert c.live[:32].any() and c.live[32:].any() and not c.live[:32].all()
    assert c.K % 4 == 0 and c.z.shape == (ac.N_VOX, c.R * c.K, 2)
    ref = c.ref
    assert np.all(np.isfinite(ref["log_p"])) and np.all(np.isfinite(ref["ess"])) and np.all(np.isfinite(ref["q_out"]))
    assert np.all(ref["flags"] & 1 == 0)
    ties = ar.near_tie(ref["ess"])
    print(f"[adapt] {name}: near ties {int(ties.sum())} of {c.rows.size}; flags {np.bincount(ref['flags'], minlength=8)}")
    if name in ac.PARITY:
        assert ties.mean() <= 0.05
    over = kl_reach(c.q[c.rows]) >= LOGIT_CLIP
    if name == ac.REACH:
        assert 3 <= over.sum() < c.rows.size // 2
        h = ac.N_VOX // 3   # the GPU test's shards each hold one
        assert over[c.rows < h].any() and over[c.rows >= h].any()
    if name in ac.PARITY:
        assert not over.any()
    if name == "ref11_clip_R3_K20":
        assert (ref["flags"] & 2).any() or np.any(np.abs(c.q[c.rows][:, [0, 2]]) > 13.0)
    if name == "odd33_saturated_R3_K20":
        assert (ref["flags"] & 4).any()


@pytest.mark.parametrize("name", list(ac.FLOORS))
def test_float32_floors(params, name):
    """The same composition on the float32 oracle with float32 update arithmetic against the float64 run: what float32
    alone does to the rounds after the first.  The recorded floors (the GPU test holds the kernel to 4 x them, never
    below the round-0 bound) are not above what is measured here."""
    c = ac.build(params, name, want_f32=True)
    e = ac.errors(c.f32, c.ref)
    worst = e[1:].max(0)
    print(f"[adapt] {name} float32 floor: round 0 {e[0, :2]}; later rounds log_p {worst[0]:.3e} ess {worst[1]:.3e} "
          f"q {worst[2]:.3e}; recorded {ac.FLOORS[name]}; bounds {ac.later_round_bounds(name)}")
    for got, rec in zip(worst, ac.FLOORS[name]):
        assert rec <= 1.05 * got, (name, rec, got)
    assert set(ac.FLOORS) == {n for n in ac.PARITY if ac.CASES[n][1] > 1}
