"""Gradient of the importance-weighted bound on any tau grid (qbold_log_evidence_bwd_anyt, iw_bwd_generic_kernel;
Context.log_evidence_bwd(kernel=...)) and iw_samples fine-tuning on a protocol that is not the reference's: the head
gradients and `out` against the float64 references on the eight protocols of tests/test_gpu_forward_protocols.py, the
Philox stream, the bitwise structure, the run-time-T kernel against the specialised one at 11 / 24 taus, the C ABI's
errors, an optimisation check and a training run at 20 taus.

The float64 reference's own distance to central differences of the oracle on these protocols is held without a GPU by
tests/test_iw_bwd_anyt_host.py; the bounds here are those of tests/test_gpu_iw_grad.py."""
import configparser
import ctypes as C
import os

import numpy as np
import pytest

import _refine_anyt_cases as rc
import test_gpu_forward_protocols as fp
from _iw_grad_reference import LOGIT_CLIP, iw_grad_reference, logits
from _iw_reference import iw_reference, rel, rel1

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "qbold_log_evidence_bwd_anyt"
IW_STREAM = 6
ERR_INVALID, ERR_UNSUPPORTED = -1, -3
N_REF = 48               # a partial wave in either lane mapping; two blocks at four lanes per voxel (32 voxels each)
KS = (1, 7, 32, 40)      # one lane per voxel up to 32, four beyond
dev, _same_bits = fp.dev, fp._same_bits


def ref_mask(n):
    """0, 0.5 and 1"""
    i = np.arange(n)
    return np.where(i % 5 == 2, 0.0, np.where(i % 3 == 0, 0.5, 1.0)).astype(np.float32)


def normals(n, K):
    return np.random.default_rng(K).standard_normal((n, K, 2)).astype(np.float32)


def tensors(d, n=None):
    """x, q, prior, log_sigma on the device"""
    sl = slice(None, n)
    return (dev(d["x"][sl]), dev(d["q"][sl]), dev(d["prior"][sl]), dev(np.log(d["sigma"][sl]).astype(np.float32)))


def column_errors(got, want):
    """max |d| per column over the column's max |ref| + 1e-3 (test_gpu_iw_grad.py)"""
    got = got.cpu().numpy().astype(np.float64)
    return [np.abs(got[:, k] - want[:, k]).max() / (np.abs(want[:, k]).max() + 1e-3) for k in range(want.shape[1])]


def log_sigma64(d):
    """sigma as the kernel has it: exp of the float32 log sigma it is given"""
    return np.exp(np.log(d["sigma"]).astype(np.float32).astype(np.float64))


# ---- 1. the float64 reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", list(fp.PROTOCOLS))
def test_matches_float64_reference(params, name, K):
    """Explicit normals, 48 voxels under a mask of 0 / 0.5 / 1.  With node 0's slope off: every column of g_q and
    g_log_sigma within 2e-3 of the column's scale against the reference with central-difference Jacobians.  Under the
    default policy: every live entry <= 2e-4 A against the reference with the oracle's analytic Jacobian.  Masked rows
    are exact zeros on both paths (with `out`, where a masked voxel is still scored, and without)."""
    from _elbo_bwd_reference import analytic_jac
    d = rc.case(params, name, N_REF)
    n = N_REF
    mask = ref_mask(n)
    z = normals(n, K)
    x, q, prior, ls = tensors(d)
    sigma = log_sigma64(d)
    dead = mask == 0
    with rc.float64_oracle(d) as o64:
        ref_fd = iw_grad_reference(o64, d["x"], d["q"], d["prior"], sigma, z, mask=mask)
        ref_an = iw_grad_reference(o64, d["x"], d["q"], d["prior"], sigma, z, mask=mask, jac=analytic_jac)
    c = fp.context(d)
    c.set_grad_node0(False)
    _, gq, gls, out = c.log_evidence_bwd(x, dev(mask), q, prior, ls, K, z=dev(z), want_out=True)
    assert out.shape == (n, 3) and bool(torch.isfinite(out).all())
    for what, got, want in (("g_q", gq, ref_fd["g_q"]), ("g_log_sigma", gls, ref_fd["g_log_sigma"])):
        errs = column_errors(got, want)
        print(f"{name} K={K} node0 off {what}: worst column {max(errs):.2e}")
        assert bool((got[dev(dead)] == 0).all()) and not bool(torch.signbit(got[dev(dead)]).any())
        assert max(errs) < 2e-3, (name, K, what, errs)
    c = fp.context(d)   # the shipped policy: a context whose grad_node0 nobody set
    _, gq, gls, _ = c.log_evidence_bwd(x, dev(mask), q, prior, ls, K, z=dev(z))
    worst = {}
    for what, got, want, A in (("g_q", gq, ref_an["g_q"], ref_an["A_q"]),
                               ("g_log_sigma", gls, ref_an["g_log_sigma"], ref_an["A_ls"])):
        assert bool((got[dev(dead)] == 0).all()) and not bool(torch.signbit(got[dev(dead)]).any())
        got = got.cpu().numpy().astype(np.float64)
        worst[what] = float(np.max(np.abs(got - want)[~dead] / A[~dead]))
    print(f"{name} K={K} default policy: worst |d| / A  g_q {worst['g_q']:.2e}  g_log_sigma {worst['g_log_sigma']:.2e}")
    assert worst["g_q"] <= 2e-4 and worst["g_log_sigma"] <= 2e-4, (name, K, worst)


@pytest.mark.parametrize("K", [7, 40])
def test_clipped_draws_match_float64_reference(params, K):
    """odd33 with heads near the logit clip and wide spreads (test_gpu_iw_grad._case(wide=True)): some draws reach the
    clip, so the clipped form of log q - log p runs beside the whitened one; the column bound of the first test."""
    d = rc.case(params, "odd33", N_REF)
    n = N_REF
    rng = np.random.default_rng(3)
    q = d["q"].copy()
    q[:, 0] += np.where(rng.uniform(size=n) < 0.5, -12.5, 12.5)
    q[:, 1] = 0.5
    q[:, 3] = 0.5
    q = q.astype(np.float32)
    z = normals(n, K)
    clipped = np.abs(logits(q, z)).max(-1) > LOGIT_CLIP
    print(f"K={K}: {int(clipped.sum())} of {clipped.size} draws reach the clip")
    assert clipped.any() and not clipped.all()
    x, _, prior, ls = tensors(d)
    c = fp.context(d)
    c.set_grad_node0(False)
    _, gq, gls, _ = c.log_evidence_bwd(x, None, dev(q), prior, ls, K, z=dev(z))
    with rc.float64_oracle(d) as o64:
        ref = iw_grad_reference(o64, d["x"], q, d["prior"], log_sigma64(d), z)
    for what, got, want in (("g_q", gq, ref["g_q"]), ("g_log_sigma", gls, ref["g_log_sigma"])):
        errs = column_errors(got, want)
        print(f"wide heads K={K} {what}: worst column {max(errs):.2e}")
        assert max(errs) < 2e-3, (K, what, errs)


# ---- 2. out against float64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fp.PROTOCOLS))
def test_out_matches_float64_reference(params, name):
    """(log p^, ELBO_same, ESS) against _iw_reference.iw_reference within fp.IW_TOL, what the any-T forward is held to,
    at K = 1, 7, 40 on explicit normals; the distance to Context.log_evidence on the same Philox draws is printed."""
    d = rc.case(params, name, N_REF)
    n = N_REF
    x, q, prior, ls = tensors(d)
    sigma = log_sigma64(d)
    c = fp.context(d)
    fails = []
    with rc.float64_oracle(d) as o64:
        for K in (1, 7, 40):
            z = normals(n, K)
            ref = iw_reference(o64, d["x"], d["q"], d["prior"], sigma, z, d["p"])
            sums, _, _, out = c.log_evidence_bwd(x, None, q, prior, ls, K, z=dev(z), want_out=True)
            out, sums = out.cpu().numpy().astype(np.float64), sums.cpu().numpy()
            errs = dict(log_p=rel1(out[:, 0], ref["log_p"]), elbo=rel1(out[:, 1], ref["elbo"]),
                        ess=rel(out[:, 2], ref["ess"]))
            print(f"[iw bwd any-T] out {name} K={K}", " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
            fails += [(name, K, k, v) for k, v in errs.items() if not v <= fp.IW_TOL[k]]
            want = np.array([-out[:, 0].sum(), -out[:, 1].sum(), float(n)])
            assert np.all(np.abs(sums - want) <= 1e-8 * np.abs(want)), (name, K, sums, want)
    s1, _, _, o1 = c.log_evidence_bwd(x, None, q, prior, ls, 16, seed=4, voxel0=9, want_out=True)
    s2, o2, _ = c.log_evidence(x, None, q, prior, torch.exp(ls), 16, seed=4, voxel0=9)
    a, b = o1.cpu().numpy(), o2.cpu().numpy()
    print(f"[iw bwd any-T] {name} K=16 against Context.log_evidence at the same seed: out rel1",
          " ".join(f"{rel1(a[:, j], b[:, j]):.2e}" for j in range(3)),
          f"sums {rel1(s1.cpu().numpy(), s2.cpu().numpy()):.2e}")
    assert not fails, fails


# ---- 3. the stream ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def odd33(params):
    d = rc.case(params, "odd33", 777)
    c = fp.context(d)
    c.set_grad_node0(False)
    return c, tensors(d)


@pytest.mark.parametrize("K", [1, 7, 16, 40])
def test_philox_stream_equals_explicit_normals(odd33, K):
    c, (x, q, prior, ls) = odd33
    seed, v0 = 11, 12345
    a = c.log_evidence_bwd(x, None, q, prior, ls, K, seed=seed, voxel0=v0, want_out=True)
    z = c.normals(777, K, stream_id=IW_STREAM, seed=seed, voxel0=v0)
    b = c.log_evidence_bwd(x, None, q, prior, ls, K, z=z, seed=seed, voxel0=v0, want_out=True)
    for u, v in zip(a, b):
        assert _same_bits(u, v)


# ---- 4. bitwise structure --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 16, 40])
def test_bitwise_structure(odd33, K):
    c, t = odd33
    n = 333
    x, q, prior, ls = (a[:n] for a in t)
    kw = dict(seed=3, want_out=True)
    a = c.log_evidence_bwd(x, None, q, prior, ls, K, voxel0=100, **kw)
    b = c.log_evidence_bwd(x, None, q, prior, ls, K, voxel0=100, **kw)
    for u, v in zip(a, b):   # run to run
        assert _same_bits(u, v)
    parts = []               # three shards against one call
    for lo, hi in ((0, 100), (100, 101), (101, n)):
        parts.append(c.log_evidence_bwd(x[lo:hi], None, q[lo:hi], prior[lo:hi], ls[lo:hi], K, voxel0=100 + lo, **kw))
    for i in (1, 2, 3):
        assert _same_bits(torch.cat([p[i] for p in parts]), a[i]), i
    ssum = sum(p[0].cpu().numpy() for p in parts)
    assert np.all(np.abs(ssum - a[0].cpu().numpy()) <= 1e-9 * np.abs(a[0].cpu().numpy()))
    # a voxel moved to another batch position (its explicit normals move with it)
    z = c.normals(n, K, stream_id=IW_STREAM, seed=3, voxel0=100)
    perm = torch.as_tensor(np.random.default_rng(1).permutation(n), device="cuda")
    p = c.log_evidence_bwd(x[perm], None, q[perm], prior[perm], ls[perm], K, z=z[perm], want_out=True)
    for i in (1, 2, 3):
        assert _same_bits(p[i], a[i][perm]), i
    # masked and NaN-mask voxels: +0.0, nothing in the sums; m = 0.5 halves the gradients exactly
    m = np.ones(n, np.float32)
    m[::3] = 0.0
    m[1::7] = np.nan
    m[2::5] = 0.5
    md = dev(m)
    for want_out in (False, True):
        sm, gqm, glm, _ = c.log_evidence_bwd(x, md, q, prior, ls, K, seed=3, voxel0=100, want_out=want_out)
        out_ = torch.isnan(md) | (md <= 0)
        for g in (gqm, glm):
            assert bool((g[out_] == 0).all()) and not bool(torch.signbit(g[out_]).any())
        half, one = md == 0.5, md == 1.0
        assert _same_bits(gqm[half], a[1][half] * 0.5) and _same_bits(glm[half], a[2][half] * 0.5)
        assert _same_bits(gqm[one], a[1][one]) and _same_bits(glm[one], a[2][one])
        mm = md[~out_].double()
        lp = a[3][~out_, 0].double()
        assert float(sm[2]) == float(mm.sum())
        assert abs(float(sm[0]) + float((mm * lp).sum())) < 1e-9 * abs(float(sm[0]))
    e = [torch.empty((0, w), device="cuda") for w in (33, 5, 5, 33)]
    s0, g0, l0, o0 = c.log_evidence_bwd(e[0], None, e[1], e[2], e[3], K, want_out=True)
    assert s0.cpu().tolist() == [0.0, 0.0, 0.0] and g0.shape == (0, 5) and l0.shape == (0, 33) and o0.shape == (0, 3)


# ---- 5. the run-time-T kernel against the specialised one ----------------------------------------------------------
# d = max |g_gen - g_spec| / (max |g_spec| + 1e-3): the two kernels differ in the order of the gradient sums only, a few
# float32 roundings of the largest term.  The bound is four times the value measured on the MI355X and never looser
# than 1e-4 (tests/test_gpu_elbo_bwd_protocols.py's pattern); None = not measured yet, which leaves the cap.
# Measured: 1.951e-6 / 1.008e-6 (T = 11, K = 8 / 40), 1.596e-6 / 1.883e-6 (T = 24); MEASUREMENTS.md section 31.
GENERIC_VS_SPECIALISED_MEASURED = 1.951e-6
GENERIC_VS_SPECIALISED_BOUND = 1e-4 if GENERIC_VS_SPECIALISED_MEASURED is None else \
    min(4 * GENERIC_VS_SPECIALISED_MEASURED, 1e-4)


@pytest.mark.parametrize("K", [8, 40])
@pytest.mark.parametrize("name", ["ref11", "ref24"])
def test_generic_kernel_against_the_specialised_one(params, name, K):
    d = rc.case(params, name, 300)
    c = fp.context(d)
    assert c.T in (11, 24)
    x, q, prior, ls = tensors(d)
    mask = dev(d["mask"])
    kw = dict(seed=17, voxel0=5, want_out=True)
    s0, gq0, gl0, o0 = c.log_evidence_bwd(x, mask, q, prior, ls, K, kernel="auto", **kw)
    s1, gq1, gl1, o1 = c.log_evidence_bwd(x, mask, q, prior, ls, K, kernel="generic", **kw)
    live = d["live"]
    do = rel1(o1.cpu().numpy()[live], o0.cpu().numpy()[live])
    dg = 0.0
    for g1, g0 in ((gq1, gq0), (gl1, gl0)):
        g1, g0 = g1.cpu().numpy().astype(np.float64), g0.cpu().numpy().astype(np.float64)
        dg = max(dg, np.max(np.abs(g1 - g0)) / (np.abs(g0).max() + 1e-3))
    print(f"{name} K={K}: out rel1 {do:.2e}, sums rel1 {rel1(s1.cpu().numpy(), s0.cpu().numpy()):.2e}, "
          f"gradients d = {dg:.3e}")
    assert do < 1e-4
    assert dg < GENERIC_VS_SPECIALISED_BOUND


# ---- 6. errors through the C ABI -------------------------------------------------------------------------------------
def test_bad_arguments_and_unsupported(odd33, params):
    from qbold_vi_amd import _lib
    from qbold_vi_amd.ops import Context
    c, t = odd33
    n = 64
    x, q, prior, ls = (a[:n] for a in t)
    gq = torch.empty((n, 5), device="cuda")
    gls = torch.empty((n, 33), device="cuda")
    sums = torch.empty(3, dtype=torch.float64, device="cuda")
    P = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None   # noqa: E731

    def call(cx, K, g=gq, gl=gls, s=sums, xx=x):
        return getattr(cx.lib, ENTRY)(cx.handle, P(xx), None, P(q), P(prior), P(ls), None, int(K), 1, 0, P(g), P(gl),
                                      None, P(s), P(cx._workspace()), n, None)
    assert call(c, 0) == ERR_INVALID and call(c, -3) == ERR_INVALID and call(c, (1 << 30) + 1) == ERR_INVALID
    assert call(c, 8, g=None) == ERR_INVALID and call(c, 8, gl=None) == ERR_INVALID
    assert call(c, 8, s=None) == ERR_INVALID and call(c, 8, xx=None) == ERR_INVALID
    assert call(c, 8) == _lib.QBOLD_OK
    torch.cuda.synchronize()
    with pytest.raises(_lib.QboldError):
        c.log_evidence_bwd(x, None, q, prior, ls, 0)
    p33 = fp.protocol(params, "odd33")
    for sw, word in ((dict(student_t_df=5.0), "Student-t"), (dict(predict_log_data=True), "log")):
        other = Context(p33, True, True, **sw)
        assert call(other, 4) == ERR_UNSUPPORTED
        with pytest.raises(_lib.QboldError, match=word):
            other.log_evidence_bwd(x, None, q, prior, ls, 4)
    lit = Context(p33, True, True)
    lit.set_tissue_mode("literal")
    assert call(lit, 4) == ERR_UNSUPPORTED
    with pytest.raises(_lib.QboldError, match="literal"):
        lit.log_evidence_bwd(x, None, q, prior, ls, 4)
    with pytest.raises(ValueError):
        c.log_evidence_bwd(x, None, q, prior, ls, 4, kernel="fast")


# ---- 7. optimisation -------------------------------------------------------------------------------------------------
def test_sgd_on_the_gradient_raises_the_bound(params):
    """odd33, 4,096 synthetic voxels from noisy heads: 100 plain SGD steps on g_q with fresh seeds raise the mean
    log p^_16 on a seed no step used."""
    d = rc.case(params, "odd33", 4096)
    c = fp.context(d)
    x, q, prior, ls = tensors(d)
    sigma = torch.exp(ls)

    def mean_lp(qq):
        s, _, _ = c.log_evidence(x, None, qq, prior, sigma, 16, seed=999)
        return float(-s[0] / s[2])
    before = mean_lp(q)
    qq = q.clone()
    for j in range(100):
        _, gq, _, _ = c.log_evidence_bwd(x, None, qq, prior, ls, 16, seed=1 + j)
        qq = qq - 2e-4 * gq
    after = mean_lp(qq)
    print(f"odd33 mean log p^_16: {before:.4f} -> {after:.4f}")
    assert bool(torch.isfinite(qq).all()) and after > before


# ---- 8. training -----------------------------------------------------------------------------------------------------
def test_iw_samples_fine_tuning_on_a_20_tau_protocol(tmp_path, monkeypatch):
    """training.train_model with iw_samples = 8 on the 20-tau INI protocol of
    test_gpu_elbo_bwd_protocols.test_train_model_on_a_20_tau_protocol (-16 .. 60 ms in 4 ms steps, tau_weighted =
    False): both phases complete, every validation key is finite and the bound improves."""
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
    cfg.update(no_units=24, no_intermediate_layers=1, no_pt_epochs=10, no_ft_epochs=3,
               save_directory=str(tmp_path / "run"), synthetic_voxels=4096, mc_samples=1, iw_samples=8)
    _, trainer, hist = training.train_model(cfg, pt_sample_size=200)
    assert trainer.context.T == 20
    ft = [h for h in hist if "val_elbo" in h]
    assert len(ft) == 3
    for h in ft:
        assert "val_log_evidence" in h and "iw_elbo_same" in h
        for k, v in h.items():
            if k.startswith("val_") or k in ("iw_elbo_same", "loss"):
                assert np.isfinite(v), (k, h)
    print("fine-tuning losses", [h["loss"] for h in ft])
    assert ft[-1]["loss"] < ft[0]["loss"]
    assert ft[-1]["iw_elbo_same"] >= ft[-1]["loss"] - 1e-6   # -ELBO_same >= -log p^ draw by draw (Jensen)
