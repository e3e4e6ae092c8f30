"""Host-side checks of the importance-weighted evidence: the float64 reference the GPU tests hold
qbold_log_evidence_fwd to (tests/_iw_reference.py), the C ABI entry, and the sums helper.  No GPU needed."""
import numpy as np
import pytest

from _iw_reference import iw_reference, log_weights


@pytest.fixture(scope="module")
def inputs(params):
    from oracle.oracle import Oracle, init_weights, synth_inputs
    o32 = Oracle("f32", params)
    n = 64
    x, _ = synth_inputs(n, params, seed=5, oracle=o32)
    w = init_weights(T=11, U=60, L=2, seed=3)
    w["gate_offset"] = -3.0
    prior, q, sigma = o32.encoder_fwd(w, x)
    return x, q, prior, sigma


def test_reference_at_one_draw_is_the_oracle_elbo_on_that_draw(oracle64, inputs):
    """K = 1: log p^ = ELBO_same = log w = -(nll + log q - log p) of the draw, which is what the oracle's ELBO gives
    when its one likelihood draw and its one KL draw are the same normals."""
    x, q, prior, sigma = inputs
    n = x.shape[0]
    z = np.random.default_rng(2).standard_normal((n, 1, 2))
    ref = iw_reference(oracle64, x, q, prior, sigma, z)
    want = oracle64.elbo(x, np.ones(n), q, prior, sigma, z, z)
    np.testing.assert_allclose(ref["log_p"], -(want["nll_v"] + want["kl_v"]), rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(ref["log_p"], ref["elbo"])
    np.testing.assert_allclose(ref["ess"], 1.0, rtol=0, atol=1e-15)
    y = oracle64.reparam(q, z.reshape(n, 2))
    np.testing.assert_allclose(ref["means"][:, :2], y, rtol=1e-12)


def test_reference_bound_and_ess_range(oracle64, inputs):
    x, q, prior, sigma = inputs
    n, K = x.shape[0], 16
    z = np.random.default_rng(3).standard_normal((n, K, 2))
    ref = iw_reference(oracle64, x, q, prior, sigma, z)
    assert np.all(ref["log_p"] >= ref["elbo"])
    assert np.all((ref["ess"] >= 1.0) & (ref["ess"] <= K * (1 + 1e-12)))
    # the K draws one at a time give the per-draw log weights
    lw1, _ = log_weights(oracle64, x, q, prior, sigma, z[:, 3:4])
    np.testing.assert_allclose(ref["lw"][:, 3], lw1[:, 0], rtol=1e-13)


def test_abi_declares_the_entry_point():
    import os
    from qbold_vi_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "qbold_hip.h")) as f:
        hdr = f.read()
    assert "int qbold_log_evidence_fwd(" in hdr and "#define QBOLD_IW_MAX_K" in hdr
    assert "#define QBOLD_ABI_VERSION 5" in hdr
    res, args = _lib.SIGNATURES["qbold_log_evidence_fwd"]
    assert len(args) == 16


def test_log_evidence_from_sums():
    torch = pytest.importorskip("torch")
    from qbold_vi_amd import distributed as qd
    sums = torch.tensor([-30.0, -26.0, 4.0], dtype=torch.float64)
    lp, el, gap = qd.log_evidence_from_sums(sums)
    assert float(lp) == 7.5 and float(el) == 6.5 and float(gap) == 1.0


def test_fine_tuner_log_evidence_rejects_the_diagonal_family(params):
    """use_mvg=False: a different density (exp(raw_s), model.py:696-698); refused before any device work."""
    from qbold_vi_amd.model import FineTuner

    class _Tr:
        _use_mvg = False
        _heteroscedastic_noise = True
        _use_population_prior = False
        _mog_components = 1
        _seed = 1

    ft = FineTuner(_Tr(), None, None)
    with pytest.raises(NotImplementedError, match="use_mvg"):
        ft.log_evidence(None, None, None)
