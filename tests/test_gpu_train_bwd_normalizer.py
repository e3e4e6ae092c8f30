"""The gelu, layer-norm and dropout backward (train_bwd_gelu, train_bwd_norm and the norm_* kernels) against the float64
VJP of tests/_train_bwd_reference.py, per weight tensor and per GroupNormalization row: max |hip - ref| <= EPS max |ref|
(biases and GroupNormalization rows: over the larger of that and their cancellation bound).  The shapes are the smallest
that leave the first iteration of each loop of the row, group and parameter-partial kernels (_train_bwd_reference.py,
NORM_CASES).  The dropout keep factors of the step come from the oracle (Oracle.dropout_factors) at the seed the
forward used.

relu cases on voxel batches (group = one voxel) keep the per-voxel relu screen; relu + layer-norm crop cases cannot be
screened (the group sums carry every voxel's delta to every site of its crop) and run at seeds for which the float64
forward has no relu site within 1e-5 rms of zero -- asserted before anything is compared; gelu needs no screen.

Worst ratios measured on an MI355X are in MEASUREMENTS.md ("Normalizer and gelu backward against a float64 VJP")."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _train_bwd_reference as ref  # noqa: E402
from test_gpu_train_bwd_reference import Path, check, heads  # noqa: E402

EPS = ref.EPS


class NormPath(Path):
    """A NORM_CASES entry on the default kernel selection."""

    def __init__(self, params, oracle32, oracle64, name, layer_norm=None):
        _, stream, act, _, rate = ref.NORM_CASES[name][:5]
        w, ln, x = ref.norm_case(name, oracle32)
        if layer_norm is False:
            ln = None
        super().__init__(params, 0, w, x, stream, activation=act, ln=ln, dropout_rate=rate, oracle=oracle64)
        self.name = name
        self.grouped = self.ln is not None and self.crops and int(np.prod(x.shape[1:4])) > 1

    def screened(self, g_q, g_ls, min_keep=0.8):
        """gelu: nothing to screen.  relu with groups of one voxel: the per-voxel screen.  relu + layer norm on crops:
        the band must be empty."""
        if self.act == "gelu":
            grads, _, babs = self.reference(g_q, g_ls)
            return g_q, g_ls, grads, babs
        if self.grouped:
            grads, reach, babs = self.reference(g_q, g_ls)
            assert (reach < 0).all(), ("relu sites in the band", int((reach >= 0).sum()))
            return g_q, g_ls, grads, babs
        return super().screened(g_q, g_ls, min_keep)


def case(params, oracle32, oracle64, name, seed=1):
    p = NormPath(params, oracle32, oracle64, name)
    g_q, g_ls = heads(np.random.default_rng(seed), p.n, p.stream)
    return (p,) + p.screened(g_q, g_ls)


@pytest.mark.parametrize("name", list(ref.NORM_CASES))
def test_every_tensor_within_eps(params, oracle32, oracle64, name):
    """One forward and one backward at the same step: every weight tensor and every GroupNormalization row finite and
    within EPS of the float64 VJP, without and with a `sums` normaliser.

    Worst ratios measured on an MI355X: v-ln-relu 7.6e-7, v-ln-gelu-wide 6.0e-7, v-ln-drop-65 6.1e-7, v-drop-128 4.5e-7,
    v-ln-stride 6.9e-7, v-gelu 5.0e-7, v-gelu-s1 2.7e-7, v-ln-s1 3.0e-7, c-ln-gelu 1.2e-6, c-ln-relu 4.1e-7,
    c-ln-drop-relu 7.2e-7, c-drop-odd 3.2e-7, c-gelu 7.6e-7, c-rows 6.4e-7 (MEASUREMENTS.md, section 22)."""
    p, g_q, g_ls, want, babs = case(params, oracle32, oracle64, name)
    _, stream, _, with_ln, rate = ref.NORM_CASES[name][:5]
    assert ("ln" in want) == with_ln
    if rate > 0:
        assert p.seed == ref.FIRST_STEP_SEED       # the step whose band the host test measured
    worst = 0.0
    for s in (None, 1.1e5):
        got = p.grad(g_q, g_ls, s)
        worst = max(worst, check(p, got, want, babs, 1.0 / (1.0 if s is None else s), (name, s)))
        arrs = p.arrays(got)
        if with_ln and stream == 1:                # the normalizers sit on stream 2's residual path only
            assert not arrs["ln"].any() and not want["ln"].any()
        elif with_ln:
            assert all(np.abs(a["ln"][l, i]).max() > 0 for a in (arrs, want) for l in range(p.L) for i in range(4))
    print(f"{name}: worst ratio {worst:.2e}")


SCALED = ("v-ln-relu", "c-ln-gelu", "v-gelu")


@pytest.mark.parametrize("name", SCALED)
def test_scales(params, oracle32, oracle64, name):
    """Head gradients 2^k g0, k in {-40, 24, 40}, with sums[2] in {none, 3e9}: every entry finite and every tensor within
    EPS of the scaled float64 VJP of g0."""
    p, g_q, g_ls, want, babs = case(params, oracle32, oracle64, name)
    worst = 0.0
    for k in (-40, 24, 40):
        f = 2.0 ** k
        for s in (None, 3e9):
            got = p.grad(g_q * f, g_ls * f, s)
            worst = max(worst, check(p, got, want, babs, f / (1.0 if s is None else s), (name, k, s)))
    print(f"{name}: worst ratio over the scales {worst:.2e}")


def test_impulse_stays_in_its_crop(params, oracle32, oracle64):
    """c-ln-gelu with a single non-zero head-gradient voxel at a corner of batch element 1: the group sums spread one
    voxel's delta over its own crop and not into element 0 -- every tensor within EPS of the float64 VJP."""
    p = NormPath(params, oracle32, oracle64, "c-ln-gelu")
    B, X, Y, Z = p.x.shape[:4]
    g_q0, g_ls0 = heads(np.random.default_rng(4), p.n, 2)
    for spot in ((1, 0, 0, 0), (1, X - 1, Y - 1, Z - 1)):
        v = np.ravel_multi_index(spot, (B, X, Y, Z))
        g_q, g_ls = np.zeros_like(g_q0), np.zeros_like(g_ls0)
        g_q[v], g_ls[v] = g_q0[v], g_ls0[v]
        want, _, babs = p.reference(g_q, g_ls)
        r = check(p, p.grad(g_q, g_ls, None), want, babs, 1.0, spot)
        print(f"impulse at {spot}: worst ratio {r:.2e}")


def test_backward_regenerates_the_forward_mask(params, oracle32, oracle64):
    """v-ln-drop-65: the gradient is within EPS of the reference under the step's own keep factors (the case test) and
    misses the reference whose backward sees the next step's factors by at least 10 EPS on some tensor: the comparison
    tells the masks apart."""
    p, g_q, g_ls, want, babs = case(params, oracle32, oracle64, "v-ln-drop-65")
    got = p.grad(g_q, g_ls, None)
    check(p, got, want, babs, 1.0, "own mask")
    rate, U, L = ref.NORM_CASES["v-ln-drop-65"][4:7]
    stale = ref.drop_factors(oracle64, rate, p.seed + 1, L, p.n, U)
    wrong, _, _ = ref.vjp(p.w, p.x, g_q, g_ls, None, se_idx=2, act=p.act, ln=p.ln, drop=p.drop, stale_mask=stale)
    r = ref.error_ratios(p.arrays(got), wrong, babs)
    print(f"against the stale mask: worst ratio {max(r.values()):.2e}")
    assert max(r.values()) >= 10 * EPS


@pytest.mark.parametrize("name", ["v-ln-drop-65", "c-ln-gelu"])
def test_bitwise_reproducible(params, oracle32, oracle64, name):
    """Two forward + backward calls at the same step give the same bits (the GroupNormalization partials are added in
    block order, as every other weight gradient)."""
    p = NormPath(params, oracle32, oracle64, name)
    g_q, g_ls = heads(np.random.default_rng(1), p.n, p.stream)
    a = p.grad(g_q, g_ls, 1.1e5)
    b = p.grad(g_q, g_ls, 1.1e5)
    assert np.array_equal(a, b)


def test_layer_norm_is_dispatched(params, oracle32, oracle64):
    """v-ln-relu against the same weights without use_layer_norm: the Wr1 gradients differ by far more than EPS -- no
    silent fall-through to the plain path."""
    p = NormPath(params, oracle32, oracle64, "v-ln-relu")
    q = NormPath(params, oracle32, oracle64, "v-ln-relu", layer_norm=False)
    assert q.ln is None and not q.ew.shape.layer_norm and p.ew.shape.layer_norm
    g_q, g_ls = heads(np.random.default_rng(1), p.n, p.stream)
    a, b = p.arrays(p.grad(g_q, g_ls, None))["Wr1"], q.arrays(q.grad(g_q, g_ls, None))["Wr1"]
    assert np.abs(a - b).max() >= 10 * EPS * max(np.abs(a).max(), np.abs(b).max())
