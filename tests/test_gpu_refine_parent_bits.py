"""The refinement kernels (specialised and run-time-T, per voxel and under the TV prior) and the Laplace kernel give
the bits that the build of the parent commit gave, before their step, draw, update and signal-slope code was shared
(qbold_vi_amd/csrc/signal_grad.h, refine_kernels.hip).  tests/golden/make_refine_bits_goldens.py defines the cases and
recorded tests/golden/refine_bits_goldens.npz from that parent build; this test replays every case on the current build
and compares the uint32 views: no tolerance, no case left out.  The fixture names the parent commit and the compiler
it was built with; a new toolchain regenerates it from the same sources."""
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_refine_bits_goldens",
                                               os.path.join(GOLDEN, "make_refine_bits_goldens.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def golden():
    with np.load(gen.FIXTURE) as f:
        return {k: f[k] for k in f.files}


def test_the_fixture_holds_every_case(golden):
    assert {k for k in golden if not k.startswith("meta/")} == set(gen.CASES)
    assert len(str(golden["meta/parent_commit"])) == 40 and "HIP version" in str(golden["meta/hipcc_version"])


@pytest.mark.parametrize("key", list(gen.CASES))
def test_bits_are_the_parent_builds(params, golden, key):
    want = golden[key]
    got = gen.run_case(params, key)
    assert want.dtype == np.uint32 and got.dtype == np.uint32 and got.shape == want.shape
    differ = np.argwhere(got != want)
    assert np.array_equal(got, want), (key, len(differ), "first (voxel, column):", differ[:5].tolist(),
                                       "parent", str(golden["meta/parent_commit"]))
