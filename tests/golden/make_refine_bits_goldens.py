#!/usr/bin/env python3
"""Runs the refinement and Laplace kernels of ONE build on the GPU and stores their output bits as a fixture.

    QBOLD_LIB=/path/to/parent/libqbold_hip.so python tests/golden/make_refine_bits_goldens.py --commit <parent id>

The library named by QBOLD_LIB is a build of the PARENT of the commit that shares the refinement step and the
signal-slope code between the kernels (the same C ABI, so this tree's Python drives it).  Output:
tests/golden/refine_bits_goldens.npz -- per case one uint32 array [200, 7] = the bits of (q_out[5], loss[2]), for the
Laplace cases [200, 20] = (q_out[5], out[15]) -- plus the parent's commit id and the `hipcc --version` text of the
build.  tests/test_gpu_refine_parent_bits.py imports CASES and run_case from this file and replays them on the current
build: sharing code between kernels must not move a bit.  After a toolchain change the fixture is regenerated from a
build of the same sources with the new toolchain, never loosened.

Every case: 200 voxels (a partial last tile; two blocks of the 128-thread kernels, one of the 256-thread kernels),
the case's own mask (live and masked voxels), 5 steps (tail = 1, five roundings of Adam's bias products, both head
buffers of the TV loop), S = 5 (Sp = 8: a full Philox quad and one holding a single draw), lr 0.05 -> 0.005,
voxel0 = 3; inputs from tests/_refine_anyt_cases.case, explicit normals seeded here.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(HERE, "refine_bits_goldens.npz")
N, STEPS, S, SP, SEED, VOXEL0 = 200, 5, 5, 8, 31, 3
LEAD = (2, 5, 4, 5)          # (B, X, Y, Z) of the spatial cases: N voxels
TV_WEIGHT = 0.02
THREE_IMAGE = dict(multi_image_normalisation=True)

# per-voxel cases: (label, inputs of _refine_anyt_cases.case, switches on top of the case's, kernel, optimisers)
_VOXEL = (
    ("ref11", "ref11", {}, "auto", ("adam", "sgd")),               # refine_kernel<11, 2>
    ("ref11_3img", "ref11", THREE_IMAGE, "auto", ("adam",)),       # refine_kernel<11, -1>
    ("ref24", "ref24", {}, "auto", ("adam",)),                     # refine_kernel<24, -1>
    ("odd33", "odd33", {}, "generic", ("adam", "sgd")),            # refine_generic_kernel from here on
    ("full64", "full64", {}, "generic", ("adam",)),
    ("two", "two", {}, "generic", ("adam",)),
    ("odd33_student_t", "odd33_student_t", {}, "generic", ("adam",)),
    ("odd33_log_data", "odd33_log_data", {}, "generic", ("adam",)),
    ("ref11_anyt", "ref11", {}, "generic", ("adam", "sgd")),
    ("ref24_anyt", "ref24", {}, "generic", ("adam",)),
)
# spatial cases: (label, inputs, kernel, steps, draws); ref11 / ref24 run refine_tv_step_kernel<11, 2> / <24, -1>
_SPATIAL = (
    ("ref11", "ref11", "auto", STEPS, ("philox", "z")),
    ("ref24", "ref24", "auto", STEPS, ("philox", "z")),
    ("odd33", "odd33", "generic", STEPS, ("philox", "z")),
    ("ref11_1step", "ref11", "auto", 1, ("philox",)),              # reads q_in, the result is copied out
    ("odd33_1step", "odd33", "generic", 1, ("z",)),
)
_LAPLACE = ("ref11", "odd33", "full64")


def _cases():
    out = {}
    for label, name, extra, kernel, opts in _VOXEL:
        for opt in opts:
            for draws in ("philox", "z"):
                out[f"voxel/{label}/{opt}/{draws}"] = ("voxel", name, extra, kernel, opt, STEPS, draws)
    for label, name, kernel, steps, draw_kinds in _SPATIAL:
        for draws in draw_kinds:
            out[f"spatial/{label}/adam/{draws}"] = ("spatial", name, {}, kernel, "adam", steps, draws)
    for name in _LAPLACE:
        out[f"laplace/{name}"] = ("laplace", name)
    return out


CASES = _cases()
_CONTEXTS = {}
_NORMALS = {}


def _context(p, sw):
    from qbold_vi_amd.ops import Context
    key = (tuple(sorted(p.items())), tuple(sorted(sw.items())))
    if key not in _CONTEXTS:
        _CONTEXTS[key] = Context(p, True, True, **sw)
    return _CONTEXTS[key]


def _normals(steps):
    if steps not in _NORMALS:
        z = np.random.default_rng(20261020).standard_normal((N, steps, SP, 2)).astype(np.float32)
        z.setflags(write=False)
        _NORMALS[steps] = z
    return _NORMALS[steps]


def run_case(params, key):
    """The uint32 bits [N, 7] (Laplace: [N, 20]) of case `key` on the library that qbold_vi_amd loads."""
    import torch

    import _laplace_reference as lr
    import _refine_anyt_cases as rc
    import test_gpu_forward_protocols as fp
    spec = CASES[key]
    dev = fp.dev
    if spec[0] == "laplace":
        from oracle.oracle import Oracle
        p, sw = lr.setup(params, spec[1])
        d = lr.inputs(Oracle("f32", p, **sw), spec[1], n=N)
        q_out, out = _context(p, sw).laplace_posterior(dev(fp.poisoned(d)), dev(d["mask"]), dev(d["prior"]),
                                                       dev(d["sigma"]))
        got = torch.cat([q_out, out], 1)
    else:
        kind, name, extra, kernel, opt, steps, draws = spec
        d = rc.case(params, name, N)
        c = _context(d["p"], dict(d["sw"], **extra))
        kw = dict(steps=steps, S=S, lr=0.05, lr_final=0.005, optimizer=opt, seed=SEED, voxel0=VOXEL0, want_loss=True,
                  z=dev(_normals(steps)) if draws == "z" else None, kernel=kernel)
        x, m, q, prior, sigma = (dev(d[k]) for k in ("x", "mask", "q", "prior", "sigma"))
        if kind == "voxel":
            q_out, loss = c.refine_posterior(x, m, q, prior, sigma, **kw)
        else:
            r5 = lambda t: t.reshape(LEAD + t.shape[1:])   # noqa: E731
            q_out, loss = c.refine_posterior_spatial(r5(x), r5(m), r5(q), r5(prior), r5(sigma), TV_WEIGHT, **kw)
        got = torch.cat([q_out.reshape(N, 5), loss.reshape(N, 2)], 1)
    torch.cuda.synchronize()
    return got.cpu().numpy().view(np.uint32)


def main():
    import argparse
    import configparser
    import subprocess
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="id of the commit the library in QBOLD_LIB was built from")
    ap.add_argument("--out", default=FIXTURE)
    a = ap.parse_args()
    if not os.environ.get("QBOLD_LIB"):
        raise SystemExit("make_refine_bits_goldens.py: set QBOLD_LIB to the parent build's libqbold_hip.so")
    cfg = configparser.ConfigParser()
    cfg.read(os.path.join(ROOT, "config"))
    params = dict(cfg["DEFAULT"])
    from qbold_vi_amd.build import _hipcc
    G = {key: run_case(params, key) for key in CASES}
    for key, bits in G.items():
        live = np.isfinite(bits.view(np.float32)).all(1)
        print(f"{key}: {bits.shape}, {int(live.sum())} finite rows")
    G["meta/parent_commit"] = np.array(a.commit)
    G["meta/hipcc_version"] = np.array(subprocess.run([_hipcc(), "--version"], capture_output=True, text=True,
                                                      check=True).stdout)
    np.savez_compressed(a.out, **G)
    print(f"wrote {a.out}: {len(G)} arrays, {os.path.getsize(a.out) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
