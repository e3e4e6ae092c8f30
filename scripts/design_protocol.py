#!/usr/bin/env python3
"""Which taus should I acquire, and how often?  A greedy search with pairwise exchanges for the allocation of a budget of
M averages over the tau grid of CONFIG.yaml's protocol that maximises the Bayesian D-criterion
E_theta log det(I(theta; w) + Lambda) (Context.design_scores) over N truths drawn from the configuration's prior.
  python scripts/design_protocol.py CONFIG.yaml --budget M [--voxels N] [--require-se] [--sigma S] [--seed S]
The information is that of the likelihood the library fits with: independent noise sigma on the NORMALISED data, the
normaliser's own noise ignored.  Under one-image normalisation the spin-echo row therefore carries ~ no information and
an unconstrained search drops that image although it must be acquired to normalise by: --require-se keeps at least one
average on every image of the normalisation window.
The search starts from the uniform allocation, moves one average at a time between two taus, scores all T (T - 1) moves
of a round in ONE design_scores call, keeps the best and stops when the criterion no longer rises.  The sums are
bit-reproducible, so the allocation is the same run to run."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

PRIOR_HEADS = (0.0, 0.3, -1.0, 0.3, 0.0)   # the logit-Normal the bounds are regularised with (raw heads)


def uniform_allocation(T, budget):
    """budget // T averages per tau, the remainder one each to the first taus."""
    w = np.full(T, budget // T, np.float32)
    w[:budget % T] += 1
    return w


def neighbours(w, locked=()):
    """Every allocation one move away: an average taken from tau i (which keeps at least one when i is locked) and given
    to tau j != i.  [n, T] float32, in (i, j) order."""
    T = len(w)
    out = []
    for i in range(T):
        if w[i] < 1 or (i in locked and w[i] < 2):
            continue
        for j in range(T):
            if j != i:
                v = w.copy()
                v[i] -= 1
                v[j] += 1
                out.append(v)
    return np.array(out, np.float32).reshape(-1, T)


def d_criterion(ctx, theta, sigma, prior, designs):
    """Mean over the truths of log det(I + Lambda) per design [B] (float64, on the host)."""
    s = ctx.design_scores(theta, sigma, torch.as_tensor(designs, device=theta.device), prior).cpu().numpy()
    return s[:, 0] / s[:, 4]


def search(ctx, theta, sigma, prior, budget, require_se=False, multi=False, log=None):
    """(allocation [T], its criterion, the uniform allocation's criterion, rounds); multi: the context normalises by
    three images."""
    T = ctx.T
    se = ctx.se_idx
    locked = ()
    if require_se:
        locked = tuple(range(se - 1, se + 2)) if multi else (se,)
        if budget < len(locked):
            raise ValueError("--require-se needs a budget of at least one average per image of the normalisation window")
    w = uniform_allocation(T, budget)
    for i in locked:   # a budget below T leaves zeros: give the window its images from the fullest taus
        while w[i] < 1:
            w[int(np.argmax(w))] -= 1
            w[i] += 1
    start = cur = float(d_criterion(ctx, theta, sigma, prior, w[None])[0])
    rounds = 0
    while True:
        cand = neighbours(w, locked)
        if not len(cand):
            break
        d = d_criterion(ctx, theta, sigma, prior, cand)
        best = int(np.argmax(d))
        if not d[best] > cur:
            break
        w, cur, rounds = cand[best], float(d[best]), rounds + 1
        if log:
            log(f"round {rounds:3d}: D = {cur:.6f}  {w.astype(int).tolist()}")
    return w, cur, start, rounds


def main():
    from qbold_vi_amd import training
    from qbold_vi_amd.ops import Context
    from qbold_vi_amd.utils import load_arguments
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("config")
    ap.add_argument("--budget", type=int, required=True, help="total number of averages to allocate")
    ap.add_argument("--voxels", type=int, default=4096, help="truths drawn from the configuration's prior")
    ap.add_argument("--require-se", action="store_true", help="keep >= 1 average on the normalisation window")
    ap.add_argument("--sigma", type=float, default=0.02, help="noise sd of one average on the normalised data")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    config = os.path.abspath(a.config)
    os.chdir(ROOT)   # the INI `config` is read from the CWD
    cfg = load_arguments(["train.py", config], entry="train")
    params = training.get_params("config")
    multi = bool(cfg.get("multi_image_normalisation", False))
    ctx = Context(params, cfg.get("full_model", True), cfg.get("use_blood", True), multi_image_normalisation=multi)
    _, _, theta = training.synthetic_voxel_dataset(params, cfg, a.voxels, ctx.device, a.seed)
    sigma = torch.full((ctx.T,), a.sigma, device=theta.device)
    prior = torch.tensor(PRIOR_HEADS, device=theta.device).repeat(a.voxels, 1)
    w, d, d0, rounds = search(ctx, theta.contiguous(), sigma, prior, a.budget, a.require_se, multi, log=print)
    taus = np.asarray(ctx.taus)
    print(f"{'tau (ms)':>10s} {'averages':>9s}")
    for t, n in zip(taus, w.astype(int)):
        print(f"{1e3 * t:10.2f} {n:9d}")
    print(f"D-criterion {d:.6f} after {rounds} moves; uniform {d0:.6f}; gain {d - d0:.6f} "
          f"(the posterior area shrinks by exp(-gain / 2) = {np.exp(-(d - d0) / 2):.3f})")


if __name__ == "__main__":
    main()
