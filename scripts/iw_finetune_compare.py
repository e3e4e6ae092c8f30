#!/usr/bin/env python3
"""End-to-end comparison of the two fine-tuning objectives (MEASUREMENTS.md section 14): pre-train once on synthetic
voxels, then fine-tune from the SAME pre-trained weights with iw_samples = 0 (the reference's ELBO) and with
iw_samples = K (the K-sample importance-weighted bound, DReG gradients), and report on held-out synthetic voxels with
known noise: mean log p^_1024, the ELBO of the same draws, the VI gap, and the learned sigma against the true noise
level of the normalised data.  Not a test: one run, one seed; prints one JSON object.
  python scripts/iw_finetune_compare.py [--iw K] [--voxels N] [--pt-epochs E] [--ft-epochs E] [--out DIR]"""
import argparse
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from qbold_vi_amd import training  # noqa: E402
from qbold_vi_amd.signals import SignalGenerationLayer  # noqa: E402
from qbold_vi_amd.utils import load_arguments  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iw", type=int, default=16)
    ap.add_argument("--voxels", type=int, default=65536)
    ap.add_argument("--pt-epochs", type=int, default=40)
    ap.add_argument("--ft-epochs", type=int, default=10)
    ap.add_argument("--held-out", type=int, default=16384)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.chdir(ROOT)   # the INI `config` is read from the CWD
    base = a.out or tempfile.mkdtemp(prefix="iw_compare_")
    cfg = load_arguments(["train.py", os.path.join(ROOT, "configurations", "optimal.yaml")], entry="train")
    cfg.update(synthetic_voxels=a.voxels, no_pt_epochs=a.pt_epochs, no_ft_epochs=a.ft_epochs, mc_samples=1)
    params = training.get_params("config")
    # held-out voxels with known noise: the same draws of (OEF, DBV) through the forward model with and without noise
    xh, mh, yh = training.synthetic_voxel_dataset(params, cfg, a.held_out, "cuda", seed=12345)
    clean = SignalGenerationLayer(dict(params, simulate_noise="False"), True, True)(yh)
    T = xh.shape[-1]
    se = int(abs(float(params["tau_start"]) / float(params["tau_step"])))
    true_sigma = ((xh - clean) / (xh[:, se:se + 1] + 1e-3)).pow(2).mean().sqrt().item()   # RMS noise, normalised data
    res = {"iw_samples": a.iw, "voxels": a.voxels, "pt_epochs": a.pt_epochs, "ft_epochs": a.ft_epochs,
           "held_out": a.held_out, "true_noise_rms_normalised": true_sigma}
    for name, iw in (("elbo", 0), (f"iw{a.iw}", a.iw)):
        d = os.path.join(base, name)
        os.makedirs(d, exist_ok=True)
        if iw > 0:   # the same pre-trained weights: phase skipping loads <dir>/pt_model.npz
            shutil.copy(os.path.join(base, "elbo", "pt_model.npz"), os.path.join(d, "pt_model.npz"))
        model, trainer, hist = training.train_model(dict(cfg, save_directory=d, iw_samples=iw))
        ft = trainer.build_fine_tuner(model, SignalGenerationLayer(dict(params, simulate_noise="False"), True, True))
        x5 = xh.reshape(-1, 1, 1, 1, T)
        prior5 = model(x5)[0]
        ev = ft.log_evidence(x5, mh.reshape(-1, 1, 1, 1, 1), prior5, no_samples=1024, seed=777)
        _, _, sg = model.predict(x5)
        res[name] = {"mean_log_evidence_1024": float(ev["mean_log_evidence"]), "mean_elbo_1024": float(ev["mean_elbo"]),
                     "gap": float(ev["gap"]), "median_ess": float(ev["ess"].median()),
                     "learned_sigma_median": float(sg.median()), "learned_sigma_rms": float(sg.pow(2).mean().sqrt()),
                     "last_epoch": hist[-1]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
