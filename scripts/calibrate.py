#!/usr/bin/env python3
"""Do the intervals of a trained encoder cover as often as they claim?  Simulation-based calibration (Talts et al. 2018)
on synthetic voxels with known (OEF, DBV): EncoderTrainer.calibration on the encoder of CONFIG.yaml with the weights of
FILE (.npz as save_weights writes them), the coverage table on stdout and the whole summary as JSON.
  python scripts/calibrate.py CONFIG.yaml --weights FILE [--voxels N] [--samples L] [--psis] [--first-op]
                              [--seed S] [--out calibration.json]
--psis ranks under the Pareto-smoothed importance weights of the fine-tuning model (stream 1's heads as the prior, as
the fine-tuning loop takes them) and adds the table over the voxels whose k^ is below the threshold."""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from qbold_vi_amd import training  # noqa: E402
from qbold_vi_amd.calibration import format_table  # noqa: E402
from qbold_vi_amd.signals import SignalGenerationLayer  # noqa: E402
from qbold_vi_amd.utils import load_arguments  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--weights", required=True)
    ap.add_argument("--voxels", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=255)
    ap.add_argument("--psis", action="store_true")
    ap.add_argument("--first-op", action="store_true", help="score stream 1 (the pre-training output)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="calibration.json")
    a = ap.parse_args()
    config, weights, out = (os.path.abspath(p) for p in (a.config, a.weights, a.out))
    os.chdir(ROOT)   # the INI `config` is read from the CWD
    cfg = load_arguments(["train.py", config], entry="train")
    params = training.get_params("config")
    model, _, trainer = training.create_encoder_model(cfg, params)
    model.load_weights(weights)
    ft = prior = None
    if a.psis:
        ft = trainer.build_fine_tuner(model, SignalGenerationLayer(dict(params, simulate_noise="False"),
                                                                   cfg.get("full_model", True), cfg.get("use_blood", True)))
        # the prior of the fine-tuning loss: stream 1's heads on the same voxels (the dataset is a function of the seed)
        x, _, _ = training.synthetic_voxel_dataset(params, cfg, a.voxels, trainer.context.device, a.seed)
        prior = model.predict(x, want=("out1",))[0][..., :5].contiguous()
    res = trainer.calibration(model, n_voxels=a.voxels, no_samples=a.samples, seed=a.seed, fine_tuner=ft, prior=prior,
                              psis=a.psis, use_first_op=a.first_op,
                              uniform_prop=float(cfg.get("uniform_prop", 0.0) or 0.0))
    s = res["summary"]
    print(format_table(s))
    print("z_mean (OEF, DBV, R2')", [round(v, 4) for v in s["z_mean"]], " z_rms", [round(v, 4) for v in s["z_rms"]])
    with open(out, "w") as f:
        json.dump(dict(config=os.path.basename(config), voxels=a.voxels, samples=a.samples, psis=a.psis,
                       first_op=a.first_op, seed=a.seed, summary=s), f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
