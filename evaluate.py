"""Evaluation CLI (the reference's evaluate.py, SURVEY §3.C: a working
replacement for its broken one).

    python evaluate.py --checkpoint best_model.pth --data-root data/voicebank_demand
    python evaluate.py --checkpoint best_model.pth --noisy-dir noisy/ --clean-dir clean/ \\
        --frontend device --batch-size 32 --save-enhanced --output-dir results/evaluation

The reference's flags (evaluate.py:27-73) with its meaning: the test pairs are
``noisy_testset_wav`` / ``clean_testset_wav`` under ``--data-root`` unless
``--noisy-dir`` / ``--clean-dir`` name them; ``--config-dir`` is merged by
``load_all_configs`` and an unreadable directory falls back to the defaults
with a warning (:79-83); the scores go to ``evaluation_results.json`` under
``--output-dir`` and, with ``--save-enhanced``, the enhanced clips to its
``enhanced`` folder.  Additions: ``--config`` (one more YAML merged on top),
``--precision``, ``--frontend``, ``--batch-size``, ``--resample`` (files at
another rate than the configured one are resampled to it on the GPU instead of
refused; the scores are always computed at the configured rate) and ``--stoi``
(``native``: STOI by the project's own implementation, csrc/stoi.hip on the
device front end, instead of the ``pystoi`` package).  With ``--frontend
device`` the clips are enhanced and scored on the GPU in batches of
``--batch-size`` (SI-SDR, SNR, SegSNR, LSD: csrc/metrics.hip); PESQ and, by
default, STOI need the ``pesq`` / ``pystoi`` packages and read 0.0 without them.
"""

import argparse
import os
import sys
from pathlib import Path

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Evaluate the HybridViT on a test set (MI355X HIP path)")
    ap.add_argument("--checkpoint", required=True, help="model checkpoint")
    ap.add_argument("--config-dir", default="config", help="directory of data/model/train_config.yaml")
    ap.add_argument("--config", default=None, help="one more YAML merged on top of --config-dir's")
    ap.add_argument("--data-root", default="data/voicebank_demand", help="root of the VoiceBank-DEMAND dataset")
    ap.add_argument("--noisy-dir", default=None, help="noisy test audio (default: <data-root>/noisy_testset_wav)")
    ap.add_argument("--clean-dir", default=None, help="clean test audio (default: <data-root>/clean_testset_wav)")
    ap.add_argument("--output-dir", default="results/evaluation")
    ap.add_argument("--save-enhanced", action="store_true", help="write the enhanced clips to <output-dir>/enhanced")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--frontend", default="host", choices=["host", "device"],
                    help="where STFT / iSTFT and the metrics run: the host (default) or the HIP kernels on the GPU")
    ap.add_argument("--batch-size", type=int, default=32, help="pairs per device batch (--frontend device)")
    ap.add_argument("--resample", action="store_true",
                    help="take files at any sample rate: resample them to the configured rate on the GPU")
    ap.add_argument("--stoi", default="package", choices=["package", "native"],
                    help="STOI from the pystoi package (0.0 without it) or the native implementation")
    a = ap.parse_args(argv)
    if a.batch_size < 1:
        ap.error(f"--batch-size must be at least 1, got {a.batch_size}")

    import hvit_amd_loader

    hv = hvit_amd_loader.load()
    from hvit_amd import enhancer as E

    cfg = hv.load_cli_configs(a.config_dir, a.config)
    data_root = Path(a.data_root)
    noisy_dir = Path(a.noisy_dir) if a.noisy_dir else data_root / "noisy_testset_wav"
    clean_dir = Path(a.clean_dir) if a.clean_dir else data_root / "clean_testset_wav"
    output_dir = Path(a.output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)

    model = hv.create_hybrid_vit(cfg, precision=a.precision)
    print(f"Loading checkpoint from {a.checkpoint}")
    model = E.load_model_for_inference(a.checkpoint, model, a.device)
    evaluator = hv.Evaluator(model, device=a.device, frontend=a.frontend, batch_size=a.batch_size,
                             resample=a.resample, stoi=a.stoi, **hv.audio_settings(cfg))
    print(f"Noisy directory: {noisy_dir}\nClean directory: {clean_dir}")
    enhanced_dir = output_dir / "enhanced" if a.save_enhanced else None
    results = evaluator.evaluate_dataset(noisy_dir, clean_dir, output_dir=enhanced_dir, save_enhanced=a.save_enhanced)
    evaluator.print_results(results)
    evaluator.save_results(results, output_dir / "evaluation_results.json")
    if a.save_enhanced:
        print(f"Enhanced audio saved to {enhanced_dir}")
    return results


if __name__ == "__main__":
    main()
