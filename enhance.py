"""Enhancement CLI (the reference's enhance.py, SURVEY §3.C: a working
replacement for its broken one), BASELINE config 1.

    python enhance.py --checkpoint best_model.pth --input noisy.wav --output enhanced.wav
    python enhance.py --checkpoint best_model.pth --input-dir noisy/ --output-dir enhanced/ --extension .wav
    python enhance.py --synthetic 2.0 --output enhanced.wav     # 2 s harmonic clip, no checkpoint

The reference's flags (enhance.py:26-86) with its meaning: ``--config-dir``
(default ``config``) is merged by ``load_all_configs`` (data / model / train
YAMLs, utils/config.py:77-110); an unreadable directory falls back to the
defaults with a warning (enhance.py:105-110); its ``model`` section feeds
``create_hybrid_vit`` and its ``audio`` section the enhancer's STFT settings
(:131-138); ``--extension`` picks the files of directory mode (:160-165).
Additions: ``--config`` (one more YAML merged on top), ``--synthetic``,
``--precision``, ``--frontend``, ``--batch-size``, ``--resample`` (a file at
another rate than the configured one is resampled to it on the GPU instead of
refused, and the output is written at the configured rate, as the reference
does) and ``--keep-rate`` (single file mode: the result is resampled back and
written at the input's rate with the input's sample count).  STFT / iSTFT on the host
by default, on the GPU with ``--frontend device`` (directory mode then batches
``--batch-size`` clips per forward); the HybridViT forward on the GPU (HIP path,
fp32 unless --precision bf16).
"""

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Enhance noisy audio with the HybridViT (MI355X HIP path)")
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--config-dir", default="config", help="directory of data/model/train_config.yaml")
    ap.add_argument("--config", default=None, help="one more YAML merged on top of --config-dir's")
    ap.add_argument("--input", default=None)
    ap.add_argument("--output", default=None)
    ap.add_argument("--input-dir", default=None)
    ap.add_argument("--output-dir", default=None)
    ap.add_argument("--extension", default=".wav", help="audio file extension (directory mode)")
    ap.add_argument("--synthetic", type=float, default=None, help="seconds of synthetic noisy audio")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--no-normalize", action="store_true")
    ap.add_argument("--frontend", default="host", choices=["host", "device"],
                    help="where STFT / iSTFT run: torch on the host (default) or the HIP kernels on the GPU")
    ap.add_argument("--batch-size", type=int, default=1, help="clips per forward in directory mode")
    ap.add_argument("--resample", action="store_true",
                    help="take files at any sample rate: resample them to the configured rate on the GPU")
    ap.add_argument("--keep-rate", action="store_true",
                    help="single file mode with --resample: write the result at the input file's rate and length")
    a = ap.parse_args(argv)
    if a.keep_rate and not a.resample:
        ap.error("--keep-rate needs --resample")
    single = a.input is not None and a.output is not None
    directory = a.input_dir is not None and a.output_dir is not None
    if a.synthetic is None and not single and not directory:
        ap.error("Must specify either:\n  --input and --output for single file mode, or\n"
                 "  --input-dir and --output-dir for directory mode")
    if single and directory:
        ap.error("Cannot use both single file and directory mode simultaneously")

    import torch
    import hvit_amd_loader

    hv = hvit_amd_loader.load()
    from hvit_amd import enhancer as E

    cfg = hv.load_cli_configs(a.config_dir, a.config)
    model = hv.create_hybrid_vit(cfg, precision=a.precision)
    if a.checkpoint:
        model = E.load_model_for_inference(a.checkpoint, model, a.device)
    elif a.synthetic is None:
        ap.error("--checkpoint is required unless --synthetic is given")
    enh = E.AudioEnhancer(model, device=a.device, frontend=a.frontend, resample=a.resample, **hv.audio_settings(cfg))
    norm = not a.no_normalize
    if a.synthetic is not None:
        torch.manual_seed(0)
        clip = E.synthetic_clip(a.synthetic)
        out = enh.enhance(clip, normalize=norm)
        print(f"synthetic {a.synthetic:.2f} s clip: {len(clip)} samples -> {len(out)} samples, "
              f"rms in {float((clip ** 2).mean() ** 0.5):.4f} out {float((out ** 2).mean() ** 0.5):.4f}")
        if a.output:
            E.write_wav(a.output, out, enh.sample_rate)
    elif single:
        enh.enhance_file(a.input, a.output, normalize=norm, keep_rate=a.keep_rate)
    else:
        enh.enhance_directory(a.input_dir, a.output_dir, extension=a.extension, normalize=norm,
                              batch_size=a.batch_size)


if __name__ == "__main__":
    main()
