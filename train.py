"""Training CLI (the reference's train.py).

    python train.py --config-dir config --data-root data/voicebank_demand
    python train.py --config-dir config --data-root data/voicebank_demand --resample   # the 48 kHz corpus as downloaded
    python train.py --config-dir config --resume checkpoints/best_model.pth
    python train.py --synthetic 64 --epochs 2 --batch-size 8

The reference's flags (train.py:41-75) with its meaning: ``--config-dir`` is
merged by ``load_all_configs`` (its ``data``, ``model`` and ``training``
sections), ``--data-root`` names the VoiceBank-DEMAND folder, ``--resume`` a
Trainer checkpoint, ``--seed`` the torch / numpy seed (:23-35).  The training
set is read once, framed and normalised on the GPU and kept there
(``SpectrogramStore``); every batch is assembled and augmented by one launch
(``DeviceBatchLoader``), the train loader with ``shuffle`` and ``drop_last``
and the validation loader without, as at train.py:119-135.  Additions:
``--epochs`` and ``--batch-size`` override the config, ``--precision`` picks
the model's arithmetic (default bf16), ``--resample`` sets the data config key
``resample`` (files at another rate than ``data.sample_rate`` are resampled to
it on the GPU as the store is built instead of refused), and ``--synthetic N`` trains on N
synthetic pairs (and validates on N // 4 more) so that the command runs with
no dataset.  A missing config directory means the reference's defaults.  The
last line printed is the best checkpoint's path.
"""

import argparse
import os
import random
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Train the HybridViT for speech enhancement (MI355X HIP path)")
    ap.add_argument("--config-dir", default="config", help="directory of data/model/train_config.yaml")
    ap.add_argument("--data-root", default="data/voicebank_demand", help="root of the VoiceBank-DEMAND dataset")
    ap.add_argument("--resume", default=None, help="checkpoint to resume training from")
    ap.add_argument("--epochs", type=int, default=None, help="override training.num_epochs")
    ap.add_argument("--batch-size", type=int, default=None, help="override training.batch_size")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N",
                    help="train on N synthetic pairs instead of --data-root")
    ap.add_argument("--resample", action="store_true",
                    help="take a corpus at any sample rate (VoiceBank-DEMAND ships at 48 kHz): resample every file "
                         "to data.sample_rate on the GPU (sets the data config key 'resample')")
    ap.add_argument("--precision", default="bf16", choices=["fp32", "bf16"])
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--seed", type=int, default=42)
    a = ap.parse_args(argv)

    import numpy as np
    import torch

    import hvit_amd_loader

    hv = hvit_amd_loader.load()

    random.seed(a.seed)
    np.random.seed(a.seed)
    torch.manual_seed(a.seed)

    try:
        cfg = hv.load_all_configs(a.config_dir)
    except FileNotFoundError:
        print(f"Warning: no configuration under {a.config_dir}. Using defaults.")
        cfg = {}
    data_cfg = dict(cfg.get("data", {}) or {})
    train_cfg = dict(cfg.get("training", {}) or {})
    if a.resample:
        data_cfg["resample"] = True
    if a.epochs is not None:
        train_cfg["num_epochs"] = a.epochs
    if a.batch_size is not None:
        train_cfg["batch_size"] = a.batch_size
    train_cfg["seed"] = a.seed
    batch_size = train_cfg.setdefault("batch_size", 16)

    if a.synthetic > 0:
        train_store = hv.SpectrogramStore.synthetic(a.synthetic, (1.0, 3.0), seed=a.seed, device=a.device)
        val_store = hv.SpectrogramStore.synthetic(max(1, a.synthetic // 4), (1.0, 3.0), seed=a.seed + 100003,
                                                  device=a.device)
    else:
        train_store = hv.SpectrogramStore.from_directory(a.data_root, "train", data_cfg, device=a.device)
        val_store = hv.SpectrogramStore.from_directory(a.data_root, "val", data_cfg, device=a.device)
    print(f"Training samples: {len(train_store)} ({train_store.nbytes / 2 ** 20:.1f} MiB on the device)")
    print(f"Validation samples: {len(val_store)}")

    augment = (data_cfg.get("augmentation", {}) or {}).get("enabled", True)
    train_loader = hv.DeviceBatchLoader(train_store, batch_size, shuffle=True,
                                        drop_last=len(train_store) >= batch_size,
                                        augmenter=hv.SpectrogramAugmenter(data_cfg) if augment else None,
                                        seed=a.seed)
    val_loader = hv.DeviceBatchLoader(val_store, batch_size, shuffle=False, drop_last=False, seed=a.seed)

    model = hv.create_hybrid_vit(cfg, precision=a.precision)
    counts = model.count_parameters()
    print(f"Model parameters: {counts['total']:,} ({counts['trainable']:,} trainable)")
    trainer = hv.Trainer(model, train_loader, val_loader, train_cfg, device=a.device, resume_from=a.resume)
    trainer.train()
    best = trainer.checkpoint_dir / "best_model.pth"
    if not best.exists():
        best = trainer.checkpoint_dir / "final_model.pth"
    print(f"Best checkpoint: {best}")
    return trainer


if __name__ == "__main__":
    main()
