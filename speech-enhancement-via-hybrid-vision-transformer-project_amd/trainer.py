"""The reference's Trainer (training/trainer.py) on the HIP train step.

Same constructor, config keys (trainer.py:69-106), methods and checkpoint dict
(:350-412); the step itself is ``GraphedTrainStep``: forward, CombinedLoss,
backward, fused clip + ``FusedAdamW(capturable=True,
max_grad_norm=gradient_clip_max_norm)``, replayed from one hipGraph per batch
shape.  The loaders are ``DeviceBatchLoader``s (any iterable of
``{'noisy_spec', 'clean_spec'}`` GPU batches works).

Differences from the reference, on purpose:

* no tensorboard: ``use_tensorboard`` is ignored; the per-epoch losses and
  learning rates go to ``training_history.json`` under ``log_dir`` instead;
* no GradScaler: the bf16 path needs no loss scaling (``use_amp`` is ignored;
  the model's ``precision`` decides).  A reference checkpoint's
  ``scaler_state_dict`` is skipped on load and none is written;
* ``gradient_accumulation_steps > 1`` raises: a captured step is one whole
  optimizer step;
* only the 'adamw' optimizer (the captured step needs device step counters);
* no data-parallel wiring: the loader's ``rank`` / ``world`` arguments are the
  only hook, a later change's business;
* the loss is not read back every step (trainer.py:188 calls ``.item()`` per
  batch): it is summed on the device and read every ``log_every_n_steps``
  steps and at the end of the epoch;
* the checkpoint carries three extra keys, ``loader_state_dict`` (the
  training loader's order, position and augmentation seed stream),
  ``dropout_state`` (the model's device dropout seed stream) and
  ``epochs_without_improvement``, so a resumed run continues the straight
  run's batches and masks.  A checkpoint without them (the reference's) loads.
"""

from __future__ import annotations

import json
import time
from pathlib import Path
from typing import Any, Dict, Optional

import torch
import torch.nn as nn

from .losses import create_loss_function
from .optim import FusedAdamW, create_scheduler
from .train_step import GraphedTrainStep


class Trainer:
    def __init__(self, model: nn.Module, train_loader, val_loader, config: Dict[str, Any], device: str = "cuda",
                 resume_from: Optional[str] = None):
        self.model = model.to(device)
        self.train_loader, self.val_loader = train_loader, val_loader
        self.config, self.device = config, device

        self.num_epochs = config.get("num_epochs", 100)
        self.batch_size = config.get("batch_size", 16)
        self.gradient_clip_max_norm = config.get("gradient_clip_max_norm", 1.0)
        self.gradient_accumulation_steps = config.get("gradient_accumulation_steps", 1)
        if self.gradient_accumulation_steps != 1:
            raise NotImplementedError(
                "hvit Trainer: gradient_accumulation_steps > 1 is not supported with the graphed train step "
                "(one captured step is one optimizer step); raise batch_size instead")

        self.criterion = create_loss_function(config).to(device)
        oc = config.get("optimizer", {})
        if oc.get("name", "adamw").lower() != "adamw":
            raise NotImplementedError("hvit Trainer: only the 'adamw' optimizer runs in the graphed train step")
        clip = self.gradient_clip_max_norm
        self.optimizer = FusedAdamW(self.model.parameters(), lr=oc.get("lr", 1e-4), betas=oc.get("betas", (0.9, 0.999)),
                                    eps=oc.get("eps", 1e-8), weight_decay=oc.get("weight_decay", 0.01),
                                    amsgrad=oc.get("amsgrad", False), capturable=True,
                                    max_grad_norm=clip if clip and clip > 0 else None)
        self.scheduler = create_scheduler(self.optimizer, config)
        gc = config.get("graph", {})  # not a reference key: the per-shape graph cache of GraphedTrainStep
        self.step_fn = GraphedTrainStep(self.model, self.criterion, self.optimizer, warmup=gc.get("warmup", 2),
                                        max_graphs=gc.get("max_graphs", 8))

        es = config.get("early_stopping", {})
        self.early_stopping_enabled = es.get("enabled", True)
        self.early_stopping_patience = es.get("patience", 10)
        self.early_stopping_min_delta = es.get("min_delta", 1e-4)

        cc = config.get("checkpoint", {})
        self.checkpoint_dir = Path(cc.get("save_dir", "checkpoints"))
        self.checkpoint_dir.mkdir(parents=True, exist_ok=True)
        self.save_every_n_epochs = cc.get("save_every_n_epochs", 5)
        self.save_best_only = cc.get("save_best_only", True)

        lc = config.get("logging", {})
        self.log_dir = Path(lc.get("log_dir", "logs"))
        self.log_dir.mkdir(parents=True, exist_ok=True)
        self.log_every_n_steps = lc.get("log_every_n_steps", 10)

        self.current_epoch = 0
        self.global_step = 0
        self.best_val_loss = float("inf")
        self.epochs_without_improvement = 0
        self.history = {"train_loss": [], "val_loss": [], "lr": []}
        self.best_checkpoint_path: Optional[Path] = None

        if resume_from is not None:
            self.load_checkpoint(resume_from)

    # ------------------------------------------------------------------ epochs --
    def train_epoch(self) -> Dict[str, float]:
        """trainer.py:123-205 with the whole step in ``GraphedTrainStep``."""
        self.model.train()
        loader = self.train_loader
        # (a loader restored in the middle of an epoch finishes that epoch's order first)
        if hasattr(loader, "set_epoch") and getattr(loader, "pos", 0) == 0:
            loader.set_epoch(self.current_epoch)
        total = None
        num_batches = 0
        for batch_idx, batch in enumerate(loader):
            noisy, clean = batch["noisy_spec"], batch["clean_spec"]
            if not noisy.is_cuda:
                noisy, clean = noisy.to(self.device), clean.to(self.device)
            loss = self.step_fn(noisy, clean)
            # a replay's loss is the graph's static buffer: fold it in before the next step
            total = loss.detach().to(torch.float32).clone() if total is None else total.add_(loss.detach())
            self.global_step += 1
            num_batches += 1
            if (batch_idx + 1) % self.log_every_n_steps == 0:
                print(f"  step {self.global_step}: loss {loss.item():.6f}")
        if num_batches == 0:
            raise RuntimeError("hvit Trainer: the training loader yielded no batch")
        return {"loss": total.item() / num_batches}

    @torch.no_grad()
    def validate(self) -> Dict[str, float]:
        """trainer.py:207-251: eval forwards and the loss; the mean over batches."""
        if self.val_loader is None:
            return {}
        self.model.eval()
        total = None
        num_batches = 0
        for batch in self.val_loader:
            noisy, clean = batch["noisy_spec"], batch["clean_spec"]
            if not noisy.is_cuda:
                noisy, clean = noisy.to(self.device), clean.to(self.device)
            loss = self.criterion(self.model(noisy), clean).detach().to(torch.float32)
            total = loss.clone() if total is None else total.add_(loss)
            num_batches += 1
        if num_batches == 0:
            return {}
        return {"loss": total.item() / num_batches}

    def train(self):
        """trainer.py:253-348."""
        print(f"\nStarting training for {self.num_epochs} epochs...")
        print(f"Device: {self.device}")
        print(f"Training samples: {len(self.train_loader.dataset)}")
        if self.val_loader:
            print(f"Validation samples: {len(self.val_loader.dataset)}")
        print(f"Batch size: {self.batch_size}\n")

        for epoch in range(self.current_epoch, self.num_epochs):
            self.current_epoch = epoch
            t0 = time.time()
            train_metrics = self.train_epoch()
            val_metrics = self.validate()
            print(f"Epoch {epoch + 1}/{self.num_epochs} - Train Loss: {train_metrics['loss']:.6f}")
            if val_metrics:
                print(f"  Val Loss: {val_metrics['loss']:.6f}")
            print(f"  Time: {time.time() - t0:.2f}s")
            self.history["train_loss"].append(train_metrics["loss"])
            self.history["val_loss"].append(val_metrics.get("loss"))
            self.history["lr"].append(self.optimizer.param_groups[0]["lr"])

            if self.scheduler is not None:
                if isinstance(self.scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau):
                    if val_metrics:
                        self.scheduler.step(val_metrics["loss"])
                else:
                    self.scheduler.step()

            val_loss = val_metrics.get("loss", float("inf"))
            if val_loss < self.best_val_loss:
                print(f"  Validation loss improved from {self.best_val_loss:.6f} to {val_loss:.6f}")
                self.best_val_loss = val_loss
                self.epochs_without_improvement = 0
                self.save_checkpoint("best_model.pth", is_best=True)
            else:
                self.epochs_without_improvement += 1
            if (epoch + 1) % self.save_every_n_epochs == 0:
                self.save_checkpoint(f"checkpoint_epoch_{epoch + 1}.pth")
            self._write_history()
            if self.early_stopping_enabled and self.epochs_without_improvement >= self.early_stopping_patience:
                print(f"\nEarly stopping triggered after {epoch + 1} epochs. "
                      f"No improvement for {self.early_stopping_patience} epochs.")
                break
            print()

        self.save_checkpoint("final_model.pth")
        self._write_history()
        print("\nTraining completed!")
        print(f"Best validation loss: {self.best_val_loss:.6f}")

    def _write_history(self) -> None:
        with open(self.log_dir / "training_history.json", "w") as f:
            json.dump(self.history, f, indent=2)

    # ------------------------------------------------------------- checkpoints --
    def save_checkpoint(self, filename: str, is_best: bool = False):
        """trainer.py:350-380 (+ the loader, dropout-stream and early-stopping state)."""
        path = self.checkpoint_dir / filename
        ckpt = {
            "epoch": self.current_epoch,
            "global_step": self.global_step,
            "model_state_dict": self.model.state_dict(),
            "optimizer_state_dict": self.optimizer.state_dict(),
            "best_val_loss": self.best_val_loss,
            "config": self.config,
        }
        if self.scheduler is not None:
            ckpt["scheduler_state_dict"] = self.scheduler.state_dict()
        if hasattr(self.train_loader, "state_dict"):
            ckpt["loader_state_dict"] = self.train_loader.state_dict()
        ds = self.model.dropout_state() if hasattr(self.model, "dropout_state") else None
        if ds is not None:
            ckpt["dropout_state"] = ds.cpu()
        ckpt["epochs_without_improvement"] = self.epochs_without_improvement
        ckpt["history"] = self.history
        torch.save(ckpt, path)
        if is_best:
            self.best_checkpoint_path = path
            print(f"  Saved best model to {path}")
        else:
            print(f"  Saved checkpoint to {path}")

    def load_checkpoint(self, checkpoint_path: str):
        """trainer.py:382-412.  Nothing from the file is executed (weights_only)."""
        print(f"Loading checkpoint from {checkpoint_path}")
        ckpt = torch.load(str(checkpoint_path), map_location=self.device, weights_only=True)
        self.model.load_state_dict(ckpt["model_state_dict"])
        self.optimizer.load_state_dict(ckpt["optimizer_state_dict"])
        if self.scheduler is not None and "scheduler_state_dict" in ckpt:
            self.scheduler.load_state_dict(ckpt["scheduler_state_dict"])
        self.current_epoch = ckpt["epoch"] + 1
        self.global_step = ckpt["global_step"]
        self.best_val_loss = ckpt.get("best_val_loss", float("inf"))
        self.epochs_without_improvement = ckpt.get("epochs_without_improvement", 0)
        self.history = ckpt.get("history", self.history)
        if "loader_state_dict" in ckpt and hasattr(self.train_loader, "load_state_dict"):
            self.train_loader.load_state_dict(ckpt["loader_state_dict"])
        if "dropout_state" in ckpt and hasattr(self.model, "set_dropout_state"):
            base, counter = (int(v) for v in ckpt["dropout_state"].cpu())
            self.model.set_dropout_state(base, counter)
        print(f"Resumed from epoch {self.current_epoch}")


__all__ = ["Trainer"]
