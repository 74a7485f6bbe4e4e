"""GPU: Trainer (training/trainer.py on GraphedTrainStep) over DeviceBatchLoader:
two epochs end to end with the reference's checkpoint keys, equality with a
hand-written loop, resume, validate, and the train.py command line."""

import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the tiny model of tests/test_gpu_trainer_surface.py
KW = dict(encoder_channels=[8, 16, 32], embed_dim=64, num_heads=4, num_layers=2, decoder_channels=[32, 16, 8, 1])
REF_KEYS = {"epoch", "global_step", "model_state_dict", "optimizer_state_dict", "best_val_loss", "config",
            "scheduler_state_dict"}  # trainer.py:360-370 (no scaler: bf16 needs none)


@pytest.fixture(scope="module")
def stores(hv):
    return (hv.SpectrogramStore.synthetic(12, (0.3, 0.6), seed=0, device=DEV),
            hv.SpectrogramStore.synthetic(6, (0.3, 0.6), seed=50, device=DEV))


def _config(tmp, epochs=2):
    return {"num_epochs": epochs, "batch_size": 4, "gradient_clip_max_norm": 1.0,
            "optimizer": {"name": "adamw", "lr": 1e-3, "weight_decay": 0.01},
            "scheduler": {"name": "cosine", "min_lr": 1e-6}, "loss": {},
            "early_stopping": {"enabled": True, "patience": 10},
            "checkpoint": {"save_dir": str(tmp / "ckpt"), "save_every_n_epochs": 1},
            "logging": {"log_dir": str(tmp / "logs"), "log_every_n_steps": 2},
            "graph": {"warmup": 1}}


def _loaders(hv, stores):
    train = hv.DeviceBatchLoader(stores[0], 4, shuffle=True, drop_last=True, augmenter=hv.SpectrogramAugmenter(),
                                 bucket_frames=32, seed=1)
    val = hv.DeviceBatchLoader(stores[1], 4, shuffle=False, drop_last=False, bucket_frames=32, seed=1)
    return train, val


def _model(hv, seed=0):
    torch.manual_seed(seed)
    return hv.HybridViT(**KW, precision="bf16").to(DEV)


def _close(a, b):
    """'continue identically' of tests/test_gpu_trainer_surface.py: 1e-4 max|v| + 1e-6."""
    for (k, v), v2 in zip(a.items(), b.values()):
        if v.is_floating_point():
            err, tol = (v - v2).abs().max().item(), 1e-4 * v.abs().max().item() + 1e-6
            assert err <= tol, (k, err, tol)
        else:
            assert torch.equal(v, v2), k


@pytest.fixture(scope="module")
def straight(hv, stores, tmp_path_factory):
    """Trainer.train() for 2 epochs from seed 0: the run the other tests compare with."""
    tmp = tmp_path_factory.mktemp("straight")
    train, val = _loaders(hv, stores)
    m = _model(hv)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    tr = hv.Trainer(m, train, val, _config(tmp))
    plans = []
    orig = train.prepare

    def spy(*a, **k):  # every training batch's plan, in order
        out = orig(*a, **k)
        plans.append(out[2])
        return out

    train.prepare = spy
    tr.train()
    torch.cuda.synchronize()
    return dict(tmp=tmp, trainer=tr, before=before, plans=[p.cpu() for p in plans],
                state={k: v.detach().clone() for k, v in m.state_dict().items()})


def test_two_epochs_train_and_checkpoint(hv, straight):
    tr, tmp = straight["trainer"], straight["tmp"]
    hist = json.loads((tmp / "logs" / "training_history.json").read_text())
    assert hist == tr.history and len(hist["train_loss"]) == 2 and len(hist["val_loss"]) == 2
    assert all(np.isfinite(hist["train_loss"])) and all(np.isfinite(hist["val_loss"]))
    assert hist["lr"][0] == 1e-3 and hist["lr"][1] < 1e-3  # the scheduler stepped between the epochs
    assert tr.global_step == 6 and tr.step_fn.replays > 0
    sd = tr.model.state_dict()
    assert set(sd) == set(straight["before"])
    still = [k for k, p in tr.model.named_parameters() if torch.equal(p.detach(), straight["before"][k])]
    assert not still
    for name in ("best_model.pth", "final_model.pth", "checkpoint_epoch_2.pth"):
        ck = torch.load(tmp / "ckpt" / name, map_location="cpu", weights_only=True)
        assert REF_KEYS <= set(ck) and "loader_state_dict" in ck, name
        assert set(ck["model_state_dict"]) == set(straight["before"])
        assert ck["config"]["num_epochs"] == 2
    assert ck["epoch"] == 1 and ck["global_step"] == 6
    with pytest.raises(NotImplementedError, match="gradient_accumulation_steps"):
        hv.Trainer(tr.model, tr.train_loader, None, dict(tr.config, gradient_accumulation_steps=2))


def test_hand_written_loop_reaches_the_same_parameters(hv, stores, straight, tmp_path):
    """trainer.py:269-309 by hand: GraphedTrainStep over the same loader, the
    scheduler stepped per epoch, the same seeds."""
    train, val = _loaders(hv, stores)
    m = _model(hv)
    cfg = _config(tmp_path)
    opt = hv.FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.01, capturable=True, max_grad_norm=1.0)
    sched = hv.create_scheduler(opt, cfg)
    step = hv.GraphedTrainStep(m, hv.create_loss_function(cfg), opt, warmup=1)
    for epoch in range(2):
        m.train()
        train.set_epoch(epoch)
        for batch in train:
            step(batch["noisy_spec"], batch["clean_spec"])
        m.eval()
        with torch.no_grad():
            for batch in val:
                m(batch["noisy_spec"])
        sched.step()
    torch.cuda.synchronize()
    _close(straight["state"], m.state_dict())


def test_resume_continues_the_straight_run(hv, stores, straight, tmp_path):
    train, val = _loaders(hv, stores)
    tr1 = hv.Trainer(_model(hv), train, val, _config(tmp_path, epochs=1))
    # the same schedule as the 2-epoch run: only the number of epochs run differs
    tr1.scheduler = hv.create_scheduler(tr1.optimizer, _config(tmp_path, epochs=2))
    tr1.train()
    ckpt = tmp_path / "ckpt" / "final_model.pth"
    train2, val2 = _loaders(hv, stores)
    m2 = _model(hv, seed=123)  # other initial weights: everything must come from the checkpoint
    tr2 = hv.Trainer(m2, train2, val2, _config(tmp_path, epochs=2), resume_from=str(ckpt))
    assert tr2.current_epoch == 1 and tr2.global_step == 3 and (train2.epoch, train2.pos) == (1, 0)
    plans = []
    orig = train2.prepare

    def spy(*a, **k):
        out = orig(*a, **k)
        plans.append(out[2])
        return out

    train2.prepare = spy
    tr2.train()
    torch.cuda.synchronize()
    assert len(plans) == 3 and tr2.global_step == 6
    for got, want in zip(plans, straight["plans"][3:]):
        assert torch.equal(got.cpu(), want)  # the same batches' masks, exactly
    _close(straight["state"], m2.state_dict())


def test_reference_checkpoint_without_the_extra_keys_loads(hv, stores, straight, tmp_path):
    ck = torch.load(straight["tmp"] / "ckpt" / "final_model.pth", map_location="cpu", weights_only=True)
    ref = {k: ck[k] for k in REF_KEYS}
    ref["scaler_state_dict"] = {"scale": 65536.0, "growth_factor": 2.0, "backoff_factor": 0.5,
                                "growth_interval": 2000, "_growth_tracker": 0}  # trainer.py:372-373
    path = tmp_path / "reference.pth"
    torch.save(ref, path)
    train, val = _loaders(hv, stores)
    tr = hv.Trainer(_model(hv, seed=5), train, val, _config(tmp_path), resume_from=str(path))
    assert tr.current_epoch == 2 and tr.global_step == 6 and tr.best_val_loss == ck["best_val_loss"]
    for (k, v), v2 in zip(tr.model.state_dict().items(), straight["state"].values()):
        assert torch.equal(v, v2), k


def test_validate_is_the_mean_loss_and_changes_nothing(hv, stores, straight):
    tr = straight["trainer"]
    before = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
    got = tr.validate()["loss"]
    torch.cuda.synchronize()
    for k, v in tr.model.state_dict().items():
        assert torch.equal(v, before[k]), k
    m = copy.deepcopy(tr.model).eval()
    crit = hv.create_loss_function(tr.config)
    losses = []
    with torch.no_grad():
        for batch in _loaders(hv, stores)[1]:
            losses.append(crit(m(batch["noisy_spec"]), batch["clean_spec"]).item())
    assert len(losses) == len(tr.val_loader) == 2
    assert got == pytest.approx(sum(losses) / len(losses), rel=1e-6)
    assert hv.Trainer(tr.model, tr.train_loader, None, tr.config).validate() == {}


def test_train_cli_synthetic(tmp_path):
    """train.py --synthetic 8 --epochs 1 in a fresh child process."""
    cfgdir = tmp_path / "config"
    cfgdir.mkdir()
    (cfgdir / "model_config.yaml").write_text(
        "model:\n  encoder:\n    channels: [8, 16, 32]\n  transformer:\n    embed_dim: 64\n    num_heads: 4\n"
        "    num_layers: 2\n  decoder:\n    channels: [32, 16, 8, 1]\n")
    (cfgdir / "train_config.yaml").write_text(
        f"training:\n  num_epochs: 3\n  batch_size: 4\n  checkpoint:\n    save_dir: {tmp_path / 'ckpt'}\n"
        f"  logging:\n    log_dir: {tmp_path / 'logs'}\n  graph:\n    warmup: 1\n")
    (cfgdir / "data_config.yaml").write_text("data:\n  sample_rate: 16000\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--config-dir", str(cfgdir), "--synthetic", "8",
                        "--epochs", "1", "--batch-size", "4"], capture_output=True, text=True, timeout=240,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("Best checkpoint: ")
    path = last.split(": ", 1)[1]
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert REF_KEYS <= set(ck) and ck["epoch"] == 0 and ck["config"]["num_epochs"] == 1
    assert len(ck["model_state_dict"]) > 0 and all(torch.isfinite(v).all() for v in ck["model_state_dict"].values()
                                                   if v.is_floating_point())
