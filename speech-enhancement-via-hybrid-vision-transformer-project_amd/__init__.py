"""MI355X-native HybridViT hot path (gfx950 HIP kernels behind the reference's
nn.Module API).  Import name when loaded by the repository helpers: ``hvit_amd``.

Public surface (mirrors the reference's ``models`` package, models/__init__.py,
plus the factory it forgot to export):
    HybridViT, create_hybrid_vit, ConvBlock, TransposeConvBlock, FeedForward,
    PatchEmbedding, PositionalEncoding, MultiHeadSelfAttention,
    TransformerEncoderBlock, VisionTransformer, CombinedLoss, create_loss_function,
    FusedAdamW / clip_grad_norm_ / create_optimizer (training/optimizer.py, trainer.py:170-174),
    GraphedTrainStep (the train step replayed from a hipGraph per input shape, trainer.py:142-183),
    stft_mag / istft_mag / supported / n_frames (the device STFT / iSTFT front end, frontend.py),
    resample_wave / resample_taps / resample_reference (sample-rate conversion on the device, resampler.py),
    compute_sisdr / compute_snr / compute_segsnr / compute_lsd / compute_pesq / compute_stoi /
    compute_all_metrics / print_metrics (evaluation/metrics.py on the host), wave_metrics / lsd /
    all_metrics_batch (the same scores on GPU batches, metrics.py) and Evaluator (evaluation/evaluator.py),
    stoi / stoi_reference / stoi_taps / third_octave_bands (native STOI on the device and its float64 host reference),
    SpectrogramAugmenter / plan_host / apply_plan_host (data/augmentation.py drawn on the device, augment.py),
    SpectrogramStore / DeviceBatchLoader (the dataset cached on the GPU and its loader, data.py),
    create_scheduler / WarmupCosineScheduler (training/optimizer.py:76-200) and Trainer (training/trainer.py)
"""

from .hybrid_vit import (  # noqa: F401
    ConvBlock,
    DropPath,
    FeedForward,
    HybridViT,
    MultiHeadSelfAttention,
    PatchEmbedding,
    PositionalEncoding,
    TransformerEncoderBlock,
    TransposeConvBlock,
    VisionTransformer,
    create_hybrid_vit,
)
from .losses import CombinedLoss, create_loss_function  # noqa: F401
from .optim import (  # noqa: F401
    FusedAdamW,
    WarmupCosineScheduler,
    clip_grad_norm_,
    create_optimizer,
    create_scheduler,
)
from .train_step import GraphedTrainStep  # noqa: F401
from .config import audio_settings, load_all_configs, load_cli_configs, load_config, merge_configs  # noqa: F401
from .frontend import istft_mag, n_frames, stft_mag, supported  # noqa: F401
from .resampler import resample_reference, resample_taps, resample_wave  # noqa: F401
from .metrics import (  # noqa: F401
    all_metrics_batch,
    compute_all_metrics,
    compute_lsd,
    compute_pesq,
    compute_segsnr,
    compute_sisdr,
    compute_snr,
    compute_stoi,
    lsd,
    print_metrics,
    stoi,
    stoi_reference,
    stoi_taps,
    third_octave_bands,
    wave_metrics,
)
from .evaluator import Evaluator  # noqa: F401
from .augment import SpectrogramAugmenter, apply_plan_host, plan_host  # noqa: F401
from .data import DeviceBatchLoader, SpectrogramStore  # noqa: F401
from .trainer import Trainer  # noqa: F401
from . import _lib  # noqa: F401

__all__ = [
    "HybridViT", "create_hybrid_vit", "ConvBlock", "TransposeConvBlock", "FeedForward", "PatchEmbedding",
    "PositionalEncoding", "MultiHeadSelfAttention", "TransformerEncoderBlock", "VisionTransformer",
    "CombinedLoss", "create_loss_function", "FusedAdamW", "clip_grad_norm_", "create_optimizer", "GraphedTrainStep",
    "load_all_configs", "load_config", "merge_configs", "load_cli_configs", "audio_settings", "stft_mag", "istft_mag",
    "supported", "n_frames",
    "resample_wave", "resample_taps", "resample_reference", "compute_sisdr", "compute_snr", "compute_segsnr", "compute_lsd", "compute_pesq", "compute_stoi",
    "compute_all_metrics", "print_metrics", "wave_metrics", "lsd", "all_metrics_batch", "stoi", "stoi_reference",
    "stoi_taps", "third_octave_bands", "Evaluator",
    "SpectrogramAugmenter", "plan_host", "apply_plan_host", "SpectrogramStore", "DeviceBatchLoader",
    "create_scheduler", "WarmupCosineScheduler", "Trainer",
]
