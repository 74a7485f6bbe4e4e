"""Argument checks shared by frontend.stft_mag, resampler.resample_wave and the
device half of metrics.py.  A leaf module: it imports nothing of the package.
``who`` is the caller's message prefix ("hvit frontend", ...)."""

from __future__ import annotations

from typing import Optional

import numpy as np
import torch


def canonical_device(device) -> torch.device:
    """``cuda`` without an index becomes ``cuda:<current>``: one cache key per device."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def wave_arg(t, who: str, what: str):
    """``(t, B, L, row_stride)`` of a float32 GPU batch ``[B, L]``, copied only
    when its element stride is not 1 or its rows overlap."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {what} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{who}: {what} must be a GPU tensor; there is no CPU path")
    if t.dim() != 2 or t.dtype != torch.float32 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{who}: {what} must be float32 [B, L], got {t.dtype} {tuple(t.shape)}")
    B, Ln = t.shape
    if t.stride(1) != 1 or (B > 1 and t.stride(0) < Ln):
        t = t.contiguous()
    return t, B, Ln, (t.stride(0) if B > 1 else Ln)  # a single row's stride is arbitrary (0 for a broadcast view)


def lengths_arg(lengths, B: int, device, who: str) -> Optional[torch.Tensor]:
    """Per-row lengths (a host sequence or a tensor) as int32 ``[B]`` on ``device``; None stays None."""
    if lengths is None:
        return None
    if not isinstance(lengths, torch.Tensor):
        lengths = torch.as_tensor(np.asarray(lengths, dtype=np.int32))
    lengths = lengths.to(device=device, dtype=torch.int32).contiguous()
    if lengths.shape != (B,):
        raise ValueError(f"{who}: lengths must have shape ({B},), got {tuple(lengths.shape)}")
    return lengths
