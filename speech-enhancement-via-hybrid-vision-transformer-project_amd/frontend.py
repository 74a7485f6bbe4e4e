"""Device STFT / iSTFT front end (csrc/stft.hip behind hvit_stft_fwd,
hvit_spec_normalize and hvit_istft): the framing of inference/enhancer.py:82-118
and data/dataset.py:183-219 as batched HIP kernels, so a batch of clips goes
waveform -> normalised magnitude [B, 1, F, T] -> model -> waveform without
leaving the device.

Semantics are librosa 0.10's (oracle/stft_restated.py): center=True with zero
padding, a periodic Hann window centred in n_fft, T = 1 + len // hop frames.
The phase is kept as the unit phasor X / |X| ([B, F, T, 2]), not as an angle:
the enhancer only ever forms mag' * e^{j phase}, so neither atan2 nor sincos is
needed.  There is no CPU path: a CPU tensor is an error.
"""

from __future__ import annotations

import math
from typing import Optional, Sequence, Union

import numpy as np
import torch

from . import _lib as L
from ._args import canonical_device, lengths_arg, wave_arg

N_FFTS = (256, 512, 1024)
_MODES = {None: None, "max": 0, "minmax": 1}
_windows = {}


def supported(n_fft: int, hop_length: int, win_length: int) -> bool:
    """The settings the kernels take: n_fft 256 / 512 / 1024, win_length <=
    n_fft, n_fft / 8 <= hop_length <= n_fft / 2."""
    return (n_fft in N_FFTS and 1 <= win_length <= n_fft and 8 * hop_length >= n_fft
            and 2 * hop_length <= n_fft)


def n_frames(length: int, hop_length: int) -> int:
    """Frames of a centred STFT of ``length`` samples."""
    return 1 + int(length) // int(hop_length)


def _check(n_fft, hop_length, win_length):
    if not supported(n_fft, hop_length, win_length):
        raise ValueError(f"hvit frontend: n_fft={n_fft}, hop_length={hop_length}, win_length={win_length} is not "
                         f"supported on the device (n_fft in {N_FFTS}, win_length <= n_fft, "
                         "n_fft/8 <= hop_length <= n_fft/2)")


def window_table(n_fft: int, win_length: int, device) -> torch.Tensor:
    """The periodic Hann window of win_length centred in n_fft, computed in
    float64 and rounded once; cached per device and setting."""
    device = canonical_device(device)
    key = (str(device), n_fft, win_length)
    w = _windows.get(key)
    if w is None:
        n = np.arange(win_length, dtype=np.float64)
        h = 0.5 - 0.5 * np.cos(2.0 * math.pi * n / win_length)
        lpad = (n_fft - win_length) // 2
        full = np.pad(h, (lpad, n_fft - win_length - lpad)).astype(np.float32)
        w = _windows[key] = torch.from_numpy(full).to(device)
    return w


def _need_gpu(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"hvit frontend: {what} must be a GPU tensor; there is no CPU path")


def stft_mag(wave: torch.Tensor, lengths=None, n_fft: int = 512, hop_length: int = 128, win_length: int = 512,
             return_phasor: bool = False, normalize: Optional[str] = None):
    """Magnitude spectrograms [B, 1, F, T] of a float32 GPU batch ``wave``
    [B, L] (row b is ``wave[b, :lengths[b]]`` followed by zeros).

    ``normalize``: None, "max" (mag / max, enhancer.py:96-101) or "minmax"
    ((mag - min) / (max - min), dataset.py:213-219), per row over its valid
    frames.  With ``return_phasor`` the result is ``(mag, phasor [B, F, T, 2],
    stats [B, 2])``; stats holds each row's min and max of the magnitude BEFORE
    normalisation.  Frames past a row's ``1 + len // hop`` are 0 / (1, 0)."""
    wave, B, Ln, row_stride = wave_arg(wave, "hvit frontend", "wave")
    _check(n_fft, hop_length, win_length)
    if normalize not in _MODES:
        raise ValueError(f"hvit frontend: normalize={normalize!r} (None, 'max' or 'minmax')")
    dev = wave.device
    F, T = n_fft // 2 + 1, n_frames(Ln, hop_length)
    lens = lengths_arg(lengths, B, dev, "hvit frontend")
    win = window_table(n_fft, win_length, dev)
    mag = torch.empty((B, 1, F, T), dtype=torch.float32, device=dev)
    phasor = torch.empty((B, F, T, 2), dtype=torch.float32, device=dev) if return_phasor else None
    mode = _MODES[normalize]
    stats = torch.empty((B, 2), dtype=torch.float32, device=dev) if (return_phasor or mode is not None) else None
    with torch.cuda.device(dev):
        st = L.stream_ptr(dev)
        L.call("hvit_stft_fwd", wave.data_ptr(), row_stride, L.ptr(lens), B, Ln, n_fft, hop_length,
               win.data_ptr(), T, mag.data_ptr(), L.ptr(phasor), L.ptr(stats), st)
        if mode is not None:
            L.call("hvit_spec_normalize", mag.data_ptr(), B, F, T, L.ptr(lens), hop_length, stats.data_ptr(), mode, st)
    if return_phasor:
        return mag, phasor, stats
    return mag


def istft_mag(mag: torch.Tensor, phasor: torch.Tensor, lengths_or_length: Union[int, Sequence[int], torch.Tensor],
              gain: Optional[torch.Tensor] = None, hop_length: int = 128, win_length: int = 512,
              length: Optional[int] = None) -> torch.Tensor:
    """``wave [B, L]``: row b is ``istft(gain[b] * mag[b] * phasor[b],
    length=len_b)`` followed by zeros.  ``lengths_or_length`` is one int (every
    row) or per-row lengths; ``length`` fixes L (default: the longest row,
    which reads a device tensor of lengths back)."""
    _need_gpu(mag, "mag")
    _need_gpu(phasor, "phasor")
    if mag.dim() == 4 and mag.shape[1] == 1:
        mag = mag[:, 0]
    if mag.dim() != 3 or mag.dtype != torch.float32:
        raise ValueError(f"hvit frontend: mag must be float32 [B, 1, F, T] or [B, F, T], got {tuple(mag.shape)}")
    B, F, T = mag.shape
    n_fft = 2 * (F - 1)
    _check(n_fft, hop_length, win_length)
    if tuple(phasor.shape) != (B, F, T, 2) or phasor.dtype != torch.float32:
        raise ValueError(f"hvit frontend: phasor must be float32 {(B, F, T, 2)}, got {tuple(phasor.shape)}")
    dev = mag.device
    mag, phasor = mag.contiguous(), phasor.contiguous()
    if isinstance(lengths_or_length, (int, np.integer)):
        lens, Ln = None, int(lengths_or_length)
    else:
        if length is None:
            length = int(torch.as_tensor(lengths_or_length).max())
        lens, Ln = lengths_arg(lengths_or_length, B, dev, "hvit frontend"), int(length)
    if Ln < 1:
        raise ValueError(f"hvit frontend: output length {Ln}")
    if gain is not None:
        _need_gpu(gain, "gain")
        gain = gain.to(device=dev, dtype=torch.float32).contiguous()
        if gain.shape != (B,):
            raise ValueError(f"hvit frontend: gain must have shape ({B},)")
    win = window_table(n_fft, win_length, dev)
    out = torch.empty((B, Ln), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.call("hvit_istft", mag.data_ptr(), phasor.data_ptr(), L.ptr(gain), L.ptr(lens), B, F, T, hop_length,
               win.data_ptr(), Ln, out.data_ptr(), L.stream_ptr(dev))
    return out


__all__ = ["supported", "n_frames", "stft_mag", "istft_mag", "window_table"]
