"""Host clips and device wave batches: the one place where WAV
files are read and written (``scipy.io.wavfile``; soundfile is absent), where a
list of host clips becomes a zero-padded float32 batch, and where that batch is
uploaded and resampled.  The enhancer, the Evaluator and SpectrogramStore build
their batches here; together ``read_audio`` and ``WaveBatch.from_clips`` are the
reference's ``librosa.load(path, sr=16000, mono=True)`` for a whole batch.
"""

from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional, Union

import numpy as np
import torch

from . import resampler as R

SR, N_FFT, HOP, WIN = 16000, 512, 128, 512


def read_audio(path: Union[str, Path]):
    """``(mono float32 in [-1, 1], sample rate)`` of a WAV file; the caller resamples."""
    from scipy.io import wavfile

    sr, data = wavfile.read(str(path))
    if np.issubdtype(data.dtype, np.integer):
        data = data.astype(np.float32) / float(np.iinfo(data.dtype).max + 1)
    data = data.astype(np.float32)
    return (data.mean(axis=1) if data.ndim == 2 else data), int(sr)


def read_wav(path: Union[str, Path], sample_rate: int) -> np.ndarray:
    """``read_audio`` of a file that must be at ``sample_rate``."""
    audio, sr = read_audio(path)
    if sr != sample_rate:
        raise ValueError(f"hvit enhancer: {path} is {sr} Hz, expected {sample_rate} (no resampler here)")
    return audio


def write_wav(path: Union[str, Path], audio: np.ndarray, sample_rate: int) -> None:
    from scipy.io import wavfile

    wavfile.write(str(path), sample_rate, np.asarray(audio, dtype=np.float32))


def out_length(n: int, orig_sr: int, target_sr: int) -> int:
    """Samples of an ``n``-sample clip after resampling: ``ceil(n * up / down)``."""
    return R.out_length(n, *R.ratio(orig_sr, target_sr))


def pad_rows(clips, width: Optional[int] = None) -> np.ndarray:
    """Float32 ``[B, width]`` on the host (default: the longest clip): row r is
    ``clips[r][:width]`` followed by zeros."""
    clips = [np.asarray(c, dtype=np.float32).reshape(-1) for c in clips]
    if width is None:
        width = max(c.size for c in clips)
    host = np.zeros((len(clips), int(width)), dtype=np.float32)
    for r, c in enumerate(clips):
        host[r, :min(c.size, width)] = c[:width]
    return host


def upload_rows(clips, device, width: Optional[int] = None) -> torch.Tensor:
    """``pad_rows`` as a device tensor: one upload."""
    return torch.from_numpy(pad_rows(clips, width)).to(device)


def batches(keys, batch_size: int) -> List[List[int]]:
    """Index lists over ``keys``: equal keys together, the groups in ascending
    key order, each cut into runs of at most ``batch_size`` in input order."""
    batch_size = max(1, int(batch_size))
    groups = {}
    for i, k in enumerate(keys):
        groups.setdefault(k, []).append(i)
    return [members[s:s + batch_size] for _, members in sorted(groups.items())
            for s in range(0, len(members), batch_size)]


@dataclass
class WaveBatch:
    """Clips on the device: ``wave`` float32 ``[B, L]`` with zeros past each
    row's length, ``lengths`` int32 ``[B]`` on the device, ``lens`` the same on
    the host, and optionally ``peak`` ``[B]`` = max |row| on the device."""

    wave: torch.Tensor
    lengths: torch.Tensor
    lens: List[int]
    peak: Optional[torch.Tensor] = None

    @classmethod
    def from_clips(cls, clips, device, rate: int, target_rate: int, peak: bool = False) -> "WaveBatch":
        """Host clips at ``rate`` (not all empty) as one batch at ``target_rate``:
        one upload and, when the rates differ, one resample_wave, whose ``peak``
        is that of the RESAMPLED row; at equal rates it is the host maximum."""
        clips = [np.asarray(c, dtype=np.float32).reshape(-1) for c in clips]
        lens = [int(c.size) for c in clips]
        wave = upload_rows(clips, device)
        if rate != target_rate:
            wave, lengths, *pk = R.resample_wave(wave, lens, rate, target_rate, return_peak=peak)
            return cls(wave, lengths, [out_length(n, rate, target_rate) for n in lens], pk[0] if peak else None)
        lengths = torch.as_tensor(lens, dtype=torch.int32).to(device)
        pk = None
        if peak:
            maxima = [float(np.abs(c).max()) if c.size else 0.0 for c in clips]
            pk = torch.tensor(maxima, dtype=torch.float32).to(device)
        return cls(wave, lengths, lens, pk)

    def rows(self) -> List[np.ndarray]:
        """One download: every row cut to its length, each a float32 array of its own."""
        host = self.wave.cpu().numpy()
        return [host[r, :n].copy() for r, n in enumerate(self.lens)]


__all__ = ["SR", "N_FFT", "HOP", "WIN", "read_audio", "read_wav", "write_wav", "out_length", "pad_rows", "upload_rows",
           "batches", "WaveBatch"]
