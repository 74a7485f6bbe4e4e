"""Audio enhancement around the HybridViT hot path (BASELINE
config 1): the reference's ``AudioEnhancer`` (inference/enhancer.py:15-290)
with the same call surface -- ``enhance``, ``enhance_file``,
``enhance_directory``, ``enhance_audio``, ``enhance_file`` (module level) and
``load_model_for_inference``.

STFT / iSTFT framing runs on the host by default (``frontend="host"``), as the
north star says; ``frontend="device"`` moves it to the HIP kernels of
frontend.py (csrc/stft.hip, f32), where a batch of clips goes waveform ->
spectrogram -> model -> waveform on the device (``enhance_batch``).  librosa is
not available here, so the host framing is ``torch.stft`` / ``torch.istft`` with the
reference's settings (n_fft 512, hop 128, win 512, periodic Hann,
center=True, constant padding -- librosa >= 0.10's ``pad_mode`` default;
enhancer.py:82-89, :111-118).  tests/test_enhancer.py checks both against a
numpy restatement of librosa 0.10's algorithm (oracle/stft_restated.py; an
inconsistent spectrum for the iSTFT, ragged lengths); against librosa's own
output the framing stays parity unpinned.  WAV I/O and the device
batches (``WaveBatch``) live in audio.py; ``read_wav``,
``read_audio`` and ``write_wav`` are re-exported here.  By default a file at
another sample rate is refused (``read_wav``); with ``resample=True`` it is read
at its own rate (``read_audio``), uploaded and resampled to ``sample_rate`` on
the device (resampler.py), as the reference's ``librosa.load(path, sr=16000)``
does on the host; parity with librosa's own resampler is unpinned too (DESIGN
§16).  The model call itself is the HIP path.
"""

from __future__ import annotations

from pathlib import Path
from typing import Union

import numpy as np
import torch
import torch.nn as nn

from .audio import HOP, N_FFT, SR, WIN, WaveBatch, batches, out_length, read_audio, read_wav, write_wav


def _window(win_length: int, window: str) -> torch.Tensor:
    if window != "hann":
        raise NotImplementedError(f"hvit enhancer: window {window!r} (the reference uses 'hann')")
    return torch.hann_window(win_length, dtype=torch.float64)  # periodic, like librosa's get_window


class AudioEnhancer:
    """inference/enhancer.py:15-56 (constructor) and :57-135 (enhance).
    ``resample=True``: ``enhance_file``, ``enhance_directory`` and
    ``enhance_batch(rates=...)`` take audio at any rate and resample it to
    ``sample_rate`` on the device first; the default refuses another rate."""

    def __init__(self, model: nn.Module, device: str = "cuda", sample_rate: int = SR, n_fft: int = N_FFT,
                 hop_length: int = HOP, win_length: int = WIN, window: str = "hann", frontend: str = "host",
                 resample: bool = False):
        if frontend not in ("host", "device"):
            raise ValueError(f"hvit enhancer: frontend {frontend!r} ('host' or 'device')")
        if frontend == "device":
            from . import frontend as FE

            if window != "hann":
                raise ValueError(f"hvit enhancer: the device front end has no window {window!r} (only 'hann')")
            if not FE.supported(n_fft, hop_length, win_length):
                raise ValueError(f"hvit enhancer: the device front end does not support n_fft={n_fft}, "
                                 f"hop_length={hop_length}, win_length={win_length}")
        self.frontend = frontend
        self.resample = bool(resample)
        self.model = model.to(device).eval()
        self.device = device
        self.sample_rate = sample_rate
        self.n_fft = n_fft
        self.hop_length = hop_length
        self.win_length = win_length
        self.window = window

    def stft(self, audio: np.ndarray) -> torch.Tensor:
        x = torch.as_tensor(np.asarray(audio, dtype=np.float64))
        return torch.stft(x, self.n_fft, self.hop_length, self.win_length, window=_window(self.win_length, self.window),
                          center=True, pad_mode="constant", return_complex=True)

    def istft(self, spec: torch.Tensor, length: int) -> np.ndarray:
        y = torch.istft(spec, self.n_fft, self.hop_length, self.win_length,
                        window=_window(self.win_length, self.window), center=True, length=length)
        return y.numpy()

    @torch.no_grad()
    def enhance(self, noisy_audio: np.ndarray, normalize: bool = True) -> np.ndarray:
        noisy_audio = np.asarray(noisy_audio, dtype=np.float32)
        if self.frontend == "device":
            return self.enhance_batch([noisy_audio], normalize=normalize)[0]
        max_val = 1.0
        if normalize:
            mv = float(np.abs(noisy_audio).max()) if noisy_audio.size else 0.0
            if mv > 1e-8:
                noisy_audio = noisy_audio / mv
                max_val = mv
        spec = self.stft(noisy_audio)
        mag, phase = spec.abs(), spec.angle()
        mag_max = float(mag.max())
        if mag_max > 1e-8:
            mag_n = mag / mag_max
        else:
            mag_n, mag_max = mag, 1.0
        x = mag_n.float()[None, None].to(self.device)  # [1, 1, F, T]
        enh = self.model(x).squeeze().double().cpu() * mag_max
        out = self.istft(torch.polar(enh, phase), len(noisy_audio))
        if normalize:
            out = out * max_val
        return out.astype(np.float32)

    @torch.no_grad()
    def _enhance_device_tensor(self, batch: WaveBatch, normalize: bool) -> torch.Tensor:
        """A batch of non-empty clips of one frame count (with its ``peak``)
        through the device front end: peak normalisation as a device divide,
        stft_mag (max-normalised) -> model -> istft_mag with gain = mag_max *
        peak from the kernel's stats (no read-back).  Returns the enhanced
        batch ``[B, Lmax]`` on the device (row r is clip r, then zeros)."""
        from . import frontend as FE

        pk = torch.ones_like(batch.peak)
        w = batch.wave
        if normalize:
            pk = torch.where(batch.peak > 1e-8, batch.peak, pk)
            w = w / pk[:, None]
        mag, phasor, stats = FE.stft_mag(w, batch.lengths, self.n_fft, self.hop_length, self.win_length,
                                         return_phasor=True, normalize="max")
        enh = self.model(mag)
        enh = enh.reshape(mag.shape).float().contiguous()
        mx = stats[:, 1]
        gain = torch.where(mx > 1e-8, mx, torch.ones_like(mx)) * pk
        return FE.istft_mag(enh, phasor, batch.lengths, gain, self.hop_length, self.win_length,
                            length=int(w.shape[1]))

    def frame_count_batches(self, lengths, batch_size: int):
        """Index lists for ``enhance_batch``: clips grouped by frame count
        ``1 + len // hop``, the groups in ascending order, each cut into runs of
        at most ``batch_size`` in input order."""
        return batches([1 + int(n) // self.hop_length for n in lengths], batch_size)

    def enhance_batch(self, clips, normalize: bool = True, batch_size: int = 32, rates=None):
        """Enhance a list of clips; results in input order.  Clips are grouped
        by (rate, frame count ``1 + len // hop`` at ``sample_rate``) and, within
        a group, right-zero-padded to the longest member (exact: with constant
        padding a zero-extended row has the same frames); each group runs as
        ``WaveBatch``es of at most ``batch_size`` clips, which the device front
        end enhances as they stand and the host front end downloads for
        ``enhance``.  An empty clip gives an empty array and joins no batch.
        With the host front end and every clip at ``sample_rate`` this only
        loops ``enhance``: nothing but the model touches the GPU.

        ``rates`` (optional, one per clip): a clip at another rate needs
        ``resample=True``; it is uploaded raw and resampled on the device, and
        its peak normalisation uses the maximum of the RESAMPLED clip (the
        reference normalises what librosa.load returned)."""
        clips = [np.asarray(c, dtype=np.float32) for c in clips]
        rates = [self.sample_rate] * len(clips) if rates is None else [int(r) for r in rates]
        if len(rates) != len(clips):
            raise ValueError("hvit enhancer: rates must give one sample rate per clip")
        bad = next((r for r in rates if r != self.sample_rate), None)
        if bad is not None and not self.resample:
            raise ValueError(f"hvit enhancer: a clip is {bad} Hz, expected {self.sample_rate} "
                             "(construct the enhancer with resample=True)")
        if bad is None and self.frontend == "host":
            return [self.enhance(c, normalize=normalize) for c in clips]
        lens = [out_length(c.size, r, self.sample_rate) for c, r in zip(clips, rates)]
        out = [np.zeros(0, dtype=np.float32) if n == 0 else None for n in lens]
        todo = [i for i, n in enumerate(lens) if n > 0]
        for part in batches([(rates[i], 1 + lens[i] // self.hop_length) for i in todo], batch_size):
            part = [todo[j] for j in part]
            batch = WaveBatch.from_clips([clips[i] for i in part], self.device, rates[part[0]], self.sample_rate,
                                         peak=True)
            if self.frontend == "device":
                ys = WaveBatch(self._enhance_device_tensor(batch, normalize), batch.lengths, batch.lens).rows()
            else:
                ys = [self.enhance(w, normalize=normalize) for w in batch.rows()]
            for i, y in zip(part, ys):
                out[i] = y
        return out

    def _restore_rate(self, audio: np.ndarray, rate: int, n_samples: int) -> np.ndarray:
        """``audio`` (at ``sample_rate``) resampled on the device to ``rate``
        and cut to ``n_samples`` (the back-conversion never comes out shorter)."""
        if audio.size == 0:
            return np.zeros(n_samples, dtype=np.float32)
        y = WaveBatch.from_clips([audio], self.device, self.sample_rate, rate).rows()[0][:n_samples]
        return np.pad(y, (0, n_samples - y.size))

    def enhance_file(self, input_path: Union[str, Path], output_path: Union[str, Path],
                     normalize: bool = True, keep_rate: bool = False) -> None:
        """With ``resample=True`` a file at any rate is enhanced and written at
        ``sample_rate``, as the reference does; ``keep_rate`` resamples the
        result back and writes it at the input file's rate with the input's
        sample count."""
        rate = self.sample_rate
        if self.resample:
            audio, sr = read_audio(input_path)
            out = self.enhance_batch([audio], normalize=normalize, rates=[sr])[0]
            if keep_rate and sr != self.sample_rate:
                out, rate = self._restore_rate(out, sr, audio.size), sr
        else:
            audio = read_wav(input_path, self.sample_rate)
            out = self.enhance(audio, normalize=normalize)
        output_path = Path(output_path)
        output_path.parent.mkdir(parents=True, exist_ok=True)
        write_wav(output_path, out, rate)
        print(f"Enhanced audio saved to {output_path}")

    def enhance_directory(self, input_dir: Union[str, Path], output_dir: Union[str, Path], extension: str = ".wav",
                          normalize: bool = True, batch_size: int = 1) -> None:
        files = sorted(Path(input_dir).glob(f"*{extension}"))
        Path(output_dir).mkdir(parents=True, exist_ok=True)
        print(f"Found {len(files)} audio files to enhance")
        if batch_size > 1:
            for s in range(0, len(files), batch_size):
                part = files[s:s + batch_size]
                if self.resample:
                    read = [read_audio(f) for f in part]
                    outs = self.enhance_batch([a for a, _ in read], normalize=normalize, batch_size=batch_size,
                                              rates=[sr for _, sr in read])
                else:
                    outs = self.enhance_batch([read_wav(f, self.sample_rate) for f in part], normalize=normalize,
                                              batch_size=batch_size)
                for f, o in zip(part, outs):
                    write_wav(Path(output_dir) / f.name, o, self.sample_rate)
                    print(f"Enhanced audio saved to {Path(output_dir) / f.name}")
        else:
            for f in files:
                self.enhance_file(f, Path(output_dir) / f.name, normalize=normalize)
        print(f"All files enhanced and saved to {output_dir}")


def enhance_audio(noisy_audio: np.ndarray, model: nn.Module, device: str = "cuda", sample_rate: int = SR,
                  n_fft: int = N_FFT, hop_length: int = HOP) -> np.ndarray:
    """enhancer.py:198-226."""
    return AudioEnhancer(model, device, sample_rate, n_fft, hop_length).enhance(noisy_audio)


def enhance_file(input_path, output_path, model: nn.Module, device: str = "cuda", sample_rate: int = SR) -> None:
    """enhancer.py:229-255."""
    AudioEnhancer(model, device, sample_rate).enhance_file(input_path, output_path)


def load_model_for_inference(checkpoint_path: Union[str, Path], model: nn.Module, device: str = "cuda",
                             strict: bool = True) -> nn.Module:
    """enhancer.py:258-290 with a loader that executes nothing from the file
    (weights_only=True): a Trainer checkpoint dict (``model_state_dict``,
    trainer.py:350-380) or a bare state_dict."""
    ckpt = torch.load(str(checkpoint_path), map_location="cpu", weights_only=True)
    sd = ckpt["model_state_dict"] if isinstance(ckpt, dict) and "model_state_dict" in ckpt else ckpt
    model.load_state_dict(sd, strict=strict)
    return model.to(device).eval()


def synthetic_clip(seconds: float = 2.0, seed: int = 0, sample_rate: int = SR) -> np.ndarray:
    """A noisy harmonic clip (data.harmonic_pair) for plumbing checks (config 1)."""
    from .data import harmonic_pair

    return harmonic_pair(int(round(seconds * sample_rate)), seed)[1]


__all__ = ["AudioEnhancer", "enhance_audio", "enhance_file", "load_model_for_inference", "read_wav", "read_audio", "write_wav",
           "synthetic_clip"]
