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
output the framing stays parity unpinned.  WAV I/O uses
``scipy.io.wavfile`` (soundfile is absent).  By default a file at another sample
rate is refused (``read_wav``); with ``resample=True`` it is read at its own
rate (``read_audio``), uploaded and resampled to ``sample_rate`` on the device
(resampler.py, csrc/wave_resample.hip), as the reference's ``librosa.load(path,
sr=16000)`` does on the host; parity with librosa's own resampler is unpinned
too.  The model call itself is the HIP path.
"""

from __future__ import annotations

from pathlib import Path
from typing import Union

import numpy as np
import torch
import torch.nn as nn


def _window(win_length: int, window: str) -> torch.Tensor:
    if window != "hann":
        raise NotImplementedError(f"hvit enhancer: window {window!r} (the reference uses 'hann')")
    return torch.hann_window(win_length, dtype=torch.float64)  # periodic, like librosa's get_window


class AudioEnhancer:
    """inference/enhancer.py:15-56 (constructor) and :57-135 (enhance).
    ``resample=True``: ``enhance_file``, ``enhance_directory`` and
    ``enhance_batch(rates=...)`` take audio at any rate and resample it to
    ``sample_rate`` on the device first; the default refuses another rate."""

    def __init__(self, model: nn.Module, device: str = "cuda", sample_rate: int = 16000, n_fft: int = 512,
                 hop_length: int = 128, win_length: int = 512, window: str = "hann", frontend: str = "host",
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
            return self._enhance_device([noisy_audio], normalize)[0]
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
    def _enhance_device_tensor(self, clips, normalize: bool, wave=None, lengths=None, peak=None):
        """Non-empty clips of one frame count through the device front end as
        one batch: host peak normalisation, one upload, stft_mag
        (max-normalised) -> model -> istft_mag with gain = mag_max * max_val
        taken from the kernel's stats on the device (no read-back).  Returns
        the enhanced batch ``[B, Lmax]`` (row r is clip r followed by zeros) and
        the int32 lengths, both on the device.

        With ``wave`` (a device batch ``[B, Lmax]`` as resample_wave leaves it,
        zeros past each row's length), its int32 device ``lengths`` and its
        device ``peak`` (max |row|) instead of ``clips``, nothing is uploaded:
        the peak normalisation is a device divide."""
        from . import frontend as FE

        if wave is not None:
            ln, Lmax = lengths, int(wave.shape[1])
            if normalize:
                pk = torch.where(peak > 1e-8, peak, torch.ones_like(peak))
                w = wave / pk[:, None]
            else:
                pk, w = torch.ones_like(peak), wave
        else:
            lens = [int(c.size) for c in clips]
            Lmax = max(lens)
            host = np.zeros((len(clips), Lmax), dtype=np.float32)
            hpeak = np.ones(len(clips), dtype=np.float32)
            for r, c in enumerate(clips):
                if normalize:
                    mv = float(np.abs(c).max())
                    if mv > 1e-8:
                        c = c / mv
                        hpeak[r] = mv
                host[r, :lens[r]] = c
            dev = torch.device(self.device)
            w = torch.from_numpy(host).to(dev)
            ln = torch.as_tensor(lens, dtype=torch.int32).to(dev)
            pk = torch.from_numpy(hpeak).to(dev)
        mag, phasor, stats = FE.stft_mag(w, ln, self.n_fft, self.hop_length, self.win_length, return_phasor=True,
                                         normalize="max")
        enh = self.model(mag)
        enh = enh.reshape(mag.shape).float().contiguous()
        mx = stats[:, 1]
        gain = torch.where(mx > 1e-8, mx, torch.ones_like(mx)) * pk
        return FE.istft_mag(enh, phasor, ln, gain, self.hop_length, self.win_length, length=Lmax), ln

    def _enhance_device(self, clips, normalize: bool):
        """``_enhance_device_tensor`` downloaded: one float32 array per clip
        (an empty clip stays empty)."""
        lens = [int(c.size) for c in clips]
        out = [np.zeros(0, dtype=np.float32) if n == 0 else None for n in lens]
        idx = [i for i, n in enumerate(lens) if n > 0]
        if not idx:
            return out
        y = self._enhance_device_tensor([clips[i] for i in idx], normalize)[0].cpu().numpy()
        for r, i in enumerate(idx):
            out[i] = y[r, :lens[i]].copy()
        return out

    def frame_count_batches(self, lengths, batch_size: int):
        """Index lists for ``enhance_batch``: clips grouped by frame count
        ``1 + len // hop``, the groups in ascending order, each cut into runs of
        at most ``batch_size`` in input order."""
        batch_size = max(1, int(batch_size))
        groups = {}
        for i, n in enumerate(lengths):
            groups.setdefault(1 + int(n) // self.hop_length, []).append(i)
        return [members[s:s + batch_size] for _, members in sorted(groups.items())
                for s in range(0, len(members), batch_size)]

    def _resample_clips(self, clips, rate: int):
        """Host clips at ``rate`` uploaded as one zero-padded batch and resampled
        to ``sample_rate`` on the device: ``(wave [B, Lmax], lengths int32 [B],
        peak [B] = max |row|)`` on the device and the lengths as a host list."""
        from .resampler import resample_wave

        lens = [int(c.size) for c in clips]
        host = np.zeros((len(clips), max(lens)), dtype=np.float32)
        for r, c in enumerate(clips):
            host[r, :lens[r]] = c
        raw = torch.from_numpy(host).to(torch.device(self.device))
        wave, ln, peak = resample_wave(raw, lens, rate, self.sample_rate, return_peak=True)
        return wave, ln, peak, [_out_length(n, rate, self.sample_rate) for n in lens]

    @torch.no_grad()
    def _enhance_resampled(self, clips, rates, normalize: bool, batch_size: int):
        """``enhance_batch`` for clips at their own ``rates``: grouped by (rate,
        frame count of the resampled clip); a group at another rate is uploaded
        raw and resampled on the device, and its peak normalisation uses the
        maximum of the RESAMPLED clip (the reference normalises what
        librosa.load returned).  The device front end takes the resampled batch
        as it stands; the host front end downloads it and loops ``enhance``."""
        batch_size = max(1, int(batch_size))
        out = [None] * len(clips)
        groups = {}
        for i, (c, r) in enumerate(zip(clips, rates)):
            n = _out_length(c.size, r, self.sample_rate)
            if n == 0:
                out[i] = np.zeros(0, dtype=np.float32)
            else:
                groups.setdefault((int(r), 1 + n // self.hop_length), []).append(i)
        for (rate, _), members in sorted(groups.items()):
            for s in range(0, len(members), batch_size):
                part = members[s:s + batch_size]
                if rate == self.sample_rate:
                    ys = (self._enhance_device([clips[i] for i in part], normalize) if self.frontend == "device"
                          else [self.enhance(clips[i], normalize=normalize) for i in part])
                else:
                    wave, ln, peak, lens = self._resample_clips([clips[i] for i in part], rate)
                    if self.frontend == "device":
                        y = self._enhance_device_tensor(None, normalize, wave=wave, lengths=ln, peak=peak)[0]
                        y = y.cpu().numpy()
                        ys = [y[r, :lens[r]].copy() for r in range(len(part))]
                    else:
                        w = wave.cpu().numpy()
                        ys = [self.enhance(w[r, :lens[r]], normalize=normalize) for r in range(len(part))]
                for i, y in zip(part, ys):
                    out[i] = y
        return out

    def enhance_batch(self, clips, normalize: bool = True, batch_size: int = 32, rates=None):
        """Enhance a list of clips; results in input order.  Clips are grouped
        by frame count ``1 + len // hop`` and, within a group, right-zero-padded
        to the longest member (exact: with constant padding a zero-extended row
        has the same frames); each group runs as forwards of at most
        ``batch_size`` clips.  With the host front end this loops ``enhance``.

        ``rates`` (optional, one sample rate per clip): a clip at another rate
        than ``sample_rate`` needs ``resample=True``; it is resampled on the
        device and the result is at ``sample_rate``."""
        clips = [np.asarray(c, dtype=np.float32) for c in clips]
        if rates is not None:
            rates = [int(r) for r in rates]
            if len(rates) != len(clips):
                raise ValueError("hvit enhancer: rates must give one sample rate per clip")
            if any(r != self.sample_rate for r in rates):
                if not self.resample:
                    bad = next(r for r in rates if r != self.sample_rate)
                    raise ValueError(f"hvit enhancer: a clip is {bad} Hz, expected {self.sample_rate} "
                                     "(construct the enhancer with resample=True)")
                return self._enhance_resampled(clips, rates, normalize, batch_size)
        if self.frontend == "host":
            return [self.enhance(c, normalize=normalize) for c in clips]
        out = [None] * len(clips)
        for part in self.frame_count_batches([c.size for c in clips], batch_size):
            for i, y in zip(part, self._enhance_device([clips[i] for i in part], normalize)):
                out[i] = y
        return out

    def _restore_rate(self, audio: np.ndarray, rate: int, n_samples: int) -> np.ndarray:
        """``audio`` (at ``sample_rate``) resampled on the device to ``rate``
        and cut to ``n_samples`` (the back-conversion never comes out shorter)."""
        from .resampler import resample_wave

        if audio.size == 0:
            return np.zeros(n_samples, dtype=np.float32)
        w = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32))[None].to(torch.device(self.device))
        y = resample_wave(w, [audio.size], self.sample_rate, rate)[0][0, :n_samples].cpu().numpy()
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


def read_wav(path: Union[str, Path], sample_rate: int) -> np.ndarray:
    """Mono float32 in [-1, 1] (the reference's librosa.load(sr, mono=True),
    without resampling: a different rate is an error)."""
    from scipy.io import wavfile

    sr, data = wavfile.read(str(path))
    if sr != sample_rate:
        raise ValueError(f"hvit enhancer: {path} is {sr} Hz, expected {sample_rate} (no resampler here)")
    return _mono_float32(data)


def _mono_float32(data: np.ndarray) -> np.ndarray:
    if np.issubdtype(data.dtype, np.integer):
        data = data.astype(np.float32) / float(np.iinfo(data.dtype).max + 1)
    data = data.astype(np.float32)
    return data.mean(axis=1) if data.ndim == 2 else data


def read_audio(path: Union[str, Path]):
    """``(mono float32 in [-1, 1], sample rate)``: ``read_wav`` without the
    rate check (librosa.load(sr=None, mono=True)); the caller resamples."""
    from scipy.io import wavfile

    sr, data = wavfile.read(str(path))
    return _mono_float32(data), int(sr)


def _out_length(n: int, orig_sr: int, target_sr: int) -> int:
    from .resampler import out_length, ratio

    return out_length(n, *ratio(orig_sr, target_sr))


def write_wav(path: Union[str, Path], audio: np.ndarray, sample_rate: int) -> None:
    from scipy.io import wavfile

    wavfile.write(str(path), sample_rate, np.asarray(audio, dtype=np.float32))


def enhance_audio(noisy_audio: np.ndarray, model: nn.Module, device: str = "cuda", sample_rate: int = 16000,
                  n_fft: int = 512, hop_length: int = 128) -> np.ndarray:
    """enhancer.py:198-226."""
    return AudioEnhancer(model, device, sample_rate, n_fft, hop_length).enhance(noisy_audio)


def enhance_file(input_path, output_path, model: nn.Module, device: str = "cuda", sample_rate: int = 16000) -> None:
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


def synthetic_clip(seconds: float = 2.0, seed: int = 0, sample_rate: int = 16000) -> np.ndarray:
    """A noisy harmonic clip (data.harmonic_pair) for plumbing checks (config 1)."""
    from .data import harmonic_pair

    return harmonic_pair(int(round(seconds * sample_rate)), seed)[1]


__all__ = ["AudioEnhancer", "enhance_audio", "enhance_file", "load_model_for_inference", "read_wav", "read_audio", "write_wav",
           "synthetic_clip"]
