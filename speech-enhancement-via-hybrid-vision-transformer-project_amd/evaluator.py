"""Dataset evaluation (the reference's ``Evaluator``, evaluation/evaluator.py:20-309,
with the same methods, result dict and JSON schema) around ``AudioEnhancer``
and the metrics of metrics.py.

``frontend="host"`` (default) enhances clip by clip with the host framing and
scores with the numpy functions, as the reference does.  ``frontend="device"``
keeps a batch on the GPU from the noisy waveform to the scores: the pairs are
grouped by frame count as ``AudioEnhancer.enhance_batch`` groups them, each
batch is enhanced by the device front end, scored there
(``all_metrics_batch``: enhanced and noisy against clean in one
``wave_metrics`` call of 2 B rows, one ``lsd`` call) and only the small table
of scores is downloaded.  A pair is cut to its shorter member before it is
enhanced, and ``save_enhanced`` writes the waveform that was scored.  Files are
read and the batches built by audio.py (``WaveBatch``, ``upload_rows``).
"""

from __future__ import annotations

import json
from pathlib import Path
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from . import metrics as M
from .audio import HOP, N_FFT, SR, WIN, WaveBatch, read_audio, read_wav, upload_rows, write_wav
from .enhancer import AudioEnhancer


class Evaluator:
    """evaluation/evaluator.py:27-52 plus ``frontend`` ("host" or "device"),
    ``batch_size`` (pairs per device batch), ``precision`` (None keeps the
    model's; "fp32" / "bf16" sets a HybridViT's forward precision) and
    ``resample`` (True: a file at another rate is resampled to ``sample_rate``
    on the device as it is loaded, noisy and clean each at its own rate, as the
    reference's librosa.load(sr=16000) does; the metrics are always computed at
    ``sample_rate``.  The default refuses such a file) and ``stoi`` ("package":
    the ``pystoi`` package, 0.0 without it; "native": ``metrics.stoi`` on the
    device front end, ``metrics.stoi_reference`` on the host one)."""

    def __init__(self, model: nn.Module, device: str = "cuda", sample_rate: int = SR, n_fft: int = N_FFT,
                 hop_length: int = HOP, win_length: int = WIN, frontend: str = "host", batch_size: int = 32,
                 precision: Optional[str] = None, resample: bool = False, stoi: str = "package"):
        if stoi not in ("package", "native"):
            raise ValueError(f"hvit evaluator: stoi={stoi!r} ('package' or 'native')")
        if batch_size < 1:
            raise ValueError(f"hvit evaluator: batch_size={batch_size}")
        if precision is not None:
            if precision not in ("fp32", "bf16"):
                raise ValueError(f"hvit evaluator: precision {precision!r} (None, 'fp32' or 'bf16')")
            if not hasattr(model, "precision"):
                raise ValueError(f"hvit evaluator: {type(model).__name__} has no precision to set")
            model.precision = precision
        self.enhancer = AudioEnhancer(model, device, sample_rate, n_fft, hop_length, win_length, frontend=frontend)
        self.model = self.enhancer.model
        self.device = device
        self.sample_rate = sample_rate
        self.n_fft = n_fft
        self.hop_length = hop_length
        self.win_length = win_length
        self.frontend = frontend
        self.batch_size = int(batch_size)
        self.resample = bool(resample)
        self.stoi = stoi

    def enhance_audio(self, noisy_audio: np.ndarray) -> np.ndarray:
        """evaluator.py:54-117."""
        return self.enhancer.enhance(noisy_audio)

    def _read(self, path) -> np.ndarray:
        """One file at ``sample_rate``: refused at another rate by default;
        with ``resample`` read at its own rate and resampled on the device."""
        if not self.resample:
            return read_wav(path, self.sample_rate)
        audio, sr = read_audio(path)
        if sr == self.sample_rate or audio.size == 0:
            return audio
        return WaveBatch.from_clips([audio], self.device, sr, self.sample_rate).rows()[0]

    def _load_pair(self, noisy_path, clean_path):
        noisy = self._read(noisy_path)
        clean = self._read(clean_path)
        n = min(len(noisy), len(clean))
        return np.ascontiguousarray(noisy[:n]), np.ascontiguousarray(clean[:n])

    def _score_host(self, noisy: np.ndarray, clean: np.ndarray):
        enhanced = self.enhance_audio(noisy)[:len(clean)]
        return M.compute_all_metrics(clean, enhanced, noisy, self.sample_rate, stoi=self.stoi), enhanced

    @torch.no_grad()
    def _score_device(self, noisy_clips, clean_clips):
        """One batch of pairs with one frame count: a list of metric dicts and
        the enhanced batch ``[B, Lmax]`` on the device."""
        n = len(noisy_clips)
        batch = WaveBatch.from_clips(noisy_clips, self.device, self.sample_rate, self.sample_rate, peak=True)
        enhanced = self.enhancer._enhance_device_tensor(batch, True)
        ref = upload_rows(clean_clips + noisy_clips, enhanced.device, width=enhanced.shape[1])
        scores = M.all_metrics_batch(ref[:n], enhanced, ref[n:], batch.lengths, stoi=self.stoi, sr=self.sample_rate)
        names = list(scores)
        table = torch.stack([scores[k] for k in names]).cpu().numpy()  # the batch's one download
        return [{k: float(table[j, r]) for j, k in enumerate(names)} for r in range(n)], enhanced

    def evaluate_pair(self, noisy_path: Path, clean_path: Path) -> Dict[str, float]:
        """evaluator.py:119-155."""
        noisy, clean = self._load_pair(noisy_path, clean_path)
        if self.frontend == "device":
            return self._score_device([noisy], [clean])[0][0]
        return self._score_host(noisy, clean)[0]

    def evaluate_dataset(self, noisy_dir: Path, clean_dir: Path, output_dir: Optional[Path] = None,
                         save_enhanced: bool = False) -> Dict[str, object]:
        """evaluator.py:157-231: every ``*.wav`` of ``noisy_dir`` with a file of
        the same name in ``clean_dir``."""
        noisy_files = sorted(Path(noisy_dir).glob("*.wav"))
        if not noisy_files:
            raise ValueError(f"No .wav files found in {noisy_dir}")
        print(f"Evaluating {len(noisy_files)} audio files...")
        save = bool(save_enhanced and output_dir)
        if save:
            output_dir = Path(output_dir)
            output_dir.mkdir(parents=True, exist_ok=True)
        names, pairs = [], []
        for f in noisy_files:
            if not (Path(clean_dir) / f.name).exists():
                print(f"Warning: No clean file found for {f.name}")
                continue
            pair = self._load_pair(f, Path(clean_dir) / f.name)
            if pair[0].size == 0:
                print(f"Warning: {f.name} has no samples")
                continue
            names.append(f.name)
            pairs.append(pair)

        per_file = {}
        if self.frontend == "device" and names:
            for part in self.enhancer.frame_count_batches([p[0].size for p in pairs], self.batch_size):
                rows, enhanced = self._score_device([pairs[i][0] for i in part], [pairs[i][1] for i in part])
                waves = enhanced.cpu().numpy() if save else None
                for r, i in enumerate(part):
                    per_file[names[i]] = rows[r]
                    if save:
                        write_wav(output_dir / names[i], waves[r, :pairs[i][0].size], self.sample_rate)
            per_file = {k: per_file[k] for k in names}
        else:
            for k, (noisy, clean) in zip(names, pairs):
                per_file[k], enhanced = self._score_host(noisy, clean)
                if save:
                    write_wav(output_dir / k, enhanced, self.sample_rate)

        average = {}
        if per_file:
            for key in next(iter(per_file.values())):
                values = [m[key] for m in per_file.values()]
                average[key] = np.mean(values)
                average[f"{key}_std"] = np.std(values)
        return {"per_file_metrics": per_file, "average_metrics": average, "num_files": len(per_file)}

    def save_results(self, results: Dict, output_path: Path) -> None:
        """evaluator.py:233-263: ``num_files``, ``average_metrics``, ``per_file_metrics`` as JSON."""
        output_path = Path(output_path)
        output_path.parent.mkdir(parents=True, exist_ok=True)
        doc = {
            "num_files": results["num_files"],
            "average_metrics": {k: float(v) for k, v in results["average_metrics"].items()},
            "per_file_metrics": {name: {k: float(v) for k, v in m.items()}
                                 for name, m in results["per_file_metrics"].items()},
        }
        with open(output_path, "w") as f:
            json.dump(doc, f, indent=2)
        print(f"Results saved to {output_path}")

    def print_results(self, results: Dict) -> None:
        """evaluator.py:265-309: the averages in the reference's three groups."""
        avg = results["average_metrics"]
        main = ["pesq", "stoi", "sisdr", "snr"]
        improvement = [f"{k}_improvement" for k in main]
        other = [k for k in avg if not k.endswith("_std") and k not in main and k not in improvement]

        def line(key, label):
            print(f"{label.upper():15s}: {avg[key]:7.4f} ± {avg.get(f'{key}_std', 0.0):6.4f}")

        print(f"\nEvaluation Results ({results['num_files']} files)\n" + "=" * 70)
        for title, keys in (("Main Metrics:", main), ("Improvement Over Noisy:", improvement), ("Other Metrics:", other)):
            print(f"\n{title}\n" + "-" * 70)
            for key in keys:
                if key in avg:
                    line(key, key.replace("_improvement", ""))
        print("=" * 70)


__all__ = ["Evaluator"]
