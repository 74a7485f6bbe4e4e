"""Synthetic VoiceBank-shaped spectrogram batches (host-side, no dataset).

Waveforms follow the reference notebook's synthetic generator (demo.ipynb
cell 6): f0 ~ 200 + 50 N(0,1), 7 harmonics with amplitude 1/h and random
phase, a 5 Hz envelope, peak 0.8, plus N(0, 0.15^2) noise for the noisy copy.
Spectrograms use the reference's host STFT settings (n_fft 512, hop 128,
win 512, periodic Hann, center=True; inference/enhancer.py:82-89,
data/dataset.py:183-190) and per-utterance min-max scaling
(data/dataset.py:213-219).  The framing runs on the host by default (north
star); ``spectrogram_batch(..., device=...)`` runs it and the scaling on the GPU
as one batch (frontend.py, csrc/stft.hip).  ``SpectrogramStore.from_waves``
builds its wave batches with audio.py, which defines ``SR`` etc.
"""

from __future__ import annotations

import numpy as np
import torch

from .audio import HOP, N_FFT, SR, WIN, WaveBatch, out_length, read_audio, read_wav, upload_rows


def harmonic_pair(n_samples: int, seed: int):
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n_samples) / SR
    f0 = 200.0 + 50.0 * rng.standard_normal()
    clean = np.zeros(n_samples)
    for h in range(1, 8):
        clean += (1.0 / h) * np.sin(2 * np.pi * f0 * h * t + rng.random() * 2 * np.pi)
    clean *= 0.5 + 0.5 * np.sin(2 * np.pi * 5 * t)
    clean = clean / np.abs(clean).max() * 0.8
    noisy = clean + 0.15 * rng.standard_normal(n_samples)
    return clean.astype(np.float32), noisy.astype(np.float32)


def magnitude(wave: np.ndarray) -> torch.Tensor:
    x = torch.as_tensor(wave)
    spec = torch.stft(x, N_FFT, HOP, WIN, window=torch.hann_window(WIN), center=True, pad_mode="constant",
                      return_complex=True)
    return spec.abs()


def minmax(m: torch.Tensor) -> torch.Tensor:
    lo, hi = m.min(), m.max()
    return (m - lo) / (hi - lo) if hi > lo else m


def spectrogram_batch(batch: int, freq: int = 256, frames: int = 256, seed: int = 1234, device=None):
    """(noisy, clean) magnitude batches [B, 1, freq, frames] in [0, 1].

    ``device=None`` (default) frames every clip on the host with torch.stft.
    With a GPU device the waveforms are still synthesised on the host, but the
    framing and min-max scaling of all 2 B clips run as one batch through
    frontend.stft_mag(normalize="minmax") and the result stays on the device."""
    n = (frames - 1) * HOP
    if device is not None:
        from .frontend import stft_mag

        pairs = [harmonic_pair(n, seed + i) for i in range(batch)]
        wave = np.stack([p[1] for p in pairs] + [p[0] for p in pairs])
        m = stft_mag(torch.from_numpy(wave).to(device), None, N_FFT, HOP, WIN, normalize="minmax")
        m = m[:, :, :freq, :frames]
        return m[:batch].contiguous(), m[batch:].contiguous()
    noisy, clean = [], []
    for i in range(batch):
        c, nz = harmonic_pair(n, seed + i)
        noisy.append(minmax(magnitude(nz))[:freq, :frames])
        clean.append(minmax(magnitude(c))[:freq, :frames])
    return torch.stack(noisy)[:, None].contiguous(), torch.stack(clean)[:, None].contiguous()


# ---------------------------------------------------------------------------
# Device-resident training data: the reference's VoiceBankDataset
# with cache_spectrograms (data/dataset.py:233-294), its collate_fn (:297-347)
# and get_data_loader (:350-380), with the cache in GPU memory and __getitem__,
# augment and collate as one launch per batch (csrc/batch_prep.hip).
# ---------------------------------------------------------------------------

TRAIN_DIRS = ("noisy_trainset_28spk_wav", "clean_trainset_28spk_wav")
TEST_DIRS = ("noisy_testset_wav", "clean_testset_wav")


def pack_offsets(frames, F: int):
    """Element offset of every utterance in a packed store and the store's
    total element count: utterance i is [F, frames[i]] row-major, unpadded,
    right after utterance i - 1."""
    frames = np.asarray(frames, dtype=np.int64)
    if frames.ndim != 1 or (frames < 1).any():
        raise ValueError("hvit data: frames must be a 1-D list of counts >= 1")
    sizes = frames * int(F)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    return offsets, int(sizes.sum())


def split_pairs(pairs, split: str, train_val_split: float = 0.9):
    """data/dataset.py:137-145: 'train' is the first int(n * train_val_split)
    pairs, 'val' the rest, 'test' all of them."""
    if split == "test":
        return list(pairs)
    k = int(len(pairs) * train_val_split)
    return list(pairs[:k]) if split == "train" else list(pairs[k:])


def pair_files(data_root, split: str = "train", config=None):
    """The (noisy, clean) file pairs of a split as VoiceBankDataset._load_file_pairs
    lists them (data/dataset.py:96-147): the sorted *.wav of the noisy directory,
    each with the clean file of the same name (a noisy file without one is
    reported and skipped), then the 90/10 train/val cut."""
    from pathlib import Path

    if split in ("train", "val"):
        nd, cd = TRAIN_DIRS
    elif split == "test":
        nd, cd = TEST_DIRS
    else:
        raise ValueError(f"Invalid split: {split}. Must be 'train', 'val', or 'test'")
    noisy_dir, clean_dir = Path(data_root) / nd, Path(data_root) / cd
    for d, what in ((noisy_dir, "Noisy"), (clean_dir, "Clean")):
        if not d.exists():
            raise FileNotFoundError(f"{what} audio directory not found: {d}")
    pairs = []
    for p in sorted(noisy_dir.glob("*.wav")):
        c = clean_dir / p.name
        if c.exists():
            pairs.append((p, c))
        else:
            print(f"Warning: No clean file found for {p.name}")
    return split_pairs(pairs, split, (config or {}).get("train_val_split", 0.9))


class SpectrogramStore:
    """Every utterance's normalised noisy and clean magnitude, float32, packed
    in two device arrays: utterance i is ``[F, T_i]`` row-major at element
    ``offsets[i]`` of both (no row padding: csrc/batch_prep.hip loads unaligned).
    ``frames`` / ``offsets`` are kept on the host too, so a loader sizes a
    batch without asking the device."""

    def __init__(self, noisy: torch.Tensor, clean: torch.Tensor, frames: np.ndarray, F: int):
        self.frames = np.asarray(frames, dtype=np.int32)
        self.F = int(F)
        self.offsets, total = pack_offsets(self.frames, F)
        if noisy.numel() != total or clean.numel() != total or noisy.dtype != torch.float32:
            raise ValueError("hvit data: store size does not match frames")
        self.noisy, self.clean = noisy, clean
        self.device = noisy.device
        self.frames_dev = torch.from_numpy(self.frames).to(self.device)
        self.offsets_dev = torch.from_numpy(self.offsets).to(self.device)

    def __len__(self) -> int:
        return int(self.frames.shape[0])

    @property
    def nbytes(self) -> int:
        """Device bytes of the two magnitude arrays."""
        return 4 * (self.noisy.numel() + self.clean.numel())

    def get(self, i: int):
        """(noisy, clean) views ``[1, F, T_i]`` of utterance i."""
        o, n = int(self.offsets[i]), self.F * int(self.frames[i])
        shape = (1, self.F, int(self.frames[i]))
        return self.noisy[o:o + n].view(shape), self.clean[o:o + n].view(shape)

    @classmethod
    def from_waves(cls, noisy_list, clean_list, device, n_fft: int = N_FFT, hop: int = HOP, win: int = WIN,
                   chunk: int = 64, rates=None, sample_rate: int = SR) -> "SpectrogramStore":
        """Build the stores from host waveforms.  Each pair is cut to its common
        length (data/dataset.py:260-263); ``chunk`` pairs at a time go through
        frontend.stft_mag(normalize="minmax") as one ragged batch (the STFT of
        :183-190 and the per-utterance min-max of :213-219) and each clip's
        valid frames are copied to its slot.

        ``rates`` (optional, per pair a sample rate or a ``(noisy, clean)`` pair
        of them): a clip at another rate than ``sample_rate`` is uploaded raw
        and resampled on the device (resampler.resample_wave) before the cut
        to the common length, so a chunk is still uploaded once."""
        from .frontend import n_frames, stft_mag

        if len(noisy_list) != len(clean_list) or not len(noisy_list):
            raise ValueError("hvit data: need as many noisy as clean clips, at least one")
        device = torch.device(device)
        if rates is None:
            lens = [min(len(a), len(b)) for a, b in zip(noisy_list, clean_list)]
        else:
            sr = int(sample_rate)
            if len(rates) != len(noisy_list):
                raise ValueError("hvit data: rates must give one entry per pair")
            rates = [(int(r), int(r)) if np.isscalar(r) else (int(r[0]), int(r[1])) for r in rates]
            lens = [min(out_length(len(a), ra, sr), out_length(len(b), rb, sr))
                    for a, b, (ra, rb) in zip(noisy_list, clean_list, rates)]
        if min(lens) < 1:
            raise ValueError("hvit data: empty clip")
        frames = np.array([n_frames(n, hop) for n in lens], dtype=np.int32)
        F = n_fft // 2 + 1
        offsets, total = pack_offsets(frames, F)
        noisy = torch.empty(total, dtype=torch.float32, device=device)
        clean = torch.empty(total, dtype=torch.float32, device=device)
        for s in range(0, len(lens), max(1, int(chunk))):
            part = range(s, min(s + max(1, int(chunk)), len(lens)))
            Lmax = max(lens[i] for i in part)
            if rates is None:
                wave = upload_rows([noisy_list[i][:lens[i]] for i in part] + [clean_list[i][:lens[i]] for i in part],
                                   device, width=Lmax)
            else:
                wave = cls._resampled_rows([(noisy_list[i], rates[i][0]) for i in part]
                                           + [(clean_list[i], rates[i][1]) for i in part], sr, Lmax, device)
            ln = [lens[i] for i in part] * 2
            mag = stft_mag(wave, ln, n_fft, hop, win, normalize="minmax")
            for k, i in enumerate(part):
                o, T = int(offsets[i]), int(frames[i])
                noisy[o:o + F * T].view(F, T).copy_(mag[k, 0, :, :T])
                clean[o:o + F * T].view(F, T).copy_(mag[len(part) + k, 0, :, :T])
        return cls(noisy, clean, frames, F)

    @staticmethod
    def _resampled_rows(rows, sr: int, Lmax: int, device) -> torch.Tensor:
        """A chunk's device batch ``[len(rows), Lmax]`` from ``(host clip, rate)``
        rows: one raw upload per distinct rate, resampled to ``sr`` on the
        device and gathered into place.  A row may hold samples past the cut
        its pair is given (stft_mag takes the lengths and ignores them)."""
        wave = torch.zeros((len(rows), Lmax), dtype=torch.float32, device=device)
        by_rate = {}
        for k, (_, r) in enumerate(rows):
            by_rate.setdefault(r, []).append(k)
        for r, ks in sorted(by_rate.items()):
            dev_rows = WaveBatch.from_clips([rows[k][0] for k in ks], device, r, sr).wave
            W = min(Lmax, dev_rows.shape[1])  # at least every member's cut
            wave[torch.as_tensor(ks, device=device), :W] = dev_rows[:, :W]
        return wave

    @classmethod
    def from_directory(cls, data_root, split: str = "train", config=None, device="cuda",
                       chunk: int = 64) -> "SpectrogramStore":
        """The split's pairs (``pair_files``) read with audio.read_wav and
        built with ``from_waves``; ``config`` is the reference's data config
        (sample_rate, n_fft, hop_length, win_length, train_val_split) plus one
        key of this project's own, ``resample`` (not a reference key; default
        false): when true every file is read at its own rate
        (audio.read_audio) and resampled to ``sample_rate`` on the device,
        noisy and clean each, before the cut to the common length, as the
        reference's librosa.load(sr=sample_rate) does; without it a file at
        another rate raises.  Of the
        reference's waveform preprocessing (dataset.py:256-258) the default, peak
        normalisation, is a positive scale that the per-utterance min-max takes
        out again; pre-emphasis and silence trimming (off by default) are not
        implemented here and raise when the config turns them on."""
        config = config or {}
        pre = config.get("preprocessing", {}) or {}
        for key in ("apply_pre_emphasis", "trim_silence"):
            if pre.get(key, False) or config.get(key, False):
                raise NotImplementedError(f"hvit data: preprocessing option {key!r} is not implemented")
        if config.get("normalization_type", "per_utterance") != "per_utterance":
            raise NotImplementedError("hvit data: only normalization_type 'per_utterance' (min-max) is implemented")
        sr = config.get("sample_rate", SR)
        pairs = pair_files(data_root, split, config)
        if not pairs:
            raise FileNotFoundError(f"hvit data: no audio pairs for split {split!r} under {data_root}")
        rates = None
        if config.get("resample", False):
            noisy, clean = [read_audio(n) for n, _ in pairs], [read_audio(c) for _, c in pairs]
            rates = [(a[1], b[1]) for a, b in zip(noisy, clean)]
            noisy, clean = [a[0] for a in noisy], [b[0] for b in clean]
            if all(ra == sr and rb == sr for ra, rb in rates):
                rates = None
        else:
            noisy = [read_wav(n, sr) for n, _ in pairs]
            clean = [read_wav(c, sr) for _, c in pairs]
        print(f"Loaded {len(pairs)} audio pairs for {split} split")
        return cls.from_waves(noisy, clean, device, config.get("n_fft", N_FFT), config.get("hop_length", HOP),
                              config.get("win_length", WIN), chunk, rates=rates, sample_rate=sr)

    @classmethod
    def synthetic(cls, n: int, seconds_range=(2.0, 4.0), seed: int = 0, device="cuda") -> "SpectrogramStore":
        """``n`` harmonic_pair clips with lengths uniform in ``seconds_range``."""
        rng = np.random.Generator(np.random.PCG64(seed))
        lo, hi = seconds_range
        lens = [int(round(rng.uniform(lo, hi) * SR)) for _ in range(n)]
        pairs = [harmonic_pair(m, seed + 1 + i) for i, m in enumerate(lens)]
        return cls.from_waves([p[1] for p in pairs], [p[0] for p in pairs], device)


def _mix63(seed: int) -> int:
    return ((int(seed) * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & 0x7FFFFFFFFFFFFFFF)


class DeviceBatchLoader:
    """Iterates ``{'noisy_spec', 'clean_spec'}`` batches [B, 1, F, Tb] from a
    SpectrogramStore, as the reference's DataLoader over VoiceBankDataset does
    (data/dataset.py:289-294, :341-347; the phases are not kept: training never
    reads them), one hvit_batch_prep launch per batch.

    * Each epoch's order is one permutation from the loader's own
      ``torch.Generator`` (identity without ``shuffle``), uploaded once; a batch
      passes a view of it as the launch's ``idx``.  ``set_epoch(e)`` re-seeds
      the generator with ``seed + e`` (every rank then draws the same order).
    * ``Tb = ceil(max T_i / bucket_frames) * bucket_frames`` from the host copy
      of ``frames``: few distinct shapes for GraphedTrainStep's per-shape graphs.
    * The augmentation draws come from a device seed stream of the loader's own:
      ``hvit_rng_advance`` steps ``{base, counter}`` before every launch, the
      pattern of HybridViT._seed.  ``last_plan`` / ``last_seed`` are the latest
      batch's plan tensor and seed word.
    * ``rank`` / ``world``: rank r takes every world-th sample of the epoch's
      order (cut to a multiple of ``world``).  Nothing else of data parallelism
      is wired here.
    * ``state_dict()`` holds the generator state at the start of the current
      epoch, the epoch, the position (batches already yielded) and the device
      RNG state; it reads that state back, so it synchronises."""

    def __init__(self, store: SpectrogramStore, batch_size: int, shuffle: bool = True, drop_last: bool = False,
                 augmenter=None, bucket_frames: int = 32, seed: int = 0, rank: int = 0, world: int = 1):
        if batch_size < 1 or bucket_frames < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError("hvit DeviceBatchLoader: batch_size, bucket_frames >= 1 and 0 <= rank < world")
        self.store, self.batch_size, self.shuffle, self.drop_last = store, int(batch_size), shuffle, drop_last
        self.augmenter, self.bucket_frames = augmenter, int(bucket_frames)
        self.augment = True  # False: the launch's enable flag off (plain gather and pad, an all-zero plan)
        self.seed, self.rank, self.world = int(seed), int(rank), int(world)
        self.dataset = store  # len(loader.dataset), as the reference's trainer prints it
        self.gen = torch.Generator()
        self.gen.manual_seed(self.seed)
        self.epoch = 0
        self.pos = 0
        self._epoch_gen_state = self.gen.get_state()
        self._rng_state = torch.tensor([_mix63(self.seed), 0], dtype=torch.int64).to(store.device)
        self.last_plan = None
        self.last_seed = None
        self.last_idx = None  # host copy of the latest batch's indices
        if augmenter is not None:
            from .augment import _check
            _check(augmenter)

    def _count(self) -> int:
        return len(self.store) // self.world if self.world > 1 else len(self.store)

    def __len__(self) -> int:
        n = self._count()
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def set_epoch(self, epoch: int) -> None:
        self.epoch, self.pos = int(epoch), 0
        self.gen.manual_seed(self.seed + self.epoch)
        self._epoch_gen_state = self.gen.get_state()

    def set_rng_state(self, base: int, counter: int = 0) -> None:
        """Reset the device seed stream of the augmentation draws."""
        # in place: a captured launch keeps reading (and advancing) this buffer
        self._rng_state.copy_(torch.tensor([int(base) & 0x7FFFFFFFFFFFFFFF, int(counter)], dtype=torch.int64))

    def rng_state(self) -> torch.Tensor:
        return self._rng_state.clone()

    def state_dict(self):
        return {"generator_state": self._epoch_gen_state.clone(), "epoch": self.epoch, "position": self.pos,
                "rng_state": self._rng_state.cpu().clone()}

    def load_state_dict(self, sd) -> None:
        self._epoch_gen_state = sd["generator_state"].cpu().to(torch.uint8).clone()
        self.gen.set_state(self._epoch_gen_state)
        self.epoch, self.pos = int(sd["epoch"]), int(sd["position"])
        self._rng_state.copy_(sd["rng_state"].to(dtype=torch.int64))

    def _order(self) -> np.ndarray:
        n = len(self.store)
        self.gen.set_state(self._epoch_gen_state)
        order = torch.randperm(n, generator=self.gen).numpy() if self.shuffle else np.arange(n)
        if self.world > 1:
            order = order[:n - n % self.world][self.rank::self.world]
        return order.astype(np.int32)

    def prepare(self, idx_dev: torch.Tensor, idx_host: np.ndarray, Tb: int = None, out=None):
        """One launch: the batch of the store's utterances ``idx_host`` (device
        copy ``idx_dev``, int32) padded to ``Tb`` frames (default: the bucketed
        maximum).  Returns (noisy, clean, plan), written to ``out`` when given
        (float32 [B, 1, F, Tb] twice and int32 [B, plan width]); advances the
        seed stream."""
        from . import _lib as L

        st = self.store
        idx_host = np.asarray(idx_host)
        B = int(idx_host.shape[0])
        if (B < 1 or idx_dev.dtype != torch.int32 or idx_dev.numel() != B or idx_dev.device != st.device
                or not idx_dev.is_contiguous() or idx_host.min() < 0 or idx_host.max() >= len(st)):
            raise ValueError("hvit DeviceBatchLoader: idx must be B >= 1 int32 store indices, on the store's device")
        maxT = int(st.frames[idx_host].max())
        if Tb is None:
            Tb = -(-maxT // self.bucket_frames) * self.bucket_frames
        aug = self.augmenter
        cfg = aug.c_struct(self.augment) if aug is not None else L.AugmentCfg(0, 0, 0, 0, 0, 0.0, 0.0, 0.0)
        width = aug.plan_width if aug is not None else 2
        dev = st.device
        with torch.cuda.device(dev):
            if out is not None:
                noisy, clean, plan = out
                for t, shape, dt in ((noisy, (B, 1, st.F, Tb), torch.float32), (clean, (B, 1, st.F, Tb), torch.float32),
                                     (plan, (B, width), torch.int32)):
                    if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != dev:
                        raise ValueError(f"hvit DeviceBatchLoader: output must be contiguous {dt} {shape} on {dev}")
            else:
                noisy = torch.empty((B, 1, st.F, Tb), dtype=torch.float32, device=dev)
                clean = torch.empty((B, 1, st.F, Tb), dtype=torch.float32, device=dev)
                plan = torch.empty((B, width), dtype=torch.int32, device=dev)
            seed_t = torch.empty(1, dtype=torch.int64, device=dev)
            stream = L.stream_ptr(dev)
            L.call("hvit_rng_advance", self._rng_state.data_ptr(), seed_t.data_ptr(), stream)
            L.call("hvit_batch_prep", st.noisy.data_ptr(), st.clean.data_ptr(), st.offsets_dev.data_ptr(),
                   st.frames_dev.data_ptr(), len(st), idx_dev.data_ptr(), B, st.F, int(Tb), maxT, cfg,
                   seed_t.data_ptr(), noisy.data_ptr(), clean.data_ptr(), plan.data_ptr(), stream)
        self.last_plan, self.last_seed, self.last_idx = plan, seed_t, idx_host
        return noisy, clean, plan

    def __iter__(self):
        order = self._order()
        order_dev = torch.from_numpy(order).to(self.store.device)
        nb, bs = len(self), self.batch_size
        while self.pos < nb:
            s = self.pos * bs
            host = order[s:s + bs]
            noisy, clean, _ = self.prepare(order_dev[s:s + len(host)], host)
            self.pos += 1
            yield {"noisy_spec": noisy, "clean_spec": clean}
        # the next epoch: a new permutation from the generator as it stands
        self.epoch += 1
        self.pos = 0
        self._epoch_gen_state = self.gen.get_state()


__all__ = ["harmonic_pair", "magnitude", "minmax", "spectrogram_batch", "pack_offsets", "split_pairs", "pair_files",
           "SpectrogramStore", "DeviceBatchLoader"]
