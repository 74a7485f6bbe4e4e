"""SpecAugment and random gain for training batches, drawn on the device.

The reference augments the noisy spectrogram in its DataLoader workers
(data/augmentation.py:48-118, called from data/dataset.py:284-287).  Here the
draws and the masking happen inside the batch-preparation launch
(csrc/batch_prep.hip, hvit_batch_prep); this module holds

* ``SpectrogramAugmenter`` -- the reference's config keys and defaults
  (augmentation.py:22-46) as parameters for that launch, nothing else;
* ``plan_host`` -- the numpy restatement of the kernel's draws: what the
  launch records in its plan tensor, recomputed from the batch's seed word;
* ``apply_plan_host`` -- one plan row applied to one spectrogram with the
  reference's slice assignments (augmentation.py:92, :98, :118).

Draw contract (include/hvit.h, hvit_batch_prep): sample b's j-th draw is
``u32 = hash32(rng_key(seed_word, 0xBA7C) ^ (64 b + j))``; ``randint(0, n)`` is
``(u32 * n) >> 32``; the gain is drawn iff ``u32 < floor(p * 2^32)``; its dB is
``lo + (hi - lo) * ((u32 >> 8) * 2^-24)`` in float32.
"""

from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib as L

SITE = 0xBA7C
DRAWS = 64


class SpectrogramAugmenter:
    """augmentation.py:22-46: the ``augmentation`` section of the data config.
    A disabled part is passed to the kernel as a count (or probability) of 0."""

    def __init__(self, config: Optional[Dict] = None):
        self.config = config or {}
        aug = self.config.get("augmentation", {}) or {}
        sa = aug.get("spec_augment", {}) or {}
        self.spec_augment_enabled = sa.get("enabled", True)
        self.freq_mask_num = sa.get("freq_mask_num", 2)
        self.freq_mask_width = sa.get("freq_mask_width", 15)
        self.time_mask_num = sa.get("time_mask_num", 2)
        self.time_mask_width = sa.get("time_mask_width", 30)
        rg = aug.get("random_gain", {}) or {}
        self.random_gain_enabled = rg.get("enabled", True)
        self.gain_db_range = rg.get("gain_db_range", [-3, 3])
        self.gain_probability = rg.get("probability", 0.5)

    # what the launch sees
    @property
    def nf(self) -> int:
        return int(self.freq_mask_num) if self.spec_augment_enabled else 0

    @property
    def nt(self) -> int:
        return int(self.time_mask_num) if self.spec_augment_enabled else 0

    @property
    def gain_prob(self) -> float:
        return float(self.gain_probability) if self.random_gain_enabled else 0.0

    @property
    def plan_width(self) -> int:
        return 2 * self.nf + 2 * self.nt + 2

    def c_struct(self, enabled: bool = True) -> "L.AugmentCfg":
        return L.AugmentCfg(1 if enabled else 0, self.nf, int(self.freq_mask_width), self.nt,
                            int(self.time_mask_width), self.gain_prob, float(self.gain_db_range[0]),
                            float(self.gain_db_range[1]))


# ---- numpy mirror of csrc/common.h (mix64, rng_key, hash32) ------------------
_M64 = (1 << 64) - 1


def _mix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def rng_key(seed: int, site: int) -> int:
    m = _mix64((int(seed) & _M64) ^ ((site << 48) & _M64))
    return (m ^ (m >> 32)) & 0xFFFFFFFF


def hash32(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    return x ^ (x >> np.uint64(16))


def draws_host(seed_word: int, B: int) -> np.ndarray:
    """u32(b, j) for b < B, j < 64 as uint64 [B, 64]."""
    key = np.uint64(rng_key(seed_word, SITE))
    b = np.arange(B, dtype=np.uint64)[:, None]
    j = np.arange(DRAWS, dtype=np.uint64)[None, :]
    return hash32(key ^ ((b * np.uint64(DRAWS) + j) & np.uint64(0xFFFFFFFF)))


def _check(cfg: SpectrogramAugmenter):
    if not (0 <= cfg.nf <= L.AUG_MAX_MASKS and 0 <= cfg.nt <= L.AUG_MAX_MASKS):
        raise ValueError(f"hvit augment: mask counts must be 0..{L.AUG_MAX_MASKS}")
    if (cfg.nf > 0 and cfg.freq_mask_width < 1) or (cfg.nt > 0 and cfg.time_mask_width < 1):
        raise ValueError("hvit augment: a mask width below 1 with a count above 0 (numpy's randint(0, 0) raises)")


def gain_db_host(seed_word: int, B: int, cfg: SpectrogramAugmenter) -> np.ndarray:
    """The float32 dB value of each sample's gain draw (whether or not the
    Bernoulli draw then applies it), rounded as the kernel rounds it."""
    u = draws_host(seed_word, B)[:, 2 * cfg.nf + 2 * cfg.nt + 1]
    r = (u >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    lo, hi = np.float32(cfg.gain_db_range[0]), np.float32(cfg.gain_db_range[1])
    return (lo + ((hi - lo) * r).astype(np.float32)).astype(np.float32)


def plan_host(seed_word: int, frames: Sequence[int], F: int, cfg: SpectrogramAugmenter) -> np.ndarray:
    """The plan [B, 2 nf + 2 nt + 2] (int32) that hvit_batch_prep records for a
    batch whose samples have ``frames[b]`` frames and whose seed word is
    ``seed_word``: (f0, f) per frequency mask, (t0, t) per time mask
    (augmentation.py:89-98), the gain-drawn flag (:63) and the float32 bits of
    10^(dB / 20) (:115-116; computed in float64 here and rounded once)."""
    _check(cfg)
    frames = np.asarray(frames, dtype=np.int64)
    B = frames.shape[0]
    nf, nt = cfg.nf, cfg.nt
    u = draws_host(seed_word, B)

    def randint(col, n):  # (u32 * n) >> 32 with n [B] >= 1
        return ((u[:, col] * np.asarray(n, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)

    plan = np.zeros((B, 2 * nf + 2 * nt + 2), dtype=np.int32)
    j = 0
    for m in range(nf):
        f = randint(j, np.full(B, int(cfg.freq_mask_width)))
        f0 = randint(j + 1, np.maximum(1, F - f))
        plan[:, 2 * m], plan[:, 2 * m + 1] = f0, f
        j += 2
    for m in range(nt):
        t = randint(j, np.minimum(int(cfg.time_mask_width), frames))
        t0 = randint(j + 1, np.maximum(1, frames - t))
        plan[:, 2 * nf + 2 * m], plan[:, 2 * nf + 2 * m + 1] = t0, t
        j += 2
    p = float(np.float32(cfg.gain_prob))
    thr = (1 << 32) if p >= 1.0 else (0 if p <= 0.0 else int(p * 4294967296.0))
    drawn = u[:, j] < np.uint64(thr)
    db = gain_db_host(seed_word, B, cfg).astype(np.float64)
    gain = np.where(drawn, 10.0 ** (db / 20.0), 1.0).astype(np.float32)
    plan[:, -2] = drawn
    plan[:, -1] = gain.view(np.int32)
    return plan


def disabled_plan(B: int, cfg: Optional[SpectrogramAugmenter]) -> np.ndarray:
    """The plan of a launch with augmentation disabled: zeros, gain 1.0."""
    w = cfg.plan_width if cfg is not None else 2
    plan = np.zeros((B, w), dtype=np.int32)
    plan[:, -1] = np.float32(1.0).view(np.int32)
    return plan


def apply_plan_host(spec: np.ndarray, plan_row: np.ndarray, nf: Optional[int] = None) -> np.ndarray:
    """``spec`` [F, T] (or [1, F, T]) with the masks of ``plan_row`` set to 0 by
    slice assignment (augmentation.py:92, :98: a slice past the edge stops
    there).  The first ``nf`` pairs of the row are frequency masks (default:
    half of them, as with equal counts like the reference's 2 + 2).  The gain
    (the row's last two words) is NOT applied: multiply by
    ``plan_gain(plan_row)`` in float32 for the launch's noisy output."""
    out = np.array(spec, dtype=np.float32, copy=True)
    pairs = np.asarray(plan_row, dtype=np.int64)[:-2].reshape(-1, 2)
    nf = len(pairs) // 2 if nf is None else int(nf)
    for k, (a0, w) in enumerate(pairs):
        if k < nf:
            out[..., a0:a0 + w, :] = 0
        else:
            out[..., :, a0:a0 + w] = 0
    return out


def plan_gain(plan_row: np.ndarray) -> np.float32:
    """The float32 gain recorded in a plan row."""
    return np.asarray(plan_row, dtype=np.int32)[-1:].view(np.float32)[0]


__all__ = ["SpectrogramAugmenter", "plan_host", "apply_plan_host", "plan_gain", "gain_db_host",
           "disabled_plan", "draws_host"]
