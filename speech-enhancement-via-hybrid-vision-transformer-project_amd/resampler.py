"""Sample-rate conversion on the device (csrc/wave_resample.hip behind
hvit_wave_resample): the resampling half of the reference's
``librosa.load(path, sr=16000)`` (data/dataset.py:160, inference/enhancer.py:152,
evaluation/evaluator.py:135), so a corpus that ships at 48 kHz loads as
downloaded and a clip stays on the GPU from raw samples to spectrogram.

The filter is a Kaiser-windowed sinc applied as a rational-ratio polyphase FIR,
with the semantics of ``scipy.signal.resample_poly(x, up, down, window=taps,
padtype="constant")``.  The default design is the "kaiser_best"
class librosa used before 0.10 (64 zero crossings, roll-off 0.9476, beta
14.77).  librosa 0.10 resamples with ``soxr_hq``; that library is absent here,
so parity with librosa's own output is unpinned, as enhancer.py says of its
framing.  ``resample_reference`` is the formula in numpy float64 on the host:
the yardstick the kernel is tested against.  There is no CPU path for
``resample_wave``: a CPU tensor is an error.
"""

from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from ._args import canonical_device, lengths_arg, wave_arg

TILE = 256  # outputs per workgroup (csrc/wave_resample.hip: WR_TILE)
ZEROS, ROLLOFF, BETA = 64, 0.9475937167399596, 14.769656459379492
_tables = {}


def ratio(orig_sr: int, target_sr: int):
    """``(up, down)``: target / orig reduced by their gcd."""
    orig_sr, target_sr = int(orig_sr), int(target_sr)
    if orig_sr < 1 or target_sr < 1:
        raise ValueError(f"hvit resampler: sample rates {orig_sr} -> {target_sr}")
    g = math.gcd(orig_sr, target_sr)
    return target_sr // g, orig_sr // g


def out_length(length: int, up: int, down: int) -> int:
    """``ceil(length * up / down)``: the outputs of ``length`` input samples."""
    return -(-int(length) * int(up) // int(down))


def resample_taps(orig_sr: int, target_sr: int, zeros: int = ZEROS, rolloff: float = ROLLOFF, beta: float = BETA):
    """``(h float64 [2 * half + 1], up, down, half)``: a Kaiser-windowed sinc
    with ``q = max(up, down)``, ``half = zeros * q``, ``fc = rolloff / q`` and
    ``h[n] = up * fc * sinc(fc * n) * kaiser(2 * half + 1, beta)[n + half]`` for
    ``-half <= n <= half``.  The defaults are the "kaiser_best" class of librosa
    before 0.10; parity with librosa 0.10's ``soxr_hq`` is unpinned (the
    library is absent here)."""
    up, down = ratio(orig_sr, target_sr)
    if zeros < 1:
        raise ValueError(f"hvit resampler: zeros={zeros}")
    q = max(up, down)
    half = int(zeros) * q
    fc = float(rolloff) / q
    n = np.arange(-half, half + 1, dtype=np.float64)
    h = up * fc * np.sinc(fc * n) * np.kaiser(2 * half + 1, float(beta))
    return h, up, down, half


def taps_phase_major(h, up: int) -> np.ndarray:
    """``taps_pp [up, J]``, ``J = ceil(len(h) / up)``: ``taps_pp[p, j] =
    h[p + j * up]``, zero past the end (the layout hvit_wave_resample reads)."""
    h = np.asarray(h)
    J = -(-h.shape[0] // int(up))
    pp = np.zeros(J * int(up), dtype=h.dtype)
    pp[:h.shape[0]] = h
    return np.ascontiguousarray(pp.reshape(J, int(up)).T)


def taps_from_phase_major(taps_pp, n_taps: int) -> np.ndarray:
    """The inverse of ``taps_phase_major``: the first ``n_taps`` taps."""
    return np.ascontiguousarray(np.asarray(taps_pp).T.reshape(-1)[:int(n_taps)])


def resample_reference(x, orig_sr: int, target_sr: int, taps=None, out_range=None, stats: bool = False):
    """The resampling formula in float64 on the host: for ``0 <= m <
    ceil(len * up / down)``, ``out[m] = sum_k h[half + m * down - k * up] *
    x[k]`` over ``0 <= k < len`` with the tap index in ``[0, 2 * half]``.

    ``taps`` (default: ``resample_taps(orig_sr, target_sr)[0]``) has odd length
    ``2 * half + 1``.  ``out_range=(m0, m1)`` evaluates only those outputs; every
    output accumulates its own terms one by one in ascending tap-row order, so
    a range equals the slice of the full result bit for bit.  With ``stats``
    the result is ``(out, sum_abs, terms)``: each output's ``sum |h x|`` and its
    term count (what an f32 error bound for the kernel is made of)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    up, down = ratio(orig_sr, target_sr)
    h = resample_taps(orig_sr, target_sr)[0] if taps is None else np.asarray(taps, dtype=np.float64).reshape(-1)
    if h.shape[0] % 2 != 1 or h.shape[0] < 3:
        raise ValueError(f"hvit resampler: taps must have odd length 2 * half + 1 >= 3, got {h.shape[0]}")
    half = (h.shape[0] - 1) // 2
    n = x.shape[0]
    Lo = out_length(n, up, down)
    m0, m1 = (0, Lo) if out_range is None else (int(out_range[0]), int(out_range[1]))
    if not 0 <= m0 <= m1 <= Lo:
        raise ValueError(f"hvit resampler: out_range {out_range} outside [0, {Lo}]")
    J = (2 * half) // up + 1
    out = np.zeros(m1 - m0, dtype=np.float64)
    sabs = np.zeros(m1 - m0, dtype=np.float64) if stats else None
    cnt = np.zeros(m1 - m0, dtype=np.int64) if stats else None
    step = 1 << 15
    for s in range(m0, m1, step):
        m = np.arange(s, min(s + step, m1), dtype=np.int64)
        pos = half + m * down
        q = pos // up
        p = pos - q * up
        acc = np.zeros(m.shape[0], dtype=np.float64)
        a = np.zeros(m.shape[0], dtype=np.float64) if stats else None
        c = np.zeros(m.shape[0], dtype=np.int64) if stats else None
        for j in range(J):
            t = p + j * up
            k = q - j
            ok = (t <= 2 * half) & (k >= 0) & (k < n)
            if not ok.any():
                continue
            term = np.where(ok, h[np.minimum(t, 2 * half)] * x[np.clip(k, 0, n - 1)], 0.0)
            acc = acc + term
            if stats:
                a = a + np.abs(term)
                c = c + ok
        out[s - m0:s - m0 + m.shape[0]] = acc
        if stats:
            sabs[s - m0:s - m0 + m.shape[0]] = a
            cnt[s - m0:s - m0 + m.shape[0]] = c
    return (out, sabs, cnt) if stats else out


def taps_table(orig_sr: int, target_sr: int, device, zeros: int = ZEROS, rolloff: float = ROLLOFF,
               beta: float = BETA):
    """``(taps_pp f32 device [up, J], up, down, half)``: the design rounded
    once from float64, in phase-major layout; cached per device, ratio and
    design."""
    device = canonical_device(device)
    up, down = ratio(orig_sr, target_sr)
    key = (str(device), up, down, int(zeros), float(rolloff), float(beta))
    hit = _tables.get(key)
    if hit is None:
        h, up, down, half = resample_taps(orig_sr, target_sr, zeros, rolloff, beta)
        pp = torch.from_numpy(taps_phase_major(h.astype(np.float32), up)).to(device)
        hit = _tables[key] = (pp, up, down, half)
    return hit


def custom_taps_table(name: str, design, device):
    """``taps_table`` for a caller's filter: ``design()`` returns ``(h float64
    [2 * half + 1] already times up, up, down, half)``; it is rounded once to
    float32, laid out phase-major and cached per device and ``name`` (which
    must identify the design: ``design`` runs only on a miss)."""
    device = canonical_device(device)
    key = (str(device), "custom", name)
    hit = _tables.get(key)
    if hit is None:
        h, up, down, half = design()
        h = np.asarray(h, dtype=np.float64).reshape(-1)
        if h.shape[0] != 2 * half + 1 or math.gcd(up, down) != 1:
            raise ValueError(f"hvit resampler: table {name!r} needs 2 * half + 1 taps and coprime up / down")
        pp = torch.from_numpy(taps_phase_major(h.astype(np.float32), up)).to(device)
        hit = _tables[key] = (pp, int(up), int(down), int(half))
    return hit


def resample_wave(wave: torch.Tensor, lengths, orig_sr: int, target_sr: int, return_peak: bool = False,
                  out_len: Optional[int] = None, taps=None, acc64: bool = False):
    """Resample a float32 GPU batch ``wave`` [B, L] (row b is ``wave[b,
    :lengths[b]]``; what the buffer holds past it is ignored) from ``orig_sr``
    to ``target_sr``: ``(out [B, L_out], out_lengths int32 [B])``, plus ``peak
    [B] = max |out[b]|`` with ``return_peak``.  Row b of ``out`` is its
    ``ceil(len_b * up / down)`` outputs followed by zeros.

    ``lengths``: None (every row is L long), a host sequence (``out_lengths``
    and ``L_out`` then come from the integer formula on the host: nothing is
    read back) or an int32 device tensor (``L_out`` is then sized for L).
    ``out_len`` fixes ``L_out``; outputs past it are dropped.  Equal rates return
    ``wave`` itself without a launch.  ``taps`` replaces the default design by a
    table of ``taps_table``'s form for the same ratio (``custom_taps_table``);
    ``acc64`` sums every output in float64 before its one rounding to float32
    (hvit_wave_resample_f64acc) instead of in float32."""
    given = wave
    wave, B, Ln, row_stride = wave_arg(wave, "hvit resampler", "wave")
    dev = wave.device
    up, down = ratio(orig_sr, target_sr)
    host_lens = None
    if lengths is not None and not isinstance(lengths, torch.Tensor):
        host_lens = np.asarray(lengths, dtype=np.int64).reshape(-1)
        if host_lens.shape != (B,) or (host_lens < 0).any() or (host_lens > Ln).any():
            raise ValueError(f"hvit resampler: lengths must be {B} values in [0, {Ln}]")
    lens = lengths_arg(lengths if host_lens is None else host_lens, B, dev, "hvit resampler")

    if up == down:
        ol = lens if lens is not None else torch.full((B,), Ln, dtype=torch.int32, device=dev)
        return (given, ol, given.abs().amax(1)) if return_peak else (given, ol)

    if host_lens is not None:
        olens = -(-host_lens * up // down)
        L_out = int(out_len) if out_len is not None else max(1, int(olens.max()))
        out_lengths = torch.from_numpy(np.minimum(olens, L_out).astype(np.int32)).to(dev)
    else:
        L_out = int(out_len) if out_len is not None else out_length(Ln, up, down)
        if lens is None:
            out_lengths = torch.full((B,), min(out_length(Ln, up, down), L_out), dtype=torch.int32, device=dev)
        else:
            ol = (lens.clamp(0, Ln).to(torch.int64) * up + (down - 1)) // down
            out_lengths = ol.clamp(max=L_out).to(torch.int32)
    if L_out < 1:
        raise ValueError(f"hvit resampler: output length {L_out}")
    if taps is None:
        taps = taps_table(orig_sr, target_sr, dev)
    elif (taps[1], taps[2]) != (up, down) or taps[0].device != dev:
        raise ValueError(f"hvit resampler: taps table for {taps[1]}/{taps[2]} on {taps[0].device}, "
                         f"call is {up}/{down} on {dev}")
    taps_pp, up, down, half = taps
    out = torch.empty((B, L_out), dtype=torch.float32, device=dev)
    peak = torch.empty(B, dtype=torch.float32, device=dev) if return_peak else None
    with torch.cuda.device(dev):
        L.call("hvit_wave_resample_f64acc" if acc64 else "hvit_wave_resample", wave.data_ptr(), row_stride, L.ptr(lens), B, Ln, up, down, taps_pp.data_ptr(),
               half, out.data_ptr(), L_out, L_out, L.ptr(peak), L.stream_ptr(dev))
    return (out, out_lengths, peak) if return_peak else (out, out_lengths)


__all__ = ["TILE", "ratio", "out_length", "resample_taps", "taps_phase_major", "taps_from_phase_major",
           "resample_reference", "taps_table", "custom_taps_table", "resample_wave"]
