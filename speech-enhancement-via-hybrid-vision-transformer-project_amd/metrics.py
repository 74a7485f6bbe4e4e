"""Speech quality metrics (the reference's evaluation/metrics.py): the host
functions with its names and signatures, in numpy float64, and the same
figures on GPU batches through csrc/metrics.hip (hvit_wave_metrics, hvit_lsd).

Host: ``compute_sisdr``, ``compute_snr``, ``compute_segsnr`` follow
metrics.py:100-243 term by term on float64 copies of the samples, so an exactly
silent signal gives ``-inf`` as numpy's log10(0) does.  ``compute_lsd``
(:246-296) frames with the enhancer's host STFT (``torch.stft``, periodic Hann,
center=True, zero padding: librosa is not installed here, where the reference
itself returns 0.0).  ``compute_pesq`` / ``compute_stoi`` (:16-97) call the
``pesq`` / ``pystoi`` packages when they can be imported and otherwise return
0.0 after one warning per process; there is no kernel for PESQ.  STOI also has
a native form: ``stoi_reference`` is its definition in numpy
float64 and ``stoi`` the same on GPU batches (csrc/stoi.hip behind hvit_stoi);
``stoi="native"`` on ``compute_all_metrics`` / ``all_metrics_batch`` selects it.

Device: ``wave_metrics`` gives {SI-SDR, SNR, SegSNR} per row of a ragged f32
batch as float64 ``[B, 3]``; ``lsd`` is two ``stft_mag`` calls and hvit_lsd;
``all_metrics_batch`` returns the reference's keys as float64 ``[B]`` device
tensors.  The calls do not synchronise and can be captured in a hipGraph; a
row's result is bit-identical whichever batch it rides in.  There is no CPU
path behind them: a CPU tensor is an error.
"""

from __future__ import annotations

import importlib
import math
import warnings
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L
from . import frontend as FE
from . import resampler as RS
from ._args import lengths_arg, wave_arg

_warned = set()


def _pair(clean, other):
    """Float64 copies cut to the shorter of the two (metrics.py:121-123)."""
    clean = np.asarray(clean, dtype=np.float64).reshape(-1)
    other = np.asarray(other, dtype=np.float64).reshape(-1)
    n = min(len(clean), len(other))
    return clean[:n], other[:n]


def _optional(package: str, attr: str):
    """``package.attr`` or None, with one warning per process when the package is absent."""
    try:
        return getattr(importlib.import_module(package), attr)
    except ImportError:
        if package not in _warned:
            _warned.add(package)
            warnings.warn(f"hvit metrics: the {package} package is not installed; its score is reported as 0.0")
        return None


def compute_pesq(clean: np.ndarray, enhanced: np.ndarray, sr: int = 16000, mode: str = "wb") -> float:
    """ITU-T P.862 through the ``pesq`` package (metrics.py:16-55); 0.0 without it."""
    fn = _optional("pesq", "pesq")
    if fn is None:
        return 0.0
    c, e = _pair(clean, enhanced)
    try:
        return float(fn(sr, c, e, mode))
    except Exception as err:  # the package refuses some clips (no utterance found): the reference reports 0.0
        warnings.warn(f"hvit metrics: PESQ failed ({err}); reported as 0.0")
        return 0.0


def compute_stoi(clean: np.ndarray, enhanced: np.ndarray, sr: int = 16000, extended: bool = False) -> float:
    """Short-time objective intelligibility through ``pystoi`` (metrics.py:58-97); 0.0 without it."""
    fn = _optional("pystoi", "stoi")
    if fn is None:
        return 0.0
    c, e = _pair(clean, enhanced)
    try:
        return float(fn(c, e, sr, extended=extended))
    except Exception as err:  # as compute_pesq
        warnings.warn(f"hvit metrics: STOI failed ({err}); reported as 0.0")
        return 0.0


def _db(ratio) -> float:
    with np.errstate(divide="ignore"):
        return float(10.0 * np.log10(ratio))


def compute_sisdr(clean: np.ndarray, enhanced: np.ndarray, eps: float = 1e-8) -> float:
    """Scale-invariant SDR in dB (metrics.py:100-145): both signals lose their
    mean, the target is the projection of the estimate on the clean signal, and
    ``eps`` joins the two unnormalised sums."""
    c, e = _pair(clean, enhanced)
    c = c - np.mean(c)
    e = e - np.mean(e)
    target = (np.dot(e, c) / (np.dot(c, c) + eps)) * c
    return _db(np.sum(target ** 2) / (np.sum((e - target) ** 2) + eps))


def compute_snr(clean: np.ndarray, noisy_or_enhanced: np.ndarray, eps: float = 1e-8) -> float:
    """SNR in dB from the mean powers over the clip (metrics.py:148-184); ``eps`` joins the noise power."""
    c, e = _pair(clean, noisy_or_enhanced)
    return _db(np.mean(c ** 2) / (np.mean((e - c) ** 2) + eps))


def compute_segsnr(clean: np.ndarray, enhanced: np.ndarray, frame_length: int = 512, hop_length: int = 256,
                   eps: float = 1e-8) -> float:
    """Segmental SNR in dB (metrics.py:187-243): frames start at 0, hop, ...
    while start < len - frame_length; a frame counts when its signal and noise
    powers both exceed ``eps``, clipped to [-10, 35]; 0.0 when none counts."""
    c, e = _pair(clean, enhanced)
    values = []
    for start in range(0, len(c) - frame_length, hop_length):
        cf = c[start:start + frame_length]
        p_sig = np.mean(cf ** 2)
        p_noise = np.mean((e[start:start + frame_length] - cf) ** 2)
        if p_sig > eps and p_noise > eps:
            values.append(min(max(10.0 * np.log10(p_sig / p_noise), -10.0), 35.0))
    return float(np.mean(values)) if values else 0.0


def _host_mag(x: np.ndarray, n_fft: int, hop_length: int) -> np.ndarray:
    w = torch.hann_window(n_fft, dtype=torch.float64)
    spec = torch.stft(torch.as_tensor(x), n_fft, hop_length, n_fft, window=w, center=True, pad_mode="constant",
                      return_complex=True)
    return spec.abs().numpy()


def compute_lsd(clean: np.ndarray, enhanced: np.ndarray, sr: int = 16000, n_fft: int = 512, hop_length: int = 128,
                eps: float = 1e-10) -> float:
    """Log-spectral distance (metrics.py:246-296): the mean over frames of the
    RMS over bins of log(|C| + eps) - log(|E| + eps)."""
    c, e = _pair(clean, enhanced)
    d = np.log(_host_mag(c, n_fft, hop_length) + eps) - np.log(_host_mag(e, n_fft, hop_length) + eps)
    return float(np.mean(np.sqrt(np.mean(d ** 2, axis=0))))


# ------------------------------------------------------------- native STOI --
# Taal et al. 2011, non-extended, with the constants pystoi uses.
STOI_FS, STOI_FRAME, STOI_HOP, STOI_NFFT, STOI_BANDS, STOI_MINF = 10000, 256, 128, 512, 15, 150.0
STOI_SEG, STOI_BETA, STOI_DYN = 30, -15.0, 40.0
STOI_SHORT = 1e-5  # the score of a clip with fewer than STOI_SEG frames left
EPS = float(np.finfo(float).eps)


def stoi_taps(sr: int):
    """``(h float64 [2 * half + 1], up, down, half)``: the Kaiser-windowed sinc
    STOI resamples ``sr`` -> 10 kHz with (60 dB stop band, transition a tenth of
    the cut-off), before normalisation: ``resample_poly(x, up, down,
    window=h / sum(h))`` is the resampled clip."""
    g = math.gcd(STOI_FS, int(sr))
    up, down = STOI_FS // g, int(sr) // g
    fc = 1.0 / (2 * max(up, down))
    half = int(math.ceil((60.0 - 8.0) / (28.714 * (fc / 10.0))))
    t = np.arange(-half, half + 1, dtype=np.float64)
    h = np.kaiser(2 * half + 1, 0.1102 * (60.0 - 8.7)) * (2 * up * fc) * np.sinc(2 * fc * t)
    return h, up, down, half


def third_octave_bands():
    """The 15 half-open rfft bin ranges ``[(lo, hi), ...]`` at 10 kHz / 512: the
    edges 150 * 2^((2 b -+ 1) / 6) Hz, each snapped to the nearest bin."""
    f = np.linspace(0, STOI_FS, STOI_NFFT + 1)[:STOI_NFFT // 2 + 1]
    k = np.arange(STOI_BANDS, dtype=np.float64)
    lo = STOI_MINF * 2.0 ** ((2 * k - 1) / 6)
    hi = STOI_MINF * 2.0 ** ((2 * k + 1) / 6)
    return [(int(np.argmin((f - a) ** 2)), int(np.argmin((f - b) ** 2))) for a, b in zip(lo, hi)]


def stoi_resample(x: np.ndarray, sr: int) -> np.ndarray:
    """``x`` at 10 kHz in float64: ``x`` itself when ``sr`` is 10000."""
    if int(sr) == STOI_FS:
        return x
    from scipy.signal import resample_poly

    h, up, down, _ = stoi_taps(sr)
    return resample_poly(np.asarray(x, dtype=np.float64), up, down, window=h / np.sum(h))


def _stoi_frames(x: np.ndarray) -> np.ndarray:
    """Every full frame of ``x`` under hanning(258)[1:-1]: ``[frames, 256]``."""
    w = np.hanning(STOI_FRAME + 2)[1:-1]
    n = (len(x) - STOI_FRAME) // STOI_HOP + 1 if len(x) >= STOI_FRAME else 0
    idx = STOI_HOP * np.arange(n)[:, None] + np.arange(STOI_FRAME)[None, :]
    return w * x[idx]


def _stoi_rebuild(frames: np.ndarray) -> np.ndarray:
    out = np.zeros((len(frames) + 1) * STOI_HOP)
    for i, f in enumerate(frames):
        out[i * STOI_HOP:i * STOI_HOP + STOI_FRAME] += f
    return out


def _stoi_tob(x: np.ndarray) -> np.ndarray:
    """Third-octave band magnitudes ``[15, frames]`` of a rebuilt signal."""
    spec = np.fft.rfft(_stoi_frames(x), STOI_NFFT, axis=1)
    power = spec.real ** 2 + spec.imag ** 2
    return np.sqrt(np.stack([power[:, lo:hi].sum(axis=1) for lo, hi in third_octave_bands()]))


def stoi_reference(clean, est, sr: int = 16000, details: bool = False):
    """STOI of ``est`` against ``clean`` in numpy float64: the
    yardstick hvit_stoi is tested against.  Every full frame counts, the last
    one included.  With ``details`` the result is ``(score, K, margin, cond)``:
    the kept frames, the smallest distance in dB of a frame energy from the
    silence threshold and the smallest ``|x - mean x| / |x|`` over segments and
    bands (``inf`` where there is nothing to take the minimum of)."""
    x, y = _pair(clean, est)
    x, y = stoi_resample(x, sr), stoi_resample(y, sr)
    xf, yf = _stoi_frames(x), _stoi_frames(y)
    margin = cond = float("inf")
    if len(xf):
        e = 20.0 * np.log10(np.sqrt(np.sum(xf ** 2, axis=1)) + EPS)
        thr = np.max(e) - STOI_DYN
        keep = e > thr
        margin = float(np.min(np.abs(e - thr)))
        xf, yf = xf[keep], yf[keep]
    K = len(xf)
    if K < STOI_SEG:
        return (STOI_SHORT, K, margin, cond) if details else STOI_SHORT
    X, Y = _stoi_tob(_stoi_rebuild(xf)), _stoi_tob(_stoi_rebuild(yf))
    seg = np.arange(K - STOI_SEG + 1)[:, None] + np.arange(STOI_SEG)[None, :]
    xs, ys = X[:, seg], Y[:, seg]  # [15, segments, 30]
    nx = np.sqrt(np.sum(xs ** 2, axis=2, keepdims=True))
    ny = np.sqrt(np.sum(ys ** 2, axis=2, keepdims=True))
    yp = np.minimum((nx / (ny + EPS)) * ys, xs * (1.0 + 10.0 ** (-STOI_BETA / 20.0)))
    xm = xs - np.mean(xs, axis=2, keepdims=True)
    ym = yp - np.mean(yp, axis=2, keepdims=True)
    nxm = np.sqrt(np.sum(xm ** 2, axis=2, keepdims=True))
    xn = xm / (nxm + EPS)
    yn = ym / (np.sqrt(np.sum(ym ** 2, axis=2, keepdims=True)) + EPS)
    score = float(np.sum(xn * yn) / (STOI_BANDS * (K - STOI_SEG + 1)))
    if details:
        with np.errstate(divide="ignore", invalid="ignore"):
            r = nxm / nx
        if np.isfinite(r).any():
            cond = float(np.nanmin(r))
        return score, K, margin, cond
    return score


def _stoi_host(clean, est, sr: int, stoi: str) -> float:
    if stoi not in ("package", "native"):
        raise ValueError(f"hvit metrics: stoi={stoi!r} ('package' or 'native')")
    return compute_stoi(clean, est, sr) if stoi == "package" else stoi_reference(clean, est, sr)


def compute_all_metrics(clean: np.ndarray, enhanced: np.ndarray, noisy: Optional[np.ndarray] = None,
                        sr: int = 16000, stoi: str = "package") -> Dict[str, float]:
    """The reference's dict (metrics.py:299-349): six scores of ``enhanced`` and,
    with ``noisy``, four improvements over it.  ``stoi="native"`` takes STOI
    from ``stoi_reference`` instead of the ``pystoi`` package."""
    m = {
        "pesq": compute_pesq(clean, enhanced, sr),
        "stoi": _stoi_host(clean, enhanced, sr, stoi),
        "sisdr": compute_sisdr(clean, enhanced),
        "snr": compute_snr(clean, enhanced),
        "segsnr": compute_segsnr(clean, enhanced),
        "lsd": compute_lsd(clean, enhanced, sr),
    }
    if noisy is not None:
        m["pesq_improvement"] = m["pesq"] - compute_pesq(clean, noisy, sr)
        m["stoi_improvement"] = m["stoi"] - _stoi_host(clean, noisy, sr, stoi)
        m["sisdr_improvement"] = m["sisdr"] - compute_sisdr(clean, noisy)
        m["snr_improvement"] = m["snr"] - compute_snr(clean, noisy)
    return m


def print_metrics(metrics: Dict[str, float], title: str = "Metrics") -> None:
    """metrics.py:352-368."""
    rule = "=" * 50
    print(f"\n{title}\n{rule}")
    for name, value in metrics.items():
        print(f"{name.upper().replace('_', ' '):30s}: {value:8.4f}")
    print(rule)


# ------------------------------------------------------------------ device --

def _pair_arg(clean, est):
    """``(clean, est, B, L, row strides)`` of two batches of one shape and device."""
    clean, B, Ln, cs = wave_arg(clean, "hvit metrics", "clean")
    est, _, _, es = wave_arg(est, "hvit metrics", "est")
    if clean.shape != est.shape or clean.device != est.device:
        raise ValueError(f"hvit metrics: clean {tuple(clean.shape)} on {clean.device} and est {tuple(est.shape)} on "
                         f"{est.device} must match")
    return clean, est, B, Ln, cs, es


def _lengths(lengths, B: int, Ln: int, device) -> Optional[torch.Tensor]:
    """Host lengths are checked here (1 <= len <= L); a device tensor is the
    caller's word, since reading it back would synchronise."""
    if lengths is not None and not (isinstance(lengths, torch.Tensor) and lengths.is_cuda):
        host = np.asarray(lengths.numpy() if isinstance(lengths, torch.Tensor) else lengths).reshape(-1)
        if host.size and (host.min() < 1 or host.max() > Ln):
            raise ValueError(f"hvit metrics: lengths must lie in [1, {Ln}], got min {host.min()} max {host.max()}")
    return lengths_arg(lengths, B, device, "hvit metrics")


def wave_metrics(clean: torch.Tensor, est: torch.Tensor, lengths=None, frame_length: int = 512,
                 hop_length: int = 256, eps: float = 1e-8) -> torch.Tensor:
    """{SI-SDR, SNR, SegSNR} in dB of every row of ``est`` against ``clean``
    (float32 GPU ``[B, L]``; row b is ``[b, :lengths[b]]``) as float64 ``[B, 3]``,
    with compute_sisdr / compute_snr / compute_segsnr's definitions.
    ``frame_length`` must be a multiple of ``hop_length``, at most 16 times it."""
    clean, est, B, Ln, cs, es = _pair_arg(clean, est)
    if hop_length < 1 or frame_length < hop_length or frame_length % hop_length or frame_length > 16 * hop_length:
        raise ValueError(f"hvit metrics: frame_length={frame_length} must be a positive multiple of "
                         f"hop_length={hop_length}, at most 16 times it")
    dev = clean.device
    lens = _lengths(lengths, B, Ln, dev)
    n_ws = L.lib().hvit_wave_metrics_ws_elems(B, Ln, hop_length)
    ws = torch.empty(n_ws, dtype=torch.float64, device=dev)
    out = torch.empty((B, 3), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        L.call("hvit_wave_metrics", clean.data_ptr(), cs, est.data_ptr(), es, L.ptr(lens), B, Ln, frame_length,
               hop_length, float(eps), ws.data_ptr(), n_ws, out.data_ptr(), L.stream_ptr(dev))
    return out


def lsd(clean: torch.Tensor, est: torch.Tensor, lengths=None, n_fft: int = 512, hop_length: int = 128,
        eps: float = 1e-10) -> torch.Tensor:
    """Log-spectral distance of every row (compute_lsd's definition on the
    device front end's magnitudes) as float64 ``[B]``."""
    clean, est, B, Ln, _, _ = _pair_arg(clean, est)
    dev = clean.device
    lens = _lengths(lengths, B, Ln, dev)
    mag_c = FE.stft_mag(clean, lens, n_fft, hop_length, n_fft)
    mag_e = FE.stft_mag(est, lens, n_fft, hop_length, n_fft)
    F, T = mag_c.shape[2], mag_c.shape[3]
    n_ws = L.lib().hvit_lsd_ws_elems(B, T)
    ws = torch.empty(n_ws, dtype=torch.float64, device=dev)
    out = torch.empty(B, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        L.call("hvit_lsd", mag_c.data_ptr(), mag_e.data_ptr(), L.ptr(lens), B, F, T, hop_length, float(eps),
               ws.data_ptr(), n_ws, out.data_ptr(), L.stream_ptr(dev))
    return out


def _stoi_design(sr: int):
    h, up, down, half = stoi_taps(sr)
    return up * h / np.sum(h), up, down, half


def stoi(clean: torch.Tensor, est: torch.Tensor, lengths=None, sr: int = 16000) -> torch.Tensor:
    """STOI of every row of ``est`` against ``clean`` (``stoi_reference``'s
    definition) as float64 ``[B]``.  At another rate than 10 kHz both batches
    are first resampled in one call of 2 B rows with STOI's own filter
    (``stoi_taps``, rounded once to float32; the resampler sums in float64 and
    rounds each 10 kHz sample to float32 once: hvit_wave_resample_f64acc)."""
    clean, est, B, Ln, cs, es = _pair_arg(clean, est)
    dev = clean.device
    lens = _lengths(lengths, B, Ln, dev)
    if int(sr) != STOI_FS:
        table = RS.custom_taps_table(f"stoi-{int(sr)}", lambda: _stoi_design(sr), dev)
        both, out_lens = RS.resample_wave(torch.cat([clean, est]), None if lens is None else torch.cat([lens, lens]),
                                          sr, STOI_FS, taps=table, acc64=True)
        clean, est, lens, Ln = both[:B], both[B:], out_lens[:B], both.shape[1]
        cs = es = Ln
    n_ws = L.lib().hvit_stoi_ws_elems(B, Ln)
    ws = torch.empty(n_ws, dtype=torch.float64, device=dev)
    out = torch.empty(B, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        L.call("hvit_stoi", clean.data_ptr(), cs, est.data_ptr(), es, L.ptr(lens), B, Ln, ws.data_ptr(), n_ws,
               out.data_ptr(), L.stream_ptr(dev))
    return out


_stoi_device = stoi  # all_metrics_batch has a keyword of the same name


def _host_rows(package: str, attr: str, fn, clean, other, lens):
    """A host-only score (PESQ, STOI) per row; zeros without a download when its package is absent."""
    B, Ln = clean.shape
    if _optional(package, attr) is None:
        return torch.zeros(B, dtype=torch.float64, device=clean.device)
    c, o = clean.cpu().numpy(), other.cpu().numpy()
    n = [Ln] * B if lens is None else lens.cpu().tolist()
    return torch.tensor([fn(c[b, :n[b]], o[b, :n[b]]) for b in range(B)], dtype=torch.float64, device=clean.device)


def all_metrics_batch(clean: torch.Tensor, enhanced: torch.Tensor, noisy: Optional[torch.Tensor] = None,
                      lengths=None, stoi: str = "package", sr: int = 16000) -> Dict[str, torch.Tensor]:
    """compute_all_metrics for a ragged GPU batch: float64 ``[B]`` device
    tensors under the reference's keys.  With ``noisy`` the enhanced and the
    noisy rows are scored against clean in one ``wave_metrics`` call of 2 B
    rows.  PESQ and STOI are host libraries: they are zeros unless the package
    can be imported, in which case the rows are downloaded for them.
    ``stoi="native"`` fills ``stoi`` (and ``stoi_improvement``) on the device
    instead (``stoi`` at ``sr``, enhanced and noisy in one call of 2 B rows)."""
    if stoi not in ("package", "native"):
        raise ValueError(f"hvit metrics: stoi={stoi!r} ('package' or 'native')")
    clean, B, Ln, _ = wave_arg(clean, "hvit metrics", "clean")
    enhanced = wave_arg(enhanced, "hvit metrics", "enhanced")[0]
    lens = _lengths(lengths, B, Ln, clean.device)
    if noisy is None:
        wm = wave_metrics(clean, enhanced, lens)
        st = _stoi_device(clean, enhanced, lens, sr) if stoi == "native" else None
    else:
        noisy = wave_arg(noisy, "hvit metrics", "noisy")[0]
        clean2, est2 = torch.cat([clean, clean]), torch.cat([enhanced, noisy])
        lens2 = None if lens is None else torch.cat([lens, lens])
        both = wave_metrics(clean2, est2, lens2)
        wm, wm_noisy = both[:B], both[B:]
        if stoi == "native":
            st2 = _stoi_device(clean2, est2, lens2, sr)
            st, st_noisy = st2[:B].contiguous(), st2[B:]
    m = {
        "pesq": _host_rows("pesq", "pesq", compute_pesq, clean, enhanced, lens),
        "stoi": st if stoi == "native" else _host_rows("pystoi", "stoi", compute_stoi, clean, enhanced, lens),
        "sisdr": wm[:, 0].contiguous(),
        "snr": wm[:, 1].contiguous(),
        "segsnr": wm[:, 2].contiguous(),
        "lsd": lsd(clean, enhanced, lens),
    }
    if noisy is not None:
        m["pesq_improvement"] = m["pesq"] - _host_rows("pesq", "pesq", compute_pesq, clean, noisy, lens)
        m["stoi_improvement"] = m["stoi"] - (st_noisy if stoi == "native" else
                                             _host_rows("pystoi", "stoi", compute_stoi, clean, noisy, lens))
        m["sisdr_improvement"] = m["sisdr"] - wm_noisy[:, 0]
        m["snr_improvement"] = m["snr"] - wm_noisy[:, 1]
    return m


__all__ = ["compute_pesq", "compute_stoi", "compute_sisdr", "compute_snr", "compute_segsnr", "compute_lsd",
           "compute_all_metrics", "print_metrics", "wave_metrics", "lsd", "all_metrics_batch", "stoi_taps",
           "third_octave_bands", "stoi_reference", "stoi"]
