"""CPU: the float64 STOI reference of hvit_amd/metrics.py (``stoi_taps``,
``third_octave_bands``, ``stoi_reference``) against the figures of
its definition and against its own invariants.  ``stoi_clip`` / ``stoi_pair``
are the fixtures the GPU tests (tests/test_gpu_stoi.py) share.

Every fixture is first checked for its conditioning (``details=True``): the
silence threshold is at least 0.01 dB away from every frame energy and no
segment is close to constant, so a comparison does not rest on a knife edge."""

import numpy as np
import pytest

BANDS = [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87),
         (87, 109), (109, 138), (138, 174), (174, 219)]
PARTIALS = (140.0, 310.0, 620.0, 1100.0, 1750.0, 2500.0, 3400.0)
SNRS = (20.0, 5.0, -5.0)
MIN_MARGIN_DB, MIN_COND = 0.01, 1e-3


def stoi_clip(n, seed, sr=16000):
    """A float32 clip of ``n`` samples: seven partials under a slow envelope
    (3 Hz and 0.7 Hz) over a Gaussian floor of 0.002; the leading tenth and a
    middle fifth are scaled by 1e-4 (silence)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n, dtype=np.float64) / sr
    phase = rng.uniform(0, 2 * np.pi, len(PARTIALS))
    carrier = sum(np.sin(2 * np.pi * f * t + p) / (1 + i) for i, (f, p) in enumerate(zip(PARTIALS, phase)))
    env = 0.5 + 0.35 * np.sin(2 * np.pi * 3.0 * t) + 0.15 * np.sin(2 * np.pi * 0.7 * t + 1.0)
    x = 0.2 * env * carrier + 0.002 * rng.standard_normal(n)
    x[:n // 10] *= 1e-4
    x[2 * n // 5:3 * n // 5] *= 1e-4
    return x.astype(np.float32)


def stoi_pair(n, seed, snr_db, sr=16000):
    """``(clean, clean + white noise at snr_db)``, float32."""
    clean = stoi_clip(n, seed, sr)
    noise = np.random.Generator(np.random.PCG64(7000 + seed)).standard_normal(n)
    gain = np.sqrt(np.mean(clean.astype(np.float64) ** 2) / np.mean(noise ** 2)) * 10.0 ** (-snr_db / 20.0)
    return clean, (clean + gain * noise).astype(np.float32)


def checked_reference(hv, clean, est, sr):
    """``(score, K)`` after asserting the fixture's two conditions."""
    score, K, margin, cond = hv.stoi_reference(clean, est, sr, details=True)
    assert margin >= MIN_MARGIN_DB, f"threshold margin {margin:.3e} dB"
    assert cond >= MIN_COND, f"conditioning {cond:.3e}"
    return score, K


def test_band_ranges_and_tap_figures(hv):
    assert hv.third_octave_bands() == BANDS
    h, up, down, half = hv.stoi_taps(16000)
    assert (up, down, half, len(h)) == (5, 8, 290, 581)
    assert abs(np.sum(h) - 4.99962522358066) <= 1e-12
    assert h.dtype == np.float64 and np.array_equal(h, h[::-1]) and np.argmax(h) == half
    assert hv.stoi_taps(48000)[1:3] == (5, 24) and hv.stoi_taps(8000)[1:3] == (5, 4)


@pytest.mark.parametrize("n, frames", [(16000, 77), (24001, 116)])
def test_identity_order_and_scale(hv, n, frames):
    from hvit_amd import metrics as M

    scores = []
    for snr in SNRS:
        clean, est = stoi_pair(n, 21, snr)
        assert len(M._stoi_frames(M.stoi_resample(clean, 16000))) == frames
        s, K = checked_reference(hv, clean, est, 16000)
        assert 30 <= K < frames
        for scale in (0.1, 10.0):  # scaled in float64: the scaling itself adds no rounding
            d = abs(hv.stoi_reference(clean, est.astype(np.float64) * scale, 16000) - s)
            assert d <= 1e-9, (snr, scale, d)
        scores.append(s)
    same = hv.stoi_reference(clean, clean, 16000)
    print(f"n={n}: K={K} of {frames} frames, STOI {scores} at {SNRS} dB, identity 1 - {1 - same:.2e}")
    assert abs(same - 1.0) <= 1e-12
    assert 1.0 > scores[0] > scores[1] > scores[2] > 0.0


def test_short_clip_scores_1e_5_exactly(hv):
    clean, est = stoi_pair(6400, 22, 5.0)
    score, K, margin, _ = hv.stoi_reference(clean, est, 16000, details=True)
    assert margin >= MIN_MARGIN_DB and 0 < K < 30  # 4000 samples at 10 kHz: 30 frames, not all of them kept
    assert score == 1e-5
    assert hv.stoi_reference(clean[:300], est[:300], 16000) == 1e-5  # no full frame at all
    assert hv.stoi_reference(clean[:4000], est[:4000], 10000, details=True)[1] < 30


def test_all_zero_rows_give_finite_values(hv):
    clean, est = stoi_pair(16000, 23, 5.0)
    zero = np.zeros_like(clean)
    for c, e in ((zero, est), (clean, zero), (zero, zero)):
        s = hv.stoi_reference(c, e, 16000)
        assert np.isfinite(s) and abs(s) <= 1.0, s


def test_10_khz_is_not_resampled(hv, monkeypatch):
    from hvit_amd import metrics as M
    import scipy.signal

    clean, est = stoi_pair(10000, 24, 5.0, sr=10000)
    x = clean.astype(np.float64)
    assert M.stoi_resample(x, 10000) is x
    y = M.stoi_resample(x, 16000)
    assert len(y) == 6250 and y.dtype == np.float64
    want, K = checked_reference(hv, clean, est, 10000)
    assert K >= 30

    def refuse(*a, **k):
        raise AssertionError("resample_poly called at 10 kHz")

    monkeypatch.setattr(scipy.signal, "resample_poly", refuse)
    assert hv.stoi_reference(clean, est, 10000) == want


def test_host_option_and_package_default(hv):
    clean, est = stoi_pair(16000, 25, 5.0)
    noisy = stoi_pair(16000, 25, -5.0)[1]
    native = hv.compute_all_metrics(clean, est, noisy, stoi="native")
    assert native["stoi"] == hv.stoi_reference(clean, est, 16000)
    assert native["stoi_improvement"] == native["stoi"] - hv.stoi_reference(clean, noisy, 16000) > 0
    default = hv.compute_all_metrics(clean, est, noisy)
    assert list(default) == list(native)
    assert {k: v for k, v in default.items() if "stoi" not in k} == {k: v for k, v in native.items() if "stoi" not in k}
    with pytest.raises(ValueError, match="stoi"):
        hv.compute_all_metrics(clean, est, stoi="fast")
