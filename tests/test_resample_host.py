"""CPU: the host side of the resampler (resampler.py): the float64 formula
``resample_reference`` against scipy.signal.resample_poly, its ``out_range``,
the quality of the default Kaiser-windowed sinc at 48 -> 16 kHz, the
phase-major taps layout, and ``read_audio`` beside the unchanged ``read_wav``.

Bounds.  Reference against scipy: 1e-13 of max sum |h x| (both are float64
sums of the same <= 400 products; measured <= 9.1e-16).  Filter quality: the
Kaiser formula gives A = 8.7 + beta / 0.1102 = 143 dB, a ripple of 7e-8; the
bounds 1e-5 (passband, 7 kHz sits at the transition edge) and 1e-6 (stopband)
leave more than an order of magnitude (measured: passband 2.7e-9, 1.5e-8,
3.8e-7; stopband 2.7e-8, 2.2e-8, 9.5e-9, 5.6e-9; f32 taps at 10 kHz 7.6e-9)."""

import numpy as np
import pytest

CASES = [(48000, 16000, 1, 3, 1), (48000, 16000, 1, 3, 2), (48000, 16000, 1, 3, 1000),
         (44100, 16000, 160, 441, 3000), (22050, 16000, 320, 441, 2001), (8000, 16000, 2, 1, 700),
         (16000, 48000, 3, 1, 500)]


def _signal(n, seed):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal(n)


@pytest.mark.parametrize("orig,target,up,down,n", CASES)
def test_reference_matches_scipy_resample_poly(hv, orig, target, up, down, n):
    from scipy.signal import resample_poly

    from hvit_amd import resampler as R

    h, u, d, half = R.resample_taps(orig, target)
    assert (u, d) == (up, down) and h.shape == (2 * half + 1,) and h.dtype == np.float64
    assert half == 64 * max(up, down)
    x = _signal(n, 7 + n)
    want = resample_poly(x, up, down, window=h / up, padtype="constant")
    got, sabs, terms = R.resample_reference(x, orig, target, stats=True)
    assert got.shape == want.shape == (R.out_length(n, up, down),)
    scale = sabs.max()
    err = np.abs(got - want).max() / scale
    print(f"{orig}->{target} n={n}: |ref - scipy| / max sum|h x| = {err:.2e}")
    assert err <= 1e-13
    assert terms.max() <= (2 * half) // up + 1 and terms.min() >= 1
    assert np.array_equal(got, R.resample_reference(x, orig, target, taps=h))


def test_out_range_equals_the_slice_bit_for_bit(hv):
    from hvit_amd import resampler as R

    for orig, n, ranges in ((48000, 5000, [(0, 1), (0, 7), (500, 777), (1600, 1667), (1667, 1667)]),
                            (44100, 3000, [(0, 3), (1000, 1089), (1080, 1089)]),
                            (8000, 700, [(0, 1400), (1390, 1400), (3, 4)])):
        x = _signal(n, n)
        full, fs, ft = R.resample_reference(x, orig, 16000, stats=True)
        for m0, m1 in ranges:
            part, ps, pt = R.resample_reference(x, orig, 16000, out_range=(m0, m1), stats=True)
            assert part.shape == (m1 - m0,)
            assert np.array_equal(part, full[m0:m1]) and np.array_equal(ps, fs[m0:m1])
            assert np.array_equal(pt, ft[m0:m1])
        with pytest.raises(ValueError):
            R.resample_reference(x, orig, 16000, out_range=(0, full.size + 1))


def _tone_48_to_16(R, f, taps=None):
    x = np.sin(2 * np.pi * f * np.arange(48000) / 48000.0)
    y = R.resample_reference(x, 48000, 16000, taps=taps)
    assert y.shape == (16000,)
    m = np.arange(200, 16000 - 200)
    return y[m], np.sin(2 * np.pi * f * m / 16000.0)


@pytest.mark.parametrize("f", [1000.0, 6000.0, 7000.0])
def test_passband_tone_is_kept(hv, f):
    from hvit_amd import resampler as R

    y, want = _tone_48_to_16(R, f)
    err = np.abs(y - want).max()
    print(f"passband {f:.0f} Hz: {err:.2e}")
    assert err < 1e-5


@pytest.mark.parametrize("f", [8500.0, 9000.0, 10000.0, 12000.0])
def test_stopband_tone_is_removed(hv, f):
    from hvit_amd import resampler as R

    y, _ = _tone_48_to_16(R, f)
    print(f"stopband {f:.0f} Hz: {np.abs(y).max():.2e}")
    assert np.abs(y).max() < 1e-6


def test_stopband_with_f32_rounded_taps(hv):
    from hvit_amd import resampler as R

    h = R.resample_taps(48000, 16000)[0].astype(np.float32).astype(np.float64)
    y, _ = _tone_48_to_16(R, 10000.0, taps=h)
    print(f"stopband 10000 Hz, f32 taps: {np.abs(y).max():.2e}")
    assert np.abs(y).max() < 1e-6


@pytest.mark.parametrize("orig,target", [(48000, 16000), (44100, 16000), (22050, 16000), (8000, 16000), (16000, 48000)])
def test_phase_major_layout_round_trips(hv, orig, target):
    from hvit_amd import resampler as R

    h, up, down, half = R.resample_taps(orig, target)
    pp = R.taps_phase_major(h, up)
    J = -(-(2 * half + 1) // up)
    assert pp.shape == (up, J) and pp.flags["C_CONTIGUOUS"]
    for p, j in ((0, 0), (up - 1, 0), (0, J - 1), (up // 2, J // 2), (up - 1, J - 1)):
        t = p + j * up
        assert pp[p, j] == (h[t] if t <= 2 * half else 0.0)
    assert np.count_nonzero(pp) <= 2 * half + 1
    assert np.array_equal(R.taps_from_phase_major(pp, 2 * half + 1), h)


def test_taps_are_a_unit_gain_symmetric_lowpass(hv):
    from hvit_amd import resampler as R

    for orig, target in ((48000, 16000), (44100, 16000), (16000, 48000)):
        h, up, down, half = R.resample_taps(orig, target)
        assert np.array_equal(h, h[::-1])
        assert abs(h.sum() / up - 1.0) < 1e-6  # DC gain 1 after the polyphase split
    assert R.ratio(16000, 16000) == (1, 1)
    with pytest.raises(ValueError):
        R.ratio(0, 16000)


def test_read_audio_returns_the_rate_and_read_wav_still_refuses(hv, tmp_path):
    from scipy.io import wavfile

    from hvit_amd import enhancer as E

    clip = E.synthetic_clip(0.1, seed=2)
    p = tmp_path / "a48.wav"
    E.write_wav(p, clip, 48000)
    audio, sr = E.read_audio(p)
    assert sr == 48000 and audio.dtype == np.float32 and np.array_equal(audio, clip)
    with pytest.raises(ValueError, match="48000 Hz, expected 16000"):
        E.read_wav(p, 16000)
    assert np.array_equal(E.read_wav(p, 48000), clip)
    # integer stereo: the same scaling and mixdown as read_wav
    st = (np.stack([clip, -0.5 * clip], axis=1) * 32767).astype(np.int16)
    q = tmp_path / "s.wav"
    wavfile.write(str(q), 44100, st)
    audio, sr = E.read_audio(q)
    assert sr == 44100 and audio.shape == clip.shape and audio.dtype == np.float32
    assert np.array_equal(audio, E.read_wav(q, 44100))
    assert np.array_equal(audio, (st.astype(np.float32) / 32768.0).mean(axis=1))


def test_resample_wave_refuses_a_cpu_tensor(hv):
    import torch

    with pytest.raises(RuntimeError, match="GPU"):
        hv.resample_wave(torch.zeros(1, 100), None, 48000, 16000)
