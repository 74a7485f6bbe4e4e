"""GPU: ``audio.WaveBatch`` and the one batching loop of
``AudioEnhancer.enhance_batch`` built on it.

``from_clips`` must give, row by row, exactly what a B = 1 ``resample_wave`` of
that clip gives (a row's result does not depend on its batch: bit equality),
with the lengths of the integer formula, the kernel's peak and zeros past each
row.  ``enhance_batch`` is compared with ``enhance`` of the clip resampled by
hand, within the bar tests/test_gpu_resample_pipeline.py sets between a batched
and a clip-by-clip run (its ``wave_tol``).  The shapes are the smallest at
which this can go wrong: a one-sample clip and a polyphase ratio that is no
plain decimation (160:441) for ``from_clips``; for ``enhance_batch`` an empty
clip, lengths on both sides of a hop boundary and two clips of one rate that
share a frame count but not a length.  The model's geometry (two 2x pools,
then 4x4 patches) asks for 16 frames or more, and a one-frame clip such as
127 samples is refused by its first block, with or without batching; so that
hop boundary is the first one the model can run: 2047 | 2048 samples, 16 | 17
frames."""

import numpy as np
import pytest
import torch

from test_gpu_resample_pipeline import KW, resampled, sine_mix, wave_tol

pytestmark = pytest.mark.gpu
DEV = "cuda"
SR = 16000
LENS = [1, 2, 383, 4001]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("rate,up,down", [(48000, 1, 3), (44100, 160, 441)])
def test_from_clips_resamples_each_row_as_alone(hv, rate, up, down):
    from hvit_amd import audio as A

    clips = [sine_mix(n, rate, 3 + i) for i, n in enumerate(LENS)]
    b = A.WaveBatch.from_clips(clips, DEV, rate, SR, peak=True)
    want_lens = [-(-n * up // down) for n in LENS]
    assert b.lens == want_lens and b.lengths.dtype == torch.int32 and b.lengths.cpu().tolist() == want_lens
    assert b.wave.is_cuda and b.wave.dtype == torch.float32 and tuple(b.wave.shape) == (len(LENS), max(want_lens))
    wave, peak = b.wave.cpu().numpy(), b.peak.cpu().numpy()
    for r, c in enumerate(clips):
        one, _ = hv.resample_wave(torch.from_numpy(c)[None].to(DEV), [c.size], rate, SR)
        one = one[0].cpu().numpy()
        assert one.shape == (want_lens[r],)
        assert np.array_equal(bits(wave[r, :want_lens[r]]), bits(one)), r
        assert not wave[r, want_lens[r]:].any(), r
        assert bits(peak[r]) == bits(np.abs(wave[r]).max()), r
    rows = b.rows()
    assert [y.shape for y in rows] == [(n,) for n in want_lens]
    assert all(np.array_equal(bits(y), bits(wave[r, :y.size])) for r, y in enumerate(rows))
    assert A.WaveBatch.from_clips(clips, DEV, rate, SR).peak is None


def test_from_clips_at_equal_rates_only_uploads(hv, monkeypatch):
    from hvit_amd import _lib as L
    from hvit_amd import audio as A

    called = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    clips = [sine_mix(n, SR, 20 + i) for i, n in enumerate(LENS)]
    clips[2] = 0.25 * clips[2]
    b = A.WaveBatch.from_clips(clips, DEV, SR, SR, peak=True)
    assert called == []  # no hvit_wave_resample launch, nor any other of the library's
    assert b.lens == LENS and b.lengths.dtype == torch.int32 and b.lengths.cpu().tolist() == LENS
    assert np.array_equal(bits(b.wave.cpu().numpy()), bits(A.pad_rows(clips)))
    assert np.array_equal(bits(b.peak.cpu().numpy()), bits([np.abs(c).max() for c in clips]))


def test_rows_are_copies(hv):
    from hvit_amd import audio as A

    clips = [sine_mix(n, SR, 30 + i) for i, n in enumerate((5, 3))]
    b = A.WaveBatch.from_clips(clips, DEV, SR, SR)
    rows = b.rows()
    assert all(y.flags.owndata and y.flags.writeable for y in rows)
    assert not np.shares_memory(rows[0], rows[1])
    rows[0][:] = 7.0
    again = b.rows()
    assert np.array_equal(again[0], clips[0]) and np.array_equal(again[1], clips[1])
    assert np.array_equal(rows[1], clips[1])


@pytest.fixture(scope="module")
def tiny(hv):
    torch.manual_seed(0)
    return hv.HybridViT(**KW, precision="fp32").to(DEV).eval()


@pytest.mark.parametrize("frontend", ["device", "host"])
def test_enhance_batch_mixed_rates_equals_by_hand(hv, tiny, frontend):
    from hvit_amd import enhancer as E

    # at 16 kHz: 0, 2047 (16 frames), 2048 (17), 4000 (32), 1934 (16, batched with the 2047), 4001 (32)
    lens = [0, 6141, 2048, 11025, 5800, 4001]
    rates = [16000, 48000, 16000, 44100, 48000, 16000]
    clips = [sine_mix(n, sr, 40 + i) if n else np.zeros(0, dtype=np.float32)
             for i, (n, sr) in enumerate(zip(lens, rates))]
    enh = E.AudioEnhancer(tiny, device=DEV, frontend=frontend, resample=True)
    plain = E.AudioEnhancer(tiny, device=DEV, frontend=frontend)
    got = enh.enhance_batch(clips, batch_size=2, rates=rates)
    assert len(got) == len(clips)
    assert got[0].dtype == np.float32 and got[0].shape == (0,)
    for i in range(1, len(clips)):  # input order: every result against its own clip's
        by_hand = resampled(hv, clips[i], rates[i])
        want = plain.enhance(by_hand)
        assert got[i].dtype == np.float32 and got[i].shape == want.shape == (-(-lens[i] * SR // rates[i]),)
        err = np.abs(got[i] - want).max()
        print(f"{frontend} clip {i} ({lens[i]} samples at {rates[i]} Hz): |batched - by hand| = {err:.2e} "
              f"(tol {wave_tol(want):.2e})")
        assert err < wave_tol(want), i
