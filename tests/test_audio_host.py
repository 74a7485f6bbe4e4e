"""CPU: the host half of hvit_amd/audio.py -- the padded batch, the grouping,
the resampled length, WAV I/O -- and config.audio_settings.
tests/test_gpu_wave_batch.py runs ``WaveBatch`` on the device."""

import numpy as np
import pytest
import torch.nn as nn


class Identity(nn.Module):
    def forward(self, x):
        return x


def test_pad_rows_ragged(hv):
    from hvit_amd import audio as A

    rng = np.random.Generator(np.random.PCG64(1))
    clips = [rng.standard_normal(n).astype(np.float32) for n in (5, 0, 1, 3)]
    got = A.pad_rows(clips)
    assert got.dtype == np.float32 and got.shape == (4, 5) and got.flags.c_contiguous
    for r, c in enumerate(clips):
        assert np.array_equal(got[r, :c.size], c) and not got[r, c.size:].any()
    wide = A.pad_rows(clips, width=8)
    assert wide.shape == (4, 8) and np.array_equal(wide[:, :5], got) and not wide[:, 5:].any()


def test_pad_rows_width_shorter_than_a_clip(hv):
    from hvit_amd import audio as A

    clips = [np.arange(1, 6, dtype=np.float32), np.arange(1, 3, dtype=np.float32)]
    got = A.pad_rows(clips, width=3)
    assert got.tolist() == [[1.0, 2.0, 3.0], [1.0, 2.0, 0.0]]


def test_pad_rows_converts_to_float32(hv):
    from hvit_amd import audio as A

    f64 = np.array([0.1, -0.2, 1.0 / 3.0], dtype=np.float64)
    pcm = np.array([-32768, 12345, 32767, 1], dtype=np.int16)
    from_pcm = pcm.astype(np.float32) / 32768.0
    got = A.pad_rows([f64, from_pcm, [0.5, 0.25]])
    assert got.dtype == np.float32 and got.shape == (3, 4)
    assert np.array_equal(got[0, :3], f64.astype(np.float32)) and got[0, 3] == 0.0
    assert np.array_equal(got[1], from_pcm)
    assert got[2].tolist() == [0.5, 0.25, 0.0, 0.0]


def test_batches(hv):
    from hvit_amd import audio as A

    assert A.batches([3, 1, 3, 3, 1], 2) == [[1, 4], [0, 2], [3]]
    assert A.batches([3, 1, 3, 3, 1], 0) == [[1], [4], [0], [2], [3]]  # a batch size below 1 counts as 1
    assert A.batches([(48000, 2), (16000, 9), (48000, 2)], 8) == [[1], [0, 2]]
    assert A.batches([], 4) == []


def test_frame_count_batches(hv):
    from hvit_amd import enhancer as E

    enh = E.AudioEnhancer(Identity(), "cpu")
    lens = [9600, 8000, 9650, 8050, 9600]  # 76, 63, 76, 63, 76 frames
    assert enh.frame_count_batches(lens, 2) == [[1, 3], [0, 2], [4]]
    assert enh.frame_count_batches(lens, 32) == [[1, 3], [0, 2, 4]]
    assert enh.frame_count_batches(lens, 1) == [[1], [3], [0], [2], [4]]


def test_out_length(hv):
    from hvit_amd import audio as A

    assert [A.out_length(n, 48000, 16000) for n in (0, 1, 2, 441)] == [0, 1, 1, 147]
    assert [A.out_length(n, 44100, 16000) for n in (0, 1, 2, 441)] == [0, 1, 1, 160]
    assert A.out_length(441, 16000, 16000) == 441 and A.out_length(160, 16000, 44100) == 441


def test_wav_round_trip(hv, tmp_path):
    from scipy.io import wavfile

    from hvit_amd import audio as A
    from hvit_amd import enhancer as E

    assert E.read_wav is A.read_wav and E.read_audio is A.read_audio and E.write_wav is A.write_wav
    assert {"read_wav", "read_audio", "write_wav"} <= set(E.__all__)
    rng = np.random.Generator(np.random.PCG64(2))
    x = rng.uniform(-1, 1, 321).astype(np.float32)
    A.write_wav(tmp_path / "x.wav", x.astype(np.float64), 44100)  # written as float32 whatever comes in
    got, sr = A.read_audio(tmp_path / "x.wav")
    assert sr == 44100 and got.dtype == np.float32 and np.array_equal(got, x)
    assert np.array_equal(A.read_wav(tmp_path / "x.wav", 44100), x)
    with pytest.raises(ValueError, match=r"is 44100 Hz, expected 16000 \(no resampler here\)"):
        A.read_wav(tmp_path / "x.wav", 16000)

    pcm = rng.integers(-32768, 32768, size=(200, 2)).astype(np.int16)
    pcm[0], pcm[1] = (-32768, -32768), (32767, 32767)
    wavfile.write(str(tmp_path / "stereo.wav"), 48000, pcm)
    got, sr = A.read_audio(tmp_path / "stereo.wav")
    want = (pcm.astype(np.float32) / 32768.0).mean(axis=1)
    assert sr == 48000 and got.dtype == np.float32 and got.shape == (200,) and np.array_equal(got, want)
    assert got[0] == -1.0 and got[1] == np.float32(32767.0 / 32768.0)
    assert np.array_equal(A.read_wav(tmp_path / "stereo.wav", 48000), want)


def test_audio_settings(hv):
    from hvit_amd import audio as A
    from hvit_amd import data as D

    assert (A.SR, A.N_FFT, A.HOP, A.WIN) == (16000, 512, 128, 512) == (D.SR, D.N_FFT, D.HOP, D.WIN)
    defaults = {"sample_rate": 16000, "n_fft": 512, "hop_length": 128, "win_length": 512}
    assert hv.audio_settings({}) == defaults
    assert hv.audio_settings({"audio": None}) == defaults
    assert hv.audio_settings({"audio": {"hop_length": 256, "sample_rate": 8000}, "model": {}}) == {
        "sample_rate": 8000, "n_fft": 512, "hop_length": 256, "win_length": 512}


def test_load_cli_configs_falls_back_with_a_warning(hv, tmp_path, capsys):
    (tmp_path / "extra.yaml").write_text("audio:\n  n_fft: 1024\n")
    cfg = hv.load_cli_configs(tmp_path / "absent", tmp_path / "extra.yaml")
    assert "Warning: Could not load config files. Using defaults." in capsys.readouterr().out
    assert cfg == {"audio": {"n_fft": 1024}}
    assert hv.load_cli_configs(tmp_path / "absent") == {}
