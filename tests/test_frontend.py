"""CPU: the host-visible side of the device STFT / iSTFT front end
(hvit_amd/frontend.py) and of the batched enhancement built on it: the table
of supported settings, the frame count, the refusal of CPU tensors, and
``enhance_batch`` / ``enhance_directory(batch_size=...)`` / the CLI flags with
the host front end, where batching must change nothing.
tests/test_gpu_frontend.py runs the kernels."""

import numpy as np
import pytest
import torch
import torch.nn as nn


class Identity(nn.Module):
    def forward(self, x):
        return x


def test_supported_table_edges(hv):
    from hvit_amd import frontend as FE

    for n_fft in (256, 512, 1024):
        assert FE.supported(n_fft, n_fft // 8, n_fft)
        assert FE.supported(n_fft, n_fft // 2, n_fft)
        assert FE.supported(n_fft, n_fft // 4, n_fft - 112)
        assert not FE.supported(n_fft, n_fft // 8 - 1, n_fft)
        assert not FE.supported(n_fft, n_fft // 2 + 1, n_fft)
        assert not FE.supported(n_fft, n_fft // 4, n_fft + 1)
    assert FE.supported(512, 128, 512) and FE.supported(512, 256, 400)
    assert not FE.supported(2048, 512, 2048)
    assert not FE.supported(128, 32, 128)
    assert not FE.supported(500, 125, 500)
    assert hv.supported is FE.supported and hv.stft_mag is FE.stft_mag and hv.istft_mag is FE.istft_mag


def test_n_frames(hv):
    from hvit_amd import frontend as FE

    assert [FE.n_frames(n, 128) for n in (0, 1, 127, 128, 300, 4001, 32000, 32640)] == [1, 1, 1, 2, 3, 32, 251, 256]
    assert FE.n_frames(4001, 256) == 16 and FE.n_frames(4001, 32) == 126
    assert hv.n_frames(255, 128) == 2


def test_cpu_tensor_is_refused(hv):
    from hvit_amd import frontend as FE

    with pytest.raises(RuntimeError, match="there is no CPU path"):
        FE.stft_mag(torch.zeros(1, 1000))
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        FE.istft_mag(torch.zeros(1, 1, 257, 8), torch.zeros(1, 257, 8, 2), 1000)


def test_device_frontend_refuses_unsupported_settings(hv):
    from hvit_amd import enhancer as E

    with pytest.raises(ValueError):
        E.AudioEnhancer(Identity(), device="cpu", n_fft=2048, hop_length=512, win_length=2048, frontend="device")
    with pytest.raises(ValueError):
        E.AudioEnhancer(Identity(), device="cpu", hop_length=63, frontend="device")
    with pytest.raises(ValueError):
        E.AudioEnhancer(Identity(), device="cpu", frontend="elsewhere")
    assert E.AudioEnhancer(Identity(), device="cpu").frontend == "host"


def test_enhance_batch_host_equals_per_clip(hv):
    """Two frame-count groups (63 and 76 frames), shuffled: the results come
    back in input order and equal the per-clip calls exactly."""
    from hvit_amd import enhancer as E

    lens = [9600, 8000, 9650, 8050, 9600]
    clips = [E.synthetic_clip(n / 16000.0, seed=50 + i)[:n] for i, n in enumerate(lens)]
    assert [len(c) for c in clips] == lens
    enh = E.AudioEnhancer(Identity(), "cpu")
    for normalize in (True, False):
        got = enh.enhance_batch(clips, normalize=normalize, batch_size=2)
        assert len(got) == len(clips)
        for c, g in zip(clips, got):
            assert g.dtype == np.float32 and np.array_equal(g, enh.enhance(c, normalize=normalize))


def test_enhance_directory_batched_writes_the_same_files(hv, tmp_path):
    from hvit_amd import enhancer as E

    d_in, d1, d4 = tmp_path / "in", tmp_path / "b1", tmp_path / "b4"
    d_in.mkdir()
    lens = [3200, 3300, 4000, 3200, 4100]
    for i, n in enumerate(lens):
        E.write_wav(d_in / f"n{i}.wav", E.synthetic_clip(n / 16000.0, seed=i)[:n], 16000)
    enh = E.AudioEnhancer(Identity(), device="cpu")
    enh.enhance_directory(d_in, d1)
    enh.enhance_directory(d_in, d4, batch_size=4)
    assert sorted(p.name for p in d4.iterdir()) == sorted(p.name for p in d1.iterdir()) == [
        f"n{i}.wav" for i in range(5)]
    for i in range(5):
        assert (d4 / f"n{i}.wav").read_bytes() == (d1 / f"n{i}.wav").read_bytes()


def test_cli_accepts_frontend_and_batch_size(hv):
    """The new flags parse (the mode checks, which come right after parsing,
    still fire) and bad values are argparse errors."""
    import enhance

    with pytest.raises(SystemExit):
        enhance.main(["--checkpoint", "x.pth", "--frontend", "device", "--batch-size", "4"])  # neither mode
    with pytest.raises(SystemExit):
        enhance.main(["--checkpoint", "x.pth", "--frontend", "host", "--batch-size", "2", "--input", "a.wav",
                      "--output", "b.wav", "--input-dir", "i", "--output-dir", "o"])  # both modes
    with pytest.raises(SystemExit):
        enhance.main(["--synthetic", "0.1", "--frontend", "gpu"])
    with pytest.raises(SystemExit):
        enhance.main(["--synthetic", "0.1", "--batch-size", "many"])


def test_cli_flags_reach_the_enhancer(hv, tmp_path, monkeypatch):
    """--frontend / --batch-size are passed on (directory mode, host front end,
    CPU identity model in place of the HybridViT)."""
    import enhance
    from hvit_amd import enhancer as E

    seen = {}
    real = E.AudioEnhancer

    class Spy(real):
        def __init__(self, model, **kw):
            seen["frontend"] = kw.get("frontend")
            kw["device"] = "cpu"
            super().__init__(Identity(), **kw)

        def enhance_directory(self, *a, **kw):
            seen["batch_size"] = kw.get("batch_size")
            return super().enhance_directory(*a, **kw)

    monkeypatch.setattr(E, "AudioEnhancer", Spy)
    monkeypatch.setattr(E, "load_model_for_inference", lambda ck, model, device: model)
    d_in, d_out = tmp_path / "in", tmp_path / "out"
    d_in.mkdir()
    clip = E.synthetic_clip(0.2, seed=1)
    E.write_wav(d_in / "a.wav", clip, 16000)
    (tmp_path / "cfg.yaml").write_text("model:\n  encoder:\n    channels: [8, 16, 32]\n  transformer:\n"
                                       "    embed_dim: 64\n    num_heads: 4\n    num_layers: 2\n  decoder:\n"
                                       "    channels: [32, 16, 8, 1]\n")
    enhance.main(["--checkpoint", "unused.pth", "--config", str(tmp_path / "cfg.yaml"), "--input-dir", str(d_in),
                  "--output-dir", str(d_out), "--frontend", "host", "--batch-size", "3", "--device", "cpu"])
    assert seen == {"frontend": "host", "batch_size": 3}
    assert np.abs(E.read_wav(d_out / "a.wav", 16000) - clip).max() < 1e-5
