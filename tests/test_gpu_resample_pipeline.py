"""GPU: the opt-in resampling of the three entry points -- AudioEnhancer
(resample=True, keep_rate), SpectrogramStore.from_directory (data-config key
``resample``), Evaluator(resample=True) and the --resample flags of enhance.py
and train.py -- each against the same work done by hand: ``resample_wave`` of the
uploaded file, downloaded, through the path that existed before.

Tolerances.  Enhanced waveforms: ``1e-4 * max|want| + 1e-4``, the bar
tests/test_gpu_frontend.py sets between a batched and a clip-by-clip run of
the enhancer (test_enhance_batch_device, test_cli_device_frontend_directory);
the resampled clip itself is bit-identical on both sides (a row's result does
not depend on its batch).  Stores: bit equality.  Device scores: 1e-9, the bar
of tests/test_gpu_metrics.py between the Evaluator's report and B = 1 metrics;
host scores against the device metrics: its TOL_DB = 1e-5 dB (twice that for an
improvement, a difference of two scores)."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 16000
KW = dict(encoder_channels=[8, 16, 32], embed_dim=64, num_heads=4, num_layers=2, decoder_channels=[32, 16, 8, 1])
MODEL_YAML = ("model:\n  encoder:\n    channels: [8, 16, 32]\n  transformer:\n    embed_dim: 64\n    num_heads: 4\n"
              "    num_layers: 2\n  decoder:\n    channels: [32, 16, 8, 1]\n")
TOL_DB = 1e-5


def wave_tol(want):
    return 1e-4 * max(np.abs(want).max(), 1e-6) + 1e-4


@pytest.fixture(scope="module")
def tiny(hv):
    torch.manual_seed(0)
    return hv.HybridViT(**KW, precision="fp32").to(DEV).eval()


def sine_mix(n, sr, seed):
    """A mix of sines below 7 kHz generated at ``sr``, float32, peak below 1."""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / float(sr)
    x = np.zeros(n)
    for f in (220.0, 1310.0, 3170.0, 5900.0):
        x += rng.uniform(0.2, 1.0) * np.sin(2 * np.pi * f * (1 + 0.001 * seed) * t + rng.uniform(0, 2 * np.pi))
    return (0.7 * x / np.abs(x).max()).astype(np.float32)


def resampled(hv, audio, sr):
    """The clip resampled to SR by one B = 1 call, downloaded."""
    if sr == SR:
        return audio
    out, ol = hv.resample_wave(torch.from_numpy(audio)[None].to(DEV), [audio.size], sr, SR)
    return out[0, :int(ol[0])].cpu().numpy()


@pytest.mark.parametrize("frontend", ["device", "host"])
def test_enhance_file_resamples_on_the_device(hv, tiny, tmp_path, frontend):
    from hvit_amd import enhancer as E

    enh = E.AudioEnhancer(tiny, device=DEV, frontend=frontend, resample=True)
    plain = E.AudioEnhancer(tiny, device=DEV, frontend=frontend)
    for sr, n in ((48000, 14400), (44100, 11025)):
        src, dst = tmp_path / f"in{sr}.wav", tmp_path / f"out{sr}.wav"
        audio = sine_mix(n, sr, sr % 7)
        E.write_wav(src, audio, sr)
        enh.enhance_file(src, dst)
        got = E.read_wav(dst, SR)  # written at the enhancer's rate
        clip = resampled(hv, audio, sr)
        want = plain.enhance(clip)
        assert got.shape == want.shape == (-(-n * SR // sr),)
        err = np.abs(got - want).max()
        print(f"{frontend} {sr}: |file - by hand| = {err:.2e} (tol {wave_tol(want):.2e})")
        assert err < wave_tol(want)
        with pytest.raises(ValueError):
            plain.enhance_file(src, tmp_path / "never.wav")
        with pytest.raises(ValueError):
            plain.enhance_batch([audio], rates=[sr])
    assert not (tmp_path / "never.wav").exists()


def test_keep_rate_writes_the_input_rate_and_length(hv, tiny, tmp_path):
    from hvit_amd import enhancer as E
    from hvit_amd import resampler as R

    enh = E.AudioEnhancer(tiny, device=DEV, frontend="device", resample=True)
    n = 14401
    audio = sine_mix(n, 48000, 3)
    E.write_wav(tmp_path / "in.wav", audio, 48000)
    enh.enhance_file(tmp_path / "in.wav", tmp_path / "kept.wav", keep_rate=True)
    enh.enhance_file(tmp_path / "in.wav", tmp_path / "at16.wav")
    got, sr = E.read_audio(tmp_path / "kept.wav")
    assert sr == 48000 and got.shape == (n,) and np.isfinite(got).all()
    at16 = E.read_wav(tmp_path / "at16.wav", SR)
    back, _ = hv.resample_wave(torch.from_numpy(at16)[None].to(DEV), [at16.size], SR, 48000)
    want = back[0, :n].cpu().numpy()
    # the back-conversion is linear: an input difference grows by at most the largest phase's sum |taps|
    amp = float(R.taps_table(SR, 48000, DEV)[0].abs().sum(1).max())
    assert np.abs(got - want).max() < amp * wave_tol(at16)


def test_directory_with_mixed_rates_batched_equals_one_by_one(hv, tiny, tmp_path):
    from hvit_amd import enhancer as E

    d_in, d_b, d_1 = tmp_path / "in", tmp_path / "batched", tmp_path / "single"
    d_in.mkdir()
    files = [(48000, 14400), (44100, 11025), (16000, 4800), (48000, 14350), (44100, 13230), (48000, 12000)]
    for i, (sr, n) in enumerate(files):
        E.write_wav(d_in / f"f{i}.wav", sine_mix(n, sr, 10 + i), sr)
    enh = E.AudioEnhancer(tiny, device=DEV, frontend="device", resample=True)
    enh.enhance_directory(d_in, d_b, batch_size=4)
    enh.enhance_directory(d_in, d_1)
    for i, (sr, n) in enumerate(files):
        a, b = E.read_wav(d_b / f"f{i}.wav", SR), E.read_wav(d_1 / f"f{i}.wav", SR)
        assert a.shape == b.shape == (-(-n * SR // sr),)
        assert np.abs(a - b).max() < wave_tol(b)


def _write_pairs(E, noisy_dir, clean_dir, sr, lengths, seed):
    from hvit_amd.data import harmonic_pair

    noisy_dir.mkdir(parents=True)
    clean_dir.mkdir(parents=True)
    pairs = []
    for i, (nn, nc) in enumerate(lengths):
        c = sine_mix(nc, sr, seed + i)
        nz = (sine_mix(nn, sr, seed + i) + 0.05 * harmonic_pair(nn, seed + i)[1]).astype(np.float32)
        E.write_wav(noisy_dir / f"p{i}.wav", nz, sr)
        E.write_wav(clean_dir / f"p{i}.wav", c, sr)
        pairs.append((nz, c))
    return pairs


def test_store_from_a_48k_directory(hv, tmp_path):
    from hvit_amd import enhancer as E
    from hvit_amd.data import TEST_DIRS

    lengths = [(14400, 14400), (12000, 12010), (9700, 9600), (14400, 13000), (6000, 6000)]
    pairs = _write_pairs(E, tmp_path / TEST_DIRS[0], tmp_path / TEST_DIRS[1], 48000, lengths, 30)
    got = hv.SpectrogramStore.from_directory(tmp_path, "test", {"resample": True}, device=DEV, chunk=3)
    noisy16 = [resampled(hv, nz, 48000) for nz, _ in pairs]
    clean16 = [resampled(hv, c, 48000) for _, c in pairs]
    cut = [min(a.size, b.size) for a, b in zip(noisy16, clean16)]
    want = hv.SpectrogramStore.from_waves([a[:n] for a, n in zip(noisy16, cut)],
                                          [b[:n] for b, n in zip(clean16, cut)], DEV, chunk=3)
    assert np.array_equal(got.frames, want.frames) and len(got) == len(pairs)
    assert got.frames.tolist() == [1 + n // 128 for n in cut]
    for i in range(len(pairs)):
        for g, w in zip(got.get(i), want.get(i)):
            assert torch.equal(g, w), i
    # from_waves(rates=...) itself, with a pair whose two files differ in rate
    mixed = hv.SpectrogramStore.from_waves([p[0] for p in pairs[:2]], [clean16[0], pairs[1][1]], DEV,
                                           rates=[(48000, SR), 48000])
    for i in range(2):
        for g, w in zip(mixed.get(i), want.get(i)):
            assert torch.equal(g, w), i
    with pytest.raises(ValueError):
        hv.SpectrogramStore.from_directory(tmp_path, "test", {}, device=DEV)
    with pytest.raises(ValueError):
        hv.SpectrogramStore.from_directory(tmp_path, "test", {"resample": False}, device=DEV)


@pytest.mark.parametrize("frontend", ["device", "host"])
def test_evaluator_on_48k_pairs(hv, tiny, tmp_path, frontend):
    from hvit_amd import enhancer as E
    from hvit_amd import metrics as M

    noisy_dir, clean_dir, out_dir = tmp_path / "noisy", tmp_path / "clean", tmp_path / "enh"
    lengths = [(12000, 12000), (11907, 12000), (9000, 8990), (7500, 7500)]
    pairs = _write_pairs(E, noisy_dir, clean_dir, 48000, lengths, 50)
    with pytest.raises(ValueError):
        hv.Evaluator(tiny, device=DEV, frontend=frontend).evaluate_dataset(noisy_dir, clean_dir)
    ev = hv.Evaluator(tiny, device=DEV, frontend=frontend, batch_size=4, resample=True)
    res = ev.evaluate_dataset(noisy_dir, clean_dir, output_dir=out_dir, save_enhanced=True)
    assert res["num_files"] == len(pairs)
    worst = worst_host = 0.0
    for i, (nz, c) in enumerate(pairs):
        noisy, clean = resampled(hv, nz, 48000), resampled(hv, c, 48000)
        n = min(noisy.size, clean.size)
        noisy, clean = noisy[:n], clean[:n]
        saved = E.read_wav(out_dir / f"p{i}.wav", SR)  # the waveform that was scored, at the evaluator's rate
        assert saved.shape == (n,)
        row = res["per_file_metrics"][f"p{i}.wav"]
        want = hv.all_metrics_batch(*(torch.from_numpy(np.ascontiguousarray(a))[None].to(DEV)
                                      for a in (clean, saved, noisy)))
        assert list(row) == list(want)
        if frontend == "device":
            for k, v in want.items():
                worst = max(worst, abs(row[k] - float(v[0])))
        else:
            for k in ("sisdr", "snr", "segsnr", "sisdr_improvement", "snr_improvement"):
                worst = max(worst, abs(row[k] - float(want[k][0])) / (2.0 if k.endswith("improvement") else 1.0))
            host = M.compute_all_metrics(clean, saved, noisy, SR)
            for k, v in host.items():
                worst_host = max(worst_host, abs(row[k] - v))
    print(f"{frontend}: evaluator on 48 kHz files vs metrics of the resampled tensors: worst |diff| = {worst:.3e}")
    assert worst <= (1e-9 if frontend == "device" else TOL_DB)
    assert worst_host <= 1e-9


def test_cli_resample_flags(hv, tiny, tmp_path):
    """enhance.py --resample and train.py --resample in fresh child processes on
    two-file 48 kHz directories."""
    from hvit_amd import enhancer as E
    from hvit_amd.data import TRAIN_DIRS

    cfgdir = tmp_path / "config"
    cfgdir.mkdir()
    (cfgdir / "model_config.yaml").write_text(MODEL_YAML)
    (cfgdir / "train_config.yaml").write_text(
        f"training:\n  num_epochs: 1\n  batch_size: 2\n  checkpoint:\n    save_dir: {tmp_path / 'ckpt'}\n"
        f"  logging:\n    log_dir: {tmp_path / 'logs'}\n  graph:\n    warmup: 1\n")
    (cfgdir / "data_config.yaml").write_text("data:\n  sample_rate: 16000\n  train_val_split: 0.7\n")
    ck = tmp_path / "best_model.pth"
    torch.save({"epoch": 1, "model_state_dict": tiny.state_dict()}, ck)

    d_in, d_out = tmp_path / "noisy", tmp_path / "enhanced"
    d_in.mkdir()
    clips = [(48000, sine_mix(14400, 48000, 1)), (44100, sine_mix(11025, 44100, 2))]
    for i, (sr, c) in enumerate(clips):
        E.write_wav(d_in / f"u{i}.wav", c, sr)
    base = [sys.executable, os.path.join(ROOT, "enhance.py"), "--checkpoint", str(ck), "--config-dir", str(cfgdir),
            "--input-dir", str(d_in), "--output-dir", str(d_out), "--frontend", "device", "--batch-size", "2"]
    r = subprocess.run(base + ["--resample"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    plain = E.AudioEnhancer(tiny, device=DEV, frontend="device")
    for i, (sr, c) in enumerate(clips):
        got = E.read_wav(d_out / f"u{i}.wav", SR)
        want = plain.enhance(resampled(hv, c, sr))
        assert got.shape == want.shape and np.abs(got - want).max() < wave_tol(want)

    root = tmp_path / "corpus"
    # three pairs, two of them the training split: a training batch of one sample has no batch statistics to speak of
    _write_pairs(E, root / TRAIN_DIRS[0], root / TRAIN_DIRS[1], 48000,
                 [(14400, 14400), (12000, 12010), (14400, 14000)], 70)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--config-dir", str(cfgdir), "--data-root",
                        str(root), "--resample", "--precision", "fp32"], capture_output=True, text=True, timeout=240,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Training samples: 2" in r.stdout and "Validation samples: 1" in r.stdout
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("Best checkpoint: ")
    sd = torch.load(last.split(": ", 1)[1], map_location="cpu", weights_only=True)["model_state_dict"]
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
