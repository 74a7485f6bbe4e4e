"""sha256 of what the waveform entry points give -- AudioEnhancer
(enhance_batch, enhance_file), SpectrogramStore.from_waves, Evaluator,
stft_mag, wave_metrics and lsd -- on the tiny fp32 model with seeded host
inputs: one ``case name sha256`` line per output.  Only public API is used, so
the same file runs on two trees (``--root`` names the other checkout; it needs
its own built library): diff the listings, and a refactor of the Python around
those kernels must leave the diff empty."""

import argparse
import contextlib
import hashlib
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the checkout whose package is hashed (default: this file's)")
ROOT = os.path.abspath(ap.parse_args().root)
sys.path.insert(0, ROOT)
import hvit_amd_loader  # noqa: E402

hv = hvit_amd_loader.load()
from hvit_amd import enhancer as E  # noqa: E402

DEV = "cuda"
SR = 16000
KW = dict(encoder_channels=[8, 16, 32], embed_dim=64, num_heads=4, num_layers=2, decoder_channels=[32, 16, 8, 1])
# The model's geometry asks for 16 frames or more (two 2x pools, then 4x4 patches; its first block refuses a one-frame
# clip): the hop boundary that is hashed is the first one it can run, 2047 | 2048 samples (16 | 17 frames).
LENS = [0, 2047, 2048, 4001, 9600, 9650]
MIXED = [(0, 16000), (6141, 48000), (2048, 16000), (11025, 44100), (28800, 48000), (26600, 44100)]  # samples, rate


def emit(case, **arrays):
    torch.cuda.synchronize()
    for name, a in arrays.items():
        if isinstance(a, torch.Tensor):
            a = a.detach().cpu().contiguous().numpy()
        a = np.ascontiguousarray(a)
        print(f"{case} {name} {a.dtype}{list(a.shape)} {hashlib.sha256(a.tobytes()).hexdigest()}", flush=True)


def clip(n, seed, sr=SR):
    """Seeded sines plus noise, float32, peak below 1 (0.9 for every other seed, so the peaks differ)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.arange(n) / float(sr)
    x = 0.1 * rng.standard_normal(n)
    for f in (220.0, 1310.0, 5900.0):
        x += rng.uniform(0.2, 1.0) * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
    if n:
        x *= (0.9 if seed % 2 else 0.6) / np.abs(x).max()
    return x.astype(np.float32)


def model():
    torch.manual_seed(0)
    return hv.HybridViT(**KW, precision="fp32").to(DEV).eval()


def enhance_batch(m):
    plain = [clip(n, 10 + i) for i, n in enumerate(LENS)]
    mixed = [clip(n, 10 + i, sr) for i, (n, sr) in enumerate(MIXED)]
    for frontend in ("device", "host"):
        enh = E.AudioEnhancer(m, device=DEV, frontend=frontend, resample=True)
        for normalize in (True, False):
            for what, clips, rates in (("no rates", plain, None), ("mixed rates", mixed, [sr for _, sr in MIXED])):
                if frontend == "host" and rates is None:
                    clips = clips[1:]  # this path hands every clip to enhance(), and the model refuses an empty one
                ys = enh.enhance_batch(clips, normalize=normalize, batch_size=2, rates=rates)
                emit(f"enhance_batch {frontend} normalize={int(normalize)} {what}",
                     **{f"clip{i}_{c.size}": y for i, (c, y) in enumerate(zip(clips, ys))})


def enhance_file(m, tmp):
    E.write_wav(tmp / "in48.wav", clip(14401, 3, 48000), 48000)
    for frontend in ("device", "host"):
        enh = E.AudioEnhancer(m, device=DEV, frontend=frontend, resample=True)
        with contextlib.redirect_stdout(sys.stderr):  # its "saved to" line names the temporary folder
            enh.enhance_file(tmp / "in48.wav", tmp / f"kept_{frontend}.wav", keep_rate=True)
        y, sr = E.read_audio(tmp / f"kept_{frontend}.wav")
        emit(f"enhance_file keep_rate {frontend} sr={sr}", wave=y)


def store():
    noisy = [clip(n, 20 + i) for i, n in enumerate((14400, 4001, 11025))]
    clean = [clip(n, 30 + i) for i, n in enumerate((14400, 4100, 11000))]
    for what, kw in (("no rates", {}), ("rates", {"rates": [(48000, 16000), 48000, 44100]})):
        st = hv.SpectrogramStore.from_waves(noisy, clean, DEV, chunk=2, **kw)
        emit(f"from_waves {what}", noisy=st.noisy, clean=st.clean, frames=st.frames)


def evaluator(m, tmp):
    nd, cd = tmp / "noisy", tmp / "clean"
    nd.mkdir()
    cd.mkdir()
    for i, (nn, nc) in enumerate([(12000, 12000), (11907, 12000), (9000, 8990), (7500, 7500)]):
        E.write_wav(nd / f"p{i}.wav", clip(nn, 40 + i, 48000), 48000)
        E.write_wav(cd / f"p{i}.wav", clip(nc, 50 + i, 48000), 48000)
    for frontend in ("device", "host"):
        ev = hv.Evaluator(m, device=DEV, frontend=frontend, batch_size=4, resample=True)
        with contextlib.redirect_stdout(sys.stderr):
            res = ev.evaluate_dataset(nd, cd, output_dir=tmp / f"enh_{frontend}", save_enhanced=True)
        names = sorted(res["per_file_metrics"])
        keys = list(res["per_file_metrics"][names[0]])
        table = np.array([[res["per_file_metrics"][n][k] for k in keys] for n in names], dtype=np.float64)
        emit(f"evaluator {frontend}", scores=table,
             **{n: E.read_audio(tmp / f"enh_{frontend}" / n)[0] for n in names})


def stft():
    x = torch.from_numpy(np.stack([clip(4001, 60 + i) for i in range(3)])).to(DEV)
    wide = torch.zeros((3, 2 * 4001), device=DEV)
    wide[:, ::2] = x
    lens = [4001, 383, 128]
    for what, ln in (("none", None), ("host", lens), ("device", torch.tensor(lens, dtype=torch.int32, device=DEV))):
        mag, phasor, stats = hv.stft_mag(wide[:, ::2], ln, return_phasor=True, normalize="max")
        emit(f"stft_mag strided lengths={what}", mag=mag, phasor=phasor, stats=stats)


def metrics():
    for B in (1, 3):
        c = torch.from_numpy(np.stack([clip(5000, 70 + i) for i in range(B)])).to(DEV)
        e = torch.from_numpy(np.stack([clip(5000, 80 + i) for i in range(B)])).to(DEV)
        c, e = c[:, 17:4018], e[:, 17:4018]  # column-sliced: row stride 5000, 4001 columns
        lens = [4001, 383, 2000][:B]
        emit(f"metrics B={B}", wave_metrics=hv.wave_metrics(c, e, lens), lsd=hv.lsd(c, e, lens),
             wave_metrics_full=hv.wave_metrics(c, e), lsd_full=hv.lsd(c, e))


def main():
    m = model()
    with tempfile.TemporaryDirectory() as d:
        tmp = Path(d)
        enhance_batch(m)
        enhance_file(m, tmp)
        store()
        evaluator(m, tmp)
    stft()
    metrics()


if __name__ == "__main__":
    main()
