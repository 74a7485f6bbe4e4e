"""Times scoring a batch of enhanced clips two ways: on the GPU, where the
device front end leaves them (hvit_amd/metrics.py, csrc/metrics.hip), and on
the host after a download (the numpy functions of the same module).

    python tools/bench_metrics.py [--batch 32] [--seconds 4.0] [--out profiles/metrics_bench.txt]

Shape: B = 32 clips of 4 s at 16 kHz (L = 64000).  Device times are taken
from a hipGraph that holds ``--inner`` back-to-back calls, replayed between two
events after a warm-up (kernel time, not Python enqueue time): the median over
``--rounds`` replays divided by the calls; the eager per-call time (Python +
ctypes + allocator included) is printed beside it.  Bytes are the algorithmic
minimum from the shapes (8 * sum of L for the waveform kernel: two f32 reads
per sample); the HBM fraction is bytes / time over the 8 TB/s peak.  The host
path is timed with a wall clock around the download and the numpy functions.
The same calls on 0.25 s clips and on one 10 min clip show the launch-bound and
the one-row ends.  Everything printed is also written to ``--out``.
"""

import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_frontend import HBM_PEAK, eager_time, graph_time, host_time  # noqa: E402

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def report(name, med, best, eager, nbytes):
    say(f"{name:<46s} {med:9.2f} us (min {best:8.2f})  eager {eager:8.1f} us/call  {nbytes / 1e6:8.2f} MB  "
        f"{nbytes / (med * 1e-6) / 1e12:5.2f} TB/s  HBM fraction {nbytes / (med * 1e-6) / HBM_PEAK:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=31)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics: needs the GPU (a CPU run measures nothing)")

    import hvit_amd_loader

    hv = hvit_amd_loader.load()
    from hvit_amd import data as Dt

    B, Ln = a.batch, int(round(a.seconds * Dt.SR))
    F, T = 257, 1 + Ln // 128
    say(f"device {torch.cuda.get_device_name(0)}, torch threads {torch.get_num_threads()}, B={B} L={Ln} "
        f"({a.seconds:g} s clips), SegSNR 512 / 256, LSD n_fft 512 hop 128 (F={F} T={T})")
    pairs = [Dt.harmonic_pair(Ln, 100 + i) for i in range(B)]
    clean_h, noisy_h = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    enh_h = (0.9 * clean_h + 0.1 * noisy_h).astype(np.float32)  # a stand-in for the enhancer's output
    clean, noisy, enh = (torch.from_numpy(x).cuda() for x in (clean_h, noisy_h, enh_h))
    clean2, est2 = torch.cat([clean, clean]), torch.cat([enh, noisy])

    wave_b = 8 * B * Ln                      # two f32 reads per sample
    stft_b = B * Ln * 4 + B * F * T * 4      # one stft_mag: the waveform in, the magnitude out
    lsd_b = 2 * B * F * T * 4                # hvit_lsd alone: two magnitudes in
    say("\n-- device (graph-replayed), waveforms resident on the GPU --")
    mag_c, mag_e = hv.stft_mag(clean, None), hv.stft_mag(enh, None)
    L = hv._lib
    ws = torch.empty(L.lib().hvit_lsd_ws_elems(B, T), dtype=torch.float64, device="cuda")
    out = torch.empty(B, dtype=torch.float64, device="cuda")

    def lsd_kernel():
        L.call("hvit_lsd", mag_c.data_ptr(), mag_e.data_ptr(), None, B, F, T, 128, 1e-10, ws.data_ptr(), ws.numel(),
               out.data_ptr(), L.stream_ptr())

    cases = [
        (f"wave_metrics, {B} rows", lambda: hv.wave_metrics(clean, enh), wave_b),
        (f"wave_metrics, {2 * B} rows (enhanced + noisy)", lambda: hv.wave_metrics(clean2, est2), 2 * wave_b),
        ("hvit_lsd alone (two magnitudes in)", lsd_kernel, lsd_b),
        ("lsd = 2 x stft_mag + hvit_lsd", lambda: hv.lsd(clean, enh), 2 * stft_b + lsd_b),
        ("all_metrics_batch(clean, enhanced, noisy)", lambda: hv.all_metrics_batch(clean, enh, noisy),
         2 * wave_b + 2 * stft_b + lsd_b + 2 * wave_b),  # + the two torch.cat copies feeding the 2 B-row call
    ]
    res = {}
    for name, fn, nbytes in cases:
        med, best = graph_time(fn, a.inner, a.rounds)
        res[name] = med
        report(name, med, best, eager_time(fn, 100), nbytes)
    dev_all = res[cases[-1][0]]

    def scores_to_host():
        m = hv.all_metrics_batch(clean, enh, noisy)
        return torch.stack(list(m.values())).cpu()

    t_dev = host_time(scores_to_host, 20)
    say(f"all_metrics_batch + download of the [10, {B}] scores, eager, wall: {t_dev:9.3f} ms")

    say("\n-- host: download the enhanced batch, numpy functions per clip --")

    def host_path():
        e = enh.cpu().numpy()
        return [hv.compute_all_metrics(clean_h[b], e[b], noisy_h[b]) for b in range(B)]

    def host_wave_only():
        e = enh.cpu().numpy()
        for b in range(B):
            hv.compute_sisdr(clean_h[b], e[b]), hv.compute_snr(clean_h[b], e[b]), hv.compute_segsnr(clean_h[b], e[b])
            hv.compute_sisdr(clean_h[b], noisy_h[b]), hv.compute_snr(clean_h[b], noisy_h[b])

    t_host = host_time(host_path, 3)
    t_wave = host_time(host_wave_only, 3)
    t_dl = host_time(lambda: enh.cpu(), 10)
    say(f"download {B} x {Ln} f32:                          {t_dl:9.3f} ms")
    say(f"compute_all_metrics x {B} (with the download):   {t_host:9.3f} ms  ({t_host / B:.3f} ms / clip)")
    say(f"  of which SI-SDR / SNR / SegSNR (no LSD):       {t_wave:9.3f} ms")
    say(f"host / device, end to end (wall, scores on the host): {t_host / t_dev:.1f}x; "
        f"device kernel time alone {dev_all / 1e3:.3f} ms")

    say("\n-- the same calls on short clips (0.25 s) and on one long clip (10 min) --")
    for label, b2, n2 in (("32 x 0.25 s", 32, 4000), ("1 x 600 s", 1, 600 * Dt.SR)):
        c = torch.from_numpy(np.stack([Dt.harmonic_pair(n2, 7 + i)[0] for i in range(b2)])).cuda()
        e = (c * 0.9 + 0.01).contiguous()
        med, best = graph_time(lambda: hv.wave_metrics(c, e), a.inner, a.rounds)
        report(f"wave_metrics {label}", med, best, eager_time(lambda: hv.wave_metrics(c, e), 100), 8 * b2 * n2)
        if n2 <= 64000:
            med, best = graph_time(lambda: hv.lsd(c, e), a.inner, a.rounds)
            t2 = 1 + n2 // 128
            report(f"lsd {label}", med, best, eager_time(lambda: hv.lsd(c, e), 100),
                   2 * (b2 * n2 * 4 + b2 * F * t2 * 4) + 2 * b2 * F * t2 * 4)
    say("wave_metrics is two launches and lsd four: where a call's time is a few microseconds per launch whatever "
        "the bytes, it is launch-bound, and its HBM fraction says nothing about the kernels.")

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
