"""Times the device resampler (hvit_amd/resampler.py, csrc/wave_resample.hip)
in front of the device STFT, and the host path it replaces.

    python tools/bench_resample.py [--batch 32] [--seconds 4.0] [--out profiles/resample_bench.txt]

Workload: B = 32 clips of 4 s at 48 kHz, and the same at 44.1 kHz, to 16 kHz.
Two paths from raw host samples to the magnitude batch, each timed end to end
by a host clock around work that ends in a device synchronise (median and
minimum over ``--reps`` passes after a warm-up of every shape):

    device   upload raw [B, L] -> resample_wave -> stft_mag(minmax)
    host     scipy.signal.resample_poly with the same taps, clip by clip, on this
             machine's CPUs -> upload [B, L_out] -> stft_mag(minmax)

and the resampling kernel alone, from a hipGraph holding ``--inner``
back-to-back launches replayed between two events (kernel time, not Python
enqueue time).  Its bytes are the algorithmic minimum from the shapes (input
read once, output written once); the HBM fraction is bytes / time over the
8 TB/s peak, and the FMA rate is terms / time.  Nothing is gated: the figures
are recorded (``--out`` gets a copy of everything printed).
"""

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, spec


def graph_time(fn, inner, rounds):
    """Median and minimum microseconds per call of fn() from a captured graph of `inner` calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / inner)
    return statistics.median(ts), min(ts)


def wall_ms(fn, reps, warm=2):
    """Median and minimum milliseconds of fn(), which must end synchronised."""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=31)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample: needs the GPU (a CPU run measures nothing)")
    from scipy.signal import resample_poly

    import hvit_amd_loader

    hv = hvit_amd_loader.load()
    from hvit_amd import resampler as R

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    B, SR = a.batch, 16000
    say(f"device {torch.cuda.get_device_name(0)}, torch threads {torch.get_num_threads()}, B={B} clips of "
        f"{a.seconds:g} s to {SR} Hz, then stft_mag(n_fft 512, hop 128, minmax)")
    for orig in (48000, 44100):
        Ln = int(round(a.seconds * orig))
        h, up, down, half = R.resample_taps(orig, SR)
        Lo = R.out_length(Ln, up, down)
        terms = (2 * half) // up + 1
        rng = np.random.Generator(np.random.PCG64(orig))
        raw = (0.3 * rng.standard_normal((B, Ln))).astype(np.float32)
        dev_raw = torch.from_numpy(raw).cuda()
        lens = [Ln] * B
        say(f"\n== {orig} -> {SR} Hz: up:down = {up}:{down}, {2 * half + 1} taps (table {4 * up * terms / 1e3:.1f} KB), "
            f"L = {Ln} -> L_out = {Lo}, about {terms} terms per output ==")

        def device_path():
            w = torch.from_numpy(raw).cuda()
            y, ol = R.resample_wave(w, lens, orig, SR)
            m = hv.stft_mag(y, ol, normalize="minmax")
            torch.cuda.synchronize()
            return m

        def host_resample():
            return np.stack([resample_poly(raw[b].astype(np.float64), up, down, window=h / up,
                                           padtype="constant").astype(np.float32) for b in range(B)])

        def host_path():
            y = torch.from_numpy(host_resample()).cuda()
            m = hv.stft_mag(y, None, normalize="minmax")
            torch.cuda.synchronize()
            return m

        md, mh = device_path(), host_path()
        say(f"magnitudes of the two paths differ by at most {float((md - mh).abs().max()):.2e} (min-max scaled to [0, 1])")
        d_med, d_min = wall_ms(device_path, a.reps)
        h_med, h_min = wall_ms(host_path, max(3, a.reps // 3), warm=1)
        r_med, _ = wall_ms(lambda: host_resample(), max(3, a.reps // 3), warm=0)
        say(f"device path (upload raw + resample_wave + stft_mag)   {d_med:9.3f} ms (min {d_min:8.3f})  "
            f"= {d_med / B:7.4f} ms / clip")
        say(f"host path (resample_poly + upload + stft_mag)         {h_med:9.3f} ms (min {h_min:8.3f})  "
            f"= {h_med / B:7.4f} ms / clip, of which resample_poly {r_med:.3f} ms")
        say(f"end to end: host / device = {h_med / d_med:.1f} x")

        # lengths=None (every row is L long): a host list would be uploaded inside the capture
        k_med, k_min = graph_time(lambda: R.resample_wave(dev_raw, None, orig, SR, return_peak=True), a.inner,
                                  a.rounds)
        nbytes = 4 * B * (Ln + Lo)
        fma = B * Lo * terms
        say(f"resample kernel alone (with peak), graph-replayed     {k_med:9.2f} us (min {k_min:8.2f})  "
            f"{nbytes / 1e6:6.2f} MB  {nbytes / (k_med * 1e-6) / 1e12:5.3f} TB/s  HBM fraction "
            f"{nbytes / (k_med * 1e-6) / HBM_PEAK:.4f}  {fma / (k_med * 1e-6) / 1e12:5.2f} T fma/s")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
