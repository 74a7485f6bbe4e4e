"""Times the device STFT / iSTFT front end (hvit_amd/frontend.py) on the GPU
and the host framing it replaces on this machine's CPUs.

    python tools/bench_frontend.py [--batch 32] [--samples 32640] [--no-directory]

Shape: B = 32 clips of L = 32640 samples (T = 256 frames), n_fft 512, hop 128.
Device times are taken from a hipGraph that holds ``--inner`` back-to-back
launches, replayed between two events after a warm-up (so they are kernel
time, not Python enqueue time); the figure is the median over ``--rounds``
replays divided by the launches.  The eager per-call time (Python + ctypes +
allocator included) is printed beside it.  Bytes are the algorithmic minimum
from the shapes; the HBM fraction is bytes / time over the 8 TB/s peak.
"""

import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, spec


def graph_time(fn, inner, rounds):
    """Median microseconds per call of fn() from a captured graph of `inner` calls."""
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


def eager_time(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters


def host_time(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def report(name, med, best, eager, nbytes):
    print(f"{name:<44s} {med:9.2f} us (min {best:8.2f})  eager {eager:8.1f} us/call  "
          f"{nbytes / 1e6:7.2f} MB  {nbytes / (med * 1e-6) / 1e12:5.2f} TB/s  "
          f"HBM fraction {nbytes / (med * 1e-6) / HBM_PEAK:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=32640)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=31)
    ap.add_argument("--no-directory", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frontend: needs the GPU (a CPU run measures nothing)")

    import hvit_amd_loader

    hv = hvit_amd_loader.load()
    from hvit_amd import data as Dt
    from hvit_amd import enhancer as E

    B, Ln, N, HOP = a.batch, a.samples, 512, 128
    F, T = N // 2 + 1, 1 + Ln // HOP
    print(f"device {torch.cuda.get_device_name(0)}, torch threads {torch.get_num_threads()}, "
          f"B={B} L={Ln} F={F} T={T} n_fft={N} hop={HOP}")
    clips = [Dt.harmonic_pair(Ln, 100 + i)[1] for i in range(B)]
    wave = torch.from_numpy(np.stack(clips)).cuda()
    wave64 = torch.cat([wave, wave.flip(0)])[:2 * B].contiguous()
    mag, ph, st = hv.stft_mag(wave, None, return_phasor=True, normalize="max")
    gain = st[:, 1].contiguous()

    w_b, m_b, p_b, o_b = B * Ln * 4, B * F * T * 4, B * F * T * 8, B * Ln * 4
    print("\n-- device kernels (graph-replayed) --")
    cases = [
        ("stft_fwd (mag + phasor + stats)", lambda: hv.stft_mag(wave, None, return_phasor=True), w_b + m_b + p_b),
        ("stft_fwd (mag only)", lambda: hv.stft_mag(wave, None, normalize=None), w_b + m_b),
        ("stft_mag(max, phasor) = fwd + normalize", lambda: hv.stft_mag(wave, None, return_phasor=True,
                                                                       normalize="max"), w_b + 3 * m_b + p_b),
        ("istft_mag (gain)", lambda: hv.istft_mag(mag, ph, Ln, gain), m_b + p_b + o_b),
        (f"train input: stft_mag(minmax) of {2 * B} clips", lambda: hv.stft_mag(wave64, None, normalize="minmax"),
         2 * (w_b + 3 * m_b)),
    ]
    res = {}
    for name, fn, nbytes in cases:
        med, best = graph_time(fn, a.inner, a.rounds)
        res[name] = med
        report(name, med, best, eager_time(fn, 200), nbytes)
    norm = res[cases[2][0]] - res[cases[0][0]]
    print(f"spec_normalize alone (difference)            {norm:9.2f} us  {2 * m_b / 1e6:7.2f} MB  "
          f"HBM fraction {2 * m_b / (max(norm, 1e-3) * 1e-6) / HBM_PEAK:.3f}")
    print(f"device front end for {2 * B} training clips: {res[cases[4][0]] / 1e3:.4f} ms "
          f"(the B=32 train step it feeds replays in 4.47 ms)")

    # the same kernels at 8x the batch: B = 32 is two workgroups per CU, one round of
    # workgroups, so launch and per-workgroup latency weigh on the figures above
    big = wave.repeat(8, 1)
    mag8, ph8, st8 = hv.stft_mag(big, None, return_phasor=True, normalize="max")
    print(f"\n-- the same at B = {8 * B} --")
    for name, fn, nbytes in (
            ("stft_fwd (mag + phasor + stats)", lambda: hv.stft_mag(big, None, return_phasor=True),
             8 * (w_b + m_b + p_b)),
            ("istft_mag", lambda: hv.istft_mag(mag8, ph8, Ln, None), 8 * (m_b + p_b + o_b))):
        med, best = graph_time(fn, 10, a.rounds)
        report(name, med, best, eager_time(fn, 50), nbytes)
    del big, mag8, ph8, st8

    print("\n-- host framing of the same clips on this machine's CPUs (the default code path) --")
    host = E.AudioEnhancer(torch.nn.Identity(), device="cpu")

    def host_train():
        for c in clips:
            Dt.minmax(Dt.magnitude(c))

    def host_enh():
        for c in clips:
            s = host.stft(c)
            m, p = s.abs(), s.angle()
            host.istft(torch.polar(m, p), len(c))

    t_tr = host_time(host_train, 5)
    t_en = host_time(host_enh, 3)
    print(f"data.magnitude + minmax, {B} clips:            {t_tr:9.2f} ms  ({t_tr / B:.3f} ms / clip)")
    print(f"enhancer stft + abs/angle + polar + istft, {B}: {t_en:9.2f} ms  ({t_en / B:.3f} ms / clip)")

    if not a.no_directory:
        print("\n-- enhance_directory wall time (default HybridViT, fp32, random weights, WAV I/O included) --")
        torch.manual_seed(0)
        model = hv.create_hybrid_vit({}, precision="fp32").cuda().eval()
        with tempfile.TemporaryDirectory() as td:
            d_in = os.path.join(td, "in")
            os.makedirs(d_in)
            for i in range(B):
                E.write_wav(os.path.join(d_in, f"c{i:02d}.wav"), Dt.harmonic_pair(32000, 200 + i)[1], 16000)
            import contextlib
            import io

            for name, fe, bs in (("host front end, batch_size 1", "host", 1),
                                 (f"device front end, batch_size {B}", "device", B)):
                enh = E.AudioEnhancer(model, device="cuda", frontend=fe)
                ts = []
                for r in range(4):
                    out = os.path.join(td, f"out_{fe}_{r}")
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    with contextlib.redirect_stdout(io.StringIO()):
                        enh.enhance_directory(d_in, out, batch_size=bs)
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
                best = statistics.median(ts[1:])  # the first pass warms the code objects up
                print(f"{name:<34s} {best:9.2f} ms for {B} clips = {best / B:7.3f} ms / clip  (passes: "
                      + ", ".join(f"{t:.1f}" for t in ts) + ")")


if __name__ == "__main__":
    main()
