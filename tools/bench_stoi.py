"""Times native STOI (hvit_amd.stoi: hvit_wave_resample with STOI's filter, then
csrc/stoi.hip) on a batch that is resident on the GPU, and the host path it
replaces (download, then ``stoi_reference`` clip by clip).

    python tools/bench_stoi.py [--batch 32] [--seconds 4.0] [--out profiles/stoi_bench.txt]

Shape: B = 32 clips of 4 s at 16 kHz (L = 64000, 40000 samples at 10 kHz, 311
frames).  Device times are per call from a hipGraph of ``--inner`` back-to-back
calls, the median over ``--rounds`` replays between two events after a warm-up;
the eager per-call time (Python + ctypes + allocator) is printed beside it, as
tools/bench_metrics.py does.  Bytes are the algorithmic minimum from the
shapes: the resampler reads 2 B L and writes 2 B L10 floats; hvit_stoi reads the
clean rows once for the energies and both rows once per kept frame pair (hop
128 of 256: each sample twice), writes and reads 30 band values per frame as
f64.  The synthetic clips keep most frames, so the band stage runs at close to
its "every frame kept" size.  Everything printed is also written to ``--out``.
"""

import argparse
import os
import sys

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
    say(f"{name:<52s} {med:9.2f} us (min {best:8.2f})  eager {eager:8.1f} us/call  {nbytes / 1e6:8.2f} MB  "
        f"{nbytes / (med * 1e-6) / 1e12:5.2f} TB/s  HBM fraction {nbytes / (med * 1e-6) / HBM_PEAK:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=31)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stoi_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stoi: needs the GPU (a CPU run measures nothing)")

    import hvit_amd_loader

    hv = hvit_amd_loader.load()
    from hvit_amd import data as Dt
    from hvit_amd import metrics as M
    from hvit_amd import resampler as RS

    B, Ln = a.batch, int(round(a.seconds * Dt.SR))
    L10 = -(-Ln * 5 // 8)
    T = (L10 - 256) // 128 + 1
    say(f"device {torch.cuda.get_device_name(0)}, torch threads {torch.get_num_threads()}, B={B} L={Ln} "
        f"({a.seconds:g} s clips at 16 kHz), {L10} samples and {T} frames at 10 kHz")
    pairs = [Dt.harmonic_pair(Ln, 100 + i) for i in range(B)]
    # a white floor under the harmonics: without it the upper bands hold float32 rounding noise only and their
    # correlations say nothing (the device-against-reference figure below would measure that, not the kernels)
    floor = np.random.Generator(np.random.PCG64(5)).standard_normal((B, Ln))
    clean_h = (np.stack([p[0] for p in pairs]) + 1e-2 * floor).astype(np.float32)
    noisy_h = np.stack([p[1] for p in pairs])
    enh_h = (0.9 * clean_h + 0.1 * noisy_h).astype(np.float32)  # a stand-in for the enhancer's output
    clean, noisy, enh = (torch.from_numpy(x).cuda() for x in (clean_h, noisy_h, enh_h))
    kept = [hv.stoi_reference(clean_h[b], enh_h[b], 16000, details=True)[1] for b in range(2)]
    say(f"frames kept by the first two clips: {kept} of {T}")

    table = RS.custom_taps_table("stoi-16000", lambda: M._stoi_design(16000), clean.device)
    both10 = hv.resample_wave(torch.cat([clean, enh]), None, 16000, 10000, taps=table)[0]
    c10, e10 = both10[:B].contiguous(), both10[B:].contiguous()

    def stoi_bytes(rows):
        return rows * (L10 * 4 + 2 * 2 * L10 * 4 + 2 * 2 * 15 * T * 8)

    resample_b = 2 * B * (Ln + L10) * 4
    say("\n-- device (graph-replayed), waveforms resident on the GPU --")
    cases = [
        (f"hvit_stoi alone, {B} rows at 10 kHz", lambda: hv.stoi(c10, e10, sr=10000), stoi_bytes(B)),
        (f"stoi(sr=16000), {B} rows: resample 2B rows + hvit_stoi", lambda: hv.stoi(clean, enh, sr=16000),
         2 * B * Ln * 4 + resample_b + stoi_bytes(B)),  # the torch.cat feeding the 2 B-row resample
        ("all_metrics_batch(clean, enhanced, noisy)", lambda: hv.all_metrics_batch(clean, enh, noisy), 0),
        ("all_metrics_batch(..., stoi='native')", lambda: hv.all_metrics_batch(clean, enh, noisy, stoi="native"), 0),
    ]
    res = {}
    for name, fn, nbytes in cases:
        med, best = graph_time(fn, a.inner, a.rounds)
        res[name] = med
        if nbytes:
            report(name, med, best, eager_time(fn, 100), nbytes)
        else:
            say(f"{name:<52s} {med:9.2f} us (min {best:8.2f})  eager {eager_time(fn, 100):8.1f} us/call")
    say(f"native STOI adds {res[cases[3][0]] - res[cases[2][0]]:.2f} us to all_metrics_batch "
        f"({2 * B} rows resampled twice over: clean rides with enhanced and with noisy)")

    say("\n-- host: download the enhanced batch, stoi_reference per clip --")

    def host_path():
        e = enh.cpu().numpy()
        return [hv.stoi_reference(clean_h[b], e[b], 16000) for b in range(B)]

    t_host = host_time(host_path, 3)
    t_dl = host_time(lambda: enh.cpu(), 10)
    t_dev = host_time(lambda: hv.stoi(clean, enh, sr=16000).cpu(), 20)
    say(f"download {B} x {Ln} f32:                          {t_dl:9.3f} ms")
    say(f"stoi_reference x {B} (with the download):        {t_host:9.3f} ms  ({t_host / B:.3f} ms / clip)")
    say(f"stoi(sr=16000) + download of the [{B}] scores, eager, wall: {t_dev:9.3f} ms")
    say(f"host / device, end to end (wall, scores on the host): {t_host / t_dev:.1f}x")
    got = hv.stoi(clean, enh, sr=16000).cpu().numpy()
    want = np.array(host_path())
    say(f"device against stoi_reference on these clips: worst |diff| = {np.abs(got - want).max():.3e}")

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
