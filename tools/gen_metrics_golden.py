"""Generate tests/golden/metrics_cases.npz (build container only).

The reference's ``evaluation/metrics.py`` is loaded BY FILE PATH (the
``evaluation`` package itself imports librosa, which is not installed; the
module needs numpy alone) and its compute_sisdr / compute_snr / compute_segsnr
are recorded on harmonic clips (data.harmonic_pair) with white noise:

    clean_<i>, est_<i>   the float32 samples of case i
    names [K]            the case names
    expected [K, 3]      {SI-SDR, SNR, SegSNR} from the reference fed float64
                         casts of those samples (what the tests compare with)
    expected_f32 [K, 3]  the reference fed the float32 arrays as they are
                         (information only: its own f32 / f64 spread)

LSD is not recorded: without librosa the reference returns 0.0 for it.  The
script refuses to write a fixture with a NaN in ``expected`` or with a SegSNR
frame whose signal or noise power lies within a factor 2 of the 1e-8
threshold, where a rounding difference could flip the frame in or out.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_metrics_golden.py [--reference DIR]
"""

import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

OUT = os.path.join(ROOT, "tests", "golden", "metrics_cases.npz")
EDGE_LENGTHS = (1, 2, 511, 512, 513, 768, 769, 1024, 1025)
FRAME, HOP, EPS = 512, 256, 1e-8


def ref_metrics(reference):
    spec = importlib.util.spec_from_file_location("ref_evaluation_metrics",
                                                  os.path.join(reference, "evaluation", "metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases():
    import hvit_amd_loader

    hvit_amd_loader.load()
    from hvit_amd.data import harmonic_pair

    def pair(n, seed):
        c = harmonic_pair(n, seed)[0].astype(np.float64)
        return c, np.random.Generator(np.random.PCG64(1000 + seed)).standard_normal(n)

    out = []
    for seed, n in enumerate((4000, 769)):
        c, w = pair(n, seed)
        out.append((f"noisy_{n}", c, c + 0.15 * w))
    c, w = pair(4001, 2)
    out.append(("scaled_4001", c, 0.7 * c + 0.01 * w))
    c, w = pair(513, 3)
    out.append(("dc_513", c + 0.1, c + 0.05 * w + 0.3))
    c, w = pair(16000, 4)
    out.append(("hi_16000", c, 0.7 * c + 1e-4 * w + 0.25))
    c, w = pair(3000, 5)
    out.append(("quiet_3000", QUIET_CLEAN * c, QUIET_CLEAN * c + QUIET_NOISE * w))
    for k, n in enumerate(EDGE_LENGTHS):
        c, w = pair(n, 10 + k)
        out.append((f"len_{n}", c, c + 0.15 * w))
    c, w = pair(4000, 30)
    out.append(("same_4000", c, c))
    out.append(("zero_clean_4000", np.zeros(4000), c + 0.15 * w))
    out.append(("zero_est_4000", c, np.zeros(4000)))
    return [(name, a.astype(np.float32), b.astype(np.float32)) for name, a, b in out]


# The quiet case straddles the SegSNR threshold: at these scales the noise power of every frame is near
# 4e-8 and the signal power of 3 frames in 10 falls under 1e-8 (the nearest are 4.8e-9 and 2.1e-8).  At
# 1e-3 / 1e-4 the noise power sits on the threshold (about 1e-8 in every frame) and the assert below trips.
QUIET_CLEAN, QUIET_NOISE = 1.2e-3, 2e-4


def frame_powers(clean, est):
    c, e = clean.astype(np.float64), est.astype(np.float64)
    p = []
    for i in range(0, len(c) - FRAME, HOP):
        p += [np.mean(c[i:i + FRAME] ** 2), np.mean((e[i:i + FRAME] - c[i:i + FRAME]) ** 2)]
    return np.asarray(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference", help="checkout of the reference project")
    a = ap.parse_args()
    R = ref_metrics(a.reference)
    fns = (R.compute_sisdr, R.compute_snr, R.compute_segsnr)
    data, names, exp, exp32 = {}, [], [], []
    for i, (name, clean, est) in enumerate(cases()):
        with np.errstate(divide="ignore"):
            exp.append([f(clean.astype(np.float64), est.astype(np.float64)) for f in fns])
            exp32.append([f(clean, est) for f in fns])
        p = frame_powers(clean, est)
        near = p[(p >= 0.5 * EPS) & (p <= 2.0 * EPS)]
        assert near.size == 0, f"{name}: frame powers {near} within a factor 2 of eps"
        counted = int(np.sum((p[0::2] > EPS) & (p[1::2] > EPS)))
        print(f"{name:18s} n={len(clean):6d} sisdr={exp[-1][0]:12.6f} snr={exp[-1][1]:12.6f} "
              f"segsnr={exp[-1][2]:10.6f} frames counted {counted}/{p.size // 2}")
        data[f"clean_{i}"], data[f"est_{i}"] = clean, est
        names.append(name)
    exp, exp32 = np.asarray(exp, dtype=np.float64), np.asarray(exp32, dtype=np.float64)
    assert not np.isnan(exp).any(), "NaN in expected"
    fin = np.isfinite(exp) & np.isfinite(exp32)
    print(f"reference f32 / f64 spread: {np.abs(exp - exp32)[fin].max():.3e} dB")
    np.savez_compressed(OUT, names=np.asarray(names), expected=exp, expected_f32=exp32, **data)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(names)} cases")
    assert os.path.getsize(OUT) < 500_000


if __name__ == "__main__":
    main()
