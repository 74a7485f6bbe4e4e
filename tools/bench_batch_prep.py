"""Times assembling one training batch two ways: the hvit_batch_prep launch over
a device-resident SpectrogramStore (hvit_amd/data.py, csrc/batch_prep.hip), and
the same batch built on the host the way the reference's workers and collate_fn
do (index the cached spectrograms, mask, gain, pad, stack, upload).

    python tools/bench_batch_prep.py [--batch 32] [--frames 400] [--out profiles/batch_prep_bench.txt]

Shape: B = 32 clips of F = 257 bins drawn from a store of 1024 utterances of 300
to ``--frames`` frames, padded to Tb = ``--frames``, the reference's default
augmentation.  The device time is taken from a hipGraph that holds ``--inner``
back-to-back launches (each with its hvit_rng_advance, each on another batch of
the store and into outputs of its own, so that nothing a launch touches is
left in the 256 MiB Infinity Cache by an earlier one), replayed between two
events after a warm-up:
the median over ``--rounds`` replays divided by the launches; the eager
per-call time (Python, ctypes and the allocator included) is printed beside it.
Bytes are the algorithmic minimum from the shapes: both stores' valid frames
read once (masked frames counted too: an upper bound of at most a few per cent)
plus both padded outputs written once; the HBM fraction is bytes / time over
the 8 TB/s peak.  The host path is timed with a wall clock, upload and
synchronisation included.  Also prints the device footprint of a synthetic
store and what it extrapolates to for VoiceBank-DEMAND's training set.
Everything printed is also written to ``--out``.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--utterances", type=int, default=1024)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=31)
    ap.add_argument("--synthetic", type=int, default=128, help="clips of the synthetic store whose footprint is printed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_prep_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_batch_prep: needs the GPU (a CPU run measures nothing)")

    import hvit_amd_loader

    hv = hvit_amd_loader.load()
    from hvit_amd import data as D

    B, F, Tb, N = a.batch, 257, a.frames, a.utterances
    rng = np.random.Generator(np.random.PCG64(1))
    frames = rng.integers(min(300, Tb), Tb + 1, size=N).astype(np.int32)
    _, total = D.pack_offsets(frames, F)
    g = torch.Generator().manual_seed(2)
    noisy_h, clean_h = torch.rand(total, generator=g), torch.rand(total, generator=g)
    store = hv.SpectrogramStore(noisy_h.cuda(), clean_h.cuda(), frames, F)
    aug = hv.SpectrogramAugmenter()
    ld = hv.DeviceBatchLoader(store, B, shuffle=True, augmenter=aug, bucket_frames=1, seed=0)
    # disjoint batches, one per launch of the timed graph: with the store and the graph's outputs together far past
    # the 256 MiB Infinity Cache, every launch reads clips and writes outputs that no earlier launch left there
    order = rng.permutation(N).astype(np.int32)
    batches = [order[k * B:(k + 1) * B] for k in range(N // B)]
    if len(batches) < a.inner:
        raise SystemExit(f"bench_batch_prep: --utterances must be at least --inner * --batch = {a.inner * B}")
    batches_dev = [torch.from_numpy(h).cuda() for h in batches]
    idx_host = batches[0]
    read_b = 2 * 4 * F * int(np.mean([frames[h].sum() for h in batches[:a.inner]]))
    write_b = 2 * 4 * B * F * Tb + 4 * B * aug.plan_width
    nbytes = read_b + write_b
    say(f"device {torch.cuda.get_device_name(0)}, torch threads {torch.get_num_threads()}, B={B} F={F} Tb={Tb}, "
        f"store of {N} utterances of {int(frames.min())}..{int(frames.max())} frames ({store.nbytes / 2 ** 20:.1f} MiB), "
        f"{a.inner} disjoint batches per graph")
    say(f"bytes per batch (mean): {read_b / 1e6:.2f} MB read + {write_b / 1e6:.2f} MB written = {nbytes / 1e6:.2f} MB")

    say("\n-- device: hvit_rng_advance + hvit_batch_prep (graph-replayed) --")
    for name, loader in (("default augmentation", ld),
                         ("augmentation off (gather + pad)", hv.DeviceBatchLoader(store, B, augmenter=None,
                                                                                  bucket_frames=1))):
        turn, keep = [0], []

        def fn(loader=loader, turn=turn, keep=keep):
            k = turn[0] % a.inner
            turn[0] += 1
            keep.append(loader.prepare(batches_dev[k], batches[k], Tb=Tb))  # held: no launch reuses another's outputs

        med, best = graph_time(fn, a.inner, a.rounds)
        keep.clear()
        eag = eager_time(fn, 100)
        keep.clear()
        say(f"{name:<34s} {med:8.2f} us (min {best:7.2f})  eager {eag:7.1f} us/call  "
            f"{nbytes / (med * 1e-6) / 1e12:5.2f} TB/s  HBM fraction {nbytes / (med * 1e-6) / HBM_PEAK:.3f}")
        if loader is ld:
            dev_us = med

    say("\n-- host: index the cached clips, mask + gain (numpy draws), pad, stack, upload --")
    cache = [(noisy_h[o:o + F * t].view(1, F, t), clean_h[o:o + F * t].view(1, F, t))
             for o, t in ((int(o), int(t)) for o, t in zip(store.offsets, frames))]
    nrng = np.random.RandomState(0)

    def host_batch(upload=True):
        ns, cs = [], []
        for i in idx_host:  # dataset.py:247-294 with the cache hit, augmentation.py:48-118
            n, c = cache[i]
            n = n.clone()
            for _ in range(aug.freq_mask_num):
                f = nrng.randint(0, aug.freq_mask_width)
                f0 = nrng.randint(0, max(1, F - f))
                n[:, f0:f0 + f, :] = 0
            for _ in range(aug.time_mask_num):
                t = nrng.randint(0, min(aug.time_mask_width, n.shape[-1]))
                t0 = nrng.randint(0, max(1, n.shape[-1] - t))
                n[:, :, t0:t0 + t] = 0
            if nrng.rand() < aug.gain_probability:
                n = n * 10 ** (nrng.uniform(*aug.gain_db_range) / 20)
            ns.append(n), cs.append(c)
        mt = max(x.shape[-1] for x in ns)  # dataset.py:309-347
        nb = torch.stack([torch.nn.functional.pad(x, (0, mt - x.shape[-1])) for x in ns])
        cb = torch.stack([torch.nn.functional.pad(x, (0, mt - x.shape[-1])) for x in cs])
        if upload:
            nb, cb = nb.cuda(), cb.cuda()
            torch.cuda.synchronize()
        return nb, cb

    t_host = host_time(host_batch, 10)
    t_cpu = host_time(lambda: host_batch(False), 10)
    say(f"one batch in this process (no worker pool):   {t_host:8.3f} ms  (of which before the upload: {t_cpu:.3f} ms)")
    say(f"host / device: {t_host * 1e3 / dev_us:.0f}x; a 4.5 ms train step leaves the host path "
        f"{4.5 / t_host:.2f} batches per step and process")

    say("\n-- store footprint --")
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    syn = hv.SpectrogramStore.synthetic(a.synthetic, (2.0, 4.0), seed=0, device="cuda")
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - m0
    secs = float((syn.frames.astype(np.int64) - 1).sum()) * D.HOP / D.SR
    say(f"SpectrogramStore.synthetic({a.synthetic}, (2.0, 4.0) s): {syn.nbytes / 2 ** 20:.1f} MiB of magnitudes "
        f"({held / 2 ** 20:.1f} MiB allocated with the index arrays), {int(syn.frames.sum())} frames, "
        f"{secs:.0f} s of audio: {syn.nbytes / secs / 1e3:.1f} kB per second of a pair")
    vb = 11572 * 2 * 4 * F * (1 + 3 * D.SR // D.HOP)
    say(f"VoiceBank-DEMAND training set at that rate (11572 pairs of 3 s, {1 + 3 * D.SR // D.HOP} frames each): "
        f"{vb / 1e9:.2f} GB")

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
