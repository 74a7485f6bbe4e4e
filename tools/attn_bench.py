"""Attention micro-benchmark at the HybridViT shape (B=32, N=256, H=8, hd=64,
bf16, attention dropout 0.1): fwd and bwd timed with HIP events.  --tokens N
times another token count (N > 256: the chunked kernels); --fp8 the fp8 forms."""

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hvit_amd_loader  # noqa: E402
from gemm_bench import timeit as timeit_reps  # noqa: E402

hv = hvit_amd_loader.load()
L = hv._lib


def timeit(fn, window_us=3e5):
    """us per call over a timed window of about window_us (20 calls of a 16 us
    kernel time the clock).  The repetition count comes from a 50-call first
    pass after three warm-up calls, so the window is only as long as that pass
    is representative; the first pass runs every kernel once more, untimed."""
    return timeit_reps(fn, reps=max(20, int(window_us / timeit_reps(fn, reps=50)) + 1))


def main(p=0.1, N=256):
    B, H, hd = 32, 8, 64
    D = H * hd
    qkv = (torch.randn(B * N, 3 * D, device="cuda") * 0.7).to(torch.bfloat16)
    o = torch.empty(B * N, D, device="cuda", dtype=torch.bfloat16)
    lse = torch.empty(B, H, N, device="cuda")
    dr = L.dropout(p, 1, 2)
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    fwd = lambda: L.call("hvit_mhsa_fwd", L.BF16, qkv.data_ptr(), B, N, H, hd, hd ** -0.5, dr, o.data_ptr(),  # noqa
                         lse.data_ptr(), None, st())
    us = timeit(fwd)
    fl = 4 * B * H * N * N * hd
    print(f"N={N} mhsa fwd p={p}: {us:7.1f} us  {fl / us / 1e6:6.1f} TF/s", flush=True)
    do = torch.randn_like(o)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty(B, H, N, device="cuda")
    bwd = lambda: L.call("hvit_mhsa_bwd", L.BF16, qkv.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(),  # noqa
                         B, N, H, hd, hd ** -0.5, dr, dqkv.data_ptr(), delta.data_ptr(), st())
    us = timeit(bwd)
    print(f"N={N} mhsa bwd p={p}: {us:7.1f} us  {2 * fl / us / 1e6:6.1f} TF/s", flush=True)
    if p > 0:  # keep-bit variants (the training path)
        kb = torch.empty(L.lib().hvit_mhsa_keep_bits_elems(B, N, H), dtype=torch.int32, device="cuda")
        fwdk = lambda: L.call("hvit_mhsa_fwd_kb", L.BF16, qkv.data_ptr(), B, N, H, hd, hd ** -0.5, dr,  # noqa
                              o.data_ptr(), lse.data_ptr(), kb.data_ptr(), st())
        us = timeit(fwdk)
        print(f"N={N} mhsa fwd_kb p={p}: {us:7.1f} us  {fl / us / 1e6:6.1f} TF/s", flush=True)
        bwdk = lambda: L.call("hvit_mhsa_bwd_kb", L.BF16, qkv.data_ptr(), o.data_ptr(), do.data_ptr(),  # noqa
                              lse.data_ptr(), B, N, H, hd, hd ** -0.5, dr, kb.data_ptr(), dqkv.data_ptr(),
                              delta.data_ptr(), st())
        us = timeit(bwdk)
        print(f"N={N} mhsa bwd_kb p={p}: {us:7.1f} us  {2 * fl / us / 1e6:6.1f} TF/s", flush=True)
        rows = L.lib().hvit_mhsa_bias_rows(L.BF16, B, N, H, hd)
        parts = torch.empty(rows, 3 * D, device="cuda")
        bwdb = lambda: L.call("hvit_mhsa_bwd_db", L.BF16, qkv.data_ptr(), o.data_ptr(), do.data_ptr(),  # noqa
                              lse.data_ptr(), B, N, H, hd, hd ** -0.5, dr, kb.data_ptr(), dqkv.data_ptr(),
                              delta.data_ptr(), parts.data_ptr(), st())
        us = timeit(bwdb)
        print(f"N={N} mhsa bwd_kb+bias p={p}: {us:7.1f} us  {2 * fl / us / 1e6:6.1f} TF/s", flush=True)


def fp8_main(p=0.1, N=256):
    """config 5's attention (B=16, N=256, H=12, hd=64; N < 256: the partial-tile forms): the bf16 forward against
    the fp8 forms (hvit_gemm_tune(L.TUNE_FP8_FWD, form): 0 round-4 kernel, 1 v2 16 waves,
    2 v2 8 waves), keep-bit entry points (the training path)."""
    B, H, hd = 16, 12, 64
    D = H * hd
    qkv = (torch.randn(B * N, 3 * D, device="cuda") * 0.7).to(torch.bfloat16)
    o = torch.empty(B * N, D, device="cuda", dtype=torch.bfloat16)
    lse = torch.empty(B, H, N, device="cuda")
    dr = L.dropout(p, 1, 2)
    kb = torch.empty(L.lib().hvit_mhsa_keep_bits_elems(B, N, H), dtype=torch.int32, device="cuda")
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    fl = 4 * B * H * N * N * hd
    fb = lambda: L.call("hvit_mhsa_fwd_kb", L.BF16, qkv.data_ptr(), B, N, H, hd, hd ** -0.5, dr,  # noqa
                        o.data_ptr(), lse.data_ptr(), kb.data_ptr(), st())
    us = timeit(fb)
    print(f"N={N} config5 bf16 fwd_kb p={p}: {us:7.1f} us  {fl / us / 1e6:6.1f} TF/s", flush=True)
    f8 = lambda: L.call("hvit_mhsa_fwd_fp8_kb", qkv.data_ptr(), B, N, H, hd, hd ** -0.5, dr,  # noqa
                        o.data_ptr(), lse.data_ptr(), kb.data_ptr(), st())
    old = L.lib().hvit_gemm_tune(L.TUNE_FP8_FWD, 1)
    try:
        for form in (0, 1, 2):
            L.lib().hvit_gemm_tune(L.TUNE_FP8_FWD, form)
            us = timeit(f8)
            print(f"N={N} config5 fp8 form {form} fwd_kb p={p}: {us:7.1f} us  {fl / us / 1e6:6.1f} TF/s", flush=True)
    finally:
        L.lib().hvit_gemm_tune(L.TUNE_FP8_FWD, old)


if __name__ == "__main__":
    n = int(sys.argv[sys.argv.index("--tokens") + 1]) if "--tokens" in sys.argv else 256
    if "--fp8" in sys.argv:
        fp8_main(0.1, n)
        fp8_main(0.0, n)
    else:
        main(0.1, n)
        main(0.0, n)
