"""sha256 of every attention entry point's outputs over the shapes that reach
each kernel branch: one line per case and output tensor.  Run once per library
(HVIT_LIB selects an in-tree build) and diff the listings: a refactor of the
attention kernels must leave the diff empty.  Inputs come from a seeded CPU
generator, so two processes see the same bytes."""

import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hvit_amd_loader  # noqa: E402

hv = hvit_amd_loader.load()
L = hv._lib
DEV = "cuda"


def st():
    return torch.cuda.current_stream().cuda_stream


def emit(case, **tensors):
    torch.cuda.synchronize()
    for name, t in tensors.items():
        h = hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
        print(f"{case} {name} {h}", flush=True)


def inputs(dt, B, N, H, hd, seed):
    g = torch.Generator().manual_seed(seed)
    tdt = torch.bfloat16 if dt == L.BF16 else torch.float32
    D = H * hd
    qkv = (torch.randn(B * N, 3 * D, generator=g) * 0.7).to(tdt).to(DEV)
    go = torch.randn(B * N, D, generator=g).to(tdt).to(DEV)
    return qkv, go


def run(tag, dt, B, N, H, hd, p, probs=False):
    """fwd + bwd, fwd_kb + bwd_kb, bwd_db with and without keep bits"""
    lib = L.lib()
    D = H * hd
    qkv, go = inputs(dt, B, N, H, hd, 1000 * hd + N)
    dr = L.dropout(p, 77, 23) if p > 0 else None
    sc = hd ** -0.5
    new = lambda *s: torch.zeros(*s, device=DEV, dtype=qkv.dtype)  # noqa: E731
    o, lse, dq, delta = new(B * N, D), torch.zeros(B, H, N, device=DEV), new(B * N, 3 * D), torch.zeros(B, H, N,
                                                                                                         device=DEV)
    pr = torch.zeros(B, H, N, N, device=DEV) if probs else None
    L.call("hvit_mhsa_fwd", dt, qkv.data_ptr(), B, N, H, hd, sc, dr, o.data_ptr(), lse.data_ptr(),
           pr.data_ptr() if probs else None, st())
    L.call("hvit_mhsa_bwd", dt, qkv.data_ptr(), o.data_ptr(), go.data_ptr(), lse.data_ptr(), B, N, H, hd, sc, dr,
           dq.data_ptr(), delta.data_ptr(), st())
    emit(tag + " fwd+bwd", o=o, lse=lse, dqkv=dq, delta=delta, **({"probs": pr} if probs else {}))
    if probs:
        return
    kb = torch.zeros(max(1, lib.hvit_mhsa_keep_bits_elems(B, N, H)), dtype=torch.int32, device=DEV)
    o2, lse2, dq2, delta2 = torch.zeros_like(o), torch.zeros_like(lse), torch.zeros_like(dq), torch.zeros_like(delta)
    L.call("hvit_mhsa_fwd_kb", dt, qkv.data_ptr(), B, N, H, hd, sc, dr, o2.data_ptr(), lse2.data_ptr(), kb.data_ptr(),
           st())
    L.call("hvit_mhsa_bwd_kb", dt, qkv.data_ptr(), o2.data_ptr(), go.data_ptr(), lse2.data_ptr(), B, N, H, hd, sc, dr,
           kb.data_ptr(), dq2.data_ptr(), delta2.data_ptr(), st())
    emit(tag + " fwd_kb+bwd_kb", o=o2, lse=lse2, bits=kb, dqkv=dq2, delta=delta2)
    for with_kb in (False, True):
        rows = lib.hvit_mhsa_bias_rows(dt, B, N, H, hd)
        parts = torch.zeros(rows, 3 * D, device=DEV)
        dq3, delta3 = torch.zeros_like(dq), torch.zeros_like(delta)
        L.call("hvit_mhsa_bwd_db", dt, qkv.data_ptr(), o2.data_ptr(), go.data_ptr(), lse2.data_ptr(), B, N, H, hd, sc,
               dr, kb.data_ptr() if with_kb else None, dq3.data_ptr(), delta3.data_ptr(), parts.data_ptr(), st())
        emit(tag + f" bwd_db kb={int(with_kb)}", dqkv=dq3, delta=delta3, bias_rows=parts)


def run_fp8(B, N, H, p):
    lib = L.lib()
    hd, D = 64, H * 64
    qkv, _ = inputs(L.BF16, B, N, H, hd, 8000 + N)
    dr = L.dropout(p, 77, 23) if p > 0 else None
    old = lib.hvit_gemm_tune(L.TUNE_FP8_FWD, 1)
    try:
        for form in (0, 1, 2):
            lib.hvit_gemm_tune(L.TUNE_FP8_FWD, form)
            for with_kb in (False, True):
                o = torch.zeros(B * N, D, device=DEV, dtype=torch.bfloat16)
                lse = torch.zeros(B, H, N, device=DEV)
                kb = torch.zeros(lib.hvit_mhsa_keep_bits_elems(B, N, H), dtype=torch.int32, device=DEV)
                L.call("hvit_mhsa_fwd_fp8_kb", qkv.data_ptr(), B, N, H, hd, hd ** -0.5, dr, o.data_ptr(),
                       lse.data_ptr(), kb.data_ptr() if with_kb else None, st())
                emit(f"fp8 N={N} p={p} form={form} kb={int(with_kb)}", o=o, lse=lse, bits=kb)
    finally:
        lib.hvit_gemm_tune(L.TUNE_FP8_FWD, old)


def main():
    lib = L.lib()
    B, H = 2, 2
    for N in (16, 36, 100, 228, 240, 256, 300, 496, 512):
        for p in (0.0, 0.3):
            for fused in ((0, 1) if N <= 256 else (1,)):  # hvit_gemm_tune(L.TUNE_ATTN_BWD, .): kernel pair / single pass
                old = lib.hvit_gemm_tune(L.TUNE_ATTN_BWD, fused)
                try:
                    run(f"bf16 hd=64 N={N} p={p} tune4={fused}", L.BF16, B, N, H, 64, p)
                finally:
                    lib.hvit_gemm_tune(L.TUNE_ATTN_BWD, old)
    # the generic kernels
    for p in (0.0, 0.3):
        run(f"generic bf16 hd=64 N=520 p={p}", L.BF16, B, 520, H, 64, p)
        for dt, name in ((L.BF16, "bf16"), (L.F32, "f32")):
            run(f"generic {name} hd=64 N=30 p={p}", dt, B, 30, H, 64, p)
            for hd in (16, 32):
                for probs in (False, True):
                    run(f"generic {name} hd={hd} N=16 p={p} probs={int(probs)}", dt, B, 16, H, hd, p, probs)
    for N in (100, 240, 256):
        for p in (0.0, 0.3):
            run_fp8(B, N, H, p)


if __name__ == "__main__":
    main()
