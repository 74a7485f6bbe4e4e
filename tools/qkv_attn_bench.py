"""In-process A/B of the qkv Linear + attention forward: hvit_linear_fwd, hvit_mhsa_fwd_kb, the two back to
back, and the fused hvit_qkv_mhsa_fwd with and without a kept qkv (csrc/qkv_attention.hip), at the default
(B=32, 8 heads) and the large (B=16, 12 heads) shapes, with and without attention dropout.  HIP events
around 200 launches, four interleaved rounds (profiles/r12_qkv_attn_fused.txt).

    python tools/qkv_attn_bench.py
"""
import sys, os
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hvit_amd_loader
hv = hvit_amd_loader.load()
l = hv._lib
DEV = "cuda"
N, HD = 256, 64

def s():
    return torch.cuda.current_stream().cuda_stream

def timeit(fn, iters=200):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters

for B, H in ((32, 8), (16, 12)):
    D = H * HD
    x = torch.randn(B * N, D, device=DEV).to(torch.bfloat16)
    w = (torch.randn(3 * D, D, device=DEV) * D ** -0.5).to(torch.bfloat16)
    b = torch.randn(3 * D, device=DEV) * 0.1
    qkv = torch.empty(B * N, 3 * D, device=DEV, dtype=torch.bfloat16)
    o = torch.empty(B * N, D, device=DEV, dtype=torch.bfloat16)
    lse = torch.empty(B, H, N, device=DEV)
    kb = torch.zeros(l.lib().hvit_mhsa_keep_bits_elems(B, N, H), dtype=torch.int32, device=DEV)
    for p in (0.1, 0.0):
        dr = l.dropout(p, 4242, 17)
        kbp = kb.data_ptr() if p > 0 else None
        lin = lambda: l.call("hvit_linear_fwd", l.BF16, x.data_ptr(), w.data_ptr(), b.data_ptr(), B * N, 3 * D, D, qkv.data_ptr(), l.BF16, None, s())
        att = lambda: l.call("hvit_mhsa_fwd_kb", l.BF16, qkv.data_ptr(), B, N, H, HD, HD ** -0.5, dr, o.data_ptr(), lse.data_ptr(), kbp, s())
        two = lambda: (lin(), att())
        fus = lambda: l.call("hvit_qkv_mhsa_fwd", l.BF16, x.data_ptr(), w.data_ptr(), b.data_ptr(), B, N, H, HD, HD ** -0.5, dr, qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), kbp, s())
        fnq = lambda: l.call("hvit_qkv_mhsa_fwd", l.BF16, x.data_ptr(), w.data_ptr(), b.data_ptr(), B, N, H, HD, HD ** -0.5, dr, None, o.data_ptr(), lse.data_ptr(), kbp, s())
        for rnd in range(4):
            print(f"B={B} H={H} p={p} round {rnd}: linear {timeit(lin):6.2f}  attn {timeit(att):6.2f}  two {timeit(two):6.2f}  fused {timeit(fus):6.2f}  fused(no qkv) {timeit(fnq):6.2f} us", flush=True)
