"""sha256 of the outputs of every entry point whose kernels use csrc/chan_vec.h
or csrc/bn_tail.h (the BN/ReLU/Dropout2d/pool tail, the fused first block, the
thin convs, the resize kernels, the LayerNorm backward), over the shapes that
reach each kernel branch: one line per case and output tensor.  Run once per
library (HVIT_LIB selects an in-tree build) and diff the listings: a refactor
of those kernels must leave the diff empty.  Inputs come from a seeded CPU
generator, so two processes see the same bytes; outputs start as zeros."""

import ctypes
import hashlib
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hvit_amd_loader  # noqa: E402

hv = hvit_amd_loader.load()
L = hv._lib
HF = importlib.import_module(hv.__name__ + ".functional")
DEV = "cuda"
DTS = (("f32", L.F32, torch.float32), ("bf16", L.BF16, torch.bfloat16))
TD = {L.F32: torch.float32, L.BF16: torch.bfloat16}
NAME = {L.F32: "f32", L.BF16: "bf16"}

BN_SHAPES = [(2, 32, 32, 64, 2, 0.0), (3, 15, 17, 16, 2, 0.3), (2, 16, 16, 256, 1, 0.1), (1, 8, 8, 8, 1, 0.0)]
C1_CASES = [(2, 32, 32, 64, 2, 0.0), (3, 15, 17, 16, 2, 0.3), (2, 16, 24, 128, 1, 0.1), (1, 9, 8, 8, 2, 0.5),
            (2, 64, 251, 64, 2, 0.1), (2, 40, 36, 32, 2, 0.2)]  # CASES of tests/test_gpu_c1block.py
THIN_CASES = [  # N, Hs, Ws, C1, U, Cout: the Cin = 1 and Cout = 1 rows of CONV_CASES in tests/test_gpu_kernels.py
    (2, 33, 47, 1, 1, 8), (3, 20, 256, 1, 1, 64), (2, 12, 10, 64, 1, 1), (2, 64, 64, 64, 1, 1), (3, 5, 7, 32, 1, 1),
    (1, 8, 6, 16, 2, 1)]


def st():
    return torch.cuda.current_stream().cuda_stream


def emit(case, **tensors):
    torch.cuda.synchronize()
    for name, t in tensors.items():
        h = hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
        print(f"{case} {name} {h}", flush=True)


def rnd(g, *shape, dt=torch.float32, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dt).to(DEV)


def zeros(*shape, dt=torch.float32):
    return torch.zeros(*shape, device=DEV, dtype=dt)


def affine(g, C):
    """mean, invstd, gamma, beta"""
    return (rnd(g, C, scale=0.1), (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.rand(C, generator=g) + 0.5).to(DEV),
            rnd(g, C, scale=0.3))


def bn_act():
    for N, H, W, C, pool, p in BN_SHAPES:
        for name, dtc, tdt in DTS:
            g = torch.Generator().manual_seed(N * 1000 + C + pool)
            z = rnd(g, N, H, W, C, dt=tdt)
            mean, inv, gamma, beta = affine(g, C)
            gy32 = rnd(g, N, H // pool, W // pool, C)
            word = torch.tensor([0x5151], dtype=torch.int64, device=DEV)
            for seed_t in (None, word):
                dr = L.dropout(p, 31, 9, seed_t)
                tag = f"bn_act {name} {N}x{H}x{W}x{C} pool={pool} p={p} word={int(seed_t is not None)}"
                for io in (L.F32, L.BF16):
                    y = zeros(N, H // pool, W // pool, C, dt=TD[io])
                    L.call("hvit_bn_act_fwd", dtc, z.data_ptr(), N, H, W, C, mean.data_ptr(), inv.data_ptr(),
                           gamma.data_ptr(), beta.data_ptr(), dr, pool, y.data_ptr(), io, st())
                    emit(f"{tag} fwd y_dt={NAME[io]}", y=y)
                    gy = gy32.to(TD[io])
                    for training in (0, 1):
                        dz = zeros(N, H, W, C, dt=tdt)
                        sums = zeros(L.lib().hvit_bn_act_bwd_sums_elems(C))
                        L.call("hvit_bn_act_bwd", dtc, z.data_ptr(), N, H, W, C, mean.data_ptr(), inv.data_ptr(),
                               gamma.data_ptr(), beta.data_ptr(), dr, pool, gy.data_ptr(), io, training, dz.data_ptr(),
                               dtc, sums.data_ptr(), 0, st())
                        emit(f"{tag} bwd dy_dt={NAME[io]} training={training}", dz=dz, sums=sums)


def c1block():
    lib = L.lib()
    for N, H, W, C, pool, p in C1_CASES:
        for name, dtc, tdt, knob in (("f32", L.F32, torch.float32, 1), ("bf16 mfma", L.BF16, torch.bfloat16, 1),
                                     ("bf16 valu", L.BF16, torch.bfloat16, 0)):
            old = lib.hvit_gemm_tune(1, knob)
            try:
                g = torch.Generator().manual_seed(N * 100 + C + W)
                x = rnd(g, N, H, W, 1, dt=tdt)
                w = rnd(g, C, 1, 3, 3, scale=1 / 3)
                wp = HF.pack_conv(w, 0, dtc)
                mean, inv, gamma, beta = affine(g, C)
                gy32 = rnd(g, N, H // pool, W // pool, C)
                geo = HF.geom(x, 1, None, 0, N, H, W, 1, 3, 1, 1, C)
                tag = f"c1block {name} {N}x{H}x{W}x{C} pool={pool} p={p}"
                tr = lib.hvit_conv_bn_tile_rows(ctypes.byref(geo))
                part = zeros((N * H * W + tr - 1) // tr, C, 2)
                L.call("hvit_c1block_stats", dtc, geo, wp.data_ptr(), part.data_ptr(), st())
                emit(f"{tag} stats", part=part)
                for training in (0, 1):
                    dr = L.dropout(p, 1234, 100) if training else None
                    for io in (L.F32, L.BF16):
                        y = zeros(N, H // pool, W // pool, C, dt=TD[io])
                        L.call("hvit_c1block_fwd", dtc, geo, wp.data_ptr(), mean.data_ptr(), inv.data_ptr(),
                               gamma.data_ptr(), beta.data_ptr(), dr, pool, y.data_ptr(), io, st())
                        gy = gy32.to(TD[io])
                        sums, dw = zeros(2 * C), zeros(C * 9)
                        ws_n = lib.hvit_c1block_bwd_ws(ctypes.byref(geo), pool)
                        ws = zeros(max(ws_n, 1))
                        L.call("hvit_c1block_bwd", dtc, geo, wp.data_ptr(), mean.data_ptr(), inv.data_ptr(),
                               gamma.data_ptr(), beta.data_ptr(), dr, pool, gy.data_ptr(), io, training,
                               sums.data_ptr(), 0, dw.data_ptr(), ws.data_ptr(), ws_n, st())
                        emit(f"{tag} training={training} io={NAME[io]}", y=y, sums=sums, dw=dw)
            finally:
                lib.hvit_gemm_tune(1, old)


def thin_convs():
    lib = L.lib()
    for N, Hs, Ws, C1, U, Cout in THIN_CASES:
        for name, dtc, tdt in DTS:
            g = torch.Generator().manual_seed(N * 1000 + Hs * Ws + C1 + Cout)
            H, W = Hs * U, Ws * U
            x = rnd(g, N, Hs, Ws, C1, dt=tdt)
            w = rnd(g, Cout, C1, 3, 3, scale=(C1 * 9) ** -0.5)
            dz = rnd(g, N, H, W, Cout, dt=tdt)
            geo = HF.geom(x, C1, None, 0, N, Hs, Ws, U, 3, 1, 1, Cout)
            wp, wd = HF.pack_conv(w, 0, dtc), HF.pack_conv(w, 1, dtc)
            tag = f"thinconv {name} {N}x{Hs}x{Ws} Cin={C1} U={U} Cout={Cout}"
            tr = lib.hvit_conv_bn_tile_rows(ctypes.byref(geo))
            for zdt in dict.fromkeys((L.F32, dtc)):
                z = zeros(N, H, W, Cout, dt=TD[zdt])
                part = zeros((N * H * W + tr - 1) // tr, Cout, 2)
                L.call("hvit_conv_fwd", dtc, geo, wp.data_ptr(), None, z.data_ptr(), zdt, part.data_ptr(), None, st())
                emit(f"{tag} fwd z_dt={NAME[zdt]}", z=z, part=part)
            ws_n = lib.hvit_conv_wgrad_workspace(geo)
            ws, dwp = zeros(max(ws_n, 1)), zeros(w.numel())
            L.call("hvit_conv_wgrad", dtc, geo, dz.data_ptr(), dwp.data_ptr(), ws.data_ptr(), ws_n, st())
            du = zeros(N, H, W, C1, dt=tdt)
            L.call("hvit_conv_dgrad", dtc, geo, dz.data_ptr(), wd.data_ptr(), du.data_ptr(), dtc, st())
            emit(f"{tag} bwd", dw=dwp, du=du)


def resample():
    # N, Hi, Wi, C, Ho, Wo (x [N, Hi, Wi, C] <-> y [N, Ho, Wo, C]), dtype, the backward's branch
    cases = [(2, 16, 23, 8, 4, 4, L.BF16, "rows bf16"), (3, 30, 20, 1, 100, 77, L.F32, "rows f32 C=1"),
             (2, 10, 14, 8, 5, 7, L.BF16, "down kd=2"), (2, 12, 20, 16, 3, 5, L.BF16, "down kd=4"),
             (2, 16, 23, 8, 4, 4, L.F32, "vec f32"), (1, 8, 8, 8, 40, 44, L.BF16, "vec bf16"),
             (1, 8, 8, 3, 33, 47, L.F32, "scalar")]
    for N, Hi, Wi, C, Ho, Wo, dtc, what in cases:
        g = torch.Generator().manual_seed(Hi * Wi + C + Ho)
        x = rnd(g, N, Hi, Wi, C, dt=TD[dtc])
        gy = rnd(g, N, Ho, Wo, C, dt=TD[dtc])
        tag = f"bilinear {what} {N}x{Hi}x{Wi}x{C}->{Ho}x{Wo}"
        y = zeros(N, Ho, Wo, C, dt=TD[dtc])
        L.call("hvit_bilinear_fwd", x.data_ptr(), dtc, N, Hi, Wi, C, Ho, Wo, y.data_ptr(), dtc, st())
        emit(f"{tag} fwd", y=y)
        for acc in (0, 1):
            dx = x.clone() if acc else zeros(N, Hi, Wi, C, dt=TD[dtc])
            L.call("hvit_bilinear_bwd", gy.data_ptr(), dtc, N, Ho, Wo, C, Hi, Wi, dx.data_ptr(), dtc, acc, st())
            emit(f"{tag} bwd accumulate={acc}", dx=dx)
    for N, H, W, U, C1, C2 in ((3, 7, 9, 3, 8, 24), (2, 32, 32, 2, 256, 0)):
        g = torch.Generator().manual_seed(N * H + C1)
        du = rnd(g, N, H * U, W * U, C1 + C2, dt=torch.bfloat16)
        for odt, what in ((L.BF16, "vec"), (L.F32, "scalar")):
            dx1, dx2 = zeros(N, H, W, C1, dt=TD[odt]), zeros(N, H, W, max(C2, 1), dt=TD[odt])
            L.call("hvit_upsample_split_bwd", du.data_ptr(), L.BF16, N, H, W, U, C1, C2, dx1.data_ptr(), odt,
                   dx2.data_ptr() if C2 else None, odt, st())
            emit(f"upsample_split_bwd {what} {N}x{H}x{W} U={U} C={C1}+{C2}", dx1=dx1, dx2=dx2)


def layernorm_bwd():
    lib = L.lib()
    for M, D, p, rps in ((300, 512, 0.1, 100), (37, 64, 0.3, 5), (16, 768, 0.0, 4)):
        g = torch.Generator().manual_seed(M + D)
        x = rnd(g, M, D, scale=2.0) + 0.5
        gam = (torch.rand(D, generator=g) + 0.5).to(DEV)
        mean, rstd = x.mean(1), (x.var(1, unbiased=False) + 1e-5).rsqrt()
        dy32, resid = rnd(g, M, D), rnd(g, M, D)
        rs = (torch.rand((M + rps - 1) // rps, generator=g) + 0.5).to(DEV)
        for dy_dt in (L.F32, L.BF16):
            dy = dy32.to(TD[dy_dt])
            tag = f"layernorm_bwd M={M} D={D} dy={NAME[dy_dt]}"
            ws_n = lib.hvit_layernorm_bwd_ws_elems(M, D)
            ws, dx, acc = zeros(max(ws_n, 1)), zeros(M, D), zeros(2 * D)
            L.call("hvit_layernorm_bwd", dy.data_ptr(), dy_dt, x.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                   gam.data_ptr(), M, D, resid.data_ptr(), dx.data_ptr(), acc.data_ptr(), acc[D:].data_ptr(),
                   ws.data_ptr(), ws_n, L.ACC_ZEROED, st())
            emit(f"{tag} slab", dx=dx, dgamma_dbeta=acc)
            for gdt in (L.F32, L.BF16):
                ws_n = lib.hvit_layernorm_bwd_drop_ws_elems(M, D)
                ws, dx, acc, gg = zeros(max(ws_n, 1)), zeros(M, D), zeros(3 * D), zeros(M, D, dt=TD[gdt])
                L.call("hvit_layernorm_bwd_drop", dy.data_ptr(), dy_dt, x.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                       gam.data_ptr(), M, D, resid.data_ptr(), dx.data_ptr(), acc.data_ptr(), L.dropout(p, 77, 9),
                       rs.data_ptr(), rps, gg.data_ptr(), gdt, ws.data_ptr(), ws_n, L.ACC_ZEROED, st())
                emit(f"{tag} drop p={p} g={NAME[gdt]}", dx=dx, g=gg, sums=acc)


def main():
    bn_act()
    c1block()
    thin_convs()
    resample()
    layernorm_bwd()


if __name__ == "__main__":
    main()
