"""GPU: the halo-resident A operand of the bf16 3x3 conv forward and data-gradient
GEMMs (csrc/gemm_conv_halo.h; hvit_gemm_tune(9, v): 0 per-tap im2col, 1 halo
where measured faster, 2 wherever it applies).

* bitwise against the per-tap path: z (bf16 and f32), the BatchNorm partials,
  hvit_bn_finalize's mean / invstd, and du of hvit_conv_dgrad, at the real
  widths and channel counts.  The halo geometry depends on W and C, not on N,
  but the tile's column count follows the per-tap path's tile choice, which
  depends on the row count M: the small batches run the 64-column kernels (and,
  under the default setting, the per-tap path: their grids are below the
  measured sizes), the larger ones the 128-column kernels with their 8-row
  statistics merge, and the default setting takes the halo path there;
* element-wise against torch fp32 with the bounds of test_gpu_bf16_exact.py
  (ACC = 2e-5 of the largest reference value; half a bf16 ulp for bf16 outputs),
  the conv input carved out of a NaN-filled allocation so that a halo read that
  should have been a zero shows;
* shapes the predicate must refuse stay within the same bounds with the switch on.
The launch counter (hvit_gemm_tune(10, 0)) tells which path ran.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ACC = 2e-5

# ((N, H, W, Cin, Cout), halo launches expected under the default setting)
FWD = [((1, 128, 128, 64, 128), 0), ((1, 64, 64, 128, 256), 0),
       # 128x128 tiles on the per-tap path, 256 workgroups of the halo kernel: the default takes the halo
       ((4, 128, 128, 64, 128), 1), ((8, 64, 64, 128, 256), 1)]
# N, H, W, Cin (columns of du), Cout (channels of dy, the A operand)
DGRAD = [((2, 128, 128, 64, 128), 0), ((2, 64, 64, 128, 256), 0), ((2, 64, 64, 192, 64), 0),
         ((2, 32, 32, 384, 128), 0), ((2, 16, 16, 512, 256), 0), ((3, 16, 16, 512, 256), 0),
         # the dec1 class on 128 columns and the dec2 class on 64, at grids the default sends to the halo
         ((32, 32, 32, 384, 128), 1), ((8, 64, 64, 192, 64), 1)]


@pytest.fixture(scope="module")
def env(hv):
    import sys

    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    HF = sys.modules["hvit_amd.functional"]
    old = hv._lib.lib().hvit_gemm_tune(9, 1)
    yield hv._lib, HF
    hv._lib.lib().hvit_gemm_tune(9, old)


def s():
    return torch.cuda.current_stream().cuda_stream


def check_f32(out, ref, what=""):
    out, ref = out.double(), ref.double()
    bound = ACC * ref.abs().max().item() + 1e-30
    d = (out - ref).abs()
    n = int((~(d <= bound)).sum())  # NaN counts as off
    assert n == 0, f"{what}: {n} of {ref.numel()} elements off (max |d| {d.max().item():.3e}, bound {bound:.3e})"


def check_bf16(out, ref, what=""):
    out, ref = out.double(), ref.double()
    bound = ref.abs() * 2.0 ** -8 + ACC * ref.abs().max().item() + 1e-30
    n = int((~((out - ref).abs() <= bound)).sum())
    assert n == 0, f"{what}: {n} of {ref.numel()} elements beyond half a bf16 ulp"


def in_nan(shape, seed):
    """A bf16 tensor of random values inside a larger NaN-filled allocation."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    n = 1
    for d in shape:
        n *= d
    pad = 1 << 16
    big = torch.full((n + 2 * pad,), float("nan"), device=DEV, dtype=BF)
    x = big[pad:pad + n].view(*shape)
    x.copy_(torch.randn(*shape, device=DEV, generator=g).to(BF))
    return x


@functools.lru_cache(maxsize=None)
def fwd_case(case):
    N, H, W, Cin, Cout = case
    x = in_nan((N, H, W, Cin), 11)
    g = torch.Generator(device=DEV).manual_seed(12)
    w = torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) / (Cin * 9) ** 0.5
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), w.to(BF).float(), None, 1, 1).permute(0, 2, 3, 1).contiguous()
    return x, w, ref


@functools.lru_cache(maxsize=None)
def dgrad_case(case):
    N, H, W, Cin, Cout = case
    dz = in_nan((N, H, W, Cout), 21)
    g = torch.Generator(device=DEV).manual_seed(22)
    w = torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) / (Cout * 9) ** 0.5
    ref = F.conv_transpose2d(dz.float().permute(0, 3, 1, 2), w.to(BF).float(), None, 1, 1)
    return dz, w, ref.permute(0, 2, 3, 1).contiguous()


def run_fwd(L, HF, case, mode, out_dt, x=None, x2=None, C2=0, U=1, dt=None):
    """(z, partials, mean, invstd, halo launches) of hvit_conv_fwd under tune 9 = mode."""
    N, H, W, Cin, Cout = case
    if x is None:
        x, w, _ = fwd_case(case)
    else:
        w = x[1]
        x = x[0]
    dt = L.BF16 if dt is None else dt
    lib = L.lib()
    lib.hvit_gemm_tune(9, mode)
    c0 = lib.hvit_gemm_tune(10, 0)
    Ho, Wo = H * U, W * U
    g = HF.geom(x, Cin - C2, x2, C2, N, H, W, U, 3, 1, 1, Cout)
    wp = HF.pack_conv(w, 0, dt)
    z = torch.empty(N, Ho, Wo, Cout, device=DEV, dtype=BF if out_dt == L.BF16 else torch.float32)
    tr = lib.hvit_conv_bn_tile_rows(g)
    P = N * Ho * Wo
    nt = (P + tr - 1) // tr
    part = torch.zeros(nt, Cout, 2, device=DEV)
    L.call("hvit_conv_fwd", dt, g, wp.data_ptr(), None, z.data_ptr(), out_dt, part.data_ptr(), None, s())
    keep = part.clone()
    mean, inv = torch.empty(Cout, device=DEV), torch.empty(Cout, device=DEV)
    L.call("hvit_bn_finalize", part.data_ptr(), nt, tr, P, Cout, mean.data_ptr(), inv.data_ptr(), None, None, None,
           0.1, 1e-5, s())
    torch.cuda.synchronize()
    return z, keep, mean, inv, lib.hvit_gemm_tune(10, 0) - c0


def run_dgrad(L, HF, case, mode, out_dt, dt=None, ops=None):
    N, H, W, Cin, Cout = case
    dz, w, _ = ops if ops is not None else dgrad_case(case)
    dt = L.BF16 if dt is None else dt
    lib = L.lib()
    lib.hvit_gemm_tune(9, mode)
    c0 = lib.hvit_gemm_tune(10, 0)
    g = HF.geom(dz, Cin, None, 0, N, H, W, 1, 3, 1, 1, Cout)  # src1 is not read by the data gradient
    wd = HF.pack_conv(w, 1, dt)
    du = torch.empty(N, H, W, Cin, device=DEV, dtype=BF if out_dt == L.BF16 else torch.float32)
    L.call("hvit_conv_dgrad", dt, g, dz.data_ptr(), wd.data_ptr(), du.data_ptr(), out_dt, s())
    torch.cuda.synchronize()
    return du, lib.hvit_gemm_tune(10, 0) - c0


@pytest.mark.parametrize("case,dflt", FWD)
def test_fwd_bitwise_and_exact(env, case, dflt):
    L, HF = env
    _, _, ref = fwd_case(case)
    for out_dt in (L.BF16, L.F32):
        z0, p0, m0, i0, n0 = run_fwd(L, HF, case, 0, out_dt)
        z1, p1, m1, i1, n1 = run_fwd(L, HF, case, 2, out_dt)
        assert n0 == 0 and n1 == 1, "the switch did not select the paths"
        assert torch.equal(z0, z1), "z differs between the per-tap and the halo path"
        assert torch.equal(p0, p1), "BatchNorm partials differ"
        assert torch.equal(m0, m1) and torch.equal(i0, i1), "hvit_bn_finalize results differ"
        (check_bf16 if out_dt == L.BF16 else check_f32)(z1, ref, what=f"halo conv fwd {case}")
        # the default setting: the expected path, the same bits
        zd, pd, md, idv, nd = run_fwd(L, HF, case, 1, out_dt)
        assert nd == dflt, "the default setting took the other path"
        assert torch.equal(zd, z0) and torch.equal(pd, p0) and torch.equal(md, m0) and torch.equal(idv, i0)


@pytest.mark.parametrize("case,dflt", DGRAD)
def test_dgrad_bitwise_and_exact(env, case, dflt):
    L, HF = env
    _, _, ref = dgrad_case(case)
    for out_dt in (L.BF16, L.F32):
        d0, n0 = run_dgrad(L, HF, case, 0, out_dt)
        d1, n1 = run_dgrad(L, HF, case, 2, out_dt)
        assert n0 == 0 and n1 == 1, "the switch did not select the paths"
        assert torch.equal(d0, d1), "du differs between the per-tap and the halo path"
        (check_bf16 if out_dt == L.BF16 else check_f32)(d1, ref, what=f"halo conv dgrad {case}")
        dd, nd = run_dgrad(L, HF, case, 1, out_dt)
        assert nd == dflt, "the default setting took the other path"
        assert torch.equal(dd, d0)


# shapes the predicate must refuse: N, H, W, Cin, Cout
REFUSED = [(2, 96, 96, 64, 64), (4, 40, 24, 64, 128), (6, 8, 8, 256, 256)]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("case", REFUSED)
def test_refused_geometries_stay_exact(env, case, mode):
    """W = 96 and a 40 x 24 map (neither whole rows nor a row segment), an 8 x 8 map (a tile would span images)."""
    L, HF = env
    N, H, W, Cin, Cout = case
    x, w, ref = fwd_case(case)
    z, _, _, _, n = run_fwd(L, HF, case, mode, L.F32)
    assert n == 0
    check_f32(z, ref, what=f"conv fwd {case}")
    dz, wd, dref = dgrad_case(case)
    du, n = run_dgrad(L, HF, case, mode, L.F32)
    assert n == 0
    check_f32(du, dref, what=f"conv dgrad {case}")


@pytest.mark.parametrize("mode", [1, 2])
def test_refused_two_source_upsampled_forward(env, mode):
    """The decoder forward (two sources, x2 upsample) keeps the per-tap loader."""
    L, HF = env
    N, Hs, Ws, C1, C2, Cout = 2, 32, 32, 128, 64, 64
    x1, x2 = in_nan((N, Hs, Ws, C1), 31), in_nan((N, Hs, Ws, C2), 32)
    g = torch.Generator(device=DEV).manual_seed(33)
    w = torch.randn(Cout, C1 + C2, 3, 3, device=DEV, generator=g) / ((C1 + C2) * 9) ** 0.5
    xr = torch.cat([x1, x2], 3).float().permute(0, 3, 1, 2)
    ref = F.conv2d(F.interpolate(xr, scale_factor=2, mode="nearest"), w.to(BF).float(), None, 1, 1)
    z, _, _, _, n = run_fwd(L, HF, (N, Hs, Ws, C1 + C2, Cout), mode, L.F32, x=(x1, w), x2=x2, C2=C2, U=2)
    assert n == 0
    check_f32(z, ref.permute(0, 2, 3, 1), what="decoder conv fwd")


@pytest.mark.parametrize("mode", [1, 2])
def test_refused_f32(env, mode):
    L, HF = env
    case = (1, 64, 64, 64, 64)
    N, H, W, Cin, Cout = case
    g = torch.Generator(device=DEV).manual_seed(41)
    x = torch.randn(N, H, W, Cin, device=DEV, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) / (Cin * 9) ** 0.5
    # float64 on the host: the reference's own error is far below the bound
    ref = F.conv2d(x.cpu().double().permute(0, 3, 1, 2), w.cpu().double(), None, 1, 1).permute(0, 2, 3, 1).to(DEV)
    z, _, _, _, n = run_fwd(L, HF, case, mode, L.F32, x=(x, w), dt=L.F32)
    assert n == 0
    check_f32(z, ref, what="f32 conv fwd")
    dz = torch.randn(N, H, W, Cout, device=DEV, generator=g)
    dref = F.conv_transpose2d(dz.cpu().double().permute(0, 3, 1, 2), w.cpu().double(), None, 1, 1)
    dref = dref.permute(0, 2, 3, 1).to(DEV)
    du, n = run_dgrad(L, HF, case, mode, L.F32, dt=L.F32, ops=(dz, w, None))
    assert n == 0
    check_f32(du, dref, what="f32 conv dgrad")
