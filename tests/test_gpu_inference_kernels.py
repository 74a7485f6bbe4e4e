"""GPU: the inference-only fused kernels pinned element-wise against torch.

The eval + no_grad forward does not run the kernels the rest of the suite
pins: eval BatchNorm is folded into the conv weights (hvit_bn_eval_prep +
hvit_bn_fold, or hvit_weight_prep kind 3), the conv epilogue adds the folded
bias and applies the ReLU (ACT_RELU), a pooling block also keeps each 2x2
window's maximum there (ACT_RELU_POOL2, window-major row order), the final conv
applies tanh (ACT_TANH: two thin Cout = 1 kernels and the GEMM epilogue), and
fc1 stores gelu(h) only (ACT_GELU).  hvit_tanh_bwd is the final conv's first
backward step.

As in test_gpu_bf16_exact.py every kernel is fed operands already rounded to
its compute dtype, the reference is torch arithmetic on exactly those operands
(fp32, or fp64 where stated), and the checks are ELEMENT-WISE:

* f32 outputs:  |out - ref| <= ACC * max|ref|               (ACC = 2e-5)
* bf16 outputs: |out - ref| <= 2^-8 |ref| + ACC * max|ref|  (half a bf16 ulp)

with acc = 1e-4 where a GELU is involved (its approximation error is
<= 1.5e-7, test_gpu_bf16_exact.py).  Every output buffer is NaN-filled before
the call, so a row or element the kernel does not write fails the check.

Conv shapes are (N, Hs, Ws, C1, C2, U, Cout), sized against the tile rule of
launch_gemm (gemm.h, M = P = N * Hs*U * Ws*U output pixels, N = Cout):
128x64 when Cout <= 64 and cdiv(P, 128) >= 160; 128x128 when Cout > 64 and
cdiv(P, 128) * cdiv(Cout, 128) >= 160 (and the two 128x64 preferences above it
do not apply); 64x64 otherwise.  Loaders: general (LdConv: any channel count,
and every f32 conv), fast register (LdConvF: bf16, C1 % 64 == C2 % 64 == 0, a
ragged P or Cout), LDS-DMA (LdConvF with P and Cout multiples of the tile)."""

import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import keep_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ACC = 2e-5
NAN = float("nan")


@pytest.fixture(scope="module")
def env(hv):
    import sys

    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    HF = sys.modules["hvit_amd.functional"]
    yield hv._lib, HF
    hv._lib.lib().hvit_gemm_tune(0, -1)
    HF.prep_cache_clear()


def s():
    return torch.cuda.current_stream().cuda_stream


# test_gpu_bf16_exact.py's two checks, with the comparison turned round so that a
# NaN (an element the kernel left unwritten) counts as off instead of passing
def check_f32(out, ref, acc=ACC, what=""):
    out, ref = out.double(), ref.double()
    bound = acc * ref.abs().max().item() + 1e-30
    bad = ~((out - ref).abs() <= bound)  # (a NaN is off)
    n = int(bad.sum())
    assert n == 0, f"{what}: {n} of {ref.numel()} elements off (max |d| {(out - ref).abs().max().item():.3e}, " \
                   f"bound {bound:.3e})"


def check_bf16(out, ref, acc=ACC, what=""):
    out, ref = out.double(), ref.double()
    bound = ref.abs() * 2.0 ** -8 + acc * ref.abs().max().item() + 1e-30
    bad = ~((out - ref).abs() <= bound)  # (a NaN is off)
    n = int(bad.sum())
    assert n == 0, f"{what}: {n} of {ref.numel()} elements beyond half a bf16 ulp"


def tdt(L, dt):
    return torch.float32 if dt == L.F32 else BF


def nans(shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def dts(name):
    return 0 if name == "f32" else 1  # L.F32, L.BF16


# ------------------------------------------------------------------ BN fold ---
# the model's conv blocks (enc0 .. dec2), odd shapes (Cin / Cout no power of
# two, a 2x2 kernel) and one block above the LDS tile of hvit_weight_prep on
# either side (Cin * 9 or Cout * 9 > 40960 floats: the flat-gather form)
FOLD_SHAPES = [(64, 1, 3), (128, 64, 3), (256, 128, 3), (256, 512, 3), (128, 384, 3), (64, 192, 3), (24, 3, 3),
               (12, 20, 2), (8, 4608, 3), (4616, 6, 3)]
EPS = 1e-5


def bn_params(co, wide=True, gen=None):
    """gamma (both signs), beta, running mean, running variance (log-uniform
    over [1e-3, 10] with both ends present; ``wide`` False: [0.5, 2] and
    |gamma| in [0.5, 1.5], so every channel of a conv test weighs alike)."""
    r = lambda *sh: torch.rand(*sh, device=DEV, generator=gen)  # noqa: E731
    n = lambda *sh: torch.randn(*sh, device=DEV, generator=gen)  # noqa: E731
    if wide:
        gamma = n(co)
        rvar = 10.0 ** (r(co) * 4.0 - 3.0)
        rvar[0] = 1e-3
        rvar[-1] = 10.0
    else:
        gamma = (0.5 + r(co)) * torch.where(r(co) < 0.5, -1.0, 1.0)
        rvar = 2.0 ** (r(co) * 2.0 - 1.0)
    if co > 1:
        gamma[0], gamma[1] = gamma[0].abs() + 0.1, -gamma[1].abs() - 0.1
    return gamma.contiguous(), n(co), n(co), rvar.contiguous()


def fold_ref(w, gamma, beta, rmean, rvar):
    """fp64: the mode-0 packed [Cout][KS][KS][Cin] folded weight and the bias."""
    sc = gamma.double() * (rvar.double() + EPS).rsqrt()
    wf = (w.double() * sc[:, None, None, None]).permute(0, 2, 3, 1).reshape(-1)
    return wf, beta.double() - rmean.double() * sc


def bn_fold(L, w, bn, dt):
    """hvit_bn_eval_prep + hvit_bn_fold into NaN-filled buffers."""
    gamma, beta, rmean, rvar = bn
    co, ci, ks, _ = w.shape
    mean, invstd = nans((co,)), nans((co,))
    L.call("hvit_bn_eval_prep", rmean.data_ptr(), rvar.data_ptr(), co, EPS, mean.data_ptr(), invstd.data_ptr(), s())
    wf, bias = nans((w.numel(),), tdt(L, dt)), nans((co,))
    L.call("hvit_bn_fold", w.data_ptr(), co, ci, ks, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
           beta.data_ptr(), wf.data_ptr(), dt, bias.data_ptr(), s())
    return wf, bias, mean, invstd


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_bn_fold_and_weight_prep_kind3(env, dt):
    """hvit_bn_eval_prep + hvit_bn_fold, and hvit_weight_prep kind 3 (through
    functional.prep_weights: every shape as a kind-3 item plus kind-1 items in
    the same call; the LDS-tile form and, for the two shapes above the tile,
    the flat gather) against the fp64 fold: w * gamma * rsqrt(rvar + eps) per
    output channel in the mode-0 pack, bias = beta - rmean * gamma *
    rsqrt(rvar + eps).  f32 destinations and the bias at ACC, bf16
    destinations at half a bf16 ulp + ACC (the kernel rounds its f32 product
    once).

    Kind 3 is asserted BIT-IDENTICAL to hvit_bn_fold: both compute invstd =
    rsqrtf(rvar + eps) (bn_eval_prep_kernel / inline), sc = gamma * invstd,
    w * sc rounded once to the destination dtype, and bias = beta - mean *
    (gamma * invstd) -- the same f32 expressions in the same order in
    bn_fold_kernel, weight_pack_tiled_kernel and weight_pack_flat_kernel."""
    L, HF = env
    dtc = dts(dt)
    gen = torch.Generator(device=DEV).manual_seed(11)
    ws = [torch.randn(co, ci, k, k, device=DEV, generator=gen) for co, ci, k in FOLD_SHAPES]
    bns = [bn_params(w.shape[0], gen=gen) for w in ws]
    chk = check_f32 if dt == "f32" else check_bf16
    direct = []
    for w, bn in zip(ws, bns):
        wf, bias, mean, invstd = bn_fold(L, w, bn, dtc)
        what = f"bn_fold {tuple(w.shape)} {dt}"
        wr, br = fold_ref(w, *bn)
        assert torch.equal(mean, bn[2]), what
        check_f32(invstd, (bn[3].double() + EPS).rsqrt(), what=what + " invstd")
        chk(wf, wr, what=what + " weight")
        check_f32(bias, br, what=what + " bias")
        direct.append((wf, bias))
    # the multi-tensor launch: kind 3 for every shape, kind 1 for some of them
    # (a pooling block keeps both), all in one call
    plain = [ws[1], ws[6], ws[8]]
    items = [(w, 3, dtc, bn + (EPS,)) for w, bn in zip(ws, bns)] + [(w, 1, dtc) for w in plain]
    HF.prep_cache_clear()
    HF.prep_weights(items, torch.device(DEV))
    got3 = [HF._prep_get(w, 3, dtc) for w in ws]
    got1 = [HF._prep_get(w, 1, dtc).clone() for w in plain]
    HF.prep_cache_clear()
    # the same items straight through the C entry point into NaN-filled buffers
    # (prep_weights allocates its own): nothing is left unwritten
    arr = (L.WPrepItem * len(items))()
    raw = []
    for i, (w, bn) in enumerate(zip(ws, bns)):
        co, ci, ks, _ = w.shape
        out, bias = nans((w.numel(),), tdt(L, dtc)), nans((co,))
        raw.append((out, bias))
        arr[i] = L.WPrepItem(w.data_ptr(), out.data_ptr(), w.numel(), 3, dtc, co, ci, ks, bn[0].data_ptr(),
                             bn[1].data_ptr(), bn[2].data_ptr(), bn[3].data_ptr(), bias.data_ptr(), EPS)
    raw1 = []
    for i, w in enumerate(plain):
        co, ci, ks, _ = w.shape
        out = nans((w.numel(),), tdt(L, dtc))
        raw1.append(out)
        arr[len(ws) + i] = L.WPrepItem(w.data_ptr(), out.data_ptr(), w.numel(), 1, dtc, co, ci, ks)
    L.call("hvit_weight_prep", len(items), arr, s())
    torch.cuda.synchronize()
    for w, bn, (wf, bias), (w3, b3), (wn, bnn) in zip(ws, bns, direct, got3, raw):
        what = f"weight_prep kind 3 {tuple(w.shape)} {dt}"
        wr, br = fold_ref(w, *bn)
        chk(w3, wr, what=what + " weight")
        check_f32(b3, br, what=what + " bias")
        assert torch.equal(w3, wn) and torch.equal(b3, bnn), what + " (NaN-filled destination)"
        assert torch.equal(w3, wf) and torch.equal(b3, bias), what + " vs hvit_bn_fold"
    for w, g1, r1 in zip(plain, got1, raw1):
        ref = w.permute(0, 2, 3, 1).reshape(-1).to(tdt(L, dtc))
        assert torch.equal(g1, ref) and torch.equal(r1, ref), f"kind 1 next to kind 3 {tuple(w.shape)}"


# ------------------------------------------------------ conv + bias + ReLU ---
def conv_setup(L, HF, case, dt, seed):
    """Rounded NHWC inputs, the geometry, the kernel's own folded weights and
    bias (hvit_bn_fold), and relu(conv2d(x, unpacked folded weights) + bias) in
    fp32, NCHW: the test isolates the conv's loader and epilogue."""
    N, Hs, Ws, C1, C2, U, Cout = case
    gen = torch.Generator(device=DEV).manual_seed(seed)
    td = tdt(L, dt)
    x1 = torch.randn(N, Hs, Ws, C1, device=DEV, generator=gen).to(td)
    x2 = torch.randn(N, Hs, Ws, C2, device=DEV, generator=gen).to(td) if C2 else None
    Cin = C1 + C2
    w = torch.randn(Cout, Cin, 3, 3, device=DEV, generator=gen) / (Cin * 9) ** 0.5
    bn = bn_params(Cout, wide=False, gen=gen)
    wf, bias, _, _ = bn_fold(L, w, bn, dt)
    wu = wf.float().view(Cout, 3, 3, Cin).permute(0, 3, 1, 2).contiguous()
    xr = (torch.cat([x1, x2], 3) if C2 else x1).float().permute(0, 3, 1, 2).contiguous()
    xu = F.interpolate(xr, scale_factor=U, mode="nearest") if U > 1 else xr
    ref = F.relu(F.conv2d(xu, wu, bias, 1, 1))
    g = HF.geom(x1, C1, x2, C2, N, Hs, Ws, U, 3, 1, 1, Cout)
    return g, (x1, x2), wf, bias, ref


RELU_CASES = [
    # N, Hs, Ws, C1, C2, U, Cout
    (1, 9, 7, 32, 16, 2, 16),     # 64x64 tile, general loader (C % 64 != 0), x2 upsample + concat, P = 252 ragged
    (2, 33, 47, 8, 0, 1, 8),      # 64x64 tile, general loader, P = 3102 ragged, tiles spanning the two images
    (1, 9, 7, 64, 0, 1, 128),     # 64x64 tile, fast register loader (bf16), P = 63: one partial tile, C % 64 == 0
    (3, 9, 7, 64, 64, 1, 128),    # 64x64 tile, fast register loader, two sources, P = 189 ragged over three images
    (2, 8, 8, 128, 64, 2, 64),    # 64x64 tile, P = 512 full tiles, concat + x2 upsample: LDS-DMA (bf16)
    (5, 64, 64, 64, 0, 1, 128),   # 128x128 tile (cdiv(P, 128) = 160), full tiles: LDS-DMA (bf16)
    (5, 62, 66, 64, 0, 1, 128),   # 128x128 tile (cdiv(20460, 128) = 160), ragged P: fast register loader (bf16)
    (5, 64, 64, 64, 0, 1, 64),    # 128x64 tile (Cout <= 64, cdiv(P, 128) = 160), LDS-DMA (bf16)
    (5, 62, 66, 64, 0, 1, 64),    # 128x64 tile, ragged P: fast register loader (bf16)
    (1, 9, 7, 64, 0, 1, 6),       # Cout % 4 != 0: the general epilogue (EK_GEN), 64x64 tile, fast register loader
    (2, 5, 6, 24, 0, 1, 10),      # Cout % 4 != 0 with the general loader
]


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("case", RELU_CASES)
def test_conv_bias_relu(env, dt, case):
    """hvit_conv_fwd with ACT_RELU (eval BatchNorm folded: bias + ReLU in the
    epilogue), bf16 in -> bf16 out and f32 in -> f32 out, against
    relu(conv2d(x, wf) + bias) in fp32 on the folded weights the kernel itself
    produced.  The tile and loader each shape reaches are listed with
    RELU_CASES (the f32 runs take the same tiles with the general loader);
    Cout % 4 == 0 stores through EK_STORE, else through EK_GEN."""
    L, HF = env
    dtc = dts(dt)
    N, Hs, Ws, C1, C2, U, Cout = case
    g, keep, wf, bias, ref = conv_setup(L, HF, case, dtc, 21)
    y = nans((N, Hs * U, Ws * U, Cout), tdt(L, dtc))
    L.call("hvit_conv_fwd", dtc, g, wf.data_ptr(), bias.data_ptr(), y.data_ptr(), dtc, None,
           HF.epilogue(act=L.ACT_RELU), s())
    (check_f32 if dt == "f32" else check_bf16)(y.permute(0, 3, 1, 2), ref, what=f"conv + bias + relu {case} {dt}")


POOL_CASES = [
    # N, Hs, Ws, C1, C2, U, Cout: all bf16, fast loader in its window-major row order (LdConvF::pool2)
    (1, 10, 6, 64, 0, 1, 8),      # 64x64 tile, P = 60: a single partial tile (fast register loader)
    (3, 10, 6, 64, 0, 1, 64),     # 64x64 tile, 15 windows per image: the 16-window halves span images
    (3, 10, 14, 64, 0, 1, 64),    # 64x64 tile, P = 420: ragged last tile (fast register loader)
    (2, 8, 16, 64, 0, 1, 64),     # 64x64 tile, P = 256 full tiles: LDS-DMA
    (5, 64, 64, 64, 0, 1, 128),   # 128x128 tile, full (LDS-DMA): two 16-window halves per tile
    (5, 62, 66, 64, 0, 1, 128),   # 128x128 tile, ragged P = 20460 (fast register loader)
    (5, 64, 64, 64, 0, 1, 64),    # 128x64 tile (LDS-DMA)
]


@pytest.mark.parametrize("case", POOL_CASES)
def test_conv_bias_relu_pool2(env, case):
    """hvit_conv_fwd with ACT_RELU_POOL2 (bf16): GEMM rows walk the output
    pixels window by window and the epilogue keeps each 2x2 window's maximum,
    against max_pool2d(relu(conv2d(x, wf) + bias), 2) in fp32 on the kernel's
    own folded weights.  The maximum is monotone, so ties cannot matter."""
    L, HF = env
    N, Hs, Ws, C1, C2, U, Cout = case
    g, keep, wf, bias, ref = conv_setup(L, HF, case, L.BF16, 22)
    y = nans((N, Hs * U // 2, Ws * U // 2, Cout), BF)
    L.call("hvit_conv_fwd", L.BF16, g, wf.data_ptr(), bias.data_ptr(), y.data_ptr(), L.BF16, None,
           HF.epilogue(act=L.ACT_RELU_POOL2), s())
    check_bf16(y.permute(0, 3, 1, 2), F.max_pool2d(ref, 2), what=f"conv + bias + relu + pool {case}")


@pytest.mark.parametrize("why,case,dt", [
    ("odd Ho", (1, 9, 6, 64, 0, 1, 8), "bf16"),
    ("odd Wo", (1, 10, 7, 64, 0, 1, 8), "bf16"),
    ("C1 % 64 != 0", (1, 10, 6, 32, 0, 1, 8), "bf16"),
    ("f32 request", (1, 10, 6, 64, 0, 1, 8), "f32"),
    ("f32 output", (1, 10, 6, 64, 0, 1, 8), "bf16->f32"),
])
def test_conv_pool2_refusals(env, why, case, dt):
    """What the pooled epilogue cannot do is refused with HVIT_ERR_ARG and a
    message, and nothing is written."""
    L, HF = env
    N, Hs, Ws, C1, C2, U, Cout = case
    dtc = L.F32 if dt == "f32" else L.BF16
    ydt = L.BF16 if dt == "bf16" else L.F32
    x = torch.randn(N, Hs, Ws, C1, device=DEV).to(tdt(L, dtc))
    wf = torch.randn(Cout * C1 * 9, device=DEV).to(tdt(L, dtc))
    bias = torch.randn(Cout, device=DEV)
    g = HF.geom(x, C1, None, 0, N, Hs, Ws, U, 3, 1, 1, Cout)
    y = nans((N * Hs * Ws * Cout,), tdt(L, ydt))  # (room for an unpooled output)
    rc = L.lib().hvit_conv_fwd(dtc, ctypes.byref(g), wf.data_ptr(), bias.data_ptr(), y.data_ptr(), ydt, None,
                               ctypes.byref(HF.epilogue(act=L.ACT_RELU_POOL2)), s())
    torch.cuda.synchronize()
    assert rc == 1, why  # HVIT_ERR_ARG
    assert b"RELU_POOL2" in L.lib().hvit_last_error(), why
    assert bool(torch.isnan(y).all()), why


# ------------------------------------------------------- final conv + tanh ---
TANH_CASES = [
    # N, Hs, Ws, C1, U, Cout, dt
    (2, 12, 10, 64, 1, 1, "bf16"),   # thin_o1 strip kernel, C / 8 = 8, two workgroups (128 pixels each)
    (3, 5, 7, 32, 1, 1, "bf16"),     # strip, C / 8 = 4, one partial workgroup spanning three images
    (2, 9, 20, 16, 1, 1, "bf16"),    # strip, C / 8 = 2
    (1, 33, 47, 8, 1, 1, "bf16"),    # strip, C / 8 = 1, 13 workgroups, the last one partial
    (1, 8, 6, 16, 2, 1, "bf16"),     # thin_o1 flat kernel: x2 upsample
    (2, 7, 9, 128, 1, 1, "bf16"),    # flat: C / 8 = 16
    (2, 12, 10, 64, 1, 1, "f32"),    # flat: f32 input
    (3, 5, 7, 32, 2, 1, "f32"),      # flat: f32 input with x2 upsample
    (2, 9, 7, 12, 1, 1, "bf16"),     # GEMM epilogue (EK_GEN): C1 % 8 != 0, 64x64 tile, general loader
    (2, 9, 7, 12, 1, 1, "f32"),
    (2, 12, 10, 64, 1, 2, "bf16"),   # GEMM epilogue: Cout = 2, 64x64 tile, fast register loader
    (2, 12, 10, 64, 1, 2, "f32"),    # GEMM epilogue: Cout = 2, general loader
]


@pytest.mark.parametrize("case", TANH_CASES)
def test_final_conv_tanh(env, case):
    """hvit_conv_fwd with ACT_TANH, f32 out (the decoder's final block), on each
    of its three kernels, against tanh(conv2d(...)) in fp32 on the rounded
    operands at ACC."""
    L, HF = env
    N, Hs, Ws, C, U, Cout, dt = case
    dtc = dts(dt)
    gen = torch.Generator(device=DEV).manual_seed(23)
    x = torch.randn(N, Hs, Ws, C, device=DEV, generator=gen).to(tdt(L, dtc))
    w = torch.randn(Cout, C, 3, 3, device=DEV, generator=gen) / (C * 9) ** 0.5
    xr = x.float().permute(0, 3, 1, 2).contiguous()
    xu = F.interpolate(xr, scale_factor=U, mode="nearest") if U > 1 else xr
    ref = torch.tanh(F.conv2d(xu, w.to(tdt(L, dtc)).float(), None, 1, 1))
    g = HF.geom(x, C, None, 0, N, Hs, Ws, U, 3, 1, 1, Cout)
    wp = HF.pack_conv(w, 0, dtc)
    y = nans((N, Hs * U, Ws * U, Cout))
    L.call("hvit_conv_fwd", dtc, g, wp.data_ptr(), None, y.data_ptr(), L.F32, None, HF.epilogue(act=L.ACT_TANH), s())
    check_f32(y.permute(0, 3, 1, 2), ref, what=f"conv + tanh {case}")


@pytest.mark.parametrize("odt", ["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 7, 4096, 4099])
def test_tanh_bwd(env, n, odt):
    """hvit_tanh_bwd: dz = dy * (1 - y^2) against fp64, f32 and bf16 dz, with
    y at +-1 and 0 and lengths that end inside a vector."""
    L, HF = env
    gen = torch.Generator(device=DEV).manual_seed(24)
    dy = torch.randn(n, device=DEV, generator=gen)
    y = torch.tanh(2.0 * torch.randn(n, device=DEV, generator=gen))
    if n >= 7:
        y[0], y[1], y[2], y[-1] = 1.0, -1.0, 0.0, -1.0
    dz = nans((n,), tdt(L, dts(odt)))
    L.call("hvit_tanh_bwd", dy.data_ptr(), L.F32, y.data_ptr(), n, dz.data_ptr(), dts(odt), s())
    ref = dy.double() * (1.0 - y.double() ** 2)
    (check_f32 if odt == "f32" else check_bf16)(dz, ref, what=f"tanh_bwd n={n} {odt}")
    if n >= 7:
        assert dz[0].item() == 0.0 and dz[1].item() == 0.0 and dz[-1].item() == 0.0
        assert dz[2].item() == dy[2].to(dz.dtype).item()


# ---------------------------------------------------------- fc1 with GELU ---
_MASKS = {}


def gelu_mask(seed, site, M, N, p):
    key = (seed, site, M, N, p)
    if key not in _MASKS:
        _MASKS[key] = torch.as_tensor(keep_mask(seed, site, M * N, p).reshape(M, N), device=DEV)
    return _MASKS[key]


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("M,N,K", [(228, 2048, 512), (300, 2048, 512), (512, 2048, 512), (8192, 2048, 512),
                                   (37, 136, 72)])
def test_linear_fwd_gelu_only(env, dt, M, N, K):
    """hvit_linear_fwd with ACT_GELU (the inference fc1: only dropout(gelu(x w^T
    + b)) is stored, no out2 and no aux passed), bf16 and f32, with and
    without a dropout descriptor, on the automatic pipeline choice and on
    gemm.h's kernels alone (hvit_gemm_tune(0, -1 / 0): at M = 8192 the automatic
    choice is the 256x256 LDS-ring kernel, M = 512 takes the full-tile
    GELU epilogue, the ragged M the general one) and, bf16, on each LDS-ring
    configuration forced (2 / 4 / 5: 128x128, 256x256, 128x64 where M is a
    multiple of the tile, gemm.h's kernels otherwise), against gelu(x w^T + b)
    * mask / (1 - p) in fp32 with the mask of conftest.keep_mask; acc = 1e-4
    (GELU)."""
    L, HF = env
    dtc = dts(dt)
    gen = torch.Generator(device=DEV).manual_seed(25)
    x = torch.randn(M, K, device=DEV, generator=gen).to(tdt(L, dtc))
    w = (torch.randn(N, K, device=DEV, generator=gen) * K ** -0.5).to(tdt(L, dtc))
    b = torch.randn(N, device=DEV, generator=gen)
    ref = F.gelu(x.float() @ w.float().t() + b)
    chk = check_f32 if dt == "f32" else check_bf16
    p = 0.1
    for cfg in (-1, 0) + ((2, 4, 5) if dt == "bf16" else ()):
        L.lib().hvit_gemm_tune(0, cfg)
        for drop in (False, True):
            a = nans((M, N), tdt(L, dtc))
            e = HF.epilogue(act=L.ACT_GELU, drop=L.dropout(p, 26, 305) if drop else None)
            assert not e.out2 and not e.aux
            L.call("hvit_linear_fwd", dtc, x.data_ptr(), w.data_ptr(), b.data_ptr(), M, N, K, a.data_ptr(), dtc, e,
                   s())
            want = ref * gelu_mask(26, 305, M, N, p) / (1.0 - p) if drop else ref
            chk(a, want, acc=1e-4, what=f"fc1 gelu {M}x{N}x{K} {dt} cfg {cfg} dropout {drop}")
