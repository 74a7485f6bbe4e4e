// C-ABI conv forward and data gradient (3x3 implicit GEMM, patch embedding / col2im) on the MFMA GEMM.
#include "gemm_host.h"
#include "gemm_conv_halo.h"

// rows per BatchNorm partial tile written by hvit_conv_fwd for geometry g
extern "C" int hvit_conv_bn_tile_rows(const hvit_conv_geom_t* g) {
  return g && thin_c1(g) ? hvit_thin_c1_bn_tile_rows() : 64;
}

extern "C" int hvit_conv_fwd(int dt, const hvit_conv_geom_t* g, const void* w_packed, const float* bias,
                             void* y, int y_dt, float* bn_partials, const hvit_epilogue_t* epi, void* stream) {
  if (int rc = check_geom(g)) return rc;
  HVIT_CHECK(w_packed && y, "hvit_conv_fwd: null pointer");
  if (int rc = check_epi(epi)) return rc;
  HVIT_CHECK(!epi || epi->act == HVIT_ACT_NONE || epi->act == HVIT_ACT_TANH || epi->act == HVIT_ACT_RELU ||
                 epi->act == HVIT_ACT_RELU_POOL2,
             "hvit_conv_fwd: act must be NONE, TANH, RELU or RELU_POOL2");
  HVIT_CHECK(!epi || (epi->act != HVIT_ACT_RELU && epi->act != HVIT_ACT_RELU_POOL2) || !bn_partials,
             "hvit_conv_fwd: RELU with BatchNorm partials");
  const bool pool2 = epi && epi->act == HVIT_ACT_RELU_POOL2;
  HVIT_CHECK(!epi || !epi->resid, "hvit_conv_fwd: residual epilogue unsupported");
  HVIT_CHECK(aligned16(w_packed), "hvit_conv_fwd: weight alignment");
  const bool plain_epi = !epi || (epi->dropout.p == 0.f && !epi->rowadd && !epi->colsum);
  if (pool2) {
    // the eval-mode encoder block with its max-pool (components.py:55-85 with pool 2, BatchNorm folded):
    // the implicit-im2col loader walks output pixels window by window, the epilogue keeps each
    // window's maximum; y is [N, Ho/2, Wo/2, Cout]
    HVIT_CHECK(dt == HVIT_BF16 && y_dt == HVIT_BF16 && plain_epi && !epi->resid && aligned16(y) && g->Cout % 4 == 0,
               "hvit_conv_fwd: RELU_POOL2 needs bf16 in / out, no dropout / rowadd / colsum, aligned output");
    auto la = conv_a<bf16_t>(g, g->src1, g->C1, g->src2, g->C2, g->Hs, g->Ws, g->U, g->KS, g->stride, g->pad);
    HVIT_CHECK(la.Ho > 0 && la.Wo > 0 && la.Ho % 2 == 0 && la.Wo % 2 == 0, "hvit_conv_fwd: RELU_POOL2 needs even Ho, Wo");
    HVIT_CHECK(conv_fast_ok(la, g->N), "hvit_conv_fwd: RELU_POOL2 needs 64-channel-multiple sources (fast loader)");
    Epi ep = to_epi(epi, y, y_dt, g->Cout);
    ep.bias = bias;
    LdConvF<bf16_t> f = conv_fast(la, g->N);
    f.pool2 = 1;
    return launch_gemm<bf16_t>(f, dense<bf16_t, true>(w_packed, la.Kt, g->Cout, la.Kt), la.P, g->Cout, la.Kt, 1, ep,
                               (hipStream_t)stream);
  }
  if (thin_c1(g) && plain_epi && !bias && (!epi || epi->act == HVIT_ACT_NONE) && aligned16(y))
    return hvit_thin_c1_fwd(dt, g, w_packed, y, y_dt, bn_partials, (hipStream_t)stream);
  // BN partial tiles follow hvit_conv_bn_tile_rows(g): the thin path must have been taken
  HVIT_CHECK(!bn_partials || !thin_c1(g), "hvit_conv_fwd: Cin=1 BatchNorm partials need the thin path "
                                           "(no bias / epilogue, 16-byte aligned output)");
  if (thin_o1(g) && plain_epi && !bias && !bn_partials && (!epi || epi->act != HVIT_ACT_RELU))
    return hvit_thin_o1_fwd(dt, g, w_packed, y, y_dt, epi && epi->act == HVIT_ACT_TANH, (hipStream_t)stream);
  HVIT_CHECK(!epi || epi->side.n <= 0, "hvit_conv_fwd: epilogue side jobs are for the linear entry points");
  Epi ep = to_epi(epi, y, y_dt, g->Cout);
  ep.bias = bias;
  ep.stats = bn_partials;
  DT_DISPATCH(dt, {
    auto la = conv_a<T>(g, g->src1, g->C1, g->src2, g->C2, g->Hs, g->Ws, g->U, g->KS, g->stride, g->pad);
    HVIT_CHECK(la.Ho > 0 && la.Wo > 0, "hvit_conv_fwd: empty output");
    int Kt = la.Kt;
    if constexpr (sizeof(T) == 2) {
      if (conv_fast_ok(la, g->N)) {
        // one source, no upsample, whole-row tiles: the input halo stays in LDS (gemm_conv_halo.h)
        if (conv_halo_try(conv_fast(la, g->N), dense<T, true>(w_packed, Kt, g->Cout, Kt), la.P, g->Cout, Kt, ep,
                          (hipStream_t)stream, true)) {
          HVIT_LAUNCH_CHECK();
          return HVIT_OK;
        }
        // automatic tile (forced 128x128 5.344 / 128x64 5.189 vs 5.152-5.155 ms/step: DESIGN.md §8)
        return launch_gemm<T>(conv_fast(la, g->N), dense<T, true>(w_packed, Kt, g->Cout, Kt), la.P, g->Cout, Kt, 1,
                              ep, (hipStream_t)stream);
      }
    }
    // odd reduction length (Cin=1 first conv): weights take the scalar load path
    return launch_gemm<T>(la, dense<T, true>(w_packed, Kt, g->Cout, Kt), la.P, g->Cout, Kt, 1, ep,
                          (hipStream_t)stream);
  });
}

// The 3x3 path is the forward's GEMM over dy (the same loader pairs, so the
// same kernels); the patch path is a dense GEMM with the col2im scatter epilogue.
extern "C" int hvit_conv_dgrad(int dt, const hvit_conv_geom_t* g, const void* dy, const void* w, void* dx,
                               int dx_dt, void* stream) {
  if (int rc = check_geom(g)) return rc;
  HVIT_CHECK(dy && w && dx, "hvit_conv_dgrad: null pointer");
  HVIT_CHECK(aligned16(dy) && aligned16(w), "hvit_conv_dgrad: alignment");
  hipStream_t st = (hipStream_t)stream;
  const int Ctot = g->C1 + g->C2;
  const int Hi = g->Hs * g->U, Wi = g->Ws * g->U;
  const int Ho = (Hi + 2 * g->pad - g->KS) / g->stride + 1;
  const int Wo = (Wi + 2 * g->pad - g->KS) / g->stride + 1;
  if (g->KS == g->stride && g->pad == 0) {
    // non-overlapping patches: dX[patch pixel] = dT[token] . W  scattered back (col2im)
    HVIT_CHECK(g->U == 1 && g->C2 == 0, "hvit_conv_dgrad: patch path needs U=1, one source");
    if (Ho * g->KS != Hi || Wo * g->KS != Wi)
      (void)hipMemsetAsync(dx, 0, (size_t)g->N * Hi * Wi * Ctot * (dx_dt == HVIT_F32 ? 4 : 2), st);
    Epi ep;
    ep.mode = EPI_PATCH;
    ep.out = dx;
    ep.out_dt = dx_dt;
    ep.pP = g->KS;
    ep.pC = Ctot;
    ep.pHp = Ho;
    ep.pWp = Wo;
    ep.pH = Hi;
    ep.pW = Wi;
    const int Kt = g->KS * g->KS * Ctot;
    const int M = g->N * Ho * Wo;
    return hvit_gemm_kc_mn(dt, dy, w, M, Kt, g->Cout, ep, st, "hvit_conv_dgrad: patch alignment");
  }
  HVIT_CHECK(g->stride == 1 && g->pad == g->KS / 2 && (g->KS & 1), "hvit_conv_dgrad: only odd same-convs");
  if (thin_o1(g) && dx_dt == dt && aligned16(dx)) return hvit_thin_o1_dgrad(dt, g, dy, w, dx, st);
  Epi ep;
  ep.out = dx;
  ep.out_dt = dx_dt;
  ep.ldo = Ctot;
  DT_DISPATCH(dt, {
    // dU = conv(dy, flipped/transposed W): im2col over dy (Cout channels, stride 1)
    auto la = conv_a<T>(g, dy, g->Cout, nullptr, 0, Ho, Wo, 1, g->KS, 1, g->pad);
    int Kt = la.Kt;
    if constexpr (sizeof(T) == 2) {
      if (conv_fast_ok(la, g->N)) {
        // whole-row tiles of dy: its halo stays in LDS (gemm_conv_halo.h)
        if (conv_halo_try(conv_fast(la, g->N), dense<T, true>(w, Kt, Ctot, Kt), la.P, Ctot, Kt, ep, st, false)) {
          HVIT_LAUNCH_CHECK();
          return HVIT_OK;
        }
        return launch_gemm<T>(conv_fast(la, g->N), dense<T, true>(w, Kt, Ctot, Kt), la.P, Ctot, Kt, 1, ep, st);
      }
    }
    return launch_gemm<T>(la, dense<T, true>(w, Kt, Ctot, Kt), la.P, Ctot, Kt, 1, ep, st);
  });
}

// HVIT_TUNE_CONV_HALO: the A operand of the 3x3 forward / data-gradient GEMMs
// (conv_halo_mode_ref); returns the previous mode, other values change nothing
int hvit_conv_halo_tune(int value) {
  const int old = conv_halo_mode_ref();
  if (value >= 0 && value <= 2) conv_halo_mode_ref() = value;
  return old;
}
// HVIT_TUNE_CONV_HALO_COUNT: halo-resident launches so far
int hvit_conv_halo_count() { return (int)conv_halo_count_ref(); }

// the halo image's address map, for the CPU check of its slots and bank pattern
extern "C" int hvit_conv_halo_off(int H, int W, int C, int rows, int hy, int hx, int chunk) {
  HaloGeom hg;
  if ((rows != 128 && rows != 256) || !halo_geom(H, W, C, rows, &hg)) return -1;
  const int TW = 1 << hg.tws, TR = rows >> hg.tws;
  if (hy < 0 || hy >= TR + 2 || hx < 0 || hx >= TW + 2 || chunk < 0 || chunk >= C / 8) return -1;
  return halo_off(hy, hx, chunk, TW + 2, C);
}
