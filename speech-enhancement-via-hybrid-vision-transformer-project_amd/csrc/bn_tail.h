// The BatchNorm2d -> ReLU -> Dropout2d -> MaxPool2d tail, per channel: the
// pieces that bnact.hip (z in HBM) and both kernel families of c1block.hip (z
// recomputed on the fly, VALU and matrix-core) must evaluate as the same
// function -- the per-(sample, channel) keep multiplier, BatchNorm as one
// scale / shift, its training backward as two coefficients, and the max-pool's
// first-maximum routing.  Callers pass values (a kernel keeps its own loads,
// window predicates and accumulation order).
#pragma once

#include "common.h"

namespace hvit {

// Dropout2d multipliers of channels c .. c+CV-1 of sample n (element index
// n*C + c).  CV a multiple of 4 (c too): two pair hashes per four channels;
// smaller CV: one channel at a time, the same value as its keep4_at lane.
template <int CV>
__device__ __forceinline__ void chan_keep(const DropKey& k, int n, int C, int c, float* m) {
  const uint64_t i0 = (uint64_t)n * C + c;
  if constexpr (CV % 4 == 0) {
    if (!k.thr) {
#pragma unroll
      for (int e = 0; e < CV; ++e) m[e] = 1.f;
      return;
    }
#pragma unroll
    for (int e4 = 0; e4 < CV; e4 += 4) {
      const f32x4 kp = keep4_at(k.key, i0 + e4, k.thr, k.dscale);
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e4 + e] = kp[e];
    }
  } else {
#pragma unroll
    for (int e = 0; e < CV; ++e) m[e] = k.thr ? (rng_u16k(k.key, i0 + e) >= k.thr ? k.dscale : 0.f) : 1.f;
  }
}

// relu(bn(z)) = max(z*sc + sh, 0)
__device__ __forceinline__ void bn_scale_shift(float mean, float invstd, float gamma, float beta, float& sc,
                                               float& sh) {
  sc = invstd * gamma;
  sh = beta - mean * sc;
}

// backward of y = bn(z) given g = dL/dy: with s1 = sum g / M, s2 = sum g*xhat / M
// (training; both 0 in eval mode, where the statistics are constants)
//   dz = sc*(g - s1 - xhat*s2) = sc*g + ca + cb*z,  xhat = (z - mean)*invstd
__device__ __forceinline__ void bn_bwd_coeffs(float sc, float mean, float invstd, float sum_g, float sum_gx,
                                              float invM, int training, float& ca, float& cb) {
  const float s1 = training ? sum_g * invM : 0.f, s2 = training ? sum_gx * invM : 0.f;
  cb = -sc * s2 * invstd;
  ca = -sc * s1 - cb * mean;
}

// dz of one pixel from its routed gradient g and the coefficients above.  Two
// explicit fmas: left to the compiler's contraction, one instantiation paired
// sc*g with cb*z in a packed multiply and added both unfused (an ulp apart from
// its siblings)
__device__ __forceinline__ float bn_bwd_dz(float sc, float g, float ca, float cb, float z) {
  return __builtin_fmaf(cb, z, __builtin_fmaf(sc, g, ca));
}

// The max-pool's routing for one channel: the first maximum (scan order) of
// relu(bn(z[q])) over the nq <= NQ window positions -- torch's max_pool2d tie
// rule.  Every value is one explicit fma (in the forward too): equal inputs
// must give equal values so that a tie stays with the first (compiler-chosen
// contraction made tied bf16 inputs differ by an ulp and moved the gradient).
struct FirstMax {
  int arg;     // window position of the maximum
  float best;  // relu(bn(z)) there; the gradient passes where best > 0
  float z;     // z there
};
template <int NQ>
__device__ __forceinline__ FirstMax route_first_max(const float (&z)[NQ], float sc, float sh, int nq = NQ) {
  FirstMax r = {0, fmaxf(__builtin_fmaf(z[0], sc, sh), 0.f), z[0]};
#pragma unroll
  for (int q = 1; q < NQ; ++q) {
    if (q >= nq) break;
    const float v = fmaxf(__builtin_fmaf(z[q], sc, sh), 0.f);
    const bool gt = v > r.best;
    r.best = gt ? v : r.best;
    r.z = gt ? z[q] : r.z;
    r.arg = gt ? q : r.arg;
  }
  return r;
}

}  // namespace hvit
