// GEMM tile epilogues, written once for the kernel families (gemm.h's
// gemm_kernel, gemm_ring.h, wgrad_group.hip; gemm_conv_halo.h shares
// bn_tile_stats and keeps its own uniform staging and store row).
//
// A kernel's accumulators are staged through LDS in 64-row passes (epi_stage)
// and leave row-contiguously, 4 or 8 adjacent columns per thread.  What a kind
// computes on its 4 columns (bias, GELU pair, dropout mask, residual, GELU
// backward, column sums) is one function per kind here (epi_*4); the 8-column
// row of the LDS-DMA and ring kernels (epi_wide_row) applies it to each half
// and stores 16 bytes per lane.  Also here: the plain-store row of a full tile
// with its BatchNorm tile statistics, the deterministic column-sum rows, the
// bf16 pack / unpack helpers and the split-K last-arriver step.
//
// The shared code takes values, never addresses to fetch from: where a kernel
// loads h / the residual / the row scale (before its K loop, before or after
// the staging barrier) and how it rounds them (the ring kernels hand in an f32
// h rounded to bf16, gemm_kernel the exact f32) stays that kernel's choice.
#pragma once
#include "chan_vec.h"  // pack4 / unpack4 / pack8 / unpack8
#include "common.h"

namespace hvit {

enum EpiMode { EPI_STORE = 0, EPI_SLAB = 1, EPI_PATCH = 2, EPI_SPLIT2 = 3 };
enum EpiAct { ACT_NONE = 0, ACT_GELU_DUAL = 1, ACT_TANH = 2, ACT_GELU_BWD = 3 };
// compile-time epilogue kind: a lean kernel for plain stores (+bias, BN stats,
// column sums) and for split-K slabs; everything else takes the generic one
// and for the three fused ViT epilogues (fc1 GELU, residual adds, GELU
// backward), which are only chosen when every tile is full and vector-aligned
enum EpiKind { EK_GEN = 0, EK_STORE = 1, EK_SLAB = 2, EK_GELU_DUAL = 3, EK_RESID = 4, EK_GELU_BWD = 5, EK_PATCH = 6 };

struct Epi {
  int mode = EPI_STORE;
  void* out = nullptr;
  int out_dt = HVIT_F32;
  long ldo = 0;
  void* out2 = nullptr;  // GELU_DUAL: activation output; SPLIT2: columns >= split_col
  int out2_dt = HVIT_F32;
  long ldo2 = 0;
  int split_col = 0;
  const float* bias = nullptr;
  const float* rowadd = nullptr;  // v += rowadd[(m % rowadd_mod) * rowadd_ld + n]
  long rowadd_ld = 0;
  int rowadd_mod = 1;
  int act = ACT_NONE;
  const void* aux = nullptr;  // GELU_BWD: pre-activation h[m][n] (gd: gelu'(h) itself)
  int gd = 0;  // GELU_DUAL: out receives gelu'(h) instead of h; GELU_BWD: aux already is gelu'(h)
  int relu = 0;  // v = max(v, 0) after bias (the eval-mode folded BatchNorm + ReLU of the conv blocks)
  int pool2 = 0;  // EK_STORE of a pooled conv (LdConvF::pool2 row order): 2x2 max of each 4-row window, row m/4
  int aux_dt = HVIT_F32;
  long ldaux = 0;
  uint32_t drop_thr = 0;  // dropout keep test (0 = off)
  float drop_scale = 1.f;
  uint32_t drop_key = 0;  // rng_key(seed, site) (host-resolved when drop_seedp is NULL)
  const unsigned long long* drop_seedp = nullptr;  // device seed word (hvit_dropout_t.seed_ptr)
  unsigned long long drop_seed = 0;
  uint32_t drop_site = 0;
  const float* resid = nullptr;  // v = resid[m][n] + rowscale[m / rps] * v
  long ldr = 0;
  const float* rowscale = nullptr;
  int rows_per_sample = 1;
  float* stats = nullptr;   // BN partials [64-row tile][N][2] = (mean, M2)
  float* colsum = nullptr;  // column sums of the final v: partial row per 64-row block ([cdiv(M,64)][N])
  long slab_stride = 0;     // EPI_SLAB: elements between split-K slabs (0: M * ldo)
  unsigned* tickets = nullptr;  // EPI_SLAB (ring kernels): per-tile arrival counters, zeroed; the last
  float* red_out = nullptr;     //   slice of a tile sums the slabs into red_out (ld = ldo) in-kernel
  float* rs_ptr = nullptr;  // row sums of the A operand (wgrad bias grad): rs_ptr[z * rs_stride + m]
  long rs_stride = 0;
  bool vec_ok = false;      // N % 4 == 0, every operand 16-B aligned with ld % 4 == 0
  int xcd_remap = 1;        // XCD-aware block order (see tile_of); 0 = hardware order
  int dma = 1;              // host: LDS-DMA kernels allowed (GemmCoreDma); 0 = register staging only
  // EPI_PATCH: m = token (b, py, px) of Hp x Wp, n = (ky*P + kx)*C + c
  int pP = 0, pC = 0, pHp = 0, pWp = 0, pH = 0, pW = 0;
  // side job (hvit_slab_sum_t): a deferred weight gradient's split-K slabs
  // summed by this launch's workgroups before their own tiles (epi_side)
  const float* sj_src = nullptr;
  float* sj_dst = nullptr;
  long sj_n4 = 0;      // float4 granules
  long sj_stride4 = 0;
  int sj_splits = 0;
};

// dst[i] = sum_z src[z * stride + i] over the side job's granules, spread over
// every workgroup of the launch.  gemm_kernel runs it after its tile's
// epilogue (two or three workgroups per CU, out of phase: the load latency
// overlaps a co-resident workgroup's K loop); the ring kernels after issuing
// their DMA prologue (one workgroup per CU: the latency overlaps the first
// stages' flight).  Any in-flight stores only make a later counted vmcnt wait
// stricter.  Two forms by the job's slab count alone -- so the order is the
// job's, whatever launch carries it, and hvit_sum_slabs_strided (the job run
// as a launch of its own: side stream, M = 0 carriers) is bit-identical:
//  * fewer than SIDE_WAVE_SPLITS slabs (split-K weight-gradient slabs: ~10^5
//    granules, 4-32 slabs): a granule per thread, even | odd slabs paired as
//    sum_slabs_strided_kernel, eight slabs' loads in flight per step;
//  * SIDE_WAVE_SPLITS or more (partial column-sum rows, the tall-skinny weight
//    gradients' slabs: 10^2-10^3 granules x 128-512 slabs): a granule per wave,
//    its slabs over the lanes, then a butterfly, as sum_slabs_wave_kernel.  (One
//    thread walking 128 slabs held its workgroup ~20 us past the others: round
//    4, the fc1 weight gradient carrying the fc1 bias rows.)
// (SIDE_WAVE_SPLITS, side_wave_granule: common.h)
__device__ __forceinline__ void epi_side(const Epi& ep) {
  if (!ep.sj_n4) return;
  const long nwg = (long)gridDim.x * gridDim.y * gridDim.z;
  const long b = blockIdx.x + (long)gridDim.x * (blockIdx.y + (long)gridDim.y * blockIdx.z);
  const f32x4* src = (const f32x4*)ep.sj_src;
  f32x4* dst = (f32x4*)ep.sj_dst;
  const long st = ep.sj_stride4;
  const int wpb = blockDim.x >> 6;
  if (ep.sj_splits >= SIDE_WAVE_SPLITS) {
    for (long i = b * wpb + (threadIdx.x >> 6); i < ep.sj_n4; i += nwg * wpb) {
      const f32x4 s = side_wave_granule(src, st, ep.sj_splits, i);
      if ((threadIdx.x & 63) == 0) dst[i] = s;
    }
    return;
  }
  const long nthr = nwg * blockDim.x;
  for (long i = b * blockDim.x + threadIdx.x; i < ep.sj_n4; i += nthr) {
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
    int k = 0;
    for (; k + 7 < ep.sj_splits; k += 8) {
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = src[(long)(k + u) * st + i];
#pragma unroll
      for (int u = 0; u < 8; u += 2) {
        s0 += v[u];
        s1 += v[u + 1];
      }
    }
    for (; k + 1 < ep.sj_splits; k += 2) {
      s0 += src[(long)k * st + i];
      s1 += src[(long)(k + 1) * st + i];
    }
    if (k < ep.sj_splits) s0 += src[(long)k * st + i];
    dst[i] = s0 + s1;
  }
}

// 4 adjacent output columns (n .. n+nv-1) of row m: store helpers and the
// fused epilogue math.
// ragged / misaligned fallbacks are out of line: they are rare and would
// otherwise be inlined once per unrolled epilogue row (code size, i-cache)
__device__ __attribute__((noinline)) void store4_slow(void* p, long off, f32x4 v, int nv, int dt) {
  for (int e = 0; e < nv; ++e) st_dt(p, off + e, v[e], dt);
}
__device__ __attribute__((noinline)) f32x4 load4_slow(const void* p, long off, int nv, int dt) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  for (int e = 0; e < nv; ++e) v[e] = ld_dt(p, off + e, dt);
  return v;
}

__device__ __forceinline__ void store4(void* p, long off, const f32x4& v, int nv, int dt) {
  if (dt == HVIT_F32) {
    float* q = (float*)p + off;
    if (nv == 4 && (((uintptr_t)q) & 15) == 0) *(f32x4*)q = v;
    else store4_slow(p, off, v, nv, dt);
  } else {
    bf16_t* q = (bf16_t*)p + off;
    if (nv == 4 && (((uintptr_t)q) & 7) == 0) *(uint2*)q = pack4(v);
    else store4_slow(p, off, v, nv, dt);
  }
}

__device__ __forceinline__ f32x4 load4(const void* p, long off, int nv, int dt) {
  if (dt == HVIT_F32) {
    const float* q = (const float*)p + off;
    if (nv == 4 && (((uintptr_t)q) & 15) == 0) return *(const f32x4*)q;
  } else {
    const bf16_t* q = (const bf16_t*)p + off;
    if (nv == 4 && (((uintptr_t)q) & 7) == 0) return unpack4(*(const uint2*)q);
  }
  return load4_slow(p, off, nv, dt);
}

// FAST: caller guarantees 4 in-range columns and 16-byte (f32) / 8-byte (bf16)
// alignment -- plain vector accesses, no per-lane branches
template <bool FAST>
__device__ __forceinline__ void store4v(void* p, long off, const f32x4& v, int nv, int dt) {
  if constexpr (FAST) {
    if (dt == HVIT_F32) *(f32x4*)((float*)p + off) = v;
    else *(uint2*)((bf16_t*)p + off) = pack4(v);
  } else {
    store4(p, off, v, nv, dt);
  }
}
template <bool FAST>
__device__ __forceinline__ f32x4 load4v(const void* p, long off, int nv, int dt) {
  if constexpr (FAST) {
    if (dt == HVIT_F32) return *(const f32x4*)((const float*)p + off);
    return unpack4(*(const uint2*)((const bf16_t*)p + off));
  } else {
    return load4(p, off, nv, dt);
  }
}
// 8 adjacent columns of a full, aligned row: one 16-byte store (bf16) or two (f32)
__device__ __forceinline__ void store8(void* p, long off, const f32x4& a, const f32x4& b, int dt) {
  if (dt == HVIT_BF16) {
    *(u32x4*)((bf16_t*)p + off) = pack8(a, b);
  } else {
    *(f32x4*)((float*)p + off) = a;
    *(f32x4*)((float*)p + off + 4) = b;
  }
}

// dropout multipliers of 4 adjacent elements (index i0 = m*N + n, i0 even):
// two pair hashes give the four 16-bit uniforms
__device__ __forceinline__ f32x4 keep4(const Epi& ep, uint32_t key, int m, int n, int N) {
  const uint64_t i0 = (uint64_t)m * (uint64_t)N + (uint64_t)n;
  return keep4_at(key, i0, ep.drop_thr, ep.drop_scale);
}
// the dropout key of a launch: folds in the device seed word (one scalar load)
__device__ __forceinline__ uint32_t epi_key(const Epi& ep) {
  return (ep.drop_seedp && ep.drop_thr) ? rng_key(ep.drop_seed ^ *ep.drop_seedp, ep.drop_site) : ep.drop_key;
}

// Inputs the epilogue reads besides the accumulator, loaded for all of a
// thread's rows BEFORE any of its stores: the compiler cannot reorder a load
// above a store that may alias it, so loading inside the store loop would
// serialise one global-load latency per row.
struct EpiIn {
  f32x4 rowadd, aux, resid;
  float rowscale;
};

template <bool FAST>
__device__ __forceinline__ void epi_load4(const Epi& ep, int m, int n, int nv, bool ok, EpiIn& in) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  in.rowadd =
      (ep.rowadd && ok) ? load4v<FAST>(ep.rowadd, (long)(m % ep.rowadd_mod) * ep.rowadd_ld + n, nv, HVIT_F32) : z;
  in.aux = (ep.act == ACT_GELU_BWD && ok) ? load4v<FAST>(ep.aux, (long)m * ep.ldaux + n, nv, ep.aux_dt) : z;
  in.resid = (ep.resid && ok) ? load4v<FAST>(ep.resid, (long)m * ep.ldr + n, nv, HVIT_F32) : z;
  in.rowscale = (ep.resid && ep.rowscale && ok) ? ep.rowscale[m / ep.rows_per_sample] : 1.f;
}

// the generic kind (EK_GEN): every Epi field honoured, ragged tiles allowed
template <bool FAST>
__device__ __forceinline__ void epi_apply4(const Epi& ep, uint32_t dkey, int m, int n, int nv, int N, f32x4& v,
                                           const f32x4& bias, const EpiIn& in) {
  v += bias;
  if (ep.rowadd) v += in.rowadd;
  float keep[4] = {1.f, 1.f, 1.f, 1.f};
  if (ep.drop_thr) {
    const uint64_t i0 = (uint64_t)m * (uint64_t)N + (uint64_t)n;
    if (FAST || (i0 & 1) == 0) {
      const f32x4 k = keep4_at(dkey, i0, ep.drop_thr, ep.drop_scale);
#pragma unroll
      for (int e = 0; e < 4; ++e) keep[e] = k[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) keep[e] = rng_u16k(dkey, i0 + e) >= ep.drop_thr ? ep.drop_scale : 0.f;
    }
  } else if (ep.drop_scale != 1.f) {
#pragma unroll
    for (int e = 0; e < 4; ++e) keep[e] = ep.drop_scale;
  }
  if (ep.act == ACT_GELU_DUAL) {
    f32x4 g, d;
    gelu_gg4(v, g, d);
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] *= keep[e];
    if (ep.gd == 2) {
#pragma unroll
      for (int e = 0; e < 4; ++e) d[e] *= keep[e];
    }
    if (ep.out) store4v<FAST>(ep.out, (long)m * ep.ldo + n, ep.gd ? d : v, nv, ep.out_dt);
    store4v<FAST>(ep.out2, (long)m * ep.ldo2 + n, g, nv, ep.out2_dt);
    return;
  }
  if (ep.act == ACT_TANH) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = tanhf(v[e]);
  }
  if (ep.relu) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] *= keep[e];
  if (ep.act == ACT_GELU_BWD) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] *= ep.gd ? in.aux[e] : gelu_grad(in.aux[e]);
  }
  if (ep.resid) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = in.resid[e] + in.rowscale * v[e];
  }
  if (ep.mode == EPI_STORE) {
    store4v<FAST>(ep.out, (long)m * ep.ldo + n, v, nv, ep.out_dt);
  } else if (ep.mode == EPI_SPLIT2) {
    for (int e = 0; e < nv; ++e) {
      if (n + e < ep.split_col) st_dt(ep.out, (long)m * ep.ldo + n + e, v[e], ep.out_dt);
      else st_dt(ep.out2, (long)m * ep.ldo2 + (n + e - ep.split_col), v[e], ep.out2_dt);
    }
  } else {  // EPI_PATCH: m = token (b, py, px), n = (ky*P + kx)*C + c
    const int hw = ep.pHp * ep.pWp;
    const int b = m / hw, rem = m - b * hw;
    const int py = rem / ep.pWp, px = rem - py * ep.pWp;
    for (int e = 0; e < nv; ++e) {
      const int nn = n + e;
      const int tap = nn / ep.pC, c = nn - tap * ep.pC;
      const int ky = tap / ep.pP, kx = tap - ky * ep.pP;
      const long o = (((long)b * ep.pH + py * ep.pP + ky) * ep.pW + px * ep.pP + kx) * ep.pC + c;
      st_dt(ep.out, o, v[e], ep.out_dt);
    }
  }
}

// Epilogue barrier over LDS only: the tile image and reduction scratch are the
// only data shared between waves there.  __syncthreads() is a workgroup
// release/acquire fence as well, which makes every wave wait (vmcnt(0)) for
// all of its output stores to land before the next half can be staged.
__device__ __forceinline__ void epi_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// Staging: 64-row half hh of a workgroup's accumulators into the LDS image Cs
// (f32, pitch CP floats).  Wave (wm, wn) holds the 16 FM x 16 FN block at rows
// wm * 16 FM, columns wn * 16 FN, as 16x16 MFMA fragments (lane l: column l & 15,
// rows 4 (l >> 4) .. + 3); hh, i, j, r are static after unrolling, so every
// acc[][] index is (no scratch), and a wave's row test is uniform.
template <int CP, int FM, int FN>
__device__ __forceinline__ void epi_stage(float* Cs, const f32x4 (&acc)[FM][FN], int hh, int wm, int wn, int lane) {
  const int frow = lane & 15, fq = lane >> 4;
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm * (16 * FM) + i * 16 + fq * 4 + r - hh * 64;
        if (row >= 0 && row < 64) Cs[row * CP + wn * (16 * FN) + j * 16 + frow] = acc[i][j][r];
      }
}

// ---- kind arithmetic on 4 adjacent columns (n .. n + 3 of row m) of a full tile ---
// x: the staged accumulators; the dropout mask is keep4 of (dkey, m, n); cs: the
// thread's running column sums of the final value (nullptr: none kept).
// EK_STORE: x + bias
__device__ __forceinline__ f32x4 epi_store4(const f32x4& x, const f32x4& bias, float* cs) {
  const f32x4 v = x + bias;
#pragma unroll
  for (int e = 0; e < 4; ++e) cs[e] += v[e];
  return v;
}
// EK_GELU_DUAL: h = x + bias (saved for backward), g = dropout(gelu(h)), d = gelu'(h)
// (gd == 2, GELU_DUAL_DK: the backward's multiplier carries the mask).  Epi::out
// receives h, or d with gd
__device__ __forceinline__ void epi_gelu_dual4(const Epi& ep, uint32_t dkey, int m, int n, int N, const f32x4& x,
                                               const f32x4& bias, f32x4& h, f32x4& d, f32x4& g) {
  h = x + bias;
  const f32x4 k = ep.drop_thr ? keep4(ep, dkey, m, n, N) : (f32x4){1.f, 1.f, 1.f, 1.f};
  gelu_gg4(h, g, d);
  g *= k;
  if (ep.gd == 2) d *= k;
}
// EK_RESID: resid + rowscale * dropout(x + bias)   (f32 residual stream)
__device__ __forceinline__ f32x4 epi_resid4(const Epi& ep, uint32_t dkey, int m, int n, int N, const f32x4& x,
                                            const f32x4& bias, const f32x4& resid, float rowscale, float* cs) {
  f32x4 v = x + bias;
  if (ep.drop_thr) v *= keep4(ep, dkey, m, n, N);
  v = resid + rowscale * v;
  if (cs) {
#pragma unroll
    for (int e = 0; e < 4; ++e) cs[e] += v[e];
  }
  return v;
}
// EK_GELU_BWD: dh = dropout_mask(x + bias) * gelu'(h) (gd: h already is gelu'(h));
// its column sums are the bias gradient
__device__ __forceinline__ f32x4 epi_gelu_bwd4(const Epi& ep, uint32_t dkey, int m, int n, int N, const f32x4& x,
                                               const f32x4& bias, const f32x4& h, float* cs) {
  f32x4 v = x + bias;
  if (ep.drop_thr) v *= keep4(ep, dkey, m, n, N);
  if (ep.gd) {
    v *= h;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] *= gelu_grad(h[e]);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) cs[e] += v[e];
  return v;
}

// Row m of the wide (8 adjacent columns per thread) epilogue of the LDS-DMA
// gemm_kernel and the ring kernels: the kind's arithmetic on each half, then
// 16-byte stores.  crow: the thread's 8 staged values; (sa, sb): the kind's side
// operand halves -- h (EK_GELU_BWD) or the residual (EK_RESID, with its row scale
// rsc) -- loaded by the caller where its pipeline hides them best.
template <int EK>
__device__ __forceinline__ void epi_wide_row(const Epi& ep, uint32_t dkey, const float* crow, int m, int n8, int N,
                                             const f32x4& ba, const f32x4& bb, const f32x4& sa, const f32x4& sb,
                                             float rsc, float (&cs8)[8]) {
  static_assert(EK == EK_STORE || EK == EK_GELU_DUAL || EK == EK_RESID || EK == EK_GELU_BWD, "wide epilogue kinds");
  const f32x4 xa = *(const f32x4*)crow, xb = *(const f32x4*)(crow + 4);
  if constexpr (EK == EK_GELU_DUAL) {
    f32x4 ha, hb, da, db, ga, gb;
    epi_gelu_dual4(ep, dkey, m, n8, N, xa, ba, ha, da, ga);
    epi_gelu_dual4(ep, dkey, m, n8 + 4, N, xb, bb, hb, db, gb);
    // (no out: the inference form, HVIT_ACT_GELU -- only gelu(v) is stored)
    if (ep.out) *(u32x4*)((bf16_t*)ep.out + (long)m * ep.ldo + n8) = ep.gd ? pack8(da, db) : pack8(ha, hb);
    *(u32x4*)((bf16_t*)ep.out2 + (long)m * ep.ldo2 + n8) = pack8(ga, gb);
  } else {
    f32x4 va, vb;
    if constexpr (EK == EK_STORE) {
      va = epi_store4(xa, ba, cs8);
      vb = epi_store4(xb, bb, cs8 + 4);
    } else if constexpr (EK == EK_RESID) {
      va = epi_resid4(ep, dkey, m, n8, N, xa, ba, sa, rsc, cs8);
      vb = epi_resid4(ep, dkey, m, n8 + 4, N, xb, bb, sb, rsc, cs8 + 4);
    } else {
      va = epi_gelu_bwd4(ep, dkey, m, n8, N, xa, ba, sa, cs8);
      vb = epi_gelu_bwd4(ep, dkey, m, n8 + 4, N, xb, bb, sb, cs8 + 4);
    }
    store8(ep.out, (long)m * ep.ldo + n8, va, vb, ep.out_dt);
  }
}

// The wide epilogue's column sums: thread (q0, c8) of RS8 x (BN / 8) holds cs8 over
// its rows of the BM x BN tile at (m0, n8 - 8 c8).  Deterministic: the tile's sums
// leave as partial row m0/64 (plain stores; the tile's other 64-row rows get
// zeros), summed in row order by the caller (hvit_epilogue_t.colsum).  red:
// [RS8][BN] floats of LDS that no wave still reads.
template <int BM, int BN, int RS8>
__device__ __forceinline__ void epi_colsum8(float* colsum, float* red, const float (&cs8)[8], int q0, int c8, int m0,
                                            int n8, int N) {
  epi_barrier();
#pragma unroll
  for (int e = 0; e < 8; ++e) red[q0 * BN + c8 * 8 + e] = cs8[e];
  epi_barrier();
  if (q0 == 0) {
    float t8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float t = 0.f;
      for (int k = 0; k < RS8; ++k) t += red[k * BN + c8 * 8 + e];
      t8[e] = t;
    }
    float* row = colsum + (long)(m0 / 64) * N + n8;
    *(f32x4*)row = (f32x4){t8[0], t8[1], t8[2], t8[3]};
    *(f32x4*)(row + 4) = (f32x4){t8[4], t8[5], t8[6], t8[7]};
#pragma unroll
    for (int r = 1; r < BM / 64; ++r) {
      *(f32x4*)(row + (long)r * N) = (f32x4){0.f, 0.f, 0.f, 0.f};
      *(f32x4*)(row + (long)r * N + 4) = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  }
}

// Plain-store row of a full tile (gemm_kernel's EK_STORE; the halo-resident conv
// kernel's own row is this text): bias, ReLU flag, f32 / bf16 store of row m, columns n .. n + 3 (the host
// guarantees N % 4 == 0, ldo % 4 == 0 and an aligned output).  Returns the stored
// value for bn_tile_stats' sv[], added to the column sums csum (nullptr: none
// kept) and the half's st_sum.
__device__ __forceinline__ f32x4 epi_store_row4(const Epi& ep, const f32x4& x, const f32x4& bias, int m, int n,
                                                float* csum, float (&st_sum)[4]) {
  f32x4 v = x + bias;
  if (ep.relu) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
  }
  if (ep.out_dt == HVIT_F32) {
    *(f32x4*)((float*)ep.out + (long)m * ep.ldo + n) = v;
  } else {
    uint2 u;
    u.x = f2bf2(v[0], v[1]);
    u.y = f2bf2(v[2], v[3]);
    *(uint2*)((bf16_t*)ep.out + (long)m * ep.ldo + n) = u;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (csum) csum[e] += v[e];
    st_sum[e] += v[e];
  }
  return v;
}

// BatchNorm partial of one 64-row sub-tile, shared by gemm_kernel's plain-store / generic
// epilogues and the halo-resident conv kernel (gemm_conv_halo.h), whose partials must stay
// bit-identical: thread (r0, c4) of a 256-thread group holds its output values sv[i] of rows
// r0 + i*RSTEP, columns 4 c4 .. 4 c4 + 3, and their sums st_sum; Cs is the group's staging
// image, reused as scratch; tile = the sub-tile's index (row / 64); n = the thread's first column.
template <int BN, int RSTEP, int NR>
__device__ __forceinline__ void bn_tile_stats(float* stats, float* Cs, int rows_here, int r0, int c4, int n, int N,
                                              long tile, const float (&st_sum)[4], const f32x4 (&sv)[NR]) {
  // per-column (mean, M2) of this 64-row sub-tile.  Each thread holds its
  // rows r0 + i*RSTEP (i < cnt) of 4 columns in registers: local mean and
  // M2 there; the RSTEP partials of a column are then merged by one thread
  // per column (r0 < 4 picks column n + r0), 128 columns in parallel.  Full
  // halves (every partial over NR rows) merge without divisions:
  //   mean = sum(m_k) / RSTEP,  M2 = sum(M2_k) + NR sum((m_k - mean)^2);
  // ragged ones by Chan's pairwise rule.  (A single-wave sequential merge
  // with IEEE divisions cost ~1.5 us per tile, 34 us of the enc1 conv.)
  const bool fullh = rows_here == 64;  // uniform
  const int cnt = fullh ? NR : (rows_here > r0 ? min(NR, (rows_here - r0 + RSTEP - 1) / RSTEP) : 0);
  const float inv = fullh ? 1.f / (float)NR : (cnt ? 1.f / (float)cnt : 0.f);
  float mean[4], q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e) mean[e] = st_sum[e] * inv;
#pragma unroll
  for (int i = 0; i < NR; ++i)
    if (fullh || i < cnt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = sv[i][e] - mean[e];
        q[e] += d * d;
      }
  float* red = Cs;  // [2][RSTEP][BN]; the tile's LDS image is no longer read
  epi_barrier();
  *(f32x4*)(red + r0 * BN + c4 * 4) = (f32x4){mean[0], mean[1], mean[2], mean[3]};
  *(f32x4*)(red + (RSTEP + r0) * BN + c4 * 4) = (f32x4){q[0], q[1], q[2], q[3]};
  epi_barrier();
  if (r0 < 4 && n + r0 < N) {
    const int col = c4 * 4 + r0;
    float mk[RSTEP], qs = 0.f, mu = 0.f, m2 = 0.f;
#pragma unroll
    for (int k = 0; k < RSTEP; ++k) {
      mk[k] = red[k * BN + col];
      qs += red[(RSTEP + k) * BN + col];
    }
    if (fullh) {
#pragma unroll
      for (int k = 0; k < RSTEP; ++k) mu += mk[k];
      mu *= 1.f / (float)RSTEP;
      float dd = 0.f;
#pragma unroll
      for (int k = 0; k < RSTEP; ++k) dd += (mk[k] - mu) * (mk[k] - mu);
      m2 = qs + (float)NR * dd;
    } else {
      float na = 0.f;
      m2 = qs;
#pragma unroll
      for (int k = 0; k < RSTEP; ++k) {
        const int ck = rows_here > k ? min(NR, (rows_here - k + RSTEP - 1) / RSTEP) : 0;
        if (ck == 0) continue;
        const float nn = na + (float)ck, wb = (float)ck / nn;
        const float d = mk[k] - mu;
        mu += d * wb;
        m2 += d * d * (na * wb);
        na = nn;
      }
    }
    *(float2*)(stats + (tile * N + n + r0) * 2) = make_float2(mu, m2);
  }
}

// In-launch split-K reduction, the ticket step (cdna_hip_programming.md section 5,
// "In-launch split-K reduction", counter form).  Every slice of a tile has stored
// its slab with plain stores; here it publishes it (each wave's vmcnt(0), barrier,
// one agent release) and takes a ticket.  Returns (uniformly) whether this
// workgroup drew pieces - 1, i.e. is the last to arrive: it has then acquired the
// other slices' slabs and goes on to sum them, and has reset the ticket for the
// next call (tickets start zeroed: the caller's zero pool).  Correct for any
// placement of the slices; no slice waits on another, so no co-residency is
// assumed.  flag: one int of LDS inside the caller's one array.
__device__ __forceinline__ bool splitk_last_arriver(unsigned* ticket, int pieces, int* flag) {
  const int tid = threadIdx.x;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned prev = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = prev == (unsigned)(pieces - 1);
    if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *flag = last;
  }
  __syncthreads();
  if (!*flag) return false;
  if (tid == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  return true;
}

}  // namespace hvit
