// FP8 (OCP e4m3) multi-head self-attention forward for gfx950: the
// "fp8 MFMA attention path" of BASELINE config 5 (D=768, 12 heads, hd 64),
// restating MultiHeadSelfAttention's core (models/attention.py:91-107:
// softmax(q k^T * scale) -> dropout -> @ v) with fp8 matrix operands.
//
// One workgroup per (b, h), 16 waves x 16 queries (N <= 256).  The head's K
// and V are read once (bf16, the qkv Linear output in place), scaled by a
// power of two chosen from their absolute maximum so that e4m3's range is
// used (448 / amax, rounded down to 2^e), converted to e4m3 and staged in LDS:
//   K   [key][64 d]  (80-B rows: conflict-free 8-byte fragment reads),
//   V^T [d][256 keys] (264-B rows), keys >= N zero.
// Each query row gets its own power-of-two scale the same way.
//   S^T = K Q^T        v_mfma_f32_16x16x32_fp8_fp8 (2 per 16-key tile)
//   softmax            f32, exactly as the bf16 kernel (running max, exp2)
//   O^T = V^T P^T      v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 x e4m3), one
//                      per 128 keys and 16 d: twice the bf16 MFMA rate.  P in
//                      [0, 1] is stored as 256 * P in e4m3 and the MFMA's
//                      block scales undo both the P and the V scaling exactly
//                      (E8M0 exponents).
// The dropout mask is the bf16 kernel's (same hash, same indices), so the
// backward -- bf16, recomputing P from the saved lse (FlashAttention-3's fp8
// recipe: fp8 forward, bf16 backward) -- sees the forward's mask; with
// keep_bits the forward also stores the mask in the bf16 kernel's keep-bit
// layout, so that backward reads it instead of re-hashing.
#include "attention_tile.h"
#include "common.h"

namespace hvit {
namespace {

constexpr int F8_KMAX = 256;
constexpr int F8_KP = 80;         // K image row pitch (64 fp8 + 16 pad)
constexpr int F8_VP = 256 + 8;    // V^T image row pitch (256 fp8 keys + 8 pad)
constexpr float F8_MAX = 448.f;   // e4m3 largest finite
typedef int i32x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float clamp8(float x) { return fminf(fmaxf(x, -F8_MAX), F8_MAX); }
// 4 floats -> 4 e4m3 bytes (byte i = value i)
__device__ __forceinline__ uint32_t f8x4(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(clamp8(a), clamp8(b), 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(clamp8(c), clamp8(d), w, true);
  return (uint32_t)w;
}
// power-of-two exponent e with amax * 2^e <= 448 (0 for an all-zero block)
__device__ __forceinline__ int pow2_exp(float amax) {
  if (!(amax > 0.f)) return 0;
  const float r = F8_MAX / amax;
  int e = (int)((__float_as_uint(r) >> 23) & 0xff) - 127;  // floor(log2(r)) for normal r
  return e < -60 ? -60 : (e > 60 ? 60 : e);
}
__device__ __forceinline__ float exp2i(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }
__device__ __forceinline__ float absmax8(const u32x4& u) {
  float m = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    m = fmaxf(m, fmaxf(fabsf(__uint_as_float(u[e] << 16)), fabsf(__uint_as_float(u[e] & 0xffff0000u))));
  return m;
}
// 8 bf16 (u32x4) * s -> 8 e4m3 bytes
__device__ __forceinline__ uint2 to_f8(const u32x4& u, float s) {
  uint2 r;
  r.x = f8x4(__uint_as_float(u[0] << 16) * s, __uint_as_float(u[0] & 0xffff0000u) * s,
             __uint_as_float(u[1] << 16) * s, __uint_as_float(u[1] & 0xffff0000u) * s);
  r.y = f8x4(__uint_as_float(u[2] << 16) * s, __uint_as_float(u[2] & 0xffff0000u) * s,
             __uint_as_float(u[3] << 16) * s, __uint_as_float(u[3] & 0xffff0000u) * s);
  return r;
}

template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void mhsa_fwd_fp8_kernel(const bf16_t* __restrict__ qkv,
                                                                  bf16_t* __restrict__ o, float* __restrict__ lse,
                                                                  int N, int H, float scale, uint32_t thr,
                                                                  float dscale, DSeed seed_,
                                                                  uint32_t site, uint32_t* __restrict__ kbits) {
  const unsigned long long seed = seed_;
  constexpr int NT = WAVES * 64;
  constexpr int PER = F8_KMAX * 8 / NT;  // 16-byte chunks of K (and of V) per thread
  __shared__ __attribute__((aligned(16))) char Ks[F8_KMAX * F8_KP];
  __shared__ __attribute__((aligned(16))) char Vt[64 * F8_VP];
  __shared__ float red[2][WAVES];
  const int D = H * 64;
  const long pitch = 3L * D;
  const int h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int frow = lane & 15, fq = lane >> 4;
  const bf16_t* base = qkv + (long)b * N * pitch + h * 64;
  const uint64_t bh = (uint64_t)b * H + h;

  // ---- K, V (bf16) -> registers, block absmax
  u32x4 kr[PER], vr[PER];
  float mk = 0.f, mv = 0.f;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int c = tid + i * NT, key = c >> 3, dc = c & 7;
    kr[i] = vr[i] = (u32x4){0u, 0u, 0u, 0u};
    if (key < N) {
      kr[i] = *(const u32x4*)(base + D + (long)key * pitch + dc * 8);
      vr[i] = *(const u32x4*)(base + 2 * D + (long)key * pitch + dc * 8);
    }
    mk = fmaxf(mk, absmax8(kr[i]));
    mv = fmaxf(mv, absmax8(vr[i]));
  }
  // this lane's query row (2 x 8 d per lane), its own scale
  const int q = blockIdx.x * WAVES * 16 + w * 16 + frow;
  u32x4 qb[2];
  float mq = 0.f;
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    qb[s2] = q < N ? *(const u32x4*)(base + (long)q * pitch + 32 * s2 + 8 * fq) : (u32x4){0u, 0u, 0u, 0u};
    mq = fmaxf(mq, absmax8(qb[s2]));
  }
  mq = fmaxf(mq, __shfl_xor(mq, 16, 64));
  mq = fmaxf(mq, __shfl_xor(mq, 32, 64));
  mk = wave_max(mk);
  mv = wave_max(mv);
  if (lane == 0) {
    red[0][w] = mk;
    red[1][w] = mv;
  }
  __syncthreads();
  mk = mv = 0.f;
#pragma unroll
  for (int i = 0; i < WAVES; ++i) {
    mk = fmaxf(mk, red[0][i]);
    mv = fmaxf(mv, red[1][i]);
  }
  const int ek = pow2_exp(mk), ev = pow2_exp(mv), eq = pow2_exp(mq);
  const float sk = exp2i(ek), sv = exp2i(ev), sq = exp2i(eq);
  // ---- e4m3 images: K row-major, V transposed (keys >= N are zero)
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int c = tid + i * NT, key = c >> 3, dc = c & 7;
    *(uint2*)(Ks + key * F8_KP + dc * 8) = to_f8(kr[i], sk);
    const uint2 v8 = to_f8(vr[i], sv);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      Vt[(dc * 8 + e) * F8_VP + key] = (char)(((e < 4 ? v8.x : v8.y) >> (8 * (e & 3))) & 0xffu);
  }
  long q8[2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) q8[s2] = __builtin_bit_cast(long, to_f8(qb[s2], sq));
  __syncthreads();

  const int nkt = (N + 15) >> 4;
  // S^T tiles: st[j][r] = score(key 16j + 4fq + r, query q) in log2 units
  const float c2 = scale * 1.4426950408889634f / (sq * sk);
  f32x4 st[F8_KMAX / 16];
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < F8_KMAX / 16; ++j) {
    if (j < nkt) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const long kf = *(const long*)(Ks + (16 * j + frow) * F8_KP + 32 * s2 + 8 * fq);
        a = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(kf, q8[s2], a, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = (16 * j + 4 * fq + r < N) ? a[r] * c2 : -INFINITY;
        a[r] = v;
        mx = fmaxf(mx, v);
      }
      st[j] = a;
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < F8_KMAX / 16; ++j) {
    if (j < nkt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f(st[j][r] - mx);
        st[j][r] = p;
        sum += p;
      }
    }
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.f / sum;
  // O^T[d][q] = V^T[d][keys] (256 P^T[keys][q]) per 128-key block; lane (q, g)
  // supplies keys 128kb + 16m + 4g + r (m = 0..7, r = 0..3) for both operands
  f32x4 ot[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) ot[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int qq = q < N ? q : 0;
  // this lane's keep-bit pair (attention_tile.h's layout, one 256-key chunk)
  unsigned long long kw = 0ull;
#pragma unroll
  for (int kb = 0; kb < F8_KMAX / 128; ++kb) {
    if (128 * kb < N) {
      i32x8 pb;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const int j = 8 * kb + m;
        f32x4 p = (j < nkt) ? st[j] * 256.f : (f32x4){0.f, 0.f, 0.f, 0.f};
        // 0/1 keep mask only: 256 P stays <= 256 < 448 (e4m3 max) for any p;
        // the 1/(1-p) scale is folded into the output's 1/sum below
        if (thr && j < nkt) {
          const f32x4 k4 = v2_keep(bh, N, qq, 16 * j + 4 * fq, thr, 1.f, seed, site);
          p *= k4;
          kw |= (unsigned long long)((k4[0] > 0.f ? 1u : 0u) | (k4[1] > 0.f ? 2u : 0u) | (k4[2] > 0.f ? 4u : 0u) |
                                     (k4[3] > 0.f ? 8u : 0u))
                << kb_nibble(j);
        }
        pb[m] = (int)f8x4(p[0], p[1], p[2], p[3]);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const char* vrow = Vt + (16 * t + frow) * F8_VP + 128 * kb + 4 * fq;
        i32x8 va;
#pragma unroll
        for (int m = 0; m < 8; ++m) va[m] = *(const int*)(vrow + 16 * m);
        // scale_a = 2^-ev (undo V's scale), scale_b = 2^-8 (undo 256 P)
        ot[t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(va, pb, ot[t], 0, 0, 0, 127 - ev, 0, 127 - 8);
      }
    }
  }
  if (q < N) {
    v2_store_row(o + ((long)b * N + q) * D + h * 64, ot, thr ? inv * dscale : inv, fq);
    if (fq == 0) lse[bh * N + q] = (mx + log2f(sum)) * 0.6931471805599453f;
    if (kbits && thr) *(uint2*)(kbits + kb_pair(0, 0, bh * N, q, fq)) = make_uint2((uint32_t)kw, (uint32_t)(kw >> 32));
  }
}

// ============================================================================
// Round-5 form (mhsa_fwd_fp8_v2): the same arithmetic -- the same e4m3
// roundings, scales, mask and normaliser, so the emulation tests pin both --
// with the bf16 v2 kernel's economy:
//  * staging in units of 4 keys x 16 bytes: a thread converts its unit and
//    writes K as 8-byte rows and V^T as one dword per d (a 4x4 byte transpose
//    in registers by v_perm) instead of 16 single-byte LDS writes;
//  * the d (k) order of the S^T MFMAs is per-lane contiguous (lane group g
//    supplies d = 16g .. 16g + 15 to both MFMAs: any order both operands agree
//    on sums the same), so a K fragment pair is one 16-byte LDS read;
//  * the key order of the P V MFMA is the P registers' own (lane group g,
//    register m, byte r <-> key 128kb + 16m + 4g + r): V^T is stored in that
//    permuted key order, so a lane's 32 bytes of V^T are two 16-byte reads
//    (row pitch 272 B: 16 lanes of a read phase hit disjoint banks);
//  * 256 P comes out of the exponent (exp2(s c2 - max + 8)), the e4m3
//    conversion needs no clamp (256 P <= 256 < 448), the block scale of P is
//    2^0 and the normaliser is the sum of the 256 P values;
//  * the dropout mask as selects from one hash per key pair.
// ============================================================================
constexpr int F8V_KP = 80;   // K image row pitch (64 e4m3 + 16 pad)
constexpr int F8V_VP = 272;  // V^T image row pitch (256 keys + 16 pad)

// position of key k in a V^T row (see above)
__device__ __forceinline__ int f8v_pos(int k) {
  return (k & ~127) + 32 * ((k >> 2) & 3) + 4 * ((k >> 4) & 7) + (k & 3);
}
// 4x4 byte transpose: o[e] = {w0.b_e, w1.b_e, w2.b_e, w3.b_e}
__device__ __forceinline__ void bt4(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t (&o)[4]) {
  const uint32_t t0 = __builtin_amdgcn_perm(w1, w0, 0x05010400u), t1 = __builtin_amdgcn_perm(w1, w0, 0x07030602u);
  const uint32_t t2 = __builtin_amdgcn_perm(w3, w2, 0x05010400u), t3 = __builtin_amdgcn_perm(w3, w2, 0x07030602u);
  o[0] = __builtin_amdgcn_perm(t2, t0, 0x05040100u);
  o[1] = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
  o[2] = __builtin_amdgcn_perm(t3, t1, 0x05040100u);
  o[3] = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
}
// 4 non-negative floats <= 448 -> 4 e4m3 bytes
__device__ __forceinline__ int f8x4_pos(f32x4 p) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(p[0], p[1], 0, false);
  return __builtin_amdgcn_cvt_pk_fp8_f32(p[2], p[3], w, true);
}
// |x| maximum of 8 bf16 as bf16 bits in both 16-bit halves' maximum: the sign
// bits cleared, the magnitudes compared as unsigned integers two at a time
// (v_pk_max_u16; finite non-negative bf16 order like their bit patterns)
typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u16x2_t amax_pk(u16x2_t m, const u32x4& u) {
#pragma unroll
  for (int e = 0; e < 4; ++e) m = __builtin_elementwise_max(m, __builtin_bit_cast(u16x2_t, u[e] & 0x7fff7fffu));
  return m;
}
__device__ __forceinline__ float amax_f(u16x2_t m) {
  return __uint_as_float((uint32_t)(m.x > m.y ? m.x : m.y) << 16);
}
// 8 bf16 * 2^e -> 8 e4m3 bytes by the scaled conversion (v_cvt_scalef32_pk_fp8_bf16
// divides by its scale operand -- measured, tools/probes/cvt_probe.hip -- and
// rounds to nearest even like the emulation's float8_e4m3fn cast): inv = 2^-e
typedef __bf16 bf16x2v_t __attribute__((ext_vector_type(2)));
typedef short s16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t f8w(uint32_t a, uint32_t b, float inv) {
  s16x2_t r = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16((s16x2_t){0, 0}, __builtin_bit_cast(bf16x2v_t, a), inv, false);
  r = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(r, __builtin_bit_cast(bf16x2v_t, b), inv, true);
  return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ uint2 f8_bf(const u32x4& u, float inv) {
  return make_uint2(f8w(u[0], u[1], inv), f8w(u[2], u[3], inv));
}

// FULL: N == 256 (every key tile whole, every query in range)
template <int WAVES, bool FULL>
__global__ __launch_bounds__(WAVES * 64) void mhsa_fwd_fp8_v2(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ o,
                                                             float* __restrict__ lse, int N, int H, float scale,
                                                             uint32_t thr, float dscale, DSeed seed_, uint32_t site,
                                                             uint32_t* __restrict__ kbits) {
  const unsigned long long seed = seed_;
  constexpr int NT = WAVES * 64;
  constexpr int UPT = 1024 / NT;  // staging units (4 keys x 8 d of K or V) per thread
  __shared__ __attribute__((aligned(16))) char Ks[F8_KMAX * F8V_KP];
  __shared__ __attribute__((aligned(16))) char Vt[64 * F8V_VP];
  __shared__ float red[2][WAVES];
  const int D = H * 64;
  const long pitch = 3L * D;
  const int h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int frow = lane & 15, fq = lane >> 4;
  const bf16_t* base = qkv + (long)b * N * pitch + h * 64;
  const uint64_t bh = (uint64_t)b * H + h;

  // ---- this lane's query row: d = 16 fq .. 16 fq + 15 (both S^T MFMAs)
  const int q = blockIdx.x * WAVES * 16 + w * 16 + frow;
  const bool qin = FULL || q < N;
  u32x4 qb[2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2)
    qb[s2] = qin ? *(const u32x4*)(base + (long)q * pitch + 16 * fq + 8 * s2) : (u32x4){0u, 0u, 0u, 0u};
  // ---- K / V units -> registers, per-tensor absmax
  u32x4 ur[UPT][4];
  float mk = 0.f, mv = 0.f;
#pragma unroll
  for (int i = 0; i < UPT; ++i) {
    const int u = tid + i * NT, tv = u >> 9, a = (u >> 3) & 63, dc = u & 7;
    const bf16_t* src = base + (tv + 1) * D + dc * 8;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = 4 * a + r;
      ur[i][r] = FULL || key < N ? *(const u32x4*)(src + (long)key * pitch) : (u32x4){0u, 0u, 0u, 0u};
    }
    u16x2_t m2 = {0, 0};
#pragma unroll
    for (int r = 0; r < 4; ++r) m2 = amax_pk(m2, ur[i][r]);
    const float m = amax_f(m2);
    if (tv) mv = fmaxf(mv, m);
    else mk = fmaxf(mk, m);
  }
  float mq = amax_f(amax_pk(amax_pk((u16x2_t){0, 0}, qb[0]), qb[1]));
  mq = fmaxf(mq, __shfl_xor(mq, 16, 64));
  mq = fmaxf(mq, __shfl_xor(mq, 32, 64));
  mk = wave_max(mk);
  mv = wave_max(mv);
  if (lane == 0) {
    red[0][w] = mk;
    red[1][w] = mv;
  }
  __syncthreads();
  mk = mv = 0.f;
#pragma unroll
  for (int i = 0; i < WAVES; ++i) {
    mk = fmaxf(mk, red[0][i]);
    mv = fmaxf(mv, red[1][i]);
  }
  const int ek = pow2_exp(mk), ev = pow2_exp(mv), eq = pow2_exp(mq);
  const float sk = exp2i(ek), sq = exp2i(eq);
  // ---- e4m3 images (values * 2^e stay <= 448: no saturation)
#pragma unroll
  for (int i = 0; i < UPT; ++i) {
    const int u = tid + i * NT, tv = u >> 9, a = (u >> 3) & 63, dc = u & 7;
    if (!tv) {
      const float ik = exp2i(-ek);
#pragma unroll
      for (int r = 0; r < 4; ++r) *(uint2*)(Ks + (4 * a + r) * F8V_KP + dc * 8) = f8_bf(ur[i][r], ik);
    } else {
      const float iv = exp2i(-ev);
      uint2 c[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) c[r] = f8_bf(ur[i][r], iv);
      uint32_t lo[4], hi[4];
      bt4(c[0].x, c[1].x, c[2].x, c[3].x, lo);  // d = 8 dc + 0..3
      bt4(c[0].y, c[1].y, c[2].y, c[3].y, hi);  // d = 8 dc + 4..7
      char* vcol = Vt + f8v_pos(4 * a);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        *(uint32_t*)(vcol + (8 * dc + e) * F8V_VP) = lo[e];
        *(uint32_t*)(vcol + (8 * dc + 4 + e) * F8V_VP) = hi[e];
      }
    }
  }
  long q8[2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) q8[s2] = __builtin_bit_cast(long, f8_bf(qb[s2], exp2i(-eq)));
  __syncthreads();

  const int nkt = FULL ? 16 : (N + 15) >> 4;
  const float c2 = scale * 1.4426950408889634f / (sq * sk);
  // S^T tiles: st[j][r] = raw score(key 16j + 4fq + r, query q)
  f32x4 st[F8_KMAX / 16];
  float mx = -INFINITY;
  const char* krow = Ks + frow * F8V_KP + 16 * fq;
#pragma unroll
  for (int j = 0; j < F8_KMAX / 16; ++j) {
    if (j < nkt) {
      const u32x4 kf = *(const u32x4*)(krow + 16 * j * F8V_KP);
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      a = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(__builtin_bit_cast(long, (uint2){kf[0], kf[1]}), q8[0], a, 0,
                                                     0, 0);
      a = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(__builtin_bit_cast(long, (uint2){kf[2], kf[3]}), q8[1], a, 0,
                                                     0, 0);
      v2_settle(a);  // (the MFMA result read on a taken branch edge)
      if (!FULL && 16 * j + 16 > N) {  // wave-uniform: only a partial last tile
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (16 * j + 4 * fq + r >= N) a[r] = -INFINITY;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, a[r]);
      st[j] = a;
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float mxs = mx * c2;  // c2 > 0: the max commutes with the scale
  const float off = 8.f - mxs;
  float sum = 0.f;  // of 256 P (unrounded, undropped)
#pragma unroll
  for (int j = 0; j < F8_KMAX / 16; ++j) {
    if (j < nkt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f(fmaf(st[j][r], c2, off));
        st[j][r] = p;
        sum += p;
      }
    }
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  f32x4 ot[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) ot[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const uint32_t rk = rng_key(seed, site);
  const uint64_t qrow = (bh * N + (qin ? q : 0)) * (uint64_t)N;
  const uint32_t hq = (uint32_t)(qrow >> 1) + 2u * (uint32_t)fq;
  unsigned long long kw = 0ull;  // this lane's keep-bit pair (one chunk)
  const char* vrow = Vt + frow * F8V_VP + 32 * fq;
#pragma unroll
  for (int kb = 0; kb < F8_KMAX / 128; ++kb) {
    if (FULL || 128 * kb < N) {
      i32x8 pb;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const int j = 8 * kb + m;
        f32x4 p = (j < nkt) ? st[j] : (f32x4){0.f, 0.f, 0.f, 0.f};
        if (thr && j < nkt) {
          // rng_pair(rk, qrow + 16j + 4fq) and (.. + 2): even terms, 32-bit pair index
          kw |= (unsigned long long)v2_keep_step(rk, hq + (uint32_t)(8 * j), thr, p) << kb_nibble(j);
        }
        pb[m] = f8x4_pos(p);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const char* vr = vrow + 16 * t * F8V_VP + 128 * kb;
        const u32x4 v0 = *(const u32x4*)vr, v1 = *(const u32x4*)(vr + 16);
        const i32x8 va = {(int)v0[0], (int)v0[1], (int)v0[2], (int)v0[3],
                          (int)v1[0], (int)v1[1], (int)v1[2], (int)v1[3]};
        // scale_a = 2^-ev (undo V's scale), scale_b = 2^0 (the normaliser is the sum of 256 P)
        ot[t] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(va, pb, ot[t], 0, 0, 0, 127 - ev, 0, 127);
      }
    }
  }
  if (qin) {
    const float inv = 1.f / sum;
    v2_store_row(o + ((long)b * N + q) * D + h * 64, ot, thr ? inv * dscale : inv, fq);
    if (fq == 0) lse[bh * N + q] = (mxs - 8.f + log2f(sum)) * 0.6931471805599453f;
    if (kbits && thr) *(uint2*)(kbits + kb_pair(0, 0, bh * N, q, fq)) = make_uint2((uint32_t)kw, (uint32_t)(kw >> 32));
  }
}

// 0: the round-4 kernel, 1: v2 with one 16-wave workgroup per (b, h), 2: v2 with
// two 8-wave workgroups per (b, h) (hvit_gemm_tune(5, v) for A/B)
int& fp8_form_ref() {
  static int v = 1;
  return v;
}

}  // namespace
}  // namespace hvit

using namespace hvit;

int hvit_fp8_tune(int value) {
  const int old = fp8_form_ref();
  fp8_form_ref() = value;
  return old;
}

extern "C" int hvit_mhsa_fwd_fp8_kb(const void* qkv, int B, int N, int H, int hd, float scale,
                                    const hvit_dropout_t* dropout, void* o, float* lse, unsigned* keep_bits,
                                    void* stream) {
  HVIT_CHECK(qkv && o && lse, "hvit_mhsa_fwd_fp8: null pointer");
  HVIT_CHECK(B > 0 && N > 0 && H > 0, "hvit_mhsa_fwd_fp8: bad shape B=%d N=%d H=%d", B, N, H);
  HVIT_CHECK(hd == 64, "hvit_mhsa_fwd_fp8: head_dim %d unsupported (64)", hd);
  HVIT_CHECK(N <= F8_KMAX, "hvit_mhsa_fwd_fp8: N=%d exceeds %d tokens", N, F8_KMAX);
  HVIT_CHECK(aligned16(qkv) && aligned16(o), "hvit_mhsa_fwd_fp8: qkv/o must be 16-byte aligned");
  HVIT_CHECK(!keep_bits || (((uintptr_t)keep_bits & 15) == 0 && N % 4 == 0),
             "hvit_mhsa_fwd_fp8: keep_bits alignment / N %% 4 (the bf16 backward's keep-bit layout)");
  // P is held as 256 * P * keep (0/1) in e4m3 (max 448), 1/(1-p) applied with
  // the normaliser: no saturation for any dropout p
  const DropArgs da = drop_args(dropout);
  const int form = fp8_form_ref();
  if (form == 1 || form == 2) {
    auto go = [&](auto kern, int waves) {
      hipLaunchKernelGGL(kern, dim3(cdiv(N, 16 * waves), H, B), dim3(64 * waves), 0, (hipStream_t)stream,
                         (const bf16_t*)qkv, (bf16_t*)o, lse, N, H, scale, da.thr, da.dscale, da.seed, da.site, keep_bits);
    };
    if (form == 2) N == 256 ? go(mhsa_fwd_fp8_v2<8, true>, 8) : go(mhsa_fwd_fp8_v2<8, false>, 8);
    else N == 256 ? go(mhsa_fwd_fp8_v2<16, true>, 16) : go(mhsa_fwd_fp8_v2<16, false>, 16);
  } else {
    // round 4: one 16-wave workgroup per (b, h) (measured faster than two 8-wave
    // ones at config 5's B*H = 192: 24.4 vs 26.4 us per layer)
    constexpr int WAVES = 16;
    hipLaunchKernelGGL(mhsa_fwd_fp8_kernel<WAVES>, dim3(cdiv(N, 16 * WAVES), H, B), dim3(64 * WAVES), 0,
                       (hipStream_t)stream, (const bf16_t*)qkv, (bf16_t*)o, lse, N, H, scale, da.thr, da.dscale,
                       da.seed, da.site, keep_bits);
  }
  HVIT_LAUNCH_CHECK();
  return HVIT_OK;
}

extern "C" int hvit_mhsa_fwd_fp8(const void* qkv, int B, int N, int H, int hd, float scale,
                                 const hvit_dropout_t* dropout, void* o, float* lse, void* stream) {
  return hvit_mhsa_fwd_fp8_kb(qkv, B, N, H, hd, scale, dropout, o, lse, nullptr, stream);
}
