// N consecutive elements of T (channels of an NHWC pixel, columns of a row)
// moved as one vector access and used as floats: the one definition of the
// bf16 unpack / pack that the kernels outside the GEMM main loops share
// (gemm_epilogue.h takes its pack functions from here).
//
// bf16 -> f32 is exact (the 16 bits become the high half of the float);
// f32 -> bf16 rounds to nearest even (f2bf2: one v_cvt_pk_bf16_f32 per pair).
#pragma once

#include <type_traits>

#include "common.h"

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// the two bf16 values of one 32-bit word: the lower address in the low half
__device__ __forceinline__ float bf_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }

// bf16 <-> f32 on 4 / 8 adjacent values (round to nearest even on the way down)
__device__ __forceinline__ uint2 pack4(const f32x4& v) {
  uint2 u;
  u.x = f2bf2(v[0], v[1]);
  u.y = f2bf2(v[2], v[3]);
  return u;
}
__device__ __forceinline__ f32x4 unpack4(uint32_t lo, uint32_t hi) {
  return (f32x4){__uint_as_float(lo << 16), __uint_as_float(lo & 0xffff0000u), __uint_as_float(hi << 16),
                 __uint_as_float(hi & 0xffff0000u)};
}
__device__ __forceinline__ f32x4 unpack4(const uint2& u) { return unpack4(u.x, u.y); }
__device__ __forceinline__ u32x4 pack8(const f32x4& a, const f32x4& b) {
  u32x4 u;
  u[0] = f2bf2(a[0], a[1]);
  u[1] = f2bf2(a[2], a[3]);
  u[2] = f2bf2(b[0], b[1]);
  u[3] = f2bf2(b[2], b[3]);
  return u;
}
__device__ __forceinline__ void unpack8(const u32x4& u, f32x4& a, f32x4& b) {
  a = unpack4(u[0], u[1]);
  b = unpack4(u[2], u[3]);
}

// N elements of T held raw in registers: load() issues the vector load and
// get() converts at the use, so a kernel can keep loads in flight ahead of the
// arithmetic without holding their floats.  p must be aligned to the vector
// (N * sizeof(T) bytes, at most 16).
template <typename T, int N>
struct ChanVec;

template <int N>
struct ChanVec<bf16_t, N> {  // u32x4 / u32x2 / uint32_t / bf16_t
  static_assert(N == 1 || N == 2 || N == 4 || N == 8, "bf16 vectors of 1, 2, 4 or 8");
  using Raw = std::conditional_t<N == 8, u32x4,
                                 std::conditional_t<N == 4, u32x2, std::conditional_t<N == 2, uint32_t, bf16_t>>>;
  Raw r;
  __device__ __forceinline__ void load(const bf16_t* p) { r = *(const Raw*)p; }
  __device__ __forceinline__ void zero() { r = Raw(0); }
  __device__ __forceinline__ void get(float* f) const {
    if constexpr (N >= 4) {
#pragma unroll
      for (int i = 0; i < N / 2; ++i) {
        f[2 * i] = bf_lo(r[i]);
        f[2 * i + 1] = bf_hi(r[i]);
      }
    } else if constexpr (N == 2) {
      f[0] = bf_lo(r);
      f[1] = bf_hi(r);
    } else {
      f[0] = bf2f(r);
    }
  }
  __device__ __forceinline__ float at(int e) const {  // element e alone (e a constant after unrolling)
    if constexpr (N >= 4) return (e & 1) ? bf_hi(r[e >> 1]) : bf_lo(r[e >> 1]);
    else if constexpr (N == 2) return (e & 1) ? bf_hi(r) : bf_lo(r);
    else return bf2f(r);
  }
  __device__ __forceinline__ static void store(bf16_t* p, const float* f) {
    if constexpr (N >= 4) {
      Raw o;
#pragma unroll
      for (int i = 0; i < N / 2; ++i) o[i] = f2bf2(f[2 * i], f[2 * i + 1]);
      *(Raw*)p = o;
    } else if constexpr (N == 2) {
      *(Raw*)p = f2bf2(f[0], f[1]);
    } else {
      *p = f2bf(f[0]);
    }
  }
};

template <int N>
struct ChanVec<float, N> {  // f32x4 x N/4, or N < 4 single floats
  static_assert(N % 4 == 0 || N < 4, "f32 vectors of 1, 2, 3 or a multiple of 4");
  using Raw = std::conditional_t<N % 4 == 0, f32x4, float>;
  static constexpr int NR = N % 4 == 0 ? N / 4 : N;
  Raw r[NR];
  __device__ __forceinline__ void load(const float* p) {
#pragma unroll
    for (int i = 0; i < NR; ++i) r[i] = ((const Raw*)p)[i];
  }
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < NR; ++i) r[i] = Raw(0.f);
  }
  __device__ __forceinline__ void get(float* f) const {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if constexpr (N % 4 == 0) f[i] = r[i / 4][i % 4];
      else f[i] = r[i];
    }
  }
  __device__ __forceinline__ float at(int e) const {
    if constexpr (N % 4 == 0) return r[e / 4][e % 4];
    else return r[e];
  }
  __device__ __forceinline__ static void store(float* p, const float* f) {
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      if constexpr (N % 4 == 0) ((f32x4*)p)[i] = (f32x4){f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]};
      else p[i] = f[i];
    }
  }
};

// load and convert in one step (the common case: the value is used at once)
template <int N, typename T>
__device__ __forceinline__ void load_chan(const T* p, float* f) {
  ChanVec<T, N> v;
  v.load(p);
  v.get(f);
}
template <int N, typename T>
__device__ __forceinline__ void store_chan(T* p, const float* f) {
  ChanVec<T, N>::store(p, f);
}
// 4 elements as one f32x4 (kernels whose arithmetic is on float vectors)
template <typename T>
__device__ __forceinline__ f32x4 load_chan4(const T* p) {
  float f[4];
  load_chan<4>(p, f);
  return (f32x4){f[0], f[1], f[2], f[3]};
}
