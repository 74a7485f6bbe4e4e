// Rational-ratio polyphase FIR resampling of a ragged f32 waveform batch for
// gfx950 (scipy.signal.resample_poly(x, up, down, window=taps,
// padtype="constant") semantics; include/hvit.h has the formula).
//
// One workgroup per (row, tile of WR_TILE consecutive outputs), one output per
// thread.  With pos = half + m * down (64 bits: at 441:160 it passes 2^31 after
// five minutes of audio), q = pos / up and p = pos % up, output m is
//   sum_j taps_pp[p][j] * wave[q - j]   over the j with p + j * up <= 2 * half
//                                       and 0 <= q - j < len,
// summed in ascending j with one fma per term: a fixed order, so results are
// bit-identical from run to run and a row's result does not depend on the
// batch.  The tile's input span wave[q(m0) - (J - 1) .. q(m_last)] is staged in
// LDS with coalesced loads (zeros outside [0, len): nothing at or past len is
// ever read).  Neighbouring outputs start down / up samples apart, so a wave's
// LDS reads are a small-stride sweep (a broadcast when up > down).  The taps
// come straight from the phase-major table: with up == 1 every lane reads the
// same word, with up > 1 each lane walks its own contiguous phase row; the
// 441:160 table (225 KB) stays in L2.
//
// peak[b] = max |out[b, :]|: a maximum is exact in any order, so one integer
// atomicMax per workgroup on the bit image of the non-negative float keeps it
// deterministic (no float atomics).
//
// The accumulator is f32 (hvit_wave_resample) or f64 (hvit_wave_resample_f64acc:
// every f32 x f32 product is exact in f64 and the sum is rounded to f32 once,
// for callers that measure in f64 downstream, native STOI).
#include "common.h"

namespace hvit {

constexpr int WR_TILE = 256;  // outputs per workgroup (resampler.TILE mirrors it)
constexpr int WR_THREADS = 256;
constexpr size_t WR_MAX_LDS = 160 * 1024;

__global__ void wave_resample_peak_init_kernel(unsigned* peak, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) peak[i] = 0u;
}

__device__ __forceinline__ float wr_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double wr_fma(float a, float b, double c) { return fma((double)a, (double)b, c); }

// LDS: span [<= (WR_TILE - 1) * down / up + 1 + J] float
template <typename Acc>
__global__ __launch_bounds__(WR_THREADS) void wave_resample_kernel(const float* __restrict__ wave, long wave_stride,
                                                                   const int* __restrict__ lengths, int L, int up,
                                                                   int down, const float* __restrict__ taps_pp,
                                                                   int half, int J, float* __restrict__ out,
                                                                   long out_stride, int L_out,
                                                                   unsigned* __restrict__ peak) {
  extern __shared__ __attribute__((aligned(16))) float span[];
  __shared__ float red[WR_THREADS / 64];
  const int tid = threadIdx.x;
  const int b = blockIdx.y, m0 = blockIdx.x * WR_TILE;
  int len = lengths ? lengths[b] : L;
  len = len < 0 ? 0 : (len > L ? L : len);
  const long lo_full = ((long)len * up + down - 1) / down;
  const int Lo = lo_full < (long)L_out ? (int)lo_full : L_out;
  float* orow = out + (size_t)b * out_stride;
  const int m = m0 + tid;

  if (m0 >= Lo) {  // a tile past the row's outputs: zeros, and peak keeps its 0
    if (m < L_out) orow[m] = 0.f;
    return;
  }

  const int m_last = (m0 + WR_TILE < Lo ? m0 + WR_TILE : Lo) - 1;
  const long kb = ((long)half + (long)m0 * down) / up - (J - 1);  // the sample index of span[0]
  const int nS = (int)(((long)half + (long)m_last * down) / up - kb) + 1;
  const float* src = wave + (size_t)b * wave_stride;
  for (int i = tid; i < nS; i += WR_THREADS) {
    const long idx = kb + i;
    span[i] = (idx >= 0 && idx < (long)len) ? src[idx] : 0.f;
  }
  __syncthreads();

  float res = 0.f;
  if (m < Lo) {
    const long pos = (long)half + (long)m * down;
    const long q = pos / up;
    const int p = (int)(pos - q * up);
    const long jt = (2L * half - p) / up;  // the phase row's last tap
    const int jhi = (int)(jt < q ? jt : q);
    const long jl = q - len + 1;
    const int jlo = jl > 0 ? (int)jl : 0;
    const float* h = taps_pp + (size_t)p * J;
    const float* x = span + (q - kb);
    Acc acc = 0;
    for (int j = jlo; j <= jhi; ++j) acc = wr_fma(h[j], x[-j], acc);
    res = (float)acc;
    orow[m] = res;
  } else if (m < L_out) {
    orow[m] = 0.f;
  }

  if (peak) {
    const float v = wave_max(fabsf(res));
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
      float hi = red[0];
#pragma unroll
      for (int w = 1; w < WR_THREADS / 64; ++w) hi = fmaxf(hi, red[w]);
      atomicMax(peak + b, __float_as_uint(hi));
    }
  }
}

}  // namespace hvit

using namespace hvit;

static long long wr_gcd(long long a, long long b) {
  while (b) {
    const long long t = a % b;
    a = b;
    b = t;
  }
  return a;
}

long long hvit_wave_resample_out_len(long long len, int up, int down) {
  if (len < 1 || up < 1 || down < 1) return 0;
  return (len * up + down - 1) / down;
}

template <typename Acc>
static int wave_resample(const float* wave, long long wave_stride, const int* lengths, int B, int L, int up, int down,
                         const float* taps_pp, int half, float* out, long long out_stride, int L_out, float* peak,
                         void* stream) {
  HVIT_CHECK(wave && taps_pp && out, "hvit_wave_resample: null pointer");
  HVIT_CHECK(B >= 1 && B <= 65535 && L >= 1 && wave_stride >= L, "hvit_wave_resample: B=%d L=%d stride=%lld", B, L,
             wave_stride);
  HVIT_CHECK(up >= 1 && down >= 1, "hvit_wave_resample: up=%d down=%d (both must be >= 1)", up, down);
  HVIT_CHECK(wr_gcd(up, down) == 1, "hvit_wave_resample: up=%d and down=%d are not coprime", up, down);
  HVIT_CHECK(half >= 1 && half < (1 << 29), "hvit_wave_resample: half=%d", half);
  HVIT_CHECK(L_out >= 1 && out_stride >= L_out, "hvit_wave_resample: L_out=%d out_stride=%lld", L_out, out_stride);
  const long long need = hvit_wave_resample_out_len(L, up, down);
  HVIT_CHECK(lengths || L_out >= need, "hvit_wave_resample: L_out=%d below the %lld outputs of L=%d at %d:%d", L_out,
             need, L, up, down);
  const int J = (int)((2LL * half + up) / up);  // ceil((2 * half + 1) / up)
  const size_t smem = sizeof(float) * ((size_t)(WR_TILE - 1) * down / up + 2 + J);
  HVIT_CHECK(smem <= WR_MAX_LDS, "hvit_wave_resample: a tile's input span at %d:%d with half=%d needs %zu bytes of LDS",
             up, down, half, smem);
  hipStream_t st = (hipStream_t)stream;
  if (peak) {
    hipLaunchKernelGGL(wave_resample_peak_init_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, (unsigned*)peak, B);
    HVIT_LAUNCH_CHECK();
  }
  if (smem > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)wave_resample_kernel<Acc>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)smem);
  hipLaunchKernelGGL(wave_resample_kernel<Acc>, dim3(cdiv(L_out, WR_TILE), B), dim3(WR_THREADS), smem, st, wave,
                     (long)wave_stride, lengths, L, up, down, taps_pp, half, J, out, (long)out_stride, L_out,
                     (unsigned*)peak);
  HVIT_LAUNCH_CHECK();
  return HVIT_OK;
}

int hvit_wave_resample(const float* wave, long long wave_stride, const int* lengths, int B, int L, int up, int down,
                       const float* taps_pp, int half, float* out, long long out_stride, int L_out, float* peak,
                       void* stream) {
  return wave_resample<float>(wave, wave_stride, lengths, B, L, up, down, taps_pp, half, out, out_stride, L_out, peak,
                              stream);
}

int hvit_wave_resample_f64acc(const float* wave, long long wave_stride, const int* lengths, int B, int L, int up,
                              int down, const float* taps_pp, int half, float* out, long long out_stride, int L_out,
                              float* peak, void* stream) {
  return wave_resample<double>(wave, wave_stride, lengths, B, L, up, down, taps_pp, half, out, out_stride, L_out,
                               peak, stream);
}
