// STFT / iSTFT framing around the model for gfx950 (librosa 0.10 semantics as
// restated in oracle/stft_restated.py: center=True, zero padding of n_fft/2,
// window centred in n_fft, T = 1 + len / hop), f32 arithmetic:
//  * stft_fwd: one workgroup per (sample, 16 consecutive frames).  The tile's
//    15*hop + n_fft samples are staged in LDS once; two real frames ride one
//    complex FFT (z = x_a + i x_b, split by Hermitian symmetry: no extra
//    twiddle), so a tile is 8 in-place radix-4 DIF FFTs in LDS, 32 lanes
//    each.  The (bit-reversed) result is read with the frame index fastest, so
//    every store covers runs of 16 frames (64 B of mag, 128 B of phasor)
//    along the T-contiguous outputs.
//  * spec_normalize: the per-utterance scaling, in place, from the min / max
//    the forward left in stats.
//  * istft: one workgroup per (sample, run of output hops).  It re-transforms
//    the (at most 16) frames that touch its run -- the halo frames included,
//    no partial sums cross workgroups -- with the same two-for-one packing run
//    backwards (DIT, natural-order output), then every output sample GATHERS
//    its frames in ascending order and divides by the window-square envelope
//    it accumulates beside them.  No float atomics: bit-identical run to run.
// Twiddles are rounded once from double sincospi into an LDS table laid out
// per stage (entry h + pos = exp(-i pi pos / h)), so every stage reads them
// contiguously.  FFT rows are padded by 2 complex words: the output pass reads
// 8 rows at one bin, and a power-of-two row stride would put them on one bank.
#include <float.h>

#include "common.h"

namespace hvit {

constexpr int FT_FRAMES = 16;  // frames per workgroup (8 two-for-one FFTs x 32 lanes = 256 threads)
constexpr int FT_PAIRS = FT_FRAMES / 2;
constexpr int FT_THREADS = 256;
constexpr int FT_ROWPAD = 2;

__device__ __forceinline__ float2 cmul(float2 a, float2 w) {
  return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

template <int LOGN>
__device__ __forceinline__ int brev(int k) {
  return (int)(__brev((unsigned)k) >> (32 - LOGN));
}

// tw[h + pos] = exp(-2 pi i pos / (2h)) for h = 1, 2, ..., N/2 and pos < h
template <int LOGN>
__device__ __forceinline__ void fill_twiddles(float2* tw) {
  constexpr int N = 1 << LOGN;
  for (int j = threadIdx.x; j < N; j += FT_THREADS) {
    float2 v = make_float2(1.f, 0.f);
    if (j > 0) {
      const int h = 1 << (31 - __clz(j));
      double s, c;
      sincospi(-(double)(j - h) / (double)h, &s, &c);
      v = make_float2((float)c, (float)s);
    }
    tw[j] = v;
  }
}

// In-place forward FFT of one row by 32 lanes, decimation in frequency:
// natural-order input, bit-reversed output.  Two radix-2 stages per pass.
template <int LOGN>
__device__ __forceinline__ void fft_dif(float2* z, const float2* tw, int l32) {
  constexpr int N = 1 << LOGN;
#pragma unroll
  for (int s = LOGN - 1; s >= 1; s -= 2) {  // stages h = 2q and h = q
    const int q = 1 << (s - 1);
    for (int i = l32; i < N / 4; i += 32) {
      const int pos = i & (q - 1);
      const int a = ((i >> (s - 1)) << (s + 1)) + pos;
      const float2 x0 = z[a], x1 = z[a + q], x2 = z[a + 2 * q], x3 = z[a + 3 * q];
      const float2 w0 = tw[2 * q + pos], w1 = tw[3 * q + pos], w2 = tw[q + pos];
      const float2 y0 = cadd(x0, x2), y2 = cmul(csub(x0, x2), w0);
      const float2 y1 = cadd(x1, x3), y3 = cmul(csub(x1, x3), w1);
      z[a] = cadd(y0, y1);
      z[a + q] = cmul(csub(y0, y1), w2);
      z[a + 2 * q] = cadd(y2, y3);
      z[a + 3 * q] = cmul(csub(y2, y3), w2);
    }
    __syncthreads();
  }
  if (LOGN & 1) {  // the last stage, h = 1 (twiddle 1)
    for (int i = l32; i < N / 2; i += 32) {
      const float2 u = z[2 * i], v = z[2 * i + 1];
      z[2 * i] = cadd(u, v);
      z[2 * i + 1] = csub(u, v);
    }
    __syncthreads();
  }
}

// The same transform, decimation in time: bit-reversed input, natural output.
template <int LOGN>
__device__ __forceinline__ void fft_dit(float2* z, const float2* tw, int l32) {
  constexpr int N = 1 << LOGN;
  if (LOGN & 1) {  // the first stage, h = 1
    for (int i = l32; i < N / 2; i += 32) {
      const float2 u = z[2 * i], v = z[2 * i + 1];
      z[2 * i] = cadd(u, v);
      z[2 * i + 1] = csub(u, v);
    }
    __syncthreads();
  }
#pragma unroll
  for (int s = LOGN & 1; s < LOGN; s += 2) {  // stages h = q and h = 2q
    const int q = 1 << s;
    for (int i = l32; i < N / 4; i += 32) {
      const int pos = i & (q - 1);
      const int a = ((i >> s) << (s + 2)) + pos;
      const float2 x0 = z[a], x1 = z[a + q], x2 = z[a + 2 * q], x3 = z[a + 3 * q];
      const float2 w0 = tw[2 * q + pos], w1 = tw[3 * q + pos], w2 = tw[q + pos];
      const float2 v1 = cmul(x1, w2), v3 = cmul(x3, w2);
      const float2 y0 = cadd(x0, v1), y1 = csub(x0, v1), y2 = cadd(x2, v3), y3 = csub(x2, v3);
      const float2 u2 = cmul(y2, w0), u3 = cmul(y3, w1);
      z[a] = cadd(y0, u2);
      z[a + 2 * q] = csub(y0, u2);
      z[a + q] = cadd(y1, u3);
      z[a + 3 * q] = csub(y1, u3);
    }
    __syncthreads();
  }
}

__device__ __forceinline__ int clamp_len(const int* lengths, int b, int L) {
  const int len = lengths ? lengths[b] : L;
  return len < 0 ? 0 : (len > L ? L : len);
}

__global__ void stft_stats_init_kernel(unsigned* stats, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 2 * B) stats[i] = (i & 1) ? 0u : 0x7f800000u;  // {min = +inf, max = 0}
}

// LDS: tw [N] float2 | z [8][N + 2] float2 | samples [15 * hop + N] float
template <int LOGN>
__global__ __launch_bounds__(FT_THREADS) void stft_fwd_kernel(const float* __restrict__ wave, long wave_stride,
                                                              const int* __restrict__ lengths, int L, int hop,
                                                              const float* __restrict__ window, int T,
                                                              float* __restrict__ mag, float2* __restrict__ phasor,
                                                              unsigned* __restrict__ stats) {
  constexpr int N = 1 << LOGN, F = N / 2 + 1, ZS = N + FT_ROWPAD;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float2* tw = (float2*)smem;
  float2* z = tw + N;
  float* smp = (float*)(z + FT_PAIRS * ZS);
  const int tid = threadIdx.x;
  const int b = blockIdx.y, t0 = blockIdx.x * FT_FRAMES;
  const int len = clamp_len(lengths, b, L);
  const int valid = 1 + len / hop;
  const size_t row0 = (size_t)b * F * T;

  if (t0 >= valid) {  // a tile of frames past the sample's length
    for (int e = tid; e < F * FT_FRAMES; e += FT_THREADS) {
      const int t = t0 + (e & (FT_FRAMES - 1)), f = e >> 4;
      if (t < T) {
        const size_t o = row0 + (size_t)f * T + t;
        mag[o] = 0.f;
        if (phasor) phasor[o] = make_float2(1.f, 0.f);
      }
    }
    return;
  }

  const int nS = (FT_FRAMES - 1) * hop + N;
  const int base = t0 * hop - N / 2;  // the sample index of smp[0]
  const float* src = wave + (size_t)b * wave_stride;
  for (int i = tid; i < nS; i += FT_THREADS) {
    const int idx = base + i;
    smp[i] = (idx >= 0 && idx < len) ? src[idx] : 0.f;
  }
  fill_twiddles<LOGN>(tw);
  __syncthreads();
  for (int n = tid; n < N; n += FT_THREADS) {
    const float w = window[n];
#pragma unroll
    for (int p = 0; p < FT_PAIRS; ++p) {  // a frame past the valid count rides as zeros: it is written as 0 below
      const float xa = t0 + 2 * p < valid ? smp[2 * p * hop + n] * w : 0.f;
      const float xb = t0 + 2 * p + 1 < valid ? smp[(2 * p + 1) * hop + n] * w : 0.f;
      z[p * ZS + n] = make_float2(xa, xb);
    }
  }
  __syncthreads();
  fft_dif<LOGN>(z + (tid >> 5) * ZS, tw, tid & 31);

  float lo = __uint_as_float(0x7f800000u), hi = 0.f;
  for (int e = tid; e < F * FT_FRAMES; e += FT_THREADS) {
    const int tl = e & (FT_FRAMES - 1), f = e >> 4;
    const int t = t0 + tl;
    if (t >= T) continue;
    float m = 0.f;
    float2 ph = make_float2(1.f, 0.f);
    if (t < valid) {
      const float2* zr = z + (tl >> 1) * ZS;
      const float2 u = zr[brev<LOGN>(f)], v = zr[brev<LOGN>((N - f) & (N - 1))];
      // X_a = (Z[k] + conj Z[N-k]) / 2, X_b = (Z[k] - conj Z[N-k]) / 2i
      const float re = (tl & 1) ? 0.5f * (u.y + v.y) : 0.5f * (u.x + v.x);
      const float im = (tl & 1) ? 0.5f * (v.x - u.x) : 0.5f * (u.y - v.y);
      m = hypotf(re, im);
      if (m > 0.f) ph = make_float2(re / m, im / m);
      lo = fminf(lo, m);
      hi = fmaxf(hi, m);
    }
    const size_t o = row0 + (size_t)f * T + t;
    mag[o] = m;
    if (phasor) phasor[o] = ph;
  }
  if (stats) {
    // min / max are order-independent: integer atomics on the bit image of the
    // non-negative floats stay deterministic.  One pair per workgroup (the
    // sample buffer is free by now): all tiles of a batch hit the same two
    // cache lines, and a pair per wave cost more than the rest of the kernel.
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = fminf(lo, __shfl_xor(lo, o, 64));
      hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((tid & 63) == 0) {
      smp[2 * (tid >> 6)] = lo;
      smp[2 * (tid >> 6) + 1] = hi;
    }
    __syncthreads();
    if (tid == 0) {
      lo = fminf(fminf(smp[0], smp[2]), fminf(smp[4], smp[6]));
      hi = fmaxf(fmaxf(smp[1], smp[3]), fmaxf(smp[5], smp[7]));
      atomicMin(stats + 2 * b, __float_as_uint(lo));
      atomicMax(stats + 2 * b + 1, __float_as_uint(hi));
    }
  }
}

__global__ __launch_bounds__(256) void spec_normalize_kernel(float* __restrict__ mag, int FT, int T,
                                                             const int* __restrict__ lengths, int hop,
                                                             const float* __restrict__ stats, int mode) {
  const int b = blockIdx.y;
  const float lo = stats[2 * b], hi = stats[2 * b + 1];
  if (mode == 0 ? !(hi > 1e-8f) : !(hi > lo)) return;
  const int valid = lengths ? 1 + max(lengths[b], 0) / hop : T;
  const float den = mode == 0 ? hi : hi - lo, sub = mode == 0 ? 0.f : lo;
  float* row = mag + (size_t)b * FT;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < FT; i += gridDim.x * blockDim.x) {
    if (i % T < valid) row[i] = (row[i] - sub) / den;
  }
}

// LDS: tw [N] float2 | z [8][N + 2] float2 | window [N] float
template <int LOGN>
__global__ __launch_bounds__(FT_THREADS) void istft_kernel(const float* __restrict__ mag,
                                                           const float2* __restrict__ phasor,
                                                           const float* __restrict__ gain,
                                                           const int* __restrict__ lengths, int T, int hop,
                                                           const float* __restrict__ window, int L, int run,
                                                           float* __restrict__ out) {
  constexpr int N = 1 << LOGN, F = N / 2 + 1, ZS = N + FT_ROWPAD;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float2* tw = (float2*)smem;
  float2* z = tw + N;
  float* win = (float*)(z + FT_PAIRS * ZS);
  const int tid = threadIdx.x;
  const int b = blockIdx.y, n0 = blockIdx.x * run;
  const int n1 = min(n0 + run, L);
  const int len = clamp_len(lengths, b, L);
  float* dst = out + (size_t)b * L;
  if (n0 >= len) {
    for (int n = n0 + tid; n < n1; n += FT_THREADS) dst[n] = 0.f;
    return;
  }
  const int nf = min(T, (len + N + hop - 1) / hop);  // frames the inverse uses
  const int m0 = n0 + N / 2;                         // padded index of the run's first sample
  const int t_lo = m0 - N + 1 <= 0 ? 0 : (m0 - N + hop) / hop;  // first frame with t * hop > m0 - N
  const float g = gain ? gain[b] : 1.f;
  const size_t row0 = (size_t)b * F * T;

  // Z = X_a + i X_b over all N bins (Hermitian extension), stored with re / im
  // swapped and bit-reversed: the forward DIT FFT of the swapped input is the
  // swapped inverse transform
  for (int e0 = 0; e0 < F * FT_FRAMES; e0 += FT_THREADS) {
    const int e = e0 + tid;
    const int tl = e & (FT_FRAMES - 1), f = e >> 4;
    const int t = t_lo + tl;
    float2 x = make_float2(0.f, 0.f);
    if (f < F && t < nf) {
      const size_t o = row0 + (size_t)f * T + t;
      const float m = g * mag[o];
      const float2 ph = phasor[o];
      x = make_float2(m * ph.x, (f == 0 || f == N / 2) ? 0.f : m * ph.y);  // irfft ignores those imaginary parts
    }
    const float2 y = make_float2(__shfl_xor(x.x, 1, 64), __shfl_xor(x.y, 1, 64));  // the pair's other frame
    if (f < F) {
      float2* zr = z + (tl >> 1) * ZS;
      if (!(tl & 1))  // Z[k] = (a - d, b + c)
        zr[brev<LOGN>(f)] = make_float2(x.y + y.x, x.x - y.y);
      else if (f > 0 && f < N / 2)  // Z[N - k] = (a + d, c - b)
        zr[brev<LOGN>(N - f)] = make_float2(x.x - y.y, y.x + x.y);
    }
  }
  for (int n = tid; n < N; n += FT_THREADS) win[n] = window[n];
  fill_twiddles<LOGN>(tw);
  __syncthreads();
  fft_dit<LOGN>(z + (tid >> 5) * ZS, tw, tid & 31);

  const int t_hi = min(nf - 1, t_lo + FT_FRAMES - 1);
  for (int n = n0 + tid; n < n1; n += FT_THREADS) {
    float y = 0.f;
    if (n < len) {
      const int m = n + N / 2;
      const int ta = max(t_lo, m - N + 1 <= 0 ? 0 : (m - N + hop) / hop), tb = min(t_hi, m / hop);
      float sum = 0.f, env = 0.f;
      for (int t = ta; t <= tb; ++t) {  // ascending frame order
        const int j = m - t * hop, r = t - t_lo;
        const float2 v = z[(r >> 1) * ZS + j];
        const float w = win[j];
        sum += ((r & 1) ? v.x : v.y) * w;
        env += w * w;
      }
      sum *= 1.f / (float)N;
      y = env > FLT_MIN ? sum / env : sum;
    }
    dst[n] = y;
  }
}

}  // namespace hvit

using namespace hvit;

template <typename K>
static void allow_lds(K kern, size_t bytes) {
  if (bytes > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

static int check_framing(const char* fn, int n_fft, int hop) {
  HVIT_CHECK(n_fft == 256 || n_fft == 512 || n_fft == 1024, "%s: n_fft=%d (supported: 256, 512, 1024)", fn, n_fft);
  HVIT_CHECK(hop * 8 >= n_fft && hop * 2 <= n_fft, "%s: hop=%d outside [n_fft/8, n_fft/2] for n_fft=%d", fn, hop,
             n_fft);
  return HVIT_OK;
}

int hvit_stft_fwd(const float* wave, long long wave_stride, const int* lengths, int B, int L, int n_fft, int hop,
                  const float* window, int T, float* mag, float* phasor, float* stats, void* stream) {
  HVIT_CHECK(wave && window && mag, "hvit_stft_fwd: null pointer");
  if (int rc = check_framing("hvit_stft_fwd", n_fft, hop)) return rc;
  HVIT_CHECK(B >= 1 && B <= 65535 && L >= 1 && wave_stride >= L, "hvit_stft_fwd: B=%d L=%d stride=%lld", B, L,
             wave_stride);
  HVIT_CHECK(T == 1 + L / hop, "hvit_stft_fwd: T=%d, expected 1 + L / hop = %d", T, 1 + L / hop);
  HVIT_CHECK((((uintptr_t)phasor) & 7) == 0, "hvit_stft_fwd: phasor must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (stats) {
    hipLaunchKernelGGL(stft_stats_init_kernel, dim3(cdiv(2 * B, 256)), dim3(256), 0, st, (unsigned*)stats, B);
    HVIT_LAUNCH_CHECK();
  }
  const size_t smem = sizeof(float2) * (n_fft + FT_PAIRS * (n_fft + FT_ROWPAD)) +
                      sizeof(float) * ((FT_FRAMES - 1) * hop + n_fft);
  const dim3 grid(cdiv(T, FT_FRAMES), B);
  auto go = [&](auto kern) {
    allow_lds(kern, smem);
    hipLaunchKernelGGL(kern, grid, dim3(FT_THREADS), smem, st, wave, (long)wave_stride, lengths, L, hop, window, T,
                       mag, (float2*)phasor, (unsigned*)stats);
  };
  if (n_fft == 256) go(stft_fwd_kernel<8>);
  else if (n_fft == 512) go(stft_fwd_kernel<9>);
  else go(stft_fwd_kernel<10>);
  HVIT_LAUNCH_CHECK();
  return HVIT_OK;
}

int hvit_spec_normalize(float* mag, int B, int F, int T, const int* lengths, int hop, const float* stats, int mode,
                        void* stream) {
  HVIT_CHECK(mag && stats, "hvit_spec_normalize: null pointer");
  HVIT_CHECK(mode == 0 || mode == 1, "hvit_spec_normalize: mode=%d (0 = max, 1 = min-max)", mode);
  HVIT_CHECK(B >= 1 && B <= 65535 && F >= 1 && T >= 1 && (long long)F * T < (1LL << 31),
             "hvit_spec_normalize: B=%d F=%d T=%d", B, F, T);
  HVIT_CHECK(!lengths || hop >= 1, "hvit_spec_normalize: hop=%d with lengths", hop);
  const int FT = F * T;
  const int bx = cdiv(FT, 256) < 64 ? cdiv(FT, 256) : 64;
  hipLaunchKernelGGL(spec_normalize_kernel, dim3(bx, B), dim3(256), 0, (hipStream_t)stream, mag, FT, T, lengths, hop,
                     stats, mode);
  HVIT_LAUNCH_CHECK();
  return HVIT_OK;
}

int hvit_istft(const float* mag, const float* phasor, const float* gain, const int* lengths, int B, int F, int T,
               int hop, const float* window, int L, float* wave_out, void* stream) {
  HVIT_CHECK(mag && phasor && window && wave_out, "hvit_istft: null pointer");
  const int n_fft = 2 * (F - 1);
  if (int rc = check_framing("hvit_istft", n_fft, hop)) return rc;
  HVIT_CHECK(B >= 1 && B <= 65535 && T >= 1 && L >= 1, "hvit_istft: B=%d T=%d L=%d", B, T, L);
  HVIT_CHECK((((uintptr_t)phasor) & 7) == 0, "hvit_istft: phasor must be 8-byte aligned");
  // a run of output hops whose frames (halo included) number at most 16:
  // the frames t with t * hop in (m0 - n_fft, m0 + run - 1] for a window of
  // run + n_fft - 1 positions are at most run / hop + ceil((n_fft - 1) / hop)
  const int run = (FT_FRAMES - 1 - cdiv(n_fft - 1, hop)) * hop;
  const size_t smem = sizeof(float2) * (n_fft + FT_PAIRS * (n_fft + FT_ROWPAD)) + sizeof(float) * n_fft;
  const dim3 grid(cdiv(L, run), B);
  auto go = [&](auto kern) {
    allow_lds(kern, smem);
    hipLaunchKernelGGL(kern, grid, dim3(FT_THREADS), smem, (hipStream_t)stream, mag, (const float2*)phasor, gain,
                       lengths, T, hop, window, L, run, wave_out);
  };
  if (n_fft == 256) go(istft_kernel<8>);
  else if (n_fft == 512) go(istft_kernel<9>);
  else go(istft_kernel<10>);
  HVIT_LAUNCH_CHECK();
  return HVIT_OK;
}
