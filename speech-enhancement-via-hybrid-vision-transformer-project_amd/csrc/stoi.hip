// Short-time objective intelligibility (Taal et al. 2011, non-extended; the
// definition of DESIGN §18 and metrics.py: stoi_reference) of ragged 10 kHz
// batches on gfx950.  Samples are f32; every product, transform, sum, log and
// square root is f64.  Row b is x[b, :len_b] and nothing at or past len_b is
// loaded.  The number K of frames a row keeps is known on the device only, so
// the workspace and the grids are sized for "every frame kept" and a
// workgroup reads its row's count and leaves when it has nothing to do.
//  * stoi_tables: the window hanning(258)[1:-1] and the 512 twiddles
//    (cos, sin)(2 pi j / 512), in f64, into the workspace: once per call.
//  * stoi_energy: one wave per full frame of the clean row: e_j = 20 log10(
//    |w x_j| + EPS).
//  * stoi_compact: one workgroup per row: the row's maximum, the mask e_j >
//    max - 40, a per-thread count over a contiguous run of frames, its
//    exclusive prefix, and map[i] = source frame of kept frame i written by the
//    run's owner; K.
//  * stoi_bands: one workgroup per kept frame m, both signals: the two
//    128-sample blocks m and m + 1 of the overlap-added signal, each the sum of
//    at most two windowed halves (of the kept frames m - 1, m, m + 1), windowed
//    again in LDS; a direct DFT of bins 7 .. 218 (one bin per thread, the
//    twiddles from an LDS table); the 15 band sums in ascending bin order.
//    A direct DFT is 256 x 212 complex terms per frame and signal, about 2 G
//    f64 fma for 32 clips of 4 s (a floor of about 56 us at 78.6 TFLOP/s of
//    vector f64).  An LDS FFT would need a tenth of the arithmetic but nine
//    barrier-separated passes, and only 212 of 257 bins are wanted; the two
//    were not measured against each other.
//  * stoi_segments: one thread per (segment, band) over its 30 band values,
//    then the 15 bands of a segment added in ascending order.
//  * stoi_finish: the row's segment sums in wave_finish's fixed order, over
//    15 (K - 29); 1e-5 where K < 30.
// No float atomics: results are bit-identical from run to run and do not
// depend on which other rows share the batch, on L or on the strides.
#include "wave_f64.h"

namespace hvit {

constexpr int ST_FRAME = 256, ST_HOP = 128, ST_NFFT = 512, ST_BANDS = 15, ST_SEG = 30;
constexpr int ST_K0 = 7, ST_BINS = 212;  // bins 7 .. 218
constexpr int ST_THREADS = 256;
constexpr int ST_TAB = ST_FRAME + 2 * ST_NFFT;  // doubles: the window, then (cos, sin) per twiddle
constexpr int ST_SEGS = 16;                     // segments per workgroup of stoi_segments
constexpr double ST_EPS = 2.220446049250313e-16;  // numpy.finfo(float).eps
constexpr double ST_DYN = 40.0;
constexpr double ST_CLIP = 6.623413251903491;  // 1 + 10^(15 / 20)
constexpr double ST_SHORT = 1e-5;
__device__ const int ST_EDGE[ST_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

__host__ __device__ inline int stoi_frames(int len) {
  return len < ST_FRAME ? 0 : (len - ST_FRAME) / ST_HOP + 1;
}

// the workspace, in doubles (T = stoi_frames(L), S = max(T - 29, 0)):
//   tab [ST_TAB] | energy [B, T] | tob [2, B, 15, T] | segsum [B, S] | map int [B, T] | count int [B]
struct StoiWs {
  double *tab, *energy, *tob, *segsum;
  int *map, *count;
  int T, S;
  long long elems;
};
static StoiWs stoi_ws(double* ws, int B, int L) {
  StoiWs w;
  w.T = stoi_frames(L);
  w.S = w.T >= ST_SEG ? w.T - ST_SEG + 1 : 0;
  const long long bt = (long long)B * w.T;
  w.tab = ws;
  w.energy = w.tab + ST_TAB;
  w.tob = w.energy + bt;
  w.segsum = w.tob + 2 * ST_BANDS * bt;
  double* ints = w.segsum + (long long)B * w.S;
  w.map = (int*)ints;
  w.count = (int*)(ints + (bt + 1) / 2);
  w.elems = ST_TAB + (1 + 2 * ST_BANDS) * bt + (long long)B * w.S + (bt + 1) / 2 + ((long long)B + 1) / 2;
  return w;
}

__global__ __launch_bounds__(ST_THREADS) void stoi_tables_kernel(double* __restrict__ tab) {
  const int i = blockIdx.x * ST_THREADS + threadIdx.x;
  if (i < ST_FRAME) {
    tab[i] = 0.5 + 0.5 * cospi((2.0 * i - 255.0) / 257.0);  // numpy.hanning(258)[1 + i]
  } else if (i < ST_FRAME + ST_NFFT) {
    const int j = i - ST_FRAME;
    double s, c;
    sincospi((double)j / 256.0, &s, &c);
    tab[ST_FRAME + 2 * j] = c;
    tab[ST_FRAME + 2 * j + 1] = s;
  }
}

// grid (cdiv(T, 4), B): wave v of a workgroup owns frame 4 blockIdx.x + v; lane l takes samples l, l + 64, ...
__global__ __launch_bounds__(ST_THREADS) void stoi_energy_kernel(const float* __restrict__ clean, long clean_stride,
                                                                 const int* __restrict__ lengths, int L, int T,
                                                                 const double* __restrict__ tab,
                                                                 double* __restrict__ energy) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int j = blockIdx.x * (ST_THREADS / 64) + (threadIdx.x >> 6);
  if (j >= stoi_frames(row_len(lengths, b, L))) return;  // a full frame: 128 j + 256 <= len_b
  const float* c = clean + (size_t)b * clean_stride + (size_t)j * ST_HOP;
  double s = 0;
#pragma unroll
  for (int u = 0; u < ST_FRAME / 64; ++u) {
    const int n = lane + 64 * u;
    const double v = tab[n] * (double)c[n];
    s = fma(v, v, s);
  }
  s = wave_sum_f64(s);
  if (lane == 0) energy[(size_t)b * T + j] = 20.0 * log10(sqrt(s) + ST_EPS);
}

// grid B: thread t owns the frames [t per, (t + 1) per) of the row, per = cdiv(frames, 256)
__global__ __launch_bounds__(ST_THREADS) void stoi_compact_kernel(const int* __restrict__ lengths, int L, int T,
                                                                  const double* __restrict__ energy,
                                                                  int* __restrict__ map, int* __restrict__ count) {
  __shared__ double mx[ST_THREADS];
  __shared__ int cnt[ST_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nf = stoi_frames(row_len(lengths, b, L));
  const int per = (nf + ST_THREADS - 1) / ST_THREADS;
  const int j0 = tid * per < nf ? tid * per : nf, j1 = j0 + per < nf ? j0 + per : nf;
  const double* e = energy + (size_t)b * T;
  double m = -INFINITY;
  for (int j = j0; j < j1; ++j) m = fmax(m, e[j]);
  mx[tid] = m;
  __syncthreads();
  for (int o = ST_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) mx[tid] = fmax(mx[tid], mx[tid + o]);
    __syncthreads();
  }
  const double thr = mx[0] - ST_DYN;
  int k = 0;
  for (int j = j0; j < j1; ++j) k += e[j] > thr;
  cnt[tid] = k;
  __syncthreads();
  int off = 0, total = 0;
  for (int i = 0; i < ST_THREADS; ++i) {
    off += i < tid ? cnt[i] : 0;
    total += cnt[i];
  }
  int* mp = map + (size_t)b * T;
  for (int j = j0; j < j1; ++j) {
    if (e[j] > thr) mp[off++] = j;
  }
  if (tid == 0) count[b] = total;
}

// grid (T, B): kept frame m of row b
__global__ __launch_bounds__(ST_THREADS) void stoi_bands_kernel(const float* __restrict__ clean, long clean_stride,
                                                                const float* __restrict__ est, long est_stride,
                                                                int B, int T, const double* __restrict__ tab,
                                                                const int* __restrict__ map,
                                                                const int* __restrict__ count,
                                                                double* __restrict__ tob) {
  __shared__ double2 tw[ST_NFFT];
  __shared__ double xs[ST_FRAME], ys[ST_FRAME];
  __shared__ double pw[2][ST_BINS];
  const int b = blockIdx.y, m = blockIdx.x, tid = threadIdx.x;
  const int K = count[b];
  if (K < ST_SEG || m >= K) return;  // K < 30 scores 1e-5 whatever the bands hold
  const double* twg = tab + ST_FRAME;  // 8-byte aligned only: two loads per twiddle
  tw[tid] = make_double2(twg[2 * tid], twg[2 * tid + 1]);
  tw[tid + ST_THREADS] = make_double2(twg[2 * (tid + ST_THREADS)], twg[2 * (tid + ST_THREADS) + 1]);
  {
    // sample tid of the rebuilt frame m lies in block q = m + (tid >> 7) of the overlap-added signal: the
    // second half of kept frame q - 1 plus the first half of kept frame q, where they exist
    const int q = m + (tid >> 7), r = tid & (ST_HOP - 1);
    const int* mp = map + (size_t)b * T;
    const float* c = clean + (size_t)b * clean_stride;
    const float* e = est + (size_t)b * est_stride;
    double vx = 0, vy = 0;
    if (q >= 1) {
      const size_t i = (size_t)mp[q - 1] * ST_HOP + ST_HOP + r;
      const double w = tab[ST_HOP + r];
      vx = w * (double)c[i];
      vy = w * (double)e[i];
    }
    if (q < K) {
      const size_t i = (size_t)mp[q] * ST_HOP + r;
      const double w = tab[r];
      vx += w * (double)c[i];
      vy += w * (double)e[i];
    }
    xs[tid] = tab[tid] * vx;
    ys[tid] = tab[tid] * vy;
  }
  __syncthreads();
  if (tid < ST_BINS) {
    const int k = ST_K0 + tid;
    double xr = 0, xi = 0, yr = 0, yi = 0;
    int idx = 0;
#pragma unroll 4
    for (int n = 0; n < ST_FRAME; ++n) {
      const double2 t = tw[idx];
      const double x = xs[n], y = ys[n];
      xr = fma(x, t.x, xr);
      xi = fma(x, t.y, xi);
      yr = fma(y, t.x, yr);
      yi = fma(y, t.y, yi);
      idx = (idx + k) & (ST_NFFT - 1);
    }
    pw[0][tid] = xr * xr + xi * xi;
    pw[1][tid] = yr * yr + yi * yi;
  }
  __syncthreads();
  if (tid < 2 * ST_BANDS) {
    const int sig = tid / ST_BANDS, band = tid - sig * ST_BANDS;
    double s = 0;
    for (int k = ST_EDGE[band]; k < ST_EDGE[band + 1]; ++k) s += pw[sig][k - ST_K0];
    tob[(((size_t)sig * B + b) * ST_BANDS + band) * T + m] = sqrt(s);
  }
}

// grid (cdiv(S, 16), B), 256 threads = 16 segments (fastest: T is contiguous) x 16 bands, the last idle
__global__ __launch_bounds__(ST_THREADS) void stoi_segments_kernel(int B, int T, int S,
                                                                   const double* __restrict__ tob,
                                                                   const int* __restrict__ count,
                                                                   double* __restrict__ segsum) {
  __shared__ double part[ST_BANDS][ST_SEGS];
  const int b = blockIdx.y, s0 = blockIdx.x * ST_SEGS;
  const int nseg = count[b] - ST_SEG + 1;
  if (s0 >= nseg) return;  // covers K < 30
  const int sl = threadIdx.x & (ST_SEGS - 1), band = threadIdx.x >> 4;
  const int seg = s0 + sl;
  if (band < ST_BANDS) {
    double d = 0;
    if (seg < nseg) {  // frames seg .. seg + 29 < K
      const double* px = tob + (((size_t)b) * ST_BANDS + band) * T + seg;
      const double* py = tob + (((size_t)B + b) * ST_BANDS + band) * T + seg;
      double x[ST_SEG], y[ST_SEG];
      double sxx = 0, syy = 0;
#pragma unroll
      for (int i = 0; i < ST_SEG; ++i) {
        x[i] = px[i];
        y[i] = py[i];
        sxx = fma(x[i], x[i], sxx);
        syy = fma(y[i], y[i], syy);
      }
      const double alpha = sqrt(sxx) / (sqrt(syy) + ST_EPS);
      double sx = 0, sy = 0;
#pragma unroll
      for (int i = 0; i < ST_SEG; ++i) {
        y[i] = fmin(alpha * y[i], x[i] * ST_CLIP);
        sx += x[i];
        sy += y[i];
      }
      const double mx = sx / ST_SEG, my = sy / ST_SEG;
      double cxx = 0, cyy = 0, cxy = 0;
#pragma unroll
      for (int i = 0; i < ST_SEG; ++i) {
        const double a = x[i] - mx, c = y[i] - my;
        cxx = fma(a, a, cxx);
        cyy = fma(c, c, cyy);
        cxy = fma(a, c, cxy);
      }
      d = cxy / ((sqrt(cxx) + ST_EPS) * (sqrt(cyy) + ST_EPS));
    }
    part[band][sl] = d;
  }
  __syncthreads();
  if (band == 0 && seg < nseg) {
    double tot = 0;
#pragma unroll
    for (int q = 0; q < ST_BANDS; ++q) tot += part[q][sl];
    segsum[(size_t)b * S + seg] = tot;
  }
}

__global__ __launch_bounds__(ST_THREADS) void stoi_finish_kernel(int S, const double* __restrict__ segsum,
                                                                 const int* __restrict__ count,
                                                                 double* __restrict__ out) {
  __shared__ double red[ST_THREADS / 64];
  const int b = blockIdx.x;
  const int nseg = count[b] - ST_SEG + 1;
  double s = 0;
  for (int q = threadIdx.x; q < nseg; q += ST_THREADS) s += segsum[(size_t)b * S + q];  // nseg <= S
  s = block_sum_f64(s, red);
  if (threadIdx.x == 0) out[b] = nseg < 1 ? ST_SHORT : s / ((double)ST_BANDS * (double)nseg);
}

}  // namespace hvit

using namespace hvit;

long long hvit_stoi_ws_elems(int B, int L) {
  if (B < 1 || L < 1) return 0;
  return stoi_ws(nullptr, B, L).elems;
}

int hvit_stoi(const float* clean, long long clean_stride, const float* est, long long est_stride, const int* lengths,
              int B, int L, double* ws, long long ws_elems, double* out, void* stream) {
  HVIT_CHECK(clean && est && ws && out, "hvit_stoi: null pointer");
  HVIT_CHECK(B >= 1 && B <= 65535 && L >= 1, "hvit_stoi: B=%d L=%d", B, L);
  HVIT_CHECK(B == 1 || (clean_stride >= L && est_stride >= L), "hvit_stoi: row strides %lld / %lld < L=%d",
             clean_stride, est_stride, L);
  HVIT_CHECK(ws_elems >= hvit_stoi_ws_elems(B, L), "hvit_stoi: workspace %lld < %lld doubles", ws_elems,
             hvit_stoi_ws_elems(B, L));
  HVIT_CHECK(((((uintptr_t)ws) | ((uintptr_t)out)) & 7) == 0, "hvit_stoi: ws / out must be 8-byte aligned");
  const StoiWs w = stoi_ws(ws, B, L);
  hipStream_t st = (hipStream_t)stream;
  if (w.T > 0) {
    hipLaunchKernelGGL(stoi_tables_kernel, dim3(cdiv(ST_FRAME + ST_NFFT, ST_THREADS)), dim3(ST_THREADS), 0, st, w.tab);
    HVIT_LAUNCH_CHECK();
    hipLaunchKernelGGL(stoi_energy_kernel, dim3(cdiv(w.T, ST_THREADS / 64), B), dim3(ST_THREADS), 0, st, clean,
                       (long)clean_stride, lengths, L, w.T, (const double*)w.tab, w.energy);
    HVIT_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(stoi_compact_kernel, dim3(B), dim3(ST_THREADS), 0, st, lengths, L, w.T,
                     (const double*)w.energy, w.map, w.count);
  HVIT_LAUNCH_CHECK();
  if (w.S > 0) {
    hipLaunchKernelGGL(stoi_bands_kernel, dim3(w.T, B), dim3(ST_THREADS), 0, st, clean, (long)clean_stride, est,
                       (long)est_stride, B, w.T, (const double*)w.tab, (const int*)w.map, (const int*)w.count, w.tob);
    HVIT_LAUNCH_CHECK();
    hipLaunchKernelGGL(stoi_segments_kernel, dim3(cdiv(w.S, ST_SEGS), B), dim3(ST_THREADS), 0, st, B, w.T, w.S,
                       (const double*)w.tob, (const int*)w.count, w.segsum);
    HVIT_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(stoi_finish_kernel, dim3(B), dim3(ST_THREADS), 0, st, w.S, (const double*)w.segsum,
                     (const int*)w.count, out);
  HVIT_LAUNCH_CHECK();
  return HVIT_OK;
}
