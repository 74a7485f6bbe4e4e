// Speech quality metrics on the device for gfx950 (the definitions of the
// reference's evaluation/metrics.py:100-296: SI-SDR, SNR, segmental SNR, LSD).
// Inputs are f32, every sum and every log is f64, results are f64.  Rows are
// ragged: row b is x[b, :len_b] and nothing past len_b is ever loaded.
//  * wave_chunks: grid (chunks, B); a workgroup owns WM_CHUNK consecutive
//    hop-sized blocks of one row, one block per wave at a time, and writes
//    seven doubles: the row moments of c and d = e - c over its blocks (sum c,
//    d, c^2, d^2, d c) and the sum and count of the clipped SegSNR values of
//    the frames that START in it.  A frame is frame / hop consecutive blocks,
//    so the workgroup also reads the frame / hop - 1 blocks after its own (1
//    in 16 at the reference's 512 / 256, mostly L2 hits) for their sums c^2
//    and d^2: the long log10 chain of a frame runs where its samples were
//    read, on every CU, and no per-block array crosses HBM.  Lane l of a wave
//    owns elements 4l .. 4l + 3 of every 256-element stripe of a block,
//    whether they arrive as one 16-byte load or as scalars, so a sum's order
//    depends on the position in the row alone: not on alignment, stride, the
//    batch or L.
//  * wave_finish: one workgroup per row adds the chunk records (thread i
//    takes chunks i, i + 256, ... in ascending order, then a fixed tree) and
//    forms the three dB figures.
//  * lsd_frames / lsd_finish: sqrt(mean_f (log(a + eps) - log(b + eps))^2) per
//    valid frame (16 frames x 16 bin slices per workgroup, the slices added in
//    ascending order), then the same fixed-order mean over the frames.
// No float atomics anywhere: results are bit-identical from run to run and do
// not depend on which other rows share the batch.
#include "wave_f64.h"

namespace hvit {

constexpr int WM_THREADS = 256;
constexpr int WM_WAVES = WM_THREADS / 64;
constexpr int WM_CHUNK = 16;    // hop blocks per workgroup (4 per wave; one per wave in a 16-wave workgroup
                                // measured slower: 15.4 against 12.4 us at 32 x 64000, 48 against 30 us at 1 x 9.6 M)
constexpr int WM_STRIPE = 256;  // elements one wave covers per step (64 lanes x 4)
constexpr int WM_MOM = 5;       // moments per chunk: sum c, d, c^2, d^2, d c with d = e - c
constexpr int WM_PART = WM_MOM + 2;  // doubles per chunk: the moments, then the SegSNR sum and count of its frames
constexpr int WM_MAX_RATIO = 16;     // largest seg_frame / seg_hop
constexpr int LSD_FRAMES = 16;  // frames per workgroup
constexpr int LSD_SLICES = 16;  // bin slices per workgroup

// LDS: the block sums {sum c^2, sum d^2} of the chunk's own blocks and of the WM_MAX_RATIO - 1 that follow
__global__ __launch_bounds__(WM_THREADS) void wave_chunks_kernel(const float* __restrict__ clean, long clean_stride,
                                                                 const float* __restrict__ est, long est_stride,
                                                                 const int* __restrict__ lengths, int L, int hop,
                                                                 int frame, double eps, int nchunk,
                                                                 double* __restrict__ ws) {
  __shared__ double blk[WM_CHUNK + WM_MAX_RATIO - 1][2];
  __shared__ double red[WM_WAVES][WM_MOM];
  __shared__ double val[WM_CHUNK][2];  // a frame's clipped value and 1, or {0, 0} where it does not count
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int len = row_len(lengths, b, L);
  const long first = (long)chunk * WM_CHUNK * hop;  // the chunk's first sample
  if (first >= len) return;                         // wave_finish reads no chunk past the row
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* c = clean + (size_t)b * clean_stride;
  const float* e = est + (size_t)b * est_stride;
  // 16-byte loads need both rows and every block start on a 16-byte boundary
  const bool vec = ((((uintptr_t)c) | ((uintptr_t)e)) & 15) == 0 && (hop & 3) == 0;
  const int r = frame / hop;  // blocks per SegSNR frame

  // per lane, over the wave's own blocks.  All five in one order: est == 0 gives sd == -sc and sdc == -scc,
  // est == clean gives sd == sdd == sdc == 0, bit for bit; wave_finish's -inf and est == clean values rest on it
  double sc = 0, sd = 0, scc = 0, sdd = 0, sdc = 0;
  for (int j = wave; j < WM_CHUNK + r - 1; j += WM_WAVES) {
    const long s0 = ((long)chunk * WM_CHUNK + j) * hop;
    if (s0 >= len) break;
    const int blen = (int)(len - s0 < hop ? len - s0 : hop);
    const float* cb = c + s0;
    const float* eb = e + s0;
    double pc = 0, pd = 0, pcc = 0, pdd = 0, pdc = 0;
    for (int i = 4 * lane; i < blen; i += WM_STRIPE) {
      float cv[4] = {0.f, 0.f, 0.f, 0.f}, ev[4] = {0.f, 0.f, 0.f, 0.f};
      if (vec && i + 3 < blen) {
        const float4 c4 = *(const float4*)(cb + i), e4 = *(const float4*)(eb + i);
        cv[0] = c4.x, cv[1] = c4.y, cv[2] = c4.z, cv[3] = c4.w;
        ev[0] = e4.x, ev[1] = e4.y, ev[2] = e4.z, ev[3] = e4.w;
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (i + u < blen) {
            cv[u] = cb[i + u];
            ev[u] = eb[i + u];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {  // an element past the block rides as (0, 0): it adds +0.0 to every sum
        const double x = (double)cv[u], y = (double)ev[u], d = y - x;
        pc += x;
        pd += d;
        pcc = fma(x, x, pcc);
        pdd = fma(d, d, pdd);
        pdc = fma(d, x, pdc);
      }
    }
    if (j < WM_CHUNK) {  // a block of the next chunk is read for its frame sums only
      sc += pc, sd += pd, scc += pcc, sdd += pdd, sdc += pdc;
    }
    pcc = wave_sum_f64(pcc);
    pdd = wave_sum_f64(pdd);
    if (lane == 0) blk[j][0] = pcc, blk[j][1] = pdd;
  }
  sc = wave_sum_f64(sc);
  sd = wave_sum_f64(sd);
  scc = wave_sum_f64(scc);
  sdd = wave_sum_f64(sdd);
  sdc = wave_sum_f64(sdc);
  if (lane == 0) {
    double* w = red[wave];
    w[0] = sc, w[1] = sd, w[2] = scc, w[3] = sdd, w[4] = sdc;
  }
  __syncthreads();
  // the frames that start in this chunk: frame f covers blocks f .. f + r - 1, all whole and inside the row
  // exactly when f * hop + frame < len (the reference's exclusive bound)
  if (threadIdx.x < WM_CHUNK) {
    const int j = threadIdx.x;
    double v = 0.0, counts = 0.0;
    if (((long)chunk * WM_CHUNK + j) * hop + frame < len) {
      double pcc = 0, pdd = 0;
      for (int k = j; k < j + r; ++k) pcc += blk[k][0], pdd += blk[k][1];
      pcc /= (double)frame;
      pdd /= (double)frame;
      if (pcc > eps && pdd > eps) {
        v = 10.0 * log10(pcc / pdd);
        v = v < -10.0 ? -10.0 : (v > 35.0 ? 35.0 : v);
        counts = 1.0;
      }
    }
    val[j][0] = v;
    val[j][1] = counts;
  }
  __syncthreads();
  double* o = ws + ((size_t)b * nchunk + chunk) * WM_PART;
  if (threadIdx.x < WM_MOM) {
    const int m = threadIdx.x;
    o[m] = ((red[0][m] + red[1][m]) + red[2][m]) + red[3][m];
  } else if (threadIdx.x == WM_MOM) {
    double seg = 0, cnt = 0;
    for (int j = 0; j < WM_CHUNK; ++j) seg += val[j][0], cnt += val[j][1];
    o[WM_MOM] = seg;
    o[WM_MOM + 1] = cnt;
  }
}

__global__ __launch_bounds__(WM_THREADS) void wave_finish_kernel(const int* __restrict__ lengths, int L, int hop,
                                                                 double eps, int nchunk,
                                                                 const double* __restrict__ ws,
                                                                 double* __restrict__ out) {
  __shared__ double red[WM_WAVES][WM_PART];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = row_len(lengths, b, L);
  const int chunks = (int)(((long)len + (long)WM_CHUNK * hop - 1) / ((long)WM_CHUNK * hop));
  double p[WM_PART];
#pragma unroll
  for (int m = 0; m < WM_PART; ++m) p[m] = 0;
  for (int q = tid; q < chunks; q += WM_THREADS) {  // thread i takes chunks i, i + 256, ... in ascending order
    const double* w = ws + ((size_t)b * nchunk + q) * WM_PART;
#pragma unroll
    for (int m = 0; m < WM_PART; ++m) p[m] += w[m];
  }
#pragma unroll
  for (int m = 0; m < WM_PART; ++m) p[m] = wave_sum_f64(p[m]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int m = 0; m < WM_PART; ++m) red[tid >> 6][m] = p[m];
  }
  __syncthreads();
  if (tid != 0) return;
#pragma unroll
  for (int m = 0; m < WM_PART; ++m) p[m] = ((red[0][m] + red[1][m]) + red[2][m]) + red[3][m];

  const double n = (double)len;
  const double mc = p[0] / n, md = p[1] / n;
  // moments of the mean-removed c and d = e - c; the mean-removed <e, c> is cc + dc
  const double cc = p[2] - n * mc * mc, dd = p[3] - n * md * md, dc = p[4] - n * md * mc;
  const double alpha = (cc + dc) / (cc + eps);
  const double num = alpha * alpha * cc;
  // e - alpha c = d + beta c with beta = 1 - alpha = (eps - dc) / (cc + eps), formed without the
  // cancellation of 1 - alpha: an estimate close to clean keeps its tiny distortion
  const double beta = (eps - dc) / (cc + eps);
  const double den = dd + 2.0 * beta * dc + beta * beta * cc;
  double* o = out + (size_t)b * 3;
  o[0] = 10.0 * log10(num / (den + eps));
  o[1] = 10.0 * log10((p[2] / n) / (p[3] / n + eps));
  o[2] = p[6] > 0 ? p[5] / p[6] : 0.0;
}

// grid (cdiv(T, 16), B), 256 threads = 16 frames (fastest: T is contiguous) x 16 bin slices
__global__ __launch_bounds__(256) void lsd_frames_kernel(const float* __restrict__ a, const float* __restrict__ bm,
                                                         const int* __restrict__ lengths, int F, int T, int hop,
                                                         double eps, double* __restrict__ ws) {
  __shared__ double part[LSD_SLICES][LSD_FRAMES];
  const int b = blockIdx.y, t0 = blockIdx.x * LSD_FRAMES;
  int valid = T;
  if (lengths) {
    const int len = lengths[b] < 0 ? 0 : lengths[b];
    valid = 1 + len / hop < T ? 1 + len / hop : T;
  }
  if (t0 >= valid) return;  // lsd_finish reads no frame past the row
  const int tl = threadIdx.x & (LSD_FRAMES - 1), slice = threadIdx.x >> 4;
  const int t = t0 + tl;
  double s = 0;
  if (t < valid) {
    const size_t row = (size_t)b * F * T + t;
    for (int f = slice; f < F; f += LSD_SLICES) {
      const double d = log((double)a[row + (size_t)f * T] + eps) - log((double)bm[row + (size_t)f * T] + eps);
      s = fma(d, d, s);
    }
  }
  part[slice][tl] = s;
  __syncthreads();
  if (slice == 0 && t < valid) {
    double tot = 0;
#pragma unroll
    for (int q = 0; q < LSD_SLICES; ++q) tot += part[q][tl];
    ws[(size_t)b * T + t] = sqrt(tot / (double)F);
  }
}

__global__ __launch_bounds__(WM_THREADS) void lsd_finish_kernel(const int* __restrict__ lengths, int T, int hop,
                                                                const double* __restrict__ ws,
                                                                double* __restrict__ out) {
  __shared__ double red[WM_WAVES];
  const int b = blockIdx.x;
  int valid = T;
  if (lengths) {
    const int len = lengths[b] < 0 ? 0 : lengths[b];
    valid = 1 + len / hop < T ? 1 + len / hop : T;
  }
  double s = 0;
  for (int t = threadIdx.x; t < valid; t += WM_THREADS) s += ws[(size_t)b * T + t];
  s = block_sum_f64(s, red);
  if (threadIdx.x == 0) out[b] = s / (double)valid;
}

}  // namespace hvit

using namespace hvit;

static long long wave_chunks(int L, int hop) {
  const long long per = (long long)WM_CHUNK * hop;
  return ((long long)L + per - 1) / per;
}

long long hvit_wave_metrics_ws_elems(int B, int L, int seg_hop) {
  if (B < 1 || L < 1 || seg_hop < 1) return 0;
  return (long long)B * wave_chunks(L, seg_hop) * WM_PART;
}

int hvit_wave_metrics(const float* clean, long long clean_stride, const float* est, long long est_stride,
                      const int* lengths, int B, int L, int seg_frame, int seg_hop, double eps, double* ws,
                      long long ws_elems, double* out, void* stream) {
  HVIT_CHECK(clean && est && ws && out, "hvit_wave_metrics: null pointer");
  HVIT_CHECK(B >= 1 && B <= 65535 && L >= 1, "hvit_wave_metrics: B=%d L=%d", B, L);
  HVIT_CHECK(B == 1 || (clean_stride >= L && est_stride >= L), "hvit_wave_metrics: row strides %lld / %lld < L=%d",
             clean_stride, est_stride, L);
  HVIT_CHECK(seg_hop >= 1 && seg_frame >= seg_hop && seg_frame % seg_hop == 0 &&
                 seg_frame / seg_hop <= WM_MAX_RATIO,
             "hvit_wave_metrics: seg_frame=%d must be a positive multiple of seg_hop=%d, at most %d times it",
             seg_frame, seg_hop, WM_MAX_RATIO);
  HVIT_CHECK(eps >= 0.0, "hvit_wave_metrics: eps=%g", eps);
  HVIT_CHECK(ws_elems >= hvit_wave_metrics_ws_elems(B, L, seg_hop), "hvit_wave_metrics: workspace %lld < %lld doubles",
             ws_elems, hvit_wave_metrics_ws_elems(B, L, seg_hop));
  HVIT_CHECK(((((uintptr_t)ws) | ((uintptr_t)out)) & 7) == 0, "hvit_wave_metrics: ws / out must be 8-byte aligned");
  const long long nchunk = wave_chunks(L, seg_hop);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(wave_chunks_kernel, dim3((unsigned)nchunk, B), dim3(WM_THREADS), 0, st, clean, (long)clean_stride,
                     est, (long)est_stride, lengths, L, seg_hop, seg_frame, eps, (int)nchunk, ws);
  HVIT_LAUNCH_CHECK();
  hipLaunchKernelGGL(wave_finish_kernel, dim3(B), dim3(WM_THREADS), 0, st, lengths, L, seg_hop, eps, (int)nchunk,
                     (const double*)ws, out);
  HVIT_LAUNCH_CHECK();
  return HVIT_OK;
}

long long hvit_lsd_ws_elems(int B, int T) {
  if (B < 1 || T < 1) return 0;
  return (long long)B * T;
}

int hvit_lsd(const float* mag_a, const float* mag_b, const int* lengths, int B, int F, int T, int hop, double eps,
             double* ws, long long ws_elems, double* out, void* stream) {
  HVIT_CHECK(mag_a && mag_b && ws && out, "hvit_lsd: null pointer");
  HVIT_CHECK(B >= 1 && B <= 65535 && F >= 1 && T >= 1, "hvit_lsd: B=%d F=%d T=%d", B, F, T);
  HVIT_CHECK(!lengths || hop >= 1, "hvit_lsd: hop=%d with lengths", hop);
  HVIT_CHECK(eps >= 0.0, "hvit_lsd: eps=%g", eps);
  HVIT_CHECK(ws_elems >= hvit_lsd_ws_elems(B, T), "hvit_lsd: workspace %lld < %lld doubles", ws_elems,
             hvit_lsd_ws_elems(B, T));
  HVIT_CHECK(((((uintptr_t)ws) | ((uintptr_t)out)) & 7) == 0, "hvit_lsd: ws / out must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(lsd_frames_kernel, dim3(cdiv(T, LSD_FRAMES), B), dim3(256), 0, st, mag_a, mag_b, lengths, F, T,
                     hop, eps, ws);
  HVIT_LAUNCH_CHECK();
  hipLaunchKernelGGL(lsd_finish_kernel, dim3(B), dim3(WM_THREADS), 0, st, lengths, T, hop, (const double*)ws, out);
  HVIT_LAUNCH_CHECK();
  return HVIT_OK;
}
