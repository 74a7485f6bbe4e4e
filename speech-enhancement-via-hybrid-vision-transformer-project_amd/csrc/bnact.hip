// BatchNorm2d -> ReLU -> Dropout2d -> MaxPool2d(pool) tail of ConvBlock /
// TransposeConvBlock (components.py:67-85, :161-178 of the reference) on NHWC
// activations, gfx950.
//
// One thread owns one pooling window x 16 bytes of channels (8 bf16 / 4 f32),
// so every z / y / dy / dz access is a coalesced 16-byte vector and the window
// is read once.  The backward recomputes relu(bn(z)) for the window, routes the
// pooled gradient to the first maximum in scan order (torch's max_pool2d tie
// rule; positions outside full windows get zero), applies the per-(sample,
// channel) dropout mask and relu', then
//   reduce pass: sums[0][c] = sum g, sums[1][c] = sum g * xhat  (dbeta, dgamma)
//   apply pass : dz = gamma * invstd * (g - sum g / M - xhat * sum g*xhat / M)
// Window / pixel indices stay in 32 bits.
#include <algorithm>

#include "bn_tail.h"
#include "chan_vec.h"
#include "common.h"

namespace hvit {

// partial rows of the backward sums: one per workgroup of the sums kernel
// (plain stores, summed in row order by a deterministic column reduction), so
// the sums grid is capped at BN_PART_ROWS
constexpr int BN_PART_ROWS = 1024;

// channels per 16-byte vector of T: the channel group one thread owns
template <typename T>
constexpr int CV16 = 16 / sizeof(T);

struct BnArgs {
  int N, H, W, C, pool;
  const float* mean;
  const float* invstd;
  const float* gamma;
  const float* beta;
  DropKey drop;
  // index divisors: channel groups, full windows (Wo, Ho), all windows (Ww, Hw)
  FastDiv fG, fWo, fHo, fWw, fHw;
};

// sc, sh of channels c .. c+CV-1 (and mean, invstd for the backward's xhat).
// The per-channel constants go as 16-byte vector loads (c is a multiple of
// CV): scalar loads of them came out serialised one round trip each (48 of
// them in the apply pass), a ~20 us floor on every launch
template <int CV>
__device__ __forceinline__ void bn_consts(const BnArgs& a, int c, float* sc, float* sh, float* mu, float* is) {
  float ga[CV], be[CV];
  load_chan<CV>(a.mean + c, mu);
  load_chan<CV>(a.invstd + c, is);
  load_chan<CV>(a.gamma + c, ga);
  load_chan<CV>(a.beta + c, be);
#pragma unroll
  for (int e = 0; e < CV; ++e) bn_scale_shift(mu[e], is[e], ga[e], be[e], sc[e], sh[e]);
}

// CV values of y / dy, whose dtype need not be z's: one 16-byte vector when
// the element sizes match, else element by element
template <int CV, typename TD>
__device__ __forceinline__ void load_io(const TD* p, float* f) {
  if constexpr (CV * sizeof(TD) == 16) {
    load_chan<CV>(p, f);
  } else {
#pragma unroll
    for (int e = 0; e < CV; ++e) f[e] = Elem<TD>::to_f(p[e]);
  }
}
template <int CV, typename TO>
__device__ __forceinline__ void store_io(TO* p, const float* f) {
  if constexpr (CV * sizeof(TO) == 16) {
    store_chan<CV>(p, f);
  } else {
#pragma unroll
    for (int e = 0; e < CV; ++e) p[e] = Elem<TO>::from_f(f[e]);
  }
}

// forward: y[n, oy, ox, c..] over full windows
template <typename T, typename TO>
__global__ __launch_bounds__(256) void bnact_fwd_kernel(const T* __restrict__ z, TO* __restrict__ y, BnArgs a_) {
  BnArgs a = a_;
  a.drop.resolve();
  constexpr int CV = CV16<T>;
  const int G = a.C / CV;
  const int Ho = a.H / a.pool, Wo = a.W / a.pool;
  const int total = a.N * Ho * Wo * G;
  // a thread's channel group never changes (256 % G == 0, grid stride % G == 0)
  const int c = ((blockIdx.x * blockDim.x + threadIdx.x) % G) * CV;
  float sc[CV], sh[CV], mu[CV], is[CV];
  bn_consts<CV>(a, c, sc, sh, mu, is);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int t = a.fG.div(i);
    const int t1 = a.fWo.div(t);
    const int ox = t - t1 * Wo;
    const int n = a.fHo.div(t1);
    const int oy = t1 - n * Ho;
    float best[CV];
#pragma unroll
    for (int e = 0; e < CV; ++e) best[e] = 0.f;  // relu output >= 0
    for (int dy = 0; dy < a.pool; ++dy)
      for (int dx = 0; dx < a.pool; ++dx) {
        float v[CV];
        load_chan<CV>(z + ((size_t)(n * a.H + oy * a.pool + dy) * a.W + ox * a.pool + dx) * a.C + c, v);
#pragma unroll
        for (int e = 0; e < CV; ++e) best[e] = fmaxf(best[e], __builtin_fmaf(v[e], sc[e], sh[e]));
      }
    float m[CV];
    chan_keep<CV>(a.drop, n, a.C, c, m);
    float o[CV];
#pragma unroll
    for (int e = 0; e < CV; ++e) o[e] = best[e] * m[e];
    store_io<CV>(y + ((size_t)(n * Ho + oy) * Wo + ox) * a.C + c, o);
  }
}

// backward apply pass: dz of every pixel from the routed gradient (the first
// maximum of its window, route_first_max; positions outside full windows get
// none) and, in training mode, the sums of bnact_sums_kernel
template <typename T, typename TD>
__global__ __launch_bounds__(256) void bnact_bwd_kernel(const T* __restrict__ z, const TD* __restrict__ dy,
                                                       BnArgs a_, const float* __restrict__ sums, int training,
                                                       T* __restrict__ dz) {
  BnArgs a = a_;
  a.drop.resolve();
  constexpr int CV = CV16<T>;
  constexpr int MAXW = 4;  // pool <= 2
  const int G = a.C / CV;
  const int P = a.pool;
  const int Ho = a.H / P, Wo = a.W / P;
  const int Hw = (a.H + P - 1) / P, Ww = (a.W + P - 1) / P;
  const int total = a.N * Hw * Ww * G;
  const float invM = 1.f / (float)(a.N * a.H * a.W);
  // a thread's channel group never changes (256 % G == 0, grid stride % G == 0):
  // per-channel constants are loaded once
  const int c = ((blockIdx.x * blockDim.x + threadIdx.x) % G) * CV;
  float sc[CV], sh[CV], mu[CV], is[CV], ca[CV], cb[CV], s1v[CV], s2v[CV];
  bn_consts<CV>(a, c, sc, sh, mu, is);
  load_chan<CV>(sums + c, s1v);
  load_chan<CV>(sums + a.C + c, s2v);
#pragma unroll
  for (int e = 0; e < CV; ++e) bn_bwd_coeffs(sc[e], mu[e], is[e], s1v[e], s2v[e], invM, training, ca[e], cb[e]);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int t = a.fG.div(i);
    const int t1 = a.fWw.div(t);
    const int wx = t - t1 * Ww;
    const int n = a.fHw.div(t1);
    const int wy = t1 - n * Hw;
    // window values
    float zv[MAXW][CV];
    bool inb[MAXW];
#pragma unroll
    for (int q = 0; q < MAXW; ++q) {
      const int y = wy * P + (q >> 1), x = wx * P + (q & 1);
      inb[q] = (q < P * P) && (P == 2 || q == 0) && y < a.H && x < a.W;
      if (inb[q]) load_chan<CV>(z + ((size_t)(n * a.H + y) * a.W + x) * a.C + c, zv[q]);
    }
    const bool full = wy < Ho && wx < Wo;
    // routed gradient: gv[e] at window position arg[e] (first maximum), 0 elsewhere
    int arg[CV];
    float gv[CV];
#pragma unroll
    for (int e = 0; e < CV; ++e) {
      arg[e] = 0;
      gv[e] = 0.f;
    }
    if (full) {  // (every position q < P * P of a full window is inside the image)
      float d[CV], m[CV];
      load_io<CV>(dy + ((size_t)(n * Ho + wy) * Wo + wx) * a.C + c, d);
      chan_keep<CV>(a.drop, n, a.C, c, m);
#pragma unroll
      for (int e = 0; e < CV; ++e) {
        const float w[MAXW] = {zv[0][e], zv[1][e], zv[2][e], zv[3][e]};
        const FirstMax r = route_first_max(w, sc[e], sh[e], P * P);
        arg[e] = r.arg;
        gv[e] = r.best > 0.f ? d[e] * m[e] : 0.f;
      }
    }
#pragma unroll
    for (int q = 0; q < MAXW; ++q) {
      if (!inb[q]) continue;
      float o[CV];
#pragma unroll
      for (int e = 0; e < CV; ++e) {
        const float gq = arg[e] == q ? gv[e] : 0.f;
        // f32 z keeps the plain expression and with it the compiler's contraction, which is not
        // bn_bwd_dz's: for two of the four channels it pairs sc*gq with cb*z in a packed multiply and
        // adds both unfused.  The values stay bit for bit those of the code before bn_tail.h.
        if constexpr (sizeof(T) == 2) o[e] = training ? bn_bwd_dz(sc[e], gq, ca[e], cb[e], zv[q][e]) : sc[e] * gq;
        else o[e] = training ? sc[e] * gq + ca[e] + cb[e] * zv[q][e] : sc[e] * gq;
      }
      const int y = wy * P + (q >> 1), x = wx * P + (q & 1);
      store_chan<CV>(dz + ((size_t)(n * a.H + y) * a.W + x) * a.C + c, o);
    }
  }
}

// backward reduce pass (both modes): per-channel sums of the routed gradient g
// and of g * xhat over full pooling windows.  Software-pipelined: the next
// window's z taps and dy are loaded (raw) before the current one is reduced,
// so every thread keeps two windows of loads in flight.
template <typename T, typename TD>
__global__ __launch_bounds__(256) void bnact_sums_kernel(const T* __restrict__ z, const TD* __restrict__ dy,
                                                        BnArgs a_, float* __restrict__ sums) {
  BnArgs a = a_;
  a.drop.resolve();
  constexpr int CV = CV16<T>;
  constexpr int MAXW = 4;  // pool <= 2
  __shared__ float red[2][256][CV];
  const int G = a.C / CV;
  const int P = a.pool;
  const int Ho = a.H / P, Wo = a.W / P;
  const int total = a.N * Ho * Wo * G;  // full windows only
  const int c = ((blockIdx.x * blockDim.x + threadIdx.x) % G) * CV;
  float sc[CV], sh[CV], mu[CV], is[CV], acc1[CV], acc2[CV];
  bn_consts<CV>(a, c, sc, sh, mu, is);
#pragma unroll
  for (int e = 0; e < CV; ++e) acc1[e] = acc2[e] = 0.f;
  struct Item {
    ChanVec<T, CV> zr[MAXW];
    float d[CV];
    int n;
  };
  auto load = [&](int i, Item& it) {
    if (i >= total) return;
    const int t = a.fG.div(i);
    const int t1 = a.fWo.div(t);
    const int wx = t - t1 * Wo;
    it.n = a.fHo.div(t1);
    const int wy = t1 - it.n * Ho;
#pragma unroll
    for (int q = 0; q < MAXW; ++q)
      if (q < P * P)
        it.zr[q].load(z + ((size_t)(it.n * a.H + wy * P + (q >> 1)) * a.W + wx * P + (q & 1)) * a.C + c);
    load_io<CV>(dy + ((size_t)(it.n * Ho + wy) * Wo + wx) * a.C + c, it.d);
  };
  auto reduce = [&](const Item& it) {
    float m[CV];
    chan_keep<CV>(a.drop, it.n, a.C, c, m);
#pragma unroll
    for (int e = 0; e < CV; ++e) {
      // (converted one channel at a time: all four vectors as floats at once cost 17 VGPRs and a wave per SIMD)
      const float w[MAXW] = {it.zr[0].at(e), it.zr[1].at(e), it.zr[2].at(e), it.zr[3].at(e)};
      const FirstMax r = route_first_max(w, sc[e], sh[e], P * P);
      const float gv = r.best > 0.f ? it.d[e] * m[e] : 0.f;
      acc1[e] += gv;
      acc2[e] += gv * ((r.z - mu[e]) * is[e]);
    }
  };
  const int stride = gridDim.x * blockDim.x;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  Item cur;
  load(i, cur);
  for (; i < total; i += stride) {
    Item nxt;
    load(i + stride, nxt);
    reduce(cur);
    cur = nxt;
  }
  // every thread of a block keeps one channel group (256 % G == 0 and the grid
  // stride is a multiple of G): reduce across the block
#pragma unroll
  for (int e = 0; e < CV; ++e) {
    red[0][threadIdx.x][e] = acc1[e];
    red[1][threadIdx.x][e] = acc2[e];
  }
  __syncthreads();
  if (threadIdx.x < G) {
    float t1[CV], t2[CV];
#pragma unroll
    for (int e = 0; e < CV; ++e) t1[e] = t2[e] = 0.f;
    for (int k = threadIdx.x; k < 256; k += G)
#pragma unroll
      for (int e = 0; e < CV; ++e) {
        t1[e] += red[0][k][e];
        t2[e] += red[1][k][e];
      }
    float* slot = sums + 2 * a.C * (1 + blockIdx.x);  // this workgroup's partial row (no atomics)
    const int cc = threadIdx.x * CV;
#pragma unroll
    for (int e = 0; e < CV; ++e) {
      slot[cc + e] = t1[e];
      slot[a.C + cc + e] = t2[e];
    }
  }
}


// grid-stride launches; per-kernel caps measured on the B=32 encoder shapes
// (fewer, longer-lived workgroups stream better here than one item per thread)
static int grid_for(long n, long cap) {
  long g = (n + 255) / 256;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}
constexpr long BN_GRID_FWD = 2048, BN_GRID_SUMS = BN_PART_ROWS, BN_GRID_APPLY = 1024;

static int make_args(BnArgs& a, int N, int H, int W, int C, int pool, const float* mean, const float* invstd,
                     const float* gamma, const float* beta, const hvit_dropout_t* dr, int cv) {
  HVIT_CHECK(mean && invstd && gamma && beta, "bn_act: null statistics / affine pointer");
  HVIT_CHECK(aligned16(mean) && aligned16(invstd) && aligned16(gamma) && aligned16(beta),
             "bn_act: statistics / affine vectors must be 16-byte aligned");
  HVIT_CHECK(pool == 1 || pool == 2, "bn_act: pool must be 1 or 2");
  HVIT_CHECK(C > 0 && C % cv == 0 && (C / cv) <= 256 && (256 % (C / cv)) == 0,
             "bn_act: C=%d must be a multiple of %d with C/%d dividing 256", C, cv, cv);
  HVIT_CHECK((long)N * H * W * C < (1L << 31), "bn_act: tensor too large for 32-bit indexing");
  a.N = N; a.H = H; a.W = W; a.C = C; a.pool = pool;
  a.mean = mean; a.invstd = invstd; a.gamma = gamma; a.beta = beta;
  a.drop = drop_key(dr);
  a.fG = FastDiv(C / cv);
  a.fWo = FastDiv(std::max(1, W / pool));
  a.fHo = FastDiv(std::max(1, H / pool));
  a.fWw = FastDiv((W + pool - 1) / pool);
  a.fHw = FastDiv((H + pool - 1) / pool);
  return HVIT_OK;
}

}  // namespace hvit

using namespace hvit;

extern "C" int hvit_bn_act_fwd(int dt, const void* z, int N, int H, int W, int C, const float* mean,
                               const float* invstd, const float* gamma, const float* beta,
                               const hvit_dropout_t* dropout2d, int pool, void* y, int y_dt, void* stream) {
  HVIT_CHECK(z && y, "hvit_bn_act_fwd: null pointer");
  HVIT_CHECK(aligned16(z) && aligned16(y), "hvit_bn_act_fwd: alignment");
  BnArgs a;
  const int cv = dt == HVIT_BF16 ? 8 : 4;
  if (int rc = make_args(a, N, H, W, C, pool, mean, invstd, gamma, beta, dropout2d, cv)) return rc;
  const long total = (long)N * (H / pool) * (W / pool) * (C / cv);
  if (total <= 0) return HVIT_OK;
  hipStream_t st = (hipStream_t)stream;
  dim3 g(grid_for(total, BN_GRID_FWD));
  with_elem(dt, [&](auto t) {
    with_elem(y_dt, [&](auto to) {
      using T = decltype(t);
      using TO = decltype(to);
      hipLaunchKernelGGL((bnact_fwd_kernel<T, TO>), g, dim3(256), 0, st, (const T*)z, (TO*)y, a);
    });
  });
  HVIT_LAUNCH_CHECK();
  return HVIT_OK;
}

template <typename T, typename TD>
static int bnact_bwd_t(const void* z, const void* dy, const BnArgs& a, float* sums, int training, void* dz,
                       hipStream_t st) {
  const int cv = 16 / sizeof(T);
  const int P = a.pool;
  const long total = (long)a.N * ((a.H + P - 1) / P) * ((a.W + P - 1) / P) * (a.C / cv);
  if (total <= 0) return HVIT_OK;
  dim3 g(grid_for(total, BN_GRID_SUMS)), ga(grid_for(total, BN_GRID_APPLY));
  {  // the sums are dbeta / dgamma in both modes; only training-mode dz uses them
    const long tsum = (long)a.N * (a.H / P) * (a.W / P) * (a.C / cv);
    const int gs = tsum > 0 ? grid_for(tsum, BN_GRID_SUMS) : 0;
    if (gs > 0) {
      hipLaunchKernelGGL((bnact_sums_kernel<T, TD>), dim3(gs), dim3(256), 0, st, (const T*)z, (const TD*)dy, a, sums);
      HVIT_LAUNCH_CHECK();
    }
    // sums[0 .. 2C) = the partial rows summed in row order (0 rows: zeros)
    if (int rc = hvit_reduce_rows(sums + 2 * a.C, HVIT_F32, gs, 2 * a.C, 2 * a.C, 0, sums, st)) return rc;
  }
  hipLaunchKernelGGL((bnact_bwd_kernel<T, TD>), ga, dim3(256), 0, st, (const T*)z, (const TD*)dy, a, sums,
                     training, (T*)dz);
  HVIT_LAUNCH_CHECK();
  return HVIT_OK;
}

extern "C" long long hvit_bn_act_bwd_sums_elems(int C) { return 2LL * C * (1 + BN_PART_ROWS); }

extern "C" int hvit_bn_act_bwd(int dt, const void* z, int N, int H, int W, int C, const float* mean,
                               const float* invstd, const float* gamma, const float* beta,
                               const hvit_dropout_t* dropout2d, int pool, const void* dy, int dy_dt,
                               int training, void* dz, int dz_dt, float* sums, int flags, void* stream) {
  HVIT_CHECK(z && dy && dz && sums, "hvit_bn_act_bwd: null pointer");
  HVIT_CHECK(dz_dt == dt, "hvit_bn_act_bwd: dz dtype must equal z dtype");
  HVIT_CHECK(aligned16(z) && aligned16(dz) && aligned16(dy), "hvit_bn_act_bwd: alignment");
  BnArgs a;
  const int cv = dt == HVIT_BF16 ? 8 : 4;
  if (int rc = make_args(a, N, H, W, C, pool, mean, invstd, gamma, beta, dropout2d, cv)) return rc;
  hipStream_t st = (hipStream_t)stream;
  (void)flags;  // (the partial rows are plain stores: no zeroed accumulator needed)
  int rc = HVIT_OK;
  with_elem(dt, [&](auto t) {
    with_elem(dy_dt, [&](auto td) { rc = bnact_bwd_t<decltype(t), decltype(td)>(z, dy, a, sums, training, dz, st); });
  });
  return rc;
}
