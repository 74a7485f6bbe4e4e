// Halo-resident A operand for the bf16 3x3 same-conv implicit GEMMs (forward
// and data gradient): a second delivery beside GemmCoreDma's per-tap im2col.
//
// The per-tap loader re-issues a tile's input pixels once per tap, nine times
// per tile, through LDS-DMA; those kernels run at the L2 -> LDS gather rate
// (DESIGN.md §4).  Here a workgroup loads its tile's input halo once -- the
// (TR + 2) x (TW + 2) pixels x all Cin channels around its BM consecutive
// output pixels (TR image rows of TW pixels) -- and all 9 x Cin/64 K stages
// read their A fragments from that one image at a per-stage tap offset.  Only
// B (the packed weights) still streams, through a ring of NB stage buffers.
//
// Unchanged against the per-tap path: the tap-major K order (k = (ky*3 + kx) *
// Cin + c), two k-steps of v_mfma_f32_16x16x32_bf16 per 64-channel stage, the
// pixel-major row order, the XCD tile order, and the plain-store epilogue with
// its 64-row BatchNorm partial tiles -- every output element sees the same f32
// operations in the same order, so results are bit-identical.
//
// Halo image: pixel (hy, hx) of the halo sits at (hy * (TW + 2) + hx) * 2 Cin
// bytes; inside a pixel the 16-byte channel chunks are XOR-swizzled in groups
// of eight by (hx & 7), applied on the DMA's source side (a DMA wave-instruction
// fills 1 KiB of lane-linear LDS).  With 128-byte pixels (Cin = 64) two
// neighbouring pixels share a 256-byte bank row, as the rows of the per-tap KC
// image do; from 256-byte pixels on every pixel starts a bank row and one
// k-step's four chunks would all fall into the same half of it (2-way), so
// there bit 3 of the chunk index is flipped by (hx & 1) as well.  A fragment
// read (16 consecutive pixels of one image row x four 16-byte chunks) then
// touches each 16-lane group's banks once for every tap shift (halo_key /
// halo_off below; checked exhaustively on the CPU by tests/test_conv_halo_map.py).  Padding rows / columns and the image
// tail get a source offset past num_records: the DMA writes zeros.
//
// A workgroup is G groups of 256 threads (G = 1: 128-row tiles, G = 2: 256-row
// tiles, which halve the B bytes per output row); each group runs a 128-row
// tile of the per-tap kernel's wave layout (2 x 2 waves of 64 x BN/2) and its
// own copy of the epilogue, in lock-step on the workgroup's barriers.
#pragma once
#include "gemm.h"

namespace hvit {

// ---- the halo map (host + device; the CPU test mirrors these) ---------------
// LDS byte offset of the 16-byte chunk `cc` (channel / 8) of halo pixel (hy, hx)
// swizzle key of halo column hx: chunk cc of a pixel sits at chunk cc ^ key
__host__ __device__ inline int halo_key(int hx, int C) { return (hx & 7) | (C >= 128 ? (hx & 1) << 3 : 0); }
__host__ __device__ inline int halo_off(int hy, int hx, int cc, int HW, int C) {
  return (hy * HW + hx) * (C * 2) + ((cc ^ halo_key(hx, C)) << 4);
}

__device__ __forceinline__ u32x4 ds128_asm(unsigned addr) {
  // asm like ds_tr16_asm: invisible to the wait-count pass, which would drain
  // every in-flight LDS-DMA before a read it cannot tell apart from the ring
  u32x4 r;
  asm volatile("ds_read_b128 %0, %1" : "=v"(r) : "v"(addr));
  return r;
}

struct HaloGeom {
  int tws;    // log2(TW), TW = pixels of one image row in a tile
  int cps;    // log2(Cin / 8), chunks per pixel
  int pieces; // 1-KiB DMA pieces of the halo image
};

template <int BN, int G, int NB>
struct ConvHaloCfg {
  static constexpr int THREADS = 256 * G, NW = 4 * G, BM = 128 * G;
  using IB = DmaImg<BN, true>;
  static constexpr int PB = IB::PIECES / NW;  // B pieces per wave per stage
  static_assert(IB::PIECES % NW == 0 && PB >= 1, "B stage must split over the waves");
  static_assert(NB >= 2 && NB <= 6, "B ring depth");
  static constexpr int RING = NB * IB::BYTES;
  // one group's epilogue staging: 64-row f32 tile image + statistics scratch (as gemm_kernel)
  static constexpr int SM_E = (64 * (BN + 4) + (256 / (BN / 4)) * BN) * 4;
};

// The K loop: halo, B ring, MFMAs (a __device__ function, as GemmCoreDma::run_t: its
// lambdas hold target builtins).
template <int BN, int G, int NB>
__device__ __forceinline__ void conv_halo_loop(const LdConvF<bf16_t>& la, const LdDense<bf16_t, true>& lb, char* smem,
                                               const HaloGeom& hg, int m0, int n0, int K,
                                               f32x4 (&acc)[4][BN / 32]) {
  using Cfg = ConvHaloCfg<BN, G, NB>;
  using IB = typename Cfg::IB;
  constexpr int NW = Cfg::NW, BM = Cfg::BM, PB = Cfg::PB;
  constexpr int WTN = BN / 2, FM = 4, FN = WTN / 16;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wid >> 2, wq = wid & 3;
  const int wm = wq >> 1, wn = wq & 1;
  const int frow = lane & 15, fq = lane >> 4;
  // tile geometry: BM consecutive output pixels = TR rows of TW pixels of one image
  const int C = la.C1, CB = C * 2, W = la.Wo, H = la.Ho;
  const int TW = 1 << hg.tws, TR = BM >> hg.tws, HW = TW + 2, HR = TR + 2;
  const int hw = H * W;
  const int nimg = m0 / hw, rem = m0 - nimg * hw;
  const int y0 = rem / W, x0 = rem - y0 * W;

  // ---- halo: pieces in image order (the ky = 0 rows land first) --------------
  {
    const __amdgpu_buffer_rsrc_t ra =
        __builtin_amdgcn_make_buffer_rsrc((void*)la.src1, (short)0, (int)la.bytes1, 0x00020000);
    const int q0 = wid * 64 + lane;
    const int sc = q0 & ((1 << hg.cps) - 1);
    const int hp = q0 >> hg.cps;
    int hy = hp / HW, hx = hp - hy * HW;
    const int dhp = (64 * NW) >> hg.cps;
    for (int pc = wid; pc < hg.pieces; pc += NW) {
      const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
      const bool ok = hy < HR && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
      const int cc = sc ^ halo_key(hx, C);
      const int off = (((nimg * H + iy) * W + ix) * C + cc * 8) * 2;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (__attribute__((address_space(3))) void*)(smem + pc * 1024), 16,
                                               ok ? (unsigned)off : 0x80000000u, 0, 0, 0);
      hx += dhp;
      while (hx >= HW) {
        hx -= HW;
        ++hy;
      }
    }
  }

  // ---- B ring ------------------------------------------------------------------
  char* const ring = smem + hg.pieces * 1024;
  const int nk = K / 64;
  const __amdgpu_buffer_rsrc_t rb =  // (host: the weights' bytes fit 31 bits)
      __builtin_amdgcn_make_buffer_rsrc((void*)lb.p, (short)0, (int)((long)lb.rows * lb.ld * 2), 0x00020000);
  const unsigned ob = (unsigned)(((long)n0 * lb.ld) * 2);
  unsigned vb[PB];
#pragma unroll
  for (int i = 0; i < PB; ++i) vb[i] = IB::src_off(wid + NW * i, lane, lb.ld);
  auto issue = [&](int t) {
    char* bbuf = ring + (t % NB) * IB::BYTES;
    const unsigned sb = ob + (unsigned)(t < nk ? t : nk - 1) * 128u;
#pragma unroll
    for (int i = 0; i < PB; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (__attribute__((address_space(3))) void*)(bbuf + (wid + NW * i) * 1024),
                                               16, vb[i], sb, 0, 0);
  };
#pragma unroll
  for (int u = 0; u < NB - 1; ++u) issue(u);

  // A fragment bases: row r of the tile is halo pixel (r / TW + ky, r % TW + kx);
  // (r % TW) & 7 == lane & 7 for every fragment (TW % 16 == 0)
  unsigned abase[FM];
  const unsigned s0 = lds_addr(smem);
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int r = grp * 128 + wm * 64 + i * 16 + frow;
    abase[i] = s0 + (unsigned)(((r >> hg.tws) * HW + (r & (TW - 1))) * CB);
  }
  const unsigned ringa = lds_addr(ring);
  unsigned bfo[FN][2];  // B fragment offsets inside a stage (kc_off)
#pragma unroll
  for (int j = 0; j < FN; ++j)
#pragma unroll
    for (int s = 0; s < 2; ++s) bfo[j][s] = (unsigned)kc_off(wn * WTN + j * 16 + frow, 4 * s + fq);

  auto mma = [&](const u32x4(&fa)[FM], const u32x4(&fb)[FN]) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, fa[i]),
                                                            __builtin_bit_cast(s16x8, fb[j]), acc[i][j], 0, 0, 0);
  };

  // Stage t's B landed when at most NB - 2 younger stages are in flight (the halo
  // pieces are older than every B piece, so the first wait covers the halo too).
  // Stage t + NB - 1 goes into the buffer of stage t - 1, which every wave
  // released before the barrier that opens stage t.
  constexpr int VM = (NB - 2) * PB;
  constexpr int MPD = (FM * FN) / PB;
  int c0 = 0, kx = 0, ky = 0;  // stage tap cursor (uniform)
  for (int t = 0; t < nk; ++t) {
    __builtin_amdgcn_s_waitcnt(0x0F70 | (VM & 15) | (((VM >> 4) & 3) << 14));
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // chunk (c0 / 8 + 4 s + fq) ^ key: bits 4.. of the chunk index are uniform, bits 0-3 per lane
    const unsigned ua = (unsigned)((ky * HW + kx) * CB + ((c0 * 2) & ~255));
    const unsigned x0v = (unsigned)(((((c0 >> 3) & 8) | fq) ^ halo_key(lane + kx, C)) << 4);
    const unsigned bt = ringa + (unsigned)((t % NB) * IB::BYTES);
    u32x4 fa0[FM], fb0[FN], fa1[FM], fb1[FN];
#pragma unroll
    for (int i = 0; i < FM; ++i) fa0[i] = ds128_asm(abase[i] + ua + x0v);
#pragma unroll
    for (int j = 0; j < FN; ++j) fb0[j] = ds128_asm(bt + bfo[j][0]);
    lgkm_wait0();
    lds_pin(fa0);
    lds_pin(fb0);
#pragma unroll
    for (int i = 0; i < FM; ++i) fa1[i] = ds128_asm(abase[i] + ua + (x0v ^ 64u));
#pragma unroll
    for (int j = 0; j < FN; ++j) fb1[j] = ds128_asm(bt + bfo[j][1]);
    issue(t + NB - 1);
    mma(fa0, fb0);
#pragma unroll
    for (int k = 0; k < PB && MPD * (k + 1) <= FM * FN; ++k) {
      __builtin_amdgcn_sched_group_barrier(0x008, MPD, 0);  // MFMA
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);    // one DMA piece
    }
    lgkm_wait0();
    lds_pin(fa1);
    lds_pin(fb1);
    mma(fa1, fb1);
    c0 += 64;
    if (c0 >= C) {
      c0 = 0;
      if (++kx == 3) {
        kx = 0;
        ++ky;
      }
    }
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);  // the trailing stages' DMA
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

template <int BN, int G, int NB>
__global__ __launch_bounds__(256 * G, 1) void conv_halo_kernel(LdConvF<bf16_t> la, LdDense<bf16_t, true> lb, int M,
                                                              int N, int K, Epi ep, HaloGeom hg) {
  using Cfg = ConvHaloCfg<BN, G, NB>;
  constexpr int BM = Cfg::BM;
  constexpr int WTN = BN / 2, FM = 4, FN = WTN / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wid >> 2, wq = wid & 3;
  const int wm = wq >> 1, wn = wq & 1;
  const TileId tid3 = tile_of(ep.xcd_remap);
  const int m0 = tid3.mt * BM, n0 = tid3.nt * BN;

  // epilogue column ownership and bias (fetched before the K loop), per 256-thread group
  constexpr int CP = BN + 4, C4 = BN / 4, RSTEP = 256 / C4, NR = 64 / RSTEP;
  const int tg = tid & 255;
  const int c4 = tg % C4, r0 = tg / C4;
  const int n = n0 + c4 * 4;
  const f32x4 bias4 = ep.bias ? load4(ep.bias, n, 4, HVIT_F32) : (f32x4){0.f, 0.f, 0.f, 0.f};
  const int frow = lane & 15, fq = lane >> 4;

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  GEMM_STAMP(0);
  conv_halo_loop<BN, G, NB>(la, lb, smem, hg, m0, n0, K, acc);
  GEMM_STAMP(1);

  // ---- epilogue: gemm_kernel's plain-store kind on full tiles, per group --------
  // (EK_STORE, rows(false_type): bias, ReLU flag, f32 / bf16 store, the 64-row
  // BatchNorm partial tiles' full-half merge; the staging aliases the halo)
  float* Cs = (float*)(smem + grp * Cfg::SM_E);
  const int mg0 = m0 + grp * 128;
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    if (hh > 0) epi_barrier();
    if (wm == hh) {  // (uniform) this half's 64 rows are the two waves' of wave row hh
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) Cs[(i * 16 + fq * 4 + r) * CP + wn * WTN + j * 16 + frow] = acc[i][j][r];
    }
    epi_barrier();
    const int mbase = mg0 + hh * 64;
    float st_sum[4] = {0.f, 0.f, 0.f, 0.f};
    f32x4 sv[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const int row = r0 + i * RSTEP;
      const int m = mbase + row;
      f32x4 v = *(const f32x4*)(Cs + row * CP + c4 * 4) + bias4;
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
      for (int e = 0; e < 4; ++e) st_sum[e] += v[e];
      sv[i] = v;
    }
    // the per-tap kernel's statistics from the same function, rows_here a run-time value as there
    // (always 64 here): the same code, so the same contraction of the M2 sums and the same bits
    const int rows_here = min(64, M - mbase);
    if (ep.stats && rows_here > 0)
      bn_tile_stats<BN, RSTEP, NR>(ep.stats, Cs, rows_here, r0, c4, n, N, (long)(mg0 / 64) + hh, st_sum, sv);
  }
  GEMM_STAMP(2);
}

// ---- host side -----------------------------------------------------------------
// hvit_gemm_tune(9, v): 0 = per-tap im2col everywhere, 1 = halo-resident where it
// applies and measured faster (halo_measured), 2 = wherever it applies (tests,
// tools/conv_probe.py)
inline int& conv_halo_mode_ref() {
  static int v = 1;
  return v;
}

inline long& conv_halo_count_ref() {
  static long v = 0;
  return v;
}

constexpr int HALO_LDS_MAX = 160 * 1024;

// the halo form of a BM-row tile on a H x W map of C channels, or false: tiles
// are whole image rows (BM % W == 0) or a whole-row segment (W % BM == 0) and
// never span two images
inline bool halo_geom(int H, int W, int C, int BM, HaloGeom* hg) {
  if (C < 64 || C > 512 || (C & (C - 1))) return false;
  int TW;
  if (W >= BM) {
    if (W % BM) return false;
    TW = BM;
  } else {
    if (W < 16 || BM % W || ((long)H * W) % BM) return false;
    TW = W;  // a divisor of BM = 128 G: a power of two
  }
  const int TR = BM / TW;
  int tws = 0, cps = 0;
  while ((1 << tws) < TW) ++tws;
  while ((8 << cps) < C) ++cps;
  hg->tws = tws;
  hg->cps = cps;
  hg->pieces = ((TR + 2) * (TW + 2) * C * 2 + 1023) / 1024;
  return true;
}

// Shapes kept on the halo path by default: those whose isolated time
// (tools/conv_probe.py, B = 32, tune 9 = 0 -> 2, four runs) beat the per-tap
// kernel's by more than the probe's run-to-run spread -- profiles/r7_conv_halo_ab.txt.
// Everything else that would apply stays on the per-tap path:
//  * the dec0 data gradient (W = 16, 256 channels: 90 KiB halo, 128-row tiles
//    only, one four-wave workgroup per CU) measured slower, 29.8-31.5 -> 40.5-43.3 us;
//  * the enc1 data gradient (W = 128, 128 channels, 64 columns) measured
//    121.7-127.6 -> 118.5-120.2 us: a 5 us mean gain against a 6 us spread of the
//    per-tap runs, not clear of it;
//  * small grids were not measured.
inline bool halo_measured(bool fwd, int W, int C, int BN, int G, long nwg) {
  if (nwg < 256 || G != 2) return false;
  if (fwd) return (W == 128 && C == 64 && BN == 128) ||  // enc1: 140.3-145.8 -> 124.1-124.7 us
                  (W == 64 && C == 128 && BN == 128);    // enc2: 98.1-102.3 -> 92.7-94.6 us
  return (W == 64 && C == 64 && BN == 64) ||             // dec2: 52.2-55.8 -> 35.8-36.4 us
         (W == 32 && C == 128 && BN == 128);             // dec1: 42.2-43.0 -> 39.2-40.1 us
}

template <int BN, int G, int NB>
inline bool conv_halo_launch(const LdConvF<bf16_t>& la, const LdDense<bf16_t, true>& lb, int M, int N, int K,
                             const Epi& ep, const HaloGeom& hg, int lds, hipStream_t st) {
  // dynamic LDS above the 64 KiB default needs an opt-in per kernel and device (as thinconv.hip's allow_lds)
  if (hipFuncSetAttribute((const void*)conv_halo_kernel<BN, G, NB>, hipFuncAttributeMaxDynamicSharedMemorySize,
                          HALO_LDS_MAX) != hipSuccess) {
    (void)hipGetLastError();  // not left for the per-tap launch's check to find
    return false;
  }
  dim3 g(M / (128 * G), N / BN, 1);
  hipLaunchKernelGGL((conv_halo_kernel<BN, G, NB>), g, dim3(256 * G), (size_t)lds, st, la, lb, M, N, K, ep, hg);
  return true;
}

// Launch the halo-resident kernel if it applies to this conv GEMM (A = LdConvF
// over one bf16 source, B = packed weights [N][K]); false = take launch_gemm.
// BN follows launch_gemm's tile choice, so the BatchNorm partials merge the
// same per-thread partial means in the same order.
inline bool conv_halo_try(const LdConvF<bf16_t>& la, const LdDense<bf16_t, true>& lb, int M, int N, int K,
                          const Epi& ep_in, hipStream_t st, bool fwd) {
  const int mode = conv_halo_mode_ref();
  if (mode == 0) return false;
  if (la.C2 != 0 || la.ushift != 0 || la.KS != 3 || la.S != 1 || la.Pd != 1 || la.pool2) return false;
  if (la.C1 % 64 || K != 9 * la.C1 || la.Ho != la.Hi || la.Wo != la.Wi) return false;
  const Epi& e = ep_in;
  const bool lean_store = e.mode == EPI_STORE && e.act == ACT_NONE && !e.rowadd && !e.resid && !e.drop_thr &&
                          e.drop_scale == 1.f && N % 4 == 0 && e.ldo % 4 == 0 && ((uintptr_t)e.out & 15) == 0;
  if (!lean_store || e.pool2 || e.colsum || e.sj_n4 || e.rs_ptr) return false;
  if (e.bias && ((uintptr_t)e.bias & 15)) return false;
  if (!lb.vok || dense_bytes(lb) >= (1L << 31)) return false;
  const int tile = auto_tile(M, N, 1);
  const int BN = tile == 128 ? 128 : 64;
  if (N % BN) return false;
  Epi ep = ep_in;
  ep.xcd_remap = 1;
  ep.vec_ok = true;
  for (int G = 2; G >= 1; --G) {
    const int BM = 128 * G;
    HaloGeom hg;
    if (M % BM || !halo_geom(la.Ho, la.Wo, la.C1, BM, &hg)) continue;
    constexpr int NB = 3;
    const int sme = G * (BN == 128 ? ConvHaloCfg<128, 1, NB>::SM_E : ConvHaloCfg<64, 1, NB>::SM_E);
    int lds = hg.pieces * 1024 + NB * BN * KSTAGE;
    if (lds < sme) lds = sme;
    if (lds > HALO_LDS_MAX) continue;
    const long nwg = (long)(M / BM) * (N / BN);
    if (mode == 1 && !halo_measured(fwd, la.Wo, la.C1, BN, G, nwg)) continue;
    bool ok;
    if (BN == 128) {
      ok = G == 2 ? conv_halo_launch<128, 2, NB>(la, lb, M, N, K, ep, hg, lds, st)
                  : conv_halo_launch<128, 1, NB>(la, lb, M, N, K, ep, hg, lds, st);
    } else {
      ok = G == 2 ? conv_halo_launch<64, 2, NB>(la, lb, M, N, K, ep, hg, lds, st)
                  : conv_halo_launch<64, 1, NB>(la, lb, M, N, K, ep, hg, lds, st);
    }
    if (!ok) return false;  // (the attribute was refused: the per-tap kernel takes the launch)
    ++conv_halo_count_ref();
    return true;
  }
  return false;
}

// (other element types keep the per-tap loader)
template <typename T>
inline bool conv_halo_try(const LdConvF<T>&, const LdDense<T, true>&, int, int, int, const Epi&, hipStream_t, bool) {
  return false;
}

}  // namespace hvit
