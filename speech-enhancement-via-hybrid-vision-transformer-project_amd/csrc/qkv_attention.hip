// qkv Linear + attention forward in one launch (bf16, head_dim 64, N = 256).
//
// Reference: attention.py:55 (qkv = Linear(dim, 3 dim)) followed by
// attention.py:82-107 (softmax(q k^T scale) -> dropout -> @ v).  As two
// launches the 128x128 qkv GEMM pulls 768 KiB of operands per CU through
// LDS-DMA and the attention forward then stages K, V and Q of its (b, h) back
// from the qkv the GEMM just wrote.  Here one 16-wave workgroup per (b, h)
// computes exactly the 256 x 192 block of qkv that its attention needs --
// tokens of image b against head h's 64 q, 64 k and 64 v rows of W_qkv, 448
// KiB of operands per CU -- and hands it over in LDS.
//
//   phase 1   C^T[192][256] = W_h[192][D] x_b[256][D]^T through a two-stage
//             LDS ring filled by LDS-DMA (gemm.h's DmaImg pieces and source
//             swizzle), k ascending in v_mfma_f32_16x16x32_bf16 steps, one f32
//             chain per output, + bias in f32, round-to-nearest-even to bf16:
//             the operation order of the GEMM kernels' plain-store epilogue, so
//             qkv is bit-identical to hvit_linear_fwd's.  W is the MFMA's A
//             operand: a lane then holds 4 adjacent features of one token, one
//             8-byte LDS write.
//   hand-off  the rounded tile goes into three [256][64] images in
//             attention_tile.h's layout (v2_off), laid over the finished ring;
//             from there to global qkv in 16-byte nontemporal stores (skipped
//             when the caller keeps no qkv; not waited for: they drain under
//             phase 2), and each wave's Q fragments by two 16-byte reads.
//   phase 2   v2_fwd_body, the body of mhsa_fwd_v2<16, 256, true>.
//
// LDS-DMA ordering: a stage is read only after every wave waited for its own
// DMA instructions (vmcnt(0): two buffers, nothing younger in flight) and
// passed the barrier that follows; stage t + 1 is issued after that barrier
// into the buffer whose reads (stage t - 1) every wave waited for before its
// last MFMAs.  The fragment reads are asm (gemm.h: the compiler's wait-count
// pass would drain the just-issued DMA before a plain LDS read).  The last
// stage issues nothing, so the ring is idle when the images overwrite it.
#include "attention_tile.h"
#include "common.h"
#include "gemm_ring.h"

namespace hvit {

constexpr int QA_N = 256;                                     // tokens (= queries = keys) per image
using QaImgX = DmaImg<QA_N, true>;                            // x stage: 256 tokens x 64 k, 32 pieces
using QaImgW = DmaImg<64, true>;                              // one 64-row strip of W_qkv, 8 pieces
constexpr int QA_WBYTES = 3 * QaImgW::BYTES;                  // q, k, v strips: 24 KiB
constexpr int QA_STAGE = QA_WBYTES + QaImgX::BYTES;           // 56 KiB
constexpr int QA_IMG = QA_N * V2_ROWB;                        // one [256][64] bf16 image
constexpr int QA_SMEM = 2 * QA_STAGE > 3 * QA_IMG ? 2 * QA_STAGE : 3 * QA_IMG;
static_assert(QaImgX::PIECES == 32 && QaImgW::PIECES == 8, "pieces per stage");

template <int OFF>
__device__ __forceinline__ u32x4 ds128_asm(unsigned addr) {
  u32x4 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
  return r;
}

// grid (B, H): logical (b, h) from tile_of's XCD remap, h fastest -- the heads
// of an image share an XCD's L2 (x_b is fetched from HBM once, W_qkv stays resident)
__global__ __launch_bounds__(1024) void qkv_mhsa_fwd_fused(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wq,
                                                           const float* __restrict__ bias, bf16_t* __restrict__ qkv,
                                                           bf16_t* __restrict__ o, float* __restrict__ lse, int H,
                                                           float scale, uint32_t thr, float dscale, DSeed seed_,
                                                           uint32_t site, uint32_t* __restrict__ kbits) {
  const unsigned long long seed = seed_;
  __shared__ __attribute__((aligned(1024))) char smem[QA_SMEM];
  const int D = H * 64;
  const TileId bh3 = tile_of(1);
  const int b = bh3.mt, h = bh3.nt;
  const uint32_t B = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frow = lane & 15, fq = lane >> 4;
  // wave tile: 48 features (wn) x 64 tokens (wm) = 3 x 4 MFMA tiles
  const int wn = wid & 3, wm = wid >> 2;
  const int nk = D / 64;

  // ------------------------------------------------------------- phase 1 ---
  const bf16_t* xb = x + (long)b * QA_N * D;  // image b's tokens
  const bf16_t* wh = wq + (long)h * 64 * D;   // head h's q rows; k rows D further, v rows 2 D
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)xb, (short)0, QA_N * D * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw =
      __builtin_amdgcn_make_buffer_rsrc((void*)wh, (short)0, (2 * D + 64) * D * 2, 0x00020000);
  // this wave's pieces of a stage: x pieces wid and wid + 16; W pieces wid and
  // (waves 0..7) wid + 16 of the 24 (piece p: strip p / 8, rows 8 (p % 8) ..)
  const unsigned vx0 = QaImgX::src_off(wid, lane, D), vx1 = QaImgX::src_off(wid + 16, lane, D);
  const unsigned sbytes = (unsigned)D * (unsigned)D * 2u;  // one strip further in W_qkv
  const unsigned vw0 = QaImgW::src_off(wid & 7, lane, D) + (unsigned)(wid >> 3) * sbytes;
  const unsigned vw1 = QaImgW::src_off(wid & 7, lane, D) + 2u * sbytes;
  auto issue = [&](int t) {
    char* wbuf = smem + (t & 1) * QA_STAGE;
    char* xbuf = wbuf + QA_WBYTES;
    const unsigned so = (unsigned)t * 128u;  // 64 k further along both operands' rows
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(xbuf + wid * 1024), 16, vx0,
                                             so, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(xbuf + (wid + 16) * 1024),
                                             16, vx1, so, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)(wbuf + wid * 1024), 16, vw0,
                                             so, 0, 0);
    if (wid < 8)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)(wbuf + (wid + 16) * 1024),
                                               16, vw1, so, 0, 0);
  };
  // fragment addresses of k-steps 0 / 1 in stage buffer 0: row & 7 = frow & 7 for every tile of the wave
  const unsigned lds0 = lds_addr(smem);
  unsigned aw[2], ax[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    aw[s] = lds0 + kc_off(48 * wn + frow, 4 * s + fq);
    ax[s] = lds0 + QA_WBYTES + kc_off(64 * wm + frow, 4 * s + fq);
  }
  // acc[i][j][r] = C[token 64 wm + 16 j + frow][feature 48 wn + 16 i + 4 fq + r]
  f32x4 acc[3][4];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // the wave's bias values (features 48 wn + 16 i + 4 fq + 0..3 of [q | k | v] x head h)
  f32x4 bv[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int n = 48 * wn + 16 * i + 4 * fq;
    bv[i] = bias ? *(const f32x4*)(bias + (n >> 6) * D + h * 64 + (n & 63)) : (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  issue(0);
  for (int t = 0; t < nk; ++t) {
    __builtin_amdgcn_s_waitcnt(vm_imm(0));  // this wave's pieces of stage t landed ...
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();  // ... and every wave's; every wave is done reading stage t - 1
    asm volatile("" ::: "memory");
    const unsigned bo = (unsigned)(t & 1) * QA_STAGE;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      u32x4 fw[3], fx[4];
      const unsigned a = aw[s] + bo, c = ax[s] + bo;
      fw[0] = ds128_asm<0>(a);
      fw[1] = ds128_asm<2048>(a);
      fw[2] = ds128_asm<4096>(a);
      fx[0] = ds128_asm<0>(c);
      fx[1] = ds128_asm<2048>(c);
      fx[2] = ds128_asm<4096>(c);
      fx[3] = ds128_asm<6144>(c);
      // stage t + 1 into the other buffer, behind k-step 0's fragment reads
      if (s == 0 && t + 1 < nk) issue(t + 1);
      lgkm_wait0();
      lds_pin(fw);
      lds_pin(fx);
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, fw[i]),
                                                              __builtin_bit_cast(s16x8, fx[j]), acc[i][j], 0, 0, 0);
    }
  }
  // no DMA in flight (the last stage issued none); every wave done reading the ring
  __syncthreads();

  // ------------------------------------------------------------ hand-off ---
  // images [Q | K | V], each [256 tokens][64] in v2_off layout
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int n0 = 48 * wn + 16 * i;  // uniform: one strip per tile
    char* img = smem + (n0 >> 6) * QA_IMG;
    const int d0 = (n0 & 63) + 4 * fq;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 v = acc[i][j] + bv[i];
      uint2 u;
      u.x = f2bf2(v[0], v[1]);
      u.y = f2bf2(v[2], v[3]);
      *(uint2*)(img + v2_off(64 * wm + 16 * j + frow, d0 >> 3) + (d0 & 7) * 2) = u;
    }
  }
  __syncthreads();
  if (qkv) {  // saved for the backward: [B, N, 3, H, 64], 8 lanes per 128-byte row
#pragma unroll
    for (int u = 0; u < 3 * QA_IMG / 16 / 1024; ++u) {
      const int c = tid + 1024 * u;
      const int strip = c >> 11, row = (c >> 3) & (QA_N - 1), ch = c & 7;
      const u32x4 v = *(const u32x4*)(smem + strip * QA_IMG + v2_off(row, ch));
      // (nontemporal: nothing reads qkv before the backward; the lines need not stay in L2
      // beside o, which the proj GEMM reads next)
      bf16_t* dst = qkv + ((long)b * QA_N + row) * (3L * D) + strip * D + h * 64 + ch * 8;
      __builtin_nontemporal_store(v, (u32x4*)dst);
    }
  }
  const V2Lane LN(lane);
  const int w = tid >> 6;
  u32x4 qf[2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) qf[s2] = v2_fragj(smem, LN, w, s2);

  // ------------------------------------------------------------- phase 2 ---
  v2_fwd_body<QA_N, true>(smem + QA_IMG, smem + 2 * QA_IMG, LN, qf, frow, fq, 16 * w + frow, b, h, B, o, lse, QA_N, H,
                          scale, thr, dscale, seed, site, kbits);
}

// 1: fused where it applies (default); 0: hvit_linear_fwd + hvit_mhsa_fwd_kb (hvit_gemm_tune(11, v))
static int& qkv_attn_ref() {
  static int v = 1;
  return v;
}

}  // namespace hvit

using namespace hvit;

int hvit_qkv_attn_tune(int value) {
  const int old = qkv_attn_ref();
  if (value == 0 || value == 1) qkv_attn_ref() = value;
  return old;
}

extern "C" int hvit_qkv_mhsa_fused_used(int dt, int N, int hd, int D) {
  return qkv_attn_ref() != 0 && dt == HVIT_BF16 && hd == 64 && N == QA_N && D >= 64 && D % 64 == 0 ? 1 : 0;
}

extern "C" int hvit_qkv_mhsa_fwd(int dt, const void* x, const void* w, const float* bias, int B, int N, int H, int hd,
                                 float scale, const hvit_dropout_t* dropout, void* qkv, void* o, float* lse,
                                 unsigned* keep_bits, void* stream) {
  HVIT_CHECK(x && w && o && lse, "hvit_qkv_mhsa_fwd: null pointer");
  HVIT_CHECK(B > 0 && H > 0 && B <= 65535 && H <= 65535, "hvit_qkv_mhsa_fwd: bad shape B=%d H=%d", B, H);
  HVIT_CHECK(hvit_qkv_mhsa_fused_used(dt, N, hd, H * hd),
             "hvit_qkv_mhsa_fwd: no fused kernel for dt=%d N=%d hd=%d (hvit_qkv_mhsa_fused_used)", dt, N, hd);
  HVIT_CHECK(aligned16(x) && aligned16(w) && aligned16(bias) && aligned16(qkv) && aligned16(o) && aligned16(keep_bits),
             "hvit_qkv_mhsa_fwd: tensors must be 16-byte aligned");
  HVIT_CHECK((2L * H * 64 + 64) * H * 64 * 2 < (1L << 31), "hvit_qkv_mhsa_fwd: W_qkv too large");
  const DropArgs da = drop_args(dropout);
  hipLaunchKernelGGL(qkv_mhsa_fwd_fused, dim3(B, H), dim3(1024), 0, (hipStream_t)stream, (const bf16_t*)x,
                     (const bf16_t*)w, bias, (bf16_t*)qkv, (bf16_t*)o, lse, H, scale, da.thr, da.dscale, da.seed,
                     da.site, (uint32_t*)keep_bits);
  HVIT_LAUNCH_CHECK();
  return HVIT_OK;
}
