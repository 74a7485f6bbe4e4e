// Tile pieces shared by the register-resident attention kernels (bf16, head_dim
// 64): mhsa_fwd_v2, mhsa_dq_v2, mhsa_dkv_v2, mhsa_bwd_fused (attention.hip) and
// the fp8 forwards (attention_fp8.hip).  One definition each of the LDS image
// and its fragment reads, the MFMA -> VALU hazard pad, the keep-bit layout, the
// forward's dropout step, the key-major backward tile and the small row pieces.
#pragma once
#include <type_traits>

#include "common.h"

namespace hvit {

// The whole K and V (or Q and dO) of one (b, h) live in LDS as row-major
// [row][64] bf16 images (128-B rows, 16-B chunks XOR-swizzled by row & 7), so
// every tile is staged once per workgroup with plain 16-byte copies -- no
// transposed staging.  Scores are computed TRANSPOSED (S^T = K Q^T): the
// 16x16 MFMA accumulator then holds, per lane, 4 consecutive keys of one
// query, which is exactly the B-operand layout of v_mfma_f32_16x16x16_bf16,
// so P^T (and dS^T) feed the next MFMA straight from registers; the other
// operand (V^T, K^T, dO^T, Q^T) is read with ds_read_b64_tr_b16.  A lane's 4
// keys also form one dropout-hash group (one 64-bit hash per 16x16 tile).
constexpr int V2_ROWB = 128;  // bytes per 64-element bf16 row
typedef short v4s_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s_t lds_v4s_t;

__device__ __forceinline__ int v2_off(int row, int chunk) { return row * V2_ROWB + ((chunk ^ (row & 7)) << 4); }

// Same image filled by LDS-DMA (global_load_lds_dwordx4): no registers, no
// per-chunk load->store latency chain.  One wave-instruction writes 1 KiB =
// 8 rows; the destination is lane-linear, so the XOR swizzle moves to the
// source address (lane L fetches logical chunk (L%8) ^ row&7 of row 8p + L/8).
// Rows >= n re-read row n-1 (finite data; every use of those rows is masked or
// multiplied by an exact zero).  `rows` is a multiple of 8.
template <int WAVES>
__device__ __forceinline__ void v2_stage_glds(char* dst, const bf16_t* src, long pitch, int n, int rows) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int rl = lane >> 3, cp = lane & 7;
  for (int pc = w; pc < (rows >> 3); pc += WAVES) {
    const int row = pc * 8 + rl;
    const int srow = row < n ? row : n - 1;
    const bf16_t* g = src + (long)srow * pitch + ((cp ^ rl) << 3);
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)(dst + pc * 1024), 16, 0, 0);
  }
}
// 16x16x32 operand fragment: row `row`, k = 32*s + 8*fq .. +7
__device__ __forceinline__ u32x4 v2_frag(const char* img, int row, int s, int fq) {
  return *(const u32x4*)(img + v2_off(row, 4 * s + fq));
}
// transposed 4-row read: lane (g = lane>>4, i = lane&15) receives
// img[k0 + 4g + 0..3][c0 + i]  (k0 multiple of 16, c0 multiple of 16)
__device__ __forceinline__ v4s_t v2_tr(const char* img, int k0, int c0, int lane) {
  const int g = lane >> 4, li = lane & 15;
  const int row = k0 + 4 * g + (li >> 2);
  const int col = c0 + 4 * (li & 3);
  const char* a = img + row * V2_ROWB + (((col >> 3) ^ (row & 7)) << 4) + (col & 7) * 2;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_t*)a);
}
// Per-lane constant parts of the two read patterns (row = 16*j + lane part,
// and row & 7 depends on the lane part only), so a tile read is one LDS
// instruction at base + 2048*j + const.
struct V2Lane {
  int kc[2];  // v2_frag offsets for s = 0, 1 (row = frow)
  int tr[4];  // v2_tr offsets for column block t = 0..3 (rows 4g + li/4)
  __device__ __forceinline__ V2Lane(int lane) {
    const int frow = lane & 15, fq = lane >> 4;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) kc[s2] = frow * V2_ROWB + (((4 * s2 + fq) ^ (frow & 7)) << 4);
    const int r0 = 4 * fq + (frow >> 2), cb = (frow & 3) >> 1, inner = (frow & 1) * 8;
#pragma unroll
    for (int t = 0; t < 4; ++t) tr[t] = r0 * V2_ROWB + (((2 * t + cb) ^ (r0 & 7)) << 4) + inner;
  }
};
__device__ __forceinline__ u32x4 v2_fragj(const char* img, const V2Lane& L, int j, int s2) {
  return *(const u32x4*)(img + j * 16 * V2_ROWB + L.kc[s2]);
}
__device__ __forceinline__ v4s_t v2_trj(const char* img, const V2Lane& L, int j, int t) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_t*)(img + j * 16 * V2_ROWB + L.tr[t]));
}
__device__ __forceinline__ f32x4 v2_mma32(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, a), __builtin_bit_cast(s16x8, b), c, 0,
                                                 0, 0);
}
// Score tile straight from its MFMAs into a branch (the partial-tile mask):
// hipcc pads the MFMA -> VALU-read distance on the fall-through edge but not
// on the taken one (1-3 wait states in the .s where an 8-pass XDL result needs
// 11), so the wait goes inside a statement that takes the tile as an operand.
__device__ __forceinline__ void v2_settle(f32x4& a) { asm volatile("s_nop 7\n\ts_nop 3" : "+v"(a)); }
// 16x16x32 operand from two transposed 4-row reads (tiles jj and jj + 1):
// k = 8g + e  <->  row 16*(jj + e/4) + 4g + e%4
__device__ __forceinline__ u32x4 v2_cat(v4s_t lo, v4s_t hi) {
  const uint2 a = __builtin_bit_cast(uint2, lo), b = __builtin_bit_cast(uint2, hi);
  return (u32x4){a.x, a.y, b.x, b.y};
}
__device__ __forceinline__ u32x4 v2_trj2(const char* img, const V2Lane& L, int jj, int t) {
  return v2_cat(v2_trj(img, L, jj, t), v2_trj(img, L, jj + 1, t));
}
__device__ __forceinline__ v4s_t v2_pack(f32x4 v) {
  uint2 u;
  u.x = f2bf2(v[0], v[1]);
  u.y = f2bf2(v[2], v[3]);
  return __builtin_bit_cast(v4s_t, u);
}
// dropout multipliers of 4 consecutive keys kj..kj+3 (kj % 4 == 0) of query qi
__device__ __forceinline__ f32x4 v2_keep(uint64_t bh, int N, int qi, int kj, uint32_t thr, float dscale,
                                         unsigned long long seed, uint32_t site) {
  const uint64_t idx = (bh * N + qi) * (uint64_t)N + kj;
  return keep4_at(rng_key(seed, site), idx, thr, dscale);
}

// Column sums over a workgroup's rows of one head's [rows][64] gradient block
// held as acc[t][r] (column d = 16t + 4fq + r, row = the lane's query / key):
// the 16 lanes of a quarter (frow) by xor shuffles, the waves through LDS `red`
// ([WAVES][64] f32), then one plain store per column into out[0..63] (this
// workgroup's partial of the qkv bias gradient, attention.py:55; a later pass
// sums the partials: 32 workgroups adding to one address serialised at L2
// and cost more than the reduction pass they replaced).
template <int WAVES>
__device__ __forceinline__ void v2_colsum64(const f32x4 (&acc)[4], float mul, float* red, float* out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int frow = lane & 15, fq = lane >> 4;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      // the 16 rows of a quarter are one DPP row: rotate-and-add (row_ror 8,
      // 4, 2, 1) leaves the row sum in every lane, on the VALU (no LDS
      // permutes)
      float v = acc[t][r] * mul;
      v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false));
      v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xf, 0xf, false));
      v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x122, 0xf, 0xf, false));
      v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121, 0xf, 0xf, false));
      if (frow == 0) red[w * 64 + 16 * t + 4 * fq + r] = v;
    }
  __syncthreads();
  if (threadIdx.x < 64) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) s += red[i * 64 + threadIdx.x];
    out[threadIdx.x] = s;
  }
}

// ------------------------------------------------------------ keep bits ---
// The forward's attention-dropout decisions, one bit per (query, key), as the
// forward's lanes hold them: lane (query q, quarter fq) owns keys 16j + 4fq + r
// (tile j, r = 0..3) and stores, per 256-key chunk, one 64-bit word pair with
// tile j's four bits in nibble j.  The buffer is uint32 [chunk][b*h*query][fq][2]:
// key kl = 256*chunk + 32*jp + 16*e + 4*fq + r of query q is bit 8*jp + 4*e + r
// of pair (chunk, b, h, q, fq).  Mirror: tests/test_gpu_kernels.py.
// bit of key tile j's r = 0: pair jp = j / 2, tile e = j % 2 of the pair (= 4 * (j & 15))
__host__ __device__ constexpr int kb_nibble(int j) { return 8 * ((j & 15) >> 1) + 4 * (j & 1); }
__host__ __device__ constexpr int kb_bit(int kl) { return kb_nibble(kl >> 4) + (kl & 3); }  // in the 64-bit pair
// a query's 8 words [fq][2] of one chunk: word and bit inside it of chunk-relative key kl
__host__ __device__ constexpr int kb_word(int kl) { return ((kl >> 2) & 3) * 2 + (kb_bit(kl) >> 5); }
__host__ __device__ constexpr int kb_shift(int kl) { return kb_bit(kl) & 31; }
// word index of pair (chunk, row0 + query, fq): row0 = (b*H + h)*N, rows = B*H*N
__device__ __forceinline__ uint64_t kb_pair(int chunk, uint64_t rows, uint64_t row0, int q, int fq) {
  return (((uint64_t)chunk * rows + row0 + q) * 4 + fq) * 2;
}
// One (chunk, b, h)'s bits (`src` = its first pair, n queries) transposed into
// LDS as Kb[word][query], pitch `kbp` words: a lane's 4 query rows of one word
// are one 16-byte read.
template <int THREADS>
__device__ __forceinline__ void kb_stage_t(uint32_t* Kb, int kbp, const uint32_t* src, int n) {
  for (int i = threadIdx.x; i < n * 2; i += THREADS) {
    const u32x4 v = ((const u32x4*)src)[i];
    const int q = i >> 1, w0 = 4 * (i & 1);
#pragma unroll
    for (int e = 0; e < 4; ++e) Kb[(w0 + e) * kbp + q] = v[e];
  }
}

// Forward dropout of a lane's four keys (one tile): x is the 32-bit pair index
// of the first key's element index (query row base + key, both even, halved),
// the keys' hashes are pairs x and x + 1.  Dropped probabilities become 0 (the
// 1/(1-p) goes on the output); returns the keep nibble (bit r = key r kept).
__device__ __forceinline__ uint32_t v2_keep_step(uint32_t rk, uint32_t x, uint32_t thr, f32x4& p) {
  const uint32_t h0 = hash32(rk ^ x), h1 = hash32(rk ^ (x + 1u));
  const bool k0 = (h0 & 0xffffu) >= thr, k1 = (h0 >> 16) >= thr;
  const bool k2 = (h1 & 0xffffu) >= thr, k3 = (h1 >> 16) >= thr;
  p[0] = k0 ? p[0] : 0.f;
  p[1] = k1 ? p[1] : 0.f;
  p[2] = k2 ? p[2] : 0.f;
  p[3] = k3 ? p[3] : 0.f;
  return (uint32_t)k0 | ((uint32_t)k1 << 1) | ((uint32_t)k2 << 2) | ((uint32_t)k3 << 3);
}

// ------------------------------------------------- key-major backward tile ---
// S[q][key] form of mhsa_bwd_fused's instantiations: rows = queries
// 16j + 4fq + r, column = this lane's key.  From the score accumulator s and
// dp = dO V^T:  P = exp2(s c2 - lse2),  pd = P keep,  ds = P (dp keep - delta).
// kvalid: the lane's key < N (else P = 0); query rows >= N only in a partial
// last tile (wave-uniform branch; FULL: none).  The keep multipliers by MODE:
//   NONE  1 (its own dS statement: the same bits, and the parent's code);
//   BITS  the forward's bits from kb_stage_t's image: kbw = Kb + kb_word(key) *
//         pitch, kshift = kb_shift(key)  (rows >= N: p is 0 there);
// (The re-hash form V2_KEEP_HASH of mhsa_bwd_fused and mhsa_dkv_v2 keep their
// own copies, with the reasons there.)
enum { V2_KEEP_NONE = 0, V2_KEEP_BITS = 1, V2_KEEP_HASH = 2 };
template <bool FULL, int MODE>
__device__ __forceinline__ void v2_bwd_tile_km(const f32x4& s, const f32x4& dp, const f32x4& l4, const f32x4& d4,
                                               float c2, int j, int N, bool kvalid, const uint32_t* kbw, int kshift,
                                               float dscale, f32x4& pd, f32x4& ds) {
  static_assert(MODE == V2_KEEP_NONE || MODE == V2_KEEP_BITS, "v2_bwd_tile_km: mode");
  const int fq = (threadIdx.x & 63) >> 4;
  u32x4 kw4 = {0u, 0u, 0u, 0u};
  if (MODE == V2_KEEP_BITS) kw4 = *(const u32x4*)(kbw + 16 * j + 4 * fq);
  f32x4 p;
#pragma unroll
  for (int r = 0; r < 4; ++r) p[r] = kvalid ? __builtin_amdgcn_exp2f(fmaf(s[r], c2, -l4[r])) : 0.f;
  if (!FULL && 16 * j + 16 > N) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (16 * j + 4 * fq + r >= N) p[r] = 0.f;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float kp = 1.f;
    if constexpr (MODE == V2_KEEP_BITS) {
      kp = ((kw4[r] >> kshift) & 1u) ? dscale : 0.f;
    }
    if constexpr (MODE == V2_KEEP_NONE) {
      pd[r] = p[r];
      ds[r] = p[r] * (dp[r] - d4[r]);
    } else {
      pd[r] = p[r] * kp;
      ds[r] = p[r] * fmaf(dp[r], kp, -d4[r]);
    }
  }
}

// ------------------------------------------------------------ row pieces ---
// acc + dot of 8 bf16 pairs (packed two per word), low halves then high halves per word
__device__ __forceinline__ float v2_dot8(float acc, const u32x4& x, const u32x4& y) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
    acc += __uint_as_float(x[e] << 16) * __uint_as_float(y[e] << 16) +
           __uint_as_float(x[e] & 0xffff0000u) * __uint_as_float(y[e] & 0xffff0000u);
  return acc;
}
// a lane's 4 x 4 accumulator block of one 64-wide row, x mul, as bf16: columns 16t + 4fq + r
__device__ __forceinline__ void v2_store_row(bf16_t* row, const f32x4 (&acc)[4], float mul, int fq) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    uint2 u;
    u.x = f2bf2(acc[t][0] * mul, acc[t][1] * mul);
    u.y = f2bf2(acc[t][2] * mul, acc[t][3] * mul);
    *(uint2*)(row + 16 * t + 4 * fq) = u;
  }
}

// ------------------------------------------------------- forward body ---
// The v2 forward from the staged K / V images onwards (mhsa_fwd_v2 after its
// staging barrier; qkv_mhsa_fwd_fused after its qkv tile is in LDS): scores,
// softmax, dropout + keep bits, P V, the o rows and lse of this lane's query q
// of (b, h).  qf: the query's two 16x16x32 B-operand fragments; B: the batch
// (keep-bit chunk stride).  CH = 256 keys per softmax chunk (the
// register-resident score block).  Every argument is a reference to the
// caller's own variable: with by-value parameters hipcc orders the inlined
// body differently, and mhsa_fwd_v2<16, 256, true> no longer compiles to the
// instructions it had when this text stood in the kernel.
template <int KMAX, bool FULL>
__device__ __forceinline__ void v2_fwd_body(char* const& Ks, char* const& Vs, const V2Lane& LN,
                                            const u32x4 (&qf)[2], const int& frow, const int& fq, const int& q,
                                            const int& b, const int& h, const uint32_t& B,
                                            bf16_t* __restrict__ const& o, float* __restrict__ const& lse,
                                            const int& N, const int& H, const float& scale, const uint32_t& thr,
                                            const float& dscale, const unsigned long long& seed,
                                            const uint32_t& site, uint32_t* __restrict__ const& kbits) {
  constexpr int CH = 256;
  const int D = H * 64;
  const bool qin = FULL || q < N;
  const float c2 = scale * 1.4426950408889634f;
  const uint64_t bh = (uint64_t)b * H + h;
  const uint64_t BHN = (uint64_t)B * H * N;  // keep-bit chunk stride (queries)
  const uint32_t rk = rng_key(seed, site);
  const uint64_t qrow = (bh * N + (qin ? q : 0)) * (uint64_t)N;
  const uint32_t hq = (uint32_t)(qrow >> 1) + 2u * (uint32_t)fq;  // dropout-hash pair index of key 0
  // O^T[d][q] += V^T[d][keys] P^T[keys][q]   (4 d-blocks of 16)
  f32x4 ot[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) ot[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float mxc = -INFINITY, sum = 0.f;
  // one 256-key chunk (C0 = 0 or 256, compile time): its scores, the online
  // softmax update, P V; its keep bits
  auto chunk = [&](auto c0c) {
    constexpr int c0 = decltype(c0c)::value;
    const int nkt = FULL ? CH / 16 : (min(N - c0, CH) + 15) >> 4;  // key tiles of this chunk
    const char* Kc = Ks + c0 * V2_ROWB;
    const char* Vc = Vs + c0 * V2_ROWB;
    // S^T tiles: st[j][r] = raw score(key c0 + 16j + 4fq + r, query q)
    // (keys >= N of the last, partial tile masked to -inf).  VALU diet: the 1/sum
    // and the dropout 1/(1-p) on the 16 outputs instead of the 64
    // probabilities, the dropout mask a select, masking only in a partial tile.
    f32x4 st[CH / 16];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < CH / 16; ++j) {
      if (j < nkt) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        a = v2_mma32(v2_fragj(Kc, LN, j, 0), qf[0], a);
        a = v2_mma32(v2_fragj(Kc, LN, j, 1), qf[1], a);
        v2_settle(a);
        // (this kernel's own partial-tile mask: inlined from a shared v2_mask_max, hipcc
        // lays the branch out differently and the partial-tile forms grow,
        // 2093 -> 2131 and 3957 -> 4084 instructions, N = 496 forward 67.4 ->
        // 67.7 us.  In that layout hipcc pads the taken edge itself: whether the
        // MFMA -> VALU hazard shows depends on code layout, which is why
        // v2_settle stays whatever this branch compiles to.)
        if (!FULL && c0 + 16 * j + 16 > N) {  // wave-uniform: only a partial last tile
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (c0 + 16 * j + 4 * fq + r >= N) a[r] = -INFINITY;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, a[r]);
        st[j] = a;
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // raw scores kept; the scale folds into the exponent's fma (c2 > 0, so the
    // max commutes with it).  (Round 3 measured this form run-to-run
    // nondeterministic at the bf16-ulp level and scaled every score first: that
    // was the missing MFMA -> VALU wait of v2_settle, not the fma.)
    const float mnew = fmaxf(mxc, mx * c2);  // the running max in log2 units
    if constexpr (c0 > 0) {  // online softmax: rescale what the earlier chunks accumulated
      const float rs = __builtin_amdgcn_exp2f(mxc - mnew);
      sum *= rs;
#pragma unroll
      for (int t = 0; t < 4; ++t) ot[t] *= rs;
    }
    mxc = mnew;
    float csum = 0.f;
#pragma unroll
    for (int j = 0; j < CH / 16; ++j) {
      if (j < nkt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pv = __builtin_amdgcn_exp2f(fmaf(st[j][r], c2, -mxc));
          st[j][r] = pv;
          csum += pv;
        }
      }
    }
    csum += __shfl_xor(csum, 16, 64);
    csum += __shfl_xor(csum, 32, 64);
    sum += csum;
    // two key tiles per 16x16x32 MFMA: the B operand is this lane's P of tiles
    // 2jp, 2jp + 1 (keys c0 + 16(2jp + e/4) + 4fq + e%4), the A operand the
    // matching transposed reads of V.  A missing odd tile is P = 0 against
    // staged (finite) V rows.
    // this lane's keep-bit word pair of chunk c0/256 for the backward (kbits non-null)
    uint32_t kb[2] = {0u, 0u};
#pragma unroll
    for (int jp = 0; jp < CH / 32; ++jp) {
      if (2 * jp < nkt) {
        f32x4 p0 = st[2 * jp];
        f32x4 p1 = (2 * jp + 1 < nkt) ? st[2 * jp + 1] : (f32x4){0.f, 0.f, 0.f, 0.f};
        if (thr) {
          uint32_t b8 = 0u;  // the pair's two nibbles
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const int j = 2 * jp + e;
            if (j < nkt) {
              // rng_pair(rk, qrow + c0 + 16j + 4fq) and (.. + 2) in 32 bits:
              // qrow and the offset are even, so (qrow + off) >> 1 = qrow / 2 + off / 2
              const uint32_t nib = v2_keep_step(rk, hq + (uint32_t)(c0 / 2 + 8 * j), thr, e ? p1 : p0);
              b8 |= nib << (kb_nibble(j) - kb_nibble(2 * jp));
            }
          }
          kb[kb_nibble(2 * jp) >> 5] |= b8 << (kb_nibble(2 * jp) & 31);
        }
        const u32x4 pb = v2_cat(v2_pack(p0), v2_pack(p1));
#pragma unroll
        for (int t = 0; t < 4; ++t) ot[t] = v2_mma32(v2_trj2(Vc, LN, 2 * jp, t), pb, ot[t]);
      }
    }
    if (qin && kbits && thr)
      *(uint2*)(kbits + kb_pair(c0 / CH, BHN, bh * N, q, fq)) = make_uint2(kb[0], kb[1]);
  };
  chunk(std::integral_constant<int, 0>());
  if constexpr (KMAX > CH) {
    if (N > CH) chunk(std::integral_constant<int, CH>());
  }
  if (qin) {
    const float inv = 1.f / sum;
    const float os = thr ? inv * dscale : inv;
    v2_store_row(o + ((long)b * N + q) * D + h * 64, ot, os, fq);
    if (fq == 0) lse[bh * N + q] = (mxc + log2f(sum)) * 0.6931471805599453f;
  }
}

}  // namespace hvit
