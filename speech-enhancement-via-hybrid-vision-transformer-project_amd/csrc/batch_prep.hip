// Training-batch assembly on the device: the reference's cached __getitem__
// (data/dataset.py:233-294), SpectrogramAugmenter.augment on the noisy side
// (data/augmentation.py:48-118) and collate_fn's right padding
// (data/dataset.py:297-347) as one launch over packed spectrogram stores.
//
// One block column per sample (blockIdx.y = b), blockIdx.x walks that sample's
// [F, Tb] plane in units of VEC adjacent frames.  Every block of a sample
// re-derives the sample's draws itself (about 2 * (nf + nt) + 2 hashes of
// uniform values), so no block reads a word another block writes; block x == 0
// alone records them in plan row b.
//
// Memory: destination rows start 16-byte aligned whenever Tb is a multiple of
// 4 (VEC = 4: one 16-byte store per lane and output, a wave writes 1 KiB
// contiguous).  Source rows are packed at stride T_i, which is arbitrary, so a
// unit's four source floats start at any 4-byte boundary: they are loaded as
// ONE 16-byte access of 4-byte alignment (gfx950 global loads need dword
// alignment only, and a wave still reads one contiguous 1 KiB run, touching at
// most one extra cache line).  The alternative, padding every stored row to a
// multiple of 4 frames, would cost up to 12 bytes per row of store memory and,
// more to the point, make an utterance's [F, T_i] block non-contiguous, so that
// building the store and handing out [1, F, T_i] views could no longer be plain
// copies; it buys nothing the 4-byte-aligned wide load does not already give.
// A unit that holds a masked or padded frame loads its live frames one by one
// under their predicates: masked and padded elements never touch the source.
#include "common.h"

namespace {

constexpr int BP_THREADS = 256;
constexpr uint32_t BP_SITE = 0xBA7Cu;    // rng_key site of the augmentation draws
constexpr uint32_t BP_DRAWS = 64;        // draw slots per sample (2 * 2 * HVIT_AUG_MAX_MASKS + 2 used at most)

typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));  // a 16-byte access at 4-byte alignment

struct BatchPrepArgs {
  const float* noisy_store;
  const float* clean_store;
  const long long* offsets;
  const int* frames;
  const int* idx;
  const unsigned long long* seed_ptr;
  float* noisy;
  float* clean;
  int* plan;
  int n_utts, F, Tb;
  int enabled, nf, wf, nt, wt;
  unsigned long long gain_thr;  // floor(gain_prob * 2^32), 2^32 when gain_prob >= 1
  float db_lo, db_hi;
  FastDiv row_div;  // by Tb / VEC
};

// draw j of sample b: a stateless function of (key, b, j)
__device__ __forceinline__ uint32_t draw_u32(uint32_t key, uint32_t b, uint32_t j) {
  return hash32(key ^ (b * BP_DRAWS + j));
}
// numpy.random.randint(0, n) for n >= 1 (n == 0 gives 0)
__device__ __forceinline__ int draw_int(uint32_t u, int n) { return (int)(((uint64_t)u * (uint64_t)(uint32_t)n) >> 32); }

template <int VEC>
__global__ __launch_bounds__(BP_THREADS) void batch_prep_kernel(const BatchPrepArgs a) {
  __shared__ int s_f0[HVIT_AUG_MAX_MASKS], s_f1[HVIT_AUG_MAX_MASKS];
  __shared__ int s_t0[HVIT_AUG_MAX_MASKS], s_t1[HVIT_AUG_MAX_MASKS];
  __shared__ float s_gain;
  const int b = blockIdx.y;
  int i = a.idx[b];
  i = i < 0 ? 0 : (i >= a.n_utts ? a.n_utts - 1 : i);  // a bad index reads a stored clip, never outside the stores
  int T = a.frames[i];
  T = T < 0 ? 0 : (T > a.Tb ? a.Tb : T);               // never past the destination row
  const long long off = a.offsets[i];
  const int nf = a.enabled ? a.nf : 0, nt = a.enabled ? a.nt : 0;

  if (threadIdx.x == 0) {
    const int pw = 2 * a.nf + 2 * a.nt + 2;
    int* row = (blockIdx.x == 0) ? a.plan + (long)b * pw : nullptr;
    float gain = 1.f;
    int drawn = 0;
    if (a.enabled) {
      const uint32_t key = rng_key(*a.seed_ptr, BP_SITE);
      uint32_t j = 0;
      for (int m = 0; m < nf; ++m) {  // augmentation.py:89-92
        const int f = draw_int(draw_u32(key, b, j), a.wf);
        const int hi = a.F - f;
        const int f0 = draw_int(draw_u32(key, b, j + 1), hi > 1 ? hi : 1);
        j += 2;
        s_f0[m] = f0;
        s_f1[m] = f0 + f;  // a slice end past F stops at the edge: rows f0 <= r < min(f0 + f, F)
        if (row) row[2 * m] = f0, row[2 * m + 1] = f;
      }
      for (int m = 0; m < nt; ++m) {  // augmentation.py:95-98, on the sample's own frame count
        const int t = draw_int(draw_u32(key, b, j), a.wt < T ? a.wt : T);
        const int hi = T - t;
        const int t0 = draw_int(draw_u32(key, b, j + 1), hi > 1 ? hi : 1);
        j += 2;
        s_t0[m] = t0;
        s_t1[m] = t0 + t;
        if (row) row[2 * nf + 2 * m] = t0, row[2 * nf + 2 * m + 1] = t;
      }
      drawn = (unsigned long long)draw_u32(key, b, j) < a.gain_thr;  // augmentation.py:63
      if (drawn) {  // augmentation.py:115-116: uniform dB, 10^(dB / 20), no clipping
        const float r = (float)(draw_u32(key, b, j + 1) >> 8) * 0x1p-24f;
        const float db = __fadd_rn(a.db_lo, __fmul_rn(a.db_hi - a.db_lo, r));
        gain = exp2f(__fmul_rn(db, 0.16609640474436813f));  // log2(10) / 20
      }
    } else if (row) {
      for (int k = 0; k < pw - 2; ++k) row[k] = 0;
    }
    if (row) row[pw - 2] = drawn, row[pw - 1] = __float_as_int(gain);
    s_gain = gain;
  }
  __syncthreads();
  const float gain = s_gain;

  const int per_row = a.Tb / VEC;
  const int units = a.F * per_row;
  const float* __restrict__ src_n = a.noisy_store + off;
  const float* __restrict__ src_c = a.clean_store + off;
  float* __restrict__ dst_n = a.noisy + (long)b * a.F * a.Tb;
  float* __restrict__ dst_c = a.clean + (long)b * a.F * a.Tb;
  // one unit per thread: more waves in flight measured faster than 2 or 4 units per thread (20.0 / 21.0 /
  // 22.4 us for B = 32, F = 257, Tb = 400 with the seed launch, profiles/batch_prep_bench.txt)
  const int u = blockIdx.x * BP_THREADS + threadIdx.x;
  if (u >= units) return;
  const int f = a.row_div.div(u);
  const int t = (u - f * per_row) * VEC;
  bool row_dead = false;
  for (int m = 0; m < nf; ++m) row_dead |= (f >= s_f0[m]) & (f < s_f1[m]);
  unsigned pad = 0, dead = 0;  // bit e: frame t + e is padding / is padding or masked
#pragma unroll
  for (int e = 0; e < VEC; ++e) pad |= (unsigned)(t + e >= T) << e;
  dead = row_dead ? (1u << VEC) - 1u : pad;
  if (!row_dead) {
    for (int m = 0; m < nt; ++m) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) dead |= (unsigned)((t + e >= s_t0[m]) & (t + e < s_t1[m])) << e;
    }
  }
  const long s = (long)f * T + t;
  float c[VEC], n[VEC];
  if (VEC == 4 && pad == 0) {
    const f32x4_u v = *(const f32x4_u*)(src_c + s);
#pragma unroll
    for (int e = 0; e < VEC; ++e) c[e] = v[e];
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) c[e] = ((pad >> e) & 1u) ? 0.f : src_c[s + e];
  }
  if (VEC == 4 && dead == 0) {
    const f32x4_u v = *(const f32x4_u*)(src_n + s);
#pragma unroll
    for (int e = 0; e < VEC; ++e) n[e] = v[e] * gain;
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) n[e] = ((dead >> e) & 1u) ? 0.f : src_n[s + e] * gain;
  }
  const long d = (long)f * a.Tb + t;
  if (VEC == 4) {
    *(f32x4*)(dst_c + d) = (f32x4){c[0], c[1], c[2], c[3]};
    *(f32x4*)(dst_n + d) = (f32x4){n[0], n[1], n[2], n[3]};
  } else {
    dst_c[d] = c[0];
    dst_n[d] = n[0];
  }
}

}  // namespace

extern "C" int hvit_batch_prep(const float* noisy_store, const float* clean_store, const long long* offsets,
                               const int* frames, int n_utts, const int* idx, int B, int F, int Tb, int max_frames,
                               const hvit_augment_cfg_t* cfg, const unsigned long long* seed_ptr, float* noisy,
                               float* clean, int* plan, void* stream) {
  HVIT_CHECK(noisy_store && clean_store && offsets && frames && idx && cfg && noisy && clean && plan,
             "hvit_batch_prep: null pointer");
  HVIT_CHECK(B >= 1 && B <= 65535, "hvit_batch_prep: B=%d (1..65535)", B);
  HVIT_CHECK(n_utts >= 1 && F >= 1 && Tb >= 1 && (long long)F * Tb < (1ll << 31),
             "hvit_batch_prep: n_utts=%d F=%d Tb=%d", n_utts, F, Tb);
  HVIT_CHECK(max_frames >= 1 && Tb >= max_frames,
             "hvit_batch_prep: Tb=%d is smaller than a selected clip's %d frames", Tb, max_frames);
  HVIT_CHECK(cfg->freq_mask_num >= 0 && cfg->freq_mask_num <= HVIT_AUG_MAX_MASKS && cfg->time_mask_num >= 0 &&
                 cfg->time_mask_num <= HVIT_AUG_MAX_MASKS,
             "hvit_batch_prep: freq_mask_num=%d time_mask_num=%d (0..%d)", cfg->freq_mask_num, cfg->time_mask_num,
             HVIT_AUG_MAX_MASKS);
  // numpy.random.randint(0, 0) raises (augmentation.py:90, :96)
  HVIT_CHECK(cfg->freq_mask_num == 0 || cfg->freq_mask_width >= 1,
             "hvit_batch_prep: freq_mask_width=%d with freq_mask_num=%d", cfg->freq_mask_width, cfg->freq_mask_num);
  HVIT_CHECK(cfg->time_mask_num == 0 || cfg->time_mask_width >= 1,
             "hvit_batch_prep: time_mask_width=%d with time_mask_num=%d", cfg->time_mask_width, cfg->time_mask_num);
  HVIT_CHECK(!cfg->enabled || seed_ptr, "hvit_batch_prep: augmentation enabled without a seed word");
  HVIT_CHECK(!cfg->enabled || (cfg->gain_prob == cfg->gain_prob && cfg->gain_db_lo == cfg->gain_db_lo &&
                               cfg->gain_db_hi == cfg->gain_db_hi),
             "hvit_batch_prep: NaN in the gain settings");
  HVIT_CHECK((((uintptr_t)noisy_store | (uintptr_t)clean_store | (uintptr_t)noisy | (uintptr_t)clean) & 3) == 0 &&
                 (((uintptr_t)offsets | (uintptr_t)seed_ptr) & 7) == 0,
             "hvit_batch_prep: misaligned pointer");
  BatchPrepArgs a;
  a.noisy_store = noisy_store, a.clean_store = clean_store, a.offsets = offsets, a.frames = frames, a.idx = idx;
  a.seed_ptr = seed_ptr, a.noisy = noisy, a.clean = clean, a.plan = plan;
  a.n_utts = n_utts, a.F = F, a.Tb = Tb;
  a.enabled = cfg->enabled ? 1 : 0;
  a.nf = cfg->freq_mask_num, a.wf = cfg->freq_mask_width, a.nt = cfg->time_mask_num, a.wt = cfg->time_mask_width;
  const double p = (double)cfg->gain_prob;
  a.gain_thr = p >= 1.0 ? (1ull << 32) : (p <= 0.0 ? 0ull : (unsigned long long)(p * 4294967296.0));
  a.db_lo = cfg->gain_db_lo, a.db_hi = cfg->gain_db_hi;
  const bool vec = (Tb % 4 == 0) && aligned16(noisy) && aligned16(clean);
  const int per_row = vec ? Tb / 4 : Tb;
  a.row_div = FastDiv(per_row);
  const dim3 grid(cdiv((long)F * per_row, BP_THREADS), B);
  if (vec)
    hipLaunchKernelGGL(batch_prep_kernel<4>, grid, dim3(BP_THREADS), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(batch_prep_kernel<1>, grid, dim3(BP_THREADS), 0, (hipStream_t)stream, a);
  HVIT_LAUNCH_CHECK();
  return HVIT_OK;
}
