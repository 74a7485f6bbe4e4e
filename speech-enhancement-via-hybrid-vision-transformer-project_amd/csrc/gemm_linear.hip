// C-ABI Linear fwd / dgrad / wgrad on the MFMA GEMM (see gemm_host.h).
#include "gemm_host.h"
#include "gemm_ring.h"

// The entry points below take q (hvit_gemm_plan): with it they run their own
// checks and choices on the operands as given -- the GEMM operands themselves are
// not passed and count as aligned, which the entry points require anyway -- and
// report the kernel in *q instead of launching it; no side job runs.
static int linear_fwd_impl(int dt, const void* x, const void* w, const float* bias, int M, int N, int K, void* y,
                           int y_dt, const hvit_epilogue_t* epi, void* stream, GemmPlan* q) {
  HVIT_CHECK(q || (x && w), "hvit_linear_fwd: null pointer");
  HVIT_CHECK(y, "hvit_linear_fwd: null pointer");
  HVIT_CHECK(M >= 0 && N > 0 && K > 0, "hvit_linear_fwd: bad shape M=%d N=%d K=%d", M, N, K);
  HVIT_CHECK(aligned16(x) && aligned16(w), "hvit_linear_fwd: x/w must be 16-byte aligned");
  if (int rc = check_epi(epi)) return rc;
  HVIT_CHECK(!epi || epi->act != HVIT_ACT_RELU, "hvit_linear_fwd: RELU is a conv-forward epilogue");
  Epi ep = to_epi(epi, y, y_dt, N);
  ep.bias = bias;
  if (!q)
    if (int rc = take_side(epi ? &epi->side : nullptr, ep, M, (hipStream_t)stream)) return rc;
  if (M == 0) return HVIT_OK;
  if (dt == HVIT_BF16) {
    int rc = 0;
    if (try_ring(dense<bf16_t, true>(x, K, M, K), dense<bf16_t, true>(w, K, N, K), M, N, K, 1, ep,
                 (hipStream_t)stream, &rc, -1, q))
      return rc;
  }
  DT_DISPATCH(dt, {
    HVIT_CHECK(K % Elem<T>::PER16 == 0, "hvit_linear_fwd: K=%d must be a multiple of %d", K, Elem<T>::PER16);
    return launch_gemm<T>(dense<T, true>(x, K, M, K), dense<T, true>(w, K, N, K), M, N, K, 1, ep,
                          (hipStream_t)stream, 0, q);
  });
}

extern "C" int hvit_linear_fwd(int dt, const void* x, const void* w, const float* bias, int M, int N, int K,
                               void* y, int y_dt, const hvit_epilogue_t* epi, void* stream) {
  return linear_fwd_impl(dt, x, w, bias, M, N, K, y, y_dt, epi, stream, nullptr);
}

static int linear_dgrad_impl(int dt, const void* dy, const void* w, int M, int N, int K, void* dx, int dx_dt,
                             const hvit_epilogue_t* epi, void* stream, GemmPlan* q) {
  HVIT_CHECK(q || (dy && w), "hvit_linear_dgrad: null pointer");
  HVIT_CHECK(dx, "hvit_linear_dgrad: null pointer");
  HVIT_CHECK(M >= 0 && N > 0 && K > 0, "hvit_linear_dgrad: bad shape");
  HVIT_CHECK(aligned16(dy) && aligned16(w), "hvit_linear_dgrad: alignment");
  if (int rc = check_epi(epi)) return rc;
  HVIT_CHECK(!epi || epi->act != HVIT_ACT_RELU, "hvit_linear_dgrad: RELU is a conv-forward epilogue");
  Epi ep = to_epi(epi, dx, dx_dt, K);
  if (!q)
    if (int rc = take_side(epi ? &epi->side : nullptr, ep, M, (hipStream_t)stream)) return rc;
  if (M == 0) return HVIT_OK;
  if (dt == HVIT_BF16 && N % 8 == 0) {
    int rc = 0;
    if (try_ring(dense<bf16_t, true>(dy, N, M, N), dense<bf16_t, false>(w, K, K, N), M, K, N, 1, ep,
                 (hipStream_t)stream, &rc, -1, q))
      return rc;
  }
  return hvit_gemm_kc_mn(dt, dy, w, M, K, N, ep, (hipStream_t)stream, "hvit_linear_dgrad: N, K alignment", q);
}

extern "C" int hvit_linear_dgrad(int dt, const void* dy, const void* w, int M, int N, int K, void* dx, int dx_dt,
                                 const hvit_epilogue_t* epi, void* stream) {
  return linear_dgrad_impl(dt, dy, w, M, N, K, dx, dx_dt, epi, stream, nullptr);
}

int hvit_gemm_kc_mn(int dt, const void* a, const void* b, int M, int N, int K, const Epi& ep, hipStream_t st,
                    const char* bad_align, GemmPlan* q) {
  DT_DISPATCH(dt, {
    HVIT_CHECK(N % Elem<T>::PER16 == 0 && K % Elem<T>::PER16 == 0, "%s", bad_align);
    return launch_gemm<T>(dense<T, true>(a, K, M, K), dense<T, false>(b, N, N, K), M, N, K, 1, ep, st, 0, q);
  });
}

bool hvit_wgrad_small_ok(int dt, int M, int N, int K);  // wgrad_small.hip
long long hvit_wgrad_small_ws(int M, int N, int K);
int hvit_wgrad_small(const void* dy, const void* x, int M, int N, int K, float* dw, float* db, float* ws,
                     long long ws_elems, void* stream,
                     hvit_slab_sum_t* job = nullptr);

// The plan: ring_pick / gemm.h per shape, split-K to ~256 workgroups.  (Eight
// fixed K slices for the token-major ViT shapes measured no faster, 5.179-5.185
// vs 5.174-5.187 ms/step: profiles/r6_ab_ln_dy_and_wgrad_plan.txt,
// profiles/r6_wgrad_layout_probe.txt.)
extern "C" long long hvit_wgrad_workspace(int M, int N, int K) {
  // dw is [N_out x K_in] reduced over M rows; slabs only when splitting, each
  // slab followed by N_out bias partials (enough for every tile configuration
  // the entry point may pick: gemm.h's 128x128, the ring's 128x128 / 128x64,
  // the tall-skinny kernel of wgrad_small.hip)
  const int s = std::max(wgrad_splits(N, K, M, LIN_WG_BM, LIN_WG_BN), wgrad_splits(N, K, M, 128, 64));
  const long long g = s > 1 ? (long long)s * ((long long)N * K + N) : 0;
  // + room for the two-level bias column sums of a tall dy (hvit_reduce_rows_ws)
  return std::max(std::max(g, 64LL * N),
                  hvit_wgrad_small_ok(HVIT_BF16, M, N, K) ? hvit_wgrad_small_ws(M, N, K) : 0LL);
}

// per-tile arrival counters of the in-kernel split-K reduction (ring kernels;
// the smallest tile any configuration uses, 128x64)
extern "C" long long hvit_wgrad_tickets(int M, int N, int K) {
  (void)M;
  return (long long)cdiv(N, 128) * cdiv(K, 64);
}

// db (nullable): bias gradient sum_m dy[m][n].  The fused path (bf16, db ==
// dw + N*K) takes it from the A tiles the wgrad GEMM already stages (row sums
// over the token reduction); otherwise a column reduction of dy.
static int linear_wgrad_impl(int dt, const void* dy, const void* x, int M, int N, int K, float* dw, float* db,
                             float* ws, long long ws_elems, unsigned* tickets, long long tickets_elems, int flags,
                             void* stream, hvit_slab_sum_t* job = nullptr,
                             const hvit_slab_sum_t* side = nullptr, GemmPlan* q = nullptr);

extern "C" int hvit_linear_wgrad(int dt, const void* dy, const void* x, int M, int N, int K, float* dw, float* db,
                                 float* ws, long long ws_elems, void* stream) {
  return linear_wgrad_impl(dt, dy, x, M, N, K, dw, db, ws, ws_elems, nullptr, 0, 0, stream);
}

extern "C" int hvit_linear_wgrad_tk(int dt, const void* dy, const void* x, int M, int N, int K, float* dw, float* db,
                                    float* ws, long long ws_elems, unsigned* tickets, long long tickets_elems, int flags,
                                    void* stream) {
  return linear_wgrad_impl(dt, dy, x, M, N, K, dw, db, ws, ws_elems, tickets, tickets_elems, flags, stream);
}

extern "C" int hvit_linear_wgrad_defer(int dt, const void* dy, const void* x, int M, int N, int K, float* dw,
                                       float* ws, long long ws_elems, const hvit_slab_sum_t* side,
                                       hvit_slab_sum_t* job, void* stream) {
  HVIT_CHECK(job, "hvit_linear_wgrad_defer: null job");
  *job = hvit_slab_sum_t{nullptr, nullptr, 0, 0, 0};
  return linear_wgrad_impl(dt, dy, x, M, N, K, dw, nullptr, ws, ws_elems, nullptr, 0, 0, stream, job, side);
}

// hvit_linear_wgrad_defer with the bias gradient: db == dw + N*K (or NULL);
// the tall-skinny path defers [dw | db] as one job, the others defer dw (when
// split) and finish db now
extern "C" int hvit_linear_wgrad_bias_defer(int dt, const void* dy, const void* x, int M, int N, int K, float* dw,
                                            float* db, float* ws, long long ws_elems, const hvit_slab_sum_t* side,
                                            hvit_slab_sum_t* job, void* stream) {
  HVIT_CHECK(job, "hvit_linear_wgrad_bias_defer: null job");
  *job = hvit_slab_sum_t{nullptr, nullptr, 0, 0, 0};
  return linear_wgrad_impl(dt, dy, x, M, N, K, dw, db, ws, ws_elems, nullptr, 0, 0, stream, job, side);
}

// the split-K slab sum: deferred into *job when the caller asked, else launched
static int slab_reduce(const float* ws, int splits, long long stride, long long n, float* out, void* stream,
                       hvit_slab_sum_t* job) {
  if (job) {
    *job = hvit_slab_sum_t{ws, out, n, stride, splits};
    return HVIT_OK;
  }
  return hvit_sum_slabs_strided(ws, splits, stride, n, out, stream);
}

static int linear_wgrad_impl(int dt, const void* dy, const void* x, int M, int N, int K, float* dw, float* db,
                             float* ws, long long ws_elems, unsigned* tickets, long long tickets_elems, int flags,
                             void* stream, hvit_slab_sum_t* job, const hvit_slab_sum_t* side, GemmPlan* q) {
  // (q: as linear_fwd_impl's; a workspace counts as present when ws_elems > 0)
  HVIT_CHECK(q || (dy && x), "hvit_linear_wgrad: null pointer");
  HVIT_CHECK(dw, "hvit_linear_wgrad: null pointer");
  const bool have_ws = q ? ws_elems > 0 : ws != nullptr;
  HVIT_CHECK(M >= 0 && N > 0 && K > 0, "hvit_linear_wgrad: bad shape");
  HVIT_CHECK(aligned16(dy) && aligned16(x), "hvit_linear_wgrad: alignment");
  hipStream_t st = (hipStream_t)stream;
  // a side job carried by this launch's GEMM kernels (epi_side); paths that
  // launch none of them run it first as its own reduction
  Epi sj;
  if (int rc = take_side(side, sj, M, st)) return rc;
  const long long NK = (long long)N * K;
  int splits = wgrad_splits(N, K, M, LIN_WG_BM, LIN_WG_BN);
  if ((long long)splits * (NK + N) > ws_elems || !have_ws) splits = 1;
  auto side_alone = [&]() -> int {
    if (!sj.sj_n4) return HVIT_OK;
    const int r = hvit_sum_slabs_strided(sj.sj_src, sj.sj_splits, sj.sj_stride4 * 4, sj.sj_n4 * 4, sj.sj_dst, stream);
    sj.sj_n4 = 0;
    return r;
  };
  auto carry = [&](Epi& e) {
    e.sj_src = sj.sj_src;
    e.sj_dst = sj.sj_dst;
    e.sj_n4 = sj.sj_n4;
    e.sj_stride4 = sj.sj_stride4;
    e.sj_splits = sj.sj_splits;
  };
  if (M == 0) {
    if (q) return HVIT_OK;
    if (int rc = side_alone()) return rc;
    (void)hipMemsetAsync(dw, 0, sizeof(float) * NK, st);
    if (db) (void)hipMemsetAsync(db, 0, sizeof(float) * N, st);
    return HVIT_OK;
  }
  // tall-skinny shapes (head, skip projections): one 64x64 tile per workgroup
  // over a chunk of rows
  if (!tickets && hvit_wgrad_small_ok(dt, M, N, K) && (!db || db == dw + NK) &&
      ws_elems >= hvit_wgrad_small_ws(M, N, K)) {
    if (q) return HVIT_OK;  // (the tall-skinny kernel, no GEMM tile: the plan stays empty)
    if (int rc = side_alone()) return rc;
    return hvit_wgrad_small(dy, x, M, N, K, dw, db, ws, ws_elems, stream, job);
  }
  const bool fused_db = db && dt == HVIT_BF16 && db == dw + NK;
  // ring-pipelined kernels (gemm_ring.h) for bf16 without fused bias row sums
  const int rcfg = ring_default_cfg() >= 0 ? ring_default_cfg() : ring_pick(false, false, N, K, M);
  if (dt == HVIT_BF16 && !fused_db && N % 8 == 0 && K % 8 == 0 && rcfg > 0) {
    const RingCfg r = ring_cfg(rcfg);
    int s = wgrad_splits(N, K, M, r.bm, r.bn);
    if ((long long)s * (NK + N) > ws_elems || !have_ws) s = 1;
    s = plan_splits<bf16_t>(M, s);
    Epi e;
    e.out_dt = HVIT_F32;
    e.ldo = K;
    e.mode = s > 1 ? EPI_SLAB : EPI_STORE;
    e.out = s > 1 ? (void*)ws : (void*)dw;
    e.slab_stride = NK + N;
    carry(e);
    // in-kernel reduction when the caller provides the ticket counters
    const bool tk = s > 1 && tickets && tickets_elems >= (long long)(N / r.bm) * (K / r.bn);
    if (tk) {
      e.tickets = tickets;
      e.red_out = dw;
      if (!q && !(flags & HVIT_ACC_ZEROED)) (void)hipMemsetAsync(tickets, 0, sizeof(unsigned) * (N / r.bm) * (K / r.bn), st);
    }
    int rc = 0;
    if (try_ring(dense<bf16_t, false>(dy, N, N, M), dense<bf16_t, false>(x, K, K, M), N, K, M, s, e, st, &rc, rcfg,
                 q)) {
      if (rc || q) return rc;
      if (s > 1 && !tk)
        if (int rc2 = slab_reduce(ws, s, NK + N, NK, dw, stream, job)) return rc2;
      // (the slabs are consumed on the stream before this reuses ws; a deferred job
      // has no bias gradient)
      if (db) return hvit_reduce_rows_ws(dy, dt, M, N, N, 0, db, job ? nullptr : ws, ws_elems, stream);
      return HVIT_OK;
    }
  }
  Epi ep;
  ep.out_dt = HVIT_F32;
  ep.ldo = K;
  carry(ep);
  DT_DISPATCH(dt, {
    HVIT_CHECK(N % Elem<T>::PER16 == 0 && K % Elem<T>::PER16 == 0, "hvit_linear_wgrad: N, K alignment");
    splits = plan_splits<T>(M, splits);
    ep.mode = splits > 1 ? EPI_SLAB : EPI_STORE;
    ep.out = splits > 1 ? (void*)ws : (void*)dw;
    ep.slab_stride = NK + N;
    if (fused_db) {
      ep.rs_ptr = splits > 1 ? ws + NK : db;
      ep.rs_stride = splits > 1 ? NK + N : 0;
    }
    int rc = launch_gemm<T>(dense<T, false>(dy, N, N, M), dense<T, false>(x, K, K, M), N, K, M, splits, ep, st,
                            LIN_WG_TILE, q);
    if (rc || q) return rc;
  });
  if (splits > 1) {
    // sums [dw | db] when fused (db follows dw), else dw alone
    if (int rc = slab_reduce(ws, splits, NK + N, fused_db ? NK + N : NK, dw, stream, fused_db ? nullptr : job))
      return rc;
  }
  if (db && !fused_db) return hvit_reduce_rows_ws(dy, dt, M, N, N, 0, db, job ? nullptr : ws, ws_elems, stream);
  return HVIT_OK;
}

// Diagnostics: which kernel the entry point would launch, from the entry points' own code
// (their *_impl with q set: same checks, same ring_plan / gemm_plan calls, no launch)
extern "C" int hvit_gemm_plan(int entry, int dt, int M, int N, int K, const float* bias, const void* out, int out_dt,
                              const hvit_epilogue_t* epi, long long ws_elems, hvit_gemm_plan_t* plan) {
  HVIT_CHECK(plan, "hvit_gemm_plan: null plan");
  GemmPlan q;
  int rc;
  switch (entry) {
    case HVIT_PLAN_LINEAR_FWD:
      rc = linear_fwd_impl(dt, nullptr, nullptr, bias, M, N, K, (void*)out, out_dt, epi, nullptr, &q);
      break;
    case HVIT_PLAN_LINEAR_DGRAD:
      rc = linear_dgrad_impl(dt, nullptr, nullptr, M, N, K, (void*)out, out_dt, epi, nullptr, &q);
      break;
    case HVIT_PLAN_LINEAR_WGRAD:
      rc = linear_wgrad_impl(dt, nullptr, nullptr, M, N, K, (float*)out, (float*)bias, nullptr, ws_elems, nullptr, 0, 0,
                             nullptr, nullptr, nullptr, &q);
      break;
    default: hvit_set_error("hvit_gemm_plan: bad entry %d", entry); return HVIT_ERR_ARG;
  }
  if (rc) return rc;
  plan->ring = q.ring;
  plan->tile = q.tile;
  plan->epi_kind = q.ek;
  plan->staging = q.stage;
  plan->splits = q.tile ? q.splits : 0;
  return HVIT_OK;
}

#ifdef HVIT_GEMM_STAMPS
__device__ unsigned long long hvit::g_gemm_stamps[65536 * 4];
extern "C" int hvit_debug_gemm_stamps(unsigned long long* host, int n) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(hvit::g_gemm_stamps), sizeof(unsigned long long) * n) == hipSuccess
             ? 0
             : 1;
}
#endif

// HVIT_TUNE_RING: the ring GEMM configuration of the bf16 linears (-1 =
// automatic per shape, 0 = gemm.h's kernels only, 2 / 4 / 5 = one ring
// configuration; see gemm_ring.h).  Returns the previous value; any other
// value changes nothing.
int hvit_ring_tune(int value) {
  const int old = ring_cfg_ref();
  if (value == -1 || value == 0 || value == 2 || value == 4 || value == 5) ring_cfg_ref() = value;
  return old;
}
