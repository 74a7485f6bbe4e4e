// Error reporting and the tuning-knob table of the C ABI (host only).
#include <stdarg.h>
#include <stdio.h>

#include "../../include/hvit.h"

static thread_local char g_err[1024] = "";

void hvit_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* hvit_last_error(void) { return g_err; }

extern "C" const char* hvit_version(void) { return "hvit 0.1 gfx950"; }

// Each knob lives in the file that owns the form it selects.
int hvit_ring_tune(int value);         // gemm_linear.hip
int hvit_c1_tune(int value);           // c1block.hip
int hvit_attn_tune(int value);         // attention.hip
int hvit_fp8_tune(int value);          // attention_fp8.hip
int hvit_wgrad_group_tune(int value);  // wgrad_group.hip
int hvit_conv_halo_tune(int value);    // gemm_conv.hip
int hvit_conv_halo_count();
int hvit_qkv_attn_tune(int value);     // qkv_attention.hip

extern "C" int hvit_gemm_tune(int what, int value) {
  switch (what) {
    case HVIT_TUNE_RING: return hvit_ring_tune(value);
    case HVIT_TUNE_C1_MFMA: return hvit_c1_tune(value);
    case HVIT_TUNE_ATTN_BWD: return hvit_attn_tune(value);
    case HVIT_TUNE_FP8_FWD: return hvit_fp8_tune(value);
    case HVIT_TUNE_WGRAD_GROUP: return hvit_wgrad_group_tune(value);
    case HVIT_TUNE_CONV_HALO: return hvit_conv_halo_tune(value);
    case HVIT_TUNE_CONV_HALO_COUNT: return hvit_conv_halo_count();
    case HVIT_TUNE_QKV_ATTN_FUSED: return hvit_qkv_attn_tune(value);
    default: return -1;  // 2, 3, 6, 8: retired with the forms they selected, not reused
  }
}
