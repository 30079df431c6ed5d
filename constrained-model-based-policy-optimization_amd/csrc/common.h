// Shared helpers for the gfx950 C-ABI library (not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cmbpo_hip.h"

void cmbpo_set_error(const char *fmt, ...);
// the saved-activation block a Fisher-vector product on this batch would read (NULL: recompute); part of the key of a
// captured CG graph, whose kernel arguments contain it
const void *cmbpo_pi_act_token(const cmbpo_pi_t *h, const cmbpo_pi_batch_t *b);
// the handle's sample weights (NULL: none): an argument of the captured kernels too, so part of the same key
const void *cmbpo_pi_weights_token(const cmbpo_pi_t *h);
// CMBPO_EINVAL with the error set when the handle holds weights for another number of samples than the batch brings
int cmbpo_pi_weights_check(const cmbpo_pi_t *h, const cmbpo_pi_batch_t *b, const char *who);
// slots of the first-order loop's device state block (doubles; cmbpo_hip.h documents the layout, _lib.py mirrors it)
enum { ST_STOP = 0, ST_ITERS = 1, ST_KL = 2, ST_ADAM_T = 3, ST_PEN_PARAM = 4, ST_PEN_M = 5, ST_PEN_V = 6, ST_PEN_T = 7,
       ST_PENALTY = 8, ST_CR = 9, ST_CC = 10, ST_PRE = 11, ST_POST = 19, ST_CLIP = 27 };
static_assert(ST_CLIP < CMBPO_PPO_STATE_DOUBLES && ST_POST + 8 <= ST_CLIP, "state block layout");
// the update kernel of cmbpo_vec_adam_step at the t that d_state holds (vec_ops.hip); gated: return at entry once the
// first-order loop's stop word is set
int cmbpo_vec_adam_apply(int P, const float *d_g, float *d_m, float *d_v, float *d_theta, const double *d_state, float lr,
                         float beta1, float beta2, float eps, int gated, hipStream_t stream);
// Launch state of the current device (hipGetDevice), kept per device and safe to call from several host threads.
// CU count (256 if the query fails)
int cmbpo_cu_count();
// raise the dynamic-LDS limit of `kern` on the current device to at least `bytes` (the runtime is asked only when the
// device's high-water mark for the kernel grows); CMBPO_EHIP with the error set if it refuses
int cmbpo_grant_lds(const void *kern, size_t bytes);
template <typename K>
int cmbpo_grant_lds(K *kern, size_t bytes) { return cmbpo_grant_lds(reinterpret_cast<const void *>(kern), bytes); }

// The registered rule table behind a `task` argument >= CMBPO_TASK_USER_BASE (learned-cost bit allowed), with every clause's
// columns resolved against the launch's widths: col0 absolute, n_cols a count.  Host code only.  CMBPO_EINVAL with the error set
// (prefixed with `who`) for an unregistered id, columns outside the source's width, or an act clause without actions.
// out may be NULL (validation only).  The id's derived quantities (cmbpo_rule_derived_table_t) are checked with it -- a term's
// column inside its source's width, an act term with actions -- and go out resolved through out_derived (n_derived == 0: none).
int cmbpo_internal_task_rules_resolve(const char *who, int task, int obs_dim, int act_dim, bool have_act, cmbpo_task_rules_t *out,
                                      cmbpo_rule_derived_table_t *out_derived = nullptr);

#define CMBPO_HIP_CHECK(expr)                                                  \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      cmbpo_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),   \
                      __FILE__, __LINE__);                                     \
      return CMBPO_EHIP;                                                       \
    }                                                                          \
  } while (0)

#define CMBPO_REQUIRE(cond, ...)                                               \
  do {                                                                         \
    if (!(cond)) {                                                             \
      cmbpo_set_error(__VA_ARGS__);                                            \
      return CMBPO_EINVAL;                                                     \
    }                                                                          \
  } while (0)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

static inline int cmbpo_ceil_div(int a, int b) { return (a + b - 1) / b; }

// tanh as 1 - 2 / (1 + e^{2x}) with the hardware exp / rcp (absolute error ~1e-7, saturates correctly at +-1; the libm
// tanhf is ~30 VALU instructions per value, and VALU work next to a partner wave's fp32 MFMAs is the scarce resource of
// the 128-wide kernels' epilogues)
__device__ __forceinline__ float cmbpo_fast_tanh(float x) {
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x));
}

// A workgroup barrier that orders LDS traffic only: the LDS counter is drained, then s_barrier.  __syncthreads() is a
// workgroup-scope fence + s_barrier, in front of which hipcc waits vmcnt(0), i.e. for every global access still in flight;
// here the compiler still tracks the loads and waits for each one where its value is used.  NOT for a barrier that publishes
// LDS-DMA data (counted in vmcnt).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// sum over the 64 lanes of a wave, valid in lane 0
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// maximum over the 64 lanes of a wave, valid in every lane
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
