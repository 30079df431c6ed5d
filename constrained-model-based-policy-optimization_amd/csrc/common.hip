// Error reporting, version and per-device launch state for the C-ABI library.
#include "common.h"

#include <stdarg.h>

#include <atomic>
#include <map>
#include <mutex>
#include <utility>

static thread_local char g_err[512] = "no error";

void cmbpo_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char *cmbpo_last_error(void) { return g_err; }

// 2: cmbpo_fakeenv_post_noise, cmbpo_rollout_t.xi / xi_stride; 3: cmbpo_train_extras_t, cmbpo_trainer_{step,epoch,losses}_ex
// (4: cmbpo_iv_gae_t;) 5: cmbpo_fakeenv_post_disagreement, cmbpo_disagreement_t, CMBPO_D_TOTAL_REW_VAR / _COST_VAR
// 6: cmbpo_replay_t, cmbpo_replay_{parts,compare,finish,run}
// (still 6 with cmbpo_critic_pair_predict_var, cmbpo_value_disagreement_t, CMBPO_D_TOTAL_V_VAR / _VC_VAR: additions only, and
// tests/test_replay_cpu.py holds the number at 6 -- ask for the symbols, as tests/test_value_disagreement_cabi.py does)
extern "C" int cmbpo_version(void) { return 6; }

namespace {
constexpr int kMaxDevices = 64;
std::atomic<int> g_cu_count[kMaxDevices];   // 0: not asked yet
std::mutex g_lds_mu;
std::map<std::pair<int, const void *>, size_t> g_lds_granted;   // (device, kernel) -> dynamic LDS already granted
}  // namespace

int cmbpo_cu_count() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  const bool cached = dev >= 0 && dev < kMaxDevices;
  int n = cached ? g_cu_count[dev].load(std::memory_order_relaxed) : 0;
  if (n == 0) {
    hipDeviceProp_t prop;
    n = (dev >= 0 && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount
                                                                                                       : 256;
    if (cached) g_cu_count[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

int cmbpo_grant_lds(const void *kern, size_t bytes) {
  int dev = 0;
  CMBPO_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(g_lds_mu);
  size_t &granted = g_lds_granted[{dev, kern}];
  if (bytes > granted) {
    CMBPO_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    granted = bytes;
  }
  return CMBPO_OK;
}
