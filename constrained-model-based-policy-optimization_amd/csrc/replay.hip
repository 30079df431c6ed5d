// Open-loop model validation: k-step replay of real trajectories.
//
// A replay takes B windows of up to H consecutive real steps, starts the model at each window's first real observation and
// applies the recorded actions; at every horizon h it holds the model's prediction against what was recorded.  The stepping is
// the existing cmbpo_ens_forward + cmbpo_fakeenv_post (the unpenalised means, no noise); what is new is the comparison:
//   replay_compare_kernel   one horizon step: per-row verdicts, squared errors, 2x2 counts, the row's next state
//   replay_finish_kernel    per-workgroup partials -> the [H] result table, in slot order
// Sums are float64, counts int64, every addition in a fixed order (no floating-point atomics): two runs are bitwise equal.
#include "common.h"

namespace {

constexpr int kRows = 64;       // rows of one workgroup = lanes of one wave: wave 0 owns the per-row scalars, one lane per row
constexpr int kThreads = 256;
constexpr int kScalarSums = CMBPO_REPLAY_SCALAR_SUMS;  // se_rew, se_cost, sum ep_var_mean, sum dkl_path -- behind the obs_dim column sums
constexpr int kCounts = CMBPO_REPLAY_COUNTS;           // n, n_nonfinite, cost_cm[2][2], term_cm[2][2]

__device__ __forceinline__ int64_t lanes_set(bool p) { return (int64_t)__popcll(__ballot(p)); }

// One workgroup = kRows consecutive windows.  The [rows, obs_dim] tile of a row-major array is one contiguous run of
// rows * obs_dim floats, so the threads walk it flat: thread t starts at element t and advances by `stride` =
// (kThreads / obs_dim) * obs_dim elements, a whole number of rows -- every wave-instruction reads consecutive floats, a
// thread stays on one column (its sum needs no cross-lane step), and only kThreads % obs_dim < obs_dim threads have no
// element (3 of 256 at 11 columns, 24 at 29): no wave idles on the column tail.  obs_dim > kThreads: stride = kThreads
// columns of one row, the row loop outside.
__global__ __launch_bounds__(kThreads) void replay_compare_kernel(cmbpo_replay_t rp, int h) {
  __shared__ uint8_t s_alive[kRows];   // alive on entry
  __shared__ int s_bad[kRows];         // a non-finite prediction in the row
  __shared__ uint8_t s_ok[kRows];      // alive and finite: the row is summed
  __shared__ uint8_t s_next[kRows];    // lives on to h + 1: cur_obs is written
  __shared__ double s_col[kThreads];   // per-thread column sums, folded by the first obs_dim threads

  const int t = threadIdx.x;
  const int B = rp.B, D = rp.obs_dim;
  const int row0 = blockIdx.x * kRows;
  const int rows = min(kRows, B - row0);
  const size_t hb = (size_t)h * B;
  const int C = D + kScalarSums;
  double *psum = rp.part_sum + ((size_t)h * gridDim.x + blockIdx.x) * C;
  int64_t *pcnt = rp.part_cnt + ((size_t)h * gridDim.x + blockIdx.x) * kCounts;

  float p_rew = 0.0f, p_cost = 0.0f;
  if (t < kRows) {
    const bool in = t < rows;
    const bool alive = in && rp.alive[row0 + t] != 0;
    if (alive) { p_rew = rp.p_rew[row0 + t]; p_cost = rp.p_cost[row0 + t]; }
    s_alive[t] = alive;
    s_bad[t] = (alive && !(isfinite(p_rew) && isfinite(p_cost))) ? 1 : 0;
  }
  __syncthreads();

  // pass 1: a non-finite predicted observation marks its row (integer LDS atomic: order cannot matter)
  const float *pred = rp.p_next_obs + (size_t)row0 * D;
  const int total = rows * D;
  for (int i = t; i < total; i += kThreads) {
    const float v = pred[i];
    const int r = i / D;
    if (s_alive[r] && !isfinite(v)) atomicOr(&s_bad[r], 1);
  }
  __syncthreads();

  // the rows' verdicts, scalar sums and counts: wave 0, lane = row
  if (t < kRows) {
    const bool alive = s_alive[t] != 0;
    const bool bad = alive && s_bad[t] != 0;
    const bool ok = alive && !bad;
    double se_r = 0.0, se_c = 0.0, epv = 0.0, dkl = 0.0;
    bool rc = false, pc = false, rt = false, pt = false, next = false;
    if (ok) {
      const float r_rew = rp.rew[hb + row0 + t], r_cost = rp.cost[hb + row0 + t];
      const float er = __fsub_rn(p_rew, r_rew), ec = __fsub_rn(p_cost, r_cost);
      se_r = (double)er * (double)er;
      se_c = (double)ec * (double)ec;
      epv = (double)rp.p_ep_var_mean[row0 + t];
      dkl = (double)rp.p_dkl_path[row0 + t];
      rc = r_cost > 0.0f;
      pc = p_cost > 0.5f;
      rt = rp.term[hb + row0 + t] != 0;
      pt = rp.p_term[row0 + t] != 0;
      next = h + 1 < rp.len[row0 + t] && !rt && !(rp.mode == CMBPO_REPLAY_OPEN_LOOP && pt);
    }
    s_ok[t] = ok;
    s_next[t] = next;
    if (alive && !next) rp.alive[row0 + t] = 0;
    se_r = wave_sum(se_r);
    se_c = wave_sum(se_c);
    epv = wave_sum(epv);
    dkl = wave_sum(dkl);
    const int64_t cnt[kCounts] = {lanes_set(ok),        lanes_set(bad),
                                  lanes_set(ok && !rc && !pc), lanes_set(ok && !rc && pc),
                                  lanes_set(ok && rc && !pc),  lanes_set(ok && rc && pc),
                                  lanes_set(ok && !rt && !pt), lanes_set(ok && !rt && pt),
                                  lanes_set(ok && rt && !pt),  lanes_set(ok && rt && pt)};
    if (t == 0) {
      psum[D + 0] = se_r; psum[D + 1] = se_c; psum[D + 2] = epv; psum[D + 3] = dkl;
#pragma unroll
      for (int k = 0; k < kCounts; ++k) pcnt[k] = cnt[k];
    }
  }
  __syncthreads();

  // pass 2: squared errors per column (the predictions come from L1 / L2 this time) and the rows' next state
  const float *real = rp.next_obs + (hb + row0) * D;
  float *cur = rp.cur_obs + (size_t)row0 * D;
  const bool open = rp.mode == CMBPO_REPLAY_OPEN_LOOP;
  const int W = min(D, kThreads);          // columns of one sweep
  const int rpp = kThreads / W;            // rows of one sweep: thread t starts at element t, a sweep is rpp * W of them
  for (int c0 = 0; c0 < D; c0 += W) {      // (one trip unless obs_dim > kThreads)
    const int r0 = t / W, c = c0 + t % W;
    double acc = 0.0;
    if (r0 < rpp && c < D) {
      for (int r = r0, i = r0 * D + c; r < rows; r += rpp, i += rpp * D) {
        if (!s_ok[r]) continue;
        const float p = pred[i], q = real[i];
        const float e = __fsub_rn(p, q);
        acc += (double)e * (double)e;
        if (s_next[r]) cur[i] = open ? p : q;
      }
    }
    s_col[t] = acc;
    __syncthreads();
    if (t < W && c0 + t < D) {
      double s = s_col[t];
      for (int k = 1; k < rpp; ++k) s += s_col[k * W + t];
      psum[c0 + t] = s;
    }
    __syncthreads();
  }
}

// table[h][j] = sum over the slots, in slot order; one workgroup per horizon, one thread per entry
__global__ __launch_bounds__(kThreads) void replay_finish_kernel(cmbpo_replay_t rp, int n_part) {
  const int h = blockIdx.x;
  const int C = rp.obs_dim + kScalarSums;
  for (int j = threadIdx.x; j < C + kCounts; j += kThreads) {
    if (j < C) {
      const double *p = rp.part_sum + (size_t)h * n_part * C + j;
      double s = 0.0;
      for (int k = 0; k < n_part; ++k) s += p[(size_t)k * C];
      rp.sums[(size_t)h * C + j] = s;
    } else {
      const int64_t *p = rp.part_cnt + (size_t)h * n_part * kCounts + (j - C);
      int64_t s = 0;
      for (int k = 0; k < n_part; ++k) s += p[(size_t)k * kCounts];
      rp.counts[(size_t)h * kCounts + (j - C)] = s;
    }
  }
}

int check_shape(const char *who, const cmbpo_replay_t *rp) {
  CMBPO_REQUIRE(rp != nullptr, "%s: descriptor is NULL", who);
  CMBPO_REQUIRE(rp->B >= 1, "%s: B %d < 1", who, rp->B);
  CMBPO_REQUIRE(rp->H >= 1, "%s: H %d < 1", who, rp->H);
  CMBPO_REQUIRE(rp->obs_dim >= 1 && rp->obs_dim <= 512 && rp->act_dim >= 0, "%s: bad dims (obs_dim %d, act_dim %d)", who,
                rp->obs_dim, rp->act_dim);
  CMBPO_REQUIRE(rp->mode == CMBPO_REPLAY_OPEN_LOOP || rp->mode == CMBPO_REPLAY_ONE_STEP, "%s: unknown mode %d", who, rp->mode);
  CMBPO_REQUIRE(rp->reserved == 0, "%s: reserved %d != 0", who, rp->reserved);
  return CMBPO_OK;
}

int check_compare(const char *who, const cmbpo_replay_t *rp) {
  if (int rc = check_shape(who, rp)) return rc;
  CMBPO_REQUIRE(rp->next_obs && rp->rew && rp->cost && rp->term && rp->len, "%s: NULL buffer (recorded arrays)", who);
  CMBPO_REQUIRE(rp->cur_obs && rp->alive, "%s: NULL buffer (cur_obs / alive)", who);
  CMBPO_REQUIRE(rp->p_next_obs && rp->p_rew && rp->p_term && rp->p_cost && rp->p_dkl_path && rp->p_ep_var_mean,
                "%s: NULL buffer (predictions)", who);
  CMBPO_REQUIRE(rp->part_sum && rp->part_cnt, "%s: NULL buffer (partials)", who);
  return CMBPO_OK;
}

int check_finish(const char *who, const cmbpo_replay_t *rp) {
  if (int rc = check_shape(who, rp)) return rc;
  CMBPO_REQUIRE(rp->part_sum && rp->part_cnt, "%s: NULL buffer (partials)", who);
  CMBPO_REQUIRE(rp->sums && rp->counts, "%s: NULL buffer (result table)", who);
  return CMBPO_OK;
}

int launch_compare(const cmbpo_replay_t *rp, int h, hipStream_t s) {
  hipLaunchKernelGGL(replay_compare_kernel, dim3(cmbpo_replay_parts(rp->B)), dim3(kThreads), 0, s, *rp, h);
  CMBPO_HIP_CHECK(hipGetLastError());
  return CMBPO_OK;
}

int launch_finish(const cmbpo_replay_t *rp, hipStream_t s) {
  hipLaunchKernelGGL(replay_finish_kernel, dim3(rp->H), dim3(kThreads), 0, s, *rp, cmbpo_replay_parts(rp->B));
  CMBPO_HIP_CHECK(hipGetLastError());
  return CMBPO_OK;
}

// a callee's refusal, passed on under this entry point's name
int refused_by(const char *who, int rc) {
  char inner[400];
  snprintf(inner, sizeof(inner), "%s", cmbpo_last_error());
  cmbpo_set_error("%s: %s", who, inner);
  return rc;
}

}  // namespace

extern "C" int cmbpo_replay_parts(int n_rows) { return n_rows >= 1 ? cmbpo_ceil_div(n_rows, kRows) : 0; }

extern "C" int cmbpo_replay_compare(const cmbpo_replay_t *rp, int h, void *stream) {
  const char *who = "cmbpo_replay_compare";
  if (int rc = check_compare(who, rp)) return rc;
  CMBPO_REQUIRE(h >= 0 && h < rp->H, "%s: h %d outside [0, %d)", who, h, rp->H);
  return launch_compare(rp, h, (hipStream_t)stream);
}

extern "C" int cmbpo_replay_finish(const cmbpo_replay_t *rp, void *stream) {
  if (int rc = check_finish("cmbpo_replay_finish", rp)) return rc;
  return launch_finish(rp, (hipStream_t)stream);
}

extern "C" int cmbpo_replay_run(const cmbpo_replay_t *rp, cmbpo_mlp_t *model, int task, int ensemble, const int32_t *d_elite,
                                void *stream) {
  const char *who = "cmbpo_replay_run";
  if (int rc = check_compare(who, rp)) return rc;
  if (int rc = check_finish(who, rp)) return rc;
  CMBPO_REQUIRE(model != nullptr, "%s: model handle is NULL", who);
  CMBPO_REQUIRE(d_elite != nullptr, "%s: NULL buffer (d_elite)", who);
  CMBPO_REQUIRE((rp->act_dim == 0 || rp->act) && rp->mean && rp->var, "%s: NULL buffer (act / mean / var)", who);
  const int B = rp->B, D = rp->obs_dim, A = rp->act_dim;
  // the two callees' own argument checks, on a call of no rows (neither launches anything for it)
  if (int rc = cmbpo_ens_forward(model, rp->cur_obs, D, rp->act, A, nullptr, nullptr, 0, B, rp->mean, rp->var, stream))
    return refused_by(who, rc);
  if (int rc = cmbpo_fakeenv_post(task, ensemble, D, A, rp->mean, rp->var, B, rp->cur_obs, rp->act, d_elite, nullptr, nullptr, 0,
                                  rp->p_next_obs, rp->p_rew, rp->p_term, rp->p_cost, rp->p_dkl_path, rp->p_ep_var_mean, nullptr,
                                  stream))
    return refused_by(who, rc);
  for (int h = 0; h < rp->H; ++h) {
    const float *act_h = rp->act ? rp->act + (size_t)h * B * A : nullptr;
    if (int rc = cmbpo_ens_forward(model, rp->cur_obs, D, act_h, A, nullptr, nullptr, B, B, rp->mean, rp->var, stream))
      return refused_by(who, rc);
    if (int rc = cmbpo_fakeenv_post(task, ensemble, D, A, rp->mean, rp->var, B, rp->cur_obs, act_h, d_elite + (size_t)h * B, nullptr,
                                    nullptr, B, rp->p_next_obs, rp->p_rew, rp->p_term, rp->p_cost, rp->p_dkl_path,
                                    rp->p_ep_var_mean, nullptr, stream))
      return refused_by(who, rc);
    if (int rc = launch_compare(rp, h, (hipStream_t)stream)) return rc;
  }
  return launch_finish(rp, (hipStream_t)stream);
}
