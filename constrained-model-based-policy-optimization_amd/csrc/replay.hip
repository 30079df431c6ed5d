// Open-loop model validation: k-step replay of real trajectories.
//
// A replay takes B windows of up to H consecutive real steps, starts the model at each window's first real observation and
// applies the recorded actions; at every horizon h it holds the model's prediction against what was recorded.  The stepping is
// the existing cmbpo_ens_forward + cmbpo_fakeenv_post (the unpenalised means, no noise); what is new is the comparison:
//   replay_compare_kernel   one horizon step: per-row verdicts, squared errors, 2x2 counts, the row's next state
// and, for a replay that also checks the model's variance, between post and compare of a step:
//   replay_calibrate_kernel one horizon step of the calibration table: squared errors against two predictive variances
// and, for a replay that also checks whether a logistic column is a probability, at the same place:
//   replay_reliab_kernel    one horizon step of the reliability table: the members' logits, binned, against the recorded flag
// and, for a replay whose post step runs the static rules' votes, at the same place:
//   replay_votes_kernel     one horizon step of the vote table: the two vote counts of a row against the recorded flags
// and, for a replay of S sampled particles per window (the post step with xi, a descriptor of its own), in place of
// the compare kernel:
//   replay_particles_kernel one horizon step: the recorded next state against a window's S particles -- ranks, absolute
//                           errors, pair differences, moments -- and the rows' next state
// Every step kernel writes its workgroup's slot of the table's partials, and one kernel serves all five tables:
//   replay_fold_kernel      per-workgroup partials -> the [H] table, in slot order
// Sums are float64, counts int64, every addition in a fixed order (no floating-point atomics): two runs are bitwise equal.
#include "common.h"
#include "ens_mlp_internal.h"
#include "fakeenv_post_internal.h"

namespace {

constexpr int kRows = 64;       // rows of one workgroup = lanes of one wave: wave 0 owns the per-row scalars, one lane per row
constexpr int kThreads = 256;
constexpr int kScalarSums = CMBPO_REPLAY_SCALAR_SUMS;  // se_rew, se_cost, sum ep_var_mean, sum dkl_path -- behind the obs_dim column sums
constexpr int kCounts = CMBPO_REPLAY_COUNTS;           // n, n_nonfinite, cost_cm[2][2], term_cm[2][2]

__device__ __forceinline__ int64_t lanes_set(bool p) { return (int64_t)__popcll(__ballot(p)); }

// The entries of one slot (= of one horizon of the table) per table, float64 sums and int64 counts: the step kernels, the fold's
// launches and replay.py (*_sizes) say the same.  The plain table's counts are kCounts, the vote table has kVoteCounts and no sums.
__host__ __device__ inline int cmp_sums(int obs_dim) { return obs_dim + kScalarSums; }
__host__ __device__ inline int cal_sums(int obs_dim) { return CMBPO_REPLAY_CALIB_SUMS * (obs_dim + 1); }
__host__ __device__ inline int cal_counts(int obs_dim) { return CMBPO_REPLAY_CALIB_COUNTS * (obs_dim + 1) + 2; }
__host__ __device__ inline int rel_sums(int n_bins, int n_cols) { return 2 * n_cols * (2 * n_bins + 2); }
__host__ __device__ inline int rel_counts(int n_bins, int n_cols) { return 2 * n_cols * 2 * n_bins + 2 * n_cols; }
__host__ __device__ inline int part_sums(int obs_dim) { return 4 * (obs_dim + 1) + 2; }
__host__ __device__ inline int part_counts(int obs_dim, int S) { return (obs_dim + 1) * (S + 1) + 2; }

// this workgroup's slot of horizon h in partials of n entries per slot, [H][gridDim.x][n]
template <typename T>
__device__ __forceinline__ T *slot(T *part, int h, int n) { return part + ((size_t)h * gridDim.x + blockIdx.x) * n; }

// The row verdict every table shares: a non-finite value in the [rows, obs_dim] tile `pred` of p_next_obs marks its row, if the
// row is alive (integer LDS atomic: order cannot matter).  The caller's s_bad holds the verdict on p_rew / p_cost already; a
// barrier on either side is the caller's.  The tables are subsets of the rows this leaves unmarked.
__device__ __forceinline__ void mark_nonfinite_rows(const float *pred, int rows, int D, const uint8_t *s_alive, int *s_bad) {
  for (int i = threadIdx.x, total = rows * D; i < total; i += kThreads) {
    const int r = i / D;
    if (s_alive[r] && !isfinite(pred[i])) atomicOr(&s_bad[r], 1);
  }
}

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
  double *psum = slot(rp.part_sum, h, cmp_sums(D));
  int64_t *pcnt = slot(rp.part_cnt, h, kCounts);

  float p_rew = 0.0f, p_cost = 0.0f;
  if (t < kRows) {
    const bool in = t < rows;
    const bool alive = in && rp.alive[row0 + t] != 0;
    if (alive) { p_rew = rp.p_rew[row0 + t]; p_cost = rp.p_cost[row0 + t]; }
    s_alive[t] = alive;
    s_bad[t] = (alive && !(isfinite(p_rew) && isfinite(p_cost))) ? 1 : 0;
  }
  __syncthreads();

  // pass 1: a non-finite predicted observation marks its row
  const float *pred = rp.p_next_obs + (size_t)row0 * D;
  mark_nonfinite_rows(pred, rows, D, s_alive, s_bad);
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

// table[h][j] = sum over the slots, in slot order, for any of the tables: one workgroup per horizon, its threads strided over the
// NS sums and NC counts of the horizon.  The loop over the slots is sequential on purpose: that order IS the table's bits.
// NS == 0 (the vote table): part_sum and sums are not touched and may be NULL.
__global__ __launch_bounds__(kThreads) void replay_fold_kernel(const double *part_sum, const int64_t *part_cnt, double *sums,
                                                               int64_t *counts, int NS, int NC, int n_part) {
  const int h = blockIdx.x;
  for (int j = threadIdx.x; j < NS + NC; j += kThreads) {
    if (j < NS) {
      const double *p = part_sum + (size_t)h * n_part * NS + j;
      double s = 0.0;
      for (int k = 0; k < n_part; ++k) s += p[(size_t)k * NS];
      sums[(size_t)h * NS + j] = s;
    } else {
      const int64_t *p = part_cnt + (size_t)h * n_part * NC + (j - NS);
      int64_t s = 0;
      for (int k = 0; k < n_part; ++k) s += p[(size_t)k * NC];
      counts[(size_t)h * NC + (j - NS)] = s;
    }
  }
}

// ---- predictive calibration ----------------------------------------------------------------------------------
constexpr int kCalSums = CMBPO_REPLAY_CALIB_SUMS;     // e^2/v_al, e_tot^2/v_tot, log v_al, log v_tot, v_bar, s2 -- per column
constexpr int kCalCounts = CMBPO_REPLAY_CALIB_COUNTS; // e^2 <= v_al, <= 4 v_al, e_tot^2 <= v_tot, <= 4 v_tot -- per column

// The members' values of one (row, column) are B * out_dim floats apart and a thread's sum over them is sequential by
// definition, so a loop of one load per member is a chain of E memory latencies.  Members e0 .. e0 + kCalBatch - 1 are loaded
// together instead (behind the last member: that member again, the caller masks it), the arithmetic follows in member order.
constexpr int kCalBatch = 8;
constexpr int kCalRows = 4;
__device__ __forceinline__ void load_members(const float *p, size_t member, int e0, int E, float (&out)[kCalBatch]) {
#pragma unroll
  for (int j = 0; j < kCalBatch; ++j) out[j] = p[(size_t)min(e0 + j, E - 1) * member];
}

// One horizon step of the calibration table; the geometry of replay_compare_kernel (kRows rows per workgroup, slot =
// workgroup).  The [rows, out_dim] tile of one member's mean / var is one contiguous run, walked flat like the predictions
// there: thread t sits on column t % W of row t / W and advances by kThreads / W rows, so a thread stays on one column and
// keeps that column's six sums and four counts in registers; columns >= C = obs_dim + 1 (a learned cost) have no work.
// Pass 1 settles the rows' verdicts (integer LDS flags: order cannot matter), pass 2 reads everything again (L1 / L2) and
// sums.  Reads alive / predictions / recording / mean / var, writes its partial slot only.
__global__ __launch_bounds__(kThreads) void replay_calibrate_kernel(cmbpo_replay_t rp, cmbpo_replay_calib_t rc, int h) {
  __shared__ uint8_t s_alive[kRows];              // alive on entry
  __shared__ int s_bad[kRows];                    // a non-finite prediction in the row
  __shared__ int s_rej[kRows];                    // a mean / variance this table cannot use, or no such member
  __shared__ int s_elite[kRows];
  __shared__ uint8_t s_in[kRows];                 // the row enters the table
  __shared__ double s_sum[kCalSums][kThreads];    // per-thread column sums, folded by the first W threads
  __shared__ int s_cnt[kCalCounts][kThreads];

  const int t = threadIdx.x;
  const int B = rp.B, D = rp.obs_dim, E = rc.ensemble, O = rc.out_dim;
  const int C = D + 1;
  const int row0 = blockIdx.x * kRows;
  const int rows = min(kRows, B - row0);
  const size_t hb = (size_t)h * B;
  // (cal_sums(D) and cal_counts(D), spelled on C: through the calls the compiler folds the + 1 another way and this kernel's
  // register allocation moves)
  double *psum = slot(rc.part_sum, h, kCalSums * C);
  int64_t *pcnt = slot(rc.part_cnt, h, kCalCounts * C + 2);

  if (t < kRows) {
    const bool alive = t < rows && rp.alive[row0 + t] != 0;
    bool bad = false, rej = false;
    int m = 0;
    if (alive) {
      bad = !(isfinite(rp.p_rew[row0 + t]) && isfinite(rp.p_cost[row0 + t]));
      m = rc.elite[hb + row0 + t];
      rej = m < 0 || m >= E;
      if (rej) m = 0;
    }
    s_alive[t] = alive;
    s_bad[t] = bad;
    s_rej[t] = rej;
    s_elite[t] = m;
  }
  __syncthreads();

  // pass 1a: the shared row verdict on the predicted observations
  const float *pred = rp.p_next_obs + (size_t)row0 * D;
  mark_nonfinite_rows(pred, rows, D, s_alive, s_bad);
  __syncthreads();

  // pass 1b: every member's mean and variance of the calibrated columns
  const int W = min(O, kThreads);          // columns of one sweep
  const int rpp = kThreads / W;            // rows of one sweep
  const int r0 = t / W;
  const size_t member = (size_t)B * O;     // elements of one member's [B, out_dim]
  const float *mean0 = rp.mean + (size_t)row0 * O, *var0 = rp.var + (size_t)row0 * O;
  for (int c0 = 0; c0 < C; c0 += W) {      // (one trip unless out_dim > kThreads)
    const int c = c0 + t % W;
    if (r0 < rpp && c < C) {
      // kCalRows of the thread's rows at a time (behind the last row: that row again, not marked), so that
      // 2 * kCalBatch * kCalRows loads are in flight: what this pass costs is memory round trips, not bytes
      for (int rb = r0; rb < rows; rb += kCalRows * rpp) {
        for (int e0 = 0; e0 < E; e0 += kCalBatch) {
          float mu[kCalRows][kCalBatch], v[kCalRows][kCalBatch];
#pragma unroll
          for (int k = 0; k < kCalRows; ++k) {
            const size_t i = (size_t)min(rb + k * rpp, rows - 1) * O + c;
            load_members(mean0 + i, member, e0, E, mu[k]);
            load_members(var0 + i, member, e0, E, v[k]);
          }
#pragma unroll
          for (int k = 0; k < kCalRows; ++k) {
            const int r = rb + k * rpp;
            bool good = true;
#pragma unroll
            for (int j = 0; j < kCalBatch; ++j) good = good && isfinite(mu[k][j]) && isfinite(v[k][j]) && v[k][j] > 0.0f;
            if (r < rows && !good && s_alive[r] && !s_bad[r]) atomicOr(&s_rej[r], 1);
          }
        }
      }
    }
  }
  __syncthreads();

  if (t < kRows) {
    const bool cand = s_alive[t] != 0 && s_bad[t] == 0;      // the rows the compare kernel sums
    const bool in = cand && s_rej[t] == 0;
    s_in[t] = in;
    const int64_t n_cal = lanes_set(in), n_skip = lanes_set(cand && !in);
    if (t == 0) { pcnt[kCalCounts * C] = n_cal; pcnt[kCalCounts * C + 1] = n_skip; }
  }
  __syncthreads();

  // pass 2: the sums
  const float *real = rp.next_obs + (hb + row0) * D;
  const double n_mem = (double)E;
  for (int c0 = 0; c0 < C; c0 += W) {
    const int c = c0 + t % W;
    double a_zal = 0.0, a_ztot = 0.0, a_lal = 0.0, a_ltot = 0.0, a_vbar = 0.0, a_s2 = 0.0;
    int n1_al = 0, n2_al = 0, n1_tot = 0, n2_tot = 0;
    if (r0 < rpp && c < C) {
      for (int r = r0; r < rows; r += rpp) {
        if (!s_in[r]) continue;
        const int m = s_elite[r];
        const size_t i = (size_t)r * O + c;
        const float ef = c < D ? __fsub_rn(pred[(size_t)r * D + c], real[(size_t)r * D + c])
                               : __fsub_rn(rp.p_rew[row0 + r], rp.rew[hb + row0 + r]);
        const double err = (double)ef;
        // the first kCalBatch members stay in registers for the second loop and the elite's pick (E <= kCalBatch: one
        // round trip per row); members behind them are read again (L1 / L2)
        float mu0[kCalBatch], v0[kCalBatch];
        load_members(mean0 + i, member, 0, E, mu0);
        load_members(var0 + i, member, 0, E, v0);
        float mu_mf = 0.0f, v_mf = 0.0f;
        if (m >= kCalBatch) { mu_mf = mean0[m * member + i]; v_mf = var0[m * member + i]; }
        double s_mu = 0.0, s_v = 0.0;
#pragma unroll
        for (int j = 0; j < kCalBatch; ++j) {
          if (j < E) { s_mu += (double)mu0[j]; s_v += (double)v0[j]; }
          if (j == m) { mu_mf = mu0[j]; v_mf = v0[j]; }
        }
        for (int e0 = kCalBatch; e0 < E; e0 += kCalBatch) {
          float mu[kCalBatch], v[kCalBatch];
          load_members(mean0 + i, member, e0, E, mu);
          load_members(var0 + i, member, e0, E, v);
#pragma unroll
          for (int j = 0; j < kCalBatch; ++j)
            if (e0 + j < E) { s_mu += (double)mu[j]; s_v += (double)v[j]; }
        }
        const double mu_bar = s_mu / n_mem, v_bar = s_v / n_mem;
        double dev = 0.0;
#pragma unroll
        for (int j = 0; j < kCalBatch; ++j)
          if (j < E) { const double d = (double)mu0[j] - mu_bar; dev += d * d; }
        for (int e0 = kCalBatch; e0 < E; e0 += kCalBatch) {
          float mu[kCalBatch];
          load_members(mean0 + i, member, e0, E, mu);
#pragma unroll
          for (int j = 0; j < kCalBatch; ++j)
            if (e0 + j < E) { const double d = (double)mu[j] - mu_bar; dev += d * d; }
        }
        const double s2 = dev / n_mem;
        const double v_al = (double)v_mf;
        const double v_tot = v_bar + s2;
        const double e_tot = err + (mu_bar - (double)mu_mf);
        const double q_al = err * err, q_tot = e_tot * e_tot;
        a_zal += q_al / v_al;
        a_ztot += q_tot / v_tot;
        a_lal += log(v_al);
        a_ltot += log(v_tot);
        a_vbar += v_bar;
        a_s2 += s2;
        n1_al += q_al <= v_al;
        n2_al += q_al <= 4.0 * v_al;
        n1_tot += q_tot <= v_tot;
        n2_tot += q_tot <= 4.0 * v_tot;
      }
    }
    s_sum[0][t] = a_zal; s_sum[1][t] = a_ztot; s_sum[2][t] = a_lal; s_sum[3][t] = a_ltot; s_sum[4][t] = a_vbar; s_sum[5][t] = a_s2;
    s_cnt[0][t] = n1_al; s_cnt[1][t] = n2_al; s_cnt[2][t] = n1_tot; s_cnt[3][t] = n2_tot;
    __syncthreads();
    if (t < W && c0 + t < C) {             // the rpp accumulators of a column, in a fixed order
#pragma unroll
      for (int k = 0; k < kCalSums; ++k) {
        double s = s_sum[k][t];
        for (int j = 1; j < rpp; ++j) s += s_sum[k][j * W + t];
        psum[k * C + c0 + t] = s;
      }
#pragma unroll
      for (int k = 0; k < kCalCounts; ++k) {
        int64_t s = s_cnt[k][t];
        for (int j = 1; j < rpp; ++j) s += s_cnt[k][j * W + t];
        pcnt[k * C + c0 + t] = s;
      }
    }
    __syncthreads();
  }
}

// ---- reliability tables of the logistic columns -------------------------------------------------------------
constexpr int kRelBins = CMBPO_RELIAB_MAX_BINS;
constexpr int kRelCols = CMBPO_RELIAB_MAX_COLS;
static_assert(CMBPO_RELIAB_MAX_ENSEMBLE <= kCalBatch, "one batch of loads holds every member's logit");
static_assert(2 * kRelCols * kRows == kThreads, "one thread per (column, reading, row)");
static_assert(2 * kRelCols * kRelBins <= kThreads / 2, "the bin owners sit below the owners of the per-reading and per-column entries");

// One horizon step of the reliability table; the geometry of replay_compare_kernel (kRows rows per workgroup, slot =
// workgroup).  Thread t sits on row t % kRows of (column, reading) pair t / kRows, j = pair / 2 and r = pair % 2: it loads every
// member's logit of its row and column in one batch (they are B * out_dim floats apart; the two readings of a row load the
// same 2 E floats, the second from L1), settles the row's verdict, computes its own reading's z, bin and terms and leaves them in
// LDS.  Then thread u < 2 C K owns bin u % K of pair u / K and adds its rows in row order, threads kThreads / 2 + pair own the
// two sums of a reading, threads 3 kThreads / 4 + j the two counts of a column: every entry of the slot has one writer, the
// order is fixed.  Reads alive / predictions / recording / mean, writes its partial slot only.
__global__ __launch_bounds__(kThreads) void replay_reliab_kernel(cmbpo_replay_t rp, cmbpo_replay_reliab_t rr, int h) {
  __shared__ uint8_t s_alive[kRows];    // alive on entry
  __shared__ int s_bad[kRows];          // a non-finite prediction in the row
  __shared__ double s_edge[kRelBins];
  __shared__ int s_bin[kThreads];       // the bin of (pair, row); -1: the row does not enter
  __shared__ uint8_t s_y[kThreads], s_skip[kThreads];
  __shared__ double s_p[kThreads], s_z[kThreads], s_br[kThreads], s_ll[kThreads];

  const int t = threadIdx.x;
  const int B = rp.B, D = rp.obs_dim, E = rr.ensemble, O = rr.out_dim, K = rr.n_bins, nc = rr.n_cols;
  const int row0 = blockIdx.x * kRows;
  const int rows = min(kRows, B - row0);
  const size_t hb = (size_t)h * B;
  double *psum = slot(rr.part_sum, h, rel_sums(K, nc));
  int64_t *pcnt = slot(rr.part_cnt, h, rel_counts(K, nc));

  if (t < kRows) {
    const bool alive = t < rows && rp.alive[row0 + t] != 0;
    s_alive[t] = alive;
    s_bad[t] = (alive && !(isfinite(rp.p_rew[row0 + t]) && isfinite(rp.p_cost[row0 + t]))) ? 1 : 0;
  } else if (t - kRows < K - 1) {
    s_edge[t - kRows] = (double)rr.edges[t - kRows];
  }
  __syncthreads();

  // the members' logits of (row, column): issued ahead of the scan of the predictions, used behind it
  const int row = t % kRows, pair = t / kRows, j = pair >> 1, rd = pair & 1;
  const bool mine = j < nc && s_alive[row] != 0;
  const int col = j ? rr.col[1] : rr.col[0];                     // (selects, not indexed: the descriptor stays in scalars)
  const int target = j ? rr.target[1] : rr.target[0];
  const float shift = j ? rr.shift[1] : rr.shift[0];
  float zm[kCalBatch];
#pragma unroll
  for (int e = 0; e < kCalBatch; ++e) zm[e] = 0.0f;
  int m = -1;
  if (mine) {
    load_members(rp.mean + (size_t)(row0 + row) * O + col, (size_t)B * O, 0, E, zm);
    m = rr.elite[hb + row0 + row];
  }

  // the shared row verdict on the predicted observations
  mark_nonfinite_rows(rp.p_next_obs + (size_t)row0 * D, rows, D, s_alive, s_bad);
  __syncthreads();

  int bin = -1;
  bool skip = false, y = false;
  double z = 0.0, p = 0.0, br = 0.0, ll = 0.0;
  if (mine && s_bad[row] == 0) {
    bool ok = m >= 0 && m < E;
    double s = 0.0;
    float z_m = 0.0f;
#pragma unroll
    for (int e = 0; e < kCalBatch; ++e) {
      if (e < E) {
        const float v = shift != 0.0f ? __fsub_rn(zm[e], shift) : zm[e];
        ok = ok && isfinite(v);
        s += (double)v;
        if (e == m) z_m = v;
      }
    }
    skip = !ok;
    if (ok) {
      z = rd ? s / (double)E : (double)z_m;
      const uint8_t *flags = rr.term ? rr.term : rp.term;
      y = target == CMBPO_RELIAB_COST ? rp.cost[hb + row0 + row] > 0.5f : flags[hb + row0 + row] != 0;
      bin = 0;
      for (int k = 0; k < K - 1; ++k) bin += z > s_edge[k];
      const double yd = y ? 1.0 : 0.0;
      p = 1.0 / (1.0 + exp(-z));
      ll = fmax(z, 0.0) - yd * z + log1p(exp(-fabs(z)));
      const double q = 1.0 / (1.0 + exp(y ? z : -z));      // |p - y| without the cancellation of p - 1
      br = q * q;
    }
  }
  s_bin[t] = bin; s_y[t] = y; s_skip[t] = skip;
  s_p[t] = p; s_z[t] = z; s_br[t] = br; s_ll[t] = ll;
  __syncthreads();

  if (t < 2 * nc * K) {                                  // one bin of one (column, reading)
    const int pr = t / K, k = t % K;
    int64_t n = 0, pos = 0;
    double sp = 0.0, sz = 0.0;
    for (int r = 0; r < kRows; ++r) {
      const int i = pr * kRows + r;
      if (s_bin[i] == k) { n += 1; pos += s_y[i]; sp += s_p[i]; sz += s_z[i]; }
    }
    psum[pr * (2 * K + 2) + k] = sp;
    psum[pr * (2 * K + 2) + K + k] = sz;
    pcnt[pr * 2 * K + k] = n;
    pcnt[pr * 2 * K + K + k] = pos;
  } else if (t >= kThreads / 2 && t - kThreads / 2 < 2 * nc) {      // the two sums of one (column, reading)
    const int pr = t - kThreads / 2;
    double sb = 0.0, sl = 0.0;
    for (int r = 0; r < kRows; ++r) {
      const int i = pr * kRows + r;
      if (s_bin[i] >= 0) { sb += s_br[i]; sl += s_ll[i]; }
    }
    psum[pr * (2 * K + 2) + 2 * K] = sb;
    psum[pr * (2 * K + 2) + 2 * K + 1] = sl;
  } else if (t >= 3 * kThreads / 4 && t - 3 * kThreads / 4 < nc) {  // the two counts of one column (its reading 0 decides)
    const int c = t - 3 * kThreads / 4;
    int64_t n_rel = 0, n_skip = 0;
    for (int r = 0; r < kRows; ++r) {
      const int i = 2 * c * kRows + r;
      n_rel += s_bin[i] >= 0;
      n_skip += s_skip[i];
    }
    pcnt[2 * nc * 2 * K + 2 * c] = n_rel;
    pcnt[2 * nc * 2 * K + 2 * c + 1] = n_skip;
  }
}

// ---- the static rules' votes ---------------------------------------------------------------------------------
constexpr int kVoteCounts = CMBPO_REPLAY_VOTE_COUNTS;            // hist_cost[9][2] | hist_term[9][2] | n_vote | n_skipped
constexpr int kVoteSlots = CMBPO_REPLAY_VOTES_MAX_ENSEMBLE + 1;  // v = 0 .. 8
static_assert(kVoteCounts == 2 * kVoteSlots * 2 + 2 && kVoteCounts <= kRows, "one lane of wave 0 per entry of a slot");

// One horizon step of the vote table; the geometry of replay_compare_kernel (kRows rows per workgroup, slot = workgroup).  All
// threads scan the predicted observations for the shared row verdict, then wave 0, lane = row, reads its row's two vote
// counts and flags.  An entry of the slot is the number of lanes with one (signal, v, y): a ballot and its population count, a
// wave-uniform scalar, which lane k keeps when it is entry k's -- 36 ballots on registers in place of LDS atomics on 36
// addresses, no second barrier, and the slot leaves as one coalesced store of 38 lanes.  Reads alive / predictions / recording
// and the vote arrays, writes its partial slot only.
__global__ __launch_bounds__(kThreads) void replay_votes_kernel(cmbpo_replay_t rp, cmbpo_replay_votes_t rv, int h) {
  __shared__ uint8_t s_alive[kRows];   // alive on entry
  __shared__ int s_bad[kRows];         // a non-finite prediction in the row

  const int t = threadIdx.x;
  const int B = rp.B, D = rp.obs_dim, E = rv.ensemble;
  const int row0 = blockIdx.x * kRows;
  const int rows = min(kRows, B - row0);
  const size_t hb = (size_t)h * B;
  int64_t *pcnt = slot(rv.part_cnt, h, kVoteCounts);

  // the row's votes and flags: issued ahead of the scan of the predictions, used behind it
  bool alive = false, y_c = false, y_t = false;
  int v_c = 0, v_d = 0;
  if (t < kRows) {
    alive = t < rows && rp.alive[row0 + t] != 0;
    bool bad = false;
    if (alive) {
      bad = !(isfinite(rp.p_rew[row0 + t]) && isfinite(rp.p_cost[row0 + t]));
      v_d = rv.done_votes[row0 + t];
      if (rv.cost_votes != nullptr) {
        v_c = rv.cost_votes[row0 + t];
        y_c = rp.cost[hb + row0 + t] > 0.0f;
      }
      const uint8_t *flags = rv.term ? rv.term : rp.term;
      y_t = flags[hb + row0 + t] != 0;
    }
    s_alive[t] = alive;
    s_bad[t] = bad;
  }
  __syncthreads();

  // the shared row verdict on the predicted observations
  mark_nonfinite_rows(rp.p_next_obs + (size_t)row0 * D, rows, D, s_alive, s_bad);
  __syncthreads();

  if (t >= kRows) return;
  const bool cand = alive && s_bad[t] == 0;                      // the rows the compare kernel sums
  const bool in = cand && v_c <= E && v_d <= E;
  const bool cost_on = rv.cost_votes != nullptr;
  int64_t mine = 0;
#pragma unroll
  for (int v = 0; v < kVoteSlots; ++v) {
#pragma unroll
    for (int y = 0; y < 2; ++y) {
      const int64_t n_c = lanes_set(in && cost_on && v_c == v && y_c == (y != 0));
      const int64_t n_t = lanes_set(in && v_d == v && y_t == (y != 0));
      if (t == 2 * v + y) mine = n_c;
      if (t == 2 * kVoteSlots + 2 * v + y) mine = n_t;
    }
  }
  const int64_t n_vote = lanes_set(in), n_skip = lanes_set(cand && !in);
  if (t == kVoteCounts - 2) mine = n_vote;
  if (t == kVoteCounts - 1) mine = n_skip;
  if (t < kVoteCounts) pcnt[t] = mine;
}

// ---- particle replay: rank histograms and CRPS of sampled rollouts ------------------------------------------
constexpr int kWaves = kThreads / kRows;
// CMBPO_REPLAY_PARTICLES_MAX_OBS is a chosen constant, so that the refusal needs no HIP call; the one place that holds it
// against the LDS of a gfx950 workgroup is the static_assert below.  The launch asks cmbpo_grant_lds for the bytes of its shape.
constexpr size_t kLdsWorkgroup = 160 * 1024;

// row stride of the staged tile in floats: the C = obs_dim + 1 columns (the reward behind the observation), made odd -- in the
// column phase lane = row reads column c of its row, 64 addresses `ld` floats apart, which an odd stride spreads over all banks
__host__ __device__ inline int part_ld(int obs_dim) { return (obs_dim + 1) | 1; }
// the staged tile: kRows rows of predictions and the recording of the kRows / S windows behind them
inline size_t part_lds_bytes(int obs_dim, int S) { return (size_t)(kRows + kRows / S) * part_ld(obs_dim) * sizeof(float); }
static_assert((size_t)(kRows + kRows / 2) * ((CMBPO_REPLAY_PARTICLES_MAX_OBS + 1) | 1) * sizeof(float) + 1024 <= kLdsWorkgroup,
              "the tile of the widest observation at the smallest S, and the static arrays, fit one workgroup's LDS");

// sum over the S lanes of a window (S consecutive lanes, S a power of two): a butterfly, so every lane of the window holds the
// same bits (each level adds the same two numbers in both partners, and a + b == b + a)
__device__ __forceinline__ double group_sum(double v, int S) {
  for (int o = S >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One horizon step of the particle table.  One workgroup = kRows consecutive rows = kRows / S whole windows (slot = workgroup).
// The [rows, obs_dim] tile of p_next_obs is one contiguous run: all threads walk it once, row by column, into LDS (stride part_ld, the
// reward in column obs_dim), marking non-finite rows on the way (integer LDS flag: order cannot matter); the windows' recording
// goes in behind it.  Wave 0, lane = row, settles the windows' verdicts (a window's flags are the bits of one ballot under the
// window's lane mask), the two Brier terms and the counts.  Then every thread writes the rows' next state from the staged tile,
// and the waves take the columns in turn, lane = row: the rank is the population count of a ballot under the window's mask, the
// sums over a window's particles are butterflies over its S lanes, the S (S - 1) pair differences come from S - 1 lane
// rotations inside the window (registers only), and a column's sum over the windows is wave_sum over the windows' first lanes.
// Every entry of the slot has one writer and a fixed order.  Global memory: every input is read once.
__global__ __launch_bounds__(kThreads) void replay_particles_kernel(cmbpo_replay_particles_t rp, int h) {
  extern __shared__ float s_tile[];    // [kRows][ld] predictions | [kRows / S][ld] recording
  __shared__ uint8_t s_alive[kRows];   // alive on entry
  __shared__ int s_bad[kRows];         // a non-finite prediction in the row
  __shared__ uint8_t s_ok[kRows];      // the row's window is alive and finite: it is summed
  __shared__ uint8_t s_next[kRows];    // the row's window lives on to h + 1: cur_obs is written

  const int t = threadIdx.x, lane = t & (kRows - 1), wave = t / kRows;
  const int S = rp.S, D = rp.obs_dim, C = D + 1, ld = part_ld(D);
  const int lgS = 31 - __clz(S);
  const int R = rp.B * S;
  const int row0 = blockIdx.x * kRows;
  const int rows = min(kRows, R - row0);           // a multiple of S
  const int win0 = row0 >> lgS, wins = rows >> lgS;
  const size_t hb = (size_t)h * rp.B;
  float *s_x = s_tile, *s_q = s_tile + kRows * ld;
  double *psum = slot(rp.part_sum, h, part_sums(D));
  int64_t *pcnt = slot(rp.part_cnt, h, part_counts(D, S));
  const uint64_t gmask = (S == 64 ? ~0ull : (1ull << S) - 1) << (lane & ~(S - 1));      // the lanes of this lane's window
  const bool first = (lane & (S - 1)) == 0;                                             // the window's first lane speaks for it

  float p_rew = 0.0f, p_cost = 0.0f;
  bool p_term = false, alive = false;
  if (t < kRows) {
    alive = t < rows && rp.alive[row0 + t] != 0;
    if (alive) { p_rew = rp.p_rew[row0 + t]; p_cost = rp.p_cost[row0 + t]; p_term = rp.p_term[row0 + t] != 0; }
    s_alive[t] = alive;
    s_bad[t] = (alive && !(isfinite(p_rew) && isfinite(p_cost))) ? 1 : 0;
    s_x[t * ld + D] = p_rew;
    if (t < wins) s_q[t * ld + D] = rp.rew[hb + win0 + t];
  }
  __syncthreads();

  // the tile, once.  The walk of replay_compare_kernel: thread t sits on column t % W of row t / W and advances by kThreads / W
  // rows -- consecutive threads read consecutive floats, and the one division is per thread, not per element (obs_dim >
  // kThreads: a second trip over the columns)
  const int W = min(D, kThreads), rpp = kThreads / W;
  const int tr = t / W, tc = t - tr * W;
  const bool walker = tr < rpp;
  const float *pred = rp.p_next_obs + (size_t)row0 * D;
  const float *real = rp.next_obs + (hb + win0) * D;
  if (walker) {
    for (int c = tc; c < D; c += W) {
      for (int r = tr; r < rows; r += rpp) {
        const float v = pred[r * D + c];
        s_x[r * ld + c] = v;
        if (s_alive[r] && !isfinite(v)) atomicOr(&s_bad[r], 1);
      }
      for (int w = tr; w < wins; w += rpp) s_q[w * ld + c] = real[w * D + c];
    }
  }
  __syncthreads();

  // the windows' verdicts, Brier terms and counts: wave 0, lane = row
  if (t < kRows) {
    const bool wbad = (__ballot(s_bad[t] != 0) & gmask) != 0;
    const bool ok = alive && !wbad, bad = alive && wbad;
    const int n_term = __popcll(__ballot(ok && p_term) & gmask);
    const double m_cost = group_sum(ok ? (double)p_cost : 0.0, S) / (double)S;
    double b_term = 0.0, b_cost = 0.0;
    bool next = false;
    if (ok) {
      const int w = win0 + (t >> lgS);
      const bool y_t = rp.term[hb + w] != 0, y_c = rp.cost[hb + w] > 0.0f;
      const double dt = (double)n_term / (double)S - (y_t ? 1.0 : 0.0), dc = m_cost - (y_c ? 1.0 : 0.0);
      b_term = dt * dt;
      b_cost = dc * dc;
      next = h + 1 < rp.len[w] && !y_t;
    }
    s_ok[t] = ok;
    s_next[t] = next;
    if (alive && !next) rp.alive[row0 + t] = 0;
    b_term = wave_sum(first ? b_term : 0.0);
    b_cost = wave_sum(first ? b_cost : 0.0);
    const int64_t n = lanes_set(ok && first), n_bad = lanes_set(bad && first);
    if (t == 0) { psum[4 * C] = b_term; psum[4 * C + 1] = b_cost; pcnt[C * (S + 1)] = n; pcnt[C * (S + 1) + 1] = n_bad; }
  }
  __syncthreads();

  // the rows' next state, from the staged tile: the same walk
  float *cur = rp.cur_obs + (size_t)row0 * D;
  const bool open = rp.mode == CMBPO_REPLAY_OPEN_LOOP;
  if (walker) {
    for (int c = tc; c < D; c += W)
      for (int r = tr; r < rows; r += rpp)
        if (s_next[r]) cur[r * D + c] = open ? s_x[r * ld + c] : s_q[(r >> lgS) * ld + c];
  }

  // the columns: wave `wave` takes c = wave, wave + kWaves, ..., lane = row
  const bool ok = s_ok[lane] != 0, keep = ok && first;
  const int gl = lane & ~(S - 1);
  const double dS = (double)S;
  for (int c = wave; c < C; c += kWaves) {
    const float x = ok ? s_x[lane * ld + c] : 0.0f, q = ok ? s_q[(lane >> lgS) * ld + c] : 0.0f;
    const int k = __popcll(__ballot(ok && x < q) & gmask);
    double pr = 0.0;
    for (int j = 1; j < S; ++j) {
      const float xo = __shfl(x, gl + ((lane + j) & (S - 1)), 64);
      pr += (double)fabsf(__fsub_rn(x, xo));
    }
    const double a = group_sum((double)fabsf(__fsub_rn(x, q)), S) / dS;
    const double g = group_sum(pr, S) / (dS * (dS - 1.0));           // every pair from both ends: 2 sum_{p < p'}
    const double m = group_sum((double)x, S) / dS;
    const double dq = m - (double)q, dx = (double)x - m;
    const double v = group_sum(dx * dx, S) / (dS - 1.0);
    const double s_a = wave_sum(keep ? a : 0.0), s_g = wave_sum(keep ? g : 0.0);
    const double s_e = wave_sum(keep ? dq * dq : 0.0), s_v = wave_sum(keep ? v : 0.0);
    if (lane == 0) { psum[c] = s_a; psum[C + c] = s_g; psum[2 * C + c] = s_e; psum[3 * C + c] = s_v; }
    // rank_hist[c][kk]: the windows with k == kk, a ballot each; lane kk keeps entry kk (lane 0 also entry 64 at S = 64)
    int64_t mine = 0, last = 0;
    for (int kk = 0; kk <= S; ++kk) {
      const int64_t n = lanes_set(keep && k == kk);
      if (kk < kRows) { if (lane == kk) mine = n; } else last = n;
    }
    int64_t *hist = pcnt + (size_t)c * (S + 1);
    if (lane <= S && lane < kRows) hist[lane] = mine;
    if (S == kRows && lane == 0) hist[kRows] = last;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// every launch of this file: kThreads threads; a step kernel takes one workgroup per slot, the fold one per horizon
template <typename... P, typename... A>
int launch(void (*kern)(P...), int grid, size_t lds, hipStream_t s, A... args) {
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), lds, s, args...);
  CMBPO_HIP_CHECK(hipGetLastError());
  return CMBPO_OK;
}

int launch_fold(const double *part_sum, const int64_t *part_cnt, double *sums, int64_t *counts, int NS, int NC, int H, int n_part,
                hipStream_t s) {
  return launch(replay_fold_kernel, H, 0, s, part_sum, part_cnt, sums, counts, NS, NC, n_part);
}

int check_h(const char *who, int h, int H) {
  CMBPO_REQUIRE(h >= 0 && h < H, "%s: h %d outside [0, %d)", who, h, H);
  return CMBPO_OK;
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
  return launch(replay_compare_kernel, cmbpo_replay_parts(rp->B), 0, s, *rp, h);
}

int launch_finish(const cmbpo_replay_t *rp, hipStream_t s) {
  return launch_fold(rp->part_sum, rp->part_cnt, rp->sums, rp->counts, cmp_sums(rp->obs_dim), kCounts, rp->H, cmbpo_replay_parts(rp->B), s);
}

int check_calib(const char *who, const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *rc) {
  CMBPO_REQUIRE(rc != nullptr, "%s: calibration descriptor is NULL", who);
  CMBPO_REQUIRE(rc->ensemble >= 1, "%s: ensemble %d < 1", who, rc->ensemble);
  CMBPO_REQUIRE(rc->out_dim >= rp->obs_dim + 1, "%s: out_dim %d < obs_dim + 1 = %d", who, rc->out_dim, rp->obs_dim + 1);
  CMBPO_REQUIRE(rc->reserved == 0, "%s: calibration reserved %d != 0", who, rc->reserved);
  return CMBPO_OK;
}

int check_calibrate(const char *who, const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *rc) {
  if (int r = check_compare(who, rp)) return r;
  if (int r = check_calib(who, rp, rc)) return r;
  CMBPO_REQUIRE(rp->mean && rp->var, "%s: NULL buffer (mean / var)", who);
  CMBPO_REQUIRE(rc->elite, "%s: NULL buffer (elite)", who);
  CMBPO_REQUIRE(rc->part_sum && rc->part_cnt, "%s: NULL buffer (calibration partials)", who);
  return CMBPO_OK;
}

int check_calib_finish(const char *who, const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *rc) {
  if (int r = check_shape(who, rp)) return r;
  if (int r = check_calib(who, rp, rc)) return r;
  CMBPO_REQUIRE(rc->part_sum && rc->part_cnt, "%s: NULL buffer (calibration partials)", who);
  CMBPO_REQUIRE(rc->sums && rc->counts, "%s: NULL buffer (calibration table)", who);
  return CMBPO_OK;
}

int launch_calibrate(const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *rc, int h, hipStream_t s) {
  return launch(replay_calibrate_kernel, cmbpo_replay_parts(rp->B), 0, s, *rp, *rc, h);
}

int launch_calib_finish(const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *rc, hipStream_t s) {
  return launch_fold(rc->part_sum, rc->part_cnt, rc->sums, rc->counts, cal_sums(rp->obs_dim), cal_counts(rp->obs_dim), rp->H,
                     cmbpo_replay_parts(rp->B), s);
}

int check_reliab(const char *who, const cmbpo_replay_reliab_t *rr) {
  CMBPO_REQUIRE(rr != nullptr, "%s: reliability descriptor is NULL", who);
  CMBPO_REQUIRE(rr->ensemble >= 1 && rr->ensemble <= CMBPO_RELIAB_MAX_ENSEMBLE, "%s: reliability ensemble %d outside [1, %d]", who,
                rr->ensemble, CMBPO_RELIAB_MAX_ENSEMBLE);
  CMBPO_REQUIRE(rr->n_bins >= 1 && rr->n_bins <= kRelBins, "%s: n_bins %d outside [1, %d]", who, rr->n_bins, kRelBins);
  CMBPO_REQUIRE(rr->n_cols >= 1 && rr->n_cols <= kRelCols, "%s: n_cols %d outside [1, %d]", who, rr->n_cols, kRelCols);
  CMBPO_REQUIRE(rr->reserved == 0, "%s: reliability reserved %d != 0", who, rr->reserved);
  for (int j = 0; j < rr->n_cols; ++j) {
    CMBPO_REQUIRE(rr->col[j] >= 0 && rr->col[j] < rr->out_dim, "%s: col[%d] %d outside [0, out_dim = %d)", who, j, rr->col[j],
                  rr->out_dim);
    CMBPO_REQUIRE(rr->target[j] == CMBPO_RELIAB_COST || rr->target[j] == CMBPO_RELIAB_TERM, "%s: unknown target[%d] %d", who, j,
                  rr->target[j]);
    CMBPO_REQUIRE(std::isfinite(rr->shift[j]), "%s: shift[%d] is not finite", who, j);
  }
  return CMBPO_OK;
}

int check_reliab_step(const char *who, const cmbpo_replay_t *rp, const cmbpo_replay_reliab_t *rr) {
  if (int r = check_compare(who, rp)) return r;
  if (int r = check_reliab(who, rr)) return r;
  CMBPO_REQUIRE(rp->mean, "%s: NULL buffer (mean)", who);
  CMBPO_REQUIRE(rr->elite, "%s: NULL buffer (reliability elite)", who);
  CMBPO_REQUIRE(rr->n_bins == 1 || rr->edges, "%s: NULL buffer (edges)", who);
  CMBPO_REQUIRE(rr->part_sum && rr->part_cnt, "%s: NULL buffer (reliability partials)", who);
  return CMBPO_OK;
}

int check_reliab_finish(const char *who, const cmbpo_replay_t *rp, const cmbpo_replay_reliab_t *rr) {
  if (int r = check_shape(who, rp)) return r;
  if (int r = check_reliab(who, rr)) return r;
  CMBPO_REQUIRE(rr->part_sum && rr->part_cnt, "%s: NULL buffer (reliability partials)", who);
  CMBPO_REQUIRE(rr->sums && rr->counts, "%s: NULL buffer (reliability table)", who);
  return CMBPO_OK;
}

int launch_reliab(const cmbpo_replay_t *rp, const cmbpo_replay_reliab_t *rr, int h, hipStream_t s) {
  return launch(replay_reliab_kernel, cmbpo_replay_parts(rp->B), 0, s, *rp, *rr, h);
}

int launch_reliab_finish(const cmbpo_replay_t *rp, const cmbpo_replay_reliab_t *rr, hipStream_t s) {
  return launch_fold(rr->part_sum, rr->part_cnt, rr->sums, rr->counts, rel_sums(rr->n_bins, rr->n_cols),
                     rel_counts(rr->n_bins, rr->n_cols), rp->H, cmbpo_replay_parts(rp->B), s);
}

// `modes`: the single-step entries check ensemble <= 8 and the two modes' ranges themselves; the run entry leaves them to the
// post step, whose refusal it passes on
int check_votes(const char *who, const cmbpo_replay_votes_t *rv, bool modes) {
  CMBPO_REQUIRE(rv != nullptr, "%s: vote descriptor is NULL", who);
  CMBPO_REQUIRE(rv->ensemble >= 1, "%s: vote ensemble %d < 1", who, rv->ensemble);
  CMBPO_REQUIRE(rv->reserved == 0, "%s: vote reserved %d != 0", who, rv->reserved);
  if (!modes) return CMBPO_OK;
  CMBPO_REQUIRE(rv->ensemble <= CMBPO_REPLAY_VOTES_MAX_ENSEMBLE, "%s: vote ensemble %d outside [1, %d]", who, rv->ensemble,
                CMBPO_REPLAY_VOTES_MAX_ENSEMBLE);
  const cmbpo_rule_votes_t post{rv->done_members, rv->cost_members, rv->done_votes, rv->cost_votes};
  return cmbpo_internal_rule_votes_check_struct(who, &post);
}

int check_votes_step(const char *who, const cmbpo_replay_t *rp, const cmbpo_replay_votes_t *rv, bool modes) {
  if (int r = check_compare(who, rp)) return r;
  if (int r = check_votes(who, rv, modes)) return r;
  CMBPO_REQUIRE(rv->done_votes, "%s: NULL buffer (done_votes)", who);
  CMBPO_REQUIRE(rv->part_cnt, "%s: NULL buffer (vote partials)", who);
  return CMBPO_OK;
}

int check_votes_finish(const char *who, const cmbpo_replay_t *rp, const cmbpo_replay_votes_t *rv, bool modes) {
  if (int r = check_shape(who, rp)) return r;
  if (int r = check_votes(who, rv, modes)) return r;
  CMBPO_REQUIRE(rv->part_cnt, "%s: NULL buffer (vote partials)", who);
  CMBPO_REQUIRE(rv->counts, "%s: NULL buffer (vote table)", who);
  return CMBPO_OK;
}

int launch_votes(const cmbpo_replay_t *rp, const cmbpo_replay_votes_t *rv, int h, hipStream_t s) {
  return launch(replay_votes_kernel, cmbpo_replay_parts(rp->B), 0, s, *rp, *rv, h);
}

int launch_votes_finish(const cmbpo_replay_t *rp, const cmbpo_replay_votes_t *rv, hipStream_t s) {
  return launch_fold(nullptr, rv->part_cnt, nullptr, rv->counts, 0, kVoteCounts, rp->H, cmbpo_replay_parts(rp->B), s);
}

// a callee's refusal, passed on under this entry point's name
int refused_by(const char *who, int rc) {
  char inner[400];
  snprintf(inner, sizeof(inner), "%s", cmbpo_last_error());
  cmbpo_set_error("%s: %s", who, inner);
  return rc;
}

// the heads of a run against the model's width
int check_heads(const char *who, int obs_dim, const cmbpo_mlp_t *model, int task, const cmbpo_term_head_t *th, const cmbpo_cost_head_t *ch) {
  if (ch && ch->kind == 1)
    CMBPO_REQUIRE(model->out_dim == obs_dim + 2 + (th ? 1 : 0),
                  "%s: logistic cost head (cmbpo_cost_head_t, kind 1): model out_dim %d does not match obs_dim %d + 2 (+ 1 with a "
                  "termination head), task 0x%x", who, model->out_dim, obs_dim, task);
  if (th) {
    const int want = obs_dim + 1 + ((task & CMBPO_TASK_LEARNED_COST) ? 1 : 0) + 1;
    CMBPO_REQUIRE(model->out_dim == want,
                  "%s: termination head (cmbpo_term_head_t): model out_dim %d does not match obs_dim %d + 1 (+ 1 with CMBPO_TASK_LEARNED_COST) "
                  "+ 1 for the head's column, task 0x%x", who, model->out_dim, obs_dim, task);
  }
  return CMBPO_OK;
}

// The stepping of a run, for either descriptor (RP: cmbpo_replay_t or cmbpo_replay_particles_t; R rows a horizon, B or B S).
// post_call: the post step of a replay; act, elite, xi and n_rows follow the horizon (step_model), rv is the vote run's.
template <typename RP>
FakeenvPostCall post_call(const RP *rp, int R, int task, int ensemble, const cmbpo_term_head_t *th, const cmbpo_cost_head_t *ch) {
  FakeenvPostCall pc{};
  pc.task = task; pc.ensemble = ensemble; pc.obs_dim = rp->obs_dim; pc.act_dim = rp->act_dim;
  pc.mean = rp->mean; pc.var = rp->var; pc.ld_rows = R; pc.obs = rp->cur_obs;
  pc.next_obs = rp->p_next_obs; pc.rew = rp->p_rew; pc.term = rp->p_term; pc.cost = rp->p_cost;
  pc.dkl_path = rp->p_dkl_path; pc.ep_var_mean = rp->p_ep_var_mean;
  pc.th = th;
  pc.ch = ch;
  return pc;
}

// h >= 0: the forward and the post step of horizon h.  h < 0: the two callees' own argument checks, on a call of no rows (neither
// launches anything for it).  xi: the particle run's noise [H][R][obs_dim], NULL for the plain run.
template <typename RP>
int step_model(const char *who, const RP *rp, FakeenvPostCall &pc, int h, cmbpo_mlp_t *model, const int32_t *d_elite, const float *xi,
               void *stream) {
  const int R = pc.ld_rows, D = rp->obs_dim, A = rp->act_dim;
  const size_t at = h < 0 ? 0 : (size_t)h * R;
  const float *act_h = rp->act ? rp->act + at * A : nullptr;
  if (int rc = cmbpo_ens_forward(model, rp->cur_obs, D, act_h, A, nullptr, nullptr, h < 0 ? 0 : R, R, rp->mean, rp->var, stream))
    return refused_by(who, rc);
  pc.act = act_h; pc.elite = d_elite + at; pc.xi = xi ? xi + at * D : nullptr; pc.n_rows = h < 0 ? 0 : R;
  if (int rc = cmbpo_internal_fakeenv_post(pc, stream)) return refused_by(who, rc);
  return CMBPO_OK;
}

// the steps of a run: cal == nullptr is exactly cmbpo_replay_run's launches, else the calibrate kernel goes between post and
// compare and its finish behind the plain one; rel != nullptr: the reliability kernel behind it, its finish last; th / ch !=
// nullptr: the heads' instances of the post kernel; vot != nullptr: the vote kernel behind the post kernel (FakeenvPostCall::rv), the
// vote table's kernel behind the reliability kernel, its finish last.  Every argument has been checked by the caller.
int run_steps(const char *who, const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *cal, const cmbpo_replay_reliab_t *rel,
              const cmbpo_replay_votes_t *vot, cmbpo_mlp_t *model, int task, int ensemble, const int32_t *d_elite,
              const cmbpo_term_head_t *th, const cmbpo_cost_head_t *ch, void *stream) {
  FakeenvPostCall pc = post_call(rp, rp->B, task, ensemble, th, ch);
  cmbpo_rule_votes_t post_votes{};
  if (vot) {
    post_votes.done_members = vot->done_members; post_votes.cost_members = vot->cost_members;
    post_votes.done_votes = vot->done_votes; post_votes.cost_votes = vot->cost_votes;
    pc.rv = &post_votes;
    // the votes' own refusals come first: they need nothing of the model, so they can be had without one
    pc.act = rp->act; pc.elite = d_elite; pc.n_rows = 0;
    if (int rc = cmbpo_internal_fakeenv_post(pc, stream)) return refused_by(who, rc);
  }
  if (int rc = step_model(who, rp, pc, -1, model, d_elite, nullptr, stream)) return rc;
  for (int h = 0; h < rp->H; ++h) {
    if (int rc = step_model(who, rp, pc, h, model, d_elite, nullptr, stream)) return rc;
    if (cal)
      if (int rc = launch_calibrate(rp, cal, h, (hipStream_t)stream)) return rc;
    if (rel)
      if (int rc = launch_reliab(rp, rel, h, (hipStream_t)stream)) return rc;
    if (vot)
      if (int rc = launch_votes(rp, vot, h, (hipStream_t)stream)) return rc;
    if (int rc = launch_compare(rp, h, (hipStream_t)stream)) return rc;
  }
  if (int rc = launch_finish(rp, (hipStream_t)stream)) return rc;
  if (cal)
    if (int rc = launch_calib_finish(rp, cal, (hipStream_t)stream)) return rc;
  if (rel)
    if (int rc = launch_reliab_finish(rp, rel, (hipStream_t)stream)) return rc;
  return vot ? launch_votes_finish(rp, vot, (hipStream_t)stream) : CMBPO_OK;
}

// The six run entry points: ONE check list, keyed on which of rc (calibration), rr (reliability), rv (votes), th (termination head)
// and ch (cost head) are given.  The messages carry the name of the narrowest entry point that can express the call (DESIGN): rv
// given -- cmbpo_replay_run_votes, else rr given -- cmbpo_replay_run_reliab, else ch given --
// cmbpo_replay_run_cost, else th given -- cmbpo_replay_run_term, else rc given -- cmbpo_replay_run_calibrated, else
// cmbpo_replay_run.  Where the entry points have always differed in the order
// or the wording of a check, each combination keeps its own.
int replay_run(const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *rc, const cmbpo_replay_reliab_t *rr,
               const cmbpo_replay_votes_t *rv, const cmbpo_term_head_t *th, const cmbpo_cost_head_t *ch, cmbpo_mlp_t *model,
               int task, int ensemble, const int32_t *d_elite, void *stream) {
  const bool ext = th || ch || rr || rv;      // (the entries that take d_elite beside a calibration descriptor share their checks)
  const char *who = rv ? "cmbpo_replay_run_votes" : rr ? "cmbpo_replay_run_reliab" : ch ? "cmbpo_replay_run_cost" : th ? "cmbpo_replay_run_term" : rc ? "cmbpo_replay_run_calibrated" : "cmbpo_replay_run";
  if (int r = rc ? check_calibrate(who, rp, rc) : check_compare(who, rp)) return r;      // (check_calibrate: mean / var as well)
  if (int r = check_finish(who, rp)) return r;
  if (rc)
    if (int r = check_calib_finish(who, rp, rc)) return r;
  if (rr) {
    if (int r = check_reliab_step(who, rp, rr)) return r;
    if (int r = check_reliab_finish(who, rp, rr)) return r;
  }
  if (rv) {
    if (int r = check_votes_step(who, rp, rv, false)) return r;
    if (int r = check_votes_finish(who, rp, rv, false)) return r;
  }
  CMBPO_REQUIRE(model != nullptr, "%s: model handle is NULL", who);
  if (!rc && !ext) CMBPO_REQUIRE(d_elite != nullptr, "%s: NULL buffer (d_elite)", who);     // (the plain run names it before act)
  if (rc && !ext) CMBPO_REQUIRE(rp->act_dim == 0 || rp->act, "%s: NULL buffer (act)", who);
  else CMBPO_REQUIRE((rp->act_dim == 0 || rp->act) && rp->mean && rp->var, "%s: NULL buffer (act / mean / var)", who);
  if (rc) {
    CMBPO_REQUIRE(ensemble == rc->ensemble, "%s: ensemble %d, the calibration descriptor's is %d", who, ensemble, rc->ensemble);
    // (cmbpo_replay_run_calibrated has no d_elite; without a head cmbpo_replay_run_term has always ignored its own)
    if (ext) CMBPO_REQUIRE(d_elite == nullptr || d_elite == rc->elite, "%s: d_elite differs from the calibration descriptor's elite", who);
    d_elite = rc->elite;
  }
  if (rr) {
    CMBPO_REQUIRE(ensemble == rr->ensemble, "%s: ensemble %d, the reliability descriptor's is %d", who, ensemble, rr->ensemble);
    CMBPO_REQUIRE(model->out_dim == rr->out_dim, "%s: the reliability descriptor's out_dim %d is not the model's %d", who, rr->out_dim,
                  model->out_dim);
    CMBPO_REQUIRE(!rc || rc->elite == rr->elite, "%s: the calibration descriptor's elite differs from the reliability descriptor's", who);
    CMBPO_REQUIRE(d_elite == nullptr || d_elite == rr->elite, "%s: d_elite differs from the reliability descriptor's elite", who);
    d_elite = rr->elite;
  }
  if (rv) CMBPO_REQUIRE(ensemble == rv->ensemble, "%s: ensemble %d, the vote descriptor's is %d", who, ensemble, rv->ensemble);
  if (ext) CMBPO_REQUIRE(d_elite != nullptr, "%s: NULL buffer (d_elite)", who);
  if (int r = check_heads(who, rp->obs_dim, model, task, th, ch)) return r;
  return run_steps(who, rp, rc, rr, rv, model, task, ensemble, d_elite, th, ch, stream);
}

// ---- particle replay: host side ---------------------------------------------------------------------------------------------
bool particles_ok(int S) { return S >= 2 && S <= kRows && (S & (S - 1)) == 0; }

int check_part_shape(const char *who, const cmbpo_replay_particles_t *rp) {
  CMBPO_REQUIRE(rp != nullptr, "%s: descriptor is NULL", who);
  CMBPO_REQUIRE(rp->B >= 1, "%s: B %d < 1", who, rp->B);
  CMBPO_REQUIRE(rp->H >= 1, "%s: H %d < 1", who, rp->H);
  CMBPO_REQUIRE(particles_ok(rp->S), "%s: S %d is not a power of two in 2..%d (the particles of a window are the lanes of a part of "
                "one wave)", who, rp->S, kRows);
  CMBPO_REQUIRE(rp->B <= INT32_MAX / kRows, "%s: B %d windows of S %d particles: the rows B S must stay below 2^31", who, rp->B, rp->S);
  CMBPO_REQUIRE(rp->obs_dim >= 1 && rp->act_dim >= 0, "%s: bad dims (obs_dim %d, act_dim %d)", who, rp->obs_dim, rp->act_dim);
  CMBPO_REQUIRE(rp->obs_dim <= CMBPO_REPLAY_PARTICLES_MAX_OBS,
                "%s: obs_dim %d above %d: the 64-row tile a workgroup stages in LDS cannot hold it, and it is not split", who,
                rp->obs_dim, CMBPO_REPLAY_PARTICLES_MAX_OBS);
  CMBPO_REQUIRE(rp->mode == CMBPO_REPLAY_OPEN_LOOP || rp->mode == CMBPO_REPLAY_ONE_STEP, "%s: unknown mode %d", who, rp->mode);
  CMBPO_REQUIRE(rp->reserved == 0 && rp->reserved2 == 0, "%s: reserved %d, %d != 0", who, rp->reserved, rp->reserved2);
  return CMBPO_OK;
}

int check_part_step(const char *who, const cmbpo_replay_particles_t *rp) {
  if (int rc = check_part_shape(who, rp)) return rc;
  CMBPO_REQUIRE(rp->next_obs && rp->rew && rp->cost && rp->term && rp->len, "%s: NULL buffer (recorded arrays)", who);
  CMBPO_REQUIRE(rp->cur_obs && rp->alive, "%s: NULL buffer (cur_obs / alive)", who);
  CMBPO_REQUIRE(rp->p_next_obs && rp->p_rew && rp->p_term && rp->p_cost, "%s: NULL buffer (predictions)", who);
  CMBPO_REQUIRE(rp->part_sum && rp->part_cnt, "%s: NULL buffer (partials)", who);
  return CMBPO_OK;
}

int check_part_finish(const char *who, const cmbpo_replay_particles_t *rp) {
  if (int rc = check_part_shape(who, rp)) return rc;
  CMBPO_REQUIRE(rp->part_sum && rp->part_cnt, "%s: NULL buffer (partials)", who);
  CMBPO_REQUIRE(rp->sums && rp->counts, "%s: NULL buffer (result table)", who);
  return CMBPO_OK;
}

int launch_particles(const cmbpo_replay_particles_t *rp, int h, hipStream_t s) {
  const size_t lds = part_lds_bytes(rp->obs_dim, rp->S);
  if (int rc = cmbpo_grant_lds(replay_particles_kernel, lds)) return rc;
  return launch(replay_particles_kernel, cmbpo_replay_particles_parts(rp->B, rp->S), lds, s, *rp, h);
}

int launch_particles_finish(const cmbpo_replay_particles_t *rp, hipStream_t s) {
  return launch_fold(rp->part_sum, rp->part_cnt, rp->sums, rp->counts, part_sums(rp->obs_dim), part_counts(rp->obs_dim, rp->S), rp->H,
                     cmbpo_replay_particles_parts(rp->B, rp->S), s);
}

int run_particles(const cmbpo_replay_particles_t *rp, const cmbpo_term_head_t *th, const cmbpo_cost_head_t *ch, cmbpo_mlp_t *model,
                  int task, int ensemble, const int32_t *d_elite, void *stream) {
  const char *who = "cmbpo_replay_run_particles";
  if (int r = check_part_step(who, rp)) return r;
  if (int r = check_part_finish(who, rp)) return r;
  CMBPO_REQUIRE(model != nullptr, "%s: model handle is NULL", who);
  CMBPO_REQUIRE(rp->xi != nullptr, "%s: NULL buffer (xi): a particle replay samples its transitions", who);
  CMBPO_REQUIRE(d_elite != nullptr, "%s: NULL buffer (d_elite)", who);
  CMBPO_REQUIRE((rp->act_dim == 0 || rp->act) && rp->mean && rp->var, "%s: NULL buffer (act / mean / var)", who);
  CMBPO_REQUIRE(rp->p_dkl_path && rp->p_ep_var_mean, "%s: NULL buffer (p_dkl_path / p_ep_var_mean)", who);
  if (int r = check_heads(who, rp->obs_dim, model, task, th, ch)) return r;
  FakeenvPostCall pc = post_call(rp, rp->B * rp->S, task, ensemble, th, ch);
  if (int rc = step_model(who, rp, pc, -1, model, d_elite, rp->xi, stream)) return rc;
  for (int h = 0; h < rp->H; ++h) {
    if (int rc = step_model(who, rp, pc, h, model, d_elite, rp->xi, stream)) return rc;
    if (int rc = launch_particles(rp, h, (hipStream_t)stream)) return rc;
  }
  return launch_particles_finish(rp, (hipStream_t)stream);
}

}  // namespace

extern "C" int cmbpo_replay_particles_parts(int B, int S) {
  return B >= 1 && particles_ok(S) && B <= INT32_MAX / kRows ? cmbpo_ceil_div(B * S, kRows) : 0;
}

extern "C" int cmbpo_replay_particles(const cmbpo_replay_particles_t *rp, int h, void *stream) {
  const char *who = "cmbpo_replay_particles";
  if (int rc = check_part_step(who, rp)) return rc;
  if (int r = check_h(who, h, rp->H)) return r;
  return launch_particles(rp, h, (hipStream_t)stream);
}

extern "C" int cmbpo_replay_particles_finish(const cmbpo_replay_particles_t *rp, void *stream) {
  if (int rc = check_part_finish("cmbpo_replay_particles_finish", rp)) return rc;
  return launch_particles_finish(rp, (hipStream_t)stream);
}

extern "C" int cmbpo_replay_run_particles(const cmbpo_replay_particles_t *rp, const cmbpo_term_head_t *th, const cmbpo_cost_head_t *ch,
                                          cmbpo_mlp_t *model, int task, int ensemble, const int32_t *d_elite, void *stream) {
  return run_particles(rp, th, ch, model, task, ensemble, d_elite, stream);
}

extern "C" int cmbpo_replay_parts(int n_rows) { return n_rows >= 1 ? cmbpo_ceil_div(n_rows, kRows) : 0; }

extern "C" int cmbpo_replay_compare(const cmbpo_replay_t *rp, int h, void *stream) {
  const char *who = "cmbpo_replay_compare";
  if (int rc = check_compare(who, rp)) return rc;
  if (int r = check_h(who, h, rp->H)) return r;
  return launch_compare(rp, h, (hipStream_t)stream);
}

extern "C" int cmbpo_replay_finish(const cmbpo_replay_t *rp, void *stream) {
  if (int rc = check_finish("cmbpo_replay_finish", rp)) return rc;
  return launch_finish(rp, (hipStream_t)stream);
}

extern "C" int cmbpo_replay_run(const cmbpo_replay_t *rp, cmbpo_mlp_t *model, int task, int ensemble, const int32_t *d_elite,
                                void *stream) {
  return replay_run(rp, nullptr, nullptr, nullptr, nullptr, nullptr, model, task, ensemble, d_elite, stream);
}

extern "C" int cmbpo_replay_calibrate(const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *rc, int h, void *stream) {
  const char *who = "cmbpo_replay_calibrate";
  if (int r = check_calibrate(who, rp, rc)) return r;
  if (int r = check_h(who, h, rp->H)) return r;
  return launch_calibrate(rp, rc, h, (hipStream_t)stream);
}

extern "C" int cmbpo_replay_calib_finish(const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *rc, void *stream) {
  if (int r = check_calib_finish("cmbpo_replay_calib_finish", rp, rc)) return r;
  return launch_calib_finish(rp, rc, (hipStream_t)stream);
}

extern "C" int cmbpo_replay_run_calibrated(const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *rc, cmbpo_mlp_t *model, int task,
                                           int ensemble, void *stream) {
  if (rc == nullptr) return check_calibrate("cmbpo_replay_run_calibrated", rp, rc);      // (this entry's own error, not the plain run)
  return replay_run(rp, rc, nullptr, nullptr, nullptr, nullptr, model, task, ensemble, nullptr, stream);
}

extern "C" int cmbpo_replay_run_term(const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *rc, const cmbpo_term_head_t *th,
                                     cmbpo_mlp_t *model, int task, int ensemble, const int32_t *d_elite, void *stream) {
  return replay_run(rp, rc, nullptr, nullptr, th, nullptr, model, task, ensemble, d_elite, stream);
}

extern "C" int cmbpo_replay_run_cost(const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *rc, const cmbpo_term_head_t *th,
                                     const cmbpo_cost_head_t *ch, cmbpo_mlp_t *model, int task, int ensemble, const int32_t *d_elite,
                                     void *stream) {
  return replay_run(rp, rc, nullptr, nullptr, th, ch, model, task, ensemble, d_elite, stream);
}

extern "C" int cmbpo_replay_reliab(const cmbpo_replay_t *rp, const cmbpo_replay_reliab_t *rr, int h, void *stream) {
  const char *who = "cmbpo_replay_reliab";
  if (int r = check_reliab_step(who, rp, rr)) return r;
  if (int r = check_h(who, h, rp->H)) return r;
  return launch_reliab(rp, rr, h, (hipStream_t)stream);
}

extern "C" int cmbpo_replay_reliab_finish(const cmbpo_replay_t *rp, const cmbpo_replay_reliab_t *rr, void *stream) {
  if (int r = check_reliab_finish("cmbpo_replay_reliab_finish", rp, rr)) return r;
  return launch_reliab_finish(rp, rr, (hipStream_t)stream);
}

extern "C" int cmbpo_replay_run_reliab(const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *rc, const cmbpo_replay_reliab_t *rr,
                                       const cmbpo_term_head_t *th, const cmbpo_cost_head_t *ch, cmbpo_mlp_t *model, int task,
                                       int ensemble, const int32_t *d_elite, void *stream) {
  return replay_run(rp, rc, rr, nullptr, th, ch, model, task, ensemble, d_elite, stream);
}

extern "C" int cmbpo_replay_votes(const cmbpo_replay_t *rp, const cmbpo_replay_votes_t *rv, int h, void *stream) {
  const char *who = "cmbpo_replay_votes";
  if (int r = check_votes_step(who, rp, rv, true)) return r;
  if (int r = check_h(who, h, rp->H)) return r;
  return launch_votes(rp, rv, h, (hipStream_t)stream);
}

extern "C" int cmbpo_replay_votes_finish(const cmbpo_replay_t *rp, const cmbpo_replay_votes_t *rv, void *stream) {
  if (int r = check_votes_finish("cmbpo_replay_votes_finish", rp, rv, true)) return r;
  return launch_votes_finish(rp, rv, (hipStream_t)stream);
}

extern "C" int cmbpo_replay_run_votes(const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *rc, const cmbpo_replay_reliab_t *rr,
                                      const cmbpo_replay_votes_t *rv, const cmbpo_term_head_t *th, const cmbpo_cost_head_t *ch,
                                      cmbpo_mlp_t *model, int task, int ensemble, const int32_t *d_elite, void *stream) {
  return replay_run(rp, rc, rr, rv, th, ch, model, task, ensemble, d_elite, stream);
}
