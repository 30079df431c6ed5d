// Start states of an imagined-rollout round, drawn on the device from the mirror of CPOBuffer's archive
// (algorithms/cmbpo.py:239-251: epoch_batch -> compute_DKL -> boltz_dist -> distributed_batch_from_archive -> reset).
//
// The archive's epoch column is written as contiguous slabs (one per CPOBuffer.get), so it is a handful of runs of equal
// tags: n_epochs of them, plus one or two after a wrap-around, plus the empty tail (-1).  Everything here works on that
// run table instead of the [N] column:
//   table   the runs in ascending archive order, the sorted epochs present, their sample counts (np.bincount) and, per
//           epoch, its runs with the number of members in front of each -- the k-th member of an epoch
//           (np.flatnonzero(epoch_archive == e)[k]) is a walk over that epoch's runs;
//   (b)     members_e[min(floor(u n_e), n_e - 1)] for u[n_epochs][B], the drawn rows' observations / mu / log_std gathered;
//   (c)     per-row diagonal-Gaussian KL(current || stored) (network/ac_network.py:50-55, the expression MODE_EVAL of
//           policy_update.hip accumulates), float64 partial sums per workgroup in a fixed order;
//   (d)     the partials folded per epoch, clipped at 0 (cmbpo.py:220); Boltzmann weights, the per-sample probability
//           rounded to float32 (boltz_dist stores it in a float32 array) and the float64 CDF np.random.choice builds.  A
//           sample's probability is constant inside a run, so the inclusive sum at member k of run r is
//           prefix_r + (k + 1) p_r: the product is exact in float64 (24-bit p, < 2^24 members), so the value carries ONE
//           rounding where a sequential cumsum carries one per archive slot, and it does not depend on any launch shape.
//           A draw is searchsorted(cdf, u, side='right'): a binary search over the runs, then over the members of one run.
// No float atomics anywhere: the same archive, policy and uniforms give the same bits.
#include "common.h"

namespace {

constexpr int M = CMBPO_START_MAX_RUNS;
// int32 table: header, then sections of M entries
enum { T_NRUNS = 0, T_NEPOCHS = 1, T_OVERFLOW = 2, T_FILLED = 3, T_HDR = 8 };
enum { S_RUN_START = 0, S_RUN_LEN, S_RUN_RANK, S_EP_LIST, S_EP_COUNT, S_G_START, S_G_CUM, S_EP_OFF, S_EP_OFF_TAIL, S_RAW };
__host__ __device__ constexpr int sec(int k) { return T_HDR + k * M; }
static_assert(sec(S_RAW) + 1 + M <= CMBPO_START_TABLE_INTS, "table size");
// float64 cdf block
enum { C_TOTAL = 0, C_STATUS = 1, C_HDR = 8 };
__host__ __device__ constexpr int csec(int k) { return C_HDR + k * M; }   // 0 cdf_end, 1 prefix, 2 p, 3 ep_probs
static_assert(csec(4) <= CMBPO_START_CDF_DOUBLES, "cdf size");

constexpr int KL_ROWS_PER_BLOCK = 1024;

// ---- table -----------------------------------------------------------------------------------------------------------------
// run heads in whatever order the workgroups arrive (an integer ticket); start_table_kernel sorts them
__global__ __launch_bounds__(256) void start_heads_kernel(const int32_t *__restrict__ ep, long n, int32_t *__restrict__ table) {
  int32_t *raw = table + sec(S_RAW);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int32_t e = ep[i];
    if (i == 0 || ep[i - 1] != e) {
      const int pos = atomicAdd(&raw[0], 1);
      if (pos < M) raw[1 + pos] = (int32_t)i;
    }
  }
}

__global__ __launch_bounds__(M) void start_table_kernel(const int32_t *__restrict__ ep, long n, int32_t *__restrict__ table) {
  __shared__ int32_t s_start[M], s_ep[M], s_len[M], s_first[M], s_nruns[M], s_off[M];
  const int t = threadIdx.x;
  const int32_t *raw = table + sec(S_RAW);
  const int n_raw = raw[0], nr = n_raw < M ? n_raw : M;
  // ascending starts: the rank of a start among distinct starts is its place
  if (t < nr) {
    const int32_t s = raw[1 + t];
    int place = 0;
    for (int j = 0; j < nr; ++j) place += raw[1 + j] < s;
    s_start[place] = s;
  }
  __syncthreads();
  int32_t start = 0, len = 0, e = -1;
  if (t < nr) {
    start = s_start[t];
    len = (int32_t)((t + 1 < nr ? (long)s_start[t + 1] : n) - start);
    e = ep[start];
    s_ep[t] = e;
    s_len[t] = len;
  }
  __syncthreads();
  const bool live = t < nr && e >= 0;
  int within = 0, cum = 0, count = 0, runs = 0;
  if (live)
    for (int j = 0; j < nr; ++j)
      if (s_ep[j] == e) {
        if (j < t) { ++within; cum += s_len[j]; }
        count += s_len[j];
        ++runs;
      }
  const bool first = live && within == 0;
  if (t < nr) s_first[t] = first;
  const int n_ep = __syncthreads_count(first);
  int rank = -1;
  if (live) {
    rank = 0;
    for (int j = 0; j < nr; ++j) rank += s_first[j] && s_ep[j] < e;
  }
  if (first) {
    s_nruns[rank] = runs;
    table[sec(S_EP_LIST) + rank] = e;
    table[sec(S_EP_COUNT) + rank] = count;
  }
  __syncthreads();
  if (t < n_ep || t == 0) {      // ep_off[0 .. n_ep]: M + 1 entries when every run is an epoch of its own
    int off = 0;
    for (int j = 0; j < t; ++j) off += s_nruns[j];
    s_off[t] = off;
    table[sec(S_EP_OFF) + t] = off;
    if (t == n_ep - 1) table[sec(S_EP_OFF) + n_ep] = off + s_nruns[t];
  }
  __syncthreads();
  if (t < nr) {
    table[sec(S_RUN_START) + t] = start;
    table[sec(S_RUN_LEN) + t] = len;
    table[sec(S_RUN_RANK) + t] = rank;
    if (live) {
      const int g = s_off[rank] + within;
      table[sec(S_G_START) + g] = start;
      table[sec(S_G_CUM) + g] = cum;
    }
  }
  int filled = 0;
  if (first) filled = count;
  // (sum of the epochs' counts: a tree over the workgroup, integer)
  __shared__ int32_t s_fill[M / 64];
  filled = wave_sum(filled);
  if ((t & 63) == 0) s_fill[t >> 6] = filled;
  __syncthreads();
  if (t == 0) {
    int f = 0;
    for (int w = 0; w < M / 64; ++w) f += s_fill[w];
    table[T_NRUNS] = nr;
    table[T_NEPOCHS] = n_ep;
    table[T_OVERFLOW] = n_raw > M;
    table[T_FILLED] = f;
  }
}

// ---- gathers ---------------------------------------------------------------------------------------------------------------
// rows idx[0..rows) of src[.][width] -> dst[row0 + .][width], the workgroup's 256 rows; dst is written coalesced
__device__ __forceinline__ void gather_rows(const float *__restrict__ src, float *__restrict__ dst, const int32_t *idx,
                                            long row0, int rows, int width) {
  const int total = rows * width;
  for (int x = threadIdx.x; x < total; x += 256) {
    const int r = x / width, c = x - r * width;
    dst[(size_t)(row0 + r) * width + c] = src[(size_t)idx[r] * width + c];
  }
}

// (b) epoch_batch, buffers/cpobuffer.py:466-524
__global__ __launch_bounds__(256) void start_epoch_draw_kernel(const int32_t *__restrict__ table, const int32_t *__restrict__ sel,
                                                               int n_epochs, int batch,
                                                               const double *__restrict__ u, const float *__restrict__ obs,
                                                               const float *__restrict__ mu, const float *__restrict__ ls, long n,
                                                               int obs_dim, int act_dim, int32_t *__restrict__ idx_out,
                                                               float *__restrict__ obs_out, float *__restrict__ mu_out,
                                                               float *__restrict__ ls_out) {
  __shared__ int32_t s_idx[256];
  const long rows_all = (long)n_epochs * batch;
  const long row0 = (long)blockIdx.x * 256, j = row0 + threadIdx.x;
  if (j < rows_all) {
    int e = (int)(j / batch);
    if (sel) e = sel[e];                                        // group -> place in epochs_list
    e = max(min(e, table[T_NEPOCHS] - 1), 0);                   // (a table of the same archive never needs it)
    const int n_e = table[sec(S_EP_COUNT) + e];
    long k = (long)floor(u[j] * (double)n_e);
    k = k < 0 ? 0 : (k > n_e - 1 ? n_e - 1 : k);
    const int g0 = table[sec(S_EP_OFF) + e], g1 = table[sec(S_EP_OFF) + e + 1];
    int g = g0;
    while (g + 1 < g1 && table[sec(S_G_CUM) + g + 1] <= k) ++g;
    long i = (long)table[sec(S_G_START) + g] + (k - table[sec(S_G_CUM) + g]);
    i = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);       // (a consistent table never needs it)
    s_idx[threadIdx.x] = (int32_t)i;
    idx_out[j] = (int32_t)i;
  }
  __syncthreads();
  const long left = rows_all - row0;
  const int rows = left < 256 ? (int)left : 256;
  gather_rows(obs, obs_out, s_idx, row0, rows, obs_dim);
  gather_rows(mu, mu_out, s_idx, row0, rows, act_dim);
  gather_rows(ls, ls_out, s_idx, row0, rows, act_dim);
}

// ---- (c) ---------------------------------------------------------------------------------------------------------------------
// rows [blk * 1024, ..) of epoch group e: every thread adds its rows (tid, tid + 256, ..) in float64, the wave tree and the
// four waves are added in a fixed order
__global__ __launch_bounds__(256) void start_kl_kernel(const float *__restrict__ mu, const float *__restrict__ ls,
                                                       const float *__restrict__ mu_old, const float *__restrict__ ls_old,
                                                       int batch, int act_dim, double *__restrict__ part, int n_part) {
  __shared__ double s_w[4];
  const int e = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
  const int b0 = blk * KL_ROWS_PER_BLOCK, b1 = min(batch, b0 + KL_ROWS_PER_BLOCK);
  double acc = 0.0;
  for (int b = b0 + tid; b < b1; b += 256) {
    const size_t at = ((size_t)e * batch + b) * act_dim;
    double row = 0.0;
    for (int a = 0; a < act_dim; ++a) {
      // gaussian_kl(mu, log_std, mu_old, log_std_old), ac_network.py:50-55
      const float l = ls[at + a], lo = ls_old[at + a];
      const float dm = mu_old[at + a] - mu[at + a];
      const float pre = 0.5f * ((dm * dm + expf(2.0f * l)) / (expf(2.0f * lo) + 1e-8f) - 1.0f) + lo - l;
      row += (double)pre;
    }
    acc += row;
  }
  acc = wave_sum(acc);
  if ((tid & 63) == 0) s_w[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) part[(size_t)e * n_part + blk] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// ---- (d) ---------------------------------------------------------------------------------------------------------------------
// np.sum of a float64 array as NumPy adds it (pairwise_sum: eight running sums below 128 elements); above that, the
// 128-element blocks in order
__device__ double numpy_sum(const double *a, int n) {
  double total = 0.0;
  for (int base = 0; base < n; base += 128) {
    const int m = n - base < 128 ? n - base : 128;
    const double *x = a + base;
    double res;
    if (m < 8) {
      res = 0.0;
      for (int i = 0; i < m; ++i) res += x[i];
    } else {
      double r[8];
      for (int q = 0; q < 8; ++q) r[q] = x[q];
      int i = 8;
      for (; i < m - (m % 8); i += 8)
        for (int q = 0; q < 8; ++q) r[q] += x[i + q];
      res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
      for (; i < m; ++i) res += x[i];
    }
    total = base == 0 ? res : total + res;
  }
  return total;
}

__global__ __launch_bounds__(M) void start_cdf_kernel(const int32_t *__restrict__ table, const double *__restrict__ part,
                                                      int n_part, int batch, double *__restrict__ kl, double alpha,
                                                      double *__restrict__ cdf) {
  __shared__ double s_w[M], s_p[M], s_pre[M], s_end[M];
  __shared__ double s_tot[2];
  const int t = threadIdx.x;
  const int nr = table[T_NRUNS], n_ep = table[T_NEPOCHS];
  if (t < n_ep) {
    double k;
    if (part) {
      double s = 0.0;
      for (int b = 0; b < n_part; ++b) s += part[(size_t)t * n_part + b];
      k = s / (double)batch;
      k = k < 0.0 ? 0.0 : k;               // np.clip(kls, a_min=0), cmbpo.py:220
      kl[t] = k;
    } else {
      k = kl[t];
    }
    s_w[t] = exp(alpha * -k);              // boltz_dist, cpobuffer.py:385-396
  }
  __syncthreads();
  if (t == 0) s_tot[0] = numpy_sum(s_w, n_ep);
  __syncthreads();
  if (t < n_ep) {
    const double pe = s_w[t] / s_tot[0];
    const float p32 = (float)(pe / (double)(float)table[sec(S_EP_COUNT) + t]);   // (a float32 array holds it)
    s_p[t] = (double)p32;
    cdf[csec(3) + t] = pe;
  }
  __syncthreads();
  if (t == 0) {
    double acc = 0.0;
    for (int r = 0; r < nr; ++r) {
      const int rank = table[sec(S_RUN_RANK) + r];
      const double p = rank >= 0 ? s_p[rank] : 0.0;
      s_pre[r] = acc;
      acc = acc + (double)table[sec(S_RUN_LEN) + r] * p;
      s_end[r] = acc;
    }
    s_tot[1] = acc;
    cdf[C_TOTAL] = acc;
    if (!(acc > 0.0 && acc < 1e300)) cdf[C_STATUS] = 1.0;       // no mass, or a NaN / inf weight: the draw is void (sticky:
                                                                 // the host looks at it where it synchronises anyway)
  }
  __syncthreads();
  if (t < nr) {
    const int rank = table[sec(S_RUN_RANK) + t];
    cdf[csec(0) + t] = s_end[t] / s_tot[1];
    cdf[csec(1) + t] = s_pre[t];
    cdf[csec(2) + t] = rank >= 0 ? s_p[rank] : 0.0;
  }
}

// np.random.choice(p=): cdf.searchsorted(u, side='right') -- the first slot whose inclusive sum exceeds u
__global__ __launch_bounds__(256) void start_boltz_draw_kernel(const int32_t *__restrict__ table, const double *__restrict__ cdf,
                                                               const double *__restrict__ u, int batch,
                                                               const float *__restrict__ obs, long n, int obs_dim,
                                                               int32_t *__restrict__ idx_out, float *__restrict__ out) {
  __shared__ int32_t s_idx[256];
  const long row0 = (long)blockIdx.x * 256, j = row0 + threadIdx.x;
  if (j < batch) {
    const int nr = table[T_NRUNS];
    double v = u[j];
    v = v >= 0.0 ? v : 0.0;
    v = v < 1.0 ? v : 0.99999999999999989;
    int lo = 0, hi = nr - 1;                      // first run whose end exceeds v (the last run's end is 1)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cdf[csec(0) + mid] > v) hi = mid; else lo = mid + 1;
    }
    const double total = cdf[C_TOTAL], pre = cdf[csec(1) + lo], p = cdf[csec(2) + lo];
    int klo = 0, khi = table[sec(S_RUN_LEN) + lo] - 1;   // first member whose inclusive sum exceeds v
    while (klo < khi) {
      const int mid = (klo + khi) >> 1;
      if ((pre + (double)(mid + 1) * p) / total > v) khi = mid; else klo = mid + 1;
    }
    long i = (long)table[sec(S_RUN_START) + lo] + klo;
    i = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
    s_idx[threadIdx.x] = (int32_t)i;
    idx_out[j] = (int32_t)i;
  }
  __syncthreads();
  const long left = (long)batch - row0;
  gather_rows(obs, out, s_idx, row0, left < 256 ? (int)left : 256, obs_dim);
}

}  // namespace

extern "C" int cmbpo_start_table_build(const int32_t *d_epochs, long n, int32_t *d_table, void *stream) {
  CMBPO_REQUIRE(d_epochs && d_table, "cmbpo_start_table_build: NULL buffer");
  CMBPO_REQUIRE(n >= 1 && n <= 0x7fffffffL, "cmbpo_start_table_build: archive size %ld outside [1, 2^31)", n);
  hipStream_t s = (hipStream_t)stream;
  CMBPO_HIP_CHECK(hipMemsetAsync(d_table + sec(S_RAW), 0, sizeof(int32_t), s));
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(start_heads_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, d_epochs, n, d_table);
  hipLaunchKernelGGL(start_table_kernel, dim3(1), dim3(M), 0, s, d_epochs, n, d_table);
  CMBPO_HIP_CHECK(hipGetLastError());
  return CMBPO_OK;
}

extern "C" int cmbpo_start_epoch_draw(const int32_t *d_table, const int32_t *d_epoch_sel, int n_epochs, int batch, const double *d_u,
                                      const float *d_obs, const float *d_mu, const float *d_logstd, long n,
                                      int obs_dim, int act_dim, int32_t *d_idx, float *d_obs_out, float *d_mu_out,
                                      float *d_logstd_out, void *stream) {
  CMBPO_REQUIRE(d_table && d_u && d_obs && d_mu && d_logstd && d_idx && d_obs_out && d_mu_out && d_logstd_out,
                "cmbpo_start_epoch_draw: NULL buffer");
  CMBPO_REQUIRE(n_epochs >= 1 && n_epochs <= M, "cmbpo_start_epoch_draw: n_epochs %d outside [1, %d]", n_epochs, M);
  CMBPO_REQUIRE(batch >= 1 && n >= 1 && n <= 0x7fffffffL && obs_dim >= 1 && act_dim >= 1,
                "cmbpo_start_epoch_draw: batch %d / archive size %ld / obs_dim %d / act_dim %d", batch, n, obs_dim, act_dim);
  const long blocks = ((long)n_epochs * batch + 255) / 256;
  CMBPO_REQUIRE(blocks <= 0x7fffffffL, "cmbpo_start_epoch_draw: n_epochs * batch too large");
  hipLaunchKernelGGL(start_epoch_draw_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_table, d_epoch_sel,
                     n_epochs, batch, d_u, d_obs, d_mu, d_logstd, n, obs_dim, act_dim, d_idx, d_obs_out, d_mu_out, d_logstd_out);
  CMBPO_HIP_CHECK(hipGetLastError());
  return CMBPO_OK;
}

extern "C" int cmbpo_start_kl_parts(int batch) { return batch >= 1 ? cmbpo_ceil_div(batch, KL_ROWS_PER_BLOCK) : 0; }

extern "C" int cmbpo_start_kl_partials(const float *d_mu, const float *d_logstd, const float *d_mu_old,
                                       const float *d_logstd_old, int n_epochs, int batch, int act_dim,
                                       double *d_part, int n_part, void *stream) {
  CMBPO_REQUIRE(d_mu && d_logstd && d_mu_old && d_logstd_old && d_part, "cmbpo_start_kl_partials: NULL buffer");
  CMBPO_REQUIRE(n_epochs >= 1 && n_epochs <= M && batch >= 1 && act_dim >= 1,
                "cmbpo_start_kl_partials: n_epochs %d / batch %d / act_dim %d", n_epochs, batch, act_dim);
  CMBPO_REQUIRE(n_part == cmbpo_start_kl_parts(batch), "cmbpo_start_kl_partials: n_part %d, cmbpo_start_kl_parts(%d) = %d",
                n_part, batch, cmbpo_start_kl_parts(batch));
  hipLaunchKernelGGL(start_kl_kernel, dim3(n_part, n_epochs), dim3(256), 0, (hipStream_t)stream, d_mu, d_logstd, d_mu_old,
                     d_logstd_old, batch, act_dim, d_part, n_part);
  CMBPO_HIP_CHECK(hipGetLastError());
  return CMBPO_OK;
}

extern "C" int cmbpo_start_cdf(const int32_t *d_table, const double *d_part, int n_part, int batch, double *d_kl,
                               double alpha, double *d_cdf, void *stream) {
  CMBPO_REQUIRE(d_table && d_kl && d_cdf, "cmbpo_start_cdf: NULL buffer");
  CMBPO_REQUIRE(d_part == nullptr || (n_part >= 1 && batch >= 1), "cmbpo_start_cdf: n_part %d / batch %d with partial sums given",
                n_part, batch);
  CMBPO_REQUIRE(alpha == alpha, "cmbpo_start_cdf: alpha is NaN");
  hipLaunchKernelGGL(start_cdf_kernel, dim3(1), dim3(M), 0, (hipStream_t)stream, d_table, d_part, n_part, batch, d_kl, alpha, d_cdf);
  CMBPO_HIP_CHECK(hipGetLastError());
  return CMBPO_OK;
}

extern "C" int cmbpo_start_boltz_draw(const int32_t *d_table, const double *d_cdf, const double *d_u, int batch,
                                      const float *d_obs, long n, int obs_dim, int32_t *d_idx, float *d_out,
                                      void *stream) {
  CMBPO_REQUIRE(d_table && d_cdf && d_u && d_obs && d_idx && d_out, "cmbpo_start_boltz_draw: NULL buffer");
  CMBPO_REQUIRE(batch >= 1 && n >= 1 && n <= 0x7fffffffL && obs_dim >= 1,
                "cmbpo_start_boltz_draw: batch %d / archive size %ld / obs_dim %d", batch, n, obs_dim);
  hipLaunchKernelGGL(start_boltz_draw_kernel, dim3(cmbpo_ceil_div(batch, 256)), dim3(256), 0, (hipStream_t)stream, d_table, d_cdf,
                     d_u, batch, d_obs, n, obs_dim, d_idx, d_out);
  CMBPO_HIP_CHECK(hipGetLastError());
  return CMBPO_OK;
}
