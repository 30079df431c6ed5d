// Ensemble-voted static rules (include/cmbpo_hip.h, cmbpo_rule_votes_t): the task's termination / cost rule evaluated
// on every member's predicted next state, the votes counted, and term / cost (/ cost_var) of the post step rewritten from them.
// A kernel of its own, launched by cmbpo_internal_fakeenv_post right behind the post kernel when the votes are given: the post
// kernel's instances and argument blocks are untouched, so a call without the votes is the call it always was.
//
// The per-value clause test, the derived-quantity formula and the two built-in formulas below are a SECOND definition: the first
// is fakeenv_post_kernel's tail (csrc/fakeenv_post.hip, `RULES != 0`, `RULES == 2`, CMBPO_TASK_ANTSAFE, CMBPO_TASK_HCS), which
// spreads a clause's columns over a row's eight lanes; here a lane owns a MEMBER and walks the columns itself.  Every operation
// is the same single-rounded float32 operation in the same order (the file is built without contraction), and the GPU tests
// hold the elite's verdict of this kernel against the post kernel's bit for bit.  Change one, change the other.
#include "common.h"
#include "fakeenv_post_internal.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kLoads = 8;                 // image elements a thread requests before it waits for the first
constexpr int kRowsMax = 32;             // rows per workgroup: eight lanes per row, all 256 threads busy in the vote phase
constexpr size_t kLdsBudget = 32 * 1024;  // the next-state image of a workgroup stays below this: rows are sized down, no LDS grant

struct VotesArgs {
  int task, ensemble, obs_dim, act_dim, out_dim;
  int rules_on;         // a registered clause table (p.rules / p.der) in place of the built-in rule sets
  int learned_cost;     // the static cost rule is skipped: cost / cost_var stay the post kernel's
  int dis_on;           // write cost_var (static cost only)
  int rows_wg;          // rows per workgroup (a power of two <= kRowsMax)
  const float *mean, *var;
  int ld_rows;
  const float *obs, *act, *xi;      // xi NULL: the deterministic transition (var is not read)
  const int32_t *elite, *row_idx, *n_rows_dev;
  int n_rows;
  uint8_t *term;
  float *cost, *cost_var;
  float kappa_cost;
  // learned_done, recovered from what the post kernel wrote for the termination head (th_on == 0: no head)
  int th_on, th_members;
  float threshold;
  const float *term_pred;
  const uint8_t *term_votes;
  const float *term_thr;            // sampled terminations: the row's own threshold, or NULL
  int done_members, cost_members;
  uint8_t *done_votes, *cost_votes;
  cmbpo_task_rules_t rules;         // resolved on the host, by value (uniform: scalar loads from the kernel-argument segment)
  cmbpo_rule_derived_table_t der;
};

__global__ __launch_bounds__(kThreads) void rule_votes_kernel(const VotesArgs p) {
  extern __shared__ float sm[];
  const int D = p.obs_dim, E = p.ensemble, R = p.rows_wg;
  const int Dp = D | 1;                                     // odd row pitch: a row's eight lanes walk eight members' images side by side
  float *s_nx = sm;                                         // [R][E][Dp]
  int *s_row = reinterpret_cast<int *>(s_nx + (size_t)R * E * Dp);   // [R]

  const int tid = threadIdx.x;
  const int n_rows = p.n_rows_dev ? *p.n_rows_dev : p.n_rows;
  const int row0 = blockIdx.x * R;
  if (row0 >= n_rows) return;
  if (tid < R) {
    const int r = row0 + tid;
    s_row[tid] = (r < n_rows) ? (p.row_idx ? p.row_idx[r] : r) : -1;
  }
  __syncthreads();

  // Phase 1: every member's next state of the workgroup's rows, nx_e = fl32(mu_e + obs) with mu_e the member's mean or, with
  // draws, fl32(mean_e + fl32(sqrtf(var_e) * xi)) -- the post kernel's expression for the elite, for every member.  d runs
  // fastest: the loads of a member's row are coalesced.
  const size_t mstride = (size_t)p.ld_rows * p.out_dim;
  // kLoads elements per thread and pass, every load of the pass requested before the first is used: written element by element,
  // a workgroup walked two dozen dependent memory round trips (the row-past-the-end branch keeps hipcc from hoisting the loads).
  const int ED = E * D, total = R * ED;
  const bool noise = p.xi != nullptr;
  for (int i0 = tid; i0 < total; i0 += kThreads * kLoads) {
    float mu[kLoads], ob[kLoads], vr[kLoads], xs[kLoads];
    int at[kLoads];
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
      const int i = i0 + u * kThreads;
      at[u] = -1;
      mu[u] = ob[u] = vr[u] = xs[u] = 0.0f;
      if (i < total) {
        const int b = i / ED, j = i - b * ED;
        const int e = j / D, d = j - e * D;
        const int r = s_row[b];
        if (r >= 0) {
          const size_t o = e * mstride + (size_t)r * p.out_dim + d;
          at[u] = (b * E + e) * Dp + d;
          mu[u] = p.mean[o];
          ob[u] = p.obs[(size_t)r * D + d];
          if (noise) {
            vr[u] = p.var[o];
            xs[u] = p.xi[(size_t)r * D + d];
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
      if (at[u] < 0) continue;
      float m = mu[u];
      if (noise) m = __fadd_rn(m, __fmul_rn(sqrtf(vr[u]), xs[u]));
      s_nx[at[u]] = __fadd_rn(m, ob[u]);
    }
  }
  __syncthreads();

  // Phase 2: lane k of a row's eight lanes owns member k (as the post kernel's DIS and TERM parts do) and evaluates the whole
  // rule on that member's image.  Rows past the end and lanes past E evaluate nothing and vote 0.
  if (tid >= 8 * R) return;
  const int rw = tid >> 3, k = tid & 7;
  const int r = s_row[rw];
  const bool valid = r >= 0 && k < E;
  bool done_e = false, cost_e = false;
  if (valid) {
    const float *nx = s_nx + (size_t)(rw * E + k) * Dp;
    bool fin = true;
    for (int d = 0; d < D; ++d) fin = fin && isfinite(nx[d]);
    if (p.rules_on) {
      // a derived quantity: g = bias; per term t = fl32(x - c), squared with pow 2, g = fl32(g + fl32(w * t))
      auto derived_g = [&](int j) {
        const cmbpo_rule_derived_t &dq = p.der.derived[j];
        float g = dq.bias;
        for (int t = 0; t < dq.n_terms; ++t) {
          const int col = dq.term[t].col;
          const float x = dq.term[t].src == CMBPO_RULE_SRC_NEXT_OBS ? nx[col]
                          : dq.term[t].src == CMBPO_RULE_SRC_OBS    ? p.obs[(size_t)r * D + col]
                                                                    : p.act[(size_t)r * p.act_dim + col];
          float tt = __fsub_rn(x, dq.term[t].c);
          if (dq.term[t].pow == 2) tt = __fmul_rn(tt, tt);
          g = __fadd_rn(g, __fmul_rn(dq.term[t].w, tt));
        }
        return g;
      };
      bool rule_done = false, rule_obj = false;
      for (int c = 0; c < p.rules.n_clauses; ++c) {
        const cmbpo_rule_clause_t &cl = p.rules.clause[c];
        bool all_k = true, any_k = false;
        for (int d = cl.col0; d < cl.col0 + cl.n_cols; ++d) {
          const float x = cl.src == CMBPO_RULE_SRC_NEXT_OBS  ? nx[d]
                          : cl.src == CMBPO_RULE_SRC_DERIVED ? derived_g(d)
                          : cl.src == CMBPO_RULE_SRC_OBS     ? p.obs[(size_t)r * D + d]
                                                             : p.act[(size_t)r * p.act_dim + d];
          float f = __fmul_rn(x, cl.scale);
          if (cl.flags & CMBPO_RULE_ABS) f = fabsf(f);
          // positive tests: false for a NaN, like NumPy's comparisons
          const bool lo_ok = (cl.flags & CMBPO_RULE_LO_STRICT) ? f > cl.lo : f >= cl.lo;
          const bool hi_ok = (cl.flags & CMBPO_RULE_HI_STRICT) ? f < cl.hi : f <= cl.hi;
          all_k = all_k && lo_ok && hi_ok;
          any_k = any_k || (lo_ok && hi_ok);
        }
        const bool holds = (cl.flags & CMBPO_RULE_ANY) ? any_k : all_k;
        if (cl.role == CMBPO_RULE_HEALTHY) rule_done = rule_done || !holds;
        else if (cl.role == CMBPO_RULE_FATAL) rule_done = rule_done || holds;
        else rule_obj = rule_obj || holds;
      }
      done_e = (p.rules.require_finite && !fin) || rule_done;
      cost_e = p.rules.cost_on_term ? (done_e || rule_obj) : rule_obj;      // min(1, done + obj) > 0
    } else if (p.task == CMBPO_TASK_ANTSAFE) {
      // statics.py:17-53, the precedence quirk included: the product of the three conditions gates z_rot
      const float z = nx[0];
      const float q1 = nx[2], q2 = nx[3];
      const float zrot = __fsub_rn(1.0f, __fmul_rn(2.0f, __fadd_rn(__fmul_rn(q1, q1), __fmul_rn(q2, q2))));
      const float gate = (fin && z >= 0.2f && z <= 1.0f) ? 1.0f : 0.0f;
      done_e = !(__fmul_rn(gate, zrot) >= -0.7f);
      cost_e = done_e || fabsf(nx[D - 1]) > 3.2f;                           // clip(done + obj, 0, 1) > 0
    } else if (p.task == CMBPO_TASK_HCS) {
      cost_e = fabsf(__fmul_rn(nx[D - 1], 10.0f)) < 2.0f;                   // statics.py:10-15
    }
    if (p.learned_cost) cost_e = false;
  }
  // one ballot per verdict: the row's member mask in the row's byte of its wave; the elite's bit is me & 7, the votes a popcount
  const int sh = 8 * (rw & 7);
  const unsigned dmask = (unsigned)(__ballot(done_e) >> sh) & 0xffu;
  const unsigned cmask = (unsigned)(__ballot(cost_e) >> sh) & 0xffu;
  if (r < 0 || k != 0) return;
  const int me = p.elite[r] & 7;
  const int dv = __popc(dmask), cv = __popc(cmask);
  const bool rule_done = p.done_members == CMBPO_TERM_ELITE ? ((dmask >> me) & 1u) != 0u
                         : p.done_members == CMBPO_TERM_ANY ? dv > 0 : 2 * dv > E;
  // learned_done from the head's own outputs of this step (the post kernel ahead of this one on the stream wrote them)
  bool learned = false;
  if (p.th_on) {
    if (p.th_members == CMBPO_TERM_ELITE) {
      const float thr = p.term_thr != nullptr ? p.term_thr[r] : p.threshold;
      learned = p.term_pred[r] > thr;                       // a positive test: a NaN on either side never hits
    } else {
      const int tv = p.term_votes[r];
      learned = p.th_members == CMBPO_TERM_ANY ? tv > 0 : 2 * tv > E;
    }
  }
  p.term[r] = (rule_done || learned) ? 1 : 0;
  if (p.done_votes != nullptr) p.done_votes[r] = (uint8_t)dv;
  if (p.learned_cost) return;                               // cost, cost_var: the learned column's, as the post kernel left them
  if (p.cost_votes != nullptr) p.cost_votes[r] = (uint8_t)cv;
  float cost;
  if (p.cost_members == CMBPO_TERM_ELITE) cost = ((cmask >> me) & 1u) ? 1.0f : 0.0f;
  else if (p.cost_members == CMBPO_TERM_ANY) cost = cv > 0 ? 1.0f : 0.0f;
  else if (p.cost_members == CMBPO_TERM_MAJORITY) cost = 2 * cv > E ? 1.0f : 0.0f;
  else cost = (float)cv / (float)E;
  if (p.dis_on) {
    // np.var over the members in cmbpo_fakeenv_post_disagreement's order: s = ((x0 + x1) + x2) + ..., m = s / E,
    // q = sum (x_e - m)^2 in member order, var = q / E
    float s = 0.0f;
    for (int e = 0; e < E; ++e) s = __fadd_rn(s, ((cmask >> e) & 1u) ? 1.0f : 0.0f);
    const float mbar = s / (float)E;
    float sq = 0.0f;
    for (int e = 0; e < E; ++e) {
      const float dlt = __fsub_rn(((cmask >> e) & 1u) ? 1.0f : 0.0f, mbar);
      sq = __fadd_rn(sq, __fmul_rn(dlt, dlt));
    }
    const float var = sq / (float)E;
    p.cost_var[r] = var;
    if (p.kappa_cost > 0.0f) {
      const float c = __fadd_rn(cost, __fmul_rn(p.kappa_cost, sqrtf(var)));
      cost = c > 1.0f ? 1.0f : c;
    }
  }
  p.cost[r] = cost;
}

}  // namespace

// host code only: the checks of the struct (before any HIP call; `who` is cmbpo_fakeenv_post_votes or the attach's name)
int cmbpo_internal_rule_votes_check_struct(const char *who, const cmbpo_rule_votes_t *rv) {
  CMBPO_REQUIRE(rv->done_members >= CMBPO_TERM_ELITE && rv->done_members <= CMBPO_TERM_MAJORITY,
                "%s: rule votes: done_members %d not in 0..2 (CMBPO_TERM_ELITE / _ANY / _MAJORITY; CMBPO_VOTE_MEAN is for the cost only)",
                who, rv->done_members);
  CMBPO_REQUIRE(rv->cost_members >= CMBPO_TERM_ELITE && rv->cost_members <= CMBPO_VOTE_MEAN,
                "%s: rule votes: cost_members %d not in 0..3 (CMBPO_TERM_ELITE / _ANY / _MAJORITY / CMBPO_VOTE_MEAN)", who,
                rv->cost_members);
  return CMBPO_OK;
}

int cmbpo_internal_rule_votes_check(const char *who, const FakeenvPostCall &c) {
  const cmbpo_rule_votes_t *rv = c.rv;
  if (int rc = cmbpo_internal_rule_votes_check_struct(who, rv)) return rc;
  CMBPO_REQUIRE(c.ensemble <= 8, "%s: rule votes: ensemble %d above 8 (the votes of a row live in a byte mask)", who, c.ensemble);
  if (c.task & CMBPO_TASK_LEARNED_COST) {
    CMBPO_REQUIRE(rv->cost_members == CMBPO_TERM_ELITE,
                  "%s: rule votes: cost_members %d with CMBPO_TASK_LEARNED_COST (the static cost rule is skipped, there is nothing to vote "
                  "on; the learned cost has cmbpo_fakeenv_post_disagreement), task 0x%x", who, rv->cost_members, c.task);
    CMBPO_REQUIRE(rv->cost_votes == nullptr,
                  "%s: rule votes: cost_votes given with CMBPO_TASK_LEARNED_COST (the static cost rule is skipped, there is nothing to "
                  "count), task 0x%x", who, c.task);
  }
  if (c.th != nullptr)
    CMBPO_REQUIRE(c.th->term_pred != nullptr && c.th->term_votes != nullptr,
                  "%s: rule votes with a termination head need th->term_pred and th->term_votes (the vote kernel recovers learned_done "
                  "from them)", who);
  return CMBPO_OK;
}

int cmbpo_internal_rule_votes_launch(const FakeenvPostCall &c, int task, int out_dim, const cmbpo_task_rules_t *rules,
                                     const cmbpo_rule_derived_table_t *der, void *stream) {
  const cmbpo_rule_votes_t *rv = c.rv;
  VotesArgs a{};
  a.task = task; a.ensemble = c.ensemble; a.obs_dim = c.obs_dim; a.act_dim = c.act_dim; a.out_dim = out_dim;
  a.rules_on = rules != nullptr ? 1 : 0;
  a.learned_cost = (c.task & CMBPO_TASK_LEARNED_COST) ? 1 : 0;
  a.dis_on = c.dis_on ? 1 : 0;
  a.mean = c.mean; a.var = c.var; a.ld_rows = c.ld_rows; a.obs = c.obs; a.act = c.act; a.xi = c.xi;
  a.elite = c.elite; a.row_idx = c.row_idx; a.n_rows_dev = c.n_rows_dev; a.n_rows = c.n_rows;
  a.term = c.term; a.cost = c.cost; a.cost_var = c.dis_on ? c.dis.cost_var : nullptr; a.kappa_cost = c.dis_on ? c.dis.kappa_cost : 0.0f;
  if (c.th != nullptr) {
    a.th_on = 1; a.th_members = c.th->members; a.threshold = c.th->threshold;
    a.term_pred = c.th->term_pred; a.term_votes = c.th->term_votes; a.term_thr = c.term_thr;
  }
  a.done_members = rv->done_members; a.cost_members = rv->cost_members;
  a.done_votes = rv->done_votes; a.cost_votes = rv->cost_votes;
  if (rules != nullptr) a.rules = *rules;
  if (der != nullptr) a.der = *der;
  // rows per workgroup: the largest power of two whose image [rows][E][obs_dim | 1] fits the budget (1 row at the widest
  // observation the post step takes: 8 x 513 floats = 16 KB)
  const size_t per_row = (size_t)c.ensemble * (size_t)(c.obs_dim | 1) * sizeof(float) + sizeof(int);
  int rows = kRowsMax;
  while (rows > 1 && rows * per_row > kLdsBudget) rows >>= 1;
  CMBPO_REQUIRE(rows * per_row <= 64 * 1024, "cmbpo_fakeenv_post_votes: obs_dim %d too wide for the vote kernel's image", c.obs_dim);
  a.rows_wg = rows;
  hipLaunchKernelGGL(rule_votes_kernel, dim3(cmbpo_ceil_div(c.n_rows, rows)), dim3(kThreads), rows * per_row, (hipStream_t)stream, a);
  CMBPO_HIP_CHECK(hipGetLastError());
  return CMBPO_OK;
}
