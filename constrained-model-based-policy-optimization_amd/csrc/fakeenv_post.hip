// FakeEnv.step after the ensemble forward: uncertainty measures, elite pick,
// delta add, static termination / cost rules.  HBM-bound: reads the
// (E, B, out) mean / var once, writes O(obs) floats per branch.
//
// Follows, line for line in arithmetic order:
//   models/fake_env.py:104-151   (std, ep_var, dkl path, elite gather, delta, statics, reward)
//   models/pens/utils.py:15-57   (gaussian_kl_np, average_dkl: all E*E ordered pairs, clip [0, 1e10])
//   models/statics.py:3-53       (no_done, hcs_cost_f, antsafe_term_fn, antsafe_c_fn incl. the
//                                 `a*b*c*z_rot >= -0.7` precedence quirk)
// and, for a registered rule id (csrc/task_rules.hip), the user's clause table in place of the three built-in rule sets.
#include "common.h"
#include "fakeenv_post_internal.h"

#include <math.h>

#include <type_traits>

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kThreads = 256;
constexpr int kRows = 8;     // branches per workgroup
constexpr int kEMaxRt = 8;   // ensemble members held in registers (largest ensemble)
constexpr int kEMax = kEMaxRt;

struct PostArgs {
  int task, ensemble, obs_dim, act_dim, out_dim;
  int learned_cost;   // 1: cost = column obs_dim + 1 of the elite member (fake_env.py:139-143), the task's cost rule is skipped
  const float *mean, *var;
  int ld_rows;
  const float *obs, *act;
  const int32_t *elite, *row_idx, *n_rows_dev;
  int n_rows;
  float *next_obs, *rew;
  uint8_t *term;
  float *cost, *dkl_path, *ep_var_mean, *ep_var;
};

// RULES: the launch of a registered rule id carries its clause table behind the arguments, by value (528 bytes, uniform: scalar
// loads from the kernel-argument segment) -- instances of their own, so the built-in tasks' kernels are what they were
struct PostArgsRules : PostArgs {
  cmbpo_task_rules_t rules;     // columns resolved on the host: col0 absolute, n_cols a count, all inside the source's width
};
// NOISE: stochastic transitions (fake_env.py:103-108 with a random factor: mean + std * xi) -- the draws' pointer exists only
// in the argument types of the NOISE instances, the same device: a launch without draws runs the kernels it always ran
struct PostArgsNoise : PostArgs {
  const float *xi;              // [., obs_dim] N(0, 1) draws, slot indexed like obs; one draw per (row, dim) for all members
};
struct PostArgsRulesNoise : PostArgsRules {
  const float *xi;
};
// RULES == 2: a rule id with derived quantities (include/cmbpo_hip.h, cmbpo_rule_derived_table_t) -- their table travels behind the
// clause table, by value again (656 bytes), and again only in the argument types of instances of their own: a built-in task and a
// registered table without derived quantities launch the instances, with the argument blocks, they always launched
struct PostArgsDerived : PostArgsRules {
  cmbpo_rule_derived_table_t der;   // term columns resolved on the host: absolute, inside the source's width
};
struct PostArgsDerivedNoise : PostArgsDerived {
  const float *xi;
};
template <int RULES, bool NOISE>
using PostArgsBase =
    std::conditional_t<NOISE, std::conditional_t<RULES == 2, PostArgsDerivedNoise, std::conditional_t<RULES == 1, PostArgsRulesNoise, PostArgsNoise>>,
                       std::conditional_t<RULES == 2, PostArgsDerived, std::conditional_t<RULES == 1, PostArgsRules, PostArgs>>>;
// DIS: ensemble disagreement on the reward and the learned-cost column (np.var over ALL members, like ens_ep_var on the
// observation columns) and the pessimistic reward / cost made from it -- again fields that exist only in the argument types
// of instances of their own: a launch without the feature runs the kernels it always ran, with the arguments it always had
template <int RULES, bool NOISE>
struct PostArgsDis : PostArgsBase<RULES, NOISE> {
  float kappa_rew, kappa_cost;    // >= 0, finite; 0: the elite member's value goes out untouched
  float *rew_var, *cost_var;      // [.] slot indexed like rew / cost
};
template <int RULES, bool NOISE, bool DIS = false>
using PostArgsT = std::conditional_t<DIS, PostArgsDis<RULES, NOISE>, PostArgsBase<RULES, NOISE>>;
// TERM: the learned termination head (include/cmbpo_hip.h, cmbpo_term_head_t) -- the model's LAST column, out_dim - 1, read by
// the row's eight lanes in the tail; once more fields that exist only in the argument types of instances of their own
template <int RULES, bool NOISE, bool DIS>
struct PostArgsTerm : PostArgsT<RULES, NOISE, DIS> {
  float threshold;                // finite
  int members;                    // CMBPO_TERM_ELITE / _ANY / _MAJORITY
  float *term_pred;               // [.] slot indexed like term, or NULL
  uint8_t *term_votes;            // [.] or NULL
};
// DRAW: sampled terminations (include/cmbpo_hip.h, cmbpo_fakeenv_post_term_draws) -- a threshold per row in place of the head's one
// scalar; it exists only together with TERM, and its pointer only in the argument types of instances of their own
template <int RULES, bool NOISE, bool DIS>
struct PostArgsDraw : PostArgsTerm<RULES, NOISE, DIS> {
  const float *term_thr;          // [.] slot indexed like term, the column's own units; any value (a NaN never hits)
};
template <int RULES, bool NOISE, bool DIS = false, bool TERM = false, bool DRAW = false>
using PostArgsX = std::conditional_t<DRAW, PostArgsDraw<RULES, NOISE, DIS>,
                                     std::conditional_t<TERM, PostArgsTerm<RULES, NOISE, DIS>, PostArgsT<RULES, NOISE, DIS>>>;
// COST: the logistic learned-cost head (include/cmbpo_hip.h, cmbpo_cost_head_t, kind 1) -- column obs_dim + 1 is a logit and the
// cost its probability; the same pattern: fields of an argument type of their own, selecting instances of their own.  They are
// launched with CMBPO_TASK_LEARNED_COST only (checked on the host), so `learned_cost` is not read in their COST parts.
template <int RULES, bool NOISE, bool DIS, bool TERM, bool DRAW = false>
struct PostArgsCost : PostArgsX<RULES, NOISE, DIS, TERM, DRAW> {
  float logit_shift;              // finite; 0: the logit goes into sigma32 bit for bit
  float *cost_logit;              // [.] slot indexed like cost: the elite's raw logit, or NULL
};
template <int RULES, bool NOISE, bool DIS = false, bool TERM = false, bool COST = false, bool DRAW = false>
using PostArgsY = std::conditional_t<COST, PostArgsCost<RULES, NOISE, DIS, TERM, DRAW>, PostArgsX<RULES, NOISE, DIS, TERM, DRAW>>;

// np.clip(x, lo, hi): comparisons are false for a NaN, which therefore passes through (fminf / fmaxf would drop it)
__device__ __forceinline__ float clip_np(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// The ONE logistic function of the cost head: every instance and every lane computes a member's probability with it, so the
// probability of a logit has the same bits wherever it is computed.  float32, no contraction (the file is built with
// -ffp-contract=off; the division is the correctly rounded one); +inf -> 1, -inf -> 0, NaN -> NaN (`zs >= 0` is false for it).
__device__ __forceinline__ float sigma32(float zs) {
  if (zs >= 0.0f) return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-zs)));
  const float e = expf(zs);
  return __fdiv_rn(e, __fadd_rn(1.0f, e));
}
// zs = fl32(z - logit_shift); a shift of 0 executes no subtraction (uniform over the launch)
__device__ __forceinline__ float cost_prob(float z, float logit_shift) {
  return sigma32(logit_shift != 0.0f ? __fsub_rn(z, logit_shift) : z);
}

// EC: the ensemble size at compile time (0: read it at run time) -- with a run-time size the member loops are unrolled to
// kEMax and masked: 56 pair terms computed and selected for the 42 that exist, a third more instructions
#define POST_WAVES 5      // waves per SIMD the register allocation aims at (swept 4 / 5 / 6 / 8: 57.7 / 51.1 / 51.3 / 77.4 us at 100 k rows)
template <int EC, int RULES = 0, bool NOISE = false, bool DIS = false, bool TERM = false, bool COST = false, bool DRAW = false>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(POST_WAVES, POST_WAVES))) void fakeenv_post_kernel(const PostArgsY<RULES, NOISE, DIS, TERM, COST, DRAW> p) {
  static_assert(TERM || !DRAW, "DRAW exists only together with TERM");
  extern __shared__ float sm[];
  const int D = p.obs_dim;
  float *s_dkl = sm;                  // [kRows][D]
  float *s_var = s_dkl + kRows * D;   // [kRows][D]
  float *s_next = s_var + kRows * D;  // [kRows][D]
  int *s_row = reinterpret_cast<int *>(s_next + kRows * D);  // [kRows]

  const int tid = threadIdx.x;
  const int n_rows = p.n_rows_dev ? *p.n_rows_dev : p.n_rows;
  const int row0 = blockIdx.x * kRows;
  if (row0 >= n_rows) return;
  if (tid < kRows) {
    const int r = row0 + tid;
    s_row[tid] = (r < n_rows) ? (p.row_idx ? p.row_idx[r] : r) : -1;
  }
  __syncthreads();

  const int E = EC > 0 ? EC : p.ensemble;
  constexpr int kEMax = EC > 0 ? EC : ::kEMaxRt;
  const size_t mstride = (size_t)p.ld_rows * p.out_dim;
  for (int i = tid; i < kRows * D; i += kThreads) {
    const int b = i / D, d = i - b * D;
    const int r = s_row[b];
    if (r < 0) continue;
    float mu[kEMax], ls[kEMax], vr[kEMax];
    bool fast = EC > 0;     // every member's (mean, var) of this (row, dim) finite and far from the float range's ends
    const size_t base = (size_t)r * p.out_dim + d;
    // every load of the thread first -- 2 E + 2 requests in flight: written member by member next to their use, the loads of
    // a member waited for its own memory round trip (the out-of-range branch below keeps hipcc from hoisting them), seven
    // round trips in a row per workgroup
    float v0s[kEMax];
#pragma unroll
    for (int e = 0; e < kEMax; ++e) {
      mu[e] = p.mean[(e < E ? e : 0) * mstride + base];
      v0s[e] = p.var[(e < E ? e : 0) * mstride + base];
    }
    const int me = p.elite[r];
    float mean_me = p.mean[me * mstride + base];
    const float obs_rd = p.obs[(size_t)r * D + d];
    if constexpr (NOISE) {
      // fake_env.py:104-106 with a random factor: every member's mean moves by fl32(fl32(sqrt(var)) * xi), two roundings (the
      // reference's `+ pred_std` is xi == 1), BEFORE the uncertainty measures (:112-113 run on the shifted means) and the fast-path
      // test; the variances stay what they are.  sqrtf, not __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS the latter is
      // v_sqrt_f32 (1 ulp), and np.sqrt rounds correctly.
      const float xi = p.xi[(size_t)r * D + d], var_me = p.var[me * mstride + base];
#pragma unroll
      for (int e = 0; e < kEMax; ++e) mu[e] = __fadd_rn(mu[e], __fmul_rn(sqrtf(v0s[e]), xi));
      mean_me = __fadd_rn(mean_me, __fmul_rn(sqrtf(var_me), xi));
    }
#pragma unroll
    for (int e = 0; e < kEMax; ++e) {
      if (e < E) {
        // fake_env.py:104 std = sqrt(var); average_dkl: log_std = clip(log(std), -100, 1e8); gaussian_kl_np:
        // var = exp(2 log_std).  Inside the clip range that is log_std = 0.5 log(var) and exp(2 log_std) = var up to
        // rounding (the KL is compared at 1e-4, not bit for bit): one log instead of sqrt + log + exp per member.
        const float v0 = v0s[e];
        float l = __fmul_rn(0.5f, __logf(v0));              // (v_log_f32: the KL is compared at 1e-4; libm's logf is ~25 instructions)
        const bool inside = l >= -100.0f && l <= 1e8f;       // false for NaN as well
        if (!inside) l = clip_np(logf(sqrtf(v0)), -100.0f, 1e8f);   // np.clip: a NaN stays a NaN
        ls[e] = l;
        vr[e] = inside ? v0 : expf(__fmul_rn(2.0f, l));
        fast = fast && inside && fabsf(mu[e]) < 1e18f && v0 < 1e30f;      // (false for a NaN mean as well)
      }
    }
    // ensemble epistemic variance over ALL members (np.var, axis 0), fake_env.py:112
    float s = 0.0f;
#pragma unroll
    for (int e = 0; e < kEMax; ++e)
      if (e < E) s = __fadd_rn(s, mu[e]);
    const float mbar = s / (float)E;
    float sq = 0.0f;
#pragma unroll
    for (int e = 0; e < kEMax; ++e)
      if (e < E) {
        const float dlt = __fsub_rn(mu[e], mbar);
        sq = __fadd_rn(sq, __fmul_rn(dlt, dlt));
      }
    s_var[i] = sq / (float)E;
    float acc;
    if (fast) {
      // The common case, on packed float32 arithmetic: two ordered pairs (a, c), (a, c + 1) per instruction, the pair term as
      //   clip(fma(fma(dm, dm, var_a), 0.5 / (var_c + 1e-10), log_std_c - 0.5) - log_std_a, 0, 1e10)
      // (the reference's sum, regrouped: the KL is compared at 1e-4, and its own pair term carries a cancellation error of a few
      // 1e-7 in `0.5 (q - 1) + log_std_c - log_std_a`), the clip as one v_med3 -- with every operand finite no NaN can arise, so
      // nothing has to pass through it -- and the a == c term left out: it is <= 0 before the clip (see below).  3.5 vector
      // instructions per ordered pair instead of 11.
      constexpr int EH = (kEMax + 1) / 2;
      f32x2 mu2[EH], hr2[EH], k2[EH];
#pragma unroll
      for (int h = 0; h < EH; ++h)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int c = 2 * h + u;
          const bool real = c < kEMax;
          mu2[h][u] = real ? mu[real ? c : 0] : 0.0f;
          hr2[h][u] = real ? 0.5f * __builtin_amdgcn_rcpf(vr[real ? c : 0] + 1e-10f) : 0.0f;
          k2[h][u] = real ? ls[real ? c : 0] - 0.5f : -1.0f;
        }
      f32x2 acc2 = {0.0f, 0.0f};
#pragma unroll
      for (int a = 0; a < kEMax; ++a) {
        const f32x2 nmu = {-mu[a], -mu[a]}, va = {vr[a], vr[a]}, nls = {-ls[a], -ls[a]};
#pragma unroll
        for (int h = 0; h < EH; ++h) {
          const f32x2 dm = mu2[h] + nmu;
          const f32x2 num = __builtin_elementwise_fma(dm, dm, va);
          const f32x2 pre = __builtin_elementwise_fma(num, hr2[h], k2[h]) + nls;
          f32x2 cl;
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int c = 2 * h + u;
            cl[u] = (c < kEMax && c != a) ? __builtin_amdgcn_fmed3f(pre[u], 0.0f, 1e10f) : 0.0f;
          }
          acc2 += cl;
        }
      }
      acc = acc2[0] + acc2[1];
    } else {
      asm volatile("" ::: "memory");      // a real branch: the code below has no side effects, hipcc would run BOTH sides and select
      // average KL over all ordered pairs (i outer, j inner), models/pens/utils.py:49-56.  Two exact savings: an a == c term
      // is 0.5 (v / (v + 1e-10) - 1) <= 0 for finite v and mu, which np.clip turns into +0 -- adding +0 to the
      // non-negative running sum changes nothing, so those are skipped (for a member whose variance is inf / NaN or whose
      // mean is non-finite the term is NaN, np.clip keeps it, and the reference's KL of that branch is NaN: added below); and
      // (mu_c - mu_a)^2 == (mu_a - mu_c)^2 bit for bit, so the squared difference of a pair is computed once.
      float dm2[kEMax][kEMax];
  #pragma unroll
      for (int a = 0; a < kEMax; ++a)
  #pragma unroll
        for (int c = a + 1; c < kEMax; ++c)
          if (c < E) {
            const float dm = __fsub_rn(mu[c], mu[a]);
            dm2[a][c] = __fmul_rn(dm, dm);
          }
      // 1 / (var_c + 1e-10) once per member instead of a division per ordered pair (E - 1 times fewer divisions; the
      // quotient differs from the reference's by an ulp at most)
      float rden[kEMax];
  #pragma unroll
      for (int c = 0; c < kEMax; ++c)
        if (c < E) rden[c] = __builtin_amdgcn_rcpf(__fadd_rn(vr[c], 1e-10f));   // v_rcp_f32: 1 ulp
      acc = 0.0f;
  #pragma unroll
      for (int a = 0; a < kEMax; ++a) {
        if (a < E) {
  #pragma unroll
          for (int c = 0; c < kEMax; ++c) {
            if (c < E && c != a) {
              const float d2 = (a < c) ? dm2[a][c] : dm2[c][a];
              const float num = __fadd_rn(d2, vr[a]);
              const float q = __fmul_rn(num, rden[c]);
              float pre = __fmul_rn(0.5f, __fsub_rn(q, 1.0f));
              pre = __fsub_rn(__fadd_rn(pre, ls[c]), ls[a]);
              pre = clip_np(pre, 0.0f, 1e10f);
              acc = __fadd_rn(acc, pre);
            }
          }
          // the a == a term of a member with a non-finite variance or mean: (0 or NaN + v) / (v + 1e-10) is inf / inf or NaN
          if (!isfinite(vr[a]) || !isfinite(mu[a])) acc = __fadd_rn(acc, __builtin_nanf(""));
        }
      }
    }
    s_dkl[i] = acc / ((float)(E * (E - 1)) + 1e-10f);
    // elite pick + delta add, fake_env.py:121-131
    const float nx = __fadd_rn(mean_me, obs_rd);
    s_next[i] = nx;
    p.next_obs[(size_t)r * D + d] = nx;
    if (p.ep_var) p.ep_var[(size_t)r * D + d] = s_var[i];
  }
  __syncthreads();

  // Eight lanes per row: numpy's float32 pairwise sum for n < 128 (the contiguous-axis np.mean / np.sum path) IS eight strided
  // partial sums -- lane k carries r[k] -- combined in a fixed tree, then the tail added in order; done here operation for
  // operation, so the row means reproduce numpy's bit for bit while the dependent chain of D additions that one thread per row
  // walked (twice, with 248 threads of the workgroup waiting) becomes D / 8 + 3.
  if (tid < 8 * kRows) {
    const int rw = tid >> 3, k = tid & 7;
    const int r = s_row[rw];
    const float *nx = s_next + rw * D;
    // DIS: lane k of the row owns member k -- its reward (and learned-cost) mean and the row's elite index are requested
    // here, ahead of the row sums that hide the round trip; one lane walking 2 E dependent loads behind everything else
    // would add them to the end of the workgroup's life.  Rows past the end and lanes past E load nothing.
    [[maybe_unused]] float xr = 0.0f, xc = 0.0f;
    [[maybe_unused]] int me_k = 0;
    if constexpr (DIS) {
      if (r >= 0) {
        me_k = p.elite[r];
        if (k < E) {
          const size_t o = k * mstride + (size_t)r * p.out_dim + D;
          xr = p.mean[o];
          if constexpr (COST) xc = p.mean[o + 1];
          else if (p.learned_cost) xc = p.mean[o + 1];
        }
      }
    }
    // TERM: lane k of the row owns member k's value of the termination column (the model's last), requested here like the DIS
    // loads; rows past the end and lanes past E load nothing
    [[maybe_unused]] float xt = 0.0f;
    [[maybe_unused]] int me_t = 0;
    if constexpr (TERM) {
      if (r >= 0) {
        if constexpr (DIS) me_t = me_k;
        else me_t = p.elite[r];
        if (k < E) xt = p.mean[k * mstride + (size_t)r * p.out_dim + (p.out_dim - 1)];
      }
    }
    // DRAW: the row's own threshold, one address for the row's eight lanes (one request, broadcast), requested with the column
    [[maybe_unused]] float thr_r = 0.0f;
    if constexpr (DRAW) {
      if (r >= 0) thr_r = p.term_thr[r];
    }
    // RULES == 2: lane k of the row owns derived quantity k.  Its table entry is picked out of the (uniform, scalar-loaded) table
    // by a chain of selects -- indexing the argument block by the lane would put it into scratch or behind a memory round trip of
    // its own -- and its operands are requested here, like the DIS / TERM loads ahead of the row sums: next_obs from the s_next
    // image, obs / act from global memory.  Rows past the end read nothing from global memory, lanes past n_derived nothing at all.
    [[maybe_unused]] cmbpo_rule_derived_t dq{};
    [[maybe_unused]] float dx[CMBPO_RULE_MAX_TERMS] = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (RULES == 2) {
#pragma unroll
      for (int j = 0; j < CMBPO_RULE_MAX_DERIVED; ++j)
        if (j < p.der.n_derived && k == j) dq = p.der.derived[j];
#pragma unroll
      for (int t = 0; t < CMBPO_RULE_MAX_TERMS; ++t)
        if (t < dq.n_terms) {
          const int col = dq.term[t].col;
          if (dq.term[t].src == CMBPO_RULE_SRC_NEXT_OBS) dx[t] = nx[col];
          else if (r >= 0) dx[t] = dq.term[t].src == CMBPO_RULE_SRC_OBS ? p.obs[(size_t)r * D + col] : p.act[(size_t)r * p.act_dim + col];
        }
    }
    auto row_sum = [&](const float *a) {
      float res;
      if (D < 8) {
        res = 0.0f;
        for (int i = 0; i < D; ++i) res = __fadd_rn(res, a[i]);
        return res;
      }
      float rk = a[k];
      const int full = D - (D % 8);
      for (int i = 8; i < full; i += 8) rk = __fadd_rn(rk, a[i + k]);
      rk = __fadd_rn(rk, __shfl_down(rk, 1, 64));      // lanes 0, 2, 4, 6: r0 + r1, r2 + r3, r4 + r5, r6 + r7
      rk = __fadd_rn(rk, __shfl_down(rk, 2, 64));      // lanes 0, 4
      rk = __fadd_rn(rk, __shfl_down(rk, 4, 64));      // lane 0
      for (int i = full; i < D; ++i) rk = __fadd_rn(rk, a[i]);
      return rk;
    };
    const float sd = row_sum(s_dkl + rw * D), sv = row_sum(s_var + rw * D);
    bool fin = true;
    for (int d = k; d < D; d += 8) fin = fin && isfinite(nx[d]);
    const unsigned long long okm = __ballot(fin);
    fin = ((okm >> (8 * rw)) & 0xffull) == 0xffull;
    // The clause table (include/cmbpo_hip.h): a clause's columns go over the row's eight lanes like `fin`, one ballot per
    // clause; the loop and every field of a clause are uniform over the launch.  All 64 lanes are still here (rows past the
    // end read their stale LDS image and nothing from global memory; their result is dropped below).
    [[maybe_unused]] bool rule_done = false, rule_obj = false;
    // RULES == 2: g = bias; per term t = fl32(x - c), squared with pow 2, g = fl32(g + fl32(w * t)) -- single roundings in the
    // header's order (the file is built without contraction); a lane past n_derived holds +0, which no clause can address
    [[maybe_unused]] float g = 0.0f;
    if constexpr (RULES == 2) {
      g = dq.bias;
#pragma unroll
      for (int t = 0; t < CMBPO_RULE_MAX_TERMS; ++t)
        if (t < dq.n_terms) {
          float tt = __fsub_rn(dx[t], dq.term[t].c);
          if (dq.term[t].pow == 2) tt = __fmul_rn(tt, tt);
          g = __fadd_rn(g, __fmul_rn(dq.term[t].w, tt));
        }
    }
    if constexpr (RULES != 0) {
      for (int c = 0; c < p.rules.n_clauses; ++c) {
        const cmbpo_rule_clause_t &cl = p.rules.clause[c];
        const bool any = (cl.flags & CMBPO_RULE_ANY) != 0;
        bool all_k = true, any_k = false;
        // a derived clause: lane k of the row tests quantity col0 + k, fetched from the lane that owns it -- here, where all 64
        // lanes are converged (the column loop below is not), at most 8 quantities: one pass of that loop
        [[maybe_unused]] float xg = 0.0f;
        if constexpr (RULES == 2)
          if (cl.src == CMBPO_RULE_SRC_DERIVED) xg = __shfl(g, 8 * rw + ((cl.col0 + k) & 7), 64);
        for (int d = cl.col0 + k; d < cl.col0 + cl.n_cols; d += 8) {
          float x = 0.0f;
          if (cl.src == CMBPO_RULE_SRC_NEXT_OBS) x = nx[d];
          else if (RULES == 2 && cl.src == CMBPO_RULE_SRC_DERIVED) x = xg;
          else if (r >= 0) x = cl.src == CMBPO_RULE_SRC_OBS ? p.obs[(size_t)r * D + d] : p.act[(size_t)r * p.act_dim + d];
          float f = __fmul_rn(x, cl.scale);
          if (cl.flags & CMBPO_RULE_ABS) f = fabsf(f);
          // positive tests: false for a NaN, like NumPy's comparisons
          const bool lo_ok = (cl.flags & CMBPO_RULE_LO_STRICT) ? f > cl.lo : f >= cl.lo;
          const bool hi_ok = (cl.flags & CMBPO_RULE_HI_STRICT) ? f < cl.hi : f <= cl.hi;
          all_k = all_k && lo_ok && hi_ok;
          any_k = any_k || (lo_ok && hi_ok);
        }
        const unsigned lanes = (unsigned)(__ballot(any ? any_k : all_k) >> (8 * rw)) & 0xffu;
        const bool holds = any ? lanes != 0u : lanes == 0xffu;
        if (cl.role == CMBPO_RULE_HEALTHY) rule_done = rule_done || !holds;
        else if (cl.role == CMBPO_RULE_FATAL) rule_done = rule_done || holds;
        else rule_obj = rule_obj || holds;
      }
    }
    // DIS: np.var over the members (axis 0) in the order of the observation columns above -- s = ((x0 + x1) + x2) + ...,
    // m = s / E, q = sum (x_e - m)^2 in member order, var = q / E -- with the row's lane 0 reading member e from lane e.  All
    // 64 lanes are still here; the elite's own values come from the same registers (the bits the plain entry loads).
    [[maybe_unused]] float rew_var = 0.0f, cost_var = 0.0f, rew_me = 0.0f, cost_me = 0.0f;
    if constexpr (DIS) {
      const int l0 = 8 * rw;
      auto member_var = [&](float x, float *x_me) {
        float xe[kEMax];
#pragma unroll
        for (int e = 0; e < kEMax; ++e) xe[e] = __shfl(x, l0 + e, 64);
        *x_me = __shfl(x, l0 + (me_k & 7), 64);
        float s = 0.0f;
#pragma unroll
        for (int e = 0; e < kEMax; ++e)
          if (e < E) s = __fadd_rn(s, xe[e]);
        const float mbar = s / (float)E;
        float sq = 0.0f;
#pragma unroll
        for (int e = 0; e < kEMax; ++e)
          if (e < E) {
            const float dlt = __fsub_rn(xe[e], mbar);
            sq = __fadd_rn(sq, __fmul_rn(dlt, dlt));
          }
        return sq / (float)E;
      };
      rew_var = member_var(xr, &rew_me);
      if constexpr (COST) {
        // lane k holds member k's logit: the elite's goes out raw from the lane that loaded it, then every lane turns its own
        // into the probability -- E exponentials side by side -- and the variance is taken on the probabilities
        if (p.cost_logit != nullptr && r >= 0 && k == (me_k & 7)) p.cost_logit[r] = xc;
        xc = cost_prob(xc, p.logit_shift);
        cost_var = member_var(xc, &cost_me);
      } else if (p.learned_cost) cost_var = member_var(xc, &cost_me);     // (uniform over the launch; a static cost rule has no spread: +0)
    }
    // TERM: hit_e = x_e > threshold (DRAW: the header's rule, the row's own threshold), written positively (a NaN never hits); one ballot gives the row's member mask in the row's
    // byte -- the elite's bit is me & 7, the votes are a popcount.  All 64 lanes are still here.  The elite's own value goes out
    // from the lane that loaded it.
    [[maybe_unused]] unsigned term_mask = 0u;
    if constexpr (TERM) {
      bool hit;
      if constexpr (DRAW) hit = r >= 0 && k < E && xt > thr_r;
      else hit = r >= 0 && k < E && xt > p.threshold;
      term_mask = (unsigned)(__ballot(hit) >> (8 * rw)) & 0xffu;
      if (p.term_pred != nullptr && r >= 0 && k == (me_t & 7)) p.term_pred[r] = xt;
    }
    if (r < 0 || k != 0) return;
    p.dkl_path[r] = sd / (float)D;      // fake_env.py:113
    p.ep_var_mean[r] = sv / (float)D;   // model_sampler.py:322
    int me;
    if constexpr (DIS) me = me_k;
    else me = p.elite[r];
    if constexpr (DIS) {
      // r - kappa * sigma only where kappa > 0 (uniform over the launch): with kappa == 0 the elite's value goes out bit for
      // bit whatever the other members hold, a NaN included.  sqrtf: correctly rounded, as in the NOISE path.
      p.rew_var[r] = rew_var;
      p.cost_var[r] = cost_var;
      p.rew[r] = p.kappa_rew > 0.0f ? __fsub_rn(rew_me, __fmul_rn(p.kappa_rew, sqrtf(rew_var))) : rew_me;
    } else {
      p.rew[r] = p.mean[me * mstride + (size_t)r * p.out_dim + D];    // fake_env.py:148-151
    }
    uint8_t done = 0;
    float cost = 0.0f;
    if constexpr (RULES != 0) {
      done = ((p.rules.require_finite && !fin) || rule_done) ? 1 : 0;
      const float obj = rule_obj ? 1.0f : 0.0f;
      cost = p.rules.cost_on_term ? fminf(__fadd_rn((float)done, obj), 1.0f) : obj;      // statics.py:51-52
    } else if (p.task == CMBPO_TASK_ANTSAFE) {
      // statics.py:17-53
      const float z = nx[0];
      const float q1 = nx[2], q2 = nx[3];
      const float zrot = __fsub_rn(1.0f, __fmul_rn(2.0f, __fadd_rn(__fmul_rn(q1, q1), __fmul_rn(q2, q2))));
      const float gate = (fin && z >= 0.2f && z <= 1.0f) ? 1.0f : 0.0f;
      const bool notdone = __fmul_rn(gate, zrot) >= -0.7f;
      done = notdone ? 0 : 1;
      const float obj = (fabsf(nx[D - 1]) > 3.2f) ? 1.0f : 0.0f;
      cost = fminf(fmaxf((float)done + obj, 0.0f), 1.0f);
    } else if (p.task == CMBPO_TASK_HCS) {
      // statics.py:10-15
      const float xdist = __fmul_rn(nx[D - 1], 10.0f);
      cost = (fabsf(xdist) < 2.0f) ? 1.0f : 0.0f;
    }
    // learned cost head (fake_env.py:139-143, predicts_cost=True): the elite member's mean of the last column, stored as it is;
    // the termination rule above still applies (TERMS_BY_TASK does not depend on predicts_cost).  A branch uniform over the
    // launch, taken by one lane per row: as a template parameter it would double the instances for one load.
    // COST: the column is a logit and the cost its probability; the pessimistic cost is clipped at 1 (c > 1 ? 1 : c: a NaN passes).
    // Without DIS only the elite's logit is read, by this lane.
    if constexpr (COST && DIS) {
      cost = cost_me;
      if (p.kappa_cost > 0.0f) {
        const float c = __fadd_rn(cost_me, __fmul_rn(p.kappa_cost, sqrtf(cost_var)));
        cost = c > 1.0f ? 1.0f : c;
      }
    } else if constexpr (COST) {
      const float z = p.mean[me * mstride + (size_t)r * p.out_dim + D + 1];
      if (p.cost_logit != nullptr) p.cost_logit[r] = z;
      cost = cost_prob(z, p.logit_shift);
    } else if constexpr (DIS) {
      if (p.learned_cost) cost = p.kappa_cost > 0.0f ? __fadd_rn(cost_me, __fmul_rn(p.kappa_cost, sqrtf(cost_var))) : cost_me;
    } else {
      if (p.learned_cost) cost = p.mean[me * mstride + (size_t)r * p.out_dim + D + 1];
    }
    // TERM: term = rule_done || learned_done; the cost above has used the rule's own done.  `members` is uniform over the launch.
    if constexpr (TERM) {
      const int votes = __popc(term_mask);
      const bool learned = p.members == CMBPO_TERM_ELITE ? ((term_mask >> (me_t & 7)) & 1u) != 0u
                           : p.members == CMBPO_TERM_ANY ? votes > 0 : 2 * votes > E;
      if (learned) done = 1;
      if (p.term_votes != nullptr) p.term_votes[r] = (uint8_t)votes;
    }
    p.term[r] = done;
    p.cost[r] = cost;
  }
}

// one launch of the instance for (ensemble size, RULES, NOISE, DIS, TERM, COST, DRAW)
template <int RULES, bool NOISE, bool DIS = false, bool TERM = false, bool COST = false, bool DRAW = false>
void launch_post(int ensemble, dim3 grid, size_t lds, hipStream_t stream, const PostArgsY<RULES, NOISE, DIS, TERM, COST, DRAW> &a) {
  if (ensemble == 7) hipLaunchKernelGGL((fakeenv_post_kernel<7, RULES, NOISE, DIS, TERM, COST, DRAW>), grid, dim3(kThreads), lds, stream, a);   // the shipped configs
  else if (ensemble == 5) hipLaunchKernelGGL((fakeenv_post_kernel<5, RULES, NOISE, DIS, TERM, COST, DRAW>), grid, dim3(kThreads), lds, stream, a);
  else hipLaunchKernelGGL((fakeenv_post_kernel<0, RULES, NOISE, DIS, TERM, COST, DRAW>), grid, dim3(kThreads), lds, stream, a);
}
// ... and the logistic cost head (ch == NULL: the instances without it, with the argument block they always had)
template <int RULES, bool NOISE, bool DIS, bool TERM, bool DRAW = false>
void launch_post_cost(int ensemble, dim3 grid, size_t lds, hipStream_t stream, const PostArgsX<RULES, NOISE, DIS, TERM, DRAW> &a,
                      const cmbpo_cost_head_t *ch) {
  if (ch == nullptr) return launch_post<RULES, NOISE, DIS, TERM, false, DRAW>(ensemble, grid, lds, stream, a);
  PostArgsCost<RULES, NOISE, DIS, TERM, DRAW> ac{};
  static_cast<PostArgsX<RULES, NOISE, DIS, TERM, DRAW> &>(ac) = a;
  ac.logit_shift = ch->logit_shift; ac.cost_logit = ch->cost_logit;
  launch_post<RULES, NOISE, DIS, TERM, true, DRAW>(ensemble, grid, lds, stream, ac);
}

// DisExtra (fakeenv_post_internal.h): what the disagreement adds to the arguments (NULL: the instances without the feature)
// ... and cmbpo_fakeenv_post_term (th == NULL: the instances without the head, with the argument block they always had)
// ... and cmbpo_fakeenv_post_term_draws (thr == NULL: the TERM instances without the draws, likewise)
template <int RULES, bool NOISE, bool DIS>
void launch_post_term(int ensemble, dim3 grid, size_t lds, hipStream_t stream, const PostArgsT<RULES, NOISE, DIS> &a,
                      const cmbpo_term_head_t *th, const float *thr, const cmbpo_cost_head_t *ch) {
  if (th == nullptr) return launch_post_cost<RULES, NOISE, DIS, false>(ensemble, grid, lds, stream, a, ch);
  PostArgsTerm<RULES, NOISE, DIS> at{};
  static_cast<PostArgsT<RULES, NOISE, DIS> &>(at) = a;
  at.threshold = th->threshold; at.members = th->members; at.term_pred = th->term_pred; at.term_votes = th->term_votes;
  if (thr == nullptr) return launch_post_cost<RULES, NOISE, DIS, true>(ensemble, grid, lds, stream, at, ch);
  PostArgsDraw<RULES, NOISE, DIS> aw{};
  static_cast<PostArgsTerm<RULES, NOISE, DIS> &>(aw) = at;
  aw.term_thr = thr;
  launch_post_cost<RULES, NOISE, DIS, true, true>(ensemble, grid, lds, stream, aw, ch);
}
template <int RULES, bool NOISE>
void launch_post_ext(int ensemble, dim3 grid, size_t lds, hipStream_t stream, const PostArgsBase<RULES, NOISE> &a, const DisExtra *dis,
                     const cmbpo_term_head_t *th, const float *thr, const cmbpo_cost_head_t *ch) {
  if (dis == nullptr) return launch_post_term<RULES, NOISE, false>(ensemble, grid, lds, stream, a, th, thr, ch);
  PostArgsDis<RULES, NOISE> ad{};
  static_cast<PostArgsBase<RULES, NOISE> &>(ad) = a;
  ad.kappa_rew = dis->kappa_rew; ad.kappa_cost = dis->kappa_cost; ad.rew_var = dis->rew_var; ad.cost_var = dis->cost_var;
  launch_post_term<RULES, NOISE, true>(ensemble, grid, lds, stream, ad, th, thr, ch);
}

}  // namespace

int cmbpo_internal_fakeenv_post(const FakeenvPostCall &c, void *stream) {
  const cmbpo_term_head_t *th = c.th;
  const DisExtra *dis = c.dis_on ? &c.dis : nullptr;
  // the naming rule (fakeenv_post_internal.h, DESIGN): the narrowest entry point that can express the call
  // (kind 0 is the magnitude reading: the instances without the head; `ch` below is the LOGISTIC head or NULL)
  const cmbpo_cost_head_t *ch = (c.ch != nullptr && c.ch->kind == 1) ? c.ch : nullptr;
  const char *who = c.rv ? "cmbpo_fakeenv_post_votes" : c.term_thr ? "cmbpo_fakeenv_post_term_draws" : c.ch ? "cmbpo_fakeenv_post_cost" : th ? "cmbpo_fakeenv_post_term" : dis ? "cmbpo_fakeenv_post_disagreement"
                    : c.xi ? "cmbpo_fakeenv_post_noise" : "cmbpo_fakeenv_post";
  const int obs_dim = c.obs_dim, act_dim = c.act_dim, ensemble = c.ensemble;
  const int learned_cost = (c.task & CMBPO_TASK_LEARNED_COST) ? 1 : 0;     // every other bit outside the rule id is an error
  const int task_arg = c.task, task = c.task & ~CMBPO_TASK_LEARNED_COST;
  const bool user = task >= CMBPO_TASK_USER_BASE && task < CMBPO_TASK_USER_BASE + CMBPO_TASK_USER_SLOTS;
  CMBPO_REQUIRE((task >= CMBPO_TASK_DEFAULT && task <= CMBPO_TASK_ANTSAFE) || user, "%s: bad task %d", who, task_arg);
  CMBPO_REQUIRE(ensemble >= 2 && ensemble <= kEMax, "%s: ensemble %d not in [2, %d]", who, ensemble, kEMax);
  CMBPO_REQUIRE(obs_dim >= 1 && obs_dim <= 512 && act_dim >= 0, "%s: bad dims", who);
  if (task == CMBPO_TASK_ANTSAFE)
    CMBPO_REQUIRE(obs_dim >= 5, "%s: AntSafe rules need obs_dim >= 5", who);
  if (th != nullptr) {
    // (isfinite is false for a NaN; kEMax is what the row's eight lanes hold -- checked above, named again for the head)
    CMBPO_REQUIRE(isfinite(th->threshold), "%s: termination head: threshold %g is not a finite number", who, (double)th->threshold);
    CMBPO_REQUIRE(th->members >= CMBPO_TERM_ELITE && th->members <= CMBPO_TERM_MAJORITY,
                  "%s: termination head: members %d not in 0..2 (CMBPO_TERM_ELITE / _ANY / _MAJORITY)", who, th->members);
  }
  // (host code: nothing reads the draws here, any float may stand in them)
  CMBPO_REQUIRE(c.term_thr == nullptr || th != nullptr,
                "%s: termination draws (d_term_thr) need a termination head: th is NULL, and there is no column to compare them with", who);
  if (c.ch != nullptr) {
    CMBPO_REQUIRE(c.ch->kind == 0 || c.ch->kind == 1, "%s: cost head: kind %d not in {0, 1} (0 magnitude, 1 logistic)", who, c.ch->kind);
    CMBPO_REQUIRE(isfinite(c.ch->logit_shift), "%s: cost head: logit_shift %g is not a finite number", who, (double)c.ch->logit_shift);
    CMBPO_REQUIRE(c.ch->kind == 0 || learned_cost,
                  "%s: cost head: kind 1 (logistic) needs CMBPO_TASK_LEARNED_COST (a static cost rule has no logit), task %d", who, task_arg);
  }
  // (host code: the votes' modes, the byte mask, the learned-cost refusal, the head's two outputs)
  if (c.rv != nullptr)
    if (int rc = cmbpo_internal_rule_votes_check(who, c)) return rc;
  PostArgsDerived ar{};
  if (user)     // (registered? columns inside obs_dim / act_dim? -- host code, before any HIP call)
    if (int rc = cmbpo_internal_task_rules_resolve(who, task_arg, obs_dim, act_dim, c.act != nullptr, &ar.rules, &ar.der)) return rc;
  const bool derived = user && ar.der.n_derived > 0;      // the instances with the derived table in their arguments
  CMBPO_REQUIRE(c.mean && c.var && c.obs && c.elite && c.next_obs && c.rew && c.term && c.cost && c.dkl_path && c.ep_var_mean,
                "%s: NULL buffer", who);
  if (dis != nullptr) {
    // (x >= 0 is false for a NaN; the infinities are excluded on their own)
    CMBPO_REQUIRE(dis->kappa_rew >= 0.0f && isfinite(dis->kappa_rew), "%s: kappa_rew %g is not a finite number >= 0", who, (double)dis->kappa_rew);
    CMBPO_REQUIRE(dis->kappa_cost >= 0.0f && isfinite(dis->kappa_cost), "%s: kappa_cost %g is not a finite number >= 0", who, (double)dis->kappa_cost);
    // (with the votes a static cost has a member spread: the vote kernel applies kappa_cost, the post kernel gets 0 below)
    CMBPO_REQUIRE(!(dis->kappa_cost > 0.0f) || learned_cost || c.rv != nullptr,
                  "%s: kappa_cost %g > 0 needs CMBPO_TASK_LEARNED_COST (a static cost rule has no member spread), task %d", who,
                  (double)dis->kappa_cost, task_arg);
    CMBPO_REQUIRE(dis->rew_var && dis->cost_var, "%s: NULL buffer (d_rew_var / d_cost_var)", who);
  }
  CMBPO_REQUIRE(c.n_rows >= 0 && c.ld_rows >= c.n_rows, "%s: n_rows %d / ld_rows %d", who, c.n_rows, c.ld_rows);
  if (c.n_rows == 0) return CMBPO_OK;
  DisExtra dis_post;
  if (dis != nullptr && c.rv != nullptr && !learned_cost) {
    dis_post = *dis;
    dis_post.kappa_cost = 0.0f;     // (the post kernel does not read it with a static cost; its check of the call is the one above)
    dis = &dis_post;
  }
  PostArgs a{};
  a.task = task; a.ensemble = ensemble; a.obs_dim = obs_dim; a.act_dim = act_dim;
  a.out_dim = obs_dim + 1 + learned_cost + (th ? 1 : 0);  // delta-obs + reward (+ cost: algorithms/cmbpo.py:121-123, m_learn_cost) (+ the termination head's column)
  a.learned_cost = learned_cost;
  a.mean = c.mean; a.var = c.var; a.ld_rows = c.ld_rows; a.obs = c.obs; a.act = c.act;
  a.elite = c.elite; a.row_idx = c.row_idx; a.n_rows_dev = c.n_rows_dev; a.n_rows = c.n_rows;
  a.next_obs = c.next_obs; a.rew = c.rew; a.term = c.term; a.cost = c.cost;
  a.dkl_path = c.dkl_path; a.ep_var_mean = c.ep_var_mean; a.ep_var = c.ep_var;
  const size_t lds = (size_t)3 * kRows * obs_dim * sizeof(float) + kRows * sizeof(int);
  const dim3 grid(cmbpo_ceil_div(c.n_rows, kRows));
  hipStream_t s = (hipStream_t)stream;
  if (user) static_cast<PostArgs &>(ar) = a;
  if (c.xi != nullptr) {
    if (derived) {
      PostArgsDerivedNoise an{};
      static_cast<PostArgsDerived &>(an) = ar;
      an.xi = c.xi;
      launch_post_ext<2, true>(ensemble, grid, lds, s, an, dis, th, c.term_thr, ch);
    } else if (user) {
      PostArgsRulesNoise an{};
      static_cast<PostArgsRules &>(an) = ar;
      an.xi = c.xi;
      launch_post_ext<1, true>(ensemble, grid, lds, s, an, dis, th, c.term_thr, ch);
    } else {
      PostArgsNoise an{};
      static_cast<PostArgs &>(an) = a;
      an.xi = c.xi;
      launch_post_ext<0, true>(ensemble, grid, lds, s, an, dis, th, c.term_thr, ch);
    }
  } else if (derived) launch_post_ext<2, false>(ensemble, grid, lds, s, ar, dis, th, c.term_thr, ch);
  else if (user) launch_post_ext<1, false>(ensemble, grid, lds, s, ar, dis, th, c.term_thr, ch);
  else launch_post_ext<0, false>(ensemble, grid, lds, s, a, dis, th, c.term_thr, ch);
  CMBPO_HIP_CHECK(hipGetLastError());
  // the votes: one more kernel behind the post kernel, on the same stream; it overwrites term, cost and (dis_on) cost_var
  if (c.rv != nullptr) return cmbpo_internal_rule_votes_launch(c, task, a.out_dim, user ? &ar.rules : nullptr, derived ? &ar.der : nullptr, stream);
  return CMBPO_OK;
}

// The seven public entry points fill the descriptor and make that call; none forwards to another.  POST_COMMON: the 20 leading
// parameters they share (the stream goes beside the descriptor).
#define POST_COMMON                                                                                                              \
  int task, int ensemble, int obs_dim, int act_dim, const float *d_mean, const float *d_var, int ld_rows, const float *d_obs,    \
      const float *d_act, const int32_t *d_elite, const int32_t *d_row_idx, const int32_t *d_n_rows, int n_rows, float *d_next_obs, \
      float *d_rew, uint8_t *d_term, float *d_cost, float *d_dkl_path, float *d_ep_var_mean, float *d_ep_var
#define POST_COMMON_ARGS                                                                                                        \
  task, ensemble, obs_dim, act_dim, d_mean, d_var, ld_rows, d_obs, d_act, d_elite, d_row_idx, d_n_rows, n_rows, d_next_obs, d_rew, \
      d_term, d_cost, d_dkl_path, d_ep_var_mean, d_ep_var

static FakeenvPostCall post_common(POST_COMMON) {
  FakeenvPostCall c{};      // (every feature off)
  c.task = task; c.ensemble = ensemble; c.obs_dim = obs_dim; c.act_dim = act_dim;
  c.mean = d_mean; c.var = d_var; c.ld_rows = ld_rows; c.obs = d_obs; c.act = d_act;
  c.elite = d_elite; c.row_idx = d_row_idx; c.n_rows_dev = d_n_rows; c.n_rows = n_rows;
  c.next_obs = d_next_obs; c.rew = d_rew; c.term = d_term; c.cost = d_cost;
  c.dkl_path = d_dkl_path; c.ep_var_mean = d_ep_var_mean; c.ep_var = d_ep_var;
  return c;
}

extern "C" int cmbpo_fakeenv_post(POST_COMMON, void *stream) {
  return cmbpo_internal_fakeenv_post(post_common(POST_COMMON_ARGS), stream);
}

// ... with stochastic transitions: next_obs = mean + std * xi + obs (see the kernel); d_xi == NULL is cmbpo_fakeenv_post
extern "C" int cmbpo_fakeenv_post_noise(POST_COMMON, const float *d_xi, void *stream) {
  FakeenvPostCall c = post_common(POST_COMMON_ARGS);
  c.xi = d_xi;
  return cmbpo_internal_fakeenv_post(c, stream);
}

// ... with the ensemble's disagreement on the reward and the learned-cost column measured, and the pessimistic reward / cost made
// from it (see the kernel's DIS parts and the header); d_xi may be NULL: the deterministic transition.  Always on here: NULL
// variance buffers are refused under this entry's name.
extern "C" int cmbpo_fakeenv_post_disagreement(POST_COMMON, const float *d_xi, float kappa_rew, float kappa_cost, float *d_rew_var,
                                               float *d_cost_var, void *stream) {
  FakeenvPostCall c = post_common(POST_COMMON_ARGS);
  c.xi = d_xi;
  c.dis_on = true;
  c.dis = DisExtra{kappa_rew, kappa_cost, d_rew_var, d_cost_var};
  return cmbpo_internal_fakeenv_post(c, stream);
}

// ... with the learned termination head (see the kernel's TERM parts and the header): the superset -- every feature is optional
extern "C" int cmbpo_fakeenv_post_term(POST_COMMON, const float *d_xi, float kappa_rew, float kappa_cost, float *d_rew_var,
                                       float *d_cost_var, const cmbpo_term_head_t *th, void *stream) {
  FakeenvPostCall c = post_common(POST_COMMON_ARGS);
  c.xi = d_xi;
  // (kappa != 0 is true for a NaN: the disagreement's own check names it)
  c.dis_on = d_rew_var != nullptr || d_cost_var != nullptr || kappa_rew != 0.0f || kappa_cost != 0.0f;
  c.dis = DisExtra{kappa_rew, kappa_cost, d_rew_var, d_cost_var};
  c.th = th;
  return cmbpo_internal_fakeenv_post(c, stream);
}

// ... with the learned cost head's reading (see the kernel's COST parts and the header): the superset -- every feature is optional;
// ch == NULL or kind 0 is cmbpo_fakeenv_post_term's call
extern "C" int cmbpo_fakeenv_post_cost(POST_COMMON, const float *d_xi, float kappa_rew, float kappa_cost, float *d_rew_var,
                                       float *d_cost_var, const cmbpo_term_head_t *th, const cmbpo_cost_head_t *ch, void *stream) {
  FakeenvPostCall c = post_common(POST_COMMON_ARGS);
  c.xi = d_xi;
  c.dis_on = d_rew_var != nullptr || d_cost_var != nullptr || kappa_rew != 0.0f || kappa_cost != 0.0f;
  c.dis = DisExtra{kappa_rew, kappa_cost, d_rew_var, d_cost_var};
  c.th = th;
  c.ch = ch;
  return cmbpo_internal_fakeenv_post(c, stream);
}

// ... with sampled terminations (see the kernel's DRAW parts and the header): the superset -- every feature is optional;
// d_term_thr == NULL is cmbpo_fakeenv_post_cost's call
extern "C" int cmbpo_fakeenv_post_term_draws(POST_COMMON, const float *d_xi, float kappa_rew, float kappa_cost, float *d_rew_var,
                                             float *d_cost_var, const cmbpo_term_head_t *th, const cmbpo_cost_head_t *ch,
                                             const float *d_term_thr, void *stream) {
  FakeenvPostCall c = post_common(POST_COMMON_ARGS);
  c.xi = d_xi;
  c.dis_on = d_rew_var != nullptr || d_cost_var != nullptr || kappa_rew != 0.0f || kappa_cost != 0.0f;
  c.dis = DisExtra{kappa_rew, kappa_cost, d_rew_var, d_cost_var};
  c.th = th;
  c.ch = ch;
  c.term_thr = d_term_thr;
  return cmbpo_internal_fakeenv_post(c, stream);
}

// ... with the ensemble-voted static rules (csrc/rule_votes.hip and the header): the superset -- every feature is optional;
// rv == NULL is cmbpo_fakeenv_post_term_draws's call
extern "C" int cmbpo_fakeenv_post_votes(POST_COMMON, const float *d_xi, float kappa_rew, float kappa_cost, float *d_rew_var,
                                        float *d_cost_var, const cmbpo_term_head_t *th, const cmbpo_cost_head_t *ch,
                                        const float *d_term_thr, const cmbpo_rule_votes_t *rv, void *stream) {
  FakeenvPostCall c = post_common(POST_COMMON_ARGS);
  c.xi = d_xi;
  c.dis_on = d_rew_var != nullptr || d_cost_var != nullptr || kappa_rew != 0.0f || kappa_cost != 0.0f;
  c.dis = DisExtra{kappa_rew, kappa_cost, d_rew_var, d_cost_var};
  c.th = th;
  c.ch = ch;
  c.term_thr = d_term_thr;
  c.rv = rv;
  return cmbpo_internal_fakeenv_post(c, stream);
}

#undef POST_COMMON
#undef POST_COMMON_ARGS
