/*
 * cmbpo_hip.h -- C-ABI of the MI355X (gfx950) hot path for CMBPO.
 *
 * The reference (anyboby/Constrained-Model-Based-Policy-Optimization) is pure
 * Python on TF 1.14 + NumPy: it has no FFI.  The "binding" a maintainer adds is
 * therefore a ctypes stub; every entry point below names
 * the reference Python interface (file:line, relative to the reference tree)
 * whose arithmetic it replaces.
 *
 * Conventions
 *   - every function returns 0 on success, a negative CMBPO_E* code otherwise;
 *     cmbpo_last_error() returns a static, human-readable string for the last
 *     failure on the calling thread.
 *   - all pointers named d_* are DEVICE pointers owned by the caller (the
 *     Python side allocates them as torch tensors); h_* are HOST pointers.
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous on
 *     that stream, nothing in here synchronises or allocates per call.
 *   - handles own only packed weight copies; one host thread per handle.
 *   - float is IEEE fp32; masks are uint8_t (0/1); indices are int32_t.
 */
#ifndef CMBPO_HIP_H
#define CMBPO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMBPO_OK 0
#define CMBPO_EINVAL (-1)   /* bad argument / unsupported shape            */
#define CMBPO_EHIP (-2)     /* a HIP runtime call failed                   */
#define CMBPO_ENOMEM (-3)   /* allocation failed                           */
#define CMBPO_ESTATE (-4)   /* handle used before weights were loaded      */

/* activations (models/pens/fc.py:13-20, network/ac_network.py:26-33) */
#define CMBPO_ACT_SWISH 0
#define CMBPO_ACT_TANH 1

/* output heads */
#define CMBPO_HEAD_PROB 0     /* mean|logvar split, models/pens/pe.py:789-838 */
#define CMBPO_HEAD_DETMEAN 1  /* single head, mean over members, pe.py:338-343,648-669 */
#define CMBPO_HEAD_GAUSS_PI 2 /* tanh-MLP Gaussian policy, network/ac_network.py:99-123 */

/* static termination / cost rules (models/statics.py:56-69) */
#define CMBPO_TASK_DEFAULT 0  /* no_done, zero (bool) cost: Hopper/Humanoid */
#define CMBPO_TASK_HCS 1      /* HalfCheetahSafe-v2: no_done + hcs_cost_f    */
#define CMBPO_TASK_ANTSAFE 2  /* AntSafe-v2: antsafe_term_fn + antsafe_c_fn  */
/* Flag bit, or-ed into the `task` argument of cmbpo_fakeenv_post / cmbpo_rollout_step / cmbpo_rollout_run: the model has a
 * learned cost head (algorithms/cmbpo.py:46,123 m_learn_cost; models/fake_env.py:139-151 predicts_cost).  (mean, var) are
 * then [E, ld_rows, obs + 2], the cost is column obs + 1 of the elite member's mean (stored as it is, non-finite values
 * included), the reward column obs; the task's termination rule still applies, its cost rule does not.  Any other bit
 * outside the rule id is rejected. */
#define CMBPO_TASK_LEARNED_COST 0x100

/* User-defined termination / cost rules: what a user of the reference adds to TERMS_BY_TASK / COST_BY_TASK as a NumPy
 * function (models/statics.py:56-69), declared as a table of at most 16 clauses and evaluated by cmbpo_fakeenv_post on the
 * device.  A registered table is a rule id CMBPO_TASK_USER_BASE + slot (16..79, below the flag bit), valid wherever a
 * built-in id is.
 *
 * A clause tests the columns [col0, col0 + n_cols) of one source row (col0 < 0 counts from the end, n_cols == -1 means
 * through the last column; resolved against obs_dim / act_dim at launch).  Per column, in float32 with single roundings:
 *   f = fl32(x * scale);  f = |f| with CMBPO_RULE_ABS;
 *   the column holds iff (LO_STRICT ? f > lo : f >= lo) && (HI_STRICT ? f < hi : f <= hi)
 * -- written positively, so a NaN never holds (NumPy's comparisons); lo = -inf / hi = +inf leave a side open.  The clause
 * holds iff all its columns hold, or any of them with CMBPO_RULE_ANY.
 *   done = (require_finite && !isfinite(next_obs).all()) || some HEALTHY clause does not hold || some FATAL clause holds
 *   obj  = 1.0f if some COST clause holds, else 0.0f
 *   cost = cost_on_term ? min(1, done + obj) : obj            (the shape of models/statics.py:51-52)
 * With CMBPO_TASK_LEARNED_COST the cost is the model's column; COST clauses and cost_on_term are ignored, done is not.
 * What an interval on one column cannot say (a distance, a speed, a tilt) is a derived quantity, below: a fourth source,
 * CMBPO_RULE_SRC_DERIVED, known to cmbpo_task_rules_register_ex only. */
#define CMBPO_TASK_USER_BASE 16
#define CMBPO_TASK_USER_SLOTS 64
#define CMBPO_RULE_MAX_CLAUSES 16
#define CMBPO_RULE_HEALTHY 0      /* role: the branch is done if the clause does NOT hold */
#define CMBPO_RULE_FATAL 1        /*       the branch is done if the clause holds         */
#define CMBPO_RULE_COST 2         /*       the step costs 1 if the clause holds           */
#define CMBPO_RULE_SRC_NEXT_OBS 0 /* src */
#define CMBPO_RULE_SRC_OBS 1
#define CMBPO_RULE_SRC_ACT 2
#define CMBPO_RULE_ABS 1          /* flags */
#define CMBPO_RULE_LO_STRICT 2
#define CMBPO_RULE_HI_STRICT 4
#define CMBPO_RULE_ANY 8

typedef struct cmbpo_rule_clause {
  int32_t role, src, col0, n_cols, flags;
  float scale, lo, hi;
} cmbpo_rule_clause_t; /* 32 bytes */

typedef struct cmbpo_task_rules {
  int32_t n_clauses, require_finite, cost_on_term, reserved;
  cmbpo_rule_clause_t clause[CMBPO_RULE_MAX_CLAUSES];
} cmbpo_task_rules_t; /* 528 bytes */

/* Validates the table (host code only: n_clauses in 0..16, known role / src / flags, finite scale, lo / hi not NaN with
 * lo <= hi, n_cols >= 1 or -1, require_finite / cost_on_term 0 or 1, reserved == 0) and stores it; *out_task is its rule
 * id.  A table byte-identical to a stored one gets that one's id.  CMBPO_EINVAL with a message naming the field, or
 * saying that all CMBPO_TASK_USER_SLOTS slots are taken.  Safe to call from several threads. */
int cmbpo_task_rules_register(const cmbpo_task_rules_t *rules, int *out_task);
/* the table behind a registered rule id (the learned-cost bit is ignored); CMBPO_EINVAL if the id is not registered */
int cmbpo_task_rules_get(int task, cmbpo_task_rules_t *out);
/* number of registered tables */
int cmbpo_task_rules_count(void);

/* Derived quantities: what an interval on a single column cannot say -- "within radius r of a point", a planar speed limit,
 * a tilt limit 1 - 2 (q1^2 + q2^2) >= c (models/statics.py:22, z_rot).  A rule set may declare up to 8 of them, each a bias
 * and up to 4 terms, evaluated per branch in float32 with single roundings, in this order, without contraction:
 *   g = bias
 *   for each term in order:
 *     t = fl32(x - c)                     x: column `col` of the term's source row (next_obs, obs or act; col < 0 counts
 *     if pow == 2: t = fl32(t * t)           from the end, resolved against obs_dim / act_dim at launch)
 *     g = fl32(g + fl32(w * t))
 * A clause with src CMBPO_RULE_SRC_DERIVED tests derived quantities instead of columns: col0 / n_cols index them (col0 < 0
 * counts from the last one, n_cols == -1 means through the last one) and everything else about the clause -- scale, ABS,
 * the interval, ANY, the role -- applies to g unchanged.  A NaN g never holds; inf - inf is NaN by the arithmetic above.
 * Products of two different columns stay out. */
#define CMBPO_RULE_SRC_DERIVED 3
#define CMBPO_RULE_MAX_DERIVED 8
#define CMBPO_RULE_MAX_TERMS 4

typedef struct cmbpo_rule_term {
  int16_t src; /* CMBPO_RULE_SRC_NEXT_OBS / _OBS / _ACT */
  int16_t pow; /* 1 or 2 */
  int32_t col;
  float w, c;  /* finite */
} cmbpo_rule_term_t; /* 16 bytes */

typedef struct cmbpo_rule_derived {
  int32_t n_terms; /* 1..4 */
  float bias;      /* finite */
  int32_t reserved[2];
  cmbpo_rule_term_t term[CMBPO_RULE_MAX_TERMS];
} cmbpo_rule_derived_t; /* 80 bytes */

typedef struct cmbpo_rule_derived_table {
  int32_t n_derived; /* 0 (none) .. 8 */
  int32_t reserved[3];
  cmbpo_rule_derived_t derived[CMBPO_RULE_MAX_DERIVED];
} cmbpo_rule_derived_table_t; /* 656 bytes */

/* cmbpo_task_rules_register with derived quantities.  derived == NULL or n_derived == 0 IS cmbpo_task_rules_register (the
 * same checks, the same messages, the same id for a byte-identical table; src CMBPO_RULE_SRC_DERIVED stays unknown there).
 * Otherwise the clause table is checked as before, with CMBPO_RULE_SRC_DERIVED a known source, and the derived table:
 * n_derived in 1..8, n_terms in 1..4, a term's src in {next_obs, obs, act}, pow in {1, 2}, finite w / c / bias, reserved
 * fields zero, a derived clause's indices inside [0, n_derived).  Every rejection names the field and its place
 * ("derived 2: term 1: w ...", "clause 0: ... derived ...").  Ids are deduplicated on the pair of byte images and share
 * the slots of cmbpo_task_rules_register. */
int cmbpo_task_rules_register_ex(const cmbpo_task_rules_t *rules, const cmbpo_rule_derived_table_t *derived, int *out_task);
/* the derived table behind a registered rule id (all zeros for an id registered without one); CMBPO_EINVAL if the id is
 * not registered */
int cmbpo_task_rules_get_derived(int task, cmbpo_rule_derived_table_t *out);

const char *cmbpo_last_error(void);
int cmbpo_version(void);

/* Matrix path of the 512-wide probabilistic ensemble forward (cmbpo_ens_forward / cmbpo_rollout_step): same
 * function, same float32 inputs / outputs, two ways to form the float32 products of its three GEMMs.
 * CMBPO_ENS_FP32: v_mfma_f32_32x32x2f32.  CMBPO_ENS_SPLIT_BF16 (default): every operand is split exactly into
 * three bf16 pieces (3 x 8 = 24 mantissa bits) and a.b = sum_{i+j<=4} a_i b_j runs as six
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- every partial product exact, dropped terms <= 2^-24 |ab|,
 * measured error 6.2e-7 of sum|a_k b_k| at K = 512 against 7.6e-7 for the fp32 MFMA chain
 * (tools/split_bf16_probe.hip) -- at about twice the matrix rate.  Both pass the same parity tests.  The switch
 * also covers the critics
 * (cmbpo_ens_predict_mean at 128 hidden units, one output; paths 1 and 2 both mean the bf16 split there); every other
 * shape / head uses fp32 MFMAs.
 * CMBPO_ENS_SPLIT_F16 (default since round 2, csrc/ens_h3.hip): every operand is lifted by a power of two into the top
 * of the f16 range and split exactly into two f16 pieces (11 + 1 + 11 significant bits = a float32 rounding);
 * a.b = a2 b1 + a1 b2 + a1 b1 runs as three v_mfma_f32_32x32x16_f16 with fp32 accumulation -- measured error 3.2e-7 of
 * sum|a_k b_k| at K = 512 (tools/split_f16_probe.hip) -- with scales derived from norm bounds so that no finite input
 * can overflow a piece.  Rows of a call below cmbpo_set_ens_f16_min_rows take the bf16 path (smaller items). */
#define CMBPO_ENS_FP32 0
#define CMBPO_ENS_SPLIT_BF16 1
#define CMBPO_ENS_SPLIT_F16 2
int cmbpo_set_ens_matrix_path(int path);
int cmbpo_get_ens_matrix_path(void);
/* Tuning knob: calls of the 512-wide probabilistic forward with fewer rows than this use CMBPO_ENS_SPLIT_BF16 even when
 * CMBPO_ENS_SPLIT_F16 is selected (its 128-row items leave CUs idle at small rollout batches); 0 = never. */
int cmbpo_set_ens_f16_min_rows(int rows);
/* Tuning knob: 32-row tiles per item of the CMBPO_ENS_SPLIT_F16 kernel: 4 (128-row items, the throughput shape), 2 or 1
 * (the same kernel for rollout batches too small to give every CU a 128-row item); 0 (default) chooses by row count. */
int cmbpo_set_ens_f16_row_tiles(int rt);
/* Tuning knob: calls of the CMBPO_ENS_SPLIT_F16 forward with at least this many rows build the split input image once per
 * row (a small launch in front of the main one, which reads it by LDS-DMA) instead of once per (member, row) inside the
 * main launch; only main launches of 128-row items on the stage-ahead instances (input width <= 48) take it.  0 (default):
 * from the row count at which every workgroup of the main launch has at least two items; < 0: never; 1: whenever the main
 * launch has 128-row items.  The outputs do not depend on it, bit for bit. */
int cmbpo_set_ens_f16_image_min_rows(int rows);

/* ------------------------------------------------------------------------ *
 * Ensemble MLP handle: a 3-layer (in -> H -> H -> O) ensemble of E members.
 * Replaces the TF variables of models/pens/pe.py:150-213 (PE.finalize: layers
 * FC0..FC2 + TensorStandardScaler in/out) and, for HEAD_GAUSS_PI, the `pi`
 * scope of network/ac_network.py:99-123 (dense x3 + log_std).
 * ------------------------------------------------------------------------ */
typedef struct cmbpo_mlp cmbpo_mlp_t;

/* hidden must be 128, 256 or 512 (256: the general fp32-MFMA kernels only).  out_width is the network's last-layer width
 * (2*out_dim for HEAD_PROB, out_dim otherwise), <= 128. */
int cmbpo_mlp_create(cmbpo_mlp_t **out, int ensemble, int in_dim, int hidden,
                     int out_width, int activation, int head);
void cmbpo_mlp_destroy(cmbpo_mlp_t *m);

/* Weights in the reference's layout (models/pens/fc.py:135-166): W[E,in,out]
 * row-major, b[E,out] (the reference's [E,1,out]).  Scaler vectors are the
 * TensorStandardScaler mu/var ([1,dim], models/pens/utils.py:100-115); pass
 * NULL for "no scaler".  h_log_std (HEAD_GAUSS_PI only) is the [out] vector of
 * network/ac_network.py:104.  Packs on the host, copies on `stream`. */
int cmbpo_mlp_load(cmbpo_mlp_t *m, const float *h_w0, const float *h_b0,
                   const float *h_w1, const float *h_b1, const float *h_w2,
                   const float *h_b2, const float *h_in_mu,
                   const float *h_in_var, const float *h_out_mu,
                   const float *h_out_var, const float *h_log_std,
                   void *stream);

/* A Gaussian policy's parameters as ONE flat device vector in the order of
 * get_vars('pi') (network/ac_network.py:35-36, the order trust_region.py:21-25
 * assigns them in): W0[in,H] | b0 | W1[H,H] | b1 | W2[H,out] | b2 | log_std.
 * The trust-region update leaves the accepted parameters on the device
 * (policies/cpo_policy.py:278-300); this packs them into a handle that was
 * loaded once through cmbpo_mlp_load (one network, GAUSS_PI head, no scalers)
 * without a trip through the host. */
int cmbpo_mlp_load_policy_flat(cmbpo_mlp_t *m, const float *d_flat, void *stream);

/* PE.predict_ensemble, 2-D input path (models/pens/pe.py:688-697 ->
 * _compile_outputs(scale_output=True) :789-838 -> FC.compute_output_tensor
 * models/pens/fc.py:74-95 -> TensorStandardScaler models/pens/utils.py:156-187).
 * x = [obs | act] per row (the concat of models/fake_env.py:81); d_act may be
 * NULL with act_dim 0.  Row i of the call is branch d_row_idx[i] (or i when
 * d_row_idx is NULL); d_n_rows (device int, may be NULL) overrides n_rows so a
 * captured launch follows a device-side alive count.  Outputs are indexed
 * [member][branch slot][out_dim] with leading dimension ld_rows.
 * Forwards on one handle are stream-ordered: the handle owns the f16 weight images and the split input image of the call's
 * rows (both allocated on first use; the input image for ceil(ld_rows / 128) row tiles, regrown -- with a device
 * synchronisation -- when a call needs more), and a forward reads what its own launches wrote there.  CMBPO_ENOMEM
 * with a message, and no launch, when an allocation fails. */
int cmbpo_ens_forward(cmbpo_mlp_t *m, const float *d_obs, int obs_dim,
                      const float *d_act, int act_dim, const int32_t *d_row_idx,
                      const int32_t *d_n_rows, int n_rows, int ld_rows,
                      float *d_mean, float *d_var, void *stream);

/* PE.predict for the critics (models/pens/pe.py:648-669; mean over ALL members
 * :338-343), as used by CPOPolicy.get_v/get_vc (policies/cpo_policy.py:825-835).
 * d_out is [branch slot][out_dim]. */
int cmbpo_ens_predict_mean(cmbpo_mlp_t *m, const float *d_obs, int obs_dim,
                           const int32_t *d_row_idx, const int32_t *d_n_rows,
                           int n_rows, float *d_out, void *stream);

/* Both critics of a rollout step in one launch: CPOPolicy.get_v and get_vc (policies/cpo_policy.py:825-835) on the same
 * observation rows -- two loaded HEAD_DETMEAN ensembles of 128 hidden units, swish, one output, equal input width and
 * member count (<= 4).  Same function as two cmbpo_ens_predict_mean calls; float32 products run as three f16 MFMAs
 * (csrc/critic_f16.hip), one wave per (critic, member).  d_v / d_vc are [branch slot]. */
int cmbpo_critic_pair_supported(const cmbpo_mlp_t *v, const cmbpo_mlp_t *vc);
int cmbpo_critic_pair_predict(cmbpo_mlp_t *v, cmbpo_mlp_t *vc, const float *d_obs, int obs_dim,
                              const int32_t *d_row_idx, const int32_t *d_n_rows, int n_rows,
                              float *d_v, float *d_vc, void *stream);
/* The same launch with the critics' own disagreement measured and, where a coefficient is > 0, held against the value.  With
 * x_e the value of member e (float32, after its inverse_transform: the bits cmbpo_critic_pair_predict adds up), per critic:
 *   mean  = (((x_0 + x_1) + x_2) + ...) / E                          cmbpo_critic_pair_predict's bits
 *   var   = q / E, q = sum_e (x_e - mean)^2 in member order          np.var over the members, every operation rounded to
 *                                                                    float32 on its own, no contraction; E = 1: +0
 *   d_v   = fl32(mean - fl32(kappa_v  * sqrtf(var_v )))   if kappa_v  > 0, else mean bit for bit
 *   d_vc  = fl32(mean + fl32(kappa_vc * sqrtf(var_vc)))   if kappa_vc > 0, else mean bit for bit
 * (sqrtf correctly rounded; the variances are in output units, after the output scaler).  With a coefficient > 0 non-finite
 * members propagate as NumPy propagates them.  d_v_var / d_vc_var are slot indexed like d_v / d_vc and required.
 * cmbpo_critic_pair_predict's argument checks; kappa_* finite and >= 0, non-NULL variance outputs -- all before any HIP call.
 * Same choice of kernel by n_rows as the plain entry (the member-after-member kernel's instances of this entry take chunks of
 * 448 instead of 512 rows at up to 32 inputs: every member's value of a row stays in LDS). */
int cmbpo_critic_pair_predict_var(cmbpo_mlp_t *v, cmbpo_mlp_t *vc, const float *d_obs, int obs_dim,
                                  const int32_t *d_row_idx, const int32_t *d_n_rows, int n_rows,
                                  float kappa_v, float kappa_vc, float *d_v, float *d_vc,
                                  float *d_v_var, float *d_vc_var, void *stream);

/* mlp_gaussian_policy forward (network/ac_network.py:99-123) behind
 * CPOPolicy.get_action_outs (policies/cpo_policy.py:801-823): mu = MLP(obs),
 * pi = mu + eps*exp(log_std), logp_pi = gaussian_likelihood(pi, mu, log_std)
 * (:46-48).  eps is an input (the reference draws tf.random_normal, :109);
 * outputs indexed by branch slot: d_pi,d_mu,d_logstd [.,act_dim], d_logp [.]. */
int cmbpo_policy_forward(cmbpo_mlp_t *m, const float *d_obs, int obs_dim,
                         const float *d_eps, const int32_t *d_row_idx,
                         const int32_t *d_n_rows, int n_rows, float *d_pi,
                         float *d_logp, float *d_mu, float *d_logstd,
                         void *stream);

/* FakeEnv.step after the ensemble forward (models/fake_env.py:104-151):
 * std = sqrt(var); ens_ep_var = var_E(mean[..., :obs]); dkl_path = mean_d
 * average_dkl(mean, std) (models/pens/utils.py:15-57, all E members);
 * next_obs = mean[elite[b], b, :obs] + obs (delta model, deterministic=True; cmbpo_fakeenv_post_noise below samples it);
 * r = mean[elite[b], b, obs]; term / cost from models/statics.py evaluated on
 * (obs, act, next_obs).  d_elite is the per-row member index (the draw of
 * models/fake_env.py:174-178, injected by the caller).  Row addressing as in
 * cmbpo_ens_forward.  d_cost is float (bool cast for the default task),
 * d_term is uint8.  d_mean / d_var are [E, ld_rows, obs + 1], or
 * [E, ld_rows, obs + 2] with CMBPO_TASK_LEARNED_COST set in `task`.  d_ep_var_mean = mean over obs dims of ens_ep_var (what
 * samplers/model_sampler.py:322,343 consume); d_ep_var [.,obs_dim] optional.
 * `task` is a built-in rule id or one cmbpo_task_rules_register returned (term / cost from its clause table), with or
 * without CMBPO_TASK_LEARNED_COST; an unregistered id, a clause whose columns lie outside obs_dim / act_dim, or a clause on
 * the actions with d_act == NULL is CMBPO_EINVAL, decided before any HIP call. */
int cmbpo_fakeenv_post(int task, int ensemble, int obs_dim, int act_dim,
                       const float *d_mean, const float *d_var, int ld_rows,
                       const float *d_obs, const float *d_act,
                       const int32_t *d_elite, const int32_t *d_row_idx,
                       const int32_t *d_n_rows, int n_rows, float *d_next_obs,
                       float *d_rew, uint8_t *d_term, float *d_cost,
                       float *d_dkl_path, float *d_ep_var_mean,
                       float *d_ep_var, void *stream);
/* The same step with stochastic transitions: the imagined next state is drawn from the elite member's predictive
 * distribution, N(mean, var) per observation dimension, instead of placed at its mean (the `deterministic=False` hook of
 * models/fake_env.py:103-108, whose `+ pred_std` carries no random factor: it is the special case xi == 1).  d_xi is
 * [., obs_dim] float32, slot indexed like d_obs (leading dimension ld_rows rows), one draw per (row, dimension) shared by
 * all members of the row; only the observation columns move:
 *   std_e = fl32(sqrt(var_e)) (correctly rounded);  m~_e = fl32(mean_e[:obs] + fl32(std_e * xi))   (no fused multiply-add)
 *   ens_ep_var, dkl_path: cmbpo_fakeenv_post's formulas on m~_e and the unperturbed var_e (fake_env.py:112-113 run on the
 *   shifted means);  next_obs = fl32(m~_elite + obs);  r and the learned cost: the elite's unperturbed mean columns;
 *   term / cost rules on (obs, act, next_obs) as in cmbpo_fakeenv_post.
 * d_xi == NULL forwards to cmbpo_fakeenv_post; the same argument checks, all before any HIP call. */
int cmbpo_fakeenv_post_noise(int task, int ensemble, int obs_dim, int act_dim,
                             const float *d_mean, const float *d_var, int ld_rows,
                             const float *d_obs, const float *d_act,
                             const int32_t *d_elite, const int32_t *d_row_idx,
                             const int32_t *d_n_rows, int n_rows, float *d_next_obs,
                             float *d_rew, uint8_t *d_term, float *d_cost,
                             float *d_dkl_path, float *d_ep_var_mean,
                             float *d_ep_var, const float *d_xi, void *stream);
/* The same step with the ensemble's disagreement on the reward and the learned-cost column measured and, where a coefficient is
 * > 0, held against the branch (cmbpo_fakeenv_post_noise's arguments, d_xi may be NULL: the deterministic transition):
 *   d_rew_var[r]  = np.var(mean[:, r, obs], axis=0) over ALL E members, float32, in ens_ep_var's order of operations:
 *                   s = ((x_0 + x_1) + x_2) + ...; m = s / E; q = sum_e (x_e - m)^2 in member order; var = q / E (no contraction)
 *   d_cost_var[r] = the same on column obs + 1 with CMBPO_TASK_LEARNED_COST, else +0 (a static cost rule has no member spread)
 *   r    = fl32(r_elite - fl32(kappa_rew * sqrtf(rew_var)))     if kappa_rew > 0, else r_elite bit for bit
 *   cost = fl32(c_elite + fl32(kappa_cost * sqrtf(cost_var)))   if kappa_cost > 0, else c_elite bit for bit
 * (sqrtf correctly rounded).  Both columns are never moved by d_xi, so the variances are those of the unperturbed means.  With
 * a coefficient of 0 no other member's value reaches the output (a NaN there stays there); with one > 0 non-finite members
 * propagate as NumPy propagates them.  next_obs, term, dkl_path, ep_var* do not depend on the feature.  Both new outputs are
 * slot indexed like d_rew and required.  cmbpo_fakeenv_post's argument checks; kappa_* finite and >= 0, kappa_cost > 0 only
 * with CMBPO_TASK_LEARNED_COST, non-NULL outputs -- all before any HIP call. */
int cmbpo_fakeenv_post_disagreement(int task, int ensemble, int obs_dim, int act_dim,
                                    const float *d_mean, const float *d_var, int ld_rows,
                                    const float *d_obs, const float *d_act,
                                    const int32_t *d_elite, const int32_t *d_row_idx,
                                    const int32_t *d_n_rows, int n_rows, float *d_next_obs,
                                    float *d_rew, uint8_t *d_term, float *d_cost,
                                    float *d_dkl_path, float *d_ep_var_mean,
                                    float *d_ep_var, const float *d_xi,
                                    float kappa_rew, float kappa_cost,
                                    float *d_rew_var, float *d_cost_var, void *stream);

/* A learned termination head: the model has one more output column, trained on the real `done` flags, and the
 * post-processing ends a branch where that column says so -- by the elite member's value or by a vote of the members.
 *   tc   = obs_dim + 1 + (1 with CMBPO_TASK_LEARNED_COST): the LAST column; d_mean / d_var are [E, ld_rows, tc + 1]
 *   x_e  = mean[e][r][tc]   (target units: 0 / 1)
 *   hit_e = x_e > threshold   (a positive test: a NaN never hits; +inf does, -inf does not)
 *   votes = sum_e hit_e over ALL E members
 *   learned_done = hit_elite[r]  (CMBPO_TERM_ELITE) | votes > 0  (CMBPO_TERM_ANY) | 2 * votes > E  (CMBPO_TERM_MAJORITY)
 *   term = rule_done || learned_done      for built-in ids, registered tables and the default task alike
 * The cost keeps the RULE's own done (cost_on_term, AntSafe's clip(done + obj)): apart from the two optional outputs the head
 * changes d_term and nothing else.  The column takes no transition noise; DKL, ep_var, next_obs, reward, cost and the
 * disagreement variances do not read it.  term_pred[r] = x_elite (float32, stored as it is) and term_votes[r] = votes (uint8)
 * are slot indexed like d_term; either may be NULL. */
#define CMBPO_TERM_ELITE 0
#define CMBPO_TERM_ANY 1
#define CMBPO_TERM_MAJORITY 2
typedef struct cmbpo_term_head {
  float threshold;        /* finite */
  int32_t members;        /* CMBPO_TERM_* */
  float *term_pred;       /* [.] or NULL */
  uint8_t *term_votes;    /* [.] or NULL */
} cmbpo_term_head_t; /* 24 bytes */
/* cmbpo_fakeenv_post_disagreement's arguments plus the head.  d_xi may be NULL (the deterministic transition);
 * d_rew_var == d_cost_var == NULL with both kappas 0 means no disagreement (the instances without it); th == NULL forwards to
 * the existing entry points, which then run what they always ran.  Beside their checks: a finite threshold, members in 0..2,
 * ensemble <= 8 -- each refused with a message naming the field, before any HIP call. */
int cmbpo_fakeenv_post_term(int task, int ensemble, int obs_dim, int act_dim,
                            const float *d_mean, const float *d_var, int ld_rows,
                            const float *d_obs, const float *d_act,
                            const int32_t *d_elite, const int32_t *d_row_idx,
                            const int32_t *d_n_rows, int n_rows, float *d_next_obs,
                            float *d_rew, uint8_t *d_term, float *d_cost,
                            float *d_dkl_path, float *d_ep_var_mean,
                            float *d_ep_var, const float *d_xi,
                            float kappa_rew, float kappa_cost,
                            float *d_rew_var, float *d_cost_var,
                            const cmbpo_term_head_t *th, void *stream);

/* How the learned-cost column is READ.  Every cost of the built-in tasks and of a rule table is an indicator; a
 * model that learns it with the Bernoulli likelihood (cmbpo_trainer_set_column_kinds, kind 1 on column obs_dim + 1) puts a
 * logit there, and the cost of an imagined step is its probability.  THE definition -- cc = obs_dim + 1, which needs
 * CMBPO_TASK_LEARNED_COST; with a logistic head (kind 1) the members' means there are logits z_e = mean[e][r][cc]:
 *   zs_e     = fl32(z_e - logit_shift)               (logit_shift == 0: z_e bit for bit, no subtraction executed)
 *   p_e      = sigma32(zs_e) = 1 / (1 + expf(-zs))  for zs >= 0,  expf(zs) / (1 + expf(zs))  otherwise;
 *              float32, no contraction, the division correctly rounded; +inf -> 1, -inf -> 0, NaN -> NaN
 *   cost     = p_elite                                without disagreement, or with kappa_cost == 0: bit for bit
 *   cost_var = np.var(p_e over ALL E members) in cmbpo_fakeenv_post_disagreement's order of operations, on the probabilities
 *   cost     = clip1(fl32(p_elite + fl32(kappa_cost * sqrtf(cost_var))))   if kappa_cost > 0;  clip1(c) = c > 1 ? 1 : c
 *              (a positive test: a NaN passes)
 *   cost_logit[r] = z_elite   (raw, unshifted; slot indexed like d_cost; may be NULL)
 * sigma32 is one device function used by every instance and every lane: a member's probability has the same bits wherever it
 * is computed.  logit_shift undoes a class weight: a weight omega on the positive class shifts the fitted logit by log omega
 * (DESIGN 3v), and logit_shift = log omega reads the column as if it had been fitted without.  Nothing else moves: next_obs,
 * term, rew, rew_var, dkl_path and ep_var* do not depend on the head; the termination rule's own `done` is what it was; the
 * column takes no transition noise.  With a termination head as well, the termination column stays the LAST one and cc stays
 * obs_dim + 1.  kind 0 is the magnitude reading -- the call without the struct, logit_shift and cost_logit unused.  There is no
 * bit for it in `task`. */
#define CMBPO_COST_MAGNITUDE 0
#define CMBPO_COST_LOGISTIC 1
typedef struct cmbpo_cost_head {
  int32_t kind;           /* CMBPO_COST_* */
  float logit_shift;      /* finite */
  float *cost_logit;      /* [.] or NULL */
} cmbpo_cost_head_t; /* 16 bytes */
/* cmbpo_fakeenv_post_term's arguments plus the cost head: the superset, every feature optional.  ch == NULL or kind 0 is exactly
 * cmbpo_fakeenv_post_term's call (the same kernel instances with the same argument block).  Beside its checks: kind in {0, 1},
 * a finite logit_shift, kind 1 only with CMBPO_TASK_LEARNED_COST -- each refused with a message naming the cost head, before
 * any HIP call. */
int cmbpo_fakeenv_post_cost(int task, int ensemble, int obs_dim, int act_dim,
                            const float *d_mean, const float *d_var, int ld_rows,
                            const float *d_obs, const float *d_act,
                            const int32_t *d_elite, const int32_t *d_row_idx,
                            const int32_t *d_n_rows, int n_rows, float *d_next_obs,
                            float *d_rew, uint8_t *d_term, float *d_cost,
                            float *d_dkl_path, float *d_ep_var_mean,
                            float *d_ep_var, const float *d_xi,
                            float kappa_rew, float kappa_cost,
                            float *d_rew_var, float *d_cost_var,
                            const cmbpo_term_head_t *th, const cmbpo_cost_head_t *ch, void *stream);

/* Sampled terminations: the termination head read as a hazard, not as a classifier.  THE rule:
 *   hit_e = x_e > thr[r]          thr[r] replaces th->threshold for row r
 *   everything else of cmbpo_term_head_t is unchanged
 * The test is written positively: a NaN on either side never hits; thr = -inf hits every non-NaN x, -inf excepted; thr = +inf
 * never hits; x == thr does not hit.  d_term_thr: float32 [.], slot indexed like d_term, in the column's own units, any value.
 * votes, the three `members` modes, term_pred, term_votes and term = rule_done || learned_done are cmbpo_term_head_t's; all
 * members of a row share the row's threshold; the cost still reads the rule's own done; th->threshold is checked and not read.
 * The kernel knows nothing about uniform numbers: the caller turns a draw u in (0, 1] into a threshold -- logit(u) for a column
 * trained with the Bernoulli likelihood, u itself for one in 0 / 1 target units -- so a branch whose column says p ends with
 * probability p (u = 1 gives +inf under the logit: a probability of exactly 0 never ends a branch).
 * cmbpo_fakeenv_post_cost's arguments plus the thresholds: the superset, every feature optional.  d_term_thr == NULL is exactly
 * cmbpo_fakeenv_post_cost's call (the same kernel instances with the same argument block).  Beside its checks: d_term_thr != NULL
 * needs th != NULL -- refused with a message naming the draws, before any HIP call. */
int cmbpo_fakeenv_post_term_draws(int task, int ensemble, int obs_dim, int act_dim,
                                  const float *d_mean, const float *d_var, int ld_rows,
                                  const float *d_obs, const float *d_act,
                                  const int32_t *d_elite, const int32_t *d_row_idx,
                                  const int32_t *d_n_rows, int n_rows, float *d_next_obs,
                                  float *d_rew, uint8_t *d_term, float *d_cost,
                                  float *d_dkl_path, float *d_ep_var_mean,
                                  float *d_ep_var, const float *d_xi,
                                  float kappa_rew, float kappa_cost,
                                  float *d_rew_var, float *d_cost_var,
                                  const cmbpo_term_head_t *th, const cmbpo_cost_head_t *ch,
                                  const float *d_term_thr, void *stream);

/* Ensemble-voted static rules: the task's own termination and cost rule evaluated on EVERY member's predicted next
 * state, not only on the elite's.  THE rule -- for row r and every member e in 0..E-1, over ALL members like ens_ep_var and the
 * termination head's votes:
 *   nx_e[d]  = fl32(mu_e[d] + obs[d]);  mu_e = mean_e, with d_xi fl32(mean_e + fl32(sqrtf(var_e) * xi[d])) -- the expression
 *              cmbpo_fakeenv_post_noise applies to every member, so nx_elite has the bits of next_obs
 *   done_e, cost_e = the task's rule on (obs, act, nx_e), exactly as cmbpo_fakeenv_post defines it for the elite: AntSafe with its
 *              finite gate and the `gate * z_rot >= -0.7` quirk, HCS, a registered clause table with or without derived
 *              quantities, require_finite and cost_on_term; the default task and every no_done task: done_e = 0.  cost_e uses the
 *              member's own done_e and is an indicator in {0, 1}
 *   done_votes[r] = #{e : done_e},  cost_votes[r] = #{e : cost_e > 0}      (uint8, slot indexed like d_term, either may be NULL)
 *   rule_done = done_elite (CMBPO_TERM_ELITE: what cmbpo_fakeenv_post writes) | votes > 0 (_ANY) | 2 * votes > E (_MAJORITY)
 *   term      = rule_done || learned_done      learned_done: the termination head's verdict, unchanged, sampled thresholds included
 *   cost      = cost_elite (CMBPO_TERM_ELITE) | cost_votes > 0 ? 1 : 0 (_ANY) | 2 * cost_votes > E ? 1 : 0 (_MAJORITY)
 *               | (float)cost_votes / (float)E (CMBPO_VOTE_MEAN: one division, a probability like the logistic head's)
 * With the disagreement on and a static cost (no CMBPO_TASK_LEARNED_COST):
 *   cost_var[r] = np.var(cost_e over ALL E members) in cmbpo_fakeenv_post_disagreement's order of operations (without the votes: +0)
 *   cost        = clip1(fl32(cost + fl32(kappa_cost * sqrtf(cost_var))))  if kappa_cost > 0;  clip1(c) = c > 1 ? 1 : c
 * so kappa_cost > 0 is accepted with a static cost once the votes are given.  next_obs, rew, rew_var, dkl_path, ep_var*,
 * term_pred, term_votes and cost_logit do not depend on any of it.  With CMBPO_TASK_LEARNED_COST the static cost rule is skipped
 * as it always was: cost, cost_var and kappa_cost are the learned column's, cost_members != CMBPO_TERM_ELITE or a non-NULL
 * cost_votes is refused, done_members and done_votes stay available. */
#define CMBPO_VOTE_MEAN 3     /* cost_members only: the expected indicator votes / E */
typedef struct cmbpo_rule_votes {
  int32_t done_members;   /* CMBPO_TERM_ELITE / _ANY / _MAJORITY */
  int32_t cost_members;   /* CMBPO_TERM_ELITE / _ANY / _MAJORITY / CMBPO_VOTE_MEAN */
  uint8_t *done_votes;    /* [.] or NULL */
  uint8_t *cost_votes;    /* [.] or NULL */
} cmbpo_rule_votes_t; /* 24 bytes */
/* cmbpo_fakeenv_post_term_draws's arguments plus the votes: the superset, every feature optional.  rv == NULL is exactly
 * cmbpo_fakeenv_post_term_draws's call (the same kernel instances with the same argument blocks, no further launch).  With rv,
 * one more kernel (csrc/rule_votes.hip) runs behind the post kernel on the same stream and overwrites d_term, d_cost and, with
 * the disagreement on and a static cost, d_cost_var.  It recovers learned_done from the head's own outputs: with th != NULL both
 * th->term_pred and th->term_votes are required.  Beside cmbpo_fakeenv_post_term_draws's checks: done_members in 0..2,
 * cost_members in 0..3 (CMBPO_VOTE_MEAN for the cost only), the learned-cost refusal above, ensemble <= 8 (the votes of a row
 * live in a byte mask) -- each refused with a message naming the votes, before any HIP call. */
int cmbpo_fakeenv_post_votes(int task, int ensemble, int obs_dim, int act_dim,
                             const float *d_mean, const float *d_var, int ld_rows,
                             const float *d_obs, const float *d_act,
                             const int32_t *d_elite, const int32_t *d_row_idx,
                             const int32_t *d_n_rows, int n_rows, float *d_next_obs,
                             float *d_rew, uint8_t *d_term, float *d_cost,
                             float *d_dkl_path, float *d_ep_var_mean,
                             float *d_ep_var, const float *d_xi,
                             float kappa_rew, float kappa_cost,
                             float *d_rew_var, float *d_cost_var,
                             const cmbpo_term_head_t *th, const cmbpo_cost_head_t *ch,
                             const float *d_term_thr, const cmbpo_rule_votes_t *rv, void *stream);

/* ------------------------------------------------------------------------ *
 * Device-resident rollout state: the fused counterpart of ModelSampler
 * (samplers/model_sampler.py:203-444) + ModelBuffer (buffers/modelbuffer.py).
 * Every array is owned by the caller; branch slots never move (mask-in-place
 * + an ordered alive list instead of the reference's per-step compaction,
 * samplers/model_sampler.py:300-311).  Buffers are TIME-MAJOR [T][B][...]
 * so that per-step stores and the per-branch GAE scan are both coalesced; the
 * reference's (B, T) order is restored by cmbpo_buffer_flatten (get()).
 * ------------------------------------------------------------------------ */
typedef struct cmbpo_rollout {
  int32_t B, T, obs_dim, act_dim;
  int32_t max_path_length;  /* sampler horizon (model_sampler.py:352)          */
  int32_t ptr;              /* column of the next store (modelbuffer.py:135)   */
  int32_t uncertainty_mode; /* rollout_mode == 'uncertainty' (:275-279)        */
  int32_t rank, world;      /* shard id / count (budget rule offsets)          */
  int64_t max_samples;      /* budget of sample(max_samples); 0: none (the reference tests `if max_samples:`, so a
                             * negative budget early-terminates every surviving branch, model_sampler.py:282-287) */
  double dkl_lim;           /* set_rollout_dkl (:169-170)                      */
  double gamma, lam, cost_gamma, cost_lam; /* modelbuffer.py:41-51             */
  /* ordered alive list (ascending slot ids) and scalars */
  int32_t *alive_idx;       /* [B] current list                                */
  int32_t *alive_idx_out;   /* [B] list written by cmbpo_rollout_compact       */
  int32_t *iscal;           /* [32] see CMBPO_I_*                              */
  double *dscal;            /* [32] see CMBPO_D_*                              */
  int32_t use_host_budget;  /* 1: take the two fields below instead of local counts */
  int32_t host_rank_off;    /* surviving rows on lower ranks (global index order)   */
  int64_t host_excess;      /* global rows to early-terminate this step              */
  uint8_t *alive;           /* [B] !terminated_paths_mask                      */
  uint8_t *fin_code;        /* [B] 0 keep, 1 finish w/ bootstrap, 2 terminal   */
  int32_t *len;             /* [B] populated entries of the branch             */
  /* per-step values, slot indexed */
  const float *cur_obs;     /* [B,obs]  observation the step starts from       */
  const float *next_obs;    /* [B,obs]                                         */
  const float *act_t, *logp_t, *mu_t, *ls_t; /* [B,act] / [B]                  */
  const float *v_t, *vc_t;  /* [B] critics at cur_obs                          */
  const float *v_n, *vc_n;  /* [B] critics at next_obs                         */
  const float *rew_t, *cost_t, *dkl_t, *epv_t; /* [B]                          */
  const uint8_t *term_t;    /* [B]                                             */
  double *dkl_acc, *path_ret, *path_cost, *path_dyn_var; /* [B] (float64 in the reference) */
  double *store_part;   /* [ceil(B / 64)][8] per-workgroup sampler sums of cmbpo_rollout_store (scratch) */
  /* time-major buffers */
  float *obs_buf, *act_buf, *mu_buf, *ls_buf;             /* [T,B,dim]         */
  float *rew_buf, *val_buf, *cost_buf, *cval_buf, *logp_buf; /* [T,B]          */
  float *adv_buf, *ret_buf, *cadv_buf, *cret_buf;         /* [T,B]             */
  /* stochastic transitions (cmbpo_fakeenv_post_noise): NULL = off */
  const float *xi;          /* [B,obs] N(0,1) draws of the step, slot indexed   */
  int64_t xi_stride;        /* cmbpo_rollout_run: step k of a call reads xi + k * xi_stride */
} cmbpo_rollout_t;

/* iscal slots */
#define CMBPO_I_N_ALIVE 0   /* length of alive_idx                              */
#define CMBPO_I_N_UNC 1     /* too-uncertain rows of this step (local)          */
#define CMBPO_I_N_FIN_PRE 2 /* rows finished before the store                   */
#define CMBPO_I_N_STORED 3  /* rows stored this step                            */
#define CMBPO_I_N_ALIVE_OUT 4 /* length of alive_idx_out after compact          */
#define CMBPO_I_SIZE 5      /* populated entries in the buffer (pool.size)      */
#define CMBPO_I_N_FIN_POST 6 /* rows finished after the store (horizon / terminal) */
/* (8 .. 11: the row other shards gather -- {n_alive, n_unc, total_samples, 0}) */
#define CMBPO_I_HALT 12     /* cmbpo_rollout_run's look-ahead: the step just taken met a stop test, the step enqueued behind it is void */
#define CMBPO_I_N_EFF 13    /* ... and the row count that step's forward kernels read (0 once halted)   */
/* dscal slots (sampler accumulators, model_sampler.py:314-333) */
#define CMBPO_D_TOTAL_SAMPLES 0
#define CMBPO_D_TOTAL_COST 1
#define CMBPO_D_TOTAL_REW 2
#define CMBPO_D_TOTAL_VS 3
#define CMBPO_D_TOTAL_CVS 4
#define CMBPO_D_TOTAL_DKL 5
#define CMBPO_D_TOTAL_DYN_EP_VAR 6
#define CMBPO_D_MAX_DKL 7
#define CMBPO_D_MAX_PATH_RETURN 8
#define CMBPO_D_DKL_SUM_T 9     /* sum of dkl_t over the rows stepped this call */
#define CMBPO_D_STEP_MAX_DKL 10
#define CMBPO_D_SUM_PATH_RET 11
#define CMBPO_D_SUM_PATH_COST 12
#define CMBPO_D_TOTAL_REW_VAR 13   /* sums of rew_var_t / cost_var_t over the stored rows (cmbpo_rollout_disagreement_attach; */
#define CMBPO_D_TOTAL_COST_VAR 14  /* the reference declares _total_rew_var / _total_cost_var and never fills them)          */
#define CMBPO_D_TOTAL_V_VAR 15     /* sums of v_var / vc_var (the critics' member variance at the stored rows' observations)   */
#define CMBPO_D_TOTAL_VC_VAR 16    /* over the stored rows (cmbpo_rollout_value_disagreement_attach)                           */

/* ModelSampler.reset + ModelBuffer.reset (model_sampler.py:203-237,
 * modelbuffer.py:53-98): all B branches alive, lists / accumulators zeroed.
 * Does not touch the big buffers (no realloc, no memset: entries are only
 * read below `len`). */
int cmbpo_rollout_reset(const cmbpo_rollout_t *r, void *stream);

/* Uncertainty test on accumulated + new DKL BEFORE storing and the budget
 * early-termination of the first n surviving rows by index
 * (model_sampler.py:275-287) -> fin_code, counters. */
int cmbpo_rollout_decide(const cmbpo_rollout_t *r, void *stream);
/* Counting half of the above only: writes iscal[8..11] = {n_alive, n_unc,
 * total_samples, 0}, the row a sharded run all-gathers; the host turns the
 * gathered rows into (host_excess, host_rank_off) for cmbpo_rollout_decide
 * (budget rule across shards; dist.budget_plan). */
int cmbpo_rollout_count(const cmbpo_rollout_t *r, void *stream);

/* ModelBuffer.finish_path_multiple (modelbuffer.py:138-182) = reward + cost GAE
 * (utilities/utils.py:184-188 discount_cumsum, float64 recurrence) for the rows
 * selected by `mode`, then marks them terminated:
 *   0 PRE : rows with fin_code != 0, bootstrap V/VC of the pre-step obs (:290,401-407)
 *   1 POST: stored rows; horizon (path_length >= max_path_length-1, :350-353) finishes
 *           all with V/VC(next_obs); else env-terminal rows with last_val = 0 but
 *           last_cval = VC(next_obs) (:357-367)
 *   2 ALL : finish_all_paths (:418-444), bootstrap V/VC of the current obs. */
int cmbpo_rollout_finish(const cmbpo_rollout_t *r, int mode, void *stream);

/* ModelBuffer.store_multiple for the surviving rows at column ptr + the sampler
 * accumulators (modelbuffer.py:114-135, model_sampler.py:314-346). */
int cmbpo_rollout_store(const cmbpo_rollout_t *r, void *stream);

/* Rebuild the ordered alive list from `alive` (replaces the boolean-mask
 * compaction of model_sampler.py:300-311,361-372). */
int cmbpo_rollout_compact(const cmbpo_rollout_t *r, void *stream);
/* The whole step in one call (single-GPU jobs without a cross-shard budget exchange): cmbpo_policy_forward ->
 * cmbpo_ens_forward -> cmbpo_fakeenv_post -> decide -> finish(PRE) -> store -> cmbpo_ens_predict_mean x 2 at next_obs ->
 * finish(POST), every buffer taken from *r (slot-indexed d_eps [B, act], d_elite [B]; scratch d_mean / d_var
 * [E, B, model out_dim]: obs + 1, or obs + 2 with CMBPO_TASK_LEARNED_COST in `task`).  n_alive = the host's copy of iscal[CMBPO_I_N_ALIVE].
 * (With a cmbpo_cost_head_t attached -- cmbpo_rollout_cost_head_attach below -- the post-processing is cmbpo_fakeenv_post_cost.)
 * With r->xi != NULL the post-processing is cmbpo_fakeenv_post_noise on those draws; with a cmbpo_disagreement_t attached it is
 * cmbpo_fakeenv_post_disagreement (with or without draws); with a cmbpo_value_disagreement_t attached the critics at next_obs are
 * cmbpo_critic_pair_predict_var (refused before the first launch unless cmbpo_critic_pair_supported(v, vc)). */
/* Small rollout batches: decide + finish(PRE) + store (+ its statistics) as one single-workgroup launch for up to
 * cmbpo_rollout_book_pre_max_rows() alive rows (same decisions and per-branch arithmetic as the separate calls;
 * single-rank path).  cmbpo_rollout_step uses it by itself. */
int cmbpo_rollout_book_pre_max_rows(void);
int cmbpo_rollout_book_pre(const cmbpo_rollout_t *r, int n_alive, void *stream);
/* ... and finish(POST) + the compaction likewise: the ordered alive list of the survivors is ALWAYS written to
 * alive_idx_out (iscal[CMBPO_I_N_ALIVE] updated), so the host swaps the two lists after every such step.
 * cmbpo_rollout_step returns 1 (instead of 0) when it took this path. */
int cmbpo_rollout_book_post(const cmbpo_rollout_t *r, int n_alive, void *stream);
/* The step's counters and accumulators (iscal[32] | dscal[32], one 384-byte block) into host memory + a stream
 * synchronisation: the one host sync of a rollout step (the reference's per-step `alive_ratio`,
 * samplers/model_sampler.py:371-375). */
int cmbpo_rollout_read_scalars(const cmbpo_rollout_t *r, void *h_out384, void *stream);
int cmbpo_rollout_step(const cmbpo_rollout_t *r, int n_alive, cmbpo_mlp_t *policy, cmbpo_mlp_t *model,
                       cmbpo_mlp_t *v, cmbpo_mlp_t *vc, int task, int ensemble, const float *d_eps,
                       const int32_t *d_elite, float *d_mean, float *d_var, void *stream);

/* Several steps in one call (single-rank path; replaces the body of the rollout loop of algorithms/cmbpo.py:352-360
 * around ModelSampler.sample): step -> counters -> swap of the alive lists and of the cur / next arrays, repeated
 * until max_steps, no branch alive, at most min_alive alive (`alive_ratio <= 0.1`), total_samples >= stop_total
 * (stop_total = NaN: no such test; a threshold <= 0 is reached by the first step, as in the reference's
 * `_total_samples + samples_added >= .99 * approx_model_batch`) or a full buffer.  *r is left as the caller of cmbpo_rollout_step would leave it.
 * d_eps / d_elite: the draws of the first step; step k reads them k * eps_stride / k * elite_stride elements on, and, with
 * r->xi != NULL, the transition noise at r->xi + k * r->xi_stride (the field itself is left as it was found).
 * h_scalars: [max_steps][384 bytes] of host memory (pinned), the counters of every step taken (iscal | dscal);
 * *list_swaps = how often alive_idx / alive_idx_out changed places. */
int cmbpo_rollout_run(cmbpo_rollout_t *r, int n_alive, cmbpo_mlp_t *policy, cmbpo_mlp_t *model, cmbpo_mlp_t *v,
                      cmbpo_mlp_t *vc, int task, int ensemble, const float *d_eps, const int32_t *d_elite,
                      long eps_stride, long elite_stride, float *d_mean, float *d_var, int max_steps,
                      double stop_total, int min_alive, void *h_scalars, int *steps_done, int *n_alive_out,
                      int *list_swaps, void *stream);

/* Inverse-variance-weighted GAE for imagined rollouts: the weighted branch of the reference's
 * discount_cumsum(x, discount, lam, weights=..., axis=-1) (utilities/utils.py:189-208) with the weights
 *   w[u] = 1 / (eps + sum_{s<=u} (double)epv_s)       (the branch's accumulated epistemic variance, path_dyn_var)
 * applied to the reward and the cost deltas of every finished branch (DESIGN 3k has the recurrence).  cmbpo_rollout_t
 * stays as it is; the feature's arrays travel beside it: attach them to a buffer (the key is r->iscal) and every call
 * above that stores (cmbpo_rollout_store, _book_pre, _step, _run) writes path_dyn_var into cumvar_buf[ptr * B + b] and
 * every call that finishes paths (cmbpo_rollout_finish, _book_pre, _book_post, _step, _run) takes the weighted branch.
 * Device pointers, owned by the caller, valid until the detach; attach again after any of them or r->iscal moved.
 * lam_vec[0] = 1, lam_vec[u] = lam * lam_vec[u - 1]; lam_pow[L] = lam ** L (the host's pow); clam_*: the same for cost_lam.
 * Constant weights do not give plain GAE: the reference folds the weight beyond the last step into the last one. */
typedef struct cmbpo_iv_gae {
  double *cumvar_buf;            /* [T,B] */
  const double *lam_vec, *lam_pow, *clam_vec, *clam_pow;   /* [T], [T+1], [T], [T+1] */
  double eps;
} cmbpo_iv_gae_t;
int cmbpo_rollout_iv_attach(const cmbpo_rollout_t *r, const cmbpo_iv_gae_t *iv);
/* Back to the un-weighted recurrence (no error when nothing was attached). */
int cmbpo_rollout_iv_detach(const cmbpo_rollout_t *r);

/* Ensemble disagreement on reward and cost along imagined rollouts, and the pessimistic rollout made from it.  Like the
 * weighted GAE the state travels beside an unchanged cmbpo_rollout_t (key: r->iscal).  Attached,
 *   - every call that post-processes (cmbpo_rollout_step, _run) runs cmbpo_fakeenv_post_disagreement with kappa_rew /
 *     kappa_cost into rew_var_t / cost_var_t, so rew_t / cost_t -- and with them the buffers, the sums and the GAE -- are the
 *     penalised values; the alive masks and the budget rule do not depend on them;
 *   - every call that stores (cmbpo_rollout_store, _book_pre, _step, _run) adds, for the stored rows, rew_var_t[b] to
 *     path_rew_var[b] and cost_var_t[b] to path_cost_var[b] (float64, in step order) and the step's sums over those rows to
 *     dscal[CMBPO_D_TOTAL_REW_VAR] / [CMBPO_D_TOTAL_COST_VAR] (per-workgroup partial sums in `part`, added in a fixed order);
 *   - cmbpo_rollout_reset zeroes path_rew_var / path_cost_var.
 * A caller that post-processes by itself passes the same arrays to cmbpo_fakeenv_post_disagreement.  Device pointers, owned by
 * the caller, valid until the detach; attach again after any of them or r->iscal moved.  part: 2 * ceil(B / 64) doubles. */
typedef struct cmbpo_disagreement {
  float kappa_rew, kappa_cost;
  float *rew_var_t, *cost_var_t;          /* [B] this step, slot indexed */
  double *path_rew_var, *path_cost_var;   /* [B] sums over the branch's stored steps */
  double *part;                           /* scratch for per-workgroup partial sums, sized by the builder */
} cmbpo_disagreement_t;
int cmbpo_rollout_disagreement_attach(const cmbpo_rollout_t *r, const cmbpo_disagreement_t *dg);
/* Back to the elite member's reward and cost, nothing measured (no error when nothing was attached). */
int cmbpo_rollout_disagreement_detach(const cmbpo_rollout_t *r);

/* Critic disagreement along imagined rollouts, and the pessimistic value bootstraps made from it.  The state travels beside
 * an unchanged cmbpo_rollout_t in the same table (key: r->iscal).  Attached,
 *   - cmbpo_rollout_step / _run evaluate the critics at next_obs with cmbpo_critic_pair_predict_var(kappa_v, kappa_vc) into
 *     v_n / vc_n and v_var / vc_var, so the values every later store, bootstrap and GAE reads are the penalised ones; they
 *     refuse (-1, before the first launch of the step) critics for which cmbpo_critic_pair_supported is false;
 *   - every call that stores (cmbpo_rollout_store, _book_pre, _step, _run) adds v_var[b] / vc_var[b] over the stored rows to
 *     dscal[CMBPO_D_TOTAL_V_VAR] / [CMBPO_D_TOTAL_VC_VAR] (per-workgroup partial sums in `part`, added in a fixed order).  The
 *     store of a step runs BEFORE that step's critic launch: what it reads is the variance at cur_obs, written by the previous
 *     step's launch or by the caller's evaluation at the start states -- no swap of the two arrays is needed.
 * A caller that evaluates the critics by itself (the start states; a step made of separate calls) passes the same arrays and
 * coefficients to cmbpo_critic_pair_predict_var.  Alive masks, the budget rule, next_obs, rewards, costs and DKL do not depend
 * on the feature.  Device pointers, owned by the caller, valid until the detach; attach again after any of them or r->iscal
 * moved.  part: 2 * ceil(B / 64) doubles; part == NULL means nothing is attached. */
typedef struct cmbpo_value_disagreement {
  float kappa_v, kappa_vc;
  float *v_var, *vc_var;                  /* [B] slot indexed */
  double *part;                           /* scratch for per-workgroup partial sums */
} cmbpo_value_disagreement_t;
int cmbpo_rollout_value_disagreement_attach(const cmbpo_rollout_t *r, const cmbpo_value_disagreement_t *vd);
/* Back to the members' mean, nothing measured (no error when nothing was attached). */
int cmbpo_rollout_value_disagreement_detach(const cmbpo_rollout_t *r);

/* The learned termination head along imagined rollouts: a copy of *th travels beside an unchanged cmbpo_rollout_t in the same
 * table (key: r->iscal).  Attached, cmbpo_rollout_step / _run post-process with cmbpo_fakeenv_post_term (with or without
 * draws, with or without an attached cmbpo_disagreement_t), so term_t -- and with it every finish decision -- is
 * rule_done || learned_done; before the first launch of a step they require model->out_dim == obs + 1 + learned cost + 1 and
 * refuse (-1) any other width with a message naming the termination head.  term_pred / term_votes: [B] slot indexed, this
 * step's values, or NULL.  Owned by the caller, valid until the detach.  The same checks as cmbpo_fakeenv_post_term. */
int cmbpo_rollout_term_head_attach(const cmbpo_rollout_t *r, const cmbpo_term_head_t *th);
/* Back to the rules alone (no error when nothing was attached). */
int cmbpo_rollout_term_head_detach(const cmbpo_rollout_t *r);
/* Sampled terminations along imagined rollouts: {d_thr, step_stride} travels in the same table.  Attached, cmbpo_rollout_step /
 * _run post-process with cmbpo_fakeenv_post_term_draws: cmbpo_rollout_step reads d_thr, step j of a cmbpo_rollout_run call reads
 * d_thr + j * step_stride (floats; as the run reads xi + j * xi_stride).  d_thr: [B] per step, slot indexed, owned by the caller,
 * valid until the detach; d_thr == NULL detaches (no error when nothing was attached).  Draws attached without a termination
 * head are refused (-1) before the first launch of a step, with a message naming both.  Nothing else of a step or of the native
 * loop changes.  Checked here: the struct, and step_stride >= 0. */
int cmbpo_rollout_term_draws_attach(const cmbpo_rollout_t *r, const float *d_thr, long step_stride);

/* The cost head's reading along imagined rollouts: a copy of *ch travels beside an unchanged cmbpo_rollout_t in the same table.
 * Attached, cmbpo_rollout_step / _run post-process with cmbpo_fakeenv_post_cost (with whatever else is attached), so cost_t --
 * and with it cost_buf, the cost GAE, path_cost and the cost totals -- holds probabilities; with kind 1 they refuse (-1), before
 * the first launch of a step, a task without CMBPO_TASK_LEARNED_COST and a model whose out_dim is not obs + 2 (+ 1 with a
 * termination head), with a message naming the cost head.  cost_logit: [B] slot indexed, this step's raw logits, or NULL; owned
 * by the caller, valid until the detach.  Checked here: kind in {0, 1} and a finite logit_shift. */
int cmbpo_rollout_cost_head_attach(const cmbpo_rollout_t *r, const cmbpo_cost_head_t *ch);
/* Back to the magnitude reading (no error when nothing was attached). */
int cmbpo_rollout_cost_head_detach(const cmbpo_rollout_t *r);

/* Ensemble-voted static rules along imagined rollouts: a copy of *rv travels beside an unchanged cmbpo_rollout_t in the same
 * table.  Attached, cmbpo_rollout_step / _run post-process with cmbpo_fakeenv_post_votes (with whatever else is attached), so
 * term_t -- and with it every finish decision -- and cost_t -- and with it cost_buf, the cost GAE, path_cost and the cost
 * totals -- are the voted ones, and with a cmbpo_disagreement_t attached cost_var_t and its totals carry the static cost's spread
 * (kappa_cost > 0 is then accepted with a static cost).  done_votes / cost_votes: [B] slot indexed, this step's values, or NULL;
 * owned by the caller, valid until the detach.  With a termination head attached its term_pred / term_votes are required, and
 * with CMBPO_TASK_LEARNED_COST cost_members != CMBPO_TERM_ELITE or cost_votes is refused: both at the step, with the post step's
 * messages.  Checked here: the two modes' ranges.  rv == NULL detaches, as cmbpo_rollout_rule_votes_detach does (no error when
 * nothing was attached).  Nothing else of a step or of the native loop changes. */
int cmbpo_rollout_rule_votes_attach(const cmbpo_rollout_t *r, const cmbpo_rule_votes_t *rv);
int cmbpo_rollout_rule_votes_detach(const cmbpo_rollout_t *r);

/* ModelBuffer.get (modelbuffer.py:184-226): d_offsets[B+1] = exclusive scan of
 * len; d_stats[8] = {n, adv_mean, adv_std, cadv_mean, ret_mean, cret_mean}
 * (two-pass mean / std of utilities/mpi_tools.py:71-92).  With d_gstats
 * (global statistics after an all-reduce) NULL the local ones are used. */
int cmbpo_buffer_offsets(const cmbpo_rollout_t *r, int32_t *d_offsets, void *stream);
int cmbpo_buffer_moments(const cmbpo_rollout_t *r, int pass, double *d_stats, void *stream);
/* The same offsets and statistics on ONE GPU as two launches (four beyond 32 768 branches, where the fold of the
 * workgroups' partial sums is a launch of its own; r->world <= 1; replaces cmbpo_buffer_offsets + the four
 * cmbpo_buffer_moments passes of ModelBuffer.get, buffers/modelbuffer.py:184-204 / utilities/mpi_tools.py:71-92): the
 * scan of the path lengths and the first moments in one pass over the buffers, the offsets and the centred second
 * moment in another; the last workgroup of each launch adds the workgroups' partial sums in a fixed order. */
int cmbpo_buffer_prepare(const cmbpo_rollout_t *r, int32_t *d_offsets, double *d_stats, void *stream);
/* Flatten in branch-major, time-minor order into the 12-array list
 * [obs, act, adv, cadv, ret, cret, logp, val, cval, cost, log_std, mu]
 * (modelbuffer.py:212-218), normalising adv by (mean, std + 1e-8) and centring
 * cadv (:198-204).  d_out[12] are device pointers sized for offsets[B] rows. */
int cmbpo_buffer_flatten(const cmbpo_rollout_t *r, const int32_t *d_offsets,
                         const double *d_stats, float *const *h_out12, void *stream);
/* Trust weights of the stored entries in the order of cmbpo_buffer_flatten:
 * d_out[offsets[b] + t] = (float)(ref_var / (ref_var + cumvar[t][b])), t < len[b],
 * computed in float64 from the accumulated model variance that the
 * inverse-variance GAE keeps (cmbpo_rollout_iv_attach; an error without it):
 * 1 where the model has accumulated no variance, 1/2 at ref_var (> 0, finite).
 * d_out holds offsets[B] floats. */
int cmbpo_buffer_trust_weights(const cmbpo_rollout_t *r, const int32_t *d_offsets, double ref_var, float *d_out,
                               void *stream);

/* ------------------------------------------------------------------------ *
 * CPO trust-region update: the policy-graph fetches of CPOAgent.update_pi
 * (policies/cpo_policy.py:153-300) as fused HIP kernels.  All results are RAW
 * SUMS over the samples of this call (the caller divides by the global sample
 * count after an all-reduce, instead of mpi_avg's equal-shard assumption,
 * utilities/mpi_tools.py:67-69).  Parameter vectors are flat float32[P] in the
 * order of get_vars('pi') (network/ac_network.py:35-36): W0[obs,H], b0,
 * W1[H,H], b1, W2[H,act], b2, log_std.  Hidden width H: 128 (every shipped
 * experiment; both matrix paths) or 256 (configs/baseconfig/base.py:7, the
 * default: fp32 MFMAs whatever cmbpo_set_pi_matrix_path says); obs <= 64,
 * act <= 32.
 * ------------------------------------------------------------------------ */
typedef struct cmbpo_pi cmbpo_pi_t;

typedef struct cmbpo_pi_batch {   /* the actor feed (actor_phs, cpo_policy.py:479-487) */
  int32_t n, obs_dim, act_dim;
  const float *obs;        /* [n,obs]                                       */
  const float *act;        /* [n,act]                                       */
  const float *adv;        /* [n]                                           */
  const float *cadv;       /* [n]                                           */
  const float *logp_old;   /* [n]                                           */
  const float *cost;       /* [n]   cur_cost_ph                             */
  const float *mu_old;     /* [n,act] pi_info 'mu'                          */
  const float *logstd_old; /* [n,act] pi_info 'log_std'                     */
} cmbpo_pi_batch_t;

int cmbpo_pi_create(cmbpo_pi_t **out, int obs_dim, int hidden, int act_dim);
void cmbpo_pi_destroy(cmbpo_pi_t *h);
int cmbpo_pi_num_params(const cmbpo_pi_t *h);

/* set_pi_params (utilities/trust_region.py:21-25, cpo_policy.py:559): d_flat is
 * a DEVICE vector; packing into MFMA fragment order happens on the device. */
int cmbpo_pi_set_params(cmbpo_pi_t *h, const float *d_flat, void *stream);

/* flat_g / flat_b with their losses (cpo_policy.py:169-171, 522-555):
 * which = 0: d_vec = sum_n grad(-ratio*adv)   (divide by N, subtract ent_reg on
 *            the log_std block, to get flat_g); which = 1: sum_n grad(ratio*cadv).
 * d_sums[8] = {n, sum ratio*adv, sum ratio*cadv, -, sum cost}. */
int cmbpo_pi_loss_grad(cmbpo_pi_t *h, const cmbpo_pi_batch_t *b, int which,
                       float *d_vec, double *d_sums, void *stream);

/* hessian_vector_product(d_kl, pi_params) (utilities/trust_region.py:15-19) in
 * its Gauss-Newton / Fisher form: d_vec = sum_n J^T diag(1/(exp(2 ls_old)+1e-8))
 * J v on the MLP block and sum_n 2 exp(2 ls)/(exp(2 ls_old)+1e-8) * v on log_std.
 * The caller divides by N and adds damping_coeff * v (cpo_policy.py:550-552). */
int cmbpo_pi_fvp(cmbpo_pi_t *h, const cmbpo_pi_batch_t *b, const float *d_v,
                 float *d_vec, void *stream);

/* The reference re-feeds the batch through the whole policy graph for every one
 * of the 10-20 Hx evaluations of an update (cpo_policy.py:168, 550-552), although
 * parameters and batch are fixed from flat_g to the end of the CG solves.  With
 * enable != 0, cmbpo_pi_loss_grad saves the two hidden activation images of the
 * batch (1 KB per sample, owned by the handle, grow-only) and every later
 * Fisher-vector product on the same (obs pointer, n) reads them instead of
 * recomputing the forward chain -- bit-identical results.  The saved images are
 * dropped by cmbpo_pi_set_params and by any call of this function; the caller
 * must not change the batch in place between loss_grad and the products.  Off by
 * default; if the memory cannot be had the products silently recompute. */
int cmbpo_pi_keep_activations(cmbpo_pi_t *h, int enable);
/* Fisher-vector product launches that read saved activations so far (a launch
 * captured into the CG graph counts once); diagnostics / tests. */
long cmbpo_pi_saved_activation_uses(const cmbpo_pi_t *h);
/* Workgroups (= partial vectors) of the last loss_grad / fvp / eval / ppo_grad
 * launch on this handle, 0 before the first; with fewer workgroups than 32-sample
 * tiles each persistent workgroup walked more than one tile.  Read-only; tests. */
int cmbpo_pi_last_grid(const cmbpo_pi_t *h);
/* Per-sample weights of every later launch on this handle (loss_grad, fvp, eval,
 * the CG calls, ppo_grad, ppo_run): a sample of weight w counts as w copies of
 * itself.  Every per-sample sum becomes a weighted sum: d_sums[0] = sum w,
 * [1] = sum w ratio adv, [2] = sum w ratio cadv, [3] = sum w kl, [4] = sum w cost
 * (first-order sums: [1] objective, [5] clipped-away, [6] ratio adv, each times
 * w); vectors are sum w grad / sum w J^T M J v, and callers divide by sum w
 * where they divided by n.  d_w: n finite floats >= 0 with a positive sum, on
 * the device, kept alive by the caller; NULL clears the weights (n ignored).
 * They stay with the handle until cleared or replaced; a launch whose batch has
 * another n returns CMBPO_EINVAL before any HIP call.  Nothing is enqueued; saved
 * activations do not depend on the weights and are kept; a cached CG graph is
 * re-captured when the pointer changes.  Without weights every launch runs the
 * kernel it ran before this function existed. */
int cmbpo_pi_set_sample_weights(cmbpo_pi_t *h, const float *d_w, int n, void *stream);

/* Arithmetic of the policy kernels' matrix products (forward, JVP, backward and
 * weight-gradient): 1 (default) = three f16 MFMAs on two-piece operands (11 + 1 +
 * 11 mantissa bits, fp32 accumulation: the error of a product stays at fp32's,
 * see DESIGN.md 3a), 0 = fp32 MFMAs throughout (round 1). */
void cmbpo_set_pi_matrix_path(int path);
int cmbpo_get_pi_matrix_path(void);

/* [d_kl, pi_loss, surr_cost] at the current parameters (set_and_eval,
 * cpo_policy.py:278-280): d_sums[8] = {n, sum ratio*adv, sum ratio*cadv,
 * sum_n sum_a kl, sum cost}. */
int cmbpo_pi_eval(cmbpo_pi_t *h, const cmbpo_pi_batch_t *b, double *d_sums,
                  void *stream);

/* CPOBuffer.finish_path (buffers/cpobuffer.py:179-207) / any set of contiguous
 * paths cut out of flat [N] arrays by d_offsets[n_paths+1]: reward + cost GAE
 * (utilities/utils.py:184-188) with per-path bootstraps.  d_f64_mask (may be
 * NULL) bit0/bit1: compute the reward/cost deltas in float64, which is what
 * np.append does to the float32 buffers when the bootstrap is not float32
 * (the np.zeros((1,)) of samplers/cpo_sampler.py:205-212). */
int cmbpo_gae_segments(int n_paths, const int32_t *d_offsets, const float *d_rew,
                       const float *d_val, const float *d_cost, const float *d_cval,
                       const float *d_last_val, const float *d_last_cval,
                       const uint8_t *d_f64_mask, double gamma, double lam,
                       double cost_gamma, double cost_lam, float *d_adv,
                       float *d_ret, float *d_cadv, float *d_cret, void *stream);

/* CPOBuffer.get normalisation (buffers/cpobuffer.py:261-268): in place
 * adv = (adv - mean) / (std + 1e-8), cadv -= mean(cadv), two-pass statistics of
 * utilities/mpi_tools.py:71-87.  d_stats[16]: [0] n [1] adv_mean [2] adv_std
 * [3] cadv_mean. */
int cmbpo_adv_normalize(int n, float *d_adv, float *d_cadv, double *d_stats, void *stream);

/* Parameter-vector algebra of the update kept on the device (csrc/vec_ops.hip).
 * cg_init / cg_step are utilities/trust_region.py:32-45 (x = 0, r = p = b; then per
 * iteration z = hp_sum * inv_n + damping * p, alpha = rr / (p.z + 1e-8), x += alpha p,
 * r -= alpha z, p = r + (rr_new / rr) p); d_scal[0] carries r.r.  d_hp_sum is the raw
 * cmbpo_pi_fvp output for direction d_p. */
int cmbpo_cg_init(int P, const float *d_b, float *d_x, float *d_r, float *d_p, double *d_scal, void *stream);
int cmbpo_cg_step(int P, const float *d_hp_sum, double inv_n, float damping, float *d_x, float *d_r,
                  float *d_p, double *d_scal, void *stream);
/* The whole solve x = cg(Hx, b) in one call (single-GPU jobs): cg_init, then `iters` times [cmbpo_pi_fvp on direction
 * d_p into d_vec, cg_step].  With use_graph != 0 the iterations after the first are captured into a hipGraph that is
 * cached per handle (re-captured when a pointer / size changes); cmbpo_pi_cg_release drops it. */
int cmbpo_pi_cg_solve(cmbpo_pi_t *h, const cmbpo_pi_batch_t *b, const float *d_b, double inv_n, float damping,
                      int iters, float *d_x, float *d_r, float *d_p, float *d_vec, double *d_scal,
                      int use_graph, void *stream);
void cmbpo_pi_cg_release(cmbpo_pi_t *h);
/* The iteration cmbpo_pi_cg_solve repeats: Fisher-vector product of direction d_p (kept as per-workgroup partial
 * vectors), z = Hp / N + damping p, alpha, x, r, beta, p updated by three multi-workgroup kernels with ordered float64
 * dot products.  d_scal[0] = r.r; d_scal[1] < 0 on entry to the first iteration; cmbpo_pi_cg_commit after the last. */
int cmbpo_pi_cg_iter(cmbpo_pi_t *h, const cmbpo_pi_batch_t *b, double inv_n, float damping, float *d_x,
                     float *d_r, float *d_p, double *d_scal, void *stream);
int cmbpo_pi_cg_commit(double *d_scal, void *stream);
long cmbpo_pi_cg_graph_launches(void);   /* graph replays so far; -1: stream capture unavailable, eager loop in use */
long cmbpo_pi_cg_graph_captures(void);   /* graphs captured so far: one per (handle, solution vector) while the arguments repeat */
/* d_out = a * d_x + b * d_y (d_y may be NULL): Hx = hvp / N + damping v, the step x = (v + nu w) / (lam + eps)
 * (policies/cpo_policy.py:266) and the trial parameters old - step * x (:278). */
int cmbpo_vec_lincomb(int P, float a, const float *d_x, float b, const float *d_y, float *d_out, void *stream);
/* d_out[k] = sum_i x_k[i] * y_k[i], k < n <= 8 (q, r, s, b.b of policies/cpo_policy.py:212-226); h_x / h_y are
 * host arrays of device pointers. */
int cmbpo_vec_dots(int P, int n, const float *const *h_x, const float *const *h_y, double *d_out, void *stream);

/* ---- first-order penalised policy updates (PPO-Lagrangian; the `first_order` family that the reference's Agent declares,
 * policies/cpo_policy.py:30-123, and its graph builder leaves unimplemented, :568-569) -------------------------------
 * pi_objective = mean(clipped_adv ? min(ratio adv, min_adv) : ratio adv) + ent_reg entropy, with
 * min_adv = adv > 0 ? (1 + clip) adv : (1 - clip) adv; with objective_penalized it becomes
 * (pi_objective - penalty mean(ratio cadv)) / (1 + penalty); pi_loss = -pi_objective.
 *
 * d_state: CMBPO_PPO_STATE_DOUBLES doubles on the device, owned by the caller, zeroed once, persistent across updates:
 *   [0]      stop word: 0 while the loop runs; the 1-based index of the iteration whose KL exceeded
 *            kl_margin * target_kl once it has stopped (that iteration's step is not taken)
 *   [1]      steps taken by the current / last cmbpo_pi_ppo_run
 *   [2]      KL of the last iteration that was evaluated
 *   [3]      Adam t of the parameter vector (advances only when a step is taken)
 *   [4..7]   penalty_param, its Adam m, v, t
 *   [8..10]  penalty = softplus(penalty_param), c_r = 1 / (1 + penalty), c_c = penalty / (1 + penalty)
 *   [11..18] the loss sums of the first iteration of the last run (the "pre" measures), layout below
 *   [19..26] the cmbpo_pi_eval sums at the final parameters of the last run (the "post" measures)
 *   [27]     clip count of the last iteration that was evaluated;  [28..31] reserved
 * Loss sums of a MODE_PPO pass, d_sums[8] = {n, sum objective term, sum ratio cadv, sum_n sum_a kl, sum cost,
 * number of samples whose advantage term is clipped away, sum ratio adv (unclipped), 0}; they are added up in
 * workgroup order, so equal inputs give equal bits. */
#define CMBPO_PPO_STATE_DOUBLES 32
typedef struct cmbpo_pi_ppo_cfg {
  float clip_ratio;
  int32_t clipped_adv;          /* 0: plain surrogate ratio adv */
  int32_t objective_penalized;  /* 0: c_r = 1, c_c = 0 whatever d_state holds */
  float ent_reg;
  float pi_lr, beta1, beta2, adam_eps;
  float target_kl, kl_margin;
} cmbpo_pi_ppo_cfg_t;

/* One pass over the batch: d_vec = sum_n grad of the per-sample loss -c_r (active ? ratio adv : 0) + c_c ratio cadv (divide
 * by N and subtract c_r ent_reg on the log_std block to get grad pi_loss), d_sums as above, KL included.  Reads c_r / c_c
 * from d_state and ignores its stop word, which stays set after a run that the gate ended. */
int cmbpo_pi_ppo_grad(cmbpo_pi_t *h, const cmbpo_pi_batch_t *b, const cmbpo_pi_ppo_cfg_t *cfg, const double *d_state,
                      float *d_vec, double *d_sums, void *stream);
/* tf.train.AdamOptimizer on a flat vector: t = ++d_state[3]; lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t);
 * m += (g - m)(1 - beta1); v += (g^2 - v)(1 - beta2); theta -= lr_t m / (sqrt(v) + eps). */
int cmbpo_vec_adam_step(int P, const float *d_g, float *d_m, float *d_v, float *d_theta, double *d_state, float lr,
                        float beta1, float beta2, float eps, void *stream);
/* The learned penalty: cur_cost = d_sums[4] / d_sums[0] * max_path_length (cpo_policy.py:533); penalty_loss =
 * -penalty_param (cur_cost - cost_lim), or -softplus(penalty_param) (cur_cost - cost_lim) with penalty_param_loss == 0;
 * one scalar Adam step (beta 0.9 / 0.999, eps 1e-8), then penalty, c_r, c_c are refreshed.  d_sums == NULL: no step,
 * only the refresh (after penalty_param was written from outside, e.g. from a checkpoint). */
int cmbpo_ppo_penalty_step(double *d_state, const double *d_sums, double cost_lim, double max_path_length,
                           double penalty_lr, int penalty_param_loss, void *stream);
/* `iters` iterations of [MODE_PPO pass -> reduce, / N, entropy term -> gate -> Adam on d_theta -> pack d_theta into the
 * handle], every launch returning at entry once the gate has set the stop word, then cmbpo_pi_eval at the parameters that
 * survived; nothing waits for the host.  d_theta must hold the handle's current parameters (16-byte aligned). */
int cmbpo_pi_ppo_run(cmbpo_pi_t *h, const cmbpo_pi_batch_t *b, const cmbpo_pi_ppo_cfg_t *cfg, float *d_theta,
                     float *d_m, float *d_v, double *d_state, int iters, void *stream);

/* ---- ensemble training (csrc/ens_train.hip) -------------------------
 * The TensorFlow train_op of the reference ensembles (models/pens/pe.py:252-274,312-318:
 * train_loss = sum_e loss_e + sum_l decay_l * l2_loss(W_l), tf.train.AdamOptimizer(lr)) for the
 * two losses the shipped configs use: 'MSPE' on HEAD_PROB handles (pe.py:921-973, dynamics)
 * and 'MSE' on HEAD_DETMEAN handles (pe.py:840-919 with inc_var_loss=False, critics).  The
 * trainer owns the row-major master weights and Adam moments and keeps the handle's packed
 * weights (what cmbpo_ens_forward / cmbpo_ens_predict_mean read) in step with them. */
typedef struct cmbpo_trainer cmbpo_trainer_t;

/* decays[3] = weight_decay of the three FC layers (pe_factory.py:50-55: decay/4, decay/2,
 * decay); max_batch bounds the rows of one step (activations are kept for the backward pass). */
int cmbpo_trainer_create(cmbpo_trainer_t **out, cmbpo_mlp_t *m, int max_batch, float lr,
                         const double *decays);
void cmbpo_trainer_destroy(cmbpo_trainer_t *t);
/* Train loss (PE.finalize, models/pens/pe.py:240-300).  DEFAULT: 'MSPE' (_mspe_loss, :921-973) for probabilistic
 * heads, 'MSE' (_nll_loss(inc_var_loss=False), :840-919) for deterministic ones -- what the shipped configs use.
 * NLL: _nll_loss(inc_var_loss=True) = mean 0.5 exp(-log_var)(mean - t)^2 + mean 0.5 log_var, probabilistic heads
 * only (the class default of PE, pe.py:65).  `self.loss` (cmbpo_trainer_losses) is the same for all of them. */
#define CMBPO_LOSS_DEFAULT 0
#define CMBPO_LOSS_NLL 1
int cmbpo_trainer_set_loss(cmbpo_trainer_t *t, int loss);
/* Host weights in the reference variable layout (W[E][in][out], b[E][out]) -> masters and the
 * handle's packed images; the Adam state is untouched (the reference keeps it across train()
 * calls, pe.py:318).  get_weights copies the masters back (checkpointing, models/pens/pe.py:736-764). */
int cmbpo_trainer_set_weights(cmbpo_trainer_t *t, const float *h_w0, const float *h_b0,
                              const float *h_w1, const float *h_b1, const float *h_w2,
                              const float *h_b2, void *stream);
int cmbpo_trainer_get_weights(cmbpo_trainer_t *t, float *h_w0, float *h_b0, float *h_w1,
                              float *h_b1, float *h_w2, float *h_b2, void *stream);
int cmbpo_trainer_reset_optimizer(cmbpo_trainer_t *t, void *stream);
/* Adam moments (which: 0 = m, 1 = v) in the layout of the weights, and the step count t of
 * lr_t = lr sqrt(1 - b2^t) / (1 - b1^t): optimizer checkpoint / resume (the reference saves
 * optimizer.variables() with the model, pe.py:318,736-764). */
int cmbpo_trainer_get_moments(cmbpo_trainer_t *t, int which, float *h_w0, float *h_b0, float *h_w1,
                              float *h_b1, float *h_w2, float *h_b2, void *stream);
int cmbpo_trainer_set_moments(cmbpo_trainer_t *t, int which, const float *h_w0, const float *h_b0,
                              const float *h_w1, const float *h_b1, const float *h_w2,
                              const float *h_b2, long steps_done, void *stream);
/* TensorStandardScaler.fit result (models/pens/utils.py:119-138) -> the handle, without touching
 * the weights; NULL pairs are left as they are. */
int cmbpo_mlp_set_scalers(cmbpo_mlp_t *m, const float *h_in_mu, const float *h_in_var,
                          const float *h_out_mu, const float *h_out_var, void *stream);
/* One sess.run(train_op) (pe.py:541-563): member e trains on rows d_idx[e * idx_stride + b],
 * b < batch, of d_inputs[N][in_dim] / d_targets[N][target_dim] (inputs[batch_idxs], pe.py:543-547);
 * d_idx == NULL takes rows 0..batch-1 for every member. */
int cmbpo_trainer_step(cmbpo_trainer_t *t, const float *d_inputs, int in_dim,
                       const float *d_targets, int target_dim, const int32_t *d_idx,
                       int idx_stride, int batch, void *stream);
/* The minibatch loop of one epoch (pe.py:541-563): ceil(n_rows / batch) train steps on columns
 * [k * batch, (k + 1) * batch) of the index lists, enqueued without returning to the caller. */
int cmbpo_trainer_epoch(cmbpo_trainer_t *t, const float *d_inputs, int in_dim,
                        const float *d_targets, int target_dim, const int32_t *d_idx,
                        int idx_stride, int n_rows, int batch, void *stream);
/* sess.run(self.loss) (pe.py:264,582-603,629-635): d_losses[e] = 0.5 * mean over rows and
 * target dims of (mean head - scaled target)^2; idx_stride 0 evaluates every member on the same
 * rows (the tiled holdout set). */
int cmbpo_trainer_losses(cmbpo_trainer_t *t, const float *d_inputs, int in_dim,
                         const float *d_targets, int target_dim, const int32_t *d_idx,
                         int idx_stride, int n_rows, float *d_losses, void *stream);
/* Optional terms of the deterministic ('MSE') loss, _nll_loss(inc_var_loss=False, weights=, oldpred_v=), pe.py:866-868,
 * 881-905,917.  Both arrays are addressed through the same row indices as inputs and targets.
 *   d_weights   [N] float32, non-negative, or NULL: loss_e = mean_b w[r] mean_d 0.5 (m - t')^2 (the mean divides by the batch,
 *               not by the sum of the weights), in the train loss and in `self.loss`;
 *   d_old_pred  [N][target_dim] float32 or NULL: the clipped prediction m_c = old' + clip(m - old', -c, c) replaces m in the
 *               TRAIN loss, c = sqrt(2) sqrt(kl_cliprange old_var), old_var = mean over every member, row and output of the
 *               step of 0.5 (old' - t')^2.  old' is d_old_pred through the output scaler, like the targets t' (the reference
 *               subtracts scaled targets from unscaled predictions, pe.py:879,890-893; with the scaler off the two agree).
 *               `self.loss` is never clipped: cmbpo_trainer_losses_ex ignores d_old_pred and kl_cliprange;
 *   kl_cliprange  finite, >= 0; read when d_old_pred is set.
 * A NULL block, or one that sets neither array, is the plain entry, bit for bit.  Refused (CMBPO_EINVAL before any device
 * work): a probabilistic head (the 'MSPE' loss takes neither term, clipping an 'NLL' head needs old_pred_var), a negative or
 * non-finite kl_cliprange. */
typedef struct cmbpo_train_extras {
  const float *d_weights;
  const float *d_old_pred;
  float kl_cliprange;
} cmbpo_train_extras_t;
int cmbpo_trainer_step_ex(cmbpo_trainer_t *t, const float *d_inputs, int in_dim,
                          const float *d_targets, int target_dim, const int32_t *d_idx,
                          int idx_stride, int batch, const cmbpo_train_extras_t *extras, void *stream);
int cmbpo_trainer_epoch_ex(cmbpo_trainer_t *t, const float *d_inputs, int in_dim,
                           const float *d_targets, int target_dim, const int32_t *d_idx,
                           int idx_stride, int n_rows, int batch, const cmbpo_train_extras_t *extras,
                           void *stream);
int cmbpo_trainer_losses_ex(cmbpo_trainer_t *t, const float *d_inputs, int in_dim,
                            const float *d_targets, int target_dim, const int32_t *d_idx,
                            int idx_stride, int n_rows, float *d_losses,
                            const cmbpo_train_extras_t *extras, void *stream);
/* Column and class weights of the probabilistic train losses ('MSPE', 'NLL'); DESIGN §3s.  Two host arrays of target_dim
 * floats, h_col_weight (NULL: all ones) and h_pos_weight (NULL: all ones).  For member e, batch row b with gathered data row r
 * and target column d
 *     w[b][d] = col_weight[d] * (targets[r][d] > 0.5f ? pos_weight[d] : 1)
 * The test reads the RAW target, before the output scaler, and is written positively: a NaN target takes the plain weight.
 * Every mean over (row, column) of a per-element data term becomes the mean of w times that term; the divisor stays B D (the
 * mean divides by the batch, not by the weight sum, as with d_weights above); the log-variance regulariser stays unweighted:
 *   MSPE  total_e = mean(w (m - t')^2) + ratio mean(w (var - sg(mse))^2) + 0.05 mean_all(lv^2),
 *         ratio = 0.05 sum_all(w mse) / sum_all(w (var - mse)^2) over all members;
 *         d/dm = 2 w (m - t') / (B D),   d/dlv = [2 ratio w (var - mse) var + 0.1 lv] / (B D)
 *   NLL   total_e = mean(w 0.5 exp(-lv) (m - t')^2) + mean(w 0.5 lv);
 *         d/dm = w exp(-lv) (m - t') / (B D),   d/dlv = w (0.5 - 0.5 exp(-lv) (m - t')^2) / (B D)
 *   `self.loss` (cmbpo_trainer_losses) = 0.5 mean(w (m - t')^2): members are ranked by the loss they were trained on.
 * On a 0/1 column with positive rate p and class weight omega the weighted least-squares level is
 * q = omega p / (omega p + 1 - p), not p: whoever thresholds the column reads q.
 * The weights are copied to the device and are trainer state: cmbpo_trainer_step, _epoch and _losses honour them until both
 * arrays are NULL (detach: the plain kernels run again, bit for bit).  The *_ex entries go on refusing probabilistic heads.
 * Refused (CMBPO_EINVAL before any device work): a negative or non-finite entry, a col_weight with no positive entry, a NULL
 * trainer, a deterministic head (its per-sample weights go through cmbpo_trainer_step_ex), target_dim != the head's. */
int cmbpo_trainer_set_column_weights(cmbpo_trainer_t *t, const float *h_col_weight, const float *h_pos_weight,
                                     int target_dim, void *stream);
/* Column kinds of the probabilistic train losses: a Bernoulli likelihood for binary target columns; DESIGN §3v.  One host array
 * h_kind of target_dim bytes: 0 Gaussian (the formulas above, term for term), 1 logistic.  NULL or all zeros detaches (the
 * kernels that ran before run again, bit for bit).  For a logistic column d, member e, batch row b with gathered data row r:
 *     z = o[e][b][d]                       the raw mean output, read as a logit; the output scaler is NOT applied to this
 *                                          column, neither to the target nor to the output
 *     y = targets[r][d] > 0.5f ? 1 : 0     on the RAW float32 target, written positively: a NaN target is 0 (the rule of
 *                                          cmbpo_trainer_set_column_weights)
 *     w = col_weight[d] * (y ? pos_weight[d] : 1)   with column weights attached, else 1
 *     l = max(z, 0) - y z + log1p(exp(-|z|))        = softplus(z) - y z, finite for every finite z
 *     sigma(z) = 1 / (1 + exp(-z)) for z >= 0, exp(z) / (1 + exp(z)) otherwise
 * For both losses total_e adds mean(w l) over the logistic elements (the divisor stays B D), so d/dz = w (sigma(z) - y) / (B D).
 * The log-variance output D + d of a logistic column has no data term: under 'MSPE' it keeps the unweighted regulariser alone
 * (delta 0.1 lv / (B D)), under 'NLL' its delta is 0; nothing in the rollout reads that variance.  'MSPE''s
 * ratio = 0.05 sum w mse / sum w (var - mse)^2 runs over the Gaussian columns only (all members, as before).
 * `self.loss` (cmbpo_trainer_losses) = mean over (row, column) of 0.5 w (m - t')^2 on Gaussian columns and w l on logistic ones.
 * With a class weight omega on a logistic column of positive rate p the fitted odds are omega times the true odds: the level is
 * still q = omega p / (omega p + 1 - p).
 * Reading the column: p = sigma(z); the test sigma(z) > tau is z > (float)log(tau / (1 - tau)), the logit taken in double on
 * the host for tau strictly inside (0, 1).
 * The kinds are copied to the device and are trainer state, like the column weights, and combine with them.  The *_ex entries
 * go on refusing probabilistic heads.  Refused (CMBPO_EINVAL before any device work): a NULL trainer, a deterministic head,
 * target_dim != the head's, a kind outside {0, 1}, an array that makes every column logistic. */
int cmbpo_trainer_set_column_kinds(cmbpo_trainer_t *t, const unsigned char *h_kind, int target_dim, void *stream);
long cmbpo_trainer_steps_done(const cmbpo_trainer_t *t);
/* Which kernels a training step of this trainer runs: bit 0 the f16 backward chain, bit 1 the f16 training forward
 * (0: the fp32 kernels; -1: NULL handle).  Fixed at creation by the network's shapes. */
int cmbpo_trainer_f16_paths(const cmbpo_trainer_t *t);
/* 1: a training step of this trainer is one fused_mse_step_kernel launch in front of Adam (128-wide deterministic heads of at
 * most 32 outputs and 64 padded inputs), 0: the general forward / backward-chain / weight-gradient kernels; -1: NULL handle. */
int cmbpo_trainer_fused(const cmbpo_trainer_t *t);

/* ---- start states of an imagined-rollout round (csrc/start_states.hip) -----
 * algorithms/cmbpo.py:239-251 on a device mirror of CPOBuffer's archive: observations [n][obs_dim],
 * mu / log_std [n][act_dim] float32 and the epoch column int32 [n] (-1 = empty slot).  The epoch
 * column is a few runs of equal tags (one slab per CPOBuffer.get, split by a wrap-around); every
 * entry works on the run table of cmbpo_start_table_build, never on the [n] column.  d_table is
 * int32[CMBPO_START_TABLE_INTS]: [0] runs, [1] epochs present, [2] != 0 if the column has more
 * than CMBPO_START_MAX_RUNS runs (the table is then unusable), [3] filled slots; from
 * [8 + 3 * MAX_RUNS] the sorted epochs present (epochs_list, buffers/cpobuffer.py:148-153), from
 * [8 + 4 * MAX_RUNS] their sample counts (np.bincount). */
#define CMBPO_START_MAX_RUNS 1024
#define CMBPO_START_TABLE_INTS (8 + 11 * CMBPO_START_MAX_RUNS)
#define CMBPO_START_CDF_DOUBLES (8 + 4 * CMBPO_START_MAX_RUNS)
int cmbpo_start_table_build(const int32_t *d_epochs, long n, int32_t *d_table, void *stream);
/* CPOBuffer.epoch_batch (buffers/cpobuffer.py:466-524) with the uniforms handed in: row e * batch + b
 * is member min(floor(d_u[e][b] * n_e), n_e - 1) of np.flatnonzero(epoch_archive == epochs_list[e]);
 * d_idx gets the archive indices, the three outputs the drawn rows ([n_epochs * batch][.]).
 * d_epoch_sel (may be NULL) makes group e the epoch at place d_epoch_sel[e] of epochs_list. */
int cmbpo_start_epoch_draw(const int32_t *d_table, const int32_t *d_epoch_sel, int n_epochs, int batch, const double *d_u,
                           const float *d_obs, const float *d_mu, const float *d_logstd, long n,
                           int obs_dim, int act_dim, int32_t *d_idx, float *d_obs_out, float *d_mu_out,
                           float *d_logstd_out, void *stream);
/* CPOPolicy.compute_DKL (policies/cpo_policy.py:837-845) after the actor's forward pass on the
 * gathered rows: gaussian_kl(current, stored) per row (network/ac_network.py:50-55), summed in
 * float64 per workgroup in a fixed order into d_part[n_epochs][n_part], n_part =
 * cmbpo_start_kl_parts(batch); cmbpo_start_cdf folds them. */
int cmbpo_start_kl_parts(int batch);
int cmbpo_start_kl_partials(const float *d_mu, const float *d_logstd, const float *d_mu_old,
                            const float *d_logstd_old, int n_epochs, int batch, int act_dim,
                            double *d_part, int n_part, void *stream);
/* np.clip(kls, 0) (algorithms/cmbpo.py:220), CPOBuffer.boltz_dist (buffers/cpobuffer.py:385-396) and
 * the normalised float64 cumulative sum np.random.choice(p=) searches (:454), per run.  d_part != NULL:
 * d_kl[e] = max(sum_k d_part[e][k] / batch, 0) is written; NULL: d_kl is read.  d_cdf is
 * double[CMBPO_START_CDF_DOUBLES]: [0] the unnormalised total, [1] set to 1 (never cleared here) when
 * it is not a positive finite number -- a NaN KL, no mass: draws from such a CDF are void --, from
 * [8 + 3 * MAX_RUNS] the epochs' Boltzmann probabilities. */
int cmbpo_start_cdf(const int32_t *d_table, const double *d_part, int n_part, int batch, double *d_kl,
                    double alpha, double *d_cdf, void *stream);
/* CPOBuffer.distributed_batch_from_archive (buffers/cpobuffer.py:413-464) with the uniforms handed in:
 * d_idx[b] = cdf.searchsorted(d_u[b], side='right'), row d_idx[b] of d_obs -> d_out[b] (the rollout
 * state's cur_obs). */
int cmbpo_start_boltz_draw(const int32_t *d_table, const double *d_cdf, const double *d_u, int batch,
                           const float *d_obs, long n, int obs_dim, int32_t *d_idx, float *d_out,
                           void *stream);

/* ---- open-loop model validation: k-step replay of real trajectories (csrc/replay.hip) -----
 * The reference has no such diagnostic.  A replay takes B windows of up to H consecutive REAL steps (time-major arrays, step h
 * of window b at [h][b]), starts the model at each window's first real observation (cur_obs, alive = 1 on entry) and applies
 * the recorded actions; at every horizon h the prediction of cmbpo_ens_forward + the plain cmbpo_fakeenv_post from cur_obs is
 * held against the recording.  The noise and disagreement entries are never called: a replay measures the unpenalised means.
 *
 * cmbpo_replay_compare, for every row alive on entry to step h, in this order:
 *   1. a non-finite value in p_next_obs[b], p_rew[b] or p_cost[b]: the row counts in n_nonfinite[h], dies, adds nothing else;
 *   2. otherwise it counts in n[h] and adds
 *        se_obs[h][d] += (double)e * (double)e,  e = fl32(p_next_obs[b][d] - next_obs[h][b][d]);  se_rew, se_cost likewise;
 *        cost_cm[h][cost[h][b] > 0][p_cost[b] > 0.5] += 1;   term_cm[h][term[h][b] != 0][p_term[b] != 0] += 1;
 *        sum_ep_var[h] += (double)p_ep_var_mean[b];   sum_dkl[h] += (double)p_dkl_path[b];
 *   3. it lives on to h + 1 iff h + 1 < len[b], term[h][b] == 0 and (CMBPO_REPLAY_OPEN_LOOP only) p_term[b] == 0; then
 *        cur_obs[b] = p_next_obs[b] (CMBPO_REPLAY_OPEN_LOOP) or next_obs[h][b] (CMBPO_REPLAY_ONE_STEP: teacher-forced; a
 *        predicted termination is counted and does not end the window); otherwise alive[b] = 0;
 *   4. a dead row is frozen: its cur_obs is not written (neither by the step at which it dies), nothing of it is read.
 * Sums are float64, counts int64: per-workgroup partials (slot = workgroup, cmbpo_replay_parts(B) slots per horizon) written by
 * cmbpo_replay_compare, added in slot order by cmbpo_replay_finish; no floating-point atomics, two runs are bitwise equal.
 *   sums   [H][obs_dim + 4]: se_obs[0 .. obs_dim) | se_rew | se_cost | sum_ep_var | sum_dkl
 *   counts [H][10]:          n | n_nonfinite | cost_cm[0][0], [0][1], [1][0], [1][1] ([real][pred]) | term_cm likewise
 * A horizon no compare call was made for holds whatever the partials held.  len is not checked (1 <= len[b] <= H). */
#define CMBPO_REPLAY_OPEN_LOOP 0
#define CMBPO_REPLAY_ONE_STEP 1
#define CMBPO_REPLAY_SCALAR_SUMS 4
#define CMBPO_REPLAY_COUNTS 10

typedef struct cmbpo_replay {
  int32_t B, H, obs_dim, act_dim, mode, reserved;
  /* recorded, time-major */
  const float *act;         /* [H,B,act]   (cmbpo_replay_run only)              */
  const float *next_obs;    /* [H,B,obs]                                        */
  const float *rew, *cost;  /* [H,B]                                            */
  const uint8_t *term;      /* [H,B]                                            */
  const int32_t *len;       /* [B] real steps of the window, 1 .. H             */
  /* state */
  float *cur_obs;           /* [B,obs] the observation step h starts from       */
  uint8_t *alive;           /* [B]                                              */
  /* cmbpo_fakeenv_post's outputs for the step, slot indexed */
  float *p_next_obs;        /* [B,obs]                                          */
  float *p_rew;             /* [B]                                              */
  uint8_t *p_term;          /* [B]                                              */
  float *p_cost, *p_dkl_path, *p_ep_var_mean; /* [B]                            */
  float *mean, *var;        /* [E,B,model out_dim] scratch of the forward (cmbpo_replay_run only) */
  /* partial sums and the result table */
  double *part_sum;         /* [H][cmbpo_replay_parts(B)][obs + 4]              */
  int64_t *part_cnt;        /* [H][cmbpo_replay_parts(B)][10]                   */
  double *sums;             /* [H][obs + 4]                                     */
  int64_t *counts;          /* [H][10]                                          */
} cmbpo_replay_t; /* 184 bytes */

/* Every entry: CMBPO_EINVAL with a message naming the entry point for B < 1, H < 1, bad dims, an unknown mode, a NULL array it
 * uses, h outside [0, H) -- all before any HIP call. */
/* partial-sum slots per horizon of a replay of n_rows windows (0 for n_rows < 1) */
int cmbpo_replay_parts(int n_rows);
/* one horizon step of comparison and advance on the prediction arrays in *rp */
int cmbpo_replay_compare(const cmbpo_replay_t *rp, int h, void *stream);
/* partials -> sums / counts, all H horizons */
int cmbpo_replay_finish(const cmbpo_replay_t *rp, void *stream);
/* H x (cmbpo_ens_forward on all B rows -> cmbpo_fakeenv_post -> cmbpo_replay_compare), then cmbpo_replay_finish, enqueued
 * without a host wait; bitwise the result of the same calls issued one at a time.  d_elite is [H][B]: the member of window b
 * at step h.  `task` as for cmbpo_fakeenv_post; the two callees' own refusals are passed on under this entry point's name. */
int cmbpo_replay_run(const cmbpo_replay_t *rp, cmbpo_mlp_t *model, int task, int ensemble, const int32_t *d_elite,
                     void *stream);

/* ---- predictive calibration in the replay (csrc/replay.hip) ---------------------------------
 * Is the ensemble's VARIANCE right?  At horizon h of a replay the forward's (mean, var)[E][B][out_dim] scratch sits beside
 * the post kernel's prediction and the recording; the calibration table holds the squared error of every CALIBRATED column
 * against two predictive variances.  Calibrated columns: c = 0 .. obs_dim - 1 (the observation deltas) and c = obs_dim (the
 * reward), C = obs_dim + 1 in all; a learned-cost column (binary) is left out.
 *
 * A row ENTERS the table at h iff (a) alive[b] != 0 on entry to the step -- which is why the calibrate call of a step goes
 * BEFORE its compare call, the one that clears alive and overwrites cur_obs --, (b) p_next_obs[b], p_rew[b], p_cost[b] are
 * finite (the compare call's rule), (c) mean[e][b][c] and var[e][b][c] are finite and var[e][b][c] > 0 for every member e and
 * every c < C, and elite[h][b] lies in [0, ensemble).  Rows with (a) and (b) but not (c) count in n_skipped[h], rows with all
 * three in n_cal[h]; nothing else of a row that does not enter is summed.
 *
 * Per entering row and column, float64 arithmetic on the float32 inputs, every operation rounded separately, members in the
 * order 0 .. E-1, m = elite[h][b]:
 *   e      = (double)fl32(p_next_obs[b][c] - next_obs[h][b][c])   (c < obs_dim),   (double)fl32(p_rew[b] - rew[h][b])   (c = obs_dim)
 *   mu_bar = (sum_e mu_e) / E     v_bar = (sum_e v_e) / E     s2 = (sum_e (mu_e - mu_bar)^2) / E
 *   v_al   = v_m                  v_tot = v_bar + s2          e_tot = e + (mu_bar - mu_m)
 *   sums   [h][k][c], k = 0..5:  e^2 / v_al | e_tot^2 / v_tot | log v_al | log v_tot | v_bar | s2
 *   counts [h][k][c], k = 0..3:  e^2 <= v_al | e^2 <= 4 v_al | e_tot^2 <= v_tot | e_tot^2 <= 4 v_tot
 *   counts [h][4 C], [h][4 C + 1]:  n_cal | n_skipped
 * In CMBPO_REPLAY_ONE_STEP every horizon is a one-step prediction; in CMBPO_REPLAY_OPEN_LOOP only h = 0 is: the later rows
 * show how far the one-step variance falls short of the compounded error, they are no k-step predictive distribution.
 * Per-workgroup partials (slot = workgroup, every entry written on every call) added in slot order by the finish call: no
 * floating-point atomics, two runs are bitwise equal.  The prediction, recording, alive, mean and var arrays are those of
 * the cmbpo_replay_t handed in beside the descriptor; which is not changed by any of this (184 bytes). */
#define CMBPO_REPLAY_CALIB_SUMS 6
#define CMBPO_REPLAY_CALIB_COUNTS 4

typedef struct cmbpo_replay_calib {
  int32_t ensemble, out_dim, reserved;  /* members E; columns of mean / var (>= obs_dim + 1); must be 0 */
  const int32_t *elite;     /* [H,B] the member each window steps through at h     */
  double *part_sum;         /* [H][cmbpo_replay_parts(B)][6 (obs + 1)]             */
  int64_t *part_cnt;        /* [H][cmbpo_replay_parts(B)][4 (obs + 1) + 2]         */
  double *sums;             /* [H][6 (obs + 1)]                                    */
  int64_t *counts;          /* [H][4 (obs + 1) + 2]                                */
} cmbpo_replay_calib_t; /* 56 bytes (4 of padding behind `reserved`) */

/* Every entry: CMBPO_EINVAL with a message naming the entry point for a NULL descriptor, a NULL array it uses, ensemble < 1,
 * out_dim < obs_dim + 1, reserved != 0, h outside [0, H) and every shape refusal of the compare call -- all before any HIP
 * call. */
/* one horizon step of the calibration table, from the arrays the compare call of the same step reads plus rp->mean / rp->var.
 * Enqueue it BEFORE that step's compare call (see above); it writes nothing but its partial slot. */
int cmbpo_replay_calibrate(const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *rc, int h, void *stream);
/* partials -> rc->sums / rc->counts, all H horizons */
int cmbpo_replay_calib_finish(const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *rc, void *stream);
/* The run call with the calibrate call in every step: H x (forward -> post -> calibrate -> compare), then both finish calls,
 * enqueued without a host wait; bitwise the single calls.  The members are rc->elite; `ensemble` must equal rc->ensemble.  The
 * plain table, cur_obs and alive are bitwise those of the run call without calibration on the same inputs. */
int cmbpo_replay_run_calibrated(const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *rc, cmbpo_mlp_t *model, int task,
                                int ensemble, void *stream);
/* The replay with the learned termination head in its post step (cmbpo_fakeenv_post_term without noise or disagreement): p_term
 * is rule_done || learned_done, so the termination counts of the table describe the head.  rc == NULL: cmbpo_replay_run's
 * launches, else cmbpo_replay_run_calibrated's (the members are then rc->elite and d_elite may be NULL or equal to it).  The
 * model's out_dim must be obs_dim + 1 + learned cost + 1 (refused with a message naming the termination head); th == NULL
 * forwards to the two existing entry points.  Bitwise the result of the same calls issued one at a time. */
int cmbpo_replay_run_term(const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *rc, const cmbpo_term_head_t *th,
                          cmbpo_mlp_t *model, int task, int ensemble, const int32_t *d_elite, void *stream);
/* ... and with the cost head's reading in its post step (cmbpo_fakeenv_post_cost without noise or disagreement): the superset of
 * the run entries.  With kind 1 p_cost is the elite's probability, so the table's `p_cost > 0.5` counts are a decision rule on a
 * probability and the cost's squared error is the Brier score of the column.  The model's out_dim must be obs_dim + 2 (+ 1 with
 * th), refused with a message naming the cost head; ch == NULL is cmbpo_replay_run_term's call.  Bitwise the result of the same
 * calls issued one at a time. */
int cmbpo_replay_run_cost(const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *rc, const cmbpo_term_head_t *th,
                          const cmbpo_cost_head_t *ch, cmbpo_mlp_t *model, int task, int ensemble, const int32_t *d_elite,
                          void *stream);

/* ---- reliability tables of the logistic columns in the replay (csrc/replay.hip) -------------
 * Is a logistic column a PROBABILITY?  At horizon h of a replay the forward's mean[E][B][out_dim] scratch holds every member's
 * logit beside the recorded cost / term flags; the reliability table bins the logits and holds, per bin, how often the event
 * happened against what the column said.  Up to two RELIABILITY COLUMNS j: col[j] indexes the model's output (obs_dim + 1 for
 * the logistic cost, the last column for the logistic termination head), shift[j] is subtracted from the logit first (the
 * cost head's class-weight undo; 0 executes no subtraction, as in the post kernel's cost_prob), target[j] names the recorded
 * flag: CMBPO_RELIAB_COST y = cost[h][b] > 0.5 (the rule the logistic cost is trained with), CMBPO_RELIAB_TERM y = term[h][b] != 0
 * -- with the descriptor's own `term` array where it is given: the recorded `done` of a step is not always the head's training
 * target (a time-out is target 0), and the table must be held against what the column was trained on, while the replay
 * itself goes on ending windows at rp->term.
 *   z'_e = fl32(mean[e][b][col[j]] - shift[j])
 *
 * A row ENTERS column j at h iff (a) alive[b] != 0 on entry to the step -- the call goes BEFORE that step's compare call, like
 * the calibrate call --, (b) p_next_obs[b], p_rew[b], p_cost[b] are finite (the compare call's rule), (c) elite[h][b] lies in
 * [0, ensemble) and z'_e is finite for every member e.  Rows with (a) and (b) but not (c) count in n_skipped[h][j], rows with
 * all three in n_rel[h][j]; both per column; nothing else of a row that does not enter is summed.
 *
 * Two READINGS r per column, float64 arithmetic on the float32 inputs, every operation rounded separately, members in the
 * order 0 .. E-1, m = elite[h][b]:
 *   r = 0, elite:   z = (double)z'_m                    (what the cost and the 'elite' vote read)
 *   r = 1, pooled:  z = (sum_e (double)z'_e) / E        (the mean logit: geometric pooling of the odds)
 * The bin of z is #{k : z > (double)edges[k]}, k < n_bins - 1: bins live in LOGIT space, equality stays in the lower bin, no
 * exponential decides a bin, so membership and every count are exact.  The rule is defined for ANY edges (a bin index is a
 * count of edges below z); ascending, finite edges are what makes the bins intervals, and the host's to insist on.
 *   y = 0.0 / 1.0     p = 1 / (1 + exp(-z))     l = max(z, 0) - y z + log1p(exp(-|z|))
 *   brier = (p - y)^2, evaluated as q^2 with q = |p - y| = 1 / (1 + exp(y ? z : -z)): no cancellation where p is close to y
 * Layout, with K = n_bins and C = n_cols, [j][r] running over 2 C (column, reading) pairs, j outermost:
 *   sums   [H][2 C][2 K + 2]:  sum p [0 .. K) | sum z [0 .. K) | sum brier | sum l
 *   counts [H][2 C (2 K) + 2 C]:  per [j][r]: n [0 .. K) | pos [0 .. K) (rows with y = 1);  behind all of them per j: n_rel | n_skipped
 * Per-workgroup partials (slot = workgroup, cmbpo_replay_parts(B) slots per horizon, every entry of a slot written on every
 * call; inside a slot a bin's rows are added in row order) added in slot order by the finish call: no floating-point atomics,
 * two runs are bitwise equal.  Reads alive / predictions / recording / mean of the cmbpo_replay_t handed in beside the
 * descriptor, writes its partial slot only; cmbpo_replay_t (184 bytes) and cmbpo_replay_calib_t (56) are what they were. */
#define CMBPO_RELIAB_COST 0
#define CMBPO_RELIAB_TERM 1
#define CMBPO_RELIAB_MAX_BINS 32
#define CMBPO_RELIAB_MAX_COLS 2
#define CMBPO_RELIAB_MAX_ENSEMBLE 8

typedef struct cmbpo_replay_reliab {
  int32_t ensemble, out_dim, n_bins, n_cols, reserved;  /* members E (1..8); columns of mean; K (1..32); C (1..2); must be 0 */
  int32_t col[2], target[2];  /* column of mean; CMBPO_RELIAB_COST / _TERM -- entries j >= n_cols are ignored */
  float shift[2];           /* finite                                              */
  const int32_t *elite;     /* [H,B] the member each window steps through at h     */
  const float *edges;       /* [n_bins - 1] bin edges in logit space (may be NULL for n_bins == 1) */
  const uint8_t *term;      /* [H,B] the flags CMBPO_RELIAB_TERM columns are held against; NULL: rp->term */
  double *part_sum;         /* [H][cmbpo_replay_parts(B)][2 C (2 K + 2)]           */
  int64_t *part_cnt;        /* [H][cmbpo_replay_parts(B)][4 C K + 2 C]             */
  double *sums;             /* [H][2 C (2 K + 2)]                                  */
  int64_t *counts;          /* [H][4 C K + 2 C]                                    */
} cmbpo_replay_reliab_t; /* 104 bytes (4 of padding behind `shift`) */

/* Every entry: CMBPO_EINVAL with a message naming the entry point for a NULL descriptor, a NULL array it uses, n_bins outside
 * [1, 32], n_cols outside [1, 2], col[j] outside [0, out_dim), an unknown target, a non-finite shift, reserved != 0, ensemble
 * outside [1, 8], h outside [0, H) and every shape refusal of the compare call -- all before any HIP call. */
/* one horizon step of the reliability table, from the arrays the compare call of the same step reads plus rp->mean.  Enqueue it
 * BEFORE that step's compare call (beside a calibrate call: in either order); it writes nothing but its partial slot. */
int cmbpo_replay_reliab(const cmbpo_replay_t *rp, const cmbpo_replay_reliab_t *rr, int h, void *stream);
/* partials -> rr->sums / rr->counts, all H horizons */
int cmbpo_replay_reliab_finish(const cmbpo_replay_t *rp, const cmbpo_replay_reliab_t *rr, void *stream);
/* The superset of the run entries: H x (forward -> post -> [calibrate] -> [reliab] -> compare), then the finish calls (plain,
 * calibration, reliability), enqueued without a host wait; bitwise the single calls.  rr == NULL is exactly
 * cmbpo_replay_run_cost's call.  With rr: `ensemble` must equal rr->ensemble and the model's out_dim rr->out_dim; the members
 * are rr->elite, d_elite may be NULL or equal to it, and rc->elite (rc given) must equal it.  The plain table, the calibration
 * table, cur_obs and alive are bitwise those of the run without rr on the same inputs. */
int cmbpo_replay_run_reliab(const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *rc, const cmbpo_replay_reliab_t *rr,
                            const cmbpo_term_head_t *th, const cmbpo_cost_head_t *ch, cmbpo_mlp_t *model, int task,
                            int ensemble, const int32_t *d_elite, void *stream);

/* ---- the static rules' votes in the replay (csrc/replay.hip) -------------------------------
 * Which of the vote's readings is right, and is the vote SHARE a probability?  With a vote descriptor the post step of a replay
 * is cmbpo_fakeenv_post_votes's (the vote kernel of csrc/rule_votes.hip behind the post kernel at every horizon, without noise,
 * disagreement or kappa_cost): p_term / p_cost are the vote's verdicts under done_members / cost_members, so the plain table's
 * term_cm / cost_cm describe the rule in force, a CMBPO_REPLAY_OPEN_LOOP window ends where the vote ends it, and under
 * CMBPO_VOTE_MEAN p_cost = votes / E: se_cost is the Brier score of the share and the compare call's `p_cost > 0.5` the strict
 * majority.  CMBPO_TERM_ELITE / CMBPO_TERM_ELITE measures: the verdicts are the elite's, only the vote table is new.
 *
 * The vote table is a histogram of the two vote counts the vote kernel left in done_votes / cost_votes [B] for the step, against
 * the recorded flags.  A row ENTERS at h iff (a) alive[b] != 0 on entry to the step -- the call goes BEFORE that step's compare
 * call, like the calibrate and reliab calls --, (b) p_next_obs[b], p_rew[b], p_cost[b] are finite (the compare call's rule).  An
 * entering row with done_votes[b] > ensemble or cost_votes[b] > ensemble counts in n_skipped[h] and adds nothing else (the vote
 * kernel never writes such a count: only caller-made arrays handed to the single-step entry reach it); every other entering row
 * counts in n_vote[h] and adds
 *   hist_cost[h][v_c][y_c] += 1,   v_c = cost_votes[b],  y_c = cost[h][b] > 0        (the compare call's rule for a real cost)
 *   hist_term[h][v_d][y_t] += 1,   v_d = done_votes[b],  y_t = term[h][b] != 0       (the descriptor's `term` where given)
 * The descriptor's own `term` serves as in cmbpo_replay_reliab_t: the termination RULE is held against a head's training targets
 * (a time-out is 0 there) while the replay goes on ending windows at rp->term.  cost_votes == NULL (a learned cost: the static
 * cost rule is skipped) leaves the cost half 0.  Layout, int64:
 *   counts [H][38]:  hist_cost [9][2] ([v][y], v = 0 .. 8) | hist_term [9][2] | n_vote | n_skipped      slots v > ensemble stay 0
 * Integers only: inside a workgroup every entry is one wave ballot's population count, per-workgroup partials (slot = workgroup,
 * cmbpo_replay_parts(B) slots per horizon, every entry of a slot written on every call) are added in slot order by the finish
 * call; no atomics on global memory, no floating point, two runs are bitwise equal.  Reads alive / predictions / recording of the
 * cmbpo_replay_t handed in beside the descriptor and the two vote arrays, writes its partial slot only; the three other
 * descriptors (184, 56 and 104 bytes) are what they were. */
#define CMBPO_REPLAY_VOTE_COUNTS 38
#define CMBPO_REPLAY_VOTES_MAX_ENSEMBLE 8

typedef struct cmbpo_replay_votes {
  int32_t ensemble;         /* members E (1..8)                                     */
  int32_t done_members;     /* CMBPO_TERM_ELITE / _ANY / _MAJORITY                  */
  int32_t cost_members;     /* CMBPO_TERM_ELITE / _ANY / _MAJORITY / CMBPO_VOTE_MEAN */
  int32_t reserved;         /* must be 0                                            */
  uint8_t *done_votes;      /* [B] step scratch: the vote kernel writes, the table kernel reads */
  uint8_t *cost_votes;      /* [B] likewise; NULL with CMBPO_TASK_LEARNED_COST      */
  const uint8_t *term;      /* [H,B] the flags hist_term is held against; NULL: rp->term */
  int64_t *part_cnt;        /* [H][cmbpo_replay_parts(B)][38]                       */
  int64_t *counts;          /* [H][38]                                              */
} cmbpo_replay_votes_t; /* 56 bytes */

/* Every entry: CMBPO_EINVAL with a message naming the entry point for a NULL descriptor, a NULL array it uses (cost_votes and
 * term may be NULL), ensemble outside [1, 8], done_members outside 0..2, cost_members outside 0..3, reserved != 0, h outside
 * [0, H) and every shape refusal of the compare call -- all before any HIP call. */
/* one horizon step of the vote table, from the arrays the compare call of the same step reads plus the two vote arrays.  Enqueue
 * it BEFORE that step's compare call (beside a calibrate / reliab call: in any order); it writes nothing but its partial slot. */
int cmbpo_replay_votes(const cmbpo_replay_t *rp, const cmbpo_replay_votes_t *rv, int h, void *stream);
/* partials -> rv->counts, all H horizons */
int cmbpo_replay_votes_finish(const cmbpo_replay_t *rp, const cmbpo_replay_votes_t *rv, void *stream);
/* The superset of the run entries: H x (forward -> post [-> vote kernel] -> [calibrate] -> [reliab] -> [votes] -> compare), then
 * the finish calls (plain, calibration, reliability, votes), enqueued without a host wait; bitwise the single calls (the post
 * step: cmbpo_fakeenv_post_votes with rv's modes and vote arrays, d_xi NULL, kappa 0).  rv == NULL is exactly
 * cmbpo_replay_run_reliab's call: the same launches, the same messages.  With rv: `ensemble` must equal rv->ensemble; with th,
 * th->term_pred and th->term_votes [B] are required (the vote kernel recovers learned_done from them).  The post step's own
 * refusals are passed on under this entry's name: a mode out of range, ensemble above 8, and with CMBPO_TASK_LEARNED_COST
 * cost_members != CMBPO_TERM_ELITE or a non-NULL cost_votes.  Under CMBPO_TERM_ELITE / CMBPO_TERM_ELITE the plain, calibration
 * and reliability tables, cur_obs and alive are bitwise those of the run without rv on the same inputs. */
int cmbpo_replay_run_votes(const cmbpo_replay_t *rp, const cmbpo_replay_calib_t *rc, const cmbpo_replay_reliab_t *rr,
                           const cmbpo_replay_votes_t *rv, const cmbpo_term_head_t *th, const cmbpo_cost_head_t *ch,
                           cmbpo_mlp_t *model, int task, int ensemble, const int32_t *d_elite, void *stream);

/* ---- particle replay: rank histograms and CRPS of sampled rollouts (csrc/replay.hip) --------
 * Is the CLOUD of sampled branches as wide as the real spread, k compounded steps out?  Every window is replayed by S sampled
 * particles, each with its own member draws and its own transition noise; at every horizon the recorded next state is held
 * against the S particles.
 *
 * Layout.  B windows, H horizons, S particles per window, S a power of two in 2..64.  The stepping runs on R = B S rows: particle
 * p of window b is row b S + p, a window's particles are adjacent rows.  Step h: cmbpo_ens_forward on all R rows from the
 * particles' own cur_obs (act [H][R][act]: the recorded action of window b, repeated for its S rows), then the post step with
 * xi + h R obs_dim and d_elite + h R, the environment's termination head (th) and cost head (ch) as the plain replay passes them;
 * never term_thr, disagreement or votes.  Then cmbpo_replay_particles, on windows:
 *   1. a window is ALIVE at h iff h < len[b], no recorded terminal came before h and it has not gone non-finite; alive [R] holds
 *      the same value in all S rows of a window (the S particles live and die together).  A PREDICTED termination does not end
 *      a particle -- its state goes on through the model: a fixed S per window is what makes the ranks comparable.  It is
 *      only measured (brier_term);
 *   2. a non-finite value in any of the window's S rows of p_next_obs, p_rew or p_cost: the window counts in n_nonfinite[h],
 *      ends, and enters nothing else.  Otherwise it counts in n[h];
 *   3. columns c = 0 .. obs_dim - 1: x_p = p_next_obs[b S + p][c] against q = next_obs[h][b][c]; c = obs_dim: x_p = p_rew[b S + p]
 *      against q = rew[h][b]; C = obs_dim + 1 in all.  (The reward carries no aleatoric draw by design, DESIGN 3i: its particles
 *      differ by member and by state only.)  Per (h, c):
 *        rank_hist[h][c][k] += 1,  k = #{p : x_p < q}: strict, float32, k in 0 .. S; a tie counts as not below
 *        sum_abs  += a = (sum_p |fl32(x_p - q)|) / S
 *        sum_pair += g = (2 sum_{p < p'} |fl32(x_p - x_p')|) / (S (S - 1))
 *        sum_se   += (m - q)^2,  m = (sum_p x_p) / S
 *        sum_var  += (sum_p (x_p - m)^2) / (S - 1)            (two-pass)
 *      float64 arithmetic on the float32 terms; the order of the additions inside a window is the kernel's own and fixed;
 *   4. per window: brier_term += (mean_p [p_term != 0] - [term[h][b] != 0])^2,  brier_cost += (mean_p p_cost - [cost[h][b] > 0])^2;
 *   5. the window lives on to h + 1 iff h + 1 < len[b] and term[h][b] == 0; then for each of its rows cur_obs[row] =
 *      p_next_obs[row] (CMBPO_REPLAY_OPEN_LOOP) or next_obs[h][b] (CMBPO_REPLAY_ONE_STEP: every particle restarts from the
 *      recording, a one-step PIT at every h); otherwise alive = 0 in its S rows.  Rows of a dead window are frozen.
 *   sums   [H][4 C + 2]:        sum_abs [C] | sum_pair [C] | sum_se [C] | sum_var [C] | brier_term | brier_cost
 *   counts [H][C (S + 1) + 2]:  rank_hist [C][S + 1] | n | n_nonfinite
 * One workgroup takes 64 consecutive rows = 64 / S whole windows; per-workgroup partials (slot = workgroup,
 * cmbpo_replay_particles_parts(B, S) slots per horizon, every entry of a slot written on every call) are added in slot order by
 * the finish call: no floating-point atomics, two runs are bitwise equal.  The workgroup stages its 64 x obs_dim tile of
 * predictions and its windows' recording in LDS; an obs_dim above CMBPO_REPLAY_PARTICLES_MAX_OBS (a chosen cap, below
 * what the LDS of a gfx950 workgroup holds at every S: the tile of 384 columns at S = 2 takes 144 of its 160 KiB) is refused, not
 * split.  cmbpo_replay_t and the three other descriptors are what they were. */
#define CMBPO_REPLAY_PARTICLES_MAX_OBS 384

typedef struct cmbpo_replay_particles {
  int32_t B, H, S, obs_dim, act_dim, mode, reserved, reserved2;  /* windows; horizons; particles; ...; the last two must be 0 */
  /* recorded, time-major */
  const float *act;         /* [H,R,act]  the recorded actions, expanded to rows (cmbpo_replay_run_particles only) */
  const float *next_obs;    /* [H,B,obs]                                        */
  const float *rew, *cost;  /* [H,B]                                            */
  const uint8_t *term;      /* [H,B]                                            */
  const int32_t *len;       /* [B] real steps of the window, 1 .. H             */
  const float *xi;          /* [H,R,obs] N(0,1) draws of the transition noise (cmbpo_replay_run_particles only) */
  /* state, R = B S rows */
  float *cur_obs;           /* [R,obs] the observation step h starts from       */
  uint8_t *alive;           /* [R]                                              */
  /* the post step's outputs, row indexed */
  float *p_next_obs;        /* [R,obs]                                          */
  float *p_rew;             /* [R]                                              */
  uint8_t *p_term;          /* [R]                                              */
  float *p_cost, *p_dkl_path, *p_ep_var_mean; /* [R] (the last two: cmbpo_replay_run_particles only) */
  float *mean, *var;        /* [E,R,model out_dim] scratch of the forward (cmbpo_replay_run_particles only) */
  /* partial sums and the result table */
  double *part_sum;         /* [H][parts][4 (obs + 1) + 2]                      */
  int64_t *part_cnt;        /* [H][parts][(obs + 1) (S + 1) + 2]                */
  double *sums;             /* [H][4 (obs + 1) + 2]                             */
  int64_t *counts;          /* [H][(obs + 1) (S + 1) + 2]                       */
} cmbpo_replay_particles_t; /* 200 bytes */

/* Every entry: CMBPO_EINVAL with a message naming the entry point for a NULL descriptor, B < 1, H < 1, S not a power of two in
 * 2..64, B S beyond int32, obs_dim outside [1, CMBPO_REPLAY_PARTICLES_MAX_OBS], an unknown mode, reserved != 0, a NULL array it
 * uses, h outside [0, H) -- all before any HIP call. */
/* partial-sum slots per horizon of B windows of S particles: ceil(B S / 64) (0 for B < 1 or a refused S) */
int cmbpo_replay_particles_parts(int B, int S);
/* one horizon step of the particle statistics and the advance, on the prediction arrays in *rp */
int cmbpo_replay_particles(const cmbpo_replay_particles_t *rp, int h, void *stream);
/* partials -> sums / counts, all H horizons */
int cmbpo_replay_particles_finish(const cmbpo_replay_particles_t *rp, void *stream);
/* H x (cmbpo_ens_forward on all R rows -> the post step with xi, th, ch -> cmbpo_replay_particles), then the finish call, enqueued
 * without a host wait; bitwise the result of the same calls issued one at a time.  d_elite is [H][R]: the member of every row at
 * every step.  xi == NULL is refused (a particle replay without noise is S copies of the plain replay's rows per member draw:
 * hand zeros if that is what is wanted).  th / ch and `task` as for cmbpo_replay_run_cost, with the same out_dim refusals; the
 * callees' own refusals are passed on under this entry point's name. */
int cmbpo_replay_run_particles(const cmbpo_replay_particles_t *rp, const cmbpo_term_head_t *th, const cmbpo_cost_head_t *ch,
                               cmbpo_mlp_t *model, int task, int ensemble, const int32_t *d_elite, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CMBPO_HIP_H */
