// Internal (not part of the C-ABI): the ONE call behind the seven cmbpo_fakeenv_post* entry points (fakeenv_post.hip), which the
// one-call rollout step (rollout_step.hip) and the model replay (replay.hip) make directly.
#pragma once
#include "common.h"

// what the ensemble disagreement adds to the post kernel's arguments
struct DisExtra {
  float kappa_rew, kappa_cost;
  float *rew_var, *cost_var;
};

// One post step: the arguments every entry point shares, in the order of cmbpo_fakeenv_post (include/cmbpo_hip.h), and the six
// optional features.  A feature that is off selects the kernel instances without it, with the argument block they always had.
struct FakeenvPostCall {
  int task, ensemble, obs_dim, act_dim;
  const float *mean, *var;
  int ld_rows;
  const float *obs, *act;
  const int32_t *elite, *row_idx, *n_rows_dev;
  int n_rows;
  float *next_obs, *rew;
  uint8_t *term;
  float *cost, *dkl_path, *ep_var_mean, *ep_var;
  const float *xi;                // transition noise; NULL: off
  bool dis_on;                    // ensemble disagreement (its own flag: NULL variance buffers with it on are an error)
  DisExtra dis;
  const cmbpo_term_head_t *th;    // learned termination head; NULL: off
  const cmbpo_cost_head_t *ch;    // how the learned-cost column is read; NULL or kind 0: as a magnitude
  const float *term_thr;          // sampled terminations: a threshold per slot in place of th->threshold; NULL: off (needs th)
  const cmbpo_rule_votes_t *rv;   // ensemble-voted static rules: one more kernel behind the post kernel (rule_votes.hip); NULL: off
};

// Checks the call, then launches the instance for (ensemble size, rule table, xi, dis_on, th, ch, term_thr) and, with rv, the vote
// kernel behind it.  The messages carry the name of the
// narrowest public entry point that can express the call, derived here and nowhere else:
//   0. rv != NULL     cmbpo_fakeenv_post_votes
//   1. else term_thr != NULL cmbpo_fakeenv_post_term_draws
//   2. else ch != NULL cmbpo_fakeenv_post_cost
//   3. else th != NULL cmbpo_fakeenv_post_term
//   4. else dis_on    cmbpo_fakeenv_post_disagreement
//   5. else xi != NULL cmbpo_fakeenv_post_noise
//   6. else           cmbpo_fakeenv_post
int cmbpo_internal_fakeenv_post(const FakeenvPostCall &c, void *stream);

// The vote kernel's host side (rule_votes.hip).  _check_struct: the two modes' ranges; _check: that, ensemble <= 8, the
// learned-cost refusal and the head's two outputs -- host code, before any HIP call.  _launch: one launch on `stream`; `task` is
// the rule id without the flag bit, rules / der the resolved tables of a registered id or NULL.
int cmbpo_internal_rule_votes_check_struct(const char *who, const cmbpo_rule_votes_t *rv);
int cmbpo_internal_rule_votes_check(const char *who, const FakeenvPostCall &c);
int cmbpo_internal_rule_votes_launch(const FakeenvPostCall &c, int task, int out_dim, const cmbpo_task_rules_t *rules,
                                     const cmbpo_rule_derived_table_t *der, void *stream);
