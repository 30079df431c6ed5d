// Internal (not part of the C-ABI): the ONE call behind the six cmbpo_fakeenv_post* entry points (fakeenv_post.hip), which the
// one-call rollout step (rollout_step.hip) and the model replay (replay.hip) make directly.
#pragma once
#include "common.h"

// what the ensemble disagreement adds to the post kernel's arguments
struct DisExtra {
  float kappa_rew, kappa_cost;
  float *rew_var, *cost_var;
};

// One post step: the arguments every entry point shares, in the order of cmbpo_fakeenv_post (include/cmbpo_hip.h), and the five
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
};

// Checks the call, then launches the instance for (ensemble size, rule table, xi, dis_on, th, ch, term_thr).  The messages carry the name of the
// narrowest public entry point that can express the call, derived here and nowhere else:
//   1. term_thr != NULL cmbpo_fakeenv_post_term_draws
//   2. else ch != NULL cmbpo_fakeenv_post_cost
//   3. else th != NULL cmbpo_fakeenv_post_term
//   4. else dis_on    cmbpo_fakeenv_post_disagreement
//   5. else xi != NULL cmbpo_fakeenv_post_noise
//   6. else           cmbpo_fakeenv_post
int cmbpo_internal_fakeenv_post(const FakeenvPostCall &c, void *stream);
