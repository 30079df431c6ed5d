// Internal (not part of the C-ABI): the pieces of rollout_state.hip that the one-call rollout step (rollout_step.hip) launches.
#pragma once
#include "common.h"

// what is attached beside *r (cmbpo_rollout_iv_attach / _disagreement_attach / _value_disagreement_attach / _term_head_attach /
// _cost_head_attach / _term_draws_attach / _rule_votes_attach); a feature that is not: all-zero (an all-zero cmbpo_term_head_t is a valid head and an all-zero
// cmbpo_cost_head_t the magnitude reading, so those two have a flag)
struct RolloutSide {
  cmbpo_iv_gae_t iv;
  cmbpo_disagreement_t dg;
  cmbpo_value_disagreement_t vd;
  cmbpo_term_head_t th;
  int th_on;
  cmbpo_cost_head_t ch;
  int ch_on;
  const float *thr;       // sampled terminations: this step's thresholds [B], slot indexed; NULL: the head's own threshold
  long thr_stride;        // floats between two steps of a cmbpo_rollout_run call
  cmbpo_rule_votes_t rv;  // ensemble-voted static rules (an all-zero struct is the valid measure-nothing vote: a flag)
  int rv_on;
};
RolloutSide cmbpo_internal_side_lookup(const cmbpo_rollout_t *r);

// One host launcher per bookkeeping kernel: the public entry of the same name calls it with the side state it looked up, the
// one-call step with the one it looked up for the whole step.  `who` names the entry point in the messages.
// with_stats == 0: without the statistics launch -- finish(POST) with fold_stats == 1 folds the step's sums instead
int cmbpo_internal_store(const cmbpo_rollout_t *r, const RolloutSide &sd, int with_stats, const char *who, void *stream);
int cmbpo_internal_finish(const cmbpo_rollout_t *r, const RolloutSide &sd, int mode, int fold_stats, const char *who, void *stream);
// spec: the step was enqueued ahead of the previous step's counters (n_alive is an upper bound then).  with_vec == 0: the vector
// half of the store rides in the critics' launch (CmbpoStoreVec) instead of store_vec_kernel.
int cmbpo_internal_book_pre(const cmbpo_rollout_t *r, const RolloutSide &sd, int n_alive, int spec, int with_vec, const char *who,
                            void *stream);
// d_host_out != NULL: the counters mirrored into host-mapped memory (device address of 128 dwords) and `seq` behind them
int cmbpo_internal_book_post(const cmbpo_rollout_t *r, const RolloutSide &sd, int n_alive, uint32_t *d_host_out, uint32_t seq, int spec,
                             int min_alive, double stop_total, const char *who, void *stream);
int cmbpo_internal_scalars_mirror(const cmbpo_rollout_t *r, uint32_t *d_host_out, uint32_t seq, void *stream);
int cmbpo_internal_spec_words(const cmbpo_rollout_t *r, int begin, void *stream);
