// Internal (not part of the C-ABI): the pieces of rollout_state.hip that the one-call rollout step (rollout_step.hip) launches.
#pragma once
#include "common.h"

int cmbpo_internal_book_post_mirror(const cmbpo_rollout_t *r, int n_alive, uint32_t *d_host_out, uint32_t seq, int spec, int min_alive,
                                    double stop_total, void *stream);
int cmbpo_internal_scalars_mirror(const cmbpo_rollout_t *r, uint32_t *d_host_out, uint32_t seq, void *stream);
int cmbpo_internal_book_pre(const cmbpo_rollout_t *r, int n_alive, int spec, int with_vec, void *stream);
int cmbpo_internal_store_nostats(const cmbpo_rollout_t *r, void *stream);
int cmbpo_internal_finish_post_fold(const cmbpo_rollout_t *r, void *stream);
int cmbpo_internal_spec_words(const cmbpo_rollout_t *r, int begin, void *stream);
// the disagreement state attached beside *r (all-zero and 0 if none): the one-call step post-processes with it
int cmbpo_internal_disagreement_lookup(const cmbpo_rollout_t *r, cmbpo_disagreement_t *out);
