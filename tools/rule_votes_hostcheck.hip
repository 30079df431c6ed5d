// Stand-alone host program for a sanitizer build: every host-side check of the ensemble-voted static rules
// (cmbpo_fakeenv_post_votes, cmbpo_rollout_rule_votes_attach / _detach), reached with buffers that are compared with
// NULL and never followed and with n_rows == 0, so nothing is launched and no device is needed.  Build it from the library's
// sources with the host side instrumented and run it on a CPU:
//
//   C=constrained-model-based-policy-optimization_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined tools/rule_votes_hostcheck.hip $C/fakeenv_post.hip $C/rule_votes.hip \
//       $C/task_rules.hip $C/rollout_state.hip $C/common.hip -o tools/_build/rule_votes_hostcheck
//   tools/_build/rule_votes_hostcheck
//
// Exit status 0 and "rule_votes_hostcheck: N checks ok" when every call returned what it should; any sanitizer report fails it.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../include/cmbpo_hip.h"

static int g_checks = 0, g_bad = 0;

static void expect(bool ok, const char *what) {
  ++g_checks;
  if (!ok) {
    ++g_bad;
    fprintf(stderr, "FAILED: %s (last error: %s)\n", what, cmbpo_last_error());
  }
}

static bool says(const char *a, const char *b = nullptr, const char *c = nullptr) {
  const char *m = cmbpo_last_error();
  return strncmp(m, "cmbpo_fakeenv_post_votes", 24) == 0 && strstr(m, a) && (!b || strstr(m, b)) && (!c || strstr(m, c));
}

// one call on host memory: `buf` stands for every required buffer (NULL: none given)
static int post(int task, int ensemble, int obs_dim, int act_dim, float *buf, float kappa_cost, bool dis, const cmbpo_term_head_t *th,
                const float *thr, const cmbpo_rule_votes_t *rv) {
  float *v = dis ? buf : nullptr;
  return cmbpo_fakeenv_post_votes(task, ensemble, obs_dim, act_dim, buf, buf, 0, buf, nullptr, reinterpret_cast<int32_t *>(buf), nullptr,
                                  nullptr, 0, buf, buf, reinterpret_cast<uint8_t *>(buf), buf, buf, buf, nullptr, nullptr, 0.0f, kappa_cost,
                                  v, v, th, nullptr, thr, rv, nullptr);
}

int main() {
  static float host[64];
  uint8_t votes_out[8] = {0};
  const int ANT = CMBPO_TASK_ANTSAFE, HCS = CMBPO_TASK_HCS, LC = CMBPO_TASK_LEARNED_COST;

  for (int bad : {-1, 3, 17}) {
    cmbpo_rule_votes_t rv = {bad, 0, nullptr, nullptr};
    expect(post(ANT, 7, 29, 8, nullptr, 0.0f, false, nullptr, nullptr, &rv) == CMBPO_EINVAL && says("rule votes", "done_members"), "done_members range");
  }
  for (int bad : {-1, 4, 17}) {
    cmbpo_rule_votes_t rv = {0, bad, nullptr, nullptr};
    expect(post(ANT, 7, 29, 8, nullptr, 0.0f, false, nullptr, nullptr, &rv) == CMBPO_EINVAL && says("rule votes", "cost_members"), "cost_members range");
  }
  for (int E : {1, 9, 16}) {
    cmbpo_rule_votes_t rv = {0, 0, nullptr, nullptr};
    expect(post(ANT, E, 29, 8, nullptr, 0.0f, false, nullptr, nullptr, &rv) == CMBPO_EINVAL && says("ensemble"), "ensemble range");
  }
  for (int cm : {CMBPO_TERM_ANY, CMBPO_TERM_MAJORITY, CMBPO_VOTE_MEAN}) {
    cmbpo_rule_votes_t rv = {0, cm, nullptr, nullptr};
    expect(post(ANT | LC, 7, 29, 8, host, 0.0f, false, nullptr, nullptr, &rv) == CMBPO_EINVAL &&
               says("rule votes", "cost_members", "CMBPO_TASK_LEARNED_COST"), "learned cost: cost_members");
  }
  {
    cmbpo_rule_votes_t rv = {0, 0, nullptr, votes_out};
    expect(post(ANT | LC, 7, 29, 8, host, 0.0f, false, nullptr, nullptr, &rv) == CMBPO_EINVAL &&
               says("rule votes", "cost_votes", "CMBPO_TASK_LEARNED_COST"), "learned cost: cost_votes");
    for (int dm = 0; dm <= 2; ++dm) {
      cmbpo_rule_votes_t ok = {dm, 0, votes_out, nullptr};
      expect(post(ANT | LC, 7, 29, 8, host, 0.0f, false, nullptr, nullptr, &ok) == CMBPO_OK, "learned cost: the termination votes stay");
    }
  }
  {
    cmbpo_rule_votes_t rv = {CMBPO_TERM_ANY, 0, nullptr, nullptr};
    cmbpo_term_head_t bare = {0.5f, CMBPO_TERM_ANY, nullptr, nullptr};
    cmbpo_term_head_t full = {0.5f, CMBPO_TERM_ANY, host, votes_out};
    expect(post(ANT, 7, 29, 8, host, 0.0f, false, &bare, nullptr, &rv) == CMBPO_EINVAL && says("rule votes", "term_pred", "term_votes"),
           "a termination head without its outputs");
    expect(post(ANT, 7, 29, 8, host, 0.0f, false, &full, host, &rv) == CMBPO_OK, "a termination head with its outputs and draws");
    expect(post(ANT, 7, 29, 8, host, 0.0f, false, nullptr, host, &rv) == CMBPO_EINVAL && says("termination draws"), "draws without a head");
  }
  {
    cmbpo_rule_votes_t rv = {0, 0, nullptr, nullptr};
    expect(post(0x200 | ANT, 7, 29, 8, nullptr, 0.0f, false, nullptr, nullptr, &rv) == CMBPO_EINVAL && says("bad task"), "bad task");
    expect(post(ANT, 7, 29, 8, nullptr, 0.0f, false, nullptr, nullptr, &rv) == CMBPO_EINVAL && says("NULL buffer"), "NULL buffer");
    expect(post(HCS, 7, 18, 6, host, 0.5f, true, nullptr, nullptr, &rv) == CMBPO_OK, "kappa_cost > 0 on a static cost with the votes");
    expect(post(HCS, 7, 18, 6, host, 0.5f, true, nullptr, nullptr, nullptr) == CMBPO_EINVAL && strstr(cmbpo_last_error(), "kappa_cost"),
           "kappa_cost > 0 on a static cost without the votes");
    expect(post(HCS, 7, 18, 6, host, NAN, true, nullptr, nullptr, &rv) == CMBPO_EINVAL && says("kappa_cost"), "a NaN kappa_cost");
  }
  for (int dm = 0; dm <= 2; ++dm)
    for (int cm = 0; cm <= 3; ++cm) {
      cmbpo_rule_votes_t rv = {dm, cm, votes_out, votes_out};
      expect(post(ANT, 8, 29, 8, host, 0.0f, false, nullptr, nullptr, &rv) == CMBPO_OK, "every mode on no rows");
    }
  // a registered table with derived quantities: resolved on the host before the (absent) launch
  {
    cmbpo_task_rules_t tr = {};
    tr.n_clauses = 1; tr.require_finite = 1; tr.cost_on_term = 1;
    tr.clause[0] = {CMBPO_RULE_COST, CMBPO_RULE_SRC_DERIVED, 0, 1, 0, 1.0f, -INFINITY, 0.25f};
    cmbpo_rule_derived_table_t dt = {};
    dt.n_derived = 1;
    dt.derived[0].n_terms = 1;
    dt.derived[0].term[0] = {CMBPO_RULE_SRC_NEXT_OBS, 2, -1, 1.0f, 0.0f};
    int id = -1;
    expect(cmbpo_task_rules_register_ex(&tr, &dt, &id) == CMBPO_OK && id >= CMBPO_TASK_USER_BASE, "register a derived table");
    cmbpo_rule_votes_t rv = {CMBPO_TERM_MAJORITY, CMBPO_VOTE_MEAN, votes_out, votes_out};
    expect(post(id, 5, 5, 2, host, 0.0f, false, nullptr, nullptr, &rv) == CMBPO_OK, "a registered table on no rows");
    expect(post(id + 1, 5, 5, 2, host, 0.0f, false, nullptr, nullptr, &rv) == CMBPO_EINVAL && says("not registered"), "an unregistered id");
  }
  // the attach beside a rollout struct
  {
    cmbpo_rollout_t r = {};
    int32_t key[32] = {0};
    cmbpo_rule_votes_t rv = {0, 0, nullptr, nullptr}, bad_d = {3, 0, nullptr, nullptr}, bad_c = {0, 4, nullptr, nullptr};
    expect(cmbpo_rollout_rule_votes_attach(&r, &rv) == CMBPO_EINVAL, "attach without iscal");
    expect(cmbpo_rollout_rule_votes_attach(nullptr, nullptr) == CMBPO_EINVAL && cmbpo_rollout_rule_votes_detach(nullptr) == CMBPO_EINVAL, "NULL struct");
    r.iscal = key;
    expect(cmbpo_rollout_rule_votes_attach(&r, &bad_d) == CMBPO_EINVAL && strstr(cmbpo_last_error(), "done_members"), "attach: done_members");
    expect(cmbpo_rollout_rule_votes_attach(&r, &bad_c) == CMBPO_EINVAL && strstr(cmbpo_last_error(), "cost_members"), "attach: cost_members");
    expect(cmbpo_rollout_rule_votes_detach(&r) == CMBPO_OK && cmbpo_rollout_rule_votes_attach(&r, nullptr) == CMBPO_OK, "detach of nothing");
    expect(cmbpo_rollout_rule_votes_attach(&r, &rv) == CMBPO_OK, "attach");
    rv.done_members = CMBPO_TERM_MAJORITY; rv.cost_members = CMBPO_VOTE_MEAN; rv.done_votes = votes_out;
    expect(cmbpo_rollout_rule_votes_attach(&r, &rv) == CMBPO_OK, "attach again replaces");
    expect(cmbpo_rollout_rule_votes_attach(&r, nullptr) == CMBPO_OK && cmbpo_rollout_rule_votes_detach(&r) == CMBPO_OK, "NULL detaches");
  }
  if (g_bad) {
    fprintf(stderr, "rule_votes_hostcheck: %d of %d checks FAILED\n", g_bad, g_checks);
    return 1;
  }
  printf("rule_votes_hostcheck: %d checks ok\n", g_checks);
  return 0;
}
