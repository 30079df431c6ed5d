// Stand-alone host program for a sanitizer build: every host-side check of the static rules' votes in the model replay
// (cmbpo_replay_votes, cmbpo_replay_votes_finish, cmbpo_replay_run_votes), reached with buffers that are compared with
// NULL and never followed; every call fails a check, so nothing is launched and no device is needed.  The ensemble forward is
// this program's own stub (the run entry asks it to check a call of no rows; the real one lives in four more sources).  Build it
// from the library's sources with the host side instrumented and run it on a CPU:
//
//   C=constrained-model-based-policy-optimization_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined tools/replay_votes_hostcheck.hip $C/replay.hip $C/fakeenv_post.hip \
//       $C/rule_votes.hip $C/task_rules.hip $C/common.hip -o tools/_build/replay_votes_hostcheck
//   tools/_build/replay_votes_hostcheck
//
// Exit status 0 and "replay_votes_hostcheck: N checks ok" when every call returned what it should; any sanitizer report fails it.
#include <stdio.h>
#include <string.h>

#include "../constrained-model-based-policy-optimization_amd/csrc/ens_mlp_internal.h"
#include "../include/cmbpo_hip.h"

static int g_checks = 0, g_bad = 0, g_forward_calls = 0;

extern "C" int cmbpo_ens_forward(cmbpo_mlp_t *, const float *, int, const float *, int, const int32_t *, const int32_t *, int n_rows, int,
                                 float *, float *, void *) {
  ++g_forward_calls;
  return n_rows == 0 ? CMBPO_OK : CMBPO_EINVAL;      // (a call with rows would mean a check let something through)
}

static void expect(bool ok, const char *what) {
  ++g_checks;
  if (!ok) {
    ++g_bad;
    fprintf(stderr, "FAILED: %s (last error: %s)\n", what, cmbpo_last_error());
  }
}

static bool says(const char *who, const char *a, const char *b = nullptr, const char *c = nullptr) {
  const char *m = cmbpo_last_error();
  const size_t n = strlen(who);
  return strncmp(m, who, n) == 0 && m[n] == ':' && strstr(m, a) && (!b || strstr(m, b)) && (!c || strstr(m, c));
}

static double g_host[64];

static cmbpo_replay_t replay_image() {
  cmbpo_replay_t rp = {};
  rp.B = 5; rp.H = 3; rp.obs_dim = 27; rp.act_dim = 8; rp.mode = CMBPO_REPLAY_OPEN_LOOP;
  float *f = reinterpret_cast<float *>(g_host);
  uint8_t *u = reinterpret_cast<uint8_t *>(g_host);
  rp.act = rp.next_obs = rp.rew = rp.cost = f; rp.term = u; rp.len = reinterpret_cast<int32_t *>(g_host);
  rp.cur_obs = f; rp.alive = u; rp.p_next_obs = rp.p_rew = f; rp.p_term = u; rp.p_cost = rp.p_dkl_path = rp.p_ep_var_mean = f;
  rp.mean = rp.var = f; rp.part_sum = rp.sums = g_host; rp.part_cnt = rp.counts = reinterpret_cast<int64_t *>(g_host);
  return rp;
}

static cmbpo_replay_votes_t votes_image() {
  cmbpo_replay_votes_t rv = {};
  rv.ensemble = 7;
  rv.done_votes = rv.cost_votes = reinterpret_cast<uint8_t *>(g_host);
  rv.term = reinterpret_cast<uint8_t *>(g_host);
  rv.part_cnt = rv.counts = reinterpret_cast<int64_t *>(g_host);
  return rv;
}

static const char *STEP = "cmbpo_replay_votes", *FIN = "cmbpo_replay_votes_finish", *RUN = "cmbpo_replay_run_votes";

int main() {
  const int ANT = CMBPO_TASK_ANTSAFE, LC = CMBPO_TASK_LEARNED_COST;
  cmbpo_mlp model = {};
  model.out_dim = 28;
  const int32_t *elite = reinterpret_cast<int32_t *>(g_host);
  auto run = [&](const cmbpo_replay_t *rp, const cmbpo_replay_votes_t *rv, int task = CMBPO_TASK_ANTSAFE, int ens = 7,
                 const cmbpo_term_head_t *th = nullptr, cmbpo_mlp *m = nullptr, const int32_t *el = nullptr) {
    return cmbpo_replay_run_votes(rp, nullptr, nullptr, rv, th, nullptr, m ? m : &model, task, ens, el ? el : elite, nullptr);
  };

  // the shape refusals of the compare call, in all three
  for (int k = 0; k < 5; ++k) {
    cmbpo_replay_t rp = replay_image();
    const cmbpo_replay_votes_t rv = votes_image();
    const char *word = k == 0 ? (rp.B = 0, "B 0") : k == 1 ? (rp.H = -1, "H -1") : k == 2 ? (rp.mode = 2, "unknown mode 2")
                       : k == 3 ? (rp.obs_dim = 0, "bad dims") : (rp.reserved = 1, "reserved");
    expect(cmbpo_replay_votes(&rp, &rv, 0, nullptr) == CMBPO_EINVAL && says(STEP, word), "shape: step");
    expect(cmbpo_replay_votes_finish(&rp, &rv, nullptr) == CMBPO_EINVAL && says(FIN, word), "shape: finish");
    expect(run(&rp, &rv) == CMBPO_EINVAL && says(RUN, word), "shape: run");
  }
  // the descriptor's own
  {
    const cmbpo_replay_t rp = replay_image();
    cmbpo_replay_votes_t rv = votes_image();
    rv.ensemble = 0;
    expect(cmbpo_replay_votes(&rp, &rv, 0, nullptr) == CMBPO_EINVAL && says(STEP, "vote ensemble 0"), "ensemble 0: step");
    expect(cmbpo_replay_votes_finish(&rp, &rv, nullptr) == CMBPO_EINVAL && says(FIN, "vote ensemble 0"), "ensemble 0: finish");
    expect(run(&rp, &rv, ANT, 0) == CMBPO_EINVAL && says(RUN, "vote ensemble 0"), "ensemble 0: run");
    rv = votes_image();
    rv.reserved = 2;
    expect(cmbpo_replay_votes(&rp, &rv, 0, nullptr) == CMBPO_EINVAL && says(STEP, "vote reserved 2"), "reserved: step");
    expect(cmbpo_replay_votes_finish(&rp, &rv, nullptr) == CMBPO_EINVAL && says(FIN, "vote reserved 2"), "reserved: finish");
    expect(run(&rp, &rv) == CMBPO_EINVAL && says(RUN, "vote reserved 2"), "reserved: run");
    rv = votes_image();
    rv.ensemble = 9;
    expect(cmbpo_replay_votes(&rp, &rv, 0, nullptr) == CMBPO_EINVAL && says(STEP, "vote ensemble 9 outside [1, 8]"), "ensemble 9: step");
    expect(cmbpo_replay_votes_finish(&rp, &rv, nullptr) == CMBPO_EINVAL && says(FIN, "vote ensemble 9 outside [1, 8]"), "ensemble 9: finish");
    expect(run(&rp, &rv, ANT, 9) == CMBPO_EINVAL && says(RUN, "cmbpo_fakeenv_post_votes", "ensemble 9"), "ensemble 9: run passes it on");
    for (int bad : {-1, 3, 17}) {
      rv = votes_image();
      rv.done_members = bad;
      expect(cmbpo_replay_votes(&rp, &rv, 0, nullptr) == CMBPO_EINVAL && says(STEP, "rule votes", "done_members"), "done_members: step");
      expect(cmbpo_replay_votes_finish(&rp, &rv, nullptr) == CMBPO_EINVAL && says(FIN, "rule votes", "done_members"), "done_members: finish");
      expect(run(&rp, &rv) == CMBPO_EINVAL && says(RUN, "cmbpo_fakeenv_post_votes: rule votes", "done_members"), "done_members: run");
    }
    for (int bad : {-1, 4, 17}) {
      rv = votes_image();
      rv.cost_members = bad;
      expect(cmbpo_replay_votes(&rp, &rv, 0, nullptr) == CMBPO_EINVAL && says(STEP, "rule votes", "cost_members"), "cost_members: step");
      expect(cmbpo_replay_votes_finish(&rp, &rv, nullptr) == CMBPO_EINVAL && says(FIN, "rule votes", "cost_members"), "cost_members: finish");
      expect(run(&rp, &rv) == CMBPO_EINVAL && says(RUN, "cmbpo_fakeenv_post_votes: rule votes", "cost_members"), "cost_members: run");
    }
    // a learned cost: nothing to vote on, nothing to count
    for (int cm : {CMBPO_TERM_ANY, CMBPO_TERM_MAJORITY, CMBPO_VOTE_MEAN}) {
      rv = votes_image();
      rv.cost_members = cm;
      expect(run(&rp, &rv, ANT | LC) == CMBPO_EINVAL && says(RUN, "rule votes", "cost_members", "CMBPO_TASK_LEARNED_COST"), "learned cost: cost_members");
    }
    rv = votes_image();
    expect(run(&rp, &rv, ANT | LC) == CMBPO_EINVAL && says(RUN, "rule votes", "cost_votes", "CMBPO_TASK_LEARNED_COST"), "learned cost: cost_votes");
    // a termination head must bring both of its outputs
    cmbpo_mlp with_head = {};
    with_head.out_dim = 29;
    const cmbpo_term_head_t bare = {0.5f, CMBPO_TERM_ELITE, nullptr, nullptr};
    expect(run(&rp, &rv, ANT, 7, &bare, &with_head) == CMBPO_EINVAL && says(RUN, "term_pred", "term_votes"), "a termination head without its outputs");
    expect(run(&rp, &rv, ANT, 7, &bare) == CMBPO_EINVAL && says(RUN, "termination head", "out_dim 28"), "a termination head on a model without its column");
    // the run entry's own: the handle, the ensemble, d_elite
    expect(cmbpo_replay_run_votes(&rp, nullptr, nullptr, &rv, nullptr, nullptr, nullptr, ANT, 7, elite, nullptr) == CMBPO_EINVAL && says(RUN, "model"),
           "model handle");
    expect(run(&rp, &rv, ANT, 5) == CMBPO_EINVAL && says(RUN, "ensemble 5, the vote descriptor's is 7"), "the run's ensemble");
    expect(cmbpo_replay_run_votes(&rp, nullptr, nullptr, &rv, nullptr, nullptr, &model, ANT, 7, nullptr, nullptr) == CMBPO_EINVAL && says(RUN, "d_elite"),
           "d_elite");
    // h outside [0, H); cost_votes and the descriptor's own terminals are optional
    rv = votes_image();
    rv.cost_votes = nullptr; rv.term = nullptr;
    for (int h : {-1, 3, 1 << 20})
      expect(cmbpo_replay_votes(&rp, &rv, h, nullptr) == CMBPO_EINVAL && says(STEP, "outside [0, 3)"), "h range");
  }
  // NULL descriptors and arrays
  {
    const cmbpo_replay_t rp = replay_image();
    const cmbpo_replay_votes_t rv = votes_image();
    expect(cmbpo_replay_votes(nullptr, &rv, 0, nullptr) == CMBPO_EINVAL && says(STEP, "NULL"), "NULL rp: step");
    expect(cmbpo_replay_votes(&rp, nullptr, 0, nullptr) == CMBPO_EINVAL && says(STEP, "NULL"), "NULL rv: step");
    expect(cmbpo_replay_votes_finish(nullptr, &rv, nullptr) == CMBPO_EINVAL && says(FIN, "NULL"), "NULL rp: finish");
    expect(cmbpo_replay_votes_finish(&rp, nullptr, nullptr) == CMBPO_EINVAL && says(FIN, "NULL"), "NULL rv: finish");
    expect(run(nullptr, &rv) == CMBPO_EINVAL && says(RUN, "NULL"), "NULL rp: run");
    // rv == NULL is cmbpo_replay_run_reliab's call, under that entry's name rules (nothing else given: the plain run's)
    expect(cmbpo_replay_run_votes(&rp, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 7, nullptr, nullptr) == CMBPO_EINVAL &&
               says("cmbpo_replay_run", "model"), "rv == NULL: the plain run's name");
    cmbpo_replay_votes_t v = votes_image();
    v.done_votes = nullptr;
    expect(cmbpo_replay_votes(&rp, &v, 0, nullptr) == CMBPO_EINVAL && says(STEP, "done_votes"), "NULL done_votes: step");
    expect(run(&rp, &v) == CMBPO_EINVAL && says(RUN, "done_votes"), "NULL done_votes: run");
    v = votes_image();
    v.part_cnt = nullptr;
    expect(cmbpo_replay_votes(&rp, &v, 0, nullptr) == CMBPO_EINVAL && says(STEP, "vote partials"), "NULL partials: step");
    expect(cmbpo_replay_votes_finish(&rp, &v, nullptr) == CMBPO_EINVAL && says(FIN, "vote partials"), "NULL partials: finish");
    expect(run(&rp, &v) == CMBPO_EINVAL && says(RUN, "vote partials"), "NULL partials: run");
    v = votes_image();
    v.counts = nullptr;
    expect(cmbpo_replay_votes_finish(&rp, &v, nullptr) == CMBPO_EINVAL && says(FIN, "vote table"), "NULL table: finish");
    expect(run(&rp, &v) == CMBPO_EINVAL && says(RUN, "vote table"), "NULL table: run");
    cmbpo_replay_t r = replay_image();
    r.alive = nullptr;
    expect(cmbpo_replay_votes(&r, &rv, 0, nullptr) == CMBPO_EINVAL && says(STEP, "NULL buffer"), "NULL alive: step");
    r = replay_image();
    r.mean = nullptr;
    expect(run(&r, &rv) == CMBPO_EINVAL && says(RUN, "NULL buffer"), "NULL mean: run");
  }
  expect(g_forward_calls == 0, "no call got as far as the forward");
  if (g_bad) {
    fprintf(stderr, "replay_votes_hostcheck: %d of %d checks FAILED\n", g_bad, g_checks);
    return 1;
  }
  printf("replay_votes_hostcheck: %d checks ok\n", g_checks);
  return 0;
}
