// Stand-alone host program for a sanitizer build: every host-side check of the particle replay (cmbpo_replay_particles,
// cmbpo_replay_particles_finish, cmbpo_replay_run_particles, cmbpo_replay_particles_parts), reached with buffers that
// are compared with NULL and never followed; every call fails a check, so nothing is launched and no device is needed.  The
// ensemble forward is this program's own stub (the run entry asks it to check a call of no rows; the real one lives in four more
// sources).  Build it from the library's sources with the host side instrumented and run it on a CPU:
//
//   C=constrained-model-based-policy-optimization_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined tools/replay_particles_hostcheck.hip $C/replay.hip $C/fakeenv_post.hip \
//       $C/rule_votes.hip $C/task_rules.hip $C/common.hip -o tools/_build/replay_particles_hostcheck
//   tools/_build/replay_particles_hostcheck
//
// Exit status 0 and "replay_particles_hostcheck: N checks ok" when every call returned what it should; any sanitizer report fails it.
#include <stdio.h>
#include <string.h>

#include "../constrained-model-based-policy-optimization_amd/csrc/ens_mlp_internal.h"
#include "../include/cmbpo_hip.h"

static int g_checks = 0, g_bad = 0, g_forward_calls = 0, g_forward_rows = 0;

extern "C" int cmbpo_ens_forward(cmbpo_mlp_t *, const float *, int, const float *, int, const int32_t *, const int32_t *, int n_rows, int,
                                 float *, float *, void *) {
  ++g_forward_calls;
  g_forward_rows += n_rows;
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

static cmbpo_replay_particles_t image() {
  cmbpo_replay_particles_t rp = {};
  rp.B = 5; rp.H = 3; rp.S = 8; rp.obs_dim = 27; rp.act_dim = 8; rp.mode = CMBPO_REPLAY_OPEN_LOOP;
  float *f = reinterpret_cast<float *>(g_host);
  uint8_t *u = reinterpret_cast<uint8_t *>(g_host);
  rp.act = rp.next_obs = rp.rew = rp.cost = rp.xi = f; rp.term = u; rp.len = reinterpret_cast<int32_t *>(g_host);
  rp.cur_obs = f; rp.alive = u; rp.p_next_obs = rp.p_rew = f; rp.p_term = u; rp.p_cost = rp.p_dkl_path = rp.p_ep_var_mean = f;
  rp.mean = rp.var = f; rp.part_sum = rp.sums = g_host; rp.part_cnt = rp.counts = reinterpret_cast<int64_t *>(g_host);
  return rp;
}

static const char *STEP = "cmbpo_replay_particles", *FIN = "cmbpo_replay_particles_finish", *RUN = "cmbpo_replay_run_particles";

int main() {
  static_assert(sizeof(cmbpo_replay_particles_t) == 200, "the descriptor's documented size");
  static_assert(sizeof(cmbpo_replay_t) == 184, "cmbpo_replay_t is what it was");
  const int ANT = CMBPO_TASK_ANTSAFE, LC = CMBPO_TASK_LEARNED_COST;
  cmbpo_mlp model = {};
  model.out_dim = 28;
  const int32_t *elite = reinterpret_cast<int32_t *>(g_host);
  auto run = [&](const cmbpo_replay_particles_t *rp, int task = CMBPO_TASK_ANTSAFE, int ens = 7, const cmbpo_term_head_t *th = nullptr,
                 const cmbpo_cost_head_t *ch = nullptr, cmbpo_mlp *m = nullptr) {
    return cmbpo_replay_run_particles(rp, th, ch, m ? m : &model, task, ens, elite, nullptr);
  };
  auto all_three = [&](const cmbpo_replay_particles_t &rp, const char *word, const char *what) {
    expect(cmbpo_replay_particles(&rp, 0, nullptr) == CMBPO_EINVAL && says(STEP, word), what);
    expect(cmbpo_replay_particles_finish(&rp, nullptr) == CMBPO_EINVAL && says(FIN, word), what);
    expect(run(&rp) == CMBPO_EINVAL && says(RUN, word), what);
  };

  // the slots per horizon: ceil(B S / 64), 0 for what the entries refuse
  expect(cmbpo_replay_particles_parts(37, 8) == 5 && cmbpo_replay_particles_parts(5, 64) == 5 && cmbpo_replay_particles_parts(130, 2) == 5 &&
             cmbpo_replay_particles_parts(1, 2) == 1 && cmbpo_replay_particles_parts(32, 2) == 1 && cmbpo_replay_particles_parts(33, 2) == 2,
         "parts");
  expect(cmbpo_replay_particles_parts(0, 8) == 0 && cmbpo_replay_particles_parts(-3, 8) == 0 && cmbpo_replay_particles_parts(4, 3) == 0 &&
             cmbpo_replay_particles_parts(4, 128) == 0 && cmbpo_replay_particles_parts(4, 1) == 0 && cmbpo_replay_particles_parts(1 << 30, 64) == 0,
         "parts of a refused shape");

  // the shape refusals, in all three
  for (int k = 0; k < 8; ++k) {
    cmbpo_replay_particles_t rp = image();
    const char *word = k == 0 ? (rp.B = 0, "B 0") : k == 1 ? (rp.H = -1, "H -1") : k == 2 ? (rp.mode = 2, "unknown mode 2")
                       : k == 3 ? (rp.obs_dim = 0, "bad dims") : k == 4 ? (rp.reserved = 1, "reserved")
                       : k == 5 ? (rp.reserved2 = 7, "reserved") : k == 6 ? (rp.act_dim = -1, "bad dims")
                                : (rp.B = 1 << 30, "below 2^31");
    all_three(rp, word, "shape");
  }
  // S: a power of two in 2..64
  for (int S : {3, 128, 1, 0, -2, 6, 48, 65}) {
    cmbpo_replay_particles_t rp = image();
    rp.S = S;
    all_three(rp, "not a power of two in 2..64", "S");
  }
  for (int S : {2, 4, 8, 16, 32, 64}) {         // every S the kernel takes gets past the shape checks: the next refusal is h
    cmbpo_replay_particles_t rp = image();
    rp.S = S;
    expect(cmbpo_replay_particles(&rp, 3, nullptr) == CMBPO_EINVAL && says(STEP, "h 3 outside [0, 3)"), "a good S");
  }
  // an obs_dim the staged tile cannot hold: refused in words, not split
  {
    cmbpo_replay_particles_t rp = image();
    rp.obs_dim = CMBPO_REPLAY_PARTICLES_MAX_OBS + 1;
    all_three(rp, "cannot hold", "obs_dim above the staging");
    rp.obs_dim = CMBPO_REPLAY_PARTICLES_MAX_OBS; rp.S = 2;      // the widest tile there is gets past it
    expect(cmbpo_replay_particles(&rp, -1, nullptr) == CMBPO_EINVAL && says(STEP, "h -1 outside"), "the widest obs_dim at S = 2");
  }
  // h outside [0, H)
  {
    const cmbpo_replay_particles_t rp = image();
    for (int h : {-1, 3, 1 << 20}) expect(cmbpo_replay_particles(&rp, h, nullptr) == CMBPO_EINVAL && says(STEP, "outside [0, 3)"), "h range");
  }
  // NULL descriptors and arrays
  {
    expect(cmbpo_replay_particles(nullptr, 0, nullptr) == CMBPO_EINVAL && says(STEP, "NULL"), "NULL rp: step");
    expect(cmbpo_replay_particles_finish(nullptr, nullptr) == CMBPO_EINVAL && says(FIN, "NULL"), "NULL rp: finish");
    expect(run(nullptr) == CMBPO_EINVAL && says(RUN, "NULL"), "NULL rp: run");
    cmbpo_replay_particles_t r;
#define NULLED(field, word, step, fin)                                                                                   \
    r = image(); r.field = nullptr;                                                                                      \
    if (step) expect(cmbpo_replay_particles(&r, 0, nullptr) == CMBPO_EINVAL && says(STEP, word), "NULL " #field ": step");  \
    if (fin) expect(cmbpo_replay_particles_finish(&r, nullptr) == CMBPO_EINVAL && says(FIN, word), "NULL " #field ": finish"); \
    expect(run(&r) == CMBPO_EINVAL && says(RUN, word), "NULL " #field ": run");
    NULLED(next_obs, "recorded arrays", 1, 0) NULLED(rew, "recorded arrays", 1, 0) NULLED(cost, "recorded arrays", 1, 0)
    NULLED(term, "recorded arrays", 1, 0) NULLED(len, "recorded arrays", 1, 0)
    NULLED(cur_obs, "cur_obs / alive", 1, 0) NULLED(alive, "cur_obs / alive", 1, 0)
    NULLED(p_next_obs, "predictions", 1, 0) NULLED(p_rew, "predictions", 1, 0) NULLED(p_term, "predictions", 1, 0)
    NULLED(p_cost, "predictions", 1, 0)
    NULLED(part_sum, "partials", 1, 1) NULLED(part_cnt, "partials", 1, 1)
    NULLED(sums, "result table", 0, 1) NULLED(counts, "result table", 0, 1)
    // what only the run entry uses
    NULLED(xi, "xi", 0, 0) NULLED(act, "act / mean / var", 0, 0) NULLED(mean, "act / mean / var", 0, 0) NULLED(var, "act / mean / var", 0, 0)
    NULLED(p_dkl_path, "p_dkl_path", 0, 0) NULLED(p_ep_var_mean, "p_dkl_path", 0, 0)
#undef NULLED
    // ... and the single-step entries do not ask for them
    r = image();
    r.xi = r.act = nullptr; r.mean = r.var = r.p_dkl_path = r.p_ep_var_mean = nullptr; r.sums = nullptr; r.counts = nullptr;
    expect(cmbpo_replay_particles(&r, 5, nullptr) == CMBPO_EINVAL && says(STEP, "h 5 outside"), "the step entry needs no run-only array");
    r = image();
    r.act_dim = 0; r.act = nullptr; r.xi = nullptr;
    expect(run(&r) == CMBPO_EINVAL && says(RUN, "xi"), "no actions: act may be NULL, xi may not");
  }
  // the run entry's own: the handle, d_elite, the heads against the model's width; the callees' refusals under this entry's name
  {
    const cmbpo_replay_particles_t rp = image();
    expect(cmbpo_replay_run_particles(&rp, nullptr, nullptr, nullptr, ANT, 7, elite, nullptr) == CMBPO_EINVAL && says(RUN, "model"), "model handle");
    expect(cmbpo_replay_run_particles(&rp, nullptr, nullptr, &model, ANT, 7, nullptr, nullptr) == CMBPO_EINVAL && says(RUN, "d_elite"), "d_elite");
    const cmbpo_term_head_t th = {0.5f, CMBPO_TERM_ELITE, nullptr, nullptr};
    expect(run(&rp, ANT, 7, &th) == CMBPO_EINVAL && says(RUN, "termination head", "out_dim 28"), "a termination head on a model without its column");
    cmbpo_cost_head_t ch = {};
    ch.kind = 1;
    expect(run(&rp, ANT | LC, 7, nullptr, &ch) == CMBPO_EINVAL && says(RUN, "logistic cost head", "out_dim 28"), "a logistic cost head on a model without its column");
    expect(run(&rp, ANT, 0) == CMBPO_EINVAL && says(RUN, "cmbpo_fakeenv_post"), "ensemble 0: the post step's refusal, passed on");
    expect(run(&rp, 9) == CMBPO_EINVAL && says(RUN, "cmbpo_fakeenv_post"), "an unknown task: the post step's refusal, passed on");
  }
  expect(g_forward_rows == 0, "no call got as far as a forward with rows");
  if (g_bad) {
    fprintf(stderr, "replay_particles_hostcheck: %d of %d checks FAILED\n", g_bad, g_checks);
    return 1;
  }
  printf("replay_particles_hostcheck: %d checks ok\n", g_checks);
  return 0;
}
