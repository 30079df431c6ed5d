// User-defined termination / cost rules: the table of registered clause sets behind the rule ids CMBPO_TASK_USER_BASE + slot.
// Host code only -- a launch takes its table by value in the kernel arguments (csrc/fakeenv_post.hip), so there is no device
// copy and nothing per device to keep in step.
#include "common.h"

#include <math.h>
#include <string.h>

#include <mutex>

namespace {

std::mutex g_mu;
cmbpo_task_rules_t g_rules[CMBPO_TASK_USER_SLOTS];
int g_count = 0;

constexpr int kAllFlags = CMBPO_RULE_ABS | CMBPO_RULE_LO_STRICT | CMBPO_RULE_HI_STRICT | CMBPO_RULE_ANY;

}  // namespace

extern "C" int cmbpo_task_rules_register(const cmbpo_task_rules_t *rules, int *out_task) {
  CMBPO_REQUIRE(rules && out_task, "cmbpo_task_rules_register: NULL argument");
  CMBPO_REQUIRE(rules->n_clauses >= 0 && rules->n_clauses <= CMBPO_RULE_MAX_CLAUSES,
                "cmbpo_task_rules_register: n_clauses %d not in [0, %d]", rules->n_clauses, CMBPO_RULE_MAX_CLAUSES);
  CMBPO_REQUIRE(rules->require_finite == 0 || rules->require_finite == 1, "cmbpo_task_rules_register: require_finite %d is not 0 or 1",
                rules->require_finite);
  CMBPO_REQUIRE(rules->cost_on_term == 0 || rules->cost_on_term == 1, "cmbpo_task_rules_register: cost_on_term %d is not 0 or 1",
                rules->cost_on_term);
  CMBPO_REQUIRE(rules->reserved == 0, "cmbpo_task_rules_register: reserved %d must be 0", rules->reserved);
  for (int i = 0; i < rules->n_clauses; ++i) {
    const cmbpo_rule_clause_t &c = rules->clause[i];
    CMBPO_REQUIRE(c.role >= CMBPO_RULE_HEALTHY && c.role <= CMBPO_RULE_COST, "cmbpo_task_rules_register: clause %d: unknown role %d", i, c.role);
    CMBPO_REQUIRE(c.src >= CMBPO_RULE_SRC_NEXT_OBS && c.src <= CMBPO_RULE_SRC_ACT, "cmbpo_task_rules_register: clause %d: unknown src %d", i,
                  c.src);
    CMBPO_REQUIRE((c.flags & ~kAllFlags) == 0, "cmbpo_task_rules_register: clause %d: unknown flags 0x%x", i, c.flags);
    CMBPO_REQUIRE(c.n_cols >= 1 || c.n_cols == -1, "cmbpo_task_rules_register: clause %d: n_cols %d is neither >= 1 nor -1", i, c.n_cols);
    CMBPO_REQUIRE(isfinite(c.scale), "cmbpo_task_rules_register: clause %d: scale is not finite", i);
    CMBPO_REQUIRE(c.lo == c.lo, "cmbpo_task_rules_register: clause %d: lo is NaN", i);
    CMBPO_REQUIRE(c.hi == c.hi, "cmbpo_task_rules_register: clause %d: hi is NaN", i);
    CMBPO_REQUIRE(c.lo <= c.hi, "cmbpo_task_rules_register: clause %d: lo %g above hi %g", i, (double)c.lo, (double)c.hi);
  }
  std::lock_guard<std::mutex> lock(g_mu);
  for (int s = 0; s < g_count; ++s)
    if (memcmp(&g_rules[s], rules, sizeof(*rules)) == 0) {
      *out_task = CMBPO_TASK_USER_BASE + s;
      return CMBPO_OK;
    }
  CMBPO_REQUIRE(g_count < CMBPO_TASK_USER_SLOTS, "cmbpo_task_rules_register: all %d rule slots are taken", CMBPO_TASK_USER_SLOTS);
  memcpy(&g_rules[g_count], rules, sizeof(*rules));
  *out_task = CMBPO_TASK_USER_BASE + g_count++;
  return CMBPO_OK;
}

extern "C" int cmbpo_task_rules_get(int task, cmbpo_task_rules_t *out) {
  CMBPO_REQUIRE(out, "cmbpo_task_rules_get: NULL argument");
  const int slot = (task & ~CMBPO_TASK_LEARNED_COST) - CMBPO_TASK_USER_BASE;
  std::lock_guard<std::mutex> lock(g_mu);
  CMBPO_REQUIRE(slot >= 0 && slot < g_count, "cmbpo_task_rules_get: rule id %d is not registered", task);
  memcpy(out, &g_rules[slot], sizeof(*out));
  return CMBPO_OK;
}

extern "C" int cmbpo_task_rules_count(void) {
  std::lock_guard<std::mutex> lock(g_mu);
  return g_count;
}

int cmbpo_internal_task_rules_resolve(const char *who, int task, int obs_dim, int act_dim, bool have_act, cmbpo_task_rules_t *out) {
  cmbpo_task_rules_t t;
  const int id = task & ~CMBPO_TASK_LEARNED_COST;
  {
    const int slot = id - CMBPO_TASK_USER_BASE;
    std::lock_guard<std::mutex> lock(g_mu);
    CMBPO_REQUIRE(slot >= 0 && slot < g_count, "%s: bad task %d (rule id %d is not registered)", who, task, id);
    memcpy(&t, &g_rules[slot], sizeof(t));
  }
  for (int i = 0; i < t.n_clauses; ++i) {
    cmbpo_rule_clause_t &c = t.clause[i];
    const int width = c.src == CMBPO_RULE_SRC_ACT ? act_dim : obs_dim;
    const char *name = c.src == CMBPO_RULE_SRC_ACT ? "act" : (c.src == CMBPO_RULE_SRC_OBS ? "obs" : "next_obs");
    const int col0 = c.col0 < 0 ? c.col0 + width : c.col0;
    const int n = c.n_cols == -1 ? width - col0 : c.n_cols;
    CMBPO_REQUIRE(col0 >= 0 && col0 < width && n >= 1 && n <= width - col0,
                  "%s: rule id %d, clause %d: columns (col0 %d, n_cols %d) outside %s's width %d", who, id, i, c.col0, c.n_cols, name, width);
    CMBPO_REQUIRE(c.src != CMBPO_RULE_SRC_ACT || have_act, "%s: rule id %d, clause %d reads act, d_act is NULL", who, id, i);
    c.col0 = col0;
    c.n_cols = n;
  }
  if (out) *out = t;
  return CMBPO_OK;
}
