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

cmbpo_rule_derived_table_t g_derived[CMBPO_TASK_USER_SLOTS];     // beside g_rules, slot for slot; all zeros: no derived quantities
const cmbpo_rule_derived_table_t kNoDerived = {};

constexpr int kAllFlags = CMBPO_RULE_ABS | CMBPO_RULE_LO_STRICT | CMBPO_RULE_HI_STRICT | CMBPO_RULE_ANY;

static_assert(sizeof(cmbpo_rule_clause_t) == 32 && sizeof(cmbpo_task_rules_t) == 528, "clause table layout");
static_assert(sizeof(cmbpo_rule_term_t) == 16 && sizeof(cmbpo_rule_derived_t) == 80 && sizeof(cmbpo_rule_derived_table_t) == 656,
              "derived table layout");

// the checks of the clause table; `who` is the entry point's name, `n_derived` the number of derived quantities a clause may
// address (0: CMBPO_RULE_SRC_DERIVED is an unknown source, as it always was for cmbpo_task_rules_register)
int check_rules(const char *who, const cmbpo_task_rules_t *rules, int n_derived) {
  CMBPO_REQUIRE(rules->n_clauses >= 0 && rules->n_clauses <= CMBPO_RULE_MAX_CLAUSES, "%s: n_clauses %d not in [0, %d]", who,
                rules->n_clauses, CMBPO_RULE_MAX_CLAUSES);
  CMBPO_REQUIRE(rules->require_finite == 0 || rules->require_finite == 1, "%s: require_finite %d is not 0 or 1", who, rules->require_finite);
  CMBPO_REQUIRE(rules->cost_on_term == 0 || rules->cost_on_term == 1, "%s: cost_on_term %d is not 0 or 1", who, rules->cost_on_term);
  CMBPO_REQUIRE(rules->reserved == 0, "%s: reserved %d must be 0", who, rules->reserved);
  const int max_src = n_derived > 0 ? CMBPO_RULE_SRC_DERIVED : CMBPO_RULE_SRC_ACT;
  for (int i = 0; i < rules->n_clauses; ++i) {
    const cmbpo_rule_clause_t &c = rules->clause[i];
    CMBPO_REQUIRE(c.role >= CMBPO_RULE_HEALTHY && c.role <= CMBPO_RULE_COST, "%s: clause %d: unknown role %d", who, i, c.role);
    CMBPO_REQUIRE(c.src >= CMBPO_RULE_SRC_NEXT_OBS && c.src <= max_src, "%s: clause %d: unknown src %d", who, i, c.src);
    CMBPO_REQUIRE((c.flags & ~kAllFlags) == 0, "%s: clause %d: unknown flags 0x%x", who, i, c.flags);
    CMBPO_REQUIRE(c.n_cols >= 1 || c.n_cols == -1, "%s: clause %d: n_cols %d is neither >= 1 nor -1", who, i, c.n_cols);
    CMBPO_REQUIRE(isfinite(c.scale), "%s: clause %d: scale is not finite", who, i);
    CMBPO_REQUIRE(c.lo == c.lo, "%s: clause %d: lo is NaN", who, i);
    CMBPO_REQUIRE(c.hi == c.hi, "%s: clause %d: hi is NaN", who, i);
    CMBPO_REQUIRE(c.lo <= c.hi, "%s: clause %d: lo %g above hi %g", who, i, (double)c.lo, (double)c.hi);
    if (c.src == CMBPO_RULE_SRC_DERIVED) {
      // the one width known at registration
      const int col0 = c.col0 < 0 ? c.col0 + n_derived : c.col0;
      const int n = c.n_cols == -1 ? n_derived - col0 : c.n_cols;
      CMBPO_REQUIRE(col0 >= 0 && col0 < n_derived && n >= 1 && n <= n_derived - col0,
                    "%s: clause %d: indices (col0 %d, n_cols %d) outside the %d derived quantities", who, i, c.col0, c.n_cols, n_derived);
    }
  }
  return CMBPO_OK;
}

int check_derived(const char *who, const cmbpo_rule_derived_table_t *t) {
  CMBPO_REQUIRE(t->n_derived >= 1 && t->n_derived <= CMBPO_RULE_MAX_DERIVED, "%s: n_derived %d not in [0, %d]", who, t->n_derived,
                CMBPO_RULE_MAX_DERIVED);
  for (int j = 0; j < 3; ++j) CMBPO_REQUIRE(t->reserved[j] == 0, "%s: derived table: reserved[%d] %d must be 0", who, j, t->reserved[j]);
  for (int i = 0; i < t->n_derived; ++i) {
    const cmbpo_rule_derived_t &d = t->derived[i];
    CMBPO_REQUIRE(d.n_terms >= 1 && d.n_terms <= CMBPO_RULE_MAX_TERMS, "%s: derived %d: n_terms %d not in [1, %d]", who, i, d.n_terms,
                  CMBPO_RULE_MAX_TERMS);
    CMBPO_REQUIRE(isfinite(d.bias), "%s: derived %d: bias is not finite", who, i);
    for (int j = 0; j < 2; ++j) CMBPO_REQUIRE(d.reserved[j] == 0, "%s: derived %d: reserved[%d] %d must be 0", who, i, j, d.reserved[j]);
    for (int k = 0; k < d.n_terms; ++k) {
      const cmbpo_rule_term_t &m = d.term[k];
      CMBPO_REQUIRE(m.src >= CMBPO_RULE_SRC_NEXT_OBS && m.src <= CMBPO_RULE_SRC_ACT, "%s: derived %d: term %d: unknown src %d", who, i, k,
                    (int)m.src);
      CMBPO_REQUIRE(m.pow == 1 || m.pow == 2, "%s: derived %d: term %d: pow %d is not 1 or 2", who, i, k, (int)m.pow);
      CMBPO_REQUIRE(isfinite(m.w), "%s: derived %d: term %d: w is not finite", who, i, k);
      CMBPO_REQUIRE(isfinite(m.c), "%s: derived %d: term %d: c is not finite", who, i, k);
    }
  }
  return CMBPO_OK;
}

// the slot of a byte-identical (clause table, derived table) pair, or a new one; g_mu is taken here
int store_rules(const char *who, const cmbpo_task_rules_t *rules, const cmbpo_rule_derived_table_t *derived, int *out_task) {
  std::lock_guard<std::mutex> lock(g_mu);
  for (int s = 0; s < g_count; ++s)
    if (memcmp(&g_rules[s], rules, sizeof(*rules)) == 0 && memcmp(&g_derived[s], derived, sizeof(*derived)) == 0) {
      *out_task = CMBPO_TASK_USER_BASE + s;
      return CMBPO_OK;
    }
  CMBPO_REQUIRE(g_count < CMBPO_TASK_USER_SLOTS, "%s: all %d rule slots are taken", who, CMBPO_TASK_USER_SLOTS);
  memcpy(&g_rules[g_count], rules, sizeof(*rules));
  memcpy(&g_derived[g_count], derived, sizeof(*derived));
  *out_task = CMBPO_TASK_USER_BASE + g_count++;
  return CMBPO_OK;
}

}  // namespace

extern "C" int cmbpo_task_rules_register(const cmbpo_task_rules_t *rules, int *out_task) {
  const char *who = "cmbpo_task_rules_register";
  CMBPO_REQUIRE(rules && out_task, "%s: NULL argument", who);
  if (int rc = check_rules(who, rules, 0)) return rc;
  return store_rules(who, rules, &kNoDerived, out_task);
}

extern "C" int cmbpo_task_rules_register_ex(const cmbpo_task_rules_t *rules, const cmbpo_rule_derived_table_t *derived, int *out_task) {
  if (derived == nullptr || derived->n_derived == 0) return cmbpo_task_rules_register(rules, out_task);
  const char *who = "cmbpo_task_rules_register_ex";
  CMBPO_REQUIRE(rules && out_task, "%s: NULL argument", who);
  if (int rc = check_derived(who, derived)) return rc;
  if (int rc = check_rules(who, rules, derived->n_derived)) return rc;
  return store_rules(who, rules, derived, out_task);
}

extern "C" int cmbpo_task_rules_get(int task, cmbpo_task_rules_t *out) {
  CMBPO_REQUIRE(out, "cmbpo_task_rules_get: NULL argument");
  const int slot = (task & ~CMBPO_TASK_LEARNED_COST) - CMBPO_TASK_USER_BASE;
  std::lock_guard<std::mutex> lock(g_mu);
  CMBPO_REQUIRE(slot >= 0 && slot < g_count, "cmbpo_task_rules_get: rule id %d is not registered", task);
  memcpy(out, &g_rules[slot], sizeof(*out));
  return CMBPO_OK;
}

extern "C" int cmbpo_task_rules_get_derived(int task, cmbpo_rule_derived_table_t *out) {
  CMBPO_REQUIRE(out, "cmbpo_task_rules_get_derived: NULL argument");
  const int slot = (task & ~CMBPO_TASK_LEARNED_COST) - CMBPO_TASK_USER_BASE;
  std::lock_guard<std::mutex> lock(g_mu);
  CMBPO_REQUIRE(slot >= 0 && slot < g_count, "cmbpo_task_rules_get_derived: rule id %d is not registered", task);
  memcpy(out, &g_derived[slot], sizeof(*out));
  return CMBPO_OK;
}

extern "C" int cmbpo_task_rules_count(void) {
  std::lock_guard<std::mutex> lock(g_mu);
  return g_count;
}

int cmbpo_internal_task_rules_resolve(const char *who, int task, int obs_dim, int act_dim, bool have_act, cmbpo_task_rules_t *out,
                                      cmbpo_rule_derived_table_t *out_derived) {
  cmbpo_task_rules_t t;
  cmbpo_rule_derived_table_t dt;
  const int id = task & ~CMBPO_TASK_LEARNED_COST;
  {
    const int slot = id - CMBPO_TASK_USER_BASE;
    std::lock_guard<std::mutex> lock(g_mu);
    CMBPO_REQUIRE(slot >= 0 && slot < g_count, "%s: bad task %d (rule id %d is not registered)", who, task, id);
    memcpy(&t, &g_rules[slot], sizeof(t));
    memcpy(&dt, &g_derived[slot], sizeof(dt));
  }
  for (int i = 0; i < t.n_clauses; ++i) {
    cmbpo_rule_clause_t &c = t.clause[i];
    const bool der = c.src == CMBPO_RULE_SRC_DERIVED;
    const int width = der ? dt.n_derived : (c.src == CMBPO_RULE_SRC_ACT ? act_dim : obs_dim);
    const char *name = der ? "derived" : (c.src == CMBPO_RULE_SRC_ACT ? "act" : (c.src == CMBPO_RULE_SRC_OBS ? "obs" : "next_obs"));
    const int col0 = c.col0 < 0 ? c.col0 + width : c.col0;
    const int n = c.n_cols == -1 ? width - col0 : c.n_cols;
    CMBPO_REQUIRE(col0 >= 0 && col0 < width && n >= 1 && n <= width - col0,
                  "%s: rule id %d, clause %d: columns (col0 %d, n_cols %d) outside %s's width %d", who, id, i, c.col0, c.n_cols, name, width);
    CMBPO_REQUIRE(c.src != CMBPO_RULE_SRC_ACT || have_act, "%s: rule id %d, clause %d reads act, d_act is NULL", who, id, i);
    c.col0 = col0;
    c.n_cols = n;
  }
  for (int i = 0; i < dt.n_derived; ++i)
    for (int k = 0; k < dt.derived[i].n_terms; ++k) {
      cmbpo_rule_term_t &m = dt.derived[i].term[k];
      const int width = m.src == CMBPO_RULE_SRC_ACT ? act_dim : obs_dim;
      const char *name = m.src == CMBPO_RULE_SRC_ACT ? "act" : (m.src == CMBPO_RULE_SRC_OBS ? "obs" : "next_obs");
      const int col = m.col < 0 ? m.col + width : m.col;
      CMBPO_REQUIRE(col >= 0 && col < width, "%s: rule id %d, derived %d: term %d: column %d outside %s's width %d", who, id, i, k, m.col,
                    name, width);
      CMBPO_REQUIRE(m.src != CMBPO_RULE_SRC_ACT || have_act, "%s: rule id %d, derived %d: term %d reads act, d_act is NULL", who, id, i, k);
      m.col = col;
    }
  if (out) *out = t;
  if (out_derived) *out_derived = dt;
  return CMBPO_OK;
}
