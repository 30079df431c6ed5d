"""NumPy specification of the ensemble-voted static rules (cmbpo_fakeenv_post_votes, include/cmbpo_hip.h).

For a row r with the members' means ``mean[E, ., out]``, variances ``var`` and ``D = obs_dim``, over ALL E members:

    nx_e      = fl32(mu_e[:D] + obs),  mu_e = mean_e, with draws fl32(mean_e + fl32(sqrt(var_e) * xi))
    done_e    = the task's termination rule on (obs, act, nx_e)          the oracle's built-in statics, or TaskRules.numpy_fns()
    cost_e    = the task's cost rule on (obs, act, nx_e) > 0             an indicator; 0 where the task has no cost rule
    votes     = sum_e done_e / sum_e cost_e                              uint8
    rule_done = done_elite (ELITE) | votes > 0 (ANY) | 2 * votes > E (MAJORITY);   term = rule_done | learned_done
    cost      = cost_elite (ELITE) | votes > 0 (ANY) | 2 * votes > E (MAJORITY) | fl32(votes) / fl32(E) (MEAN)
    cost_var  = np.var(cost_e) over the members (disagreement_ref.member_var);  with kappa_cost > 0
    cost      = clip1(disagreement_ref.penalise(cost, cost_var, kappa_cost, +1)),  clip1(c) = c > 1 ? 1 : c

The members are LOOPED through the same NumPy functions that define the elite's rule, one call per member: nothing here restates a
rule.  Pure comparisons, counts and single-rounded float32 operations: everything is compared with the device bit for bit."""
import numpy as np

import disagreement_ref as dref
from oracle import refcpu

ELITE, ANY, MAJORITY, MEAN = 0, 1, 2, 3
MODES = {"elite": ELITE, "any": ANY, "majority": MAJORITY, "mean": MEAN}
F32 = np.float32


def static_fns(task):
    """(term_fn, cost_fn or None) of a built-in task name (the oracle's tables; unknown names are the default task) or a
    TaskRules."""
    if hasattr(task, "numpy_fns"):
        return task.numpy_fns()
    return refcpu.TERMS_BY_TASK.get(task, refcpu.no_done), refcpu.COST_BY_TASK.get(task)


def member_next(obs, mean, var, rows, obs_dim, xi=None):
    """nx[E, n, D] of the rows `rows`: every member's next state, float32 with one rounding per operation."""
    D = int(obs_dim)
    mu = np.ascontiguousarray(mean[:, rows, :D])
    assert mu.dtype == F32 and obs.dtype == F32
    with np.errstate(all="ignore"):
        if xi is not None:
            std = np.sqrt(np.ascontiguousarray(var[:, rows, :D]))          # float32 in, float32 out: correctly rounded
            mu = mu + std * xi[rows][None]                                  # two roundings: the product, then the sum
        return mu + obs[rows][None]


def member_verdicts(task, obs, act, nx):
    """done[E, n] bool, cost[E, n] bool: one call of the task's functions per member."""
    term_fn, cost_fn = static_fns(task)
    E, n = nx.shape[:2]
    done, cost = np.zeros((E, n), bool), np.zeros((E, n), bool)
    with np.errstate(all="ignore"):
        for e in range(E):
            done[e] = np.asarray(term_fn(obs, act, nx[e])).reshape(n).astype(bool)
            if cost_fn is not None:
                cost[e] = np.asarray(cost_fn(obs, act, nx[e])).reshape(n) > 0
    return done, cost


def _vote(hits, inds, mode, E):
    votes = hits.sum(axis=0)
    cols = np.arange(hits.shape[1])
    if mode == ELITE:
        return hits[inds, cols], votes
    if mode == ANY:
        return votes > 0, votes
    if mode == MAJORITY:
        return 2 * votes > E, votes
    raise ValueError(mode)


def rule_votes(task, obs, act, mean, var, inds, obs_dim, done_members="elite", cost_members="elite", rows=None, xi=None,
               learned_done=None, learned_cost=False, dis_on=False, kappa_cost=0.0):
    """dict(term u8, cost f32 or None, cost_var f32 or None, done_votes u8, cost_votes u8 or None, nx_elite) of the rows `rows`
    (default: all).  learned_done: the termination head's verdict per row of `rows` (default: none).  learned_cost: the static cost
    rule is skipped -- cost, cost_var and cost_votes are None (the learned column's values stay what they are)."""
    mean, var, obs, act = (np.asarray(a) for a in (mean, var, obs, act))
    dm, cm = MODES.get(done_members, done_members), MODES.get(cost_members, cost_members)
    E = mean.shape[0]
    rows = np.arange(mean.shape[1]) if rows is None else np.asarray(rows)
    inds = np.asarray(inds)[rows]
    cols = np.arange(len(rows))
    nx = member_next(obs, mean, var, rows, obs_dim, xi)
    done, cost = member_verdicts(task, obs[rows], act[rows], nx)
    rule_done, dvotes = _vote(done, inds, dm, E)
    learned = np.zeros(len(rows), bool) if learned_done is None else np.asarray(learned_done).astype(bool)
    out = dict(term=(rule_done | learned).astype(np.uint8), done_votes=dvotes.astype(np.uint8), nx_elite=nx[inds, cols],
               cost=None, cost_var=None, cost_votes=None, done_e=done, cost_e=cost)
    if learned_cost:
        assert cm == ELITE, "a learned cost has no static cost rule to vote on"
        return out
    cvotes = cost.sum(axis=0)
    if cm == MEAN:
        c = cvotes.astype(F32) / F32(E)
    else:
        c = _vote(cost, inds, cm, E)[0].astype(F32)
    out["cost_votes"] = cvotes.astype(np.uint8)
    if dis_on:
        cv = dref.member_var(cost.astype(F32))
        out["cost_var"] = cv
        if kappa_cost > 0.0:
            c = dref.penalise(c, cv, kappa_cost, +1)
            c = np.where(c > F32(1.0), F32(1.0), c).astype(F32)
    out["cost"] = c.astype(F32)
    return out
