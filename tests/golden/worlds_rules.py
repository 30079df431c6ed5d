"""User-defined termination / cost rules of the G15 traces, twice: as the NumPy functions a user of the reference would add
to ``models/statics.py`` (TERMS_BY_TASK / COST_BY_TASK), and as the builder arguments of the equivalent
``cmbpo_amd.statics.TaskRules``, as plain data.  Shared by make_golden_task_rules.py (which records the traces with the
functions inserted into the reference's tables) and the tests (which replay them with the TaskRules).

Pure functions of their thresholds: nothing here touches the reference tree, so tests can import it on the GPU box.
The worlds are worlds.build_world's (obs + 1 outputs, no cost column).
"""
import numpy as np


# ---- Hopper form: the MBPO-style healthy conjunction, a finiteness guard, a magnitude guard over a slice; scaled cost -------
def hopper_fns(h0, a0, c0):
    def term_fn(obs, act, next_obs):
        assert len(obs.shape) == len(next_obs.shape) == len(act.shape)
        height = next_obs[..., 0]
        angle = next_obs[..., 1]
        not_done = np.isfinite(next_obs).all(axis=-1) \
            * (np.abs(next_obs[..., 1:]) < 100).all(axis=-1) \
            * (height > h0) \
            * (np.abs(angle) < a0)
        done = ~not_done
        return done[..., None]

    def cost_fn(obs, act, next_obs):
        assert len(obs.shape) == len(next_obs.shape) == len(act.shape)
        xdist = next_obs[..., -1] * 10
        return np.array(np.abs(xdist) > c0, dtype=np.float32)[..., None]

    return term_fn, cost_fn


def hopper_rules(h0, a0, c0):
    return dict(clauses=[("healthy", dict(cols=slice(1, None), abs=True, hi=100.0, hi_strict=True)),
                         ("healthy", dict(cols=0, lo=h0, lo_strict=True)),
                         ("healthy", dict(cols=1, abs=True, hi=a0, hi_strict=True)),
                         ("cost", dict(cols=-1, scale=10.0, abs=True, lo=c0, lo_strict=True))],
                require_finite=True, cost_on_term=False)


# ---- fatal form: done = (z < lo) + (z > hi), which a NaN survives; the cost of statics.py:51-52 without an object term ------
def fatal_fns(lo, hi):
    def term_fn(obs, act, next_obs):
        assert len(obs.shape) == len(next_obs.shape) == len(act.shape)
        z = next_obs[..., 0]
        done = (z < lo) + (z > hi)
        return done[..., None]

    def cost_fn(obs, act, next_obs):
        done_cost = term_fn(obs, act, next_obs) * 1.0
        return np.clip(done_cost, 0, 1).astype(np.float32)

    return term_fn, cost_fn


def fatal_rules(lo, hi):
    return dict(clauses=[("fatal", dict(cols=0, hi=lo, hi_strict=True)),
                         ("fatal", dict(cols=0, lo=hi, lo_strict=True))],
                require_finite=False, cost_on_term=True)


# ---- no termination: cost from the two other sources, the action and the observation before the step --------------------
def nodone_fns(a, b):
    def cost_fn(obs, act, next_obs):
        assert len(obs.shape) == len(next_obs.shape) == len(act.shape)
        hit = (np.abs(act) > a).any(axis=-1) | (obs[..., 0] <= b)
        return np.array(hit, dtype=np.float32)[..., None]

    return None, cost_fn


def nodone_rules(a, b):
    return dict(clauses=[("cost", dict(src="act", cols=slice(0, None), abs=True, lo=a, lo_strict=True, any=True)),
                         ("cost", dict(src="obs", cols=0, hi=b))],
                require_finite=False, cost_on_term=False)


# name -> the trace's configuration (make_golden.run_sampler_trace), the two forms of its rules, and the candidate thresholds
# in the order the generator tries them (the first that meets its conditions is recorded in the file as `thresholds`).  With
# 64 branches over ten steps, several hundred values are tested against each threshold and a round number rarely keeps the
# generator's distance from all of them: the later candidates are midpoints of the widest gap between the tested values near
# the wanted termination / cost rate, found by make_golden_task_rules.search_thresholds from the first candidate (`search`: per
# threshold the clause it belongs to and the quantile of the tested values to aim at, None: where the threshold stands).
CASES = {
    "g15_trace_rules_hopper": dict(
        cfg=dict(seed=21, task="HopperSafe-v2", B=64, T=12, hidden=128, dkl_lim=float("inf"), budget=None, mode="uncertainty"),
        fns=hopper_fns, rules=hopper_rules, guard_clauses=(0,),
        candidates=[(-0.2, 0.3, 2.0), (-0.0548, 0.3694, 0.6416)], search=[(1, 0.04), (2, 0.95), (3, 0.5)]),
    "g15_trace_rules_fatal": dict(
        cfg=dict(seed=22, task="HumanoidSafe-v2", B=64, T=10, hidden=128, dkl_lim=float("inf"), budget=200, mode="uncertainty"),
        fns=fatal_fns, rules=fatal_rules, guard_clauses=(),
        candidates=[(-0.0651, 0.2783), (-0.0651, 0.276)], search=[(0, None), (1, None)]),
    "g15_trace_rules_nodone": dict(
        cfg=dict(seed=23, task="HalfCheetahSafe-v2", B=64, T=9, hidden=128, dkl_lim=float("inf"), budget=None, mode="schedule"),
        fns=nodone_fns, rules=nodone_rules, guard_clauses=(),
        candidates=[(1.5, -0.05), (1.1745, 0.1722)], search=[(0, 0.6), (1, 0.3)]),
}


def build_rules(spec):
    """The TaskRules of a `*_rules(...)` description."""
    from cmbpo_amd import statics
    make = {"healthy": statics.healthy, "fatal": statics.fatal, "cost": statics.cost}
    return statics.TaskRules([make[role](**kw) for role, kw in spec["clauses"]], require_finite=spec["require_finite"],
                             cost_on_term=spec["cost_on_term"])
