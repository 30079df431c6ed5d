"""Rules with derived quantities of the G18 traces, twice: as the NumPy functions a user of the reference would add to
``models/statics.py`` (TERMS_BY_TASK / COST_BY_TASK) -- written the natural way, ``((p - c) ** 2).sum(-1) < r2``, which is
deliberately NOT the float32 operation order of ``cmbpo_amd.statics`` (the generator's margin is what makes the masks well
defined, and the check independent of the language) -- and as the builder arguments of the equivalent ``TaskRules``, as plain
data.  Shared by make_golden_derived_rules.py (which records the traces with the functions inserted into the reference's
tables) and the tests (which replay them with the TaskRules).

Pure functions of their thresholds: nothing here touches the reference tree.  The worlds are worlds.build_world's.
"""
import numpy as np

# ---- hazards and speed, no termination: a union of two circles on next_obs columns 2, 4 and a planar speed limit on 14, 17 ------
HAZARDS = ((0.45, -1.0), (1.0, -0.45))


def hazards_fns(r2, v2):
    def cost_fn(obs, act, next_obs):
        assert len(obs.shape) == len(next_obs.shape) == len(act.shape)
        p = next_obs[..., [2, 4]]
        inside = np.zeros(p.shape[:-1], dtype=bool)
        for c in HAZARDS:
            inside |= ((p - np.asarray(c)) ** 2).sum(-1) < r2
        fast = (next_obs[..., [14, 17]] ** 2).sum(-1) > v2
        return np.array(inside | fast, dtype=np.float32)[..., None]

    return None, cost_fn


def hazards_rules(r2, v2):
    return dict(derived=[("dist_sq", dict(cols=(2, 4), center=HAZARDS[0])), ("dist_sq", dict(cols=(2, 4), center=HAZARDS[1])),
                         ("speed_sq", dict(cols=(14, 17)))],
                clauses=[("cost", dict(src="derived", cols=slice(0, 2), any=True, hi=r2, hi_strict=True)),
                         ("cost", dict(src="derived", cols=2, lo=v2, lo_strict=True))],
                require_finite=False, cost_on_term=False)


# ---- tilt and height, with termination: the rule AntSafe's static function meant, plus an effort cost on the action ----------
def tilt_fns(zlo, zhi, c0, e0):
    def term_fn(obs, act, next_obs):
        assert len(obs.shape) == len(next_obs.shape) == len(act.shape)
        z = next_obs[..., 0]
        q1, q2 = next_obs[..., 2], next_obs[..., 3]
        z_rot = 1 - 2 * (q1 ** 2 + q2 ** 2)
        notdone = np.isfinite(next_obs).all(axis=-1) * (z >= zlo) * (z <= zhi) * (z_rot >= c0)
        return (~notdone)[..., None]

    def cost_fn(obs, act, next_obs):
        done = term_fn(obs, act, next_obs)[..., 0] * 1.0
        effort = (act ** 2).sum(-1) + (obs[..., 1] - 0.1) ** 2
        return np.clip(done + (effort > e0), 0, 1).astype(np.float32)[..., None]

    return term_fn, cost_fn


def tilt_rules(zlo, zhi, c0, e0):
    return dict(derived=[("tilt", dict(q1_col=2, q2_col=3)),
                         ("derived", dict(terms=[dict(col=0, src="act", pow=2), dict(col=1, src="act", pow=2), dict(col=2, src="act", pow=2),
                                                 dict(col=1, src="obs", c=0.1, pow=2)]))],
                clauses=[("healthy", dict(cols=0, lo=zlo, hi=zhi)),
                         ("healthy", dict(src="derived", cols=0, lo=c0)),
                         ("cost", dict(src="derived", cols=1, lo=e0, lo_strict=True))],
                require_finite=True, cost_on_term=True)


# name -> the trace's configuration (make_golden.run_sampler_trace), the two forms of its rules, and the candidate thresholds in
# the order the generator tries them (the first that meets its conditions is recorded in the file as `thresholds`); `search`: per
# threshold the clause it belongs to, the quantile of the tested values to aim at (None: where the threshold stands) and
# optionally the window around it, as a fraction of the sample -- see make_golden_derived_rules.search_thresholds.
CASES = {
    "g18_trace_derived_hazards": dict(
        cfg=dict(seed=31, task="HalfCheetahSafe-v2", B=64, T=9, hidden=128, dkl_lim=float("inf"), budget=None, mode="schedule"),
        fns=hazards_fns, rules=hazards_rules, guard_clauses=(),
        candidates=[(0.1, 1.8), (0.1288, 2.4109)], search=[(0, 0.15, 0.1), (1, 0.75)]),
    "g18_trace_derived_tilt": dict(
        cfg=dict(seed=32, task="HopperSafe-v2", B=64, T=12, hidden=128, dkl_lim=float("inf"), budget=None, mode="uncertainty"),
        fns=tilt_fns, rules=tilt_rules, guard_clauses=(),
        candidates=[(0.0, 1.05, -10.0, 1.5), (-0.0911, 0.996, -10.5911, 2.1494)], search=[(0, 0.02), (0, 0.98), (1, 0.05), (2, 0.6)]),
}


def build_rules(spec):
    """The TaskRules of a `*_rules(...)` description."""
    from cmbpo_amd import statics
    make = {"healthy": statics.healthy, "fatal": statics.fatal, "cost": statics.cost}
    quantity = {"dist_sq": statics.dist_sq, "speed_sq": statics.speed_sq, "tilt": statics.tilt,
                "derived": lambda terms, bias=0.0: statics.derived([statics.term(**t) for t in terms], bias=bias)}
    return statics.TaskRules([make[role](**kw) for role, kw in spec["clauses"]],
                             derived=[quantity[kind](**kw) for kind, kw in spec["derived"]],
                             require_finite=spec["require_finite"], cost_on_term=spec["cost_on_term"])
