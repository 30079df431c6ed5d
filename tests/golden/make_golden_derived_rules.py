"""Generate golden G18: imagined-rollout traces under rules with derived quantities (circular hazards, a planar speed limit,
a tilt limit, an effort cost), recorded the way G15 is (make_golden_task_rules.py): the REFERENCE's own FakeEnv + ModelSampler
+ ModelBuffer with hand-written natural NumPy functions (worlds_derived.py) inserted into its TERMS_BY_TASK / COST_BY_TASK at
run time.

Usage (build container only, like make_golden.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_derived_rules.py [--search]

Writes tests/golden/g18_trace_derived_*.npz (data only) with the keys of the G5 traces plus `thresholds`.  The candidate
thresholds of a case are tried in the order worlds_derived.CASES lists them; the first that meets every condition below is
recorded.  If none does, search_thresholds() looks for a tuple that does and the run stops, naming it.  Conditions (asserted,
not measured):
  * the file is at most 520 KB;
  * every derived quantity decides a clause at least once (a hazard is entered, the speed limit exceeded, ...) and every
    HEALTHY / FATAL clause except a magnitude guard ends at least one branch;
  * where the rules terminate: terminations fall on at least 3 distinct steps, at least 25 % of the branches take part in the
    last step;
  * mean(get_cost) lies in [0.2, 0.8];
  * every value a clause tested during the trace -- derived ones in the clause's scaled units -- lies at least
    1e-3 * max(1, |threshold|) from that threshold: neither the float32-class differences between the GPU forward's matrix
    paths nor the difference between the natural NumPy form and the language's float32 operation order can flip a mask.
"""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (the stubs behind which the reference imports; puts the reference on sys.path)
import worlds_derived  # noqa: E402

MAX_BYTES = 520 * 1024
MARGIN = 1e-3


def _values(rules, cl, call):
    with np.errstate(all="ignore"):
        return cl.values(*call, rules.derived_values(*call))


def _holds(rules, cl, call):
    with np.errstate(all="ignore"):
        return cl.holds(*call, rules.derived_values(*call))


def run_case(case, thr):
    """One trace with the hand-written functions of `thr` in the reference's tables; (data, reason it is rejected or None)."""
    import models.fake_env as ref_fake_env
    import models.statics as ref_statics
    assert ref_fake_env.TERMS_BY_TASK is ref_statics.TERMS_BY_TASK and ref_fake_env.COST_BY_TASK is ref_statics.COST_BY_TASK
    task = case["cfg"]["task"]
    term_fn, cost_fn = case["fns"](*thr)
    calls = []
    run_case.last_calls = calls       # (what search_thresholds looks at)

    def recording(fn):
        def wrapped(obs, act, next_obs):
            calls.append((np.array(obs), np.array(act), np.array(next_obs)))
            return fn(obs, act, next_obs)
        return wrapped

    tables = (ref_statics.TERMS_BY_TASK, ref_statics.COST_BY_TASK)
    saved = [dict(t) for t in tables]
    try:
        for t in tables:
            t.pop(task, None)
        if term_fn is not None:
            ref_statics.TERMS_BY_TASK[task] = recording(term_fn)
            ref_statics.COST_BY_TASK[task] = cost_fn
        else:
            ref_statics.COST_BY_TASK[task] = recording(cost_fn)
        data = mg.run_sampler_trace(**case["cfg"])
    finally:
        for t, s in zip(tables, saved):
            t.clear()
            t.update(s)
    data["thresholds"] = np.asarray(thr, dtype=np.float64)
    rules = worlds_derived.build_rules(case["rules"](*thr))
    B = case["cfg"]["B"]
    assert len(calls) == len(data["n_rows"]) and all(c[0].shape[0] == n for c, n in zip(calls, data["n_rows"]))
    # the language's float32 form and the natural NumPy form agree on every recorded call (what the margin is for)
    term_ref, cost_ref = rules.numpy_fns()
    for c in calls:
        if term_fn is not None and not np.array_equal(term_ref(*c), term_fn(*c)):
            return data, "the rules and the hand-written term function disagree"
        if not np.array_equal(cost_ref(*c), cost_fn(*c)):
            return data, "the rules and the hand-written cost function disagree"
    # the distance of every tested value to its thresholds
    for ci, cl in enumerate(rules.clauses):
        for bound in (float(cl.lo), float(cl.hi)):
            if not np.isfinite(bound):
                continue
            dist = min(float(np.abs(_values(rules, cl, c).astype(np.float64) - bound).min()) for c in calls)
            if not dist >= MARGIN * max(1.0, abs(bound)):
                return data, "clause %d: a value %.3g from its threshold %g" % (ci, dist, bound)
    # every derived quantity decides: the one-quantity clause over it holds on some rows and not on others
    for ci, cl in enumerate(rules.clauses):
        if cl.src != "derived":
            continue
        n = len(rules.derived)
        col0 = cl.col0 + n if cl.col0 < 0 else cl.col0
        cnt = n - col0 if cl.n_cols == -1 else cl.n_cols
        for j in range(col0, col0 + cnt):
            v = np.concatenate([_values(rules, cl, c)[..., j - col0] for c in calls])
            ok = (v > cl.lo if cl.lo_strict else v >= cl.lo) & (v < cl.hi if cl.hi_strict else v <= cl.hi)
            if not (ok.any() and not ok.all()):
                return data, "derived quantity %d never decides clause %d" % (j, ci)
    terminating = [ci for ci, cl in enumerate(rules.clauses) if cl.role in ("healthy", "fatal")]
    if terminating:
        for ci in terminating:
            if ci in case["guard_clauses"]:
                continue
            cl = rules.clauses[ci]
            ended = sum(int(((~_holds(rules, cl, c)) if cl.role == "healthy" else _holds(rules, cl, c)).sum()) for c in calls)
            if ended < 1:
                return data, "clause %d ends no branch" % ci
        steps = sum(1 for c in calls if rules.done(*c).any())
        if steps < 3:
            return data, "terminations on %d steps" % steps
        if data["n_rows"][-1] < 0.25 * B:
            return data, "only %d of %d branches take part in the last step" % (data["n_rows"][-1], B)
    rate = float(np.mean(data["get_cost"]))
    if not 0.2 <= rate <= 0.8:
        return data, "cost rate %.3f" % rate
    return data, None


def search_thresholds(case, start, rounds=12):
    """Thresholds near `start` that meet run_case's conditions, for a new entry of worlds_derived.CASES[...]['candidates'].  Per
    round: run the trace, and move every threshold to the midpoint of the widest gap between the values its clause tested,
    among the values within 4 % of the sample (or the case's own window) around the wanted quantile (case['search']: per
    threshold the clause, the quantile of the tested values to aim at, None for where the threshold stands, and optionally the
    window); a changed threshold changes the trace, hence the rounds."""
    thr = list(start)
    for _ in range(rounds):
        data, why = run_case(case, tuple(thr))
        print("  search", tuple(thr), "->", why or "meets every condition", "rows/step", data["n_rows"].tolist())
        if why is None:
            return tuple(thr)
        rules = worlds_derived.build_rules(case["rules"](*thr))
        for ti, spec in enumerate(case["search"]):
            ci, q = spec[:2]
            window = spec[2] if len(spec) > 2 else 0.04
            cl = rules.clauses[ci]
            # (every value the clause tests counts for the margin, also those of an ANY clause that do not decide their row)
            v = np.concatenate([_values(rules, cl, c) for c in run_case.last_calls], 0)
            v = np.sort(v.reshape(-1).astype(np.float64))
            if q is None:
                q = float(np.searchsorted(v, thr[ti])) / len(v)
            k, half = int(q * len(v)), max(3, int(window * len(v)))
            lo, hi = max(0, k - half), min(len(v) - 1, k + half)
            j = lo + int(np.argmax(v[lo + 1:hi + 1] - v[lo:hi]))
            thr[ti] = round(float(0.5 * (v[j] + v[j + 1])), 4)
    return None


def gen_derived_rules_traces(out):
    for name, case in worlds_derived.CASES.items():
        for thr in case["candidates"]:
            data, why = run_case(case, thr)
            if why is None:
                break
            print(name, thr, "rejected:", why)
        else:
            found = search_thresholds(case, case["candidates"][0])
            raise AssertionError("%s: no listed candidate meets the conditions; search_thresholds gives %r -- append it to "
                                 "worlds_derived.CASES[%r]['candidates'] and run again" % (name, found, name))
        blob = io.BytesIO()
        np.savez_compressed(blob, **data)
        assert blob.getbuffer().nbytes <= MAX_BYTES, (name, blob.getbuffer().nbytes)
        with open(os.path.join(out, name + ".npz"), "wb") as f:
            f.write(blob.getvalue())
        print(name, "thresholds", thr, "steps", len(data["n_rows"]), "rows/step", data["n_rows"].tolist(), "samples",
              int(data["poolm_batch_size"]), "cost rate %.3f" % float(np.mean(data["get_cost"])), "bytes", blob.getbuffer().nbytes)


if __name__ == "__main__":
    mg.install_stubs()
    if "--search" in sys.argv:
        for case_name, case_ in worlds_derived.CASES.items():
            print(case_name, "->", search_thresholds(case_, case_["candidates"][0]))
    else:
        gen_derived_rules_traces(HERE)
