"""Generate golden G15: imagined-rollout traces under user-defined termination / cost rules, recorded from the REFERENCE's
own FakeEnv + ModelSampler + ModelBuffer with hand-written NumPy functions (worlds_rules.py) inserted into its
TERMS_BY_TASK / COST_BY_TASK at run time -- what a user of the reference does by editing models/statics.py:56-69.

Usage (build container only, like make_golden.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_task_rules.py

Writes tests/golden/g15_trace_rules_*.npz (data only) with the keys of the G5 traces (make_golden.run_sampler_trace) plus
`thresholds`.  The candidate thresholds of a case are tried in the order worlds_rules.CASES lists them; the first that meets
every condition below is recorded.  If none does, search_thresholds() looks for a tuple that does and the run stops, naming it:
the list is data the tests read, so a maintainer adds the tuple there (`--search` runs the search for every case).  Conditions (asserted, not measured):
  * the file is at most 520 KB;
  * where the rules terminate: every HEALTHY / FATAL clause except the magnitude guard ends at least one branch, terminations
    fall on at least 3 distinct steps, at least 25 % of the branches take part in the last step;
  * mean(get_cost) lies in [0.2, 0.8] where a cost rule exists;
  * every value a clause tested during the trace lies at least 1e-3 * max(1, |threshold|) from that threshold, in the
    clause's scaled units: the float32-class differences between the GPU forward's matrix paths cannot flip a mask.
"""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (the stubs behind which the reference imports; puts the reference on sys.path)
import worlds_rules  # noqa: E402

MAX_BYTES = 520 * 1024
MARGIN = 1e-3


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
            if cost_fn is not None:
                ref_statics.COST_BY_TASK[task] = cost_fn
        else:
            ref_statics.COST_BY_TASK[task] = recording(cost_fn)
        data = mg.run_sampler_trace(**case["cfg"])
    finally:
        for t, s in zip(tables, saved):
            t.clear()
            t.update(s)
    data["thresholds"] = np.asarray(thr, dtype=np.float64)
    rules = worlds_rules.build_rules(case["rules"](*thr))
    B = case["cfg"]["B"]
    assert len(calls) == len(data["n_rows"]) and all(c[0].shape[0] == n for c, n in zip(calls, data["n_rows"]))
    # the distance of every tested value to its thresholds
    for ci, cl in enumerate(rules.clauses):
        for bound in (float(cl.lo), float(cl.hi)):
            if not np.isfinite(bound):
                continue
            dist = min(float(np.abs(cl.values(*c).astype(np.float64) - bound).min()) for c in calls)
            if not dist >= MARGIN * max(1.0, abs(bound)):
                return data, "clause %d: a value %.3g from its threshold %g" % (ci, dist, bound)
    terminating = [ci for ci, cl in enumerate(rules.clauses) if cl.role in ("healthy", "fatal")]
    if terminating:
        for ci in terminating:
            if ci in case["guard_clauses"]:
                continue
            cl = rules.clauses[ci]
            ended = sum(int(((~cl.holds(*c)) if cl.role == "healthy" else cl.holds(*c)).sum()) for c in calls)
            if ended < 1:
                return data, "clause %d ends no branch" % ci
        steps = sum(1 for c in calls if rules.done(*c).any())
        if steps < 3:
            return data, "terminations on %d steps" % steps
        if data["n_rows"][-1] < 0.25 * B:
            return data, "only %d of %d branches take part in the last step" % (data["n_rows"][-1], B)
    term_ref, cost_ref = rules.numpy_fns()
    if cost_ref is not None:
        rate = float(np.mean(data["get_cost"]))
        if not 0.2 <= rate <= 0.8:
            return data, "cost rate %.3f" % rate
    return data, None


def search_thresholds(case, start, rounds=12):
    """Thresholds near `start` that meet run_case's conditions, for a new entry of worlds_rules.CASES[...]['candidates'] (when
    the reference, a seed or a world changes and no listed candidate passes any more).  Per round: run the trace, and move
    every threshold to the midpoint of the widest gap between the values its clause tested, among the values within 4 % of
    the sample around the wanted quantile (case['search']: per threshold the clause, and the quantile of the tested values
    to aim at, None for where the threshold stands); a changed threshold changes the trace, hence the rounds."""
    thr = list(start)
    for _ in range(rounds):
        data, why = run_case(case, tuple(thr))
        print("  search", tuple(thr), "->", why or "meets every condition", "rows/step", data["n_rows"].tolist())
        if why is None:
            return tuple(thr)
        rules = worlds_rules.build_rules(case["rules"](*thr))
        for ti, (ci, q) in enumerate(case["search"]):
            cl = rules.clauses[ci]
            v = np.concatenate([cl.values(*c) for c in run_case.last_calls], 0)
            if cl.any:
                v = v.max(-1)     # ANY over a slice of magnitudes: the row maximum decides
            v = np.sort(v.reshape(-1).astype(np.float64))
            if q is None:
                q = float(np.searchsorted(v, thr[ti])) / len(v)
            k, half = int(q * len(v)), max(3, len(v) // 25)
            lo, hi = max(0, k - half), min(len(v) - 1, k + half)
            j = lo + int(np.argmax(v[lo + 1:hi + 1] - v[lo:hi]))
            thr[ti] = round(float(0.5 * (v[j] + v[j + 1])), 4)
    return None


def gen_task_rules_traces(out):
    for name, case in worlds_rules.CASES.items():
        for thr in case["candidates"]:
            data, why = run_case(case, thr)
            if why is None:
                break
            print(name, thr, "rejected:", why)
        else:
            found = search_thresholds(case, case["candidates"][0])
            raise AssertionError("%s: no listed candidate meets the conditions; search_thresholds gives %r -- append it to "
                                 "worlds_rules.CASES[%r]['candidates'] and run again" % (name, found, name))
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
        for case_name, case_ in worlds_rules.CASES.items():
            print(case_name, "->", search_thresholds(case_, case_["candidates"][0]))
    else:
        gen_task_rules_traces(HERE)
