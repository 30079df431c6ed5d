"""What user-defined termination / cost rules cost in the post kernel: cmbpo_fakeenv_post alone, HIP events around
REPS back-to-back launches, AntSafe dims (29 / 8), E = 7, ROWS rows, after warm-up.
  (a) with --other-lib PATH (another build of libcmbpo_hip.so, e.g. the parent commit's): TASK_ANTSAFE there against
      TASK_ANTSAFE here, alternating pairs in one process -- the built-in tasks must not pay for the feature.  The yardstick is
      the spread the other library shows against itself over its own repeats, (max - min) / median.
  (b) here: an AntSafe-sized rule set (finiteness, a two-sided z range, one slice guard, one cost clause, cost_on_term) against
      TASK_ANTSAFE, alternating (with an empty rule set as a third: what the instance costs without a clause); gated at twice that spread.
The exit status is non-zero if (a) or (b) is outside; the record is written either way.
    python tools/probe_task_rules.py [out.json] [--other-lib PATH] [--rows N] [--pairs K] [--reps R]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import cmbpo_amd  # noqa: F401
from cmbpo_amd import _lib, synthetic
from cmbpo_amd.statics import TaskRules, cost, healthy

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--other-lib")
ap.add_argument("--rows", type=int, default=100000)
ap.add_argument("--pairs", type=int, default=8)
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()

TASK, E, WARM = "AntSafe-v2", 7, 300
# rounds of each part measured and thrown away: the first timed round of a part runs up to a fifth slower than the ones behind it
# whatever the number of untimed warm-up launches, and would be all of the spread the criteria are judged against
DROP = 2
D, A = synthetic.ENV_DIMS[TASK]
N = args.rows
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
obs = t(synthetic.start_states(rng, N, TASK))
act = t(rng.uniform(-1, 1, (N, A)).astype(np.float32))
mean = t((rng.standard_normal((E, N, D + 1)) * 0.3).astype(np.float32))
var = t(np.exp(rng.uniform(-12, 1, (E, N, D + 1))).astype(np.float32))
inds = t(rng.integers(0, E, size=N).astype(np.int32))
f = dict(dtype=torch.float32, device=dev)
out = dict(next_obs=torch.empty((N, D), **f), rew=torch.empty(N, **f), term=torch.empty(N, dtype=torch.uint8, device=dev),
           cost=torch.empty(N, **f), dkl_path=torch.empty(N, **f), ep_var_mean=torch.empty(N, **f))

here = _lib.lib()
libs = {"here": here}
if args.other_lib:
    other = C.CDLL(os.path.abspath(args.other_lib))
    other.cmbpo_fakeenv_post.restype, other.cmbpo_fakeenv_post.argtypes = _lib.SIGNATURES["cmbpo_fakeenv_post"]
    other.cmbpo_last_error.restype = C.c_char_p
    libs["other"] = other

rules = TaskRules([healthy(cols=0, lo=0.2, hi=1.0), healthy(cols=slice(1, None), abs=True, hi=100.0, hi_strict=True),
                   cost(cols=-1, abs=True, lo=3.2, lo_strict=True)], require_finite=True, cost_on_term=True)


def launch(lib, task):
    rc = lib.cmbpo_fakeenv_post(task, E, D, A, _lib.ptr(mean), _lib.ptr(var), N, _lib.ptr(obs), _lib.ptr(act), _lib.ptr(inds),
                                None, None, N, _lib.ptr(out["next_obs"]), _lib.ptr(out["rew"]), _lib.ptr(out["term"]),
                                _lib.ptr(out["cost"]), _lib.ptr(out["dkl_path"]), _lib.ptr(out["ep_var_mean"]), None,
                                _lib.current_stream())
    if rc != 0:
        raise RuntimeError(lib.cmbpo_last_error())


def measure(lib, task):
    """Microseconds per launch over args.reps back-to-back launches."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        launch(lib, task)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.reps


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


# (an empty table: the rules instance and its 528 more bytes of kernel arguments, with no clause to evaluate)
configs = {"here_antsafe": (here, _lib.TASK_ANTSAFE), "here_rules": (here, rules.task_id),
           "here_empty_rules": (here, TaskRules([]).task_id)}
if args.other_lib:
    configs["other_antsafe"] = (libs["other"], _lib.TASK_ANTSAFE)
results = {}
for name, (lib, task) in configs.items():       # the same bits from every configuration that should give them
    launch(lib, task)
    torch.cuda.synchronize()
    results[name] = {k: v.clone() for k, v in out.items()}
    for _ in range(WARM):
        launch(lib, task)
torch.cuda.synchronize()
res = dict(command="python tools/probe_task_rules.py " + " ".join(sys.argv[1:]), task=TASK, rows=N, ensemble=E, reps=args.reps,
           pairs=args.pairs, warmups=WARM, dropped_rounds=DROP, device=torch.cuda.get_device_name(0))
for k in ("next_obs", "rew", "dkl_path", "ep_var_mean"):
    assert torch.equal(results["here_rules"][k].view(torch.int32), results["here_antsafe"][k].view(torch.int32)), k
res["rules_term_rate"] = float(results["here_rules"]["term"].float().mean())
res["antsafe_term_rate"] = float(results["here_antsafe"]["term"].float().mean())
if args.other_lib:
    for k in out:
        a, b = results["other_antsafe"][k], results["here_antsafe"][k]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), k
    res["antsafe_outputs_bit_identical_to_other_lib"] = True
    us = {"other_antsafe": [], "here_antsafe": []}
    for rnd in range(DROP + args.pairs):
        for name in us:
            t_us = measure(*configs[name])
            if rnd >= DROP:
                us[name].append(t_us)
    sp = spread(us["other_antsafe"])
    ratio = statistics.median(us["here_antsafe"]) / statistics.median(us["other_antsafe"])
    res["a"] = dict(us_per_launch=us, other_spread=sp, here_spread=spread(us["here_antsafe"]), median_ratio_here_over_other=ratio,
                    within_other_spread=bool(abs(ratio - 1.0) <= sp))
    print("(a) TASK_ANTSAFE here / other: %.4f (other's own spread %.4f) -> %s" % (ratio, sp, "within" if res["a"]["within_other_spread"] else "OUTSIDE"))
us = {"here_antsafe": [], "here_rules": [], "here_empty_rules": []}
for rnd in range(DROP + args.pairs):
    for name in us:
        t_us = measure(*configs[name])
        if rnd >= DROP:
            us[name].append(t_us)
sp_b = res["a"]["other_spread"] if "a" in res else spread(us["here_antsafe"])
ratio = statistics.median(us["here_rules"]) / statistics.median(us["here_antsafe"])
res["b"] = dict(us_per_launch=us, antsafe_spread=spread(us["here_antsafe"]), rules_spread=spread(us["here_rules"]),
                median_ratio_rules_over_antsafe=ratio,
                median_ratio_empty_rules_over_antsafe=statistics.median(us["here_empty_rules"]) / statistics.median(us["here_antsafe"]),
                gate=2.0 * sp_b, within_gate=bool(ratio - 1.0 <= 2.0 * sp_b))
print("(b) rule set / TASK_ANTSAFE: %.4f (gate: 1 + %.4f) -> %s" % (ratio, 2.0 * sp_b, "within" if res["b"]["within_gate"] else "OUTSIDE"))
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
# the criterion of (a) and the gate of (b) decide the exit status (the record above is written either way)
failed = [k for k, ok in (("a", res.get("a", {}).get("within_other_spread", True)), ("b", res["b"]["within_gate"])) if not ok]
if failed:
    sys.exit("outside: " + ", ".join(failed))
