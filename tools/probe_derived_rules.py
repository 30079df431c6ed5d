"""What derived quantities of the task rules cost in the post kernel: cmbpo_fakeenv_post alone, HIP events around
REPS back-to-back launches, AntSafe dims (29 / 8), E = 7, ROWS rows, after warm-up, alternating rounds in one process, the first
two timed rounds dropped (the method of tools/probe_task_rules.py).
  (a) gate, with --other-lib PATH (another build of libcmbpo_hip.so, e.g. the parent commit's): TASK_ANTSAFE, and the §3h
      AntSafe-sized rule set without derived quantities, there against here -- instances this feature must not have touched.
      Outputs bit-identical; the ratio of medians within 1 +- 2 x (max - min) / median of the other library's own repeats.
  (b) reported, here: the rule AntSafe meant with `tilt` as a derived quantity, against the same set without the tilt clause and
      against TASK_ANTSAFE; the same tilt read from `obs` (operands from global memory instead of the LDS image: what the early
      loads hide or do not); a two-hazard cost against a one-interval cost; 8 quantities of 4 terms.
The exit status is non-zero if (a) is outside; the record is written either way.
    python tools/probe_derived_rules.py [out.json] [--other-lib PATH] [--rows N] [--pairs K] [--reps R]"""
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
from cmbpo_amd.statics import TaskRules, cost, derived, dist_sq, healthy, term, tilt

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--other-lib")
ap.add_argument("--rows", type=int, default=100000)
ap.add_argument("--pairs", type=int, default=8)
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()

TASK, E, WARM, DROP = "AntSafe-v2", 7, 300, 2
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
# the §3h rule set: AntSafe-sized, no derived quantities
base = [healthy(cols=0, lo=0.2, hi=1.0), healthy(cols=slice(1, None), abs=True, hi=100.0, hi_strict=True),
        cost(cols=-1, abs=True, lo=3.2, lo_strict=True)]
rules_3h = TaskRules(base, require_finite=True, cost_on_term=True)
meant = TaskRules(base + [healthy(src="derived", cols=0, lo=-0.7)], derived=[tilt(2, 3)], require_finite=True, cost_on_term=True)
meant_obs = TaskRules(base + [healthy(src="derived", cols=0, lo=-0.7)], derived=[tilt(2, 3, src="obs")], require_finite=True,
                      cost_on_term=True)
one_interval = TaskRules([cost(cols=0, lo=0.3, hi=0.6)])
two_hazards = TaskRules([cost(src="derived", cols=slice(0, 2), any=True, hi=0.04)],
                        derived=[dist_sq((0, 1), (0.5, 0.1)), dist_sq((0, 1), (0.7, -0.2))])
eight = TaskRules([cost(src="derived", cols=slice(0, None), any=True, lo=2.0)],
                  derived=[derived([term(j, src=("next_obs", "obs", "act")[(j + k) % 3], w=0.5 + 0.1 * k, c=0.1 * j, pow=1 + k % 2)
                                    for k in range(4)], bias=0.1 * j) for j in range(8)])


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


def rounds(names):
    us = {n: [] for n in names}
    for rnd in range(DROP + args.pairs):
        for n in names:
            t_us = measure(*configs[n])
            if rnd >= DROP:
                us[n].append(t_us)
    return us


def med(us, a, b):
    return statistics.median(us[a]) / statistics.median(us[b])


configs = {"here_antsafe": (here, _lib.TASK_ANTSAFE), "here_rules_3h": (here, rules_3h.task_id), "here_meant_tilt": (here, meant.task_id),
           "here_meant_tilt_from_obs": (here, meant_obs.task_id), "here_one_interval": (here, one_interval.task_id),
           "here_two_hazards": (here, two_hazards.task_id), "here_eight_by_four": (here, eight.task_id)}
if args.other_lib:
    other = C.CDLL(os.path.abspath(args.other_lib))
    other.cmbpo_fakeenv_post.restype, other.cmbpo_fakeenv_post.argtypes = _lib.SIGNATURES["cmbpo_fakeenv_post"]
    other.cmbpo_task_rules_register.restype, other.cmbpo_task_rules_register.argtypes = _lib.SIGNATURES["cmbpo_task_rules_register"]
    other.cmbpo_last_error.restype = C.c_char_p
    s, tid = rules_3h.struct(), C.c_int(-1)
    if other.cmbpo_task_rules_register(C.byref(s), C.byref(tid)) != 0:
        raise RuntimeError(other.cmbpo_last_error())
    configs["other_antsafe"] = (other, _lib.TASK_ANTSAFE)
    configs["other_rules_3h"] = (other, tid.value)
results = {}
for name, (lib, task) in configs.items():
    launch(lib, task)
    torch.cuda.synchronize()
    results[name] = {k: v.clone() for k, v in out.items()}
    for _ in range(WARM):
        launch(lib, task)
torch.cuda.synchronize()
res = dict(command="python tools/probe_derived_rules.py " + " ".join(sys.argv[1:]), task=TASK, rows=N, ensemble=E, reps=args.reps,
           pairs=args.pairs, warmups=WARM, dropped_rounds=DROP, device=torch.cuda.get_device_name(0))
bits = lambda a: a.view(torch.int32) if a.dtype == torch.float32 else a
for name in configs:      # the rules change term and cost only
    for k in ("next_obs", "rew", "dkl_path", "ep_var_mean"):
        assert torch.equal(bits(results[name][k]), bits(results["here_antsafe"][k])), (name, k)
res["term_rate"] = {n: float(results[n]["term"].float().mean()) for n in configs}
res["cost_rate"] = {n: float(results[n]["cost"].mean()) for n in configs}
ok = True
if args.other_lib:
    res["a"] = {}
    for what in ("antsafe", "rules_3h"):
        for k in out:
            assert torch.equal(bits(results["other_" + what][k]), bits(results["here_" + what][k])), (what, k)
        us = rounds(["other_" + what, "here_" + what])
        sp, ratio = spread(us["other_" + what]), med(us, "here_" + what, "other_" + what)
        inside = bool(abs(ratio - 1.0) <= 2.0 * sp)
        ok = ok and inside
        res["a"][what] = dict(us_per_launch=us, other_spread=sp, here_spread=spread(us["here_" + what]), median_ratio_here_over_other=ratio,
                              gate=2.0 * sp, within_gate=inside, outputs_bit_identical=True)
        print("(a) %s here / other: %.4f (gate: 1 +- %.4f) -> %s" % (what, ratio, 2.0 * sp, "within" if inside else "OUTSIDE"))
names = ["here_antsafe", "here_rules_3h", "here_meant_tilt", "here_meant_tilt_from_obs", "here_one_interval", "here_two_hazards",
         "here_eight_by_four"]
us = rounds(names)
res["b"] = dict(us_per_launch=us, spread={n: spread(us[n]) for n in names},
                median_ratio=dict(rules_3h_over_antsafe=med(us, "here_rules_3h", "here_antsafe"),
                                  meant_tilt_over_rules_3h=med(us, "here_meant_tilt", "here_rules_3h"),
                                  meant_tilt_over_antsafe=med(us, "here_meant_tilt", "here_antsafe"),
                                  meant_tilt_from_obs_over_meant_tilt=med(us, "here_meant_tilt_from_obs", "here_meant_tilt"),
                                  two_hazards_over_one_interval=med(us, "here_two_hazards", "here_one_interval"),
                                  eight_by_four_over_one_interval=med(us, "here_eight_by_four", "here_one_interval")))
for k, v in res["b"]["median_ratio"].items():
    print("(b) %s: %.4f" % (k, v))
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
if not ok:
    sys.exit("outside the gate of (a)")
