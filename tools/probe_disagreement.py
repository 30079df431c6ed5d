"""What the ensemble disagreement on reward / cost costs in the post kernel: cmbpo_fakeenv_post alone, HIP events
around REPS back-to-back launches, AntSafe dims (29 / 8), E = 7, ROWS rows, after warm-up; alternating pairs in one process, the
first two timed rounds of a part dropped.
  (a) with --other-lib PATH (another build of libcmbpo_hip.so, e.g. the parent commit's): TASK_ANTSAFE there against
      TASK_ANTSAFE here -- a launch without the feature must not pay for it.  The yardstick is the spread the other library
      shows against itself over its own repeats, (max - min) / median; the median ratio has to lie within 1 + twice that.
  (b) here, with a learned cost head (obs + 2 columns): cmbpo_fakeenv_post against cmbpo_fakeenv_post_disagreement with
      kappa = (0, 0) and with kappa = (0.75, 1.5).  Reported, not gated: 2 E more loads per row in the tail.
The exit status is non-zero if (a) is outside; the record is written either way.
    python tools/probe_disagreement.py [out.json] [--other-lib PATH] [--rows N] [--pairs K] [--reps R]"""
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
mean2 = (rng.standard_normal((E, N, D + 2)) * 0.3).astype(np.float32)
var2 = np.exp(rng.uniform(-12, 1, (E, N, D + 2))).astype(np.float32)
# without the cost column: the arrays of part (a); with it: those of part (b)
mean = {False: t(mean2[..., :D + 1]), True: t(mean2)}
var = {False: t(var2[..., :D + 1]), True: t(var2)}
inds = t(rng.integers(0, E, size=N).astype(np.int32))
f = dict(dtype=torch.float32, device=dev)
out = dict(next_obs=torch.empty((N, D), **f), rew=torch.empty(N, **f), term=torch.empty(N, dtype=torch.uint8, device=dev),
           cost=torch.empty(N, **f), dkl_path=torch.empty(N, **f), ep_var_mean=torch.empty(N, **f))
rew_var, cost_var = torch.empty(N, **f), torch.empty(N, **f)

here = _lib.lib()
other = None
if args.other_lib:
    other = C.CDLL(os.path.abspath(args.other_lib))
    other.cmbpo_fakeenv_post.restype, other.cmbpo_fakeenv_post.argtypes = _lib.SIGNATURES["cmbpo_fakeenv_post"]
    other.cmbpo_last_error.restype = C.c_char_p


def launch(lib, learned, kappa):
    """kappa None: cmbpo_fakeenv_post; else cmbpo_fakeenv_post_disagreement with those coefficients."""
    task = _lib.TASK_ANTSAFE | (_lib.TASK_LEARNED_COST if learned else 0)
    a = (task, E, D, A, _lib.ptr(mean[learned]), _lib.ptr(var[learned]), N, _lib.ptr(obs), _lib.ptr(act), _lib.ptr(inds),
         None, None, N, _lib.ptr(out["next_obs"]), _lib.ptr(out["rew"]), _lib.ptr(out["term"]), _lib.ptr(out["cost"]),
         _lib.ptr(out["dkl_path"]), _lib.ptr(out["ep_var_mean"]), None)
    if kappa is None:
        rc = lib.cmbpo_fakeenv_post(*a, _lib.current_stream())
    else:
        rc = lib.cmbpo_fakeenv_post_disagreement(*a, None, kappa[0], kappa[1], _lib.ptr(rew_var), _lib.ptr(cost_var),
                                                 _lib.current_stream())
    if rc != 0:
        raise RuntimeError(lib.cmbpo_last_error())


def measure(cfg):
    """Microseconds per launch over args.reps back-to-back launches."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        launch(*cfg)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.reps


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def rounds(names):
    us = {n: [] for n in names}
    for rnd in range(DROP + args.pairs):
        for n in names:
            t_us = measure(configs[n])
            if rnd >= DROP:
                us[n].append(t_us)
    return us


configs = {"here_antsafe": (here, False, None), "here_off": (here, True, None), "here_kappa0": (here, True, (0.0, 0.0)),
           "here_pessimistic": (here, True, (0.75, 1.5))}
if other is not None:
    configs["other_antsafe"] = (other, False, None)
results = {}
for name, cfg in configs.items():       # the same bits from every configuration that should give them
    launch(*cfg)
    torch.cuda.synchronize()
    results[name] = {k: v.clone() for k, v in out.items()}
    for _ in range(WARM):
        launch(*cfg)
torch.cuda.synchronize()
bits = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x
res = dict(command="python tools/probe_disagreement.py " + " ".join(sys.argv[1:]), task=TASK, rows=N, ensemble=E, reps=args.reps,
           pairs=args.pairs, warmups=WARM, dropped_rounds=DROP, device=torch.cuda.get_device_name(0))
for k in out:
    assert torch.equal(bits(results["here_kappa0"][k]), bits(results["here_off"][k])), k
    if k not in ("rew", "cost"):
        assert torch.equal(bits(results["here_pessimistic"][k]), bits(results["here_off"][k])), k
res["kappa0_outputs_bit_identical_to_plain_entry"] = True
res["mean_rew_penalty"] = float((results["here_off"]["rew"] - results["here_pessimistic"]["rew"]).mean())
res["mean_cost_penalty"] = float((results["here_pessimistic"]["cost"] - results["here_off"]["cost"]).mean())
if other is not None:
    for k in out:
        assert torch.equal(bits(results["other_antsafe"][k]), bits(results["here_antsafe"][k])), k
    res["antsafe_outputs_bit_identical_to_other_lib"] = True
    us = rounds(["other_antsafe", "here_antsafe"])
    sp = spread(us["other_antsafe"])
    ratio = statistics.median(us["here_antsafe"]) / statistics.median(us["other_antsafe"])
    res["a"] = dict(us_per_launch=us, median_us={k: statistics.median(v) for k, v in us.items()}, other_spread=sp,
                    here_spread=spread(us["here_antsafe"]), median_ratio_here_over_other=ratio, gate=2.0 * sp,
                    within_gate=bool(ratio - 1.0 <= 2.0 * sp))
    print("(a) TASK_ANTSAFE here / other: %.4f (gate: 1 + %.4f) -> %s" % (ratio, 2.0 * sp, "within" if res["a"]["within_gate"] else "OUTSIDE"))
us = rounds(["here_off", "here_kappa0", "here_pessimistic"])
med = {k: statistics.median(v) for k, v in us.items()}
res["b"] = dict(us_per_launch=us, median_us=med, spread={k: spread(v) for k, v in us.items()},
                median_ratio_kappa0_over_off=med["here_kappa0"] / med["here_off"],
                median_ratio_pessimistic_over_off=med["here_pessimistic"] / med["here_off"])
print("(b) disagreement / plain entry: kappa 0 %.4f, kappa > 0 %.4f (%.2f / %.2f / %.2f us)" % (
    res["b"]["median_ratio_kappa0_over_off"], res["b"]["median_ratio_pessimistic_over_off"], med["here_off"], med["here_kappa0"],
    med["here_pessimistic"]))
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
if "a" in res and not res["a"]["within_gate"]:
    sys.exit("outside: a")
