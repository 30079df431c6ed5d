"""What stochastic transitions cost: the post kernel alone -- HIP events around REPS back-to-back launches, AntSafe
dims (29 / 8), E = 7, ROWS rows, after warm-up, alternating pairs, the first two rounds dropped -- and a rollout phase.
  (a) with --other-lib PATH (another build of libcmbpo_hip.so, e.g. the parent commit's): cmbpo_fakeenv_post there against
      cmbpo_fakeenv_post here, TASK_ANTSAFE, outputs bit-identical -- the deterministic launch must not pay for the feature.
      Gate: median ratio here / other <= 1 + 2 x the spread the other library shows against itself over its own repeats,
      (max - min) / median.  Outside the gate the exit status is non-zero; the record is written either way.
  (b) cmbpo_fakeenv_post_noise (the NOISE instance: 4 obs_dim more bytes read per row, E square roots per thread) against
      cmbpo_fakeenv_post here: reported, no gate.
  (c) a ROWS-branch rollout phase (bench.rollout_phase: reset, sample_many to the end, finish, get) with and without
      `stochastic`, the draws of xi included: reported.
    python tools/probe_transition_noise.py [out.json] [--other-lib PATH] [--rows N] [--pairs K] [--reps R] [--phases P]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
import cmbpo_amd  # noqa: F401
from cmbpo_amd import _lib, synthetic

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--other-lib")
ap.add_argument("--rows", type=int, default=100000)
ap.add_argument("--pairs", type=int, default=8)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--phases", type=int, default=3)
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
xi = t(rng.standard_normal((N, D)).astype(np.float32))
f = dict(dtype=torch.float32, device=dev)
out = dict(next_obs=torch.empty((N, D), **f), rew=torch.empty(N, **f), term=torch.empty(N, dtype=torch.uint8, device=dev),
           cost=torch.empty(N, **f), dkl_path=torch.empty(N, **f), ep_var_mean=torch.empty(N, **f))

here = _lib.lib()
other = None
if args.other_lib:
    other = C.CDLL(os.path.abspath(args.other_lib))
    other.cmbpo_fakeenv_post.restype, other.cmbpo_fakeenv_post.argtypes = _lib.SIGNATURES["cmbpo_fakeenv_post"]
    other.cmbpo_last_error.restype = C.c_char_p


def launch(lib, noise):
    a = (_lib.TASK_ANTSAFE, E, D, A, _lib.ptr(mean), _lib.ptr(var), N, _lib.ptr(obs), _lib.ptr(act), _lib.ptr(inds), None, None, N,
         _lib.ptr(out["next_obs"]), _lib.ptr(out["rew"]), _lib.ptr(out["term"]), _lib.ptr(out["cost"]), _lib.ptr(out["dkl_path"]),
         _lib.ptr(out["ep_var_mean"]), None)
    rc = lib.cmbpo_fakeenv_post_noise(*a, _lib.ptr(xi), _lib.current_stream()) if noise else \
        lib.cmbpo_fakeenv_post(*a, _lib.current_stream())
    if rc != 0:
        raise RuntimeError(lib.cmbpo_last_error())


def measure(lib, noise):
    """Microseconds per launch over args.reps back-to-back launches."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        launch(lib, noise)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.reps


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def rounds(names):
    us = {k: [] for k in names}
    for rnd in range(DROP + args.pairs):
        for name in us:
            t_us = measure(*configs[name])
            if rnd >= DROP:
                us[name].append(t_us)
    return us


configs = {"here_post": (here, False), "here_noise": (here, True)}
if other is not None:
    configs["other_post"] = (other, False)
results = {}
for name, cfg in configs.items():
    launch(*cfg)
    torch.cuda.synchronize()
    results[name] = {k: v.clone() for k, v in out.items()}
    for _ in range(WARM):
        launch(*cfg)
torch.cuda.synchronize()
res = dict(tool="tools/probe_transition_noise.py", against_other_lib=other is not None, phases=args.phases, task=TASK, rows=N, ensemble=E,
           reps=args.reps, pairs=args.pairs, warmups=WARM, dropped_rounds=DROP, device=torch.cuda.get_device_name(0))
same = lambda a, b: torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
assert same(results["here_noise"]["rew"], results["here_post"]["rew"])
assert not same(results["here_noise"]["next_obs"], results["here_post"]["next_obs"])
if other is not None:
    for k in out:
        assert same(results["other_post"][k], results["here_post"][k]), k
    res["post_outputs_bit_identical_to_other_lib"] = True
    us = rounds(["other_post", "here_post"])
    sp = spread(us["other_post"])
    ratio = statistics.median(us["here_post"]) / statistics.median(us["other_post"])
    res["a"] = dict(us_per_launch=us, other_spread=sp, here_spread=spread(us["here_post"]), median_ratio_here_over_other=ratio,
                    gate=2.0 * sp, within_gate=bool(ratio <= 1.0 + 2.0 * sp))
    print("(a) cmbpo_fakeenv_post here / other: %.4f (gate: 1 + %.4f) -> %s" % (ratio, 2.0 * sp, "within" if res["a"]["within_gate"] else "OUTSIDE"))
us = rounds(["here_post", "here_noise"])
ratio = statistics.median(us["here_noise"]) / statistics.median(us["here_post"])
res["b"] = dict(us_per_launch=us, post_spread=spread(us["here_post"]), noise_spread=spread(us["here_noise"]),
                median_ratio_noise_over_post=ratio)
print("(b) NOISE instance / deterministic: %.4f (%.1f us against %.1f us)" % (ratio, statistics.median(us["here_noise"]),
                                                                            statistics.median(us["here_post"])))
del mean, var, out, results

# (c) the rollout phase of the benchmark's world, xi draws included
w = bench.build_world(0, TASK)
sampler, pool, env, policy = bench.build_hip(w, TASK, N, dev, None, bench.MAXROLL, "schedule")
start = synthetic.start_states(np.random.default_rng(1), N, TASK)
phase = {}
for rnd in range(1 + args.phases):           # (the first round of both is warm-up)
    for name, flag in (("deterministic", False), ("stochastic", True)):
        sampler.stochastic = flag
        sampler._draws = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_samples, _ = bench.rollout_phase(sampler, pool, start)
        torch.cuda.synchronize()
        if rnd >= 1:
            phase.setdefault(name, []).append(dict(seconds=time.perf_counter() - t0, samples=n_samples, steps=sampler._n_episodes))
med = {k: statistics.median(p["seconds"] for p in v) for k, v in phase.items()}
res["c"] = dict(phases=phase, median_seconds=med, median_ratio_stochastic_over_deterministic=med["stochastic"] / med["deterministic"])
print("(c) rollout phase stochastic / deterministic: %.4f (%.3f s against %.3f s)" % (res["c"]["median_ratio_stochastic_over_deterministic"],
                                                                                   med["stochastic"], med["deterministic"]))
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
if not res.get("a", {}).get("within_gate", True):
    sys.exit("outside: a")
