"""What the logistic learned-cost head costs in the post kernel and what it reaches in the trainer.
  --kernel    the post kernel at ROWS rows (AntSafe's widths, 7 members, learned cost, disagreement on: the instance in which
              every lane of a row turns its member's logit into a probability), HIP events around REPS launches, the
              configurations taken in turn (alternating rounds in alternating order, the first DROP thrown away):
              `magnitude` (cmbpo_fakeenv_post_disagreement here), `logistic` (cmbpo_fakeenv_post_cost, kind 1) and, with
              --other-lib PATH (the parent commit's libcmbpo_hip.so), `parent` (cmbpo_fakeenv_post_disagreement there).  The
              yardstick is the parent's own (max - min) / median.  --plain: the same without the disagreement (one lane per row
              computes one probability).  --configs: a subset of the three.  Run it under `rocprofv3 --kernel-trace --stats --
              python tools/probe_cost_head.py --kernel` for the per-instance kernel times (the instances differ in their last
              template argument).
  --trainer   two epochs of CMBPO(m_learn_cost=True) on the box point mass with an indicator cost
              (tests/test_cost_head_cmbpo_gpu.py), seeds 0 / 1 / 2, for m_cost_loss 'gaussian' and 'logistic' at the same
              training budget: the share of imagined costs outside [0, 1], and the validation replay's Brier score
              (`mse_cost`) and `cost_cm` at h = 1 and summed over the horizons.
    python tools/probe_cost_head.py [out.json] [--kernel] [--plain] [--trainer] [--other-lib PATH]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import cmbpo_amd  # noqa: F401
from cmbpo_amd import _lib, synthetic

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--kernel", action="store_true")
ap.add_argument("--plain", action="store_true")
ap.add_argument("--trainer", action="store_true")
ap.add_argument("--other-lib")
ap.add_argument("--configs", default=None, help="--kernel: a comma-separated subset of magnitude,logistic,parent")
ap.add_argument("--rows", type=int, default=100000)
ap.add_argument("--rounds", type=int, default=12)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--seeds", type=int, default=3)
args = ap.parse_args()

DROP = 2
res = dict(command="python tools/probe_cost_head.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0))


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


if args.kernel:
    here = _lib.lib()
    libs = {"here": here}
    if args.other_lib:
        other = C.CDLL(os.path.abspath(args.other_lib))
        for name, (r, a) in _lib.SIGNATURES.items():
            if hasattr(other, name):
                fn = getattr(other, name)
                fn.restype, fn.argtypes = r, a
        libs["parent"] = other
    D, A = synthetic.ENV_DIMS["AntSafe-v2"]
    E, B, O = 7, args.rows, D + 2
    g = torch.Generator(device="cuda").manual_seed(0)
    f = dict(dtype=torch.float32, device="cuda")
    mean = 0.3 * torch.randn(E, B, O, generator=g, **f)
    mean[:, :, D + 1] = 3.0 * torch.randn(E, B, generator=g, **f)          # logits over a few units
    var = torch.exp(-12 + 13 * torch.rand(E, B, O, generator=g, **f))
    obs, act = 0.1 * torch.randn(B, D, generator=g, **f), torch.rand(B, A, generator=g, **f) * 2 - 1
    obs[:, 0] = 0.6
    inds = torch.randint(0, E, (B,), dtype=torch.int32, device="cuda", generator=g)
    out = {k: torch.empty((B, D) if k in ("next_obs", "ep_var") else (B,), **f)
           for k in ("next_obs", "rew", "cost", "dkl", "epv", "ep_var", "rew_var", "cost_var", "cost_logit")}
    term = torch.empty(B, dtype=torch.uint8, device="cuda")
    p = _lib.ptr
    common = [_lib.TASK_ANTSAFE | _lib.TASK_LEARNED_COST, E, D, A, p(mean), p(var), B, p(obs), p(act), p(inds), None, None, B,
              p(out["next_obs"]), p(out["rew"]), p(term), p(out["cost"]), p(out["dkl"]), p(out["epv"]), p(out["ep_var"]), None]
    dis = [0.5, 0.5, p(out["rew_var"]), p(out["cost_var"])] if not args.plain else [0.0, 0.0, None, None]
    ch = _lib.CostHeadStruct()
    ch.kind, ch.logit_shift, ch.cost_logit = _lib.COST_LOGISTIC, 0.25, p(out["cost_logit"])
    stream = _lib.current_stream()

    def magnitude(lib):
        if args.plain:
            return lambda: lib.cmbpo_fakeenv_post(*common[:-1], stream)
        return lambda: lib.cmbpo_fakeenv_post_disagreement(*common, *dis, stream)

    calls = {"magnitude": magnitude(here), "logistic": lambda: here.cmbpo_fakeenv_post_cost(*common, *dis, None, C.byref(ch), stream)}
    if "parent" in libs:
        calls["parent"] = magnitude(libs["parent"])

    def timed(call):
        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                rc = call()
            e1.record()
            e1.synchronize()
            assert rc == 0, _lib.lib().cmbpo_last_error()
            return e0.elapsed_time(e1) * 1e3 / args.reps
        return run

    if args.configs:
        calls = {k: calls[k] for k in args.configs.split(",")}
    fns = {k: timed(v) for k, v in calls.items()}
    got = {k: [] for k in fns}
    for rnd in range(DROP + args.rounds):
        for k, fn in (list(fns.items())[::-1] if rnd & 1 else fns.items()):
            x = fn()
            if rnd >= DROP:
                got[k].append(x)
    kern = {k: dict(us=[round(x, 3) for x in v], median=round(statistics.median(v), 3), spread=round(spread(v), 4)) for k, v in got.items()}
    base = "parent" if "parent" in got else "magnitude"
    if "logistic" in got and base in got:
        kern["ratio_logistic_over_" + base] = round(statistics.median(got["logistic"]) / statistics.median(got[base]), 4)
        kern["ratios_per_round"] = [round(a / b, 4) for a, b in zip(got["logistic"], got[base])]
    if "parent" in got and "magnitude" in got:
        kern["ratio_magnitude_over_parent"] = round(statistics.median(got["magnitude"]) / statistics.median(got["parent"]), 4)
    kern.update(rows=B, reps=args.reps, disagreement=not args.plain)
    res["kernel_plain" if args.plain else "kernel"] = kern
    print(json.dumps(kern))

if args.trainer:
    from test_cost_head_cmbpo_gpu import _imagined_costs, run_cost_loop
    runs = []
    for seed in range(args.seeds):
        for loss in ("gaussian", "logistic"):
            algo, _, diags = run_cost_loop(dict(m_cost_loss=loss), seed=seed)
            cost, _, stored = _imagined_costs(algo)
            tab = algo.last_validation
            runs.append(dict(seed=seed, m_cost_loss=loss, n_imagined=int(cost.size),
                             share_outside_01=float(((cost < 0) | (cost > 1)).mean()), min_cost=float(cost.min()), max_cost=float(cost.max()),
                             brier_h1=float(tab["mse_cost"][0]), brier_hH=float(tab["mse_cost"][-1]),
                             cost_cm_h1=tab["cost_cm"][0].tolist(), cost_cm_all=tab["cost_cm"].sum(axis=0).tolist(),
                             n_h1=int(tab["n"][0])))
            print(json.dumps(runs[-1]))
    res["trainer"] = runs

if args.out:
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
