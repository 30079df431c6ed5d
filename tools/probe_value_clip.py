"""What the clipped / sample-weighted value loss costs in the critic training step: one train_op of the critic of
bench.py --full's training line (E = 3, obs -> 128 -> 128 -> 1, 'MSE', both scalers, batch 2048 of ROWS device-resident rows,
per-member bootstrap rows), HIP events around REPS back-to-back steps, alternating pairs in one process, the first two
rounds dropped (the method of tools/probe_task_rules.py).
  (a) with --other-lib PATH (another build of libcmbpo_hip.so, e.g. the parent commit's): the plain step there against the
      plain step here -- the old path must not pay for the feature.  Three steps from the same weights must leave bit-identical
      weights and moments; the ratio of medians must stay within 1 + twice the spread the other library shows against
      itself over its own repeats, (max - min) / median.
  (b) here: the weighted, the clipped and the clipped + weighted step against the plain one.  Recorded, not gated; the two
      single variants tell where the time goes (weights: one more gather; clipping: one more gather and the two small kernels
      of the clip range in front of the step).
The exit status is non-zero if (a) is outside; the record is written either way.
    python tools/probe_value_clip.py [out.json] [--other-lib PATH] [--rows N] [--batch B] [--pairs K] [--reps R]"""
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
ap.add_argument("--rows", type=int, default=200000)
ap.add_argument("--batch", type=int, default=2048)
ap.add_argument("--pairs", type=int, default=8)
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()

TASK, E, H, WARM, DROP = "AntSafe-v2", 3, 128, 50, 2
I = synthetic.ENV_DIMS[TASK][0]
N, B = args.rows, args.batch
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
x_h = synthetic.start_states(rng, N, TASK).astype(np.float32)
ret_h = (np.tanh(x_h[:, :3]).sum(1, keepdims=True) + 0.1 * rng.standard_normal((N, 1))).astype(np.float32)
x, ret = t(x_h), t(ret_h)
old = t((ret_h + 0.3 * rng.standard_normal((N, 1))).astype(np.float32))
w = t(rng.uniform(0.25, 2.0, N).astype(np.float32))
idx = torch.randint(0, N, (E, B * 8), dtype=torch.int32, device=dev)
ws = [(rng.standard_normal(s) / (2.0 * np.sqrt(s[1]))).astype(np.float32) for s in ((E, I, H), (E, H, H), (E, H, 1))]
bs = [np.zeros((E, s), np.float32) for s in (H, H, 1)]
mom = [x_h.mean(0), x_h.var(0), ret_h.mean(0), ret_h.var(0)]
mom = [np.ascontiguousarray(m, np.float32) for m in mom]


def bind(lib, names):
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


class Trainer:
    """One critic ensemble and its trainer behind the C-ABI of `lib` (this build's or the other's)."""

    def __init__(self, lib):
        self.lib, self.m, self.h = lib, C.c_void_p(), C.c_void_p()
        self.ok(lib.cmbpo_mlp_create(C.byref(self.m), E, I, H, 1, _lib.ACT_SWISH, _lib.HEAD_DETMEAN))
        dec = (C.c_double * 3)(2.5e-7, 5e-7, 1e-6)
        self.ok(lib.cmbpo_trainer_create(C.byref(self.h), self.m, B, 1e-4, dec))
        self.reset()

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError(self.lib.cmbpo_last_error())

    def reset(self):
        p, s = _lib.ptr, _lib.current_stream()
        self.ok(self.lib.cmbpo_trainer_set_weights(self.h, p(ws[0]), p(bs[0]), p(ws[1]), p(bs[1]), p(ws[2]), p(bs[2]), s))
        self.ok(self.lib.cmbpo_mlp_set_scalers(self.m, p(mom[0]), p(mom[1]), p(mom[2]), p(mom[3]), s))
        self.ok(self.lib.cmbpo_trainer_reset_optimizer(self.h, s))

    def step(self, k, extras=None):
        a = (self.h, x.data_ptr(), I, ret.data_ptr(), 1, idx.data_ptr() + 4 * B * (k % 8), B * 8, B)
        if extras is None:
            self.ok(self.lib.cmbpo_trainer_step(*a, _lib.current_stream()))
        else:
            self.ok(self.lib.cmbpo_trainer_step_ex(*a, C.byref(extras), _lib.current_stream()))

    def state(self):
        out = []
        for get in (lambda a: self.lib.cmbpo_trainer_get_weights(self.h, *a, _lib.current_stream()),
                    lambda a: self.lib.cmbpo_trainer_get_moments(self.h, 0, *a, _lib.current_stream()),
                    lambda a: self.lib.cmbpo_trainer_get_moments(self.h, 1, *a, _lib.current_stream())):
            arrs = [np.empty_like(v) for pair in zip(ws, bs) for v in pair]
            self.ok(get([_lib.ptr(v) for v in arrs]))
            out += arrs
        return out


NAMES = ["cmbpo_last_error", "cmbpo_mlp_create", "cmbpo_trainer_create", "cmbpo_trainer_set_weights", "cmbpo_mlp_set_scalers",
         "cmbpo_trainer_reset_optimizer", "cmbpo_trainer_step", "cmbpo_trainer_get_weights", "cmbpo_trainer_get_moments"]
here = Trainer(_lib.lib())
X = _lib.TrainExtrasStruct
variants = {"plain": None, "weights": X(w.data_ptr(), None, 0.1), "clip": X(None, old.data_ptr(), 0.1),
            "clip_weights": X(w.data_ptr(), old.data_ptr(), 0.1)}
configs = {"here_" + k: (here, v) for k, v in variants.items()}
if args.other_lib:
    configs["other_plain"] = (Trainer(bind(C.CDLL(os.path.abspath(args.other_lib)), NAMES)), None)


def measure(tr, extras):
    """Microseconds per step over args.reps back-to-back steps."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(args.reps):
        tr.step(k, extras)
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


states = {}
for name, (tr, extras) in configs.items():       # three steps from the same weights, then the warm-up
    tr.reset()
    for k in range(3):
        tr.step(k, extras)
    torch.cuda.synchronize()
    states[name] = tr.state()
    for k in range(WARM):
        tr.step(k, extras)
torch.cuda.synchronize()
# (the record names the options, not where this run kept its files)
command = "python tools/probe_value_clip.py out.json%s --rows %d --batch %d --pairs %d --reps %d" % (
    " --other-lib <another build of libcmbpo_hip.so>" if args.other_lib else "", N, B, args.pairs, args.reps)
res = dict(command=command, critic=f"E={E} {I}->{H}->{H}->1 MSE + Adam",
           rows=N, batch=B, reps=args.reps, pairs=args.pairs, warmups=WARM, dropped_rounds=DROP,
           device=torch.cuda.get_device_name(0))
res["clipped_step_differs_from_plain"] = bool(any(not np.array_equal(a, b) for a, b in zip(states["here_plain"], states["here_clip_weights"])))
if args.other_lib:
    same = all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(states["here_plain"], states["other_plain"]))
    res["plain_step_bit_identical_to_other_lib"] = bool(same)
    us = rounds(["other_plain", "here_plain"])
    sp = spread(us["other_plain"])
    ratio = statistics.median(us["here_plain"]) / statistics.median(us["other_plain"])
    res["a"] = dict(us_per_step=us, other_spread=sp, here_spread=spread(us["here_plain"]), median_ratio_here_over_other=ratio,
                    gate=1.0 + 2.0 * sp, within_gate=bool(same and ratio <= 1.0 + 2.0 * sp))
    print("(a) plain step here / other: %.4f (gate 1 + 2 x %.4f), bits %s -> %s"
          % (ratio, sp, "equal" if same else "DIFFER", "within" if res["a"]["within_gate"] else "OUTSIDE"))
us = rounds(["here_plain", "here_weights", "here_clip", "here_clip_weights"])
med = {k: statistics.median(v) for k, v in us.items()}
margin = 2.0 * (res["a"]["other_spread"] if "a" in res else spread(us["here_plain"]))
res["b"] = dict(us_per_step=us, median_us=med, plain_spread=spread(us["here_plain"]), margin=margin,
                **{"median_ratio_%s_over_plain" % k[5:]: med[k] / med["here_plain"] for k in med if k != "here_plain"})
res["b"]["clip_weights_within_margin"] = bool(res["b"]["median_ratio_clip_weights_over_plain"] <= 1.0 + margin)
print("(b) over plain: weights %.4f, clip %.4f, clip + weights %.4f (margin 1 + %.4f; recorded, not gated)"
      % (res["b"]["median_ratio_weights_over_plain"], res["b"]["median_ratio_clip_over_plain"],
         res["b"]["median_ratio_clip_weights_over_plain"], margin))
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
if "a" in res and not res["a"]["within_gate"]:
    sys.exit("outside: a")
