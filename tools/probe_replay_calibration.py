"""What the calibration table adds to the open-loop replay of real trajectories: the settings of
tools/probe_replay.py -- AntSafe dims (29 / 8), 7 members of 512 hidden units, WINDOWS windows x HORIZON teacher-forced steps,
HIP events around REPS back-to-back replays, after warm-up; the two forms alternate in one process, the first two timed rounds
are dropped.
  plain        cmbpo_replay_run:            H x (forward -> post -> compare), finish
  calibrated   cmbpo_replay_run_calibrated: H x (forward -> post -> calibrate -> compare), both finishes
The recording never ends a window, so that both forms do the same work on every step.  Reported: the two medians, the scatter
of the repeated rounds ((max - min) / median), the added time per replay and per horizon step.  The plain tables of the two
forms must be the same bit for bit.  No kernel trace is taken: the added time is kernel plus launch gap, not separated.
    python tools/probe_replay_calibration.py [out.json] [--windows N] [--horizon H] [--pairs K] [--reps R]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import cmbpo_amd  # noqa: F401
from cmbpo_amd import synthetic
from cmbpo_amd.fake_env import FakeEnv
from cmbpo_amd.pens import PE
from cmbpo_amd.replay import ReplayBuffers

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--windows", type=int, default=4096)
ap.add_argument("--horizon", type=int, default=10)
ap.add_argument("--pairs", type=int, default=8)
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()

TASK, E, HID, WARM, DROP = "AntSafe-v2", 7, 512, 10, 2
D, A = synthetic.ENV_DIMS[TASK]
B, H = args.windows, args.horizon
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)


class _Space:
    def __init__(self, d):
        self.shape = (d,)


class _Env:
    observation_space, action_space = _Space(D), _Space(A)


ws, bs = synthetic.ensemble_weights(rng, E, D + A, HID, 2 * (D + 1), bias_scale=0.05)
model = PE(D + A, D + 1, hidden_dims=(HID, HID), num_networks=E, num_elites=5, loss="MSPE", use_scaler_in=True, use_scaler_out=True,
           device=dev)
model.set_weights(ws, bs, synthetic.scaler(rng, D + A), (np.zeros((1, D + 1), np.float32), np.full((1, D + 1), 2.5e-3, np.float32)))
env = FakeEnv(_Env(), TASK, model, True, True, False)
obs0 = synthetic.start_states(rng, B, TASK)
nxt = (obs0[None] + np.cumsum(rng.standard_normal((H, B, D)) * 0.05, axis=0)).astype(np.float32)
act = rng.uniform(-1, 1, (H, B, A)).astype(np.float32)
rew, cost = rng.standard_normal((H, B)).astype(np.float32), (rng.random((H, B)) < 0.3).astype(np.float32)
term = np.zeros((H, B), np.uint8)
inds = torch.from_numpy(rng.integers(0, E, (H, B)).astype(np.int32)).to(dev)
rb = ReplayBuffers(obs0, act, nxt, rew, cost, term, mode="one_step", ensemble=E, out_dim=D + 1, device=dev, calibration=True)
rb.set_elite(inds)
start = rb.t["cur_obs"].clone()


def rewind():
    rb.t["cur_obs"].copy_(start)
    rb.t["alive"].fill_(1)


def plain():
    rewind()
    rb.run(model.mlp.handle, env._task_id, E, inds)


def calibrated():
    rewind()
    rb.run_calibrated(model.mlp.handle, env._task_id, E)


forms = {"plain": plain, "calibrated": calibrated}


def measure(fn):
    """Microseconds per replay over args.reps back-to-back replays."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.reps


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


tables = {}
for name, fn in forms.items():
    fn()
    torch.cuda.synchronize()
    tables[name] = (rb.t["sums"].clone(), rb.t["counts"].clone())
assert torch.equal(tables["plain"][0].view(torch.int64), tables["calibrated"][0].view(torch.int64))
assert torch.equal(tables["plain"][1], tables["calibrated"][1])
cal = rb.calibration_table()
assert (cal["n"] + cal["n_skipped"] == rb.table()["n"]).all()
for fn in forms.values():
    for _ in range(WARM):
        fn()
torch.cuda.synchronize()
us = {n: [] for n in forms}
for rnd in range(DROP + args.pairs):
    for n, fn in forms.items():
        t_us = measure(fn)
        if rnd >= DROP:
            us[n].append(t_us)
med = {k: statistics.median(v) for k, v in us.items()}
added = med["calibrated"] - med["plain"]
res = dict(command="python tools/probe_replay_calibration.py " + " ".join(sys.argv[1:]), task=TASK, windows=B, horizon=H, ensemble=E,
           hidden=HID, reps=args.reps, pairs=args.pairs, warmups=WARM, dropped_rounds=DROP, device=torch.cuda.get_device_name(0),
           plain_tables_bit_identical=True, n_cal_per_horizon=cal["n"].tolist(), n_skipped_per_horizon=cal["n_skipped"].tolist(),
           z2_al_h1_mean_over_obs_columns=float(np.mean(cal["z2_al"][0, :D])),
           us_per_replay=us, median_us=med, spread={k: spread(v) for k, v in us.items()},
           added_us_per_replay=added, added_us_per_horizon_step=added / H, added_share_of_plain=added / med["plain"],
           kernel_trace_taken=False)
print("replay of %d windows x %d steps: plain %.1f us, calibrated %.1f us; the table adds %.1f us = %.2f us per horizon step "
      "(%.1f %% of the plain replay; scatter %.4f / %.4f)" % (B, H, med["plain"], med["calibrated"], added, added / H,
                                                             100 * added / med["plain"], res["spread"]["plain"],
                                                             res["spread"]["calibrated"]))
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
