"""What the open-loop replay of real trajectories costs: AntSafe dims (29 / 8), 7 members of 512 hidden units,
WINDOWS windows x HORIZON steps, HIP events around REPS back-to-back replays, after warm-up; the three forms alternate in one
process, the first two timed rounds are dropped.
  one_call   cmbpo_replay_run: H x (forward -> post -> compare), finish, one call
  loop       the same steps issued one call at a time (FakeEnv.step_device, cmbpo_replay_compare, cmbpo_replay_finish)
  step_only  the loop of FakeEnv.step_device alone: the existing forward and post, no comparison
The recording never ends a window (full lengths, no terminal, teacher-forced) so that every form does the same work on every
step.  Reported: the three medians, the scatter of the repeated rounds ((max - min) / median), compare + finish as a share of
the replay (loop against step_only) and the one-call form against the loop.  one_call and loop must give the same table, bit
for bit.
    python tools/probe_replay.py [out.json] [--windows N] [--horizon H] [--pairs K] [--reps R]"""
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
rb = ReplayBuffers(obs0, act, nxt, rew, cost, term, mode="one_step", ensemble=E, out_dim=D + 1, device=dev)
start = rb.t["cur_obs"].clone()


def rewind():
    rb.t["cur_obs"].copy_(start)
    rb.t["alive"].fill_(1)


def one_call():
    rewind()
    rb.run(model.mlp.handle, env._task_id, E, inds)


def loop(compare=True):
    rewind()
    outs, scratch = rb.step_outputs(), (rb.t["mean"], rb.t["var"])
    for h in range(H):
        env.step_device(rb.t["cur_obs"], rb.t["act"][h], inds[h], outs, scratch=scratch)
        if compare:
            rb.compare(h)
    if compare:
        rb.finish()


forms = {"one_call": one_call, "loop": loop, "step_only": lambda: loop(False)}


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
for name in ("one_call", "loop"):
    forms[name]()
    torch.cuda.synchronize()
    tables[name] = (rb.t["sums"].clone(), rb.t["counts"].clone())
assert torch.equal(tables["one_call"][0].view(torch.int64), tables["loop"][0].view(torch.int64))
assert torch.equal(tables["one_call"][1], tables["loop"][1])
table = rb.table()
assert (table["n"] + table["n_nonfinite"] == B).all()
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
res = dict(command="python tools/probe_replay.py " + " ".join(sys.argv[1:]), task=TASK, windows=B, horizon=H, ensemble=E, hidden=HID,
           reps=args.reps, pairs=args.pairs, warmups=WARM, dropped_rounds=DROP, device=torch.cuda.get_device_name(0),
           one_call_and_loop_tables_bit_identical=True, n_per_horizon=table["n"].tolist(),
           us_per_replay=us, median_us=med, spread={k: spread(v) for k, v in us.items()},
           compare_and_finish_share_of_loop=(med["loop"] - med["step_only"]) / med["loop"],
           median_ratio_one_call_over_loop=med["one_call"] / med["loop"])
print("replay of %d windows x %d steps: one call %.1f us, loop %.1f us, step_device alone %.1f us; compare + finish %.1f %% of "
      "the loop; one call / loop %.4f (scatter %.4f / %.4f)" % (B, H, med["one_call"], med["loop"], med["step_only"],
                                                                 100 * res["compare_and_finish_share_of_loop"],
                                                                 res["median_ratio_one_call_over_loop"], res["spread"]["one_call"],
                                                                 res["spread"]["loop"]))
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
