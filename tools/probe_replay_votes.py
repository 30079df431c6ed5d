"""What the static rules' votes add to the open-loop replay of real trajectories.  The settings of
tools/probe_replay_reliability.py -- AntSafe dims (29 / 8), 7 members of 512 hidden units, no learned head, WINDOWS windows x
HORIZON teacher-forced steps, HIP events around REPS back-to-back calls, after warm-up; the forms alternate in one process, the
first two timed rounds are dropped.
  replay   whole replays:
             other_run_reliab   with --other-lib PATH (the parent commit's libcmbpo_hip.so): its cmbpo_replay_run_reliab, rc = rr = NULL
             here_run_reliab    this library's cmbpo_replay_run_reliab, the same call: the off path.  It must sit inside the other
                                library's own (max - min) / median, and the tables of the two must be the same bit for bit
             here_run_votes     cmbpo_replay_run_votes under 'elite' / 'elite': the vote kernel and the table kernel in every step
  kernels  single calls on the arrays the last replay left, every window alive, per call (kernel plus launch gap, not separated):
             post / post_votes  cmbpo_fakeenv_post_votes with rv NULL / given: the difference is the vote kernel
             votes              cmbpo_replay_votes: the table kernel
             reliab, calibrate  cmbpo_replay_reliab (two columns, 15 bins: the reward and the last observation column stand in for
                                logits, the kernel does not care) and cmbpo_replay_calibrate at the same shape, for comparison
             compare            cmbpo_replay_compare (one_step mode; the arrays are reset behind every round)
The recording never ends a window, so that every form does the same work on every step.
    python tools/probe_replay_votes.py [out.json] [--other-lib PATH] [--windows N] [--horizon H] [--pairs K] [--reps R]"""
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
from cmbpo_amd.fake_env import FakeEnv
from cmbpo_amd.pens import PE
from cmbpo_amd.replay import ReplayBuffers

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--other-lib")
ap.add_argument("--windows", type=int, default=4096)
ap.add_argument("--horizon", type=int, default=5)
ap.add_argument("--pairs", type=int, default=8)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--kernel-reps", type=int, default=200)
args = ap.parse_args()

TASK, E, HID, WARM, DROP = "AntSafe-v2", 7, 512, 10, 2
D, A = synthetic.ENV_DIMS[TASK]
O = D + 1
B, H = args.windows, args.horizon
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
res = dict(command="python tools/probe_replay_votes.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0))


class _Space:
    def __init__(self, d):
        self.shape = (d,)


class _Env:
    observation_space, action_space = _Space(D), _Space(A)


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def timed(fn, reps):
    """Microseconds per call over `reps` back-to-back calls."""
    def run():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    return run


def alternate(fns, rounds):
    got = {k: [] for k in fns}
    for rnd in range(DROP + rounds):
        for k, fn in fns.items():
            x = fn()
            if rnd >= DROP:
                got[k].append(x)
    return got


ws, bs = synthetic.ensemble_weights(rng, E, D + A, HID, 2 * O, bias_scale=0.05)
model = PE(D + A, O, hidden_dims=(HID, HID), num_networks=E, num_elites=5, loss="MSPE", use_scaler_in=True, use_scaler_out=True, device=dev)
model.set_weights(ws, bs, synthetic.scaler(rng, D + A), (np.zeros((1, O), np.float32), np.full((1, O), 2.5e-3, np.float32)))
env = FakeEnv(_Env(), TASK, model, True, True, False, static_votes=True)
obs0 = synthetic.start_states(rng, B, TASK)
nxt = (obs0[None] + np.cumsum(rng.standard_normal((H, B, D)) * 0.05, axis=0)).astype(np.float32)
act = rng.uniform(-1, 1, (H, B, A)).astype(np.float32)
rew, cost = rng.standard_normal((H, B)).astype(np.float32), (rng.random((H, B)) < 0.3).astype(np.float32)
term = np.zeros((H, B), np.uint8)
inds = torch.from_numpy(rng.integers(0, E, (H, B)).astype(np.int32)).to(dev)
kw = dict(mode="one_step", ensemble=E, out_dim=O, device=dev)
make = lambda **k: ReplayBuffers(obs0, act, nxt, rew, cost, term, **kw, **k)
here = _lib.lib()
start = torch.from_numpy(obs0).to(dev)


def reset(rb):
    rb.t["cur_obs"].copy_(start)
    rb.t["alive"].fill_(1)


def run_reliab(lib, rb):
    def run():
        reset(rb)
        rc = lib.cmbpo_replay_run_reliab(C.byref(rb.rs), None, None, None, None, model.mlp.handle, env._task_id, E, inds.data_ptr(),
                                         _lib.current_stream())
        assert rc == 0, lib.cmbpo_last_error()
    return run


def run_votes(rb):
    def run():
        reset(rb)
        rb.run_votes(model.mlp.handle, env._task_id, E, inds)
    return run


bufs = dict(here_run_reliab=make(), here_run_votes=make(votes=dict()))
forms = dict(here_run_reliab=run_reliab(here, bufs["here_run_reliab"]), here_run_votes=run_votes(bufs["here_run_votes"]))
if args.other_lib:
    other = C.CDLL(os.path.abspath(args.other_lib))
    other.cmbpo_replay_run_reliab.restype, other.cmbpo_replay_run_reliab.argtypes = _lib.SIGNATURES["cmbpo_replay_run_reliab"]
    other.cmbpo_last_error.restype = C.c_char_p
    bufs["other_run_reliab"] = make()
    forms = dict(other_run_reliab=run_reliab(other, bufs["other_run_reliab"]), **forms)
for fn in forms.values():
    fn()
torch.cuda.synchronize()
same = lambda a, b: all(torch.equal(a.t[k].view(torch.int64), b.t[k].view(torch.int64)) for k in ("sums", "counts")) and \
    torch.equal(a.t["cur_obs"].view(torch.int32), b.t["cur_obs"].view(torch.int32)) and torch.equal(a.t["alive"], b.t["alive"])
assert same(bufs["here_run_reliab"], bufs["here_run_votes"])                 # the measure-only vote changes no verdict
res["measure_only_tables_bit_identical"] = True
if args.other_lib:
    assert same(bufs["here_run_reliab"], bufs["other_run_reliab"])
    res["tables_bit_identical_to_other_lib"] = True
vt = bufs["here_run_votes"].votes_table()
res.update(n_vote_per_horizon=vt["n_vote"].tolist(), split_rate_h1={k: float(vt[k]["split_rate"][0]) for k in ("cost", "term")})
for fn in forms.values():
    for _ in range(WARM):
        fn()
torch.cuda.synchronize()
us = alternate({k: timed(fn, args.reps) for k, fn in forms.items()}, args.pairs)
med = {k: statistics.median(v) for k, v in us.items()}
added = med["here_run_votes"] - med["here_run_reliab"]
res.update(task=TASK, windows=B, horizon=H, ensemble=E, hidden=HID, reps=args.reps, pairs=args.pairs, warmups=WARM, dropped_rounds=DROP,
           us_per_replay=us, median_us=med, spread={k: spread(v) for k, v in us.items()}, added_us_per_replay=added,
           added_us_per_horizon_step=added / H, added_share_of_run_reliab=added / med["here_run_reliab"], kernel_trace_taken=False)
print("replay of %d windows x %d steps: run_reliab here %.1f us (scatter %.4f); run_votes %.1f us: + %.1f us = %.2f us per step (%.1f %%)"
      % (B, H, med["here_run_reliab"], res["spread"]["here_run_reliab"], med["here_run_votes"], added, added / H,
         100 * added / med["here_run_reliab"]))
if args.other_lib:
    sp, ratio = spread(us["other_run_reliab"]), med["here_run_reliab"] / med["other_run_reliab"]
    res.update(other_spread=sp, median_ratio_here_over_other=ratio, within_other_spread=bool(abs(ratio - 1.0) <= sp))
    print("off path: here / the other library %.4f (the other's own spread %.4f) -> %s" % (ratio, sp, "within" if abs(ratio - 1.0) <= sp else "OUTSIDE"))

# the single calls, on the arrays of one replay under the votes with every table attached
full = make(calibration=True, reliability=dict(columns=[dict(name="a", col=D, target="cost"), dict(name="b", col=D - 1, target="term")], bins=15),
            votes=dict())
full.run_votes(model.mlp.handle, env._task_id, E, inds, calibration=True)
torch.cuda.synchronize()
reset(full)
out = full.step_outputs()
lead = (env._task_id, E, D, A, full.t["mean"].data_ptr(), full.t["var"].data_ptr(), B, full.t["cur_obs"].data_ptr(), full.t["act"].data_ptr(),
        inds.data_ptr(), None, None, B, out["next_obs"].data_ptr(), out["rew"].data_ptr(), out["term"].data_ptr(), out["cost"].data_ptr(),
        out["dkl_path"].data_ptr(), out["ep_var_mean"].data_ptr(), None, None, 0.0, 0.0, None, None, None, None, None)
rv = _lib.RuleVotesStruct()
rv.done_members, rv.cost_members = _lib.TERM_ELITE, _lib.TERM_ELITE
rv.done_votes, rv.cost_votes = full.v["done_votes"].data_ptr(), full.v["cost_votes"].data_ptr()


def post(votes):
    def run():
        rc = here.cmbpo_fakeenv_post_votes(*lead, C.byref(rv) if votes else None, _lib.current_stream())
        assert rc == 0, here.cmbpo_last_error()
    return run


def compare():
    full.compare(0)
    full.t["alive"].fill_(1)          # (one more tiny kernel per call: the fill rides in this figure)


calls = dict(post=post(False), post_votes=post(True), votes=lambda: full.votes(0), reliab=lambda: full.reliab(0),
             calibrate=lambda: full.calibrate(0), compare=compare, alive_fill=lambda: full.t["alive"].fill_(1))
for fn in calls.values():
    for _ in range(WARM):
        fn()
torch.cuda.synchronize()
kus = alternate({k: timed(fn, args.kernel_reps) for k, fn in calls.items()}, args.pairs)
kmed = {k: statistics.median(v) for k, v in kus.items()}
res["kernels"] = dict(reps=args.kernel_reps, us_per_call=kus, median_us=kmed, spread={k: spread(v) for k, v in kus.items()},
                      vote_kernel_us=kmed["post_votes"] - kmed["post"], table_kernel_us=kmed["votes"], reliab_kernel_us=kmed["reliab"],
                      calibrate_kernel_us=kmed["calibrate"], compare_kernel_us=kmed["compare"] - kmed["alive_fill"])
print("per call at %d windows: post %.2f us, with the vote kernel + %.2f us; the vote table %.2f us, reliab %.2f us, calibrate %.2f us, "
      "compare %.2f us" % (B, kmed["post"], kmed["post_votes"] - kmed["post"], kmed["votes"], kmed["reliab"], kmed["calibrate"],
                           kmed["compare"] - kmed["alive_fill"]))
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
