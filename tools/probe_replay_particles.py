"""What the particle pass adds to the open-loop replay of real trajectories.  The settings of
tools/probe_replay_votes.py -- AntSafe dims (29 / 8), 7 members of 512 hidden units, no learned head, WINDOWS windows x HORIZON
steps, S particles, HIP events around REPS back-to-back calls, after warm-up; the forms alternate in one process, the first two
timed rounds are dropped.
  replay   whole replays:
             other_run      with --other-lib PATH (the parent commit's libcmbpo_hip.so): its cmbpo_replay_run
             here_run       this library's cmbpo_replay_run, the same call: the replay without particles.  It must sit inside the
                            other library's own (max - min) / median, and the tables of the two must be the same bit for bit
             here_particles cmbpo_replay_run_particles on WINDOWS x S rows: the second pass of FakeEnv.replay(particles=S)
  kernels  single calls on the arrays the last replays left, every window alive, per call (kernel plus launch gap, not separated):
             particles      cmbpo_replay_particles (one_step mode; the alive fill that follows it is timed alone and taken off)
             compare        cmbpo_replay_compare at WINDOWS rows, likewise, for comparison
             forward_rows   cmbpo_ens_forward on the WINDOWS x S rows: what the particle pass spends most of a step in
The recording never ends a window, so that every form does the same work on every step.
    python tools/probe_replay_particles.py [out.json] [--other-lib PATH] [--windows N] [--horizon H] [--particles S] [--pairs K]
                                           [--reps R]"""
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
from cmbpo_amd.replay import ParticleBuffers, ReplayBuffers

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--other-lib")
ap.add_argument("--windows", type=int, default=4096)
ap.add_argument("--horizon", type=int, default=5)
ap.add_argument("--particles", type=int, default=8)
ap.add_argument("--pairs", type=int, default=8)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--kernel-reps", type=int, default=200)
args = ap.parse_args()

TASK, E, HID, WARM, DROP = "AntSafe-v2", 7, 512, 10, 2
D, A = synthetic.ENV_DIMS[TASK]
O = D + 1
B, H, S = args.windows, args.horizon, args.particles
R = B * S
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
res = dict(command="python tools/probe_replay_particles.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0))


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
env = FakeEnv(_Env(), TASK, model, True, True, False)
obs0 = synthetic.start_states(rng, B, TASK)
nxt = (obs0[None] + np.cumsum(rng.standard_normal((H, B, D)) * 0.05, axis=0)).astype(np.float32)
act = rng.uniform(-1, 1, (H, B, A)).astype(np.float32)
rew, cost = rng.standard_normal((H, B)).astype(np.float32), (rng.random((H, B)) < 0.3).astype(np.float32)
term = np.zeros((H, B), np.uint8)
inds = torch.from_numpy(rng.integers(0, E, (H, B)).astype(np.int32)).to(dev)
inds_rows = torch.from_numpy(rng.integers(0, E, (H, R)).astype(np.int32)).to(dev)
gen = torch.Generator(device=dev)
gen.manual_seed(1)
xi = torch.randn((H, B, S, D), generator=gen, dtype=torch.float32, device=dev)
make = lambda: ReplayBuffers(obs0, act, nxt, rew, cost, term, mode="one_step", ensemble=E, out_dim=O, device=dev)
pb = ParticleBuffers(S, obs0, act, nxt, rew, cost, term, mode="one_step", ensemble=E, out_dim=O, noise=xi, device=dev)
here = _lib.lib()
start = torch.from_numpy(obs0).to(dev)
start_rows = start.repeat_interleave(S, dim=0).contiguous()


def reset(rb):
    rb.t["cur_obs"].copy_(start)
    rb.t["alive"].fill_(1)


def run_plain(lib, rb):
    def run():
        reset(rb)
        rc = lib.cmbpo_replay_run(C.byref(rb.rs), model.mlp.handle, env._task_id, E, inds.data_ptr(), _lib.current_stream())
        assert rc == 0, lib.cmbpo_last_error()
    return run


def run_particles():
    pb.t["cur_obs"].copy_(start_rows)
    pb.t["alive"].fill_(1)
    pb.run(model.mlp.handle, env._task_id, E, inds_rows)


bufs = dict(here_run=make())
forms = dict(here_run=run_plain(here, bufs["here_run"]), here_particles=run_particles)
if args.other_lib:
    other = C.CDLL(os.path.abspath(args.other_lib))
    other.cmbpo_replay_run.restype, other.cmbpo_replay_run.argtypes = _lib.SIGNATURES["cmbpo_replay_run"]
    other.cmbpo_last_error.restype = C.c_char_p
    bufs["other_run"] = make()
    forms = dict(other_run=run_plain(other, bufs["other_run"]), **forms)
for fn in forms.values():
    fn()
torch.cuda.synchronize()
if args.other_lib:
    a, b = bufs["here_run"], bufs["other_run"]
    assert all(torch.equal(a.t[k].view(torch.int64), b.t[k].view(torch.int64)) for k in ("sums", "counts"))
    assert torch.equal(a.t["cur_obs"].view(torch.int32), b.t["cur_obs"].view(torch.int32)) and torch.equal(a.t["alive"], b.t["alive"])
    res["tables_bit_identical_to_other_lib"] = True
pt = pb.table()
res.update(n_per_horizon=pt["n"].tolist(), outlier_rate_h1=float(pt["outlier_rate"][0, :D].mean()),
           spread_skill_h1=float(pt["spread_skill"][0, :D].mean()))
for fn in forms.values():
    for _ in range(WARM):
        fn()
torch.cuda.synchronize()
us = alternate({k: timed(fn, args.reps) for k, fn in forms.items()}, args.pairs)
med = {k: statistics.median(v) for k, v in us.items()}
res.update(task=TASK, windows=B, horizon=H, particles=S, rows=R, ensemble=E, hidden=HID, reps=args.reps, pairs=args.pairs, warmups=WARM,
           dropped_rounds=DROP, us_per_replay=us, median_us=med, spread={k: spread(v) for k, v in us.items()},
           particle_pass_us_per_horizon_step=med["here_particles"] / H, particle_pass_over_plain_replay=med["here_particles"] / med["here_run"],
           kernel_trace_taken=False)
print("replay of %d windows x %d steps: plain %.1f us (scatter %.4f); the particle pass at S = %d (%d rows) %.1f us (scatter %.4f) = "
      "%.1f us per horizon step, %.2f x the plain replay" % (B, H, med["here_run"], res["spread"]["here_run"], S, R, med["here_particles"],
                                                             res["spread"]["here_particles"], med["here_particles"] / H,
                                                             med["here_particles"] / med["here_run"]))
if args.other_lib:
    sp, ratio = spread(us["other_run"]), med["here_run"] / med["other_run"]
    res.update(other_spread=sp, median_ratio_here_over_other=ratio, within_other_spread=bool(abs(ratio - 1.0) <= sp))
    print("without particles: here / the other library %.4f (the other's own spread %.4f) -> %s"
          % (ratio, sp, "within" if abs(ratio - 1.0) <= sp else "OUTSIDE"))

# the single calls, on the arrays the replays left
rb = bufs["here_run"]
reset(rb)
pb.t["alive"].fill_(1)


def particles():
    pb.particles(0)
    pb.t["alive"].fill_(1)          # (one more tiny kernel per call: timed alone below and taken off)


def compare():
    rb.compare(0)
    rb.t["alive"].fill_(1)


def forward_rows():
    rc = here.cmbpo_ens_forward(model.mlp.handle, pb.t["cur_obs"].data_ptr(), D, pb.t["act"].data_ptr(), A, None, None, R, R,
                                pb.t["mean"].data_ptr(), pb.t["var"].data_ptr(), _lib.current_stream())
    assert rc == 0, here.cmbpo_last_error()


calls = dict(particles=particles, compare=compare, fill_rows=lambda: pb.t["alive"].fill_(1), fill_windows=lambda: rb.t["alive"].fill_(1),
             forward_rows=forward_rows)
for fn in calls.values():
    for _ in range(WARM):
        fn()
torch.cuda.synchronize()
kus = alternate({k: timed(fn, args.kernel_reps) for k, fn in calls.items()}, args.pairs)
kmed = {k: statistics.median(v) for k, v in kus.items()}
res["kernels"] = dict(reps=args.kernel_reps, us_per_call=kus, median_us=kmed, spread={k: spread(v) for k, v in kus.items()},
                      particles_kernel_us=kmed["particles"] - kmed["fill_rows"], compare_kernel_us=kmed["compare"] - kmed["fill_windows"],
                      forward_rows_us=kmed["forward_rows"])
print("per call: the particle kernel at %d rows %.2f us, the compare kernel at %d rows %.2f us, the forward at %d rows %.1f us"
      % (R, kmed["particles"] - kmed["fill_rows"], B, kmed["compare"] - kmed["fill_windows"], R, kmed["forward_rows"]))
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
