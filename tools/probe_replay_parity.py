"""Is the model replay of another build of the library (the parent commit's libcmbpo_hip.so) the replay of this tree, bit for
bit -- and as fast?  The settings of tools/probe_replay_votes.py: AntSafe dims (29 / 8), 7 members of 512 hidden units, no learned
head, WINDOWS windows x HORIZON teacher-forced steps, the recording never ends a window.  Two run forms, each through both
libraries on buffers of their own built from the same inputs:
  votes      cmbpo_replay_run_votes under 'elite' / 'elite' with the calibration and the reliability table on: all four tables
             of the plain descriptor
  particles  cmbpo_replay_run_particles with S particles per window
parity: the bytes of every sums, counts, part_sum and part_cnt, of cur_obs and of alive after one run.  Any difference: exit 1.
speed:  HIP events around REPS back-to-back runs after warm-up; the four (library, form) pairs alternate in one process, the first
        two rounds are dropped.  Per form: median here / median other against the other library's own (max - min) / median.
        And per call, the same way, the five *_finish entries on the arrays the runs left (what the one fold kernel replaced).
    python tools/probe_replay_parity.py [out.json] --other-lib PATH [--windows N] [--horizon H] [--particles S] [--pairs K] [--reps R]"""
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
ap.add_argument("--other-lib", required=True)
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
ENTRIES = ("cmbpo_replay_run_votes", "cmbpo_replay_run_particles", "cmbpo_replay_finish", "cmbpo_replay_calib_finish",
           "cmbpo_replay_reliab_finish", "cmbpo_replay_votes_finish", "cmbpo_replay_particles_finish")


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


def compare(us, names):
    """{name: figures} for the pairs other_<name> / here_<name> of `us`."""
    out = {}
    for n in names:
        o, h = us["other_" + n], us["here_" + n]
        sp, ratio = spread(o), statistics.median(h) / statistics.median(o)
        out[n] = dict(median_us_other=statistics.median(o), median_us_here=statistics.median(h), spread_other=sp, spread_here=spread(h),
                      median_ratio_here_over_other=ratio, within_other_spread=bool(abs(ratio - 1.0) <= sp))
        print("%-16s here %.2f us, other %.2f us: here / other %.4f (the other's own spread %.4f) -> %s"
              % (n, out[n]["median_us_here"], out[n]["median_us_other"], ratio, sp, "within" if out[n]["within_other_spread"] else "OUTSIDE"))
    return out


ws, bs = synthetic.ensemble_weights(rng, E, D + A, HID, 2 * O, bias_scale=0.05)
model = PE(D + A, O, hidden_dims=(HID, HID), num_networks=E, num_elites=5, loss="MSPE", use_scaler_in=True, use_scaler_out=True, device=dev)
model.set_weights(ws, bs, synthetic.scaler(rng, D + A), (np.zeros((1, O), np.float32), np.full((1, O), 2.5e-3, np.float32)))
env = FakeEnv(_Env(), TASK, model, True, True, False, static_votes=True)
obs0 = synthetic.start_states(rng, B, TASK)
nxt = (obs0[None] + np.cumsum(rng.standard_normal((H, B, D)) * 0.05, axis=0)).astype(np.float32)
act = rng.uniform(-1, 1, (H, B, A)).astype(np.float32)
rew, cost = rng.standard_normal((H, B)).astype(np.float32), (rng.random((H, B)) < 0.3).astype(np.float32)
term = np.zeros((H, B), np.uint8)
inds = rng.integers(0, E, (H, B)).astype(np.int32)
inds_rows = torch.from_numpy(rng.integers(0, E, (H, R)).astype(np.int32)).to(dev)
gen = torch.Generator(device=dev)
gen.manual_seed(1)
xi = torch.randn((H, B, S, D), generator=gen, dtype=torch.float32, device=dev)
start = torch.from_numpy(obs0).to(dev)
start_rows = start.repeat_interleave(S, dim=0).contiguous()

here = _lib.lib()
other = C.CDLL(os.path.abspath(args.other_lib))
for name in ENTRIES:
    getattr(other, name).restype, getattr(other, name).argtypes = _lib.SIGNATURES[name]
other.cmbpo_last_error.restype = C.c_char_p
LIBS = dict(other=other, here=here)


def ok(lib, rc):
    assert rc == 0, lib.cmbpo_last_error()


def votes_buffers():
    rb = ReplayBuffers(obs0, act, nxt, rew, cost, term, mode="one_step", ensemble=E, out_dim=O, device=dev, calibration=True, votes=dict(),
                       reliability=dict(columns=[dict(name="a", col=D, target="cost"), dict(name="b", col=D - 1, target="term")], bins=15))
    rb.set_elite(inds)
    return rb


def run_votes(lib, rb):
    def run():
        rb.t["cur_obs"].copy_(start)
        rb.t["alive"].fill_(1)
        ok(lib, lib.cmbpo_replay_run_votes(C.byref(rb.rs), C.byref(rb.cs), C.byref(rb.rr), C.byref(rb.vs), None, None, model.mlp.handle,
                                           env._task_id, E, None, _lib.current_stream()))
    return run


def run_particles(lib, pb):
    def run():
        pb.t["cur_obs"].copy_(start_rows)
        pb.t["alive"].fill_(1)
        ok(lib, lib.cmbpo_replay_run_particles(C.byref(pb.ps), None, None, model.mlp.handle, env._task_id, E, inds_rows.data_ptr(),
                                               _lib.current_stream()))
    return run


rbs = {k: votes_buffers() for k in LIBS}
pbs = {k: ParticleBuffers(S, obs0, act, nxt, rew, cost, term, mode="one_step", ensemble=E, out_dim=O, noise=xi, device=dev) for k in LIBS}
forms = {}
for k, lib in LIBS.items():
    forms[k + "_votes"] = run_votes(lib, rbs[k])
    forms[k + "_particles"] = run_particles(lib, pbs[k])
for fn in forms.values():
    fn()
torch.cuda.synchronize()

# parity
TABLE = ("sums", "counts", "part_sum", "part_cnt")
sets = [("plain", rbs["here"].t, rbs["other"].t, TABLE + ("cur_obs", "alive")), ("calibration", rbs["here"].c, rbs["other"].c, TABLE),
        ("reliability", rbs["here"].r, rbs["other"].r, TABLE), ("votes", rbs["here"].v, rbs["other"].v, ("counts", "part_cnt")),
        ("particles", pbs["here"].t, pbs["other"].t, TABLE + ("cur_obs", "alive"))]
parity, differs = {}, []
for name, a, b, keys in sets:
    for k in keys:
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        same = x.shape == y.shape and bool(np.array_equal(x.view(np.uint8), y.view(np.uint8)))
        parity["%s.%s" % (name, k)] = dict(bytes=int(x.nbytes), nonzero=int(np.count_nonzero(x)), identical=same)
        if not same:
            differs.append("%s.%s" % (name, k))
res = dict(command="python tools/probe_replay_parity.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0), task=TASK, windows=B,
           horizon=H, particles=S, ensemble=E, hidden=HID, parity=parity, differs=differs, bit_identical=not differs)
print("parity: %d arrays compared, %d differ %s" % (len(parity), len(differs), differs))

# speed: the run forms
for fn in forms.values():
    for _ in range(WARM):
        fn()
torch.cuda.synchronize()
us = alternate({k: timed(fn, args.reps) for k, fn in forms.items()}, args.pairs)
res.update(reps=args.reps, pairs=args.pairs, warmups=WARM, dropped_rounds=DROP, us_per_run=us, runs=compare(us, ("votes", "particles")))

# speed: the finish entries, on the arrays of the last runs
calls = {}
for k, lib in LIBS.items():
    rb, pb, st = rbs[k], pbs[k], _lib.current_stream()
    calls[k + "_finish"] = lambda lib=lib, rb=rb: ok(lib, lib.cmbpo_replay_finish(C.byref(rb.rs), st))
    calls[k + "_calib_finish"] = lambda lib=lib, rb=rb: ok(lib, lib.cmbpo_replay_calib_finish(C.byref(rb.rs), C.byref(rb.cs), st))
    calls[k + "_reliab_finish"] = lambda lib=lib, rb=rb: ok(lib, lib.cmbpo_replay_reliab_finish(C.byref(rb.rs), C.byref(rb.rr), st))
    calls[k + "_votes_finish"] = lambda lib=lib, rb=rb: ok(lib, lib.cmbpo_replay_votes_finish(C.byref(rb.rs), C.byref(rb.vs), st))
    calls[k + "_particles_finish"] = lambda lib=lib, pb=pb: ok(lib, lib.cmbpo_replay_particles_finish(C.byref(pb.ps), st))
for fn in calls.values():
    for _ in range(WARM):
        fn()
torch.cuda.synchronize()
kus = alternate({k: timed(fn, args.kernel_reps) for k, fn in calls.items()}, args.pairs)
res.update(kernel_reps=args.kernel_reps, us_per_call=kus,
           finish_calls=compare(kus, ("finish", "calib_finish", "reliab_finish", "votes_finish", "particles_finish")))
res["runs_within_other_spread"] = all(v["within_other_spread"] for v in res["runs"].values())
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
sys.exit(1 if differs else 0)
