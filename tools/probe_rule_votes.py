"""What the ensemble-voted static rules cost.
  --kernel   the post step alone at ROWS rows (AntSafe dims 27 / 8, E = 7), HIP events around REPS back-to-back calls, alternating
             rounds, by the method of tools/probe_term_draws.py -- three cases per row count:
             (a) with --other-lib PATH (the parent commit's libcmbpo_hip.so): cmbpo_fakeenv_post_term_draws there;
             (b) here with the votes off: cmbpo_fakeenv_post_votes, rv == NULL (the same instances: it must sit inside the other
                 library's own (max - min) / median);
             (c) here with the votes on ('any' / 'mean', both vote arrays): the post kernel and the vote kernel behind it.  The
                 vote kernel's own time is (c) - (b); its bytes, from the shapes, over that time against the HBM peak.
  --rollout  a rollout step at B = 1000 and B = 100 000 (512-wide model, the world of tests/test_rule_votes_gpu.py, the native loop
             from a reset, per step) with FakeEnv(static_votes=True) -- the measure-only vote: the same verdicts, so the same
             branches live in both -- against the default.
    python tools/probe_rule_votes.py [out.json] [--kernel] [--rollout] [--other-lib PATH]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import cmbpo_amd  # noqa: F401
from cmbpo_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--kernel", action="store_true")
ap.add_argument("--rollout", action="store_true")
ap.add_argument("--other-lib")
ap.add_argument("--pairs", type=int, default=8)
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()

E, DROP = 7, 2
HBM_PEAK = 8.0e12          # bytes / s (MI355X, HBM3E)
dev = torch.device("cuda:0")
res = dict(command="python tools/probe_rule_votes.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0))


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def alternate(fns, rounds):
    """{name: [figure per round]} with the configurations taken in turn, DROP rounds thrown away."""
    got = {k: [] for k in fns}
    for rnd in range(DROP + rounds):
        for k, fn in fns.items():
            x = fn()
            if rnd >= DROP:
                got[k].append(x)
    return got


if args.kernel:
    import test_rule_votes_gpu as tv
    D, A = tv.DIMS["ant"]
    here = _lib.lib()
    other = None
    if args.other_lib:
        other = C.CDLL(os.path.abspath(args.other_lib))
        other.cmbpo_fakeenv_post_term_draws.restype, other.cmbpo_fakeenv_post_term_draws.argtypes = \
            _lib.SIGNATURES["cmbpo_fakeenv_post_term_draws"]
        other.cmbpo_last_error.restype = C.c_char_p
    rows = {}
    for N in (100000, 1000):
        rng = np.random.default_rng(N)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        obs, act, mean, var, inds = (t(a) for a in tv._inputs("ant", E, N, rng))
        f = dict(dtype=torch.float32, device=dev)
        out = dict(next_obs=torch.empty((N, D), **f), rew=torch.empty(N, **f), term=torch.empty(N, dtype=torch.uint8, device=dev),
                   cost=torch.empty(N, **f), dkl_path=torch.empty(N, **f), ep_var_mean=torch.empty(N, **f))
        dv, cv = torch.empty(N, dtype=torch.uint8, device=dev), torch.empty(N, dtype=torch.uint8, device=dev)
        rv = _lib.RuleVotesStruct()
        rv.done_members, rv.cost_members, rv.done_votes, rv.cost_votes = _lib.TERM_ANY, _lib.VOTE_MEAN, _lib.ptr(dv), _lib.ptr(cv)
        lead = lambda: (_lib.TASK_ANTSAFE, E, D, A, _lib.ptr(mean), _lib.ptr(var), N, _lib.ptr(obs), _lib.ptr(act), _lib.ptr(inds),
                        None, None, N, _lib.ptr(out["next_obs"]), _lib.ptr(out["rew"]), _lib.ptr(out["term"]), _lib.ptr(out["cost"]),
                        _lib.ptr(out["dkl_path"]), _lib.ptr(out["ep_var_mean"]), None, None, 0.0, 0.0, None, None, None, None, None)

        def parent_post(lib):
            rc = lib.cmbpo_fakeenv_post_term_draws(*lead(), _lib.current_stream())
            assert rc == 0, lib.cmbpo_last_error()

        def votes(on):
            def call(lib):
                rc = lib.cmbpo_fakeenv_post_votes(*lead(), C.byref(rv) if on else None, _lib.current_stream())
                assert rc == 0, lib.cmbpo_last_error()
            return call

        def timed(fn, lib):
            def run():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    fn(lib)
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) * 1e3 / args.reps
            return run

        fns = {"here_votes_off": timed(votes(False), here), "here_votes_on": timed(votes(True), here)}
        if other is not None:
            parent_post(other)
            torch.cuda.synchronize()
            theirs = {k: v.clone() for k, v in out.items()}
            votes(False)(here)
            torch.cuda.synchronize()
            for k, v in out.items():
                assert torch.equal(v.view(torch.int32) if v.dtype == torch.float32 else v,
                                   theirs[k].view(torch.int32) if v.dtype == torch.float32 else theirs[k]), k
            fns = {"other_post": timed(parent_post, other), **fns}
        for fn in fns.values():
            for _ in range(2):
                fn()
        us = alternate(fns, args.pairs)
        votes(True)(here)
        torch.cuda.synchronize()
        med = {n: statistics.median(v) for n, v in us.items()}
        vote_us = med["here_votes_on"] - med["here_votes_off"]
        # the vote kernel's traffic, from the shapes: reads E means + obs per (row, dim) and the elite index, writes term, cost
        # and two vote bytes per row (no xi, no variances, no disagreement)
        vote_bytes = N * (E * D * 4 + D * 4 + 4) + N * (1 + 4 + 1 + 1)
        # the post kernel: means and variances of every member, obs, elite; next_obs and five scalars per row
        post_bytes = N * (2 * E * D * 4 + D * 4 + 4 + 4) + N * (D * 4 + 4 + 1 + 4 + 4 + 4)
        k = dict(rows=N, reps=args.reps, pairs=args.pairs, dropped_rounds=DROP, us_per_call=us, median_us=med,
                 spread={n: spread(v) for n, v in us.items()}, vote_kernel_us=vote_us, vote_kernel_bytes=vote_bytes,
                 vote_kernel_share_of_hbm_peak=vote_bytes / (vote_us * 1e-6) / HBM_PEAK if vote_us > 0 else None,
                 post_kernel_bytes=post_bytes, post_kernel_share_of_hbm_peak=post_bytes / (med["here_votes_off"] * 1e-6) / HBM_PEAK,
                 vote_over_post=vote_us / med["here_votes_off"], mixed_cost_votes=float(((cv > 0) & (cv < E)).float().mean()))
        if other is not None:
            sp = spread(us["other_post"])
            ratio = med["here_votes_off"] / med["other_post"]
            k.update(outputs_bit_identical_to_other_lib=True, other_spread=sp, median_ratio_votes_off_over_other=ratio,
                     within_other_spread=bool(abs(ratio - 1.0) <= sp))
            print("rows %d (a / b) votes off here / the other library: %.4f (the other's own spread %.4f) -> %s"
                  % (N, ratio, sp, "within" if k["within_other_spread"] else "OUTSIDE"))
        print("rows %d (c) post %.2f us, post + votes %.2f us: the vote kernel %.2f us, %.1f %% of the HBM peak (the post kernel %.1f %%)"
              % (N, med["here_votes_off"], med["here_votes_on"], vote_us, 100 * (k["vote_kernel_share_of_hbm_peak"] or 0.0),
                 100 * k["post_kernel_share_of_hbm_peak"]))
        rows[str(N)] = k
    res["kernel"] = rows

if args.rollout:
    import test_rule_votes_gpu as tv
    T = 8
    rows = {}
    for B in (1000, 100000):
        w = tv._world(21, 512)
        start = tv._start(22, B)
        worlds = {"votes_off": tv._hip_world(w, B, T), "votes_on": tv._hip_world(w, B, T, static_votes=True)}
        steps_taken = {k: [] for k in worlds}

        def phase(name):
            sampler, pool, _ = worlds[name]

            def run():
                sampler.reset(start)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                steps = 0
                while sampler.any_alive() and pool.has_room:
                    steps += sampler.sample_many()[0]
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                steps_taken[name].append((steps, pool.n_alive))
                sampler.finish_all_paths()
                pool.get(as_tensors=True)
                return dt * 1e6 / steps
            return run
        fns = {k: phase(k) for k in worlds}
        for fn in fns.values():
            for _ in range(3):
                fn()
        us = alternate(fns, args.pairs)
        assert steps_taken["votes_off"] == steps_taken["votes_on"], steps_taken      # round by round the same steps, the same survivors
        rows[str(B)] = dict(B=B, steps_per_phase=steps_taken["votes_on"][0][0], alive_at_the_end=steps_taken["votes_on"][0][1],
                            us_per_step=us, median_us={n: statistics.median(v) for n, v in us.items()},
                            spread={n: spread(v) for n, v in us.items()},
                            on_over_off=statistics.median(us["votes_on"]) / statistics.median(us["votes_off"]))
        print("B %d: a rollout step %.1f us with the votes, %.1f us without: x %.4f" % (
            B, rows[str(B)]["median_us"]["votes_on"], rows[str(B)]["median_us"]["votes_off"], rows[str(B)]["on_over_off"]))
    res["rollout"] = rows

if args.out:
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
