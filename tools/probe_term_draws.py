"""What sampled terminations cost, and what they do to the imagined termination rate.
  --kernel   the post kernel alone at ROWS rows (AntSafe dims 29 / 8, E = 7, termination head on), HIP events around REPS
             back-to-back launches, alternating rounds, by the method of tools/probe_term_head.py -- three cases:
             (a) with --other-lib PATH (the parent commit's libcmbpo_hip.so): cmbpo_fakeenv_post_term there;
             (b) here with the draws off: cmbpo_fakeenv_post_term_draws, d_term_thr == NULL (the same instances: it must sit
                 inside the other library's own (max - min) / median);
             (c) here with the draws on: one 4-byte load per row beside 7 x 120-byte member rows.
  --rollout  a rollout step at B = 1000 and B = 100 000 (512-wide model, 8 steps of the native loop from a reset, per step) with
             ModelSampler(term_sampling=True) against False, on a termination column that never hits (logit -30: the smallest
             threshold is logit(2^-24) = -16.6), so the same branches live in both.
  --trainer  two epochs on the box point mass of tests/test_term_draws_gpu.py (m_term_loss='logistic', weight 1), seeds 0 / 1 / 2:
             the per-step termination rate of imagined rollouts from archived real states under the threshold rule and under
             sampling, each beside the real rate of the last fit's samples.
    python tools/probe_term_draws.py [out.json] [--kernel] [--rollout] [--trainer] [--other-lib PATH]"""
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
from cmbpo_amd import _lib, synthetic

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--kernel", action="store_true")
ap.add_argument("--rollout", action="store_true")
ap.add_argument("--trainer", action="store_true")
ap.add_argument("--other-lib")
ap.add_argument("--rows", type=int, default=100000)
ap.add_argument("--pairs", type=int, default=8)
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()

TASK, E, DROP = "AntSafe-v2", 7, 2
D, A = synthetic.ENV_DIMS[TASK]
dev = torch.device("cuda:0")
res = dict(command="python tools/probe_term_draws.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0))


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
    from cmbpo_amd.utils import term_thresholds
    N = args.rows
    rng = np.random.default_rng(0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    obs = t(synthetic.start_states(rng, N, TASK))
    act = t(rng.uniform(-1, 1, (N, A)).astype(np.float32))
    wide_mean = (rng.standard_normal((E, N, D + 2)) * 0.3).astype(np.float32)
    wide_var = np.exp(rng.uniform(-12, 1, (E, N, D + 2))).astype(np.float32)
    wide_mean[:, :, D + 1] = 0.35 + 0.3 * rng.standard_normal(N)[None] + 0.15 * rng.standard_normal((E, N))
    wmean, wvar = t(wide_mean), t(wide_var)
    inds = t(rng.integers(0, E, size=N).astype(np.int32))
    thr = t(term_thresholds(1.0 - rng.random(N, dtype=np.float32), "gaussian"))
    f = dict(dtype=torch.float32, device=dev)
    out = dict(next_obs=torch.empty((N, D), **f), rew=torch.empty(N, **f), term=torch.empty(N, dtype=torch.uint8, device=dev),
               cost=torch.empty(N, **f), dkl_path=torch.empty(N, **f), ep_var_mean=torch.empty(N, **f))
    pred, votes = torch.empty(N, **f), torch.empty(N, dtype=torch.uint8, device=dev)
    here = _lib.lib()
    th = _lib.TermHeadStruct()
    th.threshold, th.members, th.term_pred, th.term_votes = 0.5, _lib.TERM_MAJORITY, _lib.ptr(pred), _lib.ptr(votes)
    lead = lambda: (_lib.TASK_ANTSAFE, E, D, A, _lib.ptr(wmean), _lib.ptr(wvar), N, _lib.ptr(obs), _lib.ptr(act), _lib.ptr(inds), None,
                    None, N, _lib.ptr(out["next_obs"]), _lib.ptr(out["rew"]), _lib.ptr(out["term"]), _lib.ptr(out["cost"]),
                    _lib.ptr(out["dkl_path"]), _lib.ptr(out["ep_var_mean"]), None, None, 0.0, 0.0, None, None, C.byref(th))

    def parent_head(lib):
        rc = lib.cmbpo_fakeenv_post_term(*lead(), _lib.current_stream())
        assert rc == 0, lib.cmbpo_last_error()

    def draws(on):
        def call(lib):
            rc = lib.cmbpo_fakeenv_post_term_draws(*lead(), None, _lib.ptr(thr) if on else None, _lib.current_stream())
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

    fns = {"here_draws_off": timed(draws(False), here), "here_draws_on": timed(draws(True), here)}
    if args.other_lib:
        other = C.CDLL(os.path.abspath(args.other_lib))
        other.cmbpo_fakeenv_post_term.restype, other.cmbpo_fakeenv_post_term.argtypes = _lib.SIGNATURES["cmbpo_fakeenv_post_term"]
        other.cmbpo_last_error.restype = C.c_char_p
        parent_head(other)
        torch.cuda.synchronize()
        theirs = {k: v.clone() for k, v in dict(out, pred=pred, votes=votes).items()}
        draws(False)(here)
        torch.cuda.synchronize()
        for k, v in dict(out, pred=pred, votes=votes).items():
            assert torch.equal(v.view(torch.int32) if v.dtype == torch.float32 else v,
                               theirs[k].view(torch.int32) if v.dtype == torch.float32 else theirs[k]), k
        fns = {"other_head": timed(parent_head, other), **fns}
    for fn in fns.values():
        for _ in range(2):
            fn()
    us = alternate(fns, args.pairs)
    draws(True)(here)
    torch.cuda.synchronize()
    k = dict(rows=N, reps=args.reps, pairs=args.pairs, dropped_rounds=DROP, us_per_launch=us,
             median_us={n: statistics.median(v) for n, v in us.items()}, spread={n: spread(v) for n, v in us.items()},
             draws_on_over_off=statistics.median(us["here_draws_on"]) / statistics.median(us["here_draws_off"]),
             term_rate_with_draws=float(out["term"].float().mean()))
    if args.other_lib:
        sp = spread(us["other_head"])
        ratio = statistics.median(us["here_draws_off"]) / statistics.median(us["other_head"])
        k.update(outputs_bit_identical_to_other_lib=True, other_spread=sp, median_ratio_draws_off_over_other=ratio,
                 within_other_spread=bool(abs(ratio - 1.0) <= sp))
        print("(a / b) draws off here / the head in the other library: %.4f (the other's own spread %.4f) -> %s"
              % (ratio, sp, "within" if k["within_other_spread"] else "OUTSIDE"))
    print("(c) draws on / off, here: %.4f (%.2f us / %.2f us)" % (k["draws_on_over_off"], k["median_us"]["here_draws_on"],
                                                                   k["median_us"]["here_draws_off"]))
    res["kernel"] = k

if args.rollout:
    import test_term_draws_gpu as tt
    T = 8
    rows = {}
    for B in (1000, 100000):
        w = tt.build_world(11, 512, bias=-30.0, spread=0.0)
        start = tt._start(12, B)
        worlds = {"sampling_off": tt.hip_world(w, B, T, False, seed=3), "sampling_on": tt.hip_world(w, B, T, True, seed=3)}
        steps_taken = []

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
                steps_taken.append((steps, pool.n_alive))
                sampler.finish_all_paths()
                pool.get(as_tensors=True)
                return dt * 1e6 / steps
            return run
        fns = {k: phase(k) for k in worlds}
        for fn in fns.values():
            for _ in range(3):
                fn()
        us = alternate(fns, args.pairs)
        assert len(set(steps_taken)) == 1 and steps_taken[0][1] == B, steps_taken       # the same steps, nobody ended
        rows[str(B)] = dict(B=B, steps_per_phase=steps_taken[0][0], us_per_step=us,
                            median_us={n: statistics.median(v) for n, v in us.items()}, spread={n: spread(v) for n, v in us.items()},
                            on_over_off=statistics.median(us["sampling_on"]) / statistics.median(us["sampling_off"]))
        print("B = %d: a rollout step with sampling on / off: %.4f (%.1f us / %.1f us; spread off %.4f)"
              % (B, rows[str(B)]["on_over_off"], rows[str(B)]["median_us"]["sampling_on"], rows[str(B)]["median_us"]["sampling_off"],
                 rows[str(B)]["spread"]["sampling_off"]))
        del worlds, fns
        torch.cuda.empty_cache()
    res["rollout"] = rows

if args.trainer:
    import test_term_draws_gpu as tt

    def rate(algo, sampling):
        """ended branches / branch-steps of one imagined rollout from archived real states, the horizon's step left out"""
        algo.model_sampler.term_sampling = sampling
        algo.model_sampler._draws = None
        ended = stepped = 0
        for st in tt.imagined_rollout(algo)[:-1]:
            ended += int((~st["alive"][st["ids"]]).sum())
            stepped += len(st["ids"])
        return ended / max(stepped, 1), stepped

    runs = []
    for seed in (0, 1, 2):
        t0 = time.perf_counter()
        algo, seen, diags = tt.run_box_loop(dict(m_term_sampling=True), seed=seed)
        sampled, n_s = rate(algo, True)
        thresholded, n_t = rate(algo, False)
        algo.model_sampler.term_sampling = True
        runs.append(dict(seed=seed, real_rate_last_fit=seen["term_share"][-1], imagined_rate_sampling=sampled, branch_steps_sampling=n_s,
                         imagined_rate_threshold=thresholded, branch_steps_threshold=n_t,
                         recall_h1=float(diags[-1]['model/val_term_recall_h1']), seconds=time.perf_counter() - t0))
        print(runs[-1])
    res["trainer"] = runs

print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
