"""What the learned termination head costs, and how good it is after a short run.  AntSafe dims (29 / 8), E = 7.
  --kernel   cmbpo_fakeenv_post alone at ROWS rows, HIP events around REPS back-to-back launches, alternating pairs, by the method
             of tools/probe_task_rules.py:
             (a) with --other-lib PATH (the parent commit's libcmbpo_hip.so): TASK_ANTSAFE there against TASK_ANTSAFE here -- a
                 launch without the head must not pay for it; the yardstick is the other library's own (max - min) / median;
             (b) here: the same launch with the head (cmbpo_fakeenv_post_term, one more column in the row stride) against it.
  --rollout  a whole rollout phase (reset + the native loop over T steps, B branches, 512-wide model with the cost head) with
             the termination column (64 raw outputs, a threshold nothing exceeds: the same branches live) against without (62).
  --trainer  recall and false-alarm rate of the head at h = 1 after two epochs on the box point mass of
             tests/test_term_head_cmbpo_gpu.py, seeds 0 / 1 / 2, beside the head-off run.
    python tools/probe_term_head.py [out.json] [--kernel] [--rollout] [--trainer] [--other-lib PATH]"""
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

TASK, E, WARM, DROP = "AntSafe-v2", 7, 300, 2
D, A = synthetic.ENV_DIMS[TASK]
dev = torch.device("cuda:0")
res = dict(command="python tools/probe_term_head.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0))


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
    N = args.rows
    rng = np.random.default_rng(0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    obs = t(synthetic.start_states(rng, N, TASK))
    act = t(rng.uniform(-1, 1, (N, A)).astype(np.float32))
    wide_mean = (rng.standard_normal((E, N, D + 2)) * 0.3).astype(np.float32)
    wide_var = np.exp(rng.uniform(-12, 1, (E, N, D + 2))).astype(np.float32)
    wide_mean[:, :, D + 1] = 0.35 + 0.3 * rng.standard_normal(N)[None] + 0.15 * rng.standard_normal((E, N))
    mean, var = t(wide_mean[..., :D + 1]), t(wide_var[..., :D + 1])
    wmean, wvar = t(wide_mean), t(wide_var)
    inds = t(rng.integers(0, E, size=N).astype(np.int32))
    f = dict(dtype=torch.float32, device=dev)
    out = dict(next_obs=torch.empty((N, D), **f), rew=torch.empty(N, **f), term=torch.empty(N, dtype=torch.uint8, device=dev),
               cost=torch.empty(N, **f), dkl_path=torch.empty(N, **f), ep_var_mean=torch.empty(N, **f))
    pred, votes = torch.empty(N, **f), torch.empty(N, dtype=torch.uint8, device=dev)
    here = _lib.lib()
    th = _lib.TermHeadStruct()
    th.threshold, th.members, th.term_pred, th.term_votes = 0.5, _lib.TERM_MAJORITY, _lib.ptr(pred), _lib.ptr(votes)
    tail = lambda: (_lib.ptr(out["next_obs"]), _lib.ptr(out["rew"]), _lib.ptr(out["term"]), _lib.ptr(out["cost"]),
                    _lib.ptr(out["dkl_path"]), _lib.ptr(out["ep_var_mean"]), None)

    def plain(lib):
        rc = lib.cmbpo_fakeenv_post(_lib.TASK_ANTSAFE, E, D, A, _lib.ptr(mean), _lib.ptr(var), N, _lib.ptr(obs), _lib.ptr(act),
                                    _lib.ptr(inds), None, None, N, *tail(), _lib.current_stream())
        assert rc == 0, lib.cmbpo_last_error()

    def with_head(lib):
        rc = lib.cmbpo_fakeenv_post_term(_lib.TASK_ANTSAFE, E, D, A, _lib.ptr(wmean), _lib.ptr(wvar), N, _lib.ptr(obs), _lib.ptr(act),
                                         _lib.ptr(inds), None, None, N, *tail(), None, 0.0, 0.0, None, None, C.byref(th),
                                         _lib.current_stream())
        assert rc == 0, lib.cmbpo_last_error()

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

    fns = {"here_antsafe": timed(plain, here), "here_antsafe_head": timed(with_head, here)}
    if args.other_lib:
        other = C.CDLL(os.path.abspath(args.other_lib))
        other.cmbpo_fakeenv_post.restype, other.cmbpo_fakeenv_post.argtypes = _lib.SIGNATURES["cmbpo_fakeenv_post"]
        other.cmbpo_last_error.restype = C.c_char_p
        plain(other)
        torch.cuda.synchronize()
        theirs = {k: v.clone() for k, v in out.items()}
        plain(here)
        torch.cuda.synchronize()
        for k, v in out.items():
            assert torch.equal(v.view(torch.int32) if v.dtype == torch.float32 else v,
                               theirs[k].view(torch.int32) if v.dtype == torch.float32 else theirs[k]), k
        fns = {"other_antsafe": timed(plain, other), **fns}
    for fn in fns.values():
        for _ in range(2):
            fn()
    us = alternate(fns, args.pairs)
    k = dict(rows=N, reps=args.reps, pairs=args.pairs, dropped_rounds=DROP, us_per_launch=us,
             head_over_plain=statistics.median(us["here_antsafe_head"]) / statistics.median(us["here_antsafe"]),
             here_spread=spread(us["here_antsafe"]), term_rate_with_head=float(out["term"].float().mean()))
    if args.other_lib:
        sp = spread(us["other_antsafe"])
        ratio = statistics.median(us["here_antsafe"]) / statistics.median(us["other_antsafe"])
        k.update(outputs_bit_identical_to_other_lib=True, other_spread=sp, median_ratio_here_over_other=ratio,
                 within_other_spread=bool(abs(ratio - 1.0) <= sp))
        print("(a) TASK_ANTSAFE here / other: %.4f (other's own spread %.4f) -> %s" % (ratio, sp, "within" if k["within_other_spread"] else "OUTSIDE"))
    print("(b) with the head / without, here: %.4f" % k["head_over_plain"])
    res["kernel"] = k

if args.rollout:
    from test_term_head_gpu import NEVER, _Env, _Space
    from cmbpo_amd.cpo_policy import CPOPolicy
    from cmbpo_amd.fake_env import FakeEnv
    from cmbpo_amd.model_sampler import ModelSampler
    from cmbpo_amd.modelbuffer import ModelBuffer
    from cmbpo_amd.pens import PE
    B, T, H = 10000, 8, 512

    def world(term):
        rng = np.random.default_rng(11)
        O = D + 2 + int(term)
        ws, bs = synthetic.ensemble_weights(rng, E, D + A, H, 2 * O, bias_scale=0.05)
        sc_in = synthetic.scaler(rng, D + A, hit_clamp=False)
        mu, var = synthetic.scaler(rng, O, hit_clamp=False)
        model = PE(D + A, O, hidden_dims=(H, H), num_networks=E, num_elites=5, loss="MSPE", use_scaler_in=True, use_scaler_out=True,
                   device="cuda:0")
        model.set_weights(ws, bs, sc_in, (mu, (var * 0.01).astype(np.float32)))
        policy = CPOPolicy(_Space(D), _Space(A), a_hidden_layer_sizes=(128, 128), vf_hidden_layer_sizes=(128, 128),
                           vf_ensemble_size=3, vf_elites=2, vf_activation="swish", vf_loss="MSE", device="cuda:0")
        policy.actor.set_params(synthetic.policy_params(rng, D, A))
        prng = np.random.RandomState(3)
        policy.v.init_weights(prng)
        policy.vc.init_weights(prng)
        kw = dict(predicts_term=True, term_threshold=NEVER, term_members="majority") if term else {}
        env = FakeEnv(_Env(D, A), "default", model, predicts_delta=True, predicts_rew=True, predicts_cost=True, **kw)
        pool = ModelBuffer(B, D, A, T, device="cuda:0")
        pool.initialize(policy.pi_info_shapes)
        sampler = ModelSampler(max_path_length=T, batch_size=B, rollout_mode="schedule")
        sampler.initialize(env, policy, pool)
        return sampler, pool

    start = synthetic.start_states(np.random.default_rng(12), B, TASK)
    worlds = {"raw62": world(False), "raw64_head": world(True)}

    steps_taken = []

    def phase(name):
        sampler, pool = worlds[name]

        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sampler.reset(start)
            while sampler.any_alive() and pool.has_room:
                sampler.sample_many()
            sampler.finish_all_paths()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            steps_taken.append(pool.ptr)
            pool.get(as_tensors=True)
            return dt * 1e3
        return run
    fns = {k: phase(k) for k in worlds}
    for fn in fns.values():
        for _ in range(3):
            fn()
    ms = alternate(fns, args.pairs)
    assert len(set(steps_taken)) == 1, steps_taken       # the same number of steps in every phase of both worlds
    r = dict(B=B, T=T, steps_per_phase=steps_taken[0], hidden=H, ms_per_phase=ms, spread_raw62=spread(ms["raw62"]),
             head_over_plain=statistics.median(ms["raw64_head"]) / statistics.median(ms["raw62"]))
    print("rollout phase with the termination column / without: %.4f (%.2f ms / %.2f ms)"
          % (r["head_over_plain"], statistics.median(ms["raw64_head"]), statistics.median(ms["raw62"])))
    res["rollout"] = r

if args.trainer:
    from test_term_head_cmbpo_gpu import head_figures, run_box_loop
    runs = []
    for learn, seed in ((False, 0), (True, 0), (True, 1), (True, 2)):
        t0 = time.perf_counter()
        algo, seen, diags = run_box_loop(learn, seed=seed)
        recall, false_alarm, pos, neg = head_figures(algo)
        runs.append(dict(m_learn_term=learn, seed=seed, recall_h1=float(recall), false_alarm_h1=float(false_alarm), real_terminations=pos,
                         real_continuations=neg, target_share=seen["term_share"][-1] if learn else None, seconds=time.perf_counter() - t0))
        print(runs[-1])
    res["trainer"] = runs

print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
