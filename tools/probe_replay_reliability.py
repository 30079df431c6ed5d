"""What the reliability table adds to the open-loop replay of real trajectories, and what the recalibrated hazard does to the
imagined termination rate.  The settings of tools/probe_replay_calibration.py -- AntSafe dims (29 / 8), 7 members of
512 hidden units with a logistic cost and a logistic termination column, WINDOWS windows x HORIZON teacher-forced steps, HIP events
around REPS back-to-back replays, after warm-up; the forms alternate in one process, the first two timed rounds are dropped.
  run_cost     cmbpo_replay_run_cost:    H x (forward -> post -> compare), finish
  run_reliab   cmbpo_replay_run_reliab:  H x (forward -> post -> reliab -> compare), both finishes -- both columns, 15 bins
The recording never ends a window, so that both forms do the same work on every step.  Reported: the medians, the scatter of the
repeated rounds ((max - min) / median), the added time per replay and per horizon step.  The plain tables of the two forms must be
the same bit for bit.  No kernel trace is taken: the added time is kernel plus launch gap, not separated.
--cost-only times run_cost alone and touches nothing this feature added: the same file runs in a checkout of the commit before it.
--trainer: the two-epoch box point mass of tests/test_term_draws_gpu.py, seeds 0 / 1 / 2, with m_validate_reliability and with /
without m_recalibrate_term: the termination column's ECE at h = 1 and the per-step termination rate of imagined rollouts from
archived real states against the real rate of the last fit's samples.
    python tools/probe_replay_reliability.py [out.json] [--cost-only] [--trainer] [--windows N] [--horizon H] [--pairs K] [--reps R]"""
import argparse
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
from cmbpo_amd import synthetic
from cmbpo_amd.fake_env import FakeEnv
from cmbpo_amd.pens import PE
from cmbpo_amd.replay import ReplayBuffers

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--cost-only", action="store_true")
ap.add_argument("--trainer", action="store_true")
ap.add_argument("--windows", type=int, default=4096)
ap.add_argument("--horizon", type=int, default=10)
ap.add_argument("--pairs", type=int, default=8)
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()

TASK, E, HID, WARM, DROP = "AntSafe-v2", 7, 512, 10, 2
D, A = synthetic.ENV_DIMS[TASK]
O = D + 3
B, H = args.windows, args.horizon
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
res = dict(command="python tools/probe_replay_reliability.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0))


class _Space:
    def __init__(self, d):
        self.shape = (d,)


class _Env:
    observation_space, action_space = _Space(D), _Space(A)


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


if not args.trainer:
    ws, bs = synthetic.ensemble_weights(rng, E, D + A, HID, 2 * O, bias_scale=0.05)
    model = PE(D + A, O, hidden_dims=(HID, HID), num_networks=E, num_elites=5, loss="MSPE", use_scaler_in=True, use_scaler_out=True,
               device=dev)
    mu, var = np.zeros((1, O), np.float32), np.full((1, O), 2.5e-3, np.float32)
    mu[0, D + 1], var[0, D + 1], mu[0, O - 1], var[0, O - 1] = -0.3, 16.0, -1.0, 16.0
    model.set_weights(ws, bs, synthetic.scaler(rng, D + A), (mu, var))
    env = FakeEnv(_Env(), TASK, model, True, True, True, cost_loss="logistic", cost_logit_shift=0.2, predicts_term=True,
                  term_threshold=0.9, term_members="elite", term_loss="logistic")
    obs0 = synthetic.start_states(rng, B, TASK)
    nxt = (obs0[None] + np.cumsum(rng.standard_normal((H, B, D)) * 0.05, axis=0)).astype(np.float32)
    act = rng.uniform(-1, 1, (H, B, A)).astype(np.float32)
    rew, cost = rng.standard_normal((H, B)).astype(np.float32), (rng.random((H, B)) < 0.3).astype(np.float32)
    term = np.zeros((H, B), np.uint8)
    inds = torch.from_numpy(rng.integers(0, E, (H, B)).astype(np.int32)).to(dev)
    kw = dict(mode="one_step", ensemble=E, out_dim=O, device=dev)
    th, ch = env.term_head_struct(), env.cost_head_struct()
    plain = ReplayBuffers(obs0, act, nxt, rew, cost, term, **kw)
    bufs = {"run_cost": plain}
    if not args.cost_only:
        bufs["run_reliab"] = ReplayBuffers(obs0, act, nxt, rew, cost, term, reliability=dict(columns=env.reliability_columns(), bins=15), **kw)
    start = plain.t["cur_obs"].clone()

    def form(rb):
        def run():
            rb.t["cur_obs"].copy_(start)
            rb.t["alive"].fill_(1)
            rb.run(model.mlp.handle, env._task_id, E, inds, term_head=th, cost_head=ch)
        return run

    forms = {n: form(rb) for n, rb in bufs.items()}

    def measure(fn):
        """Microseconds per replay over args.reps back-to-back replays."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.reps

    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    if not args.cost_only:
        a, b = bufs["run_cost"], bufs["run_reliab"]
        assert torch.equal(a.t["sums"].view(torch.int64), b.t["sums"].view(torch.int64)) and torch.equal(a.t["counts"], b.t["counts"])
        rel = b.reliability_table()
        assert all((c["n_rel"] + c["n_skipped"] == a.table()["n"]).all() for c in rel.values())
        res.update(plain_tables_bit_identical=True, n_rel_per_horizon={k: c["n_rel"].tolist() for k, c in rel.items()},
                   ece_h1={k: float(c["elite"]["ece"][0]) for k, c in rel.items()})
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
    res.update(task=TASK, windows=B, horizon=H, ensemble=E, hidden=HID, reps=args.reps, pairs=args.pairs, warmups=WARM, dropped_rounds=DROP,
               us_per_replay=us, median_us=med, spread={k: spread(v) for k, v in us.items()}, kernel_trace_taken=False)
    print("replay of %d windows x %d steps: run_cost %.1f us (scatter %.4f)" % (B, H, med["run_cost"], res["spread"]["run_cost"]))
    if not args.cost_only:
        added = med["run_reliab"] - med["run_cost"]
        res.update(added_us_per_replay=added, added_us_per_horizon_step=added / H, added_share_of_run_cost=added / med["run_cost"])
        print("run_reliab %.1f us (scatter %.4f); the table of both columns adds %.1f us = %.2f us per horizon step (%.1f %% of run_cost)"
              % (med["run_reliab"], res["spread"]["run_reliab"], added, added / H, 100 * added / med["run_cost"]))

if args.trainer:
    import test_term_draws_gpu as tt

    def rate(algo):
        """ended branches / branch-steps of one imagined rollout from archived real states, the horizon's step left out"""
        algo.model_sampler._draws = None
        ended = stepped = 0
        for st in tt.imagined_rollout(algo)[:-1]:
            ended += int((~st["alive"][st["ids"]]).sum())
            stepped += len(st["ids"])
        return ended / max(stepped, 1), stepped

    runs = []
    for seed in (0, 1, 2):
        for recal in (False, True):
            t0 = time.perf_counter()
            keys = dict(m_term_sampling=True, m_validate_reliability=True, **({"m_recalibrate_term": True} if recal else {}))
            algo, seen, diags = tt.run_box_loop(keys, seed=seed)
            imagined, n = rate(algo)
            last = diags[-1]
            runs.append(dict(seed=seed, m_recalibrate_term=recal, real_rate_last_fit=seen["term_share"][-1], imagined_rate=imagined,
                             branch_steps=n, ece_term_h1=float(last["model/val_ece_term_h1"]),
                             mean_p_term_h1=float(last["model/val_mean_p_term_h1"]), base_rate_term_h1=float(last["model/val_base_rate_term_h1"]),
                             term_recal_offset=float(last.get("model/term_recal_offset", 0.0)), seconds=time.perf_counter() - t0))
            print(runs[-1])
    res["trainer"] = runs

print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
