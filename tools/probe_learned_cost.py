"""What the learned cost head costs in a rollout phase: bench.py's headline phase (AntSafe shapes, B branches,
maxroll 35: 34 stored steps) with the 60-wide model and the task's cost rule, against the same phase with a 62-wide model and
FakeEnv(predicts_cost=True).  The wide world IS the narrow one with a cost column inserted (mean and log-variance), so the
dynamics, the terminations and therefore the rows of every step are the same in both; the phases alternate, medians over
ROUNDS rounds after WARM warm-ups, in one process.
    python tools/probe_learned_cost.py [out.json] [B] [rounds] [off|on|both]
`off` / `on` run one of the two only: the target of a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/... on)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from cmbpo_amd import synthetic
from cmbpo_amd.cpo_policy import CPOPolicy
from cmbpo_amd.fake_env import FakeEnv
from cmbpo_amd.model_sampler import ModelSampler
from cmbpo_amd.modelbuffer import ModelBuffer
from cmbpo_amd.pens import PE

TASK, WARM = "AntSafe-v2", 2
out_path = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "-" else None
B = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 7
which = sys.argv[4] if len(sys.argv) > 4 else "both"
dev = torch.device("cuda:0")


def with_cost_column(w, seed=1):
    """The world of bench.build_world with one more output: column D + 1 of the mean half and of the log-variance half."""
    rng = np.random.default_rng(seed)
    D = w["obs_dim"]

    def widen(a, fill):      # [..., 2 (D + 1)] -> [..., 2 (D + 2)]
        return np.concatenate([a[..., :D + 1], fill(a[..., :1].shape), a[..., D + 1:], fill(a[..., :1].shape)], -1).astype(np.float32)

    ws, bs = list(w["ws"]), list(w["bs"])
    std = float(w["ws"][2].std())
    ws[2] = widen(ws[2], lambda s: rng.standard_normal(s) * std)
    bs[2] = widen(bs[2], lambda s: np.zeros(s))
    mu, var = w["sc_out"]
    sc_out = (np.concatenate([mu, [[0.3]]], -1).astype(np.float32), np.concatenate([var, [[0.25]]], -1).astype(np.float32))
    return dict(w, ws=ws, bs=bs, sc_out=sc_out)


def build(w, learned):
    D, A = w["obs_dim"], w["act_dim"]
    model = PE(D + A, D + 1 + int(learned), hidden_dims=(512, 512), num_networks=7, num_elites=5, loss="MSPE",
               use_scaler_in=True, use_scaler_out=True, device=dev)
    model.set_weights(w["ws"], w["bs"], w["sc_in"], w["sc_out"])
    model.set_elites(w["elites"])
    policy = CPOPolicy(bench._Space(D), bench._Space(A), a_hidden_layer_sizes=(128, 128), vf_hidden_layer_sizes=(128, 128),
                       vf_ensemble_size=3, vf_elites=2, vf_activation="swish", vf_loss="MSE", device=dev, cost_gamma=0.97,
                       cost_lam=0.5, lam=0.95, max_path_length=bench.MAXROLL)
    policy.actor.set_params(w["pol"])
    policy.v.set_weights(*w["v"])
    policy.vc.set_weights(*w["vc"])

    class _Env:
        observation_space, action_space = bench._Space(D), bench._Space(A)

    env = FakeEnv(_Env(), TASK, model, True, True, learned)
    pool = ModelBuffer(B, D, A, bench.MAXROLL, device=dev)
    pool.initialize(policy.pi_info_shapes, gamma=0.99, lam=0.95, cost_gamma=0.97, cost_lam=0.5)
    sampler = ModelSampler(max_path_length=bench.MAXROLL, batch_size=B, rollout_mode="schedule")
    sampler.initialize(env, policy, pool)
    return sampler, pool


w0 = bench.build_world(0, TASK)
worlds = {"off": (w0, False), "on": (with_cost_column(w0), True)}
if which != "both":
    worlds = {which: worlds[which]}
runs = {k: build(w, learned) for k, (w, learned) in worlds.items()}
start = torch.from_numpy(synthetic.start_states(np.random.default_rng(1), B, TASK)).to(dev)
ms = {k: [] for k in runs}
samples, cost_std = {}, {}
for r in range(WARM + ROUNDS):
    for k, (sampler, pool) in runs.items():       # alternating
        sampler._gen.manual_seed(11)              # the same draws in every phase of either mode
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n, res = bench.rollout_phase(sampler, pool, start)
        torch.cuda.synchronize()
        if r >= WARM:
            ms[k].append((time.perf_counter() - t0) * 1e3)
        samples[k], cost_std[k] = n, float(res[9].std())
out = dict(task=TASK, branches=B, maxroll=bench.MAXROLL, rounds=ROUNDS, warmups=WARM)
for k in runs:
    med = statistics.median(ms[k])
    out[k] = dict(out_dim=w0["obs_dim"] + (2 if k == "on" else 1), phase_ms=ms[k], median_ms=med, samples=samples[k],
                  steps_per_s=samples[k] / (med * 1e-3), cost_std=cost_std[k])
    print(f"{k}: median {med:.2f} ms over {ROUNDS} phases, {samples[k]} samples, {samples[k] / med / 1e3:.2f} M steps/s, "
          f"std(cost) {cost_std[k]:.3f}", flush=True)
if len(runs) == 2:
    out["on_over_off"] = out["on"]["median_ms"] / out["off"]["median_ms"]
    print("on / off = %.4f" % out["on_over_off"])
print(json.dumps(out))
if out_path:
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
