"""Generate golden G14: imagined-rollout traces with a learned cost head, recorded from the REFERENCE's own
FakeEnv(predicts_cost=True) + ModelSampler + ModelBuffer (models/fake_env.py:139-151: the cost of a branch is the elite
member's mean of the model's last output column; the task's termination rule still applies, its cost rule does not).

Usage (build container only, like make_golden.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_learned_cost.py

Writes tests/golden/g14_trace_cost_*.npz (data only), with the keys of the G5 traces (make_golden.run_sampler_trace).  The
worlds come from worlds_learned_cost.build_world_learned_cost: 2 (obs + 2) raw outputs, the cost column's scaler variance
left large so that the predicted costs spread over about a unit.  Asserted before a file is written: it is no larger than
the largest committed fixture, std(get_cost) >= 0.5, and the AntSafe trace without an uncertainty limit
contains static terminations.
"""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (the stubs behind which the reference imports; puts the reference on sys.path)
from worlds_learned_cost import build_world_learned_cost  # noqa: E402

MAX_BYTES = 520 * 1024        # the largest committed fixture
MIN_COST_STD = 0.5

TRACES = {
    # no statics entry at all (Hopper): never terminates; tight budget
    "g14_trace_cost_hopper_budget": dict(seed=9, task="HopperSafe-v2", B=50, T=15, hidden=128, dkl_lim=float("inf"),
                                         budget=333, mode="uncertainty"),
    # the AntSafe termination rule fires over several steps while its cost rule is not used
    "g14_trace_cost_ant_term": dict(seed=7, task="AntSafe-v2", B=96, T=8, hidden=128, dkl_lim=float("inf"),
                                    budget=None, mode="uncertainty", q_boost=0.8),
    # fixed horizon ('schedule'), no budget
    "g14_trace_cost_hcs_sched": dict(seed=8, task="HalfCheetahSafe-v2", B=64, T=9, hidden=128, dkl_lim=float("inf"),
                                     budget=None, mode="schedule"),
    # calibrated uncertainty limit (make_golden's widest-gap procedure): uncertainty deaths bootstrap the learned cost
    "g14_trace_cost_ant_unc": dict(seed=7, task="AntSafe-v2", B=96, T=12, hidden=128, dkl_lim=None, budget=None,
                                   mode="uncertainty", q_boost=0.8),
}


def run_sampler_trace(seed, task, B, T, hidden, dkl_lim, budget, mode, out_scale=1.0, q_boost=0.0, max_steps=100):
    """make_golden.run_sampler_trace on a world with a cost column and FakeEnv(..., predicts_cost=True)."""
    from buffers.modelbuffer import ModelBuffer
    from models.fake_env import FakeEnv
    from samplers.model_sampler import ModelSampler
    from cmbpo_amd import synthetic
    w = build_world_learned_cost(seed, task, hidden, out_scale=out_scale, q_boost=q_boost)
    rng = np.random.default_rng(seed + 1)
    model = mg.OracleModel(w["ws"], w["bs"], w["sc_in"], w["sc_out"], w["elites"])
    assert model.out_dim == w["obs_dim"] + 2
    policy = mg.OraclePolicy(w["pol"], w["v"], w["vc"], rng)
    env = FakeEnv(mg._TrueEnv(w["obs_dim"], w["act_dim"]), task, model, True, True, True)
    inds_log = []
    orig = env.random_inds

    def rec(size):
        r = orig(size)
        inds_log.append(np.asarray(r, dtype=np.int32))
        return r

    env.random_inds = rec
    buf = ModelBuffer(batch_size=B, obs_dim=w["obs_dim"], act_dim=w["act_dim"], max_path_length=T)
    buf.initialize({"mu": [w["act_dim"]], "log_std": [w["act_dim"]]}, gamma=0.99, lam=0.95,
                   cost_gamma=0.97, cost_lam=0.5)
    sampler = ModelSampler(max_path_length=T, batch_size=B, rollout_mode=mode, logger=object())
    sampler.initialize(env, policy, buf)
    sampler.set_rollout_dkl(dkl_lim)
    start = synthetic.start_states(rng, B, task)
    np.random.seed(seed)
    sampler.reset(start)
    alive_log, tot_log, ratio_log = [], [], []
    with np.errstate(all="ignore"):
        for _ in range(max_steps):
            _, _, _, info = sampler.sample(max_samples=budget)
            alive_log.append(buf.alive_paths.copy())
            tot_log.append(sampler._total_samples)
            ratio_log.append(info["alive_ratio"])
            if budget and sampler._total_samples >= .99 * budget:
                break
            if info["alive_ratio"] <= 0.1:
                break
        dkl_acc = np.array(sampler._dyn_dkl_path, dtype=np.float64)
        diag = sampler.finish_all_paths()
        res, bdiag = buf.get()
    nsteps = len(alive_log)
    eps_pad = np.zeros((nsteps, B, w["act_dim"]), np.float32)
    inds_pad = np.zeros((nsteps, B), np.int32)
    n_rows = np.zeros(nsteps, np.int32)
    for s in range(nsteps):
        k = policy.eps_log[s].shape[0]
        n_rows[s] = k
        eps_pad[s, :k] = policy.eps_log[s]
        inds_pad[s, :k] = inds_log[s]
    names = ["obs", "act", "adv", "cadv", "ret", "cret", "logp", "val", "cval", "cost", "log_std", "mu"]
    data = dict(seed=seed, task=task, B=B, T=T, hidden=hidden, dkl_lim=dkl_lim, budget=budget or 0, mode=mode,
                out_scale=out_scale, q_boost=q_boost, start=start, eps=eps_pad, inds=inds_pad, n_rows=n_rows,
                alive=np.array(alive_log), total_samples=np.array(tot_log, dtype=np.float64),
                alive_ratio=np.array(ratio_log, dtype=np.float64),
                dkl_acc=dkl_acc, poolm_batch_size=bdiag["poolm_batch_size"], poolm_ret_mean=bdiag["poolm_ret_mean"],
                poolm_cret_mean=bdiag["poolm_cret_mean"])
    for k, v in zip(names, res):
        data["get_" + k] = v
    for k, v in diag.items():
        data["diag_" + k.replace("/", "__")] = np.float64(v)
    return data


def gen_learned_cost_traces(out):
    for name, cfg in TRACES.items():
        cfg = dict(cfg)
        if cfg["dkl_lim"] is None:
            # make_golden.gen_sampler_traces: the widest gap of the accumulated DKL near its median after 4 steps
            probe = run_sampler_trace(**{**cfg, "dkl_lim": float("inf"), "budget": None, "max_steps": 4})
            acc = np.sort(probe["dkl_acc"])
            lo, hi = int(.35 * len(acc)), int(.65 * len(acc))
            k = lo + int(np.argmax(acc[lo + 1:hi + 1] - acc[lo:hi]))
            cfg["dkl_lim"] = float(0.5 * (acc[k] + acc[k + 1]))
        data = run_sampler_trace(**cfg)
        cost = data["get_cost"]
        spread = float(np.std(cost))
        assert cost.dtype == np.float32 and spread >= MIN_COST_STD, (name, cost.dtype, spread)
        if cfg["task"] == "AntSafe-v2" and cfg["dkl_lim"] == float("inf") and not cfg["budget"]:
            # nothing but the static termination rule can shrink the alive list here
            assert (np.diff(data["n_rows"]) < 0).any(), (name, data["n_rows"])
        blob = io.BytesIO()
        np.savez_compressed(blob, **data)
        assert blob.getbuffer().nbytes <= MAX_BYTES, (name, blob.getbuffer().nbytes)
        with open(os.path.join(out, name + ".npz"), "wb") as f:
            f.write(blob.getvalue())
        print(name, "steps", len(data["n_rows"]), "rows/step", data["n_rows"].tolist(), "samples",
              int(data["poolm_batch_size"]), "std(cost) %.3f" % spread, "bytes", blob.getbuffer().nbytes)


if __name__ == "__main__":
    mg.install_stubs()
    gen_learned_cost_traces(HERE)
