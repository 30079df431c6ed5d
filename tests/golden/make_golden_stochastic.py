"""Generate golden G16: stochastic model transitions, recorded from the REFERENCE's own FakeEnv.step called with
deterministic=False (models/fake_env.py:103-108: next_obs = pred_mean + pred_std, i.e. mean + std * xi at xi == 1; the
uncertainty measures of :112-113 run on the shifted means, reward and cost columns are read unshifted).

Usage (build container only, like make_golden.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stochastic.py

Writes data only, every file at most 520 KB:
  (a) g16_step_e{7,5,3}.npz -- single steps of FakeEnv.step(obs, act, deterministic=False) on a duck-typed model that
      returns given (mean, var) arrays: obs_dim in {3, 8, 21, 47}, 64 rows, variances spread over 1e-12 .. 10 with one
      zero and one 1e30, tasks AntSafe-v2 (obs_dim >= 5: the rule reads columns 0..4), HalfCheetahSafe-v2 and default on
      the same inputs; recorded: next_obs, r, terms, cost, dkl_path, ep_var and the elite indices.
  (b) g16_trace_{ant_term,ant_unc,hcs_sched}.npz -- sampler traces with the keys of the G5 traces
      (make_golden.run_sampler_trace) with every FakeEnv.step of the reference's ModelSampler forced to
      deterministic=False.

Asserted before a trace is written (a failing condition moves the search on to the next q_boost / seed): static
terminations on at least 2 steps of the first trace; uncertainty deaths in the second; a HalfCheetahSafe cost rate in
[0.1, 0.9]; every value a built-in rule tested (z against 0.2 and 1.0, gate * z_rot against -0.7, |y| against 3.2,
|x * 10| against 2) at least 1e-3 from its threshold; no accumulated DKL that the uncertainty test saw, on any step,
within the widest gap of the limit (the limit is the middle of the widest gap of the sums near their median after 4
steps; no sum may be closer to it than half that gap's width), nor closer to it than 5e-3 of the limit, the relative
tolerance the replays allow on the accumulated DKL; and at least one step on which the uncertainty test ends some but
not all of the rows it sees.  The replays evaluate the networks on three matrix paths whose results differ in the last
float32 bits; with these margins such differences cannot flip a mask.

Beside the keys of G5 a trace keeps what these conditions are computed from, so that the tests recompute them:
next_obs_log[step, row] (the next observations the rules tested, padded like eps), and for the limited trace
dkl_sum_log[step, row] (the sums the uncertainty test compared with the limit, NaN-padded) and probe_dkl_acc (the
sums of the calibrating probe).
"""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (the stubs behind which the reference imports; puts the reference on sys.path)

MAX_BYTES = 520 * 1024
MARGIN = 1e-3
DKL_REL_MARGIN = 5e-3            # the replays hold dkl_acc to rtol 5e-3 of the reference's
STEP_E = (7, 5, 3)
STEP_D = (3, 8, 21, 47)
STEP_ROWS = 64
STEP_TASKS = {"ant": "AntSafe-v2", "hcs": "HalfCheetahSafe-v2", "default": "default"}

TRACES = {
    # AntSafe terminations, no limit, no budget
    "g16_trace_ant_term": dict(seed=7, task="AntSafe-v2", B=96, T=8, hidden=128, dkl_lim=float("inf"), budget=None,
                               mode="uncertainty", q_boost=2.5),
    # calibrated uncertainty limit (make_golden's widest-gap procedure)
    "g16_trace_ant_unc": dict(seed=7, task="AntSafe-v2", B=96, T=12, hidden=128, dkl_lim=None, budget=None,
                              mode="uncertainty", q_boost=2.0),
    # fixed horizon ('schedule'), no budget, HalfCheetah cost rule
    "g16_trace_hcs_sched": dict(seed=8, task="HalfCheetahSafe-v2", B=64, T=9, hidden=128, dkl_lim=float("inf"),
                                budget=None, mode="schedule"),
}
Q_BOOSTS = (2.5, 2.0, 1.6, 1.2, 3.0)
SEED_STEPS = 12


class GivenModel:
    """Duck type of EnsembleModel whose predict_ensemble returns the arrays it was given."""
    is_ensemble, is_probabilistic = True, True

    def __init__(self, mean, var, in_dim, elites):
        self.mean, self.var = mean, var
        self.in_dim, self.out_dim = in_dim, mean.shape[-1]
        self.elite_inds = elites

    def predict_ensemble(self, x):
        assert x.shape == (self.mean.shape[1], self.in_dim)
        return self.mean.copy(), self.var.copy()


def gen_steps(out):
    from models.fake_env import FakeEnv
    for E in STEP_E:
        data = dict(E=E, rows=STEP_ROWS, dims=np.array(STEP_D))
        elites = list(range(E))[: max(1, E - 2)] if E < 7 else [0, 2, 3, 5, 6]
        data["elites"] = np.array(elites, np.int32)
        for D in STEP_D:
            rng = np.random.default_rng(1600 + 10 * E + D)
            A, n = max(1, D // 4), STEP_ROWS
            obs = rng.standard_normal((n, D)).astype(np.float32)
            act = rng.standard_normal((n, A)).astype(np.float32)
            mean = (0.3 * rng.standard_normal((E, n, D + 1))).astype(np.float32)
            var = (10.0 ** rng.uniform(-12, 1, (E, n, D + 1))).astype(np.float32)
            var[0, 0, 0], var[1, 1, 1] = 0.0, 1e30
            # observations that put the rules' columns around their thresholds: z, two quaternion columns, the last one
            obs[:, 0] = rng.uniform(-0.1, 1.3, n).astype(np.float32)
            if D >= 5:
                obs[:, 2:4] = (0.7 * rng.standard_normal((n, 2))).astype(np.float32)
            obs[:, -1] = (rng.uniform(-5, 5, n) * np.where(rng.random(n) < 0.4, 0.05, 1.0)).astype(np.float32)
            inds = np.asarray(elites, np.int32)[rng.integers(0, len(elites), n)]
            pre = f"d{D}_"
            data.update({pre + "obs": obs, pre + "act": act, pre + "mean": mean, pre + "var": var, pre + "inds": inds})
            for tag, task in STEP_TASKS.items():
                if task == "AntSafe-v2" and D < 5:
                    continue
                env = FakeEnv(mg._TrueEnv(D, A), task, GivenModel(mean, var, D + A, elites), True, True, False)
                env.random_inds = lambda size, inds=inds: inds
                with np.errstate(all="ignore"):
                    nxt, r, terms, info = env.step(obs.copy(), act.copy(), deterministic=False)
                assert nxt.dtype == np.float32 and r.dtype == np.float32 and terms.dtype == np.bool_
                data.update({pre + tag + "_next_obs": nxt, pre + tag + "_r": r, pre + tag + "_terms": terms,
                             pre + tag + "_cost": np.asarray(info["cost"]),
                             pre + tag + "_dkl_path": info["ensemble_dkl_path"],
                             pre + tag + "_ep_var": info["ensemble_ep_var"]})
                print("step E", E, "D", D, tag, "terms", int(terms.sum()), "cost sum", float(np.sum(info["cost"])))
        blob = io.BytesIO()
        np.savez_compressed(blob, **data)
        assert blob.getbuffer().nbytes <= MAX_BYTES, (E, blob.getbuffer().nbytes)
        with open(os.path.join(out, f"g16_step_e{E}.npz"), "wb") as f:
            f.write(blob.getvalue())
        print("g16_step_e%d" % E, "bytes", blob.getbuffer().nbytes)


def rule_margin(task, nxt):
    """Smallest distance of a value a built-in rule of `task` tests on these next observations from its threshold."""
    nxt = np.asarray(nxt, np.float32)
    if task == "AntSafe-v2":
        z = nxt[:, 0]
        zrot = 1 - 2 * (nxt[:, 2] ** 2 + nxt[:, 3] ** 2)
        gate = np.isfinite(nxt).all(axis=-1) * (z >= 0.2) * (z <= 1.0)
        vals = [np.abs(z - 0.2), np.abs(z - 1.0), np.abs(gate * zrot + 0.7), np.abs(np.abs(nxt[:, -1]) - 3.2)]
    elif task == "HalfCheetahSafe-v2":
        vals = [np.abs(np.abs(nxt[:, -1] * 10) - 2.0)]
    else:
        return float("inf")
    return float(min(v.min() for v in vals))


class Recorder:
    """Forces the reference's FakeEnv.step to deterministic=False and keeps what the margins are computed from."""

    def __init__(self):
        from models.fake_env import FakeEnv
        from samplers.model_sampler import ModelSampler
        self.FakeEnv, self.ModelSampler = FakeEnv, ModelSampler
        self.orig_step, self.orig_sample = FakeEnv.step, ModelSampler.sample
        rec = self

        def step(env, obs, act, deterministic=True):
            out = rec.orig_step(env, obs, act, deterministic=False)
            rec.rule.append(rule_margin(env._task, out[0]))
            rec.nxt.append(np.array(out[0], np.float32))
            rec.dkl_new = np.asarray(out[3]["ensemble_dkl_path"], np.float64)
            return out

        def sample(smp, max_samples=None):
            rec.dkl_before = np.array(smp._dyn_dkl_path[smp.pool.alive_paths], np.float64)
            out = rec.orig_sample(smp, max_samples=max_samples)
            if smp.rollout_mode == "uncertainty" and np.isfinite(smp.dkl_lim):
                rec.sums.append(rec.dkl_before + rec.dkl_new)                            # model_sampler.py:276-277
            return out

        FakeEnv.step, ModelSampler.sample = step, sample
        self.clear()

    def clear(self):
        self.rule, self.nxt, self.sums = [], [], []

    def close(self):
        self.FakeEnv.step, self.ModelSampler.sample = self.orig_step, self.orig_sample


def pad_log(per_step, B, dtype, fill):
    """[step, B, ...] from per-step arrays of the living rows, padded like run_sampler_trace pads eps."""
    out = np.full((len(per_step), B) + per_step[0].shape[1:], fill, dtype)
    for s, v in enumerate(per_step):
        out[s, :len(v)] = v
    return out


def try_trace(name, cfg, rec):
    """One candidate: the recorded trace, or the name of the condition it misses."""
    cfg = dict(cfg)
    half_gap = None
    if cfg["dkl_lim"] is None:
        # make_golden.gen_sampler_traces: the widest gap of the accumulated DKL near its median after 4 steps
        probe = mg.run_sampler_trace(**{**cfg, "dkl_lim": float("inf"), "budget": None, "max_steps": 4})
        acc = np.sort(probe["dkl_acc"])
        lo, hi = int(.35 * len(acc)), int(.65 * len(acc))
        k = lo + int(np.argmax(acc[lo + 1:hi + 1] - acc[lo:hi]))
        cfg["dkl_lim"] = float(0.5 * (acc[k] + acc[k + 1]))
        half_gap = float(0.5 * (acc[k + 1] - acc[k]))
    rec.clear()
    data = mg.run_sampler_trace(**cfg)
    n_rows = data["n_rows"]
    if not np.isfinite(data["get_obs"]).all():
        return "non-finite observations", cfg
    if min(rec.rule) < MARGIN:
        return "rule margin %.2e" % min(rec.rule), cfg
    if name == "g16_trace_ant_term" and int((np.diff(n_rows) < 0).sum()) < 2:
        return "static terminations on fewer than 2 steps %s" % n_rows.tolist(), cfg
    if name == "g16_trace_ant_unc":
        lim = cfg["dkl_lim"]
        deaths = [int((v >= lim).sum()) for v in rec.sums]
        if sum(deaths) == 0:
            return "no uncertainty deaths", cfg
        if not any(0 < d < len(v) for d, v in zip(deaths, rec.sums)):
            return "no step on which some but not all rows die of uncertainty %s of %s" % (deaths, n_rows.tolist()), cfg
        dist = min(float(np.abs(v - lim).min()) for v in rec.sums)
        if dist < max(half_gap, DKL_REL_MARGIN * lim):
            return "accumulated DKL %.3e from the limit %.3e, half gap %.3e" % (dist, lim, half_gap), cfg
        data["half_gap"], data["n_unc_deaths"], data["dkl_margin"] = half_gap, sum(deaths), np.float64(dist)
        data["probe_dkl_acc"] = probe["dkl_acc"]
        data["dkl_sum_log"] = pad_log(rec.sums, cfg["B"], np.float64, np.nan)
    if name == "g16_trace_hcs_sched":
        rate = float(data["diag_msampler__cost_rate"])
        if not 0.1 <= rate <= 0.9:
            return "cost rate %.3f" % rate, cfg
    data["rule_margin"] = np.float64(min(rec.rule))
    data.setdefault("dkl_margin", np.float64("inf"))
    data["next_obs_log"] = pad_log(rec.nxt, cfg["B"], np.float32, 0.0)
    assert [len(v) for v in rec.nxt] == n_rows.tolist()
    return data, cfg


def gen_traces(out):
    rec = Recorder()
    try:
        for name, base in TRACES.items():
            boosts = [base["q_boost"]] + [q for q in Q_BOOSTS if q != base["q_boost"]] if "q_boost" in base else [None]
            found = None
            for ds in range(SEED_STEPS):
                for q in boosts:
                    cfg = dict(base, seed=base["seed"] + 10 * ds)
                    if q is not None:
                        cfg["q_boost"] = q
                    data, cfg = try_trace(name, cfg, rec)
                    if isinstance(data, dict):
                        found = data
                        break
                    print(name, "seed", cfg["seed"], "q_boost", cfg.get("q_boost"), "rejected:", data)
                if found is not None:
                    break
            assert found is not None, name
            blob = io.BytesIO()
            np.savez_compressed(blob, **found)
            assert blob.getbuffer().nbytes <= MAX_BYTES, (name, blob.getbuffer().nbytes)
            with open(os.path.join(out, name + ".npz"), "wb") as f:
                f.write(blob.getvalue())
            print(name, "seed", int(found["seed"]), "q_boost", float(found["q_boost"]), "rows/step", found["n_rows"].tolist(),
                  "samples", int(found["poolm_batch_size"]), "rule margin %.3e" % float(found["rule_margin"]),
                  "dkl margin %.3e" % float(found["dkl_margin"]), "limit %.4e" % float(found["dkl_lim"]), "max|obs| %.2f" % float(np.abs(found["get_obs"]).max()),
                  "bytes", blob.getbuffer().nbytes)
    finally:
        rec.close()


if __name__ == "__main__":
    mg.install_stubs()
    if "--traces-only" not in sys.argv:
        gen_steps(HERE)
    if "--steps-only" not in sys.argv:
        gen_traces(HERE)
