"""CPU: golden G16 (tests/golden/make_golden_stochastic.py: the reference's FakeEnv.step called with deterministic=False)
loads, satisfies the conditions its generator asserted, and pins the semantics of stochastic transitions: `noisy_step`
below, the NumPy statement the kernel is tested against, reproduces the reference's single steps at xi == 1 -- next_obs,
r, terms and cost bit for bit, dkl_path / ep_var at the tolerances of test_fakeenv_post_matches_oracle."""
import os

import numpy as np
import pytest

from oracle import refcpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STEP_E, STEP_D = (7, 5, 3), (3, 8, 21, 47)
STEP_TASKS = {"ant": "AntSafe-v2", "hcs": "HalfCheetahSafe-v2", "default": "default"}
TRACES = ("g16_trace_ant_term", "g16_trace_ant_unc", "g16_trace_hcs_sched")
MAX_BYTES = 520 * 1024


def noisy_step(obs, act, mean, var, inds, xi, term_fn, cost_fn=None, learned_cost=False):
    """FakeEnv.step with transition noise, given the ensemble's float32 (mean, var)[E, n, out] and xi[n, obs]: every
    member's observation columns move by std * xi (float32 throughout: two roundings), the uncertainty measures run on the
    shifted means and the unshifted std, reward and learned cost are the elite's unshifted columns."""
    assert all(a.dtype == np.float32 for a in (obs, mean, var, xi))
    D, rows = obs.shape[-1], np.arange(obs.shape[0])
    std = np.sqrt(var)
    shifted = mean[..., :D] + std[..., :D] * xi[None]
    ep_var = np.var(shifted, axis=0)
    dkl_path = np.mean(refcpu.average_dkl(shifted, std[..., :D]), axis=-1)
    next_obs = shifted[inds, rows] + obs
    r = mean[inds, rows, D]
    terms = term_fn(obs, act, next_obs)
    if learned_cost:
        cost = mean[inds, rows, D + 1][:, None]
    else:
        cost = cost_fn(obs, act, next_obs) if cost_fn is not None else np.zeros_like(terms)
    return dict(next_obs=next_obs, r=r[:, None], terms=terms, cost=cost, dkl_path=dkl_path, ep_var=ep_var)


def builtin_fns(task):
    return refcpu.TERMS_BY_TASK.get(task, refcpu.no_done), refcpu.COST_BY_TASK.get(task)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def step_cases():
    return [(E, D, tag) for E in STEP_E for D in STEP_D for tag in STEP_TASKS if not (tag == "ant" and D < 5)]


def load_step(E, D, tag):
    g = np.load(os.path.join(GOLD, f"g16_step_e{E}.npz"), allow_pickle=False)
    pre = f"d{D}_"
    inp = {k: g[pre + k] for k in ("obs", "act", "mean", "var", "inds")}
    want = {k: g[pre + tag + "_" + k] for k in ("next_obs", "r", "terms", "cost", "dkl_path", "ep_var")}
    return inp, want


def test_g16_files_load_and_fit():
    for name in [f"g16_step_e{E}" for E in STEP_E] + list(TRACES):
        path = os.path.join(GOLD, name + ".npz")
        assert os.path.getsize(path) <= MAX_BYTES, name
        g = np.load(path, allow_pickle=False)
        assert len(g.files) > 10
    for E in STEP_E:
        g = np.load(os.path.join(GOLD, f"g16_step_e{E}.npz"), allow_pickle=False)
        for D in STEP_D:
            var, mean = g[f"d{D}_var"], g[f"d{D}_mean"]
            assert mean.shape == var.shape == (E, 64, D + 1) and mean.dtype == var.dtype == np.float32
            assert var[0, 0, 0] == 0.0 and var[1, 1, 1] == np.float32(1e30)
            rest = np.delete(var.reshape(-1), [0, np.ravel_multi_index((1, 1, 1), var.shape)])
            assert rest.min() >= 1e-12 * 0.99 and rest.max() <= 10.0 and rest.min() < 1e-10 and rest.max() > 1.0
            assert np.isin(g[f"d{D}_inds"], g["elites"]).all()


def rule_margin(task, nxt):
    """Smallest distance of a value a built-in rule of `task` tests on these next observations from its threshold."""
    if task == "AntSafe-v2":
        z = nxt[:, 0]
        zrot = 1 - 2 * (nxt[:, 2] ** 2 + nxt[:, 3] ** 2)
        gate = np.isfinite(nxt).all(axis=-1) * (z >= 0.2) * (z <= 1.0)
        vals = [np.abs(z - 0.2), np.abs(z - 1.0), np.abs(gate * zrot + 0.7), np.abs(np.abs(nxt[:, -1]) - 3.2)]
    else:
        vals = [np.abs(np.abs(nxt[:, -1] * 10) - 2.0)]
    return float(min(v.min() for v in vals))


def test_g16_traces_satisfy_the_generators_conditions():
    """Recomputed from the recorded arrays, not read from the scalars the generator stored beside them."""
    g = np.load(os.path.join(GOLD, "g16_trace_ant_term.npz"), allow_pickle=False)
    assert str(g["task"]) == "AntSafe-v2" and not np.isfinite(float(g["dkl_lim"])) and int(g["budget"]) == 0
    assert int((np.diff(g["n_rows"]) < 0).sum()) >= 2            # static terminations on at least 2 steps
    u = np.load(os.path.join(GOLD, "g16_trace_ant_unc.npz"), allow_pickle=False)
    assert str(u["task"]) == "AntSafe-v2" and int(u["budget"]) == 0
    h = np.load(os.path.join(GOLD, "g16_trace_hcs_sched.npz"), allow_pickle=False)
    assert str(h["mode"]) == "schedule" and 0.1 <= float(h["diag_msampler__cost_rate"]) <= 0.9
    assert (np.diff(h["n_rows"]) == 0).all()
    for t in (g, u, h):
        # every value a built-in rule tested, on every step, at least 1e-3 from its threshold
        nxt, n_rows = t["next_obs_log"], t["n_rows"]
        assert nxt.dtype == np.float32 and nxt.shape == (len(n_rows), int(t["B"]), t["start"].shape[1])
        margin = min(rule_margin(str(t["task"]), nxt[s, :n]) for s, n in enumerate(n_rows))
        assert margin >= 1e-3 and margin == float(t["rule_margin"])
        assert np.isfinite(t["get_obs"]).all() and np.abs(t["get_obs"]).max() < 10
    # the limit: the middle of the widest gap of the probe's sums near their median (make_golden.gen_sampler_traces)
    acc = np.sort(u["probe_dkl_acc"])
    lo, hi = int(.35 * len(acc)), int(.65 * len(acc))
    k = lo + int(np.argmax(acc[lo + 1:hi + 1] - acc[lo:hi]))
    lim, half_gap = float(0.5 * (acc[k] + acc[k + 1])), float(0.5 * (acc[k + 1] - acc[k]))
    assert lim == float(u["dkl_lim"]) and half_gap == float(u["half_gap"]) and half_gap > 0
    # no sum the uncertainty test saw lies within that gap, or within the replays' rtol of 5e-3, of the limit
    sums = [v[:n] for v, n in zip(u["dkl_sum_log"], u["n_rows"])]
    assert all(np.isfinite(v).all() for v in sums) and np.isnan(u["dkl_sum_log"][-1, u["n_rows"][-1]:]).all()
    dist = min(float(np.abs(v - lim).min()) for v in sums)
    assert dist >= half_gap and dist >= 5e-3 * lim and dist == float(u["dkl_margin"])
    # uncertainty deaths, and a step on which the rule ends some but not all of the rows it sees
    deaths = [int((v >= lim).sum()) for v in sums]
    assert sum(deaths) == int(u["n_unc_deaths"]) > 0
    assert any(0 < d < len(v) for d, v in zip(deaths, sums))
    # the recorded masks agree with the sums: a row over the limit is not alive after its step
    for s, v in enumerate(sums):
        before = u["alive"][s - 1] if s else np.ones(int(u["B"]), bool)
        assert before.sum() == len(v) and not u["alive"][s][np.flatnonzero(before)[v >= lim]].any()


@pytest.mark.parametrize("E,D,tag", step_cases())
def test_numpy_statement_reproduces_the_reference_at_xi_one(E, D, tag):
    inp, want = load_step(E, D, tag)
    term_fn, cost_fn = builtin_fns(STEP_TASKS[tag])
    with np.errstate(all="ignore"):
        got = noisy_step(inp["obs"], inp["act"], inp["mean"], inp["var"], inp["inds"], np.ones_like(inp["obs"]), term_fn, cost_fn)
    for k in ("next_obs", "r"):
        assert got[k].dtype == want[k].dtype == np.float32 and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(bits(got[k]), bits(want[k]), err_msg=k)
    assert want["terms"].dtype == bool and want["terms"].shape == (64, 1)
    np.testing.assert_array_equal(got["terms"], want["terms"])
    assert got["cost"].shape == want["cost"].shape == (64, 1)
    np.testing.assert_array_equal(np.asarray(got["cost"], np.float64), np.asarray(want["cost"], np.float64))
    ok = np.isfinite(want["dkl_path"])
    np.testing.assert_array_equal(np.isnan(got["dkl_path"]), np.isnan(want["dkl_path"]))
    np.testing.assert_allclose(got["dkl_path"][ok], want["dkl_path"][ok], rtol=1e-4, atol=1e-7)
    okv = np.isfinite(want["ep_var"])
    np.testing.assert_allclose(got["ep_var"][okv], want["ep_var"][okv], rtol=1e-5, atol=1e-9)
    if tag == "ant":
        assert set(want["terms"][:, 0].tolist()) == {False, True} and set(want["cost"][:, 0].tolist()) == {0.0, 1.0}
    if tag == "hcs":
        assert set(want["cost"][:, 0].tolist()) == {0.0, 1.0}
    # the shift is there: the reference's deterministic step lands elsewhere
    det = inp["mean"][inp["inds"], np.arange(64), :D] + inp["obs"]
    assert (bits(det) != bits(want["next_obs"])).mean() > 0.9
