"""GPU: user-defined termination / cost rules (cmbpo_amd.statics.TaskRules, cmbpo_task_rules_t) through every layer -- the
post kernel's clause table against ``TaskRules.numpy_fns()`` bit for bit on adversarial rows, against the built-in
HalfCheetahSafe rule, with the learned cost head, the golden traces G15 recorded from the REFERENCE's FakeEnv with
hand-written functions in its TERMS_BY_TASK / COST_BY_TASK (tests/golden/make_golden_task_rules.py) on all three matrix
paths and through the native rollout loop, and the trainer with ``static_fns=``.

Masks (term, rule costs, alive lists) are compared exactly; everything continuous at the tolerances of the files these
tests extend (test_rollout_sampler_gpu.py).  The G15 generator kept every tested value at least 1e-3 (relative to
max(1, |threshold|)) from its threshold, five times the 2e-4 at which the GPU forward is compared with the oracle.
"""
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, GOLD)
sys.path.insert(0, HERE)
NAMES = ["obs", "act", "adv", "cadv", "ret", "cret", "logp", "val", "cval", "cost", "log_std", "mu"]
TOL = dict(obs=2e-3, act=2e-3, adv=5e-3, cadv=2e-3, ret=2e-3, cret=2e-3, logp=2e-3, val=2e-3, cval=2e-3,
           cost=0.0, log_std=0.0, mu=2e-3)
G15 = ["g15_trace_rules_hopper", "g15_trace_rules_fatal", "g15_trace_rules_nodone"]
INF = float("inf")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _f32(x):
    return np.float32(x)


def _rule_sets():
    """The clause kinds of the language on columns every obs_dim >= 3 / act_dim >= 2 has; with and without the two flags."""
    from cmbpo_amd.statics import TaskRules, cost, fatal, healthy
    clauses = [
        healthy(cols=0, lo=-1.0, hi=1.0),                                            # closed interval
        healthy(cols=slice(1, None), abs=True, hi=100.0, hi_strict=True),            # magnitude guard over a slice
        healthy(cols=2, lo=0.5),                                                     # open above: +inf holds
        fatal(cols=-1, lo=2.0, lo_strict=True),                                      # a NaN survives a fatal clause
        fatal(cols=1, hi=-3.0),
        cost(cols=-1, scale=10.0, abs=True, hi=2.0, hi_strict=True),                 # the HalfCheetahSafe form
        cost(src="act", cols=slice(0, None), abs=True, lo=0.9, lo_strict=True, any=True),
        cost(src="obs", cols=slice(-2, None), hi=-0.5),                              # ALL over two columns of the old observation
        cost(cols=slice(0, 2), lo=0.25, hi=0.25, any=True),                          # a point interval
    ]
    return [TaskRules(clauses, require_finite=True, cost_on_term=True), TaskRules(clauses, require_finite=False, cost_on_term=False)]


def _adversarial(rng, E, B, D, A, live):
    """Inputs whose next_obs = mean[elite] + obs (obs zeroed where a value is planted, so the sum is the planted value) sit
    at, next to and far beyond the thresholds of _rule_sets(); rows of `live` only."""
    obs = (rng.standard_normal((B, D)) * 0.4).astype(np.float32)
    act = rng.uniform(-1, 1, (B, A)).astype(np.float32)
    mean = (rng.standard_normal((E, B, D + 1)) * 0.3).astype(np.float32)
    mean[:, :, 2] += 0.8          # most rows pass `next_obs[2] >= 0.5`, so the other clauses decide
    var = np.exp(rng.uniform(-12, 1, (E, B, D + 1))).astype(np.float32)
    inds = rng.integers(0, E, size=B).astype(np.int32)
    up, dn = lambda v: np.nextafter(_f32(v), _f32(INF)), lambda v: np.nextafter(_f32(v), _f32(-INF))
    plants = [
        (0, _f32(1.0)), (0, up(1.0)), (0, _f32(-1.0)), (0, dn(-1.0)), (0, _f32(-0.0)), (0, np.nan), (0, INF), (0, -INF),
        (1, _f32(100.0)), (1, dn(100.0)), (1, _f32(-100.0)), (1, _f32(-3.0)), (1, dn(-3.0)), (1, up(-3.0)), (1, np.nan), (1, -INF),
        (2, _f32(0.5)), (2, dn(0.5)), (2, INF), (2, np.nan), (2, _f32(-0.0)),
        (D - 1, _f32(2.0)), (D - 1, up(2.0)), (D - 1, np.nan), (D - 1, INF),
        # x * 10 rounds across 2.0: float32(0.2) * 10 is 2.0000000298 -> 2.0 (not < 2.0); one ulp below 0.2 gives 1.9999999
        (D - 1, _f32(0.2)), (D - 1, dn(0.2)), (D - 1, up(0.2)), (D - 1, _f32(-0.2)), (D - 1, up(-0.2)), (D - 1, _f32(-0.0)),
        (0, _f32(0.25)), (1, _f32(0.25)), (0, up(0.25)),
    ]
    for i, (col, val) in enumerate(plants):
        b = live[i % len(live)] if i < len(live) else live[(7 * i) % len(live)]
        obs[b, col] = 0.0
        mean[:, b, col] = val
    # the other two sources: actions at / next to 0.9, old observations at -0.5; non-finite values in an untested place
    k = len(plants)
    act[live[(k + 0) % len(live)], A - 1] = _f32(0.9)
    act[live[(k + 1) % len(live)], 0] = up(0.9)
    act[live[(k + 2) % len(live)], 1] = -up(0.9)
    act[live[(k + 3) % len(live)], 0] = np.nan
    obs[live[(k + 4) % len(live)], D - 2:] = _f32(-0.5)
    obs[live[(k + 5) % len(live)], D - 2:] = (_f32(-0.5), up(-0.5))
    mean[(inds[live[0]] + 1) % E, live[0], 0] = np.nan        # another member's NaN: reaches the KL, not this branch's next_obs
    var[:, live[1], 0] = 0.0
    return obs, act, mean, var, inds


@pytest.mark.parametrize("E", [7, 5, 3])                 # the kernel's three instances: 7 and 5 members compiled in, else run time
@pytest.mark.parametrize("D", [3, 8, 21, 47])            # the D < 8 row sums, no tail, tails of 5 and 7 columns
def test_post_kernel_rules_equal_numpy_fns_bit_for_bit(hip_lib, E, D):
    _need_gpu()
    from test_learned_cost_gpu import _run_post
    from cmbpo_amd import _lib
    rng = np.random.default_rng(zlib.crc32(f"rules/{E}/{D}".encode()))
    A, B, n = 5, 64, 37
    rows = rng.permutation(B)[:n].astype(np.int32)        # 37 rows, shuffled, of ld_rows = 64: the fifth workgroup has 5 of 8 rows
    obs, act, mean, var, inds = _adversarial(rng, E, B, D, A, rows)
    base = _run_post(_lib.TASK_DEFAULT, obs, act, mean, var, inds, D, A, rows)
    rest = np.setdiff1d(np.arange(B), rows)
    seen_done, seen_cost = set(), set()
    for rules in _rule_sets():
        assert rules.task_id >= _lib.TASK_USER_BASE
        got = _run_post(rules.task_id, obs, act, mean, var, inds, D, A, rows)
        for k in ("next_obs", "rew", "dkl_path", "ep_var_mean", "ep_var"):
            np.testing.assert_array_equal(_bits(got[k]), _bits(base[k]), err_msg=k)
        term_fn, cost_fn = rules.numpy_fns()
        nxt = got["next_obs"][rows]
        with np.errstate(all="ignore"):
            want_t = term_fn(obs[rows], act[rows], nxt)
            want_c = cost_fn(obs[rows], act[rows], nxt)
        assert want_t.dtype == bool and want_t.shape == (n, 1) and want_c.dtype == np.float32 and want_c.shape == (n, 1)
        np.testing.assert_array_equal(got["term"][rows], want_t[:, 0].astype(np.uint8))
        np.testing.assert_array_equal(_bits(got["cost"][rows]), _bits(want_c[:, 0]))
        assert (got["term"][rest] == 77).all() and (got["cost"][rest] == -7.0).all()
        seen_done |= set(want_t[:, 0].tolist())
        seen_cost |= set(want_c[:, 0].tolist())
    assert seen_done == {False, True} and seen_cost == {0.0, 1.0}        # the planted rows decide both ways


def test_hcs_rule_as_a_clause_equals_the_builtin(hip_lib):
    _need_gpu()
    from test_learned_cost_gpu import _run_post
    from cmbpo_amd import _lib, synthetic
    from cmbpo_amd.statics import TaskRules, cost
    rules = TaskRules([cost(cols=-1, scale=10, abs=True, hi=2.0, hi_strict=True)])
    rng = np.random.default_rng(11)
    task = "HalfCheetahSafe-v2"
    D, A = synthetic.ENV_DIMS[task]
    E, B = 7, 1003
    rows = np.arange(B, dtype=np.int32)
    obs, act, mean, var, inds = _adversarial(rng, E, B, D, A, rows)
    mean[..., D - 1] *= 0.5            # |next_obs[-1] * 10| on both sides of 2.0 in the random rows as well
    a = _run_post(_lib.TASK_HCS, obs, act, mean, var, inds, D, A)
    b = _run_post(rules.task_id, obs, act, mean, var, inds, D, A)
    for k in a:
        np.testing.assert_array_equal(_bits(a[k]) if a[k].dtype == np.float32 else a[k], _bits(b[k]) if b[k].dtype == np.float32 else b[k],
                                      err_msg=k)
    assert 0.05 < a["cost"].mean() < 0.95 and not a["term"].any()


def _replay(g, w, task_arg, hidden):
    """Step-by-step replay of a recorded trace with its draws injected; the assertions of
    test_rollout_sampler_gpu.test_hip_sampler_reproduces_reference_trace."""
    from test_rollout_sampler_gpu import hip_world
    B, T = int(g["B"]), int(g["T"])
    sampler, pool = hip_world(w, task_arg, T, str(g["mode"]), float(g["dkl_lim"]), B, hidden)
    sampler.reset(g["start"])
    budget = int(g["budget"]) or None
    for s in range(len(g["n_rows"])):
        n = int(g["n_rows"][s])
        assert pool.n_alive == n
        _, _, _, info = sampler.sample(max_samples=budget, eps=g["eps"][s, :n], model_inds=g["inds"][s, :n])
        np.testing.assert_array_equal(pool.alive_paths, g["alive"][s], err_msg=f"alive mask after step {s}")
        assert sampler._total_samples == g["total_samples"][s]
        assert info["alive_ratio"] == g["alive_ratio"][s]
    np.testing.assert_allclose(pool.t["dkl_acc"].cpu().numpy(), g["dkl_acc"], rtol=5e-3, atol=1e-9)
    diag = sampler.finish_all_paths()
    res, bdiag = pool.get()
    assert bdiag["poolm_batch_size"] == int(g["poolm_batch_size"])
    for k, arr in zip(NAMES, res):
        ref = g["get_" + k]
        assert arr.shape == ref.shape and arr.dtype == ref.dtype, k
        if TOL[k] == 0.0:
            np.testing.assert_array_equal(arr, ref, err_msg=k)       # cost masks / log_std copies: bit-exact
        else:
            np.testing.assert_allclose(arr, ref, rtol=TOL[k], atol=TOL[k], err_msg=k)
    np.testing.assert_allclose(bdiag["poolm_ret_mean"], float(g["poolm_ret_mean"]), rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(bdiag["poolm_cret_mean"], float(g["poolm_cret_mean"]), rtol=2e-3, atol=2e-4)
    for k in ("msampler/samples_added", "msampler/rollout_H_max"):
        assert diag[k] == float(g["diag_" + k.replace("/", "__")])
    for k in ("msampler/rollout_H_mean", "msampler/dyn_var_perstep", "msampler/cost_rate", "msampler/rew_rate",
              "msampler/v_mean", "msampler/cv_mean", "msampler/ens_DKL", "msampler/max_path_return",
              "msampler/max_dkl"):
        np.testing.assert_allclose(diag[k], float(g["diag_" + k.replace("/", "__")]), rtol=5e-3, atol=1e-6, err_msg=k)
    return res


def test_g5_hcs_trace_replays_with_the_rule_as_a_clause(hip_lib):
    _need_gpu()
    from worlds import build_world
    from cmbpo_amd.statics import TaskRules, cost
    g = np.load(os.path.join(GOLD, "g5_trace_hcs_sched.npz"), allow_pickle=False)
    task, hidden = str(g["task"]), int(g["hidden"])
    w = build_world(int(g["seed"]), task, hidden, out_scale=float(g["out_scale"]), q_boost=float(g["q_boost"]))
    res = _replay(g, w, TaskRules([cost(cols=-1, scale=10, abs=True, hi=2.0, hi_strict=True)]), hidden)
    assert 0.0 < float(res[9].mean()) < 1.0


def test_rules_with_the_learned_cost_head(hip_lib):
    """term follows the rules, cost is the elite member's column; COST clauses and cost_on_term are ignored."""
    _need_gpu()
    from test_learned_cost_gpu import _run_post
    from cmbpo_amd import _lib
    rng = np.random.default_rng(5)
    E, D, A, B = 5, 21, 5, 45
    rows = np.arange(B, dtype=np.int32)
    obs, act, mean, var, inds = _adversarial(rng, E, B, D, A, rows)
    cost_col = (rng.standard_normal((E, B, 1)) * 2).astype(np.float32)
    cost_col[inds[3], 3] = np.nan
    mean2 = np.concatenate([mean, cost_col], -1)
    var2 = np.concatenate([var, np.ones_like(cost_col)], -1)
    for rules in _rule_sets():
        plain = _run_post(rules.task_id, obs, act, mean, var, inds, D, A)
        got = _run_post(rules.task_id | _lib.TASK_LEARNED_COST, obs, act, mean2, var2, inds, D, A)
        np.testing.assert_array_equal(got["term"], plain["term"])
        np.testing.assert_array_equal(_bits(got["next_obs"]), _bits(plain["next_obs"]))
        np.testing.assert_array_equal(_bits(got["cost"]), _bits(cost_col[inds, rows, 0]))
        term_fn, _ = rules.numpy_fns()
        with np.errstate(all="ignore"):
            np.testing.assert_array_equal(got["term"], term_fn(obs, act, got["next_obs"])[:, 0].astype(np.uint8))
        assert got["term"].any() and not got["term"].all()


def _g15(name):
    import worlds_rules
    from worlds import build_world
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    case = worlds_rules.CASES[name]
    rules = worlds_rules.build_rules(case["rules"](*g["thresholds"].tolist()))
    w = build_world(int(g["seed"]), str(g["task"]), int(g["hidden"]), out_scale=float(g["out_scale"]), q_boost=float(g["q_boost"]))
    return g, w, rules


@pytest.mark.parametrize("name", G15)
@pytest.mark.parametrize("ens_path", [0, 1, 2], indirect=True, ids=["fp32mfma", "splitbf16", "splitf16"])
def test_hip_sampler_reproduces_reference_trace_with_user_rules(hip_lib, ens_path, name):
    _need_gpu()
    g, w, rules = _g15(name)
    res = _replay(g, w, rules, int(g["hidden"]))
    if name != "g15_trace_rules_nodone":
        assert (np.diff(g["n_rows"]) < 0).any()          # nothing but the rules' terminations shrinks these alive lists
    assert 0.2 <= float(res[9].mean()) <= 0.8


def _loop_vs_many(w, rules, task, B, T, mode, start, budget, hidden=128):
    from test_rollout_sampler_gpu import hip_world
    out = []
    for many in (False, True):
        sampler, pool = hip_world(w, rules, T, mode, float("inf"), B, hidden)
        sampler._gen.manual_seed(5)
        sampler.reset(start)
        steps, alive = 0, [pool.n_alive]
        if many:
            steps, info = sampler.sample_many(max_samples=budget)
        else:
            while sampler.any_alive() and pool.has_room:
                _, _, _, info = sampler.sample(max_samples=budget)
                steps += 1
                alive.append(pool.n_alive)
        state = (steps, pool.n_alive, pool.ptr, sampler._total_samples, info["alive_ratio"])
        diag = sampler.finish_all_paths()
        res, _ = pool.get()
        out.append((state, diag["msampler/samples_added"], res, alive))
    assert out[0][0] == out[1][0], (out[0][0], out[1][0])
    assert out[0][0][0] >= 2 and out[0][1] == out[1][1]
    for k, a, b in zip(NAMES, out[0][2], out[1][2]):
        np.testing.assert_array_equal(a, b, err_msg=k)
    return out[0]


@pytest.mark.parametrize("name", G15)
def test_sample_many_equals_a_loop_of_sample_with_user_rules(hip_lib, name):
    """cmbpo_rollout_run with a registered rule id takes exactly the steps a Python loop of sample() takes, bit-identical
    buffers; on the G15 worlds, rules and start states (the sampler's own draws: sample_many takes none from outside)."""
    _need_gpu()
    g, w, rules = _g15(name)
    state, _, res, alive = _loop_vs_many(w, rules, str(g["task"]), int(g["B"]), int(g["T"]), str(g["mode"]), g["start"],
                                        int(g["budget"]) or None)
    if name != "g15_trace_rules_nodone":
        assert alive[-1] < alive[0]
    assert 0.0 < float(res[9].mean()) < 1.0


def test_user_rules_across_the_small_batch_threshold(hip_lib):
    """The alive count starts above the one-workgroup bookkeeping's row limit and falls below it through the rules'
    terminations: both ways a step reaches the post kernel, in one rollout."""
    _need_gpu()
    from cmbpo_amd import synthetic
    g, w, rules = _g15("g15_trace_rules_hopper")
    limit = hip_lib.cmbpo_rollout_book_pre_max_rows()
    B = limit + 60
    start = synthetic.start_states(np.random.default_rng(78), B, str(g["task"]))
    state, _, res, alive = _loop_vs_many(w, rules, str(g["task"]), B, int(g["T"]), str(g["mode"]), start, None)
    stepped = alive[:-1]                  # the alive count each step started with
    assert sum(a > limit for a in stepped) >= 2 and sum(0 < a <= limit for a in stepped) >= 2, (alive, limit)


def test_fake_env_step_with_user_rules(hip_lib):
    """The host API: a TaskRules or a registered name as `task`; bool cost exactly where the reference returns
    np.zeros_like(terms); unknown names stay the default task."""
    _need_gpu()
    from test_learned_cost_gpu import _Space
    from test_rollout_sampler_gpu import hip_world
    from cmbpo_amd import _lib, statics
    g, w, rules = _g15("g15_trace_rules_hopper")
    D, A = w["obs_dim"], w["act_dim"]
    term_only = statics.TaskRules([c for c in rules.clauses if c.role != "cost"], require_finite=True)
    statics.register_task("RulesHopper-v0", rules)
    n = int(g["B"])
    act = np.random.default_rng(1).uniform(-1, 1, (n, A)).astype(np.float32)
    inds = g["inds"][0]
    outs = {}
    for key, task in (("rules", rules), ("name", "RulesHopper-v0"), ("term_only", term_only), ("unknown", "NoSuchTask-v0")):
        sampler, _ = hip_world(w, task, 4, "schedule", float("inf"), n, int(g["hidden"]))
        env = sampler.env if hasattr(sampler, "env") else sampler._env
        outs[key] = (env, env.step(g["start"], act, model_inds=inds))
    env, (nobs, r, terms, info) = outs["rules"]
    assert env._task_id == rules.task_id == outs["name"][0]._task_id >= _lib.TASK_USER_BASE
    term_fn, cost_fn = rules.numpy_fns()
    np.testing.assert_array_equal(terms, term_fn(g["start"], act, nobs))
    np.testing.assert_array_equal(info["cost"], cost_fn(g["start"], act, nobs))
    assert terms.dtype == bool and terms.shape == (n, 1) and info["cost"].dtype == np.float32 and info["cost"].shape == (n, 1)
    np.testing.assert_array_equal(outs["name"][1][3]["cost"], info["cost"])
    _, _, terms_t, info_t = outs["term_only"][1]
    np.testing.assert_array_equal(terms_t, terms)
    assert term_only.numpy_fns()[1] is None and info_t["cost"].dtype == bool and not info_t["cost"].any()
    env_u, (_, _, terms_u, info_u) = outs["unknown"]
    assert env_u._task_id == _lib.TASK_DEFAULT and not terms_u.any() and info_u["cost"].dtype == bool


def test_cmbpo_trainer_with_static_fns(hip_lib):
    """CMBPO(static_fns=rules) on the toy world for two epochs: the imagined rollouts end where the rules say.  Before every
    finish_all_paths the rollout state is read back: per branch, the next observation of its last step (the one of the two
    swapped observation arrays that is not the stored observation of that step) satisfies term_fn iff the kernel flagged the
    branch terminal, flagged branches are not alive, and paths shorter than the horizon exist."""
    _need_gpu()
    import toyworld
    from cmbpo_amd import _lib, synthetic
    from cmbpo_amd.cmbpo import CMBPO
    from cmbpo_amd.cpo_policy import CPOPolicy
    from cmbpo_amd.cpo_sampler import CpoSampler
    from cmbpo_amd.cpobuffer import CPOBuffer
    from cmbpo_amd.statics import TaskRules, fatal, healthy
    rules = TaskRules([fatal(cols=0, lo=0.05, lo_strict=True), healthy(cols=slice(1, None), abs=True, hi=100.0, hi_strict=True)],
                      require_finite=True, cost_on_term=True)
    term_fn, _ = rules.numpy_fns()
    np.random.seed(0)
    env = toyworld.ToyEnv()
    D, A, T = env.D, env.A, 40
    policy = CPOPolicy(env.observation_space, env.action_space, a_hidden_layer_sizes=(128, 128),
                       vf_hidden_layer_sizes=(128, 128), vf_ensemble_size=3, vf_elites=2, vf_activation="swish",
                       vf_loss="MSE", vf_lr=1e-3, vf_epochs=2, vf_batch_size=256, device="cuda:0", max_path_length=T,
                       cost_lim=5.0, target_kl=0.01)
    policy.set_params(synthetic.policy_params(np.random.default_rng(2), D, A, 128))
    rng = np.random.RandomState(1)
    policy.v.init_weights(rng)
    policy.vc.init_weights(rng)
    buf = CPOBuffer(600, 6000, env.observation_space, env.action_space)
    with pytest.raises(TypeError, match="static_fns"):
        CMBPO(env, policy, buf, sampler=CpoSampler(max_path_length=T), static_fns=term_fn, use_model=False)
    algo = CMBPO(env, policy, buf, sampler=CpoSampler(max_path_length=T), task="AntSafe-v2", static_fns=rules,
                 n_env_interacts=10 ** 9, eval_every_n_steps=1, m_train_freq=100, m_networks=4, m_elites=3,
                 m_hidden_dims=(128, 128), rollout_batch_size=400, rollout_mode="schedule", rollout_schedule=[0, 1, 4, 4],
                 maxroll=6, initial_real_samples_per_epoch=150, min_real_samples_per_epoch=100, batch_size_policy=2500,
                 n_initial_exploration_steps=300, n_epochs=50,
                 initial_model_train_kwargs=dict(min_epochs=3, max_epochs=6, batch_size=128),
                 model_train_kwargs=dict(min_epochs=1, max_epochs=2, batch_size=128))
    assert algo.fake_env._task_id == rules.task_id >= _lib.TASK_USER_BASE        # static_fns over task
    snaps = []
    finish = algo.model_sampler.finish_all_paths

    def recording(*a, **k):
        t = algo.model_buf.t
        snaps.append({k2: t[k2].cpu().numpy().copy() for k2 in ("len", "term_t", "cur_obs", "next_obs", "obs_buf")}
                     | {"alive": np.asarray(algo.model_buf.alive_paths).copy()})
        return finish(*a, **k)

    algo.model_sampler.finish_all_paths = recording
    diags = []
    for d in algo.train():
        diags.append(d)
        if len(diags) >= 2:
            break
    assert len(diags) == 2 and snaps
    checked = flagged = short = 0
    for s in snaps:
        B = s["len"].shape[0]
        horizon = int(s["len"].max())
        for b in range(B):
            L = int(s["len"][b])
            if L < 1:
                continue
            stored = s["obs_buf"][L - 1, b]
            cands = [x[b] for x in (s["cur_obs"], s["next_obs"])]
            same = [np.array_equal(c, stored) for c in cands]
            if sum(same) != 1:
                continue        # (a branch the sample budget cut before its last computed step was stored)
            last_next = cands[same.index(False)]
            is_term = bool(term_fn(stored[None], np.zeros((1, A), np.float32), last_next[None])[0, 0])
            assert is_term == bool(s["term_t"][b]), (b, L, last_next)
            if is_term:
                assert not s["alive"][b]
                flagged += 1
                short += int(L < horizon)
            checked += 1
    assert checked > 100 and flagged > 0 and short > 0, (checked, flagged, short)
    assert np.isfinite(diags[0]["model/poolm_cret_mean"])
