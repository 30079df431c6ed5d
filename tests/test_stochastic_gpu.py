"""GPU: stochastic model transitions (next_obs ~ N(mean, var) of the elite member) through every layer -- the NOISE
instances of the post kernel against the NumPy statement of tests/test_stochastic_fixtures.py and against the reference's
recorded deterministic=False steps (golden G16), the sampler's replay of the reference's traces at xi == 1 on the three
matrix paths, cmbpo_rollout_run against a loop of steps with the sampler's own draws, FakeEnv.step(noise=) and the
trainer's m_stochastic switch."""
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_stochastic_fixtures import (STEP_D, STEP_E, STEP_TASKS, TRACES, bits, builtin_fns, load_step,  # noqa: E402
                                      noisy_step, step_cases)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
OUTS = ("next_obs", "rew", "term", "cost", "dkl_path", "ep_var_mean", "ep_var")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _run_post(task_arg, obs, act, mean, var, inds, xi, row_idx=None, dev_rows=False, noise_entry=True):
    """cmbpo_fakeenv_post_noise (or cmbpo_fakeenv_post) on slot-indexed arrays ([B, .] / [E, B, .]); with row_idx only the
    listed slots are stepped; dev_rows: the row count is read on the device, the host's is an upper bound."""
    from cmbpo_amd import _lib
    dev = torch.device("cuda:0")
    B, E, D = obs.shape[0], mean.shape[0], obs.shape[1]
    n = B if row_idx is None else len(row_idx)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    f = dict(dtype=torch.float32, device=dev)
    out = dict(next_obs=torch.full((B, D), -7.0, **f), rew=torch.full((B,), -7.0, **f),
               term=torch.full((B,), 77, dtype=torch.uint8, device=dev), cost=torch.full((B,), -7.0, **f),
               dkl_path=torch.full((B,), -7.0, **f), ep_var_mean=torch.full((B,), -7.0, **f),
               ep_var=torch.full((B, D), -7.0, **f))
    d = [t(obs), t(act), t(mean), t(var), t(inds)]
    ri = d_n = None
    n_host = n
    if row_idx is not None:
        ri = t(np.concatenate([np.asarray(row_idx, np.int32), np.zeros(8, np.int32)]))
    if dev_rows:
        d_n, n_host = t(np.array([n], np.int32)), min(n + 3, B)
    args = [task_arg, E, D, act.shape[1], _lib.ptr(d[2]), _lib.ptr(d[3]), B, _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[4]),
            _lib.ptr(ri), _lib.ptr(d_n), n_host] + [_lib.ptr(out[k]) for k in OUTS]
    if noise_entry:
        d_xi = None if xi is None else t(xi)
        rc = _lib.lib().cmbpo_fakeenv_post_noise(*args, _lib.ptr(d_xi), _lib.current_stream())
    else:
        rc = _lib.lib().cmbpo_fakeenv_post(*args, _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, _lib.lib().cmbpo_last_error())
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_against_statement(got, want, rows, rest):
    """next_obs, rew, term, cost bit for bit; dkl_path / ep_var at test_fakeenv_post_matches_oracle's tolerances."""
    np.testing.assert_array_equal(bits(got["next_obs"][rows]), bits(want["next_obs"]), err_msg="next_obs")
    np.testing.assert_array_equal(bits(got["rew"][rows]), bits(want["r"][:, 0]), err_msg="rew")
    np.testing.assert_array_equal(got["term"][rows], want["terms"][:, 0].astype(np.uint8), err_msg="term")
    np.testing.assert_array_equal(bits(got["cost"][rows]), bits(np.asarray(want["cost"], np.float32)[:, 0]), err_msg="cost")
    ok = np.isfinite(want["dkl_path"])
    np.testing.assert_array_equal(np.isnan(got["dkl_path"][rows]), np.isnan(want["dkl_path"]))
    np.testing.assert_array_equal(np.isinf(got["dkl_path"][rows]), np.isinf(want["dkl_path"]))
    np.testing.assert_allclose(got["dkl_path"][rows][ok], want["dkl_path"][ok], rtol=1e-4, atol=1e-7)
    okv = np.isfinite(want["ep_var"])
    np.testing.assert_allclose(got["ep_var"][rows][okv], want["ep_var"][okv], rtol=1e-5, atol=1e-9)
    okm = okv.all(-1)
    np.testing.assert_allclose(got["ep_var_mean"][rows][okm], want["ep_var"].mean(-1)[okm], rtol=1e-5, atol=1e-9)
    assert (got["term"][rest] == 77).all() and (got["cost"][rest] == -7.0).all() and (got["next_obs"][rest] == -7.0).all()


@pytest.mark.parametrize("E", STEP_E)                    # the kernel's instances: 7 and 5 members compiled in, else run time
@pytest.mark.parametrize("D", STEP_D)                    # the D < 8 row sums, no tail, tails of 5 and 7 columns
def test_noise_kernel_equals_the_numpy_statement(hip_lib, E, D):
    _need_gpu()
    from cmbpo_amd import _lib
    from test_task_rules_gpu import _rule_sets
    rng = np.random.default_rng(zlib.crc32(f"noise/{E}/{D}".encode()))
    A, B, n = 5, 64, 37
    rows = rng.permutation(B)[:n].astype(np.int32)        # 37 rows, shuffled, of ld_rows = 64: the fifth workgroup has 5 of 8 rows
    rest = np.setdiff1d(np.arange(B), rows)
    obs = (rng.standard_normal((B, D)) * 0.4).astype(np.float32)
    obs[:, 0] = rng.uniform(-0.1, 1.3, B).astype(np.float32)
    act = rng.uniform(-1, 1, (B, A)).astype(np.float32)
    mean2 = (rng.standard_normal((E, B, D + 2)) * 0.3).astype(np.float32)         # with the learned-cost column
    var2 = np.exp(rng.uniform(-12, 1, (E, B, D + 2))).astype(np.float32)
    var2[0, rows[0], 0], var2[1, rows[1], 1], var2[:, rows[2], 2] = 0.0, 1e30, 0.0
    inds = rng.integers(0, E, size=B).astype(np.int32)
    xi = rng.standard_normal((B, D)).astype(np.float32)
    xi[rows[:10], 0] = (0.0, 1.0, -1.0, 4.0, -4.0, 0.0, 1.0, -1.0, 4.0, -4.0)
    xi[rows[10:15], D - 1] = (0.0, 1.0, -1.0, 4.0, -4.0)
    mean1, var1 = np.ascontiguousarray(mean2[..., :D + 1]), np.ascontiguousarray(var2[..., :D + 1])
    rules = _rule_sets()[0]
    cases = [("HalfCheetahSafe-v2", _lib.TASK_HCS, False), ("default", _lib.TASK_DEFAULT, False),
             ("HalfCheetahSafe-v2", _lib.TASK_HCS, True), (rules, rules.task_id, False), (rules, rules.task_id, True)]
    if D >= 5:
        cases += [("AntSafe-v2", _lib.TASK_ANTSAFE, False), ("AntSafe-v2", _lib.TASK_ANTSAFE, True)]
    zero = np.zeros_like(xi)
    for k, (task, tid, learned) in enumerate(cases):
        mean, var = (mean2, var2) if learned else (mean1, var1)
        targ = tid | (_lib.TASK_LEARNED_COST if learned else 0)
        term_fn, cost_fn = builtin_fns(task) if isinstance(task, str) else task.numpy_fns()
        got = _run_post(targ, obs, act, mean, var, inds, xi, rows, dev_rows=bool(k % 2))
        with np.errstate(all="ignore"):
            want = noisy_step(obs[rows], act[rows], mean[:, rows], var[:, rows], inds[rows], xi[rows], term_fn, cost_fn, learned)
        _check_against_statement(got, want, rows, rest)
        # xi == 0: every output is the deterministic launch's, bit for bit
        got0 = _run_post(targ, obs, act, mean, var, inds, zero, rows)
        det = _run_post(targ, obs, act, mean, var, inds, None, rows, noise_entry=False)
        fwd = _run_post(targ, obs, act, mean, var, inds, None, rows)            # a NULL draw pointer forwards
        for key in OUTS:
            np.testing.assert_array_equal(got0[key].view(np.uint8), det[key].view(np.uint8), err_msg=f"xi = 0: {key}")
            np.testing.assert_array_equal(fwd[key].view(np.uint8), det[key].view(np.uint8), err_msg=f"NULL xi: {key}")
        assert (bits(got["next_obs"][rows]) != bits(det["next_obs"][rows])).mean() > 0.8
        np.testing.assert_array_equal(bits(got["rew"]), bits(det["rew"]))        # reward (and learned cost): unperturbed columns
        if learned:
            np.testing.assert_array_equal(bits(got["cost"]), bits(det["cost"]))


@pytest.mark.parametrize("E", STEP_E)
def test_noise_entry_reproduces_the_reference_at_xi_one(hip_lib, E):
    """G16(a): the reference's FakeEnv.step(deterministic=False) on given (mean, var), through cmbpo_fakeenv_post_noise."""
    _need_gpu()
    from cmbpo_amd import _lib
    for (e, D, tag) in step_cases():
        if e != E:
            continue
        inp, want = load_step(E, D, tag)
        got = _run_post(_lib.TASK_IDS.get(STEP_TASKS[tag], 0), inp["obs"], inp["act"], inp["mean"], inp["var"], inp["inds"],
                        np.ones_like(inp["obs"]))
        np.testing.assert_array_equal(bits(got["next_obs"]), bits(want["next_obs"]), err_msg=f"{D}/{tag} next_obs")
        np.testing.assert_array_equal(bits(got["rew"]), bits(want["r"][:, 0]), err_msg=f"{D}/{tag} r")
        np.testing.assert_array_equal(got["term"].astype(bool), want["terms"][:, 0], err_msg=f"{D}/{tag} terms")
        np.testing.assert_array_equal(got["cost"], np.asarray(want["cost"], np.float32)[:, 0], err_msg=f"{D}/{tag} cost")
        ok = np.isfinite(want["dkl_path"])
        np.testing.assert_array_equal(np.isnan(got["dkl_path"]), np.isnan(want["dkl_path"]))
        np.testing.assert_array_equal(np.isinf(got["dkl_path"]), np.isinf(want["dkl_path"]))
        np.testing.assert_allclose(got["dkl_path"][ok], want["dkl_path"][ok], rtol=1e-4, atol=1e-7)
        okv = np.isfinite(want["ep_var"])
        np.testing.assert_allclose(got["ep_var"][okv], want["ep_var"][okv], rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("name", TRACES)
@pytest.mark.parametrize("ens_path", [0, 1, 2], indirect=True, ids=["fp32mfma", "splitbf16", "splitf16"])
def test_sampler_replays_the_reference_traces_at_xi_one(hip_lib, ens_path, name):
    """G16(b): the reference's ModelSampler with every FakeEnv.step at deterministic=False, replayed with xi = ones; the
    tolerances are test_hip_sampler_reproduces_reference_trace's."""
    _need_gpu()
    from test_rollout_sampler_gpu import NAMES, TOL, hip_world
    from worlds import build_world
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    task, B, T, hidden = str(g["task"]), int(g["B"]), int(g["T"]), int(g["hidden"])
    w = build_world(int(g["seed"]), task, hidden, out_scale=float(g["out_scale"]), q_boost=float(g["q_boost"]))
    sampler, pool = hip_world(w, task, T, str(g["mode"]), float(g["dkl_lim"]), B, hidden)
    sampler.reset(g["start"])
    budget = int(g["budget"]) or None
    for s in range(len(g["n_rows"])):
        n = int(g["n_rows"][s])
        assert pool.n_alive == n
        _, _, _, info = sampler.sample(max_samples=budget, eps=g["eps"][s, :n], model_inds=g["inds"][s, :n],
                                       xi=np.ones((n, w["obs_dim"]), np.float32))
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
            np.testing.assert_array_equal(arr, ref, err_msg=k)
        else:
            np.testing.assert_allclose(arr, ref, rtol=TOL[k], atol=TOL[k], err_msg=k)
    np.testing.assert_allclose(bdiag["poolm_ret_mean"], float(g["poolm_ret_mean"]), rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(bdiag["poolm_cret_mean"], float(g["poolm_cret_mean"]), rtol=2e-3, atol=2e-4)
    for k in ("msampler/samples_added", "msampler/rollout_H_max"):
        assert diag[k] == float(g["diag_" + k.replace("/", "__")])
    for k in ("msampler/rollout_H_mean", "msampler/dyn_var_perstep", "msampler/cost_rate", "msampler/rew_rate",
              "msampler/v_mean", "msampler/cv_mean", "msampler/ens_DKL", "msampler/max_path_return", "msampler/max_dkl"):
        np.testing.assert_allclose(diag[k], float(g["diag_" + k.replace("/", "__")]), rtol=5e-3, atol=1e-6, err_msg=k)


def _rollout(w, task, B, T, start, stochastic, many, seed=5):
    from test_rollout_sampler_gpu import hip_world
    sampler, pool = hip_world(w, task, T, "schedule", float("inf"), B, 128)
    sampler.stochastic = stochastic
    sampler._gen.manual_seed(seed)
    sampler.reset(start)
    steps, chunks = 0, set()
    if many:
        steps, _ = sampler.sample_many()
    else:
        while sampler.any_alive() and pool.has_room:
            sampler.sample()
            chunks.add(sampler._draws[1].data_ptr())
            steps += 1
    state = (steps, pool.n_alive, pool.ptr, sampler._total_samples)
    sampler.finish_all_paths()
    res, _ = pool.get()
    return state, res, len(chunks), sampler._draws[1].shape[0]


@pytest.mark.parametrize("B,T", [(1000, 43), (5000, 19)])      # look-ahead path (chunks of 40 steps) / plain path (chunks of 16)
def test_sample_many_equals_a_loop_of_sample_with_own_draws(hip_lib, B, T):
    _need_gpu()
    from test_rollout_sampler_gpu import NAMES
    from worlds import build_world
    from cmbpo_amd import synthetic
    # the row count decides the path of cmbpo_rollout_run: one case on each side of the threshold
    assert (B <= hip_lib.cmbpo_rollout_book_pre_max_rows()) == (B == 1000)
    task = "HalfCheetahSafe-v2"
    w = build_world(77, task, 128)
    start = synthetic.start_states(np.random.default_rng(78), B, task)
    loop = _rollout(w, task, B, T, start, True, False)
    many = _rollout(w, task, B, T, start, True, True)
    again = _rollout(w, task, B, T, start, True, True)
    det = _rollout(w, task, B, T, start, False, True)
    # (the horizon rule finishes every branch after max_path_length - 1 stored steps, model_sampler.py:350-353)
    assert loop[0] == many[0] == again[0] and loop[0][0] == T - 1, (loop[0], many[0], again[0])
    assert loop[2] >= 2 and T - 1 > loop[3], "the rollout crosses a chunk boundary"
    for k, a, b, c in zip(NAMES, loop[1], many[1], again[1]):
        np.testing.assert_array_equal(a, b, err_msg=k)           # cmbpo_rollout_run == a loop of steps, bit for bit
        np.testing.assert_array_equal(b, c, err_msg=k)           # one seed, one rollout
    assert det[0][0] == T - 1 and not np.array_equal(det[1][0], many[1][0])        # the observations differ with the switch on


def test_first_step_moves_by_the_elites_std_times_the_draw(hip_lib):
    """One step of a stochastic and of a deterministic sampler with one seed: same actions, same elite picks, and every
    next observation of the former is (mean_elite + std_elite * xi) + obs of the sampler's own chunk, bit for bit."""
    _need_gpu()
    from test_rollout_sampler_gpu import hip_world
    from worlds import build_world
    from cmbpo_amd import synthetic
    task, B, T = "AntSafe-v2", 1000, 4
    w = build_world(77, task, 128, q_boost=1.2)
    D = w["obs_dim"]
    start = synthetic.start_states(np.random.default_rng(78), B, task)
    got = {}
    for stochastic in (False, True):
        sampler, pool = hip_world(w, task, T, "schedule", float("inf"), B, 128)
        sampler.stochastic = stochastic
        sampler._gen.manual_seed(5)
        sampler.reset(start)
        nxt, _, _, _ = sampler.sample()
        ck = sampler._draws
        got[stochastic] = dict(next_obs=nxt.cpu().numpy().copy(), mean=sampler._scratch[0].cpu().numpy(),
                               var=sampler._scratch[1].cpu().numpy(), eps=ck[1][0].cpu().numpy(), inds=ck[2][0].cpu().numpy(),
                               xi=None if ck[3] is None else ck[3][0].cpu().numpy(), act=pool.t["act_t"].cpu().numpy().copy())
    d, s = got[False], got[True]
    assert d["xi"] is None and s["xi"].shape == (B, D) and abs(float(s["xi"].std()) - 1.0) < 0.05
    for k in ("eps", "inds", "mean", "var"):
        np.testing.assert_array_equal(d[k].view(np.uint8), s[k].view(np.uint8), err_msg=k)     # the same draws before xi
    rows = np.arange(B)
    mean_e, std_e = s["mean"][s["inds"], rows, :D], np.sqrt(s["var"][s["inds"], rows, :D])
    np.testing.assert_array_equal(bits(d["next_obs"]), bits(mean_e + start))
    np.testing.assert_array_equal(bits(s["next_obs"]), bits((mean_e + std_e * s["xi"]) + start))
    assert (bits(s["next_obs"]) != bits(d["next_obs"])).mean() > 0.9


def test_fake_env_step_takes_noise_as_numpy_and_as_tensors(hip_lib):
    _need_gpu()
    from test_rollout_sampler_gpu import hip_world
    from worlds import build_world
    from cmbpo_amd import synthetic
    task, n = "AntSafe-v2", 50
    w = build_world(31, task, 128, q_boost=1.2)
    sampler, _ = hip_world(w, task, 4, "schedule", float("inf"), n, 128)
    env = sampler.env
    rng = np.random.default_rng(32)
    obs = synthetic.start_states(rng, n, task)
    act = rng.uniform(-1, 1, (n, w["act_dim"])).astype(np.float32)
    xi = rng.standard_normal((n, w["obs_dim"])).astype(np.float32)
    inds = np.asarray(w["elites"], np.int32)[rng.integers(0, len(w["elites"]), n)]
    a = env.step(obs, act, model_inds=inds, noise=xi)
    dev = torch.device("cuda:0")
    b = env.step(torch.from_numpy(obs).to(dev), torch.from_numpy(act).to(dev), model_inds=inds, noise=torch.from_numpy(xi).to(dev))
    det = env.step(obs, act, model_inds=inds)
    assert isinstance(a[0], np.ndarray) and isinstance(b[0], torch.Tensor) and b[0].is_cuda
    np.testing.assert_array_equal(bits(a[0]), bits(b[0].cpu().numpy()))
    np.testing.assert_array_equal(bits(a[1]), bits(b[1].cpu().numpy()))
    np.testing.assert_array_equal(a[2], b[2].cpu().numpy())
    for k in ("cost", "ensemble_dkl_path", "ensemble_ep_var"):
        np.testing.assert_array_equal(np.asarray(a[3][k], np.float32).view(np.uint32),
                                      np.asarray(b[3][k].cpu().numpy(), np.float32).view(np.uint32), err_msg=k)
    assert (bits(a[0]) != bits(det[0])).mean() > 0.9
    np.testing.assert_array_equal(bits(a[1]), bits(det[1]))           # rewards: unperturbed
    # a single row is squeezed like the reference's
    one = env.step(obs[3], act[3], model_inds=inds[3:4], noise=xi[3])
    assert one[0].shape == (w["obs_dim"],) and one[1].shape == (1,) and one[2].shape == (1,)
    np.testing.assert_array_equal(bits(one[0]), bits(a[0][3]))
    with pytest.raises(ValueError, match="noise"):
        env.step(obs, act, model_inds=inds, noise=xi[:, :-1])
    with pytest.raises(NotImplementedError, match="noise=np.ones"):
        env.step(obs, act, deterministic=False)


def test_cmbpo_runs_epochs_with_stochastic_transitions(hip_lib):
    _need_gpu()
    import toyworld
    from cmbpo_amd import synthetic
    from cmbpo_amd.cmbpo import CMBPO
    from cmbpo_amd.cpo_policy import CPOPolicy
    from cmbpo_amd.cpo_sampler import CpoSampler
    from cmbpo_amd.cpobuffer import CPOBuffer
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
    algo = CMBPO(env, policy, buf, sampler=CpoSampler(max_path_length=T), task="default", n_env_interacts=10 ** 9,
                 eval_every_n_steps=1, m_train_freq=100, m_networks=4, m_elites=3, m_hidden_dims=(128, 128),
                 rollout_batch_size=400, rollout_mode="schedule", rollout_schedule=[0, 1, 4, 4], maxroll=6,
                 initial_real_samples_per_epoch=150, min_real_samples_per_epoch=100, batch_size_policy=2500,
                 n_initial_exploration_steps=300, n_epochs=50,
                 initial_model_train_kwargs=dict(min_epochs=3, max_epochs=6, batch_size=128),
                 model_train_kwargs=dict(min_epochs=1, max_epochs=2, batch_size=128), m_stochastic=True)
    assert algo.model_sampler.stochastic is True
    chunks = []
    draw = algo.model_sampler._draw_chunk
    algo.model_sampler._draw_chunk = lambda: chunks.append(draw()) or chunks[-1]
    diags = []
    for d in algo.train():
        diags.append(d)
        if len(diags) >= 2:
            break
    assert len(diags) == 2
    assert chunks and all(ck[3] is not None and ck[3].shape[2] == D for ck in chunks)       # the rollouts drew transition noise
    for first in diags:
        assert first["model/samples_added"] > 0
        for k, v in first.items():
            if isinstance(v, (float, np.floating)):
                assert np.isfinite(v) or k.startswith("model/max") or "Min" in k or "Max" in k, k
