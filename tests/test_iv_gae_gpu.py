"""GPU: the inverse-variance-weighted GAE of the device-resident ModelBuffer / ModelSampler (``iv_gae=True``) against
  (a) the reference's own ModelBuffer / ModelSampler run with the weighted branch of its discount_cumsum switched on
      (tests/golden/g17_iv_buffer.npz, g17_trace_iv_*.npz; tests/golden/make_golden_iv_gae.py), and
  (b) the NumPy restatement tests/iv_gae_ref.py (held against the reference bit for bit by tests/test_iv_gae_cpu.py).
ret / cret are float32 casts of one float64 recurrence whose operations the kernel takes in the reference's order: at
most 1 float32 ulp apart, bit-equal expected (the count of unequal elements is printed).  adv / cadv pass through the
normalisation of get(): rtol 1e-5, atol 1e-6, as in test_modelbuffer_api_parity_with_host_arrays."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import iv_gae_ref as ref  # noqa: E402
from oracle import refcpu  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
GAMMAS = dict(gamma=0.99, lam=0.95, cost_gamma=0.97, cost_lam=0.5)
STEP_KEYS = ("obs", "act", "rew", "val", "cost", "cval", "dyn_error", "logp", "mu", "log_std")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _variances(rng, shape):
    v = (10.0 ** rng.uniform(-12, 2, shape)).astype(np.float32)
    v[rng.random(shape) < 0.125] = 0.0
    return v


def _make_schedule(rng, B, T, D, A):
    """The ragged schedule of test_modelbuffer_api_parity_with_host_arrays by branch slot: finishes before any store,
    mid-way with float32 and with float64-zero bootstraps, at the end."""
    step = {k: rng.standard_normal((T, B)).astype(np.float32) for k in ("rew", "val", "cost", "cval", "logp")}
    step["dyn_error"] = _variances(rng, (T, B))
    step["obs"] = rng.standard_normal((T, B, D)).astype(np.float32)
    for k in ("act", "mu", "log_std"):
        step[k] = rng.standard_normal((T, B, A)).astype(np.float32)
    alive = np.ones(B, bool)
    ev = dict(step=[], mask=[], zero=[], lv=[], lcv=[])

    def event(t, mask, zero):
        ev["step"].append(t); ev["mask"].append(mask); ev["zero"].append(zero)
        ev["lv"].append(rng.standard_normal(B).astype(np.float32))
        ev["lcv"].append(rng.standard_normal(B).astype(np.float32))
        alive[mask] = False

    first = np.zeros(B, bool)
    first[[1, 5, B - 1]] = True
    event(-1, first, False)
    for t in range(T - 1):
        m = alive & (rng.random(B) < 0.25)
        if m.any():
            event(t, m, t % 2 == 1)
    event(T - 1, alive.copy(), False)
    return step, {k: np.array(v) for k, v in ev.items()}


def _drive(buf, step, ev, T):
    """The events and steps through store_multiple / finish_path_multiple in the reference's compact (alive-only) order."""
    B = step["rew"].shape[1]
    alive = np.ones(B, bool)

    def fire(t):
        for e in np.flatnonzero(ev["step"] == t):
            idx = np.flatnonzero(alive)
            tm = ev["mask"][e][idx]
            sel = idx[tm]
            lv = np.zeros(len(sel)) if ev["zero"][e] else ev["lv"][e][sel]
            buf.finish_path_multiple(tm, lv, ev["lcv"][e][sel])
            alive[sel] = False

    fire(-1)
    for t in range(T):
        idx = np.flatnonzero(alive)
        s = {k: step[k][t, idx] for k in STEP_KEYS}
        buf.store_multiple(s["obs"], s["act"], s["obs"], s["rew"], s["val"], s["cost"], s["cval"], s["dyn_error"], s["logp"],
                           {"mu": s["mu"], "log_std": s["log_std"]}, np.zeros(len(idx), bool))
        fire(t)
        np.testing.assert_array_equal(buf.alive_paths, alive)
    return buf.get()


def _expected(step, ev, T, iv_eps):
    """get() of the schedule by tests/iv_gae_ref.py: [obs, act, adv, cadv, ret, cret, logp, val, cval, cost, log_std, mu]."""
    B = step["rew"].shape[1]
    adv = np.zeros((B, T), np.float32); ret = adv.copy(); cadv = adv.copy(); cret = adv.copy()
    length = np.zeros(B, int)
    for e, t in enumerate(ev["step"]):
        rows, L = np.flatnonzero(ev["mask"][e]), int(t) + 1
        length[rows] = L
        if L == 0:
            continue
        w = ref.iv_weights(step["dyn_error"][:L, rows].T, iv_eps)
        lv = np.zeros(len(rows)) if ev["zero"][e] else ev["lv"][e][rows]
        adv[rows, :L], ret[rows, :L] = ref.iv_gae_rows(step["rew"][:L, rows].T, step["val"][:L, rows].T, lv,
                                                       GAMMAS["gamma"], GAMMAS["lam"], w)
        cadv[rows, :L], cret[rows, :L] = ref.iv_gae_rows(step["cost"][:L, rows].T, step["cval"][:L, rows].T, ev["lcv"][e][rows],
                                                         GAMMAS["cost_gamma"], GAMMAS["cost_lam"], w)
    mask = np.arange(T)[None] < length[:, None]
    m, s = refcpu.mpi_statistics_scalar(adv[mask])
    cm, _ = refcpu.mpi_statistics_scalar(cadv[mask])
    flat = lambda k: np.swapaxes(step[k], 0, 1)[mask]
    return [flat("obs"), flat("act"), (adv[mask] - m) / (s + 1e-8), cadv[mask] - cm, ret[mask], cret[mask], flat("logp"),
            flat("val"), flat("cval"), flat("cost"), flat("log_std"), flat("mu")]


def _compare(res, want, tag):
    from test_rollout_sampler_gpu import NAMES
    for k, a, b in zip(NAMES, res, want):
        assert a.shape == b.shape, k
        if k in ("ret", "cret"):
            print(f"{tag}: {k}: {int((a != b).sum())} of {a.size} elements differ from the reference")
            np.testing.assert_array_max_ulp(a, b.astype(np.float32), maxulp=1)
        elif k in ("adv", "cadv"):
            np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=k)
        else:
            np.testing.assert_array_equal(a, b, err_msg=k)        # copies, branch-major / time-minor order


def test_buffer_replays_the_reference_with_weighted_gae(hip_lib):
    """(1) g17_iv_buffer through store_multiple / finish_path_multiple / get at B = 37."""
    _need_gpu()
    from test_rollout_sampler_gpu import NAMES
    from cmbpo_amd.modelbuffer import ModelBuffer
    g = np.load(os.path.join(GOLD, "g17_iv_buffer.npz"), allow_pickle=False)
    B, T, D, A = int(g["B"]), int(g["T"]), int(g["D"]), int(g["A"])
    buf = ModelBuffer(B, D, A, T, device="cuda:0", iv_gae=True, iv_eps=float(g["iv_eps"]))
    buf.initialize({"mu": [A], "log_std": [A]}, **{k: float(g[k]) for k in GAMMAS})
    assert buf.iv_gae and tuple(buf.t["cumvar_buf"].shape) == (T, B) and buf.t["cumvar_buf"].dtype == torch.float64
    step = {k: g["step_" + k] for k in STEP_KEYS}
    ev = {k: g["ev_" + k] for k in ("step", "mask", "zero", "lv", "lcv")}
    res, diag = _drive(buf, step, ev, T)
    want = [g["get_" + k] for k in NAMES]
    assert diag["poolm_batch_size"] == int(g["poolm_batch_size"])
    _compare(res, want, "g17_iv_buffer")
    # the checker on the same schedule: the reference's ret / cret bit for bit
    chk = _expected(step, ev, T, float(g["iv_eps"]))
    np.testing.assert_array_equal(chk[4], g["get_ret"])
    np.testing.assert_array_equal(chk[5], g["get_cret"])
    # get() resets; the feature stays on
    assert buf.alive_paths.all() and buf.size == 0 and buf.ptr == 0 and buf.iv_gae


@pytest.mark.parametrize("iv_eps", [1e-8, 1e-2])
def test_large_buffer_matches_the_restatement(hip_lib, iv_eps):
    """(2) the same kind of schedule at B = 1500 (many workgroups of store_kernel / finish_kernel), T = 5."""
    _need_gpu()
    from cmbpo_amd.modelbuffer import ModelBuffer
    B, T, D, A = 1500, 5, 5, 2
    step, ev = _make_schedule(np.random.default_rng(171), B, T, D, A)
    assert ev["zero"].any() and not ev["zero"].all() and len(ev["step"]) >= 4
    buf = ModelBuffer(B, D, A, T, device="cuda:0")
    buf.initialize({"mu": [A], "log_std": [A]}, **GAMMAS)
    buf.set_iv_gae(True, iv_eps=iv_eps)
    res, _ = _drive(buf, step, ev, T)
    _compare(res, _expected(step, ev, T, iv_eps), f"B=1500 iv_eps={iv_eps}")
    # column u of cumvar_buf: the float64 running sum of the stored variances, in time order
    L = ev["step"][np.argmax(ev["mask"], axis=0)] + 1
    cum = np.cumsum(step["dyn_error"].astype(np.float64), axis=0)
    got = buf.t["cumvar_buf"].cpu().numpy()
    m = np.arange(T)[:, None] < L[None]
    np.testing.assert_array_equal(got[m], cum[m])


@pytest.mark.parametrize("name", ["g17_trace_iv_ant_term", "g17_trace_iv_hcs_sched"])
@pytest.mark.parametrize("ens_path", [0, 1, 2], indirect=True, ids=["fp32mfma", "splitbf16", "splitf16"])
def test_sampler_replays_the_reference_traces_with_weighted_gae(hip_lib, ens_path, name):
    """(3) the reference's ModelSampler over its ModelBuffer with the weighted discount_cumsum, replayed with sample();
    the tolerances are test_hip_sampler_reproduces_reference_trace's.  At least a quarter of the recorded adv and cadv
    differ from the un-weighted run's by ten times these tolerances (asserted by the generator): a replay that ignored
    the switch could not pass."""
    _need_gpu()
    from test_rollout_sampler_gpu import NAMES, TOL, hip_world
    from worlds import build_world
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    assert float(g["changed_adv"]) >= 0.25 and float(g["changed_cadv"]) >= 0.25
    task, B, T, hidden = str(g["task"]), int(g["B"]), int(g["T"]), int(g["hidden"])
    w = build_world(int(g["seed"]), task, hidden, out_scale=float(g["out_scale"]), q_boost=float(g["q_boost"]))
    sampler, pool = hip_world(w, task, T, str(g["mode"]), float(g["dkl_lim"]), B, hidden)
    pool.set_iv_gae(True, iv_eps=float(g["iv_eps"]))
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
        want = g["get_" + k]
        assert arr.shape == want.shape and arr.dtype == want.dtype, k
        if TOL[k] == 0.0:
            np.testing.assert_array_equal(arr, want, err_msg=k)
        else:
            np.testing.assert_allclose(arr, want, rtol=TOL[k], atol=TOL[k], err_msg=k)
    np.testing.assert_allclose(bdiag["poolm_ret_mean"], float(g["poolm_ret_mean"]), rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(bdiag["poolm_cret_mean"], float(g["poolm_cret_mean"]), rtol=2e-3, atol=2e-4)
    for k in ("msampler/samples_added", "msampler/rollout_H_max"):
        assert diag[k] == float(g["diag_" + k.replace("/", "__")])


def _rollout(w, task, B, T, start, lim, many, switch):
    """One rollout of a fresh sampler; switch: the set_iv_gae calls made on its buffer before the rollout."""
    from test_rollout_sampler_gpu import hip_world
    sampler, pool = hip_world(w, task, T, "uncertainty", lim, B, 128)
    for on in switch:
        pool.set_iv_gae(on)
    sampler._gen.manual_seed(5)
    sampler.reset(start)
    steps = 0
    if many:
        steps, _ = sampler.sample_many()
    else:
        while sampler.any_alive() and pool.has_room:
            sampler.sample()
            steps += 1
    state = (steps, pool.n_alive, pool.ptr, sampler._total_samples)
    sampler.finish_all_paths()
    res, _ = pool.get()
    return state, res, pool


@pytest.fixture(scope="module")
def ant_world():
    from worlds import build_world
    return build_world(77, "AntSafe-v2", 128, q_boost=1.2)


def _limit(w, task, B, T, start):
    """A limit some branches exceed: 2.5 x the median DKL of the first step (test_sample_many_equals_a_loop_of_sample)."""
    from test_rollout_sampler_gpu import hip_world
    cal, _ = hip_world(w, task, T, "uncertainty", float("inf"), B, 128)
    cal._gen.manual_seed(5)
    cal.reset(start)
    _, _, _, info = cal.sample()
    return 2.5 * float(np.median(info["ensemble_dkl_path"].cpu().numpy()[:B]))


@pytest.mark.parametrize("B", [300, 1500])     # one-workgroup bookkeeping with the look-ahead run loop / separate kernels
def test_sample_many_equals_a_loop_of_sample_and_off_is_off(hip_lib, ant_world, B):
    """(4) cmbpo_rollout_run == a loop of cmbpo_rollout_step with the feature on, bit for bit; (5) a buffer switched on and
    off again == a buffer never switched, bit for bit, and its cumvar_buf is gone."""
    _need_gpu()
    from test_rollout_sampler_gpu import NAMES
    from cmbpo_amd import synthetic
    assert (B <= hip_lib.cmbpo_rollout_book_pre_max_rows()) == (B == 300)
    task, T = "AntSafe-v2", 6
    start = synthetic.start_states(np.random.default_rng(78), B, task)
    lim = _limit(ant_world, task, B, T, start)
    loop = _rollout(ant_world, task, B, T, start, lim, False, [True])
    many = _rollout(ant_world, task, B, T, start, lim, True, [True])
    never = _rollout(ant_world, task, B, T, start, lim, True, [])
    onoff = _rollout(ant_world, task, B, T, start, lim, True, [True, False])
    assert loop[0] == many[0] == never[0] == onoff[0] and loop[0][0] >= 2, (loop[0], many[0], never[0], onoff[0])
    assert loop[2].iv_gae and "cumvar_buf" in loop[2].t and many[2].iv_gae
    assert not onoff[2].iv_gae and "cumvar_buf" not in onoff[2].t and "iv_tables" not in onoff[2].t
    assert not never[2].iv_gae and "cumvar_buf" not in never[2].t
    for k, a, b, c, d in zip(NAMES, loop[1], many[1], never[1], onoff[1]):
        np.testing.assert_array_equal(a, b, err_msg=k)
        np.testing.assert_array_equal(c, d, err_msg=k)
    # the switch does something: same samples, other advantages
    np.testing.assert_array_equal(many[1][0], never[1][0])
    # (the weighted value of a sample is another float64 expression unless its branch has one step: other float32 bits;
    # how far the values move is the replays' business, this only shows that the switch reaches the kernels)
    for i in (2, 3, 4, 5):
        assert np.mean(many[1][i] != never[1][i]) > 0.25, NAMES[i]


def test_error_handling(hip_lib):
    """(6)"""
    _need_gpu()
    from cmbpo_amd import _lib
    from cmbpo_amd.modelbuffer import ModelBuffer
    for bad in (0, 0.0, -1e-8, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="iv_eps"):
            ModelBuffer(8, 3, 2, 4, device="cuda:0", iv_gae=True, iv_eps=bad)
    buf = ModelBuffer(8, 3, 2, 4, device="cuda:0")
    buf.initialize({"mu": [2], "log_std": [2]}, **GAMMAS)
    with pytest.raises(ValueError, match="iv_eps"):
        buf.set_iv_gae(True, iv_eps=0)
    assert not buf.iv_gae
    buf.set_iv_gae(True)
    tabs = buf.t["iv_tables"]
    iv = _lib.IvGaeStruct()
    iv.cumvar_buf, iv.eps = buf.t["cumvar_buf"].data_ptr(), 1e-8
    iv.lam_vec = iv.lam_pow = iv.clam_vec = tabs.data_ptr()           # clam_pow stays NULL
    assert hip_lib.cmbpo_rollout_iv_attach(C.byref(buf.rs), C.byref(iv)) == -1
    msg = hip_lib.cmbpo_last_error()
    assert b"cmbpo_rollout_iv_attach" in msg and b"NULL" in msg, msg
    with pytest.raises(_lib.CmbpoHipError, match="cmbpo_rollout_iv_attach"):
        _lib.check(-1, "cmbpo_rollout_iv_attach")
    # the failed call left the buffer's own entry alone; the switch is refused while samples are stored
    n = 8
    z = lambda *s: np.zeros((n,) + s, np.float32)
    buf.store_multiple(z(3), z(2), z(3), z(), z(), z(), z(), np.full(n, 0.5, np.float32), z(), {"mu": z(2), "log_std": z(2)},
                       np.zeros(n, bool))
    np.testing.assert_array_equal(buf.t["cumvar_buf"][0].cpu().numpy(), np.full(n, 0.5))
    with pytest.raises(RuntimeError, match="set_iv_gae"):
        buf.set_iv_gae(False)
    buf.finish_path_multiple(np.ones(n, bool), z(), z())
    buf.get()
    buf.set_iv_gae(False)
    assert "cumvar_buf" not in buf.t


def test_cmbpo_runs_epochs_with_weighted_gae(hip_lib):
    """(7) two epochs on the toy world of test_cmbpo_runs_epochs_with_stochastic_transitions."""
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
                 model_train_kwargs=dict(min_epochs=1, max_epochs=2, batch_size=128), m_iv_gae=True, m_iv_eps=1e-6)
    mb = algo.model_buf
    assert mb.iv_gae is True and mb.iv_eps == 1e-6 and tuple(mb.t["cumvar_buf"].shape) == (6, mb.capacity)
    vec, pw = mb.t["iv_tables"].cpu().numpy()[:6], mb.t["iv_tables"].cpu().numpy()[6:13]
    np.testing.assert_array_equal(vec, ref.lam_tables(policy.lam, 6)[0])       # the tables follow initialize()'s lambdas
    np.testing.assert_array_equal(pw, ref.lam_tables(policy.lam, 6)[1])
    diags = []
    for d in algo.train():
        diags.append(d)
        if len(diags) >= 2:
            break
    assert len(diags) == 2 and algo.model_buf.iv_gae is True
    assert float(algo.model_buf.t["cumvar_buf"].max()) > 0                      # the rollouts wrote their variances
    for first in diags:
        assert first["model/samples_added"] > 0
        for k, v in first.items():
            if isinstance(v, (float, np.floating)):
                assert np.isfinite(v) or k.startswith("model/max") or "Min" in k or "Max" in k, k
