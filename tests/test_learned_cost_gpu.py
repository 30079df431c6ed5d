"""GPU: the learned cost head (algorithms/cmbpo.py:46,123 m_learn_cost; models/fake_env.py:139-151 predicts_cost) through
every layer -- the post kernel's learned-cost mode against its own rule mode and NumPy, golden traces G14 recorded from the
REFERENCE's FakeEnv(..., True, True, True) + ModelSampler + ModelBuffer on all three matrix paths, the native rollout loop,
the ensemble forward and training step at the widths the extra column gives (62 / 44 raw outputs), the FakeEnv host API,
a checkpoint round trip, the trainer closed loop on a point environment, and the sharded sampler.

Tolerances are those of the files these tests extend (test_rollout_kernels_gpu.py, test_rollout_sampler_gpu.py,
test_ens_train_gpu.py); the predicted cost of a trace is a continuous value and is compared like `ret` / `val`
(rtol = atol = 2e-3), where the rule costs of G5 are masks and compared exactly.
"""
import os
import socket
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import refcpu  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, GOLD)
NAMES = ["obs", "act", "adv", "cadv", "ret", "cret", "logp", "val", "cval", "cost", "log_std", "mu"]
TOL = dict(obs=2e-3, act=2e-3, adv=5e-3, cadv=2e-3, ret=2e-3, cret=2e-3, logp=2e-3, val=2e-3, cval=2e-3,
           cost=2e-3, log_std=0.0, mu=2e-3)
TRACES = ["g14_trace_cost_hopper_budget", "g14_trace_cost_ant_term", "g14_trace_cost_hcs_sched", "g14_trace_cost_ant_unc"]


class _Space:
    def __init__(self, d):
        self.shape = (d,)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def hip_world_cost(w, task, T, mode, dkl_lim, B, hidden, comm=None):
    """test_rollout_sampler_gpu.hip_world with an obs + 2 model and FakeEnv(predicts_cost=True)."""
    from cmbpo_amd.cpo_policy import CPOPolicy
    from cmbpo_amd.fake_env import FakeEnv
    from cmbpo_amd.model_sampler import ModelSampler
    from cmbpo_amd.modelbuffer import ModelBuffer
    from cmbpo_amd.pens import PE
    D, A = w["obs_dim"], w["act_dim"]
    E = w["ws"][0].shape[0]
    model = PE(D + A, D + 2, hidden_dims=(hidden, hidden), num_networks=E, num_elites=len(w["elites"]),
               loss="MSPE", use_scaler_in=True, use_scaler_out=True, device="cuda:0")
    model.set_weights(w["ws"], w["bs"], w["sc_in"], w["sc_out"])
    model.set_elites(w["elites"])
    policy = CPOPolicy(_Space(D), _Space(A), a_hidden_layer_sizes=(128, 128), vf_hidden_layer_sizes=(128, 128),
                       vf_ensemble_size=3, vf_elites=2, vf_activation="swish", vf_loss="MSE", device="cuda:0",
                       cost_gamma=0.97, cost_lam=0.5, lam=0.95, comm=comm)
    policy.actor.set_params(w["pol"])
    policy.v.set_weights(*w["v"])
    policy.vc.set_weights(*w["vc"])

    class _Env:
        observation_space, action_space = _Space(D), _Space(A)

    env = FakeEnv(_Env(), task, model, predicts_delta=True, predicts_rew=True, predicts_cost=True)
    pool = ModelBuffer(B, D, A, T, device="cuda:0", comm=comm)
    pool.initialize(policy.pi_info_shapes, gamma=0.99, lam=0.95, cost_gamma=0.97, cost_lam=0.5)
    sampler = ModelSampler(max_path_length=T, batch_size=B, rollout_mode=mode, comm=comm)
    sampler.initialize(env, policy, pool)
    sampler.set_rollout_dkl(dkl_lim)
    return sampler, pool


# ------------------------------------------------------------------------------------------------------------------
# the post kernel
# ------------------------------------------------------------------------------------------------------------------
def _run_post(task_arg, obs, act, mean, var, inds, obs_dim, act_dim, row_idx=None, expect_rc=0):
    """cmbpo_fakeenv_post on slot-indexed arrays ([B, .] / [E, B, .]); with row_idx only the listed slots are stepped."""
    from cmbpo_amd import _lib
    dev = torch.device("cuda:0")
    B, E = obs.shape[0], mean.shape[0]
    n = B if row_idx is None else len(row_idx)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    f = dict(dtype=torch.float32, device=dev)
    out = dict(next_obs=torch.full((B, obs_dim), -7.0, **f), rew=torch.full((B,), -7.0, **f),
               term=torch.full((B,), 77, dtype=torch.uint8, device=dev), cost=torch.full((B,), -7.0, **f),
               dkl_path=torch.full((B,), -7.0, **f), ep_var_mean=torch.full((B,), -7.0, **f),
               ep_var=torch.full((B, obs_dim), -7.0, **f))
    d = [t(obs), t(act), t(mean), t(var), t(inds)]
    ri = None if row_idx is None else t(np.asarray(row_idx, np.int32))
    rc = _lib.lib().cmbpo_fakeenv_post(
        task_arg, E, obs_dim, act_dim, _lib.ptr(d[2]), _lib.ptr(d[3]), B,
        _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[4]), _lib.ptr(ri), None, n,
        _lib.ptr(out["next_obs"]), _lib.ptr(out["rew"]), _lib.ptr(out["term"]), _lib.ptr(out["cost"]),
        _lib.ptr(out["dkl_path"]), _lib.ptr(out["ep_var_mean"]), _lib.ptr(out["ep_var"]),
        _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == expect_rc, (rc, _lib.lib().cmbpo_last_error())
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("E", [7, 5, 3])     # the kernel is compiled for 7 and 5 members; any other size at run time
@pytest.mark.parametrize("task", ["AntSafe-v2", "HalfCheetahSafe-v2", "HopperSafe-v2"])
@pytest.mark.parametrize("n,listed", [(13, False), (1001, False), (1001, True), (29, True)])     # no multiple of 8
def test_post_kernel_learned_cost_mode(hip_lib, task, n, listed, E):
    """Mode on over (mean, var)[E, n, obs + 2] == mode off over the contiguous [..., :obs + 1] copy, bit for bit, in everything
    but the cost; the cost is the elite member's mean of column obs + 1 as it is, NaN / inf included."""
    _need_gpu()
    from cmbpo_amd import _lib, synthetic
    rng = np.random.default_rng(zlib.crc32(f"{task}/{n}/{listed}/{E}/learned".encode()))
    D, A = synthetic.ENV_DIMS[task]
    B = n + 11 if listed else n
    obs = synthetic.start_states(rng, B, task)
    act = rng.uniform(-1, 1, (B, A)).astype(np.float32)
    mean = (rng.standard_normal((E, B, D + 2)) * 0.3).astype(np.float32)
    var = np.exp(rng.uniform(-12, 1, (E, B, D + 2))).astype(np.float32)
    var[:, ::7, 3] = 0.0
    inds = rng.integers(0, E, size=B).astype(np.int32)
    rows = np.sort(rng.choice(B, size=n, replace=False)).astype(np.int32) if listed else None
    live = np.arange(B) if rows is None else rows
    if task == "AntSafe-v2":
        mean[:, live[2], 2] = 2.0          # z_rot << -0.7 with z inside the gate: the static termination fires
        obs[live[2], 0] = 0.5
        mean[:, live[2], 0] = 0.0
        mean[:, live[5], D - 1] = 10.0     # where the AntSafe cost rule would say 1
    # non-finite predictions: in the cost column (the elite's and another member's), in an obs column, in the cost variance
    mean[:, live[3], D + 1] = np.nan
    mean[inds[live[4]], live[4], D + 1] = np.inf
    mean[(inds[live[6]] + 1) % E, live[6], D + 1] = np.nan      # another member's: must not reach this branch
    mean[inds[live[7]], live[7], D + 1] = -np.inf
    mean[1, live[8], 5] = np.nan
    mean[:, live[9], 1] = np.inf
    var[:, live[10], D + 1] = np.nan
    base = _lib.TASK_IDS.get(task, 0)
    on = _run_post(base | _lib.TASK_LEARNED_COST, obs, act, mean, var, inds, D, A, rows)
    off = _run_post(base, obs, act, np.ascontiguousarray(mean[..., :D + 1]), np.ascontiguousarray(var[..., :D + 1]), inds,
                    D, A, rows)
    for k in ("next_obs", "rew", "dkl_path", "ep_var_mean", "ep_var"):
        np.testing.assert_array_equal(_bits(on[k]), _bits(off[k]), err_msg=k)
    np.testing.assert_array_equal(on["term"], off["term"])
    want = mean[inds[live], live, D + 1]
    np.testing.assert_array_equal(_bits(on["cost"][live]), _bits(want))
    assert np.isnan(on["cost"][live[3]]) and on["cost"][live[4]] == np.inf and on["cost"][live[7]] == -np.inf
    assert np.isfinite(on["cost"][live[6]])
    np.testing.assert_array_equal(on["rew"][live], mean[inds[live], live, D])
    if task == "AntSafe-v2":
        assert on["term"][live[2]] == 1 and off["cost"][live[2]] == 1.0 and off["cost"][live[5]] == 1.0
    if rows is not None:
        rest = np.setdiff1d(np.arange(B), rows)
        assert (on["cost"][rest] == -7.0).all() and (on["term"][rest] == 77).all() and (on["next_obs"][rest] == -7.0).all()


def test_post_kernel_rejects_bad_task_flags(hip_lib):
    _need_gpu()
    from cmbpo_amd import _lib
    rng = np.random.default_rng(3)
    D, A, E, n = 20, 6, 5, 9
    obs = rng.standard_normal((n, D)).astype(np.float32)
    act = rng.standard_normal((n, A)).astype(np.float32)
    mean = rng.standard_normal((E, n, D + 2)).astype(np.float32)
    var = np.ones_like(mean)
    inds = np.zeros(n, np.int32)
    F = _lib.TASK_LEARNED_COST
    assert F == 0x100
    for bad in (9, F | 9, F | 3, 0x200, 0x200 | F, 0x80 | F, 0x1000, -1, F << 1 | 1):
        _run_post(bad, obs, act, mean, var, inds, D, A, expect_rc=-1)
        assert len(hip_lib.cmbpo_last_error()) > 10
    for good in (F | 0, F | 1):
        _run_post(good, obs, act, mean, var, inds, D, A)
    _run_post(F | 2, obs, act, mean[..., :7], var[..., :7], inds, 5, A)        # AntSafe rules need obs_dim >= 5
    _run_post(F | 2, obs, act, mean[..., :6], var[..., :6], inds, 4, A, expect_rc=-1)


# ------------------------------------------------------------------------------------------------------------------
# golden traces
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TRACES)
@pytest.mark.parametrize("ens_path", [0, 1, 2], indirect=True, ids=["fp32mfma", "splitbf16", "splitf16"])
def test_hip_sampler_reproduces_reference_trace_with_learned_cost(hip_lib, ens_path, name):
    _need_gpu()
    from worlds_learned_cost import build_world_learned_cost
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    task, B, T, hidden = str(g["task"]), int(g["B"]), int(g["T"]), int(g["hidden"])
    w = build_world_learned_cost(int(g["seed"]), task, hidden, out_scale=float(g["out_scale"]), q_boost=float(g["q_boost"]))
    sampler, pool = hip_world_cost(w, task, T, str(g["mode"]), float(g["dkl_lim"]), B, hidden)
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
            np.testing.assert_array_equal(arr, ref, err_msg=k)
        else:
            np.testing.assert_allclose(arr, ref, rtol=TOL[k], atol=TOL[k], err_msg=k)
    assert float(np.std(res[9])) >= 0.5                                       # a spread the tolerance means something against
    np.testing.assert_allclose(bdiag["poolm_ret_mean"], float(g["poolm_ret_mean"]), rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(bdiag["poolm_cret_mean"], float(g["poolm_cret_mean"]), rtol=2e-3, atol=2e-4)
    for k in ("msampler/samples_added", "msampler/rollout_H_max"):
        assert diag[k] == float(g["diag_" + k.replace("/", "__")])
    for k in ("msampler/rollout_H_mean", "msampler/dyn_var_perstep", "msampler/cost_rate", "msampler/rew_rate",
              "msampler/v_mean", "msampler/cv_mean", "msampler/ens_DKL", "msampler/max_path_return",
              "msampler/max_dkl"):
        np.testing.assert_allclose(diag[k], float(g["diag_" + k.replace("/", "__")]), rtol=5e-3, atol=1e-6,
                                   err_msg=k)


# ------------------------------------------------------------------------------------------------------------------
# the native loop
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,B,T,mode,lim_scale,budget,stop_frac,min_ratio", [
    ("AntSafe-v2", 1000, 12, "uncertainty", 2.5, 9000, None, None),        # one-workgroup bookkeeping + look-ahead, budget
    ("HopperSafe-v2", 1000, 9, "schedule", None, None, 0.5, 0.1),          # no rule at all, stop on the total
    ("HalfCheetahSafe-v2", 6000, 7, "uncertainty", 2.5, None, None, 0.1),  # > 4096 rows: separate bookkeeping calls + compaction
])
def test_sample_many_equals_a_loop_of_sample_with_learned_cost(hip_lib, task, B, T, mode, lim_scale, budget, stop_frac,
                                                               min_ratio):
    """cmbpo_rollout_run with the learned-cost flag takes exactly the steps a Python loop of sample() (cmbpo_rollout_step)
    takes: same stopping step, bit-identical buffers, and the costs in them are the model's."""
    _need_gpu()
    from worlds_learned_cost import build_world_learned_cost
    from cmbpo_amd import synthetic
    w = build_world_learned_cost(77, task, 128, q_boost=0.8 if task == "AntSafe-v2" else 0.0)
    start = synthetic.start_states(np.random.default_rng(78), B, task)
    stop_total = None if stop_frac is None else stop_frac * B * T
    out = []
    for many in (False, True):
        sampler, pool = hip_world_cost(w, task, T, mode, float("inf"), B, 128)
        if lim_scale is not None:
            cal, _ = hip_world_cost(w, task, T, mode, float("inf"), B, 128)
            cal._gen.manual_seed(5)
            cal.reset(start)
            _, _, _, info = cal.sample()
            sampler.set_rollout_dkl(lim_scale * float(np.median(info["ensemble_dkl_path"].cpu().numpy()[:B])))
        sampler._gen.manual_seed(5)
        sampler.reset(start)
        steps = 0
        if many:
            steps, info = sampler.sample_many(max_samples=budget, stop_total=stop_total, min_alive_ratio=min_ratio)
        else:
            while sampler.any_alive() and pool.has_room:
                _, _, _, info = sampler.sample(max_samples=budget)
                steps += 1
                if stop_total is not None and sampler._total_samples >= stop_total:
                    break
                if min_ratio is not None and info["alive_ratio"] <= min_ratio:
                    break
        state = (steps, pool.n_alive, pool.ptr, sampler._total_samples, info["alive_ratio"])
        diag = sampler.finish_all_paths()
        res, _ = pool.get()
        out.append((state, diag["msampler/samples_added"], res))
    assert out[0][0] == out[1][0], (out[0][0], out[1][0])
    assert out[0][0][0] >= 2
    assert out[0][1] == out[1][1]
    for k, a, b in zip(NAMES, out[0][2], out[1][2]):
        np.testing.assert_array_equal(a, b, err_msg=k)
    # The costs are the model's: each stored cost is an elite member's mean of column obs + 1 at the stored (obs, act), at
    # the traces' tolerance for a predicted cost.  (No bound on their spread here: within one member it is 0.04 - 0.09 for
    # these worlds, and the rest depends on how far the seed happens to put the elites' means apart.)
    obs, act, cost = out[1][2][0], out[1][2][1], out[1][2][9]
    assert cost.dtype == np.float32 and cost.shape == (len(obs),)
    mean, _ = refcpu.ens_forward(np.concatenate([obs, act], axis=1), w["ws"], w["bs"], w["sc_in"], w["sc_out"])
    pred = mean[w["elites"], :, w["obs_dim"] + 1]
    err = np.abs(pred - cost[None]) - 2e-3 * np.abs(pred)
    print(f"{task}: {len(cost)} samples, cost std {np.std(cost):.4f}, worst distance to an elite's prediction "
          f"{np.abs(pred - cost[None]).min(0).max():.3e}")
    assert (err.min(0) <= 2e-3).all()
    assert float(np.std(cost)) > 0.0 and not np.isin(cost, (0.0, 1.0)).all()


# ------------------------------------------------------------------------------------------------------------------
# forward and training at the new widths
# ------------------------------------------------------------------------------------------------------------------
def _wide_model(rng, I, O, E=7, hidden=512):
    from cmbpo_amd import synthetic
    from cmbpo_amd.pens import PE
    ws, bs = synthetic.ensemble_weights(rng, E, I, hidden, 2 * O, bias_scale=0.05)
    sc_in, sc_out = synthetic.scaler(rng, I), synthetic.scaler(rng, O)
    m = PE(I, O, hidden_dims=(hidden, hidden), num_networks=E, num_elites=5, loss="MSPE", use_scaler_in=True,
           use_scaler_out=True, device="cuda:0")
    m.set_weights(ws, bs, sc_in, sc_out)
    return m, ws, bs, sc_in, sc_out


@pytest.mark.parametrize("ens_path", [0, 1, 2], indirect=True, ids=["fp32mfma", "splitbf16", "splitf16"])
@pytest.mark.parametrize("I,O", [(37, 31), (26, 22)])         # AntSafe / HalfCheetahSafe with a cost column
@pytest.mark.parametrize("n", [1, 33, 257, 1200])
def test_ens_forward_with_a_cost_column_matches_oracle(hip_lib, ens_path, I, O, n):
    _need_gpu()
    rng = np.random.default_rng(zlib.crc32(f"{I}/{O}/{n}/cost".encode()))
    m, ws, bs, sc_in, sc_out = _wide_model(rng, I, O)
    x = rng.standard_normal((n, I)).astype(np.float32)
    mean, var = m.predict_ensemble(x)
    rmean, rvar = refcpu.ens_forward(x, ws, bs, sc_in, sc_out)
    assert mean.shape == rmean.shape == (7, n, O)
    np.testing.assert_allclose(mean, rmean, rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(var, rvar, rtol=2e-3, atol=1e-7)


def test_62_wide_model_takes_the_f16_forward(hip_lib):
    """The three matrix paths are different instruction streams (test_ens_matrix_paths_agree_and_follow_weight_updates): a
    62-wide model that fell off the f16 kernel would give the bf16 kernel's bits on path 2."""
    _need_gpu()
    rng = np.random.default_rng(62)
    m, ws, bs, sc_in, sc_out = _wide_model(rng, 37, 31)
    x = rng.standard_normal((1000, 37)).astype(np.float32)
    out = {}
    before = hip_lib.cmbpo_get_ens_matrix_path()
    hip_lib.cmbpo_set_ens_f16_min_rows(0)
    try:
        for path in (0, 1, 2):
            assert hip_lib.cmbpo_set_ens_matrix_path(path) == 0
            out[path] = m.predict_ensemble(x)
    finally:
        hip_lib.cmbpo_set_ens_matrix_path(before)
        hip_lib.cmbpo_set_ens_f16_min_rows(0)
    scale = float(np.abs(out[0][0]).max())
    for other in (0, 1):
        d = float(np.abs(out[2][0] - out[other][0]).max())
        assert 0.0 < d <= 2e-5 * scale, (other, d)


@pytest.mark.parametrize("E,I,H,D,loss,batch", [
    (7, 37, 512, 31, "MSPE", 256),      # AntSafe with a cost column: 62 raw outputs
    (7, 37, 512, 31, "MSPE", 2048),     # ... at the shipped batch size
    (3, 26, 512, 22, "MSPE", 70),       # HalfCheetahSafe with a cost column
    (7, 37, 512, 31, "NLL", 256),
])
def test_first_step_gradients_and_losses_with_a_cost_column(hip_lib, E, I, H, D, loss, batch):
    """test_ens_train_gpu.test_first_step_gradients_and_losses at the widths the cost column gives, same tolerances."""
    _need_gpu()
    from test_ens_train_gpu import _close, _make
    rng, pe, ref, x, t, ws, bs = _make(E, I, H, D, loss, max(600, 2 * batch), seed=E * 1000 + I + D)
    tr = pe._ensure_trainer(batch)
    if D == 31:
        assert tr.f16_paths == 3, tr.f16_paths      # the f16 backward chain and the f16 training forward
    idx = rng.randint(0, x.shape[0], size=(E, batch)).astype(np.int32)
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    idx_d = torch.from_numpy(idx).cuda()
    hold = rng.permutation(x.shape[0])[:157].astype(np.int32)
    got_l = tr.losses(xd, td, torch.from_numpy(hold).cuda(), 0, hold.shape[0]).cpu().numpy()
    ref_l = ref.losses(np.tile(x[hold][None], (E, 1, 1)), np.tile(t[hold][None], (E, 1, 1)))
    np.testing.assert_allclose(got_l, ref_l, rtol=2e-4)
    got_lb = tr.losses(xd, td, idx_d, batch, batch).cpu().numpy()
    np.testing.assert_allclose(got_lb, ref.losses(x[idx], t[idx]), rtol=2e-4)
    _, gs = ref.grads(x[idx], t[idx])
    tr.step(xd, td, idx_d.data_ptr(), batch, batch)
    mw, mb = tr.get_moments(0)
    n = len(ws)
    for l in range(n):
        _close(10.0 * mw[l], gs[l].numpy(), 2e-3, 5e-5, f"dW{l}")
        _close(10.0 * mb[l], gs[n + l].numpy().reshape(mb[l].shape), 2e-3, 5e-5, f"db{l}")
    assert tr.steps_done == 1


# ------------------------------------------------------------------------------------------------------------------
# host API
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task", ["AntSafe-v2", "HopperSafe-v2"])
def test_fake_env_step_with_predicted_cost(hip_lib, task):
    _need_gpu()
    from cmbpo_amd import synthetic
    from cmbpo_amd.fake_env import FakeEnv
    rng = np.random.default_rng(23)
    D, A = synthetic.ENV_DIMS[task]
    m, ws, bs, sc_in, sc_out = _wide_model(rng, D + A, D + 2)

    class _Env:
        observation_space, action_space = _Space(D), _Space(A)

    env = FakeEnv(_Env(), task, m, predicts_delta=True, predicts_rew=True, predicts_cost=True)
    assert env.output_dim == D + 2
    n = 500
    obs = synthetic.start_states(rng, n, task)
    act = rng.uniform(-1, 1, (n, A)).astype(np.float32)
    inds = rng.choice(np.asarray(m.elite_inds, np.int32), size=n).astype(np.int32)
    nobs, r, terms, info = env.step(obs, act, model_inds=inds)
    rmean, rvar = refcpu.ens_forward(np.concatenate([obs, act], -1), ws, bs, sc_in, sc_out)
    rn, rr, rt, rinfo = refcpu.fake_env_step(obs, act, np.ascontiguousarray(rmean[..., :D + 1]),
                                             np.ascontiguousarray(rvar[..., :D + 1]), inds, task)
    c = info["cost"]
    assert isinstance(c, np.ndarray) and c.shape == (n, 1) and c.dtype == np.float32
    assert nobs.shape == (n, D) and r.shape == (n, 1) and terms.shape == (n, 1) and terms.dtype == bool
    np.testing.assert_allclose(c[:, 0], rmean[inds, np.arange(n), D + 1], rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(r, rr, rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(nobs, rn, rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(info["ensemble_dkl_path"], rinfo["ensemble_dkl_path"], rtol=5e-3, atol=1e-6)
    if task == "AntSafe-v2":      # the static termination rule still applies, on the kernel's own next_obs
        np.testing.assert_array_equal(terms, refcpu.antsafe_term_fn(obs, act, nobs))
    else:
        assert not terms.any()
    # CUDA tensors in, CUDA tensors out, the same bits
    dev = torch.device("cuda:0")
    nobs_t, r_t, terms_t, info_t = env.step(torch.from_numpy(obs).to(dev), torch.from_numpy(act).to(dev), model_inds=inds)
    ct = info_t["cost"]
    assert ct.is_cuda and ct.dtype == torch.float32 and tuple(ct.shape) == (n, 1)
    np.testing.assert_array_equal(ct.cpu().numpy(), c)
    np.testing.assert_array_equal(nobs_t.cpu().numpy(), nobs)
    # a single row is squeezed like the reference's return_single
    n1, r1, t1, i1 = env.step(obs[3], act[3], model_inds=inds[3:4])
    assert n1.shape == (D,) and r1.shape == (1,) and t1.shape == (1,) and i1["cost"].shape == (1,)
    assert i1["cost"].dtype == np.float32
    np.testing.assert_allclose(i1["cost"], c[3], rtol=2e-4, atol=2e-4)
    # what stays unsupported, and a model without the column
    with pytest.raises(NotImplementedError):
        env.step(obs, act, deterministic=False)
    with pytest.raises(NotImplementedError):
        env.step(obs[None], act[None])
    for kw in (dict(predicts_delta=False, predicts_rew=True), dict(predicts_delta=True, predicts_rew=False)):
        with pytest.raises(NotImplementedError):
            FakeEnv(_Env(), task, m, predicts_cost=True, **kw)
    with pytest.raises(AssertionError):
        FakeEnv(_Env(), task, m, predicts_delta=True, predicts_rew=True, predicts_cost=False)


def test_checkpoint_round_trip_of_a_model_with_a_cost_column(hip_lib, tmp_path):
    _need_gpu()
    from cmbpo_amd.pens import PE
    rng = np.random.default_rng(5)
    D, A = 20, 6
    m, ws, bs, sc_in, sc_out = _wide_model(rng, D + A, D + 2, E=5, hidden=128)
    m.save(str(tmp_path), 3)
    m2 = PE(D + A, D + 2, hidden_dims=(128, 128), num_networks=5, num_elites=5, loss="MSPE", use_scaler_in=True,
            use_scaler_out=True, device="cuda:0")
    m2.load(str(tmp_path), 3)
    assert m2.out_dim == D + 2
    for a, b in zip(m.get_weights()[0] + m.get_weights()[1], m2.get_weights()[0] + m2.get_weights()[1]):
        np.testing.assert_array_equal(a, b)
    x = rng.standard_normal((40, D + A)).astype(np.float32)
    m1, v1 = m.predict_ensemble(x)
    mm, vv = m2.predict_ensemble(x)
    assert m1.shape == (5, 40, D + 2)
    np.testing.assert_array_equal(m1, mm)
    np.testing.assert_array_equal(v1, vv)


# ------------------------------------------------------------------------------------------------------------------
# the trainer, closed loop
# ------------------------------------------------------------------------------------------------------------------
class CostPointEnv:
    """2-D point mass with drag (the PointEnv of test_cmbpo_loop_gpu.py): obs = [pos, vel, sin / cos of a clock], reward
    = -|pos|.  Cost 1 on the right half plane (pos_x > 0), a rule of the observation no task of statics.py knows: under
    task='default' an imagined sample carries a cost only if the model predicts it."""

    def __init__(self, seed=0):
        self.observation_space, self.action_space = _Space(6), _Space(2)
        self.rng = np.random.RandomState(seed)
        self.t = 0

    def _obs(self):
        return np.concatenate([self.pos, self.vel, [np.sin(0.1 * self.t), np.cos(0.1 * self.t)]]).astype(np.float32)

    def reset(self):
        self.pos, self.vel, self.t = self.rng.uniform(-0.5, 0.5, 2), np.zeros(2), 0
        return self._obs()

    def step(self, a):
        a = np.clip(np.asarray(a, np.float64).reshape(-1)[:2], -1, 1)
        self.vel = 0.9 * self.vel + 0.1 * a + 0.01 * self.rng.standard_normal(2)
        self.pos = self.pos + 0.1 * self.vel
        self.t += 1
        return self._obs(), -float(np.abs(self.pos).sum()), False, {"cost": float(self.pos[0] > 0.0)}

    def close(self):
        pass


def _run_cost_loop(m_learn_cost):
    """A few epochs of CMBPO on CostPointEnv, built through utils.build_experiment from the reference's config schema."""
    from cmbpo_amd import synthetic
    from cmbpo_amd.utils import build_experiment
    np.random.seed(0)
    env = CostPointEnv(seed=1)
    env.max_episode_steps = 40
    params = {
        'universe': 'gym', 'task': 'default', 'environment_params': {'normalize_actions': True},
        'algorithm_params': {'type': 'CMBPO', 'kwargs': {
            'n_env_interacts': 2200, 'eval_every_n_steps': 1, 'use_model': True, 'm_learn_cost': m_learn_cost,
            'm_train_freq': 100, 'm_networks': 4, 'm_elites': 3, 'm_hidden_dims': (128, 128), 'rollout_batch_size': 400,
            'rollout_mode': 'schedule', 'rollout_schedule': [0, 1, 4, 4], 'maxroll': 6,
            'initial_real_samples_per_epoch': 150, 'min_real_samples_per_epoch': 100, 'batch_size_policy': 2500,
            'n_initial_exploration_steps': 1500, 'n_epochs': 50,
            'initial_model_train_kwargs': dict(min_epochs=40, max_epochs=60, batch_size=128),
            'model_train_kwargs': dict(min_epochs=1, max_epochs=2, batch_size=128)}},
        'policy_params': {'type': 'cpopolicy', 'kwargs': {
            'a_hidden_layer_sizes': (128, 128), 'vf_lr': 1e-3, 'vf_hidden_layer_sizes': (128, 128), 'vf_epochs': 2,
            'vf_batch_size': 256, 'vf_ensemble_size': 3, 'vf_elites': 2, 'vf_activation': 'swish', 'vf_loss': 'MSE',
            'target_kl': 0.01, 'cost_lim': 5.0}},
        'buffer_params': {'kwargs': {'size': 1600, 'archive_size': 8000}}, 'sampler_params': {'kwargs': {}},
        'run_params': {},
    }
    algo = build_experiment(params, env, device="cuda:0")
    algo._policy.set_params(synthetic.policy_params(np.random.default_rng(2), 6, 2, 128))
    rng = np.random.RandomState(1)
    algo._policy.v.init_weights(rng)
    algo._policy.vc.init_weights(rng)
    seen = dict(costs=[], target_cols=[], explore_costs=None)
    get0, train0 = algo.model_buf.get, algo._model.train

    def get(*a, **k):
        res, diag = get0(*a, **k)
        seen["costs"].append(res[9].detach().cpu().numpy().copy() if isinstance(res[9], torch.Tensor) else np.array(res[9]))
        return res, diag

    def train(x, y, *a, **k):
        if seen["explore_costs"] is None:       # the first fit: the archive holds the initial exploration only
            seen["explore_costs"] = algo._buffer.get_archive(['costs'])['costs'].copy()
        seen["target_cols"].append(int(y.shape[1]))
        return train0(x, y, *a, **k)

    algo.model_buf.get, algo._model.train = get, train
    diags = []
    for d in algo.train():
        diags.append(d)
        if d.get("done") or len(diags) > 20:
            break
    assert diags and diags[-1].get("done") is True and algo.policy_epoch >= 2
    return algo, seen


def test_cmbpo_learns_and_uses_the_cost_head(hip_lib):
    """Closed loop with m_learn_cost=True on a task without a cost rule: the model is built and trained with the cost
    column, the imagined samples carry the predicted costs, and the prediction beats the best constant predictor of the
    archived real costs (mean squared error below their variance: the bound is that of predicting the mean)."""
    _need_gpu()
    algo, seen = _run_cost_loop(True)
    frac = float(np.mean(seen["explore_costs"]))
    assert 0.1 <= frac <= 0.9, frac                                   # precondition: the cost rule splits the exploration data
    assert algo._model.out_dim == 8 and algo.fake_env.output_dim == 8 and algo.fake_env._predicts_cost
    assert seen["target_cols"] and all(c == 8 for c in seen["target_cols"])     # [delta obs | reward | cost]
    assert len(seen["costs"]) >= 2
    for c in seen["costs"]:
        assert c.dtype == np.float32 and c.ndim == 1 and np.isfinite(c).all()
    allc = np.concatenate(seen["costs"])
    assert float(np.std(allc)) > 0.05, float(np.std(allc))           # identically zero without the head
    arch = algo._buffer.get_archive(['observations', 'actions', 'costs'])
    n = arch['observations'].shape[0]
    elite = int(algo._model.elite_inds[0])
    _, _, _, info = algo.fake_env.step(arch['observations'], arch['actions'], model_inds=np.full(n, elite, np.int32))
    pred, real = info["cost"][:, 0].astype(np.float64), np.squeeze(arch['costs']).astype(np.float64)
    mse, var = float(np.mean((pred - real) ** 2)), float(np.var(real))
    print("learned cost head: mse %.4f against var(cost) %.4f over %d archived samples" % (mse, var, n))
    assert var > 0.05 and mse < var, (mse, var)


def test_cmbpo_default_keeps_zero_imagined_costs(hip_lib):
    """m_learn_cost=False (the default) on the same task: obs + 1 outputs, obs + 1 targets, imagined costs identically zero."""
    _need_gpu()
    algo, seen = _run_cost_loop(False)
    assert algo._model.out_dim == 7 and not algo.fake_env._predicts_cost
    assert seen["target_cols"] and all(c == 7 for c in seen["target_cols"])
    assert len(seen["costs"]) >= 2 and all((c == 0).all() for c in seen["costs"])


def test_cmbpo_learned_cost_with_device_start_states(hip_lib, start_state_sampling="device"):
    """The other start-state mode (the closed-loop tests above run the default, 'host')."""
    _need_gpu()
    from cmbpo_amd.cmbpo import CMBPO
    from cmbpo_amd.cpo_policy import CPOPolicy
    from cmbpo_amd.cpo_sampler import CpoSampler
    from cmbpo_amd.cpobuffer import CPOBuffer
    from cmbpo_amd import synthetic
    np.random.seed(0)
    env = CostPointEnv(seed=2)
    T = 40
    policy = CPOPolicy(env.observation_space, env.action_space, a_hidden_layer_sizes=(128, 128),
                       vf_hidden_layer_sizes=(128, 128), vf_ensemble_size=3, vf_elites=2, vf_activation="swish",
                       vf_loss="MSE", vf_lr=1e-3, vf_epochs=2, vf_batch_size=256, device="cuda:0", max_path_length=T,
                       cost_lim=5.0, target_kl=0.01)
    policy.set_params(synthetic.policy_params(np.random.default_rng(2), 6, 2, 128))
    rng = np.random.RandomState(1)
    policy.v.init_weights(rng)
    policy.vc.init_weights(rng)
    buf = CPOBuffer(600, 6000, env.observation_space, env.action_space)
    algo = CMBPO(env, policy, buf, sampler=CpoSampler(max_path_length=T), task="default", n_env_interacts=700,
                 eval_every_n_steps=1, m_learn_cost=True, m_train_freq=100, m_networks=4, m_elites=3,
                 m_hidden_dims=(128, 128), rollout_batch_size=400, rollout_mode="schedule", rollout_schedule=[0, 1, 4, 4],
                 maxroll=6, initial_real_samples_per_epoch=150, min_real_samples_per_epoch=100, batch_size_policy=2500,
                 n_initial_exploration_steps=300, n_epochs=50, start_state_sampling=start_state_sampling,
                 initial_model_train_kwargs=dict(min_epochs=3, max_epochs=6, batch_size=128),
                 model_train_kwargs=dict(min_epochs=1, max_epochs=2, batch_size=128))
    diags = []
    for d in algo.train():
        diags.append(d)
        if d.get("done") or len(diags) > 20:
            break
    assert diags and diags[-1].get("done") is True
    assert algo._model.out_dim == 8 and np.isfinite(diags[0]["model/poolm_cret_mean"])


# ------------------------------------------------------------------------------------------------------------------
# sharded: two gloo ranks on the one GPU (test_world2_gpu.py's arrangement, with this file's world)
# ------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, name, out_dir):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, GOLD)
    sys.path.insert(0, HERE)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import datetime
    import torch.distributed as td
    td.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    import cmbpo_amd  # noqa: F401
    from cmbpo_amd.dist import Comm
    from worlds_learned_cost import build_world_learned_cost
    comm = Comm(device=torch.device("cuda:0"))
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    task, B, T, hidden = str(g["task"]), int(g["B"]), int(g["T"]), int(g["hidden"])
    w = build_world_learned_cost(int(g["seed"]), task, hidden, out_scale=float(g["out_scale"]), q_boost=float(g["q_boost"]))
    cut = B // 2 + 3                                   # unequal contiguous shards
    lo, hi = (0, cut) if rank == 0 else (cut, B)
    sampler, pool = hip_world_cost(w, task, T, str(g["mode"]), float(g["dkl_lim"]), hi - lo, hidden, comm=comm)
    sampler.reset(g["start"][lo:hi])
    budget = int(g["budget"]) or None
    alive_before = np.ones(B, bool)
    ok_masks, ratios = True, []
    for s in range(len(g["n_rows"])):
        n = int(g["n_rows"][s])
        ids = np.flatnonzero(alive_before)
        assert len(ids) == n
        mine = (ids >= lo) & (ids < hi)
        assert pool.n_alive == int(mine.sum())
        _, _, _, info = sampler.sample(max_samples=budget, eps=g["eps"][s, :n][mine], model_inds=g["inds"][s, :n][mine])
        ok_masks = ok_masks and bool(np.array_equal(pool.alive_paths, g["alive"][s][lo:hi]))
        ratios.append(info["alive_ratio"])
        alive_before = g["alive"][s].astype(bool)
    sampler.finish_all_paths()
    res, bdiag = pool.get()
    out = {"ok_masks": ok_masks, "ratios": np.array(ratios), "local_samples": sampler._host["total_samples"],
           "batch": bdiag["poolm_batch_size"], "cret_mean": bdiag["poolm_cret_mean"]}
    for k, arr in zip(NAMES, res):
        out["get_" + k] = arr
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **out)
    comm.barrier()
    td.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", ["g14_trace_cost_hopper_budget", "g14_trace_cost_ant_term"])
def test_sharded_rollout_reproduces_reference_trace_with_learned_cost(hip_lib, tmp_path, name):
    """The budget trace goes through the per-step path of the cross-shard budget exchange (FakeEnv.step_device), the other
    through cmbpo_rollout_step on each shard."""
    _need_gpu()
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, name, str(tmp_path)), nprocs=world, join=True)
    r = [np.load(os.path.join(tmp_path, f"rank{k}.npz")) for k in range(world)]
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    assert all(bool(x["ok_masks"]) for x in r)
    for x in r:
        np.testing.assert_array_equal(x["ratios"], g["alive_ratio"])
    assert sum(float(x["local_samples"]) for x in r) == float(g["total_samples"][-1])
    assert sum(int(x["batch"]) for x in r) == int(g["poolm_batch_size"])
    for x in r:
        np.testing.assert_allclose(float(x["cret_mean"]), float(g["poolm_cret_mean"]), rtol=2e-3, atol=2e-4)
    for k in NAMES:
        got = np.concatenate([x["get_" + k] for x in r], axis=0)
        ref = g["get_" + k]
        assert got.shape == ref.shape and got.dtype == ref.dtype, k
        if TOL[k] == 0.0:
            np.testing.assert_array_equal(got, ref, err_msg=k)
        else:
            np.testing.assert_allclose(got, ref, rtol=TOL[k], atol=TOL[k], err_msg=k)
