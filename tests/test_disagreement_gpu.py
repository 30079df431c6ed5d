"""GPU: ensemble disagreement on reward / cost and the pessimistic imagined rollout, through every layer -- the post kernel's
DIS instances against tests/disagreement_ref.py and against the plain entry points, the rollout state beside cmbpo_rollout_t
(per-branch sums, totals, the penalised values in the buffers) on the one-workgroup bookkeeping path and just above it, the
FakeEnv host API, and the trainer.

Bit for bit throughout, except the two totals: float64 sums of fewer than 1e5 non-negative terms added in another order
than the host's, bound n * 2^-53 ~ 1e-11, compared at rtol 1e-10."""
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import disagreement_ref as ref  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
NAMES = ["obs", "act", "adv", "cadv", "ret", "cret", "logp", "val", "cval", "cost", "log_std", "mu"]
CLASSIC = ("next_obs", "rew", "term", "cost", "dkl_path", "ep_var_mean", "ep_var")


class _Space:
    def __init__(self, d):
        self.shape = (d,)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, msg=""):
    """Bit for bit where the specification is finite or infinite, NaN where it is NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=msg)
    ok = ~np.isnan(b)
    np.testing.assert_array_equal(_bits(a)[ok], _bits(b)[ok], err_msg=msg)


# ------------------------------------------------------------------------------------------------------------------
# 1. the post kernel
# ------------------------------------------------------------------------------------------------------------------
def _run_post(entry, task_arg, obs, act, mean, var, inds, obs_dim, act_dim, row_idx=None, xi=None, kappa=(0.0, 0.0)):
    """One of the three entry points on slot-indexed arrays; with row_idx only the listed slots are stepped.  Every output
    starts at a sentinel."""
    from cmbpo_amd import _lib
    dev = torch.device("cuda:0")
    B, E = obs.shape[0], mean.shape[0]
    n = B if row_idx is None else len(row_idx)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    f = dict(dtype=torch.float32, device=dev)
    out = dict(next_obs=torch.full((B, obs_dim), -7.0, **f), rew=torch.full((B,), -7.0, **f),
               term=torch.full((B,), 77, dtype=torch.uint8, device=dev), cost=torch.full((B,), -7.0, **f),
               dkl_path=torch.full((B,), -7.0, **f), ep_var_mean=torch.full((B,), -7.0, **f),
               ep_var=torch.full((B, obs_dim), -7.0, **f), rew_var=torch.full((B,), -7.0, **f),
               cost_var=torch.full((B,), -7.0, **f))
    d = [t(obs), t(act), t(mean), t(var), t(inds)]
    ri = None if row_idx is None else t(np.asarray(row_idx, np.int32))
    d_xi = None if xi is None else t(xi)
    args = (task_arg, E, obs_dim, act_dim, _lib.ptr(d[2]), _lib.ptr(d[3]), B, _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[4]),
            _lib.ptr(ri), None, n, _lib.ptr(out["next_obs"]), _lib.ptr(out["rew"]), _lib.ptr(out["term"]), _lib.ptr(out["cost"]),
            _lib.ptr(out["dkl_path"]), _lib.ptr(out["ep_var_mean"]), _lib.ptr(out["ep_var"]))
    lib = _lib.lib()
    if entry == "disagreement":
        rc = lib.cmbpo_fakeenv_post_disagreement(*args, _lib.ptr(d_xi), float(kappa[0]), float(kappa[1]), _lib.ptr(out["rew_var"]),
                                                 _lib.ptr(out["cost_var"]), _lib.current_stream())
    elif d_xi is not None:
        rc = lib.cmbpo_fakeenv_post_noise(*args, _lib.ptr(d_xi), _lib.current_stream())
    else:
        rc = lib.cmbpo_fakeenv_post(*args, _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.cmbpo_last_error())
    return {k: v.cpu().numpy() for k, v in out.items()}


def _post_task(kind):
    """(task name for the dims, rule id, learned cost?)"""
    from cmbpo_amd import _lib
    if kind == "antsafe_learned":
        return "AntSafe-v2", _lib.TASK_ANTSAFE | _lib.TASK_LEARNED_COST, True
    if kind == "hcs_static":
        return "HalfCheetahSafe-v2", _lib.TASK_HCS, False
    from cmbpo_amd.statics import TaskRules, cost, healthy
    rules = TaskRules([healthy(cols=0, lo=0.2, hi=1.5), cost(cols=-1, abs=True, lo=0.4, lo_strict=True)], require_finite=True,
                      cost_on_term=True)
    return "HopperSafe-v2", rules.task_id | _lib.TASK_LEARNED_COST, True


@pytest.mark.parametrize("noise", [False, True], ids=["mean", "noise"])
@pytest.mark.parametrize("E", [7, 5, 3])     # the kernel is compiled for 7 and 5 members; any other size at run time
@pytest.mark.parametrize("kind", ["antsafe_learned", "hcs_static", "rules_learned"])
@pytest.mark.parametrize("n,listed", [(13, False), (29, True), (1001, True)])     # never a multiple of 8
def test_post_kernel_disagreement(hip_lib, kind, n, listed, E, noise):
    """rew_var / cost_var are the specification's; kappa = (0, 0) leaves every classic output what the plain entry writes;
    kappa > 0 changes rew / cost into the specification's and nothing else."""
    _need_gpu()
    from cmbpo_amd import synthetic
    task, task_arg, learned = _post_task(kind)
    rng = np.random.default_rng(zlib.crc32(f"{kind}/{n}/{listed}/{E}/{noise}/disagreement".encode()))
    D, A = synthetic.ENV_DIMS[task]
    O = D + 1 + int(learned)
    B = n + 11 if listed else n
    obs = synthetic.start_states(rng, B, task)
    act = rng.uniform(-1, 1, (B, A)).astype(np.float32)
    mean = (rng.standard_normal((E, B, O)) * 0.3).astype(np.float32)
    var = np.exp(rng.uniform(-12, 1, (E, B, O))).astype(np.float32)
    var[:, ::7, 3] = 0.0
    inds = rng.integers(0, E, size=B).astype(np.int32)
    xi = rng.standard_normal((B, D)).astype(np.float32) if noise else None
    rows = np.sort(rng.choice(B, size=n, replace=False)).astype(np.int32) if listed else None
    live = np.arange(B) if rows is None else rows
    # non-finite predictions in the reward and the cost column: every member's, the elite's, another member's
    mean[:, live[2], D] = np.nan
    mean[inds[live[3]], live[3], D] = np.inf
    mean[(inds[live[4]] + 1) % E, live[4], D] = np.nan          # must not reach rew with kappa_rew == 0
    mean[(inds[live[5]] + 2) % E, live[5], D] = -np.inf
    mean[1, live[10], 5] = np.nan                                # an observation column: not this feature's business
    if learned:
        mean[:, live[6], D + 1] = np.nan
        mean[inds[live[7]], live[7], D + 1] = -np.inf
        mean[(inds[live[8]] + 1) % E, live[8], D + 1] = np.nan   # must not reach cost with kappa_cost == 0
        mean[(inds[live[9]] + 2) % E, live[9], D + 1] = np.inf
    plain = _run_post("plain", task_arg, obs, act, mean, var, inds, D, A, rows, xi)
    rest = np.setdiff1d(np.arange(B), live)

    def check_vars(got, tag):
        rv, cv, _, _ = ref.disagreement(mean, inds, D, learned, rows=live)
        _same(got["rew_var"][live], rv, tag + " rew_var")
        if learned:
            _same(got["cost_var"][live], cv, tag + " cost_var")
        else:
            assert (_bits(got["cost_var"][live]) == 0).all(), tag       # exactly +0.0
        assert np.isnan(got["rew_var"][live[[2, 3, 4, 5]]]).all() and np.isfinite(got["rew_var"][live[[0, 1, 11]]]).all()
        if len(rest):     # unlisted slots keep their sentinel in the new arrays too
            assert (got["rew_var"][rest] == -7.0).all() and (got["cost_var"][rest] == -7.0).all()
            assert (got["rew"][rest] == -7.0).all() and (got["term"][rest] == 77).all()

    zero = _run_post("disagreement", task_arg, obs, act, mean, var, inds, D, A, rows, xi, (0.0, 0.0))
    check_vars(zero, "kappa 0")
    for k in CLASSIC:
        np.testing.assert_array_equal(_bits(zero[k]), _bits(plain[k]), err_msg=k)
    assert np.isfinite(zero["rew"][live[4]]) and np.isfinite(zero["rew"][live[5]])
    if learned:
        assert np.isfinite(zero["cost"][live[8]]) and np.isfinite(zero["cost"][live[9]])

    kappas = [(0.75, 1.5), (0.5, 0.0), (0.0, 2.0)] if learned else [(0.75, 0.0)]
    for kr, kc in kappas:
        pes = _run_post("disagreement", task_arg, obs, act, mean, var, inds, D, A, rows, xi, (kr, kc))
        check_vars(pes, f"kappa {kr}, {kc}")
        _, _, rew, cost = ref.disagreement(mean, inds, D, learned, kr, kc, rows=live)
        if kr > 0:
            _same(pes["rew"][live], rew, "rew")
            assert np.isnan(pes["rew"][live[4]])
            fin = np.isfinite(rew)
            assert (pes["rew"][live][fin] <= plain["rew"][live][fin]).all() and (pes["rew"][live][fin] < plain["rew"][live][fin]).any()
        else:
            np.testing.assert_array_equal(_bits(pes["rew"]), _bits(plain["rew"]))
        if kc > 0:
            _same(pes["cost"][live], cost, "cost")
            assert np.isnan(pes["cost"][live[8]])
            fin = np.isfinite(cost)
            assert (pes["cost"][live][fin] >= plain["cost"][live][fin]).all() and (pes["cost"][live][fin] > plain["cost"][live][fin]).any()
        else:
            np.testing.assert_array_equal(_bits(pes["cost"]), _bits(plain["cost"]))
        for k in ("next_obs", "term", "dkl_path", "ep_var_mean", "ep_var"):
            np.testing.assert_array_equal(_bits(pes[k]), _bits(plain[k]), err_msg=k)


def test_post_kernel_refuses_a_pessimistic_static_cost(hip_lib):
    _need_gpu()
    from cmbpo_amd import _lib
    rng = np.random.default_rng(3)
    D, A, E, n = 18, 6, 5, 9
    obs = rng.standard_normal((n, D)).astype(np.float32)
    act = rng.standard_normal((n, A)).astype(np.float32)
    mean = rng.standard_normal((E, n, D + 1)).astype(np.float32)
    with pytest.raises(AssertionError):
        _run_post("disagreement", _lib.TASK_HCS, obs, act, mean, np.ones_like(mean), np.zeros(n, np.int32), D, A, kappa=(0.0, 0.5))
    msg = hip_lib.cmbpo_last_error()
    assert b"cmbpo_fakeenv_post_disagreement" in msg and b"kappa_cost" in msg


# ------------------------------------------------------------------------------------------------------------------
# 2. the rollout
# ------------------------------------------------------------------------------------------------------------------
TASK, T, HIDDEN, KAPPA = "AntSafe-v2", 6, 128, (0.75, 1.5)


def _world(w, B, dkl_lim, disagreement=False, kappa=(0.0, 0.0)):
    from cmbpo_amd.cpo_policy import CPOPolicy
    from cmbpo_amd.fake_env import FakeEnv
    from cmbpo_amd.model_sampler import ModelSampler
    from cmbpo_amd.modelbuffer import ModelBuffer
    from cmbpo_amd.pens import PE
    D, A = w["obs_dim"], w["act_dim"]
    E = w["ws"][0].shape[0]
    model = PE(D + A, D + 2, hidden_dims=(HIDDEN, HIDDEN), num_networks=E, num_elites=len(w["elites"]),
               loss="MSPE", use_scaler_in=True, use_scaler_out=True, device="cuda:0")
    model.set_weights(w["ws"], w["bs"], w["sc_in"], w["sc_out"])
    model.set_elites(w["elites"])
    policy = CPOPolicy(_Space(D), _Space(A), a_hidden_layer_sizes=(128, 128), vf_hidden_layer_sizes=(128, 128),
                       vf_ensemble_size=3, vf_elites=2, vf_activation="swish", vf_loss="MSE", device="cuda:0",
                       cost_gamma=0.97, cost_lam=0.5, lam=0.95)
    policy.actor.set_params(w["pol"])
    policy.v.set_weights(*w["v"])
    policy.vc.set_weights(*w["vc"])

    class _Env:
        observation_space, action_space = _Space(D), _Space(A)

    env = FakeEnv(_Env(), TASK, model, predicts_delta=True, predicts_rew=True, predicts_cost=True,
                  disagreement=disagreement, rew_pessimism=kappa[0], cost_pessimism=kappa[1])
    pool = ModelBuffer(B, D, A, T, device="cuda:0")
    pool.initialize(policy.pi_info_shapes, gamma=0.99, lam=0.95, cost_gamma=0.97, cost_lam=0.5)
    sampler = ModelSampler(max_path_length=T + 5, batch_size=B, rollout_mode="uncertainty")
    sampler.initialize(env, policy, pool)
    sampler.set_rollout_dkl(dkl_lim)
    return sampler, pool


def _roll(w, start, dkl_lim, budget, disagreement, kappa, how):
    """One rollout of T steps with the sampler's own draws (seed 5).  how: 'loop' (sample(): cmbpo_rollout_step), 'many'
    (sample_many(): cmbpo_rollout_run) or 'calls' (sample() with kernel events on: the separate entry points)."""
    B = start.shape[0]
    sampler, pool = _world(w, B, dkl_lim, disagreement, kappa)
    if how == "calls":
        sampler.env.kernel_events = []
    sampler._gen.manual_seed(5)
    sampler.reset(start)
    on = pool.disagreement
    assert on == (disagreement or kappa[0] > 0 or kappa[1] > 0)
    assert ("rew_var_t" in pool.t) == on and ("path_rew_var" in pool.t) == on
    rec = dict(steps=[], on=on)
    cp = lambda x: x.cpu().numpy().copy()
    if how == "many":
        steps, _ = sampler.sample_many(max_samples=budget)
        assert steps == T
    else:
        for s in range(T):
            assert sampler.any_alive() and pool.has_room
            len0 = cp(pool.t["len"])
            n_in = pool.n_alive
            stepped = cp(pool.t["alive_idx"][:n_in])
            sampler.sample(max_samples=budget)
            st = dict(stepped=stepped, stored=cp(pool.t["len"]) > len0, alive=cp(pool.t["alive_idx"][:pool.n_alive]),
                      len=cp(pool.t["len"]), next_obs=cp(pool.t["cur_obs"])[stepped], rew_t=cp(pool.t["rew_t"]),
                      cost_t=cp(pool.t["cost_t"]), n_budget=sampler.n_budget_terminated)
            if on:
                st.update(rew_var_t=cp(pool.t["rew_var_t"]), cost_var_t=cp(pool.t["cost_var_t"]))
            rec["steps"].append(st)
    rec["n_alive_end"] = pool.n_alive
    rec["n_budget"] = sampler.n_budget_terminated
    rec["len"] = cp(pool.t["len"])
    if on:
        rec["path_rew_var"], rec["path_cost_var"] = cp(pool.t["path_rew_var"]), cp(pool.t["path_cost_var"])
    rec["rew_buf"], rec["cost_buf"] = cp(pool.t["rew_buf"]), cp(pool.t["cost_buf"])
    rec["diag"] = sampler.finish_all_paths()
    rec["dscal"] = sampler._dsc.copy()
    rec["get"], _ = pool.get()
    return rec


_PLANS = {}


def _plan(B):
    """World, start states, an uncertainty limit that ends two fifths of the branches within T steps and a budget that binds
    on the last step only -- from two pilot rollouts without the feature (nothing of it moves a branch).  A branch passes every
    uncertainty test iff its DKL accumulated over all T steps stays below the limit (the terms are >= 0), so the limit is a
    quantile of that sum over the branches the pilot without a limit stored T times."""
    if B in _PLANS:
        return _PLANS[B]
    from worlds_learned_cost import build_world_learned_cost
    from cmbpo_amd import synthetic
    w = build_world_learned_cost(77, TASK, HIDDEN, q_boost=0.8)
    start = synthetic.start_states(np.random.default_rng(78), B, TASK)
    sampler, pool = _world(w, B, float("inf"))
    sampler._gen.manual_seed(5)
    sampler.reset(start)
    for _ in range(T):
        sampler.sample()
    acc = pool.t["dkl_acc"].cpu().numpy()
    full = pool.t["len"].cpu().numpy() == T
    assert full.sum() > B // 4, "the pilot's branches do not live long enough"
    sampler.finish_all_paths()
    pool.get()
    dkl_lim = float(np.quantile(acc[full], 0.6))
    pilot = _roll(w, start, dkl_lim, None, False, (0.0, 0.0), "loop")
    totals = [int(st["len"].sum()) for st in pilot["steps"]]
    last = totals[-1] - totals[-2]
    assert last >= 8, "too few branches reach the last step"
    budget = totals[-2] + last // 2
    _PLANS[B] = (w, start, dkl_lim, budget)
    return _PLANS[B]


def _rollout_batches():
    from cmbpo_amd import _lib
    return 1000, _lib.lib().cmbpo_rollout_book_pre_max_rows() + 70


@pytest.mark.parametrize("which", [0, 1], ids=["one_workgroup", "above"])
def test_rollout_with_disagreement(hip_lib, which):
    """B on the one-workgroup bookkeeping path and just above it: (a) the native loop against the per-step call, (b) kappa = 0
    against the feature off, (c) kappa moves no branch, (d) per-branch sums, (e) totals, (f) the penalised values are what the
    buffer holds and what the advantages are made from -- and the separate entry points (sample() with kernel events) agree
    with the one-call step.  get() has no reward array: the rewards are read from rew_buf in get()'s branch-major order."""
    _need_gpu()
    B = _rollout_batches()[which]
    assert (B <= hip_lib.cmbpo_rollout_book_pre_max_rows()) == (which == 0)
    w, start, dkl_lim, budget = _plan(B)
    pes = _roll(w, start, dkl_lim, budget, True, KAPPA, "loop")
    # the shapes the test is about: uncertainty ended some branches, the budget bound on the last step only, some reached the end
    assert pes["steps"][-2]["n_budget"] == 0 and pes["n_budget"] > 0
    assert sum(len(st["stepped"]) - int(st["stored"].sum()) for st in pes["steps"][:-1]) > 0 or \
        len(pes["steps"][-1]["stepped"]) - int(pes["steps"][-1]["stored"].sum()) > pes["n_budget"]
    assert pes["steps"][-1]["stored"].sum() > 0
    from cmbpo_amd import _lib

    # (a) sample_many == a loop of sample, and == the separate entry points
    for how in ("many", "calls"):
        other = _roll(w, start, dkl_lim, budget, True, KAPPA, how)
        for k, a, b in zip(NAMES, pes["get"], other["get"]):
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"{how} {k}")
        for k in ("path_rew_var", "path_cost_var", "len"):
            np.testing.assert_array_equal(pes[k], other[k], err_msg=f"{how} {k}")
        assert pes["dscal"][_lib.D_TOTAL_SAMPLES] == other["dscal"][_lib.D_TOTAL_SAMPLES]
        for slot in (_lib.D_TOTAL_REW_VAR, _lib.D_TOTAL_COST_VAR, _lib.D_SUM_PATH_COST, _lib.D_SUM_PATH_RET):
            if how == "many":       # the same kernels: the same bits
                assert pes["dscal"][slot] == other["dscal"][slot], (how, slot)
            else:                   # the store's own tiles and fold: float64 sums of the same terms in another order
                np.testing.assert_allclose(other["dscal"][slot], pes["dscal"][slot], rtol=1e-10, atol=0, err_msg=str(slot))

    # (b) feature on with kappa = 0 == feature off
    zero = _roll(w, start, dkl_lim, budget, True, (0.0, 0.0), "loop")
    off = _roll(w, start, dkl_lim, budget, False, (0.0, 0.0), "loop")
    assert zero["on"] and not off["on"]
    for k, a, b in zip(NAMES, zero["get"], off["get"]):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=k)
    assert off["dscal"][_lib.D_TOTAL_REW_VAR] == 0.0 and off["dscal"][_lib.D_TOTAL_COST_VAR] == 0.0
    assert off["diag"]["msampler/rew_var_perstep"] == 0.0 and off["diag"]["msampler/cost_var_perstep"] == 0.0

    # (c) the same branches alive after every step, the same lengths, the same next states
    for s, (p, z) in enumerate(zip(pes["steps"], zero["steps"])):
        np.testing.assert_array_equal(p["alive"], z["alive"], err_msg=f"alive list after step {s}")
        np.testing.assert_array_equal(p["len"], z["len"], err_msg=f"len after step {s}")
        np.testing.assert_array_equal(_bits(p["next_obs"]), _bits(z["next_obs"]), err_msg=f"next_obs of step {s}")
        np.testing.assert_array_equal(_bits(p["rew_var_t"][p["stepped"]]), _bits(z["rew_var_t"][z["stepped"]]))

    # (d) per-branch float64 sums in step order over the stored rows; (e) the totals
    for run in (pes, zero):
        prv, pcv = np.zeros(B, np.float64), np.zeros(B, np.float64)
        terms_r, terms_c = [], []
        for st in run["steps"]:
            m = st["stored"]
            prv[m] += st["rew_var_t"][m].astype(np.float64)
            pcv[m] += st["cost_var_t"][m].astype(np.float64)
            terms_r.append(st["rew_var_t"][m].astype(np.float64))
            terms_c.append(st["cost_var_t"][m].astype(np.float64))
        np.testing.assert_array_equal(run["path_rew_var"], prv)
        np.testing.assert_array_equal(run["path_cost_var"], pcv)
        tr, tc = np.concatenate(terms_r), np.concatenate(terms_c)
        n = len(tr)
        assert n == run["dscal"][_lib.D_TOTAL_SAMPLES] and n < 1e5 and (tr >= 0).all() and (tc >= 0).all()
        assert tr.sum() > 0 and tc.sum() > 0
        print(f"B = {B}: {n} stored samples, mean rew_var {tr.mean():.3e}, mean cost_var {tc.mean():.3e}, totals' relative "
              f"distance to the host sums {abs(run['dscal'][_lib.D_TOTAL_REW_VAR] / tr.sum() - 1):.1e} / "
              f"{abs(run['dscal'][_lib.D_TOTAL_COST_VAR] / tc.sum() - 1):.1e}")
        np.testing.assert_allclose(run["dscal"][_lib.D_TOTAL_REW_VAR], tr.sum(), rtol=1e-10, atol=0)
        np.testing.assert_allclose(run["dscal"][_lib.D_TOTAL_COST_VAR], tc.sum(), rtol=1e-10, atol=0)
        np.testing.assert_allclose(run["diag"]["msampler/rew_var_perstep"], tr.sum() / (n + 1e-8), rtol=1e-10)
        np.testing.assert_allclose(run["diag"]["msampler/cost_var_perstep"], tc.sum() / (n + 1e-8), rtol=1e-10)
        assert run["diag"]["msampler/ens_mean_var"] == 0.0

    # (f) the buffers hold the recorded penalised values, branch-major, and the advantages are made from them
    L = pes["len"]
    mask = np.arange(T)[None] < L[:, None]                  # [B, T]
    rew_rec = np.stack([st["rew_t"] for st in pes["steps"]], 1)
    cost_rec = np.stack([st["cost_t"] for st in pes["steps"]], 1)
    np.testing.assert_array_equal(_bits(pes["get"][9]), _bits(cost_rec[mask]))
    np.testing.assert_array_equal(_bits(pes["rew_buf"].T[mask]), _bits(rew_rec[mask]))
    rew0 = np.stack([st["rew_t"] for st in zero["steps"]], 1)
    cost0 = np.stack([st["cost_t"] for st in zero["steps"]], 1)
    rv = np.stack([st["rew_var_t"] for st in pes["steps"]], 1)
    cv = np.stack([st["cost_var_t"] for st in pes["steps"]], 1)
    _same(rew_rec[mask], ref.penalise(rew0[mask], rv[mask], KAPPA[0], -1))
    _same(cost_rec[mask], ref.penalise(cost0[mask], cv[mask], KAPPA[1], +1))
    assert (rew_rec[mask] <= rew0[mask]).all() and (cost_rec[mask] >= cost0[mask]).all()
    assert (rew_rec[mask] < rew0[mask]).any() and (cost_rec[mask] > cost0[mask]).any()
    assert pes["get"][2].shape == zero["get"][2].shape
    assert (pes["get"][2] != zero["get"][2]).any() and (pes["get"][3] != zero["get"][3]).any()
    np.testing.assert_array_equal(_bits(pes["get"][0]), _bits(zero["get"][0]))       # the same observations


def _roll_attached(w, start, dkl_lim, budget, how, attach, detach_iv=False):
    """One rollout with the sampler's own draws (seed 5) and the features of `attach` ('iv': the weighted GAE, 'dg': the
    disagreement with both kappas 0) attached beside the struct in that order; detach_iv: the weighted GAE is switched off
    again before the rollout.  how: 'loop' (sample()) or 'many' (sample_many()).  Returns get()'s twelve arrays and the two
    variance diagnostics."""
    sampler, pool = _world(w, start.shape[0], dkl_lim, "dg" in attach, (0.0, 0.0))
    for f in attach:
        if f == "iv":
            pool.set_iv_gae(True)
        else:
            pool.set_disagreement(True)
    if detach_iv:
        pool.set_iv_gae(False)
    sampler._gen.manual_seed(5)
    sampler.reset(start)         # (takes the environment's switch: the same as what is attached, nothing is attached again)
    assert pool.iv_gae == ("iv" in attach and not detach_iv) and pool.disagreement == ("dg" in attach)
    while sampler.any_alive() and pool.has_room:
        if how == "many":
            sampler.sample_many(max_samples=budget)
        else:
            sampler.sample(max_samples=budget)
    assert pool.ptr == T
    diag = sampler.finish_all_paths()
    return pool.get()[0], (diag["msampler/rew_var_perstep"], diag["msampler/cost_var_perstep"])


@pytest.mark.parametrize("how", ["loop", "many"])
@pytest.mark.parametrize("which", [0, 1], ids=["one_workgroup", "above"])
def test_iv_gae_and_disagreement_together(hip_lib, which, how):
    """The weighted GAE and the disagreement share one table beside the struct: attached to the same buffer, in either order,
    each computes what it computes alone (kappa = 0: the disagreement only measures), and switching one off leaves the other.
    B = 300 on the one-workgroup bookkeeping kernels, B = their limit + 76 on the separate store / finish kernels."""
    _need_gpu()
    B = (300, hip_lib.cmbpo_rollout_book_pre_max_rows() + 76)[which]
    w, start, dkl_lim, budget = _plan(B)
    iv_only = _roll_attached(w, start, dkl_lim, budget, how, ("iv",))
    dg_only = _roll_attached(w, start, dkl_lim, budget, how, ("dg",))
    assert iv_only[1] == (0.0, 0.0) and dg_only[1][0] > 0.0 and dg_only[1][1] > 0.0
    # (the weighted recurrence is another one: a run that lost it would pass as the un-weighted run)
    assert (iv_only[0][2] != dg_only[0][2]).any() and (iv_only[0][3] != dg_only[0][3]).any()
    for order in (("iv", "dg"), ("dg", "iv")):
        both = _roll_attached(w, start, dkl_lim, budget, how, order)
        for k, a, b in zip(NAMES, both[0], iv_only[0]):
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"{order} {k}")
        assert both[1] == dg_only[1], order
    left = _roll_attached(w, start, dkl_lim, budget, how, ("iv", "dg"), detach_iv=True)
    for k, a, b in zip(NAMES, left[0], dg_only[0]):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"iv switched off: {k}")
    assert left[1] == dg_only[1]


# ------------------------------------------------------------------------------------------------------------------
# 3. FakeEnv and errors
# ------------------------------------------------------------------------------------------------------------------
def _fake_env(rng, task, learned, **kw):
    from cmbpo_amd import synthetic
    from cmbpo_amd.fake_env import FakeEnv
    from cmbpo_amd.pens import PE
    D, A = synthetic.ENV_DIMS[task]
    O = D + 1 + int(learned)
    ws, bs = synthetic.ensemble_weights(rng, 7, D + A, 128, 2 * O, bias_scale=0.05)
    m = PE(D + A, O, hidden_dims=(128, 128), num_networks=7, num_elites=5, loss="MSPE", use_scaler_in=True,
           use_scaler_out=True, device="cuda:0")
    m.set_weights(ws, bs, synthetic.scaler(rng, D + A), synthetic.scaler(rng, O))

    class _Env:
        observation_space, action_space = _Space(D), _Space(A)

    return FakeEnv(_Env(), task, m, predicts_delta=True, predicts_rew=True, predicts_cost=learned, **kw), m, D, A


@pytest.mark.parametrize("learned", [True, False])
def test_fake_env_step_reports_the_disagreement(hip_lib, learned):
    _need_gpu()
    from cmbpo_amd import synthetic
    task = "AntSafe-v2"
    rng = np.random.default_rng(23)
    env, m, D, A = _fake_env(rng, task, learned)
    n = 333
    obs = synthetic.start_states(rng, n, task)
    act = rng.uniform(-1, 1, (n, A)).astype(np.float32)
    inds = rng.choice(np.asarray(m.elite_inds, np.int32), size=n).astype(np.int32)
    # off: the keys of today
    nobs0, r0, t0, info0 = env.step(obs, act, model_inds=inds)
    assert not env.disagreement and set(info0) == {"ensemble_dkl_mean", "ensemble_dkl_path", "ensemble_ep_var", "rew", "cost"}
    mean, _ = m.predict_ensemble(obs, act=act)          # the forward the step runs: the same kernel on the same rows
    # measured, nothing held against the branch
    env_on, _, _, _ = _fake_env(np.random.default_rng(23), task, learned, disagreement=True)
    assert env_on.disagreement and env_on.rew_pessimism == 0.0
    nobs1, r1, t1, info1 = env_on.step(obs, act, model_inds=inds)
    rv, cv, _, _ = ref.disagreement(mean, inds, D, learned)
    for k in ("ensemble_rew_var", "ensemble_cost_var"):
        assert isinstance(info1[k], np.ndarray) and info1[k].shape == (n,) and info1[k].dtype == np.float32
    _same(info1["ensemble_rew_var"], rv)
    _same(info1["ensemble_cost_var"], cv)
    assert (rv > 0).all() and ((cv > 0).all() if learned else not cv.any())
    np.testing.assert_array_equal(_bits(r1), _bits(r0))
    np.testing.assert_array_equal(_bits(nobs1), _bits(nobs0))
    np.testing.assert_array_equal(_bits(np.asarray(info1["cost"], np.float32)), _bits(np.asarray(info0["cost"], np.float32)))
    # pessimistic: a coefficient > 0 implies the measurement
    kr, kc = 0.75, (1.5 if learned else 0.0)
    env.set_pessimism(kr, kc)
    assert env.disagreement
    nobs2, r2, t2, info2 = env.step(obs, act, model_inds=inds)
    _, _, rew, cost = ref.disagreement(mean, inds, D, learned, kr, kc)
    _same(r2[:, 0], rew)
    _same(info2["rew"][:, 0], rew)
    if learned:
        _same(info2["cost"][:, 0], cost)
    else:
        np.testing.assert_array_equal(info2["cost"], info0["cost"])
    _same(info2["ensemble_rew_var"], rv)
    np.testing.assert_array_equal(_bits(nobs2), _bits(nobs0))
    np.testing.assert_array_equal(t2, t0)
    # CUDA tensors in, CUDA tensors out, the same bits; with transition noise the two columns do not move
    dev = torch.device("cuda:0")
    _, r_t, _, info_t = env.step(torch.from_numpy(obs).to(dev), torch.from_numpy(act).to(dev), model_inds=inds)
    for k in ("ensemble_rew_var", "ensemble_cost_var"):
        assert info_t[k].is_cuda and info_t[k].dtype == torch.float32 and tuple(info_t[k].shape) == (n,)
        np.testing.assert_array_equal(_bits(info_t[k].cpu().numpy()), _bits(info2[k]))
    np.testing.assert_array_equal(_bits(r_t.cpu().numpy()), _bits(r2))
    xi = rng.standard_normal((n, D)).astype(np.float32)
    _, r_x, _, info_x = env.step(obs, act, model_inds=inds, noise=xi)
    np.testing.assert_array_equal(_bits(r_x), _bits(r2))
    np.testing.assert_array_equal(_bits(info_x["ensemble_rew_var"]), _bits(info2["ensemble_rew_var"]))
    np.testing.assert_array_equal(_bits(info_x["ensemble_cost_var"]), _bits(info2["ensemble_cost_var"]))
    # a single row: the per-row values stay arrays of one
    _, r_1, _, info_1 = env.step(obs[3], act[3], model_inds=inds[3:4])
    assert r_1.shape == (1,) and info_1["ensemble_rew_var"].shape == (1,) and info_1["ensemble_cost_var"].shape == (1,)
    assert np.isfinite(info_1["ensemble_rew_var"]).all() and (info_1["ensemble_rew_var"] > 0).all()
    env.set_pessimism(0.0, 0.0)
    assert not env.disagreement and "ensemble_rew_var" not in env.step(obs, act, model_inds=inds)[3]


def test_value_errors(hip_lib):
    _need_gpu()
    from cmbpo_amd.modelbuffer import ModelBuffer
    rng = np.random.default_rng(1)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _fake_env(rng, "AntSafe-v2", True, rew_pessimism=bad)
        with pytest.raises(ValueError):
            _fake_env(rng, "AntSafe-v2", True, cost_pessimism=bad)
    with pytest.raises(ValueError, match="predicts_cost"):
        _fake_env(rng, "AntSafe-v2", False, cost_pessimism=0.5)
    env, _, _, _ = _fake_env(rng, "AntSafe-v2", False, rew_pessimism=0.5)
    with pytest.raises(ValueError, match="predicts_cost"):
        env.set_pessimism(0.5, 0.1)
    with pytest.raises(ValueError):
        env.set_pessimism(-1.0, 0.0)
    assert env.rew_pessimism == 0.5 and env.cost_pessimism == 0.0          # a refused call changes nothing
    buf = ModelBuffer(10, 5, 2, 4, device="cuda:0")
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            buf.set_disagreement(True, bad, 0.0)
    assert not buf.disagreement and "rew_var_t" not in buf.t
    buf.set_disagreement(False, 0.0, 0.25)                                 # a coefficient > 0 implies the measurement
    assert buf.disagreement and buf.t["path_cost_var"].dtype == torch.float64
    buf.reset(20)                                                          # new arrays: attached again
    assert tuple(buf.t["rew_var_t"].shape) == (20,)
    buf.set_disagreement(False)
    assert not buf.disagreement and "path_cost_var" not in buf.t


# ------------------------------------------------------------------------------------------------------------------
# 4. the trainer
# ------------------------------------------------------------------------------------------------------------------
def _train(**kw):
    """Two policy epochs of CMBPO on the point environment of test_learned_cost_gpu.py; the rollout diagnostics of every round."""
    from test_learned_cost_gpu import CostPointEnv
    from cmbpo_amd import synthetic
    from cmbpo_amd.utils import build_experiment
    np.random.seed(0)
    env = CostPointEnv(seed=1)
    env.max_episode_steps = 40
    kwargs = {'n_env_interacts': 2200, 'eval_every_n_steps': 1, 'use_model': True, 'm_train_freq': 100, 'm_networks': 4,
              'm_elites': 3, 'm_hidden_dims': (128, 128), 'rollout_batch_size': 400, 'rollout_mode': 'schedule',
              'rollout_schedule': [0, 1, 4, 4], 'maxroll': 6, 'initial_real_samples_per_epoch': 150,
              'min_real_samples_per_epoch': 100, 'batch_size_policy': 2500, 'n_initial_exploration_steps': 1500, 'n_epochs': 50,
              'initial_model_train_kwargs': dict(min_epochs=10, max_epochs=15, batch_size=128),
              'model_train_kwargs': dict(min_epochs=1, max_epochs=2, batch_size=128)}
    kwargs.update(kw)
    params = {
        'universe': 'gym', 'task': 'default', 'environment_params': {'normalize_actions': True},
        'algorithm_params': {'type': 'CMBPO', 'kwargs': kwargs},
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
    seen = []
    fin0 = algo.model_sampler.finish_all_paths

    def fin():
        d = fin0()
        seen.append(dict(d))
        return d

    algo.model_sampler.finish_all_paths = fin
    for d in algo.train():
        if d.get("done") or algo.policy_epoch >= 2:
            break
    assert algo.policy_epoch >= 2 and seen
    return algo, seen


def test_cmbpo_pessimistic_rollouts(hip_lib):
    _need_gpu()
    algo, seen = _train(m_learn_cost=True, m_rew_pessimism=0.5, m_cost_pessimism=1.0)
    assert algo.fake_env.disagreement and algo.fake_env.rew_pessimism == 0.5 and algo.fake_env.cost_pessimism == 1.0
    assert algo.model_buf.disagreement and algo.model_buf.rew_pessimism == 0.5 and algo.model_buf.cost_pessimism == 1.0
    for d in seen:
        for k in ("msampler/rew_var_perstep", "msampler/cost_var_perstep"):
            assert np.isfinite(d[k]) and d[k] > 0.0, (k, d[k])
        assert d["msampler/ens_mean_var"] == 0.0


def test_cmbpo_default_reports_zero_and_refuses_a_pessimistic_static_cost(hip_lib):
    _need_gpu()
    algo, seen = _train()
    assert not algo.fake_env.disagreement and not algo.model_buf.disagreement and "rew_var_t" not in algo.model_buf.t
    for d in seen:
        assert d["msampler/rew_var_perstep"] == 0.0 and d["msampler/cost_var_perstep"] == 0.0
    with pytest.raises(ValueError, match="m_learn_cost"):
        _train(m_cost_pessimism=0.5)
