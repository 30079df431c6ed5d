"""GPU: derived quantities of the task rules (cmbpo_rule_derived_table_t, cmbpo_amd.statics.derived / dist_sq / speed_sq / tilt)
through every layer -- the post kernel's tail against ``TaskRules.numpy_fns()`` bit for bit on its own next_obs, beside every
other feature of the post step, without a trace in the instances that carry no derived table, on the G18 traces recorded from
the REFERENCE's FakeEnv with hand-written natural NumPy functions (tests/golden/make_golden_derived_rules.py) on all three
matrix paths, through the native rollout loop, the host objects and the trainer.

Masks (term, rule costs, alive lists) are compared exactly; everything continuous at the tolerances of test_task_rules_gpu.py,
whose replay and loop helpers these tests share.  The G18 generator kept every tested value at least 1e-3 (relative to
max(1, |threshold|)) from its threshold."""
import ctypes as C
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
G18 = ["g18_trace_derived_hazards", "g18_trace_derived_tilt"]
INF = float("inf")
F = np.float32


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b, keys=None, msg=""):
    for k in (keys or a):
        x, y = a[k], b[k]
        np.testing.assert_array_equal(_bits(x) if x.dtype == np.float32 else x, _bits(y) if y.dtype == np.float32 else y, err_msg=msg + k)


SRCS = ("next_obs", "obs", "act")


def _eight_by_four():
    """8 quantities of 4 terms each over all three sources, columns counted from both ends (every obs_dim >= 3 / act_dim == 3 has
    them), both powers, weights of both signs."""
    from cmbpo_amd.statics import derived, term
    qs = []
    for j in range(8):
        terms = [term(col=((j + 2 * t) % 3) if (j + t) % 2 == 0 else -1 - ((j + t) % 3), src=SRCS[(j + t) % 3],
                      w=(-1.0) ** t * (0.5 + 0.25 * ((j + t) % 4)), c=0.125 * ((j * t) % 5) - 0.25, pow=1 + (j + t) % 2) for t in range(4)]
        qs.append(derived(terms, bias=0.1 * j - 0.3))
    return qs


def _rule_sets():
    from cmbpo_amd.statics import TaskRules, cost, derived, fatal, healthy, term
    q8 = _eight_by_four()
    return {
        "one_term": TaskRules([healthy(src="derived", cols=0, lo=-0.5, hi=0.5)], derived=[derived([term(0)])]),
        "eight_by_four": TaskRules([cost(src="derived", cols=slice(0, None), any=True, lo=1.0, lo_strict=True),       # ANY over all 8
                                    healthy(src="derived", cols=slice(2, 6), lo=-1.5, hi=1.5),                        # ALL over a slice
                                    fatal(src="derived", cols=-1, scale=-0.5, abs=True, lo=0.5),                      # one quantity, twice:
                                    cost(src="derived", cols=7, scale=2.0, hi=-1.0),                                  # other scale, no ABS
                                    healthy(cols=slice(1, None), abs=True, hi=100.0, hi_strict=True)],                # beside a column clause
                                   derived=q8, require_finite=True, cost_on_term=True),
        "no_flags": TaskRules([cost(src="derived", cols=slice(-3, None), lo=-0.75, hi=0.75),
                               fatal(src="derived", cols=slice(0, 3), any=True, lo=1.25)], derived=q8[:5]),
    }


def _inputs(rng, E, B, D, A, live, extra=0):
    """Random rows; NaN, +-inf and -0.0 planted in term columns of obs / act / next_obs of some live rows, and next_obs column 0 at
    and beside the one-term rule's thresholds."""
    obs = (rng.standard_normal((B, D)) * 0.4).astype(F)
    act = rng.uniform(-1, 1, (B, A)).astype(F)
    mean = (rng.standard_normal((E, B, D + 1 + extra)) * 0.3).astype(F)
    var = np.exp(rng.uniform(-12, 1, (E, B, D + 1 + extra))).astype(F)
    inds = rng.integers(0, E, size=B).astype(np.int32)
    up, dn = lambda v: np.nextafter(F(v), F(INF)), lambda v: np.nextafter(F(v), F(-INF))
    L = len(live)
    for i, v in enumerate((F(0.5), up(0.5), dn(0.5), F(-0.5), dn(-0.5), up(-0.5), np.nan, INF, -INF, F(-0.0))):
        b = live[i % L]
        obs[b, 0] = 0.0
        mean[:, b, 0] = v
    obs[live[10 % L], 1] = np.nan
    obs[live[11 % L], D - 1] = INF
    obs[live[12 % L], 0] = -INF
    act[live[13 % L], 0] = np.nan
    act[live[14 % L], A - 1] = INF
    act[live[15 % L], 1] = F(-0.0)
    obs[live[16 % L], :] = INF            # inf - inf inside a quantity
    mean[:, live[16 % L], :D] = -INF
    return obs, act, mean, var, inds


def _want(rules, obs, act, nxt):
    term_fn, cost_fn = rules.numpy_fns()
    with np.errstate(all="ignore"):
        t = term_fn(obs, act, nxt)[:, 0].astype(np.uint8)
        c = cost_fn(obs, act, nxt)[:, 0] if cost_fn is not None else np.zeros(len(t), F)
    return t, c


@pytest.mark.parametrize("E", [7, 5, 3])                 # the kernel's three instances: 7 and 5 members compiled in, else run time
@pytest.mark.parametrize("D", [3, 8, 21, 47])            # the D < 8 row sums, no tail, tails of 5 and 7 columns
def test_post_kernel_derived_rules_equal_numpy_fns_bit_for_bit(hip_lib, E, D):
    _need_gpu()
    from test_learned_cost_gpu import _run_post
    from cmbpo_amd import _lib
    rng = np.random.default_rng(zlib.crc32(f"derived/{E}/{D}".encode()))
    A, B, n = 3, 64, 37
    rows = rng.permutation(B)[:n].astype(np.int32)        # 37 rows, shuffled, of ld_rows = 64: the fifth workgroup has 5 of 8 rows
    obs, act, mean, var, inds = _inputs(rng, E, B, D, A, rows)
    base = _run_post(_lib.TASK_DEFAULT, obs, act, mean, var, inds, D, A, rows)
    rest = np.setdiff1d(np.arange(B), rows)
    for name, rules in _rule_sets().items():
        assert rules.task_id >= _lib.TASK_USER_BASE
        got = _run_post(rules.task_id, obs, act, mean, var, inds, D, A, rows)
        _same(got, base, ("next_obs", "rew", "dkl_path", "ep_var_mean", "ep_var"), name + ": ")
        want_t, want_c = _want(rules, obs[rows], act[rows], got["next_obs"][rows])
        np.testing.assert_array_equal(got["term"][rows], want_t, err_msg=name)
        np.testing.assert_array_equal(_bits(got["cost"][rows]), _bits(want_c), err_msg=name)
        assert (got["term"][rest] == 77).all() and (got["cost"][rest] == -7.0).all()
        assert set(want_t.tolist()) == {0, 1} and set(want_c.tolist()) == ({0.0, 1.0} if rules.has_cost else {0.0}), name    # both ways


def _run_post_cost(task_arg, obs, act, mean, var, inds, D, A, xi=None, dis=None, th=None, ch=None):
    """cmbpo_fakeenv_post_cost, the superset entry: every feature optional."""
    from cmbpo_amd import _lib
    dev = torch.device("cuda:0")
    B, E = obs.shape[0], mean.shape[0]
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    f = dict(dtype=torch.float32, device=dev)
    out = dict(next_obs=torch.full((B, D), -7.0, **f), rew=torch.full((B,), -7.0, **f),
               term=torch.full((B,), 77, dtype=torch.uint8, device=dev), cost=torch.full((B,), -7.0, **f),
               dkl_path=torch.full((B,), -7.0, **f), ep_var_mean=torch.full((B,), -7.0, **f), ep_var=torch.full((B, D), -7.0, **f),
               rew_var=torch.full((B,), -7.0, **f), cost_var=torch.full((B,), -7.0, **f))
    d = [t(obs), t(act), t(mean), t(var), t(inds), t(xi)]
    ths = None if th is None else _lib.TermHeadStruct(float(th), _lib.TERM_ELITE, None, None)
    chs = None if ch is None else _lib.CostHeadStruct(_lib.COST_LOGISTIC, float(ch), None)
    rc = _lib.lib().cmbpo_fakeenv_post_cost(
        task_arg, E, D, A, _lib.ptr(d[2]), _lib.ptr(d[3]), B, _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[4]), None, None, B,
        _lib.ptr(out["next_obs"]), _lib.ptr(out["rew"]), _lib.ptr(out["term"]), _lib.ptr(out["cost"]),
        _lib.ptr(out["dkl_path"]), _lib.ptr(out["ep_var_mean"]), _lib.ptr(out["ep_var"]), _lib.ptr(d[5]),
        0.0 if dis is None else float(dis), 0.0, _lib.ptr(out["rew_var"]) if dis is not None else None,
        _lib.ptr(out["cost_var"]) if dis is not None else None,
        None if ths is None else C.byref(ths), None if chs is None else C.byref(chs), _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().cmbpo_last_error()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("feature", ["learned_cost", "noise", "disagreement", "term_head", "logistic_cost", "all"])
def test_derived_rules_beside_every_other_feature_of_the_post_step(hip_lib, feature):
    """The instances that combine the derived table with another feature's arguments: term is the rules' own on the step's
    next_obs (with `noise=` the shifted one), and so is the cost wherever it is static."""
    _need_gpu()
    from cmbpo_amd import _lib
    rng = np.random.default_rng(zlib.crc32(feature.encode()))
    E, D, A, B = 7, 21, 3, 45
    rows = np.arange(B)
    learned = feature in ("learned_cost", "logistic_cost", "all")
    head = feature in ("term_head", "all")
    obs, act, mean, var, inds = _inputs(rng, E, B, D, A, rows, extra=int(learned) + int(head))
    xi = rng.standard_normal((B, D)).astype(F) if feature in ("noise", "all") else None
    kw = dict(xi=xi, dis=0.5 if feature in ("disagreement", "all") else None,
              th=1e30 if head else None,                        # a threshold no member reaches: the rules alone end branches
              ch=0.25 if feature in ("logistic_cost", "all") else None)
    for name, rules in _rule_sets().items():
        task = rules.task_id | (_lib.TASK_LEARNED_COST if learned else 0)
        got = _run_post_cost(task, obs, act, mean, var, inds, D, A, **kw)
        want_t, want_c = _want(rules, obs, act, got["next_obs"])
        np.testing.assert_array_equal(got["term"], want_t, err_msg=name)
        assert want_t.any() and not want_t.all()
        if not learned:
            np.testing.assert_array_equal(_bits(got["cost"]), _bits(want_c), err_msg=name)
        with np.errstate(all="ignore"):
            plain = _bits((mean[inds, rows, :D] + obs).astype(F))
        assert np.array_equal(_bits(got["next_obs"]), plain) == (xi is None)       # with `noise=` the rules saw the shifted state


def test_no_leak_into_the_instances_without_a_derived_table(hip_lib):
    """A table without derived quantities through the _ex entry is the id of the old entry and launches what it launched; the
    built-in AntSafe and HalfCheetahSafe rules give what models/statics.py's formulas give in NumPy, bit for bit."""
    _need_gpu()
    from test_learned_cost_gpu import _run_post
    from test_task_rules_gpu import _adversarial
    from test_task_rules_gpu import _rule_sets as plain_sets
    from cmbpo_amd import _lib, synthetic
    from oracle import refcpu
    lib = _lib.lib()
    rng = np.random.default_rng(19)
    E, D, A, B = 7, 21, 5, 203
    rows = np.arange(B, dtype=np.int32)
    obs, act, mean, var, inds = _adversarial(rng, E, B, D, A, rows)
    for rules in plain_sets():
        s, empty, a, b = rules.struct(), _lib.RuleDerivedTableStruct(), C.c_int(-1), C.c_int(-1)
        assert lib.cmbpo_task_rules_register_ex(C.byref(s), None, C.byref(a)) == 0
        assert lib.cmbpo_task_rules_register_ex(C.byref(s), C.byref(empty), C.byref(b)) == 0
        assert a.value == b.value == rules.task_id
        _same(_run_post(a.value, obs, act, mean, var, inds, D, A), _run_post(rules.task_id, obs, act, mean, var, inds, D, A))
    for task in ("AntSafe-v2", "HalfCheetahSafe-v2"):
        D, A = synthetic.ENV_DIMS[task]
        obs, act, mean, var, inds = _adversarial(rng, E, B, D, A, rows)
        if task == "AntSafe-v2":
            mean[:, :, 0] = np.abs(mean[:, :, 0]) + 0.4        # inside the height gate, so the tilt decides as well
            obs[:, 0] = 0.0
            mean[:, ::3, 2] = 0.95                             # z_rot below -0.7 on every third row
            obs[::3, 2] = 0.0
            mean[:, ::5, D - 1] = 4.0
        got = _run_post(_lib.TASK_IDS[task], obs, act, mean, var, inds, D, A)
        nxt = got["next_obs"]
        with np.errstate(all="ignore"):
            want_t = refcpu.TERMS_BY_TASK[task](obs, act, nxt)[:, 0]
            want_c = np.asarray(refcpu.COST_BY_TASK[task](obs, act, nxt), dtype=F)[:, 0]
        np.testing.assert_array_equal(got["term"], want_t.astype(np.uint8), err_msg=task)
        np.testing.assert_array_equal(_bits(got["cost"]), _bits(want_c), err_msg=task)
        assert set(got["cost"].tolist()) == {0.0, 1.0}
        if task == "AntSafe-v2":
            assert got["term"].any() and not got["term"].all()


def _g18(name):
    import worlds_derived
    from worlds import build_world
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    case = worlds_derived.CASES[name]
    rules = worlds_derived.build_rules(case["rules"](*g["thresholds"].tolist()))
    w = build_world(int(g["seed"]), str(g["task"]), int(g["hidden"]), out_scale=float(g["out_scale"]), q_boost=float(g["q_boost"]))
    return g, w, rules


@pytest.mark.parametrize("name", G18)
@pytest.mark.parametrize("ens_path", [0, 1, 2], indirect=True, ids=["fp32mfma", "splitbf16", "splitf16"])
def test_hip_sampler_reproduces_reference_trace_with_derived_rules(hip_lib, ens_path, name):
    _need_gpu()
    from test_task_rules_gpu import _replay
    g, w, rules = _g18(name)
    res = _replay(g, w, rules, int(g["hidden"]))            # alive masks and cost masks exact
    if name == "g18_trace_derived_tilt":
        assert (np.diff(g["n_rows"]) < 0).any()             # nothing but the rules' terminations shrinks this alive list
    assert 0.2 <= float(res[9].mean()) <= 0.8


@pytest.mark.parametrize("name", G18)
def test_sample_many_equals_a_loop_of_sample_with_derived_rules(hip_lib, name):
    _need_gpu()
    from test_task_rules_gpu import _loop_vs_many
    g, w, rules = _g18(name)
    state, _, res, alive = _loop_vs_many(w, rules, str(g["task"]), int(g["B"]), int(g["T"]), str(g["mode"]), g["start"],
                                        int(g["budget"]) or None)
    if name == "g18_trace_derived_tilt":
        assert alive[-1] < alive[0]
    assert 0.0 < float(res[9].mean()) < 1.0


def test_derived_rules_across_the_small_batch_threshold(hip_lib):
    """The alive count starts above the one-workgroup bookkeeping's row limit and falls below it through the tilt rule's
    terminations: both ways a step reaches the post kernel, in one rollout, loop and cmbpo_rollout_run alike."""
    _need_gpu()
    from test_task_rules_gpu import _loop_vs_many
    from cmbpo_amd import synthetic
    from cmbpo_amd.statics import TaskRules, healthy, tilt
    g, w, _ = _g18("g18_trace_derived_tilt")
    rules = TaskRules([healthy(src="derived", cols=0, lo=-6.0)], derived=[tilt(2, 3)], require_finite=True)
    limit = hip_lib.cmbpo_rollout_book_pre_max_rows()
    B = limit + 60
    start = synthetic.start_states(np.random.default_rng(78), B, str(g["task"]))
    state, _, res, alive = _loop_vs_many(w, rules, str(g["task"]), B, int(g["T"]), str(g["mode"]), start, None)
    stepped = alive[:-1]
    assert sum(a > limit for a in stepped) >= 1 and sum(0 < a <= limit for a in stepped) >= 1, (alive, limit)


def test_fake_env_step_and_replay_with_derived_rules(hip_lib):
    """The host API: FakeEnv.step returns the reference's shapes and dtypes and what numpy_fns() says; FakeEnv.replay takes the id
    -- teacher-forced, its predicted terminations per horizon are those of a loop of step() on the recorded observations."""
    _need_gpu()
    from test_rollout_sampler_gpu import hip_world
    from cmbpo_amd import _lib, statics
    g, w, rules = _g18("g18_trace_derived_tilt")
    D, A, n = w["obs_dim"], w["act_dim"], int(g["B"])
    statics.register_task("DerivedTilt-v0", rules)
    rng = np.random.default_rng(1)
    act = rng.uniform(-1, 1, (n, A)).astype(F)
    inds = g["inds"][0]
    outs = {}
    for key, task in (("rules", rules), ("name", "DerivedTilt-v0")):
        sampler, _ = hip_world(w, task, 4, "schedule", float("inf"), n, int(g["hidden"]))
        env = sampler.env if hasattr(sampler, "env") else sampler._env
        outs[key] = (env, env.step(g["start"], act, model_inds=inds))
    env, (nobs, r, terms, info) = outs["rules"]
    assert env._task_id == rules.task_id == outs["name"][0]._task_id >= _lib.TASK_USER_BASE
    term_fn, cost_fn = rules.numpy_fns()
    np.testing.assert_array_equal(terms, term_fn(g["start"], act, nobs))
    np.testing.assert_array_equal(info["cost"], cost_fn(g["start"], act, nobs))
    assert nobs.dtype == F and nobs.shape == (n, D) and r.shape == (n, 1)
    assert terms.dtype == bool and terms.shape == (n, 1) and info["cost"].dtype == F and info["cost"].shape == (n, 1)
    np.testing.assert_array_equal(outs["name"][1][2], terms)
    # replay, one step ahead: horizon h starts from the recorded observation before it
    H = 3
    steps = (rng.standard_normal((H, n, D)) * 0.3).astype(F)
    nxt = (g["start"][None] + np.cumsum(steps, axis=0)).astype(F)
    acts = rng.uniform(-1, 1, (H, n, A)).astype(F)
    minds = np.broadcast_to(inds, (H, n)).astype(np.int32).copy()
    zero = np.zeros((H, n), F)
    got = env.replay(g["start"], acts, nxt, zero, zero, np.zeros((H, n), np.uint8), model_inds=minds, mode="one_step")
    assert got["n"].tolist() == [n] * H
    pred = 0
    for h in range(H):
        cur = g["start"] if h == 0 else nxt[h - 1]
        _, _, t_h, _ = env.step(cur, acts[h], model_inds=minds[h])
        assert int(got["term_cm"][h, 0, 1]) == int(t_h.sum()) and int(got["term_cm"][h, 0, 0]) == n - int(t_h.sum())
        pred += int(t_h.sum())
    assert 0 < pred < H * n


def test_cmbpo_trainer_with_a_circular_hazard(hip_lib):
    """CMBPO(static_fns=TaskRules(..., derived=...)) on the toy world for two epochs with a circular hazard as the cost: every
    imagined sample's stored cost equals numpy_fns() on its stored next observation."""
    _need_gpu()
    import toyworld
    from cmbpo_amd import _lib, synthetic
    from cmbpo_amd.cmbpo import CMBPO
    from cmbpo_amd.cpo_policy import CPOPolicy
    from cmbpo_amd.cpo_sampler import CpoSampler
    from cmbpo_amd.cpobuffer import CPOBuffer
    from cmbpo_amd.statics import TaskRules, cost, dist_sq
    rules = TaskRules([cost(src="derived", cols=0, hi=0.09)], derived=[dist_sq((0, 1), (0.1, 0.05))])
    _, cost_fn = rules.numpy_fns()
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
    algo = CMBPO(env, policy, buf, sampler=CpoSampler(max_path_length=T), task="AntSafe-v2", static_fns=rules,
                 n_env_interacts=10 ** 9, eval_every_n_steps=1, m_train_freq=100, m_networks=4, m_elites=3,
                 m_hidden_dims=(128, 128), rollout_batch_size=400, rollout_mode="schedule", rollout_schedule=[0, 1, 4, 4],
                 maxroll=6, initial_real_samples_per_epoch=150, min_real_samples_per_epoch=100, batch_size_policy=2500,
                 n_initial_exploration_steps=300, n_epochs=50,
                 initial_model_train_kwargs=dict(min_epochs=3, max_epochs=6, batch_size=128),
                 model_train_kwargs=dict(min_epochs=1, max_epochs=2, batch_size=128))
    assert algo.fake_env._task_id == rules.task_id >= _lib.TASK_USER_BASE
    snaps = []
    finish = algo.model_sampler.finish_all_paths

    def recording(*a, **k):
        t = algo.model_buf.t
        snaps.append({k2: t[k2].cpu().numpy().copy() for k2 in ("len", "cur_obs", "next_obs", "obs_buf", "cost_buf", "term_t")})
        return finish(*a, **k)

    algo.model_sampler.finish_all_paths = recording
    diags = []
    for d in algo.train():
        diags.append(d)
        if len(diags) >= 2:
            break
    assert len(diags) == 2 and snaps
    checked, costly = 0, 0
    zero_a = np.zeros((1, A), F)
    for s in snaps:
        assert not s["term_t"].any()                  # a cost rule only: nothing ends a branch
        for b in range(s["len"].shape[0]):
            L = int(s["len"][b])
            # the next observation of stored step t is the stored observation of step t + 1; of the last one, whichever of the
            # two swapped observation arrays is not its own stored observation
            nxts = [s["obs_buf"][t + 1, b] for t in range(L - 1)]
            if L >= 1:
                cands = [x[b] for x in (s["cur_obs"], s["next_obs"])]
                same = [np.array_equal(c, s["obs_buf"][L - 1, b]) for c in cands]
                if sum(same) == 1:
                    nxts.append(cands[same.index(False)])
            for t, nx in enumerate(nxts):
                want = cost_fn(s["obs_buf"][t, b][None], zero_a, nx[None])[0, 0]
                assert s["cost_buf"][t, b] == want, (b, t, nx)
                checked += 1
                costly += int(want)
    assert checked > 500 and 0 < costly < checked, (checked, costly)
    assert np.isfinite(diags[0]["model/poolm_cret_mean"])
