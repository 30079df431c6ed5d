"""GPU: open-loop model validation -- cmbpo_replay_run / _compare / _finish and FakeEnv.replay against the existing
path: a Python loop of FakeEnv.step_device fed the recorded actions, with the life of every window applied in NumPy by
tests/replay_ref.py.

The predictions of both sides come from the same kernels on the same rows, so trajectories, masks and counts are compared
exactly.  Every float64 sum is a sum of n exact, non-negative terms added in two different orders: each order is off the true
sum by at most (n - 1) 2^-53 of it, the two differ by at most n 2^-52 relative (n = the rows in the sum); the dkl_path sum is
bounded by n 2^-52 sum|term| in case a term is negative."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import replay_ref as ref  # noqa: E402

DEV = "cuda:0"
PRED = ("next_obs", "rew", "term", "cost", "dkl_path", "ep_var_mean")
KINDS = [("ant", 7), ("hopper", 3), ("ant", 3), ("hopper", 7)]
SIZES = [1, 63, 64, 65, 257, 4099]        # the wave edge, the workgroup edge (64 rows), more than one partial slot
HORIZONS = [1, 2, 7]


class _Space:
    def __init__(self, d):
        self.shape = (d,)


class _Env:
    def __init__(self, D, A):
        self.observation_space, self.action_space = _Space(D), _Space(A)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_ENVS = {}


def _fake_env(kind, E):
    """A FakeEnv over a 128-wide ensemble of E members with small steps: AntSafe's built-in rules at AntSafe's widths, or
    Hopper-like rules through TaskRules at Hopper's.  One per (kind, E) for the module."""
    if (kind, E) in _ENVS:
        return _ENVS[kind, E]
    from cmbpo_amd import synthetic
    from cmbpo_amd.fake_env import FakeEnv
    from cmbpo_amd.pens import PE
    from cmbpo_amd.statics import TaskRules, cost, healthy
    if kind == "ant":
        (D, A), task = synthetic.ENV_DIMS["AntSafe-v2"], "AntSafe-v2"
    else:
        D, A = synthetic.ENV_DIMS["HopperSafe-v2"]
        task = TaskRules([healthy(cols=0, lo=0.2, hi=1.0), cost(cols=-1, abs=True, lo=0.05, lo_strict=True)], require_finite=True,
                         cost_on_term=True)
    rng = np.random.default_rng(zlib.crc32(f"{kind}/{E}/replay-model".encode()))
    ws, bs = synthetic.ensemble_weights(rng, E, D + A, 128, 2 * (D + 1), bias_scale=0.05)
    sc_in = synthetic.scaler(rng, D + A)
    sc_out = (np.zeros((1, D + 1), np.float32), np.full((1, D + 1), 2.5e-3, np.float32))     # steps of ~0.05 per column
    np.random.seed(5)
    model = PE(D + A, D + 1, hidden_dims=(128, 128), num_networks=E, num_elites=max(E - 2, 2), loss="MSPE", use_scaler_in=True,
               use_scaler_out=True, device=DEV)
    model.set_weights(ws, bs, sc_in, sc_out)
    env = FakeEnv(_Env(D, A), task, model, True, True, False, seed=3)
    _ENVS[kind, E] = (env, D, A)
    return _ENVS[kind, E]


def _recording(rng, B, H, D, A, ragged=True):
    """Windows of a made-up world: a random walk of small steps, with ragged lengths, terminals inside some windows, 0/1 costs.
    Column 0 (the height both rule sets test) starts inside the healthy band, for some windows at its very edge."""
    obs0 = (rng.standard_normal((B, D)) * 0.1).astype(np.float32)
    obs0[:, 0] = rng.uniform(0.3, 0.9, B).astype(np.float32)
    obs0[::5, 0] = np.float32(0.21)           # Hopper-like rules: healthy from 0.2 up
    obs0[::5, 2] = np.float32(0.925)          # AntSafe: done once 1 - 2 (q1^2 + q2^2) < -0.7, i.e. q1 beyond 0.922
    steps = (rng.standard_normal((H, B, D)) * 0.05).astype(np.float32)
    nxt = (obs0[None] + np.cumsum(steps, axis=0)).astype(np.float32)
    rec = dict(next_obs=nxt, rew=rng.standard_normal((H, B)).astype(np.float32),
               cost=(rng.random((H, B)) < 0.3).astype(np.float32),
               term=(rng.random((H, B)) < (0.15 if ragged else 0.0)).astype(np.uint8))
    act = rng.uniform(-1, 1, (H, B, A)).astype(np.float32)
    lengths = rng.integers(1, H + 1, B).astype(np.int32) if ragged else np.full(B, H, np.int32)
    return obs0, act, rec, lengths


def _oracle_step(env, act, inds):
    """step(h, cur_obs) for replay_ref: the existing device step on all B rows, recorded actions, given members."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    act_d, inds_d = t(act), t(inds.astype(np.int32))
    B, D = act.shape[1], env.obs_dim
    f = dict(dtype=torch.float32, device=DEV)
    out = dict(next_obs=torch.empty((B, D), **f), rew=torch.empty(B, **f), term=torch.empty(B, dtype=torch.uint8, device=DEV),
               cost=torch.empty(B, **f), dkl_path=torch.empty(B, **f), ep_var_mean=torch.empty(B, **f))

    def step(h, cur):
        env.step_device(t(cur), act_d[h], inds_d[h], out)
        return {k: out[k].cpu().numpy() for k in PRED}
    return step


def _check_table(got, want, tag=""):
    for k in ("n", "n_nonfinite", "cost_cm", "term_cm"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=tag + k)
    n = want["n"].astype(np.float64)
    eps = 2.0 ** -52
    for k in ("se_rew", "se_cost", "sum_ep_var"):
        assert (want[k] >= 0).all(), k
        assert (np.abs(got[k] - want[k]) <= n * eps * want[k]).all(), (tag + k, got[k], want[k])
    assert (np.abs(got["se_obs"] - want["se_obs"]) <= (n * eps)[:, None] * want["se_obs"]).all(), tag + "se_obs"
    assert (np.abs(got["sum_dkl"] - want["sum_dkl"]) <= n * eps * want["sum_abs_dkl"]).all(), tag + "sum_dkl"
    for k, v in got.items():
        if k.startswith("se_") or k.startswith("sum_"):
            assert np.isfinite(v).all(), tag + k
    # the means are the sums over n, NaN where nobody was compared
    m = ref.means({k: got[k] for k in ("n", "se_obs", "se_rew", "se_cost", "sum_ep_var", "sum_dkl")})
    for k, v in m.items():
        np.testing.assert_array_equal(got[k], v, err_msg=tag + k)
    assert (np.diff(got["n"] + got["n_nonfinite"]) <= 0).all(), tag + "n grows"


def _buffers(env, obs0, act, rec, lengths, mode):
    from cmbpo_amd.replay import ReplayBuffers
    return ReplayBuffers(obs0, act, rec["next_obs"], rec["rew"], rec["cost"], rec["term"], lengths=lengths, mode=mode,
                         ensemble=env._model.num_nets, out_dim=env.output_dim, device=DEV)


def _run(env, obs0, act, rec, lengths, inds, mode):
    rb = _buffers(env, obs0, act, rec, lengths, mode)
    rb.run(env._model.mlp.handle, env._task_id, env._model.num_nets, torch.from_numpy(inds.astype(np.int32)).to(DEV))
    torch.cuda.synchronize()
    return rb


def _case(kind, E, B, H, mode, ragged=True):
    env, D, A = _fake_env(kind, E)
    rng = np.random.default_rng(zlib.crc32(f"{kind}/{E}/{B}/{H}/{mode}/{ragged}".encode()))
    obs0, act, rec, lengths = _recording(rng, B, H, D, A, ragged)
    inds = rng.integers(0, E, (H, B)).astype(np.int32)
    return env, obs0, act, rec, lengths, inds


@pytest.mark.parametrize("H", HORIZONS)
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("kind,E", KINDS)
def test_replay_run_matches_the_step_device_loop(hip_lib, kind, E, B, H):
    """Open loop, ragged lengths, recorded terminals inside the windows, rules that terminate: table, final states and masks."""
    _need_gpu()
    env, obs0, act, rec, lengths, inds = _case(kind, E, B, H, "open_loop")
    rb = _run(env, obs0, act, rec, lengths, inds, "open_loop")
    want, cur, alive = ref.replay(_oracle_step(env, act, inds), obs0, rec, lengths, ref.OPEN_LOOP)
    _check_table(rb.table(), want)
    np.testing.assert_array_equal(rb.t["cur_obs"].cpu().numpy().view(np.uint32), cur.view(np.uint32))
    np.testing.assert_array_equal(rb.t["alive"].cpu().numpy().astype(bool), alive)
    assert want["n"][0] == B
    if B == 4099 and H == 7:     # the case does what it is for: windows end early for every reason, some reach the end
        assert 0 < want["n"][-1] < want["n"][1] < B
        assert want["term_cm"][:, 0, 1].sum() > 0 and want["term_cm"][:, 1, 0].sum() > 0
        assert want["cost_cm"][:, 1, :].sum() > 0


@pytest.mark.parametrize("B", [257, 4099])
@pytest.mark.parametrize("kind,E", KINDS[:2])
def test_replay_one_step_matches_the_step_device_loop(hip_lib, kind, E, B):
    _need_gpu()
    env, obs0, act, rec, lengths, inds = _case(kind, E, B, 7, "one_step")
    rb = _run(env, obs0, act, rec, lengths, inds, "one_step")
    want, cur, alive = ref.replay(_oracle_step(env, act, inds), obs0, rec, lengths, ref.ONE_STEP)
    _check_table(rb.table(), want)
    np.testing.assert_array_equal(rb.t["cur_obs"].cpu().numpy().view(np.uint32), cur.view(np.uint32))
    np.testing.assert_array_equal(rb.t["alive"].cpu().numpy().astype(bool), alive)
    assert want["term_cm"][:, 0, 1].sum() > 0         # predicted terminations were counted ...
    open_n = ref.replay(_oracle_step(env, act, inds), obs0, rec, lengths, ref.OPEN_LOOP)[0]["n"]
    assert (want["n"] >= open_n).all() and want["n"].sum() > open_n.sum()      # ... and ended no window


@pytest.mark.parametrize("mode", ["open_loop", "one_step"])
@pytest.mark.parametrize("kind,E,B", [("ant", 7, 257), ("hopper", 3, 65), ("hopper", 7, 4099)])
def test_run_is_the_loop_of_single_calls_bitwise_and_repeats(hip_lib, kind, E, B, mode):
    """cmbpo_replay_run against forward / post / compare issued one call at a time and cmbpo_replay_finish; two runs; and, in the
    single-call loop, the rows that are dead after a step hold the cur_obs they held before it."""
    _need_gpu()
    H = 7
    env, obs0, act, rec, lengths, inds = _case(kind, E, B, H, mode)
    a = _run(env, obs0, act, rec, lengths, inds, mode)
    b = _run(env, obs0, act, rec, lengths, inds, mode)
    c = _buffers(env, obs0, act, rec, lengths, mode)
    inds_d = torch.from_numpy(inds).to(DEV)
    n_alive = []
    for h in range(H):
        before = c.t["cur_obs"].clone()
        env.step_device(c.t["cur_obs"], c.t["act"][h], inds_d[h], c.step_outputs(), scratch=(c.t["mean"], c.t["var"]))
        c.compare(h)
        dead = c.t["alive"] == 0
        assert torch.equal(c.t["cur_obs"][dead], before[dead])
        n_alive.append(int((~dead).sum()))
    c.finish()
    torch.cuda.synchronize()
    assert n_alive == sorted(n_alive, reverse=True) and n_alive[-1] == 0 and n_alive[0] > 0
    for k in ("sums", "counts", "part_sum", "part_cnt", "cur_obs", "alive"):
        for other in (b, c):
            x, y = a.t[k].cpu().numpy(), other.t[k].cpu().numpy()
            np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=k)
    np.testing.assert_array_equal(a.table()["n"][1:], n_alive[:-1])


def test_compare_on_crafted_nonfinite_predictions(hip_lib):
    """cmbpo_replay_compare on hand-made prediction arrays with inf and NaN in next_obs, rew and cost: those rows count in
    n_nonfinite and in no sum, every sum is finite; a dead row's NaN is never read."""
    _need_gpu()
    from cmbpo_amd.replay import ReplayBuffers
    rng = np.random.default_rng(12)
    B, H, D, A = 200, 2, 21, 3
    obs0, act, rec, lengths = _recording(rng, B, H, D, A, ragged=False)
    for mode in ("open_loop", "one_step"):
        rb = ReplayBuffers(obs0, act, rec["next_obs"], rec["rew"], rec["cost"], rec["term"], lengths=lengths, mode=mode, device=DEV)
        tab = ref.new_table(H, D)
        cur, alive = obs0.copy(), np.ones(B, bool)
        alive[[7, 70]] = False                                   # dead on entry
        rb.t["alive"].copy_(torch.from_numpy(alive.astype(np.uint8)))
        for h in range(H):
            pred = dict(next_obs=(rec["next_obs"][h] + rng.standard_normal((B, D)).astype(np.float32) * 0.1).astype(np.float32),
                        rew=rng.standard_normal(B).astype(np.float32), cost=rng.random(B).astype(np.float32),
                        term=(rng.random(B) < 0.2).astype(np.uint8), ep_var_mean=rng.random(B).astype(np.float32),
                        dkl_path=rng.random(B).astype(np.float32))
            if h == 0:
                pred["term"][20] = 0                             # row 20 reaches h = 1 in both modes
                pred["next_obs"][3, 0] = np.nan
                pred["next_obs"][63, D - 1] = np.inf
                pred["next_obs"][64, 5] = -np.inf
                pred["next_obs"][199, :] = np.nan
                pred["rew"][10] = np.nan
                pred["rew"][128] = np.inf
                pred["cost"][11] = -np.inf
                pred["cost"][190] = np.nan
                pred["next_obs"][7, 2] = np.nan                  # dead rows: not counted, not read
                pred["rew"][70] = np.nan
            else:
                pred["next_obs"][20, 1] = np.nan
                pred["next_obs"][3, 1] = np.nan                  # died at h = 0
            for k, v in pred.items():
                rb.step_outputs()[k].copy_(torch.from_numpy(v))
            before = rb.t["cur_obs"].cpu().numpy()
            rb.compare(h)
            ref.compare(tab, h, cur, alive, pred, rec, lengths, mode)
            after = rb.t["cur_obs"].cpu().numpy()
            np.testing.assert_array_equal(after.view(np.uint32), cur.view(np.uint32))
            np.testing.assert_array_equal(rb.t["alive"].cpu().numpy().astype(bool), alive)
            np.testing.assert_array_equal(after[~alive], before[~alive])
        rb.finish()
        torch.cuda.synchronize()
        got = rb.table()
        np.testing.assert_array_equal(got["n_nonfinite"], [8, 1])
        np.testing.assert_array_equal(got["n"][0], B - 2 - 8)
        _check_table(got, tab, mode + " ")
        assert np.isfinite(after).all()


def test_one_step_rows_are_independent_single_step_replays(hip_lib):
    """Teacher-forced mode with full windows and no recorded terminal: row h of the table is, bit for bit, a one-step replay
    started from the real observation the recording reached at h."""
    _need_gpu()
    for kind, E, B in (("ant", 7, 257), ("hopper", 3, 65)):
        env, obs0, act, rec, lengths, inds = _case(kind, E, B, 5, "one_step", ragged=False)
        whole = _run(env, obs0, act, rec, lengths, inds, "one_step").table()
        np.testing.assert_array_equal(whole["n"] + whole["n_nonfinite"], np.full(5, B))
        for h in range(5):
            start = obs0 if h == 0 else rec["next_obs"][h - 1]
            one = _run(env, start, act[h:h + 1], {k: v[h:h + 1] for k, v in rec.items()}, None, inds[h:h + 1], "one_step").table()
            for k, v in one.items():
                np.testing.assert_array_equal(np.atleast_1d(v[0]).view(np.uint8), np.atleast_1d(whole[k][h]).view(np.uint8),
                                              err_msg=f"{kind} h={h} {k}")


def test_fake_env_replay_members_and_generators(hip_lib):
    """FakeEnv.replay: a table like the buffers' own; model_inds as an int is the [H, B] array filled with it; None draws elites
    from a generator of the replay's own and touches no other; refusals."""
    _need_gpu()
    env, obs0, act, rec, lengths, inds = _case("ant", 7, 130, 4, "open_loop")
    args = (obs0, act, rec["next_obs"], rec["rew"], rec["cost"], rec["term"])
    got = env.replay(*args, lengths=lengths, model_inds=inds)
    want = _run(env, obs0, act, rec, lengths, inds, "open_loop").table()
    assert sorted(got) == sorted(want) and {"n", "n_nonfinite", "mse_obs", "mse_rew", "mse_cost", "cost_cm", "term_cm",
                                            "ep_var_mean", "dkl_mean"} <= set(got)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["mse_obs"].shape == (4, 29) and got["cost_cm"].shape == (4, 2, 2)
    # tensors in, trailing axes of one, the same table
    t = lambda a: torch.from_numpy(a).to(DEV)
    again = env.replay(t(obs0), t(act), t(rec["next_obs"]), t(rec["rew"][..., None]), rec["cost"][..., None], t(rec["term"]),
                       lengths=t(lengths), model_inds=t(inds))
    for k in want:
        np.testing.assert_array_equal(again[k], want[k], err_msg=k)
    for member in (0, 4):
        a = env.replay(*args, lengths=lengths, model_inds=member)
        b = env.replay(*args, lengths=lengths, model_inds=np.full((4, 130), member))
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert not np.array_equal(env.replay(*args, model_inds=0)["se_obs"], env.replay(*args, model_inds=4)["se_obs"])
    # None: elites only, from the replay's own stream
    np_state, torch_state = np.random.get_state()[1].copy(), torch.get_rng_state().clone()
    cuda_state, own = torch.cuda.get_rng_state(0).clone(), env._rng.bit_generator.state
    env._model.set_elites([2, 5])
    first = env.replay(*args, lengths=lengths)
    second = env.replay(*args, lengths=lengths)
    np.testing.assert_array_equal(np.random.get_state()[1], np_state)
    assert torch.equal(torch.get_rng_state(), torch_state) and torch.equal(torch.cuda.get_rng_state(0), cuda_state)
    assert env._rng.bit_generator.state == own
    assert not np.array_equal(first["se_obs"], second["se_obs"])              # the stream advances
    env._model.set_elites([5])                                                # one elite: the draw can only be that member
    only = env.replay(*args, lengths=lengths)
    env._model.set_elites([0, 1, 2, 3, 4])
    want5 = env.replay(*args, lengths=lengths, model_inds=5)
    for k in only:
        np.testing.assert_array_equal(only[k], want5[k], err_msg=k)
    # the pessimism of the FakeEnv does not reach a replay: an env built pessimistic on the same model penalises the reward of
    # its own step (so the two paths really differ) and replays to the unpenalised table
    from cmbpo_amd.fake_env import FakeEnv
    pess_env = FakeEnv(_Env(29, 8), "AntSafe-v2", env._model, True, True, False, seed=3, disagreement=True, rew_pessimism=0.7)
    assert pess_env.disagreement and pess_env.rew_pessimism == 0.7
    f = dict(dtype=torch.float32, device=DEV)
    outs = []
    for e in (env, pess_env):
        out = dict(next_obs=torch.empty((130, 29), **f), rew=torch.empty(130, **f), cost=torch.empty(130, **f),
                   term=torch.empty(130, dtype=torch.uint8, device=DEV), dkl_path=torch.empty(130, **f),
                   ep_var_mean=torch.empty(130, **f), rew_var=torch.empty(130, **f), cost_var=torch.empty(130, **f))
        e.step_device(t(obs0), t(act[0]), t(inds[0]), out)
        outs.append(out)
    assert torch.equal(outs[0]["next_obs"], outs[1]["next_obs"])
    assert (outs[1]["rew"] <= outs[0]["rew"]).all() and (outs[1]["rew"] < outs[0]["rew"]).any()      # the step path does penalise
    pess = pess_env.replay(*args, lengths=lengths, model_inds=inds)
    for k in want:
        np.testing.assert_array_equal(pess[k], want[k], err_msg=k)
    for bad in (dict(model_inds=7), dict(model_inds=-1), dict(model_inds=np.zeros((3, 130), np.int32)), dict(mode="closed"),
                dict(lengths=np.zeros(130, np.int32)), dict(lengths=np.full(130, 5, np.int32))):
        with pytest.raises(ValueError):
            env.replay(*args, **bad)
    with pytest.raises(ValueError):
        env.replay(obs0[:, :5], act, rec["next_obs"][:, :, :5], rec["rew"], rec["cost"], rec["term"])


def test_windows_of_a_real_buffer_replay(hip_lib):
    """CPOBuffer.windows on an archive built by the real store / finish_path / get (the CPU suite checks the same properties on a
    host-only stand-in), and its arrays straight into FakeEnv.replay."""
    _need_gpu()
    import toyworld
    from cmbpo_amd.cpobuffer import CPOBuffer
    from test_replay_cpu import PATHS, check_windows, fill_paths
    env, D, A = _fake_env("hopper", 3)
    buf = CPOBuffer(32, 200, toyworld.Space(D), toyworld.Space(A), device=DEV)
    buf.initialize({"mu": [A], "log_std": [A]})
    fill_paths(buf, PATHS, epoch=0, tag=0, D=D, A=A)
    fill_paths(buf, PATHS[::-1], epoch=1, tag=1, terminal_last=False, D=D, A=A)
    path_of = np.repeat(np.arange(6), PATHS + PATHS[::-1])
    for H in (1, 5, 12):
        check_windows(buf, H, 100, None, 3, path_of)
    start, length = check_windows(buf, 5, 100, [1], 4, path_of)
    assert (start >= 14).all()
    _, length, win = buf.windows(5, 100, rng=np.random.default_rng(1))
    tab = env.replay(**win, model_inds=1)
    assert tab["n"][0] + tab["n_nonfinite"][0] == 100
    assert (tab["n"] + tab["n_nonfinite"] <= [(length > h).sum() for h in range(5)]).all()
