"""GPU: predictive calibration in the model replay -- cmbpo_replay_calibrate / _calib_finish on crafted arrays and
cmbpo_replay_run_calibrated / FakeEnv.replay(calibration=True) against a Python loop of FakeEnv.step_device, both held against
the NumPy specification tests/replay_calibration_ref.py; ModelSampler.set_noise_scale.

Both sides work on the same float32 inputs, so verdicts and counts are compared exactly.  Every term of the two z^2 sums, of
sum v_bar and of sum s2 is computed by the same IEEE float64 operations in the same order on both sides and is non-negative; a
sum of n such terms added in two different orders differs by at most n 2^-52 relative.  The terms of the two log sums come from
two implementations of log, each within 1 ulp (2^-52 relative of a term), and may be negative: the sums differ by at most
2 2^-52 sum|term| from the logs plus n 2^-52 sum|term| from the order, which n 2^-50 sum|term| covers for every n >= 1."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import replay_calibration_ref as cref  # noqa: E402
import replay_ref as ref  # noqa: E402

DEV = "cuda:0"
PRED = ("next_obs", "rew", "term", "cost", "dkl_path", "ep_var_mean")
CAL_ARRAYS = ("part_sum", "part_cnt", "sums", "counts")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _check_calibration(got, want, tag=""):
    """got: the dict of cmbpo_amd.replay.calibration_table; want: a table of the reference."""
    from cmbpo_amd import replay
    np.testing.assert_array_equal(got["n"], want["n"], err_msg=tag + "n")
    np.testing.assert_array_equal(got["n_skipped"], want["n_skipped"], err_msg=tag + "n_skipped")
    for j, k in enumerate(replay.CALIB_COUNT_KEYS):
        np.testing.assert_array_equal(got[k], want["counts"][:, j], err_msg=tag + k)
    n = want["n"].astype(np.float64)[:, None]
    for j, k in enumerate(replay.CALIB_SUM_KEYS):
        w = want["sums"][:, j]
        assert np.isfinite(got[k]).all(), tag + k
        if k.startswith("sum_log"):
            bound = n * 2.0 ** -50 * want["abs_log"][:, j - 2]
        else:
            assert (w >= 0).all(), tag + k
            bound = n * 2.0 ** -52 * w
        err = np.abs(got[k] - w)
        assert (err <= bound).all(), (tag + k, float(err.max()), got[k][err > bound], w[err > bound])
    # the derived entries are the host's arithmetic on the raw ones
    raw = dict(n=got["n"], sums=np.stack([got[k] for k in replay.CALIB_SUM_KEYS], axis=1),
               counts=np.stack([got[k] for k in replay.CALIB_COUNT_KEYS], axis=1))
    for k, v in cref.derived(raw).items():
        np.testing.assert_array_equal(got[k], v, err_msg=tag + k)


def _bytes_equal(a, b, keys, where):
    for k in keys:
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=f"{where}: {k}")


# ----------------------------------------------------------------------------------------------------------------------
# 1. the single calls on crafted arrays: no model
# ----------------------------------------------------------------------------------------------------------------------
def _crafted_run(B, E, D, O, seed):
    """H = 2 steps of calibrate -> compare on made-up predictions, means and variances, with ragged `alive` on entry, one row
    of every bad kind at h = 0 and a whole dead slot; then both finishes.  Returns (buffers, reference table, skipped at h = 0)."""
    from cmbpo_amd.replay import ReplayBuffers
    rng = np.random.default_rng(seed)
    H, A = 2, 2
    C = D + 1
    obs0 = rng.standard_normal((B, D)).astype(np.float32)
    rec = dict(next_obs=rng.standard_normal((H, B, D)).astype(np.float32), rew=rng.standard_normal((H, B)).astype(np.float32),
               cost=(rng.random((H, B)) < 0.3).astype(np.float32), term=(rng.random((H, B)) < 0.2).astype(np.uint8))
    lengths = rng.integers(1, H + 1, B).astype(np.int32)
    rb = ReplayBuffers(obs0, np.zeros((H, B, A), np.float32), rec["next_obs"], rec["rew"], rec["cost"], rec["term"], lengths=lengths,
                       mode="one_step", ensemble=E, out_dim=O, device=DEV, calibration=True)
    elite = rng.integers(0, E, (H, B)).astype(np.int32)
    rb.set_elite(elite)
    # every entry of every slot is written on every call: whatever the partials held is gone
    rb.c["part_sum"].fill_(float("nan"))
    rb.c["part_cnt"].fill_(-7)
    alive = rng.random(B) < 0.8
    alive[:min(B, 16)] = True
    if B > 128:
        alive[64:128] = False                                    # a slot whose rows are all dead
    rb.t["alive"].copy_(torch.from_numpy(alive.astype(np.uint8)))
    tab, ctab = ref.new_table(H, D), cref.new_table(H, D)
    cur = obs0.copy()
    n_bad = 0
    for h in range(H):
        pred = dict(next_obs=(rec["next_obs"][h] + rng.standard_normal((B, D)).astype(np.float32) * 0.3).astype(np.float32),
                    rew=rng.standard_normal(B).astype(np.float32), cost=rng.random(B).astype(np.float32),
                    term=(rng.random(B) < 0.2).astype(np.uint8), ep_var_mean=rng.random(B).astype(np.float32),
                    dkl_path=rng.random(B).astype(np.float32))
        mean = (rng.standard_normal((E, B, O)) * 0.3).astype(np.float32)
        var = np.exp(rng.uniform(-6.0, 2.0, (E, B, O))).astype(np.float32)
        if h == 0 and B >= 16:
            other = lambda b: (int(elite[0, b]) + 1) % E         # a member that is not the row's elite (E = 1: the elite)
            var[0, 2, 0] = np.inf
            var[E - 1, 5, D - 1] = np.nan
            var[other(7), 7, D] = 0.0                            # the reward column
            var[0, 9, 1 % D] = -1.0
            mean[other(11), 11, D // 2] = np.nan
            n_bad = 5
            pred["next_obs"][13, 0] = np.nan                     # the plain table's n_nonfinite: in neither count here,
            var[0, 13, 0] = 0.0                                  # whatever its variances are
            pred["rew"][14] = np.inf
            if O > C:                                            # a learned-cost column is not calibrated: anything goes there
                var[:, 3, C] = np.nan
                mean[0, 4, O - 1] = np.inf
        if B > 128:
            mean[:, 64:128], var[:, 64:128] = np.nan, np.nan     # dead rows: never read
        for k, v in pred.items():
            rb.step_outputs()[k].copy_(torch.from_numpy(v))
        rb.t["mean"].copy_(torch.from_numpy(mean))
        rb.t["var"].copy_(torch.from_numpy(var))
        rb.calibrate(h)
        rb.compare(h)
        cref.calibrate(ctab, h, alive, pred, mean, var, rec, elite[h], D)
        ref.compare(tab, h, cur, alive, pred, rec, lengths, ref.ONE_STEP)
        np.testing.assert_array_equal(rb.t["alive"].cpu().numpy().astype(bool), alive)
    rb.finish()
    rb.calib_finish()
    torch.cuda.synchronize()
    return rb, ctab, tab, n_bad


@pytest.mark.parametrize("E", [1, 3, 7])
@pytest.mark.parametrize("D,O", [(3, 4), (29, 30), (29, 31), (300, 301)])
def test_single_calls_on_crafted_arrays(hip_lib, D, O, E):
    _need_gpu()
    for B in (1, 63, 64, 65, 257):
        tag = f"B={B} "
        seed = zlib.crc32(f"crafted/{B}/{E}/{D}/{O}".encode())
        rb, want, plain, n_bad = _crafted_run(B, E, D, O, seed)
        got = rb.calibration_table()
        _check_calibration(got, want, tag)
        assert got["n_skipped"][0] == n_bad and got["n_skipped"][1] == 0, tag
        plain_got = rb.table()
        # the rows of the plain table are those that entered plus those skipped; a non-finite prediction is in neither
        np.testing.assert_array_equal(plain_got["n"], plain["n"])
        np.testing.assert_array_equal(got["n"] + got["n_skipped"], plain_got["n"], err_msg=tag)
        if B >= 16:
            assert plain_got["n_nonfinite"][0] == 2 and got["n"][0] > 0, tag
        if B > 128:                                              # the dead slot wrote zeros over the NaN / -7 it held
            assert not rb.c["part_sum"][:, 1].cpu().numpy().any() and not rb.c["part_cnt"][:, 1].cpu().numpy().any()
        assert np.isfinite(rb.c["part_sum"].cpu().numpy()).all() and (rb.c["part_cnt"].cpu().numpy() >= 0).all()
        again = _crafted_run(B, E, D, O, seed)[0]
        _bytes_equal(rb.c, again.c, CAL_ARRAYS, tag + "two runs")


def test_synthetic_calibrated_case_on_the_device(hip_lib):
    """The CPU suite's calibrated case at B = 20 000 through the kernel, same bounds."""
    _need_gpu()
    from cmbpo_amd.replay import ReplayBuffers
    from test_replay_calibration_cpu import check_synthetic
    B, D, E = 20000, 3, 3
    out = []
    for shrink in (1.0, 0.25):
        pred, mean, var, rec, elite = cref.synthetic_case(B, D, E, seed=7, shrink=shrink)
        z = np.zeros((1, B), np.float32)
        rb = ReplayBuffers(np.zeros((B, D), np.float32), np.zeros((1, B, 1), np.float32), rec["next_obs"], rec["rew"], z, z,
                           mode="one_step", ensemble=E, out_dim=D + 1, device=DEV, calibration=True)
        rb.set_elite(elite[None])
        rb.t["p_next_obs"].copy_(torch.from_numpy(pred["next_obs"]))
        rb.t["p_rew"].copy_(torch.from_numpy(pred["rew"]))
        rb.t["p_cost"].zero_()
        rb.t["mean"].copy_(torch.from_numpy(mean))
        rb.t["var"].copy_(torch.from_numpy(var))
        rb.calibrate(0)
        rb.calib_finish()
        torch.cuda.synchronize()
        got = rb.calibration_table()
        want = cref.new_table(1, D)
        cref.calibrate(want, 0, np.ones(B, bool), pred, mean, var, rec, elite, D)
        _check_calibration(got, want, f"shrink={shrink} ")
        assert got["n"][0] == B and got["n_skipped"][0] == 0
        out.append(got)
    d, s = out
    check_synthetic(d["z2_al"][0], d["cover1_al"][0], d["cover2_al"][0], s["z2_al"][0])


# ----------------------------------------------------------------------------------------------------------------------
# 2. the whole replay against a loop of FakeEnv.step_device
# ----------------------------------------------------------------------------------------------------------------------
class _Space:
    def __init__(self, d):
        self.shape = (d,)


class _Env:
    def __init__(self, D, A):
        self.observation_space, self.action_space = _Space(D), _Space(A)


_ENVS = {}


def _fake_env(E, learned_cost):
    if (E, learned_cost) not in _ENVS:
        from cmbpo_amd.fake_env import FakeEnv
        from cmbpo_amd.pens import PE
        w = cref.replay_world(E, learned_cost)
        np.random.seed(5)
        model = PE(w["D"] + w["A"], w["O"], hidden_dims=(128, 128), num_networks=E, num_elites=max(E - 2, 2), loss="MSPE",
                   use_scaler_in=True, use_scaler_out=True, device=DEV)
        model.set_weights(w["ws"], w["bs"], w["sc_in"], w["sc_out"])
        _ENVS[E, learned_cost] = (FakeEnv(_Env(w["D"], w["A"]), "AntSafe-v2", model, True, True, learned_cost, seed=3), w)
    return _ENVS[E, learned_cost]


def _buffers(env, case, mode, calibration):
    from cmbpo_amd.replay import ReplayBuffers
    obs0, act, rec, lengths, _ = case
    return ReplayBuffers(obs0, act, rec["next_obs"], rec["rew"], rec["cost"], rec["term"], lengths=lengths, mode=mode,
                         ensemble=env._model.num_nets, out_dim=env.output_dim, device=DEV, calibration=calibration)


def _reference_loop(env, case, mode):
    """The replay as a Python loop of the existing device step; both tables from the NumPy specifications."""
    obs0, act, rec, lengths, inds = case
    H, B, D = rec["next_obs"].shape
    E, O = env._model.num_nets, env.output_dim
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    f = dict(dtype=torch.float32, device=DEV)
    out = dict(next_obs=torch.empty((B, D), **f), rew=torch.empty(B, **f), term=torch.empty(B, dtype=torch.uint8, device=DEV),
               cost=torch.empty(B, **f), dkl_path=torch.empty(B, **f), ep_var_mean=torch.empty(B, **f))
    scratch = (torch.empty((E, B, O), **f), torch.empty((E, B, O), **f))
    act_d, inds_d = t(act), t(inds)
    tab, ctab = ref.new_table(H, D), cref.new_table(H, D)
    cur, alive = obs0.copy(), np.ones(B, bool)
    for h in range(H):
        env.step_device(t(cur), act_d[h], inds_d[h], out, scratch=scratch)
        pred = {k: out[k].cpu().numpy() for k in PRED}
        cref.calibrate(ctab, h, alive, pred, scratch[0].cpu().numpy(), scratch[1].cpu().numpy(), rec, inds[h], D)
        ref.compare(tab, h, cur, alive, pred, rec, lengths, mode)
    return tab, ctab, cur, alive


@pytest.mark.parametrize("mode", ["open_loop", "one_step"])
@pytest.mark.parametrize("learned_cost", [False, True], ids=["rules", "learned_cost"])
@pytest.mark.parametrize("E", [3, 7])
def test_run_calibrated_matches_the_step_device_loop(hip_lib, E, learned_cost, mode):
    _need_gpu()
    env, w = _fake_env(E, learned_cost)
    handle, task = env._model.mlp.handle, env._task_id
    for B in (65, 257):
        for H in (1, 3):
            tag = f"B={B} H={H} "
            rng = np.random.default_rng(zlib.crc32(f"whole/{E}/{learned_cost}/{mode}/{B}/{H}".encode()))
            case = cref.recording(rng, B, H, w["D"], w["A"]) + (rng.integers(0, E, (H, B)).astype(np.int32),)
            inds_d = torch.from_numpy(case[4]).to(DEV)
            a = _buffers(env, case, mode, True)
            a.run_calibrated(handle, task, E, inds_d)
            torch.cuda.synchronize()
            tab, ctab, cur, alive = _reference_loop(env, case, mode)
            got = a.calibration_table()
            _check_calibration(got, ctab, tag)
            assert (ctab["n_skipped"] == 0).all() and ctab["n"][0] == B, tag          # (the reference alone decides this)
            np.testing.assert_array_equal(got["n"], tab["n"], err_msg=tag)
            np.testing.assert_array_equal(a.t["cur_obs"].cpu().numpy().view(np.uint32), cur.view(np.uint32), err_msg=tag)
            np.testing.assert_array_equal(a.t["alive"].cpu().numpy().astype(bool), alive, err_msg=tag)
            if H == 3:
                assert 0 < ctab["n"][2] < B, tag                                       # windows end on the way, some reach the end
            # the plain replay on the same inputs: its table and final state, bit for bit
            p = _buffers(env, case, mode, False)
            p.run(handle, task, E, inds_d)
            _bytes_equal(a.t, p.t, ("sums", "counts", "part_sum", "part_cnt", "cur_obs", "alive"), tag + "plain run")
            # the single calls, bit for bit; a second run
            c = _buffers(env, case, mode, True)
            c.set_elite(inds_d)
            for h in range(H):
                env.step_device(c.t["cur_obs"], c.t["act"][h], inds_d[h], c.step_outputs(), scratch=(c.t["mean"], c.t["var"]))
                c.calibrate(h)
                c.compare(h)
            c.finish()
            c.calib_finish()
            b = _buffers(env, case, mode, True)
            b.run_calibrated(handle, task, E, inds_d)
            torch.cuda.synchronize()
            for other, where in ((c, "single calls"), (b, "two runs")):
                _bytes_equal(a.c, other.c, CAL_ARRAYS, tag + where)
                _bytes_equal(a.t, other.t, ("sums", "counts", "cur_obs", "alive"), tag + where)


def test_fake_env_replay_with_and_without_calibration(hip_lib):
    _need_gpu()
    E = 7
    env, w = _fake_env(E, False)
    rng = np.random.default_rng(21)
    B, H = 130, 4
    case = cref.recording(rng, B, H, w["D"], w["A"]) + (rng.integers(0, E, (H, B)).astype(np.int32),)
    obs0, act, rec, lengths, inds = case
    args = (obs0, act, rec["next_obs"], rec["rew"], rec["cost"], rec["term"])
    plain = _buffers(env, case, "open_loop", False)
    plain.run(env._model.mlp.handle, env._task_id, E, torch.from_numpy(inds).to(DEV))
    want = plain.table()
    off = env.replay(*args, lengths=lengths, model_inds=inds)
    explicit_off = env.replay(*args, lengths=lengths, model_inds=inds, calibration=False)
    on = env.replay(*args, lengths=lengths, model_inds=inds, calibration=True)
    assert sorted(off) == sorted(explicit_off) == sorted(want) and "calibration" not in off
    assert sorted(on) == sorted(list(want) + ["calibration"])
    for k in want:
        for got in (off, explicit_off, on):
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    cal = on["calibration"]
    _, ctab, _, _ = _reference_loop(env, case, "open_loop")
    _check_calibration(cal, ctab)
    assert cal["z2_al"].shape == (H, w["D"] + 1) and cal["n"].shape == (H,)
    np.testing.assert_array_equal(cal["n"] + cal["n_skipped"], want["n"])
    # the generator of the replay's own elite draws is used the same way by both forms
    state = env._replay_rng.bit_generator.state
    first = env.replay(*args, lengths=lengths)
    env._replay_rng.bit_generator.state = state
    second = env.replay(*args, lengths=lengths, calibration=True)
    for k in want:
        np.testing.assert_array_equal(first[k], second[k], err_msg=k)
    # buffers built without calibration refuse the calls in words
    with pytest.raises(ValueError, match="calibration=False"):
        plain.calibrate(0)
    with pytest.raises(ValueError, match="calibration"):
        from cmbpo_amd.replay import ReplayBuffers
        ReplayBuffers(obs0, act, rec["next_obs"], rec["rew"], rec["cost"], rec["term"], device=DEV, calibration=True)


# ----------------------------------------------------------------------------------------------------------------------
# 3. the scale of the transition noise
# ----------------------------------------------------------------------------------------------------------------------
def _rollout(scale="unset", explicit=None, stochastic=True):
    """A rollout of a HalfCheetahSafe world of 1000 branches x 7 steps with the sampler's own draws from one seed.
    scale: passed to set_noise_scale unless "unset".  explicit: the factors a loop of sample(xi=...) applies to the draws."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from test_rollout_sampler_gpu import hip_world
    from worlds import build_world
    from cmbpo_amd import synthetic
    task, B, T = "HalfCheetahSafe-v2", 1000, 8
    w = build_world(77, task, 128)
    start = synthetic.start_states(np.random.default_rng(78), B, task)
    sampler, pool = hip_world(w, task, T, "schedule", float("inf"), B, 128)
    sampler.stochastic = stochastic
    sampler._gen.manual_seed(5)
    if not isinstance(scale, str):
        sampler.set_noise_scale(scale)
    sampler.reset(start)
    steps = 0
    while sampler.any_alive() and pool.has_room:
        if explicit is None:
            sampler.sample()
        else:
            ck, k = sampler._next_draws()[:2]                   # the chunk the step is about to use, not advanced
            idx = pool.t["alive_idx"][:pool.n_alive].long()
            xi = ck[3][k][idx] * torch.from_numpy(explicit).to(DEV)        # float32 product: one rounding per element
            sampler.sample(xi=xi.cpu().numpy())
        steps += 1
    sampler.finish_all_paths()
    res, _ = pool.get()
    return steps, [np.ascontiguousarray(r.cpu().numpy() if isinstance(r, torch.Tensor) else r) for r in res], sampler


def test_noise_scale(hip_lib):
    _need_gpu()
    steps, base, sampler = _rollout()
    assert steps == 7 and sampler.noise_scale is None
    D = sampler.pool.obs_dim
    same = lambda a, b: all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))
    assert same(base, _rollout(scale=None)[1])
    assert same(base, _rollout(scale=np.ones(D, np.float32))[1])
    assert same(base, _rollout(explicit=np.ones(D, np.float32))[1])          # the loop of sample(xi=) is the same rollout
    s = np.random.default_rng(4).uniform(0.5, 2.0, D).astype(np.float32)
    _, scaled, smp = _rollout(scale=torch.from_numpy(s))
    np.testing.assert_array_equal(smp.noise_scale, s)
    assert not same(base, scaled)
    assert same(scaled, _rollout(explicit=s)[1])
    # the same scale again keeps the chunk in hand, another one drops it
    chunk = smp._draws
    smp.set_noise_scale(s.copy())
    assert smp._draws is chunk
    smp.set_noise_scale(s * np.float32(2.0))
    assert smp._draws is None
    # refusals in words
    det = _rollout(stochastic=False)[2]
    with pytest.raises(ValueError, match="stochastic=False"):
        det.set_noise_scale(np.ones(D, np.float32))
    det.set_noise_scale(None)
    for bad in (np.ones(D + 1, np.float32), np.ones((D, 1), np.float32), np.zeros(D, np.float32), np.full(D, np.nan, np.float32)):
        with pytest.raises(ValueError, match="set_noise_scale"):
            smp.set_noise_scale(bad)
