"""GPU: the particle replay -- cmbpo_replay_particles / _finish on crafted predictions against the NumPy reference
(tests/particles_ref.py), cmbpo_replay_run_particles against the loop of FakeEnv.step_device(noise=, model_inds=) and single calls,
the model replayed against recordings it made itself, and FakeEnv.replay(particles=S).

Counts, rank histograms, cur_obs and alive are compared exactly.  The float64 sums are sums of the same float32-rounded terms as
the reference's, added in another order: at most ~1e5 additions of non-negative numbers, each order within n 2^-53 of the true
sum, so rtol 1e-10 holds with four orders of magnitude to spare.

The statistical bounds of the self-replay are those of the closed-form case in tests/test_particles_cpu.py (q, x_p i.i.d.): a
recording the model sampled itself is exchangeable with its particles, so per (horizon, column) the rank is uniform on 0..S:
chi2 below the 1e-6 / n_hist quantile of chi-square with S degrees of freedom, outlier_rate in [0.15, 0.30] around 2 / 9."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import particles_ref as pref  # noqa: E402

DEV = "cuda:0"
F32, U8 = np.float32, np.uint8


class _Space:
    def __init__(self, d):
        self.shape = (d,)


class _Env:
    def __init__(self, D, A):
        self.observation_space, self.action_space = _Space(D), _Space(A)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(x):
    x = x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x.view(np.uint64) if x.dtype == np.float64 else x


# ------------------------------------------------------------------------------------------------------------------
# 1. the kernel on crafted arrays
# ------------------------------------------------------------------------------------------------------------------
SHAPES = [(37, 8, 11, 3),      # a last workgroup that is partly filled (296 rows = 4 x 64 + 40), 8 windows per workgroup
          (5, 64, 3, 2),       # one window per workgroup
          (130, 2, 29, 2)]     # 32 windows per workgroup, 260 rows


def _crafted(B, S, D, H, seed):
    rng = np.random.default_rng(seed)
    R = B * S
    rec = dict(next_obs=rng.standard_normal((H, B, D)).astype(F32), rew=rng.standard_normal((H, B)).astype(F32),
               cost=(rng.random((H, B)) < 0.4).astype(F32), term=(rng.random((H, B)) < 0.1).astype(U8))
    rec["term"][:, [0, 2, 3, B - 1]] = 0                     # (the windows below that carry a crafted value)
    rec["term"][0, 1] = 1                                    # a recorded terminal mid-window: window 1 ends after h = 0
    length = rng.integers(1, H + 1, B).astype(np.int32)      # ragged
    length[:4] = H
    preds = []
    for h in range(H):
        p = dict(p_next_obs=(rec["next_obs"][h].repeat(S, axis=0) + rng.standard_normal((R, D))).astype(F32),
                 p_rew=(rec["rew"][h].repeat(S) + rng.standard_normal(R)).astype(F32),
                 p_cost=rng.random(R).astype(F32), p_term=(rng.random(R) < 0.3).astype(U8))
        # ties: a particle that IS the recorded value ranks as not below; a window whose particles all are
        p["p_next_obs"][0 * S + 1, D - 1] = rec["next_obs"][h, 0, D - 1]
        p["p_rew"][0 * S] = rec["rew"][h, 0]
        p["p_next_obs"][3 * S:4 * S, 0] = rec["next_obs"][h, 3, 0]
        preds.append(p)
    preds[0]["p_next_obs"][2 * S + S - 1, D // 2] = np.nan      # one NaN in a particle row: window 2 ends at h = 0
    preds[H - 1]["p_rew"][0 * S + 1] = np.inf                   # one non-finite p_rew: window 0 at the last step
    preds[0]["p_rew"][(B - 1) * S] = np.nan                     # ... and one in the last window, in the partly filled workgroup
    obs0 = rng.standard_normal((B, D)).astype(F32)
    return rec, length, preds, obs0


@pytest.mark.parametrize("mode", ["open_loop", "one_step"])
@pytest.mark.parametrize("B,S,D,H", SHAPES)
def test_kernel_on_crafted_predictions(hip_lib, B, S, D, H, mode):
    _need_gpu()
    from cmbpo_amd.replay import ParticleBuffers
    rec, length, preds, obs0 = _crafted(B, S, D, H, zlib.crc32(f"particles/{B}/{S}/{D}/{H}".encode()))
    act = np.zeros((H, B, 1), F32)
    pb = ParticleBuffers(S, obs0, act, rec["next_obs"], rec["rew"], rec["cost"], rec["term"], lengths=length, mode=mode, device=DEV)
    assert pb.n_part == -(-B * S // 64)
    cur, alive = obs0.repeat(S, axis=0).copy(), np.ones(B * S, U8)
    np.testing.assert_array_equal(_bits(pb.t["cur_obs"]), _bits(cur))
    want_s, want_c = [], []
    for h in range(H):
        for k, v in preds[h].items():
            pb.t[k].copy_(torch.from_numpy(v))
        before, was_alive = cur.copy(), alive.copy()
        pb.particles(h)
        s, c = pref.step(h, S, mode, rec["next_obs"], rec["rew"], rec["cost"], rec["term"], length, cur, alive, **preds[h])
        want_s.append(s)
        want_c.append(c)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(pb.t["alive"].cpu().numpy(), alive, err_msg="alive after h = %d" % h)
        np.testing.assert_array_equal(_bits(pb.t["cur_obs"]), _bits(cur), err_msg="cur_obs after h = %d" % h)
        dead = alive == 0
        np.testing.assert_array_equal(_bits(pb.t["cur_obs"])[dead], _bits(before)[dead])      # rows of dead windows: untouched
        assert (was_alive >= alive).all()
    pb.finish()
    torch.cuda.synchronize()
    sums, counts = pb.t["sums"].cpu().numpy(), pb.t["counts"].cpu().numpy()
    np.testing.assert_array_equal(counts, np.stack(want_c))
    assert np.isfinite(sums).all()
    np.testing.assert_allclose(sums, np.stack(want_s), rtol=1e-10, atol=0)
    tab = pb.table()
    assert tab["n"][0] == B - 2 and tab["n_nonfinite"][0] == 2 and tab["n_nonfinite"][H - 1] >= 1
    np.testing.assert_array_equal(tab["rank_hist"].sum(axis=2), np.broadcast_to(tab["n"][:, None], (H, D + 1)))
    assert tab["rank_hist"][:, 0, 0].sum() >= 1           # the window whose particles all tie ranked 0
    np.testing.assert_array_equal(counts, pb.t["part_cnt"].sum(dim=1).cpu().numpy())       # the finish call: the slots, added


# ------------------------------------------------------------------------------------------------------------------
# models
# ------------------------------------------------------------------------------------------------------------------
_ENVS = {}


def _fake_env(E, head, never_ends=False, out_scale=1.0):
    """A FakeEnv over a 128-wide probabilistic ensemble of E members with small steps at AntSafe's widths: AntSafe's rules, or
    (never_ends) a rule table that never terminates; head: a learned termination column behind the reward."""
    key = (E, head, never_ends, out_scale)
    if key in _ENVS:
        return _ENVS[key]
    from cmbpo_amd import synthetic
    from cmbpo_amd.fake_env import FakeEnv
    from cmbpo_amd.pens import PE
    from cmbpo_amd.statics import TaskRules, healthy
    D, A = synthetic.ENV_DIMS["AntSafe-v2"]
    task = TaskRules([healthy(cols=0, lo=-1e30, hi=1e30)], require_finite=False, cost_on_term=False) if never_ends else "AntSafe-v2"
    O = D + 1 + int(head)
    rng = np.random.default_rng(zlib.crc32(f"particles-model/{E}/{head}/{never_ends}".encode()))
    ws, bs = synthetic.ensemble_weights(rng, E, D + A, 128, 2 * O, bias_scale=0.05, out_scale=out_scale)
    mu, var = np.zeros((1, O), F32), np.full((1, O), 2.5e-3, F32)      # steps of ~0.05 per column
    if head:
        mu[0, O - 1], var[0, O - 1] = 0.4, 1.0
    np.random.seed(5)
    model = PE(D + A, O, hidden_dims=(128, 128), num_networks=E, num_elites=max(E - 2, 2), loss="MSPE", use_scaler_in=True,
               use_scaler_out=True, device=DEV)
    model.set_weights(ws, bs, synthetic.scaler(rng, D + A), (mu, var))
    kw = dict(predicts_term=True, term_threshold=0.5, term_members="elite") if head else {}
    env = FakeEnv(_Env(D, A), task, model, True, True, False, seed=3, **kw)
    _ENVS[key] = (env, D, A)
    return _ENVS[key]


def _recording(rng, B, H, D, A):
    obs0 = (rng.standard_normal((B, D)) * 0.1).astype(F32)
    obs0[:, 0] = rng.uniform(0.3, 0.9, B).astype(F32)
    nxt = (obs0[None] + np.cumsum(rng.standard_normal((H, B, D)) * 0.05, axis=0)).astype(F32)
    rec = dict(next_obs=nxt, rew=rng.standard_normal((H, B)).astype(F32), cost=(rng.random((H, B)) < 0.3).astype(F32),
               term=(rng.random((H, B)) < 0.1).astype(U8))
    return obs0, rng.uniform(-1, 1, (H, B, A)).astype(F32), rec, rng.integers(1, H + 1, B).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------
# 2. the run is the loop
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["open_loop", "one_step"])
@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("E", [1, 7])
def test_run_is_the_loop_of_single_calls_bitwise_and_repeats(hip_lib, E, head, mode):
    """cmbpo_replay_run_particles against FakeEnv.step_device(noise=, model_inds=) on the R rows and single cmbpo_replay_particles
    calls, then the finish call; two runs.  The post step takes 2..8 members (csrc/fakeenv_post.hip, tests/test_term_draws_gpu.py
    holds the message), so at E = 1 the run is the loop in what it refuses: the post step's words, under this entry's name."""
    _need_gpu()
    from cmbpo_amd import _lib
    from cmbpo_amd.replay import ParticleBuffers
    env, D, A = _fake_env(7, head)
    B, S, H = 37, 8, 3
    R = B * S
    rng = np.random.default_rng(zlib.crc32(f"particles-run/{E}/{head}/{mode}".encode()))
    obs0, act, rec, length = _recording(rng, B, H, D, A)
    xi = rng.standard_normal((H, B, S, D)).astype(F32)
    elite = torch.from_numpy(rng.integers(0, E, (H, R)).astype(np.int32)).to(DEV)
    new = lambda: ParticleBuffers(S, obs0, act, rec["next_obs"], rec["rew"], rec["cost"], rec["term"], lengths=length, mode=mode,
                                  ensemble=7, out_dim=env.output_dim, noise=xi, device=DEV)
    th, ch = env.term_head_struct(), env.cost_head_struct()
    if E == 1:
        # a genuine one-member model: the loop's side cannot even be set up (FakeEnv takes ensembles only), the run entry
        # passes the post step's refusal on before anything is launched
        from cmbpo_amd import synthetic
        from cmbpo_amd.fake_env import FakeEnv
        from cmbpo_amd.pens import PE
        O = env.output_dim
        ws, bs = synthetic.ensemble_weights(rng, 1, D + A, 128, 2 * O, bias_scale=0.05)
        one = PE(D + A, O, hidden_dims=(128, 128), num_networks=1, num_elites=1, loss="MSPE", use_scaler_in=True, use_scaler_out=True,
                 device=DEV)
        one.set_weights(ws, bs, synthetic.scaler(rng, D + A), (np.zeros((1, O), F32), np.full((1, O), 2.5e-3, F32)))
        with pytest.raises(NotImplementedError, match="probabilistic ensemble"):
            FakeEnv(_Env(D, A), "AntSafe-v2", one, True, True, False, seed=3)
        a = ParticleBuffers(S, obs0, act, rec["next_obs"], rec["rew"], rec["cost"], rec["term"], lengths=length, mode=mode,
                            ensemble=1, out_dim=O, noise=xi, device=DEV)
        with pytest.raises(_lib.CmbpoHipError, match=r"cmbpo_replay_run_particles: cmbpo_fakeenv_post\w*: ensemble 1 not in \[2, 8\]"):
            a.run(one.mlp.handle, env._task_id, 1, elite, term_head=th, cost_head=ch)
        torch.cuda.synchronize()
        assert not a.t["counts"].any() and bool((a.t["alive"] == 1).all())       # refused before anything ran
        return
    a, b, c = new(), new(), new()
    for x in (a, b):
        x.run(env._model.mlp.handle, env._task_id, E, elite, term_head=th, cost_head=ch)
    np.testing.assert_array_equal(_bits(c.t["act"]), _bits(torch.from_numpy(act).repeat_interleave(S, dim=1)))
    for h in range(H):
        env.step_device(c.t["cur_obs"], c.t["act"][h], elite[h], c.step_outputs(), scratch=(c.t["mean"], c.t["var"]), noise=c.t["xi"][h])
        c.particles(h)
    c.finish()
    torch.cuda.synchronize()
    for k in ("sums", "counts", "part_sum", "part_cnt", "cur_obs", "alive", "p_next_obs", "p_rew", "p_cost", "p_term"):
        np.testing.assert_array_equal(_bits(a.t[k]), _bits(c.t[k]), err_msg="run against the loop: " + k)
        np.testing.assert_array_equal(_bits(a.t[k]), _bits(b.t[k]), err_msg="two runs: " + k)
    tab = a.table()
    assert tab["n"][0] == B and 0 < tab["n"][H - 1] < B and np.isfinite(tab["crps"][0]).all()
    if head:
        assert tab["sum_brier_term"].sum() > 0          # predicted terminations were measured ...
        assert tab["n"][1] == int(((length > 1) & (rec["term"][0] == 0)).sum())      # ... and ended nothing


# ------------------------------------------------------------------------------------------------------------------
# 3. the model as its own truth
# ------------------------------------------------------------------------------------------------------------------
_SELF = {}


def _self_recording():
    """H = 3 steps of W = 1024 windows, rolled forward by the model itself: FakeEnv.step with N(0, 1) noise and a member per row
    and step drawn from the elites (seed A), under rules that never terminate."""
    if _SELF:
        return _SELF["v"]
    env, D, A = _fake_env(7, False, never_ends=True, out_scale=0.3)
    W, H = 1024, 3
    rng = np.random.default_rng(0xA)
    elites = np.asarray(env._model.elite_inds, np.int32)
    obs0 = (rng.standard_normal((W, D)) * 0.1).astype(F32)
    act = rng.uniform(-1, 1, (H, W, A)).astype(F32)
    nxt, rew, cost, term = [], [], [], []
    cur = obs0
    for h in range(H):
        o, r, t, info = env.step(cur, act[h], noise=rng.standard_normal((W, D)).astype(F32),
                                 model_inds=elites[rng.integers(0, len(elites), W)])
        nxt.append(o.astype(F32)); rew.append(r[:, 0].astype(F32)); term.append(t[:, 0].astype(U8))
        cost.append(np.asarray(info["cost"])[:, 0].astype(F32))
        cur = nxt[-1]
    assert not np.stack(term).any()
    _SELF["v"] = (env, D, dict(obs0=obs0, actions=act, next_obs=np.stack(nxt), rewards=np.stack(rew), costs=np.stack(cost),
                               terminals=np.stack(term)))
    return _SELF["v"]


def test_the_model_covers_a_recording_it_sampled_itself(hip_lib):
    _need_gpu()
    from scipy.stats import chi2
    env, D, win = _self_recording()
    S, H, W = 8, 3, 1024
    tab = env.replay(**win, particles=S, particle_seed=0xB)["particles"]
    np.testing.assert_array_equal(tab["n"], [W] * H)
    np.testing.assert_array_equal(tab["n_nonfinite"], [0] * H)
    bound = chi2.isf(1e-6 / (H * D), S)
    for h in range(H):
        print("h = %d: chi2 max %.2f (bound %.2f), outlier_rate %.4f .. %.4f, spread_skill %.3f .. %.3f"
              % (h, tab["chi2"][h, :D].max(), bound, tab["outlier_rate"][h, :D].min(), tab["outlier_rate"][h, :D].max(),
                 tab["spread_skill"][h, :D].min(), tab["spread_skill"][h, :D].max()))
    assert (tab["chi2"][:, :D] < bound).all()
    assert (tab["outlier_rate"][:, :D] >= 0.15).all() and (tab["outlier_rate"][:, :D] <= 0.30).all()


@pytest.mark.parametrize("scale,low,high", [(0.5, 0.35, 1.0), (2.0, 0.0, 0.13)])
def test_a_rescaled_noise_shows_in_the_outlier_rate(hip_lib, scale, low, high):
    """The same replay through a single member with the noise halved / doubled: the cloud is too narrow / too wide at h = 0."""
    _need_gpu()
    env, D, win = _self_recording()
    m = int(np.asarray(env._model.elite_inds)[0])
    tab = env.replay(**win, model_inds=m, particles=8, particle_seed=0xB, noise_scale=np.full(D, scale, F32))["particles"]
    out = tab["outlier_rate"][0, :D]
    print("noise_scale %.1f, member %d: outlier_rate at h = 0 %.4f .. %.4f" % (scale, m, out.min(), out.max()))
    assert (out > low).all() and (out < high).all()


# ------------------------------------------------------------------------------------------------------------------
# 4. / 5. FakeEnv.replay(particles=S)
# ------------------------------------------------------------------------------------------------------------------
def _same(a, b, tag=""):
    assert sorted(a) == sorted(b), tag
    for k in a:
        if isinstance(a[k], dict):
            _same(a[k], b[k], tag + k + "/")
        elif isinstance(a[k], np.ndarray):
            np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=tag + k)
        else:
            assert a[k] == b[k], tag + k


def _states(env):
    return (repr(env._replay_rng.bit_generator.state), repr(env._rng.bit_generator.state), repr(np.random.get_state()),
            torch.get_rng_state().clone(), torch.cuda.get_rng_state(DEV).clone())


def _states_equal(a, b):
    return a[:3] == b[:3] and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])


def test_replay_with_particles_adds_a_pass_and_changes_nothing_else(hip_lib):
    _need_gpu()
    env, D, A = _fake_env(7, True)
    B, H, S = 70, 4, 8
    rng = np.random.default_rng(77)
    obs0, act, rec, length = _recording(rng, B, H, D, A)
    win = dict(obs0=obs0, actions=act, next_obs=rec["next_obs"], rewards=rec["rew"], costs=rec["cost"], terminals=rec["term"],
               lengths=length)
    # the elite draws of the plain pass come from _replay_rng: the same state in front of both calls, the same state behind them
    state = env._replay_rng.bit_generator.state
    plain = env.replay(**win, calibration=True)
    behind = repr(env._replay_rng.bit_generator.state)
    env._replay_rng.bit_generator.state = state
    before = _states(env)
    both = env.replay(**win, calibration=True, particles=S, particle_seed=11)
    after = _states(env)
    assert repr(env._replay_rng.bit_generator.state) == behind
    assert before[1:3] == after[1:3] and torch.equal(before[3], after[3]) and torch.equal(before[4], after[4])
    part = both.pop("particles")
    _same(plain, both)
    assert part["S"] == S and part["rank_hist"].shape == (H, D + 1, S + 1) and part["n"][0] == B
    # given members: no generator of the environment, of NumPy or of torch moves at all
    inds = rng.integers(0, 7, (H, B))
    before = _states(env)
    again = env.replay(**win, model_inds=inds, particles=S, particle_seed=11)["particles"]
    assert _states_equal(before, _states(env))
    _same(part, again)                                       # particle_seed reproduces (the plain pass's members do not enter)
    other = env.replay(**win, model_inds=inds, particles=S, particle_seed=12)["particles"]
    assert not np.array_equal(other["sum_abs"], part["sum_abs"])
    # the draws of a seed, handed in: the documented recipe
    gen = torch.Generator(device=DEV)
    gen.manual_seed(11)
    xi = torch.randn((H, B, S, D), generator=gen, dtype=torch.float32, device=DEV)
    elites = np.asarray(env._model.elite_inds, np.int32)
    m = elites[np.random.default_rng(np.random.SeedSequence(11, spawn_key=(1,))).integers(0, len(elites), size=(H, B, S))]
    injected = env.replay(**win, model_inds=inds, particles=S, particle_noise=xi, particle_inds=m)["particles"]
    _same(part, injected)
    injected = env.replay(**win, model_inds=inds, particles=S, particle_noise=xi.cpu().numpy(), particle_inds=torch.from_numpy(m))
    _same(part, injected["particles"])
    # noise_scale: one float32 rounding per element -- the scaled draws handed in are the scaled seed
    sc = rng.uniform(0.5, 2.0, D).astype(F32)
    scaled = env.replay(**win, model_inds=inds, particles=S, particle_seed=11, noise_scale=sc)["particles"]
    by_hand = env.replay(**win, model_inds=inds, particles=S, particle_noise=xi * torch.from_numpy(sc).to(DEV), particle_inds=m)
    _same(scaled, by_hand["particles"])
    assert not np.array_equal(scaled["sum_var"], part["sum_var"])
    # an int: every particle through that member
    one = env.replay(**win, model_inds=3, particles=S, particle_seed=11)["particles"]
    _same(one, env.replay(**win, model_inds=3, particles=S, particle_noise=xi, particle_inds=np.full((H, B, S), 3))["particles"])


def test_refusals_in_words(hip_lib):
    _need_gpu()
    env, D, A = _fake_env(7, True)
    obs0, act, rec, length = _recording(np.random.default_rng(5), 9, 2, D, A)
    win = dict(obs0=obs0, actions=act, next_obs=rec["next_obs"], rewards=rec["rew"], costs=rec["cost"], terminals=rec["term"])
    for S in (3, 128, 1, -4):
        with pytest.raises(ValueError, match="power of two in 2..64"):
            env.replay(**win, particles=S)
    with pytest.raises(ValueError, match="particles together with votes=True"):
        env.replay(**win, particles=4, votes=True)
    for kw in (dict(particle_seed=1), dict(noise_scale=np.ones(D, F32)), dict(particle_noise=np.zeros((2, 9, 4, D), F32)),
               dict(particle_inds=np.zeros((2, 9, 4), np.int32))):
        with pytest.raises(ValueError, match="need particles=S"):
            env.replay(**win, **kw)
    with pytest.raises(ValueError, match="particle_noise must be"):
        env.replay(**win, particles=4, particle_noise=np.zeros((2, 9, 8, D), F32))
    with pytest.raises(ValueError, match="particle_inds must be"):
        env.replay(**win, particles=4, particle_inds=np.full((2, 9, 4), 7))
    with pytest.raises(ValueError, match="noise_scale must be"):
        env.replay(**win, particles=4, noise_scale=np.zeros(D, F32))
    assert "particles" in env.replay(**win, particles=4, votes=False)
