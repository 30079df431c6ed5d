"""GPU: CMBPO(m_validate_calibration=, m_calibrated_noise=) on the toy world -- the calibration keys of the
per-epoch validation, that measuring calibration reads and does not steer (policy and dynamics model after two epochs are
bitwise those of the run with m_validate_horizon alone), and the scale of the transition noise after every validation."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CAL_KEYS = ("z2_al_h1", "z2_tot_h1", "z2_tot_hH", "cover1_tot_h1", "cover2_tot_h1", "nll_tot_h1", "ep_var_h1", "al_var_h1",
            "cal_skipped")


def _two_epochs(on_epoch=None, **kw):
    import toyworld
    from cmbpo_amd import synthetic
    from cmbpo_amd.cmbpo import CMBPO
    from cmbpo_amd.cpo_policy import CPOPolicy
    from cmbpo_amd.cpo_sampler import CpoSampler
    from cmbpo_amd.cpobuffer import CPOBuffer
    np.random.seed(0)
    torch.manual_seed(0)
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
                 n_initial_exploration_steps=300, n_epochs=50, shuffle_on_device=False,
                 initial_model_train_kwargs=dict(min_epochs=3, max_epochs=6, batch_size=128),
                 model_train_kwargs=dict(min_epochs=1, max_epochs=2, batch_size=128), **kw)
    diags = []
    for d in algo.train():
        diags.append(d)
        if on_epoch is not None:
            on_epoch(algo, d)
        if len(diags) >= 2:
            break
    ws, bs = algo._model.get_weights()
    return algo, diags, policy.actor.get_flat_params(), [np.asarray(a) for a in ws + bs]


def _same_bits(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def test_calibration_reports_and_does_not_steer(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    algo, on, pi_on, w_on = _two_epochs(m_validate_horizon=5, m_validate_windows=256, m_validate_calibration=True)
    _, off, pi_off, w_off = _two_epochs(m_validate_horizon=5, m_validate_windows=256)
    assert len(on) == len(off) == 2
    for d, d_off in zip(on, off):
        for k in CAL_KEYS:
            assert "model/val_" + k in d and np.isfinite(d["model/val_" + k]), k
            assert "model/val_" + k not in d_off
        assert "model/noise_scale_mean" not in d
        assert d["model/val_cal_skipped"] >= 0 and d["model/val_z2_al_h1"] > 0 and d["model/val_al_var_h1"] > 0
        assert 0.0 <= d["model/val_cover1_tot_h1"] <= d["model/val_cover2_tot_h1"] <= 1.0
        for k, v in d_off.items():                                  # the keys of the validation as it was: the same values
            if k.startswith("model/val_"):
                assert d[k] == v or (np.isnan(d[k]) and np.isnan(v)), k
    cal = algo.last_validation["calibration"]
    assert cal["z2_al"].shape == (5, algo.obs_dim + 1) and cal["n"][0] + cal["n_skipped"][0] == algo.last_validation["n"][0]
    _same_bits(pi_on, pi_off)
    assert len(w_on) == len(w_off) == 6
    for a, b in zip(w_on, w_off):
        _same_bits(a, b)


def test_calibrated_noise_follows_the_validation(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmbpo_amd import replay
    lo, hi = 0.5, 3.0
    seen = []

    def on_epoch(algo, d):
        cal = algo.last_validation["calibration"]
        assert cal["n"][0] > 0
        want = np.sqrt(replay.temperature(cal, "al", 0, lo, hi))
        got = algo.model_sampler.noise_scale
        np.testing.assert_array_equal(got, want)
        assert got.dtype == np.float32 and got.shape == (algo.obs_dim,)
        assert (got >= np.float32(np.sqrt(np.float32(lo)))).all() and (got <= np.float32(np.sqrt(np.float32(hi)))).all()
        assert d["model/noise_scale_mean"] == float(np.mean(got))
        seen.append(got)

    _two_epochs(on_epoch, m_validate_horizon=3, m_validate_windows=256, m_validate_calibration=True, m_stochastic=True,
                m_calibrated_noise=True, m_noise_temperature_range=(lo, hi))
    assert len(seen) == 2
