"""GPU: CMBPO(m_validate_horizon=...) on the toy world -- the model/val_* diagnostics of the per-epoch open-loop validation
(DESIGN 3m), their absence when it is off, and that validation reads and does not steer: policy and dynamics model after two
epochs are bitwise those of the run without it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KEYS = ("n_h1", "n_hH", "mse_obs_h1", "mse_obs_hH", "mse_rew_hH", "cost_miss_rate", "cost_false_alarm_rate", "term_false_rate",
        "epvar_over_mse_hH", "nonfinite")


def _two_epochs(**kw):
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
        if len(diags) >= 2:
            break
    ws, bs = algo._model.get_weights()
    return algo, diags, policy.actor.get_flat_params(), [np.asarray(a) for a in ws + bs]


def test_validation_reports_and_does_not_steer(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    algo, on, pi_on, w_on = _two_epochs(m_validate_horizon=5, m_validate_windows=256)
    assert len(on) == 2
    for d in on:
        for k in KEYS:
            assert "model/val_" + k in d, k
        assert len([k for k in d if k.startswith("model/val_")]) == len(KEYS)
        assert d["model/val_n_h1"] > 0 and np.isfinite(d["model/val_mse_obs_h1"])
        assert d["model/val_n_hH"] <= d["model/val_n_h1"] <= 256
        assert "times/validate_model" in d
    tab = algo.last_validation
    assert tab["mse_obs"].shape == (5, algo.obs_dim) and tab["n"][0] + tab["n_nonfinite"][0] == 256
    algo_off, off, pi_off, w_off = _two_epochs()
    assert len(off) == 2
    for d in off:
        assert not [k for k in d if k.startswith("model/val_")] and "times/validate_model" not in d
    np.testing.assert_array_equal(pi_on.view(np.uint32), pi_off.view(np.uint32))
    assert len(w_on) == len(w_off) == 6
    for a, b in zip(w_on, w_off):
        np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))
    # validate_model by hand on a trainer built with validation off: its own horizon works, none is refused in words
    by_hand = algo_off.validate_model(horizon=3, n_windows=64)
    assert sorted(by_hand) == sorted("val_" + k for k in KEYS) and 0 < by_hand["val_n_h1"] <= 64
    assert algo_off.last_validation["n"].shape == (3,)
    with pytest.raises(ValueError, match="horizon"):
        algo_off.validate_model()
    with pytest.raises(ValueError, match="m_validate"):
        _two_epochs(m_validate_horizon=-1)
