"""GPU: the CMBPO trainer loop with ``start_state_sampling='device'`` -- the start states of every imagined-rollout round
drawn by CPOBuffer.sample_start_states straight into the rollout state -- on the toy world of tests/toyworld.py.  As in
tests/test_cmbpo_loop_gpu.py the checks are structural invariants of one short run, plus: every start state of every
round is a row of the archive."""
import numpy as np
import pytest

import toyworld

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _build(start_state_sampling=None):
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
    kw = {} if start_state_sampling is None else dict(start_state_sampling=start_state_sampling)
    algo = CMBPO(env, policy, buf, sampler=CpoSampler(max_path_length=T), task="default", n_env_interacts=10 ** 9,
                 eval_every_n_steps=1, m_train_freq=100, m_networks=4, m_elites=3, m_hidden_dims=(128, 128),
                 rollout_batch_size=400, rollout_mode="schedule", rollout_schedule=[0, 1, 4, 4], maxroll=6,
                 initial_real_samples_per_epoch=150, min_real_samples_per_epoch=100, batch_size_policy=2500,
                 n_initial_exploration_steps=300, n_epochs=50,
                 initial_model_train_kwargs=dict(min_epochs=3, max_epochs=6, batch_size=128),
                 model_train_kwargs=dict(min_epochs=1, max_epochs=2, batch_size=128), **kw)
    return algo, policy, buf


def test_default_is_the_host_path_and_the_keyword_is_checked(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    algo, _, buf = _build()
    assert algo._start_state_sampling == 'host' and buf._dev is None
    with pytest.raises(ValueError, match="start_state_sampling"):
        _build("gpu")


def test_cmbpo_runs_three_epochs_with_device_start_states(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    algo, policy, buf = _build("device")
    rounds = []
    draw = buf.sample_start_states

    def recording(pol, batch_size, **kw):
        out = draw(pol, batch_size, **kw)
        assert out.data_ptr() == algo.model_buf.t["cur_obs"].data_ptr(), "written into the rollout state itself"
        rounds.append(dict(rows=out.cpu().numpy().copy(), idx=buf.last_start["idx"].cpu().numpy().copy(),
                           kl=buf.last_start["kl"].cpu().numpy().copy(), epochs=buf.epoch_archive.copy(),
                           archive=buf.arch_dict["observations"].copy()))
        return out
    buf.sample_start_states = recording
    choice = np.random.choice
    host_draws = []
    np.random.choice = lambda *a, **k: host_draws.append(1) or choice(*a, **k)
    p0 = policy.actor.get_flat_params().copy()
    diags = []
    try:
        for d in algo.train():
            diags.append(d)
            if len(diags) >= 3:
                break
    finally:
        np.random.choice = choice
    assert len(diags) == 3 and algo.policy_epoch >= 3
    assert not host_draws, "the host chain's np.random.choice draws are not taken"
    first = diags[0]
    for k in ("model/samples_added", "model/n_real_samples", "model/poolm_batch_size", "model/LossPi_m",
              "model/LossPi_r", "times/epoch_rollout_model", "times/train", "OptimCase", "KL", "RetEpAverage",
              "LossVEnsemble", "model/DynEns/val_loss"):
        assert k in first, (k, sorted(first))
    assert 0.9 * (2500 - 150) <= first["model/samples_added"] <= 1.1 * 2500
    assert first["model/n_real_samples"] >= 100
    assert algo._model.finalized and len(algo._model.elite_inds) == 3 and algo._model.train_grad_updates > 0
    assert float(np.abs(policy.actor.get_flat_params() - p0).max()) > 0
    for k, v in first.items():
        if isinstance(v, (float, np.floating)):
            assert np.isfinite(v) or k.startswith("model/max") or "Min" in k or "Max" in k, k
    # every start state of every round is a row of the archive as it was at that round
    assert len(rounds) >= 3
    for r in rounds:
        assert r["rows"].shape == (400, toyworld.ToyEnv.D)
        assert np.all(r["epochs"][r["idx"]] >= 0)
        np.testing.assert_array_equal(r["rows"], r["archive"][r["idx"]])
        assert np.all(np.isfinite(r["kl"])) and np.all(r["kl"] >= 0)
    # later rounds see the epochs the real sampler added in between: the mirror follows the archive
    assert len(set(np.unique(rounds[-1]["epochs"])) - {-1}) > len(set(np.unique(rounds[0]["epochs"])) - {-1})
    np.testing.assert_array_equal(buf.device_archive()["epochs"].cpu().numpy(), buf.epoch_archive)
    np.testing.assert_array_equal(buf.device_archive()["observations"].cpu().numpy(), buf.arch_dict["observations"])
