"""GPU: CMBPO(m_imagined_weight=, m_trust_var=) on the toy world -- the weights the trainer builds from the model buffer's
trust weights reach update_policy (and update_critic of a vf_weighted policy) in step with the samples; with the defaults
nothing carries weights."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _two_epochs(policy_kw=None, **kw):
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
                       cost_lim=5.0, target_kl=0.01, **(policy_kw or {}))
    policy.set_params(synthetic.policy_params(np.random.default_rng(2), D, A, 128))
    rng = np.random.RandomState(1)
    policy.v.init_weights(rng)
    policy.vc.init_weights(rng)
    seen = dict(policy=[], critic=[])
    up, uc = policy.update_policy, policy.update_critic

    def spy_policy(buf_inputs, weights=None):
        seen["policy"].append((len(buf_inputs[0]), weights))
        return up(buf_inputs, weights=weights)

    def spy_critic(buf_inputs, weights=None, **k):
        seen["critic"].append((len(buf_inputs[0]), weights))
        return uc(buf_inputs, weights=weights, **k)

    policy.update_policy, policy.update_critic = spy_policy, spy_critic
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
    return algo, diags, seen


def _check_weights(n, w, diag):
    assert isinstance(w, torch.Tensor) and tuple(w.shape) == (n,) and w.dtype == torch.float32
    w = w.cpu().numpy()
    n_real = int((w == 1.0).sum())
    assert 0 < n_real < n and np.all(w[:n_real] == 1.0)             # the real rows lead, as in train_samples
    im = w[n_real:]
    assert np.all(im > 0.0) and np.all(im <= 0.5) and im.min() < 0.5   # 0.5 x a trust weight in (0, 1]
    share = float(im.astype(np.float64).sum() / (im.astype(np.float64).sum() + n_real))
    return share


def test_trainer_hands_trust_weights_to_the_updates(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    kw = dict(m_imagined_weight=0.5, m_iv_gae=True, m_trust_var=1e-2)
    algo, diags, seen = _two_epochs(policy_kw=dict(vf_weighted=True), **kw)
    assert len(diags) == 2 and len(seen["policy"]) == 2 and len(seen["critic"]) == 2
    for (n, w), (nc, wc), d in zip(seen["policy"], seen["critic"], diags):
        share = _check_weights(n, w, d)
        assert nc == n and wc is w                                   # the critics see the same weights
        assert "policy/weight_sum_share_imagined" in d
    # (a yielded row blends the epochs it covers; with eval_every_n_steps=1 it covers one)
    np.testing.assert_allclose(diags[-1]["policy/weight_sum_share_imagined"], share, rtol=1e-5)
    assert "model/poolm_weight_mean" in diags[-1] and 0 < diags[-1]["model/poolm_weight_min"] <= diags[-1]["model/poolm_weight_mean"] <= 1
    assert algo.model_buf.trust_var == 1e-2

    # a policy without vf_weighted: the policy update is weighted, the critics' is not; a constant imagined weight needs no
    # variance table
    _, diags, seen = _two_epochs(m_imagined_weight=0.25)
    for (n, w), (nc, wc) in zip(seen["policy"], seen["critic"]):
        w = w.cpu().numpy()
        assert set(np.unique(w)) == {np.float32(0.25), np.float32(1.0)} and len(w) == n
        assert wc is None


def test_defaults_carry_no_weights_and_bad_switches_are_refused(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    algo, diags, seen = _two_epochs()
    assert len(seen["policy"]) == 2
    assert all(w is None for _, w in seen["policy"]) and all(w is None for _, w in seen["critic"])
    assert not [k for d in diags for k in d if k.startswith("policy/weight") or "poolm_weight" in k]
    assert algo.model_buf.last_weights is None
    with pytest.raises(ValueError, match="m_iv_gae"):
        _two_epochs(m_trust_var=1e-2)
    with pytest.raises(ValueError, match="m_imagined_weight"):
        _two_epochs(m_imagined_weight=0.0)
