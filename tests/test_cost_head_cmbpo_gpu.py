"""GPU: the logistic learned-cost head in the trainer -- short CMBPO runs on the box point mass of
tests/test_term_head_cmbpo_gpu.py with a cost that is an indicator (1 outside an inner box), m_learn_cost=True.

  * m_cost_loss='logistic': the model's cost column is trained with the Bernoulli likelihood and read as a logit, so every
    imagined cost in the model buffer lies in [0, 1]; m_cost_pos_weight='balanced' is logged per fit, and with
    m_cost_pos_weight_undo the FakeEnv's shift is log omega; save / load reproduce the head.
  * with the defaults, policy and model are bit for bit those of a run that never named the new keys."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_term_head_cmbpo_gpu import BoxPointEnv  # noqa: E402
from test_term_head_gpu import NAMES  # noqa: E402

INNER = 0.4


class BoxCostEnv(BoxPointEnv):
    """The box point mass with an indicator cost: 1 where the mass is outside the inner box |pos|_inf <= 0.4."""

    def step(self, a):
        obs, rew, done, info = super().step(a)
        return obs, rew, done, {"cost": float(np.abs(self.pos).max() > INNER)}


def run_cost_loop(keys, seed=0, epochs=2):
    """`epochs` epochs of CMBPO(m_learn_cost=True, **keys) on BoxCostEnv through utils.build_experiment, every generator seeded."""
    from cmbpo_amd import synthetic
    from cmbpo_amd.utils import build_experiment
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    env = BoxCostEnv(seed=seed + 1)
    env.max_episode_steps = 40
    kwargs = {
        'n_env_interacts': 10 ** 9, 'eval_every_n_steps': 1, 'use_model': True, 'm_train_freq': 100, 'm_networks': 4, 'm_elites': 3,
        'm_hidden_dims': (128, 128), 'rollout_batch_size': 400, 'rollout_mode': 'schedule', 'rollout_schedule': [0, 1, 5, 5],
        'maxroll': 6, 'initial_real_samples_per_epoch': 400, 'min_real_samples_per_epoch': 400, 'batch_size_policy': 2400,
        'n_initial_exploration_steps': 2000, 'n_epochs': epochs, 'm_validate_horizon': 3, 'm_validate_windows': 1024,
        'initial_model_train_kwargs': dict(min_epochs=40, max_epochs=60, batch_size=128),
        'model_train_kwargs': dict(min_epochs=1, max_epochs=2, batch_size=128), 'm_learn_cost': True}
    kwargs.update(keys)
    params = {
        'universe': 'gym', 'task': 'default', 'environment_params': {'normalize_actions': True},
        'algorithm_params': {'type': 'CMBPO', 'kwargs': kwargs},
        'policy_params': {'type': 'cpopolicy', 'kwargs': {
            'a_hidden_layer_sizes': (128, 128), 'vf_lr': 1e-3, 'vf_hidden_layer_sizes': (128, 128), 'vf_epochs': 2,
            'vf_batch_size': 256, 'vf_ensemble_size': 3, 'vf_elites': 2, 'vf_activation': 'swish', 'vf_loss': 'MSE',
            'target_kl': 0.01, 'cost_lim': 5.0}},
        'buffer_params': {'kwargs': {'size': 2600, 'archive_size': 12000}}, 'sampler_params': {'kwargs': {}},
        'run_params': {},
    }
    algo = build_experiment(params, env, device="cuda:0")
    algo._policy.set_params(synthetic.policy_params(np.random.default_rng(seed + 2), 6, 2, 128))
    rng = np.random.RandomState(seed + 3)
    algo._policy.v.init_weights(rng)
    algo._policy.vc.init_weights(rng)
    seen = dict(cost_targets=[])
    train0 = algo._model.train

    def train(x, y, *a, **k):
        seen["cost_targets"].append(np.asarray(y[:, 7]).copy())
        return train0(x, y, *a, **k)

    algo._model.train = train
    diags = [d for d in algo.train()]
    assert len(diags) >= 1 and algo.policy_epoch == epochs
    return algo, seen, diags


def _imagined_costs(algo, steps=5, n=400):
    """One imagined rollout from archived states with the trainer's own sampler, pool and FakeEnv: the step's costs and raw
    logits of the rows stepped, and the costs get() hands to the policy update."""
    sampler, pool = algo.model_sampler, algo.model_buf
    start = algo._buffer.get_archive(['observations'])['observations'][:n]
    sampler.set_max_path_length(steps + 1)
    sampler.reset(start)
    costs, logits = [], []
    for _ in range(steps):
        if not sampler.any_alive():
            break
        ids = pool.t["alive_idx"][:pool.n_alive].long()
        sampler.sample()
        costs.append(pool.t["cost_t"][ids].cpu().numpy())
        if pool.cost_head is not None:
            logits.append(pool.t["cost_logit_t"][ids].cpu().numpy())
    sampler.finish_all_paths()
    stored = pool.get()[0][NAMES.index("cost")]
    return np.concatenate(costs), (np.concatenate(logits) if logits else None), np.asarray(stored)


def test_logistic_cost_head_in_the_trainer(hip_lib, tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmbpo_amd.cmbpo import CMBPO, balanced_pos_weight
    from cmbpo_amd.cpo_policy import CPOPolicy
    from cmbpo_amd.cpo_sampler import CpoSampler
    from cmbpo_amd.cpobuffer import CPOBuffer
    algo, seen, diags = run_cost_loop(dict(m_cost_loss='logistic', m_cost_pos_weight='balanced', m_cost_pos_weight_undo=True))
    env, model = algo.fake_env, algo._model
    assert model.out_dim == 8 and model.logistic_columns == (7,) and env.cost_loss == "logistic" and not env.predicts_term
    if model.scaler_out is not None:      # the scaler is pinned on the logit's column
        assert model.scaler_out.cached_mu[0, 7] == 0.0 and model.scaler_out.cached_var[0, 7] == 1.0
    # the targets are an indicator with both classes; the class weight is logged, recomputed from each fit's own targets
    last = seen["cost_targets"][-1]
    assert set(np.unique(last)) == {0.0, 1.0} and 0.02 < last.mean() < 0.98
    omega = diags[-1]['model/cost_pos_weight']
    assert omega == balanced_pos_weight(last, 20.0) and 1.0 < omega <= 20.0      # (the cost is the rarer class here)
    assert model.pos_weight is not None and model.pos_weight[7] == np.float32(omega)
    # ... and undone where the column is read: the shift is log omega, and the pool picks it up at its next reset
    assert env.cost_logit_shift == float(np.log(omega))
    cost, logit, stored = _imagined_costs(algo)
    assert algo.model_buf.cost_head == ("logistic", float(np.log(omega)))
    # every imagined cost is a probability; the logits are not
    assert len(cost) >= 400 and ((cost >= 0) & (cost <= 1)).all() and ((stored >= 0) & (stored <= 1)).all()
    assert np.isfinite(logit).all() and ((logit < 0) | (logit > 1)).any()
    # the costs of the rollouts the policy was trained on went through the same pool: its validation replay read probabilities
    tab = algo.last_validation
    assert (tab['mse_cost'][tab['n'] > 0] <= 1.0).all()
    print("logistic cost head, seed 0: omega %.3f, Brier score at h = 1 %.4f, cost_cm at h = 1 %s"
          % (omega, tab['mse_cost'][0], tab['cost_cm'][0].tolist()))
    # policy and model stay finite
    assert np.isfinite(algo._policy.actor.get_flat_params()).all()
    ws, bs = model.get_weights()
    assert all(np.isfinite(a).all() for a in ws + bs)
    # save / load reproduce the head: a trainer built with the defaults reads it from the file of its own
    algo.save(str(tmp_path))

    def make(**kw):
        benv = BoxCostEnv(seed=5)
        policy = CPOPolicy(benv.observation_space, benv.action_space, a_hidden_layer_sizes=(128, 128), vf_hidden_layer_sizes=(128, 128),
                           vf_ensemble_size=3, vf_elites=2, vf_activation="swish", vf_loss="MSE", device="cuda:0", max_path_length=40)
        return CMBPO(benv, policy, CPOBuffer(600, 6000, benv.observation_space, benv.action_space), sampler=CpoSampler(max_path_length=40),
                     task="default", m_networks=4, m_elites=3, m_hidden_dims=(128, 128), rollout_batch_size=100, maxroll=6, **kw)
    b = make(m_learn_cost=True)
    assert b.fake_env.cost_loss == "gaussian" and b._model.logistic_columns == () and b._cost_pos_weight == 1.0
    b.load(str(tmp_path), algo._epoch)
    assert b.fake_env.cost_loss == "logistic" and b._model.logistic_columns == (7,) and b._m_cost_loss == "logistic"
    assert b._cost_pos_weight == "balanced" and b._cost_pos_weight_undo is True
    assert b.fake_env.cost_logit_shift == env.cost_logit_shift
    ch = b.fake_env.cost_head_struct()
    assert ch.kind == 1 and ch.logit_shift == np.float32(env.cost_logit_shift)
    for x, y in zip(ws, b._model.get_weights()[0]):
        np.testing.assert_array_equal(x, y)
    if b._model.scaler_out is not None:
        np.testing.assert_array_equal(b._model.scaler_out.cached_mu, model.scaler_out.cached_mu)
    for bad, word in ((dict(m_cost_loss="logistic"), "m_learn_cost"), (dict(m_learn_cost=True, m_cost_loss="probit"), "m_cost_loss"),
                      (dict(m_cost_pos_weight="balanced"), "m_learn_cost"),
                      (dict(m_learn_cost=True, m_cost_pos_weight_undo=True), "m_cost_pos_weight_undo")):
        with pytest.raises(ValueError, match=word):
            make(**bad)


def test_defaults_are_the_run_that_never_named_the_keys(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    plain, _, plain_diags = run_cost_loop({}, epochs=1)
    named, _, named_diags = run_cost_loop(dict(m_cost_loss='gaussian', m_cost_pos_weight=1.0, m_cost_pos_weight_undo=False), epochs=1)
    for a in (plain, named):
        assert a.fake_env.cost_loss == "gaussian" and a.fake_env.cost_head_struct() is None and a.model_buf.cost_head is None
        assert a._model.logistic_columns == () and a._model.pos_weight is None and a._model.col_weight is None
        assert "cost_logit_t" not in a.model_buf.t
    assert 'model/cost_pos_weight' not in plain_diags[-1] and 'model/cost_pos_weight' not in named_diags[-1]
    np.testing.assert_array_equal(plain._policy.actor.get_flat_params(), named._policy.actor.get_flat_params())
    for x, y in zip(sum(plain._model.get_weights(), []), sum(named._model.get_weights(), [])):
        np.testing.assert_array_equal(x, y)
    # the Gaussian head's imagined costs are a regression output: nothing keeps them inside [0, 1]
    cost, logit, _ = _imagined_costs(plain)
    assert logit is None
    print("gaussian cost head, seed 0: share of imagined costs outside [0, 1]: %.4f" % float(((cost < 0) | (cost > 1)).mean()))
