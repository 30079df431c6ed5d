"""GPU: the ensemble-voted static rules through the trainer -- CMBPO on the point environment of
test_learned_cost_gpu.py with its cost as a static rule (cost 1 on the right half plane, a clause on next_obs[0]).

One trainer is run to its first rollout round; from that round's start states (a third of them moved onto the rule's boundary,
pos_x within 0.01 of 0, where a fitted model's members can disagree at all), the model it has just fitted and ONE seed of the
sampler's generators the round is then rolled twice, with ``static_cost_members`` 'elite' (the default) and 'any', so that the two
are comparable bit for bit: the states are the same, the imagined cost under 'any' is elementwise >= the elite's, and on every
step it is the reference's maximum over the members.  A pessimistic static cost runs with the votes and is refused without; a
default trainer never calls cmbpo_rollout_rule_votes_attach."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import rule_votes_ref as ref  # noqa: E402

NAMES = ["obs", "act", "adv", "cadv", "ret", "cret", "logp", "val", "cval", "cost", "log_std", "mu"]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def _rules():
    from cmbpo_amd.statics import TaskRules, cost
    return TaskRules([cost(cols=0, lo=0.0, lo_strict=True)])          # CostPointEnv's cost: pos_x > 0


class _FirstRound(Exception):
    pass


def _build(**kw):
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
              'model_train_kwargs': dict(min_epochs=1, max_epochs=2, batch_size=128), 'static_fns': _rules()}
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
    return algo


def _to_first_round(algo):
    """Run the trainer (exploration, the first model fit, the start states of the first rollout round) up to its first
    sample_many, and return that round's start states."""
    real = algo.model_sampler.sample_many

    def stop(*a, **k):
        raise _FirstRound()

    algo.model_sampler.sample_many = stop
    with pytest.raises(_FirstRound):
        for _ in algo.train():
            pass
    algo.model_sampler.sample_many = real
    return algo.model_buf.t["cur_obs"][:algo.model_sampler.batch_size].clone()


def _round(algo, start, steps=4):
    """One rollout round from `start` with the sampler's generator re-seeded: a loop of one-call steps, every step's inputs and
    outputs kept; then finish_all_paths and get()."""
    sampler, pool = algo.model_sampler, algo.model_buf
    sampler._gen.manual_seed(1234)
    sampler.reset(start)
    per_step = []
    for _ in range(steps):
        if not (sampler.any_alive() and pool.has_room):
            break
        n = pool.n_alive
        ids = pool.t["alive_idx"][:n].cpu().numpy().copy()
        cur = pool.t["cur_obs"].cpu().numpy().copy()
        sampler.sample()
        torch.cuda.synchronize()
        k = sampler._draws[0] - 1
        per_step.append(dict(ids=ids, obs=cur, act=pool.t["act_t"].cpu().numpy().copy(),
                             inds=sampler._draws[2][k].cpu().numpy().copy(), mean=sampler._scratch[0].cpu().numpy().copy(),
                             var=sampler._scratch[1].cpu().numpy().copy(), cost=pool.t["cost_t"].cpu().numpy().copy(),
                             next_obs=pool.t["cur_obs"].cpu().numpy().copy(),
                             votes=pool.t["rule_cost_votes_t"].cpu().numpy().copy() if "rule_cost_votes_t" in pool.t else None,
                             cost_var=pool.t["cost_var_t"].cpu().numpy().copy() if "cost_var_t" in pool.t else None))
    diag = sampler.finish_all_paths()
    got = [g.cpu().numpy() for g in pool.get(as_tensors=True)[0]]
    return dict(per_step=per_step, get=dict(zip(NAMES, got)), diag=diag)


def test_any_member_cost_against_the_default_from_one_seed(hip_lib):
    _need_gpu()
    algo = _build(m_static_cost_members='any')
    env = algo.fake_env
    assert env.static_cost_members == 'any' and env.static_votes_on and not env.disagreement
    start = _to_first_round(algo)
    on_edge = torch.arange(0, start.shape[0], 3, device=start.device)
    start[on_edge, 0] = torch.linspace(-0.01, 0.01, len(on_edge), device=start.device)      # a third of the branches on the boundary
    rules, E = _rules(), env._model.num_nets
    voted = _round(algo, start)
    assert algo.model_buf.rule_votes == ('elite', 'any', True)
    env.set_static_votes(cost_members='elite')
    plain = _round(algo, start)
    assert algo.model_buf.rule_votes is None and "rule_cost_votes_t" not in algo.model_buf.t      # switched off: detached, freed
    assert len(voted["per_step"]) == len(plain["per_step"]) >= 3
    # the states are the same, bit for bit
    for k in ("obs", "act", "ret", "val", "logp", "mu"):
        np.testing.assert_array_equal(_bits(voted["get"][k]), _bits(plain["get"][k]), err_msg=k)
    # the imagined cost is elementwise >= the elite's, and somewhere greater
    assert (voted["get"]["cost"] >= plain["get"]["cost"]).all() and (voted["get"]["cost"] > plain["get"]["cost"]).any()
    mixed = 0
    for a, b in zip(voted["per_step"], plain["per_step"]):
        ids = a["ids"]
        np.testing.assert_array_equal(ids, b["ids"])
        np.testing.assert_array_equal(_bits(a["next_obs"][ids]), _bits(b["next_obs"][ids]))
        want = ref.rule_votes(rules, a["obs"], a["act"], a["mean"], a["var"], a["inds"], 6, "elite", "any", rows=ids)
        np.testing.assert_array_equal(_bits(a["cost"][ids]), _bits(want["cost"]))
        np.testing.assert_array_equal(_bits(a["cost"][ids]), _bits(want["cost_e"].max(axis=0).astype(np.float32)))   # the max over members
        np.testing.assert_array_equal(a["votes"][ids], want["cost_votes"])
        elite = ref.rule_votes(rules, b["obs"], b["act"], b["mean"], b["var"], b["inds"], 6, rows=ids)
        np.testing.assert_array_equal(_bits(b["cost"][ids]), _bits(elite["cost"]))
        mixed += int(((want["cost_votes"] > 0) & (want["cost_votes"] < E)).sum())
    assert mixed > 0
    # a pessimistic static cost: runs once the votes are on -- cost_var carries the static cost's spread
    env.set_static_votes(votes=True)
    env.set_pessimism(0.0, 0.7)
    pess = _round(algo, start)
    assert algo.model_buf.disagreement and algo.model_buf.cost_pessimism == 0.7
    for a in pess["per_step"]:
        ids = a["ids"]
        want = ref.rule_votes(rules, a["obs"], a["act"], a["mean"], a["var"], a["inds"], 6, rows=ids, dis_on=True, kappa_cost=0.7)
        np.testing.assert_array_equal(_bits(a["cost"][ids]), _bits(want["cost"]))
        np.testing.assert_array_equal(_bits(a["cost_var"][ids]), _bits(want["cost_var"]))
    assert pess["diag"]["msampler/cost_var_perstep"] > 0.0
    assert (pess["get"]["cost"] >= plain["get"]["cost"]).all() and pess["get"]["cost"].max() <= 1.0


def test_the_default_attaches_nothing_and_the_pessimistic_static_cost_needs_the_votes(hip_lib):
    _need_gpu()
    from cmbpo_amd import _lib
    lib, calls = _lib.lib(), []
    real = lib.cmbpo_rollout_rule_votes_attach

    def spy(*a):
        calls.append(a)
        return real(*a)

    lib.cmbpo_rollout_rule_votes_attach = spy
    try:
        algo = _build()
        start = _to_first_round(algo)
        out = _round(algo, start)
        assert not calls and algo.model_buf.rule_votes is None and not algo.fake_env.static_votes_on
        assert "rule_done_votes_t" not in algo.model_buf.t and out["per_step"][0]["votes"] is None
        with pytest.raises(ValueError, match="m_learn_cost"):
            _build(m_cost_pessimism=0.5)
        on = _build(m_cost_pessimism=0.5, m_static_votes=True)             # accepted with the votes (nothing is run here)
        assert on.fake_env.cost_pessimism == 0.5 and on.fake_env.static_votes_on and on.fake_env.disagreement
        assert not calls                                                  # (attached at the sampler's reset, not before)
    finally:
        lib.cmbpo_rollout_rule_votes_attach = real
