"""GPU: the learned termination head in the trainer -- two epochs of CMBPO(m_learn_term=True) on a point mass whose episode
ends when it leaves a box, a rule of the state no task of statics.py knows: under task='default' an imagined branch ends before
the horizon only if the model says so.

How good the head is after so short a run is measured, not assumed: DESIGN 3r holds recall and false-alarm rate of the one-step
row of the validation replay for three seeds (RECALL_MEASURED below repeats the recalls); the test asserts half the smallest."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BOX, THRESHOLD, MEMBERS = 0.5, 0.5, "elite"
# recall at h = 1 after two epochs, seeds 0 / 1 / 2 (tools/probe_term_head.py --trainer)
RECALL_MEASURED = (0.7328, 0.6477, 0.6061)      # false-alarm rates 0.0110, 0.0064, 0.0086; head off: 0 / 0


class _Space:
    def __init__(self, d):
        self.shape = (d,)


class BoxPointEnv:
    """2-D point mass with drag: obs = [pos, vel, sin / cos of a clock], reward = -|pos|.  The episode ends when the mass leaves
    the box |pos|_inf <= 0.5 (about one step in twelve under a random policy); the environment has no time limit of its own."""

    def __init__(self, seed=0):
        self.observation_space, self.action_space = _Space(6), _Space(2)
        self.rng = np.random.RandomState(seed)
        self.t = 0

    def _obs(self):
        return np.concatenate([self.pos, self.vel, [np.sin(0.1 * self.t), np.cos(0.1 * self.t)]]).astype(np.float32)

    def reset(self):
        self.pos, self.vel, self.t = self.rng.uniform(-0.3, 0.3, 2), np.zeros(2), 0
        return self._obs()

    def step(self, a):
        a = np.clip(np.asarray(a, np.float64).reshape(-1)[:2], -1, 1)
        self.vel = 0.9 * self.vel + 0.3 * a + 0.01 * self.rng.standard_normal(2)
        self.pos = self.pos + 0.2 * self.vel
        self.t += 1
        return self._obs(), -float(np.abs(self.pos).sum()), bool(np.abs(self.pos).max() > BOX), {"cost": 0.0}

    def close(self):
        pass


def run_box_loop(m_learn_term, seed=0, epochs=2):
    """`epochs` epochs of CMBPO on BoxPointEnv through utils.build_experiment (which passes the three m_*term* keys on)."""
    from cmbpo_amd import synthetic
    from cmbpo_amd.utils import build_experiment
    np.random.seed(seed)
    env = BoxPointEnv(seed=seed + 1)
    env.max_episode_steps = 40
    kwargs = {
        'n_env_interacts': 10 ** 9, 'eval_every_n_steps': 1, 'use_model': True, 'm_train_freq': 100, 'm_networks': 4, 'm_elites': 3,
        'm_hidden_dims': (128, 128), 'rollout_batch_size': 400, 'rollout_mode': 'schedule', 'rollout_schedule': [0, 1, 5, 5],
        'maxroll': 6, 'initial_real_samples_per_epoch': 400, 'min_real_samples_per_epoch': 400, 'batch_size_policy': 2400,
        'n_initial_exploration_steps': 2000, 'n_epochs': epochs, 'm_validate_horizon': 3, 'm_validate_windows': 1024,
        'initial_model_train_kwargs': dict(min_epochs=40, max_epochs=60, batch_size=128),
        'model_train_kwargs': dict(min_epochs=1, max_epochs=2, batch_size=128)}
    if m_learn_term:
        kwargs.update(m_learn_term=True, m_term_threshold=THRESHOLD, m_term_members=MEMBERS)
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
    seen = dict(target_cols=[], term_share=[])
    train0 = algo._model.train

    def train(x, y, *a, **k):
        seen["target_cols"].append(int(y.shape[1]))
        seen["term_share"].append(float(y[:, -1].mean()))
        return train0(x, y, *a, **k)

    algo._model.train = train
    diags = [d for d in algo.train()]
    assert len(diags) >= 1 and algo.policy_epoch == epochs
    return algo, seen, diags


def head_figures(algo):
    """(recall, false-alarm rate, real terminations, real continuations) of the one-step row of the last validation replay."""
    t1 = algo.last_validation['term_cm'][0]
    pos, neg = int(t1[1].sum()), int(t1[0].sum())
    return (t1[1, 1] / pos if pos else float('nan')), (t1[0, 1] / neg if neg else float('nan')), pos, neg


def imagined_rollout(algo, steps=5, n=400):
    """One imagined rollout from archived states with the trainer's own sampler, pool and FakeEnv, no budget: per step the
    slots stepped, term and (with the head) term_pred, and the alive mask behind the step."""
    sampler, pool = algo.model_sampler, algo.model_buf
    start = algo._buffer.get_archive(['observations'])['observations'][:n]
    sampler.set_max_path_length(steps + 1)      # (a path of max_path_length L stores L - 1 steps)
    sampler.reset(start)
    out = []
    cp = lambda x: x.cpu().numpy().copy()
    for s in range(steps):
        if not sampler.any_alive():
            break
        ids = cp(pool.t["alive_idx"][:pool.n_alive])
        sampler.sample()
        st = dict(ids=ids, term=cp(pool.t["term_t"])[ids], alive=np.asarray(pool.alive_paths).astype(bool).copy())
        if pool.term_head is not None:
            st["pred"] = cp(pool.t["term_pred_t"])[ids]
        out.append(st)
    sampler.finish_all_paths()
    pool.get()
    return out


def test_head_off_no_imagined_branch_ends_before_the_horizon(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    algo, seen, _ = run_box_loop(False)
    assert algo._model.out_dim == 7 and not algo.fake_env.predicts_term and all(c == 7 for c in seen["target_cols"])
    steps = imagined_rollout(algo)
    assert len(steps) == 5
    for st in steps[:-1]:
        assert not st["term"].any() and st["alive"].all()
    recall, false_alarm, pos, _ = head_figures(algo)
    assert pos > 0 and recall == 0.0 and false_alarm == 0.0          # by construction: nothing predicts a termination


def test_head_on_branches_end_where_the_model_says_so(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    algo, seen, diags = run_box_loop(True, seed=0)
    env = algo.fake_env
    assert algo._model.out_dim == 8 and env.predicts_term and env.output_dim == 8
    assert (env.term_threshold, env.term_members) == (THRESHOLD, MEMBERS) and algo.model_buf.term_head == (THRESHOLD, MEMBERS)
    assert seen["target_cols"] and all(c == 8 for c in seen["target_cols"])       # [delta obs | reward | term]
    assert all(0.02 < s < 0.3 for s in seen["term_share"]), seen["term_share"]    # the targets hold the real terminations
    steps = imagined_rollout(algo)
    ended = 0
    for st in steps[:-1]:
        gone = ~st["alive"][st["ids"]]
        ended += int(gone.sum())
        # task 'default' has no rule: a branch that ended before the horizon ended on the head's word
        assert (st["term"][gone] == 1).all() and (st["pred"][gone] > THRESHOLD).all()
        assert (st["pred"][~gone] <= THRESHOLD).all() and not st["term"][~gone].any()
    assert ended > 0, "no imagined branch ended before the horizon"
    # policy and model stay finite
    assert np.isfinite(algo._policy.actor.get_flat_params()).all()
    ws, bs = algo._model.get_weights()
    assert all(np.isfinite(a).all() for a in ws + bs)
    last = diags[-1]
    assert np.isfinite(last['model/val_term_recall_h1']) and np.isfinite(last['model/val_term_false_alarm_h1'])
    recall, false_alarm, pos, neg = head_figures(algo)
    print("term head, seed 0: recall %.3f (%d real terminations), false-alarm rate %.3f (%d continuations) at h = 1"
          % (recall, pos, false_alarm, neg))
    assert pos >= 10
    assert all(r is not None for r in RECALL_MEASURED), "the recall has not been measured yet"
    assert recall > 0.5 * min(RECALL_MEASURED), (recall, RECALL_MEASURED)


def test_save_and_load_keep_threshold_and_vote(hip_lib, tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmbpo_amd.cmbpo import CMBPO
    from cmbpo_amd.cpo_policy import CPOPolicy
    from cmbpo_amd.cpo_sampler import CpoSampler
    from cmbpo_amd.cpobuffer import CPOBuffer

    def make(**kw):
        env = BoxPointEnv(seed=5)
        policy = CPOPolicy(env.observation_space, env.action_space, a_hidden_layer_sizes=(128, 128), vf_hidden_layer_sizes=(128, 128),
                           vf_ensemble_size=3, vf_elites=2, vf_activation="swish", vf_loss="MSE", device="cuda:0", max_path_length=40)
        buf = CPOBuffer(600, 6000, env.observation_space, env.action_space)
        return CMBPO(env, policy, buf, sampler=CpoSampler(max_path_length=40), task="default", m_networks=4, m_elites=3,
                     m_hidden_dims=(128, 128), rollout_batch_size=100, maxroll=6, m_learn_term=True, **kw)
    a = make(m_term_threshold=0.35, m_term_members="majority")
    a._model.init_weights(np.random.RandomState(0))
    a._epoch = 3
    a.save(str(tmp_path))
    b = make()
    assert (b.fake_env.term_threshold, b.fake_env.term_members) == (0.5, "elite")
    b.load(str(tmp_path), 3)
    assert (b.fake_env.term_threshold, b.fake_env.term_members) == (0.35, "majority")
    for x, y in zip(a._model.get_weights()[0], b._model.get_weights()[0]):
        np.testing.assert_array_equal(x, y)
    with pytest.raises(ValueError):
        make(m_term_members="most")
    with pytest.raises(ValueError):
        make(m_term_threshold=float("inf"))
