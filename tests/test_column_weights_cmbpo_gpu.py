"""GPU: the class weight of the termination column in the trainer -- the two-epoch box point mass of
tests/test_term_head_cmbpo_gpu.py with CMBPO(m_term_pos_weight='balanced') against the same run with weight 1 (the behaviour
before column weights existed).

What the weight buys after so short a run is measured, not assumed: tools/probe_column_weights.py --trainer runs seeds 0 / 1 / 2
with the weight off and 'balanced', four times each, and DESIGN §3s holds the table; the constants below repeat it."""
import contextlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_term_head_cmbpo_gpu import THRESHOLD, BoxPointEnv, head_figures, imagined_rollout, run_box_loop  # noqa: E402

# Four repeats of seeds 0 / 1 / 2 (tools/probe_column_weights.py --trainer; profiles/r14/column_weights.json): the loop is
# not bitwise repeatable from run to run, so each constant is the worst of a seed's four runs -- the smallest recall gain at h = 1
# ('balanced' minus weight 1 of the same repeat) and the largest false-alarm rate with 'balanced'.  None: not measured yet.
RECALL_GAIN_MEASURED = (0.1072, 0.1604, 0.2350)      # recall 0.64-0.83 -> 0.88-1.00, 0.63-0.84 -> 0.93-1.00, 0.55-0.73 -> 0.96-0.99
FALSE_ALARM_MEASURED = (0.0903, 0.1192, 0.1296)      # with weight 1: at most 0.0257, 0.0316, 0.0257


@contextlib.contextmanager
def column_weight_keys(**keys):
    """run_box_loop builds its trainer through utils.build_experiment, which passes every algorithm key on: the keys ride in
    there, the loop itself stays the one of the termination-head test."""
    from cmbpo_amd import utils
    inner = utils.build_experiment

    def build(params, env, device=None):
        params = dict(params, algorithm_params=dict(params['algorithm_params'], kwargs=dict(params['algorithm_params']['kwargs'], **keys)))
        return inner(params, env, device=device)

    utils.build_experiment = build
    try:
        yield
    finally:
        utils.build_experiment = inner


def test_balanced_class_weight_in_the_trainer(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with column_weight_keys(m_term_pos_weight='balanced'):
        algo, seen, diags = run_box_loop(True, seed=0)
    plain, _, plain_diags = run_box_loop(True, seed=0)
    # the weight is logged, recomputed at every fit from that fit's targets, and inside its clip range
    omega = diags[-1]['model/term_pos_weight']
    assert 1.0 <= omega <= 20.0
    share = seen["term_share"][-1]
    assert omega == pytest.approx(np.clip((1 - share) / share, 1, 20), rel=1e-3), (omega, share)
    assert 'model/term_pos_weight' not in plain_diags[-1]
    assert algo._model.pos_weight is not None and algo._model.pos_weight[-1] == np.float32(omega)
    assert plain._model.pos_weight is None and plain._model.col_weight is None
    # policy and model stay finite
    assert np.isfinite(algo._policy.actor.get_flat_params()).all()
    ws, bs = algo._model.get_weights()
    assert all(np.isfinite(a).all() for a in ws + bs)
    # imagined branches end only where the head says so: the threshold keeps reading the column as it is
    ended = 0
    for st in imagined_rollout(algo)[:-1]:
        gone = ~st["alive"][st["ids"]]
        ended += int(gone.sum())
        assert (st["term"][gone] == 1).all() and (st["pred"][gone] > THRESHOLD).all()
        assert (st["pred"][~gone] <= THRESHOLD).all() and not st["term"][~gone].any()
    assert ended > 0
    recall, false_alarm, pos, neg = head_figures(algo)
    recall1, false_alarm1, _, _ = head_figures(plain)
    print("seed 0 at h = 1: 'balanced' (omega %.2f) recall %.4f false alarms %.4f; weight 1 recall %.4f false alarms %.4f; %d / %d"
          % (omega, recall, false_alarm, recall1, false_alarm1, pos, neg))
    assert pos >= 10
    assert all(g is not None for g in RECALL_GAIN_MEASURED + FALSE_ALARM_MEASURED), "the gain has not been measured yet"
    if min(RECALL_GAIN_MEASURED) > 0:       # (otherwise DESIGN §3s says so, and the test is the structure above)
        assert recall - recall1 > 0.5 * min(RECALL_GAIN_MEASURED), (recall, recall1, RECALL_GAIN_MEASURED)
        assert false_alarm <= 2.0 * max(FALSE_ALARM_MEASURED), (false_alarm, FALSE_ALARM_MEASURED)


def test_save_and_load_keep_the_four_keys(hip_lib, tmp_path):
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
                     m_hidden_dims=(128, 128), rollout_batch_size=100, maxroll=6, **kw)
    keys = dict(m_term_pos_weight='balanced', m_term_loss_weight=2.0, m_cost_loss_weight=3.0, m_pos_weight_max=15.0)
    a = make(m_learn_term=True, m_learn_cost=True, **keys)
    a._model.init_weights(np.random.RandomState(0))
    a._epoch = 3
    a.save(str(tmp_path))
    assert json.load(open(os.path.join(str(tmp_path), 'column_weights_3.json'))) == keys
    assert set(json.load(open(os.path.join(str(tmp_path), 'term_head_3.json')))) == {'threshold', 'members'}
    b = make(m_learn_term=True, m_learn_cost=True)
    assert b._column_weights == dict(m_term_pos_weight=1.0, m_term_loss_weight=1.0, m_cost_loss_weight=1.0, m_pos_weight_max=20.0)
    b.load(str(tmp_path), 3)
    assert b._column_weights == keys
    # the fit after the load sets them: termination column last, cost column after the reward
    t = np.zeros((50, 9), np.float32)
    t[:5, -1] = 1.0
    assert b._set_model_column_weights(t) == {'term_pos_weight': 9.0}
    np.testing.assert_array_equal(b._model.col_weight, np.array([1, 1, 1, 1, 1, 1, 1, 3, 2], np.float32))
    np.testing.assert_array_equal(b._model.pos_weight, np.array([1, 1, 1, 1, 1, 1, 1, 1, 9], np.float32))
    # with the defaults nothing is attached
    c = make(m_learn_term=True)
    assert c._set_model_column_weights(t[:, :8]) == {} and c._model.col_weight is None and c._model.pos_weight is None
    for bad in (dict(m_term_pos_weight=4.0), dict(m_learn_term=True, m_cost_loss_weight=2.0),
                dict(m_learn_term=True, m_term_pos_weight='auto'), dict(m_learn_term=True, m_term_pos_weight=-1.0)):
        with pytest.raises(ValueError):
            make(**bad)
