"""GPU: the logistic termination head in the rollout and in the trainer.

  * FakeEnv.step under term_loss='logistic': the kernels are the ones of the Gaussian head, handed the float32 logit of the
    threshold; `term` and `term_votes` equal tests/term_head_ref.py on the logits with that number, bit for bit.
  * sample_many against a loop of sample, bit for bit.
  * The two-epoch box point mass of tests/test_term_head_cmbpo_gpu.py with CMBPO(m_term_loss='logistic').

What the head reaches after so short a run is measured, not assumed: tools/probe_logistic_head.py --trainer runs seeds 0 / 1 / 2,
four times each (the loop is not bitwise repeatable), for the Gaussian and the logistic head with weight 1 and 'balanced';
DESIGN §3v holds the table and the constants below repeat the logistic rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import term_head_ref as ref  # noqa: E402
from test_column_weights_cmbpo_gpu import column_weight_keys  # noqa: E402  (passes any algorithm key on to the box loop)
from test_term_head_cmbpo_gpu import BoxPointEnv, head_figures, imagined_rollout, run_box_loop  # noqa: E402
from test_term_head_gpu import DEV, HIDDEN, MODES, NAMES, T, TASK, _bits, _Env, _Space, _start, build_world_term  # noqa: E402

THRESHOLD = 0.5
# recall and false-alarm rate at h = 1 after two epochs with m_term_loss='logistic', seeds 0 / 1 / 2, the worst of four runs each
# over weight 1 and 'balanced' (tools/probe_logistic_head.py --trainer; profiles/r19/logistic_head.json).  None: not measured.
RECALL_MEASURED = (0.6552, 0.5957, 0.6372)            # all three with weight 1; 'balanced': 0.8692, 0.9083, 0.9231
FALSE_ALARM_MEASURED = (0.0737, 0.0875, 0.0935)       # all three with 'balanced'; weight 1: 0.0243, 0.0285, 0.0325


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _logistic_world(seed, E=7):
    """build_world_term's world read as a logistic model: the termination column's output weights scaled up so that the logits
    spread over a few units (the output scaler is pinned there and no longer does it)."""
    w = build_world_term(seed, E=E)
    tc = w["out_dim"] - 1
    ws = [a.copy() for a in w["ws"]]
    ws[2][:, :, tc] *= 60.0
    return dict(w, ws=ws)


def _model(w):
    from cmbpo_amd.pens import PE
    D, A = w["obs_dim"], w["act_dim"]
    E = w["ws"][0].shape[0]
    model = PE(D + A, w["out_dim"], hidden_dims=(HIDDEN, HIDDEN), num_networks=E, num_elites=len(w["elites"]), loss="MSPE",
               use_scaler_in=True, use_scaler_out=True, device=DEV, logistic_columns=[-1])
    model.set_weights(w["ws"], w["bs"], w["sc_in"], w["sc_out"])
    model.set_elites(w["elites"])
    assert model.scaler_out.cached_mu[0, -1] == 0.0 and model.scaler_out.cached_var[0, -1] == 1.0
    return model


def test_fake_env_step_reads_the_logit_against_the_logit_of_the_threshold(hip_lib):
    _need_gpu()
    from cmbpo_amd.fake_env import FakeEnv
    from cmbpo_amd.utils import logit_threshold, sigmoid
    w = _logistic_world(41, E=5)
    D, A, E = w["obs_dim"], w["act_dim"], 5
    model = _model(w)
    env = FakeEnv(_Env(D, A), "default", model, True, True, True, seed=3, predicts_term=True, term_threshold=0.5,
                  term_loss="logistic")
    rng = np.random.default_rng(9)
    n = 96
    obs = _start(10, n)
    act = rng.uniform(-1, 1, (n, A)).astype(np.float32)
    inds = rng.integers(0, E, n).astype(np.int32)
    mean, _ = model.predict_ensemble(obs, act=act)             # the logit itself in the last column
    z = mean[:, :, -1]
    assert float(np.abs(z).max()) > 0.5
    for members in MODES:
        # a probability at which this vote ends about a quarter of the rows
        taus = np.linspace(0.05, 0.95, 37)
        rate = [ref.term_head(mean, inds, D, True, np.float32(logit_threshold(t)), members)[3].mean() for t in taus]
        tau = float(taus[int(np.argmin(np.abs(np.asarray(rate) - 0.25)))])
        env.set_term_head(tau, members)
        assert env.term_threshold == tau and env.term_loss == "logistic"
        _, _, terms, info = env.step(obs, act, model_inds=inds)
        term, pred, votes, hit = ref.term_head(mean, inds, D, True, np.float32(logit_threshold(tau)), members)
        # task 'default' has no rule: term is the head's word alone
        np.testing.assert_array_equal(terms[:, 0], term.astype(bool))
        np.testing.assert_array_equal(info["term_votes"], votes)
        assert hit.any() and not hit.all()
        # info['term_pred'] is sigma of the kernel's value in float32: within 4 float32 ulps of the float64 value (one rounding
        # of the result, and the device's exp and division)
        assert info["term_pred"].dtype == np.float32
        np.testing.assert_allclose(info["term_pred"], sigmoid(pred.astype(np.float64)), rtol=4 * 1.2e-7, atol=0)
        # ... and the device's value is the logit: step_device hands it out as it is
        f = dict(dtype=torch.float32, device=DEV)
        out = dict(next_obs=torch.empty((n, D), **f), rew=torch.empty(n, **f), term=torch.empty(n, dtype=torch.uint8, device=DEV),
                   cost=torch.empty(n, **f), dkl_path=torch.empty(n, **f), ep_var_mean=torch.empty(n, **f),
                   term_pred=torch.empty(n, **f), term_votes=torch.empty(n, dtype=torch.uint8, device=DEV))
        env.step_device(torch.tensor(obs, device=DEV), torch.tensor(act, device=DEV), torch.tensor(inds, device=DEV), out)
        np.testing.assert_array_equal(_bits(out["term_pred"].cpu().numpy()), _bits(pred))
        np.testing.assert_array_equal(out["term"].cpu().numpy(), term)
    with pytest.raises(ValueError, match="strictly inside"):
        env.set_term_head(1.0, "elite")


def _hip_world(w, B, tau):
    from cmbpo_amd.cpo_policy import CPOPolicy
    from cmbpo_amd.fake_env import FakeEnv
    from cmbpo_amd.model_sampler import ModelSampler
    from cmbpo_amd.modelbuffer import ModelBuffer
    D, A = w["obs_dim"], w["act_dim"]
    policy = CPOPolicy(_Space(D), _Space(A), a_hidden_layer_sizes=(128, 128), vf_hidden_layer_sizes=(128, 128),
                       vf_ensemble_size=3, vf_elites=2, vf_activation="swish", vf_loss="MSE", device=DEV,
                       cost_gamma=0.97, cost_lam=0.5, lam=0.95)
    policy.actor.set_params(w["pol"])
    policy.v.set_weights(*w["v"])
    policy.vc.set_weights(*w["vc"])
    env = FakeEnv(_Env(D, A), TASK, _model(w), predicts_delta=True, predicts_rew=True, predicts_cost=True, predicts_term=True,
                  term_threshold=tau, term_members="elite", term_loss="logistic")
    pool = ModelBuffer(B, D, A, T, device=DEV)
    pool.initialize(policy.pi_info_shapes, gamma=0.99, lam=0.95, cost_gamma=0.97, cost_lam=0.5)
    sampler = ModelSampler(max_path_length=T + 5, batch_size=B, rollout_mode="uncertainty")
    sampler.initialize(env, policy, pool)
    sampler.set_rollout_dkl(float("inf"))
    return sampler, pool, env


def _roll(w, start, tau, how):
    sampler, pool, env = _hip_world(w, start.shape[0], tau)
    sampler._gen.manual_seed(5)
    sampler.reset(start)
    # the pool holds the number the kernel compares with: the float32 logit
    assert pool.term_head == (env.term_kernel_threshold, "elite") and "term_pred_t" in pool.t
    met = []
    while sampler.any_alive() and pool.has_room:
        if how == "many":
            sampler.sample_many()
        else:
            ids = pool.t["alive_idx"][:pool.n_alive].long()
            sampler.sample()
            met.append(pool.t["term_pred_t"][ids].cpu().numpy())
    ln = pool.t["len"].cpu().numpy().copy()
    sampler.finish_all_paths()
    return pool.get()[0], ln, (np.concatenate(met) if met else None)


def test_sample_many_equals_a_loop_of_sample_with_the_logistic_head(hip_lib):
    _need_gpu()
    from cmbpo_amd.utils import sigmoid
    B = 96
    w, start = _logistic_world(31), _start(32, B)
    _, len_never, met = _roll(w, start, 1.0 - 1e-15, "loop")        # a probability whose logit (34.5) no prediction here reaches
    assert float(np.nanmax(met)) < 34.0
    tau = float(sigmoid(np.quantile(met[np.isfinite(met)], 0.9)))
    loop, len_loop, _ = _roll(w, start, tau, "loop")
    many, len_many, _ = _roll(w, start, tau, "many")
    assert (len_loop < len_never).sum() >= B // 8 and (len_loop == T).sum() >= B // 8, (len_loop < len_never).sum()
    np.testing.assert_array_equal(len_loop, len_many)
    for k, a, b in zip(NAMES, loop, many):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=k)


def test_logistic_head_in_the_trainer(hip_lib, tmp_path):
    _need_gpu()
    from cmbpo_amd.utils import logit_threshold
    with column_weight_keys(m_term_loss='logistic'):
        algo, seen, diags = run_box_loop(True, seed=0)
    env, model = algo.fake_env, algo._model
    assert model.out_dim == 8 and model.logistic_columns == (7,) and env.term_loss == "logistic"
    assert env.term_threshold == THRESHOLD and model.col_weight is None and model.pos_weight is None
    zthr = logit_threshold(THRESHOLD)
    assert zthr == 0.0 and algo.model_buf.term_head == (0.0, "elite")
    if model.scaler_out is not None:
        assert model.scaler_out.cached_mu[0, -1] == 0.0 and model.scaler_out.cached_var[0, -1] == 1.0
    assert all(0.02 < s < 0.3 for s in seen["term_share"]), seen["term_share"]
    # branches end before the horizon exactly where term_pred_t > logit(threshold), and nowhere else
    ended = 0
    for st in imagined_rollout(algo)[:-1]:
        gone = ~st["alive"][st["ids"]]
        ended += int(gone.sum())
        assert (st["term"][gone] == 1).all() and (st["pred"][gone] > zthr).all()
        assert (st["pred"][~gone] <= zthr).all() and not st["term"][~gone].any()
    assert ended > 0, "no imagined branch ended before the horizon"
    # policy and model stay finite
    assert np.isfinite(algo._policy.actor.get_flat_params()).all()
    ws, bs = model.get_weights()
    assert all(np.isfinite(a).all() for a in ws + bs)
    recall, false_alarm, pos, neg = head_figures(algo)
    print("logistic head, seed 0: recall %.4f (%d real terminations), false-alarm rate %.4f (%d continuations) at h = 1"
          % (recall, pos, false_alarm, neg))
    assert pos >= 10
    # the choice survives save / load: a trainer built with the default reads it from the file of its own
    from cmbpo_amd.cmbpo import CMBPO
    from cmbpo_amd.cpo_policy import CPOPolicy
    from cmbpo_amd.cpo_sampler import CpoSampler
    from cmbpo_amd.cpobuffer import CPOBuffer
    algo.save(str(tmp_path))
    benv = BoxPointEnv(seed=5)
    policy = CPOPolicy(benv.observation_space, benv.action_space, a_hidden_layer_sizes=(128, 128), vf_hidden_layer_sizes=(128, 128),
                       vf_ensemble_size=3, vf_elites=2, vf_activation="swish", vf_loss="MSE", device="cuda:0", max_path_length=40)
    b = CMBPO(benv, policy, CPOBuffer(600, 6000, benv.observation_space, benv.action_space), sampler=CpoSampler(max_path_length=40),
              task="default", m_networks=4, m_elites=3, m_hidden_dims=(128, 128), rollout_batch_size=100, maxroll=6,
              m_learn_term=True)
    assert b.fake_env.term_loss == "gaussian" and b._model.logistic_columns == ()
    b.load(str(tmp_path), algo._epoch)
    assert b.fake_env.term_loss == "logistic" and b._model.logistic_columns == (7,) and b._m_term_loss == "logistic"
    assert b.fake_env.term_head_struct().threshold == 0.0
    for x, y in zip(ws, b._model.get_weights()[0]):
        np.testing.assert_array_equal(x, y)
    if b._model.scaler_out is not None:
        np.testing.assert_array_equal(b._model.scaler_out.cached_mu, model.scaler_out.cached_mu)
    with pytest.raises(ValueError, match="m_learn_term"):
        CMBPO(benv, policy, CPOBuffer(600, 6000, benv.observation_space, benv.action_space), sampler=CpoSampler(max_path_length=40),
              task="default", m_networks=4, m_elites=3, m_hidden_dims=(128, 128), rollout_batch_size=100, maxroll=6,
              m_term_loss="logistic")
    assert all(r is not None for r in RECALL_MEASURED + FALSE_ALARM_MEASURED), "the head has not been measured yet"
    assert recall > 0.5 * min(RECALL_MEASURED), (recall, RECALL_MEASURED)
    assert false_alarm <= 2.0 * max(FALSE_ALARM_MEASURED), (false_alarm, FALSE_ALARM_MEASURED)
