"""CMBPO trainer loop -- host-side mirror of ``algorithms/cmbpo.py:30-542``.

The epoch structure is the reference's: Boltzmann-weighted start states from the archive -> imagined rollouts until the
model batch is full -> real-environment sampling (as many steps as the model's current uncertainty asks for) ->
dynamics-model training every ``m_train_freq`` real samples -> ``update_real_c`` / ``update_policy`` /
``update_critic`` on real + imagined samples -> diagnostics.  Everything data-parallel in it runs in the HIP kernels
behind the other modules of this package; imagined samples stay on the device from the rollout to the updates
(``ModelBuffer.get(as_tensors=True)``), the real samples of an epoch are uploaded once.

Differences from the reference, all outside the numerics: gtimer stamps are a plain ``time.perf_counter`` dict; the
logger is the in-memory ``logger.EpochLogger``.

``m_learn_cost=True`` (``algorithms/cmbpo.py:46,123``) gives the dynamics ensemble one more output column trained on the
real costs (``format_samples_for_dyn(append_c=True)``, ``:470``) and has ``FakeEnv`` take the cost of an imagined sample
from it (``predicts_cost=True``, ``:137-142``) instead of the task's cost rule: the only way an imagined sample of a
task without such a rule carries a cost at all.

``m_stochastic=True`` samples the imagined transitions from the elite member's predictive distribution N(mean, var)
instead of placing them at its mean (``ModelSampler(stochastic=True)``; the reference has the hook in
``models/fake_env.py:103-108`` but never switches it on).  The uncertainty calibration stays deterministic.

``m_iv_gae=True`` weights the k-step returns of every imagined branch by the inverse of the epistemic variance accumulated
on the way to them (``ModelBuffer(iv_gae=True, iv_eps=m_iv_eps)``: the weighted branch of the reference's
``discount_cumsum``, which its model buffer prepares for but never calls).  Real samples are not affected.

``m_disagreement=True`` measures the ensemble's disagreement on the reward and the learned-cost column along the imagined
rollouts (``msampler/rew_var_perstep``, ``msampler/cost_var_perstep``); ``m_rew_pessimism`` / ``m_cost_pessimism`` (kappa >= 0,
> 0 implies the measurement) make the imagined reward ``r - kappa_r * sigma_r`` and the imagined learned cost
``c + kappa_c * sigma_c``: a constraint is no longer satisfied on the say-so of one member (``FakeEnv(disagreement=...)``).
``m_cost_pessimism > 0`` needs ``m_learn_cost=True`` or the static votes.  ``m_static_term_members`` / ``m_static_cost_members``
('elite' | 'any' | 'majority', the cost also 'mean') and ``m_static_votes`` (measure only) let the ensemble vote on the task's
static termination / cost rule in the imagined rollouts (``FakeEnv(static_*_members=, static_votes=)``); with
``m_disagreement`` ``msampler/cost_var_perstep`` then carries the static cost's spread.  The validation replay keeps the elite's
rule.  Real samples and the rollout lengths are not affected.

``m_value_disagreement=True`` measures the variance over the members of both critics at every state an imagined rollout
evaluates (``msampler/v_var_perstep``, ``msampler/vc_var_perstep``); ``m_v_pessimism`` / ``m_vc_pessimism`` (kappa >= 0, > 0
implies the measurement) make every imagined value ``V - kappa_v * sigma_v`` and every imagined cost value
``VC + kappa_vc * sigma_vc`` -- stored values and the bootstraps that close a branch alike, so the GAE sees them
(``ModelBuffer.set_value_disagreement``).  It needs critics the one-launch critic kernel takes (two hidden layers of 128, at
most 4 members, at most 64 inputs).  Real samples, ``get_action_outs`` and the rollout lengths are not affected.  With
``vf_clipping`` the critics' losses are clipped around the buffer's old values, which for imagined samples are then the
PENALISED ones.  Critic targets built from penalised bootstraps pull the cost critic's mean upward, by at most
``gamma^T / (1 - gamma^T)`` of ``kappa sigma`` over a T-step branch; the unpenalised real-sample targets anchor it.

``m_validate_horizon=H`` (> 0; the reference has nothing like it) replays, every epoch, ``m_validate_windows`` windows of up to H
consecutive real steps of that epoch through the model with the recorded actions and reports how the prediction error
compounds, which real costs and terminations the imagined signal misses, and whether the epistemic variance is the size of
the error (``model/val_*``; ``validate_model``, ``FakeEnv.replay``).  It reads and does not steer: it draws from generators of
its own, and policy and model after a run are bitwise those of the run without it.

``m_validate_calibration=True`` (needs ``m_validate_horizon > 0``) has that replay also measure whether the model's predictive
VARIANCE is the size of the real error, per horizon and column (``model/val_z2_*``, ``val_cover*``, ``val_nll_tot_h1``,
``val_ep_var_h1``, ``val_al_var_h1``, ``val_cal_skipped``; ``last_validation['calibration']``); it still reads and does not steer.
``m_calibrated_noise=True`` (needs it and ``m_stochastic=True``) feeds the one-step result back: after every validation the
transition noise of the imagined rollouts is scaled per observation column by the root of the maximum-likelihood variance
temperature, clipped to ``m_noise_temperature_range`` (``ModelSampler.set_noise_scale``; ``model/noise_scale_mean``).

``m_learn_term=True`` (the reference has nothing like it) gives the dynamics ensemble one more output column, the
last one, trained on the real ``done`` flags (``format_samples_for_dyn(append_t=True)``: 1 only where the environment ended a
path before the sampler's horizon, a time-out is target 0) and has ``FakeEnv`` end an imagined branch where the rule of
``task`` / ``static_fns`` or that column says so (``predicts_term=True``; ``m_term_threshold``, ``m_term_members`` = 'elite' /
'any' / 'majority').  With ``m_validate_horizon > 0`` the termination counts of ``model/val_*`` are then the head's, and
``model/val_term_recall_h1`` / ``val_term_false_alarm_h1`` are added.  ``save`` / ``load`` keep threshold and vote.

``m_term_pos_weight`` (a number >= 0 or 'balanced'), ``m_term_loss_weight`` (both need ``m_learn_term``) and
``m_cost_loss_weight`` (needs ``m_learn_cost``) weigh the model's two binary columns in its train loss (DESIGN §3s;
``PE.set_column_weights``): a class weight on the real terminations, a column weight on the termination / cost column.
'balanced' is ``clip(n_neg / max(n_pos, 1), 1, m_pos_weight_max)`` of each fit's termination targets, logged as
``model/term_pos_weight``.  A class weight omega moves the level the column settles at from the termination rate p to
``utils.pos_weight_level(p, omega)``; ``m_term_threshold`` keeps reading the column as it is.  ``save`` / ``load`` keep the
four keys in ``column_weights_<epoch>.json``.  With the defaults nothing is attached.

``m_term_loss='logistic'`` (needs ``m_learn_term``) trains the termination column with the Bernoulli negative
log-likelihood on its output read as a logit (``PE.set_logistic_columns([-1])``) and builds ``FakeEnv`` with
``term_loss='logistic'``: ``m_term_threshold`` is then a probability strictly inside (0, 1), compared as a logit.  The weights
above go on applying, as weights on the Bernoulli term.  ``save`` / ``load`` keep the choice in ``term_loss_<epoch>.json`` (a
missing file means 'gaussian').

``m_term_sampling=True`` (needs ``m_learn_term`` and ``use_model``) reads the termination column as a hazard, not
as a classifier: an imagined branch whose column says p ends with probability p (``ModelSampler(term_sampling=True)``: one
uniform draw per branch and step, from a generator of the sampler's own, compared in the post kernel as a per-row threshold),
so with a calibrated head imagined branches end at the rate real episodes do, without a threshold to tune.
``m_term_threshold`` and ``m_term_members`` stay in force for the validation replay, which keeps the threshold rule
(``term_cm`` goes on describing the classifier); ``m_term_members`` also stays the vote of the sampled rule.  Recommended with
``m_term_loss='logistic'`` and ``m_term_pos_weight=1.0``: a class-weighted level is not a probability
(``utils.pos_weight_level``), and a least-squares column is one only inside [0, 1].  ``save`` / ``load`` keep the flag in
``term_sampling_<epoch>.json`` beside the head's threshold and vote (a missing file or key means off).

``m_cost_loss='logistic'`` (needs ``m_learn_cost``) does the same for the cost column, ``obs_dim + 1``: it is trained
with the Bernoulli likelihood (targets above 0.5 count as 1) and ``FakeEnv(cost_loss='logistic')`` reads it as a logit, so every
imagined cost is a probability in [0, 1].  A task whose cost is a magnitude, not an indicator, should keep 'gaussian'.
``m_cost_pos_weight`` (a number >= 0 or 'balanced', needs ``m_learn_cost``) is the class weight of that column's positive
targets, 'balanced' by the termination head's rule on each fit's cost targets and logged as ``model/cost_pos_weight``;
``m_cost_pos_weight_undo=True`` (logistic only) subtracts ``log omega`` from the logit when it is read
(``FakeEnv.set_cost_head(logit_shift=)``), which undoes what the weight did to the fitted level.  ``save`` / ``load`` keep all of
it in ``cost_loss_<epoch>.json`` (a missing file means 'gaussian').

``m_validate_votes=True`` (needs ``m_validate_horizon > 0`` and the static votes: ``m_static_votes=True`` or an
``m_static_*_members`` mode other than 'elite') has the validation replay run under the vote the rollouts use --
``model/val_cost_miss_rate`` and its neighbours then describe the rule in force -- and count the members' votes against the
recorded flags (``last_validation['votes']``): from the one-step row ``model/val_vote_ece_cost_h1`` / ``_term_h1`` (is the share
``votes / E`` a probability), ``val_vote_split_*_h1`` (how often the members split), ``val_cost_miss_rate_any`` /
``_majority``, ``val_cost_false_alarm_rate_any`` / ``_majority`` and the ``term`` counterparts (what each reading of the vote would
miss and report in vain) and ``val_vote_skipped``.  It reads and does not steer.

``m_validate_particles=S`` (S a power of two in 2..64; needs ``m_validate_horizon > 0``) adds a second pass to that
replay: the first ``m_validate_particle_windows`` windows (None: ``min(m_validate_windows, 1024)``) are replayed by S sampled
particles each, with the transition noise the rollouts actually use (``model_sampler.noise_scale``), and the recorded next
state is held against the particles at every horizon (``last_validation['particles']``): ``model/val_crps_h1`` / ``_hH`` (the fair
CRPS), ``val_rank_dev_h1`` / ``_hH`` (the rank histogram's distance from flat), ``val_outlier_rate_hH`` (recordings outside the
cloud; 2 / (S + 1) when calibrated), ``val_spread_skill_h1`` / ``_hH`` (1 when calibrated) -- means over the observation columns --
and ``val_particles_nonfinite``.  Refused in words, before anything is built: S not a power of two in 2..64, no
``m_validate_horizon``, and ``m_validate_particles`` together with ``m_validate_votes=True`` (the particle pass runs no vote kernel:
its table would describe another rule than the vote-ruled tables beside it).  It reads and does not steer: policy and model are
bitwise those of the run without it.

``m_validate_reliability=True`` (needs ``m_validate_horizon > 0`` and a logistic head, ``m_cost_loss`` or ``m_term_loss``; DESIGN
§3z) has the validation replay also measure whether each logistic column is a PROBABILITY: a reliability table per column in
``m_reliability_bins`` bins (``last_validation['reliability']``) and from its one-step row ``model/val_ece_cost_h1`` /
``val_ece_term_h1``, ``val_logloss_*_h1``, ``val_base_rate_*_h1``, ``val_mean_p_*_h1`` (the elite reading) and
``val_rel_skipped``.  It reads and does not steer.  ``m_recalibrate_cost=True`` (needs it and ``m_cost_loss='logistic'``) and
``m_recalibrate_term=True`` (needs it, ``m_term_loss='logistic'`` and ``m_term_sampling=True``) feed the one-step result back
after every validation: the logit offset that makes the column's mean probability the observed rate
(``replay.logit_offset``, clipped to ``m_recalibration_range``) goes into the imagined cost
(``FakeEnv.set_cost_recalibration``; ``model/cost_recal_offset``) and into the sampled termination thresholds
(``ModelSampler.set_term_logit_offset``; ``model/term_recal_offset``).  The offset is set absolutely each time and the table is
always measured without it.  ``save`` / ``load`` keep the switches and the two offsets in ``recalibration_<epoch>.json`` (a
missing file means off, offsets 0).

``static_fns`` takes a ``statics.TaskRules``: user-defined termination / cost rules for the imagined rollouts, with
precedence over ``task`` (which may itself be a name given to ``statics.register_task``).
"""
import time
import warnings
from collections import OrderedDict
from itertools import count

import numpy as np
import torch

from .cpo_sampler import CpoSampler
from .fake_env import FakeEnv
from .logger import EpochLogger
from .model_sampler import ModelSampler
from .modelbuffer import ModelBuffer
from .pens import build_PE

EPS = 1e-8


def update_dict(dict_a, dict_b, weight_a=.5, weight_b=.5):
    """models/pens/logger.py:7-17: keys of b overwrite a, keys in both are blended."""
    out = dict(dict_a)
    out.update(dict_b)
    for k in dict_b:
        if k in dict_a:
            out[k] = weight_b * dict_b[k] + weight_a * dict_a[k]
    return out


def format_samples_for_dyn(samples, append_r=True, append_c=False, append_t=False, horizon=None):
    """models/pens/pe_factory.py:74-107: inputs = [obs | act], outputs = [next_obs - obs | rew (| cost) (| term)].

    ``append_t`` (the learned termination head, no counterpart in the reference) adds the termination target as the LAST
    column: 1 only where ``samples['terminals']`` is set on a path shorter than the sampler's ``horizon``
    (``samples['path_lengths']``, ``CPOBuffer.get_archive(['path_lengths', ...])``); a path that ran to the horizon ended by
    time-out and is target 0, whatever the environment's own time limit reported."""
    obs, act, next_obs = samples['observations'], samples['actions'], samples['next_observations']
    inputs = np.concatenate((obs, act), axis=-1)
    outputs = next_obs - obs
    if append_r:
        outputs = np.concatenate((outputs, np.squeeze(samples['rewards'])[..., None]), axis=-1)
    if append_c:
        outputs = np.concatenate((outputs, np.squeeze(samples['costs'])[..., None]), axis=-1)
    if append_t:
        if horizon is None or 'path_lengths' not in samples:
            raise ValueError("format_samples_for_dyn(append_t=True) needs horizon= and samples['path_lengths']: a time-out is "
                             "told from a termination by the path's length")
        term = np.squeeze(samples['terminals']).astype(bool) & (np.squeeze(samples['path_lengths']) < int(horizon))
        outputs = np.concatenate((outputs, term.astype(outputs.dtype)[..., None]), axis=-1)
    return inputs, outputs


def _calibration_args(validate_horizon, use_model, stochastic, validate_calibration, calibrated_noise, temperature_range):
    """The three calibration arguments of ``CMBPO`` checked against each other: (validate_calibration, calibrated_noise,
    (lo, hi)) or a ValueError that says what is missing."""
    validate_calibration, calibrated_noise = bool(validate_calibration), bool(calibrated_noise)
    if validate_calibration and not (int(validate_horizon) > 0 and use_model):
        raise ValueError("m_validate_calibration needs m_validate_horizon > 0 (and use_model=True): the calibration table is "
                         "computed inside the validation replay")
    if calibrated_noise and not (validate_calibration and bool(stochastic)):
        raise ValueError("m_calibrated_noise needs m_stochastic=True and m_validate_calibration=True: it scales the transition "
                         "noise by the temperature the validation measures")
    try:
        lo, hi = (float(x) for x in temperature_range)
    except (TypeError, ValueError):
        raise ValueError("m_noise_temperature_range: a pair (lo, hi), got %r" % (temperature_range,))
    if not (0.0 < lo <= hi and np.isfinite(hi)):
        raise ValueError("m_noise_temperature_range: 0 < lo <= hi < inf expected, got %r" % (temperature_range,))
    return validate_calibration, calibrated_noise, (lo, hi)


def _reliability_args(validate_horizon, use_model, cost_loss, term_loss, term_sampling, validate_reliability, bins, recalibrate_cost,
                      recalibrate_term, recalibration_range):
    """The five reliability arguments of ``CMBPO`` checked against the heads they measure, or a ValueError in words:
    (validate_reliability, bins, recalibrate_cost, recalibrate_term, (lo, hi))."""
    logistic = cost_loss == 'logistic' or term_loss == 'logistic'
    if validate_reliability:
        if not (int(validate_horizon) > 0 and use_model):
            raise ValueError("m_validate_reliability needs m_validate_horizon > 0 (and use_model): it is measured in the validation replay")
        if not logistic:
            raise ValueError("m_validate_reliability needs a logistic head (m_cost_loss='logistic' or m_term_loss='logistic'): a "
                             "Gaussian column is not a logit, it has no reliability table")
    try:
        bins = int(bins)
    except (TypeError, ValueError):
        raise ValueError("m_reliability_bins: an integer in 1..32, got %r" % (bins,))
    if not 1 <= bins <= 32:
        raise ValueError("m_reliability_bins: an integer in 1..32, got %r" % (bins,))
    if recalibrate_cost and not (validate_reliability and cost_loss == 'logistic'):
        raise ValueError("m_recalibrate_cost needs m_validate_reliability=True and m_cost_loss='logistic': the offset is derived "
                         "from the cost column's reliability table")
    if recalibrate_term and not (validate_reliability and term_loss == 'logistic' and term_sampling):
        raise ValueError("m_recalibrate_term needs m_validate_reliability=True, m_term_loss='logistic' and m_term_sampling=True: "
                         "the offset is derived from the termination column's reliability table and shifts the sampled thresholds")
    try:
        lo, hi = (float(x) for x in recalibration_range)
    except (TypeError, ValueError):
        raise ValueError("m_recalibration_range: a pair (lo, hi), got %r" % (recalibration_range,))
    if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
        raise ValueError("m_recalibration_range: finite lo <= hi expected, got %r" % (recalibration_range,))
    return bool(validate_reliability), bins, bool(recalibrate_cost), bool(recalibrate_term), (lo, hi)


def _static_votes_args(use_model, learn_cost, term_members, cost_members, votes, cost_pessimism):
    """``m_static_term_members`` / ``m_static_cost_members`` / ``m_static_votes`` checked against ``m_learn_cost`` and
    ``m_cost_pessimism``, or a ValueError in words; returns whether the vote kernel runs."""
    from . import _lib
    if term_members not in _lib.RULE_DONE_MEMBERS:
        raise ValueError("m_static_term_members: 'elite', 'any' or 'majority', got %r" % (term_members,))
    if cost_members not in _lib.RULE_COST_MEMBERS:
        raise ValueError("m_static_cost_members: 'elite', 'any', 'majority' or 'mean', got %r" % (cost_members,))
    if cost_members != 'elite' and learn_cost:
        raise ValueError("m_static_cost_members=%r needs m_learn_cost=False: with a learned cost the task's static cost rule is "
                         "skipped, there is nothing to vote on" % (cost_members,))
    on = bool(use_model) and (bool(votes) or term_members != 'elite' or cost_members != 'elite')
    if float(cost_pessimism) > 0.0 and not learn_cost and not on:
        raise ValueError("m_cost_pessimism > 0 needs m_learn_cost=True: only a learned cost head has an ensemble spread (or the "
                         "static votes: m_static_votes=True or an m_static_*_members mode other than 'elite')")
    return on


def _validate_votes_args(validate_horizon, use_model, static_votes_on, validate_votes):
    """``m_validate_votes`` checked against ``m_validate_horizon`` and the static votes, or a ValueError in words."""
    if not validate_votes:
        return False
    if not (int(validate_horizon) > 0 and use_model):
        raise ValueError("m_validate_votes needs m_validate_horizon > 0 (and use_model): the vote table is measured in the "
                         "validation replay")
    if not static_votes_on:
        raise ValueError("m_validate_votes needs the static votes: m_static_votes=True or an m_static_*_members mode other than "
                         "'elite' -- the imagined rollouts use the elite's rule, and that is what the validation replay measures")
    return True


def _term_sampling_args(learn_term, term_sampling):
    """``m_term_sampling`` checked against ``m_learn_term`` (and ``use_model``), or a ValueError in words."""
    if term_sampling and not learn_term:
        raise ValueError("m_term_sampling=True needs m_learn_term=True (and use_model): it samples the imagined terminations "
                         "from the model's termination column, and there is none")
    return bool(term_sampling)


def _term_loss_args(learn_term, term_loss, term_threshold):
    """``m_term_loss`` checked against ``m_learn_term`` and ``m_term_threshold``, or a ValueError in words."""
    if term_loss not in ('gaussian', 'logistic'):
        raise ValueError("m_term_loss: 'gaussian' or 'logistic', got %r" % (term_loss,))
    if term_loss == 'logistic':
        if not learn_term:
            raise ValueError("m_term_loss='logistic' needs m_learn_term=True (and use_model): it is the likelihood of the "
                             "termination column")
        from .utils import logit_threshold
        try:
            logit_threshold(term_threshold)
        except ValueError as e:
            raise ValueError("m_term_threshold: %s" % e) from None
    return term_loss


def _cost_loss_args(learn_cost, cost_loss, cost_pos_weight, undo, pos_weight_max):
    """``m_cost_loss`` / ``m_cost_pos_weight`` / ``m_cost_pos_weight_undo`` checked against ``m_learn_cost``: the
    tuple (loss, weight -- a float or 'balanced', undo) or a ValueError in words."""
    if cost_loss not in ('gaussian', 'logistic'):
        raise ValueError("m_cost_loss: 'gaussian' or 'logistic', got %r" % (cost_loss,))
    if cost_loss == 'logistic' and not learn_cost:
        raise ValueError("m_cost_loss='logistic' needs m_learn_cost=True (and use_model): it is the likelihood of the learned "
                         "cost column")
    if isinstance(cost_pos_weight, str):
        if cost_pos_weight != 'balanced':
            raise ValueError("m_cost_pos_weight: a number >= 0 or 'balanced', got %r" % (cost_pos_weight,))
        weight = 'balanced'
    else:
        try:
            weight = float(cost_pos_weight)
        except (TypeError, ValueError):
            raise ValueError("m_cost_pos_weight: a number >= 0 or 'balanced', got %r" % (cost_pos_weight,))
        if not (np.isfinite(weight) and weight >= 0.0):
            raise ValueError("m_cost_pos_weight: a finite number >= 0 or 'balanced', got %r" % (cost_pos_weight,))
    if weight != 1.0 and not learn_cost:
        raise ValueError("m_cost_pos_weight needs m_learn_cost=True: it weighs the positive class of the learned cost column")
    if undo:
        if cost_loss != 'logistic':
            raise ValueError("m_cost_pos_weight_undo needs m_cost_loss='logistic': only a logit can be shifted back by log omega")
        if weight != 'balanced' and not weight > 0.0:
            raise ValueError("m_cost_pos_weight_undo needs m_cost_pos_weight > 0: log omega is the shift it undoes")
    return cost_loss, weight, bool(undo)


def cost_logit_shift(omega):
    """The shift that undoes a class weight omega > 0 on a logistic column: log omega (known property)."""
    return float(np.log(float(omega)))


COLUMN_WEIGHT_KEYS = ('m_term_pos_weight', 'm_term_loss_weight', 'm_cost_loss_weight', 'm_pos_weight_max')


def _column_weight_args(learn_term, learn_cost, term_pos_weight, term_loss_weight, cost_loss_weight, pos_weight_max):
    """The four column-weight arguments of ``CMBPO`` checked against the heads they weigh: a dict of
    ``COLUMN_WEIGHT_KEYS`` (floats, ``m_term_pos_weight`` possibly the string 'balanced') or a ValueError in words."""
    def number(name, v, low_ok):
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError("%s: a finite number, got %r" % (name, v))
        if not (np.isfinite(f) and (f >= 0.0 if low_ok else f > 0.0)):
            raise ValueError("%s: a finite number %s 0, got %r" % (name, ">=" if low_ok else ">", v))
        return f

    balanced = isinstance(term_pos_weight, str)
    if balanced and term_pos_weight != 'balanced':
        raise ValueError("m_term_pos_weight: a number >= 0 or 'balanced', got %r" % (term_pos_weight,))
    out = {'m_term_pos_weight': 'balanced' if balanced else number('m_term_pos_weight', term_pos_weight, True),
           'm_term_loss_weight': number('m_term_loss_weight', term_loss_weight, True),
           'm_cost_loss_weight': number('m_cost_loss_weight', cost_loss_weight, True),
           'm_pos_weight_max': number('m_pos_weight_max', pos_weight_max, False)}
    if out['m_pos_weight_max'] < 1.0:
        raise ValueError("m_pos_weight_max: the upper clip of 'balanced', >= 1, got %r" % (pos_weight_max,))
    if not learn_term and (out['m_term_pos_weight'] != 1.0 or out['m_term_loss_weight'] != 1.0):
        raise ValueError("m_term_pos_weight / m_term_loss_weight need m_learn_term=True: they weigh the termination column")
    if not learn_cost and out['m_cost_loss_weight'] != 1.0:
        raise ValueError("m_cost_loss_weight needs m_learn_cost=True: it weighs the learned cost column")
    return out


def balanced_pos_weight(targets, pos_weight_max):
    """'balanced' class weight of a 0/1 target column: clip(n_neg / max(n_pos, 1), 1, pos_weight_max)."""
    pos = int(np.count_nonzero(np.asarray(targets) > 0.5))
    neg = int(np.size(targets)) - pos
    return float(np.clip(neg / max(pos, 1), 1.0, float(pos_weight_max)))


def _validate_particles_args(horizon, use_model, windows, particles, particle_windows, validate_votes=False):
    """``m_validate_particles`` / ``m_validate_particle_windows`` checked against ``m_validate_horizon`` and
    ``m_validate_votes``, or a ValueError in words: (S, windows of the particle pass)."""
    if not particles:
        if particle_windows is not None:
            raise ValueError("m_validate_particle_windows needs m_validate_particles > 0: there is no particle pass to size")
        return 0, 0
    from .replay import check_particles
    S = check_particles(particles)
    if not (use_model and int(horizon) > 0):
        raise ValueError("m_validate_particles needs m_validate_horizon > 0 (and use_model): the particle table is measured in the "
                         "validation replay")
    if validate_votes:
        raise ValueError("m_validate_particles together with m_validate_votes=True is not supported: the particle pass runs no "
                         "vote kernel, its table would describe another rule than the vote-ruled tables beside it")
    n = min(int(windows), 1024) if particle_windows is None else int(particle_windows)
    if n < 1:
        raise ValueError("m_validate_particle_windows must be >= 1, got %r" % (particle_windows,))
    return S, n


class CMBPO:
    """Constrained Model-Based Policy Optimization (``algorithms/cmbpo.py:30``)."""
    # the reading of the cost column where the constructor has not set it: a magnitude, no class weight
    _m_cost_loss, _cost_pos_weight, _cost_pos_weight_undo = 'gaussian', 1.0, False
    # reliability of the logistic columns where the constructor has not set it: off
    _validate_reliability, _reliability_bins, _recalibrate_cost, _recalibrate_term = False, 15, False, False
    _recalibration_range = (-2.0, 2.0)
    # the validation replay under the static votes where the constructor has not set it: off
    _validate_votes = False

    def __init__(self, env, policy, buffer, sampler=None, task='default', static_fns=None, n_env_interacts=1e7,
                 eval_every_n_steps=5e3, use_model=True, m_learn_cost=False, m_train_freq=250, m_loss_type='MSPE',
                 m_use_scaler_in=True, m_use_scaler_out=True, m_lr=1e-3, m_networks=7, m_elites=5,
                 m_hidden_dims=(512, 512), max_model_t=None, rollout_batch_size=10e3, sampling_alpha=1,
                 rollout_mode='uncertainty', rollout_schedule=(20, 100, 1, 1), maxroll=80,
                 initial_real_samples_per_epoch=5000, min_real_samples_per_epoch=500, batch_size_policy=25000,
                 n_epochs=int(10e7), n_initial_exploration_steps=0, initial_exploration_policy=None, epoch_length=1000,
                 model_train_kwargs=None, initial_model_train_kwargs=None, shuffle_on_device=True, device=None,
                 session=None, start_state_sampling='host', m_stochastic=False, m_iv_gae=False, m_iv_eps=1e-8,
                 m_disagreement=False, m_rew_pessimism=0.0, m_cost_pessimism=0.0,
                 m_value_disagreement=False, m_v_pessimism=0.0, m_vc_pessimism=0.0,
                 m_validate_horizon=0, m_validate_windows=1024, m_imagined_weight=1.0, m_trust_var=None,
                 m_validate_calibration=False, m_calibrated_noise=False, m_noise_temperature_range=(0.25, 4.0),
                 m_learn_term=False, m_term_threshold=0.5, m_term_members='elite',
                 m_term_pos_weight=1.0, m_term_loss_weight=1.0, m_cost_loss_weight=1.0, m_pos_weight_max=20.0,
                 m_term_loss='gaussian', m_cost_loss='gaussian', m_cost_pos_weight=1.0, m_cost_pos_weight_undo=False,
                 m_term_sampling=False, m_validate_reliability=False, m_reliability_bins=15, m_recalibrate_cost=False,
                 m_recalibrate_term=False, m_recalibration_range=(-2.0, 2.0),
                 m_static_term_members='elite', m_static_cost_members='elite', m_static_votes=False, m_validate_votes=False,
                 m_validate_particles=0, m_validate_particle_windows=None, **_unused):
        # the particle pass of the validation replay; refused in words before anything is built
        self._validate_particles, self._validate_particle_windows = _validate_particles_args(
            m_validate_horizon, use_model, m_validate_windows, m_validate_particles, m_validate_particle_windows, m_validate_votes)
        # column / class weights of the model's binary columns; refused in words before anything is built
        self._column_weights = _column_weight_args(bool(m_learn_term) and bool(use_model), bool(m_learn_cost), m_term_pos_weight,
                                                   m_term_loss_weight, m_cost_loss_weight, m_pos_weight_max)
        # the likelihood of the termination column; likewise
        self._m_term_loss = _term_loss_args(bool(m_learn_term) and bool(use_model), m_term_loss, m_term_threshold)
        # ensemble-voted static rules; likewise
        self._static_votes_on = _static_votes_args(use_model, bool(m_learn_cost), m_static_term_members, m_static_cost_members,
                                                   m_static_votes, m_cost_pessimism)
        # the validation replay under that vote, with the vote table; likewise
        self._validate_votes = _validate_votes_args(m_validate_horizon, use_model, self._static_votes_on, m_validate_votes)
        # sampled terminations; likewise
        self._m_term_sampling = _term_sampling_args(bool(m_learn_term) and bool(use_model), m_term_sampling)
        # the likelihood and the class weight of the cost column; likewise
        self._m_cost_loss, self._cost_pos_weight, self._cost_pos_weight_undo = _cost_loss_args(
            bool(m_learn_cost) and bool(use_model), m_cost_loss, m_cost_pos_weight, m_cost_pos_weight_undo, m_pos_weight_max)
        # predictive calibration in the validation replay and, from its one-step row, the scale of the transition
        # noise; refused in words before anything is built
        self._validate_calibration, self._calibrated_noise, self._noise_temperature_range = _calibration_args(
            m_validate_horizon, use_model, m_stochastic, m_validate_calibration, m_calibrated_noise, m_noise_temperature_range)
        # reliability tables of the logistic columns in the validation replay and, from their one-step row, the logit offsets of
        # the imagined cost and the sampled terminations; likewise
        (self._validate_reliability, self._reliability_bins, self._recalibrate_cost, self._recalibrate_term,
         self._recalibration_range) = _reliability_args(
            m_validate_horizon, use_model, self._m_cost_loss, self._m_term_loss, self._m_term_sampling, m_validate_reliability,
            m_reliability_bins, m_recalibrate_cost, m_recalibrate_term, m_recalibration_range)
        # RLAlgorithm.__init__ (algorithms/rl_algorithm.py:22-74)
        self.sampler = sampler if sampler is not None else CpoSampler(max_path_length=getattr(policy, "max_path_length", 1000))
        self._n_epochs, self._epoch_length = n_epochs, epoch_length
        self._n_initial_exploration_steps = n_initial_exploration_steps
        self._epoch = self._timestep = self._num_train_steps = 0

        self.obs_space, self.act_space = env.observation_space, env.action_space
        self.obs_dim = int(np.prod(env.observation_space.shape))
        self.act_dim = int(np.prod(env.action_space.shape))
        self.n_env_interacts = n_env_interacts
        if static_fns is not None:
            from .statics import TaskRules
            if not isinstance(static_fns, TaskRules):
                raise TypeError("static_fns: a cmbpo_amd.statics.TaskRules, got %r" % (static_fns,))
        self._task = task
        self._static_fns = static_fns
        self.eval_every_n_steps = eval_every_n_steps
        self._training_environment = env
        self._policy = policy
        self._initial_exploration_policy = initial_exploration_policy or policy
        self.sampling_alpha = sampling_alpha
        self.device = torch.device(device) if device is not None else policy.device

        self._buffer = buffer
        pi_info_shapes = policy.pi_info_shapes
        self._buffer.initialize(pi_info_shapes, gamma=policy.gamma, lam=policy.lam, cost_gamma=policy.cost_gamma,
                                cost_lam=policy.cost_lam)
        self._use_model = use_model
        self._m_learn_cost = bool(m_learn_cost)
        # learned termination head: refused in words before anything is built
        self._m_learn_term = bool(m_learn_term) and bool(use_model)
        if self._m_learn_term:
            from . import _lib
            if not np.isfinite(float(m_term_threshold)):
                raise ValueError("m_term_threshold must be a finite number, got %r" % (m_term_threshold,))
            if m_term_members not in _lib.TERM_MEMBERS:
                raise ValueError("m_term_members: 'elite', 'any' or 'majority', got %r" % (m_term_members,))
        # critic disagreement: kappa > 0 implies the measurement; only the one-launch critic kernels measure it
        kv, kvc = float(m_v_pessimism), float(m_vc_pessimism)
        if not (np.isfinite(kv) and kv >= 0.0 and np.isfinite(kvc) and kvc >= 0.0):
            raise ValueError("m_v_pessimism / m_vc_pessimism must be finite numbers >= 0, got %r, %r" % (m_v_pessimism, m_vc_pessimism))
        self._value_disagreement = bool(use_model) and (bool(m_value_disagreement) or kv > 0.0 or kvc > 0.0)
        if self._value_disagreement:
            limit = policy.value_disagreement_limit()
            if limit is not None:
                raise ValueError("m_value_disagreement / m_v_pessimism / m_vc_pessimism: " + limit)
        # trust-weighted updates: a real sample weighs 1, an imagined one m_imagined_weight, times its trust weight
        # m_trust_var / (m_trust_var + accumulated model variance) when m_trust_var is set.  (1.0, None): no weights anywhere.
        self._imagined_weight = float(m_imagined_weight)
        if not (self._imagined_weight > 0.0 and np.isfinite(self._imagined_weight)):
            raise ValueError("m_imagined_weight must be a positive finite number, got %r" % (m_imagined_weight,))
        if m_trust_var is not None:
            if not m_iv_gae:
                raise ValueError("m_trust_var needs m_iv_gae=True: the accumulated model variance is only kept there")
            if not (float(m_trust_var) > 0.0 and np.isfinite(float(m_trust_var))):
                raise ValueError("m_trust_var must be a positive finite number or None, got %r" % (m_trust_var,))
        self._trust_var = None if m_trust_var is None else float(m_trust_var)
        self._weighted = bool(use_model) and (self._imagined_weight != 1.0 or self._trust_var is not None)
        self._m_train_freq = m_train_freq
        self._rollout_batch_size = int(rollout_batch_size)
        self._rollout_schedule = list(rollout_schedule)
        self._max_model_t = max_model_t
        # train_model arguments of algorithms/cmbpo.py:452,335 (first fit: 150..500 epochs; later: 1..10)
        self._initial_model_train_kwargs = dict(min_epochs=150, max_epochs=500)
        self._initial_model_train_kwargs.update(initial_model_train_kwargs or {})
        self._model_train_kwargs = dict(min_epochs=1, max_epochs=10)
        self._model_train_kwargs.update(model_train_kwargs or {})
        # per-epoch shuffle_rows of PE.train on the GPU (same distribution, other random numbers): the host argsort of
        # an [E, n] array costs more than the epoch's kernels from n ~ 1e5 on.  False restores the reference's draws.
        self._shuffle_on_device = bool(shuffle_on_device)
        # 'host': the reference's NumPy draws over the host archive (its random stream).  'device': the same chain on the
        # buffer's device mirror (CPOBuffer.sample_start_states: other random numbers, no host copy of a batch-sized array)
        if start_state_sampling not in ('host', 'device'):
            raise ValueError("start_state_sampling: 'host' or 'device', got %r" % (start_state_sampling,))
        self._start_state_sampling = start_state_sampling

        if use_model:
            # outputs: delta-obs | reward (| cost, with the learned cost head: algorithms/cmbpo.py:121-123) (| term, the last)
            self._model = build_PE(in_dim=self.obs_dim + self.act_dim, out_dim=self.obs_dim + 1 + int(self._m_learn_cost) + int(self._m_learn_term),
                                   name='DynEns', loss=m_loss_type, hidden_dims=m_hidden_dims, lr=m_lr,
                                   num_networks=m_networks, num_elites=m_elites, use_scaler_in=m_use_scaler_in,
                                   use_scaler_out=m_use_scaler_out, decay=1e-6, max_logvar=.5, min_logvar=-10,
                                   device=self.device,
                                   logistic_columns=self._logistic_columns())
            rules_task = self._task if static_fns is None else static_fns      # static_fns takes precedence over the task name
            self.fake_env = FakeEnv(true_environment=env, task=rules_task, model=self._model, predicts_delta=True,
                                    predicts_rew=True, predicts_cost=self._m_learn_cost,
                                    disagreement=bool(m_disagreement), rew_pessimism=m_rew_pessimism,
                                    cost_pessimism=m_cost_pessimism, predicts_term=self._m_learn_term,
                                    term_threshold=m_term_threshold, term_members=m_term_members, term_loss=m_term_loss,
                                    cost_loss=m_cost_loss, static_term_members=m_static_term_members,
                                    static_cost_members=m_static_cost_members, static_votes=bool(m_static_votes))
            self.rollout_mode = rollout_mode
            self.model_buf = ModelBuffer(batch_size=self._rollout_batch_size, obs_dim=self.obs_dim, act_dim=self.act_dim,
                                         max_path_length=maxroll, device=self.device, iv_gae=bool(m_iv_gae),
                                         iv_eps=m_iv_eps)
            self.model_buf.initialize(pi_info_shapes, gamma=policy.gamma, lam=policy.lam, cost_gamma=policy.cost_gamma,
                                      cost_lam=policy.cost_lam)
            if self._trust_var is not None:
                self.model_buf.set_trust_weights(self._trust_var)
            if self._value_disagreement:
                self.model_buf.set_value_disagreement(True, kv, kvc)
            self.model_sampler = ModelSampler(max_path_length=maxroll, batch_size=self._rollout_batch_size,
                                              logger=None, rollout_mode=self.rollout_mode,
                                              stochastic=bool(m_stochastic),
                                              **({'term_sampling': True} if self._m_term_sampling else {}))
        # open-loop validation of the model on each epoch's real samples (0: off -- no call, no key, no random number)
        self._validate_horizon, self._validate_windows = int(m_validate_horizon), int(m_validate_windows)
        if self._validate_horizon < 0 or (self._validate_horizon > 0 and self._validate_windows < 1):
            raise ValueError("m_validate_horizon must be >= 0 and m_validate_windows >= 1, got %r, %r"
                             % (m_validate_horizon, m_validate_windows))
        self._validate_rng = None      # the window draws: a stream of their own, made by the first validate_model()
        self.init_real_samples = initial_real_samples_per_epoch
        self.min_real_samples = min_real_samples_per_epoch
        self.batch_size_policy = batch_size_policy
        self.logger = EpochLogger()
        self._policy.set_logger(self.logger)
        self.sampler.set_logger(self.logger)
        self.times = {}

    # -- bookkeeping of RLAlgorithm ------------------------------------------------------------------------
    @property
    def _total_timestep(self):
        return self.sampler._total_samples

    @property
    def _training_started(self):
        return self._total_timestep > 0

    @property
    def ready_to_train(self):
        return self.sampler.batch_ready()

    def _do_sampling(self, timestep):
        return self.sampler.sample(timestep=timestep)

    def _stamp(self, name, t0):
        self.times[name] = self.times.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    # -- hooks ---------------------------------------------------------------------------------------------
    def _initial_exploration_hook(self, env, initial_exploration_policy, pool):
        """algorithms/cmbpo.py:432-453: gather n_initial_exploration_steps real samples, then fit the model."""
        if self._n_initial_exploration_steps < 1:
            return
        if not initial_exploration_policy:
            raise ValueError("Initial exploration policy must be provided when n_initial_exploration_steps > 0.")
        self.sampler.initialize(env, initial_exploration_policy, pool)
        while True:
            self.sampler.sample(timestep=0)
            if self.sampler._total_samples >= self._n_initial_exploration_steps:
                self.sampler.finish_all_paths(append_val=True, append_cval=True, reset_path=False)
                pool.get()       # moves the policy samples to the archive
                break
        if self._use_model:
            self.train_model(**self._initial_model_train_kwargs)

    def train_model(self, min_epochs=5, max_epochs=100, batch_size=2048):
        """algorithms/cmbpo.py:455-486"""
        fields = ['observations', 'actions', 'next_observations', 'rewards', 'costs', 'terminals', 'epochs']
        model_samples = self._buffer.get_archive(fields + (['path_lengths'] if self._m_learn_term else []))
        dyn_ins, dyn_outs = format_samples_for_dyn(model_samples, append_r=True, append_c=self._m_learn_cost,
                                                   append_t=self._m_learn_term, horizon=self.sampler.max_path_length)
        extra = self._set_model_column_weights(dyn_outs)
        out = self._model.train(dyn_ins, dyn_outs, batch_size=batch_size, max_epochs=max_epochs,
                                min_epoch_before_break=min_epochs, holdout_ratio=0.2, max_t=self._max_model_t,
                                shuffle_on_device=self._shuffle_on_device)
        out.update(extra)
        return out

    def _set_model_column_weights(self, dyn_outs):
        """The column / class weights of this fit onto the model: the termination column is the last one, the
        cost column the one after the reward; 'balanced' is recomputed from this call's termination targets.  With the
        defaults nothing is attached and nothing is logged."""
        cw = self._column_weights
        if (cw['m_term_pos_weight'], cw['m_term_loss_weight'], cw['m_cost_loss_weight'], self._cost_pos_weight) == (1.0, 1.0, 1.0, 1.0):
            return {}
        col, pos, extra = {}, {}, {}
        if self._m_learn_term:
            omega = cw['m_term_pos_weight']
            if omega == 'balanced':
                omega = balanced_pos_weight(dyn_outs[:, -1], cw['m_pos_weight_max'])
            pos[-1], col[-1] = omega, cw['m_term_loss_weight']
            extra['term_pos_weight'] = omega
        if self._m_learn_cost:
            col[self.obs_dim + 1] = cw['m_cost_loss_weight']
            if self._cost_pos_weight != 1.0:
                # the class weight of the cost column, the termination head's rule on this fit's cost targets
                omega = self._cost_pos_weight
                if omega == 'balanced':
                    omega = balanced_pos_weight(dyn_outs[:, self.obs_dim + 1], cw['m_pos_weight_max'])
                pos[self.obs_dim + 1] = omega
                extra['cost_pos_weight'] = omega
                if self._cost_pos_weight_undo:
                    self.fake_env.set_cost_head(logit_shift=cost_logit_shift(omega))
        self._model.set_column_weights(col, pos)
        return extra

    def validate_model(self, epochs=None, horizon=None, n_windows=None):
        """Open-loop validation of the dynamics model: ``n_windows`` windows of up to ``horizon`` consecutive
        real steps from the archive (``epochs``: only windows starting in these) replayed through the model with the
        recorded actions, ``FakeEnv.replay``.  The loop calls it right after the epoch's real samples have moved into the
        archive, on that epoch only: ``train_model`` ran before the move, so no training run has seen them (prequential
        validation -- nothing is held back from training).  Returns the ``val_*`` diagnostics; ``last_validation`` keeps
        the whole per-horizon table."""
        if not self._use_model:
            raise ValueError("validate_model: the trainer was built with use_model=False, there is no model to validate")
        H = int(horizon or self._validate_horizon)
        if H < 1:
            raise ValueError("validate_model: pass horizon >= 1 (the trainer was built with m_validate_horizon=0)")
        if self._validate_rng is None:
            self._validate_rng = np.random.default_rng(0x76616c)
        start, length, win = self._buffer.windows(H, int(n_windows or self._validate_windows), epochs=epochs, rng=self._validate_rng)
        # (every switch that is off is left out of the call: the call of a trainer that never heard of it)
        kw = {'calibration': True} if self._validate_calibration else {}
        if self._validate_reliability:
            kw.update(reliability=True, reliability_bins=self._reliability_bins)
            if self._m_learn_term and self._m_term_loss == 'logistic':
                # the windows carry the recorded `done`; the column was trained on term_targets, where a time-out is 0: the
                # table is held against the training target, the same steps of the same windows
                idx = start[None, :] + np.minimum(np.arange(H)[:, None], length[None, :] - 1)
                kw.update(reliability_terminals=self._buffer.term_targets(self.sampler.max_path_length)[idx])
        if self._validate_votes:
            # the static rule knows no time-out either: its histogram is held against the same targets
            idx = start[None, :] + np.minimum(np.arange(H)[:, None], length[None, :] - 1)
            kw.update(votes=True, reliability_terminals=self._buffer.term_targets(self.sampler.max_path_length)[idx])
        S = self._validate_particles
        n_part = min(self._validate_particle_windows, len(length)) if S else 0
        pkw = dict(noise_scale=self.model_sampler.noise_scale) if S else {}      # (the noise the rollouts actually use)
        if S and n_part == len(length):
            kw.update(particles=S, **pkw)
        tab = self.fake_env.replay(**win, **kw)
        if S and 'particles' not in tab:
            # fewer windows than the plain replay's: the particle pass alone, on the first of them (the windows are a random draw)
            head = {k: (v[:n_part] if k in ('obs0', 'lengths') else v[:, :n_part]) for k, v in win.items()}
            tab['particles'] = self.fake_env._replay_particles(S, **head, **pkw)
        self.last_validation = tab
        ratio = lambda a, b: float(a) / float(b) if b > 0 else float('nan')
        cm, tm = tab['cost_cm'].sum(axis=0), tab['term_cm'].sum(axis=0)      # [real, predicted], all horizons
        last = H - 1
        extra = {}
        if self._validate_calibration:
            # the per-column entries: means over the observation columns (the reward column is in the table)
            cal, D = tab['calibration'], self.obs_dim
            col = lambda k, h: float(np.mean(cal[k][h, :D]))
            extra = {'val_z2_al_h1': col('z2_al', 0), 'val_z2_tot_h1': col('z2_tot', 0), 'val_z2_tot_hH': col('z2_tot', last),
                     'val_cover1_tot_h1': col('cover1_tot', 0), 'val_cover2_tot_h1': col('cover2_tot', 0),
                     'val_nll_tot_h1': col('nll_tot', 0), 'val_ep_var_h1': col('ep_var', 0), 'val_al_var_h1': col('al_var', 0),
                     'val_cal_skipped': int(cal['n_skipped'].sum())}
            if self._calibrated_noise:
                if cal['n'][0] > 0:
                    from .replay import temperature
                    self.model_sampler.set_noise_scale(np.sqrt(temperature(cal, 'al', 0, *self._noise_temperature_range)))
                scale = self.model_sampler.noise_scale
                extra['noise_scale_mean'] = 1.0 if scale is None else float(np.mean(scale))
        if self._validate_reliability:
            extra.update(self._reliability_diagnostics(tab['reliability']))
        if self._validate_votes:
            extra.update(self._votes_diagnostics(tab['votes']))
        if S:
            extra.update(self._particles_diagnostics(tab['particles'], self.obs_dim))
        if self._m_learn_term:
            # the head at h = 1, the one-step row: the share of real terminations it reports, of continuing steps it ends
            t1 = tab['term_cm'][0]
            extra.update({'val_term_recall_h1': ratio(t1[1, 1], t1[1, 0] + t1[1, 1]),
                          'val_term_false_alarm_h1': ratio(t1[0, 1], t1[0, 0] + t1[0, 1])})
        return {**extra,
                'val_n_h1': int(tab['n'][0]), 'val_n_hH': int(tab['n'][last]),
                'val_mse_obs_h1': float(np.mean(tab['mse_obs'][0])), 'val_mse_obs_hH': float(np.mean(tab['mse_obs'][last])),
                'val_mse_rew_hH': float(tab['mse_rew'][last]),
                'val_cost_miss_rate': ratio(cm[1, 0], cm[1, 0] + cm[1, 1]),
                'val_cost_false_alarm_rate': ratio(cm[0, 1], cm[0, 0] + cm[0, 1]),
                'val_term_false_rate': ratio(tm[0, 1], tm[0, 0] + tm[0, 1]),
                'val_epvar_over_mse_hH': ratio(tab['ep_var_mean'][last], np.mean(tab['mse_obs'][last])),
                'val_nonfinite': int(tab['n_nonfinite'].sum())}

    @staticmethod
    def _particles_diagnostics(pt, obs_dim):
        """The first and the last horizon of the particle table as ``val_*`` entries, means over the observation columns: the
        fair CRPS, the rank histogram's distance from flat, the share of recordings outside the cloud, spread over skill."""
        last = len(pt['n']) - 1
        col = lambda k, h: float(np.mean(pt[k][h, :obs_dim]))
        return {'val_crps_h1': col('crps', 0), 'val_crps_hH': col('crps', last),
                'val_rank_dev_h1': col('rank_dev', 0), 'val_rank_dev_hH': col('rank_dev', last),
                'val_outlier_rate_hH': col('outlier_rate', last),
                'val_spread_skill_h1': col('spread_skill', 0), 'val_spread_skill_hH': col('spread_skill', last),
                'val_particles_nonfinite': int(pt['n_nonfinite'].sum())}

    @staticmethod
    def _votes_diagnostics(vt):
        """The one-step row of the vote table as ``val_*`` entries: is the share a probability (ECE), how often do the members
        split, and what each reading of the vote would miss and report in vain."""
        ratio = lambda a, b: float(a) / float(b) if b > 0 else float('nan')
        out = {'val_vote_skipped': int(vt['n_skipped'].sum())}
        for name in ('cost', 'term'):
            if name not in vt:
                continue
            d = vt[name]
            out.update({'val_vote_ece_%s_h1' % name: float(d['ece'][0]), 'val_vote_split_%s_h1' % name: float(d['split_rate'][0])})
            for mode in ('any', 'majority'):
                c = d['cm'][mode][0]
                out.update({'val_%s_miss_rate_%s' % (name, mode): ratio(c[1, 0], c[1, 0] + c[1, 1]),
                            'val_%s_false_alarm_rate_%s' % (name, mode): ratio(c[0, 1], c[0, 0] + c[0, 1])})
        return out

    def _reliability_diagnostics(self, rel):
        """The one-step row of the reliability tables (the elite reading) as ``val_*`` entries and, with the recalibration
        switches, the offsets derived from it: set absolutely (the table is measured without them, so nothing winds up), kept
        where fewer than 100 rows entered."""
        from .replay import logit_offset
        out = {'val_rel_skipped': int(sum(col['n_skipped'].sum() for col in rel.values()))}
        for name, col in rel.items():
            d = col['elite']
            out.update({'val_ece_%s_h1' % name: float(d['ece'][0]), 'val_logloss_%s_h1' % name: float(d['logloss'][0]),
                        'val_base_rate_%s_h1' % name: float(d['base_rate'][0]), 'val_mean_p_%s_h1' % name: float(d['mean_p'][0])})
        if self._recalibrate_cost:
            b = logit_offset(rel, 'cost', 'elite', 0, *self._recalibration_range)
            if b is not None:
                self.fake_env.set_cost_recalibration(b)
            out['cost_recal_offset'] = float(self.fake_env.cost_recalibration)
        if self._recalibrate_term:
            b = logit_offset(rel, 'term', 'elite', 0, *self._recalibration_range)
            if b is not None:
                self.model_sampler.set_term_logit_offset(b)
            out['term_recal_offset'] = float(self.model_sampler.term_logit_offset or 0.0)
        return out

    def _set_rollout_length(self):
        """algorithms/cmbpo.py:494-512"""
        min_epoch, max_epoch, min_length, max_length = self._rollout_schedule
        if self._epoch <= min_epoch:
            y = min_length
        else:
            dx = min((self._epoch - min_epoch) / (max_epoch - min_epoch), 1)
            y = dx * (max_length - min_length) + min_length
        self._rollout_length = int(y)
        self.model_sampler.set_max_path_length(self._rollout_length)

    def _to_device(self, arrays):
        return [a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32,
                                                                      device=self.device) for a in arrays]

    def _reset_to_start_states(self, policy):
        """algorithms/cmbpo.py:239-251: draw the start states of a rollout round and reset the model sampler to them."""
        B = self._rollout_batch_size
        if self._start_state_sampling == 'device':
            self.model_sampler.reset(None, batch_size=B, fill=lambda cur_obs: self._buffer.sample_start_states(
                policy, B, alpha=self.sampling_alpha, out=cur_obs))
            return
        ep_b = self._buffer.epoch_batch(batch_size=B, epochs=self._buffer.epochs_list, fields=['observations', 'pi_infos'])
        kls = np.clip(policy.compute_DKL(ep_b['observations'], ep_b['mu'], ep_b['log_std']), a_min=0, a_max=None)
        btz_dist = self._buffer.boltz_dist(kls, alpha=self.sampling_alpha)
        btz_b = self._buffer.distributed_batch_from_archive(B, btz_dist, fields=['observations', 'pi_infos'])
        self.model_sampler.reset(btz_b['observations'])

    # -- the loop ------------------------------------------------------------------------------------------
    def _train(self):
        """Generator over diagnostics dicts; ``{'done': True, ...}`` ends it (algorithms/cmbpo.py:177-430)."""
        env_r, policy, pool = self._training_environment, self._policy, self._buffer
        if not self._training_started:
            self._initial_exploration_hook(env_r, self._initial_exploration_policy, pool)
        self.sampler.initialize(env_r, policy, pool)
        if self._use_model:
            self.model_sampler.initialize(self.fake_env, policy, self.model_buf)
            obs0 = self._buffer.rand_batch_from_archive(5000, fields=['observations'])['observations']
            rollout_dkl_lim = self.model_sampler.compute_dynamics_dkl(obs_batch=obs0, depth=self._rollout_schedule[2])
            self.model_sampler.set_rollout_dkl(rollout_dkl_lim)
            self.initial_model_dkl = self.model_sampler.dyn_dkl
            self.approx_model_batch = self.batch_size_policy - self.init_real_samples
        self.policy_epoch = 0
        self.new_real_samples = 0
        self.diag_counter = 0
        running_diag = {}

        for self._epoch in range(self._epoch, self._n_epochs):
            t0 = time.perf_counter()
            self.times = {}
            samples_added = 0
            model_samples = None
            model_weights = None      # (weighted updates only) one weight per row of model_samples
            keep_rolling = True
            metrics = {}
            if self._use_model:
                if self.rollout_mode == 'schedule':
                    self._set_rollout_length()
                while keep_rolling:
                    # starting states: Boltzmann distribution over the archived epochs, temperature = policy KL
                    self._reset_to_start_states(policy)
                    # the reference's loop over sample() (:352-360: stop at 99 % of the batch or at alive_ratio <= 0.1),
                    # taken in native code
                    self.model_sampler.sample_many(max_samples=int(self.approx_model_batch - samples_added),
                                                   stop_total=.99 * self.approx_model_batch - samples_added,
                                                   min_alive_ratio=0.1)
                    if self.model_sampler.global_total_samples + samples_added >= .99 * self.approx_model_batch:
                        keep_rolling = False
                    rollout_diagnostics = self.model_sampler.finish_all_paths()
                    model_samples_new, buffer_diagnostics_new = self.model_buf.get(as_tensors=True)
                    model_samples = [torch.cat((o, n), dim=0) for o, n in zip(model_samples, model_samples_new)] \
                        if model_samples else model_samples_new
                    if self._weighted:
                        w_new_rows = self.model_buf.last_weights * self._imagined_weight if self._trust_var is not None else \
                            torch.full((len(model_samples_new[0]),), self._imagined_weight, dtype=torch.float32, device=self.device)
                        model_weights = w_new_rows if model_weights is None else torch.cat((model_weights, w_new_rows))
                    new_n_samples = len(model_samples_new[0]) + EPS
                    w_old = samples_added / (new_n_samples + samples_added)
                    w_new = new_n_samples / (new_n_samples + samples_added)
                    metrics = update_dict(metrics, rollout_diagnostics, weight_a=w_old, weight_b=w_new)
                    metrics = update_dict(metrics, buffer_diagnostics_new, weight_a=w_old, weight_b=w_new)
                    if buffer_diagnostics_new['poolm_batch_size'] > 0:
                        model_data_diag = {k + '_m': v for k, v in policy.run_diagnostics(model_samples_new).items()}
                        metrics = update_dict(metrics, model_data_diag, weight_a=w_old, weight_b=w_new)
                    samples_added += new_n_samples
                    metrics.update({'samples_added': samples_added})
                metrics.update({'cached_var': np.mean(self._model.scaler_out.cached_var)})
                metrics.update({'cached_mu': np.mean(self._model.scaler_out.cached_mu)})
                t0 = self._stamp('epoch_rollout_model', t0)

            # ---- real sampling: as many steps as the model's uncertainty (vs its calibration) asks for ----------
            if self._use_model:
                n_real_samples = self.model_sampler.dyn_dkl / self.initial_model_dkl * self.init_real_samples
                n_real_samples = max(n_real_samples, self.min_real_samples)
            else:
                n_real_samples = self.batch_size_policy
            metrics.update({'n_real_samples': n_real_samples})
            start_samples = self.sampler._total_samples
            for i in count():
                self._timestep = self.sampler._total_samples - start_samples
                self._do_sampling(timestep=self.policy_epoch)
                if self.ready_to_train or self._timestep > n_real_samples:
                    self.sampler.finish_all_paths(append_val=True, append_cval=True, reset_path=False)
                    self.new_real_samples += self._timestep
                    break
            t0 = self._stamp('sample', t0)

            if self.new_real_samples > self._m_train_freq and self._use_model:
                metrics.update(self.train_model(**self._model_train_kwargs))
                self.new_real_samples = 0
            t0 = self._stamp('train_model', t0)

            real_samples, buf_diag = self._buffer.get()
            metrics.update({k + '_r': v for k, v in policy.run_diagnostics(real_samples).items()})
            metrics.update(buf_diag)
            if self._validate_horizon > 0 and self._use_model:
                t_val = time.perf_counter()      # a stamp of its own: 'train' keeps what it always contained
                metrics.update(self.validate_model(epochs=[self.policy_epoch]))
                self.times['validate_model'] = time.perf_counter() - t_val
                t0 += self.times['validate_model']

            # ---- updates on real + imagined samples ------------------------------------------------------------
            if model_samples:
                train_samples = [torch.cat((r, m), dim=0) for r, m in zip(self._to_device(real_samples), model_samples)]
            else:
                train_samples = real_samples
            weights = None
            if model_samples and model_weights is not None:
                n_real = len(real_samples[0])
                weights = torch.cat((torch.ones(n_real, dtype=torch.float32, device=self.device), model_weights))
                w_imagined = float(model_weights.sum(dtype=torch.float64))
                metrics_policy = {'policy/weight_sum_share_imagined': w_imagined / (w_imagined + n_real)}
            else:
                metrics_policy = {}
            policy.update_real_c(real_samples)
            policy.update_policy(train_samples, weights=weights)
            critic_kw = {'weights': weights} if weights is not None and getattr(policy, 'vf_weighted', False) else {}
            policy.update_critic(train_samples, train_vc=bool((train_samples[-3] > 0).any()),
                                 shuffle_on_device=self._shuffle_on_device, **critic_kw)
            if self._use_model:
                self.approx_model_batch = self.batch_size_policy - n_real_samples
            self.policy_epoch += 1
            policy.log()
            t0 = self._stamp('train', t0)

            self.sampler.log()
            new_diagnostics = dict(self.logger.dump_tabular(print_out=False))
            new_diagnostics.update(metrics_policy)
            new_diagnostics.update(OrderedDict((
                *((f'times/{k}', self.times[k]) for k in sorted(self.times)),
                *((f'model/{k}', metrics[k]) for k in sorted(metrics)),
            )))
            old_ts = running_diag.get('timestep', 0)
            new_ts = self._total_timestep - self.diag_counter - old_ts
            w_old, w_new = old_ts / (new_ts + old_ts), new_ts / (new_ts + old_ts)
            running_diag = update_dict(running_diag, new_diagnostics, weight_a=w_old, weight_b=w_new)
            running_diag.update({'timestep': new_ts + old_ts})
            if new_ts + old_ts > self.eval_every_n_steps:
                running_diag.update({'epoch': self._epoch, 'timesteps_total': self._total_timestep,
                                     'train-steps': self._num_train_steps})
                self.diag_counter = self._total_timestep
                diag, running_diag = running_diag.copy(), {}
                yield diag
            if self._total_timestep >= self.n_env_interacts:
                self.sampler.terminate()
                yield {'done': True, **running_diag}
                break

    def train(self, *args, **kwargs):
        return self._train(*args, **kwargs)

    def get_diagnostics(self, iteration, obs_batch=None, training_paths=None, evaluation_paths=None):
        warnings.warn('diagnostics not implemented yet!')     # as the reference (algorithms/cmbpo.py:520-533)
        return {}

    def save(self, savedir):
        if self._use_model:
            self._model.save(savedir, self._epoch)
            if self._m_learn_term:      # threshold and vote of the termination head, beside the model's files
                import json
                import os
                with open(os.path.join(savedir, 'term_head_%d.json' % self._epoch), 'w') as fh:
                    json.dump({'threshold': self.fake_env.term_threshold, 'members': self.fake_env.term_members}, fh)
                # the column's likelihood, a file of its own: term_head_<epoch>.json keeps exactly its keys
                with open(os.path.join(savedir, 'term_loss_%d.json' % self._epoch), 'w') as fh:
                    json.dump({'m_term_loss': self._m_term_loss}, fh)
                # sampled terminations, likewise
                with open(os.path.join(savedir, 'term_sampling_%d.json' % self._epoch), 'w') as fh:
                    json.dump({'m_term_sampling': bool(getattr(self, '_m_term_sampling', False))}, fh)
            if self._m_learn_cost:      # the reading of the cost column, a file of its own
                import json
                import os
                with open(os.path.join(savedir, 'cost_loss_%d.json' % self._epoch), 'w') as fh:
                    json.dump({'m_cost_loss': self._m_cost_loss, 'm_cost_pos_weight': self._cost_pos_weight,
                               'm_cost_pos_weight_undo': self._cost_pos_weight_undo,
                               'cost_logit_shift': self.fake_env.cost_logit_shift}, fh)
            if self._m_learn_term or self._m_learn_cost:      # the column weights of the fits, a file of their own
                import json
                import os
                with open(os.path.join(savedir, 'column_weights_%d.json' % self._epoch), 'w') as fh:
                    json.dump(self._column_weights, fh)

            if self._m_learn_term or self._m_learn_cost:      # reliability and recalibration, a file of their own
                import json
                import os
                with open(os.path.join(savedir, 'recalibration_%d.json' % self._epoch), 'w') as fh:
                    json.dump(self._recalibration_state(), fh)

    RECALIBRATION_KEYS = ('m_validate_reliability', 'm_reliability_bins', 'm_recalibrate_cost', 'm_recalibrate_term',
                          'm_recalibration_range', 'cost_recal_offset', 'term_recal_offset')

    def _recalibration_state(self):
        """What ``recalibration_<epoch>.json`` keeps: the five switches and the two offsets in force."""
        sampler = getattr(self, 'model_sampler', None)
        return {'m_validate_reliability': self._validate_reliability, 'm_reliability_bins': self._reliability_bins,
                'm_recalibrate_cost': self._recalibrate_cost, 'm_recalibrate_term': self._recalibrate_term,
                'm_recalibration_range': list(self._recalibration_range),
                'cost_recal_offset': float(getattr(self.fake_env, 'cost_recalibration', 0.0)),
                'term_recal_offset': float(getattr(sampler, 'term_logit_offset', None) or 0.0)}

    def _load_recalibration(self, savedir, timestep):
        """The switches and offsets ``save`` wrote, checked like the constructor's and handed to the environment and the model
        sampler (a checkpoint from before them has no such file: the constructor's switches stay, the offsets are 0)."""
        import json
        import os
        path = os.path.join(savedir, 'recalibration_%d.json' % int(timestep))
        kw = {'cost_recal_offset': 0.0, 'term_recal_offset': 0.0}
        if os.path.exists(path):
            with open(path) as fh:
                kw = json.load(fh)
            (self._validate_reliability, self._reliability_bins, self._recalibrate_cost, self._recalibrate_term,
             self._recalibration_range) = _reliability_args(
                getattr(self, '_validate_horizon', 0), self._use_model, self._m_cost_loss, getattr(self, '_m_term_loss', 'gaussian'),
                getattr(self, '_m_term_sampling', False), kw['m_validate_reliability'], kw['m_reliability_bins'],
                kw['m_recalibrate_cost'], kw['m_recalibrate_term'], kw['m_recalibration_range'])
        # (an offset is handed over only where it changes something: an environment or a sampler without one is left alone)
        b_cost = float(kw['cost_recal_offset']) if self._m_cost_loss == 'logistic' else 0.0
        if b_cost != getattr(self.fake_env, 'cost_recalibration', 0.0):
            self.fake_env.set_cost_recalibration(b_cost)
        sampler = getattr(self, 'model_sampler', None)
        on = getattr(self, '_m_term_sampling', False) and getattr(self, '_m_term_loss', 'gaussian') == 'logistic'
        b_term = (float(kw['term_recal_offset']) if on else 0.0) or None
        if sampler is not None and b_term != getattr(sampler, 'term_logit_offset', None):
            sampler.set_term_logit_offset(b_term)

    def _load_column_weights(self, savedir, timestep):
        """The four keys ``save`` wrote (a checkpoint from before them has no such file: the constructor's stay)."""
        import json
        import os
        path = os.path.join(savedir, 'column_weights_%d.json' % int(timestep))
        if not os.path.exists(path):
            return
        with open(path) as fh:
            kw = json.load(fh)
        self._column_weights = _column_weight_args(self._m_learn_term, self._m_learn_cost, *(kw[k] for k in COLUMN_WEIGHT_KEYS))
        if (kw['m_term_pos_weight'], kw['m_term_loss_weight'], kw['m_cost_loss_weight']) == (1.0, 1.0, 1.0):
            self._model.set_column_weights(None, None)

    def _logistic_columns(self):
        """The model columns trained with the Bernoulli likelihood: the cost column obs_dim + 1 and / or the last one."""
        cols = ([self.obs_dim + 1] if self._m_cost_loss == 'logistic' else []) + ([-1] if self._m_term_loss == 'logistic' else [])
        return cols or None

    def _load_cost_loss(self, savedir, timestep):
        """The reading of the cost column that ``save`` wrote (a checkpoint from before it has no such file: 'gaussian', no
        class weight, no shift); read before the model's weights and scalers come in, like the termination column's."""
        import json
        import os
        if not self._m_learn_cost:
            return None
        path = os.path.join(savedir, 'cost_loss_%d.json' % int(timestep))
        kw = {'m_cost_loss': 'gaussian', 'm_cost_pos_weight': 1.0, 'm_cost_pos_weight_undo': False, 'cost_logit_shift': 0.0}
        if os.path.exists(path):
            with open(path) as fh:
                kw.update(json.load(fh))
        self._m_cost_loss, self._cost_pos_weight, self._cost_pos_weight_undo = _cost_loss_args(
            True, kw['m_cost_loss'], kw['m_cost_pos_weight'], kw['m_cost_pos_weight_undo'], self._column_weights['m_pos_weight_max'])
        return kw

    def _load_term_loss(self, savedir, timestep):
        """The likelihood of the termination column that ``save`` wrote (a checkpoint from before it has no such file:
        'gaussian'), set on the model before its weights and scalers come in."""
        import json
        import os
        if not self._m_learn_term:
            return None
        path = os.path.join(savedir, 'term_loss_%d.json' % int(timestep))
        term_loss = 'gaussian'
        if os.path.exists(path):
            with open(path) as fh:
                term_loss = json.load(fh)['m_term_loss']
        if term_loss not in ('gaussian', 'logistic'):
            raise ValueError("%s: m_term_loss %r" % (path, term_loss))
        self._m_term_loss = term_loss
        self._model.set_logistic_columns(self._logistic_columns())
        return term_loss

    def _load_term_sampling(self, savedir, timestep):
        """The flag of the sampled terminations that ``save`` wrote (a checkpoint from before it has no such file, or no such
        key: off), handed to the model sampler."""
        import json
        import os
        if not self._m_learn_term:
            return
        path = os.path.join(savedir, 'term_sampling_%d.json' % int(timestep))
        on = False
        if os.path.exists(path):
            with open(path) as fh:
                on = bool(json.load(fh).get('m_term_sampling', False))
        self._m_term_sampling = on
        sampler = getattr(self, 'model_sampler', None)
        if sampler is not None and sampler.term_sampling != on:
            sampler.term_sampling = on
            sampler._draws = None       # (the next step draws a chunk with / without the thresholds)

    def load(self, savedir, timestep):
        """The model ``save`` wrote at epoch ``timestep`` and, with the termination head, its threshold and vote."""
        if not self._use_model:
            raise ValueError("load: the trainer was built with use_model=False, there is no model to load")
        cost_head = self._load_cost_loss(savedir, timestep)
        term_loss = self._load_term_loss(savedir, timestep)
        if cost_head is not None and not self._m_learn_term:      # (with a termination head _load_term_loss has set both)
            self._model.set_logistic_columns(self._logistic_columns())
        self._model.load(savedir, timestep)
        self._load_column_weights(savedir, timestep)
        if cost_head is not None:
            self.fake_env.set_cost_head(cost_head['m_cost_loss'], cost_head['cost_logit_shift'] if cost_head['m_cost_loss'] == 'logistic' else 0.0)
        if self._m_learn_term:
            import json
            import os
            with open(os.path.join(savedir, 'term_head_%d.json' % int(timestep))) as fh:
                head = json.load(fh)
            self.fake_env.set_term_head(head['threshold'], head['members'], loss=term_loss)
            self._load_term_sampling(savedir, timestep)
        self._load_recalibration(savedir, timestep)
