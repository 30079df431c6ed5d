"""FakeEnv -- host-side mirror of ``models/fake_env.py:15-197``.

Same constructor, ``step(obs, act, deterministic=True)`` signature and return tuple
``(next_obs, r, terms, info)`` with the info keys of ``models/fake_env.py:164-170``.  The ensemble
forward and everything after it run in HIP (``cmbpo_ens_forward`` + ``cmbpo_fakeenv_post``).

Differences that are part of the contract:
  * the per-branch elite draw (``random_inds``, :174-178, global NumPy RNG) can be injected through
    ``model_inds=`` so a test / a sharded run can reproduce it; by default it is drawn with a
    seeded ``numpy.random.Generator`` owned by this object;
  * ``deterministic=False`` (mean + std, :105-106) and the 3-D input path (:84-101, unused by the
    trainer and not an inverse) raise NotImplementedError;
  * ``noise=`` ([n, obs_dim], NumPy or CUDA tensor, in the order of ``obs``) samples the transition:
    ``next_obs = mean + std * noise + obs`` per observation dimension, one draw per (row, dimension) for all members;
    the uncertainty measures are taken on the shifted means, reward and learned cost are the elite's unperturbed columns
    (``cmbpo_fakeenv_post_noise``).  ``noise=np.ones(...)`` is the reference's ``deterministic=False``.

``predicts_cost=True`` (:139-143, ``m_learn_cost`` of the trainer) takes the cost of a branch from the
elite member's mean of the model's last output column (``output_dim == obs_dim + 2``) instead of the
task's cost rule; the task's termination rule still applies.  ``info['cost']`` is then the float32
prediction, not thresholded.

``disagreement=True`` measures what the members that were not picked say about reward and cost: ``step()`` adds
``info['ensemble_rew_var']`` / ``info['ensemble_cost_var']`` (``np.var`` over all members of the reward column and, with
``predicts_cost``, of the cost column; without it the cost variance is 0).  ``rew_pessimism`` / ``cost_pessimism`` (kappa >= 0;
> 0 switches the measurement on) make the returned reward ``r - kappa_r * sqrt(rew_var)`` and the learned cost
``c + kappa_c * sqrt(cost_var)`` (``cmbpo_fakeenv_post_disagreement``); ``set_pessimism(rew, cost)`` changes them later.
``cost_pessimism > 0`` needs ``predicts_cost`` or the static votes below: a static cost rule judged on the elite's state alone
has no member spread.  Off (the default) the calls made
and the keys returned are what they were.

``predicts_term=True`` (no counterpart in the reference, ``m_learn_term`` of the trainer): the model has one more
output column, the LAST one, trained on the real ``done`` flags, and a branch also ends where that column says so:
``term = rule_done or learned_done`` with ``learned_done`` the elite member's ``x > term_threshold`` (``term_members='elite'``),
any member's (``'any'``) or more than half of all members' (``'majority'``).  The cost keeps the rule's own ``done``.  ``step()``
adds ``info['term_pred']`` (the elite's value of the column) and ``info['term_votes']`` (members above the threshold, uint8);
``set_term_head(threshold, members)`` changes the head later.  Off (the default) nothing changes.
``term_loss='logistic'`` (a model whose last column is logistic, ``PE(logistic_columns=[-1])``): the column is a
logit z, ``term_threshold`` a probability tau strictly inside (0, 1), and the test ``sigma(z) > tau`` runs in the same kernel as
``z > float32(logit(tau))``; ``info['term_pred']`` is ``sigma(z)`` in float32.

``term_draws=`` of ``step()`` ([n] uniform draws u in (0, 1], in the order of ``obs``) and ``term_thr=`` of ``step_device()``
(a slot-indexed float32 CUDA tensor of thresholds) SAMPLE the learned termination: row r's members are compared
with the row's own threshold instead of ``term_threshold`` -- ``utils.term_thresholds(u, term_loss)``: ``logit(u)`` under
'logistic', ``u`` under 'gaussian' -- so a branch whose column says p ends with probability p
(``cmbpo_fakeenv_post_term_draws``).  The vote, ``info['term_pred']`` and ``info['term_votes']`` are what they were; all members
of a row share the row's draw.  Both need ``predicts_term=True``.

``cost_loss='logistic'`` (needs ``predicts_cost=True``; a model whose cost column is logistic,
``PE(logistic_columns=[obs_dim + 1])``): the column is a logit z and the cost of a step its probability
``sigma(z - cost_logit_shift)`` in [0, 1], computed in the kernel; the disagreement variance is taken on the members'
probabilities and the pessimistic cost ``p + kappa_c * sqrt(var)`` is clipped at 1.  ``step()`` returns the probability as cost
and adds ``info['cost_logit']`` (the elite's raw logit); ``set_cost_head(loss, logit_shift)`` changes the head later.
``cost_logit_shift = log(omega)`` undoes a class weight omega the column was trained with.  Targets above 0.5 count as 1, so a
task whose cost is a magnitude, not an indicator, should keep the default ``'gaussian'``.

``static_term_members`` / ``static_cost_members`` (``'elite'`` | ``'any'`` | ``'majority'``, the cost also ``'mean'``)
let the ensemble VOTE on the task's own static rules: the termination and cost rule (``AntSafe``, ``HCS``, a ``TaskRules`` table)
are evaluated on every member's predicted next state, not only on the elite's, and a branch ends / a step costs by the elite's
verdict (what it always was), any member's, more than half of all members', or -- the cost only -- the share of members
``votes / E``.  ``static_votes=True`` measures without changing a verdict.  The vote kernel runs iff a mode is not ``'elite'`` or
``static_votes`` is set; ``step()`` then adds ``info['static_term_votes']`` / ``info['static_cost_votes']`` (uint8), and with
``disagreement`` ``info['ensemble_cost_var']`` carries the static cost's spread, which ``cost_pessimism > 0`` may now act on
(``min(1, c + kappa_c * sqrt(var))``).  ``static_cost_members != 'elite'`` needs ``predicts_cost=False`` (a learned cost skips the
static rule).  ``set_static_votes(...)`` changes them later.  A replay keeps the elite's rule unless asked: ``replay(..., votes=True)`` replays
under the vote and adds the vote table.  Off (the default) the calls made and
the keys returned are what they were.

``replay(...)`` has no counterpart in the reference: it replays windows of real steps through the model with the recorded
actions and returns, per horizon, how far the predictions are from the recording (open-loop model validation).
``replay(..., reliability=True)`` also measures whether a logistic column is a probability, and
``set_cost_recalibration(b)`` feeds the measured logit offset of the cost column back: the kernels then subtract
``float32(cost_logit_shift + b)``.  ``replay(..., particles=S)`` adds a second pass in which every window is replayed by S
sampled particles and the recording is held against their cloud (rank histograms, CRPS, spread against skill).

``task`` is a built-in task name, a name given to ``statics.register_task``, or a ``statics.TaskRules`` (user-defined
termination / cost rules, evaluated by the same kernel); any other name is the default task, as in the reference.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, statics


class FakeEnv:
    def __init__(self, true_environment, task, model, predicts_delta, predicts_rew, predicts_cost,
                 seed=0, disagreement=False, rew_pessimism=0.0, cost_pessimism=0.0,
                 predicts_term=False, term_threshold=0.5, term_members='elite', term_loss='gaussian',
                 cost_loss='gaussian', cost_logit_shift=0.0,
                 static_term_members='elite', static_cost_members='elite', static_votes=False):
        self.env = true_environment
        self.obs_dim = int(np.prod(self.observation_space.shape))
        self.act_dim = int(np.prod(self.action_space.shape))
        self._task = task
        self._model = model
        self._uses_ensemble = model.is_ensemble
        self._is_probabilistic = model.is_probabilistic
        if not (self._uses_ensemble and self._is_probabilistic):
            raise NotImplementedError("the HIP path needs a probabilistic ensemble (all CMBPO configs)")
        if not (predicts_delta and predicts_rew):
            raise NotImplementedError("HIP path: predicts_delta=True, predicts_rew=True (algorithms/cmbpo.py:137-142)")
        self._predicts_delta, self._predicts_rew, self._predicts_cost = True, True, bool(predicts_cost)
        self.input_dim = model.in_dim
        self.output_dim = model.out_dim
        assert self.input_dim == self.obs_dim + self.act_dim
        self._predicts_term = bool(predicts_term)
        assert self.output_dim == self.obs_dim + 1 + int(self._predicts_cost) + int(self._predicts_term)
        # the `task` argument of the native entry points: the rule id, with the learned-cost flag where the model has the head
        # (every caller that passes it -- this class, ModelSampler, the probes -- thereby runs the mode the scratch is sized for)
        self._task_id, self._rules = statics.lookup(task)
        # where the reference's step() returns np.zeros_like(terms), a bool array (models/fake_env.py:145-146): no learned
        # cost and no cost function for the task
        self._bool_cost = not self._predicts_cost and (
            self._task_id == _lib.TASK_DEFAULT or (self._rules is not None and not self._rules.has_cost))
        if self._predicts_cost:
            self._task_id |= _lib.TASK_LEARNED_COST
        self._rng = np.random.default_rng(seed)
        # the elite draws of replay(): a stream of its own, so that a run that validates is in all else the run that does not
        self._replay_rng = np.random.default_rng(np.random.SeedSequence(seed, spawn_key=(1,)))
        # the seeds of replay(particles=S) calls without a particle_seed: a third stream, for the same reason
        self._particle_seeds = np.random.default_rng(np.random.SeedSequence(seed, spawn_key=(2,)))
        self._disagreement = bool(disagreement)
        self.rew_pessimism = self.cost_pessimism = 0.0
        self.static_term_members, self.static_cost_members, self.static_votes = 'elite', 'elite', False
        self.set_static_votes(static_term_members, static_cost_members, static_votes)
        self.set_pessimism(rew_pessimism, cost_pessimism)
        self.term_threshold, self.term_members, self.term_loss = 0.5, 'elite', 'gaussian'
        if term_loss not in ('gaussian', 'logistic'):
            raise ValueError(f"term_loss: 'gaussian' or 'logistic', got {term_loss!r}")
        if self._predicts_term:
            self.set_term_head(term_threshold, term_members, term_loss)
        elif term_loss != 'gaussian':
            raise ValueError("term_loss='logistic' needs predicts_term=True: the model has no termination column")
        self.cost_loss, self.cost_logit_shift = 'gaussian', 0.0
        self.cost_recalibration = 0.0               # see set_cost_recalibration()
        self.set_cost_head(cost_loss, cost_logit_shift)
        self.device = model.device
        # bench.py sets this to a list to collect (start, end) HIP events around the dominant kernel
        self.kernel_events = None

    @property
    def observation_space(self):
        return self.env.observation_space

    @property
    def action_space(self):
        return self.env.action_space

    @property
    def disagreement(self):
        """True when the ensemble's disagreement on reward / cost is measured (switched on, or a coefficient > 0)."""
        return self._disagreement or self.rew_pessimism > 0.0 or self.cost_pessimism > 0.0

    def set_pessimism(self, rew, cost):
        """The coefficients of the pessimistic reward r - rew * sigma_r and learned cost c + cost * sigma_c."""
        rew, cost = float(rew), float(cost)
        if not (np.isfinite(rew) and rew >= 0.0 and np.isfinite(cost) and cost >= 0.0):
            raise ValueError(f"rew_pessimism / cost_pessimism must be finite numbers >= 0, got {rew}, {cost}")
        if cost > 0.0 and not self._predicts_cost and not self.static_votes_on:
            raise ValueError("cost_pessimism > 0 needs predicts_cost=True: a static cost rule has no ensemble spread (unless the "
                             "members vote on it: static_votes=True or a static_*_members mode other than 'elite')")
        self.rew_pessimism, self.cost_pessimism = rew, cost

    @property
    def static_votes_on(self):
        """True when the vote kernel runs behind the post kernel: a mode other than 'elite', or ``static_votes``."""
        return self.static_votes or self.static_term_members != 'elite' or self.static_cost_members != 'elite'

    def set_static_votes(self, term_members=None, cost_members=None, votes=None):
        """Whose verdict of the task's static termination rule ends a branch ('elite' / 'any' / 'majority') and whose verdict of
        its static cost rule a step costs (those, or 'mean': votes / E); ``votes=True`` measures the votes without changing a
        verdict.  None leaves a setting as it is."""
        tm = self.static_term_members if term_members is None else term_members
        cm = self.static_cost_members if cost_members is None else cost_members
        on = self.static_votes if votes is None else bool(votes)
        if tm not in _lib.RULE_DONE_MEMBERS:
            raise ValueError(f"static_term_members: 'elite', 'any' or 'majority', got {tm!r}")
        if cm not in _lib.RULE_COST_MEMBERS:
            raise ValueError(f"static_cost_members: 'elite', 'any', 'majority' or 'mean', got {cm!r}")
        if cm != 'elite' and self._predicts_cost:
            raise ValueError(f"static_cost_members={cm!r} needs predicts_cost=False: with a learned cost the task's static cost "
                             "rule is skipped, there is nothing to vote on")
        if not (on or tm != 'elite' or cm != 'elite') and self.cost_pessimism > 0.0 and not self._predicts_cost:
            raise ValueError("the static votes cannot be switched off while cost_pessimism > 0 acts on a static cost "
                             "(set_pessimism(rew, 0.0) first)")
        self.static_term_members, self.static_cost_members, self.static_votes = tm, cm, on

    def rule_votes_struct(self, done_votes=None, cost_votes=None):
        """The ``cmbpo_rule_votes_t`` of the static votes (None when they are off: the call without the vote kernel); the two
        optional outputs are device tensors or None (no cost votes with a learned cost)."""
        if not self.static_votes_on:
            return None
        rv = _lib.RuleVotesStruct()
        rv.done_members = _lib.RULE_DONE_MEMBERS[self.static_term_members]
        rv.cost_members = _lib.RULE_COST_MEMBERS[self.static_cost_members]
        rv.done_votes = _lib.ptr(done_votes)
        rv.cost_votes = None if self._predicts_cost else _lib.ptr(cost_votes)
        return rv

    @property
    def predicts_term(self):
        return self._predicts_term

    def set_term_head(self, threshold, members, loss=None):
        """Threshold and vote ('elite' / 'any' / 'majority') of the learned termination head; ``loss`` ('gaussian' /
        'logistic', None: as it is) says how the column was trained.  Under 'logistic' the threshold is a probability strictly
        inside (0, 1)."""
        if not self._predicts_term:
            raise ValueError("set_term_head needs predicts_term=True: the model has no termination column")
        loss = self.term_loss if loss is None else loss
        if loss not in ('gaussian', 'logistic'):
            raise ValueError(f"term_loss: 'gaussian' or 'logistic', got {loss!r}")
        threshold = float(threshold)
        if not np.isfinite(threshold):
            raise ValueError(f"term_threshold must be a finite number, got {threshold}")
        if loss == 'logistic':
            from .utils import logit_threshold
            logit_threshold(threshold)
        if members not in _lib.TERM_MEMBERS:
            raise ValueError(f"term_members: 'elite', 'any' or 'majority', got {members!r}")
        self.term_threshold, self.term_members, self.term_loss = threshold, members, loss

    @property
    def term_kernel_threshold(self):
        """The number the kernels compare the termination column with: ``term_threshold``, under 'logistic' its float32 logit."""
        if self.term_loss == 'logistic':
            from .utils import logit_threshold
            return logit_threshold(self.term_threshold)
        return self.term_threshold

    def term_head_struct(self, term_pred=None, term_votes=None):
        """The ``cmbpo_term_head_t`` of this head (None without one); the two optional outputs are device tensors or None."""
        if not self._predicts_term:
            return None
        th = _lib.TermHeadStruct()
        th.threshold, th.members = self.term_kernel_threshold, _lib.TERM_MEMBERS[self.term_members]
        th.term_pred, th.term_votes = _lib.ptr(term_pred), _lib.ptr(term_votes)
        return th

    def set_cost_head(self, loss=None, logit_shift=None):
        """How the learned-cost column is read: ``loss`` 'gaussian' (a magnitude, the reference's reading) or 'logistic' (a
        logit; the cost is its probability), ``logit_shift`` the finite number subtracted from the logit first (log omega
        undoes a class weight omega).  None leaves a setting as it is."""
        loss = self.cost_loss if loss is None else loss
        shift = self.cost_logit_shift if logit_shift is None else float(logit_shift)
        if loss not in _lib.COST_KINDS:
            raise ValueError(f"cost_loss: 'gaussian' or 'logistic', got {loss!r}")
        if loss == 'logistic' and not self._predicts_cost:
            raise ValueError("cost_loss='logistic' needs predicts_cost=True: the model has no cost column to read as a logit")
        if not np.isfinite(shift):
            raise ValueError(f"cost_logit_shift must be a finite number, got {shift}")
        self.cost_loss, self.cost_logit_shift = loss, shift

    def set_cost_recalibration(self, offset):
        """The logit offset b of a measured recalibration of the logistic cost column (``replay.logit_offset``): the
        shift handed to the kernels becomes ``float32(cost_logit_shift + b)``, the cost ``sigma(z - cost_logit_shift - b)``.  It is
        set absolutely, not accumulated; 0.0 (the default) hands over ``cost_logit_shift`` as it always was.  ``replay(...,
        reliability=True)`` measures the column WITHOUT it.  A rollout pool picks it up at the sampler's ``reset()``."""
        offset = float(offset)
        if not np.isfinite(offset):
            raise ValueError(f"set_cost_recalibration: the offset must be a finite number, got {offset}")
        if offset != 0.0 and self.cost_loss != 'logistic':
            raise ValueError("set_cost_recalibration needs cost_loss='logistic': a Gaussian cost column is not a logit, there is "
                             "nothing to shift")
        self.cost_recalibration = offset

    @property
    def cost_kernel_shift(self):
        """The number the kernels subtract from the cost logit: ``cost_logit_shift``, with a recalibration offset b the float32
        sum ``cost_logit_shift + b``."""
        if self.cost_recalibration == 0.0:
            return self.cost_logit_shift
        return float(np.float32(self.cost_logit_shift + self.cost_recalibration))

    def cost_head_struct(self, cost_logit=None):
        """The ``cmbpo_cost_head_t`` of this head (None under 'gaussian': the call without one); the optional output is a device
        tensor or None."""
        if self.cost_loss != 'logistic':
            return None
        ch = _lib.CostHeadStruct()
        ch.kind, ch.logit_shift, ch.cost_logit = _lib.COST_LOGISTIC, self.cost_kernel_shift, _lib.ptr(cost_logit)
        return ch

    def reliability_columns(self):
        """The columns ``replay(..., reliability=True)`` measures: whichever of the cost and the termination head is logistic, as
        the list ``ReplayBuffers(reliability=dict(columns=...))`` takes.  The cost column carries ``cost_logit_shift`` (the class-
        weight undo, NOT the recalibration offset: the table measures what the offset is derived from), the termination column 0."""
        cols = []
        if self.cost_loss == 'logistic':
            cols.append(dict(name='cost', col=self.obs_dim + 1, target='cost', shift=self.cost_logit_shift))
        if self._predicts_term and self.term_loss == 'logistic':
            cols.append(dict(name='term', col=self.output_dim - 1, target='term', shift=0.0))
        if not cols:
            raise ValueError("reliability=True needs a logistic head (cost_loss='logistic' or term_loss='logistic'): a Gaussian "
                             "column is not a logit, it has no reliability table")
        return cols

    def random_inds(self, size):
        """One elite per branch (models/fake_env.py:174-178), from this object's seeded generator."""
        elites = np.asarray(self._model.elite_inds, dtype=np.int32)
        return elites[self._rng.integers(0, len(elites), size=size)]

    def step_device(self, obs, act, model_inds, out, row_idx=None, n_rows=None, scratch=None, noise=None, term_thr=None):
        """Device-resident step: all arguments are CUDA tensors indexed by branch slot (noise: [B, obs_dim] float32
        N(0, 1) draws for stochastic transitions, None: the elite member's mean).

        out: dict with next_obs[B,obs], rew[B], term[B] u8, cost[B], dkl_path[B], ep_var_mean[B]
        (and optionally ep_var[B,obs]).  scratch: (mean, var)[E,B,output_dim].  With `disagreement` on, out also needs
        rew_var[B] and cost_var[B]; they are filled, and rew / cost are the penalised values.  With `predicts_term`, term is
        rule_done or learned_done, and out's optional term_pred[B] / term_votes[B] u8 are filled (under
        ``term_loss='logistic'`` term_pred carries the logit).  With ``cost_loss='logistic'`` cost is the probability and out's
        optional cost_logit[B] is filled with the elite's raw logit.  term_thr: [B] float32 thresholds of the sampled
        terminations, in the column's own units (``utils.term_thresholds``), in place of the head's threshold; None: the head's.
        With the static votes on (``static_votes_on``) term / cost are the voted ones, out's optional static_term_votes[B] /
        static_cost_votes[B] u8 are filled, and with `predicts_term` out's term_pred and term_votes are required.
        """
        B = obs.shape[0]
        if term_thr is not None:
            if not self._predicts_term:
                raise ValueError("term_thr needs predicts_term=True: the model has no termination column to compare the "
                                 "thresholds with")
            if not (term_thr.is_cuda and term_thr.dtype == torch.float32 and term_thr.is_contiguous()
                    and tuple(term_thr.shape) == (B,)):
                raise ValueError("term_thr must be a contiguous float32 CUDA tensor of shape [%d]" % B)
        if noise is not None and not (noise.is_cuda and noise.dtype == torch.float32 and noise.is_contiguous()
                                      and tuple(noise.shape) == (B, self.obs_dim)):
            raise ValueError("noise must be a contiguous float32 CUDA tensor of shape [%d, %d]" % (B, self.obs_dim))
        n = B if row_idx is None else (row_idx.shape[0] if n_rows is None else n_rows)
        E = self._model.num_nets
        if scratch is None:
            mean = torch.empty((E, B, self.output_dim), dtype=torch.float32, device=self.device)
            var = torch.empty_like(mean)
        else:
            mean, var = scratch
        lib = _lib.lib()
        stream = _lib.current_stream()
        ev = None
        if self.kernel_events is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()      # same stream the kernel is launched on (torch's current stream)
        _lib.check(lib.cmbpo_ens_forward(self._model.mlp.handle, _lib.ptr(obs), self.obs_dim,
                                         _lib.ptr(act), self.act_dim, _lib.ptr(row_idx), None, n, B,
                                         _lib.ptr(mean), _lib.ptr(var), stream), "cmbpo_ens_forward")
        if ev is not None:
            ev[1].record()
            self.kernel_events.append((ev[0], ev[1], n))
        # one call of the superset entry point, NULL / 0 for what is off (the library's message names the narrowest entry)
        dis = (self.rew_pessimism, self.cost_pessimism, _lib.ptr(out["rew_var"]), _lib.ptr(out["cost_var"])) \
            if self.disagreement else (0.0, 0.0, None, None)
        th = self.term_head_struct(out.get("term_pred"), out.get("term_votes"))
        ch = self.cost_head_struct(out.get("cost_logit"))
        args = (self._task_id, E, self.obs_dim, self.act_dim, _lib.ptr(mean), _lib.ptr(var), B, _lib.ptr(obs), _lib.ptr(act),
                _lib.ptr(model_inds), _lib.ptr(row_idx), None, n, _lib.ptr(out["next_obs"]), _lib.ptr(out["rew"]),
                _lib.ptr(out["term"]), _lib.ptr(out["cost"]), _lib.ptr(out["dkl_path"]), _lib.ptr(out["ep_var_mean"]),
                _lib.ptr(out.get("ep_var")), _lib.ptr(noise), *dis, C.byref(th) if th is not None else None,
                C.byref(ch) if ch is not None else None)
        rv = self.rule_votes_struct(out.get("static_term_votes"), out.get("static_cost_votes"))
        if rv is not None:      # the votes on the static rules: the same call with the thresholds (or NULL) and the votes behind it
            _lib.check(lib.cmbpo_fakeenv_post_votes(*args, _lib.ptr(term_thr), C.byref(rv), stream), "cmbpo_fakeenv_post_votes")
        elif term_thr is None:
            _lib.check(lib.cmbpo_fakeenv_post_cost(*args, stream), "cmbpo_fakeenv_post_cost")
        else:       # sampled terminations: the same call with the thresholds behind it
            _lib.check(lib.cmbpo_fakeenv_post_term_draws(*args, _lib.ptr(term_thr), stream), "cmbpo_fakeenv_post_term_draws")
        return out

    def step(self, obs, act, deterministic=True, model_inds=None, noise=None, term_draws=None):
        assert len(obs.shape) == len(act.shape)
        assert obs.shape[-1] == self.obs_dim and act.shape[-1] == self.act_dim
        if term_draws is not None and not self._predicts_term:
            raise ValueError("term_draws needs predicts_term=True: the model has no termination column to sample from")
        if not deterministic:
            raise NotImplementedError("deterministic=False (mean + std) is never used by the trainer; pass "
                                      "noise=np.ones((n, obs_dim), np.float32) for the reference's mean + std, or "
                                      "N(0, 1) draws to sample the transition")
        if len(obs.shape) == 3:
            raise NotImplementedError("3-D inputs (forward_shuffle) are never used by the trainer")
        single = len(obs.shape) == 1
        if single:
            obs, act = obs[None], act[None]
            if noise is not None and len(noise.shape) == 1:
                noise = noise[None]
        was_np = not isinstance(obs, torch.Tensor)
        with torch.cuda.device(self.device):
            o = torch.as_tensor(np.ascontiguousarray(obs, dtype=np.float32) if was_np else obs,
                                dtype=torch.float32, device=self.device).contiguous()
            a = torch.as_tensor(np.ascontiguousarray(act, dtype=np.float32) if was_np else act,
                                dtype=torch.float32, device=self.device).contiguous()
            n = o.shape[0]
            xi = None
            if noise is not None:
                xi = torch.as_tensor(np.ascontiguousarray(noise, dtype=np.float32) if not isinstance(noise, torch.Tensor)
                                     else noise, dtype=torch.float32, device=self.device).contiguous()
                if tuple(xi.shape) != (n, self.obs_dim):
                    raise ValueError("noise must have shape [%d, %d], got %s" % (n, self.obs_dim, tuple(xi.shape)))
            thr = None
            if term_draws is not None:
                from .utils import term_thresholds
                u = term_draws if isinstance(term_draws, torch.Tensor) else np.asarray(term_draws)
                if tuple(u.shape) == () and single:
                    u = u[None]
                if tuple(u.shape) != (n,):
                    raise ValueError("term_draws must have shape [%d], got %s" % (n, tuple(u.shape)))
                thr = term_thresholds(u, self.term_loss)      # (rows are slots here)
                thr = torch.as_tensor(thr, dtype=torch.float32, device=self.device).contiguous()
            if model_inds is None:
                model_inds = self.random_inds(n)
            inds = torch.as_tensor(np.asarray(model_inds, dtype=np.int32), device=self.device) \
                if not isinstance(model_inds, torch.Tensor) else model_inds.to(self.device, torch.int32)
            f = dict(dtype=torch.float32, device=self.device)
            out = dict(next_obs=torch.empty((n, self.obs_dim), **f), rew=torch.empty(n, **f),
                       term=torch.empty(n, dtype=torch.uint8, device=self.device),
                       cost=torch.empty(n, **f), dkl_path=torch.empty(n, **f),
                       ep_var_mean=torch.empty(n, **f), ep_var=torch.empty((n, self.obs_dim), **f))
            if self.disagreement:
                out.update(rew_var=torch.empty(n, **f), cost_var=torch.empty(n, **f))
            if self._predicts_term:
                out.update(term_pred=torch.empty(n, **f), term_votes=torch.empty(n, dtype=torch.uint8, device=self.device))
            if self.cost_loss == 'logistic':
                out.update(cost_logit=torch.empty(n, **f))
            if self.static_votes_on:
                out.update(static_term_votes=torch.zeros(n, dtype=torch.uint8, device=self.device),
                           static_cost_votes=torch.zeros(n, dtype=torch.uint8, device=self.device))
            self.step_device(o, a, inds, out, noise=xi, term_thr=thr)
        next_obs, r, terms = out["next_obs"], out["rew"][:, None], out["term"].bool()[:, None]
        c = out["cost"][:, None]
        if self._bool_cost:      # (not with a learned cost: the float32 prediction is the cost)
            c = c.bool()  # np.zeros_like(terms) is a bool array (models/fake_env.py:145-146)
        dkl_path, ep_var = out["dkl_path"], out["ep_var"]
        dkl_mean = dkl_path.mean()
        if was_np:
            next_obs, r, terms, c = (t.cpu().numpy() for t in (next_obs, r, terms, c))
            dkl_path, ep_var = dkl_path.cpu().numpy(), ep_var.cpu().numpy()
            dkl_mean = float(np.mean(dkl_path))
        if single:
            next_obs, r, c, terms = next_obs[0], r[0], c[0], terms[0]
        info = {"ensemble_dkl_mean": dkl_mean, "ensemble_dkl_path": dkl_path,
                "ensemble_ep_var": ep_var, "rew": r, "cost": c}
        if self.disagreement:
            rv, cv = out["rew_var"], out["cost_var"]
            if was_np:
                rv, cv = rv.cpu().numpy(), cv.cpu().numpy()
            info["ensemble_rew_var"], info["ensemble_cost_var"] = rv, cv
        if self._predicts_term:
            tp, tv = out["term_pred"], out["term_votes"]
            if self.term_loss == 'logistic':
                tp = torch.sigmoid(tp)      # float32, of the kernel's value
            if was_np:
                tp, tv = tp.cpu().numpy(), tv.cpu().numpy()
            info["term_pred"], info["term_votes"] = tp, tv
        if self.cost_loss == 'logistic':
            cl = out["cost_logit"]
            info["cost_logit"] = cl.cpu().numpy() if was_np else cl
        if self.static_votes_on:
            tv, cv = out["static_term_votes"], out["static_cost_votes"]      # (cost votes with a learned cost: zeros, nothing voted)
            if was_np:
                tv, cv = tv.cpu().numpy(), cv.cpu().numpy()
            info["static_term_votes"], info["static_cost_votes"] = tv, cv
        return next_obs, r, terms, info

    def replay(self, obs0, actions, next_obs, rewards, costs, terminals, lengths=None, model_inds=None, mode='open_loop',
               calibration=False, reliability=False, reliability_bins=15, reliability_terminals=None, votes=False,
               particles=0, particle_seed=None, noise_scale=None, particle_noise=None, particle_inds=None):
        """Open-loop model validation: replay B windows of up to H consecutive REAL steps through the model and hold its
        predictions against the recording, horizon by horizon (``cmbpo_replay_run``).

        obs0 [B, obs] is each window's first real observation; actions [H, B, act], next_obs [H, B, obs], rewards / costs /
        terminals [H, B] are the recorded steps, time-major (NumPy arrays or CUDA tensors; ``CPOBuffer.windows`` gathers
        them); lengths [B] in 1..H is the number of real steps of each window (None: H), the steps behind it are padding.
        ``mode='open_loop'`` feeds the model its own prediction, a window ends with its length, at a recorded terminal or at
        a predicted termination; ``mode='one_step'`` feeds it the real next observation (teacher-forced), a predicted
        termination is counted and does not end the window.  A window whose prediction is not finite counts in
        ``n_nonfinite`` at that horizon, ends, and enters no sum.

        model_inds: None -- one elite per window and step, drawn from a generator this method owns (nothing is consumed from
        ``np.random``, torch's generators or ``random_inds``' generator); an int -- every window through that member; an
        [H, B] array.

        A replay always measures the UNPENALISED means: it runs ``cmbpo_ens_forward`` and the plain ``cmbpo_fakeenv_post``,
        never the noise or disagreement entries, whatever ``disagreement`` / ``rew_pessimism`` / ``cost_pessimism`` are, and
        -- unless ``votes`` is given -- the ELITE's verdict of the static rules, whatever ``static_term_members`` /
        ``static_cost_members`` are.  With
        ``predicts_term`` the post step carries the head (``cmbpo_replay_run_term``): the predicted terminations, ``term_cm``
        among them, are ``rule_done or learned_done``.  With ``cost_loss='logistic'`` it carries the cost head
        (``cmbpo_replay_run_cost``): the predicted cost is the probability, so ``cost_cm``'s ``cost > 0.5`` is a decision rule
        on a probability and ``mse_cost`` is the Brier score of the column.

        Returns a dict of NumPy arrays, one row per horizon h = 0..H-1: ``n`` (windows compared), ``n_nonfinite``,
        ``mse_obs`` [H, obs], ``mse_rew``, ``mse_cost``, ``cost_cm`` / ``term_cm`` [H, 2, 2] indexed [real, predicted] (a
        real cost is ``cost > 0``, a predicted one ``cost > 0.5``), ``ep_var_mean`` and ``dkl_mean`` (the means of the step's
        ``ep_var_mean`` / ``dkl_path`` over the same windows), and the float64 sums they were divided from: ``se_obs``,
        ``se_rew``, ``se_cost``, ``sum_ep_var``, ``sum_dkl``.  A horizon with ``n == 0`` has NaN means and zero counts.

        ``calibration=True`` runs ``cmbpo_replay_run_calibrated`` instead: the same launches with one more kernel
        per step, the same table bit for bit, and under the key ``'calibration'`` the dict of
        ``cmbpo_amd.replay.calibration_table`` -- is the predictive VARIANCE the size of the real error, per horizon and per
        column (the observation columns, then the reward).  False is the call as it always was.

        ``reliability=True`` runs ``cmbpo_replay_run_reliab``: one more kernel per step again, every other table
        bit for bit, and under the key ``'reliability'`` the dict of ``cmbpo_amd.replay.reliability_table`` with one entry per
        logistic head, ``'cost'`` and / or ``'term'`` -- is the column a PROBABILITY: per horizon, in ``reliability_bins`` bins
        of equal probability width, what the column said against how often the event happened, with ECE, MCE, Brier score and log
        loss, for the elite member's logit and for the members' mean logit.  The cost column is measured with
        ``cost_logit_shift`` and WITHOUT the offset of ``set_cost_recalibration``, the termination column as it is.  With neither
        head logistic it raises ValueError: a Gaussian column is not a logit.  ``reliability_terminals`` [H, B]: the flags the
        termination column's table is held against where they are not ``terminals`` -- the head's training targets, which
        count a time-out as 0 (``CPOBuffer.term_targets``); the replay itself goes on ending windows at ``terminals``.  False is
        the call as it always was.

        ``votes=True`` (needs ``static_votes_on``) runs ``cmbpo_replay_run_votes``: the post step of every horizon is
        the rollouts' own, the vote kernel behind the post kernel under this environment's ``static_term_members`` /
        ``static_cost_members`` -- still without noise, disagreement or pessimism.  The predicted terminations and costs are the
        vote's verdicts: ``cost_cm`` / ``term_cm`` describe the rule in force, an ``open_loop`` window ends where the vote ends
        it, and under ``'mean'`` the predicted cost is ``votes / E``, so ``mse_cost`` is the Brier score of the share and
        ``cost_cm``'s ``cost > 0.5`` the strict majority.  Under the key ``'votes'``: the dict of ``cmbpo_amd.replay.votes_table``
        -- per horizon the histogram of the vote count against the recorded flag, the reliability of the share and the 2x2
        counts of the ``'any'`` and ``'majority'`` readings, for ``'cost'`` (not with ``predicts_cost``) and ``'term'``.
        ``votes='measure'`` runs the vote kernel under ``'elite'`` / ``'elite'`` whatever the environment's modes are: every
        other table is the call's without votes bit for bit, only the histogram is new.  ``reliability_terminals`` also serves
        as the flags the ``'term'`` histogram is held against.  False is the call as it always was.

        ``particles=S`` (S a power of two in 2..64) adds a SECOND pass of its own behind the replay above, which
        runs exactly as without it (every other key bit for bit): each window is replayed by S sampled particles
        (``cmbpo_replay_run_particles``: B S rows, the post step with transition noise, the termination and cost heads as above,
        no sampled terminations, disagreement, pessimism or votes), and under the key ``'particles'`` comes the dict of
        ``cmbpo_amd.replay.particles_table`` -- per horizon and column (the observation columns, then the reward) the rank
        histogram of the recorded value among the S particles, the fair CRPS, the particles' spread against the error of
        their mean, and the Brier scores of their termination share and mean cost.  Is the CLOUD of sampled branches as wide
        as the real spread after h compounded steps (``mode='open_loop'``), or after one (``mode='one_step'``: every particle
        restarts from the recording)?  A predicted termination does not end a particle; the particles of a window live and
        die together, with ``lengths`` and the recorded terminals.  The reward carries no transition noise by design (§3i):
        its histogram shows the spread over members and states only.
        The draws: the noise ``xi ~ N(0, 1)`` [H, B, S, obs] comes from a device generator of this call's own, the members
        [H, B, S] uniformly from ``elite_inds`` from a NumPy generator of its own, both seeded by ``particle_seed`` (None: the
        next seed of a stream this object keeps for nothing else) -- nothing is consumed from the replay's elite stream,
        ``np.random``, torch's global generators or a sampler's.  (The recipe, for a seed s: ``xi = torch.randn((H, B, S, obs),
        generator=g, dtype=torch.float32, device=...)`` with ``g = torch.Generator(device)`` after ``g.manual_seed(s)``; members
        ``elite_inds[np.random.default_rng(np.random.SeedSequence(s, spawn_key=(1,))).integers(0, len(elite_inds), (H, B, S))]``.)
        ``model_inds`` as an int sends every particle through that
        member too (the aleatoric spread alone); as an [H, B] array it names the plain pass's member per window and the
        particles still draw their own.  ``noise_scale`` [obs] multiplies the draws, one float32 rounding per element,
        as ``ModelSampler`` scales its own (``set_noise_scale``).  ``particle_noise`` [H, B, S, obs] / ``particle_inds``
        [H, B, S] supply the N(0, 1) draws (``noise_scale`` still applies) / the members directly.  Refused in words:
        S not a power of two in 2..64; ``particles`` together with ``votes=True`` (the particle pass runs no vote kernel, its
        table would describe another rule than the tables beside it; ``votes='measure'`` changes no verdict and is allowed);
        any of the four particle arguments without ``particles``.  0 is the call as it always was."""
        from .replay import ReplayBuffers, check_particles
        if votes not in (False, True, 'measure'):
            raise ValueError(f"replay: votes is False, True or 'measure', got {votes!r}")
        if particles:
            particles = check_particles(particles)
            if votes is True:
                raise ValueError("replay: particles together with votes=True is not supported: the particle pass runs no vote "
                                 "kernel, its table would describe another rule than the tables beside it (votes='measure' is "
                                 "allowed)")
        elif not (particle_seed is None and noise_scale is None and particle_noise is None and particle_inds is None):
            raise ValueError("replay: particle_seed / noise_scale / particle_noise / particle_inds need particles=S")
        if votes is True and not self.static_votes_on:
            raise ValueError("replay: votes=True needs the static votes on (static_votes=True or a static_*_members mode other "
                             "than 'elite'): there is no vote in force to replay under; votes='measure' only counts them")
        if reliability_terminals is not None and not (reliability or votes):
            raise ValueError("replay: reliability_terminals needs reliability=True: they are the flags of the reliability table")
        rel = dict(columns=self.reliability_columns(), bins=int(reliability_bins), terminals=reliability_terminals) \
            if reliability else None
        E = self._model.num_nets
        vot = None
        if votes:
            measure = votes == 'measure'
            vot = dict(done_members='elite' if measure else self.static_term_members,
                       cost_members='elite' if measure else self.static_cost_members, learned_cost=self._predicts_cost,
                       terminals=reliability_terminals)
        with torch.cuda.device(self.device):
            rb = ReplayBuffers(obs0, actions, next_obs, rewards, costs, terminals, lengths=lengths, mode=mode, ensemble=E,
                               out_dim=self.output_dim, device=self.device, calibration=bool(calibration), reliability=rel,
                               votes=vot)
            if (rb.obs_dim, rb.act_dim) != (self.obs_dim, self.act_dim):
                raise ValueError("replay: windows of width (%d, %d), the model's is (%d, %d)"
                                 % (rb.obs_dim, rb.act_dim, self.obs_dim, self.act_dim))
            H, B = rb.H, rb.B
            if model_inds is None:
                elites = np.asarray(self._model.elite_inds, dtype=np.int32)
                inds = elites[self._replay_rng.integers(0, len(elites), size=(H, B))]
            elif isinstance(model_inds, torch.Tensor):
                inds = model_inds.detach().cpu().numpy()
            elif np.ndim(model_inds) == 0:
                inds = np.full((H, B), int(model_inds))
            else:
                inds = np.asarray(model_inds)
            if inds.shape != (H, B) or inds.min() < 0 or inds.max() >= E:
                raise ValueError("replay: model_inds must be an int or an [%d, %d] array of members in 0..%d" % (H, B, E - 1))
            elite = torch.from_numpy(np.ascontiguousarray(inds, dtype=np.int32)).to(self.device)
            th, ch = self.term_head_struct(), self.cost_head_struct()
            if votes:
                rb.run_votes(self._model.mlp.handle, self._task_id, E, elite, term_head=th, cost_head=ch,
                             calibration=bool(calibration), reliability=bool(reliability))
                tab = rb.table()
                if calibration:
                    tab['calibration'] = rb.calibration_table()
                tab['votes'] = rb.votes_table()
            elif calibration:
                rb.run_calibrated(self._model.mlp.handle, self._task_id, E, elite, term_head=th, cost_head=ch)
                tab = rb.table()
                tab['calibration'] = rb.calibration_table()
            else:
                rb.run(self._model.mlp.handle, self._task_id, E, elite, term_head=th, cost_head=ch)
                tab = rb.table()
            if reliability:
                tab['reliability'] = rb.reliability_table()
            if particles:
                tab['particles'] = self._replay_particles(particles, obs0, actions, next_obs, rewards, costs, terminals,
                                                         lengths=lengths, model_inds=model_inds, mode=mode,
                                                         particle_seed=particle_seed, noise_scale=noise_scale,
                                                         particle_noise=particle_noise, particle_inds=particle_inds)
            return tab

    def _replay_particles(self, S, obs0, actions, next_obs, rewards, costs, terminals, lengths=None, model_inds=None,
                          mode='open_loop', particle_seed=None, noise_scale=None, particle_noise=None, particle_inds=None):
        """The second pass of ``replay(particles=S)`` alone -- its own buffers, its own draws, ``cmbpo_replay_run_particles`` --,
        with that call's arguments; returns the dict of ``cmbpo_amd.replay.particles_table``.  Internal: ``replay`` (which has
        refused ``votes=True`` by then) and the trainer (which refuses ``m_validate_votes`` beside it) call it.  ``model_inds``
        counts only as an int -- every particle through that member --: an [H, B] array names one member per window, the
        particles draw their own."""
        from .replay import ParticleBuffers, check_particles
        S, seed, noise, inds = check_particles(S), particle_seed, particle_noise, particle_inds
        E, D = self._model.num_nets, self.obs_dim
        H, B = tuple(actions.shape[:2]) if hasattr(actions, "shape") else np.shape(actions)[:2]
        widths = (int(np.shape(next_obs)[-1]), int(np.shape(actions)[-1]))
        if widths != (self.obs_dim, self.act_dim):
            raise ValueError("replay: windows of width (%d, %d), the model's is (%d, %d)" % (widths + (self.obs_dim, self.act_dim)))
        if seed is None:
            seed = int(self._particle_seeds.integers(0, 2 ** 62))
        seed = int(seed)
        if noise is None:
            gen = torch.Generator(device=self.device)
            gen.manual_seed(seed)
            xi = torch.randn((H, B, S, D), generator=gen, dtype=torch.float32, device=self.device)
        else:
            xi = torch.as_tensor(noise, dtype=torch.float32).to(self.device).clone()
            if tuple(xi.shape) != (H, B, S, D):
                raise ValueError("replay: particle_noise must be [%d, %d, %d, %d], got %s" % (H, B, S, D, tuple(xi.shape)))
        if noise_scale is not None:
            sc = torch.as_tensor(np.asarray(noise_scale, dtype=np.float32).reshape(-1))
            if tuple(sc.shape) != (D,) or not bool(torch.isfinite(sc).all()) or not bool((sc > 0).all()):
                raise ValueError("replay: noise_scale must be %d finite positive factors, one per observation column" % D)
            xi.mul_(sc.to(self.device))
        if inds is not None:
            m = inds.detach().cpu().numpy() if isinstance(inds, torch.Tensor) else np.asarray(inds)
        elif model_inds is not None and not isinstance(model_inds, torch.Tensor) and np.ndim(model_inds) == 0:
            m = np.full((H, B, S), int(model_inds))
        else:
            elites = np.asarray(self._model.elite_inds, dtype=np.int32)
            rng = np.random.default_rng(np.random.SeedSequence(seed, spawn_key=(1,)))
            m = elites[rng.integers(0, len(elites), size=(H, B, S))]
        if m.shape != (H, B, S) or m.min() < 0 or m.max() >= E:
            raise ValueError("replay: particle_inds must be an [%d, %d, %d] array of members in 0..%d" % (H, B, S, E - 1))
        elite = torch.from_numpy(np.ascontiguousarray(m.reshape(H, B * S), dtype=np.int32)).to(self.device)
        with torch.cuda.device(self.device):
            pb = ParticleBuffers(S, obs0, actions, next_obs, rewards, costs, terminals, lengths=lengths, mode=mode, ensemble=E,
                                 out_dim=self.output_dim, noise=xi, device=self.device)
            pb.run(self._model.mlp.handle, self._task_id, E, elite, term_head=self.term_head_struct(),
                   cost_head=self.cost_head_struct())
            return pb.table()

    def close(self):
        pass
