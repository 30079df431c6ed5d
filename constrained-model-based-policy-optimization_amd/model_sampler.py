"""ModelSampler -- host-side mirror of ``samplers/model_sampler.py:13-444`` over device-resident state.

Same constructor / ``initialize(env, policy, pool)`` / ``reset(observations)`` / ``sample(max_samples)``
/ ``finish_all_paths()`` / ``compute_dynamics_dkl`` / ``set_rollout_dkl`` / ``set_max_path_length`` and the
``dyn_dkl`` / ``_total_samples`` attributes the trainer reads (``algorithms/cmbpo.py:197-201,251-266``).

One ``sample()`` = one imagined step of every alive branch, entirely on the GPU:

    policy forward (HIP)  ->  ensemble forward + FakeEnv post (HIP)  ->  decide  ->  finish(PRE)
    ->  store  ->  critics on next_obs (HIP)  ->  finish(POST)  ->  compact

Event order, bootstraps and the budget rule follow ``model_sampler.py:239-375`` (see the kernels in
``csrc/rollout_state.hip``).  Two restructurings that do not change results:
  * V / VC of the *next* observation are evaluated once after the store: they bootstrap the horizon /
    terminal finishes of this step (``:350-367``) and ARE the ``v_t`` / ``vc_t`` of the next step (the critics
    are deterministic), so the extra ``get_v`` / ``get_vc`` calls of ``_finish_paths`` (``:401-407``) vanish;
  * branches never move: an ordered alive list replaces the boolean-mask compaction (``:300-311``).

``ModelSampler(stochastic=True)`` samples every imagined transition from the elite member's N(mean, var) (``xi`` draws of
the sampler's generator, ``cmbpo_fakeenv_post_noise``); off, the draws and the results are what they were without it.

``reset()`` takes the disagreement switch and the pessimism coefficients of its ``env`` (``FakeEnv(disagreement=...,
rew_pessimism=..., cost_pessimism=...)``) and hands them to the pool: every step then measures the ensemble's disagreement on
reward and cost, stores the penalised values and adds the variances of the stored rows to two more accumulators.

``reset()`` likewise takes the learned termination head of its ``env`` (``FakeEnv(predicts_term=True, term_threshold=...,
term_members=...)``): every step then ends a branch where the rule or the model's termination column says so, on the one-call
step, the native loop and the sharded per-step path alike; ``pool.t['term_pred_t']`` / ``['term_votes_t']`` hold the step's values.

``reset()`` also takes the reading of the learned-cost column (``FakeEnv(cost_loss='logistic', cost_logit_shift=...)``, DESIGN
§3w): every step then stores the cost as a probability, and ``pool.t['cost_logit_t']`` holds the step's raw logits.

``reset()`` also takes the votes on the task's static rules (``FakeEnv(static_term_members=..., static_cost_members=...,
static_votes=...)``): every step then evaluates the rules on every member's next state, ends a branch / charges a
step by the vote, and ``pool.t['rule_done_votes_t']`` / ``['rule_cost_votes_t']`` hold the step's votes; no new random numbers.

``ModelSampler(term_sampling=True)`` SAMPLES the learned termination (needs an ``env`` with ``predicts_term``): a
branch whose termination column says p ends with probability p instead of where p is above the head's threshold.  The sampler
draws u = 1 - rand() in (0, 1] per branch and step from a generator of its own (seeded ``seed + 1``), a whole chunk ``[K, B]``
at a time with the chunk's K, turns them into thresholds (``utils.term_thresholds`` with the environment's ``term_loss``) and
attaches them beside the rollout struct (``cmbpo_rollout_term_draws_attach``) for the one-call step and the native loop.  The
action noise, the elite picks and the transition noise are the numbers they were, at the same chunk boundaries; off (the
default) no generator is made and no call is added.  Sharded samplers refuse it: per-rank streams are not defined here.
``set_term_logit_offset(b)`` (a logistic head only) adds a measured recalibration offset to every chunk of thresholds
drawn from then on: the hazard becomes ``sigma(z - b)``.

``sample()`` returns ``(next_obs, reward, terminal, info)`` like the reference, but as slot-indexed CUDA
tensors (the trainer only reads ``info['alive_ratio']``, ``algorithms/cmbpo.py:254-263``).
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .dist import budget_plan

EPS = 1e-8  # utilities/utils.py:19


class ModelSampler:
    def __init__(self, max_path_length, batch_size=1000, rollout_mode=False, logger=None, seed=0,
                 comm=None, stochastic=False, term_sampling=False):
        self._max_path_length = int(max_path_length)
        self.batch_size = int(batch_size)
        self.rollout_mode = rollout_mode
        self.logger = logger
        self.comm = comm
        self.stochastic = bool(stochastic)     # transitions drawn from N(mean, var) instead of the elite member's mean
        self.term_sampling = bool(term_sampling)    # learned terminations drawn from the head's probability, not thresholded
        if self.term_sampling and comm is not None and comm.world > 1:
            raise NotImplementedError("term_sampling=True on a sharded sampler (world size %d): per-rank streams of termination "
                                      "draws are not defined here" % comm.world)
        self._term_gen = None                       # the generator of the termination draws (term_sampling only)
        self._thr_attached = False                  # thresholds are attached beside the pool's struct
        self.dkl_lim = float("inf")
        self.env = self.policy = self.pool = None
        self._n_episodes = 0
        self._seed = int(seed)
        self._gen = None
        self._host = dict(total_samples=0.0, total_dkl=0.0)
        self._calib_total_dkl = 0.0
        self._calib_total_samples = 0.0
        self._diag = None
        self._noise_scale = None                    # [obs] factors on the xi draws (host tensor), see set_noise_scale()
        self._term_logit_offset = None              # added to the termination thresholds, see set_term_logit_offset()
        self.global_alive = 1                     # alive branches over all shards (sharded samplers), see reset()
        self._global_total_samples = 0.0

    # -- wiring -----------------------------------------------------------------------------------
    def initialize(self, env, policy, pool):
        if self.term_sampling and not getattr(env, "predicts_term", False):
            raise ValueError("term_sampling=True needs an environment with predicts_term=True: the model has no termination "
                             "column to sample from")
        if self._term_logit_offset is not None:
            self._check_term_logit_offset(env)
        self.env, self.policy, self.pool = env, policy, pool
        self.device = pool.device
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(self._seed)
        self._term_gen = None                       # (made with the first chunk of termination draws)
        # everything bound to the device starts over
        self._elites = self._elites_host = None     # the model's elite indices on the device / as last uploaded
        self._draws = None                          # chunk of draws, see _draw_chunk()
        self._scratch = self._handles = None        # see _prepare_call()
        self._run_host = self._run_out = None       # sample_many(): pinned counters of a call's steps, its three out-words

    def set_policy(self, policy):
        self.policy = policy
        self._handles = None

    def set_logger(self, logger):
        self.logger = logger

    def terminate(self):
        self.env.close()

    def set_rollout_dkl(self, dkl):
        self.dkl_lim = float(dkl)

    def set_max_path_length(self, path_length):
        self._max_path_length = int(path_length)

    @property
    def noise_scale(self):
        """The factors of ``set_noise_scale`` as a float32 NumPy array, or None."""
        return None if self._noise_scale is None else self._noise_scale.numpy().copy()

    def set_noise_scale(self, scale):
        """Calibrated transition noise: a `stochastic` sampler multiplies every xi chunk it draws from now on by
        ``scale`` [obs] (array or tensor; one float32 rounding per element), which is the elite member's std scaled per
        column.  An explicit ``xi=`` argument of ``sample`` is never scaled.  A scale that differs from the one in force drops
        the rest of the chunk of draws in hand (the next step draws a new one under the new scale); the same scale again drops
        nothing.  None (the default): the draws as they come, exactly the generator calls of a sampler that never heard of this."""
        if scale is None:
            if self._noise_scale is not None:
                self._noise_scale, self._draws = None, None
            return
        if not self.stochastic:
            raise ValueError("set_noise_scale: this sampler was built with stochastic=False, it draws no transition noise to scale")
        s = torch.as_tensor(np.asarray(scale.detach().cpu() if isinstance(scale, torch.Tensor) else scale, dtype=np.float32))
        if s.dim() != 1 or (self.pool is not None and s.shape[0] != self.pool.obs_dim):
            raise ValueError("set_noise_scale: one factor per observation column expected, got shape %s" % (tuple(s.shape),))
        if not bool(torch.isfinite(s).all()) or not bool((s > 0).all()):
            raise ValueError("set_noise_scale: the factors must be finite and positive")
        if self._noise_scale is None or not torch.equal(self._noise_scale, s):
            self._noise_scale, self._draws = s, None

    @property
    def term_logit_offset(self):
        """The offset of ``set_term_logit_offset`` as a float, or None."""
        return self._term_logit_offset

    def _check_term_logit_offset(self, env):
        if not self.term_sampling:
            raise ValueError("set_term_logit_offset: this sampler was built with term_sampling=False, it draws no termination "
                             "thresholds to shift")
        if env is not None and getattr(env, "term_loss", "gaussian") != 'logistic':
            raise ValueError("set_term_logit_offset needs an environment with term_loss='logistic': a Gaussian termination column "
                             "is not a logit, an offset in logit space means nothing to it")

    def set_term_logit_offset(self, offset):
        """Recalibrated termination hazard: a `term_sampling` sampler under a logistic head adds ``offset`` (b of
        ``replay.logit_offset``) to every chunk of termination thresholds it draws from now on -- one float32 rounding per element,
        +inf stays +inf --, since ``z - b > logit(u)`` is ``z > logit(u) + b``.  Explicit ``term_draws=`` of ``sample`` are never
        shifted.  An offset that differs from the one in force drops the rest of the chunk of draws in hand; the same offset again
        drops nothing.  None or 0.0 (the default): the thresholds as they come, exactly the calls of a sampler that never heard
        of this."""
        b = None if offset is None else float(offset)
        if b is not None and not np.isfinite(b):
            raise ValueError("set_term_logit_offset: the offset must be a finite number, got %r" % (offset,))
        if b == 0.0:
            b = None
        if b is not None:
            self._check_term_logit_offset(self.env)
        if b != self._term_logit_offset:
            self._term_logit_offset, self._draws = b, None

    def batch_ready(self):
        return self.pool.size >= self.pool.max_size

    # -- accumulators ---------------------------------------------------------------------------------
    def _read_scalars(self):
        isc, dsc = self.pool.read_scalars()
        self._dsc = dsc
        return isc, dsc

    @property
    def _total_samples(self):
        return self._host["total_samples"]

    @property
    def global_total_samples(self):
        """`_total_samples` summed over the shards (== `_total_samples` on one GPU): what a stop rule on the job's sample
        count has to read (algorithms/cmbpo.py:356-357)."""
        if self.comm is not None and self.comm.world > 1:
            return self._global_total_samples
        return self._host["total_samples"]

    @property
    def _total_dkl(self):
        return self._host["total_dkl"]

    @property
    def dyn_dkl(self):
        """model_sampler.py:175-177."""
        return self._host["total_dkl"] / (self._host["total_samples"] + EPS)

    def get_diagnostics(self):
        """model_sampler.py:89-133 (same keys; variance terms the reference never fills stay 0).

        With the environment's disagreement switch on, ``rew_var_perstep`` / ``cost_var_perstep`` are the ensemble's variance
        on the reward / cost column averaged over the stored samples (the reference declares ``_total_rew_var`` /
        ``_total_cost_var`` and never fills them), and with a pessimism coefficient > 0 ``rew_rate`` / ``cost_rate`` are rates
        of the PENALISED values: the pool stores what the constrained update will see.  ``ens_mean_var`` stays 0.

        With the pool's critic disagreement on (``ModelBuffer.set_value_disagreement``), ``v_var_perstep`` / ``vc_var_perstep``
        are the variance over the critic members of V / VC at the stored samples' observations, averaged over the stored
        samples (0.0 when off), and with a coefficient > 0 ``v_mean`` / ``cv_mean`` are means of the PENALISED values
        ``V - kappa_v sigma_v`` / ``VC + kappa_vc sigma_vc``, again what the pool stores."""
        _, d = self._read_scalars()
        L = _lib
        tot = d[L.D_TOTAL_SAMPLES]
        on = bool(getattr(self.pool, "disagreement", False))
        von = bool(getattr(self.pool, "value_disagreement", False))
        diagnostics = OrderedDict({"pool-size": self.pool.size})
        diagnostics.update({
            "msampler/samples_added": tot,
            "msampler/rollout_H_max": self._n_episodes,
            "msampler/rollout_H_mean": tot / (self.batch_size + EPS),
            "msampler/rew_var_perstep": d[L.D_TOTAL_REW_VAR] / (tot + EPS) if on else 0.0,
            "msampler/cost_var_perstep": d[L.D_TOTAL_COST_VAR] / (tot + EPS) if on else 0.0,
            "msampler/dyn_var_perstep": d[L.D_TOTAL_DYN_EP_VAR] / (tot + EPS),
            "msampler/cost_rate": d[L.D_SUM_PATH_COST] / (tot + EPS),
            "msampler/rew_rate": d[L.D_SUM_PATH_RET] / (tot + EPS),
            "msampler/v_mean": d[L.D_TOTAL_VS] / (tot + EPS),
            "msampler/cv_mean": d[L.D_TOTAL_CVS] / (tot + EPS),
            "msampler/v_var_perstep": d[L.D_TOTAL_V_VAR] / (tot + EPS) if von else 0.0,
            "msampler/vc_var_perstep": d[L.D_TOTAL_VC_VAR] / (tot + EPS) if von else 0.0,
            "msampler/ens_DKL": d[L.D_TOTAL_DKL] / (tot + EPS),
            "msampler/ens_mean_var": 0.0,
            "msampler/max_path_return": d[L.D_MAX_PATH_RETURN],
            "msampler/max_dkl": d[L.D_MAX_DKL],
        })
        return diagnostics

    # -- rollout -------------------------------------------------------------------------------------
    def _critics(self, obs_key, v_key, vc_key, n):
        t = self.pool.t
        idx = t["alive_idx"]
        lib, stream = _lib.lib(), _lib.current_stream()
        v, vc = self.policy.v.mlp.handle, self.policy.vc.mlp.handle
        pool = self.pool
        if getattr(pool, "value_disagreement", False):
            # critic disagreement: penalised values and the members' variances, into the arrays attached beside the struct (the
            # next store reads them; critics the one-launch kernels do not take are refused by the entry)
            _lib.check(lib.cmbpo_critic_pair_predict_var(v, vc, t[obs_key].data_ptr(), pool.obs_dim, idx.data_ptr(), None, n,
                                                         pool.v_pessimism, pool.vc_pessimism, t[v_key].data_ptr(),
                                                         t[vc_key].data_ptr(), t["v_var"].data_ptr(), t["vc_var"].data_ptr(), stream),
                       "cmbpo_critic_pair_predict_var")
            return
        if lib.cmbpo_critic_pair_supported(v, vc):       # both critics in one launch
            _lib.check(lib.cmbpo_critic_pair_predict(v, vc, t[obs_key].data_ptr(), self.pool.obs_dim, idx.data_ptr(), None, n,
                                                     t[v_key].data_ptr(), t[vc_key].data_ptr(), stream),
                       "cmbpo_critic_pair_predict")
            return
        for net, key in ((self.policy.v, v_key), (self.policy.vc, vc_key)):
            _lib.check(lib.cmbpo_ens_predict_mean(net.mlp.handle, t[obs_key].data_ptr(), self.pool.obs_dim,
                                                  idx.data_ptr(), None, n, t[key].data_ptr(), stream),
                       "cmbpo_ens_predict_mean")

    def reset(self, observations, fill=None, batch_size=None):
        """model_sampler.py:203-237: start all branches from `observations` [B, obs].  With `observations` None,
        `fill(cur_obs)` writes the `batch_size` start states into the rollout state's own [B, obs] device tensor
        (CPOBuffer.sample_start_states: no staging copy)."""
        if observations is None:
            if fill is None or batch_size is None:
                raise ValueError("reset(None) needs fill= and batch_size=")
            self.batch_size = int(batch_size)
        else:
            self.batch_size = int(observations.shape[0])
        self.policy.reset()
        pool = self.pool
        with torch.cuda.device(self.device):
            pool.reset(self.batch_size)
            # the environment's disagreement switch and pessimism coefficients (nothing is stored here; arrays allocated by
            # the call start at zero, arrays that were attached have just been zeroed)
            pool.set_disagreement(getattr(self.env, "disagreement", False), getattr(self.env, "rew_pessimism", 0.0),
                                  getattr(self.env, "cost_pessimism", 0.0))
            # ... and its learned termination head
            # (the number the kernels compare with: under term_loss='logistic' the logit of the threshold, and the pool's
            # term_pred_t then carries the logit)
            pool.set_term_head(getattr(self.env, "predicts_term", False),
                               getattr(self.env, "term_kernel_threshold", getattr(self.env, "term_threshold", 0.5)),
                               getattr(self.env, "term_members", "elite"))
            # ... and the reading of its learned-cost column (a shift changed between two fits is picked up here)
            # (with a recalibration offset: the float32 sum of the two, FakeEnv.cost_kernel_shift)
            pool.set_cost_head(getattr(self.env, "cost_loss", "gaussian"),
                               getattr(self.env, "cost_kernel_shift", getattr(self.env, "cost_logit_shift", 0.0)))
            # ... and whose verdict of the task's static rules counts (the vote kernel behind the post kernel; off: nothing attached)
            pool.set_rule_votes(getattr(self.env, "static_votes_on", False), getattr(self.env, "static_term_members", "elite"),
                                getattr(self.env, "static_cost_members", "elite"),
                                not getattr(self.env, "_predicts_cost", False))
            if observations is None:
                fill(pool.t["cur_obs"])
            else:
                obs = observations if isinstance(observations, torch.Tensor) else \
                    torch.from_numpy(np.ascontiguousarray(observations, dtype=np.float32))
                pool.t["cur_obs"].copy_(obs.to(self.device, torch.float32))
            pool.rs.max_path_length = self._max_path_length
            pool.rs.uncertainty_mode = 1 if self.rollout_mode == "uncertainty" else 0
            pool.rs.dkl_lim = float(self.dkl_lim)
            if self.comm is not None:
                pool.rs.rank, pool.rs.world = self.comm.rank, self.comm.world
            # critics at the start states: v_t / vc_t of the first step
            self._critics("cur_obs", "v_t", "vc_t", self.batch_size)
        self._n_episodes = 0
        self.global_alive = 1
        self._global_total_samples = 0.0
        self.n_budget_terminated = 0     # branches the `max_samples` rule ended early (model_sampler.py:282-287), this shard
        self._host = dict(total_samples=0.0, total_dkl=0.0)
        elites = np.asarray(self.env._model.elite_inds, dtype=np.int32)
        if self._elites_host is None or not np.array_equal(self._elites_host, elites):
            # (uploaded again only when the elites changed: a host-to-device copy per reset otherwise)
            self._elites_host = elites.copy()
            self._elites = torch.as_tensor(elites, device=self.device)
        self._draws = None
        self._handles = None

    def _scatter(self, compact, idx, width=None, dtype=torch.float32):
        """Test hook: a draw given in the reference's compact (alive-only) order -> slot order."""
        B = self.batch_size
        shape = (B,) if width is None else (B, width)
        full = torch.zeros(shape, dtype=dtype, device=self.device)
        full[idx.long()] = torch.as_tensor(np.ascontiguousarray(compact), device=self.device).to(dtype)
        return full

    def _attach_thresholds(self, ptr, stride):
        """The thresholds of the next native call: step j reads ptr + 4 * j * stride (None: back to the head's threshold)."""
        if ptr is None and not self._thr_attached:
            return
        _lib.check(_lib.lib().cmbpo_rollout_term_draws_attach(C.byref(self.pool.rs), ptr, stride),
                   "cmbpo_rollout_term_draws_attach")
        self._thr_attached = ptr is not None

    def sample(self, max_samples=None, eps=None, model_inds=None, xi=None, term_draws=None):
        """One imagined step of every alive branch (model_sampler.py:239-375).

        eps / model_inds (optional, compact alive-only order like the reference's arrays) inject the
        N(0,1) action noise (ac_network.py:109) and the per-branch elite draw (fake_env.py:174-178);
        xi ([n, obs_dim], the same order) the transition noise: next_obs = mean + std * xi + obs.  Without it a
        `stochastic` sampler draws its own, any other sampler steps to the elite member's mean.  term_draws ([n] uniform
        numbers in (0, 1], the same order) sample the learned termination of this step; without them a `term_sampling`
        sampler draws its own, any other sampler keeps the head's threshold.
        """
        if term_draws is not None and not getattr(self.env, "predicts_term", False):
            raise ValueError("term_draws needs an environment with predicts_term=True: the model has no termination column to "
                             "sample from")
        pool = self.pool
        assert pool.has_room                       # pool full! empty before sampling.
        sharded = self.comm is not None and self.comm.world > 1
        if sharded and pool.n_alive == 0:
            # this shard has nothing left but the others may: keep the collectives of the step matched
            return self._idle_step(max_samples)
        assert pool.n_alive > 0                    # reset before sampling !
        if torch.cuda.current_device() != self.device.index:
            with torch.cuda.device(self.device):
                return self._step(sharded, max_samples, eps, model_inds, xi, term_draws)
        return self._step(sharded, max_samples, eps, model_inds, xi, term_draws)

    def _step(self, sharded, max_samples, eps, model_inds, xi, term_draws=None):
        """sample() on the sampler's device.  On one rank with the sampler's own draws the whole step is ONE C call
        (cmbpo_rollout_step) plus the read of the step's counters -- at the shipped configurations' 1e3 - 1e4 branches a step
        is ~100 us of kernels, so the host side of that case is kept to pointer arithmetic."""
        pool, env, pol = self.pool, self.env, self.policy
        self._n_episodes += 1
        t, rs = pool.t, pool.rs
        n = pool.n_alive
        h = self._prepare_call(max_samples)
        exchange = sharded and rs.max_samples != 0      # the reference's `if max_samples:` (negative budgets count)
        separate = exchange or env.kernel_events is not None
        if eps is None or model_inds is None or (xi is None and self.stochastic) or (term_draws is None and self.term_sampling):
            ck, k, eps_ptr, inds_ptr, xi_ptr = self._next_draws()
            ck[0] = k + 1
        # sampled terminations: this step's thresholds, slot indexed (injected draws are scattered like the others)
        thr_t = None
        if term_draws is not None:
            from .utils import term_thresholds
            u = torch.as_tensor(np.ascontiguousarray(term_draws)) if not isinstance(term_draws, torch.Tensor) else term_draws
            if tuple(u.shape) != (n,):
                raise ValueError("term_draws must have shape [%d] (one draw per alive branch), got %s" % (n, tuple(u.shape)))
            thr = term_thresholds(u, getattr(env, "term_loss", "gaussian"))
            # (dead slots: +inf, which never hits)
            thr_t = torch.full((self.batch_size,), float("inf"), dtype=torch.float32, device=self.device)
            thr_t[t["alive_idx"][:n].long()] = thr.to(self.device)
        elif self.term_sampling:
            thr_t = ck[4][k]
        if separate or eps is not None or model_inds is not None or xi is not None:
            # injected draws are scattered to slot order; the separate entries below take tensors
            idx = t["alive_idx"][:n]
            eps_t = ck[1][k] if eps is None else self._scatter(eps, idx, pool.act_dim)
            inds_t = ck[2][k] if model_inds is None else self._scatter(model_inds, idx, None, torch.int32)
            if xi is not None:
                xi_t = self._scatter(xi, idx, pool.obs_dim)
            else:
                xi_t = ck[3][k] if self.stochastic else None
            eps_ptr, inds_ptr, xi_ptr = eps_t.data_ptr(), inds_t.data_ptr(), None if xi_t is None else xi_t.data_ptr()
        rs.xi = xi_ptr
        rc = 0
        if not separate:
            self._attach_thresholds(None if thr_t is None else thr_t.data_ptr(), 0)
            # the whole step in one call: at small rollout batches a step is bound by host latency
            rc = _lib.lib().cmbpo_rollout_step(C.byref(rs), n, h[0], h[1], h[2], h[3], env._task_id, env._model.num_nets,
                                               eps_ptr, inds_ptr, h[4], h[5], _lib.current_stream())
            if rc != 1:         # (1, small batch: finish(POST) and the compaction ran inside the call)
                _lib.check(rc, "cmbpo_rollout_step")
        else:
            idx = t["alive_idx"]
            # policy: pi, logp, mu, log_std at the current observations
            pol.actor.forward_device(t["cur_obs"], eps_t,
                                     dict(pi=t["act_t"], logp_pi=t["logp_t"], mu=t["mu_t"], log_std=t["ls_t"]),
                                     row_idx=idx, n_rows=n)
            # dynamics ensemble + FakeEnv post-processing
            outs = dict(next_obs=t["next_obs"], rew=t["rew_t"], term=t["term_t"], cost=t["cost_t"],
                        dkl_path=t["dkl_t"], ep_var_mean=t["epv_t"])
            if pool.disagreement:       # (the arrays attached beside the struct: the store below reads them)
                outs.update(rew_var=t["rew_var_t"], cost_var=t["cost_var_t"])
            if pool.term_head is not None:
                outs.update(term_pred=t["term_pred_t"], term_votes=t["term_votes_t"])
            if pool.cost_head is not None:
                outs.update(cost_logit=t["cost_logit_t"])
            if pool.rule_votes is not None:
                outs.update(static_term_votes=t["rule_done_votes_t"], static_cost_votes=t["rule_cost_votes_t"])
            env.step_device(t["cur_obs"], t["act_t"], inds_t, outs,
                            row_idx=idx, n_rows=n, scratch=self._scratch, noise=xi_t,
                            **({} if thr_t is None else dict(term_thr=thr_t)))
            if exchange:
                # budget rule across shards: gather {n_alive, n_unc, total}, rank the survivors globally
                pool._call("cmbpo_rollout_count")
                rows = self.comm.all_gather_i32(t["iscal"][8:12]).cpu().numpy()
                excess, rank_off = budget_plan(rows, self.comm.rank, rs.max_samples)
                rs.use_host_budget, rs.host_excess, rs.host_rank_off = 1, int(excess), int(rank_off)
            pool._call("cmbpo_rollout_decide")
            pool._call("cmbpo_rollout_finish", 0)
            pool._call("cmbpo_rollout_store")
            self._critics("next_obs", "v_n", "vc_n", n)
            pool._call("cmbpo_rollout_finish", 1)
        isc, dsc = self._read_scalars()         # the host sync of the step: what finished / was stored + the accumulators
        info = self._after_step(rc == 1, isc, dsc, n, sharded)
        # after the swap the step's next_obs is the new cur_obs
        return t["cur_obs"], t["rew_t"], t["term_t"], info

    def _draw_chunk(self):
        """Action noise and elite picks for several steps at a time (three torch launches per chunk instead of per step:
        at small rollout batches a step is a chain of launch latencies).  Returns the chunk list
        [next step, eps [K, B, A], elite indices [K, B], xi [K, B, obs] or None, termination thresholds [K, B] or None].  A
        `stochastic` sampler draws the transition noise after the elite picks, with K such that the chunk's bytes stay under
        the same cap; any other sampler makes exactly the generator calls it always made.  A `term_sampling` sampler draws the
        chunk's termination draws from a generator of its own: K and the other streams are what they are without it."""
        B, A = self.batch_size, self.pool.act_dim
        step_bytes = max(B * (A + (self.pool.obs_dim if self.stochastic else 0)) * 4, 1)
        K = max(1, min(40, max(2 ** 23 // step_bytes, min(8, 2 ** 28 // step_bytes))))    # a whole rollout at small batches
        e_ck = torch.randn((K, B, A), generator=self._gen, dtype=torch.float32, device=self.device)
        d_ck = torch.randint(0, len(self._elites), (K, B), generator=self._gen, device=self.device)
        x_ck = None
        if self.stochastic:
            x_ck = torch.randn((K, B, self.pool.obs_dim), generator=self._gen, dtype=torch.float32, device=self.device)
            if self._noise_scale is not None:
                x_ck.mul_(self._noise_scale.to(self.device))
        t_ck = None
        if self.term_sampling:
            from .utils import term_thresholds
            if self._term_gen is None:
                self._term_gen = torch.Generator(device=self.device)
                self._term_gen.manual_seed(self._seed + 1)
            # u = 1 - rand() in (0, 1]: a probability of exactly 0 never ends a branch
            u_ck = 1.0 - torch.rand((K, B), generator=self._term_gen, dtype=torch.float32, device=self.device)
            t_ck = term_thresholds(u_ck, getattr(self.env, "term_loss", "gaussian"), check=False).contiguous()
            if self._term_logit_offset is not None:
                t_ck.add_(torch.tensor(self._term_logit_offset, dtype=torch.float32, device=self.device))
        self._draws = [0, e_ck, self._elites[d_ck], x_ck, t_ck]
        return self._draws

    def _next_draws(self):
        """The draw chunk, its first unused step k and the device addresses of that step's eps, elite indices and xi (None without
        transition noise).  The chunk is drawn again when it is used up or was drawn for another batch size or another
        `stochastic` / `term_sampling`.  The caller advances chunk[0] by the steps it takes; step k's thresholds are chunk[4][k]."""
        ck = self._draws
        B = self.batch_size
        if ck is None or ck[0] >= ck[1].shape[0] or ck[1].shape[1] != B or (ck[3] is None) == self.stochastic \
                or (ck[4] is None) == self.term_sampling:
            ck = self._draw_chunk()
        k = ck[0]
        return (ck, k, ck[1].data_ptr() + k * B * self.pool.act_dim * 4, ck[2].data_ptr() + k * B * ck[2].element_size(),
                ck[3].data_ptr() + k * B * self.pool.obs_dim * 4 if ck[3] is not None else None)

    def _prepare_call(self, max_samples):
        """What every native step call needs first: the ensemble's scratch, the handle tuple (actor, model, v, vc, scratch mean,
        scratch var; rebuilt after reset(), set_policy() and a new scratch) and the step's limits in the struct."""
        env, pol, rs = self.env, self.policy, self.pool.rs
        if self._scratch is None or self._scratch[0].shape[1] != self.batch_size:
            shape = (env._model.num_nets, self.batch_size, env.output_dim)
            self._scratch = (torch.empty(shape, dtype=torch.float32, device=self.device),
                             torch.empty(shape, dtype=torch.float32, device=self.device))
            self._handles = None
        if self._handles is None:
            self._handles = (pol.actor.mlp.handle, env._model.mlp.handle, pol.v.mlp.handle, pol.vc.mlp.handle,
                             self._scratch[0].data_ptr(), self._scratch[1].data_ptr())
        rs.max_samples = int(max_samples) if max_samples else 0
        rs.dkl_lim = float(self.dkl_lim)
        rs.max_path_length = self._max_path_length
        rs.use_host_budget = 0
        return self._handles

    def _after_step(self, compacted, isc, dsc, n, sharded):
        """The host's part of a step of `n` alive rows, from the counters it left: the alive list (`compacted`: already rebuilt
        inside the call), the cur / next arrays, the column, the totals.  Returns the step's info."""
        pool = self.pool
        self.n_budget_terminated += int(isc[_lib.I_N_FIN_PRE]) - int(isc[_lib.I_N_UNC])
        if compacted:
            pool.swap("alive_idx", "alive_idx_out")
        elif int(isc[_lib.I_N_FIN_PRE]) + int(isc[_lib.I_N_FIN_POST]) > 0:
            pool._call("cmbpo_rollout_compact")      # the alive list only changes when a branch finished
            pool.swap("alive_idx", "alive_idx_out")
            # the survivors' count follows from the counters just read: no second host synchronisation
            pool._n_alive = n - int(isc[_lib.I_N_FIN_PRE]) - int(isc[_lib.I_N_FIN_POST])
        pool.swap("cur_obs", "next_obs")
        pool.swap("v_t", "v_n")
        pool.swap("vc_t", "vc_n")
        pool.ptr += 1
        pool.rs.ptr = pool.ptr
        return self._step_info(dsc, sharded)

    def _step_info(self, dsc, sharded):
        """The info of a step, after taking the sampler's totals from the accumulators `dsc` it left (None: an idle step, nothing
        moved).  `sharded`: alive_ratio and the totals over all shards (one collective)."""
        pool, t = self.pool, self.pool.t
        if dsc is not None:
            self._host["total_samples"] = float(dsc[_lib.D_TOTAL_SAMPLES])
            self._host["total_dkl"] = float(dsc[_lib.D_TOTAL_DKL])
        if sharded:
            g = self.comm.all_reduce_host([pool.n_alive, self.batch_size, self._host["total_samples"]])
            alive_ratio, self._global_total_samples = g[0] / g[1], g[2]
            self.global_alive = int(g[0])
        else:
            alive_ratio = pool.n_alive / self.batch_size
        return {"alive_ratio": alive_ratio, "ensemble_dkl_path": t["dkl_t"], "cost": t["cost_t"]}

    def sample_many(self, max_steps=None, max_samples=None, stop_total=None, min_alive_ratio=None):
        """Consecutive sample() calls without the interpreter between them (cmbpo_rollout_run): the rollout loop of
        algorithms/cmbpo.py:352-360.  Steps until `max_steps` are taken, no branch is alive, the buffer is full,
        alive / batch_size <= min_alive_ratio (:358-359) or the sampler's total_samples >= stop_total (:356-357) -- each
        test made after a step, as the reference's loop makes them.  `max_samples` is the budget every step is given.
        Returns (steps taken, info of the last step).  On a sharded sampler, with injected draws or with kernel events
        on, the same loop runs over sample()."""
        pool, env = self.pool, self.env
        sharded = self.comm is not None and self.comm.world > 1
        min_alive = int(np.floor(min_alive_ratio * self.batch_size + 1e-9)) if min_alive_ratio is not None else 0
        left = int(max_steps) if max_steps is not None else (1 << 30)
        steps, info = 0, None
        # shards without a budget or stop rule between them roll independently: the native loop runs each shard to its
        # end and the counts are exchanged ONCE (one collective per call instead of one per step)
        local_only = sharded and not max_samples and stop_total is None and min_alive_ratio is None and max_steps is None
        if (sharded and not local_only) or env.kernel_events is not None:
            while left > 0 and self.any_alive() and pool.has_room:
                _, _, _, info = self.sample(max_samples=max_samples)
                steps += 1
                left -= 1
                # every quantity of the stop tests is GLOBAL on a sharded sampler (the budget and alive_ratio already are):
                # all ranks leave the loop after the same step, so the step's collectives stay matched
                if stop_total is not None and self.global_total_samples >= stop_total:
                    break
                if min_alive_ratio is not None and info["alive_ratio"] <= min_alive_ratio:
                    break
            return steps, info
        t, rs = pool.t, pool.rs
        B = self.batch_size
        lib = _lib.lib()
        with torch.cuda.device(self.device):
            h = self._prepare_call(max_samples)
            if self._run_host is None:
                self._run_host = torch.empty((64, 384), dtype=torch.uint8, pin_memory=True)
                self._run_out = (C.c_int(0), C.c_int(0), C.c_int(0))
            stream = _lib.current_stream()
            stop = float("nan") if stop_total is None else float(stop_total)     # NaN: no stop rule on the total
            done_o, alive_o, swaps_o = self._run_out
            while left > 0 and pool.n_alive > 0 and pool.has_room:
                # (transition noise: step j of the call reads xi + j * xi_stride)
                ck, k, eps_ptr, inds_ptr, rs.xi = self._next_draws()
                take = min(left, ck[1].shape[0] - k, 64)
                rs.xi_stride = B * pool.obs_dim
                # (sampled terminations: step j of the call reads the chunk's thresholds + j * B)
                self._attach_thresholds(ck[4].data_ptr() + k * B * 4 if ck[4] is not None else None, B)
                _lib.check(lib.cmbpo_rollout_run(
                    C.byref(rs), pool.n_alive, h[0], h[1], h[2], h[3], env._task_id, env._model.num_nets,
                    eps_ptr, inds_ptr, B * pool.act_dim, B,
                    h[4], h[5], take, stop, min_alive, self._run_host.data_ptr(), C.byref(done_o), C.byref(alive_o),
                    C.byref(swaps_o), stream), "cmbpo_rollout_run")
                done = done_o.value
                if done == 0:
                    break
                # the struct was advanced in native code (what _after_step does per step): bring the tensor table to the same state
                if done & 1:
                    for a, b in (("cur_obs", "next_obs"), ("v_t", "v_n"), ("vc_t", "vc_n")):
                        t[a], t[b] = t[b], t[a]
                if swaps_o.value & 1:
                    t["alive_idx"], t["alive_idx_out"] = t["alive_idx_out"], t["alive_idx"]
                ck[0] = k + done
                pool.ptr += done
                self._n_episodes += done
                steps += done
                left -= done
                blk = self._run_host[:done, :128].view(torch.int32).numpy()
                self.n_budget_terminated += int(blk[:, _lib.I_N_FIN_PRE].sum() - blk[:, _lib.I_N_UNC].sum())
                last = self._run_host[done - 1]
                isc, dsc = last[:128].view(torch.int32).numpy().copy(), last[128:].view(torch.float64).numpy().copy()
                pool._n_alive, pool._size = alive_o.value, int(isc[_lib.I_SIZE])
                self._dsc = dsc
                info = self._step_info(dsc, False)
                if done < take:       # a stop test fired inside the call
                    break
        if local_only:
            # (a shard whose buffer is full cannot continue: its rows do not keep the other shards in the caller's loop --
            # every shard leaves `while any_alive() and has_room` after the same call, the collectives stay matched)
            g = self.comm.all_reduce_host([pool.n_alive, self.batch_size, self._host["total_samples"],
                                           pool.n_alive if pool.has_room else 0])
            self.global_alive, self._global_total_samples = int(g[3]), g[2]
            info = self._step_info(None, False)
            info["alive_ratio"] = g[0] / g[1]
        return steps, info

    def _idle_step(self, max_samples):
        pool, t = self.pool, self.pool.t
        with torch.cuda.device(self.device):
            if max_samples:
                pool.rs.max_samples = int(max_samples)
                pool._call("cmbpo_rollout_count")
                self.comm.all_gather_i32(t["iscal"][8:12])
        return t["cur_obs"], t["rew_t"], t["term_t"], self._step_info(None, True)

    def any_alive(self):
        """True while any shard still has alive branches (== pool.n_alive > 0 on one GPU)."""
        if self.comm is not None and self.comm.world > 1:
            return self.global_alive > 0
        return self.pool.n_alive > 0

    def finish_all_paths(self):
        """model_sampler.py:418-444: bootstrap-finish whatever is still alive, return diagnostics."""
        if self.pool.n_alive > 0:
            with torch.cuda.device(self.device):
                self.pool._call("cmbpo_rollout_finish", 2)
                self.pool._call("cmbpo_rollout_compact")
                self.pool.swap("alive_idx", "alive_idx_out")
            self.pool.sync_counters()
            assert self.pool.n_alive == 0   # something went wrong with finishing all paths
        return self.get_diagnostics()

    def compute_dynamics_dkl(self, obs_batch, depth=1):
        """model_sampler.py:151-167: mean per-step ensemble DKL along `depth` policy steps (calibration)."""
        obs = obs_batch if isinstance(obs_batch, torch.Tensor) else \
            torch.from_numpy(np.ascontiguousarray(obs_batch, dtype=np.float32))
        obs = obs.to(self.device, torch.float32)
        for _ in range(depth):
            n = obs.shape[0]
            if n == 0:
                break
            outs = self.policy.get_action_outs(obs)
            next_obs, _, terminal, info = self.env.step(obs, outs["pi"])
            self._host["total_dkl"] += float(info["ensemble_dkl_mean"]) * n
            self._host["total_samples"] += n
            obs = next_obs[~terminal[:, 0]]
        return self.dyn_dkl * depth
