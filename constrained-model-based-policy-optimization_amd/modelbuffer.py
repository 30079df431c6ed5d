"""ModelBuffer -- host-side mirror of ``buffers/modelbuffer.py:18-226`` over device-resident state.

Same constructor / ``initialize`` / ``reset`` / ``store_multiple`` / ``finish_path_multiple`` / ``get``
and the ``size`` / ``has_room`` / ``alive_paths`` properties.  The arrays live on the GPU as torch
tensors and every operation is a HIP kernel behind the C-ABI (``csrc/rollout_state.hip``).

Layout differences (performance only, invisible through the API):
  * buffers are time-major ``[T, B, ...]`` and allocated once; ``reset()`` zeroes pointers instead of
    re-allocating 17 arrays (``modelbuffer.py:53-98``);
  * ``next_obs`` / ``dyn_error`` / ``term`` / ``roll_lengths`` buffers are never read by ``get()`` in the
    reference (``modelbuffer.py:212-218``) and are not kept -- except with ``iv_gae=True``, which keeps the running float64
    sum of ``dyn_error`` per stored entry (``cumvar_buf``): the weights of the inverse-variance-weighted GAE;
  * ``populated_mask[b, t]`` is represented as ``t < len[b]`` (alive branches share ``ptr``).

``get()`` returns the reference's 12-array list ``[obs, act, adv, cadv, ret, cret, logp, val, cval, cost,
log_std, mu]`` (``pi_info`` sorted by key) in branch-major, time-minor order.

``iv_gae=True`` (or ``set_iv_gae(True)``) switches ``finish_path_multiple`` -- and every finish of the device-resident
sampler -- to the weighted branch of the reference's ``discount_cumsum(x, discount, lam, weights=...)``
(``utilities/utils.py:189-208``) with ``w[u] = 1 / (iv_eps + sum_{s<=u} dyn_error_s)``: a k-step return counts by the inverse
of the epistemic variance accumulated on the way to it.  The reference's buffer keeps ``dyn_error_buf`` for this and comments
both GAE lines accordingly (``modelbuffer.py:167,176``) but calls the un-weighted branch; off (the default) is that behaviour.
Constant weights do not reduce to plain GAE: the reference folds the weight beyond the last step into the last one.

``set_disagreement(on, rew_pessimism, cost_pessimism)`` attaches the arrays of the ensemble disagreement on reward and cost
(``cmbpo_disagreement_t``: this step's ``rew_var_t`` / ``cost_var_t``, the per-branch float64 sums ``path_rew_var`` /
``path_cost_var`` over the stored steps, the scratch of the step's totals) beside the rollout struct; ``ModelSampler.reset``
calls it with its environment's settings.  Off (the default) nothing is allocated and nothing is measured.

``set_value_disagreement(on, v_pessimism, vc_pessimism)`` attaches the arrays of the critics' own disagreement
(``cmbpo_value_disagreement_t``: ``v_var`` / ``vc_var``, the variance over the critic members at the observation each slot was
last evaluated at, and the scratch of the step's totals).  With it every critic evaluation of an imagined rollout goes through
``cmbpo_critic_pair_predict_var``: ``v_t / vc_t / v_n / vc_n`` -- and with them ``val_buf`` / ``cval_buf``, every bootstrap, the
GAE and ``get()`` -- hold ``V - v_pessimism * sigma_v`` and ``VC + vc_pessimism * sigma_vc``.  Off (the default) nothing is
allocated and nothing is measured.

``set_trust_weights(ref_var)`` (needs ``iv_gae``): every ``get()`` also leaves, in ``last_weights``, one trust weight per
returned sample, ``ref_var / (ref_var + accumulated variance)`` from the same ``cumvar_buf`` (1 where the model has accumulated
no variance, 1/2 at ``ref_var``; with ``ref_var = iv_eps`` proportional to the GAE's own weight) -- for the weighted policy and
critic updates.  What ``get()`` returns is unchanged.

``set_rule_votes(on, term_members, cost_members)`` attaches the votes on the task's static rules (``cmbpo_rule_votes_t``, DESIGN
3za): the one-call step and the native loop then evaluate the termination / cost rule on every member's next state, ``term_t`` /
``cost_t`` (and, with the disagreement, ``cost_var_t``) are the voted ones, and ``rule_done_votes_t`` / ``rule_cost_votes_t`` [B]
hold the step's votes.  Off (the default) nothing is allocated, nothing is attached and no kernel is added.
"""
import collections
import ctypes as C
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import RolloutStruct

EPS = 1e-8  # utilities/utils.py:19


def iv_tables(lam, T):
    """The two float64 lambda tables of the weighted GAE: lam_vec[T] by lfilter's recurrence (lam_vec[0] = 1, lam_vec[u] =
    lam * lam_vec[u-1], utilities/utils.py:195-197) and lam ** L for L = 0..T by Python's pow (:192) -- built on the host so
    that the device has no pow of its own to disagree with."""
    lam = float(lam)
    vec = np.empty(int(T), np.float64)
    v = 1.0
    for u in range(int(T)):
        vec[u] = v
        v = lam * v
    return vec, np.array([lam ** L for L in range(int(T) + 1)], np.float64)


def _iv_fill(buf, iv):
    """The weighted GAE's struct: the accumulated variance, eps, and the four lambda tables -- rewritten in place (same
    addresses: ordered on the stream behind the kernels that read the old values) whenever the lambdas may have changed."""
    t, T = buf.t, buf.max_path_length
    t["iv_tables"].copy_(torch.from_numpy(np.concatenate(iv_tables(buf.lam, T) + iv_tables(buf.cost_lam, T))))
    base = t["iv_tables"].data_ptr()
    iv.cumvar_buf = t["cumvar_buf"].data_ptr()
    iv.lam_vec, iv.lam_pow = base, base + 8 * T
    iv.clam_vec, iv.clam_pow = base + 8 * (2 * T + 1), base + 8 * (3 * T + 1)
    iv.eps = buf.iv_eps


def _dis_fill(buf, dg):
    t = buf.t
    dg.kappa_rew, dg.kappa_cost = buf.rew_pessimism, buf.cost_pessimism
    dg.rew_var_t, dg.cost_var_t = t["rew_var_t"].data_ptr(), t["cost_var_t"].data_ptr()
    dg.path_rew_var, dg.path_cost_var = t["path_rew_var"].data_ptr(), t["path_cost_var"].data_ptr()
    dg.part = t["dis_part"].data_ptr()


def _vdis_fill(buf, vd):
    t = buf.t
    vd.kappa_v, vd.kappa_vc = buf.v_pessimism, buf.vc_pessimism
    vd.v_var, vd.vc_var = t["v_var"].data_ptr(), t["vc_var"].data_ptr()
    vd.part = t["vdis_part"].data_ptr()


def _term_fill(buf, th):
    t = buf.t
    th.threshold, th.members = buf.term_head[0], _lib.TERM_MEMBERS[buf.term_head[1]]
    th.term_pred, th.term_votes = t["term_pred_t"].data_ptr(), t["term_votes_t"].data_ptr()


def _cost_fill(buf, ch):
    ch.kind, ch.logit_shift = _lib.COST_KINDS[buf.cost_head[0]], buf.cost_head[1]
    ch.cost_logit = buf.t["cost_logit_t"].data_ptr()


def _votes_fill(buf, rv):
    t = buf.t
    rv.done_members = _lib.RULE_DONE_MEMBERS[buf.rule_votes[0]]
    rv.cost_members = _lib.RULE_COST_MEMBERS[buf.rule_votes[1]]
    rv.done_votes = t["rule_done_votes_t"].data_ptr()
    rv.cost_votes = t["rule_cost_votes_t"].data_ptr() if buf.rule_votes[2] else None


# The features kept beside the rollout struct, in the order they are attached: is it on, the arrays it owns in ``self.t``
# ((name, shape, dtype) for capacity B and horizon T: allocated zeroed when it is switched on, freed when it is switched off), its
# struct and how to fill it, the entry points that attach and detach it.  The next feature is one more row.
_Side = collections.namedtuple("_Side", "on arrays struct fill attach detach")
_part = lambda B: ((B + 63) // 64) * 2      # scratch of a step's two totals, per 64 branches
_SIDE = {
    "iv": _Side(lambda buf: buf.iv_gae,
                lambda B, T: (("cumvar_buf", (T, B), torch.float64), ("iv_tables", (4 * T + 2,), torch.float64)),
                _lib.IvGaeStruct, _iv_fill, "cmbpo_rollout_iv_attach", "cmbpo_rollout_iv_detach"),
    "dis": _Side(lambda buf: buf.disagreement,
                 lambda B, T: (("rew_var_t", (B,), torch.float32), ("cost_var_t", (B,), torch.float32),
                               ("path_rew_var", (B,), torch.float64), ("path_cost_var", (B,), torch.float64),
                               ("dis_part", (_part(B),), torch.float64)),
                 _lib.DisagreementStruct, _dis_fill, "cmbpo_rollout_disagreement_attach", "cmbpo_rollout_disagreement_detach"),
    "vdis": _Side(lambda buf: buf.value_disagreement,
                  lambda B, T: (("v_var", (B,), torch.float32), ("vc_var", (B,), torch.float32),
                                ("vdis_part", (_part(B),), torch.float64)),
                  _lib.ValueDisagreementStruct, _vdis_fill, "cmbpo_rollout_value_disagreement_attach",
                  "cmbpo_rollout_value_disagreement_detach"),
    "term": _Side(lambda buf: buf.term_head is not None,
                  lambda B, T: (("term_pred_t", (B,), torch.float32), ("term_votes_t", (B,), torch.uint8)),
                  _lib.TermHeadStruct, _term_fill, "cmbpo_rollout_term_head_attach", "cmbpo_rollout_term_head_detach"),
    "votes": _Side(lambda buf: buf.rule_votes is not None,
                   lambda B, T: (("rule_done_votes_t", (B,), torch.uint8), ("rule_cost_votes_t", (B,), torch.uint8)),
                   _lib.RuleVotesStruct, _votes_fill, "cmbpo_rollout_rule_votes_attach", "cmbpo_rollout_rule_votes_detach"),
    "cost": _Side(lambda buf: buf.cost_head is not None,
                  lambda B, T: (("cost_logit_t", (B,), torch.float32),),
                  _lib.CostHeadStruct, _cost_fill, "cmbpo_rollout_cost_head_attach", "cmbpo_rollout_cost_head_detach"),
}


def _detach_all(rs):
    """Drop whatever the library's table holds under this struct's key (its iscal)."""
    for side in _SIDE.values():
        _lib.check(getattr(_lib.lib(), side.detach)(C.byref(rs)), side.detach)
    # (the sampler's termination thresholds travel in the same entry: ModelSampler(term_sampling=True))
    _lib.check(_lib.lib().cmbpo_rollout_term_draws_attach(C.byref(rs), None, 0), "cmbpo_rollout_term_draws_attach")


def _iv_release(key):
    """Finaliser of a buffer: no entry of the library's tables may outlive the arrays it points to."""
    try:
        if key[0]:
            rs = RolloutStruct()
            rs.iscal = key[0]
            _detach_all(rs)
    except Exception:      # interpreter shutdown
        pass


def _np_or_t(x, device, dtype=torch.float32):
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=dtype)
    return torch.as_tensor(np.ascontiguousarray(x), device=device).to(dtype)


class ModelBuffer:
    def __init__(self, batch_size, obs_dim, act_dim, max_path_length, device=None, comm=None,
                 *args, iv_gae=False, iv_eps=1e-8, **kwargs):
        self.max_path_length = int(max_path_length)
        self.batch_size = int(batch_size)
        self.capacity = int(batch_size)
        self.obs_shape, self.act_shape = obs_dim, act_dim
        self.obs_dim = int(np.prod(obs_dim))
        self.act_dim = int(np.prod(act_dim))
        self.device = torch.device(device if device is not None else "cuda")
        self.comm = comm                      # optional dist.Comm for sharded statistics
        self.pi_info_shapes = None
        self.gamma, self.lam, self.cost_gamma, self.cost_lam = 0.99, 0.95, 0.99, 0.95
        self.iv_gae, self.iv_eps = bool(iv_gae), self._check_iv_eps(iv_eps)
        self.disagreement, self.rew_pessimism, self.cost_pessimism = False, 0.0, 0.0
        self.value_disagreement, self.v_pessimism, self.vc_pessimism = False, 0.0, 0.0
        self.term_head = None                 # (threshold, members) of the learned termination head, None: off
        self.cost_head = None                 # (loss, logit_shift) of a logistic learned-cost head, None: the magnitude reading
        self.rule_votes = None                # (term members, cost members, count the cost votes) of the static votes, None: off
        self.trust_var, self.last_weights = None, None
        self.rs = None
        self._iv_key = [0]                    # iscal of the arrays the library's table may hold an entry for
        weakref.finalize(self, _iv_release, self._iv_key)
        self._alloc(self.capacity)
        self.reset()

    # ------------------------------------------------------------------------------------------
    def _alloc(self, B):
        T, D, A, dev = self.max_path_length, self.obs_dim, self.act_dim, self.device
        if self.rs is not None:               # the table's key is the old iscal
            _detach_all(self.rs)
        f = dict(dtype=torch.float32, device=dev)
        d = dict(dtype=torch.float64, device=dev)
        t = {}
        for name, dim in (("obs_buf", D), ("act_buf", A), ("mu_buf", A), ("ls_buf", A)):
            t[name] = torch.empty((T, B, dim), **f)
        for name in ("rew_buf", "val_buf", "cost_buf", "cval_buf", "logp_buf",
                     "adv_buf", "ret_buf", "cadv_buf", "cret_buf"):
            t[name] = torch.empty((T, B), **f)
        t["alive_idx"] = torch.empty(B, dtype=torch.int32, device=dev)
        t["alive_idx_out"] = torch.empty(B, dtype=torch.int32, device=dev)
        # device scalar block: int32[32] counters | float64[32] accumulators, one D2H copy reads both
        t["scal_bytes"] = torch.zeros(32 * 4 + 32 * 8, dtype=torch.uint8, device=dev)
        t["iscal"] = t["scal_bytes"][:128].view(torch.int32)
        t["dscal"] = t["scal_bytes"][128:].view(torch.float64)
        t["alive"] = torch.empty(B, dtype=torch.uint8, device=dev)
        t["fin_code"] = torch.empty(B, dtype=torch.uint8, device=dev)
        t["len"] = torch.empty(B, dtype=torch.int32, device=dev)
        for name in ("dkl_acc", "path_ret", "path_cost", "path_dyn_var"):
            t[name] = torch.empty(B, **d)
        t["store_part"] = torch.empty(((B + 63) // 64) * 8, **d)
        # per-step values (slot indexed); cur/next and t/n pairs are swapped every step
        for name, dim in (("cur_obs", D), ("next_obs", D), ("act_t", A), ("mu_t", A), ("ls_t", A)):
            t[name] = torch.zeros((B, dim), **f)
        for name in ("logp_t", "v_t", "vc_t", "v_n", "vc_n", "rew_t", "cost_t", "dkl_t", "epv_t"):
            t[name] = torch.zeros(B, **f)
        t["term_t"] = torch.zeros(B, dtype=torch.uint8, device=dev)
        t["offsets"] = torch.empty(B + 1, dtype=torch.int32, device=dev)
        t["stats"] = torch.zeros(16, **d)
        self.t = t
        self.capacity = B
        self.rs = RolloutStruct()
        self.rs.T, self.rs.obs_dim, self.rs.act_dim = T, D, A
        self.rs.rank, self.rs.world = 0, 1
        self.rs.max_samples = 0
        self.rs.dkl_lim = float("inf")
        self.rs.max_path_length = T
        self._bind_all()
        self._iv_key[0] = self.t["iscal"].data_ptr()
        for feature in _SIDE:
            self._side_sync(feature)

    def _bind_all(self):
        for name, _ in RolloutStruct._fields_:
            if name in self.t:
                setattr(self.rs, name, self.t[name].data_ptr())
        self.rs.use_host_budget = 0

    # -- inverse-variance-weighted GAE ----------------------------------------------------------
    @staticmethod
    def _check_iv_eps(iv_eps):
        iv_eps = float(iv_eps)
        if not (iv_eps > 0.0 and np.isfinite(iv_eps)):
            raise ValueError(f"iv_eps must be a positive finite number, got {iv_eps}")
        return iv_eps

    def set_iv_gae(self, on, iv_eps=1e-8):
        """Switch the inverse-variance-weighted GAE on or off; legal whenever nothing is stored."""
        iv_eps = self._check_iv_eps(iv_eps)
        if self.ptr != 0 or self._size != 0:
            raise RuntimeError("set_iv_gae: the buffer holds samples (call it after get() / reset())")
        if not on and self.trust_var is not None:
            raise ValueError("set_iv_gae(False): the trust weights read the variance it keeps (set_trust_weights(None) first)")
        self.iv_gae, self.iv_eps = bool(on), iv_eps
        self._side_sync("iv")

    def set_trust_weights(self, ref_var):
        """Switch the trust weights of get() on (ref_var > 0: the accumulated variance at which a sample weighs 1/2) or off
        (None); legal whenever nothing is stored."""
        if ref_var is not None:
            ref_var = float(ref_var)
            if not (ref_var > 0.0 and np.isfinite(ref_var)):
                raise ValueError(f"ref_var must be a positive finite number or None, got {ref_var}")
            if not self.iv_gae:
                raise ValueError("set_trust_weights needs iv_gae=True: the accumulated variance is only kept there")
        if self.ptr != 0 or self._size != 0:
            raise RuntimeError("set_trust_weights: the buffer holds samples (call it after get() / reset())")
        self.trust_var = ref_var
        if ref_var is None:
            self.last_weights = None

    # -- ensemble disagreement on reward / cost --------------------------------------------------
    def set_disagreement(self, on, rew_pessimism=0.0, cost_pessimism=0.0):
        """Measure the ensemble's disagreement on reward and cost along the rollout (and hold kappa * sigma against the
        branch where a coefficient is > 0, which implies `on`); legal whenever nothing is stored."""
        kr, kc = float(rew_pessimism), float(cost_pessimism)
        if not (np.isfinite(kr) and kr >= 0.0 and np.isfinite(kc) and kc >= 0.0):
            raise ValueError(f"rew_pessimism / cost_pessimism must be finite numbers >= 0, got {kr}, {kc}")
        on = bool(on) or kr > 0.0 or kc > 0.0
        if (on, kr, kc) == (self.disagreement, self.rew_pessimism, self.cost_pessimism):
            return
        if self.ptr != 0 or self._size != 0:
            raise RuntimeError("set_disagreement: the buffer holds samples (call it after get() / reset())")
        self.disagreement, self.rew_pessimism, self.cost_pessimism = on, kr, kc
        self._side_sync("dis")

    # -- critic disagreement: pessimistic value bootstraps ----------------------------------------
    def set_value_disagreement(self, on, v_pessimism=0.0, vc_pessimism=0.0):
        """Measure the variance over the critic members at every state the rollout evaluates (and hold kappa * sigma against
        the branch where a coefficient is > 0, which implies `on`: V - kappa_v sigma_v, VC + kappa_vc sigma_vc); legal
        whenever nothing is stored."""
        kv, kc = float(v_pessimism), float(vc_pessimism)
        if not (np.isfinite(kv) and kv >= 0.0 and np.isfinite(kc) and kc >= 0.0):
            raise ValueError(f"v_pessimism / vc_pessimism must be finite numbers >= 0, got {kv}, {kc}")
        on = bool(on) or kv > 0.0 or kc > 0.0
        if (on, kv, kc) == (self.value_disagreement, self.v_pessimism, self.vc_pessimism):
            return
        if self.ptr != 0 or self._size != 0:
            raise RuntimeError("set_value_disagreement: the buffer holds samples (call it after get() / reset())")
        self.value_disagreement, self.v_pessimism, self.vc_pessimism = on, kv, kc
        self._side_sync("vdis")

    # -- learned termination head ------------------------------------------------------------------
    def set_term_head(self, on, threshold=0.5, members='elite'):
        """End imagined branches where the model's termination column says so (``FakeEnv(predicts_term=True)``: the sampler
        hands its environment's head over at every reset); legal whenever nothing is stored.  The step's ``term_pred_t`` /
        ``term_votes_t`` [B] are kept beside the per-step arrays.  ``threshold`` is the number the kernel compares with: for a
        logistic head (``FakeEnv(term_loss='logistic')``) the logit of the probability, and ``term_pred_t`` then
        carries the logit."""
        head = None
        if on:
            threshold = float(threshold)
            if not np.isfinite(threshold):
                raise ValueError(f"term_threshold must be a finite number, got {threshold}")
            if members not in _lib.TERM_MEMBERS:
                raise ValueError(f"term_members: 'elite', 'any' or 'majority', got {members!r}")
            head = (threshold, members)
        if head == self.term_head:
            return
        if self.ptr != 0 or self._size != 0:
            raise RuntimeError("set_term_head: the buffer holds samples (call it after get() / reset())")
        self.term_head = head
        self._side_sync("term")

    # -- the reading of the learned-cost column -------------------------------------------------------
    def set_cost_head(self, loss='gaussian', logit_shift=0.0):
        """Read the model's cost column as a logit (``loss='logistic'``, ``FakeEnv(cost_loss='logistic')``, DESIGN §3w: the
        sampler hands its environment's head over at every reset) or as a magnitude ('gaussian': nothing attached); legal
        whenever nothing is stored.  Under 'logistic' ``cost_t`` / ``cost_buf`` hold probabilities and the step's raw logits
        are kept in ``cost_logit_t`` [B]."""
        if loss not in _lib.COST_KINDS:
            raise ValueError(f"cost_loss: 'gaussian' or 'logistic', got {loss!r}")
        shift = float(logit_shift)
        if not np.isfinite(shift):
            raise ValueError(f"cost_logit_shift must be a finite number, got {shift}")
        head = (loss, shift) if loss == 'logistic' else None
        if head == self.cost_head:
            return
        if self.ptr != 0 or self._size != 0:
            raise RuntimeError("set_cost_head: the buffer holds samples (call it after get() / reset())")
        self.cost_head = head
        self._side_sync("cost")

    # -- ensemble-voted static rules --------------------------------------------------------------------
    def set_rule_votes(self, on, term_members='elite', cost_members='elite', cost_votes=True):
        """Let the ensemble vote on the task's static termination / cost rule along the rollout (``FakeEnv(static_*_members=,
        static_votes=)``, DESIGN §3za: the sampler hands its environment's setting over at every reset); legal whenever nothing is
        stored.  The step's ``rule_done_votes_t`` / ``rule_cost_votes_t`` [B] are kept beside the per-step arrays;
        ``cost_votes=False`` (a learned cost: the static cost rule is skipped) counts no cost votes."""
        votes = None
        if on:
            if term_members not in _lib.RULE_DONE_MEMBERS:
                raise ValueError(f"static_term_members: 'elite', 'any' or 'majority', got {term_members!r}")
            if cost_members not in _lib.RULE_COST_MEMBERS:
                raise ValueError(f"static_cost_members: 'elite', 'any', 'majority' or 'mean', got {cost_members!r}")
            votes = (term_members, cost_members, bool(cost_votes))
        if votes == self.rule_votes:
            return
        if self.ptr != 0 or self._size != 0:
            raise RuntimeError("set_rule_votes: the buffer holds samples (call it after get() / reset())")
        self.rule_votes = votes
        self._side_sync("votes")

    # -- the state beside the struct ------------------------------------------------------------
    def _side_sync(self, feature):
        """Attach (on: for the current arrays and settings) or detach (off: and free) one feature of _SIDE beside the struct."""
        side, lib, t = _SIDE[feature], _lib.lib(), self.t
        arrays = side.arrays(self.capacity, self.max_path_length)
        if not side.on(self):
            _lib.check(getattr(lib, side.detach)(C.byref(self.rs)), side.detach)
            for name, _, _ in arrays:
                t.pop(name, None)
            return
        for name, shape, dtype in arrays:
            if name not in t:
                t[name] = torch.zeros(shape, dtype=dtype, device=self.device)
        st = side.struct()
        side.fill(self, st)
        _lib.check(getattr(lib, side.attach)(C.byref(self.rs), C.byref(st)), side.attach)

    def swap(self, a, b):
        """Exchange two same-shaped state arrays (cur_obs <-> next_obs, v_t <-> v_n, ...)."""
        self.t[a], self.t[b] = self.t[b], self.t[a]
        setattr(self.rs, a, self.t[a].data_ptr())
        setattr(self.rs, b, self.t[b].data_ptr())

    def _call(self, fn, *args):
        with torch.cuda.device(self.device):
            _lib.check(getattr(_lib.lib(), fn)(C.byref(self.rs), *args, _lib.current_stream()), fn)

    # ------------------------------------------------------------------------------------------
    def initialize(self, pi_info_shapes, gamma=0.99, lam=0.95, cost_gamma=0.99, cost_lam=0.95):
        """modelbuffer.py:41-51."""
        self.pi_info_shapes = pi_info_shapes
        keys = sorted(pi_info_shapes.keys())
        if keys != ["log_std", "mu"]:
            raise NotImplementedError("HIP buffer stores the Gaussian pi_info {mu, log_std} (ac_network.py:120)")
        self.sorted_pi_info_keys = keys
        self.gamma, self.lam, self.cost_gamma, self.cost_lam = gamma, lam, cost_gamma, cost_lam
        self.rs.gamma, self.rs.lam = float(gamma), float(lam)
        self.rs.cost_gamma, self.rs.cost_lam = float(cost_gamma), float(cost_lam)
        if self.iv_gae:
            self._side_sync("iv")             # the tables follow the lambdas

    def reset(self, batch_size=None):
        """modelbuffer.py:53-98 (pointers only; the buffers are reused unless the batch size changes)."""
        if batch_size is not None and int(batch_size) != self.capacity:
            self.batch_size = int(batch_size)
            self._alloc(self.batch_size)
        self.rs.B = self.batch_size
        self.rs.gamma, self.rs.lam = float(self.gamma), float(self.lam)
        self.rs.cost_gamma, self.rs.cost_lam = float(self.cost_gamma), float(self.cost_lam)
        self.ptr = 0
        self.rs.ptr = 0
        self.path_start_idx = 0
        self.max_size = self.max_path_length
        self._call("cmbpo_rollout_reset")
        self._n_alive = self.batch_size
        self._size = 0

    # ------------------------------------------------------------------------------------------
    def read_scalars(self):
        """One small D2H copy (the host sync of a step): (int32 counters, float64 accumulators)."""
        if getattr(self, "_scal_host", None) is None:
            # pinned once: the copy is a true async D2H and the NumPy views below never change
            self._scal_host = torch.empty(384, dtype=torch.uint8, pin_memory=True)
            self._scal_views = (self._scal_host[:128].view(torch.int32).numpy(), self._scal_host[128:].view(torch.float64).numpy())
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().cmbpo_rollout_read_scalars(C.byref(self.rs), self._scal_host.data_ptr(), _lib.current_stream()),
                       "cmbpo_rollout_read_scalars")
        isc, dsc = self._scal_views[0].copy(), self._scal_views[1].copy()     # (the pinned block is rewritten by the next read)
        self._n_alive = int(isc[_lib.I_N_ALIVE])
        self._size = int(isc[_lib.I_SIZE])
        return isc, dsc

    def sync_counters(self):
        return self.read_scalars()[0]

    @property
    def size(self):
        return self._size

    @property
    def has_room(self):
        return self.ptr < self.max_size

    @property
    def alive_paths(self):
        """bool[B], modelbuffer.py:110-112."""
        return self.t["alive"].bool().cpu().numpy()

    @property
    def n_alive(self):
        return self._n_alive

    def alive_indices(self):
        return self.t["alive_idx"][: self._n_alive]

    # -- API-parity entry points taking host arrays in compact (alive-only) order --------------
    def store_multiple(self, obs, act, next_obs, rew, val, cost, cval, dyn_error, logp, pi_info, term):
        """modelbuffer.py:114-135.  Arguments cover the currently alive paths, in index order."""
        assert self.ptr < self.max_size
        idx = self.alive_indices().long()
        t, dev = self.t, self.device
        t["cur_obs"][idx] = _np_or_t(obs, dev)
        t["act_t"][idx] = _np_or_t(act, dev)
        t["rew_t"][idx] = _np_or_t(rew, dev)
        t["v_t"][idx] = _np_or_t(val, dev)
        t["cost_t"][idx] = _np_or_t(cost, dev)
        t["vc_t"][idx] = _np_or_t(cval, dev)
        t["epv_t"][idx] = _np_or_t(dyn_error, dev)
        t["logp_t"][idx] = _np_or_t(logp, dev)
        t["mu_t"][idx] = _np_or_t(pi_info["mu"], dev)
        t["ls_t"][idx] = _np_or_t(pi_info["log_std"], dev)
        t["fin_code"].zero_()
        self._call("cmbpo_rollout_store")
        self.ptr += 1
        self.rs.ptr = self.ptr
        self.sync_counters()

    def finish_path_multiple(self, term_mask, last_val=0, last_cval=0):
        """modelbuffer.py:138-182.  term_mask covers the alive paths; last_* the paths to finish."""
        term_mask = np.asarray(term_mask, dtype=bool)
        if not term_mask.any():
            return
        assert self._n_alive == len(term_mask)
        idx = self.alive_indices().long()
        dev = self.device
        sel = idx[torch.as_tensor(term_mask, device=dev)]
        lv = np.asarray(last_val)
        # float64 zeros (append_vals=False, model_sampler.py:404) promote the reward deltas to float64
        zero_boot = lv.dtype == np.float64 and not lv.any()
        code = torch.zeros_like(self.t["fin_code"])
        code[sel] = 2 if zero_boot else 1
        self.t["fin_code"].copy_(code)
        self.t["v_t"][sel] = _np_or_t(np.broadcast_to(lv, (int(term_mask.sum()),)), dev)
        self.t["vc_t"][sel] = _np_or_t(np.broadcast_to(np.asarray(last_cval), (int(term_mask.sum()),)), dev)
        self._call("cmbpo_rollout_finish", 0)
        self._call("cmbpo_rollout_compact")
        self.swap("alive_idx", "alive_idx_out")
        self.sync_counters()

    # ------------------------------------------------------------------------------------------
    def get(self, as_tensors=False):
        """modelbuffer.py:184-226: normalise adv, centre cadv, flatten populated entries, reset."""
        self.sync_counters()
        assert self._n_alive == 0, "all paths have to be finished"          # modelbuffer.py:194
        t = self.t
        ev = None
        if getattr(self, "get_events", None) is not None:    # bench.py: HIP events around get()'s kernels
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True),
                  torch.cuda.Event(enable_timing=True))
        # the number of stored samples is the pool's size counter, read with the step counters: no device round trip here --
        # and the output block is sized and split BEFORE the first launch, so that the scan / moment launches and the flatten
        # follow each other on the stream without the interpreter between them
        n = int(self._size)
        D, A, dev = self.obs_dim, self.act_dim, self.device
        dims = [D, A, 0, 0, 0, 0, 0, 0, 0, 0, A, A]
        # one allocation for the twelve arrays (each starts on a 256-byte boundary) and one split: the list holds views of it
        sizes = []
        for d in dims:
            m = n * max(d, 1)
            sizes += [m, -m % 64]
        flat = torch.empty(max(sum(sizes), 1), dtype=torch.float32, device=dev)
        parts = flat.split_with_sizes(sizes)[0::2] if n > 0 else [flat[:0]] * 12
        outs = [p_.view(n, d) if d else p_ for p_, d in zip(parts, dims)]
        ptrs = (C.c_void_p * 12)(*[o.data_ptr() for o in outs])
        if ev is not None:
            ev[0].record()
        sharded = self.comm is not None and self.comm.world > 1
        if sharded:
            self._call("cmbpo_buffer_offsets", t["offsets"].data_ptr())
            self._call("cmbpo_buffer_moments", 0, t["stats"].data_ptr())
            self.comm.all_reduce_sum(t["stats"][8:13])
            self._call("cmbpo_buffer_moments", 1, t["stats"].data_ptr())
            self._call("cmbpo_buffer_moments", 2, t["stats"].data_ptr())
            self.comm.all_reduce_sum(t["stats"][13:14])
            self._call("cmbpo_buffer_moments", 3, t["stats"].data_ptr())
        else:
            # one GPU: the scan and both moment passes as two launches
            self._call("cmbpo_buffer_prepare", t["offsets"].data_ptr(), t["stats"].data_ptr())
        if n > 0:
            if ev is not None:
                ev[1].record()
            self._call("cmbpo_buffer_flatten", t["offsets"].data_ptr(), t["stats"].data_ptr(), ptrs)
            if ev is not None:
                ev[2].record()
                self.get_events.append((ev[0], ev[1], ev[2], n))
            wts = None
            if self.trust_var is not None:      # (before reset(): the variance table is this rollout's)
                wts = torch.empty(n, dtype=torch.float32, device=dev)
                self._call("cmbpo_buffer_trust_weights", t["offsets"].data_ptr(), C.c_double(self.trust_var), wts.data_ptr())
                w_stat = torch.stack([wts.mean(dtype=torch.float64), wts.min().double()])
            st = t["stats"].cpu().numpy()
            ret_mean, cret_mean = float(st[4]), float(st[5])
        else:
            ret_mean, cret_mean = 0, 0
            wts = torch.empty(0, dtype=torch.float32, device=dev) if self.trust_var is not None else None
            w_stat = torch.zeros(2, dtype=torch.float64)
        diagnostics = dict(poolm_batch_size=n, poolm_ret_mean=ret_mean, poolm_cret_mean=cret_mean)
        if self.trust_var is not None:
            w_stat = w_stat.cpu().numpy()
            diagnostics.update(poolm_weight_mean=float(w_stat[0]), poolm_weight_min=float(w_stat[1]))
            self.last_weights = wts if as_tensors else wts.cpu().numpy()
        else:
            self.last_weights = None
        res = outs if as_tensors else [o.cpu().numpy() for o in outs]
        self.reset()
        return res, diagnostics
