"""Open-loop model validation: the device buffers of a k-step replay of real trajectories and its result table
(``csrc/replay.hip``).  The reference has no counterpart.

``ReplayBuffers`` owns every array ``cmbpo_replay_t`` names -- the recorded windows (time-major ``[H, B, .]``), the rows'
state, the post kernel's outputs of the step, the partial sums and the table -- and the ctypes image handed to
``cmbpo_replay_compare`` / ``_finish`` / ``_run``.  ``FakeEnv.replay`` is the user's entry; the tests and
``tools/probe_replay.py`` drive the single calls through this class.

Predictive calibration: ``ReplayBuffers(..., calibration=True)`` also owns the arrays of
``cmbpo_replay_calib_t``; ``calibration_table`` builds the per-horizon, per-column table from its raw sums and counts, and
``temperature`` turns one row of it into the variance temperature ``ModelSampler.set_noise_scale`` takes the root of.

Reliability of the logistic columns: ``ReplayBuffers(..., reliability=dict(columns=[...], bins=K))`` also owns the
arrays of ``cmbpo_replay_reliab_t``; ``reliability_table`` builds, per column and reading, the per-bin confidence against the
observed frequency with ECE / MCE / Brier / log loss from the raw sums and counts, and ``logit_offset`` turns one horizon of
it into the logit offset that makes the column's mean probability the observed rate (calibration-in-the-large).

The static rules' votes: ``ReplayBuffers(..., votes=dict(done_members=, cost_members=, learned_cost=))`` also owns
the arrays of ``cmbpo_replay_votes_t``; ``run_votes`` replays with the vote kernel in the post step, and ``votes_table`` builds,
per signal and horizon, the histogram of the vote count against the recorded flag, the reliability of the share ``v / E`` and the
2x2 counts of the 'any' and 'majority' readings from the raw integer counts.

The particle replay: ``ParticleBuffers`` owns the arrays of ``cmbpo_replay_particles_t`` -- every window replayed
by S sampled particles, R = B S rows --, and ``particles_table`` builds, per horizon and column, the rank histogram of the
recorded value among the particles, the fair CRPS and the spread / skill ratio from the raw sums and counts.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

MODES = {"open_loop": _lib.REPLAY_OPEN_LOOP, "one_step": _lib.REPLAY_ONE_STEP}
SUM_KEYS = ("se_rew", "se_cost", "sum_ep_var", "sum_dkl")      # columns obs_dim .. obs_dim + 3 of `sums`
# the calibration table's raw arrays, [H, obs + 1] each, in the order of `sums` [H, 6, obs + 1] / `counts` [H, 4, obs + 1]
CALIB_SUM_KEYS = ("sum_z2_al", "sum_z2_tot", "sum_log_v_al", "sum_log_v_tot", "sum_v_bar", "sum_s2")
CALIB_COUNT_KEYS = ("n_cover1_al", "n_cover2_al", "n_cover1_tot", "n_cover2_tot")
READINGS = ("elite", "pooled")     # reading 0 / 1 of a reliability column: the elite member's logit / the members' mean logit


def _as(x, dtype, device):
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=dtype).contiguous()
    np_dtype = {torch.float32: np.float32, torch.uint8: np.uint8, torch.int32: np.int32}[dtype]
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np_dtype)).to(device)


def _windows(obs0, actions, next_obs, rewards, costs, terminals, lengths, mode, dev, max_obs=None):
    """The recorded windows, validated and on the device: ``H, B, D, A`` and the tensors ``act``, ``next_obs``, ``rew``, ``cost``,
    ``term``, ``len`` (the descriptors' names) and ``obs0``.  ``max_obs``: the particle kernel's limit on obs_dim."""
    if mode not in MODES:
        raise ValueError("replay mode: 'open_loop' or 'one_step', got %r" % (mode,))
    f32, u8, i32 = torch.float32, torch.uint8, torch.int32
    act, nxt = _as(actions, f32, dev), _as(next_obs, f32, dev)
    if nxt.dim() != 3 or act.dim() != 3 or act.shape[:2] != nxt.shape[:2]:
        raise ValueError("replay: actions [H, B, act] and next_obs [H, B, obs] expected, got %s and %s"
                         % (tuple(act.shape), tuple(nxt.shape)))
    H, B, D = nxt.shape
    if H < 1 or B < 1:
        raise ValueError("replay: at least one window of one step, got H = %d, B = %d" % (H, B))
    if max_obs is not None and D > max_obs:
        raise ValueError("replay: particles need obs_dim <= %d (the 64-row tile a workgroup stages in LDS), got %d" % (max_obs, D))
    obs0 = _as(obs0, f32, dev)
    if tuple(obs0.shape) != (B, D):
        raise ValueError("replay: obs0 must be [%d, %d], got %s" % (B, D, tuple(obs0.shape)))
    flat = lambda x, dt: _as(x, dt, dev).reshape(H, B)
    t = dict(act=act, next_obs=nxt, rew=flat(rewards, f32), cost=flat(costs, f32), term=flat(terminals, u8), obs0=obs0)
    if lengths is None:
        t["len"] = torch.full((B,), H, dtype=i32, device=dev)
    else:
        t["len"] = _as(lengths, i32, dev).reshape(B)
        lo, hi = int(t["len"].min()), int(t["len"].max())
        if lo < 1 or hi > H:
            raise ValueError("replay: lengths must lie in 1..%d, got %d..%d" % (H, lo, hi))
    return H, B, D, act.shape[2], t


def _table(H, n_part, ns, nc, dev):
    """The four arrays of a table of ``ns`` float64 sums and ``nc`` int64 counts per horizon: the per-slot partials and the
    table, zeros.  ``ns == 0`` (the vote table): the counts only."""
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    t = dict(part_cnt=z((H, n_part, nc), torch.int64), counts=z((H, nc), torch.int64))
    if ns:
        t.update(part_sum=z((H, n_part, ns), torch.float64), sums=z((H, ns), torch.float64))
    return t


# the entries of one horizon of each table, (float64 sums, int64 counts): what csrc/replay.hip's *_sums / *_counts say
def calib_sizes(obs_dim):
    return _lib.REPLAY_CALIB_SUMS * (obs_dim + 1), _lib.REPLAY_CALIB_COUNTS * (obs_dim + 1) + 2


def reliab_sizes(n_bins, n_cols):
    return 2 * n_cols * (2 * n_bins + 2), 2 * n_cols * 2 * n_bins + 2 * n_cols


def particle_sizes(obs_dim, S):
    return 4 * (obs_dim + 1) + 2, (obs_dim + 1) * (S + 1) + 2


class _Buffers:
    def step_outputs(self):
        """The dict ``FakeEnv.step_device`` fills: the prediction arrays ``cmbpo_replay_compare`` / ``cmbpo_replay_particles``
        read."""
        t = self.t
        return dict(next_obs=t["p_next_obs"], rew=t["p_rew"], term=t["p_term"], cost=t["p_cost"], dkl_path=t["p_dkl_path"],
                    ep_var_mean=t["p_ep_var_mean"])


class ReplayBuffers(_Buffers):
    def __init__(self, obs0, actions, next_obs, rewards, costs, terminals, lengths=None, mode="open_loop", ensemble=0,
                 out_dim=0, device="cuda", calibration=False, reliability=None, votes=None):
        """obs0 [B, obs]; actions [H, B, act]; next_obs [H, B, obs]; rewards / costs / terminals [H, B] (a trailing axis
        of one is dropped); lengths [B] in 1..H (None: H).  NumPy arrays or tensors.  ``ensemble`` / ``out_dim`` > 0 also
        allocate the forward's scratch ``cmbpo_replay_run`` needs.  ``calibration=True`` (needs both) also allocates the
        arrays of the calibration table and its member indices ``elite`` [H, B] int32, zeros until ``set_elite``.
        ``reliability=dict(columns=[dict(name=, col=, target='cost' | 'term', shift=0.0), ...], bins=15, edges=None,
        terminals=None)`` (needs both too) also allocates the arrays of the reliability table of one or two logistic columns;
        ``edges`` [bins - 1] (ascending, finite; None: ``default_edges(bins)``) are the bin edges in logit space; ``terminals``
        [H, B] are the flags the 'term' columns are held against where they are not the recorded ones (a head's training
        targets).  It shares ``elite`` with the calibration table.
        ``votes=dict(done_members='elite', cost_members='elite', learned_cost=False, terminals=None)`` (needs ``ensemble`` in
        1..8) also allocates the arrays of the vote table: the two ``[B]`` uint8 vote arrays of a step (no cost votes under
        ``learned_cost``), the ``[B]`` ``term_pred`` / ``term_votes`` scratch a termination head needs beside the vote kernel, the
        partials and the table; the modes are those of the post step (``'elite'`` / ``'elite'`` measures only); ``terminals``
        [H, B] as for ``reliability``."""
        dev = torch.device(device)
        H, B, D, A, w = _windows(obs0, actions, next_obs, rewards, costs, terminals, lengths, mode, dev)
        cur = w.pop("obs0").clone()
        self.device, self.mode = dev, mode
        f32, u8, i32 = torch.float32, torch.uint8, torch.int32
        self.B, self.H, self.obs_dim, self.act_dim = B, H, D, A
        self.n_part = _lib.lib().cmbpo_replay_parts(B)
        f = dict(dtype=f32, device=dev)
        self.t = dict(w, cur_obs=cur, alive=torch.ones(B, dtype=u8, device=dev),
                      p_next_obs=torch.empty((B, D), **f), p_rew=torch.empty(B, **f),
                      p_term=torch.empty(B, dtype=u8, device=dev), p_cost=torch.empty(B, **f),
                      p_dkl_path=torch.empty(B, **f), p_ep_var_mean=torch.empty(B, **f),
                      **_table(H, self.n_part, D + _lib.REPLAY_SCALAR_SUMS, _lib.REPLAY_COUNTS, dev))
        if ensemble > 0:
            self.t["mean"] = torch.empty((ensemble, B, out_dim), **f)
            self.t["var"] = torch.empty_like(self.t["mean"])
        rs = _lib.ReplayStruct()
        rs.B, rs.H, rs.obs_dim, rs.act_dim, rs.mode, rs.reserved = B, H, D, A, MODES[mode], 0
        for k, v in self.t.items():
            setattr(rs, k, v.data_ptr())
        self.rs = rs
        self.cs = self.c = self.elite = None
        self.rr = self.r = None
        if calibration:
            if ensemble < 1 or out_dim < D + 1:
                raise ValueError("replay: calibration needs the forward's scratch: ensemble >= 1 and out_dim >= obs + 1 = %d, "
                                 "got %d and %d" % (D + 1, ensemble, out_dim))
            self.elite = torch.zeros((H, B), dtype=i32, device=dev)
            self.c = dict(elite=self.elite, **_table(H, self.n_part, *calib_sizes(D), dev))
            cs = _lib.ReplayCalibStruct()
            cs.ensemble, cs.out_dim, cs.reserved = int(ensemble), int(out_dim), 0
            for k, v in self.c.items():
                setattr(cs, k, v.data_ptr())
            self.cs = cs
        if reliability is not None:
            self._init_reliability(dict(reliability), int(ensemble), int(out_dim))
        self.vs = self.v = None
        if votes is not None:
            self._init_votes(dict(votes), int(ensemble))

    def _init_votes(self, spec, ensemble):
        H, B, dev = self.H, self.B, self.device
        dm, cm = spec.pop("done_members", "elite"), spec.pop("cost_members", "elite")
        learned = bool(spec.pop("learned_cost", False))
        terminals = spec.pop("terminals", None)
        if spec:
            raise ValueError("replay: unknown votes keys %s" % sorted(spec))
        if not 1 <= ensemble <= _lib.REPLAY_VOTES_MAX_ENSEMBLE or "mean" not in self.t:
            raise ValueError("replay: votes need the forward's scratch and ensemble in 1..%d (the votes of a row live in a byte "
                             "mask), got %d" % (_lib.REPLAY_VOTES_MAX_ENSEMBLE, ensemble))
        if dm not in _lib.RULE_DONE_MEMBERS:
            raise ValueError("replay: votes done_members is 'elite', 'any' or 'majority', got %r" % (dm,))
        if cm not in _lib.RULE_COST_MEMBERS:
            raise ValueError("replay: votes cost_members is 'elite', 'any', 'majority' or 'mean', got %r" % (cm,))
        if learned and cm != "elite":
            raise ValueError("replay: votes cost_members=%r with learned_cost: the static cost rule is skipped, there is nothing to "
                             "vote on" % (cm,))
        u8 = dict(dtype=torch.uint8, device=dev)
        self.v = dict(done_votes=torch.zeros(B, **u8), cost_votes=torch.zeros(0 if learned else B, **u8),
                      term=torch.zeros(0, **u8) if terminals is None else _as(terminals, torch.uint8, dev).reshape(H, B),
                      **_table(H, self.n_part, 0, _lib.REPLAY_VOTE_COUNTS, dev))
        self.head_scratch = dict(term_pred=torch.zeros(B, dtype=torch.float32, device=dev), term_votes=torch.zeros(B, **u8))
        vs = _lib.ReplayVotesStruct()
        vs.ensemble, vs.reserved = ensemble, 0
        vs.done_members, vs.cost_members = _lib.RULE_DONE_MEMBERS[dm], _lib.RULE_COST_MEMBERS[cm]
        for k, v in self.v.items():
            setattr(vs, k, v.data_ptr() if v.numel() else None)
        self.vs, self.vote_modes, self.learned_cost, self.vote_ensemble = vs, (dm, cm), learned, ensemble

    def _init_reliability(self, spec, ensemble, out_dim):
        H, B, dev = self.H, self.B, self.device
        columns = list(spec.pop("columns", ()))
        K = int(spec.pop("bins", 15))
        edges = spec.pop("edges", None)
        terminals = spec.pop("terminals", None)
        if spec:
            raise ValueError("replay: unknown reliability keys %s" % sorted(spec))
        if not 1 <= ensemble <= _lib.RELIAB_MAX_ENSEMBLE or out_dim < 1:
            raise ValueError("replay: reliability needs the forward's scratch: ensemble in 1..%d and out_dim >= 1, got %d and %d"
                             % (_lib.RELIAB_MAX_ENSEMBLE, ensemble, out_dim))
        if not 1 <= len(columns) <= _lib.RELIAB_MAX_COLS:
            raise ValueError("replay: reliability takes 1..%d columns, got %d" % (_lib.RELIAB_MAX_COLS, len(columns)))
        if not 1 <= K <= _lib.RELIAB_MAX_BINS:
            raise ValueError("replay: reliability bins must lie in 1..%d, got %d" % (_lib.RELIAB_MAX_BINS, K))
        edges = default_edges(K) if edges is None else np.asarray(edges, np.float32).reshape(-1)
        if edges.shape != (K - 1,) or not np.isfinite(edges).all() or not (np.diff(edges) > 0).all():
            raise ValueError("replay: reliability edges must be %d ascending finite numbers" % (K - 1))
        rr = _lib.ReplayReliabStruct()
        rr.ensemble, rr.out_dim, rr.n_bins, rr.n_cols, rr.reserved = ensemble, out_dim, K, len(columns), 0
        names = []
        for j, c in enumerate(columns):
            col, shift = int(c["col"]), float(c.get("shift", 0.0))
            if not 0 <= col < out_dim:
                raise ValueError("replay: reliability column %d outside the model's %d outputs" % (col, out_dim))
            if c["target"] not in _lib.RELIAB_TARGETS:
                raise ValueError("replay: reliability target is 'cost' or 'term', got %r" % (c["target"],))
            if not np.isfinite(np.float32(shift)):
                raise ValueError("replay: reliability shift must be a finite number, got %r" % (shift,))
            rr.col[j], rr.target[j], rr.shift[j] = col, _lib.RELIAB_TARGETS[c["target"]], shift
            names.append(str(c.get("name", c["target"])))
        if len(set(names)) != len(names):
            raise ValueError("replay: reliability columns need distinct names, got %s" % (names,))
        if self.elite is None:
            self.elite = torch.zeros((H, B), dtype=torch.int32, device=dev)
        self.r = dict(elite=self.elite, edges=torch.from_numpy(np.ascontiguousarray(edges)).to(dev),
                      term=torch.zeros(0, dtype=torch.uint8, device=dev) if terminals is None
                      else _as(terminals, torch.uint8, dev).reshape(H, B),
                      **_table(H, self.n_part, *reliab_sizes(K, len(columns)), dev))
        for k, v in self.r.items():
            setattr(rr, k, v.data_ptr() if v.numel() else None)
        self.rr, self.rel_names, self.rel_edges, self.n_bins = rr, tuple(names), edges, K

    def compare(self, h):
        _lib.check(_lib.lib().cmbpo_replay_compare(C.byref(self.rs), int(h), _lib.current_stream()), "cmbpo_replay_compare")

    def finish(self):
        _lib.check(_lib.lib().cmbpo_replay_finish(C.byref(self.rs), _lib.current_stream()), "cmbpo_replay_finish")

    def _run_reliab(self, calib, model_handle, task_id, ensemble, elite, term_head, cost_head):
        if elite is not None:
            self.set_elite(elite)
        ref = lambda s: C.byref(s) if s is not None else None
        _lib.check(_lib.lib().cmbpo_replay_run_reliab(C.byref(self.rs), calib, C.byref(self.rr), ref(term_head), ref(cost_head),
                                                      model_handle, int(task_id), int(ensemble), None, _lib.current_stream()),
                   "cmbpo_replay_run_reliab")

    def run_votes(self, model_handle, task_id, ensemble, elite, term_head=None, cost_head=None, calibration=False,
                  reliability=True):
        """``cmbpo_replay_run_votes``: the replay with the vote kernel in its post step and the vote table (buffers built with
        ``votes=``); elite, term_head, cost_head as in ``run``.  ``calibration`` / ``reliability``: also the tables these buffers
        were built with.  A termination head without outputs of its own gets these buffers' ``[B]`` scratch."""
        self._votes()
        ref = lambda s: C.byref(s) if s is not None else None
        lib = _lib.lib()
        if elite is not None and self.elite is not None:
            self.set_elite(elite)
        if term_head is not None and not (term_head.term_pred and term_head.term_votes):
            th = _lib.TermHeadStruct()
            th.threshold, th.members = term_head.threshold, term_head.members
            th.term_pred = term_head.term_pred or self.head_scratch["term_pred"].data_ptr()
            th.term_votes = term_head.term_votes or self.head_scratch["term_votes"].data_ptr()
            term_head = th
        rr = self.rr if reliability else None
        cal = self._calib() if calibration else None
        d_elite = None if (rr is not None or cal is not None) else elite.data_ptr()
        _lib.check(lib.cmbpo_replay_run_votes(C.byref(self.rs), cal, ref(rr), C.byref(self.vs), ref(term_head), ref(cost_head),
                                              model_handle, int(task_id), int(ensemble), d_elite, _lib.current_stream()),
                   "cmbpo_replay_run_votes")

    def run(self, model_handle, task_id, ensemble, elite, term_head=None, cost_head=None, reliability=True):
        """The narrowest run entry that can express the call.  ``cmbpo_replay_run``; elite: [H, B] int32 device tensor.
        term_head: a ``_lib.TermHeadStruct`` -- the learned termination head in the post step (``cmbpo_replay_run_term``).
        cost_head: a ``_lib.CostHeadStruct`` -- the reading of the learned-cost column (``cmbpo_replay_run_cost``).  Buffers built
        with ``reliability=`` go through ``cmbpo_replay_run_reliab`` (elite is copied into their own array) unless
        ``reliability=False``."""
        if self.rr is not None and reliability:
            return self._run_reliab(None, model_handle, task_id, ensemble, elite, term_head, cost_head)
        if cost_head is not None:
            _lib.check(_lib.lib().cmbpo_replay_run_cost(C.byref(self.rs), None, C.byref(term_head) if term_head is not None else None,
                                                        C.byref(cost_head), model_handle, int(task_id), int(ensemble),
                                                        elite.data_ptr(), _lib.current_stream()), "cmbpo_replay_run_cost")
            return
        if term_head is not None:
            _lib.check(_lib.lib().cmbpo_replay_run_term(C.byref(self.rs), None, C.byref(term_head), model_handle, int(task_id),
                                                        int(ensemble), elite.data_ptr(), _lib.current_stream()),
                       "cmbpo_replay_run_term")
            return
        _lib.check(_lib.lib().cmbpo_replay_run(C.byref(self.rs), model_handle, int(task_id), int(ensemble), elite.data_ptr(),
                                               _lib.current_stream()), "cmbpo_replay_run")

    def table(self):
        return table(self.t["sums"].cpu().numpy(), self.t["counts"].cpu().numpy(), self.obs_dim)

    # -- predictive calibration (calibration=True) ---------------------------------------------------------------------
    def _calib(self):
        if self.cs is None:
            raise ValueError("replay: these buffers were built with calibration=False")
        return C.byref(self.cs)

    def set_elite(self, elite):
        """The member of every window at every step, [H, B] (what ``calibrate``, ``reliab`` and the runs with either read)."""
        if self.elite is None:
            self._calib()
        self.elite.copy_(_as(elite, torch.int32, self.device).reshape(self.H, self.B))

    def calibrate(self, h):
        """``cmbpo_replay_calibrate``: call it BEFORE ``compare(h)``, which clears ``alive`` and overwrites ``cur_obs``."""
        _lib.check(_lib.lib().cmbpo_replay_calibrate(C.byref(self.rs), self._calib(), int(h), _lib.current_stream()),
                   "cmbpo_replay_calibrate")

    def calib_finish(self):
        _lib.check(_lib.lib().cmbpo_replay_calib_finish(C.byref(self.rs), self._calib(), _lib.current_stream()),
                   "cmbpo_replay_calib_finish")

    def run_calibrated(self, model_handle, task_id, ensemble, elite=None, term_head=None, cost_head=None, reliability=True):
        """``cmbpo_replay_run_calibrated``; elite: [H, B] members (None: those of the last ``set_elite``).  term_head,
        cost_head, reliability: as in ``run``."""
        if self.rr is not None and reliability:
            return self._run_reliab(self._calib(), model_handle, task_id, ensemble, elite, term_head, cost_head)
        if elite is not None:
            self.set_elite(elite)
        if cost_head is not None:
            _lib.check(_lib.lib().cmbpo_replay_run_cost(C.byref(self.rs), self._calib(),
                                                        C.byref(term_head) if term_head is not None else None, C.byref(cost_head),
                                                        model_handle, int(task_id), int(ensemble), None, _lib.current_stream()),
                       "cmbpo_replay_run_cost")
            return
        if term_head is not None:
            _lib.check(_lib.lib().cmbpo_replay_run_term(C.byref(self.rs), self._calib(), C.byref(term_head), model_handle,
                                                        int(task_id), int(ensemble), None, _lib.current_stream()),
                       "cmbpo_replay_run_term")
            return
        _lib.check(_lib.lib().cmbpo_replay_run_calibrated(C.byref(self.rs), self._calib(), model_handle, int(task_id),
                                                          int(ensemble), _lib.current_stream()), "cmbpo_replay_run_calibrated")

    def calibration_table(self):
        self._calib()
        return calibration_table(self.c["sums"].cpu().numpy(), self.c["counts"].cpu().numpy(), self.obs_dim)

    # -- reliability of the logistic columns (reliability=dict(...)) ---------------------------------------------------
    def _reliab(self):
        if self.rr is None:
            raise ValueError("replay: these buffers were built with reliability=None")
        return C.byref(self.rr)

    def reliab(self, h):
        """``cmbpo_replay_reliab``: call it BEFORE ``compare(h)``, which clears ``alive`` and overwrites ``cur_obs``."""
        _lib.check(_lib.lib().cmbpo_replay_reliab(C.byref(self.rs), self._reliab(), int(h), _lib.current_stream()),
                   "cmbpo_replay_reliab")

    def reliab_finish(self):
        _lib.check(_lib.lib().cmbpo_replay_reliab_finish(C.byref(self.rs), self._reliab(), _lib.current_stream()),
                   "cmbpo_replay_reliab_finish")

    def reliability_table(self):
        self._reliab()
        return reliability_table(self.r["sums"].cpu().numpy(), self.r["counts"].cpu().numpy(), self.n_bins, self.rel_names,
                                 edges=self.rel_edges)

    # -- the static rules' votes (votes=dict(...)) ---------------------------------------------------------------------
    def _votes(self):
        if self.vs is None:
            raise ValueError("replay: these buffers were built with votes=None")
        return C.byref(self.vs)

    def votes(self, h):
        """``cmbpo_replay_votes``: call it BEFORE ``compare(h)``, behind the step's ``cmbpo_fakeenv_post_votes``."""
        rv = self._votes()
        _lib.check(_lib.lib().cmbpo_replay_votes(C.byref(self.rs), rv, int(h), _lib.current_stream()), "cmbpo_replay_votes")

    def votes_finish(self):
        rv = self._votes()
        _lib.check(_lib.lib().cmbpo_replay_votes_finish(C.byref(self.rs), rv, _lib.current_stream()), "cmbpo_replay_votes_finish")

    def votes_table(self):
        self._votes()
        return votes_table(self.v["counts"].cpu().numpy(), self.vote_ensemble, self.learned_cost)


def table(sums, counts, obs_dim):
    """The result dict from the raw ``sums`` [H, obs + 4] (float64) and ``counts`` [H, 10] (int64): means over the rows
    summed at each horizon (NaN where there were none) next to the sums and counts they were divided from."""
    sums, counts = np.asarray(sums, np.float64), np.asarray(counts, np.int64)
    H, D = sums.shape[0], int(obs_dim)
    n = counts[:, 0].copy()
    out = dict(n=n, n_nonfinite=counts[:, 1].copy(), se_obs=sums[:, :D].copy(),
               cost_cm=counts[:, 2:6].reshape(H, 2, 2).copy(), term_cm=counts[:, 6:10].reshape(H, 2, 2).copy())
    for j, k in enumerate(SUM_KEYS):
        out[k] = sums[:, D + j].copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        den = np.where(n > 0, n, 1).astype(np.float64)
        nan = np.where(n > 0, 0.0, np.nan)
        out["mse_obs"] = out["se_obs"] / den[:, None] + nan[:, None]
        out["mse_rew"] = out["se_rew"] / den + nan
        out["mse_cost"] = out["se_cost"] / den + nan
        out["ep_var_mean"] = out["sum_ep_var"] / den + nan
        out["dkl_mean"] = out["sum_dkl"] / den + nan
    return out


def calibration_table(sums, counts, obs_dim):
    """The calibration dict from the raw ``sums`` [H, 6 (obs + 1)] (float64) and ``counts`` [H, 4 (obs + 1) + 2] (int64).
    Column c < obs is observation column c, column obs the reward.  ``n`` / ``n_skipped`` [H]: the rows that entered / that the
    plain table sums and this one rejects.  Per horizon and column, [H, obs + 1]: ``z2_al`` / ``z2_tot`` the mean squared
    standardised error against the elite member's variance / the moment-matched mixture's (1 when calibrated; the maximum-
    likelihood temperature of that variance), ``nll_*`` = 0.5 (log 2 pi + mean log v + z2), ``cover1_*`` / ``cover2_*`` the
    share of errors inside one / two sigma (0.6827 / 0.9545 when calibrated), ``al_var`` / ``ep_var`` the means of the members'
    mean variance and of the variance of their means, in the column's own units -- and the raw sums and counts
    (``CALIB_SUM_KEYS``, ``CALIB_COUNT_KEYS``).  NaN means where ``n == 0``.  In ``open_loop`` mode only horizon 0 is a
    one-step prediction: later rows show how far the one-step variance falls short of the compounded error."""
    sums, counts = np.asarray(sums, np.float64), np.asarray(counts, np.int64)
    H, Cc = sums.shape[0], int(obs_dim) + 1
    ks, kc = _lib.REPLAY_CALIB_SUMS, _lib.REPLAY_CALIB_COUNTS
    ns, nc = calib_sizes(int(obs_dim))
    if sums.shape != (H, ns) or counts.shape != (H, nc):
        raise ValueError("calibration_table: sums [H, %d] and counts [H, %d] expected for obs_dim %d, got %s and %s"
                         % (ns, nc, obs_dim, sums.shape, counts.shape))
    s, c = sums.reshape(H, ks, Cc), counts[:, :kc * Cc].reshape(H, kc, Cc)
    n = counts[:, kc * Cc].copy()
    out = dict(n=n, n_skipped=counts[:, kc * Cc + 1].copy())
    for j, k in enumerate(CALIB_SUM_KEYS):
        out[k] = s[:, j].copy()
    for j, k in enumerate(CALIB_COUNT_KEYS):
        out[k] = c[:, j].copy()
    den = np.where(n > 0, n, 1).astype(np.float64)[:, None]
    nan = np.where(n > 0, 0.0, np.nan)[:, None]
    mean = lambda k: out[k] / den + nan
    log2pi = np.log(2.0 * np.pi)
    for which in ("al", "tot"):
        out["z2_" + which] = mean("sum_z2_" + which)
        out["nll_" + which] = 0.5 * (log2pi + mean("sum_log_v_" + which) + out["z2_" + which])
        out["cover1_" + which] = mean("n_cover1_" + which)
        out["cover2_" + which] = mean("n_cover2_" + which)
    out["al_var"], out["ep_var"] = mean("sum_v_bar"), mean("sum_s2")
    return out


def temperature(cal, which="al", horizon=0, lo=0.25, hi=4.0):
    """The variance temperature per observation column, [obs] float32: ``clip(z2_<which>[horizon, :obs], lo, hi)``, 1.0 where
    the table has no value (NaN).  Its square root scales a standard deviation."""
    if which not in ("al", "tot"):
        raise ValueError("temperature: which is 'al' or 'tot', got %r" % (which,))
    lo, hi = float(lo), float(hi)
    if not (0.0 < lo <= hi and np.isfinite(hi)):
        raise ValueError("temperature: 0 < lo <= hi < inf expected, got %r, %r" % (lo, hi))
    z2 = np.asarray(cal["z2_" + which], np.float64)[int(horizon), :-1]
    return np.where(np.isnan(z2), 1.0, np.clip(z2, lo, hi)).astype(np.float32)


def default_edges(n_bins):
    """The bin edges of ``n_bins`` equal-width PROBABILITY bins, in logit space: ``float32(logit(k / n_bins))``, k = 1 ..
    n_bins - 1 (the logarithm in float64, one rounding to float32)."""
    q = np.arange(1, int(n_bins), dtype=np.float64) / float(n_bins)
    return np.log(q / (1.0 - q)).astype(np.float32)


def reliability_table(sums, counts, n_bins, names, edges=None):
    """The reliability dict from the raw ``sums`` [H, 2 C (2 K + 2)] (float64) and ``counts`` [H, 4 C K + 2 C] (int64) of C =
    ``len(names)`` columns and K = ``n_bins`` bins: ``{name: column}``.  A column holds ``n_rel`` / ``n_skipped`` [H] (the rows
    that entered / that the plain table sums and this column rejects), ``edges`` and, under ``'elite'`` and ``'pooled'`` (the
    elite member's logit / the members' mean logit), the raw ``n``, ``pos``, ``sum_p``, ``sum_z`` [H, K], ``sum_brier``,
    ``sum_logloss`` [H] and what follows from them: per bin ``conf = sum_p / n`` (what the column said), ``freq = pos / n`` (what
    happened), ``zbar = sum_z / n``; per horizon ``ece = sum_k (n_k / N) |conf_k - freq_k|`` and ``mce`` (its largest gap) over
    the non-empty bins, ``brier``, ``logloss``, ``base_rate = pos / N`` and ``mean_p``.  NaN where ``n == 0``."""
    sums, counts = np.asarray(sums, np.float64), np.asarray(counts, np.int64)
    H, K, Cn = sums.shape[0], int(n_bins), len(names)
    ns, nc = reliab_sizes(K, Cn)
    if sums.shape != (H, ns) or counts.shape != (H, nc):
        raise ValueError("reliability_table: sums [H, %d] and counts [H, %d] expected for %d columns of %d bins, got %s and %s"
                         % (ns, nc, Cn, K, sums.shape, counts.shape))
    s = sums.reshape(H, Cn, 2, 2 * K + 2)
    c = counts[:, :4 * Cn * K].reshape(H, Cn, 2, 2 * K)
    tail = counts[:, 4 * Cn * K:].reshape(H, Cn, 2)
    out = {}
    for j, name in enumerate(names):
        col = dict(n_rel=tail[:, j, 0].copy(), n_skipped=tail[:, j, 1].copy(),
                   edges=None if edges is None else np.asarray(edges, np.float32).copy())
        for r, reading in enumerate(READINGS):
            n, pos = c[:, j, r, :K].copy(), c[:, j, r, K:].copy()
            d = dict(n=n, pos=pos, sum_p=s[:, j, r, :K].copy(), sum_z=s[:, j, r, K:2 * K].copy(),
                     sum_brier=s[:, j, r, 2 * K].copy(), sum_logloss=s[:, j, r, 2 * K + 1].copy())
            N = n.sum(axis=1)
            with np.errstate(divide="ignore", invalid="ignore"):
                nf, Nf = n.astype(np.float64), N.astype(np.float64)
                d["conf"], d["freq"], d["zbar"] = d["sum_p"] / nf, pos / nf, d["sum_z"] / nf
                gap = np.where(n > 0, np.abs(d["conf"] - d["freq"]), 0.0)
                nan = np.where(N > 0, 0.0, np.nan)
                d["ece"] = (nf * gap).sum(axis=1) / Nf + nan
                d["mce"] = gap.max(axis=1) + nan
                d["brier"], d["logloss"] = d["sum_brier"] / Nf + nan, d["sum_logloss"] / Nf + nan
                d["base_rate"], d["mean_p"] = pos.sum(axis=1) / Nf + nan, d["sum_p"].sum(axis=1) / Nf + nan
            col[reading] = d
        out[name] = col
    return out


def logit_offset(rel, column, reading="elite", horizon=0, lo=-2.0, hi=2.0, min_n=100):
    """The logit offset b that makes the column's mean probability the observed rate at one horizon of a reliability table:
    the root of ``sum_k n_k sigma(zbar_k - b) = sum_k pos_k`` over the non-empty bins, by 100 bisections of [-30, 30] in float64,
    clipped to [lo, hi].  ``None`` where fewer than ``min_n`` rows entered (keep what you had).  This is calibration-in-the-
    large THROUGH THE BIN MEANS -- every row of a bin stands at the bin's mean logit --, not an exact per-row solve; no positives
    give ``hi``, only positives ``lo``.  Subtract b from the logit: ``sigma(z - b)``."""
    if reading not in READINGS:
        raise ValueError("logit_offset: reading is 'elite' or 'pooled', got %r" % (reading,))
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
        raise ValueError("logit_offset: finite lo <= hi expected, got %r, %r" % (lo, hi))
    d = rel[column][reading]
    n, pos = np.asarray(d["n"])[int(horizon)], np.asarray(d["pos"])[int(horizon)]
    N = int(n.sum())
    if N < max(int(min_n), 1):
        return None
    keep = n > 0
    nk, zk, want = n[keep].astype(np.float64), np.asarray(d["zbar"], np.float64)[int(horizon)][keep], float(pos.sum())
    a, b = -30.0, 30.0
    for _ in range(100):
        mid = 0.5 * (a + b)
        if float((nk / (1.0 + np.exp(-(zk - mid)))).sum()) > want:       # too many predicted: a larger offset
            a = mid
        else:
            b = mid
    return float(min(max(0.5 * (a + b), lo), hi))


def check_particles(S):
    """S as the particle kernel takes it: a power of two in 2..64 (ValueError in words otherwise)."""
    if isinstance(S, bool) or int(S) != S or not (2 <= int(S) <= _lib.REPLAY_PARTICLES_MAX and (int(S) & (int(S) - 1)) == 0):
        raise ValueError("replay: particles must be a power of two in 2..%d (the particles of a window are lanes of one wave), "
                         "got %r" % (_lib.REPLAY_PARTICLES_MAX, S))
    return int(S)


class ParticleBuffers(_Buffers):
    """The device arrays of a particle replay (``cmbpo_replay_particles_t``): B windows of S particles, stepped as
    R = B S rows, particle p of window b in row ``b * S + p``.  A sibling of ``ReplayBuffers`` with arrays of its own -- the
    plain replay's are not touched."""

    def __init__(self, S, obs0, actions, next_obs, rewards, costs, terminals, lengths=None, mode="open_loop", ensemble=0,
                 out_dim=0, noise=None, device="cuda"):
        """obs0 [B, obs]; actions [H, B, act]; next_obs [H, B, obs]; rewards / costs / terminals [H, B]; lengths [B] in 1..H
        (None: H) -- as ``ReplayBuffers`` takes them.  noise: [H, B, S, obs] (or [H, B S, obs]) float32 N(0, 1) draws, needed by
        ``run`` only.  ``ensemble`` / ``out_dim`` > 0 also allocate the forward's scratch for R rows.  The recorded actions are
        expanded to the R rows on the device."""
        if mode not in MODES:      # (ahead of S, as it has always been)
            raise ValueError("replay mode: 'open_loop' or 'one_step', got %r" % (mode,))
        S = check_particles(S)
        dev = torch.device(device)
        H, B, D, A, w = _windows(obs0, actions, next_obs, rewards, costs, terminals, lengths, mode, dev, _lib.REPLAY_PARTICLES_MAX_OBS)
        obs0, R = w.pop("obs0"), B * S
        self.device, self.mode, self.S = dev, mode, S
        f32, u8 = torch.float32, torch.uint8
        self.B, self.H, self.R, self.obs_dim, self.act_dim = B, H, R, D, A
        self.n_part = _lib.lib().cmbpo_replay_particles_parts(B, S)
        f = dict(dtype=f32, device=dev)
        self.t = dict(w, act=w["act"].repeat_interleave(S, dim=1).contiguous(),
                      cur_obs=obs0.repeat_interleave(S, dim=0).contiguous(), alive=torch.ones(R, dtype=u8, device=dev),
                      p_next_obs=torch.empty((R, D), **f), p_rew=torch.empty(R, **f), p_term=torch.empty(R, dtype=u8, device=dev),
                      p_cost=torch.empty(R, **f), p_dkl_path=torch.empty(R, **f), p_ep_var_mean=torch.empty(R, **f),
                      **_table(H, self.n_part, *particle_sizes(D, S), dev))
        if noise is not None:
            xi = _as(noise, f32, dev)
            if xi.numel() != H * R * D or xi.shape[0] != H or xi.shape[-1] != D:
                raise ValueError("replay: particle noise must be [%d, %d, %d, %d], got %s" % (H, B, S, D, tuple(xi.shape)))
            self.t["xi"] = xi.reshape(H, R, D)
        if ensemble > 0:
            self.t["mean"] = torch.empty((ensemble, R, out_dim), **f)
            self.t["var"] = torch.empty_like(self.t["mean"])
        ps = _lib.ReplayParticlesStruct()
        ps.B, ps.H, ps.S, ps.obs_dim, ps.act_dim, ps.mode, ps.reserved, ps.reserved2 = B, H, S, D, A, MODES[mode], 0, 0
        for k, v in self.t.items():
            setattr(ps, k, v.data_ptr() if v.numel() else None)
        self.ps = ps

    def particles(self, h):
        _lib.check(_lib.lib().cmbpo_replay_particles(C.byref(self.ps), int(h), _lib.current_stream()), "cmbpo_replay_particles")

    def finish(self):
        _lib.check(_lib.lib().cmbpo_replay_particles_finish(C.byref(self.ps), _lib.current_stream()),
                   "cmbpo_replay_particles_finish")

    def run(self, model_handle, task_id, ensemble, elite, term_head=None, cost_head=None):
        """``cmbpo_replay_run_particles``; elite: [H, R] int32 device tensor, the member of every row at every step."""
        ref = lambda s: C.byref(s) if s is not None else None
        _lib.check(_lib.lib().cmbpo_replay_run_particles(C.byref(self.ps), ref(term_head), ref(cost_head), model_handle, int(task_id),
                                                         int(ensemble), _lib.ptr(elite), _lib.current_stream()),
                   "cmbpo_replay_run_particles")

    def table(self):
        return particles_table(self.t["sums"].cpu().numpy(), self.t["counts"].cpu().numpy(), self.obs_dim, self.S)


def particles_table(sums, counts, obs_dim, S):
    """The particle dict from the raw ``sums`` [H, 4 C + 2] (float64) and ``counts`` [H, C (S + 1) + 2] (int64) of C = obs_dim + 1
    columns (the observation columns, then the reward) and S particles per window.  ``n`` / ``n_nonfinite`` [H]: the windows
    held against their particles / that went non-finite at the horizon; ``S``.  Per horizon and column, [H, C]: ``rank_hist``
    [H, C, S + 1] (windows by the number of particles strictly below the recorded value), ``rank_freq`` = rank_hist / n,
    ``rank_dev = 0.5 sum_k |freq_k - 1 / (S + 1)|`` (the total-variation distance from the flat histogram of a calibrated cloud),
    ``outlier_rate = freq_0 + freq_S`` (the recording outside the cloud; 2 / (S + 1) when calibrated, more when the cloud is too
    narrow), ``chi2 = sum_k (hist_k - n / (S + 1))^2 / (n / (S + 1))`` (S degrees of freedom), ``mae`` (mean absolute error of a
    particle), ``crps = mean(a - g / 2)`` (the fair CRPS of the S-particle ensemble), ``spread`` (mean unbiased variance of the
    particles), ``mse_mean`` (squared error of the particle mean), ``spread_skill = sqrt((S + 1) / S * spread / mse_mean)`` (1 when
    calibrated).  Per horizon: ``brier_term`` / ``brier_cost`` (the particles' share of predicted terminations / mean predicted
    cost against the recorded flag).  And the raw ``sum_abs``, ``sum_pair``, ``sum_se``, ``sum_var`` [H, C], ``sum_brier_term``,
    ``sum_brier_cost`` [H].  A horizon with ``n == 0`` has NaN means and zero counts.  The reward column carries no transition
    noise by design: its histogram shows the member and state spread only."""
    sums, counts = np.asarray(sums, np.float64), np.asarray(counts, np.int64)
    S = check_particles(S)
    H, Cc = sums.shape[0], int(obs_dim) + 1
    ns, nc = particle_sizes(int(obs_dim), S)
    if sums.shape != (H, ns) or counts.shape != (H, nc):
        raise ValueError("particles_table: sums [H, %d] and counts [H, %d] expected for obs_dim %d and S %d, got %s and %s"
                         % (ns, nc, obs_dim, S, sums.shape, counts.shape))
    hist = counts[:, :Cc * (S + 1)].reshape(H, Cc, S + 1).copy()
    n = counts[:, Cc * (S + 1)].copy()
    s = sums[:, :4 * Cc].reshape(H, 4, Cc)
    out = dict(n=n, n_nonfinite=counts[:, Cc * (S + 1) + 1].copy(), S=S, rank_hist=hist,
               sum_abs=s[:, 0].copy(), sum_pair=s[:, 1].copy(), sum_se=s[:, 2].copy(), sum_var=s[:, 3].copy(),
               sum_brier_term=sums[:, 4 * Cc].copy(), sum_brier_cost=sums[:, 4 * Cc + 1].copy())
    den = np.where(n > 0, n, 1).astype(np.float64)
    nan = np.where(n > 0, 0.0, np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        freq = hist / den[:, None, None] + nan[:, None, None]
        flat = 1.0 / (S + 1)
        expect = den[:, None, None] * flat
        out["rank_freq"] = freq
        out["rank_dev"] = 0.5 * np.abs(freq - flat).sum(axis=2)
        out["outlier_rate"] = freq[:, :, 0] + freq[:, :, S]
        out["chi2"] = ((hist - expect) ** 2 / expect).sum(axis=2) + nan[:, None]
        out["mae"] = out["sum_abs"] / den[:, None] + nan[:, None]
        out["crps"] = (out["sum_abs"] - 0.5 * out["sum_pair"]) / den[:, None] + nan[:, None]
        out["spread"] = out["sum_var"] / den[:, None] + nan[:, None]
        out["mse_mean"] = out["sum_se"] / den[:, None] + nan[:, None]
        out["spread_skill"] = np.sqrt((S + 1.0) / S * out["spread"] / out["mse_mean"])
        out["brier_term"] = out["sum_brier_term"] / den + nan
        out["brier_cost"] = out["sum_brier_cost"] / den + nan
    return out


VOTE_SIGNALS = ("cost", "term")      # signal 0 / 1 of the vote table's histogram


def votes_table(counts, E, learned_cost=False):
    """The vote dict from the raw ``counts`` [H, 38] (int64: ``hist_cost`` [9, 2] | ``hist_term`` [9, 2] | ``n_vote`` |
    ``n_skipped``) of an ensemble of ``E`` members: ``n_vote`` / ``n_skipped`` [H] (the rows that entered / whose vote count lay
    above E) and, per signal -- ``'cost'`` (not under ``learned_cost``) and ``'term'`` --, ``hist`` [H, E + 1, 2] indexed [votes,
    recorded flag], ``n`` [H], ``conf`` [E + 1] = v / E (what the share says), ``freq`` [H, E + 1] (how often the flag was set
    among the rows with v votes), ``ece = sum_v n_v / n |v / E - freq_v|`` and ``mce`` (its largest gap) over the non-empty vote
    counts, ``brier = sum_v (n_v0 (v / E)^2 + n_v1 (1 - v / E)^2) / n``, ``base_rate``, ``mean_share``, ``split_rate`` (the
    share of rows with 0 < v < E: where the modes can differ at all) and ``cm['any']`` / ``cm['majority']`` [H, 2, 2] indexed
    [real, predicted]: the 2x2 counts of ``v > 0`` and of ``2 v > E``.  Float64 from exact integers; a horizon with ``n == 0``
    has NaN rates and zero counts."""
    counts = np.asarray(counts, np.int64)
    E, S = int(E), _lib.REPLAY_VOTE_SLOTS
    if counts.ndim != 2 or counts.shape[1] != _lib.REPLAY_VOTE_COUNTS:
        raise ValueError("votes_table: counts [H, %d] expected, got %s" % (_lib.REPLAY_VOTE_COUNTS, counts.shape))
    if not 1 <= E <= _lib.REPLAY_VOTES_MAX_ENSEMBLE:
        raise ValueError("votes_table: E must lie in 1..%d, got %d" % (_lib.REPLAY_VOTES_MAX_ENSEMBLE, E))
    H = counts.shape[0]
    full = counts[:, :4 * S].reshape(H, 2, S, 2)
    if full[:, :, E + 1:].any():
        raise ValueError("votes_table: counts hold rows with more than E = %d votes" % E)
    out = dict(n_vote=counts[:, 4 * S].copy(), n_skipped=counts[:, 4 * S + 1].copy())
    v = np.arange(E + 1, dtype=np.float64)
    conf = v / float(E)
    for j, name in enumerate(VOTE_SIGNALS):
        if name == "cost" and learned_cost:
            continue
        hist = full[:, j, :E + 1].copy()
        nv = hist.sum(axis=2)                                   # [H, E + 1]
        n = nv.sum(axis=1)
        hf, nvf, nf = hist.astype(np.float64), nv.astype(np.float64), n.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            nan = np.where(n > 0, 0.0, np.nan)
            freq = hf[:, :, 1] / nvf
            gap = np.where(nv > 0, np.abs(conf[None] - freq), 0.0)
            d = dict(hist=hist, n=n, conf=conf.copy(), freq=freq, ece=(nvf * gap).sum(axis=1) / nf + nan, mce=gap.max(axis=1) + nan,
                     brier=(hf[:, :, 0] * conf[None] ** 2 + hf[:, :, 1] * (1.0 - conf[None]) ** 2).sum(axis=1) / nf + nan,
                     base_rate=hf[:, :, 1].sum(axis=1) / nf + nan, mean_share=(nvf * conf[None]).sum(axis=1) / nf + nan,
                     split_rate=nvf[:, 1:E].sum(axis=1) / nf + nan)
        cm = {}
        for mode, hit in (("any", v > 0), ("majority", 2 * v > E)):
            m = np.zeros((H, 2, 2), np.int64)
            m[:, :, 1] = hist[:, hit].sum(axis=1)               # [real][pred = 1]
            m[:, :, 0] = hist[:, ~hit].sum(axis=1)
            cm[mode] = m
        d["cm"] = cm
        out[name] = d
    return out
