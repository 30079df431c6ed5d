"""CPOBuffer -- host-side mirror of ``buffers/cpobuffer.py:15-534`` (the real-env on-policy buffer).

Real-env samples arrive one at a time from a serial MuJoCo step on the host, so storage stays in host NumPy
arrays (as in the reference); the arithmetic of the path runs in HIP behind the C-ABI:

  * ``finish_path`` (``cpobuffer.py:179-207``): reward + cost GAE of the finished path -> ``cmbpo_gae_segments``
    (float64 ``lfilter`` recurrence, float32 stores, float64 deltas when the bootstrap is the float64 zeros
    of ``samplers/cpo_sampler.py:205-212`` -- NumPy's promotion in ``np.append``);
  * ``get`` (``cpobuffer.py:249-290``): advantage normalisation / cost-advantage centring -> ``cmbpo_adv_normalize``,
    then the reference's 12-array list ``[obs, act, adv, cadv, ret, cret, logp, val, cval, cost, log_std, mu]``
    truncated to ``ptr`` and a dump into the off-policy archive.

The archive accessors the trainer uses for start-state sampling (``epoch_batch``, ``boltz_dist``,
``distributed_batch_from_archive``, ``algorithms/cmbpo.py:241-245``) are kept as thin NumPy index plumbing, as the
reference has them.  The same chain also runs on the device: ``enable_device_archive``
keeps a device mirror of the four archive columns it reads (observations, mu, log_std, epochs), appended to by
``dump_to_archive``, and ``sample_start_states`` draws the start states of a rollout round from it with the kernels of
``csrc/start_states.hip`` -- per-epoch uniform draw, per-epoch policy KL, Boltzmann CDF, inverse-CDF draw written into
the rollout state -- without a host copy of any batch-sized array.  The mirror is opt-in: nothing is allocated or
written until it is enabled, and the host archive and the NumPy random stream of the accessors above are untouched.
"""
import warnings

import numpy as np
import torch

from . import _lib

EPS = 1e-8  # utilities/utils.py:19

_SCALARS = ("advantages", "rewards", "returns", "values", "cadvantages", "costs", "creturns", "cvalues", "log_probs")


class CPOBuffer:
    def __init__(self, size, archive_size, observation_space, action_space, device=None, *args, **kwargs):
        self.obs_shape = tuple(observation_space.shape)
        self.act_shape = tuple(action_space.shape)
        self.archive_size = int(archive_size)
        self.max_size = int(size)
        self.device = torch.device(device if device is not None else "cuda")
        self.pi_info_shapes = None
        self.gamma, self.lam, self.cost_gamma, self.cost_lam = 0.99, 0.95, 0.99, 0.95
        self._dev = None              # device mirror of the archive (enable_device_archive)
        self.reset_buffers()
        self.reset_arch()

    # -- storage --------------------------------------------------------------------------------------------
    def _new(self, n, with_pi=True):
        d = {"observations": np.zeros((n,) + self.obs_shape, np.float32),
             "actions": np.zeros((n,) + self.act_shape, np.float32),
             "next_observations": np.zeros((n,) + self.obs_shape, np.float32),
             "terminals": np.zeros(n, np.bool_)}
        for k in _SCALARS:
            d[k] = np.zeros(n, np.float32)
        return d

    def reset_buffers(self):
        """cpobuffer.py:99-117."""
        self.buf_dict = self._new(self.max_size)
        self.buf_dict["epochs"] = np.ones(self.max_size, np.float32) * -1
        if self.pi_info_shapes:
            self.pi_info_bufs = {k: np.zeros([self.max_size] + list(v), np.float32)
                                 for k, v in self.pi_info_shapes.items()}
            self.buf_dict["pi_infos"] = self.pi_info_bufs
        self.ptr, self.path_start_idx, self.path_finished = 0, 0, False

    def reset_arch(self):
        """cpobuffer.py:119-138."""
        self.archive_full = False
        self.arch_dict = self._new(self.archive_size)
        self.arch_dict["epochs"] = np.ones(self.archive_size, np.int64) * -1
        if self.pi_info_shapes:
            self.pi_info_archive = {k: np.zeros([self.archive_size] + list(v), np.float32)
                                    for k, v in self.pi_info_shapes.items()}
            self.arch_dict["pi_infos"] = self.pi_info_archive
        self.archive_ptr = 0
        self.max_pointer = 0
        if self._dev is not None:
            for k, t in self._dev.items():
                t.fill_(-1) if k == "epochs" else t.zero_()
            self._dev_version += 1

    def initialize(self, pi_info_shapes, gamma=0.99, lam=0.95, cost_gamma=0.99, cost_lam=0.95):
        """cpobuffer.py:79-97."""
        self.pi_info_shapes = pi_info_shapes
        self.pi_info_bufs = {k: np.zeros([self.max_size] + list(v), np.float32) for k, v in pi_info_shapes.items()}
        self.pi_info_archive = {k: np.zeros([self.archive_size] + list(v), np.float32)
                                for k, v in pi_info_shapes.items()}
        self.buf_dict["pi_infos"] = self.pi_info_bufs
        self.arch_dict["pi_infos"] = self.pi_info_archive
        self.sorted_pi_info_keys = sorted(pi_info_shapes.keys())
        self.gamma, self.lam, self.cost_gamma, self.cost_lam = gamma, lam, cost_gamma, cost_lam
        if self._dev is not None:       # (the pi_info archives were just replaced)
            self._dev = None
            self.enable_device_archive()

    # convenient views with the reference's attribute names
    @property
    def epoch_archive(self):
        return self.arch_dict["epochs"]

    @property
    def size(self):
        return self.ptr

    @property
    def arch_size(self):
        return self.max_pointer

    @property
    def max_ep(self):
        return int(np.max(self.epoch_archive))

    @property
    def min_ep(self):
        return int(np.min(self.epoch_archive[self.epoch_archive > -1]))

    @property
    def epochs_list(self):
        """cpobuffer.py:148-153: the epochs present in the archive."""
        return np.flatnonzero(np.bincount(self.epoch_archive[self.epoch_archive >= 0]))

    def store(self, obs, act, next_obs, rew, val, cost, cval, logp, pi_info, term, epoch):
        """cpobuffer.py:160-176."""
        assert self.ptr < self.max_size     # buffer has to have room so you can store
        b, p = self.buf_dict, self.ptr
        b["observations"][p], b["actions"][p], b["next_observations"][p] = obs, act, next_obs
        one = lambda x: np.asarray(x).reshape(-1)[0]     # the policy hands over batch-of-one arrays
        b["rewards"][p], b["values"][p], b["costs"][p], b["cvalues"][p] = one(rew), one(val), one(cost), one(cval)
        b["log_probs"][p], b["terminals"][p], b["epochs"][p] = one(logp), one(term), epoch
        for k in self.sorted_pi_info_keys:
            self.pi_info_bufs[k][p] = pi_info[k]
        self.ptr += 1
        self.path_finished = False

    # -- the path arithmetic (HIP) -----------------------------------------------------------------------------
    def finish_path(self, last_val=0, last_cval=0):
        """cpobuffer.py:179-207."""
        lo, hi = self.path_start_idx, self.ptr
        n = hi - lo
        b = self.buf_dict
        lv, lcv = np.asarray(last_val), np.asarray(last_cval)
        # np.append(float32 buffer, x): anything but a float32 bootstrap promotes the deltas to float64
        mask = (1 if lv.dtype != np.float32 else 0) | (2 if lcv.dtype != np.float32 else 0)
        if n > 0:
            dev = self.device
            with torch.cuda.device(dev):
                up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
                rew, val, cost, cval = (up(b[k][lo:hi]) for k in ("rewards", "values", "costs", "cvalues"))
                offs = torch.tensor([0, n], dtype=torch.int32, device=dev)
                lvd, lcvd = up(lv.reshape(-1)[:1]), up(lcv.reshape(-1)[:1])
                fm = torch.tensor([mask], dtype=torch.uint8, device=dev)
                out = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(4)]
                _lib.check(_lib.lib().cmbpo_gae_segments(
                    1, offs.data_ptr(), rew.data_ptr(), val.data_ptr(), cost.data_ptr(), cval.data_ptr(),
                    lvd.data_ptr(), lcvd.data_ptr(), fm.data_ptr(), float(self.gamma), float(self.lam),
                    float(self.cost_gamma), float(self.cost_lam), out[0].data_ptr(), out[1].data_ptr(),
                    out[2].data_ptr(), out[3].data_ptr(), _lib.current_stream()), "cmbpo_gae_segments")
                for k, t in zip(("advantages", "returns", "cadvantages", "creturns"), out):
                    b[k][lo:hi] = t.cpu().numpy()
        self.path_start_idx = self.ptr
        self.path_finished = True

    def dump_to_archive(self):
        """cpobuffer.py:210-248: copy the finished on-policy samples behind the archive pointer."""
        assert self.path_finished
        if self.archive_ptr >= self.archive_size - self.ptr:
            self.archive_full = True
            self.archive_ptr = 0
            warnings.warn('Archive is full, deleting old samples.')
        dst = slice(self.archive_ptr, self.archive_ptr + self.ptr)
        for k, a in self.arch_dict.items():
            if k == "pi_infos":
                for kk in self.sorted_pi_info_keys:
                    a[kk][dst] = self.pi_info_bufs[kk][:self.ptr]
            else:
                a[dst] = self.buf_dict[k][:self.ptr]
        if self._dev is not None:
            self._mirror(dst)
        self.archive_ptr += self.ptr
        self.max_pointer = max(self.archive_ptr, self.max_pointer)

    def get(self):
        """cpobuffer.py:249-290."""
        b, n = self.buf_dict, self.ptr
        if n > 0:
            dev = self.device
            with torch.cuda.device(dev):
                adv = torch.from_numpy(b["advantages"][:n].copy()).to(dev)
                cadv = torch.from_numpy(b["cadvantages"][:n].copy()).to(dev)
                stats = torch.zeros(16, dtype=torch.float64, device=dev)
                _lib.check(_lib.lib().cmbpo_adv_normalize(n, adv.data_ptr(), cadv.data_ptr(), stats.data_ptr(),
                                                         _lib.current_stream()), "cmbpo_adv_normalize")
                b["advantages"][:n] = adv.cpu().numpy()
                b["cadvantages"][:n] = cadv.cpu().numpy()
        self.dump_to_archive()
        keys = ["observations", "actions", "advantages", "cadvantages", "returns", "creturns", "log_probs", "values",
                "cvalues", "costs"]
        res = [b[k][:n].copy() for k in keys] + [self.pi_info_bufs[k][:n].copy() for k in self.sorted_pi_info_keys]
        diagnostics = dict(poolr_ret_mean=b["returns"][:n].mean(), poolr_cret_mean=b["creturns"][:n].mean())
        self.reset_buffers()
        return res, diagnostics

    # -- archive access (NumPy index plumbing; callers of the path) ----------------------------
    def _fields(self, fields):
        if fields is None:
            return ['observations', 'actions', 'next_observations', 'rewards', 'terminals'], False
        fields = list(fields)
        want_pi = 'pi_infos' in fields
        if 'all' in fields:
            return [k for k in self.arch_dict if k != 'pi_infos'], True
        return [f for f in fields if f != 'pi_infos'], want_pi

    def _take(self, idx, fields):
        names, want_pi = self._fields(fields)
        # ('path_lengths': derived from the path ends, not stored)
        out = {k: (self.path_lengths() if k == 'path_lengths' else self.arch_dict[k])[idx] for k in names}
        if want_pi:
            out.update({k: self.pi_info_archive[k][idx] for k in self.sorted_pi_info_keys})
        return out

    def get_archive(self, fields=None):
        return self._take(slice(0, self.arch_size), fields)

    def rand_batch_from_archive(self, batch_size, fields=None):
        idx = np.random.randint(0, self.arch_size, batch_size) if self.arch_size else np.arange(0, 0)
        return self._take(idx, fields)

    def boltz_dist(self, kls, alpha=1):
        """cpobuffer.py:385-396: per-sample probabilities, Boltzmann over the epochs' mean policy KL."""
        ep_probs = np.exp(alpha * np.negative(kls))
        ep_probs /= np.sum(ep_probs)
        ea = self.epoch_archive
        sample_p = np.bincount(ea[ea >= 0]).astype(np.float32)
        sample_p[sample_p > 0] = ep_probs / sample_p[sample_p > 0]
        return np.where(ea >= 0, sample_p[ea], 0)

    def distributed_batch_from_archive(self, batch_size, dist, fields=None):
        idx = np.random.choice(np.arange(self.archive_size), size=batch_size, p=dist)
        return self._take(idx, fields)

    def epoch_batch(self, batch_size, epochs, fields=None):
        assert len(np.shape(epochs)) == 1
        ep = np.array(epochs)
        if np.any(ep > self.max_ep) or np.any(ep < self.min_ep):
            print('Warning: epoch not contained in buffer.')
            return None
        idx = np.array([np.random.choice(np.flatnonzero(self.epoch_archive == e), size=batch_size) for e in epochs])
        return self._take(idx, fields)

    # -- windows of consecutive real steps for FakeEnv.replay (open-loop model validation) --------------
    def path_continues(self):
        """bool [arch_size]: archive step i continues into step i + 1.  The archive stores no path boundaries, so this test
        is the boundary: ``terminals[i]`` is False, ``next_observations[i]`` equals ``observations[i + 1]`` in every column
        bit for bit, i + 1 is a filled slot, and -- once the archive has wrapped -- the pair does not straddle
        ``archive_ptr`` (the newest sample in front of it, the oldest behind it)."""
        N = self.arch_size
        cont = np.zeros(N, np.bool_)
        if N > 1:
            a = self.arch_dict
            nxt = np.ascontiguousarray(a["next_observations"][:N - 1]).reshape(N - 1, -1).view(np.uint32)
            obs = np.ascontiguousarray(a["observations"][1:N]).reshape(N - 1, -1).view(np.uint32)
            cont[:N - 1] = ~a["terminals"][:N - 1] & (nxt == obs).all(axis=1)
        if self.archive_full and 0 < self.archive_ptr <= N:
            cont[self.archive_ptr - 1] = False
        return cont

    def path_lengths(self):
        """int32 [archive_size]: the number of steps of the real path every archived step belongs to (0 in unfilled slots),
        from the path ends of ``path_continues``.  Once the archive has wrapped, the oldest path -- the one behind
        ``archive_ptr`` -- may have lost its first steps to newer samples: its length is not known and reported as the
        largest int32, so that no test ``length < horizon`` holds for it."""
        N = self.arch_size
        out = np.zeros(self.archive_size, np.int32)
        if N == 0:
            return out
        ends = np.flatnonzero(~self.path_continues())            # the last step of every path (slot N - 1 is always one)
        starts = np.concatenate(([0], ends[:-1] + 1))
        out[:N] = np.repeat((ends - starts + 1).astype(np.int32), ends - starts + 1)
        if self.archive_full and 0 < self.archive_ptr < N:
            k = np.searchsorted(ends, self.archive_ptr)           # the path that starts behind the newest sample
            out[starts[k]:ends[k] + 1] = np.iinfo(np.int32).max
        return out

    def term_targets(self, horizon):
        """float32 [archive_size]: the training target of a learned termination head -- 1 only where the
        environment reported ``done`` on a path shorter than the sampler's ``horizon``.  A path that ran to the horizon ended
        by time-out, which is no property of the state: target 0, even when the environment's own time limit set ``done`` on
        that step.  ``terminals`` itself is not changed."""
        return (self.arch_dict["terminals"] & (self.path_lengths() < int(horizon))).astype(np.float32)

    def windows(self, horizon, n, epochs=None, rng=None):
        """``n`` windows of up to ``horizon`` consecutive archived steps, for ``FakeEnv.replay``.  Start indices are drawn
        uniformly, with replacement, from the filled slots (``epochs``: only from slots tagged with one of these epochs)
        with ``rng`` (a ``numpy.random.Generator``; None: a fresh one -- NumPy's global stream is never touched).  A window
        runs to the end of its path (``path_continues``) or ``horizon`` steps, whichever comes first: paths shorter than the
        horizon are kept, with their length, not discarded.

        Returns ``(start, length, arrays)``: archive index [n] and number of real steps [n] of every window, and the
        keyword arguments of ``FakeEnv.replay`` -- ``obs0`` [n, obs], ``actions`` / ``next_obs`` [H, n, .], ``rewards`` /
        ``costs`` / ``terminals`` [H, n], ``lengths`` -- time-major; the steps behind ``length`` repeat the window's last
        real step (padding, never compared)."""
        H, n = int(horizon), int(n)
        if H < 1 or n < 1:
            raise ValueError("windows: horizon and n must be >= 1, got %d, %d" % (H, n))
        N = self.arch_size
        ok = np.ones(N, np.bool_)
        if epochs is not None:
            ok = np.isin(self.epoch_archive[:N], np.asarray(epochs).reshape(-1))
        cand = np.flatnonzero(ok)
        if cand.size == 0:
            raise ValueError("windows: no archived sample%s" % ("" if epochs is None else " of epochs %r" % (list(np.ravel(epochs)),)))
        rng = np.random.default_rng() if rng is None else rng
        start = cand[rng.integers(0, cand.size, size=n)]
        ends = np.flatnonzero(~self.path_continues())            # the last step of every path (slot N - 1 is always one)
        remaining = ends[np.searchsorted(ends, start)] - start + 1
        length = np.minimum(H, remaining).astype(np.int32)
        idx = start[None, :] + np.minimum(np.arange(H)[:, None], length[None, :] - 1)
        a = self.arch_dict
        flat = lambda x: x.reshape(x.shape[:2] + (-1,))
        arrays = dict(obs0=a["observations"][start].reshape(n, -1), actions=flat(a["actions"][idx]),
                      next_obs=flat(a["next_observations"][idx]), rewards=a["rewards"][idx], costs=a["costs"][idx],
                      terminals=a["terminals"][idx], lengths=length)
        return start, length, arrays

    # -- device mirror of the archive and start-state sampling on it (csrc/start_states.hip) ------------
    _MIRRORED = ("observations", "mu", "log_std", "epochs")

    def _host_column(self, k):
        return self.pi_info_archive[k] if k in ("mu", "log_std") else self.arch_dict[k]

    def enable_device_archive(self):
        """Allocate the device mirror of the columns start-state sampling reads -- observations [archive_size, obs],
        mu / log_std [archive_size, A] float32, epochs [archive_size] int32 (-1 = empty) -- and fill it from the host
        archive.  From here on ``dump_to_archive`` appends every slab to it and ``reset_arch`` resets it."""
        if self._dev is not None:
            return
        if not self.pi_info_shapes or sorted(self.pi_info_shapes) != ["log_std", "mu"]:
            raise _lib.CmbpoHipError("enable_device_archive: initialize() the buffer with the Gaussian pi_info "
                                     "{mu, log_std} first")
        if self.archive_size > 2 ** 31 - 1:
            raise _lib.CmbpoHipError("enable_device_archive: archive indices are int32")
        n, dev = self.archive_size, self.device
        self._dev = {k: torch.empty((n,) + self._host_column(k).shape[1:], device=dev,
                                    dtype=torch.int32 if k == "epochs" else torch.float32) for k in self._MIRRORED}
        self._dev_version = 0          # bumped by every write to the mirror; the run table is rebuilt when it lags
        self._table_version = -1
        self._table = torch.zeros(_lib.START_TABLE_INTS, dtype=torch.int32, device=dev)
        self._cdf = torch.zeros(_lib.START_CDF_DOUBLES, dtype=torch.float64, device=dev)
        self._start_scratch = {}
        self.start_generator = torch.Generator(device=dev)     # the uniforms of sample_start_states
        self.start_generator.manual_seed(0)
        self.last_start = {}
        self._mirror(slice(0, n))

    def _mirror(self, dst):
        for k in self._MIRRORED:
            h = self._host_column(k)[dst]
            if k == "epochs":
                h = h.astype(np.int32)
            self._dev[k][dst].copy_(torch.from_numpy(np.ascontiguousarray(h)))
        self._dev_version += 1

    def device_archive(self):
        """The mirror's tensors by column name (enabled on first use)."""
        self.enable_device_archive()
        return self._dev

    def _start_table(self):
        """The run table of the mirrored epoch column, rebuilt only after the archive changed; its epochs present and
        their sample counts are read back once per rebuild (the only host read of the path)."""
        self.enable_device_archive()
        if self._table_version != self._dev_version:
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().cmbpo_start_table_build(self._dev["epochs"].data_ptr(), self.archive_size,
                                                               self._table.data_ptr(), _lib.current_stream()),
                           "cmbpo_start_table_build")
                t = self._table.cpu().numpy()
                void = float(self._cdf[1].item())       # (a synchronising read: taken here, once per archive change)
                self._cdf[1] = 0.0
            if void:
                raise _lib.CmbpoHipError("start states: a round since the last archive change had no finite Boltzmann "
                                         "mass (NaN or infinite policy KL): its start states are void")
            M = _lib.START_MAX_RUNS
            if t[2]:
                raise _lib.CmbpoHipError("start-state table: the archive's epoch column has more than %d runs of equal "
                                         "tags (epochs are expected in contiguous slabs)" % M)
            n_ep = int(t[1])
            self._start_info = dict(n_runs=int(t[0]), n_epochs=n_ep, filled=int(t[3]),
                                    epochs=t[8 + 3 * M:8 + 3 * M + n_ep].astype(np.int64),
                                    counts=t[8 + 4 * M:8 + 4 * M + n_ep].astype(np.int64),
                                    run_start=t[8:8 + int(t[0])].copy(), run_len=t[8 + M:8 + M + int(t[0])].copy())
            self._table_version = self._dev_version
        return self._start_info

    def _scratch(self, name, shape, dtype):
        """Scratch tensors live until a call asks for another shape (a new batch size reallocates)."""
        t = self._start_scratch.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = torch.zeros(shape, dtype=dtype, device=self.device)
            self._start_scratch[name] = t
        return t

    def _uniforms(self, shape, u):
        if u is None:
            return torch.rand(shape, generator=self.start_generator, dtype=torch.float64, device=self.device)
        if isinstance(u, torch.Tensor):
            t = u.to(device=self.device, dtype=torch.float64).contiguous()
        else:
            t = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float64)).to(self.device)
        if tuple(t.shape) != tuple(shape):
            raise _lib.CmbpoHipError("start states: uniforms of shape %r, expected %r" % (tuple(t.shape), tuple(shape)))
        return t

    def device_epoch_batch(self, batch_size, epochs=None, u=None):
        """``epoch_batch`` (cpobuffer.py:466-524) on the mirror: for every epoch (default: all present, ascending)
        ``batch_size`` members drawn with the uniforms ``u`` [n_epochs, batch_size] (float64 in [0, 1); drawn from
        ``start_generator`` when None) as ``members_e[min(floor(u n_e), n_e - 1)]``.  Returns device tensors
        ``idx`` [n_epochs, B] int32 and ``observations`` / ``mu`` / ``log_std`` [n_epochs, B, .]."""
        info = self._start_table()
        if info["n_epochs"] == 0:
            raise _lib.CmbpoHipError("start states: the archive is empty")
        B, dev = int(batch_size), self.device
        if B < 1:
            raise _lib.CmbpoHipError("start states: batch_size %d" % B)
        sel = None
        if epochs is not None:
            assert len(np.shape(epochs)) == 1
            ep = np.array(epochs)
            if np.any(ep > info["epochs"][-1]) or np.any(ep < info["epochs"][0]):
                print('Warning: epoch not contained in buffer.')
                return None
            place = np.searchsorted(info["epochs"], ep)
            if np.any(info["epochs"][np.minimum(place, info["n_epochs"] - 1)] != ep):
                raise _lib.CmbpoHipError("start states: epoch without samples in the archive")
            sel = torch.from_numpy(place.astype(np.int32)).to(dev)
        E = info["n_epochs"] if sel is None else int(sel.numel())
        D, A = self._dev["observations"].shape[1], self._dev["mu"].shape[1]
        with torch.cuda.device(dev):
            ut = self._uniforms((E, B), u)
            out = dict(idx=self._scratch("idx_epoch", (E, B), torch.int32),
                       observations=self._scratch("obs_epoch", (E, B, D), torch.float32),
                       mu=self._scratch("mu_epoch", (E, B, A), torch.float32),
                       log_std=self._scratch("ls_epoch", (E, B, A), torch.float32))
            _lib.check(_lib.lib().cmbpo_start_epoch_draw(
                self._table.data_ptr(), _lib.ptr(sel), E, B, ut.data_ptr(), self._dev["observations"].data_ptr(),
                self._dev["mu"].data_ptr(), self._dev["log_std"].data_ptr(), self.archive_size, D, A,
                out["idx"].data_ptr(), out["observations"].data_ptr(), out["mu"].data_ptr(), out["log_std"].data_ptr(),
                _lib.current_stream()), "cmbpo_start_epoch_draw")
        return out

    def device_epoch_kl(self, policy, ep_b, alpha=1):
        """``np.clip(policy.compute_DKL(...), 0)`` (cmbpo.py:220, cpo_policy.py:837-845) on the rows of
        ``device_epoch_batch``: the actor's forward pass, the per-row KL(current || stored) with ordered float64 sums, and
        -- in the same launch that folds them -- the Boltzmann CDF for ``alpha`` that ``device_boltz_draw`` searches.
        Returns the device tensor kl [n_epochs] float64."""
        obs, mu_old, ls_old = ep_b["observations"], ep_b["mu"], ep_b["log_std"]
        E, B, A = mu_old.shape
        if E != self._start_table()["n_epochs"]:
            raise _lib.CmbpoHipError("start states: the KL needs a batch of every epoch present")
        lib, dev = _lib.lib(), self.device
        with torch.cuda.device(dev):
            n_part = lib.cmbpo_start_kl_parts(B)
            o = {k: self._scratch("pi_" + k, (E * B, A), torch.float32) for k in ("pi", "mu", "log_std", "eps")}
            o["logp_pi"] = self._scratch("pi_logp", (E * B,), torch.float32)
            part = self._scratch("kl_part", (E, n_part), torch.float64)
            kl = self._scratch("kl", (E,), torch.float64)
            policy.actor.forward_device(obs.view(E * B, -1), o["eps"], o)     # (eps stays zero: pi = mu, unused)
            _lib.check(lib.cmbpo_start_kl_partials(o["mu"].data_ptr(), o["log_std"].data_ptr(), mu_old.data_ptr(),
                                                   ls_old.data_ptr(), E, B, A, part.data_ptr(), n_part,
                                                   _lib.current_stream()), "cmbpo_start_kl_partials")
            _lib.check(lib.cmbpo_start_cdf(self._table.data_ptr(), part.data_ptr(), n_part, B, kl.data_ptr(), float(alpha),
                                           self._cdf.data_ptr(), _lib.current_stream()), "cmbpo_start_cdf")
        return kl

    def device_boltz_draw(self, batch_size, u=None, out=None, kls=None, alpha=1):
        """``boltz_dist`` + ``distributed_batch_from_archive`` (cpobuffer.py:385-396,413-464) on the mirror: ``batch_size``
        archive rows drawn as ``searchsorted(cdf, u, side='right')`` and their observations written into ``out``
        [B, obs] (allocated when None).  ``kls`` [n_epochs] (host or device, already clipped) rebuilds the CDF for
        ``alpha`` first; None uses the one ``device_epoch_kl`` left.  Returns (out, idx [B] int32), device tensors."""
        info = self._start_table()
        if info["n_epochs"] == 0:
            raise _lib.CmbpoHipError("start states: the archive is empty")
        B, dev, lib = int(batch_size), self.device, _lib.lib()
        D = self._dev["observations"].shape[1]
        with torch.cuda.device(dev):
            if kls is not None:
                k = self._uniforms((info["n_epochs"],), kls)
                _lib.check(lib.cmbpo_start_cdf(self._table.data_ptr(), None, 0, 0, k.data_ptr(), float(alpha),
                                               self._cdf.data_ptr(), _lib.current_stream()), "cmbpo_start_cdf")
            ut = self._uniforms((B,), u)
            if out is None:
                out = self._scratch("start_obs", (B, D), torch.float32)
            if not (isinstance(out, torch.Tensor) and out.device == ut.device and out.dtype == torch.float32
                    and tuple(out.shape) == (B, D) and out.is_contiguous()):
                raise _lib.CmbpoHipError("start states: `out` must be a contiguous float32 [%d, %d] tensor on %s" % (B, D, dev))
            idx = self._scratch("idx_draw", (B,), torch.int32)
            _lib.check(lib.cmbpo_start_boltz_draw(self._table.data_ptr(), self._cdf.data_ptr(), ut.data_ptr(), B,
                                                  self._dev["observations"].data_ptr(), self.archive_size, D,
                                                  idx.data_ptr(), out.data_ptr(), _lib.current_stream()),
                       "cmbpo_start_boltz_draw")
        return out, idx

    def sample_start_states(self, policy, batch_size, alpha=1, out=None, u_epoch=None, u_draw=None):
        """Lines 239-251 of algorithms/cmbpo.py in five launches on the device: a batch of every archived epoch, the
        current policy's mean KL to each, the Boltzmann distribution over the epochs, ``batch_size`` archive rows drawn
        from it.  Their observations are written into ``out`` (e.g. the rollout state's ``cur_obs``) and returned.  The
        uniforms come from ``start_generator`` unless handed in (``u_epoch`` [n_epochs, B], ``u_draw`` [B], float64 in
        [0, 1)).  ``last_start`` keeps the device tensors of the round (epoch-batch indices, KLs, drawn indices)."""
        ep_b = self.device_epoch_batch(batch_size, u=u_epoch)
        kl = self.device_epoch_kl(policy, ep_b, alpha=alpha)
        out, idx = self.device_boltz_draw(batch_size, u=u_draw, out=out)
        self.last_start = dict(idx_epoch=ep_b["idx"], kl=kl, idx=idx,
                               ep_probs=self._cdf[8 + 3 * _lib.START_MAX_RUNS:][:kl.numel()])
        return out
