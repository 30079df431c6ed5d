"""Open-loop model validation: the device buffers of a k-step replay of real trajectories and its result table
(``csrc/replay.hip``).  The reference has no counterpart.

``ReplayBuffers`` owns every array ``cmbpo_replay_t`` names -- the recorded windows (time-major ``[H, B, .]``), the rows'
state, the post kernel's outputs of the step, the partial sums and the table -- and the ctypes image handed to
``cmbpo_replay_compare`` / ``_finish`` / ``_run``.  ``FakeEnv.replay`` is the user's entry; the tests and
``tools/probe_replay.py`` drive the single calls through this class.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

MODES = {"open_loop": _lib.REPLAY_OPEN_LOOP, "one_step": _lib.REPLAY_ONE_STEP}
SUM_KEYS = ("se_rew", "se_cost", "sum_ep_var", "sum_dkl")      # columns obs_dim .. obs_dim + 3 of `sums`


def _as(x, dtype, device):
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=dtype).contiguous()
    np_dtype = {torch.float32: np.float32, torch.uint8: np.uint8, torch.int32: np.int32}[dtype]
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np_dtype)).to(device)


class ReplayBuffers:
    def __init__(self, obs0, actions, next_obs, rewards, costs, terminals, lengths=None, mode="open_loop", ensemble=0,
                 out_dim=0, device="cuda"):
        """obs0 [B, obs]; actions [H, B, act]; next_obs [H, B, obs]; rewards / costs / terminals [H, B] (a trailing axis
        of one is dropped); lengths [B] in 1..H (None: H).  NumPy arrays or tensors.  ``ensemble`` / ``out_dim`` > 0 also
        allocate the forward's scratch ``cmbpo_replay_run`` needs."""
        if mode not in MODES:
            raise ValueError("replay mode: 'open_loop' or 'one_step', got %r" % (mode,))
        dev = torch.device(device)
        self.device, self.mode = dev, mode
        f32, u8, i32 = torch.float32, torch.uint8, torch.int32
        act, nxt = _as(actions, f32, dev), _as(next_obs, f32, dev)
        if nxt.dim() != 3 or act.dim() != 3 or act.shape[:2] != nxt.shape[:2]:
            raise ValueError("replay: actions [H, B, act] and next_obs [H, B, obs] expected, got %s and %s"
                             % (tuple(act.shape), tuple(nxt.shape)))
        H, B, D = nxt.shape
        A = act.shape[2]
        if H < 1 or B < 1:
            raise ValueError("replay: at least one window of one step, got H = %d, B = %d" % (H, B))
        cur = _as(obs0, f32, dev).clone()
        if tuple(cur.shape) != (B, D):
            raise ValueError("replay: obs0 must be [%d, %d], got %s" % (B, D, tuple(cur.shape)))
        flat = lambda x, dt: _as(x, dt, dev).reshape(H, B)
        rew, cost = flat(rewards, f32), flat(costs, f32)
        term = flat(terminals, u8)
        if lengths is None:
            ln = torch.full((B,), H, dtype=i32, device=dev)
        else:
            ln = _as(lengths, i32, dev).reshape(B)
            lo, hi = int(ln.min()), int(ln.max())
            if lo < 1 or hi > H:
                raise ValueError("replay: lengths must lie in 1..%d, got %d..%d" % (H, lo, hi))
        self.B, self.H, self.obs_dim, self.act_dim = B, H, D, A
        self.n_part = _lib.lib().cmbpo_replay_parts(B)
        f = dict(dtype=f32, device=dev)
        ncol = D + _lib.REPLAY_SCALAR_SUMS
        self.t = dict(act=act, next_obs=nxt, rew=rew, cost=cost, term=term, len=ln, cur_obs=cur,
                      alive=torch.ones(B, dtype=u8, device=dev),
                      p_next_obs=torch.empty((B, D), **f), p_rew=torch.empty(B, **f),
                      p_term=torch.empty(B, dtype=u8, device=dev), p_cost=torch.empty(B, **f),
                      p_dkl_path=torch.empty(B, **f), p_ep_var_mean=torch.empty(B, **f),
                      part_sum=torch.zeros((H, self.n_part, ncol), dtype=torch.float64, device=dev),
                      part_cnt=torch.zeros((H, self.n_part, _lib.REPLAY_COUNTS), dtype=torch.int64, device=dev),
                      sums=torch.zeros((H, ncol), dtype=torch.float64, device=dev),
                      counts=torch.zeros((H, _lib.REPLAY_COUNTS), dtype=torch.int64, device=dev))
        if ensemble > 0:
            self.t["mean"] = torch.empty((ensemble, B, out_dim), **f)
            self.t["var"] = torch.empty_like(self.t["mean"])
        rs = _lib.ReplayStruct()
        rs.B, rs.H, rs.obs_dim, rs.act_dim, rs.mode, rs.reserved = B, H, D, A, MODES[mode], 0
        for k, v in self.t.items():
            setattr(rs, k, v.data_ptr())
        self.rs = rs

    def step_outputs(self):
        """The dict ``FakeEnv.step_device`` fills: the prediction arrays ``cmbpo_replay_compare`` reads."""
        t = self.t
        return dict(next_obs=t["p_next_obs"], rew=t["p_rew"], term=t["p_term"], cost=t["p_cost"], dkl_path=t["p_dkl_path"],
                    ep_var_mean=t["p_ep_var_mean"])

    def compare(self, h):
        _lib.check(_lib.lib().cmbpo_replay_compare(C.byref(self.rs), int(h), _lib.current_stream()), "cmbpo_replay_compare")

    def finish(self):
        _lib.check(_lib.lib().cmbpo_replay_finish(C.byref(self.rs), _lib.current_stream()), "cmbpo_replay_finish")

    def run(self, model_handle, task_id, ensemble, elite):
        """``cmbpo_replay_run``; elite: [H, B] int32 device tensor."""
        _lib.check(_lib.lib().cmbpo_replay_run(C.byref(self.rs), model_handle, int(task_id), int(ensemble), elite.data_ptr(),
                                               _lib.current_stream()), "cmbpo_replay_run")

    def table(self):
        return table(self.t["sums"].cpu().numpy(), self.t["counts"].cpu().numpy(), self.obs_dim)


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
