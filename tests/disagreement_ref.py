"""NumPy specification of the ensemble disagreement on the reward and the learned-cost column of a stepped row, and of the
pessimistic reward / cost made from it (cmbpo_fakeenv_post_disagreement, include/cmbpo_hip.h).

For a row r with the members' means ``mean[E, ., out]`` and ``D = obs_dim``:

    rew_var[r]  = np.var(mean[:, r, D], axis=0)          float32, over ALL E members
    cost_var[r] = np.var(mean[:, r, D + 1], axis=0)      with a learned cost head, else +0.0
    rew[r]      = fl32(rew_elite  - fl32(kappa_rew  * sqrt(rew_var)))    where kappa_rew  > 0, else rew_elite  bit for bit
    cost[r]     = fl32(cost_elite + fl32(kappa_cost * sqrt(cost_var)))   where kappa_cost > 0, else cost_elite bit for bit

``np.var(axis=0)`` on a float32 [E, n] array is the sequential arithmetic ``member_var_loop`` spells out (s = ((x0 + x1) + x2)
+ ..., m = s / E, q = sum_e (x_e - m)^2 in member order, var = q / E, every operation rounded to float32 on its own);
tests/test_disagreement_cpu.py holds the two against each other bit for bit.  Transition noise never moves the two columns, so
the variances are those of the unperturbed means.  With kappa == 0 nothing but the elite's value reaches the output; with
kappa > 0 non-finite members propagate as NumPy propagates them."""
import numpy as np


def member_var(x):
    """np.var over the members (axis 0) of a float32 [E, n] array or strided view.

    NumPy adds along axis 0 member by member only while that axis is the outer loop of the reduction: handed an array whose
    member axis has the smallest stride (what ``mean[:, rows, col]`` with an index array returns) or a single row, it reduces
    each row with its pairwise sum, which from eight members on is another order of additions.  The specification is the
    member-by-member order, so the array is brought to C order with at least two rows first."""
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    n = x.shape[1]
    if n == 1:
        x = np.ascontiguousarray(np.concatenate([x, x], axis=1))
    with np.errstate(all="ignore"):
        return np.var(x, axis=0)[:n]


def member_var_loop(x):
    """The same as a plain sequential float32 loop over the members (vectorised over the rows only)."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    E = x.shape[0]
    with np.errstate(all="ignore"):
        s = x[0].copy()
        for e in range(1, E):
            s = (s + x[e]).astype(np.float32)
        m = (s / np.float32(E)).astype(np.float32)
        q = None
        for e in range(E):
            d = (x[e] - m).astype(np.float32)
            t = (d * d).astype(np.float32)
            q = t if q is None else (q + t).astype(np.float32)
        return (q / np.float32(E)).astype(np.float32)


def penalise(elite, var, kappa, sign):
    """elite + sign * kappa * sqrt(var) in float32 with every operation rounded on its own; kappa == 0: elite itself."""
    elite = np.asarray(elite, np.float32)
    if not kappa > 0.0:
        return elite.copy()
    with np.errstate(all="ignore"):
        pen = (np.float32(kappa) * np.sqrt(np.asarray(var, np.float32))).astype(np.float32)
        return (elite - pen if sign < 0 else elite + pen).astype(np.float32)


def disagreement(mean, inds, obs_dim, learned_cost, kappa_rew=0.0, kappa_cost=0.0, rows=None):
    """(rew_var, cost_var, rew, cost) of the rows `rows` (default: all) of mean[E, B, out]; cost is None without a learned cost
    head (the task's cost rule gives it, and no member spread exists)."""
    mean = np.asarray(mean)
    assert mean.dtype == np.float32 and mean.ndim == 3
    if kappa_cost > 0.0 and not learned_cost:
        raise ValueError("kappa_cost > 0 needs the learned cost head")
    rows = np.arange(mean.shape[1]) if rows is None else np.asarray(rows)
    inds = np.asarray(inds)[rows]
    D = int(obs_dim)
    xr = mean[:, rows, D]
    rew_var = member_var(xr)
    rew = penalise(xr[inds, np.arange(len(rows))], rew_var, kappa_rew, -1)
    if not learned_cost:
        return rew_var, np.zeros(len(rows), np.float32), rew, None
    xc = mean[:, rows, D + 1]
    cost_var = member_var(xc)
    cost = penalise(xc[inds, np.arange(len(rows))], cost_var, kappa_cost, +1)
    return rew_var, cost_var, rew, cost
