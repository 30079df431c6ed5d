"""NumPy reference of the particle replay's statistics (include/cmbpo_hip.h, "particle replay"), float64, written
from the semantics there: B windows of S particles, rows b * S + p, columns = the observation columns then the reward.

``step`` is one horizon step on given predictions (what ``cmbpo_replay_particles`` does): it returns the step's row of ``sums``
[4 C + 2] and ``counts`` [C (S + 1) + 2] and advances ``cur_obs`` / ``alive`` in place.  The terms are the float32-rounded
numbers the definition names, added in float64 in NumPy's own order."""
import numpy as np

OPEN_LOOP, ONE_STEP = "open_loop", "one_step"


def sizes(obs_dim, S):
    C = obs_dim + 1
    return 4 * C + 2, C * (S + 1) + 2


def window_stats(x, q):
    """x [S] float32 particles, q float32: (k, a, g, se_mean, v) of one (window, column)."""
    x = np.asarray(x, np.float32)
    q = np.float32(q)
    S = x.shape[0]
    k = int((x < q).sum())
    a = np.abs((x - q).astype(np.float32)).astype(np.float64).sum() / S
    with np.errstate(over="ignore"):
        pair = np.triu(np.abs(x[:, None] - x[None, :]).astype(np.float64), 1).sum()      # float32 differences, p < p'
    g = 2.0 * pair / (S * (S - 1))
    m = x.astype(np.float64).sum() / S
    se = (m - float(q)) ** 2
    v = ((x.astype(np.float64) - m) ** 2).sum() / (S - 1)
    return k, a, g, se, v


def step(h, S, mode, next_obs, rew, cost, term, length, cur_obs, alive, p_next_obs, p_rew, p_cost, p_term):
    """One horizon step.  Recorded: next_obs [H, B, D], rew / cost / term [H, B], length [B].  State (changed in place): cur_obs
    [R, D] float32, alive [R] uint8.  Predictions: p_next_obs [R, D], p_rew / p_cost [R] float32, p_term [R] uint8."""
    H, B, D = next_obs.shape
    C = D + 1
    ns, nc = sizes(D, S)
    sums, counts = np.zeros(ns, np.float64), np.zeros(nc, np.int64)
    hist = counts[:C * (S + 1)].reshape(C, S + 1)
    for b in range(B):
        rows = slice(b * S, (b + 1) * S)
        if not alive[rows].all():
            assert not alive[rows].any(), "the particles of a window live and die together"
            continue
        x_obs, x_rew, x_cost = p_next_obs[rows], p_rew[rows], p_cost[rows]
        if not (np.isfinite(x_obs).all() and np.isfinite(x_rew).all() and np.isfinite(x_cost).all()):
            counts[C * (S + 1) + 1] += 1
            alive[rows] = 0
            continue
        counts[C * (S + 1)] += 1
        for c in range(C):
            x = x_obs[:, c] if c < D else x_rew
            q = next_obs[h, b, c] if c < D else rew[h, b]
            k, a, g, se, v = window_stats(x, q)
            hist[c, k] += 1
            sums[c] += a
            sums[C + c] += g
            sums[2 * C + c] += se
            sums[3 * C + c] += v
        y_t, y_c = float(term[h, b] != 0), float(cost[h, b] > 0)
        sums[4 * C] += ((p_term[rows] != 0).astype(np.float64).sum() / S - y_t) ** 2
        sums[4 * C + 1] += (x_cost.astype(np.float64).sum() / S - y_c) ** 2
        if h + 1 < length[b] and term[h, b] == 0:
            cur_obs[rows] = x_obs if mode == OPEN_LOOP else next_obs[h, b][None]
        else:
            alive[rows] = 0
    return sums, counts


def iid_case(rng, W, S, scale=1.0):
    """One horizon, one observation column (plus a reward column of the same law): q, x_p ~ N(0, 1) i.i.d., the particles
    scaled by ``scale``.  Returns the raw (sums [1, 6], counts [1, 2 (S + 1) + 2]) of W windows."""
    q = rng.standard_normal((1, W, 1)).astype(np.float32)
    qr = rng.standard_normal((1, W)).astype(np.float32)
    x = (scale * rng.standard_normal((W * S, 1))).astype(np.float32)
    xr = (scale * rng.standard_normal(W * S)).astype(np.float32)
    z = np.zeros((1, W), np.float32)
    s, c = step(0, S, OPEN_LOOP, q, qr, z, z.astype(np.uint8), np.ones(W, np.int32), np.zeros((W * S, 1), np.float32),
                np.ones(W * S, np.uint8), x, xr, np.zeros(W * S, np.float32), np.zeros(W * S, np.uint8))
    return s[None], c[None]
