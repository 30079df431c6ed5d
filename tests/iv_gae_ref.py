"""Restatement of the weighted branch of the reference's ``discount_cumsum(x, discount, lam, weights=w, axis=-1)``
(utilities/utils.py:189-208) as one reverse pass in NumPy float64 -- TEST INFRASTRUCTURE, the checker of
tests/test_iv_gae_*.py.  tests/test_iv_gae_cpu.py holds it against calls of the reference's own function recorded in
tests/golden/g17_iv_cumsum.npz, bit for bit.

For a row of length L with weights w[0..L-1]:

    lam_vec[0] = 1, lam_vec[u] = lam * lam_vec[u-1]          (lfilter([1], [1, -lam]) on a unit impulse)
    lw  = w[L-1] * lam ** L                                  (Python float power)
    S_t = sum_{u=t}^{L-2} w[u] * lam_vec[u]                  (accumulated from u = L-2 downwards, S_{L-1} = 0)
    W_t = (1 - lam) * S_t + lw
    Y_t = x_t * W_t + gamma * Y_{t+1},  Y_L = 0
    out_t = Y_t / W_t

Every product, sum and division is one correctly rounded float64 operation (NumPy's element-wise ufuncs), in the order
the HIP kernel takes them (csrc/rollout_state.hip, gae_finish_path).
"""
import numpy as np

F32 = np.float32


def lam_tables(lam, T):
    """(lam_vec[T], lam ** L for L = 0..T), float64."""
    lam = float(lam)
    vec = np.empty(T, np.float64)
    v = 1.0
    for u in range(T):
        vec[u] = v
        v = lam * v
    return vec, np.array([lam ** L for L in range(T + 1)], np.float64)


def iv_weights(var, iv_eps):
    """w[b, u] = 1 / (iv_eps + sum_{s<=u} float64(var[b, s])) for float32 variances [n, L], summed in time order."""
    return 1.0 / (iv_eps + np.cumsum(np.asarray(var).astype(np.float64), axis=-1))


def iv_discount_cumsum(x, gamma, lam, w):
    """x [n, L] (float32 or float64), w [n, L] float64 -> float64 [n, L]."""
    x = np.asarray(x).astype(np.float64)
    w = np.asarray(w, np.float64)
    n, L = x.shape
    out = np.empty((n, L), np.float64)
    if L == 0:
        return out
    gamma, lam = float(gamma), float(lam)
    lam_vec, lam_pow = lam_tables(lam, L)
    lw = w[:, L - 1] * lam_pow[L]
    oml = 1.0 - lam
    s, y = np.zeros(n), np.zeros(n)
    with np.errstate(all="ignore"):
        for t in range(L - 1, -1, -1):
            if t < L - 1:
                s = w[:, t] * lam_vec[t] + s
            wn = oml * s + lw
            y = x[:, t] * wn + gamma * y
            out[:, t] = y / wn
    return out


def iv_gae_rows(rew, val, last_val, gamma, lam, w):
    """buffers/modelbuffer.py:163-170 with the weighted discount_cumsum, rows [n, L]: (adv float32, ret float32).  The
    deltas follow NumPy promotion as in the reference: a float64 bootstrap (np.zeros) promotes them to float64."""
    last_val = np.asarray(last_val)
    rews = np.append(rew, last_val[..., None], axis=-1)
    vals = np.append(val, last_val[..., None], axis=-1)
    deltas = rews[..., :-1] + gamma * vals[..., 1:] - vals[..., :-1]
    adv = iv_discount_cumsum(deltas, gamma, lam, w).astype(F32)
    return adv, (adv + val).astype(F32)
