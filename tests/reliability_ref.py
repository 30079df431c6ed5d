"""NumPy specification of the reliability table of the logistic columns in a replay (csrc/replay.hip): one horizon step.

The table is computed from what the model step of horizon h returned -- pred: dict(next_obs [B, D], rew [B], cost [B]) and the
forward's mean [E, B, out_dim] --, the recording rec: dict(cost [H, B], term [H, B]; with a key term_target [H, B] the TERM
columns are held against that array instead, the descriptor's own `term`), the members elite_h [B] of the step and
`alive` AS IT IS ON ENTRY to the step (before tests/replay_ref.compare of that h clears rows).

cols: a list of (col, target, shift) per reliability column -- the index into the model's output, COST (y = cost > 0.5) or TERM
(y = term != 0), and the float32 number subtracted from the logit first (0: no subtraction is executed).  z'_e = fl32(mean[e][b][col]
- shift).  A row enters column j iff it is alive, its prediction is finite (the compare rule), its elite lies in [0, E) and every
member's z'_e is finite.

Two readings per column, float64 arithmetic on the float32 inputs, one operation at a time, members in the order 0..E-1:
  0, elite:   z = (double)z'_m, m = elite_h[b]          1, pooled:  z = (sum_e (double)z'_e) / E
bin(z) = #{k : z > (double)edges[k]}     p = 1 / (1 + exp(-z))     l = max(z, 0) - y z + log1p(exp(-|z|))
brier = (p - y)^2 evaluated as q^2, q = |p - y| = 1 / (1 + exp(z if y else -z)): no cancellation where p is close to y
Sums are added row by row in row order (the device adds each slot of 64 rows in row order and the slots in slot order)."""
import numpy as np

COST, TERM = 0, 1
READINGS = ("elite", "pooled")


def default_edges(K):
    q = np.arange(1, K, dtype=np.float64) / float(K)
    return np.log(q / (1.0 - q)).astype(np.float32)


def new_table(H, n_cols, K):
    z = lambda *s: np.zeros(s, np.float64)
    i = lambda *s: np.zeros(s, np.int64)
    return dict(n_rel=i(H, n_cols), n_skipped=i(H, n_cols), n=i(H, n_cols, 2, K), pos=i(H, n_cols, 2, K),
                sum_p=z(H, n_cols, 2, K), sum_z=z(H, n_cols, 2, K), sum_brier=z(H, n_cols, 2), sum_logloss=z(H, n_cols, 2),
                abs_z=z(H, n_cols, 2, K), abs_logloss=z(H, n_cols, 2))      # sum |z|, sum |l|: for an error bound only


def shifted(mean, col, shift):
    """z'_e [E, B] float32: one float32 subtraction, none at all for a shift of 0."""
    z = np.asarray(mean, np.float32)[:, :, col]
    shift = np.float32(shift)
    with np.errstate(invalid="ignore", over="ignore"):
        return z.copy() if shift == 0 else (z - shift).astype(np.float32)


def verdicts(alive, pred, zs, elite_h):
    """(enters, skipped) [B] bool of one column with the shifted logits zs [E, B]."""
    f32 = lambda a: np.asarray(a, np.float32)
    E = zs.shape[0]
    alive = np.asarray(alive).astype(bool)
    finite = np.isfinite(f32(pred["next_obs"])).all(axis=1) & np.isfinite(f32(pred["rew"])) & np.isfinite(f32(pred["cost"]))
    m = np.asarray(elite_h)
    usable = np.isfinite(zs).all(axis=0) & (m >= 0) & (m < E)
    cand = alive & finite
    return cand & usable, cand & ~usable


def terms(z, y):
    """(p, logloss, brier) of float64 logits z and 0 / 1 flags y, every operation rounded separately."""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-z))
    ll = np.maximum(z, 0.0) - y * z + np.log1p(np.exp(-np.abs(z)))
    with np.errstate(over="ignore"):
        q = 1.0 / (1.0 + np.exp(np.where(y > 0, z, -z)))       # |p - y| without the cancellation of p - 1
    return p, ll, q * q


def bins(z, edges):
    e = np.asarray(edges, np.float32).astype(np.float64)
    return (np.asarray(z, np.float64)[:, None] > e[None, :]).sum(axis=1) if e.size else np.zeros(len(z), np.int64)


def reliab(tab, h, alive, pred, mean, rec, elite_h, cols, edges):
    """Row h of the table, in place.  Returns the masks [n_cols, B] of the rows that entered."""
    E = np.asarray(mean).shape[0]
    K = tab["n"].shape[3]
    masks = []
    for j, (col, target, shift) in enumerate(cols):
        zs = shifted(mean, col, shift)
        enters, skipped = verdicts(alive, pred, zs, elite_h)
        masks.append(enters)
        tab["n_rel"][h, j] += int(enters.sum())
        tab["n_skipped"][h, j] += int(skipped.sum())
        rows = np.nonzero(enters)[0]
        if rows.size == 0:
            continue
        y = (np.asarray(rec["cost"][h], np.float32)[rows] > np.float32(0.5)) if target == COST else (np.asarray(rec.get("term_target", rec["term"])[h])[rows] != 0)
        zd = zs[:, rows].astype(np.float64)
        s = np.zeros(rows.size)
        for e in range(E):                                     # member order 0..E-1
            s = s + zd[e]
        readings = (zd[np.asarray(elite_h)[rows], np.arange(rows.size)], s / float(E))
        for r, z in enumerate(readings):
            k = bins(z, edges)
            p, ll, br = terms(z, y)
            assert K > k.max()
            zero = np.zeros(rows.size, np.int64)
            at = np.add.at                                     # unbuffered: one addition per row, in row order
            at(tab["n"][h, j, r], k, 1)
            at(tab["pos"][h, j, r], k, y.astype(np.int64))
            at(tab["sum_p"][h, j, r], k, p)
            at(tab["sum_z"][h, j, r], k, z)
            at(tab["abs_z"][h, j, r], k, np.abs(z))
            at(tab["sum_brier"][h, j], zero + r, br)
            at(tab["sum_logloss"][h, j], zero + r, ll)
            at(tab["abs_logloss"][h, j], zero + r, np.abs(ll))
    return np.stack(masks)


def raw_arrays(tab):
    """The table as the device lays it out: sums [H, 2 C (2 K + 2)] and counts [H, 4 C K + 2 C]."""
    H, C = tab["n_rel"].shape
    sums = np.concatenate([tab["sum_p"], tab["sum_z"], tab["sum_brier"][..., None], tab["sum_logloss"][..., None]], axis=3)
    cnt = np.concatenate([tab["n"], tab["pos"]], axis=3)
    tail = np.stack([tab["n_rel"], tab["n_skipped"]], axis=2)
    return sums.reshape(H, -1).copy(), np.concatenate([cnt.reshape(H, -1), tail.reshape(H, -1)], axis=1)


def derived(tab, j, r):
    """What the host derives for column j, reading r: NaN where nothing entered."""
    n, pos = tab["n"][:, j, r].astype(np.float64), tab["pos"][:, j, r].astype(np.float64)
    N = n.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        conf, freq, zbar = tab["sum_p"][:, j, r] / n, pos / n, tab["sum_z"][:, j, r] / n
        gap = np.where(n > 0, np.abs(conf - freq), 0.0)
        nan = np.where(N > 0, 0.0, np.nan)
        return dict(conf=conf, freq=freq, zbar=zbar, ece=(n * gap).sum(axis=1) / N + nan, mce=gap.max(axis=1) + nan,
                    brier=tab["sum_brier"][:, j, r] / N + nan, logloss=tab["sum_logloss"][:, j, r] / N + nan,
                    base_rate=pos.sum(axis=1) / N + nan, mean_p=tab["sum_p"][:, j, r].sum(axis=1) / N + nan)


def exact_offset(z, y):
    """The per-row solve logit_offset approximates through the bin means: the root of sum_i sigma(z_i - b) = sum_i y_i, by 100
    bisections of [-30, 30]."""
    z, want = np.asarray(z, np.float64), float(np.sum(y))
    a, b = -30.0, 30.0
    for _ in range(100):
        mid = 0.5 * (a + b)
        if float((1.0 / (1.0 + np.exp(-(z - mid)))).sum()) > want:
            a = mid
        else:
            b = mid
    return 0.5 * (a + b)


def synthetic_case(B, E, seed, offset=0.0):
    """The calibrated case: identical members whose logit z ~ N(0, 2^2), the flag y ~ Bernoulli(sigma(z)); the model then reports
    z + offset.  One column (col 0 of out_dim 1), target TERM, H = 1.  Returns (pred, mean, rec, elite_h, z_true)."""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal(B) * 2.0).astype(np.float32)
    y = rng.random(B) < 1.0 / (1.0 + np.exp(-z.astype(np.float64)))
    mean = np.repeat((z + np.float32(offset)).astype(np.float32)[None, :, None], E, axis=0)
    pred = dict(next_obs=np.zeros((B, 1), np.float32), rew=np.zeros(B, np.float32), cost=np.zeros(B, np.float32))
    rec = dict(cost=np.zeros((1, B), np.float32), term=y.astype(np.uint8)[None])
    return pred, mean, rec, rng.integers(0, E, B).astype(np.int32), z
