"""NumPy specification of the predictive calibration table of a replay (csrc/replay.hip): one horizon step.

The table is computed from what the model step of horizon h returned -- pred: dict(next_obs [B, D], rew [B], cost [B]) and the
forward's mean / var [E, B, out_dim] (columns 0..D-1 the observation deltas, D the reward, D + 1 a learned cost) --, the
recording rec: dict(next_obs [H, B, D], rew [H, B]), the members elite_h [B] of the step and `alive` AS IT IS ON ENTRY to the
step (before tests/replay_ref.compare of that h clears rows).  Calibrated columns: C = D + 1, the observations and the reward.

All arithmetic is float64 on the float32 inputs, one operation at a time, members in the order 0..E-1; only the error e is a
float32 difference (one rounding), as in replay_ref."""
import numpy as np

SUMS = ("z2_al", "z2_tot", "log_al", "log_tot", "v_bar", "s2")          # sums[h, k, c]
COUNTS = ("c1_al", "c2_al", "c1_tot", "c2_tot")                           # counts[h, k, c]
COVER1, COVER2 = 0.6827, 0.9545


def new_table(H, D):
    C = D + 1
    return dict(n=np.zeros(H, np.int64), n_skipped=np.zeros(H, np.int64), sums=np.zeros((H, len(SUMS), C), np.float64),
                counts=np.zeros((H, len(COUNTS), C), np.int64),
                abs_log=np.zeros((H, 2, C), np.float64))       # sum |log v_al|, sum |log v_tot|: for an error bound only


def verdicts(alive, pred, mean, var, elite_h, D):
    """(enters, skipped) [B] bool.  skipped: rows the plain table sums and this one rejects."""
    f32 = lambda a: np.asarray(a, np.float32)
    C = D + 1
    E = mean.shape[0]
    alive = np.asarray(alive).astype(bool)
    finite = np.isfinite(f32(pred["next_obs"])).all(axis=1) & np.isfinite(f32(pred["rew"])) & np.isfinite(f32(pred["cost"]))
    mu, v = f32(mean)[:, :, :C], f32(var)[:, :, :C]
    with np.errstate(invalid="ignore"):
        usable = (np.isfinite(mu) & np.isfinite(v) & (v > 0)).all(axis=(0, 2))
    m = np.asarray(elite_h)
    usable &= (m >= 0) & (m < E)
    cand = alive & finite
    return cand & usable, cand & ~usable


def calibrate(tab, h, alive, pred, mean, var, rec, elite_h, D):
    """Row h of the table, in place.  Returns the mask of the rows that entered."""
    f32 = lambda a: np.asarray(a, np.float32)
    C = D + 1
    E = mean.shape[0]
    enters, skipped = verdicts(alive, pred, mean, var, elite_h, D)
    tab["n"][h] += int(enters.sum())
    tab["n_skipped"][h] += int(skipped.sum())
    rows = np.nonzero(enters)[0]
    if rows.size == 0:
        return enters
    m = np.asarray(elite_h)[rows]
    p_col = np.concatenate([f32(pred["next_obs"])[rows], f32(pred["rew"])[rows, None]], axis=1)
    r_col = np.concatenate([f32(rec["next_obs"][h])[rows], f32(rec["rew"][h])[rows, None]], axis=1)
    e = (p_col - r_col).astype(np.float32).astype(np.float64)              # float32 difference, one rounding
    mu = f32(mean)[:, rows, :C].astype(np.float64)                          # [E, n, C]
    v = f32(var)[:, rows, :C].astype(np.float64)
    s_mu, s_v = np.zeros_like(e), np.zeros_like(e)
    for k in range(E):                                                      # member order 0..E-1
        s_mu = s_mu + mu[k]
        s_v = s_v + v[k]
    mu_bar, v_bar = s_mu / float(E), s_v / float(E)
    dev = np.zeros_like(e)
    for k in range(E):
        d = mu[k] - mu_bar
        dev = dev + d * d
    s2 = dev / float(E)
    pick = np.arange(rows.size)
    mu_m, v_al = mu[m, pick], v[m, pick]
    v_tot = v_bar + s2
    e_tot = e + (mu_bar - mu_m)
    q_al, q_tot = e * e, e_tot * e_tot
    terms = (q_al / v_al, q_tot / v_tot, np.log(v_al), np.log(v_tot), v_bar, s2)
    for k, x in enumerate(terms):
        tab["sums"][h, k] += x.sum(axis=0)
    tab["abs_log"][h, 0] += np.abs(terms[2]).sum(axis=0)
    tab["abs_log"][h, 1] += np.abs(terms[3]).sum(axis=0)
    for k, x in enumerate((q_al <= v_al, q_al <= 4.0 * v_al, q_tot <= v_tot, q_tot <= 4.0 * v_tot)):
        tab["counts"][h, k] += x.sum(axis=0)
    return enters


def derived(tab):
    """The means the host derives: NaN where no row entered."""
    n = tab["n"].astype(np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        s = {k: tab["sums"][:, j] / n for j, k in enumerate(SUMS)}
        c = {k: tab["counts"][:, j] / n for j, k in enumerate(COUNTS)}
    log2pi = np.log(2.0 * np.pi)
    return dict(z2_al=s["z2_al"], z2_tot=s["z2_tot"], nll_al=0.5 * (log2pi + s["log_al"] + s["z2_al"]),
                nll_tot=0.5 * (log2pi + s["log_tot"] + s["z2_tot"]), cover1_al=c["c1_al"], cover2_al=c["c2_al"],
                cover1_tot=c["c1_tot"], cover2_tot=c["c2_tot"], al_var=s["v_bar"], ep_var=s["s2"])


def raw_arrays(tab):
    """The table as the device lays it out: sums [H, 6 C] and counts [H, 4 C + 2]."""
    H = tab["n"].shape[0]
    counts = np.concatenate([tab["counts"].reshape(H, -1), tab["n"][:, None], tab["n_skipped"][:, None]], axis=1)
    return tab["sums"].reshape(H, -1).copy(), counts


def replay_world(E, learned_cost):
    """The random-weight model of the whole-replay tests: AntSafe's widths, hidden width 128, steps of ~0.05 per column, with or
    without the learned-cost column.  Returns dict(D, A, O, ws, bs, sc_in, sc_out)."""
    import zlib
    from cmbpo_amd import synthetic
    D, A = synthetic.ENV_DIMS["AntSafe-v2"]
    O = D + 1 + int(learned_cost)
    rng = np.random.default_rng(zlib.crc32(f"calibration-model/{E}/{int(learned_cost)}".encode()))
    ws, bs = synthetic.ensemble_weights(rng, E, D + A, 128, 2 * O, bias_scale=0.05)
    sc_out = (np.zeros((1, O), np.float32), np.full((1, O), 2.5e-3, np.float32))
    return dict(D=D, A=A, O=O, ws=ws, bs=bs, sc_in=synthetic.scaler(rng, D + A), sc_out=sc_out)


def recording(rng, B, H, D, A):
    """Windows of a made-up world: a random walk of small steps, ragged lengths, terminals inside some windows, 0/1 costs;
    some windows start at the edge of AntSafe's healthy set so that the rules end them."""
    obs0 = (rng.standard_normal((B, D)) * 0.1).astype(np.float32)
    obs0[:, 0] = rng.uniform(0.3, 0.9, B).astype(np.float32)
    obs0[::5, 2] = np.float32(0.925)
    steps = (rng.standard_normal((H, B, D)) * 0.05).astype(np.float32)
    rec = dict(next_obs=(obs0[None] + np.cumsum(steps, axis=0)).astype(np.float32), rew=rng.standard_normal((H, B)).astype(np.float32),
               cost=(rng.random((H, B)) < 0.3).astype(np.float32), term=(rng.random((H, B)) < 0.15).astype(np.uint8))
    act = rng.uniform(-1, 1, (H, B, A)).astype(np.float32)
    return obs0, act, rec, rng.integers(1, H + 1, B).astype(np.int32)


def synthetic_case(B, D, E, seed, shrink=1.0):
    """The calibrated case: identical members, the real values drawn from N(mu_m, v_m); the model is then told a variance
    `shrink` times the true one.  Returns (pred, mean, var, rec, elite_h) for H = 1 with out_dim = D + 1."""
    rng = np.random.default_rng(seed)
    C = D + 1
    mu1 = rng.standard_normal((B, C)).astype(np.float32)
    v1 = np.exp(rng.uniform(-4.0, 1.0, (B, C))).astype(np.float32)
    base = rng.standard_normal((B, D)).astype(np.float32)
    # the prediction is base + mu (observations) / mu (reward); the recording is the prediction minus a draw from N(0, v)
    noise = rng.standard_normal((B, C)) * np.sqrt(v1.astype(np.float64))
    p_obs = (base + mu1[:, :D]).astype(np.float32)
    p_rew = mu1[:, D].copy()
    rec = dict(next_obs=(p_obs - noise[:, :D]).astype(np.float32)[None], rew=(p_rew - noise[:, D]).astype(np.float32)[None])
    pred = dict(next_obs=p_obs, rew=p_rew, cost=np.zeros(B, np.float32))
    mean = np.repeat(mu1[None], E, axis=0)
    var = np.repeat((v1 * np.float32(shrink))[None], E, axis=0)
    return pred, mean, var, rec, rng.integers(0, E, B).astype(np.int32)
