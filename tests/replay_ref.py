"""NumPy specification of the open-loop replay of real trajectories (csrc/replay.hip): the comparison of one
horizon step and the life of a window.  A loop over h; differences in float32 (one rounding), accumulation in float64.

pred is what a model step from cur_obs returned: dict(next_obs [B, D], rew [B], cost [B], term [B], ep_var_mean [B],
dkl_path [B]).  rec holds the recording, time-major: dict(next_obs [H, B, D], rew / cost / term [H, B])."""
import numpy as np

OPEN_LOOP, ONE_STEP = "open_loop", "one_step"


def new_table(H, D):
    z = lambda *s: np.zeros((H,) + s, np.float64)
    return dict(n=np.zeros(H, np.int64), n_nonfinite=np.zeros(H, np.int64), se_obs=z(D), se_rew=z(), se_cost=z(),
                sum_ep_var=z(), sum_dkl=z(), sum_abs_dkl=z(), cost_cm=np.zeros((H, 2, 2), np.int64), term_cm=np.zeros((H, 2, 2), np.int64))


def compare(tab, h, cur_obs, alive, pred, rec, lengths, mode):
    """One horizon step, in place: tab row h, alive [B] bool, cur_obs [B, D] float32.  Returns the mask of the rows summed."""
    f32 = lambda a: np.asarray(a, np.float32)
    p_obs, p_rew, p_cost = f32(pred["next_obs"]), f32(pred["rew"]), f32(pred["cost"])
    p_term = np.asarray(pred["term"]).astype(bool)
    finite = np.isfinite(p_obs).all(axis=1) & np.isfinite(p_rew) & np.isfinite(p_cost)
    bad = alive & ~finite                  # 1. counted, dies, adds nothing else
    ok = alive & finite                    # 2.
    tab["n_nonfinite"][h] += int(bad.sum())
    tab["n"][h] += int(ok.sum())
    r_obs, r_rew, r_cost = f32(rec["next_obs"][h]), f32(rec["rew"][h]), f32(rec["cost"][h])
    r_term = np.asarray(rec["term"][h]).astype(bool)
    with np.errstate(invalid="ignore", over="ignore"):
        e_obs = (p_obs - r_obs).astype(np.float32).astype(np.float64)          # float32 difference, one rounding
        e_rew = (p_rew - r_rew).astype(np.float32).astype(np.float64)
        e_cost = (p_cost - r_cost).astype(np.float32).astype(np.float64)
    tab["se_obs"][h] += (e_obs[ok] * e_obs[ok]).sum(axis=0)
    tab["se_rew"][h] += (e_rew[ok] * e_rew[ok]).sum()
    tab["se_cost"][h] += (e_cost[ok] * e_cost[ok]).sum()
    tab["sum_ep_var"][h] += f32(pred["ep_var_mean"])[ok].astype(np.float64).sum()
    tab["sum_dkl"][h] += f32(pred["dkl_path"])[ok].astype(np.float64).sum()
    tab["sum_abs_dkl"][h] += np.abs(f32(pred["dkl_path"])[ok].astype(np.float64)).sum()     # (for an error bound, not in the kernel)
    with np.errstate(invalid="ignore"):
        rc, pc = r_cost > 0, p_cost > np.float32(0.5)
    for real in (0, 1):
        for guess in (0, 1):
            tab["cost_cm"][h, real, guess] += int((ok & (rc == bool(real)) & (pc == bool(guess))).sum())
            tab["term_cm"][h, real, guess] += int((ok & (r_term == bool(real)) & (p_term == bool(guess))).sum())
    # 3. who lives on, and from where; 4. everything else is frozen
    nxt = ok & (h + 1 < np.asarray(lengths)) & ~r_term
    if mode == OPEN_LOOP:
        nxt &= ~p_term
        cur_obs[nxt] = p_obs[nxt]
    else:
        assert mode == ONE_STEP, mode
        cur_obs[nxt] = r_obs[nxt]
    alive[:] = nxt
    return ok


def replay(step, obs0, rec, lengths, mode=OPEN_LOOP, on_step=None):
    """step(h, cur_obs) -> pred for ALL B rows (what it returns for dead rows is never read).  Returns (table, cur_obs, alive)
    as they stand after the last horizon.  on_step(h, cur_obs_before, alive_before, cur_obs, alive) sees every step."""
    H, B, D = np.asarray(rec["next_obs"]).shape
    lengths = np.full(B, H, np.int32) if lengths is None else np.asarray(lengths)
    assert lengths.min() >= 1 and lengths.max() <= H
    tab = new_table(H, D)
    cur_obs = np.array(obs0, np.float32)
    alive = np.ones(B, bool)
    for h in range(H):
        before = (cur_obs.copy(), alive.copy())
        compare(tab, h, cur_obs, alive, step(h, cur_obs), rec, lengths, mode)
        if on_step is not None:
            on_step(h, before[0], before[1], cur_obs, alive)
    return tab, cur_obs, alive


def means(tab):
    """The means FakeEnv.replay reports next to the sums: NaN where no row was summed."""
    n = tab["n"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(mse_obs=tab["se_obs"] / n[:, None], mse_rew=tab["se_rew"] / n, mse_cost=tab["se_cost"] / n,
                    ep_var_mean=tab["sum_ep_var"] / n, dkl_mean=tab["sum_dkl"] / n)
