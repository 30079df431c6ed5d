"""NumPy specification of the static rules' votes in the model replay (csrc/replay.hip).  It composes what exists:
tests/replay_ref.py's ``replay(..., on_step=)`` loop and ``compare``, tests/rule_votes_ref.py's ``rule_votes`` for the verdicts and
vote counts of a step, and the histogram and its derived table below.

    a row enters at h iff it is alive on entry and p_next_obs, p_rew, p_cost are finite (the compare call's rule)
    an entering row with a vote count above E counts in n_skipped[h], every other one in n_vote[h] and adds
    hist_cost[h][v_c][cost[h][b] > 0] += 1,   hist_term[h][v_d][term[h][b] != 0] += 1     (term: the table's own flags if given)

Everything is an integer or a float64 function of integers."""
import numpy as np

import replay_ref as ref
import rule_votes_ref as vref

SLOTS, COUNTS = 9, 38          # v = 0 .. 8; hist_cost [9][2] | hist_term [9][2] | n_vote | n_skipped
F32 = np.float32


def new_table(H):
    return dict(hist_cost=np.zeros((H, SLOTS, 2), np.int64), hist_term=np.zeros((H, SLOTS, 2), np.int64),
                n_vote=np.zeros(H, np.int64), n_skipped=np.zeros(H, np.int64))


def votes(tab, h, alive, pred, rec, E, done_votes, cost_votes=None, term=None):
    """One horizon step of the vote table, in place; BEFORE ref.compare of the step (which changes `alive`).  cost_votes None: a
    learned cost, the cost half stays 0.  term [H, B]: the flags hist_term is held against (None: rec['term'])."""
    p_obs, p_rew, p_cost = (np.asarray(pred[k], F32) for k in ("next_obs", "rew", "cost"))
    enters = np.asarray(alive, bool) & np.isfinite(p_obs).all(axis=1) & np.isfinite(p_rew) & np.isfinite(p_cost)
    vd = np.asarray(done_votes).astype(np.int64)
    vc = np.zeros_like(vd) if cost_votes is None else np.asarray(cost_votes).astype(np.int64)
    ok = enters & (vd <= E) & (vc <= E)
    tab["n_vote"][h] += int(ok.sum())
    tab["n_skipped"][h] += int((enters & ~ok).sum())
    with np.errstate(invalid="ignore"):
        y_c = np.asarray(rec["cost"][h], F32) > 0
    y_t = np.asarray(rec["term"][h] if term is None else term[h]) != 0
    if cost_votes is not None:
        np.add.at(tab["hist_cost"][h], (vc[ok], y_c[ok].astype(np.int64)), 1)
    np.add.at(tab["hist_term"][h], (vd[ok], y_t[ok].astype(np.int64)), 1)
    return ok


def raw_counts(tab):
    """[H, 38] int64 in the device's layout."""
    H = tab["n_vote"].shape[0]
    return np.concatenate([tab["hist_cost"].reshape(H, -1), tab["hist_term"].reshape(H, -1), tab["n_vote"][:, None],
                           tab["n_skipped"][:, None]], axis=1)


def derived(hist, E):
    """The derived entries of one signal from hist [H, 9, 2], each written as a loop over horizons and vote counts."""
    H = hist.shape[0]
    nan = float("nan")
    out = dict(hist=hist[:, :E + 1].copy(), n=np.zeros(H, np.int64), conf=np.array([v / E for v in range(E + 1)], np.float64),
               freq=np.full((H, E + 1), nan), cm=dict(any=np.zeros((H, 2, 2), np.int64), majority=np.zeros((H, 2, 2), np.int64)))
    for k in ("ece", "mce", "brier", "base_rate", "mean_share", "split_rate"):
        out[k] = np.full(H, nan)
    for h in range(H):
        n = int(hist[h, :E + 1].sum())
        out["n"][h] = n
        ece = mce = brier = share = 0.0
        pos = split = 0
        for v in range(E + 1):
            n0, n1 = int(hist[h, v, 0]), int(hist[h, v, 1])
            c = v / E
            for y, k in ((0, n0), (1, n1)):
                out["cm"]["any"][h, y, int(v > 0)] += k
                out["cm"]["majority"][h, y, int(2 * v > E)] += k
            if n0 + n1 == 0:
                continue
            out["freq"][h, v] = n1 / (n0 + n1)
            gap = abs(c - out["freq"][h, v])
            mce = max(mce, gap)
            if n:
                ece += (n0 + n1) * gap
                brier += n0 * c ** 2 + n1 * (1.0 - c) ** 2
                share += (n0 + n1) * c
            pos += n1
            split += (n0 + n1) if 0 < v < E else 0
        if n:
            out["ece"][h], out["mce"][h], out["brier"][h] = ece / n, mce, brier / n
            out["base_rate"][h], out["mean_share"][h], out["split_rate"][h] = pos / n, share / n, split / n
    return out


def replay_votes(forward, task, obs0, act, rec, lengths, inds, mode, E, obs_dim, done_members="elite", cost_members="elite",
                 learned_done=None, learned_cost=False, term=None, after_step=None):
    """The whole replay under the vote.  forward(h, cur_obs) -> (pred, mean, var): what a model step from cur_obs returns for ALL
    B rows WITHOUT the votes (the elite's verdicts in pred['term'] / pred['cost']) and the members' outputs [E, B, out];
    learned_done(h, mean) -> [B] bool: the termination head's verdict of the step (None: no head).  The step's term / cost are then
    rule_votes_ref.rule_votes's under the two modes.  after_step(h, record): called behind every step with its record.  Returns
    (plain table, vote table, cur_obs, alive, per-step records)."""
    H = np.asarray(rec["next_obs"]).shape[0]
    vt = new_table(H)
    steps = []
    state = {}

    def step(h, cur_obs):
        pred, mean, var = forward(h, cur_obs)
        ld = None if learned_done is None else learned_done(h, mean)
        out = vref.rule_votes(task, np.asarray(cur_obs, F32), np.asarray(act[h], F32), mean, var, inds[h], obs_dim, done_members,
                              cost_members, learned_done=ld, learned_cost=learned_cost)
        pred = dict(pred)
        pred["term"] = out["term"]
        if not learned_cost:
            pred["cost"] = out["cost"]
        state.update(pred=pred, out=out)
        return pred

    # ref.replay calls step, then compare, then on_step: the histogram needs `alive` as it stood BEFORE compare
    def on_step(h, cur_before, alive_before, cur_obs, alive):
        out, pred = state["out"], state["pred"]
        ok = votes(vt, h, alive_before, pred, rec, E, out["done_votes"], out["cost_votes"], term)
        steps.append(dict(pred=pred, done_votes=out["done_votes"], cost_votes=out["cost_votes"], alive=alive.copy(),
                          alive_before=alive_before, entered=ok, cur_obs=cur_obs.copy()))
        if after_step is not None:
            after_step(h, steps[-1])

    tab, cur, alive = ref.replay(step, obs0, rec, lengths, mode, on_step=on_step)
    return tab, vt, cur, alive, steps
