"""NumPy specification of the learned termination head (cmbpo_fakeenv_post_term, include/cmbpo_hip.h).

The model's LAST output column, ``tc = obs_dim + 1 + learned_cost``, is trained on the real ``done`` flags (target units 0 / 1).
For a row r with the members' means ``mean[E, ., tc + 1]``:

    x_e          = mean[e, r, tc]
    hit_e        = x_e > threshold                 written positively: a NaN never hits, +inf does, -inf does not
    votes        = sum_e hit_e                     over ALL E members
    learned_done = hit_elite (ELITE) | votes > 0 (ANY) | 2 * votes > E (MAJORITY)
    term         = rule_done | learned_done
    term_pred    = x_elite  (float32, as it is)    term_votes = votes (uint8)

Pure comparisons and counts: everything here is compared with the device bit for bit."""
import numpy as np

ELITE, ANY, MAJORITY = 0, 1, 2
MEMBERS = {"elite": ELITE, "any": ANY, "majority": MAJORITY}


def term_column(obs_dim, learned_cost):
    return int(obs_dim) + 1 + (1 if learned_cost else 0)


def term_head(mean, inds, obs_dim, learned_cost, threshold, members, rows=None, rule_done=None):
    """(term, term_pred, term_votes, learned_done) of the rows `rows` (default: all) of mean[E, B, tc + 1]; `rule_done` (bool or
    uint8, one per row of `rows`) is the termination rule's own verdict, default: none ends."""
    mean = np.asarray(mean)
    assert mean.dtype == np.float32 and mean.ndim == 3
    tc = term_column(obs_dim, learned_cost)
    assert mean.shape[2] == tc + 1, "the termination column is the last one"
    members = MEMBERS.get(members, members)
    assert members in (ELITE, ANY, MAJORITY)
    E = mean.shape[0]
    rows = np.arange(mean.shape[1]) if rows is None else np.asarray(rows)
    inds = np.asarray(inds)[rows]
    x = mean[:, rows, tc]                                     # [E, n]
    with np.errstate(invalid="ignore"):
        hit = x > np.float32(threshold)
    votes = hit.sum(axis=0)
    cols = np.arange(len(rows))
    if members == ELITE:
        learned = hit[inds, cols]
    elif members == ANY:
        learned = votes > 0
    else:
        learned = 2 * votes > E
    rule = np.zeros(len(rows), bool) if rule_done is None else np.asarray(rule_done).astype(bool)
    term = (rule | learned).astype(np.uint8)
    return term, x[inds, cols].copy(), votes.astype(np.uint8), learned


def term_targets(done, path_len, horizon):
    """The training target of the column for the steps of ONE path: 1 only on a last step whose `done` the environment reported
    before the sampler's horizon; a path that ran to the horizon is a time-out, whatever the environment's own time limit says."""
    done = np.asarray(done).astype(bool)
    t = np.zeros(len(done), np.float32)
    if len(done) and done[-1] and path_len < horizon:
        t[-1] = 1.0
    return t
