"""NumPy restatement of the sampled terminations (cmbpo_fakeenv_post_term_draws, include/cmbpo_hip.h): the learned termination
head of tests/term_head_ref.py with a threshold per row in place of the head's one scalar.

For a row r with the members' means ``mean[E, n, out]`` (the termination column is the LAST one), the row's elite ``elite[r]`` and
the row's threshold ``thr[r]`` (float32, the column's own units):

    x_e          = mean[e, r, out - 1]
    hit_e        = x_e > thr[r]                    the header's rule; written positively, as NumPy's comparison is
    votes        = sum_e hit_e                     over ALL E members, which share the row's threshold
    learned_done = hit_elite (ELITE) | votes > 0 (ANY) | 2 * votes > E (MAJORITY)
    term         = rule_done | learned_done
    term_pred    = x_elite  (float32, as it is)    term_votes = votes (uint8)

Pure comparisons and counts: everything here is compared with the device bit for bit."""
import numpy as np

ELITE, ANY, MAJORITY = 0, 1, 2
MEMBERS = {"elite": ELITE, "any": ANY, "majority": MAJORITY}


def term_draws(mean, elite, thr, members, rule_done=None):
    """(term uint8 [n], term_pred float32 [n], term_votes uint8 [n]) of the n rows of mean[E, n, out]; elite [n] ints, thr [n]
    float32, members 'elite' / 'any' / 'majority' (or 0 / 1 / 2), rule_done [n] the termination rule's own verdict (None: no
    rule ends a row)."""
    mean = np.asarray(mean)
    assert mean.dtype == np.float32 and mean.ndim == 3
    E, n, _ = mean.shape
    elite, thr = np.asarray(elite), np.asarray(thr)
    assert thr.dtype == np.float32 and thr.shape == (n,) and elite.shape == (n,)
    members = MEMBERS.get(members, members)
    assert members in (ELITE, ANY, MAJORITY)
    x = mean[:, :, -1]                                       # [E, n]
    with np.errstate(invalid="ignore"):
        hit = x > thr[None, :]
    votes = hit.sum(axis=0)
    cols = np.arange(n)
    if members == ELITE:
        learned = hit[elite, cols]
    elif members == ANY:
        learned = votes > 0
    else:
        learned = 2 * votes > E
    rule = np.zeros(n, bool) if rule_done is None else np.asarray(rule_done).astype(bool)
    return (rule | learned).astype(np.uint8), x[elite, cols].copy(), votes.astype(np.uint8)
