"""The worlds and recordings of the replay-votes tests, NumPy only: a small synthetic ensemble per rule set whose
members DISAGREE on the columns the rules test, windows that start and continue around the rules' boundaries, and synthetic
recorded flags.  ``first_step_votes`` runs the first replay step on the oracle's CPU forward: the fixture conditions -- at h = 0
at least a tenth of the rows split on every signal tested, each recorded class with at least 5 % of the split rows -- are checked
from it without a GPU, and again on the device's own forward by the GPU tests.

The members' disagreement is planted, not hoped for: on every column a rule tests, the last layer's biases of the E members are
the points of linspace(-1.3, 1.3, E) in a shuffled order and the output sigma is the spread wanted (RULE_COLS: 0.12 around a
threshold the start states are drawn about as wide around, 0.6 on the columns tested against 3.2), so the members' next states
differ by about that much on every row, whatever the random network adds (about 0.05 sigma)."""
import zlib

import numpy as np

F32 = np.float32
DIMS = {"ant": (27, 8), "hcs": (18, 6), "table29": (29, 8)}
SIGNALS = {"ant": ("cost", "term"), "hcs": ("cost",), "table29": ("cost", "term")}      # HCS has no termination rule
RULE_COLS = {"ant": {0: 0.12, 2: 0.12, 3: 0.12, 26: 0.6}, "hcs": {17: 0.08},
             "table29": {0: 0.12, 2: 0.12, 3: 0.12, 4: 0.15, 5: 0.15, 6: 0.1, 7: 0.3, 27: 0.6, 28: 0.6}}
_TABLE = {}


def task_of(kind):
    """What FakeEnv and the reference take as `task`: a built-in name, or the one registered TaskRules of this module (derived
    quantities, require_finite, cost_on_term)."""
    if kind == "ant":
        return "AntSafe-v2"
    if kind == "hcs":
        return "HalfCheetahSafe-v2"
    if not _TABLE:
        from cmbpo_amd.statics import TaskRules, cost, derived, dist_sq, fatal, healthy, term, tilt
        _TABLE["table29"] = TaskRules(
            [healthy(cols=0, lo=0.2, hi=1.0), healthy(src="derived", cols=0, lo=-0.7),
             cost(src="derived", cols=slice(1, 3), any=True, hi=0.25),
             cost(cols=slice(-2, None), abs=True, lo=3.2, lo_strict=True, any=True), fatal(src="derived", cols=3, lo=2.5)],
            derived=[tilt(2, 3), dist_sq((4, 5), (1.0, -2.0)), dist_sq((4, 5), (3.0, 0.5)),
                     derived([term(6, src="obs"), term(0, src="act", w=0.5), term(7, w=-1.0)], bias=0.1)],
            require_finite=True, cost_on_term=True)
    return _TABLE[kind]


def world(kind, E, extra_cols=0):
    """(ws, bs, scaler_in, scaler_out, D, A, O) of the ensemble of `kind`; extra_cols: a learned-cost or termination column behind
    the reward (its values spread around 0.5, the threshold of both readings)."""
    from cmbpo_amd import synthetic
    D, A = DIMS[kind]
    O = D + 1 + extra_cols
    rng = np.random.default_rng(zlib.crc32(f"replay-votes-world/{kind}/{E}/{extra_cols}".encode()))
    ws, bs = synthetic.ensemble_weights(rng, E, D + A, 128, 2 * O, bias_scale=0.05)
    mu, var = np.zeros((1, O), F32), np.ones((1, O), F32)
    for c, sigma in RULE_COLS[kind].items():
        var[0, c] = sigma * sigma
        bs[2][:, 0, c] = rng.permutation(np.linspace(-1.3, 1.3, E)).astype(F32)
    for c in range(D + 1, O):
        mu[0, c], var[0, c] = 0.45, 16.0
    sc_in = (np.zeros((1, D + A), F32), np.ones((1, D + A), F32))
    return ws, bs, sc_in, (mu, var), D, A, O


def states(kind, rng, n):
    """[n, D] observations with every column a rule of `kind` tests drawn around its threshold."""
    D, _ = DIMS[kind]
    obs = (rng.standard_normal((n, D)) * 0.3).astype(F32)
    put = lambda c, x: obs.__setitem__((slice(None), c), np.asarray(x, F32))
    if kind in ("ant", "table29"):
        put(0, rng.uniform(0.1, 1.1, n))                                               # the height band [0.2, 1.0]
        put(2, rng.standard_normal(n) * 0.6)                                           # the quaternion: z_rot / tilt at -0.7
        put(3, rng.standard_normal(n) * 0.6)
    if kind == "ant":
        put(D - 1, rng.standard_normal(n) * 3.0)                                       # |x| > 3.2
    if kind == "hcs":
        put(D - 1, rng.standard_normal(n) * 0.25)                                      # |10 x| < 2
    if kind == "table29":
        centre = np.where(rng.random(n) < 0.5, 0, 1)
        put(4, np.array([1.0, 3.0])[centre] + rng.standard_normal(n) * 0.35)           # the two circles of radius 0.5
        put(5, np.array([-2.0, 0.5])[centre] + rng.standard_normal(n) * 0.35)
        put(6, rng.standard_normal(n) * 1.5)
        put(7, rng.standard_normal(n) * 1.5)
        put(D - 2, rng.standard_normal(n) * 2.5)
        put(D - 1, rng.standard_normal(n) * 2.5)
    return obs


def recording(kind, B, H, seed):
    """(obs0, act, rec, lengths, term_targets): B windows of H steps whose every real state lies around the rules' boundaries
    (one_step replays continue from them), ragged lengths, a few recorded terminals, 0/1 costs on two fifths of the steps; row 3
    of a replay of 64 windows or more starts at a NaN.  term_targets [H, B]: flags of the vote table's own."""
    D, A = DIMS[kind]
    rng = np.random.default_rng(zlib.crc32(f"replay-votes-rec/{kind}/{B}/{H}/{seed}".encode()))
    obs0 = states(kind, rng, B)
    if B >= 64:
        obs0[3, 1] = np.nan
    rec = dict(next_obs=np.stack([states(kind, rng, B) for _ in range(H)]), rew=rng.standard_normal((H, B)).astype(F32),
               cost=(rng.random((H, B)) < 0.4).astype(F32), term=(rng.random((H, B)) < 0.08).astype(np.uint8))
    act = rng.uniform(-1, 1, (H, B, A)).astype(F32)
    lengths = rng.integers(1, H + 1, B).astype(np.int32)
    lengths[: max(B // 2, 1)] = H
    targets = (rng.random((H, B)) < 0.4).astype(np.uint8)
    return obs0, act, rec, lengths, targets


def fixture_conditions(kind, E, done_votes, cost_votes, entered, y_cost, y_term, learned_cost=False):
    """The two conditions on a case of B >= 64 at h = 0, from the reference's votes: {signal: (split share, share of y = 0 among
    the split rows, of y = 1)}, asserted here."""
    out = {}
    for sig in SIGNALS[kind]:
        if sig == "cost" and learned_cost:
            continue
        v, y = (cost_votes, y_cost) if sig == "cost" else (done_votes, y_term)
        split = entered & (v > 0) & (v < E)
        share = split.sum() / max(entered.sum(), 1)
        c0, c1 = (split & ~y).sum() / max(split.sum(), 1), (split & y).sum() / max(split.sum(), 1)
        out[sig] = (float(share), float(c0), float(c1))
        assert share >= 0.10, (kind, E, sig, "split share", share)
        assert c0 >= 0.05 and c1 >= 0.05, (kind, E, sig, "recorded classes among the split rows", c0, c1)
    return out


def first_step_votes(kind, E, B, H, seed, inds, extra_cols=0, learned_cost=False):
    """The first replay step on the oracle's CPU forward: (done_votes, cost_votes or None, entered) of rule_votes_ref."""
    import rule_votes_ref as vref
    from oracle import refcpu
    ws, bs, sc_in, sc_out, D, A, O = world(kind, E, extra_cols)
    obs0, act, rec, lengths, targets = recording(kind, B, H, seed)
    with np.errstate(all="ignore"):
        mean, var = refcpu.ens_forward(np.concatenate([obs0, act[0]], axis=1), ws, bs, sc_in, sc_out)
        out = vref.rule_votes(task_of(kind), obs0, act[0], mean, var, inds, D, learned_cost=learned_cost)
    entered = np.isfinite(out["nx_elite"]).all(axis=1)
    return out["done_votes"], out["cost_votes"], entered, rec, targets


H = 3
VOTES = (("elite", "elite"), ("any", "any"), ("majority", "mean"))        # measure-only, any / any, majority / mean


def cases():
    """(kind, E, (done_members, cost_members), replay mode, B, head): the pruned product.  Every rule set with two ensemble sizes
    under every vote; B in {1, 64, 65, 1003} (one partial slot, exactly one, two, many with a ragged tail) and the two replay
    modes rotate through them so that each B but 64 / 65 meets both modes; then a thresholded termination head under 'majority' and a
    learned cost (the termination half only)."""
    out = []
    pairs = ((1, 65), (64, 1003), (64, 1), (65, 1003))
    for i, (kind, E) in enumerate((("ant", 7), ("ant", 3), ("hcs", 8), ("hcs", 3), ("table29", 7), ("table29", 8))):
        for j, vm in enumerate(VOTES):
            k = 3 * i + j
            mode = "open_loop" if k % 4 in (0, 3) else "one_step"
            for B in pairs[k % 4]:
                out.append((kind, E, vm, mode, B, None))
    out.append(("ant", 7, ("majority", "mean"), "open_loop", 65, "term"))
    out.append(("table29", 8, ("any", "elite"), "one_step", 65, "cost"))
    return out


def case_id(c):
    kind, E, vm, mode, B, head = c
    return f"{kind}-E{E}-{vm[0]}.{vm[1]}-{mode}-B{B}" + (f"-{head}" if head else "")


def case_inds(c):
    """[H, B] members of the case (any member may be a window's elite here)."""
    kind, E, vm, mode, B, head = c
    rng = np.random.default_rng(zlib.crc32(("replay-votes-inds/" + case_id(c)).encode()))
    return rng.integers(0, E, (H, B)).astype(np.int32)
