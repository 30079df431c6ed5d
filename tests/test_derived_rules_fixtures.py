"""CPU: the G18 fixtures (imagined-rollout traces under rules with derived quantities, tests/golden/make_golden_derived_rules.py)
are consistent with worlds_derived.py and the world builder the GPU tests rebuild them from -- the first step of every trace,
recomputed with the oracle's generic pieces (policy forward, ensemble forward) from the recorded start states and draws and
put through ``TaskRules.numpy_fns()`` of the recorded thresholds, gives the recorded first costs and the recorded alive mask,
exactly; the hand-written natural NumPy functions of worlds_derived.py say the same.  Pins fixture, rules and builder to each
other without a GPU."""
import os
import sys

import numpy as np
import pytest

from oracle import refcpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
TRACES = ["g18_trace_derived_hazards", "g18_trace_derived_tilt"]
G5_KEYS_FROM = "g5_trace_ant_term"


@pytest.mark.parametrize("name", TRACES)
def test_fixture_first_step_follows_from_the_world_and_the_rules(name):
    import worlds_derived
    from worlds import build_world
    path = os.path.join(GOLD, name + ".npz")
    assert os.path.getsize(path) <= 520 * 1024
    g = np.load(path, allow_pickle=False)
    g5 = np.load(os.path.join(GOLD, G5_KEYS_FROM + ".npz"), allow_pickle=False)
    assert sorted(k for k in g.files if not k.startswith("diag_")) == \
        sorted([k for k in g5.files if not k.startswith("diag_")] + ["thresholds"])
    case = worlds_derived.CASES[name]
    thr = tuple(g["thresholds"].tolist())
    assert thr in [tuple(float(v) for v in c) for c in case["candidates"]]
    cfg = case["cfg"]
    assert (str(g["task"]), int(g["B"]), int(g["T"]), int(g["hidden"]), str(g["mode"]), int(g["budget"]), int(g["seed"])) == \
        (cfg["task"], cfg["B"], cfg["T"], cfg["hidden"], cfg["mode"], cfg["budget"] or 0, cfg["seed"])
    rules = worlds_derived.build_rules(case["rules"](*thr))
    assert rules.derived and any(c.src == "derived" for c in rules.clauses)
    term_fn, cost_fn = rules.numpy_fns()
    hand_term, hand_cost = case["fns"](*thr)
    B = int(g["B"])
    w = build_world(int(g["seed"]), str(g["task"]), int(g["hidden"]), out_scale=float(g["out_scale"]), q_boost=float(g["q_boost"]))
    D = w["obs_dim"]
    start, eps, inds = g["start"], g["eps"][0], g["inds"][0]
    assert int(g["n_rows"][0]) == B and set(np.unique(inds)) <= set(w["elites"])
    act = refcpu.policy_forward(start, w["pol"], eps)["pi"]
    mean, _ = refcpu.ens_forward(np.concatenate([start, act], -1).astype(np.float32), w["ws"], w["bs"], w["sc_in"], w["sc_out"])
    nxt = (mean[inds, np.arange(B), :D] + start).astype(np.float32)
    term, cost = term_fn(start, act, nxt), cost_fn(start, act, nxt)
    np.testing.assert_array_equal(cost, hand_cost(start, act, nxt))
    if hand_term is not None:
        np.testing.assert_array_equal(term, hand_term(start, act, nxt))
    else:
        assert not term.any()
    # the generator's margin, on this step: every tested value, derived ones in the clause's scaled units, keeps its distance
    dv = rules.derived_values(start, act, nxt)
    for cl in rules.clauses:
        for bound in (float(cl.lo), float(cl.hi)):
            if np.isfinite(bound):
                assert np.abs(cl.values(start, act, nxt, dv).astype(np.float64) - bound).min() >= 1e-3 * max(1.0, abs(bound))
    # get() is branch-major, time-minor: the first stored sample of a branch is its start state, bit for bit
    obs, gcost = g["get_obs"], g["get_cost"]
    first = np.array([np.flatnonzero((obs == start[b]).all(-1))[0] for b in range(B)])
    assert (np.diff(first) > 0).all()
    np.testing.assert_array_equal(gcost[first], cost[:, 0])
    np.testing.assert_array_equal(g["alive"][0], ~term[:, 0])
    # what the generator asserted about the whole trace
    assert 0.2 <= float(np.mean(gcost)) <= 0.8
    if hand_term is not None:
        assert (np.diff(g["n_rows"]) < 0).sum() >= 2 and g["n_rows"][-1] >= 0.25 * B
    else:
        assert (g["n_rows"] == B).all()
