"""CPU: the G14 fixtures (imagined-rollout traces with a learned cost head, tests/golden/make_golden_learned_cost.py) are
consistent with the world builder the GPU tests rebuild them from -- the first step of every trace, recomputed with the
oracle's generic pieces (policy forward, ensemble forward) from the recorded start states and draws, gives the recorded
first costs: the elite member's mean of column obs + 1.  Pins fixture and builder to each other without a GPU."""
import os
import sys

import numpy as np
import pytest

from oracle import refcpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
TRACES = ["g14_trace_cost_hopper_budget", "g14_trace_cost_ant_term", "g14_trace_cost_hcs_sched", "g14_trace_cost_ant_unc"]
G5_KEYS_FROM = "g5_trace_ant_term"


@pytest.mark.parametrize("name", TRACES)
def test_fixture_first_step_costs_follow_from_the_world(name):
    from worlds_learned_cost import build_world_learned_cost
    g = np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)
    g5 = np.load(os.path.join(GOLD, G5_KEYS_FROM + ".npz"), allow_pickle=False)
    assert sorted(k for k in g.files if not k.startswith("diag_")) == sorted(k for k in g5.files if not k.startswith("diag_"))
    task, B, hidden = str(g["task"]), int(g["B"]), int(g["hidden"])
    w = build_world_learned_cost(int(g["seed"]), task, hidden, out_scale=float(g["out_scale"]), q_boost=float(g["q_boost"]))
    D = w["obs_dim"]
    assert w["ws"][2].shape[2] == 2 * (D + 2) and w["sc_out"][0].shape == (1, D + 2)
    start, eps, inds = g["start"], g["eps"][0], g["inds"][0]
    assert int(g["n_rows"][0]) == B and set(np.unique(inds)) <= set(w["elites"])
    act = refcpu.policy_forward(start, w["pol"], eps)["pi"]
    mean, _ = refcpu.ens_forward(np.concatenate([start, act], -1).astype(np.float32), w["ws"], w["bs"], w["sc_in"], w["sc_out"])
    assert mean.shape == (7, B, D + 2)
    want = mean[inds, np.arange(B), D + 1]
    # get() is branch-major, time-minor: the first stored sample of a branch is its start state, bit for bit
    obs, cost = g["get_obs"], g["get_cost"]
    assert cost.dtype == np.float32 and cost.shape == (obs.shape[0],)
    first = np.array([np.flatnonzero((obs == start[b]).all(-1))[0] for b in range(B)])
    assert (np.diff(first) > 0).all()
    np.testing.assert_allclose(cost[first], want, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(g["get_act"][first], act, rtol=1e-6, atol=1e-6)
    # the spread the generator asserted, and costs that are no rule's masks
    assert float(np.std(cost)) >= 0.5 and not np.isin(cost, (0.0, 1.0)).all()
    if name == "g14_trace_cost_ant_term":
        assert (np.diff(g["n_rows"]) < 0).any()        # static terminations, with the static cost unused
