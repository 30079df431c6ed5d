"""Seeded synthetic worlds whose dynamics ensemble has a learned cost head: 2 (obs + 2) raw outputs (delta-obs | reward |
cost, algorithms/cmbpo.py:46,123 with m_learn_cost=True).  Shared by make_golden_learned_cost.py and the tests of the
G14 traces, like worlds.build_world for G5.

Pure functions of a seed: nothing here touches the reference tree, so tests can import it on the GPU box.
"""
import numpy as np

# The output scaler of worlds.build_world has its variance scaled by 0.01 (deltas of a few 1e-2 per step, so a rollout stays
# in range; the raw outputs of these small random networks have a spread of 0.05 - 0.1).  The cost column's variance is
# scaled UP instead, by this factor: the predicted costs of a trace then spread over about one unit, where the traces'
# 2e-3 tolerance means something.
COST_VAR_SCALE = 100.0


def build_world_learned_cost(seed, task, hidden, E=7, out_scale=1.0, q_boost=0.0, cost_var_scale=COST_VAR_SCALE):
    """worlds.build_world with one more output column (the same draws in the same order, at the wider shapes)."""
    from cmbpo_amd import synthetic
    rng = np.random.default_rng(seed)
    obs_dim, act_dim = synthetic.ENV_DIMS[task]
    out_dim = obs_dim + 2
    ws, bs = synthetic.ensemble_weights(rng, E, obs_dim + act_dim, hidden, 2 * out_dim, bias_scale=0.05,
                                        out_scale=out_scale)
    if q_boost:
        bs[2][:, 0, 2] += q_boost      # pushes a quaternion dim so AntSafe's z_rot < -0.7 branch fires
    sc_in = synthetic.scaler(rng, obs_dim + act_dim, hit_clamp=False)
    mu, var = synthetic.scaler(rng, out_dim, hit_clamp=False)
    scale = np.full((1, out_dim), 0.01, np.float32)
    scale[0, obs_dim + 1] = cost_var_scale
    sc_out = (mu, (var * scale).astype(np.float32))
    pol = synthetic.policy_params(rng, obs_dim, act_dim)
    crit = []
    for _ in range(2):
        cw, cb = synthetic.ensemble_weights(rng, 3, obs_dim, 128, 1, bias_scale=0.05)
        crit.append((cw, cb, synthetic.scaler(rng, obs_dim, hit_clamp=False),
                     synthetic.scaler(rng, 1, hit_clamp=False)))
    elites = [0, 2, 3, 5, 6][: max(1, E - 2)]
    return dict(obs_dim=obs_dim, act_dim=act_dim, out_dim=out_dim, ws=ws, bs=bs, sc_in=sc_in, sc_out=sc_out, pol=pol,
                v=crit[0], vc=crit[1], elites=elites)
