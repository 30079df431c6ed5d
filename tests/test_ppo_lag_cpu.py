"""CPU: the first-order update's C-ABI is exported, and its float64 reference (tests/ppo_lag_ref.py) collapses onto what is
already pinned: the trust-region oracle's gradient, central finite differences of its own objective, Adam's closed form."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import ppo_lag_ref as ref  # noqa: E402
from oracle import refupdate  # noqa: E402


def _batch(D, A, n, seed, hidden=128, shift=0.03):
    from worlds import make_update_batch
    rng = np.random.default_rng(seed)
    params, batch = make_update_batch(rng, n, D, A, hidden, 0.3, 1.0, 35)
    p = params.astype(np.float64) + shift * rng.standard_normal(params.shape)
    return rng, params, p, batch


def test_new_symbols_are_exported():
    import __graft_entry__ as g
    g.build()
    from cmbpo_amd import _lib
    lib = _lib.lib()
    for name in ("cmbpo_pi_ppo_grad", "cmbpo_vec_adam_step", "cmbpo_ppo_penalty_step", "cmbpo_pi_ppo_run"):
        assert hasattr(lib, name), name
    import ctypes as C
    assert C.sizeof(_lib.PiPpoCfgStruct) == 40
    # argument validation happens before any HIP call
    assert lib.cmbpo_vec_adam_step(0, None, None, None, None, None, 1e-3, 0.9, 0.999, 1e-8, None) == -1
    assert lib.cmbpo_ppo_penalty_step(None, None, 25.0, 1.0, 0.05, 1, None) == -1
    assert lib.cmbpo_pi_ppo_run(None, None, None, None, None, None, None, 1, None) == -1


def test_reference_without_clip_and_penalty_is_the_trust_region_gradient():
    D, A, n = 11, 3, 200
    rng, params, p, batch = _batch(D, A, n, seed=3)
    graph = ref.make_graph(D, A, batch, ent_reg=0.01)
    for penalized, penalty in ((True, 0.0), (False, 3.0)):
        sur = ref.Surrogate(graph, clipped_adv=False, objective_penalized=penalized)
        g_ref = graph.grads(p)[0]
        np.testing.assert_allclose(sur.grad(p, penalty), g_ref, rtol=1e-12, atol=1e-15)
    s = ref.Surrogate(graph, clipped_adv=False).sums(p)
    assert s[5] == 0 and s[1] == s[6]
    np.testing.assert_allclose(s[3] / n, graph.evals(p)[0], rtol=1e-12)


def test_reference_gradient_matches_finite_differences():
    D, A, n, H = 3, 1, 16, 128
    rng, params, p, batch = _batch(D, A, n, seed=D * 100 + A, shift=0.03)
    graph = ref.make_graph(D, A, batch, hidden=H, ent_reg=0.02)
    sur = ref.Surrogate(graph, clip_ratio=0.2)
    ratio = sur.ratio(p)
    assert np.min(np.abs(ratio - 0.8)) > 1e-3 and np.min(np.abs(ratio - 1.2)) > 1e-3    # no sample on a clip edge
    penalty = 1.7
    g = sur.grad(p, penalty)
    f = lambda q: float(sur.pi_loss(torch.as_tensor(q, dtype=torch.float64), penalty))
    idx = np.concatenate([rng.choice(p.size, 40, replace=False), [p.size - 1]])       # ... and log_std
    h = 1e-6
    for i in idx:
        e = np.zeros_like(p)
        e[i] = h
        fd = (f(p + e) - f(p - e)) / (2 * h)
        np.testing.assert_allclose(g[i], fd, rtol=1e-5, atol=1e-9, err_msg=str(i))
    assert np.abs(g).max() > 0


def test_agent_refuses_unknown_hyper_parameters():
    from cmbpo_amd.cpo_update import PPOLagAgent
    assert PPOLagAgent(pi_iters=3, clip_ratio=0.1).pi_iters == 3
    with pytest.raises(TypeError):
        PPOLagAgent(pi_iter=3)


@pytest.mark.parametrize("param_loss", [True, False])
def test_reference_penalty_step_is_adams_closed_form(param_loss):
    for param, excess in ((0.5413, 3.0), (0.5413, -3.0), (-2.0, 0.25), (4.0, -40.0), (0.0, 1e-3)):
        pen = ref.penalty_step(dict(param=param, m=0.0, v=0.0, t=0), 25.0 + excess, 25.0, 5e-2, param_loss)
        want = ref.penalty_first_step_closed_form(param, 25.0 + excess, 25.0, 5e-2, param_loss)
        np.testing.assert_allclose(pen["param"], want, rtol=1e-12)
        assert (pen["param"] > param) == (excess > 0) and pen["t"] == 1
        # the step is lr in size whatever the excess (Adam), the penalty moves with it
        np.testing.assert_allclose(abs(pen["param"] - param), 5e-2, rtol=2e-3)
        assert (ref.softplus(pen["param"]) > ref.softplus(param)) == (excess > 0)
