"""CPU: the weighted float64 reference (tests/policy_weights_ref.py) is pinned by the one sentence that defines the feature
-- a sample of weight w behaves as w copies of itself -- against the UNWEIGHTED oracle on the batch with row i repeated
w_i times; and the two new C entry points are exported, bound and validate their arguments before any HIP call."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import policy_weights_ref as wref  # noqa: E402
import ppo_lag_ref as ref  # noqa: E402

RTOL = 1e-10


def _case(D=11, A=3, n=150, seed=5, T=35):
    from worlds import make_update_batch
    rng = np.random.default_rng(seed)
    params, batch = make_update_batch(rng, n, D, A, 128, 0.3, 1.0, T)
    p = params.astype(np.float64) + 0.03 * rng.standard_normal(params.shape)
    w = rng.integers(0, 4, size=n)
    rep, _ = wref.replicate(batch, w)
    gw = wref.WeightedPolicyGraph(D, A, batch, w, ent_reg=0.01, max_path_length=T)
    gr = ref.make_graph(D, A, rep, ent_reg=0.01, max_path_length=T)
    return rng, p, w, gw, gr


def _vec_close(a, b, msg):
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=RTOL * float(np.abs(b).max()), err_msg=msg)


def test_weighted_reference_equals_the_oracle_on_the_replicated_batch():
    rng, p, w, gw, gr = _case()
    assert (w == 0).any() and (w == 3).any()
    for a, b, name in zip(gw.grads(p), gr.grads(p), ("flat_g", "flat_b", "pi_loss", "surr_cost")):
        _vec_close(np.asarray(a), np.asarray(b), name)
    v = rng.standard_normal(p.shape)
    _vec_close(gw.fisher_vp(p, v, 0.1), gr.fisher_vp(p, v, 0.1), "fisher_vp")
    _vec_close(gw.hvp(p, v, 0.1), gr.hvp(p, v, 0.1), "hvp")
    np.testing.assert_allclose(gw.evals(p), gr.evals(p), rtol=RTOL, atol=1e-15)
    np.testing.assert_allclose(float(gw.cur_cret_avg()), float(gr.cur_cret_avg()), rtol=RTOL)


@pytest.mark.parametrize("clipped,penalized", [(True, True), (False, True), (True, False)])
def test_weighted_surrogate_equals_the_surrogate_on_the_replicated_batch(clipped, penalized):
    rng, p, w, gw, gr = _case(seed=6)
    sw = wref.WeightedSurrogate(gw, clip_ratio=0.2, clipped_adv=clipped, objective_penalized=penalized)
    sr = ref.Surrogate(gr, clip_ratio=0.2, clipped_adv=clipped, objective_penalized=penalized)
    if clipped:
        assert sr.sums(p)[5] > 0          # some advantage terms are clipped away
    _vec_close(sw.grad(p, 0.7), sr.grad(p, 0.7), "ppo gradient")
    np.testing.assert_allclose(sw.sums(p), sr.sums(p), rtol=RTOL, atol=1e-12)


def test_trust_weight_formula_and_order():
    cumvar = np.array([[0.0, 1e-2, 3.0], [1e-2, 5.0, 7.0]])       # [T = 2, B = 3]
    got = wref.trust_weights(cumvar, [2, 0, 1], 1e-2)
    np.testing.assert_allclose(got, np.array([1.0, 0.5, 1e-2 / 3.01], np.float32), rtol=1e-7)
    assert got.dtype == np.float32


def test_new_symbols_are_exported_and_refuse_null_without_a_gpu():
    import __graft_entry__ as g
    g.build()
    from cmbpo_amd import _lib
    lib = _lib.lib()
    for name in ("cmbpo_pi_set_sample_weights", "cmbpo_buffer_trust_weights"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert lib.cmbpo_pi_set_sample_weights(None, None, 0, None) == -1
    assert b"cmbpo_pi_set_sample_weights" in lib.cmbpo_last_error()
    assert lib.cmbpo_buffer_trust_weights(None, None, 1e-2, None, None) == -1
    assert b"cmbpo_buffer_trust_weights" in lib.cmbpo_last_error()
