"""GPU: CMBPO(m_validate_votes=True) on the toy loop of test_rule_votes_cmbpo_gpu.py (the point environment whose cost is a static
rule, judged by the share of members) -- the vote keys of the per-epoch validation, and that measuring them reads and does not
steer: policy and dynamics model after two epochs are bitwise those of the run without the flag."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

VOTE_KEYS = ("vote_ece_cost_h1", "vote_split_cost_h1", "vote_ece_term_h1", "vote_split_term_h1", "vote_skipped")
RATE_KEYS = tuple(f"{s}_{k}_rate_{m}" for s in ("cost", "term") for k in ("miss", "false_alarm") for m in ("any", "majority"))


def _two_epochs(**kw):
    from test_rule_votes_cmbpo_gpu import _build
    torch.manual_seed(0)
    algo = _build(m_static_cost_members='mean', m_validate_horizon=3, m_validate_windows=256, **kw)
    diags = []
    for d in algo.train():
        diags.append(d)
        if len(diags) >= 2:
            break
    ws, bs = algo._model.get_weights()
    return algo, diags, algo._policy.actor.get_flat_params(), [np.asarray(a) for a in ws + bs]


def _same_bits(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def test_validation_under_the_vote_reports_and_does_not_steer(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    algo, on, pi_on, w_on = _two_epochs(m_validate_votes=True)
    _, off, pi_off, w_off = _two_epochs()
    assert len(on) == len(off) == 2
    for d, d_off in zip(on, off):
        for k in VOTE_KEYS:
            assert "model/val_" + k in d and np.isfinite(d["model/val_" + k]), k
        for k in VOTE_KEYS + RATE_KEYS:
            assert "model/val_" + k in d and "model/val_" + k not in d_off, k
        assert d["model/val_vote_skipped"] == 0
        assert 0.0 <= d["model/val_vote_split_cost_h1"] <= 1.0 and 0.0 <= d["model/val_vote_ece_cost_h1"] <= 1.0
        assert d["model/val_vote_split_term_h1"] == 0.0            # the rule set has no termination clause: nobody ever votes
        # what does not depend on whose verdict the replay takes is what it was
        for k in ("model/val_n_h1", "model/val_mse_obs_h1", "model/val_nonfinite"):
            assert d[k] == d_off[k], k
    tab = algo.last_validation
    votes = tab["votes"]
    assert sorted(votes) == ["cost", "n_skipped", "n_vote", "term"] and votes["cost"]["hist"].shape == (3, 5, 2)
    np.testing.assert_array_equal(votes["n_vote"], tab["n"])
    # the replay ran under the trainer's own mode, 'mean': the plain table's cost verdicts are the strict majority's
    np.testing.assert_array_equal(tab["cost_cm"], votes["cost"]["cm"]["majority"])
    np.testing.assert_allclose(tab["mse_cost"][0], votes["cost"]["brier"][0], rtol=1e-6)
    _same_bits(pi_on, pi_off)
    assert len(w_on) == len(w_off) == 6
    for a, b in zip(w_on, w_off):
        _same_bits(a, b)
