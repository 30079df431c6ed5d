"""GPU: CMBPO(m_validate_reliability=, m_recalibrate_cost=, m_recalibrate_term=) on the toy world with both logistic heads (DESIGN
3z) -- the reliability keys of the per-epoch validation, that measuring reliability reads and does not steer (policy and dynamics
model after two epochs are bitwise those of the run with m_validate_horizon alone), and the two logit offsets after every
validation, in force and in the checkpoint."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_replay_calibration_cmbpo_gpu import _same_bits, _two_epochs  # noqa: E402  (the toy-world loop; keys ride in as **kw)

HEADS = dict(m_learn_cost=True, m_cost_loss="logistic", m_learn_term=True, m_term_loss="logistic", m_term_sampling=True)
REL_KEYS = [k % name for name in ("cost", "term") for k in ("ece_%s_h1", "logloss_%s_h1", "base_rate_%s_h1", "mean_p_%s_h1")] + ["rel_skipped"]


def test_reliability_reports_and_does_not_steer(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    algo, on, pi_on, w_on = _two_epochs(m_validate_horizon=5, m_validate_windows=256, m_validate_reliability=True,
                                        m_reliability_bins=10, **HEADS)
    _, off, pi_off, w_off = _two_epochs(m_validate_horizon=5, m_validate_windows=256, **HEADS)
    assert len(on) == len(off) == 2
    for d, d_off in zip(on, off):
        for k in REL_KEYS:
            assert "model/val_" + k in d and np.isfinite(d["model/val_" + k]), k
            assert "model/val_" + k not in d_off
        assert "model/cost_recal_offset" not in d and "model/term_recal_offset" not in d
        for name in ("cost", "term"):
            assert 0.0 <= d["model/val_ece_%s_h1" % name] <= 1.0 and d["model/val_logloss_%s_h1" % name] > 0.0
            assert 0.0 <= d["model/val_base_rate_%s_h1" % name] <= 1.0 and 0.0 < d["model/val_mean_p_%s_h1" % name] < 1.0
        assert d["model/val_rel_skipped"] >= 0
        for k, v in d_off.items():                                  # the keys of the validation as it was: the same values
            if k.startswith("model/val_"):
                assert d[k] == v or (np.isnan(d[k]) and np.isnan(v)), k
    rel = algo.last_validation["reliability"]
    assert sorted(rel) == ["cost", "term"]
    for col in rel.values():
        assert col["elite"]["n"].shape == (5, 10) and col["pooled"]["conf"].shape == (5, 10)
        np.testing.assert_array_equal(col["n_rel"] + col["n_skipped"], algo.last_validation["n"])
    assert algo.fake_env.cost_recalibration == 0.0 and algo.model_sampler.term_logit_offset is None
    _same_bits(pi_on, pi_off)
    assert len(w_on) == len(w_off) == 6
    for a, b in zip(w_on, w_off):
        _same_bits(a, b)


def test_recalibration_follows_the_validation(hip_lib, tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cmbpo_amd import replay
    lo, hi = -1.5, 1.0
    seen = []

    def on_epoch(algo, d):
        rel = algo.last_validation["reliability"]
        want_c = replay.logit_offset(rel, "cost", "elite", 0, lo, hi)
        want_t = replay.logit_offset(rel, "term", "elite", 0, lo, hi)
        prev = seen[-1] if seen else (0.0, 0.0)
        want_c = prev[0] if want_c is None else want_c             # fewer than 100 rows: what it had
        want_t = prev[1] if want_t is None else want_t
        env, sampler = algo.fake_env, algo.model_sampler
        assert env.cost_recalibration == want_c and (sampler.term_logit_offset or 0.0) == want_t
        assert lo <= want_c <= hi and lo <= want_t <= hi
        assert d["model/cost_recal_offset"] == want_c and d["model/term_recal_offset"] == want_t
        # the kernels get the float32 sum, the table's own shift stays the class-weight undo
        assert env.cost_head_struct().logit_shift == float(np.float32(env.cost_logit_shift + want_c))
        assert env.reliability_columns()[0]["shift"] == env.cost_logit_shift
        seen.append((want_c, want_t, int(rel["cost"]["n_rel"][0])))

    algo, diags, pi, _ = _two_epochs(on_epoch, m_validate_horizon=3, m_validate_windows=256, m_validate_reliability=True,
                                     m_recalibrate_cost=True, m_recalibrate_term=True, m_recalibration_range=(lo, hi), **HEADS)
    assert len(seen) == 2 and np.isfinite(pi).all()
    assert max(s[2] for s in seen) >= 100, seen                        # an offset was derived, not only kept
    assert any(s[0] != 0.0 for s in seen) and any(s[1] != 0.0 for s in seen), seen
    # the rollouts of the next epoch would read them: the pool's cost head carries the sum after a reset
    algo.save(str(tmp_path))
    kept = json.load(open(tmp_path / ("recalibration_%d.json" % algo._epoch)))
    assert kept["cost_recal_offset"] == seen[-1][0] and kept["term_recal_offset"] == seen[-1][1]
    assert kept["m_recalibrate_cost"] is True and kept["m_recalibrate_term"] is True and kept["m_recalibration_range"] == [lo, hi]
    algo.fake_env.set_cost_recalibration(0.0)
    algo.model_sampler.set_term_logit_offset(None)
    algo.load(str(tmp_path), algo._epoch)
    assert algo.fake_env.cost_recalibration == seen[-1][0] and (algo.model_sampler.term_logit_offset or 0.0) == seen[-1][1]
