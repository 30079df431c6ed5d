"""GPU: CMBPO(m_validate_particles=S) on the toy world -- the particle pass of the per-epoch validation logs its
model/val_* entries with finite values, and reads without steering: policy, dynamics model and every other model/val_* entry after
two epochs are bitwise those of the run that validates without it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_replay_cmbpo_gpu import _two_epochs  # noqa: E402

NEW = ("crps_h1", "crps_hH", "rank_dev_h1", "rank_dev_hH", "outlier_rate_hH", "spread_skill_h1", "spread_skill_hH",
       "particles_nonfinite")


def test_particle_validation_reports_and_does_not_steer(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    algo, on, pi_on, w_on = _two_epochs(m_validate_horizon=5, m_validate_windows=256, m_validate_particles=4)
    _, off, pi_off, w_off = _two_epochs(m_validate_horizon=5, m_validate_windows=256)
    assert len(on) == len(off) == 2
    for d_on, d_off in zip(on, off):
        for k in NEW:
            assert "model/val_" + k in d_on and "model/val_" + k not in d_off, k
            assert np.isfinite(d_on["model/val_" + k]), (k, d_on["model/val_" + k])
        assert d_on["model/val_crps_h1"] > 0 and 0 <= d_on["model/val_rank_dev_hH"] <= 1 and 0 <= d_on["model/val_outlier_rate_hH"] <= 1
        others = sorted(k for k in d_off if k.startswith("model/val_"))
        assert others == sorted(k for k in d_on if k.startswith("model/val_") and k[len("model/val_"):] not in NEW)
        for k in others:
            assert np.float64(d_on[k]).tobytes() == np.float64(d_off[k]).tobytes(), k
    part = algo.last_validation["particles"]
    assert part["S"] == 4 and part["rank_hist"].shape == (5, algo.obs_dim + 1, 5) and part["n"][0] + part["n_nonfinite"][0] == 256
    np.testing.assert_array_equal(pi_on.view(np.uint32), pi_off.view(np.uint32))
    assert len(w_on) == len(w_off)
    for a, b in zip(w_on, w_off):
        np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))
    # fewer particle windows than plain ones: the particle pass alone, on the first of them
    few = algo.validate_model(n_windows=128)
    assert np.isfinite(few["val_crps_h1"]) and algo.last_validation["particles"]["n"][0] <= 128 == algo.last_validation["n"][0] + algo.last_validation["n_nonfinite"][0]
    algo._validate_particle_windows = 32
    few = algo.validate_model(n_windows=128)
    pt = algo.last_validation["particles"]
    assert pt["n"][0] + pt["n_nonfinite"][0] == 32 and np.isfinite(few["val_rank_dev_h1"])


def test_particles_without_a_validation_horizon_are_refused(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with pytest.raises(ValueError, match="m_validate_particles needs m_validate_horizon > 0"):
        _two_epochs(m_validate_particles=4, m_validate_horizon=0)
    with pytest.raises(ValueError, match="power of two"):
        _two_epochs(m_validate_particles=3, m_validate_horizon=5)
