"""CPU: the particle replay without a GPU -- the NumPy reference and the host's table function on a hand-checked case,
the closed form of the fair CRPS at S = 2, statistical sanity on NumPy draws (a calibrated, an under- and an over-dispersed
cloud), the struct image and the refusals of the C-ABI by name, and the FakeEnv.replay / CMBPO arguments.

The statistical bounds are the issue's: q, x_p ~ N(0, 1) i.i.d., W = 1024 windows, S = 8: chi2 below the 1e-6 quantile of
chi-square with S degrees of freedom (49.96), outlier_rate in [0.15, 0.30] around 2 / 9, crps within 0.02 of 1 / sqrt(pi) (the
expected CRPS of a standard normal forecast of a standard normal draw), spread_skill within 0.1 of 1; x_p scaled by 0.5 gives
outlier_rate > 0.35, by 2 gives < 0.13."""
import ctypes as C
import os

import numpy as np
import pytest

import particles_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cmbpo_amd import _lib
    return _lib.lib()


def _table(sums, counts, obs_dim, S):
    from cmbpo_amd.replay import particles_table
    return particles_table(sums, counts, obs_dim, S)


def _hand_case(mode):
    """S = 2, one observation column + the reward, B = 3, H = 2.  Window 0: a tie at h = 0 and a recorded terminal there;
    window 1: a NaN particle at h = 0; window 2: lives through both steps."""
    f, u8 = np.float32, np.uint8
    rec = dict(next_obs=np.array([[[3.0], [0.0], [0.0]], [[9.0], [9.0], [0.0]]], f),
               rew=np.array([[1.0, 0.0, 5.0], [0.0, 0.0, 1.0]], f), cost=np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]], f),
               term=np.array([[1, 0, 0], [0, 0, 0]], u8), length=np.array([2, 2, 2], np.int32))
    preds = [dict(p_next_obs=np.array([[1.0], [3.0], [np.nan], [2.0], [-1.0], [1.0]], f),
                  p_rew=np.array([0.5, 0.5, 0.0, 0.0, 2.0, 4.0], f), p_cost=np.array([0.25, 0.75, 0.0, 0.0, 0.0, 0.5], f),
                  p_term=np.array([1, 0, 0, 0, 0, 0], u8)),
             dict(p_next_obs=np.array([[7.0], [7.0], [7.0], [7.0], [0.0], [0.0]], f),
                  p_rew=np.array([7.0, 7.0, 7.0, 7.0, 1.0, 1.0], f), p_cost=np.zeros(6, f), p_term=np.array([1, 1, 1, 1, 1, 1], u8))]
    cur, alive = np.full((6, 1), 5.0, f), np.ones(6, u8)
    rows = [pref.step(h, 2, mode, rec["next_obs"], rec["rew"], rec["cost"], rec["term"], rec["length"], cur, alive, **preds[h])
            for h in range(2)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), cur, alive


@pytest.mark.parametrize("mode", [pref.OPEN_LOOP, pref.ONE_STEP])
def test_hand_checked_case(mode):
    sums, counts, cur, alive = _hand_case(mode)
    tab = _table(sums, counts, 1, 2)
    np.testing.assert_array_equal(tab["n"], [2, 1])
    np.testing.assert_array_equal(tab["n_nonfinite"], [1, 0])          # the NaN window: counted once, in nothing else
    # h = 0: window 0 has x = (1, 3) against q = 3 -- the tie ranks as not below, k = 1; window 2 x = (-1, 1) against 0, k = 1
    np.testing.assert_array_equal(tab["rank_hist"][0], [[0, 2, 0], [0, 0, 2]])
    np.testing.assert_array_equal(tab["rank_hist"][1], [[1, 0, 0], [1, 0, 0]])          # x = q twice: nothing below
    np.testing.assert_array_equal(tab["sum_abs"], [[2.0, 2.5], [0.0, 0.0]])
    np.testing.assert_array_equal(tab["sum_pair"], [[4.0, 2.0], [0.0, 0.0]])
    np.testing.assert_array_equal(tab["sum_se"], [[1.0, 4.25], [0.0, 0.0]])
    np.testing.assert_array_equal(tab["sum_var"], [[4.0, 2.0], [0.0, 0.0]])
    np.testing.assert_array_equal(tab["crps"], [[0.0, 0.75], [0.0, 0.0]])
    np.testing.assert_array_equal(tab["mae"], [[1.0, 1.25], [0.0, 0.0]])
    np.testing.assert_array_equal(tab["sum_brier_term"], [0.25, 1.0])     # a predicted termination is measured, it ends nothing
    np.testing.assert_array_equal(tab["sum_brier_cost"], [0.3125, 0.0])
    np.testing.assert_array_equal(tab["outlier_rate"], [[0.0, 1.0], [1.0, 1.0]])
    np.testing.assert_allclose(tab["rank_dev"][0], [2.0 / 3.0, 2.0 / 3.0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(tab["chi2"][0], [4.0, 4.0], rtol=0, atol=1e-12)
    # the recorded terminal ended window 0, the NaN window 1: their rows are frozen at what they held; window 2 went on and ended
    # with its length
    np.testing.assert_array_equal(alive, 0)
    want = [[5.0], [5.0], [5.0], [5.0], [-1.0], [1.0]] if mode == pref.OPEN_LOOP else [[5.0], [5.0], [5.0], [5.0], [0.0], [0.0]]
    np.testing.assert_array_equal(cur, np.array(want, np.float32))


def test_empty_horizon_is_nan_with_zero_counts():
    ns, nc = pref.sizes(3, 4)
    tab = _table(np.zeros((2, ns)), np.zeros((2, nc), np.int64), 3, 4)
    assert tab["S"] == 4 and tab["rank_hist"].shape == (2, 4, 5) and not tab["rank_hist"].any()
    for k in ("rank_freq", "rank_dev", "outlier_rate", "chi2", "mae", "crps", "spread", "mse_mean", "spread_skill", "brier_term",
              "brier_cost"):
        assert np.isnan(tab[k]).all(), k
    with pytest.raises(ValueError, match="particles_table"):
        _table(np.zeros((2, ns + 1)), np.zeros((2, nc), np.int64), 3, 4)
    for S in (3, 128, 1, 0):
        with pytest.raises(ValueError, match="power of two"):
            _table(np.zeros((2, ns)), np.zeros((2, nc), np.int64), 3, S)


def test_closed_form_at_two_particles():
    rng = np.random.default_rng(3)
    for _ in range(50):
        x = rng.standard_normal(2).astype(np.float32)
        q = np.float32(rng.standard_normal())
        k, a, g, se, v = pref.window_stats(x, q)
        d = lambda u, w: float(np.abs(np.float32(u - w)))
        assert a - 0.5 * g == pytest.approx(0.5 * (d(x[0], q) + d(x[1], q)) - 0.5 * d(x[0], x[1]), abs=1e-15)
        assert k == int(x[0] < q) + int(x[1] < q)
        assert v == pytest.approx(0.5 * (float(x[0]) - float(x[1])) ** 2, rel=1e-12)
        # ... and through the host's table: one window, one column (the reward column: the same particles against the same q)
        z, one = np.zeros((1, 1), np.float32), np.ones(1, np.int32)
        s, c = pref.step(0, 2, pref.OPEN_LOOP, np.full((1, 1, 1), q, np.float32), np.full((1, 1), q, np.float32), z, z.astype(np.uint8), one,
                         np.zeros((2, 1), np.float32), np.ones(2, np.uint8), x[:, None].copy(), x.copy(), np.zeros(2, np.float32),
                         np.zeros(2, np.uint8))
        tab = _table(s[None], c[None], 1, 2)
        want = 0.5 * (d(x[0], q) + d(x[1], q)) - 0.5 * d(x[0], x[1])
        np.testing.assert_allclose(tab["crps"][0], [want, want], rtol=0, atol=1e-15)
        np.testing.assert_allclose(tab["sum_abs"][0] - 0.5 * tab["sum_pair"][0], [want, want], rtol=0, atol=1e-15)
        assert tab["rank_hist"][0, 0, k] == 1 and tab["rank_hist"][0].sum() == 2


def test_statistical_sanity_of_a_calibrated_cloud():
    from scipy.stats import chi2
    W, S = 1024, 8
    tab = _table(*pref.iid_case(np.random.default_rng(20240), W, S), 1, S)
    assert tab["n"][0] == W and tab["rank_hist"][0].sum(axis=1).tolist() == [W, W]
    for c in range(2):
        print("calibrated column %d: chi2 %.3f outlier_rate %.4f crps %.4f spread_skill %.4f"
              % (c, tab["chi2"][0, c], tab["outlier_rate"][0, c], tab["crps"][0, c], tab["spread_skill"][0, c]))
        assert tab["chi2"][0, c] < chi2.isf(1e-6, S)
        assert 0.15 <= tab["outlier_rate"][0, c] <= 0.30
        assert abs(tab["crps"][0, c] - 1.0 / np.sqrt(np.pi)) < 0.02
        assert abs(tab["spread_skill"][0, c] - 1.0) < 0.1


def test_dispersion_shows_in_the_outlier_rate():
    W, S = 1024, 8
    narrow = _table(*pref.iid_case(np.random.default_rng(20241), W, S, scale=0.5), 1, S)
    wide = _table(*pref.iid_case(np.random.default_rng(20242), W, S, scale=2.0), 1, S)
    print("outlier_rate: under-dispersed %s, over-dispersed %s" % (narrow["outlier_rate"][0], wide["outlier_rate"][0]))
    assert (narrow["outlier_rate"][0] > 0.35).all() and (narrow["spread_skill"][0] < 0.9).all()
    assert (wide["outlier_rate"][0] < 0.13).all() and (wide["spread_skill"][0] > 1.1).all()


# ------------------------------------------------------------------------------------------------------------------
# the C-ABI without a device: every call fails a host-side check, the buffers are compared with NULL and never followed
# ------------------------------------------------------------------------------------------------------------------
def _image(_lib, S=8, obs_dim=11):
    ps = _lib.ReplayParticlesStruct()
    ps.B, ps.H, ps.S, ps.obs_dim, ps.act_dim, ps.mode = 5, 3, S, obs_dim, 2, 0
    host = (C.c_double * 8)()
    for name, _ in _lib.ReplayParticlesStruct._fields_[8:]:
        setattr(ps, name, C.addressof(host))
    return ps, host


def test_struct_image_and_refusals(lib):
    from cmbpo_amd import _lib
    assert C.sizeof(_lib.ReplayParticlesStruct) == 200
    assert lib.cmbpo_replay_particles_parts(37, 8) == 5 and lib.cmbpo_replay_particles_parts(5, 64) == 5
    assert lib.cmbpo_replay_particles_parts(130, 2) == 5 and lib.cmbpo_replay_particles_parts(1, 2) == 1
    assert lib.cmbpo_replay_particles_parts(0, 8) == 0 and lib.cmbpo_replay_particles_parts(4, 3) == 0
    err = lambda: lib.cmbpo_last_error().decode()
    for S in (3, 128, 1, 0, -8):
        ps, host = _image(_lib, S=S)
        assert lib.cmbpo_replay_particles(C.byref(ps), 0, None) == -1 and err().startswith("cmbpo_replay_particles: S %d" % S)
        assert lib.cmbpo_replay_particles_finish(C.byref(ps), None) == -1 and err().startswith("cmbpo_replay_particles_finish: S")
        assert lib.cmbpo_replay_run_particles(C.byref(ps), None, None, None, 2, 7, None, None) == -1
        assert err().startswith("cmbpo_replay_run_particles: S")
    ps, host = _image(_lib, obs_dim=_lib.REPLAY_PARTICLES_MAX_OBS + 1)
    assert lib.cmbpo_replay_particles(C.byref(ps), 0, None) == -1 and "cannot hold" in err()
    ps, host = _image(_lib)
    for h in (-1, 3):
        assert lib.cmbpo_replay_particles(C.byref(ps), h, None) == -1 and "outside [0, 3)" in err()
    ps.p_cost = None
    assert lib.cmbpo_replay_particles(C.byref(ps), 0, None) == -1 and "NULL buffer (predictions)" in err()
    ps, host = _image(_lib)
    ps.xi = None
    assert lib.cmbpo_replay_run_particles(C.byref(ps), None, None, C.addressof(host), 2, 7, C.addressof(host), None) == -1
    assert err().startswith("cmbpo_replay_run_particles:") and "xi" in err()
    assert lib.cmbpo_replay_particles(None, 0, None) == -1 and "NULL" in err()


def test_trainer_arguments_are_refused_in_words():
    from cmbpo_amd.cmbpo import _validate_particles_args
    assert _validate_particles_args(0, True, 1024, 0, None) == (0, 0)
    assert _validate_particles_args(5, True, 4096, 8, None) == (8, 1024)
    assert _validate_particles_args(5, True, 256, 8, None) == (8, 256)
    assert _validate_particles_args(5, True, 256, 4, 64) == (4, 64)
    with pytest.raises(ValueError, match="m_validate_horizon > 0"):
        _validate_particles_args(0, True, 1024, 4, None)
    with pytest.raises(ValueError, match="power of two"):
        _validate_particles_args(5, True, 1024, 3, None)
    with pytest.raises(ValueError, match="m_validate_particle_windows"):
        _validate_particles_args(5, True, 1024, 0, 64)
    # the particle pass runs no vote kernel: the pair is refused whatever the window counts are
    for windows, particle_windows in ((1024, None), (1024, 64), (64, 1024)):
        with pytest.raises(ValueError, match="m_validate_particles together with m_validate_votes=True"):
            _validate_particles_args(5, True, windows, 4, particle_windows, True)
    assert _validate_particles_args(5, True, 1024, 0, None, True) == (0, 0)


def test_the_trainer_refuses_particles_beside_vote_validation_before_anything_is_built():
    """The constructor's first act: no environment, policy or buffer is touched (None stands for all three)."""
    from cmbpo_amd.cmbpo import CMBPO
    with pytest.raises(ValueError, match="m_validate_particles together with m_validate_votes=True"):
        CMBPO(None, None, None, m_validate_horizon=5, m_static_votes=True, m_validate_votes=True, m_validate_particles=4)
    with pytest.raises(ValueError, match="m_validate_particles needs m_validate_horizon > 0"):
        CMBPO(None, None, None, m_validate_particles=4)
    import inspect
    assert "m_validate_votes=True" in inspect.getdoc(inspect.getmodule(CMBPO)).split("m_validate_particles=S")[1].split("\n\n")[0]
