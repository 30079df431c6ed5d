"""CPU: the specification of the critics' disagreement (tests/value_disagreement_ref.py) against a plain sequential float32
loop, and the choice of the critics the GPU tests use -- checked here with the oracle's forward, so that the comparisons on the
GPU are not vacuous."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import disagreement_ref as dref  # noqa: E402
import value_disagreement_ref as ref  # noqa: E402

KAPPA = (0.75, 1.5)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _loop(x, kappa, sign):
    """mean, var and the penalised value of x[E, n], one rounded float32 operation at a time."""
    E = x.shape[0]
    with np.errstate(all="ignore"):
        s = np.float32(0.0) + x[0]
        for e in range(1, E):
            s = (s + x[e]).astype(np.float32)
        mean = (s / np.float32(E)).astype(np.float32)
        var = dref.member_var_loop(x)
        if not kappa > 0.0:
            return mean, var, mean.copy()
        pen = (np.float32(kappa) * np.sqrt(var)).astype(np.float32)
        return mean, var, ((mean - pen) if sign < 0 else (mean + pen)).astype(np.float32)


@pytest.mark.parametrize("E", [1, 2, 3, 4])
def test_specification_is_the_sequential_loop(E):
    rng = np.random.default_rng(100 + E)
    n = 4097
    xv = (3.0 + 0.2 * rng.standard_normal((E, n))).astype(np.float32)
    xvc = (rng.standard_normal((E, n)) * np.exp(rng.standard_normal((1, n)))).astype(np.float32)
    xvc[:, ::7] += np.float32(1000.0)
    for kv, kc in ((0.0, 0.0), KAPPA, (0.0, 1.0), (2.0, 0.0)):
        v, vc, v_var, vc_var = ref.value_disagreement(xv, xvc, kv, kc)
        for got, var_got, x, k, sign in ((v, v_var, xv, kv, -1), (vc, vc_var, xvc, kc, +1)):
            mean, var, pen = _loop(x, k, sign)
            np.testing.assert_array_equal(_bits(var_got), _bits(var))
            np.testing.assert_array_equal(_bits(got), _bits(pen))
            if k == 0.0:
                np.testing.assert_array_equal(_bits(got), _bits(mean))
            np.testing.assert_array_equal(_bits(ref.member_mean(x)), _bits(mean))
    if E == 1:
        _, _, v_var, vc_var = ref.value_disagreement(xv, xvc, *KAPPA)
        assert not _bits(v_var).any() and not _bits(vc_var).any()          # +0, not -0
        v, vc, _, _ = ref.value_disagreement(xv, xvc, *KAPPA)
        np.testing.assert_array_equal(_bits(v), _bits(xv[0]))               # x - kappa * 0
        np.testing.assert_array_equal(_bits(vc), _bits(xvc[0]))


@pytest.mark.parametrize("E", [2, 3, 4])
def test_non_finite_members(E):
    """kappa = 0: the value is the mean whatever the variance is; kappa > 0: NumPy's propagation."""
    x = np.ones((E, 6), np.float32)
    x[0, 1], x[E - 1, 2], x[0, 3], x[0, 4], x[1, 4] = np.nan, np.inf, -np.inf, np.inf, -np.inf
    v0, vc0, v_var, vc_var = ref.value_disagreement(x, x, 0.0, 0.0)
    mean = ref.member_mean(x)
    for got in (v0, vc0):
        np.testing.assert_array_equal(np.isnan(got), np.isnan(mean))
        np.testing.assert_array_equal(_bits(got)[~np.isnan(mean)], _bits(mean)[~np.isnan(mean)])
    assert np.isnan(v_var[1:5]).all() and v_var[0] == 0.0 and v_var[5] == 0.0
    assert mean[2] == np.inf and mean[3] == -np.inf and np.isnan(mean[4])
    v, vc, _, _ = ref.value_disagreement(x, x, *KAPPA)
    assert np.isnan(v[1:5]).all() and np.isnan(vc[1:5]).all() and v[0] == 1.0 and vc[5] == 1.0


def _member_values(critic, obs):
    from oracle import refcpu
    E = critic[0][0].shape[0]
    return np.stack([refcpu.ens_predict_mean(obs, *ref.one_member(critic, e))[:, 0] for e in range(E)]).astype(np.float32)


@pytest.mark.parametrize("obs_dim", [3, 29, 47, 64])
@pytest.mark.parametrize("E", [2, 3, 4])
def test_the_gpu_tests_critics_are_not_vacuous(E, obs_dim):
    """The critics of tests/test_value_disagreement_gpu.py through the oracle's float32 forward: the spread is between a
    thousandth of and the whole mean on >= 90 % of the rows, and KAPPA moves >= 90 % of the values in their bits."""
    obs = ref.observations(7, 1001, obs_dim)
    for critic, kappa, sign in zip(ref.critic_weights(11, E, obs_dim), KAPPA, (-1, +1)):
        ref.check_non_vacuous(_member_values(critic, obs), kappa, sign)


def test_a_one_pass_variance_fails_where_the_specification_holds():
    """Output scaler out_mu = 1000, member spread ~ 0.1: E[x^2] - E[x]^2 in float32 has an error of the size of the variance
    itself (x^2 ~ 1e6 carries 0.06 of rounding), the two-pass specification does not."""
    obs = ref.observations(7, 1001, 29)
    for critic, kappa, sign in zip(ref.critic_weights(11, 3, 29, out_mu=1000.0), KAPPA, (-1, +1)):
        x = _member_values(critic, obs)
        ref.check_non_vacuous(x, kappa, sign, relative=False)
        assert (np.abs(x) > 990).all()
        spec = dref.member_var(x)
        exact = np.var(x.astype(np.float64), axis=0)
        np.testing.assert_allclose(spec, exact, rtol=2e-3)
        with np.errstate(all="ignore"):
            m2 = ((x * x).astype(np.float32).sum(axis=0, dtype=np.float32) / np.float32(3)).astype(np.float32)
            m = ref.member_mean(x)
            one_pass = (m2 - (m * m).astype(np.float32)).astype(np.float32)
        assert np.mean(_bits(one_pass) != _bits(spec)) > 0.9
        assert np.median(np.abs(one_pass - exact) / exact) > 0.1
