"""CPU: the NumPy specification of the ensemble disagreement on reward / cost (tests/disagreement_ref.py) against a plain
sequential float32 loop, bit for bit -- np.var(axis=0) is the arithmetic the post kernel spells out."""
import numpy as np
import pytest

import disagreement_ref as ref


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    """Bit for bit where finite or infinite, NaN where NaN (a NaN's payload is no part of the specification)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    np.testing.assert_array_equal(_bits(a)[ok], _bits(b)[ok])


@pytest.mark.parametrize("E", [3, 5, 7, 8])
def test_member_var_is_the_sequential_float32_loop(E):
    rng = np.random.default_rng(E)
    n = 4099
    x = (rng.standard_normal((E, n)) * np.exp(rng.uniform(-8, 8, n))).astype(np.float32)
    v = ref.member_var(x)
    assert v.dtype == np.float32 and v.shape == (n,)
    _same(v, ref.member_var_loop(x))
    # a strided column of [E, n, out], as the kernel's caller holds it
    mean = rng.standard_normal((E, n, 31)).astype(np.float32)
    for col in (29, 30):
        view = mean[:, :, col]
        assert not view.flags.c_contiguous
        _same(ref.member_var(view), ref.member_var_loop(np.ascontiguousarray(view)))
        _same(ref.member_var(view), ref.member_var_loop(view))
    # the layouts NumPy would reduce in another order (see member_var): an index array's result, a single row
    for rows in (np.arange(0, n, 3), np.array([5])):
        picked = mean[:, rows, 29]
        _same(ref.member_var(picked), ref.member_var_loop(np.ascontiguousarray(picked)))
    # members that agree exactly (their mean is exact): no variance
    assert (ref.member_var(np.full((E, 5), 0.5, np.float32)) == 0.0).all()


@pytest.mark.parametrize("E", [3, 5, 7, 8])
def test_non_finite_members_propagate_like_numpy(E):
    rng = np.random.default_rng(100 + E)
    x = rng.standard_normal((E, 64)).astype(np.float32)
    x[1, 3] = np.nan
    x[E - 1, 4] = np.inf
    x[0, 5] = -np.inf
    x[:, 6] = np.inf
    x[0, 7], x[2, 7] = np.inf, -np.inf
    x[1, 8] = 3e38          # the sum overflows
    x[2, 8] = 3e38
    v, w = ref.member_var(x), ref.member_var_loop(x)
    _same(v, w)
    assert np.isnan(v[[3, 4, 5, 6, 7]]).all()
    assert np.isfinite(np.delete(v, [3, 4, 5, 6, 7, 8])).all()


@pytest.mark.parametrize("E", [3, 5, 7, 8])
@pytest.mark.parametrize("learned", [False, True])
def test_disagreement_outputs(E, learned):
    rng = np.random.default_rng(200 + E)
    B, D = 37, 11
    out = D + 1 + int(learned)
    mean = rng.standard_normal((E, B, out)).astype(np.float32)
    inds = rng.integers(0, E, B).astype(np.int32)
    mean[(inds[2] + 1) % E, 2, D] = np.nan          # another member's reward
    mean[inds[3], 3, D] = np.inf                    # the elite's
    if learned:
        mean[(inds[4] + 1) % E, 4, D + 1] = np.nan
        mean[inds[5], 5, D + 1] = -np.inf
    rows = np.array([0, 2, 3, 4, 5, 9, 36])
    elite_r = mean[inds[rows], rows, D]
    # kappa == 0: the elite's value bit for bit, whatever the other members hold
    rv, cv, rew, cost = ref.disagreement(mean, inds, D, learned, 0.0, 0.0, rows)
    np.testing.assert_array_equal(_bits(rew), _bits(elite_r))
    assert np.isfinite(rew[1]) and np.isnan(rv[1]) and rew[2] == np.inf
    _same(rv, ref.member_var_loop(np.ascontiguousarray(mean[:, rows, D])))
    if learned:
        elite_c = mean[inds[rows], rows, D + 1]
        np.testing.assert_array_equal(_bits(cost), _bits(elite_c))
        assert np.isfinite(cost[3]) and np.isnan(cv[3])
        _same(cv, ref.member_var_loop(np.ascontiguousarray(mean[:, rows, D + 1])))
    else:
        assert cost is None and cv.dtype == np.float32 and not cv.any() and not np.signbit(cv).any()
        with pytest.raises(ValueError):
            ref.disagreement(mean, inds, D, False, 0.0, 0.5)
    # kappa > 0: r - k sigma_r, c + k sigma_c, each operation rounded to float32; NaN / inf go where NumPy takes them
    kr, kc = 0.75, 1.5 if learned else 0.0
    rv2, cv2, rew2, cost2 = ref.disagreement(mean, inds, D, learned, kr, kc, rows)
    _same(rv2, rv)
    _same(cv2, cv)
    with np.errstate(all="ignore"):
        want = np.array([np.float32(e) - np.float32(np.float32(kr) * np.float32(np.sqrt(np.float32(v))))
                         for e, v in zip(elite_r, rv)], np.float32)
    _same(rew2, want)
    assert np.isnan(rew2[1]) and (rew2[[0, 5, 6]] <= elite_r[[0, 5, 6]]).all() and (rew2[[0, 5, 6]] < elite_r[[0, 5, 6]]).any()
    if learned:
        with np.errstate(all="ignore"):
            wantc = np.array([np.float32(e) + np.float32(np.float32(kc) * np.float32(np.sqrt(np.float32(v))))
                              for e, v in zip(elite_c, cv)], np.float32)
        _same(cost2, wantc)
        assert np.isnan(cost2[3]) and (cost2[[0, 5, 6]] >= elite_c[[0, 5, 6]]).all()
