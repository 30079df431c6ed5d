"""CPU: the argument checks of cmbpo_fakeenv_post_noise precede any HIP call -- with a non-NULL draw pointer (the NULL one
forwards to cmbpo_fakeenv_post) a bad task, bad dims and NULL buffers return -1 with a message naming the entry point."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cmbpo_amd import _lib
    return _lib.lib()


def _post_noise(lib, task, ensemble, obs_dim, act_dim, xi, buffers=None, n_rows=0, ld_rows=0):
    b = buffers or [None] * 10       # mean, var, obs, elite, next_obs, rew, term, cost, dkl_path, ep_var_mean
    return lib.cmbpo_fakeenv_post_noise(task, ensemble, obs_dim, act_dim, b[0], b[1], ld_rows, b[2], None, b[3], None, None,
                                        n_rows, b[4], b[5], b[6], b[7], b[8], b[9], None, xi, None)


def test_post_noise_rejects_bad_arguments_without_a_gpu(lib):
    from cmbpo_amd import _lib
    assert lib.cmbpo_version() >= 2
    host = (C.c_float * 64)()                 # never dereferenced: every call below fails its checks first
    xi = C.cast(host, C.c_void_p)
    who = b"cmbpo_fakeenv_post_noise"
    for task in (9, 3, -1, _lib.TASK_ANTSAFE | 0x200, _lib.TASK_USER_BASE + _lib.TASK_USER_SLOTS):
        assert _post_noise(lib, task, 7, 29, 8, xi) == -1
        msg = lib.cmbpo_last_error()
        assert who in msg and (b"bad task" in msg or b"not registered" in msg), msg
    for E in (1, 9):
        assert _post_noise(lib, _lib.TASK_HCS, E, 18, 6, xi) == -1
        assert who in lib.cmbpo_last_error() and b"ensemble" in lib.cmbpo_last_error()
    for obs_dim, act_dim in ((0, 6), (513, 6), (18, -1)):
        assert _post_noise(lib, _lib.TASK_HCS, 7, obs_dim, act_dim, xi) == -1
        assert who in lib.cmbpo_last_error() and b"bad dims" in lib.cmbpo_last_error()
    assert _post_noise(lib, _lib.TASK_ANTSAFE, 7, 4, 2, xi) == -1
    assert b"obs_dim >= 5" in lib.cmbpo_last_error()
    # NULL buffers: all of them, then each of the ten required ones in turn
    assert _post_noise(lib, _lib.TASK_DEFAULT, 7, 11, 3, xi) == -1
    assert who in lib.cmbpo_last_error() and b"NULL buffer" in lib.cmbpo_last_error()
    for k in range(10):
        bufs = [xi] * 10
        bufs[k] = None
        assert _post_noise(lib, _lib.TASK_DEFAULT | _lib.TASK_LEARNED_COST, 7, 11, 3, xi, bufs) == -1
        assert b"NULL buffer" in lib.cmbpo_last_error()
    assert _post_noise(lib, _lib.TASK_DEFAULT, 7, 11, 3, xi, [xi] * 10, n_rows=5, ld_rows=4) == -1
    assert b"ld_rows" in lib.cmbpo_last_error()
    # no rows: nothing to launch
    assert _post_noise(lib, _lib.TASK_DEFAULT, 7, 11, 3, xi, [xi] * 10, n_rows=0, ld_rows=0) == 0
    # a NULL draw pointer is cmbpo_fakeenv_post: its checks, its name
    assert _post_noise(lib, 9, 7, 29, 8, None) == -1
    assert b"cmbpo_fakeenv_post: bad task" in lib.cmbpo_last_error()


def test_rollout_struct_carries_the_draws():
    from cmbpo_amd import _lib
    names = [f[0] for f in _lib.RolloutStruct._fields_]
    assert names[-2:] == ["xi", "xi_stride"] and names[-3] == "cret_buf"       # trailing fields: every older offset stays
    rs = _lib.RolloutStruct()
    assert rs.xi is None and rs.xi_stride == 0                                   # off unless set
    assert _lib.RolloutStruct.xi.offset % 8 == 0 and C.sizeof(_lib.RolloutStruct) == _lib.RolloutStruct.xi.offset + 16
