"""CPU: sampled terminations without a GPU -- the NumPy restatement of the rule on hand-made rows (votes, the
threshold itself, NaN and the infinities on either side), `utils.term_thresholds`, every new refusal of FakeEnv, ModelSampler and
CMBPO by its words, the C-ABI refusals by the entry's name, and the round trip of the trainer's flag through save / load."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import term_draws_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = b"cmbpo_fakeenv_post_term_draws"
INF, NAN = np.float32(np.inf), np.float32(np.nan)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cmbpo_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------
# 1. the reference on hand-made rows
# ------------------------------------------------------------------------------------------------------------------
def _rows(xs, out=4):
    """mean[E, n, out] whose last column is xs[E, n]; the other columns are junk that must not matter."""
    xs = np.asarray(xs, np.float32)
    mean = np.full(xs.shape + (out,), 123.0, np.float32)
    mean[:, :, -1] = xs
    return mean


def test_reference_votes_on_hand_made_rows():
    # E = 3, threshold 0.5 for every row.  row 0: the elite (member 1) hits alone; row 1: everybody but the elite (member 0);
    # row 2: nobody; row 3: everybody
    xs = np.array([[0.1, 0.4, 0.2, 0.8],
                   [0.9, 0.8, 0.3, 0.7],
                   [0.2, 0.7, 0.4, 0.6]], np.float32)
    elite = np.array([1, 0, 2, 1])
    thr = np.full(4, 0.5, np.float32)
    want = {"elite": [1, 0, 0, 1], "any": [1, 1, 0, 1], "majority": [0, 1, 0, 1]}
    for members, term in want.items():
        t, pred, votes = ref.term_draws(_rows(xs), elite, thr, members)
        assert t.tolist() == term and t.dtype == np.uint8, members
        assert votes.tolist() == [1, 2, 0, 3] and votes.dtype == np.uint8
        np.testing.assert_array_equal(pred, np.array([0.9, 0.4, 0.4, 0.7], np.float32))
    # the rows have thresholds of their own: the same values under per-row thresholds
    thr = np.array([0.95, 0.1, 0.35, 0.75], np.float32)
    t, _, votes = ref.term_draws(_rows(xs), elite, thr, "elite")
    assert votes.tolist() == [0, 3, 1, 1] and t.tolist() == [0, 1, 1, 0]
    # the rule's own verdict is or-ed in and never taken back
    t, _, _ = ref.term_draws(_rows(xs), elite, thr, "elite", rule_done=[1, 0, 0, 1])
    assert t.tolist() == [1, 1, 1, 1]
    t, _, _ = ref.term_draws(_rows(xs), elite, np.full(4, INF), "any", rule_done=np.array([0, 1, 0, 0], np.uint8))
    assert t.tolist() == [0, 1, 0, 0]


def test_reference_special_values():
    one = lambda x, thr: int(ref.term_draws(_rows([[x]]), [0], np.array([thr], np.float32), "elite")[2][0])
    assert one(0.25, 0.25) == 0                                         # x == thr does not hit
    assert one(np.nextafter(np.float32(0.25), INF), 0.25) == 1 and one(np.nextafter(np.float32(0.25), -INF), 0.25) == 0
    assert one(NAN, 0.0) == 0 and one(NAN, -INF) == 0 and one(NAN, INF) == 0        # a NaN x never hits
    assert one(0.0, NAN) == 0 and one(INF, NAN) == 0 and one(-INF, NAN) == 0        # a NaN thr never hits
    assert one(NAN, NAN) == 0
    assert one(-3e38, -INF) == 1 and one(0.0, -INF) == 1 and one(INF, -INF) == 1    # thr = -inf hits every non-NaN x ...
    assert one(-INF, -INF) == 0                                                     # ... -inf excepted
    assert one(3e38, INF) == 0 and one(INF, INF) == 0 and one(-INF, INF) == 0       # thr = +inf never hits
    # a NaN member neither votes nor spoils the others' votes; term_pred carries the elite's value as it is
    xs = np.array([[NAN], [1.0], [2.0]], np.float32)
    t, pred, votes = ref.term_draws(_rows(xs), [0], np.array([0.0], np.float32), "majority")
    assert votes.tolist() == [2] and t.tolist() == [1] and np.isnan(pred[0])
    t, _, _ = ref.term_draws(_rows(xs), [0], np.array([0.0], np.float32), "elite")
    assert t.tolist() == [0]


# ------------------------------------------------------------------------------------------------------------------
# 2. draws -> thresholds
# ------------------------------------------------------------------------------------------------------------------
def test_term_thresholds():
    torch = pytest.importorskip("torch")
    from cmbpo_amd.utils import term_thresholds
    u = np.array([0.0, 1e-30, 1e-6, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0 - 2.0 ** -24, 1.0], np.float32)
    z = term_thresholds(u, "logistic")
    assert isinstance(z, np.ndarray) and z.dtype == np.float32 and z.shape == u.shape
    assert z[0] == -INF and z[-1] == INF and z[5] == 0.0
    assert (np.diff(z) > 0).all()                                        # monotone in u
    u64 = u[1:-1].astype(np.float64)
    np.testing.assert_array_equal(z[1:-1], (np.log(u64) - np.log1p(-u64)).astype(np.float32))
    np.testing.assert_allclose(z[3], np.log(0.1 / 0.9), rtol=1e-6)
    g = term_thresholds(u, "gaussian")
    assert g.dtype == np.float32 and np.array_equal(g, u)                # the identity
    assert term_thresholds(np.array([[0.5, 1.0]]), "logistic").shape == (1, 2)      # float64 in, any shape
    # a torch tensor in, a torch tensor out: the same numbers
    zt = term_thresholds(torch.from_numpy(u), "logistic")
    assert isinstance(zt, torch.Tensor) and zt.dtype == torch.float32
    assert zt[0] == -INF and zt[-1] == INF and zt[5] == 0.0
    np.testing.assert_allclose(zt.numpy()[1:-1], z[1:-1], rtol=1e-6)
    assert torch.equal(term_thresholds(torch.from_numpy(u), "gaussian"), torch.from_numpy(u))
    for bad in ([-0.1], [1.5], [0.5, np.nan], [np.inf]):
        for loss in ("logistic", "gaussian"):
            with pytest.raises(ValueError, match=r"draws must lie in \[0, 1\]"):
                term_thresholds(np.array(bad, np.float32), loss)
            with pytest.raises(ValueError, match=r"draws must lie in \[0, 1\]"):
                term_thresholds(torch.tensor(bad), loss)
    with pytest.raises(ValueError, match="loss 'gaussian' or 'logistic'"):
        term_thresholds(u, "probit")


# ------------------------------------------------------------------------------------------------------------------
# 3. the host's refusals, by their words
# ------------------------------------------------------------------------------------------------------------------
def _fake_env(predicts_term, **kw):
    """A FakeEnv up to its checks: a model stub, no device."""
    from toyworld import ToyEnv
    from cmbpo_amd.fake_env import FakeEnv
    env = ToyEnv()
    obs, act = int(np.prod(env.observation_space.shape)), int(np.prod(env.action_space.shape))

    class Model:
        is_ensemble = is_probabilistic = True
        in_dim, out_dim, device = obs + act, obs + 1 + int(predicts_term), "cpu"
    return FakeEnv(env, "default", Model(), True, True, False, predicts_term=predicts_term, **kw), obs, act


def test_fake_env_refuses_draws_without_the_column():
    fe, obs, act = _fake_env(False)
    o, a = np.zeros((3, obs), np.float32), np.zeros((3, act), np.float32)
    with pytest.raises(ValueError, match="term_draws needs predicts_term=True"):
        fe.step(o, a, term_draws=np.full(3, 0.5, np.float32))
    with pytest.raises(ValueError, match="term_thr needs predicts_term=True"):
        fe.step_device(o, a, None, {}, term_thr=np.zeros(3, np.float32))


def test_model_sampler_refusals():
    from cmbpo_amd.model_sampler import ModelSampler

    class Comm:
        rank, world = 0, 2

    with pytest.raises(NotImplementedError, match="term_sampling=True on a sharded sampler"):
        ModelSampler(8, comm=Comm(), term_sampling=True)
    ModelSampler(8, comm=Comm())                                         # off: sharded samplers are what they were
    plain, _, _ = _fake_env(False)
    s = ModelSampler(8, term_sampling=True)
    assert s.term_sampling and s._term_gen is None
    with pytest.raises(ValueError, match="term_sampling=True needs an environment with predicts_term=True"):
        s.initialize(plain, None, None)
    off = ModelSampler(8)
    assert not off.term_sampling and off._term_gen is None               # no generator is made
    off.env = plain
    with pytest.raises(ValueError, match="term_draws needs an environment with predicts_term=True"):
        off.sample(term_draws=np.full(4, 0.5, np.float32))


def test_cmbpo_refusals():
    """The checks come first in the constructor: nothing is built, nothing needs a device (or an environment)."""
    from cmbpo_amd.cmbpo import CMBPO, _term_sampling_args
    with pytest.raises(ValueError, match="m_term_sampling=True needs m_learn_term=True"):
        CMBPO(None, None, None, m_term_sampling=True)
    with pytest.raises(ValueError, match="m_term_sampling=True needs m_learn_term=True"):
        CMBPO(None, None, None, m_term_sampling=True, m_learn_term=True, use_model=False)
    assert _term_sampling_args(True, True) is True and _term_sampling_args(True, False) is False
    assert _term_sampling_args(False, False) is False


# ------------------------------------------------------------------------------------------------------------------
# 4. the C-ABI
# ------------------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "cmbpo_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _head(threshold=0.5, members=0):
    from cmbpo_amd import _lib
    th = _lib.TermHeadStruct()
    th.threshold, th.members, th.term_pred, th.term_votes = threshold, members, None, None
    return th


def _post(lib, task, th, thr, n_rows=0, buffers=True):
    """cmbpo_fakeenv_post_term_draws on host memory that is never dereferenced: every call fails a check or has no rows."""
    host = (C.c_float * 64)()
    p = C.cast(host, C.c_void_p) if buffers else None
    return lib.cmbpo_fakeenv_post_term_draws(task, 7, 18, 6, p, p, n_rows, p, p, p, None, None, n_rows, p, p, p, p, p, p, None, None,
                                             0.0, 0.0, None, None, None if th is None else C.byref(th), None,
                                             C.cast(host, C.c_void_p) if thr else None, None)


def test_signatures_and_frozen_structs(lib):
    from cmbpo_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("cmbpo_fakeenv_post_term_draws", "cmbpo_rollout_term_draws_attach"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    cost, draws = _lib.SIGNATURES["cmbpo_fakeenv_post_cost"], _lib.SIGNATURES["cmbpo_fakeenv_post_term_draws"]
    assert draws[0] is C.c_int and draws[1] == cost[1][:-1] + [C.c_void_p, C.c_void_p]     # ... plus the thresholds, then the stream
    text = _header()
    args = [a.strip() for a in re.search(r"int cmbpo_fakeenv_post_term_draws\((.*?)\);", text, flags=re.S).group(1).split(",")]
    assert len(args) == len(draws[1]) and args[-3:] == ["const cmbpo_cost_head_t *ch", "const float *d_term_thr", "void *stream"]
    m = re.search(r"int cmbpo_rollout_term_draws_attach\((.*?)\);", text, flags=re.S)
    assert [a.strip() for a in m.group(1).split(",")] == ["const cmbpo_rollout_t *r", "const float *d_thr", "long step_stride"]
    assert _lib.SIGNATURES["cmbpo_rollout_term_draws_attach"] == (C.c_int, [C.POINTER(_lib.RolloutStruct), C.c_void_p, C.c_long])
    # cmbpo_rollout_t and cmbpo_term_head_t keep their sizes
    assert C.sizeof(_lib.RolloutStruct) == 440 and C.sizeof(_lib.TermHeadStruct) == 24


def test_post_refuses_draws_without_a_head_before_any_hip_call(lib):
    from cmbpo_amd import _lib
    assert _post(lib, _lib.TASK_HCS, None, True) == -1
    msg = lib.cmbpo_last_error()
    assert msg.startswith(WHO + b":") and b"draws" in msg and b"termination head" in msg, msg
    # the checks it shares with the other entries keep their words, under this entry's name
    assert _post(lib, 9, _head(), True) == -1
    assert lib.cmbpo_last_error().startswith(WHO + b": bad task 9")
    assert _post(lib, _lib.TASK_HCS, _head(float("nan")), True) == -1
    assert lib.cmbpo_last_error().startswith(WHO + b":") and b"threshold" in lib.cmbpo_last_error()
    assert _post(lib, _lib.TASK_HCS, _head(), True, buffers=False) == -1
    assert lib.cmbpo_last_error().startswith(WHO + b": NULL buffer")
    # d_term_thr == NULL is cmbpo_fakeenv_post_cost's call: the names the rule gave before
    assert _post(lib, 9, _head(), False) == -1
    assert lib.cmbpo_last_error().startswith(b"cmbpo_fakeenv_post_term: bad task 9")
    assert _post(lib, 9, None, False) == -1
    assert lib.cmbpo_last_error().startswith(b"cmbpo_fakeenv_post: bad task 9")
    # good arguments on no rows: nothing is launched
    for members in (0, 1, 2):
        assert _post(lib, _lib.TASK_HCS, _head(0.5, members), True) == 0, lib.cmbpo_last_error()
    assert _post(lib, _lib.TASK_HCS, _head(), False) == 0


def test_rollout_attach_refusals_and_the_step_without_a_head(lib):
    from cmbpo_amd import _lib
    who = b"cmbpo_rollout_term_draws_attach"
    host = (C.c_float * 64)()
    p = C.cast(host, C.c_void_p)
    assert lib.cmbpo_rollout_term_draws_attach(None, p, 4) == -1                          # NULL rollout struct
    assert lib.cmbpo_last_error().startswith(who + b": NULL rollout struct")
    rs = _lib.RolloutStruct()
    assert lib.cmbpo_rollout_term_draws_attach(C.byref(rs), p, 4) == -1                   # no iscal: no key
    assert lib.cmbpo_last_error().startswith(who)
    key = (C.c_int32 * 32)()
    rs.iscal = C.cast(key, C.c_void_p)
    assert lib.cmbpo_rollout_term_draws_attach(C.byref(rs), p, -1) == -1
    assert lib.cmbpo_last_error().startswith(who) and b"step_stride" in lib.cmbpo_last_error()
    assert lib.cmbpo_rollout_term_draws_attach(C.byref(rs), None, 0) == 0                 # nothing attached: no error
    assert lib.cmbpo_rollout_term_draws_attach(C.byref(rs), p, 4) == 0
    try:
        # draws attached without a termination head: refused in words at the step, before anything is dereferenced or launched
        rs.B = 4
        rc = lib.cmbpo_rollout_step(C.byref(rs), 2, p, p, p, p, _lib.TASK_DEFAULT, 7, p, p, p, p, None)
        msg = lib.cmbpo_last_error()
        assert rc == -1 and msg.startswith(b"cmbpo_rollout_step:") and b"termination draws" in msg and b"termination head" in msg, msg
    finally:
        assert lib.cmbpo_rollout_term_draws_attach(C.byref(rs), None, 0) == 0             # detached


# ------------------------------------------------------------------------------------------------------------------
# 5. save / load
# ------------------------------------------------------------------------------------------------------------------
def test_save_load_round_trip_of_the_flag(tmp_path):
    from cmbpo_amd.cmbpo import CMBPO

    class Model:
        def save(self, d, e):
            pass

        def load(self, d, e):
            pass

        def set_logistic_columns(self, cols):
            pass

        def set_column_weights(self, *a):
            pass

    class Env:
        term_threshold, term_members, term_loss = 0.3, "any", "logistic"

        def set_term_head(self, threshold, members, loss=None):
            pass

    class Sampler:
        term_sampling, _draws = False, "a chunk"

    def trainer(sampling):
        a = CMBPO.__new__(CMBPO)
        a._use_model, a._m_learn_term, a._m_learn_cost, a._epoch = True, True, False, 4
        a._model, a.fake_env, a._m_term_loss, a._m_term_sampling = Model(), Env(), "logistic", sampling
        a._column_weights = {"m_term_pos_weight": 1.0, "m_term_loss_weight": 1.0, "m_cost_loss_weight": 1.0, "m_pos_weight_max": 20.0}
        a.model_sampler = Sampler()
        a.model_sampler.term_sampling = sampling
        return a

    trainer(True).save(str(tmp_path))
    assert json.load(open(tmp_path / "term_sampling_4.json")) == {"m_term_sampling": True}
    assert json.load(open(tmp_path / "term_head_4.json")) == {"threshold": 0.3, "members": "any"}      # its keys stay
    b = trainer(False)
    b.load(str(tmp_path), 4)
    assert b._m_term_sampling is True and b.model_sampler.term_sampling is True
    # a checkpoint without the key, and one from before the file: off
    with open(tmp_path / "term_sampling_4.json", "w") as fh:
        json.dump({}, fh)
    c = trainer(True)
    c.load(str(tmp_path), 4)
    assert c._m_term_sampling is False and c.model_sampler.term_sampling is False
    os.remove(tmp_path / "term_sampling_4.json")
    c = trainer(True)
    c.load(str(tmp_path), 4)
    assert c._m_term_sampling is False and c.model_sampler.term_sampling is False
    trainer(False).save(str(tmp_path))
    assert json.load(open(tmp_path / "term_sampling_4.json")) == {"m_term_sampling": False}
