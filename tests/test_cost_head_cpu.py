"""CPU: the logistic learned-cost head without a GPU -- the NumPy specification against closed forms, the C-ABI
(struct image, exports, every refusal by name before any HIP call, naming rules 1 and 2 with their new first lines, on calls of
no rows), and the host side: FakeEnv's and CMBPO's refusals in words, the cost_loss_<epoch>.json round trip, the 'balanced'
class weight of the cost column and the shift that undoes it."""
import ctypes as C
import itertools
import json
import os
import re

import numpy as np
import pytest

import cost_head_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = b"cmbpo_fakeenv_post_cost"
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cmbpo_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------------------------------------
# the specification against closed forms
# ------------------------------------------------------------------------------------------------------------------
def test_sigma32_at_the_listed_points():
    z = np.array([0.0, 1e-8, -1e-8, 20.0, -20.0, 80.0, -80.0, 1e4, -1e4, np.inf, -np.inf, np.nan], f32)
    p = ref.sigma32(z)
    assert p.dtype == f32
    assert p[0] == f32(0.5)
    # 1 +- 1e-8 rounds to 1 in float32 on both branches: 1 / (1 + 1) and fl32(exp(-1e-8)) / (1 + fl32(exp(-1e-8))) = 1 / 2
    assert p[1] == f32(0.5) and p[2] == f32(0.5)
    # sigma(20) = 1 - 2.06e-9, below half an ulp of 1 (2^-25 = 2.98e-8): exactly 1; sigma(-20) = e^-20 (1 - e^-20)
    assert p[3] == f32(1.0) and abs(float(p[4]) / np.exp(-20.0) - 1.0) < 4 * 2.0 ** -23
    assert p[5] == f32(1.0) and abs(float(p[6]) / np.exp(-80.0) - 1.0) < 4 * 2.0 ** -23 and p[6] > 0
    assert p[7] == f32(1.0) and p[8] == f32(0.0)         # expf(-1e4) underflows to +0: 1 / (1 + 0) and 0 / (1 + 0)
    assert p[9] == f32(1.0) and p[10] == f32(0.0) and np.isnan(p[11])
    fin = np.isfinite(z)
    assert ((p[fin] >= 0) & (p[fin] <= 1)).all()
    # ... and against the float64 sigma inside the bound the GPU test asserts of the device
    s64 = ref.sigma64(z)
    assert s64[9] == 1.0 and s64[10] == 0.0 and np.isnan(s64[11]) and s64[0] == 0.5
    assert (np.abs(p[fin].astype(np.float64) - s64[fin]) <= ref.sigma_bound(z[fin])).all()
    grid = np.linspace(-80, 80, 4001).astype(f32)
    assert (np.abs(ref.sigma32(grid).astype(np.float64) - ref.sigma64(grid)) <= ref.sigma_bound(grid)).all()
    # symmetry of the float64 form (two roundings of a number below 1 and their sum: two ulps of 1), and a closed form
    np.testing.assert_allclose(ref.sigma64(grid) + ref.sigma64(-grid), 1.0, rtol=0, atol=2 * 2.0 ** -52)
    np.testing.assert_allclose(ref.sigma64([np.log(3.0)]), [0.75], rtol=1e-15)


def test_shift_clip_and_the_pessimistic_cost():
    z = np.array([0.5, -0.0, np.nan, 3.0], f32)
    assert ref.shift(z, 0.0) is z                                           # no subtraction: the same bits (-0 stays -0)
    np.testing.assert_array_equal(ref.shift(z, 0.25)[[0, 3]], np.array([0.25, 2.75], f32))
    c = ref.clip1(np.array([0.5, 1.0, 1.0000001, 7.0, np.nan, -0.25, np.inf], f32))
    np.testing.assert_array_equal(c[[0, 1, 2, 3, 5, 6]], np.array([0.5, 1.0, 1.0, 1.0, -0.25, 1.0], f32))
    assert np.isnan(c[4])                                                   # a NaN passes
    # kappa = 0 (and no disagreement): the elite's probability whatever the other members hold
    p = np.array([[0.25, 0.5], [np.nan, 0.9], [np.inf, 0.1]], f32)
    for kappa in (None, 0.0):
        cost, var = ref.downstream(p, [0, 2], kappa)
        np.testing.assert_array_equal(cost, np.array([0.25, 0.1], f32))
        assert (var is None) == (kappa is None)
    assert np.isnan(ref.downstream(p, [0, 2], 0.0)[1][0])
    # np.var of {0, 1}: 0.25, sqrt 0.5 -- p_elite + kappa / 2, clipped at 1
    p = np.array([[0.0, 1.0, 0.75], [1.0, 0.0, 0.75]], f32)
    cost, var = ref.downstream(p, [0, 0, 1], 0.5)
    np.testing.assert_array_equal(var, np.array([0.25, 0.25, 0.0], f32))
    np.testing.assert_array_equal(cost, np.array([0.25, 1.0, 0.75], f32))   # 1 + 0.25 is clipped; no spread adds nothing
    cost, _ = ref.downstream(p, [1, 1, 1], 4.0)
    np.testing.assert_array_equal(cost, np.array([1.0, 1.0, 0.75], f32))
    # the whole block: the logit goes out raw, the shift moves the probability
    mean = np.zeros((2, 3, 5), f32)
    mean[:, :, 3] = np.array([[0.0, np.log(3.0), -2.0], [1.0, 0.0, 9.0]], f32)
    cost, var, zl = ref.cost_head(mean, [0, 0, 1], 2, logit_shift=float(np.log(3.0)))
    assert var is None
    np.testing.assert_array_equal(zl, mean[[0, 0, 1], [0, 1, 2], 3])
    np.testing.assert_allclose(cost, [0.25, 0.5, ref.sigma64(9.0 - np.log(3.0))], rtol=1e-6)
    cost, _, _ = ref.cost_head(mean, [0, 0, 1], 2, rows=[2, 0])
    np.testing.assert_allclose(cost, [ref.sigma64(9.0), 0.5], rtol=1e-6)


# ------------------------------------------------------------------------------------------------------------------
# the C-ABI
# ------------------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "cmbpo_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _cost(kind=1, shift=0.0):
    from cmbpo_amd import _lib
    ch = _lib.CostHeadStruct()
    ch.kind, ch.logit_shift, ch.cost_logit = kind, shift, None
    return ch


def _term(threshold=0.5, members=2):
    from cmbpo_amd import _lib
    th = _lib.TermHeadStruct()
    th.threshold, th.members, th.term_pred, th.term_votes = threshold, members, None, None
    return th


def _post_cost(lib, task, ch, xi=False, dis=False, th=False, n_rows=0, buffers=True, obs_dim=18, kc=0.25):
    """cmbpo_fakeenv_post_cost on host memory that is never dereferenced: every call fails a check or has no rows."""
    host = (C.c_float * 64)()
    p = C.cast(host, C.c_void_p) if buffers else None
    head = _term()
    return lib.cmbpo_fakeenv_post_cost(task, 7, obs_dim, 6, p, p, n_rows, p, p, p, None, None, n_rows, p, p, p, p, p, p, None,
                                       p if xi else None, *((0.5, kc, p, p) if dis else (0.0, 0.0, None, None)),
                                       C.byref(head) if th else None, None if ch is None else C.byref(ch), None)


def test_struct_image_and_signatures(lib):
    from cmbpo_amd import _lib
    S = _lib.CostHeadStruct
    assert C.sizeof(S) == 16
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("kind", 0), ("logit_shift", 4), ("cost_logit", 8)]
    assert [t for _, t in S._fields_] == [C.c_int32, C.c_float, C.c_void_p]
    text = _header()
    m = re.search(r"typedef struct cmbpo_cost_head \{(.*?)\} cmbpo_cost_head_t;", text, flags=re.S)
    assert m and [d.strip() for d in m.group(1).split(";") if d.strip()] == ["int32_t kind", "float logit_shift", "float *cost_logit"]
    assert (_lib.COST_MAGNITUDE, _lib.COST_LOGISTIC) == (0, 1) == (ref.KIND_MAGNITUDE, ref.KIND_LOGISTIC)
    assert re.search(r"#define CMBPO_COST_MAGNITUDE 0\b", text) and re.search(r"#define CMBPO_COST_LOGISTIC 1\b", text)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("cmbpo_fakeenv_post_cost", "cmbpo_rollout_cost_head_attach", "cmbpo_rollout_cost_head_detach", "cmbpo_replay_run_cost"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    # cmbpo_fakeenv_post_term's arguments, then the cost head, then the stream; likewise the replay
    term, cost = _lib.SIGNATURES["cmbpo_fakeenv_post_term"], _lib.SIGNATURES["cmbpo_fakeenv_post_cost"]
    assert cost[0] is C.c_int and cost[1] == term[1][:-1] + [C.POINTER(S), C.c_void_p]
    args = [a.strip() for a in re.search(r"int cmbpo_fakeenv_post_cost\((.*?)\);", text, flags=re.S).group(1).split(",")]
    assert len(args) == len(cost[1]) and args[-3:] == ["const cmbpo_term_head_t *th", "const cmbpo_cost_head_t *ch", "void *stream"]
    rterm, rcost = _lib.SIGNATURES["cmbpo_replay_run_term"][1], _lib.SIGNATURES["cmbpo_replay_run_cost"][1]
    assert rcost == rterm[:3] + [C.POINTER(S)] + rterm[3:]
    # the frozen structs and the version are what they were; the head is no task bit
    assert C.sizeof(_lib.RolloutStruct) == 440 and C.sizeof(_lib.ReplayStruct) == 184 and C.sizeof(_lib.TermHeadStruct) == 24
    assert lib.cmbpo_version() == 6
    assert _lib.TASK_LEARNED_COST == 0x100 and not hasattr(_lib, "TASK_LOGISTIC_COST")
    for bad in (0x200 | _lib.TASK_HCS, 0x80 | _lib.TASK_HCS, 0x1000):
        assert _post_cost(lib, bad, _cost()) == -1
        assert lib.cmbpo_last_error().startswith(WHO + b": bad task"), lib.cmbpo_last_error()


def test_refusals_name_the_cost_head_before_any_hip_call(lib):
    from cmbpo_amd import _lib
    LC = _lib.TASK_HCS | _lib.TASK_LEARNED_COST
    for bad in (-1, 2, 7):
        assert _post_cost(lib, LC, _cost(kind=bad)) == -1
        msg = lib.cmbpo_last_error()
        assert msg.startswith(WHO) and b"cost head" in msg and b"kind" in msg, msg
    for bad in (float("nan"), float("inf"), float("-inf")):
        for kind in (0, 1):
            assert _post_cost(lib, LC, _cost(kind, bad)) == -1
            msg = lib.cmbpo_last_error()
            assert msg.startswith(WHO) and b"cost head" in msg and b"logit_shift" in msg, msg
    for task in (_lib.TASK_HCS, _lib.TASK_ANTSAFE, _lib.TASK_DEFAULT):
        assert _post_cost(lib, task, _cost(1), obs_dim=29) == -1
        msg = lib.cmbpo_last_error()
        assert msg.startswith(WHO) and b"cost head" in msg and b"CMBPO_TASK_LEARNED_COST" in msg, msg
        assert _post_cost(lib, task, _cost(0), obs_dim=29) == 0, lib.cmbpo_last_error()      # the magnitude reading needs no column
    # NULL buffers come after the head's own checks, and are named under this entry
    assert _post_cost(lib, LC, _cost(1), buffers=False) == -1
    assert lib.cmbpo_last_error().startswith(WHO + b": NULL buffer")
    # the attach entry: its own name, the same two checks; the learned-cost flag is the step's business
    rs = _lib.RolloutStruct()
    key = (C.c_int32 * 32)()
    assert lib.cmbpo_rollout_cost_head_attach(C.byref(rs), C.byref(_cost())) == -1              # no iscal: no key
    assert b"cmbpo_rollout_cost_head_attach" in lib.cmbpo_last_error()
    rs.iscal = C.cast(key, C.c_void_p)
    assert lib.cmbpo_rollout_cost_head_attach(C.byref(rs), None) == -1
    assert b"cmbpo_rollout_cost_head_detach" in lib.cmbpo_last_error()
    assert lib.cmbpo_rollout_cost_head_attach(C.byref(rs), C.byref(_cost(kind=2))) == -1
    assert b"cmbpo_rollout_cost_head_attach" in lib.cmbpo_last_error() and b"kind" in lib.cmbpo_last_error()
    assert lib.cmbpo_rollout_cost_head_attach(C.byref(rs), C.byref(_cost(1, float("nan")))) == -1
    assert b"logit_shift" in lib.cmbpo_last_error()
    assert lib.cmbpo_rollout_cost_head_detach(C.byref(rs)) == 0                                  # nothing attached: no error
    assert lib.cmbpo_rollout_cost_head_attach(C.byref(rs), C.byref(_cost(0, 0.0))) == 0          # an all-zero head is attached
    assert lib.cmbpo_rollout_cost_head_attach(C.byref(rs), C.byref(_cost(1, -0.5))) == 0         # replaces it
    # ... beside a termination head: detaching one leaves the other (the emptiness test has a term for each)
    assert lib.cmbpo_rollout_term_head_attach(C.byref(rs), C.byref(_term())) == 0
    assert lib.cmbpo_rollout_cost_head_detach(C.byref(rs)) == 0
    assert lib.cmbpo_rollout_term_head_detach(C.byref(rs)) == 0
    assert lib.cmbpo_rollout_cost_head_detach(C.byref(rs)) == 0
    assert lib.cmbpo_rollout_cost_head_detach(None) == -1


# naming rule 1 with its new first line: cost head present -- cmbpo_fakeenv_post_cost; else what the rule gave before
@pytest.mark.parametrize("xi,dis,th,ch", list(itertools.product((False, True), (False, True), (False, True), (None, 0, 1))))
def test_post_messages_carry_the_name_the_rule_gives(lib, xi, dis, th, ch):
    from cmbpo_amd import _lib
    head = None if ch is None else _cost(ch)
    want = (b"cmbpo_fakeenv_post_cost" if ch is not None else b"cmbpo_fakeenv_post_term" if th
            else b"cmbpo_fakeenv_post_disagreement" if dis else b"cmbpo_fakeenv_post_noise" if xi else b"cmbpo_fakeenv_post")
    assert _post_cost(lib, 9, head, xi, dis, th) == -1
    msg = lib.cmbpo_last_error()
    assert msg.startswith(want + b": bad task 9"), msg
    # good arguments and no rows: returns before the launch, with every feature subset
    assert _post_cost(lib, _lib.TASK_HCS | _lib.TASK_LEARNED_COST, head, xi, dis, th) == 0, lib.cmbpo_last_error()
    # a disagreement refusal keeps its words under the name the rule gives
    if dis:
        assert _post_cost(lib, _lib.TASK_HCS, head if ch != 1 else _cost(0), xi, dis, th) == -1
        msg = lib.cmbpo_last_error()
        assert msg.startswith((b"cmbpo_fakeenv_post_cost" if ch is not None else want) + b": kappa_cost"), msg


# naming rule 2 with its new first line: ch given -- cmbpo_replay_run_cost
@pytest.mark.parametrize("rc_given,th_given,ch_given", list(itertools.product((False, True), repeat=3)))
def test_replay_messages_carry_the_name_the_rule_gives(lib, rc_given, th_given, ch_given):
    from cmbpo_amd import _lib
    rp, cal, th, ch = _lib.ReplayStruct(), _lib.ReplayCalibStruct(), _term(), _cost()      # all-zero descriptors: the first check fails
    got = lib.cmbpo_replay_run_cost(C.byref(rp), C.byref(cal) if rc_given else None, C.byref(th) if th_given else None,
                                    C.byref(ch) if ch_given else None, None, 0, 7, None, None)
    want = (b"cmbpo_replay_run_cost" if ch_given else b"cmbpo_replay_run_term" if th_given
            else b"cmbpo_replay_run_calibrated" if rc_given else b"cmbpo_replay_run")
    msg = lib.cmbpo_last_error()
    assert got == -1 and msg.startswith(want + b": B 0 < 1"), msg


# ------------------------------------------------------------------------------------------------------------------
# the host side
# ------------------------------------------------------------------------------------------------------------------
def _fake_env(predicts_cost=True, **kw):
    from toyworld import ToyEnv
    from cmbpo_amd.fake_env import FakeEnv
    env = ToyEnv()
    n, a = int(np.prod(env.observation_space.shape)), int(np.prod(env.action_space.shape))

    class Model:
        is_ensemble = is_probabilistic = True
        in_dim, out_dim, device = n + a, n + 1 + int(predicts_cost), "cpu"
    return FakeEnv(env, "default", Model(), True, True, predicts_cost, **kw)


def test_fake_env_refusals_and_descriptor():
    from cmbpo_amd import _lib
    g = _fake_env()
    assert (g.cost_loss, g.cost_logit_shift) == ("gaussian", 0.0) and g.cost_head_struct() is None
    fe = _fake_env(cost_loss="logistic", cost_logit_shift=0.75)
    ch = fe.cost_head_struct()
    assert (ch.kind, ch.logit_shift, ch.cost_logit) == (_lib.COST_LOGISTIC, 0.75, None)
    with pytest.raises(ValueError, match="predicts_cost"):
        _fake_env(predicts_cost=False, cost_loss="logistic")
    with pytest.raises(ValueError, match="predicts_cost"):
        _fake_env(predicts_cost=False).set_cost_head(loss="logistic")
    with pytest.raises(ValueError, match="cost_loss"):
        _fake_env(cost_loss="probit")
    with pytest.raises(ValueError, match="cost_loss"):
        fe.set_cost_head(loss="probit")
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="cost_logit_shift"):
            _fake_env(cost_loss="logistic", cost_logit_shift=bad)
        with pytest.raises(ValueError, match="cost_logit_shift"):
            fe.set_cost_head(logit_shift=bad)
    assert (fe.cost_loss, fe.cost_logit_shift) == ("logistic", 0.75)            # a refusal changes nothing
    fe.set_cost_head(logit_shift=-1.5)                                          # None leaves a setting as it is
    assert (fe.cost_loss, fe.cost_logit_shift) == ("logistic", -1.5)
    fe.set_cost_head(loss="gaussian")
    assert fe.cost_head_struct() is None
    fe.set_cost_head("logistic", 0.0)
    assert fe.cost_head_struct().logit_shift == 0.0


def test_cmbpo_refusals():
    from cmbpo_amd.cmbpo import _cost_loss_args
    assert _cost_loss_args(False, "gaussian", 1.0, False, 20.0) == ("gaussian", 1.0, False)
    assert _cost_loss_args(True, "logistic", "balanced", True, 20.0) == ("logistic", "balanced", True)
    assert _cost_loss_args(True, "gaussian", 3, False, 20.0) == ("gaussian", 3.0, False)
    with pytest.raises(ValueError, match="m_learn_cost"):
        _cost_loss_args(False, "logistic", 1.0, False, 20.0)
    with pytest.raises(ValueError, match="m_cost_loss"):
        _cost_loss_args(True, "sigmoid", 1.0, False, 20.0)
    for bad in (-1.0, float("nan"), float("inf"), "most", None):
        with pytest.raises(ValueError, match="m_cost_pos_weight"):
            _cost_loss_args(True, "logistic", bad, False, 20.0)
    for bad in (2.0, "balanced"):
        with pytest.raises(ValueError, match="m_learn_cost"):
            _cost_loss_args(False, "gaussian", bad, False, 20.0)
    with pytest.raises(ValueError, match="m_cost_pos_weight_undo"):
        _cost_loss_args(True, "gaussian", 2.0, True, 20.0)
    with pytest.raises(ValueError, match="m_cost_pos_weight_undo"):
        _cost_loss_args(True, "logistic", 0.0, True, 20.0)


class _Model:
    def __init__(self, calls):
        self.calls = calls

    def save(self, d, e):
        self.calls.append(("save", e))

    def load(self, d, e):
        self.calls.append(("load", e))

    def set_logistic_columns(self, cols):
        self.calls.append(("kinds", cols))

    def set_column_weights(self, col, pos):
        self.calls.append(("weights", col, pos))


class _Env:
    def __init__(self, calls, loss="gaussian", shift=0.0):
        self.calls, self.cost_loss, self.cost_logit_shift = calls, loss, shift

    def set_cost_head(self, loss=None, logit_shift=None):
        self.calls.append(("cost_head", loss, logit_shift))
        if loss is not None:
            self.cost_loss = loss
        if logit_shift is not None:
            self.cost_logit_shift = logit_shift


def _bare(calls, learn_term=False, **env):
    from cmbpo_amd.cmbpo import CMBPO
    a = CMBPO.__new__(CMBPO)
    a._use_model, a._m_learn_term, a._m_learn_cost, a._epoch, a.obs_dim = True, learn_term, True, 4, 5
    a._model, a.fake_env, a._m_term_loss = _Model(calls), _Env(calls, **env), "gaussian"
    a._column_weights = {"m_term_pos_weight": 1.0, "m_term_loss_weight": 1.0, "m_cost_loss_weight": 1.0, "m_pos_weight_max": 20.0}
    return a


def test_save_load_round_trip_of_the_cost_loss_file(tmp_path):
    """`save` writes cost_loss_<epoch>.json, a file of its own; `load` sets the model's kinds BEFORE its weights and scalers come
    in and hands the reading to the FakeEnv; a missing file means 'gaussian'."""
    calls = []
    a = _bare(calls, loss="logistic", shift=float(np.log(4.0)))
    a._m_cost_loss, a._cost_pos_weight, a._cost_pos_weight_undo = "logistic", "balanced", True
    a.save(str(tmp_path))
    assert json.load(open(tmp_path / "cost_loss_4.json")) == {
        "m_cost_loss": "logistic", "m_cost_pos_weight": "balanced", "m_cost_pos_weight_undo": True, "cost_logit_shift": float(np.log(4.0))}
    assert not os.path.exists(tmp_path / "term_loss_4.json")              # the termination head's files are its own
    b = _bare(calls)
    assert (b._m_cost_loss, b._cost_pos_weight, b._cost_pos_weight_undo) == ("gaussian", 1.0, False)
    del calls[:]
    b.load(str(tmp_path), 4)
    assert (b._m_cost_loss, b._cost_pos_weight, b._cost_pos_weight_undo) == ("logistic", "balanced", True)
    # (column_weights_4.json holds all ones: `load` detaches the column weights, the next fit attaches the class weight anew)
    assert calls == [("kinds", [6]), ("load", 4), ("weights", None, None), ("cost_head", "logistic", float(np.log(4.0)))]
    os.remove(tmp_path / "cost_loss_4.json")
    del calls[:]
    b.load(str(tmp_path), 4)
    assert (b._m_cost_loss, b._cost_pos_weight, b._cost_pos_weight_undo) == ("gaussian", 1.0, False)
    assert calls == [("kinds", None), ("load", 4), ("weights", None, None), ("cost_head", "gaussian", 0.0)]
    # with a logistic termination head as well: both columns, the cost column first, the termination column the last
    c = _bare(calls, learn_term=True)
    c._m_cost_loss, c._m_term_loss = "logistic", "logistic"
    assert c._logistic_columns() == [6, -1]
    c._m_cost_loss = "gaussian"
    assert c._logistic_columns() == [-1]


def test_balanced_class_weight_of_the_cost_column_and_its_undo():
    from cmbpo_amd.cmbpo import balanced_pos_weight, cost_logit_shift
    calls = []
    a = _bare(calls, loss="logistic")
    a._m_cost_loss, a._cost_pos_weight, a._cost_pos_weight_undo = "logistic", "balanced", True
    outs = np.zeros((40, 7), np.float32)
    outs[:5, 6] = 1.0                      # 5 positives, 35 negatives: omega = 7
    outs[5, 6] = 0.5                       # exactly 0.5 is a negative (targets ABOVE 0.5 count as 1)
    outs[:, 5] = 1.0                       # the reward column is not the cost column
    extra = a._set_model_column_weights(outs)
    assert extra == {"cost_pos_weight": 7.0} and balanced_pos_weight(outs[:, 6], 20.0) == 7.0
    assert calls == [("cost_head", None, float(np.log(7.0))), ("weights", {6: 1.0}, {6: 7.0})]
    assert cost_logit_shift(7.0) == float(np.log(7.0)) and cost_logit_shift(1.0) == 0.0
    # the clip: no positives at all -> n_neg / 1 clipped at m_pos_weight_max; mostly positives -> 1
    outs[:, 6] = 0.0
    assert a._set_model_column_weights(outs) == {"cost_pos_weight": 20.0}
    outs[:30, 6] = 1.0
    del calls[:]
    assert a._set_model_column_weights(outs) == {"cost_pos_weight": 1.0}
    assert calls[0] == ("cost_head", None, 0.0)
    # a fixed weight, no undo: attached, logged, the head is left alone
    a._cost_pos_weight, a._cost_pos_weight_undo = 3.0, False
    del calls[:]
    assert a._set_model_column_weights(outs) == {"cost_pos_weight": 3.0}
    assert calls == [("weights", {6: 1.0}, {6: 3.0})]
    # the defaults: nothing attached, nothing logged
    a._cost_pos_weight = 1.0
    del calls[:]
    assert a._set_model_column_weights(outs) == {} and calls == []
