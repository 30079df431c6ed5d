"""CPU: user-defined termination / cost rules (cmbpo_amd.statics) -- ``TaskRules.numpy_fns()`` against hand-written NumPy
functions of the kind a user of the reference adds to models/statics.py, bit for bit on adversarial rows; registration
through the C-ABI (round trip, equal sets share an id, every invalid field is named); and the argument checks of
cmbpo_fakeenv_post for rule ids, which precede any HIP call."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cmbpo_amd import _lib
    return _lib.lib()


# ---- textbook static functions (the MBPO forms), as a user would write them for the reference ------------------------------
def walker2d_term(obs, act, next_obs):
    height = next_obs[..., 0]
    angle = next_obs[..., 1]
    not_done = (height > 0.8) * (height < 2.0) * (angle > -1.0) * (angle < 1.0)
    return (~not_done)[..., None]


def ant_term(obs, act, next_obs):
    x = next_obs[..., 0]
    not_done = np.isfinite(next_obs).all(axis=-1) * (x >= 0.2) * (x <= 1.0)
    return (~not_done)[..., None]


def inverted_pendulum_term(obs, act, next_obs):
    notdone = np.isfinite(next_obs).all(axis=-1) * (np.abs(next_obs[..., 1]) <= .2)
    return (~notdone)[..., None]


def _textbook():
    from cmbpo_amd.statics import TaskRules, healthy
    return {
        "walker2d": (walker2d_term, None, TaskRules([healthy(cols=0, lo=0.8, hi=2.0, lo_strict=True, hi_strict=True),
                                                      healthy(cols=1, lo=-1.0, hi=1.0, lo_strict=True, hi_strict=True)])),
        "ant": (ant_term, None, TaskRules([healthy(cols=0, lo=0.2, hi=1.0)], require_finite=True)),
        "pendulum": (inverted_pendulum_term, None, TaskRules([healthy(cols=1, abs=True, hi=0.2)], require_finite=True)),
    }


def _cases():
    import worlds_rules
    out = dict(_textbook())
    for name, case in worlds_rules.CASES.items():
        for thr in case["candidates"]:
            out["%s%r" % (name, thr)] = case["fns"](*thr) + (worlds_rules.build_rules(case["rules"](*thr)),)
    return out


def _thresholds(rules):
    """Every (column selector, scale, bound) of the set: where the adversarial rows put their values."""
    out = []
    for c in rules.clauses:
        for bound in (float(c.lo), float(c.hi)):
            if np.isfinite(bound):
                out.append((c, bound))
    return out


def _adversarial_rows(rules, D, A, rng):
    """[n, D] / [n, A] rows: per threshold the value whose scaled product is exactly the bound, its float32 neighbours on
    both sides (products that round across the bound), both signs; NaN, +-inf and -0.0 in tested and untested columns."""
    up, dn = lambda v: np.nextafter(np.float32(v), np.float32(INF)), lambda v: np.nextafter(np.float32(v), np.float32(-INF))
    rows = []

    def fresh():
        return dict(obs=(rng.standard_normal(D) * 0.3).astype(np.float32), act=rng.uniform(-1, 1, A).astype(np.float32),
                    next_obs=(rng.standard_normal(D) * 0.3).astype(np.float32))

    for _ in range(40):
        rows.append(fresh())
    for c, bound in _thresholds(rules):
        width = A if c.src == "act" else D
        col0 = c.col0 + width if c.col0 < 0 else c.col0
        n = width - col0 if c.n_cols == -1 else c.n_cols
        x0 = np.float32(np.float32(bound) / c.scale)
        vals = [x0, up(x0), dn(x0), up(up(x0)), dn(dn(x0)), -x0, up(-x0), dn(-x0)]
        for col in sorted({col0, col0 + n - 1}):
            for v in vals + [np.float32(np.nan), np.float32(INF), np.float32(-INF), np.float32(-0.0), np.float32(0.0)]:
                r = fresh()
                r[c.src][col] = v
                rows.append(r)
    for src, width in (("next_obs", D), ("obs", D), ("act", A)):
        for col in range(width):
            for v in (np.nan, INF, -INF, -0.0):
                r = fresh()
                r[src][col] = np.float32(v)
                rows.append(r)
    return tuple(np.stack([r[k] for r in rows]) for k in ("obs", "act", "next_obs"))


DIMS = {"g15_trace_rules_hopper": (21, 3), "g15_trace_rules_fatal": (47, 17), "g15_trace_rules_nodone": (20, 6)}


@pytest.mark.parametrize("lead", [1, 2, 3])
def test_numpy_fns_equal_hand_written_functions_bit_for_bit(lead):
    rng = np.random.default_rng(lead)
    for name, (hand_term, hand_cost, rules) in _cases().items():
        D, A = next((d for k, d in DIMS.items() if name.startswith(k)), (11, 3))
        obs, act, nxt = _adversarial_rows(rules, D, A, rng)
        n = obs.shape[0] - obs.shape[0] % 6
        shape = {1: (n,), 2: (n // 2, 2), 3: (n // 6, 2, 3)}[lead]
        obs, act, nxt = (a[:n].reshape(shape + a.shape[-1:]) for a in (obs, act, nxt))
        term_fn, cost_fn = rules.numpy_fns()
        with np.errstate(all="ignore"):
            t = term_fn(obs, act, nxt)
            assert t.dtype == bool and t.shape == shape + (1,), name
            if hand_term is not None:
                want = hand_term(obs, act, nxt)
                assert want.dtype == bool and want.shape == t.shape
                np.testing.assert_array_equal(t, want, err_msg=name)
                assert t.any() and not t.all(), name
            else:
                assert not t.any()
            if hand_cost is None:
                assert cost_fn is None, name
            else:
                c, want = cost_fn(obs, act, nxt), hand_cost(obs, act, nxt)
                assert c.dtype == np.float32 == want.dtype and c.shape == shape + (1,) == want.shape, name
                np.testing.assert_array_equal(c.view(np.uint32), want.view(np.uint32), err_msg=name)
                assert set(np.unique(c)) == {0.0, 1.0}, name


def test_nan_separates_healthy_from_fatal():
    from cmbpo_amd.statics import TaskRules, fatal, healthy
    z = np.array([[np.nan], [0.5], [1.5], [2.5], [1.0], [2.0]], np.float32)
    o, a = np.zeros((6, 1), np.float32), np.zeros((6, 1), np.float32)
    h = TaskRules([healthy(cols=0, lo=1.0, hi=2.0)]).numpy_fns()[0](o, a, z)[:, 0]
    f = TaskRules([fatal(cols=0, hi=1.0, hi_strict=True), fatal(cols=0, lo=2.0, lo_strict=True)]).numpy_fns()[0](o, a, z)[:, 0]
    assert h.tolist() == [True, True, False, True, False, False]          # 1.0 <= z <= 2.0 ends a NaN branch
    assert f.tolist() == [False, True, False, True, False, False]         # z < 1.0 or z > 2.0 keeps it alive
    inf = np.array([[INF]], np.float32)
    assert not TaskRules([healthy(cols=0, lo=3.2)]).numpy_fns()[0](o[:1], a[:1], inf)[0, 0]      # +inf holds against hi = +inf
    assert TaskRules([healthy(cols=0, lo=3.2)], require_finite=True).numpy_fns()[0](o[:1], a[:1], inf)[0, 0]


def test_builder_arguments_are_checked():
    from cmbpo_amd.statics import TaskRules, healthy, register_task
    for kw in (dict(cols=slice(0, 4, 2)), dict(cols=slice(3, 3)), dict(cols=slice(1, -1)), dict(src="state")):
        with pytest.raises(ValueError):
            healthy(**kw)
    with pytest.raises(ValueError):
        TaskRules([healthy(cols=0)] * 17)
    with pytest.raises(TypeError):
        TaskRules([dict(cols=0)])
    with pytest.raises(ValueError):
        register_task("AntSafe-v2", TaskRules())
    with pytest.raises(ValueError):
        healthy(cols=5).holds(np.zeros((2, 3)), np.zeros((2, 1)), np.zeros((2, 3)))


def test_registration_round_trip_and_equal_sets_share_an_id(lib):
    import worlds_rules
    from cmbpo_amd import _lib, statics
    case = worlds_rules.CASES["g15_trace_rules_hopper"]
    rules = worlds_rules.build_rules(case["rules"](-0.125, 0.3, 3.5))
    before = lib.cmbpo_task_rules_count()
    tid = rules.task_id
    assert _lib.TASK_USER_BASE <= tid < _lib.TASK_USER_BASE + _lib.TASK_USER_SLOTS and tid < _lib.TASK_LEARNED_COST
    assert lib.cmbpo_task_rules_count() in (before, before + 1)
    for _ in range(100):       # building the same rules again and again never takes another slot
        assert worlds_rules.build_rules(case["rules"](-0.125, 0.3, 3.5)).task_id == tid
    assert lib.cmbpo_task_rules_count() <= before + 1
    other = worlds_rules.build_rules(case["rules"](-0.125, 0.3, 3.75))
    assert other.task_id != tid
    out = _lib.TaskRulesStruct()
    assert C.sizeof(out) == 528 and C.sizeof(_lib.RuleClauseStruct) == 32
    for task in (tid, tid | _lib.TASK_LEARNED_COST):
        assert lib.cmbpo_task_rules_get(task, C.byref(out)) == 0
        assert bytes(out) == bytes(rules.struct())
    assert (out.n_clauses, out.require_finite, out.cost_on_term, out.reserved) == (4, 1, 0, 0)
    c = out.clause[3]
    assert (c.role, c.src, c.col0, c.n_cols) == (_lib.RULE_COST, _lib.RULE_SRC_NEXT_OBS, -1, 1)
    assert c.flags == _lib.RULE_ABS | _lib.RULE_LO_STRICT and (c.scale, c.lo, c.hi) == (10.0, 3.5, INF)
    c = out.clause[0]
    assert (c.col0, c.n_cols, c.flags, c.hi) == (1, -1, _lib.RULE_ABS | _lib.RULE_HI_STRICT, 100.0)
    assert lib.cmbpo_task_rules_get(_lib.TASK_USER_BASE + lib.cmbpo_task_rules_count(), C.byref(out)) == -1
    assert b"not registered" in lib.cmbpo_last_error()
    assert lib.cmbpo_task_rules_get(_lib.TASK_ANTSAFE, C.byref(out)) == -1
    statics.register_task("RoundTrip-v0", rules)
    assert statics.lookup("RoundTrip-v0") == (tid, rules) and statics.lookup(rules) == (tid, rules)
    assert statics.lookup("AntSafe-v2") == (_lib.TASK_ANTSAFE, None) and statics.lookup("Nope-v9") == (_lib.TASK_DEFAULT, None)


def test_each_invalid_field_is_rejected_by_name(lib):
    from cmbpo_amd import _lib
    from cmbpo_amd.statics import TaskRules, healthy

    def attempt(edit):
        s = TaskRules([healthy(cols=0, lo=0.0, hi=1.0)]).struct()
        edit(s)
        out = C.c_int(-5)
        rc = lib.cmbpo_task_rules_register(C.byref(s), C.byref(out))
        return rc, out.value, lib.cmbpo_last_error()

    def setter(path, value):
        def edit(s):
            obj = s.clause[0] if path != "top" and not hasattr(s, path) else s
            setattr(obj, path, value)
        return edit

    before = lib.cmbpo_task_rules_count()
    bad = [("n_clauses", 17), ("n_clauses", -1), ("reserved", 1), ("require_finite", 2), ("cost_on_term", -1),
           ("role", 3), ("role", -1), ("src", 3), ("flags", 16), ("flags", -1), ("n_cols", 0), ("n_cols", -2),
           ("scale", INF), ("scale", float("nan")), ("lo", float("nan")), ("hi", float("nan")), ("lo", 2.0)]
    for field, value in bad:
        rc, task, msg = attempt(setter(field, value))
        assert rc == -1 and task == -5, (field, value)
        # the message names the field, and for a clause's field the clause: "... clause 0: unknown role 3", "... clause 0: lo is NaN"
        top = field in ("n_clauses", "reserved", "require_finite", "cost_on_term")
        pattern = (r"cmbpo_task_rules_register: %s\b" if top else r"cmbpo_task_rules_register: clause 0: (unknown )?%s\b") % field
        assert re.search(pattern.encode(), msg), (field, value, msg)
    assert lib.cmbpo_task_rules_register(None, None) == -1
    assert lib.cmbpo_task_rules_count() == before
    rc, task, _ = attempt(lambda s: None)
    assert rc == 0 and task >= _lib.TASK_USER_BASE
    rc, task2, _ = attempt(setter("lo", 1.0))        # lo == hi: a point interval is valid
    assert rc == 0 and task2 != task


def _post(lib, task, obs_dim, act_dim, act=None):
    return lib.cmbpo_fakeenv_post(task, 7, obs_dim, act_dim, None, None, 0, None, act, None, None, None, 0,
                                  None, None, None, None, None, None, None, None)


def test_post_rejects_bad_rule_ids_and_columns_without_a_gpu(lib):
    """Validation precedes any HIP call (as in test_cabi_exports.test_bad_arguments_return_error_codes_without_a_gpu): with
    NULL buffers every call returns -1, and the message says which check it failed."""
    from cmbpo_amd import _lib
    from cmbpo_amd.statics import TaskRules, cost, healthy
    F = _lib.TASK_LEARNED_COST
    rules = TaskRules([healthy(cols=20, lo=0.0), cost(src="act", cols=slice(-3, None), abs=True, lo=0.5)])
    tid = rules.task_id
    free = _lib.TASK_USER_BASE + lib.cmbpo_task_rules_count()
    for task in (free, free | F, _lib.TASK_USER_BASE + _lib.TASK_USER_SLOTS - 1):
        if task & ~F < free:
            continue
        assert _post(lib, task, 29, 8) == -1 and b"not registered" in lib.cmbpo_last_error()
    for task in (9, _lib.TASK_USER_BASE + _lib.TASK_USER_SLOTS, F | (_lib.TASK_USER_BASE + _lib.TASK_USER_SLOTS), 0x200 | tid):
        assert _post(lib, task, 29, 8) == -1 and b"bad task" in lib.cmbpo_last_error()
    dummy = (C.c_float * 8)()
    for task in (tid, tid | F):
        assert _post(lib, task, 20, 8, dummy) == -1 and b"clause 0" in lib.cmbpo_last_error() and b"width 20" in lib.cmbpo_last_error()
        assert _post(lib, task, 21, 2, dummy) == -1 and b"clause 1" in lib.cmbpo_last_error() and b"act" in lib.cmbpo_last_error()
        assert _post(lib, task, 21, 8, None) == -1 and b"d_act is NULL" in lib.cmbpo_last_error()
        assert _post(lib, task, 21, 8, dummy) == -1 and b"NULL buffer" in lib.cmbpo_last_error()      # the rules' own checks passed
