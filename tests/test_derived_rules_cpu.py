"""CPU: derived quantities of the task rules (cmbpo_amd.statics.derived / dist_sq / speed_sq / tilt, cmbpo_rule_derived_table_t)
-- ``TaskRules.numpy_fns()`` against hand-written float32 NumPy in the kernel's operation order, bit for bit on rows at, beside
and far from every threshold; the layout of the three new structs; registration through cmbpo_task_rules_register_ex (round
trip, equal sets share a slot, every invalid field is named); and the launch-time checks, which precede any HIP call."""
import ctypes as C
import re

import numpy as np
import pytest

INF = float("inf")
F = np.float32


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cmbpo_amd import _lib
    return _lib.lib()


# ---- the hand-written side: float32 arrays, one NumPy operation per rounding, in the order of include/cmbpo_hip.h ------------
HZ = ((F(0.5), F(-0.25)), (F(-1.0), F(0.75)))      # hazard centres
R2, V2, TILT0, GOAL = F(0.25), F(2.25), F(-0.125), F(0.125)      # values the float32 arithmetic reaches exactly


def _sq(x, c):
    d = x - F(c)
    return d * d


def hazards_cost(obs, act, next_obs):
    """two circles on next_obs columns 0, 1: inside either costs 1"""
    x, y = next_obs[..., 0], next_obs[..., 1]
    hit = np.zeros(x.shape, bool)
    for cx, cy in HZ:
        g = F(0.0) + F(1.0) * _sq(x, cx)
        g = g + F(1.0) * _sq(y, cy)
        hit |= g <= R2
    return hit.astype(F)[..., None]


def speed_cost(obs, act, next_obs):
    """vx^2 + vy^2 > v^2 on the last two columns of next_obs"""
    g = F(0.0) + F(1.0) * _sq(next_obs[..., -2], 0.0)
    g = g + F(1.0) * _sq(next_obs[..., -1], 0.0)
    return (g > V2).astype(F)[..., None]


def tilt_term(obs, act, next_obs):
    """healthy: height in [0.2, 1], 1 - 2 (q1^2 + q2^2) >= -0.125, finite state"""
    z, q1, q2 = next_obs[..., 0], next_obs[..., 2], next_obs[..., 3]
    g = F(1.0) + F(-2.0) * _sq(q1, 0.0)
    g = g + F(-2.0) * _sq(q2, 0.0)
    ok = np.isfinite(next_obs).all(-1) & (z >= F(0.2)) & (z <= F(1.0)) & (g >= TILT0)
    return (~ok)[..., None]


def goal_cost(obs, act, next_obs):
    """linear: |(goal - robot) * 4| < 0.5 with goal = obs column 4 shifted by an action, robot = next_obs column 1"""
    g = F(0.25) + F(1.0) * (obs[..., 4] - F(0.0))
    g = g + F(-1.0) * (next_obs[..., 1] - F(0.0))
    g = g + F(0.5) * (act[..., -1] - GOAL)
    return (np.abs(g * F(4.0)) < F(0.5)).astype(F)[..., None]


def _cases():
    from cmbpo_amd.statics import TaskRules, cost, derived, dist_sq, healthy, speed_sq, term, tilt
    return {
        "hazards": (None, hazards_cost, TaskRules([cost(src="derived", cols=slice(0, None), any=True, hi=R2)],
                                                  derived=[dist_sq((0, 1), c) for c in HZ])),
        "speed": (None, speed_cost, TaskRules([cost(src="derived", cols=0, lo=V2, lo_strict=True)], derived=[speed_sq((-2, -1))])),
        "tilt": (tilt_term, None, TaskRules([healthy(cols=0, lo=0.2, hi=1.0), healthy(src="derived", cols=-1, lo=TILT0)],
                                            derived=[tilt(2, 3)], require_finite=True)),
        "goal": (None, goal_cost, TaskRules([cost(src="derived", cols=0, scale=4.0, abs=True, hi=0.5, hi_strict=True)],
                                            derived=[derived([term(4, src="obs"), term(1, w=-1.0), term(-1, src="act", w=0.5, c=GOAL)],
                                                             bias=0.25)])),
    }


def _rows(rules, D, A, rng):
    """Rows whose derived quantity sits at a threshold and one and two ulps beside it (found by walking one term column ulp by
    ulp), far beyond it, and NaN / +-inf / -0.0 in every column of every source."""
    up, dn = lambda v: np.nextafter(F(v), F(INF)), lambda v: np.nextafter(F(v), F(-INF))
    rows = []

    def fresh():
        return dict(obs=(rng.standard_normal(D) * 0.3).astype(F), act=rng.uniform(-1, 1, A).astype(F),
                    next_obs=(rng.standard_normal(D) * 0.3).astype(F))

    def g_of(r, q):
        return q.values(r["obs"][None], r["act"][None], r["next_obs"][None])[0]

    for _ in range(40):
        rows.append(fresh())
    for cl in rules.clauses:
        if cl.src != "derived":
            continue
        n = len(rules.derived)
        col0 = cl.col0 + n if cl.col0 < 0 else cl.col0
        cnt = n - col0 if cl.n_cols == -1 else cl.n_cols
        for q in rules.derived[col0:col0 + cnt]:
            t = q.terms[0]
            for bound in (float(cl.lo), float(cl.hi)):
                if not np.isfinite(bound):
                    continue
                want = F(F(bound) / cl.scale)
                # the other terms at their centres (they add w * 0), the first one solved for; then walk it ulp by ulp until g
                # is the threshold (the cases' thresholds are values the arithmetic reaches)
                r = fresh()
                for o in q.terms[1:]:
                    r[o.src][o.col] = o.c
                d = (float(want) - float(q.bias)) / float(t.w)
                x = F(float(t.c) + (np.sqrt(max(d, 0.0)) if t.pow == 2 else d))
                for _ in range(16):
                    r[t.src][t.col] = x
                    g = g_of(r, q)
                    if g == want:
                        break
                    x = up(x) if (g < want) == (t.w > 0) else dn(x)
                for v in (x, up(x), dn(x), up(up(x)), dn(dn(x)), F(x + 50.0), F(x - 50.0), F(1e20), F(-1e20)):
                    rr = {k: a.copy() for k, a in r.items()}
                    rr[t.src][t.col] = v
                    rows.append(rr)
    for src, width in (("next_obs", D), ("obs", D), ("act", A)):
        for col in range(width):
            for v in (np.nan, INF, -INF, -0.0):
                r = fresh()
                r[src][col] = F(v)
                rows.append(r)
    r = fresh()            # inf - inf inside one quantity: NaN by the arithmetic, never holds
    r["next_obs"][:] = F(INF)
    r["obs"][:] = F(INF)
    rows.append(r)
    return tuple(np.stack([r[k] for r in rows]) for k in ("obs", "act", "next_obs"))


@pytest.mark.parametrize("lead", [1, 2, 3])
def test_numpy_fns_equal_hand_written_float32_numpy_bit_for_bit(lead):
    rng = np.random.default_rng(10 + lead)
    for name, (hand_term, hand_cost, rules) in _cases().items():
        obs, act, nxt = _rows(rules, 7, 3, rng)
        n = obs.shape[0] - obs.shape[0] % 6
        shape = {1: (n,), 2: (n // 2, 2), 3: (n // 6, 2, 3)}[lead]
        obs, act, nxt = (a[:n].reshape(shape + a.shape[-1:]) for a in (obs, act, nxt))
        term_fn, cost_fn = rules.numpy_fns()
        with np.errstate(all="ignore"):
            t = term_fn(obs, act, nxt)
            assert t.dtype == bool and t.shape == shape + (1,), name
            if hand_term is not None:
                np.testing.assert_array_equal(t, hand_term(obs, act, nxt), err_msg=name)
                assert t.any() and not t.all(), name
            else:
                assert not t.any(), name
            if hand_cost is None:
                assert cost_fn is None, name
            else:
                c, want = cost_fn(obs, act, nxt), hand_cost(obs, act, nxt)
                assert c.dtype == F == want.dtype and c.shape == shape + (1,) == want.shape, name
                np.testing.assert_array_equal(c.view(np.uint32), want.view(np.uint32), err_msg=name)
                assert set(np.unique(c)) == {0.0, 1.0}, name
            g = rules.derived_values(obs, act, nxt)
            assert g.dtype == F and g.shape == shape + (len(rules.derived),)


def test_rows_reach_the_threshold_and_its_neighbours():
    """the adversarial rows do what their name says: for every case some row's quantity equals the threshold bit for bit and
    others sit within a few ulps on either side (the column moved by one and two of its own ulps)"""
    rng = np.random.default_rng(3)
    for name, (_, _, rules) in _cases().items():
        obs, act, nxt = _rows(rules, 7, 3, rng)
        with np.errstate(all="ignore"):
            g = rules.derived_values(obs, act, nxt)
        cl = next(c for c in rules.clauses if c.src == "derived")
        bound = F(cl.lo) if np.isfinite(cl.lo) else F(cl.hi)
        f = g[..., cl.col0] * cl.scale
        f = np.abs(f) if cl.abs else f
        assert (f == bound).any(), name
        ulp = np.abs(np.spacing(bound))          # (an ulp of the column is up to 16 ulps of a quantity near its threshold)
        assert ((f > bound) & (f <= bound + 16 * ulp)).any() and ((f < bound) & (f >= bound - 16 * ulp)).any(), name


def test_nan_never_holds_and_inf_minus_inf_is_nan():
    from cmbpo_amd.statics import TaskRules, derived, fatal, healthy, term
    rules = TaskRules([healthy(src="derived", cols=0, lo=-INF, hi=INF), fatal(src="derived", cols=1, lo=-INF, hi=INF)],
                      derived=[derived([term(0), term(1, w=-1.0)]), derived([term(0)])])
    nxt = np.array([[INF, INF], [np.nan, 0.0], [1.0, 2.0], [INF, 0.0]], F)
    z = np.zeros((4, 1), F)
    with np.errstate(all="ignore"):
        g = rules.derived_values(z, z, nxt)
        assert np.isnan(g[0, 0]) and np.isnan(g[1, 0]) and g[2, 0] == -1.0 and g[3, 0] == INF
        healthy_holds = rules.clauses[0].holds(z, z, nxt, g)
        fatal_holds = rules.clauses[1].holds(z, z, nxt, g)
    assert healthy_holds.tolist() == [False, False, True, True] and fatal_holds.tolist() == [True, False, True, True]


def test_struct_sizes_and_offsets():
    from cmbpo_amd import _lib
    T, D, TB = _lib.RuleTermStruct, _lib.RuleDerivedStruct, _lib.RuleDerivedTableStruct
    assert C.sizeof(T) == 16 and [(getattr(T, n).offset, getattr(T, n).size) for n in ("src", "pow", "col", "w", "c")] == \
        [(0, 2), (2, 2), (4, 4), (8, 4), (12, 4)]
    assert C.sizeof(D) == 80 and [(getattr(D, n).offset, getattr(D, n).size) for n in ("n_terms", "bias", "reserved", "term")] == \
        [(0, 4), (4, 4), (8, 8), (16, 64)]
    assert C.sizeof(TB) == 656 and [(getattr(TB, n).offset, getattr(TB, n).size) for n in ("n_derived", "reserved", "derived")] == \
        [(0, 4), (4, 12), (16, 640)]
    assert C.sizeof(_lib.TaskRulesStruct) == 528 and C.sizeof(_lib.RuleClauseStruct) == 32
    assert (_lib.RULE_SRC_DERIVED, _lib.RULE_MAX_DERIVED, _lib.RULE_MAX_TERMS) == (3, 8, 4)


def _hazard_rules(cx=0.5):
    from cmbpo_amd.statics import TaskRules, cost, dist_sq, healthy, tilt
    return TaskRules([cost(src="derived", cols=slice(0, 2), any=True, hi=0.09), healthy(src="derived", cols=-1, lo=-0.7)],
                     derived=[dist_sq((0, 1), (cx, -0.25)), dist_sq((0, 1), (-1.0, 0.75), src="obs"), tilt(2, 3)], require_finite=True)


def test_registration_round_trip_and_equal_sets_share_a_slot(lib):
    from cmbpo_amd import _lib, statics
    rules = _hazard_rules()
    before = lib.cmbpo_task_rules_count()
    tid = rules.task_id
    assert _lib.TASK_USER_BASE <= tid < _lib.TASK_USER_BASE + _lib.TASK_USER_SLOTS
    assert lib.cmbpo_task_rules_count() in (before, before + 1)
    for _ in range(100):
        assert _hazard_rules().task_id == tid
    assert lib.cmbpo_task_rules_count() <= before + 1
    other = _hazard_rules(cx=0.5000001)          # a changed c: another id
    assert other.task_id != tid
    out, rout = _lib.RuleDerivedTableStruct(), _lib.TaskRulesStruct()
    for task in (tid, tid | _lib.TASK_LEARNED_COST):
        assert lib.cmbpo_task_rules_get_derived(task, C.byref(out)) == 0 and bytes(out) == bytes(rules.derived_struct())
        assert lib.cmbpo_task_rules_get(task, C.byref(rout)) == 0 and bytes(rout) == bytes(rules.struct())
    assert out.n_derived == 3 and list(out.reserved) == [0, 0, 0]
    d = out.derived[2]
    assert (d.n_terms, d.bias) == (2, 1.0) and [(m.src, m.pow, m.col, m.w, m.c) for m in d.term[:2]] == [(0, 2, 2, -2.0, 0.0), (0, 2, 3, -2.0, 0.0)]
    m = out.derived[1].term[1]
    assert (m.src, m.pow, m.col, m.w, m.c) == (_lib.RULE_SRC_OBS, 2, 1, 1.0, 0.75)
    assert (rout.clause[0].src, rout.clause[0].col0, rout.clause[0].n_cols, rout.clause[1].col0) == (_lib.RULE_SRC_DERIVED, 0, 2, -1)
    # an id registered without derived quantities: all zeros; an unregistered one: an error
    plain = statics.TaskRules([statics.healthy(cols=0, lo=0.125)])
    assert lib.cmbpo_task_rules_get_derived(plain.task_id, C.byref(out)) == 0 and bytes(out) == bytes(656)
    assert lib.cmbpo_task_rules_get_derived(_lib.TASK_USER_BASE + lib.cmbpo_task_rules_count(), C.byref(out)) == -1
    assert b"not registered" in lib.cmbpo_last_error()
    assert lib.cmbpo_task_rules_get_derived(_lib.TASK_ANTSAFE, C.byref(out)) == -1
    assert lib.cmbpo_task_rules_get_derived(tid, None) == -1
    assert statics.lookup(rules) == (tid, rules)
    statics.register_task("Hazards-v0", rules)
    assert statics.lookup("Hazards-v0") == (tid, rules)


def test_ex_without_derived_is_the_old_entry(lib):
    from cmbpo_amd import _lib
    from cmbpo_amd.statics import TaskRules, cost, healthy
    s = TaskRules([healthy(cols=0, lo=0.375, hi=1.0), cost(src="act", cols=0, abs=True, lo=0.5)]).struct()
    old, a, b = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert lib.cmbpo_task_rules_register(C.byref(s), C.byref(old)) == 0
    n = lib.cmbpo_task_rules_count()
    assert lib.cmbpo_task_rules_register_ex(C.byref(s), None, C.byref(a)) == 0
    empty = _lib.RuleDerivedTableStruct()
    assert lib.cmbpo_task_rules_register_ex(C.byref(s), C.byref(empty), C.byref(b)) == 0
    assert a.value == b.value == old.value and lib.cmbpo_task_rules_count() == n
    # ... the same validation, in the same words: a derived clause without derived quantities is an unknown source
    s.clause[0].src = _lib.RULE_SRC_DERIVED
    for d in (None, C.byref(empty)):
        assert lib.cmbpo_task_rules_register_ex(C.byref(s), d, C.byref(a)) == -1
        assert re.search(rb"cmbpo_task_rules_register: clause 0: unknown src 3", lib.cmbpo_last_error())
    # the same clause table with derived quantities is another id, and the old entry does not find it
    s2 = _hazard_rules().struct()
    with_d = _hazard_rules().task_id
    s2.clause[0].src = s2.clause[1].src = _lib.RULE_SRC_NEXT_OBS
    s2.clause[1].col0 = 0
    d2 = _hazard_rules().derived_struct()
    assert lib.cmbpo_task_rules_register_ex(C.byref(s2), C.byref(d2), C.byref(a)) == 0
    assert lib.cmbpo_task_rules_register(C.byref(s2), C.byref(b)) == 0
    assert len({a.value, b.value, with_d}) == 3


def test_each_invalid_field_of_the_derived_table_is_rejected_by_name(lib):
    from cmbpo_amd import _lib

    def attempt(edit):
        r = _hazard_rules()
        s, d = r.struct(), r.derived_struct()
        edit(s, d)
        out = C.c_int(-5)
        rc = lib.cmbpo_task_rules_register_ex(C.byref(s), C.byref(d), C.byref(out))
        return rc, out.value, lib.cmbpo_last_error()

    def top(name, value):
        return lambda s, d: setattr(d, name, value)

    def res(obj_of, j):
        def edit(s, d):
            obj_of(d).reserved[j] = 1
        return edit

    def dq(name, value):
        return lambda s, d: setattr(d.derived[2], name, value)

    def tm(name, value):
        return lambda s, d: setattr(d.derived[2].term[1], name, value)

    def cl(**kw):
        def edit(s, d):
            for k, v in kw.items():
                setattr(s.clause[0], k, v)
        return edit

    W = rb"cmbpo_task_rules_register_ex: "
    bad = [(top("n_derived", 9), W + rb"n_derived\b"), (top("n_derived", -1), W + rb"n_derived\b"),
           (res(lambda d: d, 0), W + rb"derived table: reserved\b"), (res(lambda d: d, 2), W + rb"derived table: reserved\b"),
           (dq("n_terms", 0), W + rb"derived 2: n_terms\b"), (dq("n_terms", 5), W + rb"derived 2: n_terms\b"),
           (dq("bias", INF), W + rb"derived 2: bias\b"), (dq("bias", float("nan")), W + rb"derived 2: bias\b"),
           (res(lambda d: d.derived[2], 0), W + rb"derived 2: reserved\b"), (res(lambda d: d.derived[2], 1), W + rb"derived 2: reserved\b"),
           (tm("src", 3), W + rb"derived 2: term 1: unknown src\b"), (tm("src", -1), W + rb"derived 2: term 1: unknown src\b"),
           (tm("pow", 0), W + rb"derived 2: term 1: pow\b"), (tm("pow", 3), W + rb"derived 2: term 1: pow\b"),
           (tm("w", INF), W + rb"derived 2: term 1: w\b"), (tm("w", float("nan")), W + rb"derived 2: term 1: w\b"),
           (tm("c", -INF), W + rb"derived 2: term 1: c\b"), (tm("c", float("nan")), W + rb"derived 2: term 1: c\b"),
           (cl(col0=3), W + rb"clause 0: .*derived"), (cl(col0=2, n_cols=2), W + rb"clause 0: .*derived"),
           (cl(col0=-4), W + rb"clause 0: .*derived"), (cl(n_cols=4), W + rb"clause 0: .*derived"),
           # the clause table's own checks, under the new entry's name
           (cl(src=4), W + rb"clause 0: unknown src\b"), (cl(flags=16), W + rb"clause 0: unknown flags\b"),
           (lambda s, d: setattr(s, "reserved", 1), W + rb"reserved\b")]
    before = lib.cmbpo_task_rules_count()
    for edit, pattern in bad:
        rc, task, msg = attempt(edit)
        assert rc == -1 and task == -5, (pattern, msg)
        assert re.search(pattern, msg), (pattern, msg)
    assert lib.cmbpo_task_rules_register_ex(None, None, None) == -1
    assert lib.cmbpo_task_rules_count() == before
    rc, task, _ = attempt(lambda s, d: None)
    assert rc == 0 and task >= _lib.TASK_USER_BASE
    # fields past n_terms / n_derived are not read: only the byte image differs, so the id does
    rc, task2, msg = attempt(lambda s, d: setattr(d.derived[2].term[3], "pow", 7))
    assert rc == 0 and task2 != task, msg


def test_builders_check_their_arguments():
    from cmbpo_amd.statics import TaskRules, cost, derived, dist_sq, healthy, speed_sq, term
    for kw in (dict(src="derived"), dict(src="state"), dict(pow=3), dict(pow=0), dict(w=INF), dict(c=float("nan")), dict(w=1e39)):
        with pytest.raises(ValueError):
            term(0, **kw)
    with pytest.raises(TypeError):
        term(0.5)
    for args in (([],), ([term(0)] * 5,), ([term(0)], INF)):
        with pytest.raises(ValueError):
            derived(*args)
    with pytest.raises(TypeError):
        derived([dict(col=0)])
    with pytest.raises(ValueError):
        dist_sq((0, 1), (0.0,))
    with pytest.raises(ValueError):
        speed_sq((0, 1, 2, 3, 4))
    q = speed_sq((0, 1))
    with pytest.raises(ValueError):
        TaskRules([], derived=[q] * 9)
    with pytest.raises(TypeError):
        TaskRules([], derived=[term(0)])
    with pytest.raises(TypeError):
        TaskRules([], derived=q)
    for cols in (1, slice(0, 2), -2, slice(1, None)):
        with pytest.raises(ValueError, match="derived quantities"):
            TaskRules([cost(src="derived", cols=cols)], derived=[q])
    with pytest.raises(ValueError, match="derived quantities"):
        TaskRules([healthy(src="derived", cols=0)])
    ok = TaskRules([cost(src="derived", cols=slice(-2, None), any=True, hi=1.0)], derived=[q, q, q])
    assert ok.has_cost and len(ok.derived) == 3 and ok.struct().clause[0].src == 3 and "derived=" in repr(ok)
    with pytest.raises(ValueError):
        q.values(np.zeros((2, 1), F), np.zeros((2, 1), F), np.zeros((2, 1), F))           # column 1 outside width 1
    with pytest.raises(ValueError):
        ok.clauses[0].values(np.zeros((2, 3)), np.zeros((2, 1)), np.zeros((2, 3)))        # no derived values given


def _post(lib, task, obs_dim, act_dim, act=None):
    return lib.cmbpo_fakeenv_post(task, 7, obs_dim, act_dim, None, None, 0, None, act, None, None, None, 0,
                                  None, None, None, None, None, None, None, None)


def test_launch_time_checks_without_a_gpu(lib):
    """Validation precedes any HIP call: with NULL buffers every call returns -1 and the message names the check."""
    from cmbpo_amd import _lib
    from cmbpo_amd.statics import TaskRules, cost, derived, term
    L = _lib.TASK_LEARNED_COST
    rules = TaskRules([cost(src="derived", cols=slice(0, None), any=True, hi=1.0)],
                      derived=[derived([term(20), term(-21, src="obs")]), derived([term(0), term(-3, src="act", pow=2)])])
    tid = rules.task_id
    dummy = (C.c_float * 8)()
    err = lib.cmbpo_last_error
    for task in (tid, tid | L):
        assert _post(lib, task, 20, 8, dummy) == -1 and b"derived 0: term 0" in err() and b"next_obs's width 20" in err()
        assert _post(lib, task, 21, 2, dummy) == -1 and b"derived 1: term 1" in err() and b"act's width 2" in err()
        assert _post(lib, task, 21, 8, None) == -1 and b"derived 1: term 1 reads act, d_act is NULL" in err()
        assert _post(lib, task, 21, 8, dummy) == -1 and b"NULL buffer" in err()          # the rules' own checks passed
        assert err().startswith(b"cmbpo_fakeenv_post:")
    # a derived index at or above n_derived cannot be registered ...
    s, d = rules.struct(), rules.derived_struct()
    s.clause[0].col0 = 2
    out = C.c_int(-5)
    assert lib.cmbpo_task_rules_register_ex(C.byref(s), C.byref(d), C.byref(out)) == -1 and out.value == -5
    assert re.search(rb"clause 0: indices \(col0 2, n_cols -1\) outside the 2 derived quantities", err())
    s.clause[0].col0, s.clause[0].n_cols = 1, 2
    assert lib.cmbpo_task_rules_register_ex(C.byref(s), C.byref(d), C.byref(out)) == -1 and b"derived" in err()
    # ... and the other entry points of the post step go through the same checks, in the same words
    args = [tid, 7, 20, 8, None, None, 0, None, dummy, None, None, None, 0] + [None] * 7      # the 20 shared parameters
    assert lib.cmbpo_fakeenv_post_noise(*args, None, None) == -1 and b"derived 0: term 0" in err()
    assert lib.cmbpo_fakeenv_post_cost(*args, None, 0.0, 0.0, None, None, None, None, None) == -1 and b"derived 0: term 0" in err()
