"""CPU: the ensemble-voted static rules without a GPU -- the NumPy specification against the existing CPU oracle on
the golden FakeEnv fixtures ('elite' is the oracle bit for bit, the votes are the sum of per-member oracle calls), the C-ABI
(struct image, exports, every refusal by name with buffers that are never dereferenced), and the FakeEnv / CMBPO arguments."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rule_votes_ref as ref
from oracle import refcpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
WHO = b"cmbpo_fakeenv_post_votes"
TASKS = {"ant": "AntSafe-v2", "hcs": "HalfCheetahSafe-v2", "default": "default"}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cmbpo_amd import _lib
    return _lib.lib()


def _bits(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def _cases():
    for E in (3, 5, 7):
        g = np.load(os.path.join(GOLD, f"g16_step_e{E}.npz"), allow_pickle=False)
        for D in (int(d) for d in g["dims"]):
            for short, task in TASKS.items():
                if f"d{D}_{short}_terms" in g.files:
                    yield E, D, short, task, g


# ------------------------------------------------------------------------------------------------------------------
# the specification against the oracle
# ------------------------------------------------------------------------------------------------------------------
def test_elite_mode_is_the_oracle_on_the_golden_steps_bit_for_bit():
    seen = set()
    for E, D, short, task, g in _cases():
        obs, act, mean, var, inds = (g[f"d{D}_{k}"] for k in ("obs", "act", "mean", "var", "inds"))
        nxt, _, terms, info = refcpu.fake_env_step(obs, act, mean, var, inds, task)
        out = ref.rule_votes(task, obs, act, mean, var, inds, D)
        np.testing.assert_array_equal(_bits(out["nx_elite"]), _bits(nxt), err_msg=f"E{E} d{D} {short} next_obs")
        np.testing.assert_array_equal(out["term"], terms[:, 0].astype(np.uint8), err_msg=f"E{E} d{D} {short} term")
        np.testing.assert_array_equal(_bits(out["cost"]), _bits(np.asarray(info["cost"], np.float32)[:, 0]),
                                      err_msg=f"E{E} d{D} {short} cost")
        # ... and with xi == 1 (the reference's `deterministic=False`: mean + std) the recording of the reference's own step
        rec = ref.rule_votes(task, obs, act, mean, var, inds, D, xi=np.ones_like(obs))
        np.testing.assert_array_equal(_bits(rec["nx_elite"]), _bits(g[f"d{D}_{short}_next_obs"]), err_msg=f"E{E} d{D} {short} xi=1")
        np.testing.assert_array_equal(rec["term"], g[f"d{D}_{short}_terms"][:, 0].astype(np.uint8), err_msg=f"E{E} d{D} {short} xi=1")
        np.testing.assert_array_equal(_bits(rec["cost"]), _bits(np.asarray(g[f"d{D}_{short}_cost"], np.float32)[:, 0]),
                                      err_msg=f"E{E} d{D} {short} xi=1 cost")
        seen.add(short)
    assert seen == set(TASKS)


def test_votes_are_the_sum_of_per_member_oracle_calls():
    for E, D, short, task, g in _cases():
        obs, act, mean, var, inds = (g[f"d{D}_{k}"] for k in ("obs", "act", "mean", "var", "inds"))
        n = obs.shape[0]
        dv, cv = np.zeros(n, int), np.zeros(n, int)
        for e in range(E):
            _, _, terms, info = refcpu.fake_env_step(obs, act, mean, var, np.full(n, e, np.int32), task)
            dv += terms[:, 0]
            cv += np.asarray(info["cost"])[:, 0] > 0
        for dm in ("elite", "any", "majority"):
            for cm in ("elite", "any", "majority", "mean"):
                out = ref.rule_votes(task, obs, act, mean, var, inds, D, dm, cm)
                np.testing.assert_array_equal(out["done_votes"], dv)
                np.testing.assert_array_equal(out["cost_votes"], cv)
                if dm == "any":
                    np.testing.assert_array_equal(out["term"], dv > 0)
                if dm == "majority":
                    np.testing.assert_array_equal(out["term"], 2 * dv > E)
                want = {"any": (cv > 0), "majority": (2 * cv > E)}.get(cm)
                if want is not None:
                    np.testing.assert_array_equal(_bits(out["cost"]), _bits(want.astype(np.float32)))
                if cm == "mean":
                    np.testing.assert_array_equal(_bits(out["cost"]), _bits(cv.astype(np.float32) / np.float32(E)))


def test_variance_pessimism_and_learned_done_of_the_specification():
    import disagreement_ref as dref
    E, D, short, task, g = next(c for c in _cases() if c[0] == 7 and c[1] == 8 and c[2] == "ant")
    obs, act, mean, var, inds = (g[f"d{D}_{k}"] for k in ("obs", "act", "mean", "var", "inds"))
    rng = np.random.default_rng(0)
    mean = mean.copy()
    mean[:, :, 0] += (rng.standard_normal(mean.shape[:2]) * 0.5).astype(np.float32)       # the members disagree on the height
    xi = rng.standard_normal(obs.shape).astype(np.float32)
    base = ref.rule_votes(task, obs, act, mean, var, inds, D, xi=xi, dis_on=True)
    mixed = (base["cost_votes"] > 0) & (base["cost_votes"] < E)
    assert mixed.any()
    np.testing.assert_array_equal(_bits(base["cost_var"]), _bits(dref.member_var_loop(base["cost_e"].astype(np.float32))))
    assert (base["cost_var"][mixed] > 0).all() and (base["cost_var"][~mixed] == 0).all()
    pen = ref.rule_votes(task, obs, act, mean, var, inds, D, cost_members="mean", xi=xi, dis_on=True, kappa_cost=0.7)
    assert (pen["cost"] <= 1.0).all() and (pen["cost"][mixed] > (base["cost_votes"][mixed] / np.float32(E))).all()
    learned = rng.random(obs.shape[0]) < 0.3
    on = ref.rule_votes(task, obs, act, mean, var, inds, D, "majority", learned_done=learned)
    np.testing.assert_array_equal(on["term"], (2 * on["done_votes"].astype(int) > E) | learned)
    lc = ref.rule_votes(task, obs, act, mean, var, inds, D, "any", learned_cost=True)
    assert lc["cost"] is None and lc["cost_votes"] is None and lc["done_votes"].max() > 0


# ------------------------------------------------------------------------------------------------------------------
# the C-ABI
# ------------------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "cmbpo_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _votes(done=0, cost=0, done_votes=None, cost_votes=None):
    from cmbpo_amd import _lib
    rv = _lib.RuleVotesStruct()
    rv.done_members, rv.cost_members, rv.done_votes, rv.cost_votes = done, cost, done_votes, cost_votes
    return rv


def _head(members=0, outputs=False):
    from cmbpo_amd import _lib
    th = _lib.TermHeadStruct()
    host = (C.c_float * 64)()
    p = C.cast(host, C.c_void_p) if outputs else None
    th.threshold, th.members, th.term_pred, th.term_votes = 0.5, members, p, p
    th._keep = host
    return th


def _post(lib, task, ensemble, obs_dim, act_dim, rv, th=None, n_rows=0, buffers=False, kc=0.0, dis=False, thr=False):
    """cmbpo_fakeenv_post_votes on host memory that is never dereferenced: every call fails a check or has no rows."""
    host = (C.c_float * 64)()
    p = C.cast(host, C.c_void_p) if buffers else None
    v = C.cast(host, C.c_void_p) if dis else None
    return lib.cmbpo_fakeenv_post_votes(task, ensemble, obs_dim, act_dim, p, p, n_rows, p, None, p, None, None, n_rows, p, p, p, p, p, p,
                                        None, None, 0.0, kc, v, v, None if th is None else C.byref(th), None,
                                        C.cast(host, C.c_void_p) if thr else None, None if rv is None else C.byref(rv), None)


def test_struct_image_and_signatures(lib):
    from cmbpo_amd import _lib
    S = _lib.RuleVotesStruct
    assert C.sizeof(S) == 24
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("done_members", 0), ("cost_members", 4), ("done_votes", 8),
                                                                  ("cost_votes", 16)]
    text = _header()
    m = re.search(r"typedef struct cmbpo_rule_votes \{(.*?)\} cmbpo_rule_votes_t;", text, flags=re.S)
    assert m and [d.strip() for d in m.group(1).split(";") if d.strip()] == [
        "int32_t done_members", "int32_t cost_members", "uint8_t *done_votes", "uint8_t *cost_votes"]
    assert re.search(r"#define CMBPO_VOTE_MEAN 3\b", text) and _lib.VOTE_MEAN == 3 == ref.MEAN
    assert _lib.RULE_COST_MEMBERS == dict(elite=0, any=1, majority=2, mean=3) == ref.MODES
    assert _lib.RULE_DONE_MEMBERS == dict(elite=0, any=1, majority=2)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("cmbpo_fakeenv_post_votes", "cmbpo_rollout_rule_votes_attach", "cmbpo_rollout_rule_votes_detach"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    # cmbpo_fakeenv_post_term_draws's arguments, then the votes, then the stream
    draws, votes = _lib.SIGNATURES["cmbpo_fakeenv_post_term_draws"], _lib.SIGNATURES["cmbpo_fakeenv_post_votes"]
    assert votes[0] is C.c_int and votes[1] == draws[1][:-1] + [C.POINTER(S), C.c_void_p]
    args = [a.strip() for a in re.search(r"int cmbpo_fakeenv_post_votes\((.*?)\);", text, flags=re.S).group(1).split(",")]
    assert len(args) == len(votes[1]) and args[-2:] == ["const cmbpo_rule_votes_t *rv", "void *stream"]
    assert C.sizeof(_lib.RolloutStruct) == 440          # the frozen struct is what it was


def test_refusals_name_the_votes_before_any_hip_call(lib):
    from cmbpo_amd import _lib
    ANT, HCS, LC = _lib.TASK_ANTSAFE, _lib.TASK_HCS, _lib.TASK_LEARNED_COST
    fake = C.c_void_p(0x1000)      # a pointer that is compared with NULL and never followed
    for bad in (-1, 3, 17):        # CMBPO_VOTE_MEAN is for the cost only
        assert _post(lib, ANT, 7, 29, 8, _votes(done=bad)) == -1
        msg = lib.cmbpo_last_error()
        assert msg.startswith(WHO) and b"rule votes" in msg and b"done_members" in msg, msg
    for bad in (-1, 4, 17):
        assert _post(lib, ANT, 7, 29, 8, _votes(cost=bad)) == -1
        msg = lib.cmbpo_last_error()
        assert msg.startswith(WHO) and b"rule votes" in msg and b"cost_members" in msg, msg
    for E in (9, 16, 1):
        assert _post(lib, ANT, E, 29, 8, _votes()) == -1
        msg = lib.cmbpo_last_error()
        assert msg.startswith(WHO) and b"ensemble" in msg, msg
    # the learned cost: the static cost rule is skipped, there is nothing to vote on or to count
    for cm in (1, 2, 3):
        assert _post(lib, ANT | LC, 7, 29, 8, _votes(cost=cm), buffers=True) == -1
        msg = lib.cmbpo_last_error()
        assert msg.startswith(WHO) and b"rule votes" in msg and b"cost_members" in msg and b"CMBPO_TASK_LEARNED_COST" in msg, msg
    assert _post(lib, ANT | LC, 7, 29, 8, _votes(cost_votes=fake), buffers=True) == -1
    msg = lib.cmbpo_last_error()
    assert msg.startswith(WHO) and b"rule votes" in msg and b"cost_votes" in msg and b"CMBPO_TASK_LEARNED_COST" in msg, msg
    # ... while the termination votes stay available with it (no rows: nothing is launched)
    for dm in (0, 1, 2):
        assert _post(lib, ANT | LC, 7, 29, 8, _votes(done=dm, done_votes=fake), buffers=True) == 0, lib.cmbpo_last_error()
    # a termination head must bring both of its outputs
    assert _post(lib, ANT, 7, 29, 8, _votes(done=1), th=_head(1), buffers=True) == -1
    msg = lib.cmbpo_last_error()
    assert msg.startswith(WHO) and b"rule votes" in msg and b"term_pred" in msg and b"term_votes" in msg, msg
    assert _post(lib, ANT, 7, 29, 8, _votes(done=1), th=_head(1, outputs=True), buffers=True, thr=True) == 0, lib.cmbpo_last_error()
    # the checks the entry shares with the others keep their words, under this entry's name
    assert _post(lib, 0x200 | ANT, 7, 29, 8, _votes()) == -1
    assert lib.cmbpo_last_error().startswith(WHO + b": bad task")
    assert _post(lib, ANT, 7, 29, 8, _votes()) == -1
    assert lib.cmbpo_last_error().startswith(WHO + b": NULL buffer")
    assert _post(lib, ANT, 7, 29, 8, _votes(), thr=True, buffers=True) == -1
    assert lib.cmbpo_last_error().startswith(WHO) and b"termination draws" in lib.cmbpo_last_error()
    # kappa_cost > 0 on a static cost: accepted with the votes, refused without them as it always was
    assert _post(lib, HCS, 7, 18, 6, _votes(), kc=0.5, dis=True, buffers=True) == 0, lib.cmbpo_last_error()
    assert _post(lib, HCS, 7, 18, 6, None, kc=0.5, dis=True, buffers=True) == -1
    msg = lib.cmbpo_last_error()
    assert msg.startswith(b"cmbpo_fakeenv_post_disagreement:") and b"kappa_cost" in msg, msg
    # every mode of both verdicts on no rows: nothing is launched
    for dm in (0, 1, 2):
        for cm in (0, 1, 2, 3):
            assert _post(lib, ANT, 7, 29, 8, _votes(dm, cm, fake, fake), buffers=True) == 0, lib.cmbpo_last_error()


def test_null_votes_are_the_draws_entry_by_name(lib):
    """rv == NULL: the message carries the name the rule gives without the votes."""
    from cmbpo_amd import _lib
    assert _post(lib, 9, 7, 29, 8, None) == -1
    assert lib.cmbpo_last_error().startswith(b"cmbpo_fakeenv_post: bad task 9")
    assert _post(lib, 9, 7, 29, 8, None, th=_head()) == -1
    assert lib.cmbpo_last_error().startswith(b"cmbpo_fakeenv_post_term: bad task 9")
    assert _post(lib, 9, 7, 29, 8, None, th=_head(), thr=True) == -1
    assert lib.cmbpo_last_error().startswith(b"cmbpo_fakeenv_post_term_draws: bad task 9")
    assert _post(lib, 9, 7, 29, 8, _votes(), th=_head(), thr=True) == -1
    assert lib.cmbpo_last_error().startswith(WHO + b": bad task 9")
    assert _post(lib, _lib.TASK_HCS, 7, 18, 6, None, buffers=True) == 0


def test_rollout_attach_refusals(lib):
    from cmbpo_amd import _lib
    rs = _lib.RolloutStruct()
    key = (C.c_int32 * 32)()
    who = b"cmbpo_rollout_rule_votes_attach"
    assert lib.cmbpo_rollout_rule_votes_attach(C.byref(rs), C.byref(_votes())) == -1               # no iscal: no key
    assert who in lib.cmbpo_last_error()
    rs.iscal = C.cast(key, C.c_void_p)
    assert lib.cmbpo_rollout_rule_votes_attach(C.byref(rs), C.byref(_votes(done=3))) == -1
    assert lib.cmbpo_last_error().startswith(who) and b"done_members" in lib.cmbpo_last_error()
    assert lib.cmbpo_rollout_rule_votes_attach(C.byref(rs), C.byref(_votes(cost=4))) == -1
    assert lib.cmbpo_last_error().startswith(who) and b"cost_members" in lib.cmbpo_last_error()
    assert lib.cmbpo_rollout_rule_votes_detach(C.byref(rs)) == 0                                   # nothing attached: no error
    assert lib.cmbpo_rollout_rule_votes_attach(C.byref(rs), None) == 0                             # NULL detaches, likewise
    assert lib.cmbpo_rollout_rule_votes_attach(C.byref(rs), C.byref(_votes())) == 0                # an all-zero struct is a vote
    assert lib.cmbpo_rollout_rule_votes_attach(C.byref(rs), C.byref(_votes(2, 3))) == 0            # replaces it
    assert lib.cmbpo_rollout_rule_votes_attach(C.byref(rs), None) == 0
    assert lib.cmbpo_rollout_rule_votes_detach(None) == -1 and lib.cmbpo_rollout_rule_votes_attach(None, None) == -1


# ------------------------------------------------------------------------------------------------------------------
# the host side
# ------------------------------------------------------------------------------------------------------------------
def _fake_env(predicts_cost=False, **kw):
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
    assert (g.static_term_members, g.static_cost_members, g.static_votes) == ("elite", "elite", False)
    assert not g.static_votes_on and g.rule_votes_struct() is None           # the default: the call without the vote kernel
    fe = _fake_env(static_term_members="any", static_cost_members="mean")
    rv = fe.rule_votes_struct()
    assert (rv.done_members, rv.cost_members, rv.done_votes, rv.cost_votes) == (_lib.TERM_ANY, _lib.VOTE_MEAN, None, None)
    m = _fake_env(static_votes=True)
    assert m.static_votes_on and (m.rule_votes_struct().done_members, m.rule_votes_struct().cost_members) == (0, 0)
    with pytest.raises(ValueError, match="static_term_members"):
        _fake_env(static_term_members="mean")                                # the mean is for the cost only
    with pytest.raises(ValueError, match="static_cost_members"):
        _fake_env(static_cost_members="all")
    with pytest.raises(ValueError, match="predicts_cost"):
        _fake_env(predicts_cost=True, static_cost_members="any")
    with pytest.raises(ValueError, match="predicts_cost"):
        _fake_env(predicts_cost=True).set_static_votes(cost_members="mean")
    lc = _fake_env(predicts_cost=True, static_term_members="majority")       # the termination votes stay available
    assert lc.rule_votes_struct(done_votes=None).done_members == _lib.TERM_MAJORITY
    # a pessimistic static cost: with the votes only
    with pytest.raises(ValueError, match="predicts_cost"):
        _fake_env(cost_pessimism=0.5)
    with pytest.raises(ValueError, match="predicts_cost"):
        g.set_pessimism(0.0, 0.5)
    p = _fake_env(cost_pessimism=0.5, static_votes=True)
    assert p.cost_pessimism == 0.5 and p.disagreement
    fe.set_pessimism(0.0, 0.25)
    with pytest.raises(ValueError, match="cost_pessimism"):
        fe.set_static_votes("elite", "elite", False)                         # not while the pessimism acts on the static cost
    assert fe.static_votes_on and fe.static_cost_members == "mean"           # a refusal changes nothing
    fe.set_pessimism(0.0, 0.0)
    fe.set_static_votes("elite", "elite")
    assert not fe.static_votes_on and fe.rule_votes_struct() is None
    fe.set_static_votes(votes=True)                                          # None leaves a setting as it is
    assert (fe.static_term_members, fe.static_cost_members, fe.static_votes) == ("elite", "elite", True)


def test_cmbpo_refusals():
    from cmbpo_amd.cmbpo import CMBPO, _static_votes_args
    assert _static_votes_args(True, False, "elite", "elite", False, 0.0) is False
    assert _static_votes_args(True, False, "elite", "elite", True, 0.5) is True
    assert _static_votes_args(True, False, "any", "elite", False, 0.0) is True
    assert _static_votes_args(True, True, "majority", "elite", False, 0.5) is True
    assert _static_votes_args(False, False, "any", "mean", True, 0.0) is False         # no model: nothing runs
    make = lambda **kw: CMBPO(None, None, None, **kw)
    with pytest.raises(ValueError, match="m_static_term_members"):
        make(m_static_term_members="mean")
    with pytest.raises(ValueError, match="m_static_cost_members"):
        make(m_static_cost_members="most")
    with pytest.raises(ValueError, match="m_learn_cost=False"):
        make(m_learn_cost=True, m_static_cost_members="any")
    with pytest.raises(ValueError, match="m_learn_cost"):
        make(m_cost_pessimism=0.5)                                           # today's refusal, without the votes
    with pytest.raises(ValueError, match="m_learn_cost"):
        make(m_cost_pessimism=0.5, m_static_votes=True, use_model=False)
