"""CPU: the learned termination head without a GPU -- the C-ABI (struct image, exports, every refusal by name with NULL buffers,
th == NULL forwarding to the existing entry points), the training target of the column (a time-out is target 0, a termination
before the sampler's horizon target 1, the column order), and the NumPy specification itself on NaN, infinities and values at,
one ulp above and one ulp below the threshold."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import term_head_ref as ref
from toyworld import StubPolicy, ToyEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = b"cmbpo_fakeenv_post_term"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cmbpo_amd import _lib
    return _lib.lib()


def _header():
    text = open(os.path.join(ROOT, "include", "cmbpo_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _head(threshold=0.5, members=0):
    from cmbpo_amd import _lib
    th = _lib.TermHeadStruct()
    th.threshold, th.members, th.term_pred, th.term_votes = threshold, members, None, None
    return th


def _post(lib, task, ensemble, obs_dim, act_dim, th, n_rows=0, ld_rows=0, buffers=False, kr=0.0, kc=0.0, dis=False):
    """cmbpo_fakeenv_post_term on host memory that is never dereferenced: every call fails a check or has no rows."""
    host = (C.c_float * 64)()
    p = C.cast(host, C.c_void_p) if buffers else None
    v = C.cast(host, C.c_void_p) if dis else None
    return lib.cmbpo_fakeenv_post_term(task, ensemble, obs_dim, act_dim, p, p, ld_rows, p, None, p, None, None, n_rows, p, p, p, p, p, p,
                                       None, None, kr, kc, v, v, None if th is None else C.byref(th), None)


# ------------------------------------------------------------------------------------------------------------------
# the C-ABI
# ------------------------------------------------------------------------------------------------------------------
def test_struct_image_and_signatures(lib):
    from cmbpo_amd import _lib
    S = _lib.TermHeadStruct
    assert C.sizeof(S) == 24
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("threshold", 0), ("members", 4), ("term_pred", 8), ("term_votes", 16)]
    assert [t for _, t in S._fields_] == [C.c_float, C.c_int32, C.c_void_p, C.c_void_p]
    text = _header()
    m = re.search(r"typedef struct cmbpo_term_head \{(.*?)\} cmbpo_term_head_t;", text, flags=re.S)
    assert m and [d.strip() for d in m.group(1).split(";") if d.strip()] == [
        "float threshold", "int32_t members", "float *term_pred", "uint8_t *term_votes"]
    assert (_lib.TERM_ELITE, _lib.TERM_ANY, _lib.TERM_MAJORITY) == (0, 1, 2) == (ref.ELITE, ref.ANY, ref.MAJORITY)
    for name, val in (("ELITE", 0), ("ANY", 1), ("MAJORITY", 2)):
        assert re.search(r"#define CMBPO_TERM_%s %d\b" % (name, val), text)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("cmbpo_fakeenv_post_term", "cmbpo_rollout_term_head_attach", "cmbpo_rollout_term_head_detach", "cmbpo_replay_run_term"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    # cmbpo_fakeenv_post_disagreement's arguments, then the head, then the stream
    dis, term = _lib.SIGNATURES["cmbpo_fakeenv_post_disagreement"], _lib.SIGNATURES["cmbpo_fakeenv_post_term"]
    assert term[0] is C.c_int and term[1] == dis[1][:-1] + [C.POINTER(S), C.c_void_p]
    args = [a.strip() for a in re.search(r"int cmbpo_fakeenv_post_term\((.*?)\);", text, flags=re.S).group(1).split(",")]
    assert len(args) == len(term[1]) and args[-2:] == ["const cmbpo_term_head_t *th", "void *stream"]
    # the frozen structs are what they were
    assert C.sizeof(_lib.RolloutStruct) == 440 and C.sizeof(_lib.ReplayStruct) == 184 and C.sizeof(_lib.TaskRulesStruct) == 528
    assert lib.cmbpo_version() == 6


def test_refusals_name_the_field_before_any_hip_call(lib):
    from cmbpo_amd import _lib
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert _post(lib, _lib.TASK_ANTSAFE, 7, 29, 8, _head(bad, 0)) == -1
        msg = lib.cmbpo_last_error()
        assert WHO in msg and b"threshold" in msg and b"termination head" in msg, msg
    for bad in (-1, 3, 17):
        assert _post(lib, _lib.TASK_HCS, 5, 18, 6, _head(0.5, bad)) == -1
        msg = lib.cmbpo_last_error()
        assert WHO in msg and b"members" in msg, msg
    for E in (9, 16, 1):
        assert _post(lib, _lib.TASK_DEFAULT, E, 11, 3, _head()) == -1
        msg = lib.cmbpo_last_error()
        assert WHO in msg and b"ensemble" in msg, msg
    # the checks the entry shares with the others keep their words, under this entry's name
    assert _post(lib, 0x200 | _lib.TASK_ANTSAFE, 7, 29, 8, _head()) == -1
    assert WHO in lib.cmbpo_last_error() and b"bad task" in lib.cmbpo_last_error()
    assert _post(lib, _lib.TASK_ANTSAFE, 7, 29, 8, _head()) == -1
    assert WHO in lib.cmbpo_last_error() and b"NULL buffer" in lib.cmbpo_last_error()
    assert _post(lib, _lib.TASK_HCS, 7, 18, 6, _head(), kc=0.5, dis=True, buffers=True) == -1
    assert WHO in lib.cmbpo_last_error() and b"kappa_cost" in lib.cmbpo_last_error()
    # a good head on no rows: nothing is launched, every mode
    for members in (0, 1, 2):
        for dis in (False, True):
            assert _post(lib, _lib.TASK_ANTSAFE | _lib.TASK_LEARNED_COST, 7, 29, 8, _head(-0.25, members), buffers=True, dis=dis) == 0


def test_null_head_forwards_to_the_existing_entry_points(lib):
    from cmbpo_amd import _lib
    assert _post(lib, 9, 7, 29, 8, None) == -1
    msg = lib.cmbpo_last_error()
    assert msg.startswith(b"cmbpo_fakeenv_post:") and b"bad task" in msg, msg
    assert _post(lib, 9, 7, 29, 8, None, dis=True) == -1
    assert lib.cmbpo_last_error().startswith(b"cmbpo_fakeenv_post_disagreement:")
    assert _post(lib, _lib.TASK_HCS, 7, 18, 6, None, kr=-1.0, buffers=True) == -1
    msg = lib.cmbpo_last_error()
    assert msg.startswith(b"cmbpo_fakeenv_post_disagreement:") and b"kappa_rew" in msg, msg
    assert _post(lib, _lib.TASK_HCS, 7, 18, 6, None, buffers=True) == 0


# ---- the naming rule: a message carries the name of the narrowest entry point that can express the call --------------------------
# every post entry point x every subset of {xi, disagreement arguments, head} it can express
_POST_CASES = [("cmbpo_fakeenv_post", False, False, False)]
_POST_CASES += [("cmbpo_fakeenv_post_noise", xi, False, False) for xi in (False, True)]
_POST_CASES += [("cmbpo_fakeenv_post_disagreement", xi, dis, False) for xi in (False, True) for dis in (False, True)]
_POST_CASES += [("cmbpo_fakeenv_post_term", xi, dis, th) for xi in (False, True) for dis in (False, True) for th in (False, True)]


def _post_entry(lib, entry, xi, dis, th, task, n_rows=0):
    """One call of `entry` on host memory that is never dereferenced; returns (rc, the name the rule gives)."""
    host = (C.c_float * 64)()
    p = C.cast(host, C.c_void_p)
    args = [task, 7, 18, 6, p, p, n_rows, p, p, p, None, None, n_rows, p, p, p, p, p, p, None]
    if entry != "cmbpo_fakeenv_post":
        args.append(p if xi else None)
    if entry in ("cmbpo_fakeenv_post_disagreement", "cmbpo_fakeenv_post_term"):
        args += [0.5, 0.25, p, p] if dis else [0.0, 0.0, None, None]
    head = _head(0.5, 2)
    if entry == "cmbpo_fakeenv_post_term":
        args.append(C.byref(head) if th else None)
    dis_on = dis or entry == "cmbpo_fakeenv_post_disagreement"        # that entry is the feature: always on
    want = ("cmbpo_fakeenv_post_term" if th else "cmbpo_fakeenv_post_disagreement" if dis_on
            else "cmbpo_fakeenv_post_noise" if xi else "cmbpo_fakeenv_post")
    return getattr(lib, entry)(*args, None), want.encode()


@pytest.mark.parametrize("entry,xi,dis,th", _POST_CASES)
def test_post_messages_carry_the_name_the_rule_gives(lib, entry, xi, dis, th):
    rc, want = _post_entry(lib, entry, xi, dis, th, task=9)
    msg = lib.cmbpo_last_error()
    assert rc == -1 and msg.startswith(want + b": bad task 9"), msg


@pytest.mark.parametrize("entry,xi,dis,th", _POST_CASES)
def test_post_of_no_rows_launches_nothing(lib, entry, xi, dis, th):
    """Good arguments and n_rows == 0 return before the launch (there is no device here to launch on)."""
    from cmbpo_amd import _lib
    rc, want = _post_entry(lib, entry, xi, dis, th, task=_lib.TASK_HCS | _lib.TASK_LEARNED_COST)
    if entry == "cmbpo_fakeenv_post_disagreement" and not dis:      # on without its buffers: refused under its own name
        assert rc == -1 and lib.cmbpo_last_error().startswith(want + b": NULL buffer (d_rew_var / d_cost_var)")
    else:
        assert rc == 0, lib.cmbpo_last_error()


@pytest.mark.parametrize("entry,rc_given,th_given,want", [
    ("cmbpo_replay_run", False, False, b"cmbpo_replay_run"),
    ("cmbpo_replay_run_calibrated", True, False, b"cmbpo_replay_run_calibrated"),
    ("cmbpo_replay_run_calibrated", False, False, b"cmbpo_replay_run_calibrated"),     # its rc == NULL is its own error
    ("cmbpo_replay_run_term", False, False, b"cmbpo_replay_run"),
    ("cmbpo_replay_run_term", True, False, b"cmbpo_replay_run_calibrated"),
    ("cmbpo_replay_run_term", False, True, b"cmbpo_replay_run_term"),
    ("cmbpo_replay_run_term", True, True, b"cmbpo_replay_run_term")])
def test_replay_messages_carry_the_name_the_rule_gives(lib, entry, rc_given, th_given, want):
    from cmbpo_amd import _lib
    rp, cal, head = _lib.ReplayStruct(), _lib.ReplayCalibStruct(), _head()      # all-zero descriptors: the first check fails
    rc = C.byref(cal) if rc_given else None
    th = C.byref(head) if th_given else None
    if entry == "cmbpo_replay_run":
        got = lib.cmbpo_replay_run(C.byref(rp), None, 0, 7, None, None)
    elif entry == "cmbpo_replay_run_calibrated":
        got = lib.cmbpo_replay_run_calibrated(C.byref(rp), rc, None, 0, 7, None)
    else:
        got = lib.cmbpo_replay_run_term(C.byref(rp), rc, th, None, 0, 7, None, None)
    msg = lib.cmbpo_last_error()
    assert got == -1 and msg.startswith(want + b": B 0 < 1"), msg


def test_rollout_attach_and_replay_refusals(lib):
    from cmbpo_amd import _lib
    rs = _lib.RolloutStruct()
    key = (C.c_int32 * 32)()
    assert lib.cmbpo_rollout_term_head_attach(C.byref(rs), C.byref(_head())) == -1          # no iscal: no key
    assert b"cmbpo_rollout_term_head_attach" in lib.cmbpo_last_error()
    rs.iscal = C.cast(key, C.c_void_p)
    assert lib.cmbpo_rollout_term_head_attach(C.byref(rs), None) == -1
    assert lib.cmbpo_rollout_term_head_attach(C.byref(rs), C.byref(_head(float("nan")))) == -1
    assert b"threshold" in lib.cmbpo_last_error()
    assert lib.cmbpo_rollout_term_head_attach(C.byref(rs), C.byref(_head(0.5, 3))) == -1
    assert b"members" in lib.cmbpo_last_error()
    assert lib.cmbpo_rollout_term_head_detach(C.byref(rs)) == 0                              # nothing attached: no error
    assert lib.cmbpo_rollout_term_head_attach(C.byref(rs), C.byref(_head(0.0, 0))) == 0      # an all-zero head is a head
    assert lib.cmbpo_rollout_term_head_attach(C.byref(rs), C.byref(_head(0.7, 2))) == 0      # replaces it
    assert lib.cmbpo_rollout_term_head_detach(C.byref(rs)) == 0
    assert lib.cmbpo_rollout_term_head_detach(None) == -1
    # the replay: its own descriptor checks come first, under its name; th == NULL is the existing entry
    rp = _lib.ReplayStruct()
    assert lib.cmbpo_replay_run_term(C.byref(rp), None, C.byref(_head()), None, 0, 7, None, None) == -1
    assert b"cmbpo_replay_run_term" in lib.cmbpo_last_error()
    assert lib.cmbpo_replay_run_term(C.byref(rp), None, None, None, 0, 7, None, None) == -1
    assert lib.cmbpo_last_error().startswith(b"cmbpo_replay_run:")


def test_pinned_refusals_stay(lib):
    """The head is not a task bit and not a clause source."""
    from cmbpo_amd import _lib
    assert lib.cmbpo_fakeenv_post(0x200 | _lib.TASK_ANTSAFE, 7, 29, 8, None, None, 0, None, None, None, None, None, 0,
                                  None, None, None, None, None, None, None, None) == -1
    assert b"bad task" in lib.cmbpo_last_error()
    for field, val in (("src", 3), ("flags", 16)):
        tr = _lib.TaskRulesStruct()
        tr.n_clauses = 1
        tr.clause[0].n_cols, tr.clause[0].scale = 1, 1.0
        setattr(tr.clause[0], field, val)
        assert lib.cmbpo_task_rules_register(C.byref(tr), C.byref(C.c_int(0))) == -1, field
    tr = _lib.TaskRulesStruct()
    tr.reserved = 1
    assert lib.cmbpo_task_rules_register(C.byref(tr), C.byref(C.c_int(0))) == -1


# ------------------------------------------------------------------------------------------------------------------
# the training target
# ------------------------------------------------------------------------------------------------------------------
class _HostBuffer:
    """CPOBuffer whose finish_path keeps the path bookkeeping and skips the advantage kernels (no GPU here)."""

    def __new__(cls, *a, **k):
        from cmbpo_amd.cpobuffer import CPOBuffer

        class HostBuffer(CPOBuffer):
            def finish_path(self, last_val=0, last_cval=0):
                self.path_start_idx, self.path_finished = self.ptr, True

        return HostBuffer(*a, **k)


def _archive(max_path_length, lengths=(6,), steps=20):
    """`steps` real steps of the toy environment, which sets `done` at its own time limit `lengths`, into an archive."""
    from cmbpo_amd.cpo_sampler import CpoSampler
    env, pol = ToyEnv(lengths=lengths), StubPolicy()
    buf = _HostBuffer(64, 256, env.observation_space, env.action_space, device="cpu")
    buf.initialize({"mu": (ToyEnv.A,), "log_std": (ToyEnv.A,)})
    s = CpoSampler(max_path_length=max_path_length)
    s.initialize(env, pol, buf)
    for t in range(steps):
        s.sample(timestep=0)
    s.finish_all_paths(append_val=True, append_cval=True, reset_path=False)
    buf.dump_to_archive()
    return buf


def test_a_time_out_is_target_zero_and_an_early_end_target_one():
    from cmbpo_amd.cmbpo import format_samples_for_dyn
    fields = ["observations", "actions", "next_observations", "rewards", "costs", "terminals", "path_lengths"]
    col = {}
    for horizon in (6, 10):       # the environment ends every episode at its own limit of 6 steps and reports done there
        buf = _archive(horizon)
        a = buf.get_archive(fields)
        np.testing.assert_array_equal(np.flatnonzero(a["terminals"]), [5, 11, 17])      # what the archive holds does not change
        np.testing.assert_array_equal(a["path_lengths"], [6] * 18 + [2] * 2)
        ins, outs = format_samples_for_dyn(a, append_r=True, append_c=False, append_t=True, horizon=horizon)
        assert ins.shape == (20, ToyEnv.D + ToyEnv.A) and outs.shape == (20, ToyEnv.D + 2)
        col[horizon] = outs[:, -1]
        np.testing.assert_array_equal(buf.term_targets(horizon)[:20], outs[:, -1])
        # the specification's restatement, path by path
        want = np.concatenate([ref.term_targets(a["terminals"][lo:hi], hi - lo, horizon) for lo, hi in ((0, 6), (6, 12), (12, 18), (18, 20))])
        np.testing.assert_array_equal(outs[:, -1], want)
    assert not col[6].any()                                              # the same paths, ended by the sampler's time-out
    np.testing.assert_array_equal(np.flatnonzero(col[10]), [5, 11, 17])   # ... and before its horizon
    # a mixture: episodes of 3 and of 8 steps under a horizon of 8
    buf = _archive(8, lengths=(3, 8), steps=22)
    np.testing.assert_array_equal(np.flatnonzero(buf.term_targets(8)), [2, 13])
    np.testing.assert_array_equal(np.flatnonzero(buf.arch_dict["terminals"]), [2, 10, 13, 21])


def test_column_order_with_and_without_the_cost_column():
    from cmbpo_amd.cmbpo import format_samples_for_dyn
    buf = _archive(10)
    a = buf.get_archive(["observations", "actions", "next_observations", "rewards", "costs", "terminals", "path_lengths"])
    D = ToyEnv.D
    delta = a["next_observations"] - a["observations"]
    t = (a["terminals"] & (a["path_lengths"] < 10)).astype(np.float32)
    assert t.sum() == 3 and a["costs"].any()
    _, o = format_samples_for_dyn(a, append_t=True, horizon=10)
    np.testing.assert_array_equal(o, np.concatenate([delta, a["rewards"][:, None], t[:, None]], axis=1))
    _, o = format_samples_for_dyn(a, append_c=True, append_t=True, horizon=10)
    np.testing.assert_array_equal(o, np.concatenate([delta, a["rewards"][:, None], a["costs"][:, None], t[:, None]], axis=1))
    assert o.shape[1] == ref.term_column(D, True) + 1 and o.dtype == np.float32
    # off: what it always returned, and no new key is needed
    base = {k: v for k, v in a.items() if k != "path_lengths"}
    _, o = format_samples_for_dyn(base, append_c=True)
    np.testing.assert_array_equal(o, np.concatenate([delta, a["rewards"][:, None], a["costs"][:, None]], axis=1))
    with pytest.raises(ValueError, match="path_lengths"):
        format_samples_for_dyn(base, append_t=True, horizon=10)
    with pytest.raises(ValueError, match="horizon"):
        format_samples_for_dyn(a, append_t=True)


def test_a_path_cut_by_the_wrapped_archive_has_no_known_length():
    buf = _archive(10, steps=20)
    buf.archive_full, buf.archive_ptr = True, 8           # as after a wrap: slots 0..7 are the newest samples
    ln = buf.path_lengths()
    big = np.iinfo(np.int32).max
    np.testing.assert_array_equal(ln[:20], [6] * 6 + [2] * 2 + [big] * 4 + [6] * 6 + [2] * 2)
    np.testing.assert_array_equal(np.flatnonzero(buf.term_targets(10)), [5, 17])


# ------------------------------------------------------------------------------------------------------------------
# the specification itself
# ------------------------------------------------------------------------------------------------------------------
def test_reference_on_nan_infinities_and_the_threshold_itself():
    thr = np.float32(0.5)
    up, dn = np.nextafter(thr, np.float32(1)), np.nextafter(thr, np.float32(0))
    E, D = 3, 2
    # rows: all NaN | elite NaN, others above | elite +inf | elite -inf, one above | all at thr | elite one ulp above | one ulp below
    cols = np.array([[np.nan, np.nan, np.nan], [np.nan, 0.9, 0.8], [np.inf, 0.0, 0.0], [-np.inf, 0.9, 0.1], [thr, thr, thr],
                     [up, thr, dn], [dn, up, up]], np.float32).T                     # [E, n]
    n = cols.shape[1]
    mean = np.zeros((E, n, D + 2), np.float32)
    mean[:, :, D + 1] = cols
    inds = np.zeros(n, np.int32)
    want_votes = [0, 2, 1, 1, 0, 1, 2]
    want = {ref.ELITE: [0, 0, 1, 0, 0, 1, 0], ref.ANY: [0, 1, 1, 1, 0, 1, 1], ref.MAJORITY: [0, 1, 0, 0, 0, 0, 1]}
    for members, name in ((ref.ELITE, "elite"), (ref.ANY, "any"), (ref.MAJORITY, "majority")):
        term, pred, votes, learned = ref.term_head(mean, inds, D, False, thr, name)
        np.testing.assert_array_equal(term, want[members])
        np.testing.assert_array_equal(votes, want_votes)
        assert term.dtype == np.uint8 and votes.dtype == np.uint8 and pred.dtype == np.float32
        np.testing.assert_array_equal(pred.view(np.uint32), cols[0].view(np.uint32))      # the elite's value as it is, NaN included
        np.testing.assert_array_equal(learned, np.asarray(want[members], bool))
        # the rule's verdict is or-ed in; rows are picked like the kernel's row list
        rule = np.array([1, 0, 0, 0, 1, 0, 0], bool)
        np.testing.assert_array_equal(ref.term_head(mean, inds, D, False, thr, members, rule_done=rule)[0], rule | np.asarray(want[members], bool))
        rows = np.array([6, 2, 3])
        np.testing.assert_array_equal(ref.term_head(mean, inds, D, False, thr, members, rows=rows)[0], np.asarray(want[members])[rows])
    # MAJORITY is strict: 2 of 4 is no majority, 3 of 5 is one
    for E2, k, w in ((4, 2, 0), (4, 3, 1), (5, 2, 0), (5, 3, 1), (7, 4, 1), (2, 1, 0)):
        m = np.zeros((E2, 1, 2), np.float32)
        m[:k, 0, 1] = 1.0
        assert ref.term_head(m, [E2 - 1], 0, False, 0.5, "majority")[0][0] == w
    # another elite, the learned-cost column in front of the head's
    m = np.zeros((3, 2, D + 3), np.float32)
    m[:, :, D + 1] = 9.0                     # the cost column: not the head's business
    m[2, 1, D + 2] = 0.75
    term, pred, votes, _ = ref.term_head(m, [2, 2], D, True, 0.5, "elite")
    np.testing.assert_array_equal(term, [0, 1])
    np.testing.assert_array_equal(pred, np.array([0.0, 0.75], np.float32))
    with pytest.raises(AssertionError):
        ref.term_head(m, [2, 2], D, False, 0.5, "elite")          # the column must be the last one
