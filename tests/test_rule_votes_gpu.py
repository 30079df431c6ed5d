"""GPU: the ensemble-voted static rules -- the vote kernel behind the post kernel against tests/rule_votes_ref.py bit
for bit (uint8 arrays equal, float32 by bits with NaNs matched) and against cmbpo_fakeenv_post_term_draws on everything the votes
do not touch; the votes along imagined rollouts (the one-call step and the native loop).

Shapes, the smallest that reach every branch: B in {1, 13, 1003} (a partial last workgroup, no multiple of 8), E in {3, 5, 7, 8},
AntSafe (27 + 8), HCS, a clause table on 5 observation columns (below 8), a clause table on 29 with derived quantities,
require_finite and cost_on_term, and a table on 300 columns (fewer rows per workgroup); each with and without a row list and a device row count, with and without xi.  The fixtures are
drawn so that the members disagree: asserted below on the reference's output, otherwise the comparisons prove nothing."""
import ctypes as C
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import rule_votes_ref as ref  # noqa: E402
import term_draws_ref as tdref  # noqa: E402

DEV = "cuda:0"
F_OUT = ("next_obs", "rew", "cost", "dkl_path", "ep_var_mean", "ep_var", "rew_var", "cost_var", "term_pred")
U8_OUT = ("term", "term_votes", "done_votes", "cost_votes")
DONE_MODES = ("elite", "any", "majority")
COST_MODES = ("elite", "any", "majority", "mean")
DIMS = {"ant": (27, 8), "hcs": (18, 6), "table5": (5, 2), "table29": (29, 8), "wide": (300, 3)}
HAS_DONE = {"ant": True, "hcs": False, "table5": True, "table29": True, "wide": True}
NAN, INF = np.float32(np.nan), np.float32(np.inf)
_TABLES = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def _task(kind, learned=False):
    """(the `task` argument of the entry points, the task of the reference: a built-in name or the TaskRules)."""
    from cmbpo_amd import _lib
    flag = _lib.TASK_LEARNED_COST if learned else 0
    if kind == "ant":
        return _lib.TASK_ANTSAFE | flag, "AntSafe-v2"
    if kind == "hcs":
        return _lib.TASK_HCS | flag, "HalfCheetahSafe-v2"
    if not _TABLES:          # two registered tables for the module (the slots are a process-wide resource)
        from cmbpo_amd.statics import TaskRules, cost, derived, dist_sq, fatal, healthy, term, tilt
        _TABLES["table5"] = TaskRules([healthy(cols=0, lo=0.2, hi=1.5), fatal(src="act", cols=0, lo=0.95),
                                       fatal(cols=slice(1, 3), abs=True, lo=1.2, any=True),
                                       cost(cols=-1, abs=True, lo=0.4, lo_strict=True), cost(src="obs", cols=1, lo=1.0, lo_strict=True)])
        _TABLES["table29"] = TaskRules(
            [healthy(cols=0, lo=0.2, hi=1.0), healthy(src="derived", cols=0, lo=-0.7),
             cost(src="derived", cols=slice(1, 3), any=True, hi=0.25),
             cost(cols=slice(-2, None), abs=True, lo=3.2, lo_strict=True, any=True), fatal(src="derived", cols=3, lo=2.5)],
            derived=[tilt(2, 3), dist_sq((4, 5), (1.0, -2.0)), dist_sq((4, 5), (3.0, 0.5)),
                     derived([term(6, src="obs"), term(0, src="act", w=0.5), term(7, w=-1.0)], bias=0.1)],
            require_finite=True, cost_on_term=True)
        # 300 observation columns: the vote kernel's image of a row is 8 x 301 floats, so a workgroup takes 2 rows, not 32
        _TABLES["wide"] = TaskRules([healthy(cols=0, lo=0.2, hi=1.0), cost(cols=-1, abs=True, lo=0.4, lo_strict=True),
                                     cost(cols=slice(100, 290), abs=True, lo=1.9, lo_strict=True, any=True)], require_finite=True)
    return _TABLES[kind].task_id | flag, _TABLES[kind]


def _inputs(kind, E, B, rng, extra_cols=0):
    """obs, act, (mean, var)[E, B, D + 1 + extra_cols], elite indices: every column a rule of `kind` tests sits near its
    threshold, and the members' deltas are as wide as the rows' distance from it -- the members disagree by construction."""
    D, A = DIMS[kind]
    O = D + 1 + extra_cols
    f = np.float32
    obs = (rng.standard_normal((B, D)) * 0.5).astype(f)
    act = rng.uniform(-1, 1, (B, A)).astype(f)
    mean = (rng.standard_normal((E, B, O)) * 0.3).astype(f)
    var = np.exp(rng.uniform(-12, -2, (E, B, O))).astype(f)

    def col(c, obs_draw, spread):
        obs[:, c] = obs_draw.astype(f)
        mean[:, :, c] = (rng.standard_normal((E, B)) * spread).astype(f)

    if kind in ("ant", "table5", "table29", "wide"):
        col(0, rng.uniform(0.1, 1.1 if kind != "table5" else 1.6, B), 0.12)            # the height band
    if kind in ("ant", "table29"):
        col(2, rng.standard_normal(B) * 0.5, 0.12)                                      # the quaternion: z_rot / tilt at -0.7
        col(3, rng.standard_normal(B) * 0.5, 0.12)
    if kind == "ant":
        col(D - 1, rng.standard_normal(B) * 3.0, 0.6)                                   # |x| > 3.2
    if kind == "hcs":
        col(D - 1, rng.standard_normal(B) * 0.25, 0.08)                                 # |10 x| < 2
    if kind == "wide":
        col(D - 1, rng.standard_normal(B) * 0.4, 0.12)
    if kind == "table5":
        col(1, rng.standard_normal(B) * 0.7, 0.2)
        col(2, rng.standard_normal(B) * 0.7, 0.2)
        col(4, rng.standard_normal(B) * 0.4, 0.12)
    if kind == "table29":
        centre = np.where(rng.random(B) < 0.5, 0, 1)
        col(4, np.array([1.0, 3.0])[centre] + rng.standard_normal(B) * 0.35, 0.15)      # the two circles of radius 0.5
        col(5, np.array([-2.0, 0.5])[centre] + rng.standard_normal(B) * 0.35, 0.15)
        col(6, rng.standard_normal(B) * 1.5, 0.1)
        col(7, rng.standard_normal(B) * 1.5, 0.3)
        col(D - 2, rng.standard_normal(B) * 2.5, 0.6)
        col(D - 1, rng.standard_normal(B) * 2.5, 0.6)
    inds = rng.integers(0, E, size=B).astype(np.int32)
    return obs, act, mean, var, inds


def _plant(mean, inds, rows, E, D):
    """A NaN or inf in one member's mean: in the elite, in a non-elite member (as many rows as the list has)."""
    oth = lambda r: (inds[r] + 1) % E
    plans = [lambda r: mean.__setitem__((inds[r], r, 1), NAN), lambda r: mean.__setitem__((oth(r), r, 0), INF),
             lambda r: mean.__setitem__((oth(r), r, D - 1), NAN), lambda r: mean.__setitem__((inds[r], r, 0), -INF)]
    for fn, r in zip(plans, rows):
        fn(int(r))


class _Post:
    """The inputs of one post step on the device, uploaded once; run() makes one call of cmbpo_fakeenv_post_votes (or, with
    entry='draws', of cmbpo_fakeenv_post_term_draws with the same leading arguments) into outputs that start at a sentinel."""

    def __init__(self, obs, act, mean, var, inds, rows, D, A, n_dev=None):
        dev = torch.device(DEV)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.B, self.E, self.D, self.A = obs.shape[0], mean.shape[0], D, A
        self.listed = rows is not None
        self.n = len(rows) if self.listed else self.B
        self.d = [t(obs), t(act), t(mean), t(var), t(inds), t(np.asarray(rows, np.int32)) if self.listed else None,
                  None if n_dev is None else t(np.array([n_dev], np.int32))]

    def run(self, task_arg, xi=None, kappa=None, head=None, thr=None, votes=None, entry="votes", expect_rc=0, cost_votes=True):
        from cmbpo_amd import _lib
        dev = torch.device(DEV)
        B, D = self.B, self.D
        f, u8 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.uint8, device=dev)
        out = {k: torch.full((B, D) if k in ("next_obs", "ep_var") else (B,), -7.0, **f) for k in F_OUT}
        out.update({k: torch.full((B,), 77, **u8) for k in U8_OUT})
        keep = [None if xi is None else torch.from_numpy(xi).to(dev), None if thr is None else torch.from_numpy(thr).to(dev)]
        th = None
        if head is not None:
            th = _lib.TermHeadStruct()
            th.threshold, th.members = head[0], tdref.MEMBERS[head[1]]
            th.term_pred, th.term_votes = _lib.ptr(out["term_pred"]), _lib.ptr(out["term_votes"])
        kr, kc = kappa if kappa is not None else (0.0, 0.0)
        d = self.d
        args = [task_arg, self.E, D, self.A, _lib.ptr(d[2]), _lib.ptr(d[3]), B, _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[4]),
                _lib.ptr(d[5]), _lib.ptr(d[6]), self.n, _lib.ptr(out["next_obs"]), _lib.ptr(out["rew"]), _lib.ptr(out["term"]),
                _lib.ptr(out["cost"]), _lib.ptr(out["dkl_path"]), _lib.ptr(out["ep_var_mean"]), _lib.ptr(out["ep_var"]),
                _lib.ptr(keep[0]), float(kr), float(kc), _lib.ptr(out["rew_var"]) if kappa is not None else None,
                _lib.ptr(out["cost_var"]) if kappa is not None else None, None if th is None else C.byref(th), None,
                _lib.ptr(keep[1])]
        if entry == "votes":
            rv = None
            if votes is not None:
                rv = _lib.RuleVotesStruct()
                rv.done_members, rv.cost_members = ref.MODES[votes[0]], ref.MODES[votes[1]]
                rv.done_votes = _lib.ptr(out["done_votes"])
                rv.cost_votes = _lib.ptr(out["cost_votes"]) if cost_votes else None
            rc = _lib.lib().cmbpo_fakeenv_post_votes(*args, None if rv is None else C.byref(rv), _lib.current_stream())
        else:
            assert votes is None
            rc = _lib.lib().cmbpo_fakeenv_post_term_draws(*args, _lib.current_stream())
        torch.cuda.synchronize()
        assert rc == expect_rc, (rc, _lib.lib().cmbpo_last_error())
        return {k: v.cpu().numpy() for k, v in out.items()}


def _same(a, b, keys, msg):
    for k in keys:
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{msg}: {k}")


def _variants(kind, E, B, seed):
    """(post, rows, obs, act, mean, var, inds, xi or None) for B rows: all slots / a scattered list with a device row count (the
    last three listed rows lie behind it and are not stepped), each without and with draws."""
    D, A = DIMS[kind]
    for listed in (False, True):
        rng = np.random.default_rng(zlib.crc32(f"{kind}/{E}/{B}/{listed}/{seed}".encode()))
        slots = B + 11 if listed else B
        obs, act, mean, var, inds = _inputs(kind, E, slots, rng)
        if listed:
            behind = 3 if B > 3 else 0
            listed_rows = rng.permutation(slots)[:B + behind].astype(np.int32)
            rows = listed_rows[:B]
        else:
            listed_rows, rows, behind = None, np.arange(B, dtype=np.int32), 0
        _plant(mean, inds, rows, E, D)
        post = _Post(obs, act, mean, var, inds, listed_rows, D, A, n_dev=B if listed else None)
        xi_draws = rng.standard_normal((slots, D)).astype(np.float32)
        for xi in (None, xi_draws):
            yield post, rows, obs, act, mean, var, inds, xi, f"{kind} E={E} B={B} listed={listed} xi={xi is not None}"


# ------------------------------------------------------------------------------------------------------------------
# 1. the vote kernel behind the post kernel
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [3, 5, 7, 8])
@pytest.mark.parametrize("kind", ["ant", "hcs", "table5", "table29"])
def test_votes_against_the_reference(hip_lib, kind, E):
    """Checks 1 - 3: rv == NULL is cmbpo_fakeenv_post_term_draws's call on every output; the measure-only vote leaves term and
    cost bitwise the plain call's; every mode of both verdicts is the reference's; every other output is the plain call's and
    unlisted slots keep their sentinels."""
    _need_gpu()
    D, A = DIMS[kind]
    for B in (1, 13, 1003):
        for post, rows, obs, act, mean, var, inds, xi, tag in _variants(kind, E, B, "modes"):
            task_arg, task = _task(kind)
            plain = post.run(task_arg, xi, entry="draws")
            null = post.run(task_arg, xi, votes=None)
            _same(null, plain, F_OUT + U8_OUT, f"{tag} rv == NULL")
            rest = np.setdiff1d(np.arange(post.B), rows)
            base = ref.rule_votes(task, obs, act, mean, var, inds, D, rows=rows, xi=xi)
            np.testing.assert_array_equal(_bits(base["nx_elite"]), _bits(plain["next_obs"][rows]), err_msg=f"{tag}: nx_elite")
            if B == 1003:
                # the fixture: on at least 10 % of the rows the members disagree, and every vote changes some row's verdict
                cv, dv = base["cost_votes"], base["done_votes"]
                assert ((cv > 0) & (cv < E)).mean() >= 0.10, (tag, ((cv > 0) & (cv < E)).mean())
                if HAS_DONE[kind]:
                    assert ((dv > 0) & (dv < E)).mean() >= 0.10, (tag, ((dv > 0) & (dv < E)).mean())
            measured = post.run(task_arg, xi, votes=("elite", "elite"))
            _same(measured, plain, F_OUT + ("term", "term_votes"), f"{tag} measure only")
            for dm in DONE_MODES:
                for cm in COST_MODES:
                    if (dm == "elite") != (cm == "elite") and dm != "any" and cm != "mean":
                        continue            # every mode of each verdict, paired; not the whole product
                    want = ref.rule_votes(task, obs, act, mean, var, inds, D, dm, cm, rows=rows, xi=xi)
                    got = post.run(task_arg, xi, votes=(dm, cm))
                    m = f"{tag} {dm}/{cm}"
                    np.testing.assert_array_equal(got["term"][rows], want["term"], err_msg=m + " term")
                    np.testing.assert_array_equal(_bits(got["cost"][rows]), _bits(want["cost"]), err_msg=m + " cost")
                    np.testing.assert_array_equal(got["done_votes"][rows], want["done_votes"], err_msg=m + " done_votes")
                    np.testing.assert_array_equal(got["cost_votes"][rows], want["cost_votes"], err_msg=m + " cost_votes")
                    _same(got, plain, ("next_obs", "rew", "dkl_path", "ep_var_mean", "ep_var", "rew_var", "cost_var", "term_pred",
                                       "term_votes"), m)
                    for k in ("term", "done_votes", "cost_votes"):
                        assert (got[k][rest] == 77).all(), (m, k)
                    assert (got["cost"][rest] == -7.0).all(), m
                    if B == 1003:
                        if dm != "elite" and HAS_DONE[kind]:
                            assert (want["term"] != base["term"]).any(), m
                        if cm != "elite":
                            assert (_bits(want["cost"]) != _bits(base["cost"])).any(), m


@pytest.mark.parametrize("E", [8, 3])
def test_wide_observations_take_fewer_rows_per_workgroup(hip_lib, E):
    """300 observation columns: the image of a workgroup's rows is held under 32 KB by taking fewer rows (2 with eight members, 8
    with three) -- the same checks on that path, with a partial last workgroup, a row list and a device row count, draws, the
    disagreement and a registered table."""
    _need_gpu()
    kind = "wide"
    D, A = DIMS[kind]
    for B in (13, 203):
        for post, rows, obs, act, mean, var, inds, xi, tag in _variants(kind, E, B, "wide"):
            task_arg, task = _task(kind)
            plain = post.run(task_arg, xi, kappa=(0.0, 0.0), entry="draws")
            rest = np.setdiff1d(np.arange(post.B), rows)
            for dm, cm, kc in (("elite", "elite", 0.0), ("any", "mean", 0.7), ("majority", "any", 0.0)):
                want = ref.rule_votes(task, obs, act, mean, var, inds, D, dm, cm, rows=rows, xi=xi, dis_on=True, kappa_cost=kc)
                got = post.run(task_arg, xi, kappa=(0.0, kc), votes=(dm, cm))
                m = f"{tag} {dm}/{cm}"
                np.testing.assert_array_equal(got["term"][rows], want["term"], err_msg=m + " term")
                np.testing.assert_array_equal(_bits(got["cost"][rows]), _bits(want["cost"]), err_msg=m + " cost")
                np.testing.assert_array_equal(_bits(got["cost_var"][rows]), _bits(want["cost_var"]), err_msg=m + " cost_var")
                np.testing.assert_array_equal(got["done_votes"][rows], want["done_votes"], err_msg=m + " done_votes")
                np.testing.assert_array_equal(got["cost_votes"][rows], want["cost_votes"], err_msg=m + " cost_votes")
                _same(got, plain, ("next_obs", "rew", "rew_var", "dkl_path", "ep_var_mean", "ep_var"), m)
                for k in ("term", "done_votes", "cost_votes"):
                    assert (got[k][rest] == 77).all(), (m, k)
                if dm == "elite":
                    _same(got, plain, ("term", "cost"), m)
            if B == 203:
                cv, dv = want["cost_votes"], want["done_votes"]
                assert ((cv > 0) & (cv < E)).mean() >= 0.10 and ((dv > 0) & (dv < E)).mean() >= 0.10, tag


@pytest.mark.parametrize("kind,E", [("ant", 7), ("table29", 8), ("table5", 3), ("hcs", 5)])
def test_votes_with_a_termination_head(hip_lib, kind, E):
    """Check 4: with a termination head, under each of its three modes, with its scalar threshold and with per-row thresholds,
    term is the voted rule OR the head's verdict, and term_pred / term_votes are the plain call's."""
    _need_gpu()
    D, A = DIMS[kind]
    for B in (13, 1003):
        rng = np.random.default_rng(zlib.crc32(f"{kind}/{E}/{B}/head".encode()))
        obs, act, mean, var, inds = _inputs(kind, E, B, rng, extra_cols=1)
        O = D + 2
        mean[:, :, O - 1] = (np.float32(0.35) + np.float32(0.3) * rng.standard_normal(B)[None]
                             + np.float32(0.15) * rng.standard_normal((E, B))).astype(np.float32)
        rows = np.arange(B, dtype=np.int32)
        _plant(mean, inds, rows, E, D)
        mean[inds[B - 1], B - 1, O - 1] = NAN                       # the elite's NaN never hits
        post = _Post(obs, act, mean, var, inds, None, D, A)
        thr = (1.0 - rng.random(B, dtype=np.float32)).astype(np.float32)
        task_arg, task = _task(kind)
        xi = rng.standard_normal((B, D)).astype(np.float32)
        for hm in DONE_MODES:
            for row_thr in (None, thr):
                plain = post.run(task_arg, xi, head=(0.5, hm), thr=row_thr, entry="draws")
                t = np.full(B, 0.5, np.float32) if row_thr is None else row_thr
                learned = tdref.term_draws(mean, inds, t, hm)[0].astype(bool)         # (no rule: the head's verdict alone)
                for dm, cm in (("elite", "elite"), ("any", "mean"), ("majority", "any")):
                    want = ref.rule_votes(task, obs, act, mean, var, inds, D, dm, cm, xi=xi, learned_done=learned)
                    got = post.run(task_arg, xi, head=(0.5, hm), thr=row_thr, votes=(dm, cm))
                    m = f"{kind} B={B} head={hm} thr={row_thr is not None} {dm}/{cm}"
                    np.testing.assert_array_equal(got["term"], want["term"], err_msg=m + " term")
                    np.testing.assert_array_equal(_bits(got["cost"]), _bits(want["cost"]), err_msg=m + " cost")
                    _same(got, plain, ("next_obs", "rew", "dkl_path", "ep_var_mean", "ep_var", "term_pred", "term_votes"), m)
                    if dm == "elite":
                        _same(got, plain, ("term", "cost"), m)
        assert learned.any() and not learned.all()


@pytest.mark.parametrize("kind,E", [("ant", 7), ("table29", 5), ("table5", 8), ("hcs", 3)])
def test_votes_with_the_disagreement(hip_lib, kind, E):
    """Check 5: with the disagreement on, cost_var is np.var of the members' indicators for kappa_cost 0 and 0.7, the pessimistic
    cost the clipped sum; rew / rew_var are the plain call's."""
    _need_gpu()
    D, A = DIMS[kind]
    for B in (13, 1003):
        for post, rows, obs, act, mean, var, inds, xi, tag in _variants(kind, E, B, "dis"):
            task_arg, task = _task(kind)
            plain = post.run(task_arg, xi, kappa=(0.5, 0.0), entry="draws")
            assert (plain["cost_var"][rows] == 0.0).all()                          # without the votes: +0, as it always was
            for kc in (0.0, 0.7):
                for dm, cm in (("elite", "elite"), ("any", "mean"), ("elite", "any"), ("majority", "majority")):
                    want = ref.rule_votes(task, obs, act, mean, var, inds, D, dm, cm, rows=rows, xi=xi, dis_on=True, kappa_cost=kc)
                    got = post.run(task_arg, xi, kappa=(0.5, kc), votes=(dm, cm))
                    m = f"{tag} kappa_cost={kc} {dm}/{cm}"
                    np.testing.assert_array_equal(_bits(got["cost_var"][rows]), _bits(want["cost_var"]), err_msg=m + " cost_var")
                    np.testing.assert_array_equal(_bits(got["cost"][rows]), _bits(want["cost"]), err_msg=m + " cost")
                    np.testing.assert_array_equal(got["term"][rows], want["term"], err_msg=m + " term")
                    _same(got, plain, ("next_obs", "rew", "rew_var", "dkl_path", "ep_var_mean", "ep_var"), m)
                    assert (got["cost"][rows] <= 1.0).all()
            if B == 1003:
                assert (want["cost_var"] > 0).mean() >= 0.10 and (want["cost"] == 1.0).any()


def test_the_learned_cost_refusal_and_the_termination_votes_beside_it(hip_lib):
    """Check 6: with CMBPO_TASK_LEARNED_COST a cost vote or cost_votes is refused by name; the termination votes still run, and
    cost / cost_var stay the learned column's."""
    _need_gpu()
    kind, E, B = "ant", 7, 1003
    D, A = DIMS[kind]
    rng = np.random.default_rng(77)
    obs, act, mean, var, inds = _inputs(kind, E, B, rng, extra_cols=1)
    post = _Post(obs, act, mean, var, inds, None, D, A)
    task_arg, task = _task(kind, learned=True)
    for cm in ("any", "majority", "mean"):
        post.run(task_arg, votes=("elite", cm), expect_rc=-1, cost_votes=False)
        msg = hip_lib.cmbpo_last_error()
        assert msg.startswith(b"cmbpo_fakeenv_post_votes") and b"rule votes" in msg and b"cost_members" in msg, msg
    post.run(task_arg, votes=("elite", "elite"), expect_rc=-1, cost_votes=True)
    msg = hip_lib.cmbpo_last_error()
    assert msg.startswith(b"cmbpo_fakeenv_post_votes") and b"rule votes" in msg and b"cost_votes" in msg, msg
    plain = post.run(task_arg, kappa=(0.0, 0.7), entry="draws")
    for dm in DONE_MODES:
        want = ref.rule_votes(task, obs, act, mean, var, inds, D, dm, learned_cost=True)
        got = post.run(task_arg, kappa=(0.0, 0.7), votes=(dm, "elite"), cost_votes=False)
        np.testing.assert_array_equal(got["term"], want["term"], err_msg=dm)
        np.testing.assert_array_equal(got["done_votes"], want["done_votes"], err_msg=dm)
        _same(got, plain, F_OUT + ("term_votes", "cost_votes"), f"learned cost {dm}")


# ------------------------------------------------------------------------------------------------------------------
# 2. the rollout
# ------------------------------------------------------------------------------------------------------------------
OBS, ACT, ENS = 6, 2, 3


class _Space:
    def __init__(self, d):
        self.shape = (d,)


class _Env:
    observation_space, action_space = _Space(OBS), _Space(ACT)


def _world(seed, hidden=512):
    from cmbpo_amd import synthetic
    rng = np.random.default_rng(seed)
    out_dim = OBS + 1
    ws, bs = synthetic.ensemble_weights(rng, ENS, OBS + ACT, hidden, 2 * out_dim, bias_scale=0.05)
    sc_in = synthetic.scaler(rng, OBS + ACT, hit_clamp=False)
    sc_out = synthetic.scaler(rng, out_dim, hit_clamp=False)
    pol = synthetic.policy_params(rng, OBS, ACT)
    crit = []
    for _ in range(2):
        cw, cb = synthetic.ensemble_weights(rng, 3, OBS, 128, 1, bias_scale=0.05)
        crit.append((cw, cb, synthetic.scaler(rng, OBS, hit_clamp=False), synthetic.scaler(rng, 1, hit_clamp=False)))
    return dict(hidden=hidden, out_dim=out_dim, ws=ws, bs=bs, sc_in=sc_in, sc_out=sc_out, pol=pol, v=crit[0], vc=crit[1],
                elites=[0, 2])


def _hip_world(w, B, T, **env_kw):
    from cmbpo_amd.cpo_policy import CPOPolicy
    from cmbpo_amd.fake_env import FakeEnv
    from cmbpo_amd.model_sampler import ModelSampler
    from cmbpo_amd.modelbuffer import ModelBuffer
    from cmbpo_amd.pens import PE
    model = PE(OBS + ACT, w["out_dim"], hidden_dims=(w["hidden"], w["hidden"]), num_networks=ENS, num_elites=len(w["elites"]),
               loss="MSPE", use_scaler_in=True, use_scaler_out=True, device=DEV)
    model.set_weights(w["ws"], w["bs"], w["sc_in"], w["sc_out"])
    model.set_elites(w["elites"])
    policy = CPOPolicy(_Space(OBS), _Space(ACT), a_hidden_layer_sizes=(128, 128), vf_hidden_layer_sizes=(128, 128),
                       vf_ensemble_size=3, vf_elites=2, vf_activation="swish", vf_loss="MSE", device=DEV,
                       cost_gamma=0.97, cost_lam=0.5, lam=0.95)
    policy.actor.set_params(w["pol"])
    policy.v.set_weights(*w["v"])
    policy.vc.set_weights(*w["vc"])
    env = FakeEnv(_Env(), "AntSafe-v2", model, predicts_delta=True, predicts_rew=True, predicts_cost=False, **env_kw)
    pool = ModelBuffer(B, OBS, ACT, T, device=DEV)
    pool.initialize(policy.pi_info_shapes, gamma=0.99, lam=0.95, cost_gamma=0.97, cost_lam=0.5)
    sampler = ModelSampler(max_path_length=T + 5, batch_size=B, rollout_mode="uncertainty", seed=3)
    sampler.initialize(env, policy, pool)
    sampler.set_rollout_dkl(float("inf"))
    return sampler, pool, env


def _start(seed, B):
    """AntSafe on six columns: the height inside its band (outside it the rule's precedence quirk ends nothing), for a third of
    the rows q1 around 0.92, where z_rot = 1 - 2 (q1^2 + q2^2) crosses -0.7 (this world's members move q1 by about 0.06, each its
    own way), the last column around its threshold of 3.2."""
    rng = np.random.default_rng(seed)
    s = (rng.standard_normal((B, OBS)) * 0.1).astype(np.float32)
    s[:, 0] = rng.uniform(0.35, 0.75, B).astype(np.float32)
    tilted = rng.random(B) < 0.33
    s[tilted, 2] = (np.where(rng.random(B) < 0.5, -0.92, 0.92) + rng.standard_normal(B) * 0.06).astype(np.float32)[tilted]
    s[:, OBS - 1] = (np.where(rng.random(B) < 0.5, -3.2, 3.2) + rng.standard_normal(B) * 0.3).astype(np.float32)
    return s


_STATE = ("len", "alive", "fin_code", "path_ret", "path_cost", "cur_obs", "term_t", "rew_t", "cost_t", "v_t", "vc_t")


def _roll(w, start, how, steps, T, **env_kw):
    """`steps` steps as one cmbpo_rollout_run ('many') or as a loop of cmbpo_rollout_step ('loop'); with check=True ('loop' only)
    every step's term_t / cost_t / votes / cost_var_t are held against the reference on the step's own (mean, var)."""
    B = start.shape[0]
    sampler, pool, env = _hip_world(w, B, T, **env_kw)
    sampler.reset(start)
    per_step = []
    if how == "many":
        done, _ = sampler.sample_many(max_steps=steps)
    else:
        done = 0
        while done < steps and sampler.any_alive() and pool.has_room:
            n = pool.n_alive
            ids = pool.t["alive_idx"][:n].cpu().numpy().copy()
            cur = pool.t["cur_obs"].cpu().numpy().copy()
            sampler.sample()
            torch.cuda.synchronize()
            k = sampler._draws[0] - 1
            rec = dict(ids=ids, obs=cur, act=pool.t["act_t"].cpu().numpy().copy(), inds=sampler._draws[2][k].cpu().numpy().copy(),
                       mean=sampler._scratch[0].cpu().numpy().copy(), var=sampler._scratch[1].cpu().numpy().copy())
            for key in ("term_t", "cost_t", "rule_done_votes_t", "rule_cost_votes_t", "cost_var_t", "next_obs", "cur_obs", "rew_t"):
                if key in pool.t:
                    rec[key] = pool.t[key].cpu().numpy().copy()
            per_step.append(rec)
            done += 1
    torch.cuda.synchronize()
    state = {k: pool.t[k].cpu().numpy().copy() for k in _STATE}
    for k in ("rule_done_votes_t", "rule_cost_votes_t", "cost_var_t"):
        if k in pool.t:
            state[k] = pool.t[k].cpu().numpy().copy()
    state["alive_list"] = pool.t["alive_idx"][:pool.n_alive].cpu().numpy().copy()
    state["counters"] = np.array([done, pool.n_alive, pool.ptr, pool.size])
    state["dscal"] = pool.t["dscal"][:17].cpu().numpy().copy()
    return dict(state=state, per_step=per_step, steps=done, attached=pool.rule_votes)


def _check_steps(run, dm, cm, dis_on=False, kappa_cost=0.0):
    E = ENS
    mixed = mixed_done = 0
    for rec in run["per_step"]:
        ids = rec["ids"]
        want = ref.rule_votes("AntSafe-v2", rec["obs"], rec["act"], rec["mean"], rec["var"], rec["inds"], OBS, dm, cm, rows=ids,
                              dis_on=dis_on, kappa_cost=kappa_cost)
        np.testing.assert_array_equal(rec["term_t"][ids], want["term"])
        np.testing.assert_array_equal(_bits(rec["cost_t"][ids]), _bits(want["cost"]))
        np.testing.assert_array_equal(rec["rule_done_votes_t"][ids], want["done_votes"])
        np.testing.assert_array_equal(rec["rule_cost_votes_t"][ids], want["cost_votes"])
        if dis_on:
            np.testing.assert_array_equal(_bits(rec["cost_var_t"][ids]), _bits(want["cost_var"]))
        mixed += int(((want["cost_votes"] > 0) & (want["cost_votes"] < E)).sum())
        mixed_done += int(((want["done_votes"] > 0) & (want["done_votes"] < E)).sum())
    assert mixed > 0 and mixed_done > 0          # the members disagreed on both verdicts: the comparison above is about something


def test_rollout_step_and_run_with_the_votes_attached(hip_lib):
    """Check 7: B = 96, three steps.  The one-call step with the votes attached: every step's term_t, cost_t and votes are the
    reference's on the step's own (mean, var); the native loop equals the loop of steps bit for bit; with done_members 'elite'
    (cost 'mean') next_obs, rew, the lengths and the alive lists are those of the run without the votes."""
    _need_gpu()
    B, steps, T = 96, 3, 8
    w = _world(21)
    start = _start(22, B)
    off = _roll(w, start, "loop", steps, T)
    assert off["attached"] is None and "rule_done_votes_t" not in off["state"]
    for dm, cm in (("elite", "mean"), ("any", "any")):
        loop = _roll(w, start, "loop", steps, T, static_term_members=dm, static_cost_members=cm)
        many = _roll(w, start, "many", steps, T, static_term_members=dm, static_cost_members=cm)
        assert loop["attached"] == (dm, cm, True) and loop["steps"] == many["steps"] == steps
        _check_steps(loop, dm, cm)
        for k in loop["state"]:
            np.testing.assert_array_equal(_bits(loop["state"][k]), _bits(many["state"][k]), err_msg=f"run / step {dm}/{cm}: {k}")
        if dm == "elite":
            for k in ("len", "alive", "fin_code", "cur_obs", "rew_t", "term_t", "path_ret", "alive_list", "counters"):
                np.testing.assert_array_equal(_bits(loop["state"][k]), _bits(off["state"][k]), err_msg=f"votes / none: {k}")
            for a, b in zip(loop["per_step"], off["per_step"]):
                for k in ("ids", "next_obs", "cur_obs", "rew_t", "term_t"):
                    np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"votes / none per step: {k}")
            assert not np.array_equal(loop["state"]["path_cost"], off["state"]["path_cost"])       # the mean is not the elite's bit
    # with the disagreement: cost_var_t carries the static cost's spread, the pessimistic cost is clipped, the totals move
    dis = _roll(w, start, "loop", steps, T, static_votes=True, disagreement=True, cost_pessimism=0.7)
    _check_steps(dis, "elite", "elite", dis_on=True, kappa_cost=0.7)
    assert dis["state"]["dscal"][14] > 0.0                                                        # CMBPO_D_TOTAL_COST_VAR
