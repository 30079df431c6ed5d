"""CPU: the static rules' votes in the model replay without a GPU -- the host's table against the loop-written
reference on hand-made histograms, the reference's histogram against rule_votes_ref on the golden steps, the C-ABI (struct image,
exports, every refusal by name with buffers that are never dereferenced), and the FakeEnv.replay / CMBPO arguments.

Counts are compared exactly; derived rates are float64 functions of the same integers added in two orders, compared to 1e-12."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import replay_ref as ref
import replay_votes_ref as vtref
import rule_votes_ref as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = ("cmbpo_replay_votes", "cmbpo_replay_votes_finish", "cmbpo_replay_run_votes")
RATES = ("ece", "mce", "brier", "base_rate", "mean_share", "split_rate")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cmbpo_amd import _lib
    return _lib.lib()


def check_table(got, want_tab, E, learned_cost=False):
    """got: replay.votes_table's dict; want_tab: a table of the reference."""
    np.testing.assert_array_equal(got["n_vote"], want_tab["n_vote"])
    np.testing.assert_array_equal(got["n_skipped"], want_tab["n_skipped"])
    assert ("cost" in got) == (not learned_cost) and "term" in got
    for name in ("cost", "term"):
        if name not in got:
            continue
        want = vtref.derived(want_tab["hist_" + name], E)
        d = got[name]
        for k in ("hist", "n"):
            np.testing.assert_array_equal(d[k], want[k], err_msg=name + k)
        for mode in ("any", "majority"):
            np.testing.assert_array_equal(d["cm"][mode], want["cm"][mode], err_msg=name + mode)
        for k in RATES + ("freq", "conf"):
            assert d[k].dtype == np.float64
            np.testing.assert_array_equal(np.isnan(d[k]), np.isnan(want[k]), err_msg=name + k)
            np.testing.assert_allclose(d[k], want[k], rtol=0, atol=1e-12, err_msg=name + k)


# ------------------------------------------------------------------------------------------------------------------
# 1. the host's table
# ------------------------------------------------------------------------------------------------------------------
def _hand_made(E, rng, H=4):
    """Row 0: random; row 1: empty; row 2: every row at v = E; row 3: random, one recorded class only."""
    tab = vtref.new_table(H)
    for name in ("hist_cost", "hist_term"):
        h = tab[name]
        h[0, :E + 1] = rng.integers(0, 50, (E + 1, 2))
        h[2, E] = rng.integers(1, 50, 2)
        h[3, :E + 1, 0] = rng.integers(0, 50, E + 1)
    tab["n_vote"][:] = tab["hist_term"].sum(axis=(1, 2))
    for h in (2, 3):
        tab["hist_cost"][h] = tab["hist_term"][h]
    tab["n_skipped"][0] = 3
    return tab


@pytest.mark.parametrize("E", [1, 2, 3, 7, 8])
def test_votes_table_on_hand_made_histograms(E):
    from cmbpo_amd import replay
    tab = _hand_made(E, np.random.default_rng(E))
    got = replay.votes_table(vtref.raw_counts(tab), E)
    check_table(got, tab, E)
    for name in ("cost", "term"):
        d = got[name]
        assert d["hist"].shape == (4, E + 1, 2) and d["freq"].shape == (4, E + 1) and d["conf"].shape == (E + 1,)
        # the empty horizon: NaN rates, zero counts
        assert d["n"][1] == 0 and all(np.isnan(d[k][1]) for k in RATES) and np.isnan(d["freq"][1]).all()
        assert not d["cm"]["any"][1].any() and not d["cm"]["majority"][1].any()
        # every row at v = E: the share says 1, nobody is split, both readings report every row
        h = d["hist"][2]
        assert d["split_rate"][2] == 0.0 and d["mean_share"][2] == 1.0
        np.testing.assert_allclose(d["ece"][2], h[E, 0] / h[E].sum(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(d["brier"][2], h[E, 0] / h[E].sum(), rtol=0, atol=1e-12)
        np.testing.assert_array_equal(d["cm"]["any"][2][:, 1], h[E])
        np.testing.assert_array_equal(d["cm"]["majority"][2][:, 1], h[E])
        assert d["base_rate"][3] == 0.0
        if E == 1:
            assert (d["split_rate"][[0, 2, 3]] == 0.0).all()                # one member cannot split
            np.testing.assert_array_equal(d["cm"]["any"], d["cm"]["majority"])
        # the identities: the readings' positives are sums over the histogram
        for hh in range(4):
            for y in (0, 1):
                assert d["cm"]["any"][hh, y, 1] == d["hist"][hh, 1:, y].sum()
                assert d["cm"]["majority"][hh, y, 1] == sum(d["hist"][hh, v, y] for v in range(E + 1) if 2 * v > E)
                assert d["cm"]["any"][hh, y].sum() == d["cm"]["majority"][hh, y].sum() == d["hist"][hh, :, y].sum()
    learned = replay.votes_table(vtref.raw_counts(tab), E, learned_cost=True)
    assert "cost" not in learned and sorted(learned) == ["n_skipped", "n_vote", "term"]


def test_votes_table_refuses_what_does_not_fit():
    from cmbpo_amd import replay
    ok = np.zeros((2, 38), np.int64)
    with pytest.raises(ValueError, match=r"counts \[H, 38\]"):
        replay.votes_table(np.zeros((2, 37), np.int64), 3)
    for E in (0, 9):
        with pytest.raises(ValueError, match="E must lie in 1..8"):
            replay.votes_table(ok, E)
    bad = ok.copy()
    bad[1, 2 * 5 + 1] = 1                                                   # a cost row with five votes of three members
    with pytest.raises(ValueError, match="more than E = 3 votes"):
        replay.votes_table(bad, 3)
    assert replay.votes_table(bad, 5)["cost"]["hist"][1, 5, 1] == 1


# ------------------------------------------------------------------------------------------------------------------
# 2. the reference's histogram against rule_votes_ref on the golden steps
# ------------------------------------------------------------------------------------------------------------------
def test_reference_histogram_on_the_golden_steps():
    """One replay step (H = 1) whose model step is a golden FakeEnv step: the histogram is a count of rule_votes_ref's votes."""
    from cmbpo_amd import replay
    seen = 0
    for E in (3, 5, 7):
        g = np.load(os.path.join(GOLD, f"g16_step_e{E}.npz"), allow_pickle=False)
        for D in (int(d) for d in g["dims"]):
            for short, task in (("ant", "AntSafe-v2"), ("hcs", "HalfCheetahSafe-v2")):
                if f"d{D}_{short}_terms" not in g.files:
                    continue
                obs, act, mean, var, inds = (g[f"d{D}_{k}"] for k in ("obs", "act", "mean", "var", "inds"))
                rng = np.random.default_rng(E * 100 + D)
                mean = mean.copy()
                mean[:, :, 0] += (rng.standard_normal(mean.shape[:2]) * 0.4).astype(np.float32)      # the members disagree
                mean[:, :, D - 1] += (rng.standard_normal(mean.shape[:2]) * 0.4).astype(np.float32)
                B = obs.shape[0]
                rec = dict(next_obs=rng.standard_normal((1, B, D)).astype(np.float32), rew=np.zeros((1, B), np.float32),
                           cost=rng.choice(np.array([0.0, 0.0, 1.0], np.float32), (1, B)), term=(rng.random((1, B)) < 0.3).astype(np.uint8))
                own = (rng.random((1, B)) < 0.5).astype(np.uint8)

                def forward(h, cur, mean=mean, var=var, D=D, B=B):
                    z = np.zeros(B, np.float32)
                    return dict(next_obs=(mean[0, :, :D] + cur).astype(np.float32), rew=z, cost=z, term=z.astype(np.uint8),
                                ep_var_mean=z, dkl_path=z), mean, var

                for dm, cm, term in (("elite", "elite", None), ("any", "mean", own), ("majority", "any", None)):
                    plain, vt, _, _, steps = vtref.replay_votes(forward, task, obs, act[None], rec, None, inds[None], ref.ONE_STEP, E, D,
                                                                dm, cm, term=term)
                    want = vref.rule_votes(task, obs, act, mean, var, inds, D, dm, cm)
                    flags = (rec["term"] if term is None else term)[0]
                    for v in range(9):
                        for y in (0, 1):
                            assert vt["hist_term"][0, v, y] == ((want["done_votes"] == v) & (flags == y)).sum()
                            assert vt["hist_cost"][0, v, y] == ((want["cost_votes"] == v) & ((rec["cost"][0] > 0) == y)).sum()
                    assert vt["n_vote"][0] == B == plain["n"][0] and vt["n_skipped"][0] == 0
                    # the plain table under the vote describes the rule in force
                    np.testing.assert_array_equal(steps[0]["pred"]["term"], want["term"])
                    np.testing.assert_array_equal(steps[0]["pred"]["cost"], want["cost"])
                    got = replay.votes_table(vtref.raw_counts(vt), E)
                    check_table(got, vt, E)
                    if term is None and dm in ("any", "majority"):
                        np.testing.assert_array_equal(plain["term_cm"][0][:, 1], got["term"]["cm"][dm][0][:, 1])
                    if cm in ("any", "majority"):
                        np.testing.assert_array_equal(plain["cost_cm"][0][:, 1], got["cost"]["cm"][cm][0][:, 1])
                    if cm == "mean":                                        # p_cost > 0.5 of the share is the strict majority
                        np.testing.assert_array_equal(plain["cost_cm"][0][:, 1], got["cost"]["cm"]["majority"][0][:, 1])
                    seen += 1
    assert seen >= 9


def test_reference_skips_rows_with_impossible_counts_and_dead_rows():
    E, B, D = 3, 6, 2
    tab = vtref.new_table(1)
    z = np.zeros(B, np.float32)
    pred = dict(next_obs=np.zeros((B, D), np.float32), rew=z.copy(), cost=z.copy())
    pred["rew"][4] = np.nan
    rec = dict(cost=np.array([[0, 1, 1, 0, 0, 0]], np.float32), term=np.array([[1, 0, 0, 0, 0, 0]], np.uint8))
    alive = np.array([1, 1, 1, 1, 1, 0], bool)
    ok = vtref.votes(tab, 0, alive, pred, rec, E, np.array([0, 3, 4, 1, 1, 1]), np.array([3, 0, 0, 9, 1, 1]))
    np.testing.assert_array_equal(ok, [True, True, False, False, False, False])
    assert tab["n_vote"][0] == 2 and tab["n_skipped"][0] == 2               # row 4 is not finite, row 5 dead: in neither
    assert tab["hist_cost"][0, 3, 0] == 1 and tab["hist_cost"][0, 0, 1] == 1 and tab["hist_cost"].sum() == 2
    assert tab["hist_term"][0, 0, 1] == 1 and tab["hist_term"][0, 3, 0] == 1 and tab["hist_term"].sum() == 2


# ------------------------------------------------------------------------------------------------------------------
# 3. the C-ABI
# ------------------------------------------------------------------------------------------------------------------
def _header():
    text = open(os.path.join(ROOT, "include", "cmbpo_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_library_exports_the_three_symbols_and_keeps_its_version(lib):
    from cmbpo_amd import _lib
    assert lib.cmbpo_version() == 6
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES


def test_header_signatures_and_struct_image_agree():
    from cmbpo_amd import _lib
    text = _header()
    m = re.search(r"typedef struct cmbpo_replay_votes \{(.*?)\} cmbpo_replay_votes_t;", text, flags=re.S)
    assert m, "cmbpo_replay_votes_t is not declared"
    decls = [d.strip() for d in m.group(1).split(";") if d.strip()]
    assert decls == ["int32_t ensemble", "int32_t done_members", "int32_t cost_members", "int32_t reserved", "uint8_t *done_votes",
                     "uint8_t *cost_votes", "const uint8_t *term", "int64_t *part_cnt", "int64_t *counts"]
    S = _lib.ReplayVotesStruct
    assert [n for n, _ in S._fields_] == [d.split()[-1].lstrip("*") for d in decls]
    assert all((t is C.c_void_p) == ("*" in d) for (_, t), d in zip(S._fields_, decls))
    assert C.sizeof(S) == 56 and S.reserved.offset == 12 and S.done_votes.offset == 16 and S.counts.offset == 48
    # the three other descriptors are what they were
    assert (C.sizeof(_lib.ReplayStruct), C.sizeof(_lib.ReplayCalibStruct), C.sizeof(_lib.ReplayReliabStruct)) == (184, 56, 104)
    rp, cp, rr, rv = (C.POINTER(s) for s in (_lib.ReplayStruct, _lib.ReplayCalibStruct, _lib.ReplayReliabStruct, S))
    tp, chp = C.POINTER(_lib.TermHeadStruct), C.POINTER(_lib.CostHeadStruct)
    sig_ = _lib.SIGNATURES
    assert sig_["cmbpo_replay_votes"] == (C.c_int, [rp, rv, C.c_int, C.c_void_p])
    assert sig_["cmbpo_replay_votes_finish"] == (C.c_int, [rp, rv, C.c_void_p])
    # cmbpo_replay_run_reliab's arguments with the vote descriptor behind the reliability descriptor
    reliab = sig_["cmbpo_replay_run_reliab"][1]
    assert sig_["cmbpo_replay_run_votes"] == (C.c_int, reliab[:3] + [rv] + reliab[3:])
    assert re.search(r"int cmbpo_replay_votes\(const cmbpo_replay_t \*rp, const cmbpo_replay_votes_t \*rv, int h, void \*stream\);", text)
    assert re.search(r"int cmbpo_replay_votes_finish\(const cmbpo_replay_t \*rp, const cmbpo_replay_votes_t \*rv, void \*stream\);", text)
    assert re.search(r"int cmbpo_replay_run_votes\(const cmbpo_replay_t \*rp, const cmbpo_replay_calib_t \*rc, const cmbpo_replay_reliab_t \*rr,"
                     r"\s*const cmbpo_replay_votes_t \*rv, const cmbpo_term_head_t \*th, const cmbpo_cost_head_t \*ch,\s*cmbpo_mlp_t \*model, "
                     r"int task, int ensemble, const int32_t \*d_elite, void \*stream\);", text)
    assert re.search(r"#define CMBPO_REPLAY_VOTE_COUNTS 38\b", text) and _lib.REPLAY_VOTE_COUNTS == 38 == vtref.COUNTS
    assert re.search(r"#define CMBPO_REPLAY_VOTES_MAX_ENSEMBLE 8\b", text) and _lib.REPLAY_VOTES_MAX_ENSEMBLE == 8
    assert _lib.REPLAY_VOTE_SLOTS == 9 == vtref.SLOTS


def _images(rp_kw=None, rv_kw=None):
    """Descriptors whose every array points at host memory that is never read: each call below fails a check first."""
    from cmbpo_amd import _lib
    host = (C.c_double * 8)()
    addr = C.cast(host, C.c_void_p).value
    rs, rv = _lib.ReplayStruct(), _lib.ReplayVotesStruct()
    rs._keep = rv._keep = host
    rs.B, rs.H, rs.obs_dim, rs.act_dim, rs.mode = 5, 3, 27, 8, 0
    rv.ensemble = 7
    for S, s in ((_lib.ReplayStruct, rs), (_lib.ReplayVotesStruct, rv)):
        for n, t in S._fields_:
            if t is C.c_void_p:
                setattr(s, n, addr)
    for s, kw in ((rs, rp_kw), (rv, rv_kw)):
        for k, v in (kw or {}).items():
            setattr(s, k, v)
    return rs, rv


def _fake_model(out_dim):
    """Stands for a model handle of which only out_dim is read: a block of ints with out_dim where csrc/ens_mlp_internal.h declares it."""
    src = open(os.path.join(ROOT, "constrained-model-based-policy-optimization_amd", "csrc", "ens_mlp_internal.h")).read()
    first = re.search(r"struct cmbpo_mlp \{\s*int ([^;]*);", src).group(1)
    ints = (C.c_int * 256)()
    ints[[n.strip() for n in first.split(",")].index("out_dim")] = out_dim
    return ints


def test_every_entry_refuses_bad_arguments_without_a_gpu(lib):
    from cmbpo_amd import _lib
    ANT, LC = _lib.TASK_ANTSAFE, _lib.TASK_LEARNED_COST
    model = _fake_model(28)
    fake = C.cast(model, C.c_void_p)
    elite = C.cast((C.c_int32 * 16)(), C.c_void_p)

    def calls(rs, rv, h=0, ens=7, task=ANT, th=None, fake=fake):
        return (("cmbpo_replay_votes", lambda: lib.cmbpo_replay_votes(C.byref(rs), C.byref(rv), h, None)),
                ("cmbpo_replay_votes_finish", lambda: lib.cmbpo_replay_votes_finish(C.byref(rs), C.byref(rv), None)),
                ("cmbpo_replay_run_votes", lambda: lib.cmbpo_replay_run_votes(C.byref(rs), None, None, C.byref(rv), th, None, fake, task, ens,
                                                                             elite, None)))

    def refused(name, call, *words):
        assert call() == -1, name
        msg = lib.cmbpo_last_error()
        assert msg.startswith(name.encode() + b":"), msg
        for w in words:
            assert w in msg, msg

    # the shape refusals of the compare call, in all three
    for bad, word in ((dict(B=0), b"B 0"), (dict(H=-1), b"H -1"), (dict(mode=2), b"unknown mode 2"), (dict(obs_dim=0), b"bad dims"),
                      (dict(reserved=1), b"reserved")):
        for name, call in calls(*_images(rp_kw=bad)):
            refused(name, call, word)
    # the vote descriptor's own, in all three
    for bad, word in ((dict(ensemble=0), b"vote ensemble 0"), (dict(ensemble=-3), b"vote ensemble -3"), (dict(reserved=2), b"vote reserved 2")):
        for name, call in calls(*_images(rv_kw=bad), ens=bad.get("ensemble", 7)):
            refused(name, call, word)
    # ensemble above 8 and the modes' ranges: the single-step entries say it themselves ...
    for name, call in calls(*_images(rv_kw=dict(ensemble=9)), ens=9)[:2]:
        refused(name, call, b"vote ensemble 9 outside [1, 8]")
    for bad, word in ((dict(done_members=-1), b"done_members -1"), (dict(done_members=3), b"done_members 3"),
                      (dict(cost_members=4), b"cost_members 4"), (dict(cost_members=-1), b"cost_members -1")):
        for name, call in calls(*_images(rv_kw=bad))[:2]:
            refused(name, call, b"rule votes", word)
        # ... the run entry passes the post step's refusal on under its own name
        refused("cmbpo_replay_run_votes", calls(*_images(rv_kw=bad))[2][1], b"cmbpo_fakeenv_post_votes: rule votes", word)
    refused("cmbpo_replay_run_votes", calls(*_images(rv_kw=dict(ensemble=9)), ens=9)[2][1], b"cmbpo_fakeenv_post_votes", b"ensemble 9")
    # a learned cost: nothing to vote on, nothing to count -- the post step's words again
    for cm in (1, 2, 3):
        refused("cmbpo_replay_run_votes", calls(*_images(rv_kw=dict(cost_members=cm)), task=ANT | LC)[2][1], b"rule votes", b"cost_members",
                b"CMBPO_TASK_LEARNED_COST")
    refused("cmbpo_replay_run_votes", calls(*_images(), task=ANT | LC)[2][1], b"rule votes", b"cost_votes", b"CMBPO_TASK_LEARNED_COST")
    # a termination head must bring both of its outputs
    th = _lib.TermHeadStruct()
    th.threshold, th.members = 0.5, 0
    with_head = _fake_model(29)
    refused("cmbpo_replay_run_votes", calls(*_images(), th=C.byref(th), fake=C.cast(with_head, C.c_void_p))[2][1], b"term_pred", b"term_votes")
    # NULL descriptors
    rs, rv = _images()
    for name, call in (("cmbpo_replay_votes", lambda: lib.cmbpo_replay_votes(None, C.byref(rv), 0, None)),
                       ("cmbpo_replay_votes", lambda: lib.cmbpo_replay_votes(C.byref(rs), None, 0, None)),
                       ("cmbpo_replay_votes_finish", lambda: lib.cmbpo_replay_votes_finish(None, C.byref(rv), None)),
                       ("cmbpo_replay_votes_finish", lambda: lib.cmbpo_replay_votes_finish(C.byref(rs), None, None)),
                       ("cmbpo_replay_run_votes", lambda: lib.cmbpo_replay_run_votes(None, None, None, C.byref(rv), None, None, fake, ANT, 7,
                                                                                    elite, None))):
        refused(name, call, b"NULL")
    # rv == NULL is cmbpo_replay_run_reliab's call, under that entry's name rules (here: the plain run's, nothing else is given)
    assert lib.cmbpo_replay_run_votes(C.byref(rs), None, None, None, None, None, None, 0, 7, None, None) == -1
    assert lib.cmbpo_last_error().startswith(b"cmbpo_replay_run:") and b"model" in lib.cmbpo_last_error()
    rr = _lib.ReplayReliabStruct()
    assert lib.cmbpo_replay_run_votes(C.byref(rs), None, C.byref(rr), None, None, None, fake, 0, 7, None, None) == -1
    assert lib.cmbpo_last_error().startswith(b"cmbpo_replay_run_reliab:")
    # NULL arrays
    for k in ("next_obs", "rew", "cost", "term", "len", "cur_obs", "alive", "p_next_obs", "p_rew", "p_term", "p_cost", "p_dkl_path",
              "p_ep_var_mean", "part_sum", "part_cnt"):
        rs, rv = _images(rp_kw={k: None})
        refused("cmbpo_replay_votes", calls(rs, rv)[0][1], b"NULL")
        refused("cmbpo_replay_run_votes", calls(rs, rv)[2][1], b"NULL")
    for k in ("act", "mean", "var", "sums", "counts"):
        rs, rv = _images(rp_kw={k: None})
        refused("cmbpo_replay_run_votes", calls(rs, rv)[2][1], b"NULL")
    for k in ("done_votes", "part_cnt"):
        rs, rv = _images(rv_kw={k: None})
        refused("cmbpo_replay_votes", calls(rs, rv)[0][1], b"NULL")
        refused("cmbpo_replay_run_votes", calls(rs, rv)[2][1], b"NULL")
    for k in ("part_cnt", "counts"):
        rs, rv = _images(rv_kw={k: None})
        refused("cmbpo_replay_votes_finish", calls(rs, rv)[1][1], b"NULL")
        refused("cmbpo_replay_run_votes", calls(rs, rv)[2][1], b"NULL")
    # cost_votes and the descriptor's own terminals are optional: neither NULL is refused (h is, behind them)
    rs, rv = _images(rv_kw=dict(cost_votes=None, term=None))
    for h in (-1, 3, 1 << 20):
        refused("cmbpo_replay_votes", calls(rs, rv, h=h)[0][1], b"outside [0, 3)")
    # cmbpo_replay_run_votes alone: the handle, the run's ensemble, d_elite
    rs, rv = _images()
    refused("cmbpo_replay_run_votes", lambda: lib.cmbpo_replay_run_votes(C.byref(rs), None, None, C.byref(rv), None, None, None, ANT, 7, elite,
                                                                        None), b"model")
    refused("cmbpo_replay_run_votes", calls(rs, rv, ens=5)[2][1], b"ensemble 5, the vote descriptor's is 7")
    refused("cmbpo_replay_run_votes", lambda: lib.cmbpo_replay_run_votes(C.byref(rs), None, None, C.byref(rv), None, None, fake, ANT, 7, None,
                                                                        None), b"d_elite")


# ------------------------------------------------------------------------------------------------------------------
# 4. FakeEnv.replay, CMBPO
# ------------------------------------------------------------------------------------------------------------------
def _fake_env(predicts_cost=False, **kw):
    """A FakeEnv up to its checks: a model stub, no device."""
    from toyworld import ToyEnv
    from cmbpo_amd.fake_env import FakeEnv
    env = ToyEnv()
    n, a = int(np.prod(env.observation_space.shape)), int(np.prod(env.action_space.shape))

    class Model:
        is_ensemble = is_probabilistic = True
        in_dim, out_dim, device = n + a, n + 1 + int(predicts_cost), "cpu"
    return FakeEnv(env, "default", Model(), True, True, predicts_cost, **kw), n, a


def test_fake_env_replay_refuses_in_words_before_it_touches_a_device():
    plain, n, a = _fake_env()
    z = lambda *s: np.zeros(s, np.float32)
    args = (z(4, n), z(2, 4, a), z(2, 4, n), z(2, 4), z(2, 4), z(2, 4))
    with pytest.raises(ValueError, match="votes=True needs the static votes on"):
        plain.replay(*args, votes=True)
    for bad in ("any", 2, None, "elite"):
        with pytest.raises(ValueError, match="votes is False, True or 'measure'"):
            plain.replay(*args, votes=bad)
    with pytest.raises(ValueError, match="reliability_terminals needs reliability=True"):
        plain.replay(*args, reliability_terminals=z(2, 4))                    # as it always was


def test_buffers_refuse_a_vote_spec_that_does_not_fit(lib):
    """ReplayBuffers' own checks come behind its allocations, so they are exercised through the spec parser alone."""
    from cmbpo_amd.replay import ReplayBuffers

    def Stub():
        rb = object.__new__(ReplayBuffers)
        rb.H, rb.B, rb.n_part, rb.device, rb.t = 2, 4, 1, "cpu", dict(mean=None)
        return rb
    for spec, E, word in ((dict(done_members="mean"), 3, "done_members"), (dict(cost_members="all"), 3, "cost_members"),
                          (dict(cost_members="any", learned_cost=True), 3, "nothing to"), (dict(), 9, "ensemble in 1..8"),
                          (dict(), 0, "ensemble in 1..8"), (dict(members="any"), 3, "unknown votes keys")):
        with pytest.raises(ValueError, match=word):
            ReplayBuffers._init_votes(Stub(), dict(spec), E)
    no_scratch = Stub()
    no_scratch.t = {}
    with pytest.raises(ValueError, match="forward's scratch"):
        ReplayBuffers._init_votes(no_scratch, {}, 3)
    plain = Stub()
    plain.vs = None
    for call in (lambda: ReplayBuffers.votes(plain, 0), lambda: ReplayBuffers.votes_finish(plain), lambda: ReplayBuffers.votes_table(plain),
                 lambda: ReplayBuffers.run_votes(plain, None, 0, 3, None)):
        with pytest.raises(ValueError, match="votes=None"):
            call()


def test_cmbpo_refusals():
    from cmbpo_amd.cmbpo import CMBPO, _validate_votes_args
    assert _validate_votes_args(0, True, False, False) is False
    assert _validate_votes_args(5, True, True, True) is True
    make = lambda **kw: CMBPO(None, None, None, **kw)
    with pytest.raises(ValueError, match="m_validate_votes needs m_validate_horizon > 0"):
        make(m_validate_votes=True, m_static_votes=True)
    with pytest.raises(ValueError, match="m_validate_votes needs m_validate_horizon > 0"):
        make(m_validate_votes=True, m_static_votes=True, m_validate_horizon=3, use_model=False)
    with pytest.raises(ValueError, match="m_validate_votes needs the static votes"):
        make(m_validate_votes=True, m_validate_horizon=3)
    # the one-step row of a table as the trainer logs it
    tab = _hand_made(3, np.random.default_rng(0))
    from cmbpo_amd import replay
    vt = replay.votes_table(vtref.raw_counts(tab), 3)
    out = CMBPO._votes_diagnostics(vt)
    want = ["val_vote_skipped"] + [f"val_vote_{k}_{s}_h1" for s in ("cost", "term") for k in ("ece", "split")] + \
           [f"val_{s}_{k}_rate_{m}" for s in ("cost", "term") for k in ("miss", "false_alarm") for m in ("any", "majority")]
    assert sorted(out) == sorted(want) and out["val_vote_skipped"] == 3
    c = vt["cost"]["cm"]["any"][0]
    assert out["val_cost_miss_rate_any"] == c[1, 0] / (c[1, 0] + c[1, 1]) and out["val_vote_ece_cost_h1"] == vt["cost"]["ece"][0]
    learned = CMBPO._votes_diagnostics(replay.votes_table(vtref.raw_counts(tab), 3, learned_cost=True))
    assert not [k for k in learned if "cost" in k] and "val_term_miss_rate_majority" in learned


# ------------------------------------------------------------------------------------------------------------------
# 5. the GPU tests' fixtures, on the oracle's CPU forward
# ------------------------------------------------------------------------------------------------------------------
def test_gpu_fixtures_meet_their_conditions_on_the_cpu_forward():
    """Every case of B >= 64 of tests/replay_votes_cases.py: at h = 0 at least a tenth of the entering rows split on each signal
    tested, each recorded class with at least 5 % of those -- from rule_votes_ref on the oracle's forward, before any GPU run."""
    import replay_votes_cases as rc
    cases = rc.cases()
    assert 36 <= len(cases) <= 44 and len(set(map(rc.case_id, cases))) == len(cases)
    assert {c[4] for c in cases} == {1, 64, 65, 1003} and {c[1] for c in cases} == {3, 7, 8}
    assert {c[3] for c in cases} == {"open_loop", "one_step"} and {c[2] for c in cases} >= set(rc.VOTES)
    checked = 0
    for c in cases:
        kind, E, vm, mode, B, head = c
        if B < 64:
            continue
        dv, cv, entered, rec, targets = rc.first_step_votes(kind, E, B, rc.H, rc.case_id(c), rc.case_inds(c)[0], extra_cols=1 if head else 0,
                                                            learned_cost=head == "cost")
        assert entered.sum() == B - 1                                       # the window that starts at a NaN
        shares = rc.fixture_conditions(kind, E, dv.astype(int), None if cv is None else cv.astype(int), entered, rec["cost"][0] > 0,
                                       targets[0] != 0, head == "cost")
        assert shares
        checked += 1
    assert checked >= 25
