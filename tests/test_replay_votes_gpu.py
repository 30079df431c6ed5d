"""GPU: the static rules' votes in the model replay -- the single calls (forward, cmbpo_fakeenv_post_votes,
cmbpo_replay_votes, cmbpo_replay_compare) against the NumPy specification tests/replay_votes_ref.py step by step, from read-backs of
the device's own mean / var / cur_obs; cmbpo_replay_run_votes against those single calls, against cmbpo_replay_run_reliab under
the measure-only vote and against itself, bit for bit; the plain table's verdict counts against the histogram on the device.

Everything compared is an integer, a bit pattern, or (the host's derived table) a float64 function of integers to 1e-12.  The
worlds, recordings and the pruned product of cases live in tests/replay_votes_cases.py; the fixture conditions -- at h = 0 a tenth
of the entering rows split on every signal tested, each recorded class with 5 % of those -- are asserted from the reference's own
output on every case of B >= 64: a case that misses them fails."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import replay_ref as ref  # noqa: E402
import replay_votes_cases as rc  # noqa: E402
import replay_votes_ref as vtref  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
PRED = ("next_obs", "rew", "term", "cost", "dkl_path", "ep_var_mean")
PLAIN = ("sums", "counts", "part_sum", "part_cnt", "cur_obs", "alive")
TABLE = ("sums", "counts", "part_sum", "part_cnt")
PRED_ARRAYS = ("p_next_obs", "p_rew", "p_term", "p_cost", "p_dkl_path", "p_ep_var_mean")
_ENVS = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class _Space:
    def __init__(self, d):
        self.shape = (d,)


class _Env:
    def __init__(self, D, A):
        self.observation_space, self.action_space = _Space(D), _Space(A)


def _fake_env(kind, E, head):
    """The world of tests/replay_votes_cases.py on the device: head None, 'term' (a thresholded Gaussian termination column, the
    head's own vote 'majority') or 'cost' (a learned cost read as a magnitude)."""
    if (kind, E, head) not in _ENVS:
        from cmbpo_amd.fake_env import FakeEnv
        from cmbpo_amd.pens import PE
        ws, bs, sc_in, sc_out, D, A, O = rc.world(kind, E, 1 if head else 0)
        np.random.seed(5)
        model = PE(D + A, O, hidden_dims=(128, 128), num_networks=E, num_elites=max(E - 2, 2), loss="MSPE", use_scaler_in=True,
                   use_scaler_out=True, device=DEV)
        model.set_weights(ws, bs, sc_in, sc_out)
        kw = dict(predicts_term=True, term_threshold=0.5, term_members="majority") if head == "term" else {}
        _ENVS[kind, E, head] = (FakeEnv(_Env(D, A), rc.task_of(kind), model, True, True, head == "cost", seed=3, static_votes=True, **kw),
                                D, A, O)
    return _ENVS[kind, E, head]


def _bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x).view(np.uint8)


def _bytes_equal(a, b, keys, where):
    for k in keys:
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{where}: {k}")


def _buffers(env, data, mode, E, O, votes=None, tables=False):
    """votes: None or (done_members, cost_members, terminals); tables: also the calibration table and a reliability table (of the
    reward column held against the recorded cost: any column serves the kernel as a logit)."""
    from cmbpo_amd.replay import ReplayBuffers
    obs0, act, rec, lengths, _ = data
    spec = None if votes is None else dict(done_members=votes[0], cost_members=votes[1], learned_cost=env._predicts_cost,
                                           terminals=votes[2])
    rel = dict(columns=[dict(name="r", col=env.obs_dim, target="cost")], bins=7) if tables else None
    return ReplayBuffers(obs0, act, rec["next_obs"], rec["rew"], rec["cost"], rec["term"], lengths=lengths, mode=mode, ensemble=E,
                         out_dim=O, device=DEV, calibration=tables, reliability=rel, votes=spec)


def _run_votes(rb, env, E, inds_d, **kw):
    rb.run_votes(env._model.mlp.handle, env._task_id, E, inds_d, term_head=env.term_head_struct(), cost_head=env.cost_head_struct(), **kw)


def _step_outputs(rb, env):
    """The dict FakeEnv.step_device fills: the replay's prediction arrays, the vote arrays and the head's two outputs."""
    out = rb.step_outputs()
    out.update(static_term_votes=rb.v["done_votes"], static_cost_votes=None if env._predicts_cost else rb.v["cost_votes"])
    if env.predicts_term:
        out.update(rb.head_scratch)
    return out


@pytest.mark.parametrize("case", rc.cases(), ids=rc.case_id)
def test_replay_under_the_vote(hip_lib, case):
    _need_gpu()
    from test_replay_votes_cpu import check_table
    kind, E, (dm, cm), mode, B, head = case
    H = rc.H
    env, D, A, O = _fake_env(kind, E, head)
    env.set_static_votes(dm, cm, True)
    learned_cost = head == "cost"
    data = rc.recording(kind, B, H, rc.case_id(case))
    obs0, act, rec, lengths, targets = data
    inds = rc.case_inds(case)
    inds_d = torch.from_numpy(inds).to(DEV)
    tag = rc.case_id(case) + " "

    # 1. the single calls, step by step against the reference --------------------------------------------------------
    a = _buffers(env, data, mode, E, O, votes=(dm, cm, targets))
    a.v["part_cnt"].fill_(-7)                                   # every entry of every slot is written on every call
    out = _step_outputs(a, env)
    seen = {}

    def forward(h, cur):
        np.testing.assert_array_equal(_bits(a.t["cur_obs"]), _bits(cur), err_msg=tag + f"cur_obs on entry to h = {h}")
        env.step_device(a.t["cur_obs"], a.t["act"][h], inds_d[h], out, scratch=(a.t["mean"], a.t["var"]))
        seen.update(term=a.t["p_term"].cpu().numpy(), cost=a.t["p_cost"].cpu().numpy(), dv=a.v["done_votes"].cpu().numpy(),
                    cv=None if learned_cost else a.v["cost_votes"].cpu().numpy())
        return {k: out[k].cpu().numpy() for k in PRED}, a.t["mean"].cpu().numpy(), a.t["var"].cpu().numpy()

    def learned_done(h, mean):
        with np.errstate(invalid="ignore"):
            return 2 * (mean[:, :, O - 1] > F32(0.5)).sum(axis=0) > E          # the head's 'majority' of `x > threshold`

    def after_step(h, step):
        m = tag + f"h = {h}: "
        np.testing.assert_array_equal(seen["term"], step["pred"]["term"], err_msg=m + "p_term")
        np.testing.assert_array_equal(_bits(seen["cost"]), _bits(np.asarray(step["pred"]["cost"], F32)), err_msg=m + "p_cost")
        np.testing.assert_array_equal(seen["dv"], step["done_votes"], err_msg=m + "done_votes")
        if not learned_cost:
            np.testing.assert_array_equal(seen["cv"], step["cost_votes"], err_msg=m + "cost_votes")
        a.votes(h)
        a.compare(h)
        np.testing.assert_array_equal(a.t["alive"].cpu().numpy().astype(bool), step["alive"], err_msg=m + "alive")

    with np.errstate(all="ignore"):
        plain, vt, cur, alive, steps = vtref.replay_votes(forward, rc.task_of(kind), obs0, act, rec, lengths, inds, mode, E, D, dm, cm,
                                                          learned_done=learned_done if head == "term" else None,
                                                          learned_cost=learned_cost, term=targets, after_step=after_step)
    a.finish()
    a.votes_finish()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(a.t["cur_obs"]), _bits(cur), err_msg=tag + "cur_obs")
    got_c = a.t["counts"].cpu().numpy()
    np.testing.assert_array_equal(got_c[:, 0], plain["n"], err_msg=tag + "n")
    np.testing.assert_array_equal(got_c[:, 1], plain["n_nonfinite"], err_msg=tag + "n_nonfinite")
    np.testing.assert_array_equal(got_c[:, 2:6].reshape(H, 2, 2), plain["cost_cm"], err_msg=tag + "cost_cm")
    np.testing.assert_array_equal(got_c[:, 6:10].reshape(H, 2, 2), plain["term_cm"], err_msg=tag + "term_cm")
    np.testing.assert_array_equal(a.v["counts"].cpu().numpy(), vtref.raw_counts(vt), err_msg=tag + "vote table")
    assert (a.v["part_cnt"].cpu().numpy() >= 0).all(), tag
    check_table(a.votes_table(), vt, E, learned_cost)
    np.testing.assert_array_equal(vt["n_vote"], plain["n"])                 # the vote kernel never writes a count above E
    assert not vt["n_skipped"].any() and vt["n_vote"][0] == B - int(B >= 64), tag      # (the window that starts at a NaN)
    if B >= 64:
        assert plain["n_nonfinite"][0] == 1, tag
        s0 = steps[0]
        shares = rc.fixture_conditions(kind, E, s0["done_votes"].astype(int), None if learned_cost else s0["cost_votes"].astype(int),
                                       s0["entered"], rec["cost"][0] > 0, targets[0] != 0, learned_cost)
        print(tag, shares)

    # 2. the run entry is bitwise those single calls; 5. two runs are bitwise equal -------------------------------------
    b = _buffers(env, data, mode, E, O, votes=(dm, cm, targets))
    _run_votes(b, env, E, inds_d)
    c = _buffers(env, data, mode, E, O, votes=(dm, cm, targets))
    _run_votes(c, env, E, inds_d)
    torch.cuda.synchronize()
    _bytes_equal(a.t, b.t, PLAIN, tag + "run against the single calls")
    _bytes_equal(a.v, b.v, ("part_cnt", "counts"), tag + "run against the single calls")
    _bytes_equal(b.t, c.t, PLAIN + PRED_ARRAYS, tag + "two runs")
    _bytes_equal(b.v, c.v, ("part_cnt", "counts", "done_votes") + (() if learned_cost else ("cost_votes",)), tag + "two runs")

    # 3. under the measure-only vote every other table is cmbpo_replay_run_reliab's ------------------------------------
    if (dm, cm) == ("elite", "elite"):
        p = _buffers(env, data, mode, E, O, tables=True)
        p.run_calibrated(env._model.mlp.handle, env._task_id, E, inds_d, term_head=env.term_head_struct(), cost_head=env.cost_head_struct())
        q = _buffers(env, data, mode, E, O, votes=(dm, cm, targets), tables=True)
        _run_votes(q, env, E, inds_d, calibration=True)
        torch.cuda.synchronize()
        _bytes_equal(q.t, p.t, PLAIN, tag + "measure only, plain")
        _bytes_equal(q.c, p.c, TABLE, tag + "measure only, calibration")
        _bytes_equal(q.r, p.r, TABLE, tag + "measure only, reliability")
        _bytes_equal(q.v, a.v, ("counts",), tag + "measure only, the vote table beside the other two")
        assert p.r["counts"].cpu().numpy().any() and p.c["counts"].cpu().numpy().any(), tag

    # 4. on the device: the plain table's positives are the histogram's sums for the mode ------------------------------
    if head is None and (dm, cm) != ("elite", "elite"):
        d = _buffers(env, data, mode, E, O, votes=(dm, cm, None))          # the recorded flags are the table's own
        _run_votes(d, env, E, inds_d)
        torch.cuda.synchronize()
        tab, votes = d.table(), d.votes_table()
        np.testing.assert_array_equal(tab["n"], votes["n_vote"], err_msg=tag)
        cost_mode = "majority" if cm == "mean" else cm                     # p_cost > 0.5 of the share is the strict majority
        np.testing.assert_array_equal(tab["cost_cm"][:, :, 1], votes["cost"]["cm"][cost_mode][:, :, 1], err_msg=tag + "cost_cm")
        np.testing.assert_array_equal(tab["term_cm"][:, :, 1], votes["term"]["cm"][dm][:, :, 1], err_msg=tag + "term_cm")
        np.testing.assert_array_equal(tab["cost_cm"], votes["cost"]["cm"][cost_mode], err_msg=tag + "cost_cm")
        _bytes_equal(d.t, a.t, PLAIN, tag + "the table's own flags do not move the replay")
        if B >= 64:
            assert tab["cost_cm"][0, :, 1].sum() > 0 and (kind == "hcs" or tab["term_cm"][0, :, 1].sum() > 0), tag


def test_the_vote_changes_what_the_replay_measures(hip_lib):
    """The point of the feature, on one world: under 'any' the plain table reports more costs and ends open-loop windows earlier
    than under the elite's rule, and the measure-only vote changes nothing but the histogram."""
    _need_gpu()
    kind, E, B = "ant", 7, 1003
    env, D, A, O = _fake_env(kind, E, None)
    data = rc.recording(kind, B, rc.H, "changes")
    inds_d = torch.from_numpy(np.random.default_rng(4).integers(0, E, (rc.H, B)).astype(np.int32)).to(DEV)
    tabs = {}
    for dm, cm in (("elite", "elite"), ("any", "any"), ("majority", "mean")):
        rb = _buffers(env, data, "open_loop", E, O, votes=(dm, cm, None))
        _run_votes(rb, env, E, inds_d)
        tabs[dm] = (rb.table(), rb.votes_table())
    plain = _buffers(env, data, "open_loop", E, O)
    plain.run(env._model.mlp.handle, env._task_id, E, inds_d)
    for k, v in plain.table().items():
        np.testing.assert_array_equal(tabs["elite"][0][k], v, err_msg=k)
    e, a, m = (tabs[k][0] for k in ("elite", "any", "majority"))
    assert a["cost_cm"][0, :, 1].sum() > e["cost_cm"][0, :, 1].sum() and a["term_cm"][0, :, 1].sum() > e["term_cm"][0, :, 1].sum()
    assert a["n"][1] < e["n"][1]                                            # the worst case ends more windows
    np.testing.assert_array_equal(tabs["any"][1]["cost"]["hist"][0], tabs["elite"][1]["cost"]["hist"][0])     # h = 0: the same rows
    # under 'mean' the squared error of the cost is the Brier score of the share, from the same integers
    np.testing.assert_allclose(m["mse_cost"][0], tabs["majority"][1]["cost"]["brier"][0], rtol=1e-6)


def test_fake_env_replay_with_and_without_votes(hip_lib):
    _need_gpu()
    kind, E, B, H = "table29", 7, 130, rc.H
    env, D, A, O = _fake_env(kind, E, None)
    data = rc.recording(kind, B, H, "fake-env")
    obs0, act, rec, lengths, targets = data
    inds = np.random.default_rng(2).integers(0, E, (H, B)).astype(np.int32)
    args = (obs0, act, rec["next_obs"], rec["rew"], rec["cost"], rec["term"])
    env.set_static_votes("any", "mean", False)
    off = env.replay(*args, lengths=lengths, model_inds=inds)
    explicit_off = env.replay(*args, lengths=lengths, model_inds=inds, votes=False)
    measure = env.replay(*args, lengths=lengths, model_inds=inds, votes="measure", calibration=True)
    on = env.replay(*args, lengths=lengths, model_inds=inds, votes=True, reliability_terminals=targets)
    assert "votes" not in off and sorted(off) == sorted(explicit_off)
    assert sorted(measure) == sorted(list(off) + ["calibration", "votes"]) and sorted(on) == sorted(list(off) + ["votes"])
    for k in off:
        np.testing.assert_array_equal(explicit_off[k], off[k], err_msg=k)
        np.testing.assert_array_equal(measure[k], off[k], err_msg=k)           # the elite's rule, as without votes
    assert not np.array_equal(on["cost_cm"], off["cost_cm"]) and not np.array_equal(on["term_cm"], off["term_cm"])
    direct = _buffers(env, data, "open_loop", E, O, votes=("any", "mean", targets))
    _run_votes(direct, env, E, torch.from_numpy(inds).to(DEV))
    want, want_v = direct.table(), direct.votes_table()
    for k in want:
        np.testing.assert_array_equal(on[k], want[k], err_msg=k)
    for sig in ("cost", "term"):
        for k in ("hist", "n", "ece", "brier", "split_rate"):
            np.testing.assert_array_equal(on["votes"][sig][k], want_v[sig][k], err_msg=sig + k)
        assert on["votes"][sig]["split_rate"][0] >= 0.1
    np.testing.assert_array_equal(on["votes"]["cost"]["hist"][0], measure["votes"]["cost"]["hist"][0])
    # the generator of the replay's own elite draws is used the same way by every form
    state = env._replay_rng.bit_generator.state
    first = env.replay(*args, lengths=lengths)
    env._replay_rng.bit_generator.state = state
    second = env.replay(*args, lengths=lengths, votes="measure")
    for k in off:
        np.testing.assert_array_equal(first[k], second[k], err_msg=k)
    env.set_static_votes("elite", "elite", False)
    try:
        with pytest.raises(ValueError, match="votes=True needs the static votes on"):
            env.replay(*args, lengths=lengths, votes=True)
        assert "votes" in env.replay(*args, lengths=lengths, votes="measure")
    finally:
        env.set_static_votes("elite", "elite", True)
