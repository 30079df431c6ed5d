"""GPU: reliability tables of the logistic columns in the model replay -- cmbpo_replay_reliab / _reliab_finish on
crafted arrays and cmbpo_replay_run_reliab / FakeEnv.replay(reliability=True) against a Python loop of FakeEnv.step_device, both
held against the NumPy specification tests/reliability_ref.py; the two feedback paths, FakeEnv.set_cost_recalibration and
ModelSampler.set_term_logit_offset.

Both sides work on the same float32 inputs and choose a bin by comparing a float64 built from them by exact or identically
rounded operations with the edges, so verdicts, bins and every count are compared exactly.  The terms of sum z are the same
numbers on both sides; a sum of n of them added in two different orders differs by at most n 2^-52 sum|z|.  The terms of sum p,
of the Brier sum and of the log loss come from two implementations of exp and log1p, each within 1 ulp, through a few more
correctly rounded operations, all without cancellation (the Brier term is q^2 with q = 1 / (1 + exp(+-z)), never (p - 1)^2; the
log loss adds non-negative parts): a term differs by a few 2^-52 relative, the order adds n 2^-52 sum|term|, and
n 2^-50 sum|term| covers both for the sums of p and of the log loss at every n >= 1, for the Brier sum (whose square doubles a
term's error) wherever the two exponentials do not both sit at the far end of their ulp."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import reliability_ref as rref  # noqa: E402
import replay_calibration_ref as cref  # noqa: E402
import replay_ref as ref  # noqa: E402

DEV = "cuda:0"
F32 = np.float32
PRED = ("next_obs", "rew", "term", "cost", "dkl_path", "ep_var_mean")
REL_ARRAYS = ("part_sum", "part_cnt", "sums", "counts")
TARGET = {rref.COST: "cost", rref.TERM: "term"}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _spec(cols, K, edges=None, terminals=None):
    columns = [dict(name="c%d" % j, col=c, target=TARGET[t], shift=s) for j, (c, t, s) in enumerate(cols)]
    return dict(columns=columns, bins=K, edges=edges, terminals=terminals)


def _check_reliability(rb, want, tag=""):
    """rb: ReplayBuffers after reliab_finish; want: a table of the reference.  Prints the largest error over its bound."""
    from cmbpo_amd import replay
    got_s, got_c = rb.r["sums"].cpu().numpy(), rb.r["counts"].cpu().numpy()
    want_s, want_c = rref.raw_arrays(want)
    np.testing.assert_array_equal(got_c, want_c, err_msg=tag + "counts")
    H, C, _, K = want["n"].shape
    g = got_s.reshape(H, C, 2, 2 * K + 2)
    assert np.isfinite(g).all(), tag
    n = want["n"].astype(np.float64)
    N = n.sum(axis=3)
    worst = 0.0
    for name, got, w, bound in (("sum_z", g[..., K:2 * K], want["sum_z"], n * 2.0 ** -52 * want["abs_z"]),
                                ("sum_p", g[..., :K], want["sum_p"], n * 2.0 ** -50 * want["sum_p"]),
                                ("sum_brier", g[..., 2 * K], want["sum_brier"], N * 2.0 ** -50 * want["sum_brier"]),
                                ("sum_logloss", g[..., 2 * K + 1], want["sum_logloss"], N * 2.0 ** -50 * want["abs_logloss"])):
        err = np.abs(got - w)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)))))
        assert (err <= bound).all(), (tag + name, float(err.max()), got[err > bound], w[err > bound])
    # the derived entries are the host's arithmetic on the raw ones
    tab = rb.reliability_table()
    raw = dict(n=want["n"], pos=want["pos"], sum_p=g[..., :K], sum_z=g[..., K:2 * K], sum_brier=g[..., 2 * K], sum_logloss=g[..., 2 * K + 1])
    for j, name in enumerate(rb.rel_names):
        np.testing.assert_array_equal(tab[name]["n_rel"], want["n_rel"][:, j], err_msg=tag)
        np.testing.assert_array_equal(tab[name]["n_skipped"], want["n_skipped"][:, j], err_msg=tag)
        for r, reading in enumerate(replay.READINGS):
            for k, v in rref.derived(raw, j, r).items():
                np.testing.assert_array_equal(tab[name][reading][k], v, err_msg=tag + k)
    return worst


def _bytes_equal(a, b, keys, where):
    for k in keys:
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=f"{where}: {k}")


# ----------------------------------------------------------------------------------------------------------------------
# 1. the single calls on crafted arrays: no model
# ----------------------------------------------------------------------------------------------------------------------
def _crafted_run(B, E, K, n_cols, O, seed):
    """H = 2 steps of reliab -> compare on made-up predictions and logits, with ragged `alive` on entry, edge-exact logits in the
    first rows, one row of every bad kind at h = 0 and a whole dead slot over poisoned partials; then both finishes.  The columns:
    the last two of out_dim O (a cost column with a shift, a termination column without); one column: the termination column for
    E = 3, else the cost column.  E = 3 also hands the table termination flags of its own.  Returns (buffers, reference table)."""
    from cmbpo_amd.replay import ReplayBuffers
    rng = np.random.default_rng(seed)
    H, A, D = 2, 2, O - 3
    cols = [(O - 2, rref.COST, 0.375), (O - 1, rref.TERM, 0.0)]
    if n_cols == 1:
        cols = cols[1:] if E == 3 else cols[:1]
    edges = rref.default_edges(K)
    obs0 = rng.standard_normal((B, D)).astype(F32)
    rec = dict(next_obs=rng.standard_normal((H, B, D)).astype(F32), rew=rng.standard_normal((H, B)).astype(F32),
               cost=rng.choice(np.array([0.0, 0.4, 0.6, 1.0], F32), (H, B)), term=(rng.random((H, B)) < 0.2).astype(np.uint8))
    own = (rng.random((H, B)) < 0.5).astype(np.uint8) if E == 3 else None
    if own is not None:
        rec["term_target"] = own
    lengths = rng.integers(1, H + 1, B).astype(np.int32)
    rb = ReplayBuffers(obs0, np.zeros((H, B, A), F32), rec["next_obs"], rec["rew"], rec["cost"], rec["term"], lengths=lengths,
                       mode="one_step", ensemble=E, out_dim=O, device=DEV, reliability=_spec(cols, K, terminals=own))
    elite = rng.integers(0, E, (H, B)).astype(np.int32)
    if B >= 16:
        elite[0, 9] = E                                         # no such member
        elite[0, 10] = -1
    rb.set_elite(elite)
    # every entry of every slot is written on every call: whatever the partials held is gone
    rb.r["part_sum"].fill_(float("nan"))
    rb.r["part_cnt"].fill_(-7)
    alive = rng.random(B) < 0.8
    alive[:min(B, 16)] = True
    if B > 128:
        alive[64:128] = False                                   # a slot whose rows are all dead
    rb.t["alive"].copy_(torch.from_numpy(alive.astype(np.uint8)))
    tab, want = ref.new_table(H, D), rref.new_table(H, len(cols), K)
    cur = obs0.copy()
    for h in range(H):
        pred = dict(next_obs=rng.standard_normal((B, D)).astype(F32), rew=rng.standard_normal(B).astype(F32),
                    cost=rng.random(B).astype(F32), term=(rng.random(B) < 0.2).astype(np.uint8),
                    ep_var_mean=rng.random(B).astype(F32), dkl_path=rng.random(B).astype(F32))
        mean = (rng.standard_normal((E, B, O)) * 2.0).astype(F32)
        # edge-exact logits in the first rows, in every member (elite and pooled reading alike): on an edge, one ulp above, one below
        for r in range(min(B, 3 * (K - 1), 9)):
            e = edges[(r // 3 + h) % (K - 1)]
            x = (e, np.nextafter(e, F32(np.inf)), np.nextafter(e, F32(-np.inf)))[r % 3]
            for c, _, s in cols:
                mean[:, r, c] = F32(x + F32(s))                 # (with a shift: wherever float32 puts it, next to the edge)
        if h == 0 and B >= 16:
            other = lambda b: (int(elite[0, b]) + 1) % E        # a member that is not the row's elite (E = 1: the elite)
            mean[other(11), 11, O - 2] = np.nan
            mean[int(elite[0, 12]), 12, O - 1] = np.inf
            mean[other(15), 15, O - 1] = -np.inf
            pred["next_obs"][13, D - 1] = np.nan                # the plain table's n_nonfinite: in neither count here,
            mean[0, 13, O - 1] = np.nan                         # whatever its logits are
            pred["rew"][14] = np.inf
            mean[0, 4, 0] = np.nan                              # a column the table does not read: anything goes there
        if B > 128:
            mean[:, 64:128] = np.nan                            # dead rows: never read
        for k, v in pred.items():
            rb.step_outputs()[k].copy_(torch.from_numpy(v))
        rb.t["mean"].copy_(torch.from_numpy(mean))
        rb.reliab(h)
        rb.compare(h)
        rref.reliab(want, h, alive, pred, mean, rec, elite[h], cols, edges)
        ref.compare(tab, h, cur, alive, pred, rec, lengths, ref.ONE_STEP)
        np.testing.assert_array_equal(rb.t["alive"].cpu().numpy().astype(bool), alive)
    rb.finish()
    rb.reliab_finish()
    torch.cuda.synchronize()
    return rb, want, tab


@pytest.mark.parametrize("E", [1, 3, 8])
@pytest.mark.parametrize("O", [4, 31, 301])
def test_single_calls_on_crafted_arrays(hip_lib, O, E):
    _need_gpu()
    worst = 0.0
    for B in (1, 63, 64, 65, 257):
        for K in (1, 2, 15, 32):
            for n_cols in (1, 2):
                tag = f"B={B} K={K} cols={n_cols} "
                seed = zlib.crc32(f"reliab/{B}/{E}/{K}/{n_cols}/{O}".encode())
                rb, want, plain = _crafted_run(B, E, K, n_cols, O, seed)
                worst = max(worst, _check_reliability(rb, want, tag))
                got = rb.reliability_table()
                plain_got = rb.table()
                np.testing.assert_array_equal(plain_got["n"], plain["n"])
                for j, name in enumerate(rb.rel_names):
                    # the rows of the plain table are those that entered plus those skipped; a non-finite prediction is in neither
                    np.testing.assert_array_equal(got[name]["n_rel"] + got[name]["n_skipped"], plain_got["n"], err_msg=tag)
                    np.testing.assert_array_equal(got[name]["elite"]["n"].sum(axis=1), got[name]["n_rel"], err_msg=tag)
                    np.testing.assert_array_equal(got[name]["pooled"]["n"].sum(axis=1), got[name]["n_rel"], err_msg=tag)
                    if B >= 16:
                        assert got[name]["n_skipped"][0] >= 2 and got[name]["n_skipped"][1] == 0 and got[name]["n_rel"][0] > 0, tag
                if B >= 16:
                    assert plain_got["n_nonfinite"][0] == 2, tag
                    assert sum(int(got[name]["n_skipped"][0]) for name in rb.rel_names) == (7 if n_cols == 2 else 4 if E == 3 else 3), tag
                if B > 128:                                     # the dead slot wrote zeros over the NaN / -7 it held
                    assert not rb.r["part_sum"][:, 1].cpu().numpy().any() and not rb.r["part_cnt"][:, 1].cpu().numpy().any()
                assert np.isfinite(rb.r["part_sum"].cpu().numpy()).all() and (rb.r["part_cnt"].cpu().numpy() >= 0).all()
                if K == 15:
                    again = _crafted_run(B, E, K, n_cols, O, seed)[0]
                    _bytes_equal(rb.r, again.r, REL_ARRAYS, tag + "two runs")
    print("largest error over its bound: %.3f" % worst)


def test_buffers_refuse_what_does_not_fit(hip_lib):
    _need_gpu()
    from cmbpo_amd.replay import ReplayBuffers
    z = lambda *s: np.zeros(s, F32)
    make = lambda rel, E=3, O=4: ReplayBuffers(z(5, 1), z(2, 5, 1), z(2, 5, 1), z(2, 5), z(2, 5), z(2, 5), ensemble=E, out_dim=O,
                                                device=DEV, reliability=rel)
    ok = [dict(name="t", col=3, target="term")]
    for bad, word in ((dict(columns=[]), "1..2 columns"), (dict(columns=ok * 3), "1..2 columns"), (dict(columns=ok, bins=0), "bins"),
                      (dict(columns=ok, bins=33), "bins"), (dict(columns=ok, bins=3, edges=[0.5, 0.5]), "ascending"),
                      (dict(columns=ok, bins=3, edges=[0.0]), "ascending"), (dict(columns=ok, bins=3, edges=[0.0, np.inf]), "ascending"),
                      (dict(columns=[dict(col=4, target="term")]), "outside the model"), (dict(columns=[dict(col=3, target="done")]), "target"),
                      (dict(columns=[dict(col=3, target="term", shift=np.nan)]), "shift"), (dict(columns=ok * 2), "distinct names"),
                      (dict(columns=ok, bin=3), "unknown reliability keys")):
        with pytest.raises(ValueError, match=word):
            make(bad)
    with pytest.raises(ValueError, match="ensemble in 1..8"):
        make(dict(columns=ok), E=9)
    plain = make(None)
    with pytest.raises(ValueError, match="reliability=None"):
        plain.reliab(0)
    with pytest.raises(ValueError, match="reliability=None"):
        plain.reliability_table()


def test_synthetic_calibrated_case_on_the_device(hip_lib):
    """The CPU suite's calibrated case at B = 20 000 through the kernel, same bounds."""
    _need_gpu()
    from cmbpo_amd.replay import ReplayBuffers
    from test_reliability_cpu import _synthetic_tables, check_synthetic
    B, E = 20000, 3
    edges = rref.default_edges(15)

    def on_device(pred, mean, rec, elite):
        z = np.zeros((1, B), F32)
        rb = ReplayBuffers(np.zeros((B, 1), F32), np.zeros((1, B, 1), F32), np.zeros((1, B, 1), F32), z, rec["cost"], rec["term"],
                           mode="one_step", ensemble=E, out_dim=1, device=DEV,
                           reliability=dict(columns=[dict(name="c", col=0, target="term")], bins=15))
        rb.set_elite(elite[None])
        for k in ("p_next_obs", "p_rew", "p_cost"):
            rb.t[k].zero_()
        rb.t["mean"].copy_(torch.from_numpy(mean))
        rb.reliab(0)
        rb.reliab_finish()
        torch.cuda.synchronize()
        want = rref.new_table(1, 1, 15)
        rref.reliab(want, 0, np.ones(B, bool), pred, mean, rec, elite, [(0, rref.TERM, 0.0)], edges)
        _check_reliability(rb, want, "synthetic ")
        got = rb.reliability_table()["c"]
        assert got["n_rel"][0] == B and got["n_skipped"][0] == 0
        return got

    check_synthetic(*_synthetic_tables(on_device))


# ----------------------------------------------------------------------------------------------------------------------
# 2. the whole replay against a loop of FakeEnv.step_device
# ----------------------------------------------------------------------------------------------------------------------
class _Space:
    def __init__(self, d):
        self.shape = (d,)


class _Env:
    def __init__(self, D, A):
        self.observation_space, self.action_space = _Space(D), _Space(A)


_ENVS = {}
COST_SHIFT = 0.2


def _fake_env(E, heads):
    """cref.replay_world's shape (AntSafe's widths, hidden 128, steps of ~0.05 a column) with a logistic cost column, a logistic
    termination column or both behind the reward, their logits spread over a few units."""
    if (E, heads) not in _ENVS:
        from cmbpo_amd import synthetic
        from cmbpo_amd.fake_env import FakeEnv
        from cmbpo_amd.pens import PE
        cost, term = "cost" in heads, "term" in heads
        D, A = synthetic.ENV_DIMS["AntSafe-v2"]
        O = D + 1 + int(cost) + int(term)
        rng = np.random.default_rng(zlib.crc32(f"reliability-model/{E}/{heads}".encode()))
        ws, bs = synthetic.ensemble_weights(rng, E, D + A, 128, 2 * O, bias_scale=0.05)
        mu, var = np.zeros((1, O), F32), np.full((1, O), 2.5e-3, F32)
        if cost:
            mu[0, D + 1], var[0, D + 1] = -0.3, 16.0
        if term:
            mu[0, O - 1], var[0, O - 1] = -1.0, 16.0
        np.random.seed(5)
        model = PE(D + A, O, hidden_dims=(128, 128), num_networks=E, num_elites=max(E - 2, 2), loss="MSPE", use_scaler_in=True,
                   use_scaler_out=True, device=DEV)
        model.set_weights(ws, bs, synthetic.scaler(rng, D + A), (mu, var))
        kw = dict(cost_loss="logistic", cost_logit_shift=COST_SHIFT) if cost else {}
        if term:
            kw.update(predicts_term=True, term_threshold=0.9, term_members="elite", term_loss="logistic")
        _ENVS[E, heads] = (FakeEnv(_Env(D, A), "AntSafe-v2", model, True, True, cost, seed=3, **kw), D, A, O)
    return _ENVS[E, heads]


def _cols(env, D, O):
    return [(c["col"], rref.COST if c["target"] == "cost" else rref.TERM, c["shift"]) for c in env.reliability_columns()]


def _buffers(env, case, mode, calibration, reliability, K=15):
    from cmbpo_amd.replay import ReplayBuffers
    obs0, act, rec, lengths, _ = case
    rel = dict(columns=env.reliability_columns(), bins=K) if reliability else None
    return ReplayBuffers(obs0, act, rec["next_obs"], rec["rew"], rec["cost"], rec["term"], lengths=lengths, mode=mode,
                         ensemble=env._model.num_nets, out_dim=env.output_dim, device=DEV, calibration=calibration, reliability=rel)


def _reference_loop(env, case, mode, cols, K=15):
    """The replay as a Python loop of the existing device step; the plain and the reliability table from the NumPy specifications."""
    obs0, act, rec, lengths, inds = case
    H, B, D = rec["next_obs"].shape
    E, O = env._model.num_nets, env.output_dim
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    f = dict(dtype=torch.float32, device=DEV)
    out = dict(next_obs=torch.empty((B, D), **f), rew=torch.empty(B, **f), term=torch.empty(B, dtype=torch.uint8, device=DEV),
               cost=torch.empty(B, **f), dkl_path=torch.empty(B, **f), ep_var_mean=torch.empty(B, **f))
    scratch = (torch.empty((E, B, O), **f), torch.empty((E, B, O), **f))
    act_d, inds_d = t(act), t(inds)
    tab, want = ref.new_table(H, D), rref.new_table(H, len(cols), K)
    cur, alive = obs0.copy(), np.ones(B, bool)
    edges = rref.default_edges(K)
    for h in range(H):
        env.step_device(t(cur), act_d[h], inds_d[h], out, scratch=scratch)
        pred = {k: out[k].cpu().numpy() for k in PRED}
        rref.reliab(want, h, alive, pred, scratch[0].cpu().numpy(), rec, inds[h], cols, edges)
        ref.compare(tab, h, cur, alive, pred, rec, lengths, mode)
    return tab, want, cur, alive


def _run(rb, env, E, inds_d, calibration, **kw):
    th, ch = env.term_head_struct(), env.cost_head_struct()
    run = rb.run_calibrated if calibration else rb.run
    run(env._model.mlp.handle, env._task_id, E, inds_d, term_head=th, cost_head=ch, **kw)


@pytest.mark.parametrize("calibration", [False, True], ids=["plain", "rc"])
@pytest.mark.parametrize("mode", ["open_loop", "one_step"])
@pytest.mark.parametrize("heads", ["cost", "term", "cost+term"])
@pytest.mark.parametrize("E", [3, 7])
def test_run_reliab_matches_the_step_device_loop(hip_lib, E, heads, mode, calibration):
    _need_gpu()
    env, D, A, O = _fake_env(E, heads)
    cols = _cols(env, D, O)
    assert len(cols) == 1 + ("+" in heads) and cols[-1][0] == O - 1
    shared = ("sums", "counts", "part_sum", "part_cnt", "cur_obs", "alive")
    for B in (65, 257):
        for H in (1, 3):
            tag = f"B={B} H={H} "
            rng = np.random.default_rng(zlib.crc32(f"reliab-whole/{E}/{heads}/{mode}/{B}/{H}".encode()))
            case = cref.recording(rng, B, H, D, A) + (rng.integers(0, E, (H, B)).astype(np.int32),)
            inds_d = torch.from_numpy(case[4]).to(DEV)
            a = _buffers(env, case, mode, calibration, True)
            _run(a, env, E, inds_d, calibration)
            torch.cuda.synchronize()
            tab, want, cur, alive = _reference_loop(env, case, mode, cols)
            _check_reliability(a, want, tag)
            assert (want["n_skipped"] == 0).all() and (want["n_rel"][0] == B).all(), tag      # (the reference alone decides this)
            np.testing.assert_array_equal(want["n_rel"], np.repeat(tab["n"][:, None], len(cols), axis=1), err_msg=tag)
            np.testing.assert_array_equal(a.t["cur_obs"].cpu().numpy().view(np.uint32), cur.view(np.uint32), err_msg=tag)
            np.testing.assert_array_equal(a.t["alive"].cpu().numpy().astype(bool), alive, err_msg=tag)
            assert (want["n"][0].max(axis=-1) < B).all() and (want["pos"][0].sum(axis=-1) > 0).all(), tag    # more than one bin, both classes
            # cmbpo_replay_run_cost on the same inputs: the tables they share and the final state, bit for bit
            p = _buffers(env, case, mode, calibration, False)
            _run(p, env, E, inds_d, calibration)
            _bytes_equal(a.t, p.t, shared, tag + "run_cost")
            if calibration:
                _bytes_equal(a.c, p.c, ("sums", "counts", "part_sum", "part_cnt"), tag + "run_cost, calibration")
            # ... and buffers that own the arrays and are told to leave them alone make that very call
            q = _buffers(env, case, mode, calibration, True)
            _run(q, env, E, inds_d, calibration, reliability=False)
            _bytes_equal(q.t, p.t, shared, tag + "reliability=False")
            assert not q.r["counts"].cpu().numpy().any()
            # the single calls, bit for bit; a second run
            c = _buffers(env, case, mode, calibration, True)
            c.set_elite(inds_d)
            for h in range(H):
                env.step_device(c.t["cur_obs"], c.t["act"][h], inds_d[h], c.step_outputs(), scratch=(c.t["mean"], c.t["var"]))
                if calibration:
                    c.calibrate(h)
                c.reliab(h)
                c.compare(h)
            c.finish()
            if calibration:
                c.calib_finish()
            c.reliab_finish()
            b = _buffers(env, case, mode, calibration, True)
            _run(b, env, E, inds_d, calibration)
            torch.cuda.synchronize()
            for other, where in ((c, "single calls"), (b, "two runs")):
                _bytes_equal(a.r, other.r, REL_ARRAYS, tag + where)
                _bytes_equal(a.t, other.t, ("sums", "counts", "cur_obs", "alive"), tag + where)
                if calibration:
                    _bytes_equal(a.c, other.c, ("sums", "counts"), tag + where)


def test_fake_env_replay_with_and_without_reliability(hip_lib):
    _need_gpu()
    E = 7
    env, D, A, O = _fake_env(E, "cost+term")
    rng = np.random.default_rng(21)
    B, H = 130, 4
    case = cref.recording(rng, B, H, D, A) + (rng.integers(0, E, (H, B)).astype(np.int32),)
    obs0, act, rec, lengths, inds = case
    args = (obs0, act, rec["next_obs"], rec["rew"], rec["cost"], rec["term"])
    plain = _buffers(env, case, "open_loop", False, False)
    _run(plain, env, E, torch.from_numpy(inds).to(DEV), False)
    want = plain.table()
    off = env.replay(*args, lengths=lengths, model_inds=inds)
    explicit_off = env.replay(*args, lengths=lengths, model_inds=inds, reliability=False)
    on = env.replay(*args, lengths=lengths, model_inds=inds, reliability=True)
    both = env.replay(*args, lengths=lengths, model_inds=inds, reliability=True, calibration=True, reliability_bins=7)
    assert sorted(off) == sorted(explicit_off) == sorted(want) and "reliability" not in off
    assert sorted(on) == sorted(list(want) + ["reliability"]) and sorted(both) == sorted(list(want) + ["calibration", "reliability"])
    for k in want:
        for got in (off, explicit_off, on, both):
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    rel = on["reliability"]
    assert sorted(rel) == ["cost", "term"] and sorted(both["reliability"]) == ["cost", "term"]
    direct = _buffers(env, case, "open_loop", False, True)
    _run(direct, env, E, torch.from_numpy(inds).to(DEV), False)
    _, want_rel, _, _ = _reference_loop(env, case, "open_loop", _cols(env, D, O))
    _check_reliability(direct, want_rel)
    for name, col in direct.reliability_table().items():
        for reading in ("elite", "pooled"):
            for k, v in col[reading].items():
                np.testing.assert_array_equal(rel[name][reading][k], v, err_msg=k)
        np.testing.assert_array_equal(rel[name]["n_rel"] + rel[name]["n_skipped"], want["n"])
        assert rel[name]["elite"]["n"].shape == (H, 15) and both["reliability"][name]["elite"]["n"].shape == (H, 7)
        np.testing.assert_array_equal(both["reliability"][name]["n_rel"], rel[name]["n_rel"])
    # the termination flags of the table's own move the termination column alone
    own = 1 - rec["term"]
    moved = env.replay(*args, lengths=lengths, model_inds=inds, reliability=True, reliability_terminals=own)
    for k in want:
        np.testing.assert_array_equal(moved[k], want[k], err_msg=k)
    np.testing.assert_array_equal(moved["reliability"]["cost"]["elite"]["pos"], rel["cost"]["elite"]["pos"])
    np.testing.assert_array_equal(moved["reliability"]["term"]["elite"]["pos"], rel["term"]["elite"]["n"] - rel["term"]["elite"]["pos"])
    # the recalibration offset moves the imagined cost and not the table
    env.set_cost_recalibration(0.7)
    try:
        shifted = env.replay(*args, lengths=lengths, model_inds=inds, reliability=True)
    finally:
        env.set_cost_recalibration(0.0)
    assert not np.array_equal(shifted["se_cost"], want["se_cost"])
    np.testing.assert_array_equal(shifted["reliability"]["cost"]["elite"]["sum_p"][0], rel["cost"]["elite"]["sum_p"][0])
    # the generator of the replay's own elite draws is used the same way by both forms
    state = env._replay_rng.bit_generator.state
    first = env.replay(*args, lengths=lengths)
    env._replay_rng.bit_generator.state = state
    second = env.replay(*args, lengths=lengths, reliability=True)
    for k in want:
        np.testing.assert_array_equal(first[k], second[k], err_msg=k)
    # an ensemble of more than eight members is refused in words, a Gaussian model too
    genv = cref_env()
    with pytest.raises(ValueError, match="a Gaussian column is not a logit"):
        genv.replay(*args, lengths=lengths, reliability=True)


def cref_env():
    """A FakeEnv without a logistic head (the calibration tests' world, learned cost as a magnitude)."""
    from test_replay_calibration_gpu import _fake_env as gaussian_env
    return gaussian_env(3, True)[0]


# ----------------------------------------------------------------------------------------------------------------------
# 3. the two offsets
# ----------------------------------------------------------------------------------------------------------------------
def test_cost_recalibration_is_the_shift_plus_the_offset_bit_for_bit(hip_lib):
    _need_gpu()
    E = 3
    env, D, A, O = _fake_env(E, "cost")
    rng = np.random.default_rng(5)
    n = 200
    obs = (rng.standard_normal((n, D)) * 0.1).astype(F32)
    obs[:, 0] = 0.5
    act = rng.uniform(-1, 1, (n, A)).astype(F32)
    inds = rng.integers(0, E, n).astype(np.int32)
    base = env.step(obs, act, model_inds=inds)
    bits = lambda x: np.ascontiguousarray(x, F32).view(np.uint32)
    try:
        for b in (0.3, -1.1, 1e-3):
            env.set_cost_recalibration(b)
            got = env.step(obs, act, model_inds=inds)
            env.set_cost_recalibration(0.0)
            back = env.step(obs, act, model_inds=inds)
            want_shift = float(F32(COST_SHIFT + b))
            env.set_cost_head(logit_shift=want_shift)
            want = env.step(obs, act, model_inds=inds)
            env.set_cost_head(logit_shift=COST_SHIFT)
            np.testing.assert_array_equal(bits(got[3]["cost"]), bits(want[3]["cost"]))
            np.testing.assert_array_equal(bits(back[3]["cost"]), bits(base[3]["cost"]))          # the default gives the old bits
            assert not np.array_equal(got[3]["cost"], base[3]["cost"])
            np.testing.assert_array_equal(bits(got[3]["cost_logit"]), bits(base[3]["cost_logit"]))   # the raw logit is what it was
            np.testing.assert_array_equal(bits(got[0]), bits(base[0]))
    finally:
        env.set_cost_recalibration(0.0)
        env.set_cost_head(logit_shift=COST_SHIFT)
    # a rollout pool picks the sum up at reset()
    import test_cost_head_gpu as tc
    import test_term_head_gpu as tt
    sampler, pool, fe = tc._hip_world(tt.build_world_term(31, term=False), 40, 0.25, False)
    fe.set_cost_recalibration(0.4)
    sampler.reset(tt._start(3, 40))
    assert pool.cost_head == ("logistic", float(F32(0.25 + 0.4)))
    fe.set_cost_recalibration(0.0)
    sampler.reset(tt._start(3, 40))
    assert pool.cost_head == ("logistic", 0.25)


def test_term_logit_offset_shifts_the_sampled_thresholds(hip_lib):
    """A sampling sampler with an offset against a loop of sample() over a sampler without one whose chunks of thresholds are
    shifted by hand (NumPy float32, one rounding per element) as they are drawn -- explicit term_draws= carry draws, not thresholds,
    and are never shifted --, across a chunk boundary, bit for bit."""
    _need_gpu()
    import test_term_draws_gpu as td
    B, T, b = 96, 48, 0.8
    w = td.build_world(21, 512, bias=float(np.log(0.03 / 0.97)))
    start = td._start(22, B)

    def roll(offset=None, by_hand=None, explicit=None):
        sampler, pool, env = td.hip_world(w, B, T, True, seed=7)
        if offset != "unset":
            sampler.set_term_logit_offset(offset)
        sampler.reset(start)
        seen, steps, last = set(), 0, None
        while steps < T and sampler.any_alive() and pool.has_room:
            if by_hand is not None:
                ck = sampler._next_draws()[0]                     # the chunk the step is about to use, not advanced
                if ck is not last:                                # (held on to: a later chunk cannot be mistaken for it)
                    last = ck
                    seen.add(len(seen) + 1)
                    thr = ck[4].cpu().numpy()
                    assert np.isfinite(thr).all() or np.isposinf(thr[~np.isfinite(thr)]).all()
                    ck[4].copy_(torch.from_numpy((thr + F32(by_hand)).astype(F32)).to(DEV))
            else:
                seen.add(0)
            if explicit is not None:
                sampler.sample(term_draws=explicit[steps][:pool.n_alive])
            else:
                sampler.sample()
            if by_hand is None and explicit is None:
                seen.add(sampler._draws[4].data_ptr())
            steps += 1
        ln = pool.t["len"].cpu().numpy().copy()
        sampler.finish_all_paths()
        return [np.ascontiguousarray(r.cpu().numpy() if isinstance(r, torch.Tensor) else r) for r in pool.get()[0]], ln, steps, len(seen), sampler

    same = lambda x, y: all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(x, y))
    base, len_base, steps, chunks, smp = roll("unset")
    assert steps > smp._draws[1].shape[0] and chunks >= 3, (steps, chunks)      # (0 and two chunks' addresses)
    assert same(base, roll(None)[0]) and same(base, roll(0.0)[0])                # None or 0.0: exactly the calls it made
    assert same(base, roll("unset", by_hand=0.0)[0])                             # the loop with hand-made chunks is the same rollout
    got, len_got, steps_got, _, smp = roll(b)
    assert smp.term_logit_offset == b
    want, len_want, _, chunks_want, _ = roll("unset", by_hand=b)
    assert chunks_want >= 2 and steps_got > smp._draws[1].shape[0]
    np.testing.assert_array_equal(len_got, len_want)
    assert same(got, want) and not same(got, base)
    assert len_got.sum() > len_base.sum()                                         # a positive offset lowers the hazard: longer branches
    # explicit draws are never shifted
    u = 1.0 - np.random.default_rng(3).random((T, B), dtype=F32)
    assert same(roll(b, explicit=u)[0], roll("unset", explicit=u)[0])
    # the same offset again keeps the chunk in hand, another one drops it
    smp._next_draws()
    chunk = smp._draws
    smp.set_term_logit_offset(b)
    assert smp._draws is chunk
    smp.set_term_logit_offset(b + 0.5)
    assert smp._draws is None
