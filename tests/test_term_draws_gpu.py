"""GPU: sampled terminations -- the post kernel's DRAW instances against tests/term_draws_ref.py bit for bit and
against cmbpo_fakeenv_post_cost on everything the thresholds do not touch; the thresholds along imagined rollouts (the native loop
against the one-call step against the host mirror, across a draw-chunk boundary); the sampler's streams; the one statistical test
(a column that says 0.3 ends 30 % of the branches); and two epochs of the trainer.

Everything but the rate is comparisons of bits.  The rate's bound is five standard deviations of a binomial share, derived below."""
import ctypes as C
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import term_draws_ref as ref  # noqa: E402

DEV = "cuda:0"
NAMES = ["obs", "act", "adv", "cadv", "ret", "cret", "logp", "val", "cval", "cost", "log_std", "mu"]
MODES = ("elite", "any", "majority")
SLOTS = 300
F_OUT = ("next_obs", "rew", "cost", "dkl_path", "ep_var_mean", "ep_var", "rew_var", "cost_var", "term_pred", "cost_logit")
U8_OUT = ("term", "term_votes")
INF, NAN = np.float32(np.inf), np.float32(np.nan)


class _Space:
    def __init__(self, d):
        self.shape = (d,)


class _Env:
    def __init__(self, D, A):
        self.observation_space, self.action_space = _Space(D), _Space(A)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


# ------------------------------------------------------------------------------------------------------------------
# 1. the post kernel
# ------------------------------------------------------------------------------------------------------------------
class _Post:
    """The inputs of one post step on the device, uploaded once; run() makes one call of cmbpo_fakeenv_post_term_draws (or, with
    entry='cost', of cmbpo_fakeenv_post_cost with the same leading arguments) into outputs that start at a sentinel."""

    def __init__(self, obs, act, mean, var, inds, rows, D, A):
        dev = torch.device(DEV)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.B, self.E, self.D, self.A, self.n = obs.shape[0], mean.shape[0], D, A, len(rows)
        self.d = [t(obs), t(act), t(mean), t(var), t(inds), t(np.asarray(rows, np.int32))]

    def run(self, task_arg, xi=None, kappa=None, head=None, logistic_cost=False, thr=None, entry="draws"):
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
            th.threshold, th.members = head[0], ref.MEMBERS[head[1]]
            th.term_pred, th.term_votes = _lib.ptr(out["term_pred"]), _lib.ptr(out["term_votes"])
        ch = None
        if logistic_cost:
            ch = _lib.CostHeadStruct()
            ch.kind, ch.logit_shift, ch.cost_logit = _lib.COST_LOGISTIC, 0.25, _lib.ptr(out["cost_logit"])
        kr, kc = kappa if kappa is not None else (0.0, 0.0)
        d = self.d
        args = [task_arg, self.E, D, self.A, _lib.ptr(d[2]), _lib.ptr(d[3]), B, _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[4]),
                _lib.ptr(d[5]), None, self.n, _lib.ptr(out["next_obs"]), _lib.ptr(out["rew"]), _lib.ptr(out["term"]),
                _lib.ptr(out["cost"]), _lib.ptr(out["dkl_path"]), _lib.ptr(out["ep_var_mean"]), _lib.ptr(out["ep_var"]),
                _lib.ptr(keep[0]), float(kr), float(kc), _lib.ptr(out["rew_var"]) if kappa is not None else None,
                _lib.ptr(out["cost_var"]) if kappa is not None else None, None if th is None else C.byref(th),
                None if ch is None else C.byref(ch)]
        if entry == "draws":
            rc = _lib.lib().cmbpo_fakeenv_post_term_draws(*args, _lib.ptr(keep[1]), _lib.current_stream())
        else:
            assert thr is None
            rc = _lib.lib().cmbpo_fakeenv_post_cost(*args, _lib.current_stream())
        torch.cuda.synchronize()
        assert rc == 0, (rc, _lib.lib().cmbpo_last_error())
        return {k: v.cpu().numpy() for k, v in out.items()}


_TABLES = {}


def _task_arg(kind, learned):
    from cmbpo_amd import _lib
    if kind == "default":
        tid = _lib.TASK_DEFAULT
    elif kind == "antsafe":
        tid = _lib.TASK_ANTSAFE
    else:
        if not _TABLES:      # two registered tables for the module (the slots are a process-wide resource)
            from cmbpo_amd.statics import TaskRules, cost, healthy, tilt
            _TABLES["table"] = TaskRules([healthy(cols=0, lo=0.2, hi=1.5), cost(cols=-1, abs=True, lo=0.4, lo_strict=True)],
                                         require_finite=True, cost_on_term=True)
            _TABLES["derived"] = TaskRules([healthy(src="derived", cols=0, lo=-0.7), cost(cols=-1, abs=True, lo=0.4, lo_strict=True)],
                                           derived=[tilt(2, 3)], require_finite=True, cost_on_term=True)
        tid = _TABLES[kind].task_id
    return tid | (_lib.TASK_LEARNED_COST if learned else 0)


def _inputs(rng, E, D, A, n, learned):
    """Means drawn directly over SLOTS slots, `n` of them listed in a scattered, unsorted row list; the termination column is
    0.35 + 0.3 z_row + 0.15 z_member and the thresholds are draws u in (0, 1] in the column's units (the 'gaussian' reading)."""
    from cmbpo_amd.utils import term_thresholds
    O = D + 1 + int(learned) + 1
    B = SLOTS
    obs = (rng.standard_normal((B, D)) * 0.1).astype(np.float32)
    obs[:, 0] = rng.uniform(0.3, 0.9, B).astype(np.float32)
    act = rng.uniform(-1, 1, (B, A)).astype(np.float32)
    mean = (rng.standard_normal((E, B, O)) * 0.3).astype(np.float32)
    var = np.exp(rng.uniform(-12, 1, (E, B, O))).astype(np.float32)
    mean[:, :, (0, 2, 3)], var[:, :, (0, 2, 3)] = 0.0, 1e-6       # z and the quaternion stay where obs put them, with or without xi
    z_row, z_mem = rng.standard_normal(B).astype(np.float32), rng.standard_normal((E, B)).astype(np.float32)
    mean[:, :, O - 1] = np.float32(0.35) + np.float32(0.3) * z_row[None] + np.float32(0.15) * z_mem
    inds = rng.integers(0, E, size=B).astype(np.int32)
    rows = rng.permutation(B)[:n].astype(np.int32)
    obs[rows[1::4], 0] = 5.0                      # outside the table's healthy band: its rule ends the row
    obs[rows[2::4], 2] = 1.0                      # q1 = 1 at a healthy height: z_rot = -1 < -0.7, AntSafe and the tilt quantity end it
    thr = term_thresholds(1.0 - rng.random(B, dtype=np.float32), "gaussian")
    assert thr.dtype == np.float32 and (thr > 0).all() and (thr <= 1).all()
    return obs, act, mean, var, inds, rows, thr, O


def _plant(mean, thr, inds, rows, E):
    """The special values of tests/test_term_draws_cpu.py in the first rows of the list (as many as the list has)."""
    tc = mean.shape[2] - 1
    oth = lambda r, k=1: (inds[r] + k) % E
    plans = []

    def plan(fn):
        plans.append(fn)

    @plan
    def at_the_threshold(r):                      # x == thr does not hit
        mean[:, r, tc], thr[r] = 0.25, 0.25

    @plan
    def elite_alone(r):                           # the elite hits, nobody else
        mean[:, r, tc], thr[r] = 0.1, 0.5
        mean[inds[r], r, tc] = 0.9

    @plan
    def all_but_the_elite(r):
        mean[:, r, tc], thr[r] = 0.9, 0.5
        mean[inds[r], r, tc] = 0.1

    @plan
    def nan_x(r):                                 # the elite's NaN never hits, the others do
        mean[:, r, tc], thr[r] = 0.9, 0.5
        mean[inds[r], r, tc] = NAN

    @plan
    def nan_thr(r):                               # a NaN threshold: nobody hits, +inf included
        mean[:, r, tc], thr[r] = 0.9, NAN
        mean[oth(r), r, tc] = INF

    @plan
    def minus_inf_thr(r):                         # hits every non-NaN x, -inf excepted
        mean[:, r, tc], thr[r] = -3.0e38, -INF
        mean[oth(r), r, tc] = -INF
        if E > 2:
            mean[oth(r, 2), r, tc] = NAN

    @plan
    def plus_inf_thr(r):                          # never hits, +inf included
        mean[:, r, tc], thr[r] = 3.0e38, INF
        mean[inds[r], r, tc] = INF

    @plan
    def minus_inf_both(r):
        mean[:, r, tc], thr[r] = -INF, -INF

    for fn, r in zip(plans, rows):
        fn(int(r))
    return min(len(plans), len(rows))


# E = 7 at every row count (a row's eight lanes: 7, 8, 9; a wave's eight rows and a workgroup's edge: 31, 32, 33; many workgroups:
# 257), every ensemble size at 33 rows.  The entry points take ensembles of 2..8 members (an ensemble of one has no pair to
# measure a KL on: refused below), so 2 stands for the smallest; 3 and 8 run the kernel's run-time-sized instance, 7 its own.
_SHAPES = [(7, n) for n in (1, 7, 8, 9, 31, 32, 33, 257)] + [(E, 33) for E in (2, 3, 8)]


@pytest.mark.parametrize("E,n", _SHAPES)
def test_post_kernel_against_the_reference(hip_lib, E, n):
    """default / AntSafe / a clause table / a table with a derived quantity x xi NULL / given x disagreement off / on (kappa 0 and
    > 0) x the logistic cost head off / on, for every vote: term, term_pred and term_votes are the reference's bit for bit, every
    other output is cmbpo_fakeenv_post_cost's on the same inputs bit for bit, unlisted slots keep their sentinels."""
    _need_gpu()
    D, A = 8, 3
    for logistic_cost in (False, True):
        learned = logistic_cost                   # (the logistic cost head and kappa_cost > 0 need the learned-cost column)
        rng = np.random.default_rng(zlib.crc32(f"{E}/{n}/{learned}/term-draws".encode()))
        obs, act, mean, var, inds, rows, thr, O = _inputs(rng, E, D, A, n, learned)
        planted = _plant(mean, thr, inds, rows, E)
        assert planted == min(n, 8)
        post = _Post(obs, act, mean, var, inds, rows, D, A)
        narrow = _Post(obs, act, np.ascontiguousarray(mean[..., :O - 1]), np.ascontiguousarray(var[..., :O - 1]), inds, rows, D, A)
        xi_draws = rng.standard_normal((SLOTS, D)).astype(np.float32)
        rest = np.setdiff1d(np.arange(SLOTS), rows)
        sub = np.ascontiguousarray(mean[:, rows])
        for kind in ("default", "antsafe", "table", "derived"):
            task_arg = _task_arg(kind, learned)
            for xi in (None, xi_draws):
                for kappa in (None, (0.0, 0.0), (0.75, 1.5 if learned else 0.0)):
                    tag = f"{kind} cost_head={logistic_cost} xi={xi is not None} kappa={kappa}"
                    # the rule's own verdict: the head-off launch over the narrower copy of the means
                    rule = narrow.run(task_arg, xi, kappa, None, logistic_cost, entry="cost")["term"][rows]
                    assert (rule <= 1).all()
                    if kind == "default":
                        assert not rule.any(), tag
                    elif n >= 31:
                        assert rule.any() and not rule.all(), tag
                    for m in MODES:
                        on = post.run(task_arg, xi, kappa, (0.5, m), logistic_cost, thr)
                        scalar = post.run(task_arg, xi, kappa, (0.5, m), logistic_cost, entry="cost")
                        term, pred, votes = ref.term_draws(sub, inds[rows], thr[rows], m, rule_done=rule)
                        np.testing.assert_array_equal(on["term"][rows], term, err_msg=f"{tag} {m} term")
                        np.testing.assert_array_equal(_bits(on["term_pred"][rows]), _bits(pred), err_msg=f"{tag} {m} term_pred")
                        np.testing.assert_array_equal(on["term_votes"][rows], votes, err_msg=f"{tag} {m} term_votes")
                        for k in F_OUT:          # (the sentinels of what is off and of the unlisted slots included)
                            np.testing.assert_array_equal(_bits(on[k]), _bits(scalar[k]), err_msg=f"{tag} {m} {k}")
                        assert (on["term"][rest] == 77).all() and (on["term_votes"][rest] == 77).all(), tag
                        assert (on["term_pred"][rest] == -7.0).all() and (on["next_obs"][rest] == -7.0).all(), tag
                    if n >= 31 and kind == "default":
                        # the draws do something the scalar rule does not, and the planted rows are where they were planted
                        assert (on["term"][rows] != scalar["term"][rows]).any(), tag
                        assert on["term_votes"][rows[0]] == 0 and on["term_votes"][rows[4]] == 0 and on["term_votes"][rows[6]] == 0
                        assert on["term_votes"][rows[5]] == E - 1 - (E > 2) and on["term_votes"][rows[7]] == 0


def test_an_ensemble_of_one_is_refused_as_it_always_was(hip_lib):
    _need_gpu()
    from cmbpo_amd import _lib
    rng = np.random.default_rng(5)
    obs, act, mean, var, inds, rows, thr, _ = _inputs(rng, 1, 8, 3, 33, False)
    post = _Post(obs, act, mean, var, inds, rows, 8, 3)
    for entry, who in (("draws", b"cmbpo_fakeenv_post_term_draws"), ("cost", b"cmbpo_fakeenv_post_term")):
        with pytest.raises(AssertionError):
            post.run(_lib.TASK_DEFAULT, head=(0.5, "elite"), thr=thr if entry == "draws" else None, entry=entry)
        msg = hip_lib.cmbpo_last_error()
        assert msg.startswith(who + b": ensemble 1 not in [2, 8]"), msg


@pytest.mark.parametrize("E", [7, 3])
def test_null_draws_and_a_constant_threshold_are_the_scalar_rule(hip_lib, E):
    """d_term_thr == NULL is cmbpo_fakeenv_post_cost's call, and an array filled with th->threshold is the scalar rule: the same
    bits in every output, with and without every other feature."""
    _need_gpu()
    D, A, n = 8, 3, 33
    for learned in (False, True):
        rng = np.random.default_rng(zlib.crc32(f"{E}/{learned}/null-draws".encode()))
        obs, act, mean, var, inds, rows, _, O = _inputs(rng, E, D, A, n, learned)
        mean[:, rows[0], O - 1] = 0.5                                    # exactly the threshold
        post = _Post(obs, act, mean, var, inds, rows, D, A)
        xi_draws = rng.standard_normal((SLOTS, D)).astype(np.float32)
        const = np.full(SLOTS, 0.5, np.float32)
        for kind in ("antsafe", "derived"):
            for xi, kappa, m in ((None, None, "elite"), (xi_draws, (0.5, 0.25 if learned else 0.0), "majority"), (xi_draws, None, "any")):
                for head in (None, (0.5, m)):
                    cost = post.run(_task_arg(kind, learned), xi, kappa, head, learned, entry="cost")
                    null = post.run(_task_arg(kind, learned), xi, kappa, head, learned, thr=None)
                    for k in F_OUT + U8_OUT:
                        np.testing.assert_array_equal(_bits(null[k]), _bits(cost[k]), err_msg=f"{kind} {head} NULL {k}")
                scalar = post.run(_task_arg(kind, learned), xi, kappa, (0.5, m), learned, thr=const)
                assert set(cost["term"][rows].tolist()) == {0, 1} and cost["term_votes"][rows].max() > 0
                for k in F_OUT + U8_OUT:
                    np.testing.assert_array_equal(_bits(scalar[k]), _bits(cost[k]), err_msg=f"{kind} constant {k}")


# ------------------------------------------------------------------------------------------------------------------
# 2. the rollout
# ------------------------------------------------------------------------------------------------------------------
OBS, ACT, ENS = 6, 2, 3
LOGIT_SPREAD = 40.0        # on the termination column's output weights: the logits then spread over about a unit


def build_world(seed, hidden, bias, spread=LOGIT_SPREAD):
    """A default-task world (no rule ends anything) of OBS x ACT with an ensemble of ENS hidden x hidden members whose LAST column is
    the logistic termination head: logit = spread * (the drawn column) + bias.  spread 0: the column says sigma(bias) everywhere."""
    from cmbpo_amd import synthetic
    rng = np.random.default_rng(seed)
    out_dim = OBS + 2
    ws, bs = synthetic.ensemble_weights(rng, ENS, OBS + ACT, hidden, 2 * out_dim, bias_scale=0.05)
    ws[2][:, :, out_dim - 1] *= spread
    bs[2][:, :, out_dim - 1] = bias
    sc_in = synthetic.scaler(rng, OBS + ACT, hit_clamp=False)
    mu, var = synthetic.scaler(rng, out_dim, hit_clamp=False)
    pol = synthetic.policy_params(rng, OBS, ACT)
    crit = []
    for _ in range(2):
        cw, cb = synthetic.ensemble_weights(rng, 3, OBS, 128, 1, bias_scale=0.05)
        crit.append((cw, cb, synthetic.scaler(rng, OBS, hit_clamp=False), synthetic.scaler(rng, 1, hit_clamp=False)))
    return dict(hidden=hidden, out_dim=out_dim, ws=ws, bs=bs, sc_in=sc_in, sc_out=(mu, (var * 0.01).astype(np.float32)), pol=pol,
                v=crit[0], vc=crit[1], elites=[0, 2])


def hip_world(w, B, T, term_sampling, seed=0, threshold=0.5):
    from cmbpo_amd.cpo_policy import CPOPolicy
    from cmbpo_amd.fake_env import FakeEnv
    from cmbpo_amd.model_sampler import ModelSampler
    from cmbpo_amd.modelbuffer import ModelBuffer
    from cmbpo_amd.pens import PE
    model = PE(OBS + ACT, w["out_dim"], hidden_dims=(w["hidden"], w["hidden"]), num_networks=ENS, num_elites=len(w["elites"]),
               loss="MSPE", use_scaler_in=True, use_scaler_out=True, device=DEV, logistic_columns=[-1])
    model.set_weights(w["ws"], w["bs"], w["sc_in"], w["sc_out"])
    model.set_elites(w["elites"])
    policy = CPOPolicy(_Space(OBS), _Space(ACT), a_hidden_layer_sizes=(128, 128), vf_hidden_layer_sizes=(128, 128),
                       vf_ensemble_size=3, vf_elites=2, vf_activation="swish", vf_loss="MSE", device=DEV,
                       cost_gamma=0.97, cost_lam=0.5, lam=0.95)
    policy.actor.set_params(w["pol"])
    policy.v.set_weights(*w["v"])
    policy.vc.set_weights(*w["vc"])
    env = FakeEnv(_Env(OBS, ACT), "default", model, predicts_delta=True, predicts_rew=True, predicts_cost=False, predicts_term=True,
                  term_threshold=threshold, term_members="elite", term_loss="logistic")
    pool = ModelBuffer(B, OBS, ACT, T, device=DEV)
    pool.initialize(policy.pi_info_shapes, gamma=0.99, lam=0.95, cost_gamma=0.97, cost_lam=0.5)
    sampler = ModelSampler(max_path_length=T + 5, batch_size=B, rollout_mode="uncertainty", seed=seed, term_sampling=term_sampling)
    sampler.initialize(env, policy, pool)
    sampler.set_rollout_dkl(float("inf"))
    return sampler, pool, env


def _start(seed, B):
    return (np.random.default_rng(seed).standard_normal((B, OBS)) * 0.1).astype(np.float32)


_STATE = ("len", "alive", "fin_code", "path_ret", "path_cost", "path_dyn_var", "dkl_acc", "cur_obs", "term_t",
          "term_pred_t", "term_votes_t", "rew_t", "cost_t", "v_t", "vc_t")


def _roll(w, start, how, steps, T, thr=None, seed=0):
    """One rollout of at most `steps` steps with a sampling sampler: 'many' is one sample_many (cmbpo_rollout_run with the chunk's
    thresholds attached and B as the stride), 'loop' a loop of sample() (cmbpo_rollout_step, the thresholds attached again per
    step), 'host' the same loop through the host mirror (FakeEnv.step_device(term_thr=) and the separate bookkeeping entries).
    thr [steps, B]: put into the sampler's chunk in place of its own thresholds."""
    B = start.shape[0]
    sampler, pool, env = hip_world(w, B, T, True, seed=seed)
    sampler.reset(start)
    if how == "host":
        env.kernel_events = []
    chunks = set()
    if thr is not None:
        ck = sampler._draw_chunk()
        assert ck[4].shape[0] >= steps and ck[4].shape[1] == B
        ck[4][:steps].copy_(torch.from_numpy(thr).to(DEV))
    per_step = []
    if how == "many":
        done, _ = sampler.sample_many(max_steps=steps)
        chunk_len = sampler._draws[1].shape[0]
    else:
        done = 0
        while done < steps and sampler.any_alive() and pool.has_room:
            ids = pool.t["alive_idx"][:pool.n_alive].cpu().numpy().copy()
            sampler.sample()
            chunks.add(sampler._draws[4].data_ptr())
            per_step.append((ids, pool.t["term_t"].cpu().numpy()[ids].copy()))
            done += 1
        chunk_len = sampler._draws[1].shape[0]
    torch.cuda.synchronize()
    state = {k: pool.t[k].cpu().numpy().copy() for k in _STATE}
    state["alive_list"] = pool.t["alive_idx"][:pool.n_alive].cpu().numpy().copy()
    # the step's counters and the accumulators (CMBPO_I_N_ALIVE .. _N_FIN_POST, CMBPO_D_TOTAL_SAMPLES .. _TOTAL_VC_VAR; the words
    # behind them are the look-ahead's own)
    state["iscal"], state["dscal"] = pool.t["iscal"][:7].cpu().numpy().copy(), pool.t["dscal"][:17].cpu().numpy().copy()
    state["counters"] = np.array([done, pool.n_alive, pool.ptr, pool.size, sampler._total_samples])
    sampler.finish_all_paths()
    return dict(state=state, get=pool.get()[0], per_step=per_step, chunks=len(chunks), chunk_len=chunk_len, steps=done)


def _equal(a, b, what):
    for k in a["state"]:
        np.testing.assert_array_equal(_bits(a["state"][k]), _bits(b["state"][k]), err_msg=f"{what}: {k}")
    for k, x, y in zip(NAMES, a["get"], b["get"]):
        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=f"{what}: get() {k}")


def test_native_loop_equals_the_step_equals_the_host_loop(hip_lib):
    """B = 96, 12 steps, [12, B] thresholds: cmbpo_rollout_run (step j reads d_thr + j * B) against 12 calls of cmbpo_rollout_step
    (d_thr attached again per step), bit for bit on every buffer and counter; both against the host loop of
    FakeEnv.step_device(term_thr=) on term_t, the alive list, ptr and the path lengths."""
    _need_gpu()
    from cmbpo_amd.utils import term_thresholds
    B, steps, T = 96, 12, 16
    w = build_world(11, 512, bias=float(np.log(0.1 / 0.9)))             # a hazard of about one in ten per step
    start = _start(12, B)
    thr = term_thresholds(1.0 - np.random.default_rng(13).random((steps, B), dtype=np.float32), "logistic")
    loop = _roll(w, start, "loop", steps, T, thr)
    many = _roll(w, start, "many", steps, T, thr)
    host = _roll(w, start, "host", steps, T, thr)
    assert loop["steps"] == many["steps"] == host["steps"] == steps
    # some branches end on every step, on the head's word (the default task has no rule), and most do not
    ended = [int(term.sum()) for _, term in loop["per_step"]]
    assert all(e > 0 for e in ended), ended
    assert len(loop["state"]["alive_list"]) >= B // 8 and sum(ended) >= B // 2, ended
    _equal(loop, many, "run / step")
    for (ids_a, term_a), (ids_b, term_b) in zip(loop["per_step"], host["per_step"]):
        np.testing.assert_array_equal(ids_a, ids_b)
        np.testing.assert_array_equal(term_a, term_b)
    for k in ("len", "alive", "fin_code", "term_t", "alive_list", "counters"):
        np.testing.assert_array_equal(loop["state"][k], host["state"][k], err_msg=f"step / host: {k}")
    # other thresholds, another rollout: the draws are what ends the branches
    other = _roll(w, start, "many", steps, T, np.ascontiguousarray(thr[::-1]))
    assert not np.array_equal(other["state"]["len"], many["state"]["len"])


def test_sample_many_equals_a_loop_of_sample_across_a_chunk_boundary(hip_lib):
    """The sampler's own draws, more steps than a chunk holds: the native loop re-attaches the next chunk's thresholds where the
    per-step path does, and one seed gives one rollout."""
    _need_gpu()
    B, T = 96, 48
    w = build_world(21, 512, bias=float(np.log(0.03 / 0.97)))           # a low hazard: a quarter of the branches outlive a chunk
    start = _start(22, B)
    loop = _roll(w, start, "loop", T, T, seed=7)
    many = _roll(w, start, "many", T, T, seed=7)
    again = _roll(w, start, "many", T, T, seed=7)
    other = _roll(w, start, "many", T, T, seed=8)
    assert loop["steps"] == many["steps"] > loop["chunk_len"] and loop["chunks"] >= 2, (loop["steps"], loop["chunk_len"], loop["chunks"])
    assert sum(int(term.sum()) for _, term in loop["per_step"]) >= B // 4
    _equal(loop, many, "sample_many / sample")
    _equal(many, again, "one seed, one rollout")
    assert not np.array_equal(other["state"]["len"], many["state"]["len"])


def test_the_draws_move_nobody_elses_random_numbers(hip_lib):
    """A termination column at -inf (zero weights, bias -inf): nothing ever hits, and the sampling sampler's rollout is the plain
    sampler's bit for bit -- eps, the elite picks and the chunk boundaries are what they were."""
    _need_gpu()
    B, T = 96, 48
    w = build_world(31, 512, bias=-np.inf, spread=0.0)
    start = _start(32, B)
    res = {}
    for sampling in (False, True):
        sampler, pool, _ = hip_world(w, B, T, sampling, seed=3)
        sampler.reset(start)
        steps, _ = sampler.sample_many()
        assert (sampler._term_gen is not None) == sampling and (sampler._draws[4] is not None) == sampling
        ck = sampler._draws
        state = {k: pool.t[k].cpu().numpy().copy() for k in _STATE if k not in ("term_pred_t",)}
        state["eps"], state["inds"] = ck[1].cpu().numpy().copy(), ck[2].cpu().numpy().copy()
        assert not state["term_t"].any() and steps > ck[1].shape[0]          # nobody ended; the rollout crossed a chunk boundary
        sampler.finish_all_paths()
        res[sampling] = dict(state=state, get=pool.get()[0], steps=steps)
    assert res[False]["steps"] == res[True]["steps"]
    _equal(res[False], res[True], "sampling / plain")


# ------------------------------------------------------------------------------------------------------------------
# 3. the rate
# ------------------------------------------------------------------------------------------------------------------
def test_a_column_that_says_three_in_ten_ends_three_in_ten(hip_lib):
    """Zero weights and bias logit(0.3) on the termination column, the default task, 4096 branches, one step.  The ended share is
    a binomial share with p = 0.3, n = 4096: standard deviation sqrt(0.3 * 0.7 / 4096) = 0.00716, and the bound is five of them,
    0.036 (a fixed seed makes the test deterministic; the bound is derived, not tuned).  The threshold rule at 0.5 ends none."""
    _need_gpu()
    B, p = 4096, 0.3
    bound = 5.0 * np.sqrt(p * (1 - p) / B)
    assert abs(bound - 0.036) < 5e-4
    w = build_world(41, 128, bias=float(np.log(p / (1 - p))), spread=0.0)
    start = _start(42, B)
    terms = []
    for sampling in (True, True, False):
        sampler, pool, _ = hip_world(w, B, 4, sampling, seed=17)
        sampler.reset(start)
        sampler.sample()
        torch.cuda.synchronize()
        terms.append(pool.t["term_t"].cpu().numpy().copy())
        assert pool.n_alive == B - int(terms[-1].sum())
        # the column says 0.3 everywhere: the forward's means are good to 2e-4 (the smoke test's bound), which moves sigma by
        # 0.21 * 2e-4 -- three orders of magnitude inside the bound below
        pred = 1.0 / (1.0 + np.exp(-pool.t["term_pred_t"].cpu().numpy().astype(np.float64)))
        assert np.abs(pred - p).max() < 1e-3, np.abs(pred - p).max()
    share = float(terms[0].mean())
    print("sampled terminations: share %.4f of %d branches ended at p = %.1f (bound +- %.4f)" % (share, B, p, bound))
    assert abs(share - p) <= bound, (share, bound)
    np.testing.assert_array_equal(terms[0], terms[1])                          # one seed, one set of draws
    assert not terms[2].any()                                                  # 0.3 < 0.5: the classifier ends nobody


# ------------------------------------------------------------------------------------------------------------------
# 4. the trainer
# ------------------------------------------------------------------------------------------------------------------
BOX = 0.5


class BoxPointEnv:
    """The 2-D point mass of tests/test_term_head_cmbpo_gpu.py: obs = [pos, vel, sin / cos of a clock], reward = -|pos|; the
    episode ends when the mass leaves the box |pos|_inf <= 0.5 -- a rule no task of statics.py knows, so under task='default' an
    imagined branch ends before the horizon only on the model's word."""

    def __init__(self, seed=0):
        self.observation_space, self.action_space = _Space(6), _Space(2)
        self.rng = np.random.RandomState(seed)
        self.t = 0

    def _obs(self):
        return np.concatenate([self.pos, self.vel, [np.sin(0.1 * self.t), np.cos(0.1 * self.t)]]).astype(np.float32)

    def reset(self):
        self.pos, self.vel, self.t = self.rng.uniform(-0.3, 0.3, 2), np.zeros(2), 0
        return self._obs()

    def step(self, a):
        a = np.clip(np.asarray(a, np.float64).reshape(-1)[:2], -1, 1)
        self.vel = 0.9 * self.vel + 0.3 * a + 0.01 * self.rng.standard_normal(2)
        self.pos = self.pos + 0.2 * self.vel
        self.t += 1
        return self._obs(), -float(np.abs(self.pos).sum()), bool(np.abs(self.pos).max() > BOX), {"cost": 0.0}

    def close(self):
        pass


def run_box_loop(keys, seed=0, epochs=2):
    """`epochs` epochs of CMBPO(m_learn_term=True, m_term_loss='logistic', **keys) on BoxPointEnv through utils.build_experiment,
    every generator seeded."""
    from cmbpo_amd import synthetic
    from cmbpo_amd.utils import build_experiment
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    env = BoxPointEnv(seed=seed + 1)
    env.max_episode_steps = 40
    kwargs = {
        'n_env_interacts': 10 ** 9, 'eval_every_n_steps': 1, 'use_model': True, 'm_train_freq': 100, 'm_networks': 4, 'm_elites': 3,
        'm_hidden_dims': (128, 128), 'rollout_batch_size': 400, 'rollout_mode': 'schedule', 'rollout_schedule': [0, 1, 5, 5],
        'maxroll': 6, 'initial_real_samples_per_epoch': 400, 'min_real_samples_per_epoch': 400, 'batch_size_policy': 2400,
        'n_initial_exploration_steps': 2000, 'n_epochs': epochs, 'm_validate_horizon': 3, 'm_validate_windows': 1024,
        'initial_model_train_kwargs': dict(min_epochs=40, max_epochs=60, batch_size=128),
        'model_train_kwargs': dict(min_epochs=1, max_epochs=2, batch_size=128),
        'm_learn_term': True, 'm_term_threshold': 0.5, 'm_term_members': 'elite', 'm_term_loss': 'logistic'}
    kwargs.update(keys)
    params = {
        'universe': 'gym', 'task': 'default', 'environment_params': {'normalize_actions': True},
        'algorithm_params': {'type': 'CMBPO', 'kwargs': kwargs},
        'policy_params': {'type': 'cpopolicy', 'kwargs': {
            'a_hidden_layer_sizes': (128, 128), 'vf_lr': 1e-3, 'vf_hidden_layer_sizes': (128, 128), 'vf_epochs': 2,
            'vf_batch_size': 256, 'vf_ensemble_size': 3, 'vf_elites': 2, 'vf_activation': 'swish', 'vf_loss': 'MSE',
            'target_kl': 0.01, 'cost_lim': 5.0}},
        'buffer_params': {'kwargs': {'size': 2600, 'archive_size': 12000}}, 'sampler_params': {'kwargs': {}},
        'run_params': {},
    }
    algo = build_experiment(params, env, device="cuda:0")
    algo._policy.set_params(synthetic.policy_params(np.random.default_rng(seed + 2), 6, 2, 128))
    rng = np.random.RandomState(seed + 3)
    algo._policy.v.init_weights(rng)
    algo._policy.vc.init_weights(rng)
    seen = dict(term_share=[])        # the real termination rate of each fit's samples
    train0 = algo._model.train

    def train(x, y, *a, **k):
        seen["term_share"].append(float(y[:, -1].mean()))
        return train0(x, y, *a, **k)

    algo._model.train = train
    diags = [d for d in algo.train()]
    assert len(diags) >= 1 and algo.policy_epoch == epochs
    return algo, seen, diags


def imagined_rollout(algo, steps=5, n=400):
    """One imagined rollout from archived states with the trainer's own sampler, pool and FakeEnv: per step the slots stepped, the
    step's term and logit, and the alive mask behind the step."""
    sampler, pool = algo.model_sampler, algo.model_buf
    start = algo._buffer.get_archive(['observations'])['observations'][:n]
    sampler.set_max_path_length(steps + 1)      # (a path of max_path_length L stores L - 1 steps)
    sampler.reset(start)
    out = []
    cp = lambda x: x.cpu().numpy().copy()
    for _ in range(steps):
        if not sampler.any_alive():
            break
        ids = cp(pool.t["alive_idx"][:pool.n_alive])
        sampler.sample()
        out.append(dict(ids=ids, term=cp(pool.t["term_t"])[ids], pred=cp(pool.t["term_pred_t"])[ids],
                        alive=np.asarray(pool.alive_paths).astype(bool).copy()))
    sampler.finish_all_paths()
    pool.get()
    return out


def test_sampled_terminations_in_the_trainer(hip_lib, tmp_path):
    _need_gpu()
    algo, seen, diags = run_box_loop(dict(m_term_sampling=True))
    assert all(0.02 < s < 0.3 for s in seen["term_share"]), seen["term_share"]     # the targets hold the real terminations
    env, sampler = algo.fake_env, algo.model_sampler
    assert sampler.term_sampling and algo._m_term_sampling and env.term_loss == "logistic" and env.predicts_term
    assert sampler._term_gen is not None
    # the threshold and the vote stay in force for the validation replay, which keeps the classifier's reading
    assert algo.model_buf.term_head == (0.0, "elite") and env.term_threshold == 0.5
    assert np.isfinite(diags[-1]['model/val_term_recall_h1'])
    # info['term_pred'] stays a probability
    obs = algo._buffer.get_archive(['observations'])['observations'][:64]
    act = np.zeros((64, 2), np.float32)
    _, _, terms, info = env.step(obs, act, term_draws=np.full(64, 1.0, np.float32))
    assert ((info["term_pred"] >= 0) & (info["term_pred"] <= 1)).all() and not terms.any()      # u = 1: +inf, nobody ends
    # some imagined branch ends where the rule did not end it (the default task has no rule), and where the classifier would not
    ended = below = 0
    for st in imagined_rollout(algo)[:-1]:
        gone = ~st["alive"][st["ids"]]
        ended += int(gone.sum())
        below += int((st["pred"][gone] <= 0.0).sum())
        assert (st["term"][gone] == 1).all() and not st["term"][~gone].any()
    print("sampled terminations in the trainer: %d imagined branches ended before the horizon, %d of them on a probability <= 0.5"
          % (ended, below))
    assert ended > 0, "no imagined branch ended before the horizon"
    # policy and model stay finite
    assert np.isfinite(algo._policy.actor.get_flat_params()).all()
    ws, bs = algo._model.get_weights()
    assert all(np.isfinite(a).all() for a in ws + bs)
    # the flag survives save / load: a trainer built with the default reads it from the file of its own
    from cmbpo_amd.cmbpo import CMBPO
    from cmbpo_amd.cpo_policy import CPOPolicy
    from cmbpo_amd.cpo_sampler import CpoSampler
    from cmbpo_amd.cpobuffer import CPOBuffer
    algo.save(str(tmp_path))
    benv = BoxPointEnv(seed=5)
    policy = CPOPolicy(benv.observation_space, benv.action_space, a_hidden_layer_sizes=(128, 128), vf_hidden_layer_sizes=(128, 128),
                       vf_ensemble_size=3, vf_elites=2, vf_activation="swish", vf_loss="MSE", device="cuda:0", max_path_length=40)
    b = CMBPO(benv, policy, CPOBuffer(600, 6000, benv.observation_space, benv.action_space), sampler=CpoSampler(max_path_length=40),
              task="default", m_networks=4, m_elites=3, m_hidden_dims=(128, 128), rollout_batch_size=100, maxroll=6, m_learn_term=True)
    assert not b.model_sampler.term_sampling and b.model_sampler._term_gen is None
    b.load(str(tmp_path), algo._epoch)
    assert b.model_sampler.term_sampling and b._m_term_sampling and b.fake_env.term_loss == "logistic"


def test_sampling_off_is_the_run_that_never_named_the_key(hip_lib):
    _need_gpu()
    plain, _, _ = run_box_loop({})
    named, _, _ = run_box_loop(dict(m_term_sampling=False))
    for a in (plain, named):
        assert not a.model_sampler.term_sampling and a.model_sampler._term_gen is None and not a.model_sampler._thr_attached
        assert a.model_sampler._draws is None or a.model_sampler._draws[4] is None
    np.testing.assert_array_equal(plain._policy.actor.get_flat_params(), named._policy.actor.get_flat_params())
    for x, y in zip(sum(plain._model.get_weights(), []), sum(named._model.get_weights(), [])):
        np.testing.assert_array_equal(x, y)
    # ... where the classifier ends a branch only above its threshold
    for st in imagined_rollout(plain)[:-1]:
        gone = ~st["alive"][st["ids"]]
        assert (st["pred"][gone] > 0.0).all() and (st["pred"][~gone] <= 0.0).all()
