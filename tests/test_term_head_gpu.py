"""GPU: the learned termination head -- the post kernel's TERM instances against tests/term_head_ref.py and against
a head-off launch over the narrower copy of the means, then the head along imagined rollouts (the native loop against the
per-step call, a trace against a host loop, two shards over gloo), in the replay, and on the f16 paths of the widest shipped
shape.

The head is comparisons and counts: everything it decides is compared exactly.  In the trace tests the threshold is the midpoint
of the widest usable gap between the values the column takes along the trace (at least 1e-3 wide, asserted), so that no
difference between two forward kernels' roundings can move a value across it."""
import ctypes as C
import os
import socket
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import replay_ref  # noqa: E402
import term_head_ref as ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
NAMES = ["obs", "act", "adv", "cadv", "ret", "cret", "logp", "val", "cval", "cost", "log_std", "mu"]
CLASSIC = ("next_obs", "rew", "cost", "dkl_path", "ep_var_mean", "ep_var")
MODES = ("elite", "any", "majority")
THR = 0.5


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
def _run_term(task_arg, obs, act, mean, var, inds, D, A, rows=None, xi=None, kappa=None, head=None, optional=True,
              entry="cmbpo_fakeenv_post_term"):
    """cmbpo_fakeenv_post_term on slot-indexed arrays; with `rows` only the listed slots are stepped.  kappa: None -- no
    disagreement (NULL arrays, both coefficients 0); head: None -- th == NULL, or (threshold, members).  Every output starts at a
    sentinel.  entry: a narrower entry point instead, with the leading part of the same arguments that it takes."""
    from cmbpo_amd import _lib
    dev = torch.device(DEV)
    B, E = obs.shape[0], mean.shape[0]
    n = B if rows is None else len(rows)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    f = dict(dtype=torch.float32, device=dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    out = dict(next_obs=torch.full((B, D), -7.0, **f), rew=torch.full((B,), -7.0, **f), term=torch.full((B,), 77, **u8),
               cost=torch.full((B,), -7.0, **f), dkl_path=torch.full((B,), -7.0, **f), ep_var_mean=torch.full((B,), -7.0, **f),
               ep_var=torch.full((B, D), -7.0, **f), rew_var=torch.full((B,), -7.0, **f), cost_var=torch.full((B,), -7.0, **f),
               term_pred=torch.full((B,), -7.0, **f), term_votes=torch.full((B,), 77, **u8))
    d = [t(obs), t(act), t(mean), t(var), t(inds)]
    ri = None if rows is None else t(np.asarray(rows, np.int32))
    d_xi = None if xi is None else t(xi)
    th = None
    if head is not None:
        th = _lib.TermHeadStruct()
        th.threshold, th.members = head[0], ref.MEMBERS[head[1]]
        th.term_pred = _lib.ptr(out["term_pred"]) if optional else None
        th.term_votes = _lib.ptr(out["term_votes"]) if optional else None
    kr, kc = kappa if kappa is not None else (0.0, 0.0)
    args = [
        task_arg, E, D, A, _lib.ptr(d[2]), _lib.ptr(d[3]), B, _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[4]), _lib.ptr(ri), None, n,
        _lib.ptr(out["next_obs"]), _lib.ptr(out["rew"]), _lib.ptr(out["term"]), _lib.ptr(out["cost"]), _lib.ptr(out["dkl_path"]),
        _lib.ptr(out["ep_var_mean"]), _lib.ptr(out["ep_var"]), _lib.ptr(d_xi), float(kr), float(kc),
        _lib.ptr(out["rew_var"]) if kappa is not None else None, _lib.ptr(out["cost_var"]) if kappa is not None else None,
        None if th is None else C.byref(th)]
    take = {"cmbpo_fakeenv_post": 20, "cmbpo_fakeenv_post_noise": 21, "cmbpo_fakeenv_post_disagreement": 25, "cmbpo_fakeenv_post_term": 26}
    assert all(a is None or a == 0.0 for a in args[take[entry]:]), "the entry point cannot express this call"
    rc = getattr(_lib.lib(), entry)(*args[:take[entry]], _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, _lib.lib().cmbpo_last_error())
    return {k: v.cpu().numpy() for k, v in out.items()}


_TABLE = []


def _task_arg(kind, learned):
    from cmbpo_amd import _lib
    if kind == "default":
        tid = _lib.TASK_DEFAULT
    elif kind == "antsafe":
        tid = _lib.TASK_ANTSAFE
    else:
        if not _TABLE:      # one registered table for the module (the slots are a process-wide resource)
            from cmbpo_amd.statics import TaskRules, cost, healthy
            _TABLE.append(TaskRules([healthy(cols=0, lo=0.2, hi=1.5), cost(cols=-1, abs=True, lo=0.4, lo_strict=True)],
                                    require_finite=True, cost_on_term=True))
        tid = _TABLE[0].task_id
    return tid | (_lib.TASK_LEARNED_COST if learned else 0)


def _term_inputs(rng, E, D, A, n, listed, learned):
    """Means drawn directly; the termination column is 0.35 + 0.3 z_row + 0.15 z_member (float32) with eight special rows."""
    O = ref.term_column(D, learned) + 1
    B = n + 11 if listed else n
    obs = (rng.standard_normal((B, D)) * 0.1).astype(np.float32)
    obs[:, 0] = rng.uniform(0.3, 0.9, B).astype(np.float32)
    act = rng.uniform(-1, 1, (B, A)).astype(np.float32)
    mean = (rng.standard_normal((E, B, O)) * 0.3).astype(np.float32)
    var = np.exp(rng.uniform(-12, 1, (E, B, O))).astype(np.float32)
    z_row, z_mem = rng.standard_normal(B).astype(np.float32), rng.standard_normal((E, B)).astype(np.float32)
    mean[:, :, O - 1] = np.float32(0.35) + np.float32(0.3) * z_row[None] + np.float32(0.15) * z_mem
    inds = rng.integers(0, E, size=B).astype(np.int32)
    rows = np.sort(rng.choice(B, size=n, replace=False)).astype(np.int32) if listed else None
    live = np.arange(B) if rows is None else rows
    return obs, act, mean, var, inds, rows, live, O


def _special_rows(mean, var, obs, inds, live, O, E):
    tc = O - 1
    oth = lambda r, k=1: (inds[r] + k) % E
    r = live[0]                                  # the table's rule and the head both end it: z = 5 is outside its healthy band
    obs[r, 0], mean[:, r, 0], var[:, r, 0], mean[:, r, tc] = 5.0, 0.0, 1e-6, 0.9
    r = live[8]                                  # AntSafe's rule and the head both end it: q1 = 1 gives z_rot = -1 < -0.7
    obs[r, 0], mean[:, r, 0], var[:, r, 0] = 0.6, 0.0, 1e-6
    obs[r, 2], mean[:, r, 2], var[:, r, 2], mean[:, r, tc] = 1.0, 0.0, 1e-6, 0.9
    mean[:, live[1], tc] = -1.0                  # nobody hits
    mean[:, live[2], tc] = 0.9                   # the elite's NaN never hits, the others do
    mean[inds[live[2]], live[2], tc] = np.nan
    mean[:, live[3], tc] = -1.0                  # the elite's +inf hits alone
    mean[inds[live[3]], live[3], tc] = np.inf
    mean[oth(live[4]), live[4], tc] = np.nan     # another member's NaN / -inf / +inf
    mean[oth(live[5], 2), live[5], tc] = -np.inf
    mean[:, live[6], tc] = 0.0
    mean[oth(live[6]), live[6], tc] = np.inf
    mean[:, live[7], tc] = THR                   # exactly the threshold: no hit


@pytest.mark.parametrize("n,listed", [(13, False), (13, True), (29, False), (29, True), (1001, False), (1001, True)])
@pytest.mark.parametrize("D", [3, 8, 21])        # below the row's eight lanes, exactly eight, with a remainder
@pytest.mark.parametrize("E", [7, 5, 3])         # the kernel's three instances
def test_post_kernel_term_head(hip_lib, E, D, n, listed):
    """Learned cost on / off x default / AntSafe / a registered table x d_xi NULL / given x disagreement off / on, for every
    vote: term, term_pred, term_votes are the specification's; everything else is the head-off launch over the [..., :tc] copy."""
    _need_gpu()
    from cmbpo_amd import _lib
    A = 3
    for learned in (False, True):
        rng = np.random.default_rng(zlib.crc32(f"{E}/{D}/{n}/{listed}/{learned}/term-head".encode()))
        obs, act, mean, var, inds, rows, live, O = _term_inputs(rng, E, D, A, n, listed, learned)
        tc = O - 1
        if n == 1001:
            # the column's distribution does what it is for -- on the reference alone, before any special row and any launch
            learned_by = {m: ref.term_head(mean, inds, D, learned, THR, m, rows=live)[3] for m in MODES}
            for m in MODES:
                assert 0.2 <= learned_by[m].mean() <= 0.8, (m, learned_by[m].mean())
            for a, b in (("elite", "any"), ("elite", "majority"), ("any", "majority")):
                assert (learned_by[a] != learned_by[b]).mean() >= 0.05, (a, b)
        _special_rows(mean, var, obs, inds, live, O, E)
        for m in MODES:
            hit = ref.term_head(mean, inds, D, learned, THR, m, rows=live)[3]
            assert hit.any() and not hit.all(), m
        xi_draws = rng.standard_normal((obs.shape[0], D)).astype(np.float32)
        narrow_mean, narrow_var = np.ascontiguousarray(mean[..., :tc]), np.ascontiguousarray(var[..., :tc])
        rest = np.setdiff1d(np.arange(obs.shape[0]), live)
        for kind in ("default", "antsafe", "table"):
            task_arg = _task_arg(kind, learned)
            if kind == "antsafe" and D < 5:      # refused by the entry point, with or without the head
                with pytest.raises(AssertionError):
                    _run_term(task_arg, obs, act, mean, var, inds, D, A, rows, head=(THR, "elite"))
                assert b"AntSafe" in _lib.lib().cmbpo_last_error()
                continue
            for xi in (None, xi_draws):
                for kappa in (None, (0.75, 1.5 if learned else 0.0)):
                    tag = f"{kind} learned={learned} xi={xi is not None} dis={kappa is not None}"
                    off = _run_term(task_arg, obs, act, narrow_mean, narrow_var, inds, D, A, rows, xi, kappa, head=None)
                    assert (off["term"][live] <= 1).all() and (off["term_pred"] == -7.0).all() and (off["term_votes"] == 77).all()
                    if kind == "default":
                        assert not off["term"][live].any(), tag
                    else:                                               # the rule ends a row the head ends too
                        both = live[0] if kind == "table" else live[8]
                        assert off["term"][both] == 1, tag
                    for m in MODES:
                        on = _run_term(task_arg, obs, act, mean, var, inds, D, A, rows, xi, kappa, head=(THR, m))
                        term, pred, votes, hit = ref.term_head(mean, inds, D, learned, THR, m, rows=live, rule_done=off["term"][live])
                        np.testing.assert_array_equal(on["term"][live], term, err_msg=f"{tag} {m} term")
                        np.testing.assert_array_equal(_bits(on["term_pred"][live]), _bits(pred), err_msg=f"{tag} {m} term_pred")
                        np.testing.assert_array_equal(on["term_votes"][live], votes, err_msg=f"{tag} {m} term_votes")
                        assert hit[0] and hit[8] and term[0] == 1 and term[8] == 1
                        for k in CLASSIC + (("rew_var", "cost_var") if kappa is not None else ()):
                            np.testing.assert_array_equal(_bits(on[k]), _bits(off[k]), err_msg=f"{tag} {m} {k}")
                        if len(rest):    # unlisted slots keep their sentinels
                            assert (on["term"][rest] == 77).all() and (on["term_votes"][rest] == 77).all()
                            assert (on["term_pred"][rest] == -7.0).all()
                    # NULL optional outputs: the same decisions, nothing else written
                    bare = _run_term(task_arg, obs, act, mean, var, inds, D, A, rows, xi, kappa, head=(THR, "majority"), optional=False)
                    np.testing.assert_array_equal(bare["term"], on["term"], err_msg=tag)
                    assert (bare["term_pred"] == -7.0).all() and (bare["term_votes"] == 77).all()


def _narrowest(xi, dis, head):
    """The naming rule of the post step (DESIGN): the narrowest entry point that can express a feature set."""
    return ("cmbpo_fakeenv_post_term" if head else "cmbpo_fakeenv_post_disagreement" if dis
            else "cmbpo_fakeenv_post_noise" if xi else "cmbpo_fakeenv_post")


@pytest.mark.parametrize("kind", ["antsafe", "table"])
@pytest.mark.parametrize("E", [7, 5, 3])         # the kernel's three instances
def test_every_entry_point_is_the_superset_call_bitwise(hip_lib, E, kind):
    """{xi} x {disagreement} x {head}: the narrowest entry point of a feature set and cmbpo_fakeenv_post_term with the rest NULL / 0
    write the same bits into every output -- one workgroup of eight rows and a ragged second, through an unsorted row list.  With
    the head on the narrowest entry IS the superset: there the head-off outputs are those of the narrow entry over the narrower
    copy of the means, and the decisions the specification's."""
    _need_gpu()
    D, A, n, B = 5, 2, 9, 12
    rng = np.random.default_rng(zlib.crc32(f"{E}/{kind}/one-post-call".encode()))
    rows = rng.permutation(B)[:n].astype(np.int32)
    assert len(set(rows.tolist())) == n and (np.diff(rows) < 0).any()
    obs = (rng.standard_normal((B, D)) * 0.1).astype(np.float32)
    obs[rows[0::2], 0], obs[rows[1::2], 0] = 0.6, 5.0     # z: inside / outside the healthy band (the table ends the row)
    obs[rows[0::4], 2] = 1.0                               # healthy and q1 = 1: z_rot = -1 < -0.7 (AntSafe ends the row)
    act = rng.uniform(-1, 1, (B, A)).astype(np.float32)
    inds = rng.integers(0, E, size=B).astype(np.int32)
    xi_draws = rng.standard_normal((B, D)).astype(np.float32)
    for dis in (False, True):
        learned = dis                                 # kappa_cost > 0 needs the learned-cost column
        O = ref.term_column(D, learned) + 1
        mean = (rng.standard_normal((E, B, O)) * 0.3).astype(np.float32)
        var = np.exp(rng.uniform(-12, 1, (E, B, O))).astype(np.float32)
        mean[:, :, (0, 2)], var[:, :, (0, 2)] = 0.0, 1e-6      # z and q1 stay where obs put them, with or without the draws
        mean[:, :, O - 1] = (0.5 + 0.4 * rng.standard_normal((E, B))).astype(np.float32)
        narrow = np.ascontiguousarray(mean[..., :O - 1]), np.ascontiguousarray(var[..., :O - 1])
        task_arg = _task_arg(kind, learned)
        kappa = (0.5, 0.25) if dis else None
        for xi in (None, xi_draws):
            tag = f"{kind} E={E} xi={xi is not None} dis={dis}"
            entry = _narrowest(xi is not None, dis, False)
            own = _run_term(task_arg, obs, act, *narrow, inds, D, A, rows, xi, kappa, entry=entry)
            sup = _run_term(task_arg, obs, act, *narrow, inds, D, A, rows, xi, kappa)
            assert set(own["term"][rows].tolist()) == {0, 1}, tag                     # both values of done occur
            for k in own:
                np.testing.assert_array_equal(_bits(sup[k]), _bits(own[k]), err_msg=f"{tag} {k}")
            on = _run_term(task_arg, obs, act, mean, var, inds, D, A, rows, xi, kappa, head=(THR, "majority"))
            term, pred, votes, hit = ref.term_head(mean, inds, D, learned, THR, "majority", rows=rows, rule_done=own["term"][rows])
            assert hit.any() and not hit.all(), tag
            np.testing.assert_array_equal(on["term"][rows], term, err_msg=tag)
            np.testing.assert_array_equal(_bits(on["term_pred"][rows]), _bits(pred), err_msg=tag)
            np.testing.assert_array_equal(on["term_votes"][rows], votes, err_msg=tag)
            for k in CLASSIC + ("rew_var", "cost_var"):
                np.testing.assert_array_equal(_bits(on[k]), _bits(own[k]), err_msg=f"{tag} head on {k}")


_SIDE_KEYS = {"iv": {"cumvar_buf", "iv_tables"}, "dis": {"rew_var_t", "cost_var_t", "path_rew_var", "path_cost_var", "dis_part"},
              "vdis": {"v_var", "vc_var", "vdis_part"}, "term": {"term_pred_t", "term_votes_t"}}


def test_model_buffer_side_arrays_follow_the_switches(hip_lib):
    """Each feature beside the rollout struct on, off and on again: its arrays exist exactly while it is on, the other features'
    arrays stay what they are (the same tensors), and a feature switched on again gets arrays of its own."""
    _need_gpu()
    from cmbpo_amd.modelbuffer import ModelBuffer
    buf = ModelBuffer(4, 5, 2, 2, device=DEV)
    switch = {"iv": lambda on: buf.set_iv_gae(on), "dis": lambda on: buf.set_disagreement(on, 0.5 if on else 0.0),
              "vdis": lambda on: buf.set_value_disagreement(on), "term": lambda on: buf.set_term_head(on, 0.5, "majority")}
    every = set().union(*_SIDE_KEYS.values())
    base = set(buf.t)
    assert not base & every
    on_now = set()
    for feature, keys in _SIDE_KEYS.items():
        for on in (True, False, True):
            before = dict(buf.t)
            switch[feature](on)
            on_now = on_now | {feature} if on else on_now - {feature}
            assert set(buf.t) == base | set().union(*[_SIDE_KEYS[f] for f in on_now]), (feature, on)
            for k, v in before.items():
                if k not in keys:
                    assert buf.t[k] is v, (feature, on, k)
        assert buf.t["iscal"].data_ptr() == buf.rs.iscal
    # a new batch size: every array anew, every feature still on
    buf.reset(batch_size=6)
    assert set(buf.t) == base | every and buf.t["cumvar_buf"].shape == (2, 6) and buf.t["dis_part"].shape == (2,)
    assert buf.t["term_votes_t"].dtype == torch.uint8 and buf.t["v_var"].dtype == torch.float32


# ------------------------------------------------------------------------------------------------------------------
# 2. the rollout
# ------------------------------------------------------------------------------------------------------------------
TASK, T, HIDDEN = "AntSafe-v2", 8, 128
NEVER = 3.0e38            # a finite threshold no finite prediction exceeds: the head attached, no learned termination


def build_world_term(seed, E=7, term=True, term_scale=400.0):
    """tests/golden/worlds_learned_cost.build_world_learned_cost with one more column behind the cost: the termination head's,
    its output scaler's variance scaled up so that the predictions spread over a few units."""
    from cmbpo_amd import synthetic
    rng = np.random.default_rng(seed)
    D, A = synthetic.ENV_DIMS[TASK]
    out_dim = D + 2 + int(term)
    ws, bs = synthetic.ensemble_weights(rng, E, D + A, HIDDEN, 2 * out_dim, bias_scale=0.05)
    sc_in = synthetic.scaler(rng, D + A, hit_clamp=False)
    mu, var = synthetic.scaler(rng, out_dim, hit_clamp=False)
    scale = np.full((1, out_dim), 0.01, np.float32)
    scale[0, D + 1] = 100.0
    if term:
        scale[0, D + 2] = term_scale
    pol = synthetic.policy_params(rng, D, A)
    crit = []
    for _ in range(2):
        cw, cb = synthetic.ensemble_weights(rng, 3, D, 128, 1, bias_scale=0.05)
        crit.append((cw, cb, synthetic.scaler(rng, D, hit_clamp=False), synthetic.scaler(rng, 1, hit_clamp=False)))
    return dict(obs_dim=D, act_dim=A, out_dim=out_dim, ws=ws, bs=bs, sc_in=sc_in, sc_out=(mu, (var * scale).astype(np.float32)),
                pol=pol, v=crit[0], vc=crit[1], elites=[0, 2, 3, 5, 6][: max(1, E - 2)])


def hip_world_term(w, B, head, comm=None):
    """Sampler and pool over the world; head: (threshold, members), or None for a FakeEnv without the head."""
    from cmbpo_amd.cpo_policy import CPOPolicy
    from cmbpo_amd.fake_env import FakeEnv
    from cmbpo_amd.model_sampler import ModelSampler
    from cmbpo_amd.modelbuffer import ModelBuffer
    from cmbpo_amd.pens import PE
    D, A = w["obs_dim"], w["act_dim"]
    E = w["ws"][0].shape[0]
    model = PE(D + A, w["out_dim"], hidden_dims=(HIDDEN, HIDDEN), num_networks=E, num_elites=len(w["elites"]),
               loss="MSPE", use_scaler_in=True, use_scaler_out=True, device=DEV)
    model.set_weights(w["ws"], w["bs"], w["sc_in"], w["sc_out"])
    model.set_elites(w["elites"])
    policy = CPOPolicy(_Space(D), _Space(A), a_hidden_layer_sizes=(128, 128), vf_hidden_layer_sizes=(128, 128),
                       vf_ensemble_size=3, vf_elites=2, vf_activation="swish", vf_loss="MSE", device=DEV,
                       cost_gamma=0.97, cost_lam=0.5, lam=0.95, comm=comm)
    policy.actor.set_params(w["pol"])
    policy.v.set_weights(*w["v"])
    policy.vc.set_weights(*w["vc"])
    kw = {} if head is None else dict(predicts_term=True, term_threshold=head[0], term_members=head[1])
    env = FakeEnv(_Env(D, A), TASK, model, predicts_delta=True, predicts_rew=True, predicts_cost=True, **kw)
    pool = ModelBuffer(B, D, A, T, device=DEV, comm=comm)
    pool.initialize(policy.pi_info_shapes, gamma=0.99, lam=0.95, cost_gamma=0.97, cost_lam=0.5)
    sampler = ModelSampler(max_path_length=T + 5, batch_size=B, rollout_mode="uncertainty", comm=comm)
    sampler.initialize(env, policy, pool)
    sampler.set_rollout_dkl(float("inf"))
    return sampler, pool


def _start(seed, B):
    from cmbpo_amd import synthetic
    return synthetic.start_states(np.random.default_rng(seed), B, TASK)


def _roll_own_draws(w, start, head, how):
    """A whole rollout with the sampler's own draws (seed 5).  how: 'loop' (sample(): cmbpo_rollout_step) or 'many'
    (sample_many(): cmbpo_rollout_run).  Returns get()'s arrays, the lengths and, for 'loop', the elite's predictions met."""
    sampler, pool = hip_world_term(w, start.shape[0], head)
    sampler._gen.manual_seed(5)
    sampler.reset(start)
    assert pool.term_head == head and "term_pred_t" in pool.t
    met = []
    while sampler.any_alive() and pool.has_room:
        if how == "many":
            sampler.sample_many()
        else:
            ids = pool.t["alive_idx"][:pool.n_alive].long()
            sampler.sample()
            met.append(pool.t["term_pred_t"][ids].cpu().numpy())
    ln = pool.t["len"].cpu().numpy().copy()
    sampler.finish_all_paths()
    return pool.get()[0], ln, (np.concatenate(met) if met else None)


@pytest.mark.parametrize("B", [96, 1000, 6000])
def test_sample_many_equals_a_loop_of_sample_with_the_head(hip_lib, B):
    """B = 96 and one case each side of the one-workgroup bookkeeping limit (6000 is also the large-batch critics' side)."""
    _need_gpu()
    assert 1000 <= hip_lib.cmbpo_rollout_book_pre_max_rows() < 6000
    w, start = build_world_term(31), _start(32, B)
    _, len_never, met = _roll_own_draws(w, start, (NEVER, "elite"), "loop")
    thr = float(np.quantile(met[np.isfinite(met)], 0.9))
    head = (thr, "elite")
    loop, len_loop, _ = _roll_own_draws(w, start, head, "loop")
    many, len_many, _ = _roll_own_draws(w, start, head, "many")
    # the head ended branches the rules alone let live, and not all of them
    assert (len_loop < len_never).sum() >= B // 8 and (len_loop == T).sum() >= B // 8, (len_loop < len_never).sum()
    np.testing.assert_array_equal(len_loop, len_many)
    for k, a, b in zip(NAMES, loop, many):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=k)


def test_attached_step_refuses_a_model_without_the_column(hip_lib):
    _need_gpu()
    from cmbpo_amd._lib import CmbpoHipError
    w = build_world_term(31, term=False)
    sampler, pool = hip_world_term(w, 40, None)
    sampler.reset(_start(3, 40))
    assert pool.term_head is None and "term_pred_t" not in pool.t
    pool.set_term_head(True, 0.5, "any")           # beside the struct, without a column in the model
    cur = pool.t["cur_obs"].clone()
    with pytest.raises(CmbpoHipError) as e:
        sampler.sample()
    assert "cmbpo_rollout_step" in str(e.value) and "termination head" in str(e.value) and "out_dim" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert pool.ptr == 0 and pool.n_alive == 40 and torch.equal(pool.t["cur_obs"], cur)      # before any launch
    pool.set_term_head(False)
    sampler.sample()                               # detached: the step it always was
    assert pool.ptr == 1


def _roll_injected(w, start, head, eps, inds, comm=None, lo=0, hi=None, budget=None, alive_trace=None):
    """T steps of sample() with injected draws (eps [T, B, A], inds [T, B], slot indexed over the WHOLE batch; this sampler holds
    slots lo..hi).  Records, per step: the slots stepped, their observations and actions, term / term_pred / term_votes, the
    alive mask after the step."""
    B = start.shape[0]
    hi = B if hi is None else hi
    sampler, pool = hip_world_term(w, hi - lo, head, comm=comm)
    sampler.reset(start[lo:hi])
    cp = lambda x: x.cpu().numpy().copy()
    steps = []
    for s in range(T):
        if alive_trace is not None:      # a shard with nothing left still takes part in the step's collectives
            ids = np.flatnonzero(alive_trace[s][lo:hi])
            assert pool.n_alive == len(ids)
        else:
            if not (sampler.any_alive() and pool.has_room):
                break
            ids = cp(pool.t["alive_idx"][:pool.n_alive])
            assert (np.diff(ids) > 0).all()      # the ordered alive list: compact order is slot order
        cur = cp(pool.t["cur_obs"])[ids]
        sampler.sample(max_samples=budget, eps=eps[s, lo + ids], model_inds=inds[s, lo + ids])
        if len(ids) == 0:
            steps.append(dict(ids=ids, alive=np.zeros(hi - lo, bool)))
            continue
        steps.append(dict(ids=ids, cur=cur, act=cp(pool.t["act_t"])[ids], term=cp(pool.t["term_t"])[ids],
                          pred=cp(pool.t["term_pred_t"])[ids], votes=cp(pool.t["term_votes_t"])[ids],
                          alive=np.asarray(pool.alive_paths).astype(bool).copy()))
    ln = cp(pool.t["len"])
    sampler.finish_all_paths()
    return sampler, steps, ln, pool.get()[0]


def _draws(seed, w, B):
    rng = np.random.default_rng(seed)
    eps = rng.standard_normal((T, B, w["act_dim"])).astype(np.float32)
    inds = np.asarray(w["elites"], np.int32)[rng.integers(0, len(w["elites"]), (T, B))]
    return eps, inds


def _plan_trace(mode, B):
    """World, draws and a threshold for one trace: a pilot with the head attached and a threshold nothing exceeds gives every
    value the column can take along the trace (a branch's path does not depend on the others, nor on the threshold until it
    ends); the threshold is the midpoint of the widest gap for which the host loop ends branches on >= 3 steps and keeps >= 25 %
    alive behind the last step.  Both are checked here, on the host, and another seed is tried if no gap qualifies."""
    for seed in range(40, 46):
        w, start = build_world_term(seed), _start(seed + 100, B)
        eps, inds = _draws(seed + 200, w, B)
        sampler, pilot, _, _ = _roll_injected(w, start, (NEVER, "any"), eps, inds)
        assert len(pilot) == T and all(not st["votes"].any() for st in pilot)
        tc = ref.term_column(w["obs_dim"], True)
        X = [sampler.env._model.predict_ensemble(st["cur"], act=st["act"])[0][:, :, tc] for st in pilot]      # [E, n_s] each

        def host_loop(thr):
            alive, masks, steps_hit = np.ones(B, bool), [], 0
            for s, st in enumerate(pilot):
                a = alive[st["ids"]]
                mean = np.zeros((X[s].shape[0], len(st["ids"]), tc + 1), np.float32)
                mean[:, :, tc] = X[s]
                term, _, votes, hit = ref.term_head(mean, inds[s, st["ids"]], w["obs_dim"], True, thr, mode, rule_done=st["term"])
                steps_hit += int((hit & a).any())
                alive[st["ids"][term.astype(bool)]] = False
                alive &= np.isin(np.arange(B), st["ids"])           # (what the pilot's own rules ended stays ended)
                masks.append((alive.copy(), term, votes))
            return masks, steps_hit
        vals = np.unique(np.concatenate([x.ravel() for x in X]))
        vals = vals[np.isfinite(vals)]
        gaps = np.diff(vals)
        for k in np.argsort(-gaps):
            if gaps[k] < 1e-3:
                break
            thr = float(0.5 * (np.float64(vals[k]) + np.float64(vals[k + 1])))
            masks, steps_hit = host_loop(thr)
            if steps_hit >= 3 and masks[-1][0].sum() >= 0.25 * B:
                return dict(w=w, start=start, eps=eps, inds=inds, thr=thr, gap=float(gaps[k]), masks=masks, steps_hit=steps_hit,
                            ids=[st["ids"] for st in pilot])
    raise AssertionError("no seed gives a gap >= 1e-3 with terminations on >= 3 steps and >= 25 % of the branches left")


@pytest.mark.parametrize("mode", MODES)
def test_trace_against_the_host_loop(hip_lib, mode):
    """One trace per vote, B = 96, T = 8: forward -> term_head_ref on the host against the rollout, alive masks exact."""
    _need_gpu()
    B = 96
    p = _plan_trace(mode, B)
    assert p["gap"] >= 1e-3 and p["steps_hit"] >= 3 and p["masks"][-1][0].sum() >= 0.25 * B
    print(f"{mode}: threshold {p['thr']:.6f} in a gap of {p['gap']:.2e}, terminations on {p['steps_hit']} steps, "
          f"{int(p['masks'][-1][0].sum())} of {B} branches alive behind the last step")
    _, steps, _, _ = _roll_injected(p["w"], p["start"], (p["thr"], mode), p["eps"], p["inds"])
    assert len(steps) == T
    alive_before = np.ones(B, bool)
    for s, (st, (alive, term, votes)) in enumerate(zip(steps, p["masks"])):
        np.testing.assert_array_equal(st["ids"], np.flatnonzero(alive_before), err_msg=f"rows stepped at {s}")
        np.testing.assert_array_equal(st["alive"], alive, err_msg=f"alive mask after step {s}")
        # the host loop ran on the pilot's rows, a superset of this trace's: term and votes on the rows both stepped
        sel = np.isin(p["ids"][s], st["ids"])
        np.testing.assert_array_equal(st["term"], term[sel], err_msg=f"term at step {s}")
        np.testing.assert_array_equal(st["votes"], votes[sel], err_msg=f"votes at step {s}")
        alive_before = alive


# ------------------------------------------------------------------------------------------------------------------
# 3. two shards (gloo, both ranks on the one GPU) through the per-step path
# ------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, path):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import datetime
    import torch.distributed as td
    td.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    import cmbpo_amd  # noqa: F401
    from cmbpo_amd.dist import Comm
    comm = Comm(device=torch.device(DEV))
    g = np.load(os.path.join(path, "trace.npz"), allow_pickle=False)
    B = int(g["B"])
    w = build_world_term(int(g["seed"]))
    cut = B // 2 + 3                                   # unequal contiguous shards
    lo, hi = (0, cut) if rank == 0 else (cut, B)
    alive_in = [np.ones(B, bool)] + [g["alive"][s].astype(bool) for s in range(T - 1)]
    _, steps, ln, res = _roll_injected(w, g["start"], (float(g["thr"]), str(g["mode"])), g["eps"], g["inds"], comm=comm, lo=lo, hi=hi,
                                       budget=int(g["budget"]), alive_trace=alive_in)
    ok = all(np.array_equal(st["alive"], g["alive"][s][lo:hi]) for s, st in enumerate(steps))
    out = {"ok_masks": ok, "len": ln}
    for k, arr in zip(NAMES, res):
        out["get_" + k] = arr
    np.savez(os.path.join(path, f"rank{rank}.npz"), **out)
    comm.barrier()
    td.destroy_process_group()


def test_two_shards_replay_a_trace_through_the_per_step_path(hip_lib, tmp_path):
    """A budget that never binds still sends every step of a sharded sampler through the budget exchange, i.e. through
    FakeEnv.step_device and the separate bookkeeping calls; the trace is the one-process rollout (cmbpo_rollout_step)."""
    _need_gpu()
    import torch.multiprocessing as mp
    B, seed, mode, budget = 96, 40, "elite", 10 ** 8
    w, start = build_world_term(seed), _start(seed + 100, B)
    eps, inds = _draws(seed + 200, w, B)
    _, pilot, _, _ = _roll_injected(w, start, (NEVER, mode), eps, inds)
    met = np.concatenate([st["pred"] for st in pilot])
    thr = float(np.quantile(met[np.isfinite(met)], 0.9))
    _, steps, ln, res = _roll_injected(w, start, (thr, mode), eps, inds, budget=budget)
    assert len(steps) == T and (ln < T).sum() >= B // 8 and (ln == T).sum() >= B // 8
    np.savez(os.path.join(tmp_path, "trace.npz"), B=B, seed=seed, mode=mode, thr=thr, budget=budget, start=start, eps=eps, inds=inds,
             alive=np.stack([st["alive"] for st in steps]))
    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r = [np.load(os.path.join(tmp_path, f"rank{k}.npz")) for k in range(world)]
    assert all(bool(x["ok_masks"]) for x in r)
    np.testing.assert_array_equal(np.concatenate([x["len"] for x in r]), ln)
    for k, want in zip(NAMES, res):
        if k in ("adv", "cadv"):         # normalised with statistics reduced across the shards: another order of additions
            continue
        got = np.concatenate([x["get_" + k] for x in r], axis=0)
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=k)


# ------------------------------------------------------------------------------------------------------------------
# 4. the replay
# ------------------------------------------------------------------------------------------------------------------
_REPLAY_ENV = {}


def _replay_env(members):
    """FakeEnv with both heads over a 128-wide AntSafe-shaped ensemble with small steps; the termination column spreads around
    the threshold 0.5 (the replay cases set a threshold of their own)."""
    if members in _REPLAY_ENV:
        return _REPLAY_ENV[members]
    from cmbpo_amd import synthetic
    from cmbpo_amd.fake_env import FakeEnv
    from cmbpo_amd.pens import PE
    D, A = synthetic.ENV_DIMS[TASK]
    E, O = 5, D + 3
    rng = np.random.default_rng(zlib.crc32(b"term-head/replay-model"))
    ws, bs = synthetic.ensemble_weights(rng, E, D + A, 128, 2 * O, bias_scale=0.05)
    sc_in = synthetic.scaler(rng, D + A)
    mu, var = np.zeros((1, O), np.float32), np.full((1, O), 2.5e-3, np.float32)
    mu[0, O - 1], var[0, O - 1] = 0.4, 1.0
    np.random.seed(5)
    model = PE(D + A, O, hidden_dims=(128, 128), num_networks=E, num_elites=3, loss="MSPE", use_scaler_in=True,
               use_scaler_out=True, device=DEV)
    model.set_weights(ws, bs, sc_in, (mu, var))
    env = FakeEnv(_Env(D, A), TASK, model, True, True, True, seed=3, predicts_term=True, term_threshold=THR, term_members=members)
    _REPLAY_ENV[members] = (env, D, A, E)
    return _REPLAY_ENV[members]


def _pick_threshold(X, inds, D, members, share=0.25):
    """A threshold at which this vote ends about `share` of the rows of X [E, n, out]: the members of a random ensemble sit at
    offsets of their own, so it is a quantile of all members' values of the column."""
    cands = np.quantile(X[:, :, -1], np.linspace(0.02, 0.98, 49))
    rate = [ref.term_head(X, inds, D, True, float(c), members)[3].mean() for c in cands]
    return float(cands[int(np.argmin(np.abs(np.asarray(rate) - share)))])


def _replay_case(members, B, H, mode):
    from test_replay_gpu import _recording
    env, D, A, E = _replay_env(members)
    rng = np.random.default_rng(zlib.crc32(f"term-head/{members}/{B}/{H}/{mode}".encode()))
    obs0, act, rec, lengths = _recording(rng, B, H, D, A)
    inds = rng.integers(0, E, (H, B)).astype(np.int32)
    # about a quarter of the windows end per step, judged on the first step's values
    env.set_term_head(_pick_threshold(env._model.predict_ensemble(obs0, act=act[0])[0], inds[0], D, members), members)
    return env, obs0, act, rec, lengths, inds


def _replay_buffers(env, obs0, act, rec, lengths, mode, calibration=False):
    from cmbpo_amd.replay import ReplayBuffers
    return ReplayBuffers(obs0, act, rec["next_obs"], rec["rew"], rec["cost"], rec["term"], lengths=lengths, mode=mode,
                         ensemble=env._model.num_nets, out_dim=env.output_dim, device=DEV, calibration=calibration)


@pytest.mark.parametrize("calibration", [False, True])
@pytest.mark.parametrize("mode", ["open_loop", "one_step"])
@pytest.mark.parametrize("members,B", [("elite", 65), ("any", 257), ("majority", 1030)])
def test_replay_run_term_is_the_loop_of_single_calls_bitwise(hip_lib, members, B, mode, calibration):
    _need_gpu()
    H = 5
    env, obs0, act, rec, lengths, inds = _replay_case(members, B, H, mode)
    E = env._model.num_nets
    inds_d = torch.from_numpy(inds).to(DEV)
    a = _replay_buffers(env, obs0, act, rec, lengths, mode, calibration)
    th = env.term_head_struct()
    if calibration:
        a.run_calibrated(env._model.mlp.handle, env._task_id, E, inds_d, term_head=th)
    else:
        a.run(env._model.mlp.handle, env._task_id, E, inds_d, term_head=th)
    c = _replay_buffers(env, obs0, act, rec, lengths, mode, calibration)
    if calibration:
        c.set_elite(inds_d)
    for h in range(H):
        env.step_device(c.t["cur_obs"], c.t["act"][h], inds_d[h], c.step_outputs(), scratch=(c.t["mean"], c.t["var"]))
        if calibration:
            c.calibrate(h)
        c.compare(h)
    c.finish()
    if calibration:
        c.calib_finish()
    torch.cuda.synchronize()
    for k in ("sums", "counts", "cur_obs", "alive", "p_term", "p_next_obs"):
        assert torch.equal(a.t[k], c.t[k]), k
    if calibration:
        for k in ("sums", "counts"):
            assert torch.equal(a.c[k], c.c[k]), "calibration " + k
    tab = a.table()
    assert tab["term_cm"][:, :, 1].sum() > 0 and tab["term_cm"][:, :, 0].sum() > 0
    # FakeEnv.replay is that call
    got = env.replay(obs0, act, rec["next_obs"], rec["rew"], rec["cost"], rec["term"], lengths=lengths, model_inds=inds, mode=mode,
                     calibration=calibration)
    for k in ("n", "term_cm", "cost_cm", "se_obs"):
        np.testing.assert_array_equal(got[k], tab[k], err_msg=k)


@pytest.mark.parametrize("members", MODES)
def test_one_step_replay_counts_the_heads_terminations(hip_lib, members):
    """term_cm[h] of a teacher-forced replay against the reference: the forward, the head-off post kernel over the narrower
    copy for the rule's verdict and everything else, term_head_ref for the head, tests/replay_ref.py for the life of a window."""
    _need_gpu()
    B, H = 257, 6
    env, obs0, act, rec, lengths, inds = _replay_case(members, B, H, "one_step")
    D, A, model = env.obs_dim, env.act_dim, env._model
    tc = ref.term_column(D, True)
    thr = env.term_threshold
    learned_total = [0]

    def step(h, cur):
        mean, var = model.predict_ensemble(cur, act=act[h])
        off = _run_term(env._task_id, cur, act[h], np.ascontiguousarray(mean[..., :tc]), np.ascontiguousarray(var[..., :tc]),
                        inds[h], D, A, head=None)
        term, _, _, hit = ref.term_head(mean, inds[h], D, True, thr, members, rule_done=off["term"])
        learned_total[0] += int((hit & ~off["term"].astype(bool)).sum())
        return dict(next_obs=off["next_obs"], rew=off["rew"], cost=off["cost"], term=term, ep_var_mean=off["ep_var_mean"],
                    dkl_path=off["dkl_path"])
    want, _, _ = replay_ref.replay(step, obs0, rec, lengths, replay_ref.ONE_STEP)
    got = env.replay(obs0, act, rec["next_obs"], rec["rew"], rec["cost"], rec["term"], lengths=lengths, model_inds=inds, mode="one_step")
    np.testing.assert_array_equal(got["term_cm"], want["term_cm"])
    np.testing.assert_array_equal(got["n"], want["n"])
    np.testing.assert_array_equal(got["cost_cm"], want["cost_cm"])
    assert learned_total[0] > 0 and got["term_cm"][:, :, 1].sum() > 0 and got["term_cm"][:, :, 0].sum() > 0
    # the head changes the counts: the same replay through a head nothing exceeds
    env.set_term_head(NEVER, members)
    try:
        never = env.replay(obs0, act, rec["next_obs"], rec["rew"], rec["cost"], rec["term"], lengths=lengths, model_inds=inds, mode="one_step")
    finally:
        env.set_term_head(thr, members)
    assert never["term_cm"][:, :, 1].sum() < got["term_cm"][:, :, 1].sum()


# ------------------------------------------------------------------------------------------------------------------
# 5. FakeEnv.step and the widest shipped shape
# ------------------------------------------------------------------------------------------------------------------
def test_fake_env_step_reports_the_head(hip_lib):
    _need_gpu()
    env, D, A, E = _replay_env("majority")
    rng = np.random.default_rng(9)
    n = 333
    obs = _start(10, n)
    act = rng.uniform(-1, 1, (n, A)).astype(np.float32)
    inds = rng.integers(0, E, n).astype(np.int32)
    assert env.output_dim == D + 3 and env.predicts_term
    mean, _ = env._model.predict_ensemble(obs, act=act)
    for members in MODES:
        thr = _pick_threshold(mean, inds, D, members)
        env.set_term_head(thr, members)
        _, _, terms, info = env.step(obs, act, model_inds=inds)
        _, pred, votes, hit = ref.term_head(mean, inds, D, True, thr, members)
        np.testing.assert_array_equal(_bits(info["term_pred"]), _bits(pred))
        np.testing.assert_array_equal(info["term_votes"], votes)
        assert info["term_votes"].dtype == np.uint8 and terms.shape == (n, 1)
        assert (terms[:, 0] >= hit).all() and hit.any() and not hit.all()
    env.set_term_head(THR, "majority")
    with pytest.raises(ValueError):
        env.set_term_head(float("nan"), "elite")
    with pytest.raises(ValueError):
        env.set_term_head(0.5, "most")


def test_antsafe_with_both_heads_stays_on_the_f16_paths(hip_lib):
    """AntSafe's 29 observations + reward + cost + termination are 32 targets, 64 raw outputs: the widest the f16 forward and
    training paths take (31 targets, 62 raw outputs: one head)."""
    _need_gpu()
    from cmbpo_amd import synthetic
    from test_ens_train_gpu import _make
    D, A = synthetic.ENV_DIMS[TASK]
    for targets in (D + 2, D + 3):
        pe = _make(7, D + A, 512, targets, "MSPE", 64, seed=1)[1]
        assert pe._ensure_trainer(64).f16_paths == 3, targets
        assert pe.out_dim == targets
