"""GPU: the logistic learned-cost head -- the post kernel's COST instances against tests/cost_head_ref.py, then the
head along imagined rollouts (the one-call step against the per-call path), in ModelBuffer's side state, in the replay and in
FakeEnv.step.

Two kinds of statement.  The logistic function itself is compared with a float64 sigma inside the bound cost_head_ref derives
(the device's expf need not round like NumPy's exp).  Everything downstream of a member's probability -- the variance over the
members, the pessimistic cost, the clip -- is float32 arithmetic NumPy reproduces, so it is compared bit for bit, on the DEVICE's
own probabilities: E launches with elite = e and no disagreement hand out p_e for every member, which also shows that a
member's probability has the same bits in every instance and lane that computes it.

Shapes are those of test_term_head_gpu.test_post_kernel_term_head: the kernel's three ensemble instances, D below / at / above
the row's eight lanes, one ragged workgroup, a few, and 126 of them, with and without a row list."""
import ctypes as C
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import cost_head_ref as ref  # noqa: E402
import test_term_head_gpu as tt  # noqa: E402  (its worlds, rule table and helpers; nothing of it is collected here)

DEV = tt.DEV
A = 3
SPECIAL = np.array([0.0, 1e-8, -1e-8, 20.0, -20.0, 80.0, -80.0, 1e4, -1e4, np.inf, -np.inf, np.nan], np.float32)
OUT_F32 = ("next_obs", "rew", "cost", "dkl_path", "ep_var_mean", "ep_var", "rew_var", "cost_var", "term_pred", "cost_logit")
OUT_U8 = ("term", "term_votes")
SHAPES = [(13, False), (13, True), (29, False), (29, True), (1001, False), (1001, True)]


def _bits(a):
    return tt._bits(a)


def _same(a, b, err_msg=""):
    """Bit for bit on every number; a NaN must meet a NaN (its payload and sign are the hardware's choice, not the specification's)."""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    np.testing.assert_array_equal(na, nb, err_msg=err_msg + " (NaN positions)")
    np.testing.assert_array_equal(_bits(a)[~na], _bits(b)[~nb], err_msg=err_msg)


class _Case:
    """Inputs of one shape on the device, uploaded once.  The cost column: a third of the rows N(0, 2) logits (probabilities
    away from 0 and 1), the rest uniform in [-80, 80] (members at both ends: a large spread), and the special values in the
    elite's place of the first rows and in another member's place of the next."""

    def __init__(self, E, D, n, listed, term):
        rng = np.random.default_rng(zlib.crc32(f"{E}/{D}/{n}/{listed}/{term}/cost-head".encode()))
        self.E, self.D, self.n, self.term = E, D, n, term
        self.O = O = D + 2 + int(term)
        self.B = B = n + 11 if listed else n
        cc = ref.cost_column(D)
        obs = (rng.standard_normal((B, D)) * 0.1).astype(np.float32)
        obs[:, 0] = rng.uniform(0.3, 0.9, B).astype(np.float32)
        act = rng.uniform(-1, 1, (B, A)).astype(np.float32)
        mean = (rng.standard_normal((E, B, O)) * 0.3).astype(np.float32)
        var = np.exp(rng.uniform(-12, 1, (E, B, O))).astype(np.float32)
        z = rng.uniform(-80, 80, (E, B)).astype(np.float32)
        soft = rng.random(B) < 1 / 3
        z[:, soft] = (2.0 * rng.standard_normal((E, int(soft.sum())))).astype(np.float32)
        if term:
            mean[:, :, O - 1] = (0.5 + 0.4 * rng.standard_normal((E, B))).astype(np.float32)
        inds = rng.integers(0, E, size=B).astype(np.int32)
        rows = np.sort(rng.choice(B, size=n, replace=False)).astype(np.int32) if listed else None
        live = np.arange(B) if rows is None else rows
        k = min(len(SPECIAL), n)
        z[inds[live[:k]], live[:k]] = SPECIAL[:k]                         # the elite's own logit
        for j, r in enumerate(live[k:min(2 * k, n)]):                     # another member's: reaches the variance alone
            z[(inds[r] + 1) % E, r] = SPECIAL[j]
        # rows the table's rule and AntSafe's rule end (tt._special_rows' first and ninth)
        r = live[0]
        obs[r, 0], mean[:, r, 0], var[:, r, 0] = 5.0, 0.0, 1e-6
        if D >= 5 and n > 8:
            r = live[8]
            obs[r, 0], mean[:, r, 0], var[:, r, 0] = 0.6, 0.0, 1e-6
            obs[r, 2], mean[:, r, 2], var[:, r, 2] = 1.0, 0.0, 1e-6
        mean[:, :, cc] = z
        self.obs, self.act, self.mean, self.var, self.inds, self.rows, self.live, self.z = obs, act, mean, var, inds, rows, live, z
        self.rest = np.setdiff1d(np.arange(B), live)
        self.xi = rng.standard_normal((B, D)).astype(np.float32)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        self.d = dict(obs=t(obs), act=t(act), mean=t(mean), var=t(var), inds=t(inds), xi=t(self.xi),
                      rows=None if rows is None else t(rows))

    def kinds(self):
        return ("default", "table") + (("antsafe",) if self.D >= 5 else ())


_CASES = {}


def _case(E, D, n, listed, term=False):
    key = (E, D, n, listed, term)
    if key not in _CASES:
        if len(_CASES) > 4:
            _CASES.clear()
        _CASES[key] = _Case(*key)
    return _CASES[key]


def _launch(c, kind, mean=None, elite=None, xi=False, kappa=None, head=None, cost=(1, 0.0), entry="cmbpo_fakeenv_post_cost",
            logit_out=True):
    """One post call on the case's device arrays.  kappa: None -- no disagreement, or (kappa_rew, kappa_cost); head: None or
    (threshold, members); cost: None (ch == NULL) or (kind, logit_shift); mean / elite: other device tensors in place of the
    case's.  Every output starts at a sentinel."""
    from cmbpo_amd import _lib
    B, D, E, d = c.B, c.D, c.E, c.d
    f, u8 = dict(dtype=torch.float32, device=DEV), dict(dtype=torch.uint8, device=DEV)
    out = {k: torch.full((B, D) if k in ("next_obs", "ep_var") else (B,), -7.0, **f) for k in OUT_F32}
    out.update({k: torch.full((B,), 77, **u8) for k in OUT_U8})
    th = ch = None
    if head is not None:
        th = _lib.TermHeadStruct()
        th.threshold, th.members = head[0], _lib.TERM_MEMBERS[head[1]]
        th.term_pred, th.term_votes = _lib.ptr(out["term_pred"]), _lib.ptr(out["term_votes"])
    if cost is not None:
        ch = _lib.CostHeadStruct()
        ch.kind, ch.logit_shift, ch.cost_logit = cost[0], cost[1], _lib.ptr(out["cost_logit"]) if logit_out else None
    kr, kc = kappa if kappa is not None else (0.0, 0.0)
    mean_t = d["mean"] if mean is None else mean
    var_t = d["var"]
    args = [tt._task_arg(kind, True), E, D, A, _lib.ptr(mean_t), _lib.ptr(var_t), B, _lib.ptr(d["obs"]), _lib.ptr(d["act"]),
            _lib.ptr(d["inds"] if elite is None else elite), _lib.ptr(d["rows"]), None, c.n,
            _lib.ptr(out["next_obs"]), _lib.ptr(out["rew"]), _lib.ptr(out["term"]), _lib.ptr(out["cost"]), _lib.ptr(out["dkl_path"]),
            _lib.ptr(out["ep_var_mean"]), _lib.ptr(out["ep_var"]), _lib.ptr(d["xi"]) if xi else None, float(kr), float(kc),
            _lib.ptr(out["rew_var"]) if kappa is not None else None, _lib.ptr(out["cost_var"]) if kappa is not None else None,
            None if th is None else C.byref(th)]
    if entry == "cmbpo_fakeenv_post_cost":
        args.append(None if ch is None else C.byref(ch))
    else:
        assert entry == "cmbpo_fakeenv_post_term" and ch is None
    rc = getattr(_lib.lib(), entry)(*args, _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, _lib.lib().cmbpo_last_error())
    return {k: v.cpu().numpy() for k, v in out.items()}


def _member_probs(c, shift):
    """The device's own p_e for every member: E launches with elite = e, no disagreement, the default task, no noise."""
    p = np.empty((c.E, c.n), np.float32)
    for e in range(c.E):
        el = torch.full((c.B,), e, dtype=torch.int32, device=DEV)
        got = _launch(c, "default", elite=el, cost=(1, shift))
        p[e] = got["cost"][c.live]
        _same(got["cost_logit"][c.live], c.z[e, c.live])
    return p


# ------------------------------------------------------------------------------------------------------------------
# 1. the accuracy of sigma32
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,listed", SHAPES)
@pytest.mark.parametrize("D", [3, 8, 21])
@pytest.mark.parametrize("E", [7, 5, 3])
def test_sigma32_is_within_the_derived_bound_of_the_float64_sigma(hip_lib, E, D, n, listed):
    """kappa = 0, on the instances without and with the disagreement: |cost - sigma64(z)| <= 4 * 2^-23 * sigma64(z), exact
    0 / 1 / NaN at -inf / +inf / NaN, and 0 <= cost <= 1."""
    tt._need_gpu()
    c = _case(E, D, n, listed)
    z = c.z[c.inds[c.live], c.live]
    want = ref.sigma64(z)
    fin = np.isfinite(z)
    assert (np.abs(z[fin]) <= 80).sum() >= n - 5 and np.isnan(z).sum() == 1 and np.isinf(z).sum() == 2
    for kappa in (None, (0.0, 0.0)):
        got = _launch(c, "default", kappa=kappa)["cost"][c.live].astype(np.float64)
        err = np.abs(got[fin] - want[fin])
        rel = err[want[fin] > 0] / want[fin][want[fin] > 0]
        print("E %d D %d n %d dis %s: max |cost - sigma64| / sigma64 = %.3f * 2^-23" % (E, D, n, kappa is not None, rel.max() * 2.0 ** 23))
        assert (err <= ref.sigma_bound(z[fin])).all(), (rel.max() * 2.0 ** 23)
        assert ((got[fin] >= 0) & (got[fin] <= 1)).all()
        assert (got[z == np.inf] == 1.0).all() and (got[z == -np.inf] == 0.0).all() and np.isnan(got[np.isnan(z)]).all()
        assert (got[z >= 1e4] == 1.0).all() and (got[z <= -1e4] == 0.0).all() and (got[z == 0] == 0.5).all()


# ------------------------------------------------------------------------------------------------------------------
# 2. everything downstream, bit for bit
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,listed", SHAPES)
@pytest.mark.parametrize("D", [3, 8, 21])
@pytest.mark.parametrize("E", [7, 5, 3])
def test_variance_pessimistic_cost_and_clip_on_the_devices_own_probabilities(hip_lib, E, D, n, listed):
    tt._need_gpu()
    c = _case(E, D, n, listed)
    el = c.inds[c.live]
    cc = ref.cost_column(D)
    KAPPA = 1.5
    for shift in (0.0, 0.7):
        p = _member_probs(c, shift)
        p_el = p[el, np.arange(n)]
        want_k, var = ref.downstream(p, el, KAPPA)
        want_0, _ = ref.downstream(p, el, 0.0)
        _same(want_0, p_el)
        with np.errstate(invalid="ignore", over="ignore"):
            raw = (p_el + (np.float32(KAPPA) * np.sqrt(var)).astype(np.float32)).astype(np.float32)
        assert (raw > 1).sum() >= max(1, n // 8) and (raw <= 1).sum() >= 1, ((raw > 1).sum(), n)      # rows the clip cuts, rows it leaves
        assert (want_k[raw > 1] == 1.0).all()
        for kind in c.kinds():
            for xi in (False, True):
                tag = f"shift {shift} {kind} xi={xi}"
                got = _launch(c, kind, xi=xi, kappa=(0.75, KAPPA), cost=(1, shift))
                _same(got["cost_var"][c.live], var, tag + " cost_var")
                _same(got["cost"][c.live], want_k, tag + " pessimistic cost")
                _same(got["cost_logit"][c.live], c.z[el, c.live], tag + " cost_logit")
                fin = ~np.isnan(got["cost"][c.live])
                assert (got["cost"][c.live][fin] <= 1).all() and (got["cost"][c.live][fin] >= 0).all()
                # kappa_cost == 0 with the variance measured, and no disagreement at all: the elite's probability, bit for bit
                zero = _launch(c, kind, xi=xi, kappa=(0.75, 0.0), cost=(1, shift))
                _same(zero["cost"][c.live], p_el, tag + " kappa 0")
                _same(zero["cost_var"][c.live], var, tag + " kappa 0 cost_var")
                none = _launch(c, kind, xi=xi, cost=(1, shift), logit_out=False)
                _same(none["cost"][c.live], p_el, tag + " no disagreement")
                assert (none["cost_logit"] == -7.0).all() and (none["cost_var"] == -7.0).all()        # NULL outputs stay untouched
                if len(c.rest):      # unlisted slots keep their sentinels
                    assert (got["cost"][c.rest] == -7.0).all() and (got["cost_logit"][c.rest] == -7.0).all()
        if shift != 0.0:
            # zs = fl32(z - shift): the same call with shift 0 over logits the host has shifted, an instance that was never
            # given a shift -- the same probabilities bit for bit (cost_logit is the raw column of each)
            pre = c.mean.copy()
            pre[:, :, cc] = (c.z - np.float32(shift)).astype(np.float32)
            pre_t = torch.from_numpy(pre).to(DEV)
            for kappa in (None, (0.75, KAPPA)):
                a = _launch(c, "default", kappa=kappa, cost=(1, shift))
                b = _launch(c, "default", mean=pre_t, kappa=kappa, cost=(1, 0.0))
                for k in ("cost", "cost_var"):
                    _same(a[k], b[k], f"host-shifted {k}")
                _same(b["cost_logit"][c.live], pre[el, c.live, cc])
        else:
            # a shift of -0.0 is a shift of 0: no subtraction
            a, b = _launch(c, "default", kappa=(0.75, KAPPA), cost=(1, 0.0)), _launch(c, "default", kappa=(0.75, KAPPA), cost=(1, -0.0))
            for k in a:
                np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"-0.0 {k}")


# ------------------------------------------------------------------------------------------------------------------
# 3. / 4. kind 0 and ch == NULL are the existing call; the head moves the cost and nothing else
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,listed", SHAPES)
@pytest.mark.parametrize("D", [3, 8, 21])
@pytest.mark.parametrize("E", [7, 5, 3])
def test_magnitude_reading_is_the_term_entry_and_nothing_else_moves(hip_lib, E, D, n, listed):
    tt._need_gpu()
    for term in (False, True):
        c = _case(E, D, n, listed, term)
        head = (tt.THR, "majority") if term else None
        for kind in c.kinds():
            for xi in (False, True):
                for kappa in (None, (0.75, 1.5)):
                    tag = f"term={term} {kind} xi={xi} dis={kappa is not None}"
                    old = _launch(c, kind, xi=xi, kappa=kappa, head=head, cost=None, entry="cmbpo_fakeenv_post_term")
                    for ch in (None, (0, 0.0), (0, 0.37)):                 # ch == NULL; kind 0 (its shift is not read)
                        new = _launch(c, kind, xi=xi, kappa=kappa, head=head, cost=ch)
                        for k in old:                                       # every output slot, the untouched ones included
                            np.testing.assert_array_equal(_bits(new[k]), _bits(old[k]), err_msg=f"{tag} ch={ch} {k}")
                        assert (new["cost_logit"] == -7.0).all()
                    # the logistic head on the same mean / var: the cost (and its variance) change, nothing else does
                    on = _launch(c, kind, xi=xi, kappa=kappa, head=head, cost=(1, 0.3))
                    for k in old:
                        if k not in ("cost", "cost_var", "cost_logit"):
                            np.testing.assert_array_equal(_bits(on[k]), _bits(old[k]), err_msg=f"{tag} logistic {k}")
                    assert (on["cost"][c.live] != old["cost"][c.live]).mean() > 0.5
                    _same(on["cost_logit"][c.live], c.z[c.inds[c.live], c.live], tag)
                    if term:      # the termination column stayed the last one: both values of the learned verdict occur
                        assert on["term_votes"][c.live].min() < E and on["term_votes"][c.live].max() > 0
                        assert set(np.unique(on["term"][c.live])) == {0, 1}


# ------------------------------------------------------------------------------------------------------------------
# 5. the rollout: cmbpo_rollout_step with the head attached against the per-call path
# ------------------------------------------------------------------------------------------------------------------
def _hip_world(w, B, shift, term):
    from cmbpo_amd.cpo_policy import CPOPolicy
    from cmbpo_amd.fake_env import FakeEnv
    from cmbpo_amd.model_sampler import ModelSampler
    from cmbpo_amd.modelbuffer import ModelBuffer
    from cmbpo_amd.pens import PE
    D, A_, T = w["obs_dim"], w["act_dim"], tt.T
    E = w["ws"][0].shape[0]
    model = PE(D + A_, w["out_dim"], hidden_dims=(tt.HIDDEN, tt.HIDDEN), num_networks=E, num_elites=len(w["elites"]),
               loss="MSPE", use_scaler_in=True, use_scaler_out=True, device=DEV)
    model.set_weights(w["ws"], w["bs"], w["sc_in"], w["sc_out"])
    model.set_elites(w["elites"])
    policy = CPOPolicy(tt._Space(D), tt._Space(A_), a_hidden_layer_sizes=(128, 128), vf_hidden_layer_sizes=(128, 128),
                       vf_ensemble_size=3, vf_elites=2, vf_activation="swish", vf_loss="MSE", device=DEV,
                       cost_gamma=0.97, cost_lam=0.5, lam=0.95)
    policy.actor.set_params(w["pol"])
    policy.v.set_weights(*w["v"])
    policy.vc.set_weights(*w["vc"])
    kw = dict(predicts_term=True, term_threshold=tt.NEVER, term_members="elite") if term else {}
    if shift is not None:
        kw.update(cost_loss="logistic", cost_logit_shift=shift)
    env = FakeEnv(tt._Env(D, A_), tt.TASK, model, predicts_delta=True, predicts_rew=True, predicts_cost=True,
                  disagreement=True, cost_pessimism=0.5, **kw)
    pool = ModelBuffer(B, D, A_, T, device=DEV)
    pool.initialize(policy.pi_info_shapes, gamma=0.99, lam=0.95, cost_gamma=0.97, cost_lam=0.5)
    sampler = ModelSampler(max_path_length=T + 5, batch_size=B, rollout_mode="uncertainty")
    sampler.initialize(env, policy, pool)
    sampler.set_rollout_dkl(float("inf"))
    return sampler, pool, env


def _roll(w, start, shift, term, how):
    """A whole rollout with the sampler's own draws.  how: 'step' (cmbpo_rollout_step), 'calls' (the per-call path: policy,
    forward, FakeEnv.step_device -> cmbpo_fakeenv_post_cost, bookkeeping entries) or 'many' (cmbpo_rollout_run)."""
    sampler, pool, env = _hip_world(w, start.shape[0], shift, term)
    if how == "calls":
        env.kernel_events = []
    sampler._gen.manual_seed(5)
    sampler.reset(start)
    assert pool.cost_head == (None if shift is None else ("logistic", shift)) and ("cost_logit_t" in pool.t) == (shift is not None)
    costs, logits = [], []
    while sampler.any_alive() and pool.has_room:
        if how == "many":
            sampler.sample_many()
            continue
        ids = pool.t["alive_idx"][:pool.n_alive].long()
        sampler.sample()
        costs.append(pool.t["cost_t"][ids].cpu().numpy())
        if shift is not None:
            logits.append(pool.t["cost_logit_t"][ids].cpu().numpy())
    sampler.finish_all_paths()
    return pool.get()[0], costs, logits


@pytest.mark.parametrize("B,term", [(96, False), (96, True), (1000, True)])
def test_rollout_step_with_the_head_is_the_per_call_path_bitwise(hip_lib, B, term):
    tt._need_gpu()
    w, start = tt.build_world_term(31, term=term), tt._start(32, B)
    step, costs, logits = _roll(w, start, 0.25, term, "step")
    calls, costs_c, logits_c = _roll(w, start, 0.25, term, "calls")
    assert len(costs) == len(costs_c) >= 3
    for k, a, b in zip(tt.NAMES, step, calls):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=k)
    for a, b in zip(costs + logits, costs_c + logits_c):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    # the costs are probabilities (pessimistic, clipped), and the logits are not
    cost, logit = np.concatenate(costs), np.concatenate(logits)
    assert ((cost >= 0) & (cost <= 1)).all() and (np.abs(logit) > 1).any()
    stored = step[tt.NAMES.index("cost")]
    assert ((stored >= 0) & (stored <= 1)).all()
    # the same world read as a magnitude stores other costs: the head is what made them probabilities
    plain, costs_p, _ = _roll(w, start, None, term, "step")
    assert costs_p[0].shape == costs[0].shape and not np.array_equal(costs_p[0], costs[0])       # (the first step: the same rows)
    assert (np.concatenate(costs_p) > 1).any() or (np.concatenate(costs_p) < 0).any()
    if B == 96:
        many, _, _ = _roll(w, start, 0.25, term, "many")
        for k, a, b in zip(tt.NAMES, step, many):
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg="run " + k)


def test_attached_step_refuses_a_task_or_model_without_the_column(hip_lib):
    tt._need_gpu()
    from cmbpo_amd import _lib
    from cmbpo_amd._lib import CmbpoHipError
    w = tt.build_world_term(31, term=False)
    sampler, pool, env = _hip_world(w, 40, None, False)
    sampler.reset(tt._start(3, 40))
    pool.set_cost_head("logistic", 0.0)
    sampler.sample()                               # the column is there: the head reads it
    assert pool.ptr == 1
    env._task_id &= ~_lib.TASK_LEARNED_COST        # ... and without the flag the step is refused before its first launch
    cur = pool.t["cur_obs"].clone()
    with pytest.raises(CmbpoHipError) as e:
        sampler.sample()
    assert "cmbpo_rollout_step" in str(e.value) and "cost head" in str(e.value) and "CMBPO_TASK_LEARNED_COST" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert pool.ptr == 1 and torch.equal(pool.t["cur_obs"], cur)
    # a model one column wider than obs + 2 with no termination head attached
    w3 = tt.build_world_term(31, term=True)
    sampler, pool, env = _hip_world(w3, 40, None, True)
    sampler.reset(tt._start(3, 40))
    pool.set_term_head(False)
    pool.set_cost_head("logistic", 0.0)
    with pytest.raises(CmbpoHipError) as e:
        sampler.sample()
    assert "cmbpo_rollout_step" in str(e.value) and "cost head" in str(e.value) and "out_dim" in str(e.value), str(e.value)
    assert pool.ptr == 0


# ------------------------------------------------------------------------------------------------------------------
# 6. ModelBuffer's side arrays
# ------------------------------------------------------------------------------------------------------------------
def test_model_buffer_cost_logit_array_follows_the_switch(hip_lib):
    tt._need_gpu()
    from cmbpo_amd.modelbuffer import _SIDE, ModelBuffer
    assert list(_SIDE)[-1] == "cost" and _SIDE["cost"].attach == "cmbpo_rollout_cost_head_attach"
    buf = ModelBuffer(4, 5, 2, 2, device=DEV)
    buf.set_term_head(True, 0.5, "majority")
    base = dict(buf.t)
    assert "cost_logit_t" not in base and buf.cost_head is None
    buf.set_cost_head("logistic", 0.3)
    first = buf.t["cost_logit_t"]
    assert set(buf.t) == set(base) | {"cost_logit_t"} and first.shape == (4,) and first.dtype == torch.float32
    buf.set_cost_head("logistic", 0.3)                      # nothing changed: the same array
    assert buf.t["cost_logit_t"] is first
    buf.set_cost_head("logistic", -1.0)                     # a new shift: attached anew over the same array
    assert buf.t["cost_logit_t"] is first and buf.cost_head == ("logistic", -1.0)
    buf.set_cost_head("gaussian")
    assert set(buf.t) == set(base) and buf.cost_head is None
    buf.set_cost_head("logistic", 0.0)
    assert "cost_logit_t" in buf.t and buf.t["cost_logit_t"] is not first
    for k, v in base.items():
        assert buf.t[k] is v, k                             # the other features' arrays are the same tensors throughout
    buf.reset(batch_size=6)                                 # a new batch size: every array anew, the features still on
    assert buf.t["cost_logit_t"].shape == (6,) and buf.t["term_votes_t"].shape == (6,)
    with pytest.raises(ValueError, match="cost_loss"):
        buf.set_cost_head("probit")
    with pytest.raises(ValueError, match="cost_logit_shift"):
        buf.set_cost_head("logistic", float("inf"))


# ------------------------------------------------------------------------------------------------------------------
# 7. the replay
# ------------------------------------------------------------------------------------------------------------------
_REPLAY_ENV = {}


def _replay_env(term):
    """tt._replay_env's model (a 128-wide AntSafe-shaped ensemble with small steps) with the cost column spread over a few
    units of logit, read by a FakeEnv with the logistic cost head (and, with `term`, the termination head behind it)."""
    if term in _REPLAY_ENV:
        return _REPLAY_ENV[term]
    from cmbpo_amd import synthetic
    from cmbpo_amd.fake_env import FakeEnv
    from cmbpo_amd.pens import PE
    D, A_ = synthetic.ENV_DIMS[tt.TASK]
    E, O = 5, D + 2 + int(term)
    rng = np.random.default_rng(zlib.crc32(b"cost-head/replay-model"))
    ws, bs = synthetic.ensemble_weights(rng, E, D + A_, 128, 2 * O, bias_scale=0.05)
    sc_in = synthetic.scaler(rng, D + A_)
    mu, var = np.zeros((1, O), np.float32), np.full((1, O), 2.5e-3, np.float32)
    mu[0, D + 1], var[0, D + 1] = -0.3, 100.0
    if term:
        mu[0, O - 1], var[0, O - 1] = 0.4, 1.0
    np.random.seed(5)
    model = PE(D + A_, O, hidden_dims=(128, 128), num_networks=E, num_elites=3, loss="MSPE", use_scaler_in=True,
               use_scaler_out=True, device=DEV)
    model.set_weights(ws, bs, sc_in, (mu, var))
    kw = dict(predicts_term=True, term_threshold=0.9, term_members="any") if term else {}
    env = FakeEnv(tt._Env(D, A_), tt.TASK, model, True, True, True, seed=3, cost_loss="logistic", cost_logit_shift=0.2, **kw)
    _REPLAY_ENV[term] = (env, D, A_, E)
    return _REPLAY_ENV[term]


@pytest.mark.parametrize("mode,B,term,calibration", [("open_loop", 65, False, False), ("one_step", 257, True, True)])
def test_replay_run_cost_is_the_loop_of_single_calls_bitwise(hip_lib, mode, B, term, calibration):
    tt._need_gpu()
    from test_replay_gpu import _recording
    H = 5
    env, D, A_, E = _replay_env(term)
    rng = np.random.default_rng(zlib.crc32(f"cost-head/{B}/{H}/{mode}".encode()))
    obs0, act, rec, lengths = _recording(rng, B, H, D, A_)
    inds = rng.integers(0, E, (H, B)).astype(np.int32)
    inds_d = torch.from_numpy(inds).to(DEV)
    # a shift that puts the first step's probabilities on both sides of the table's 0.5
    shift = float(np.median(env._model.predict_ensemble(obs0, act=act[0])[0][:, :, D + 1]))
    env.set_cost_head(logit_shift=shift)
    a = tt._replay_buffers(env, obs0, act, rec, lengths, mode, calibration)
    th, ch = env.term_head_struct(), env.cost_head_struct()
    assert ch.kind == 1 and (th is not None) == term
    if calibration:
        a.run_calibrated(env._model.mlp.handle, env._task_id, E, inds_d, term_head=th, cost_head=ch)
    else:
        a.run(env._model.mlp.handle, env._task_id, E, inds_d, term_head=th, cost_head=ch)
    c = tt._replay_buffers(env, obs0, act, rec, lengths, mode, calibration)
    if calibration:
        c.set_elite(inds_d)
    seen = []
    for h in range(H):
        env.step_device(c.t["cur_obs"], c.t["act"][h], inds_d[h], c.step_outputs(), scratch=(c.t["mean"], c.t["var"]))
        seen.append(c.t["p_cost"].cpu().numpy().copy())
        if calibration:
            c.calibrate(h)
        c.compare(h)
    c.finish()
    if calibration:
        c.calib_finish()
    torch.cuda.synchronize()
    for k in ("sums", "counts", "cur_obs", "alive", "p_term", "p_next_obs", "p_cost"):
        assert torch.equal(a.t[k], c.t[k]), k
    if calibration:
        for k in ("sums", "counts"):
            assert torch.equal(a.c[k], c.c[k]), "calibration " + k
    # p_cost is a probability, on both sides of the table's 0.5
    p = np.concatenate(seen)
    p = p[np.isfinite(p)]
    assert ((p >= 0) & (p <= 1)).all() and (p > 0.5).any() and (p < 0.5).any()
    tab = a.table()
    assert tab["cost_cm"][:, :, 1].sum() > 0 and tab["cost_cm"][:, :, 0].sum() > 0
    # the cost's squared error of a probability against a 0 / 1 recording is a Brier score: inside [0, 1]
    assert set(np.unique(rec["cost"])) <= {0.0, 1.0}
    assert (tab["mse_cost"][tab["n"] > 0] <= 1.0).all()
    # FakeEnv.replay is that call; the magnitude reading of the same model gives another table
    args = (obs0, act, rec["next_obs"], rec["rew"], rec["cost"], rec["term"])
    got = env.replay(*args, lengths=lengths, model_inds=inds, mode=mode, calibration=calibration)
    for k in ("n", "term_cm", "cost_cm", "se_obs", "se_cost"):
        np.testing.assert_array_equal(got[k], tab[k], err_msg=k)
    env.set_cost_head("gaussian", 0.0)
    try:
        mag = env.replay(*args, lengths=lengths, model_inds=inds, mode=mode, calibration=calibration)
    finally:
        env.set_cost_head("logistic", shift)
    assert not np.array_equal(mag["se_cost"], got["se_cost"])
    np.testing.assert_array_equal(mag["se_obs"][0], got["se_obs"][0])      # (the first step's observations do not depend on it)


# ------------------------------------------------------------------------------------------------------------------
# 8. FakeEnv.step
# ------------------------------------------------------------------------------------------------------------------
def test_fake_env_step_reports_the_probability_and_the_logit(hip_lib):
    tt._need_gpu()
    env, D, A_, E = _replay_env(True)
    rng = np.random.default_rng(9)
    n = 333
    obs = tt._start(10, n)
    act = rng.uniform(-1, 1, (n, A_)).astype(np.float32)
    inds = rng.integers(0, E, n).astype(np.int32)
    mean, _ = env._model.predict_ensemble(obs, act=act)
    z = mean[inds, np.arange(n), D + 1]
    shift = env.cost_logit_shift
    assert env.cost_loss == "logistic" and shift != 0.0 and np.ptp(z) > 0.5
    _, _, _, info = env.step(obs, act, model_inds=inds)
    assert info["cost"].shape == (n, 1) and info["cost"].dtype == np.float32 and info["cost_logit"].dtype == np.float32
    np.testing.assert_array_equal(_bits(info["cost_logit"]), _bits(z))
    zs = (z - np.float32(shift)).astype(np.float32)
    assert (np.abs(info["cost"][:, 0].astype(np.float64) - ref.sigma64(zs)) <= ref.sigma_bound(zs)).all()
    assert ((info["cost"] >= 0) & (info["cost"] <= 1)).all()
    # CUDA tensors in, CUDA tensors out
    _, _, _, info_t = env.step(torch.from_numpy(obs).to(DEV), torch.from_numpy(act).to(DEV), model_inds=inds)
    assert info_t["cost_logit"].is_cuda and torch.equal(info_t["cost_logit"].cpu(), torch.from_numpy(info["cost_logit"]))
    # the magnitude reading: the raw column as the cost, no new key
    env.set_cost_head("gaussian", 0.0)
    try:
        _, _, _, plain = env.step(obs, act, model_inds=inds)
    finally:
        env.set_cost_head("logistic", shift)
    assert "cost_logit" not in plain
    np.testing.assert_array_equal(_bits(plain["cost"][:, 0]), _bits(z))
    for k in ("rew", "ensemble_dkl_path", "ensemble_ep_var", "term_pred", "term_votes"):
        np.testing.assert_array_equal(_bits(plain[k]), _bits(info[k]), err_msg=k)
