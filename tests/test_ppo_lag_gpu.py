"""GPU: the first-order penalised update (PPO-Lagrangian) against its float64 reference (tests/ppo_lag_ref.py).

Tolerances are those of tests/test_cpo_update_gpu.py (the objective is the same sum with some terms masked): gradients
|d| <= 1e-3 |ref| + 3e-5 max|ref|, scalar sums rtol 2e-4 / atol 1e-6 (KL atol 1e-7), quantities at the end of an iterated
update rtol 2e-2 / atol 1e-7.  Rows whose float64 ratio lies within 1e-3 of a clip edge are removed before binding (a
condition, capped at 2 % of the rows): the clip mask is then the same in float32 and float64 and the clip count is compared
exactly.  Everything that is "the same kernels in the same order" is compared bit for bit; the one exception is the eight
"post" sums of the loop's final cmbpo_pi_eval, whose float64 atomics add in no fixed order (rtol 1e-12).
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import ppo_lag_ref as ref  # noqa: E402

KEYS = ("obs", "act", "adv", "cadv", "logp_old", "cost", "mu_old", "log_std_old")
SHAPES = [(29, 8, 1037, 128), (47, 17, 500, 128), (21, 3, 31, 128), (3, 1, 1, 128), (64, 32, 257, 128),
          (29, 8, 4099, 256), (3, 1, 33, 256)]
CLIP = 0.2
T = 35


@pytest.fixture(autouse=True, params=[1, 0], ids=["splitf16", "fp32mfma"])
def pi_path(request, hip_lib):
    """Every test of this file on both arithmetic paths of the 128 x 128 products (cmbpo_set_pi_matrix_path)."""
    before = hip_lib.cmbpo_get_pi_matrix_path()
    hip_lib.cmbpo_set_pi_matrix_path(request.param)
    yield request.param
    hip_lib.cmbpo_set_pi_matrix_path(before)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _close(got, want, rtol=1e-3, arel=3e-5, msg=""):
    np.testing.assert_allclose(got, want, rtol=rtol, atol=arel * float(np.max(np.abs(want))) + 1e-12, err_msg=msg)


class _Space:
    def __init__(self, d):
        self.shape = (d,)


_CASES = {}


def _case(D, A, n, hidden):
    """Batch of seed D*100 + A, parameters shift * N(0,1) off theta_old, a few rows with adv == 0 / cadv == 0, rows on a clip
    edge removed; the float64 reference results are computed once per case and shared."""
    key = (D, A, n, hidden)
    if key in _CASES:
        return _CASES[key]
    from worlds import make_update_batch
    rng = np.random.default_rng(D * 100 + A)
    params, batch = make_update_batch(rng, n, D, A, hidden, 0.3, 1.0, T)
    shift = 0.03 if D == 3 else 0.01
    p = (params + shift * rng.standard_normal(params.shape)).astype(np.float32)
    if n >= 31:
        batch["adv"][[1, n // 2, n - 2]] = 0.0
        batch["cadv"][[2, n // 3, n - 1]] = 0.0
    ratio = ref.Surrogate(ref.make_graph(D, A, batch, hidden=hidden), CLIP).ratio(p)
    keep = (np.abs(ratio - (1 - CLIP)) > 1e-3) & (np.abs(ratio - (1 + CLIP)) > 1e-3)
    assert (~keep).sum() <= 0.02 * n, "clip-edge filter removed %d of %d rows" % ((~keep).sum(), n)
    batch = {k: np.ascontiguousarray(v[keep]) for k, v in batch.items()}
    graph = ref.make_graph(D, A, batch, hidden=hidden, max_path_length=T)
    ratio = ratio[keep]
    m = int(keep.sum())
    if n >= 31:      # a run in which nothing clips cannot pass
        s = ref.Surrogate(graph, CLIP).sums(p)
        assert 0.1 <= s[5] / m <= 0.9, s[5] / m
        assert (ratio > 1 + CLIP).any() and (ratio < 1 - CLIP).any()
    c = dict(D=D, A=A, n=m, hidden=hidden, params=params, p=p, batch=batch, graph=graph, refs={})
    _CASES[key] = c
    return c


def _ref(c, penalty, clipped, penalized=True):
    k = (penalty, clipped, penalized)
    if k not in c["refs"]:
        sur = ref.Surrogate(c["graph"], CLIP, clipped_adv=clipped, objective_penalized=penalized)
        c["refs"][k] = (sur.grad(c["p"], penalty), sur.sums(c["p"]))
    return c["refs"][k]


def _ops(c, params=None):
    from cmbpo_amd.cpo_update import PolicyOps
    ops = PolicyOps(c["D"], c["A"], c["hidden"], device="cuda:0")
    ops.set_params(c["p"] if params is None else params)
    ops.bind(*[c["batch"][k] for k in KEYS])
    return ops


def _set_penalty(ops, penalty):
    """the three derived slots of the state block, directly (penalty 0 has no finite penalty_param)"""
    from cmbpo_amd import _lib
    ops.ppo_state[_lib.PPO_ST_PENALTY:_lib.PPO_ST_CC + 1] = torch.tensor(
        [penalty, 1.0 / (1.0 + penalty), penalty / (1.0 + penalty)], dtype=torch.float64, device=ops.device)


def _check_sums(s, s_ref, n):
    assert s[0] == n == s_ref[0]
    for k in (1, 2, 6):
        np.testing.assert_allclose(s[k] / n, s_ref[k] / n, rtol=2e-4, atol=1e-6, err_msg="sum %d" % k)
    np.testing.assert_allclose(s[3] / n, s_ref[3] / n, rtol=2e-4, atol=1e-7, err_msg="kl")
    np.testing.assert_allclose(s[4], s_ref[4], rtol=1e-6)
    assert s[5] == s_ref[5], "clip count %r != %r" % (s[5], s_ref[5])
    assert s[7] == 0


@pytest.mark.parametrize("D,A,n,hidden", SHAPES)
def test_gradient_and_sums_match_the_float64_reference(hip_lib, D, A, n, hidden):
    _need_gpu()
    c = _case(D, A, n, hidden)
    ops = _ops(c)
    for penalty in (0.0, 1.0, 7.5):
        for clipped in (True, False):
            g_ref, s_ref = _ref(c, penalty, clipped)
            _set_penalty(ops, penalty)
            g, s = ops.ppo_grad(ops.ppo_cfg(clip_ratio=CLIP, clipped_adv=clipped, objective_penalized=True))
            _close(g, g_ref, msg="penalty %g clipped %s" % (penalty, clipped))
            _check_sums(s, s_ref, c["n"])
            if clipped and c["n"] >= 31:
                assert s[1] != s[6]


@pytest.mark.parametrize("D,A,n,hidden", SHAPES)
def test_without_clip_and_penalty_it_is_the_existing_gradient_kernel(hip_lib, D, A, n, hidden):
    _need_gpu()
    c = _case(D, A, n, hidden)
    ops = _ops(c)
    _set_penalty(ops, 7.5)      # ignored with objective_penalized off
    g, s = ops.ppo_grad(ops.ppo_cfg(clip_ratio=CLIP, clipped_adv=False, objective_penalized=False))
    g0, s0 = ops.loss_grad(0)
    print("ppo_grad == loss_grad(0) bit for bit at %r: %s" % ((D, A, n, hidden), np.array_equal(g, g0)))
    _close(g, g0)
    ev = ops.evals()
    np.testing.assert_allclose(s[3] / s[0], ev[3] / ev[0], rtol=2e-4, atol=1e-7)
    assert s[5] == 0 and s[1] == s[6]
    np.testing.assert_allclose(s[6], s0[1], rtol=1e-12)


def test_adam_step_matches_float64_tf_adam(hip_lib):
    """float32 arithmetic against float64 on the same vectors, nothing summed over samples: per step and entry the change of
    the parameter agrees within 1e-5 lr + 2 ulp(theta)."""
    _need_gpu()
    from cmbpo_amd import _lib
    from cmbpo_amd.cpo_update import PolicyOps
    ops = PolicyOps(3, 1, 128, device="cuda:0")
    rng = np.random.default_rng(5)
    P, lr = ops.P, 1e-3
    theta0 = rng.standard_normal(P).astype(np.float32)
    special = np.array([0.0, 1e-12, -1e-12, 1e3, -1e3], np.float32)
    worst = 0.0
    for same in (True, False):
        ops.params.copy_(torch.from_numpy(theta0))
        ops.adam_m.zero_()
        ops.adam_v.zero_()
        ops.ppo_state.zero_()
        th, m, v, t = theta0.astype(np.float64), np.zeros(P), np.zeros(P), 0
        prev = theta0.astype(np.float64)
        gmax = np.zeros(P)
        for step in range(5):
            if step == 0 or not same:
                g = (rng.standard_normal(P) * 10.0 ** rng.uniform(-6, 1, P)).astype(np.float32)
                g[:50] = np.tile(special, 10)
                if not same:
                    g[:50] = np.roll(g[:50], step)
            gmax = np.maximum(gmax, np.abs(g))
            ops.adam_step(g, lr)
            # (the betas as the float32 values the C-ABI takes: 1 - 0.999f differs from 0.001 by 1.3e-5 of itself)
            th_new, m, v, t = ref.adam_step(th, m, v, t, g.astype(np.float64), lr, b1=float(np.float32(0.9)),
                                            b2=float(np.float32(0.999)))
            got = ops.params.cpu().numpy().astype(np.float64)
            err = np.abs((got - prev) - (th_new - th))
            bound = 1e-5 * lr + 2 * np.spacing(np.abs(got).astype(np.float32)).astype(np.float64)
            worst = max(worst, float(np.max(err / bound)))
            assert np.all(err <= bound), "step %d: worst %g of the bound" % (step, float(np.max(err / bound)))
            prev, th = got, th_new
        assert float(ops.ppo_state[_lib.PPO_ST_ADAM_T]) == 5
        # the moments: float32 rounding of the largest term that went into them (a 1e3 followed by a 1e-12 cancels)
        assert np.all(np.abs(ops.adam_m.cpu().numpy() - m) <= 1e-5 * np.abs(m) + 1e-6 * gmax)
        assert np.all(np.abs(ops.adam_v.cpu().numpy() - v) <= 1e-5 * np.abs(v) + 1e-6 * gmax ** 2)
    print("adam_step: worst error %.3f of the bound" % worst)


def _host_step(ops, cfg, sums):
    """one iteration of the loop, driven from the host: ppo_grad -> scale (inside ppo_grad_dev) and entropy term -> adam_step
    -> set_params"""
    from cmbpo_amd import _lib
    g = ops.ppo_grad_dev(cfg, ops.work["g"], sums)
    if cfg.ent_reg:
        c_r = np.float32(float(ops.ppo_state[_lib.PPO_ST_CR])) if cfg.objective_penalized else np.float32(1.0)
        g[-ops.A:] -= float(c_r * np.float32(cfg.ent_reg))
    ops.adam_step(g, cfg.pi_lr, cfg.beta1, cfg.beta2, cfg.adam_eps)
    ops.set_params(ops.params)


def _state(ops):
    return ops.ppo_state.cpu().numpy()


@pytest.mark.parametrize("D,A,n,hidden", SHAPES)
def test_the_loop_is_its_own_composition(hip_lib, D, A, n, hidden):
    _need_gpu()
    from cmbpo_amd import _lib as L
    c = _case(D, A, n, hidden)
    run, host = _ops(c), _ops(c)
    pen_param = float(np.log(np.e - 1))
    for ops in (run, host):
        ops.set_penalty_param(pen_param)
    cfg = run.ppo_cfg(clip_ratio=CLIP, ent_reg=0.01, pi_lr=3e-4, target_kl=1e9)
    run.ppo_run(cfg, 3)
    firsts = None
    for it in range(3):
        _host_step(host, cfg, host.ppo_sums)
        last = host.ppo_sums.cpu().numpy()
        firsts = last if it == 0 else firsts
    np.testing.assert_array_equal(run.get_params(), host.get_params())
    assert np.max(np.abs(run.get_params() - c["p"])) > 0
    np.testing.assert_array_equal(run.adam_m.cpu().numpy(), host.adam_m.cpu().numpy())
    np.testing.assert_array_equal(run.adam_v.cpu().numpy(), host.adam_v.cpu().numpy())
    a, b = _state(run), _state(host)
    np.testing.assert_array_equal(a[L.PPO_ST_ADAM_T:L.PPO_ST_CC + 1], b[L.PPO_ST_ADAM_T:L.PPO_ST_CC + 1])
    assert a[L.PPO_ST_STOP] == 0 and a[L.PPO_ST_ITERS] == 3 and a[L.PPO_ST_ADAM_T] == 3
    np.testing.assert_array_equal(a[L.PPO_ST_PRE:L.PPO_ST_PRE + 8], firsts)
    assert a[L.PPO_ST_KL] == last[3] / last[0] and a[L.PPO_ST_CLIP] == last[5]
    np.testing.assert_allclose(a[L.PPO_ST_POST:L.PPO_ST_POST + 8], host.evals(), rtol=1e-12)


def test_the_gate_stops_where_the_reference_stops(hip_lib):
    _need_gpu()
    from cmbpo_amd import _lib as L
    D, A, n, hidden, lr, margin = 29, 8, 1037, 128, 3e-3, 1.2
    c = _case(D, A, n, hidden)
    theta_old = c["params"]
    sur = ref.Surrogate(c["graph"], CLIP)
    penalty = ref.softplus(float(np.log(np.e - 1)))
    P = theta_old.size
    free = ref.run_loop(sur, theta_old, np.zeros(P), np.zeros(P), 0, penalty, lr, 6, np.inf)
    k = 3                                                    # stop at iteration 3: two steps are taken
    kl_lim = float(np.sqrt(free["kls"][k - 2] * free["kls"][k - 1]))
    target_kl = kl_lim / margin
    r = ref.run_loop(sur, theta_old, np.zeros(P), np.zeros(P), 0, penalty, lr, 20, margin * target_kl)
    assert r["stop"] == k and 2 <= k <= 10 and r["t"] == k - 1
    assert np.all(r["kls"][:k - 1] <= 0.9 * margin * target_kl) and r["kls"][k - 1] >= 1.1 * margin * target_kl, r["kls"]

    run, host = _ops(c, theta_old), _ops(c, theta_old)
    for ops in (run, host):
        ops.set_penalty_param(float(np.log(np.e - 1)))
    cfg = run.ppo_cfg(clip_ratio=CLIP, pi_lr=lr, target_kl=target_kl, kl_margin=margin)
    run.ppo_run(cfg, 20)
    for _ in range(k - 1):
        _host_step(host, cfg, host.ppo_sums)
    st = _state(run)
    assert st[L.PPO_ST_STOP] == k, st[:4]
    assert st[L.PPO_ST_ADAM_T] == k - 1 and st[L.PPO_ST_ITERS] == k - 1
    np.testing.assert_array_equal(run.get_params(), host.get_params())
    np.testing.assert_array_equal(run.adam_m.cpu().numpy(), host.adam_m.cpu().numpy())
    np.testing.assert_allclose(st[L.PPO_ST_KL], r["kls"][k - 1], rtol=2e-2)
    # the handle holds the surviving parameters too: the post measures are theirs
    np.testing.assert_allclose(st[L.PPO_ST_POST:L.PPO_ST_POST + 8], host.evals(), rtol=1e-12)
    # the stop word stays set until the next run, and the building block does not look at it: ppo_grad on the stopped ops is
    # ppo_grad of a fresh ops at the same parameters, not a sum of whatever partials the loop left behind
    assert _state(run)[L.PPO_ST_STOP] == k
    fresh = _ops(c, run.get_params())
    fresh.set_penalty_param(float(np.log(np.e - 1)))
    g_run, s_run = run.ppo_grad(cfg)
    g_new, s_new = fresh.ppo_grad(cfg)
    np.testing.assert_array_equal(g_run, g_new)
    np.testing.assert_array_equal(s_run, s_new)
    assert s_run[0] == c["n"] and np.abs(g_run).max() > 0
    _close(g_run, sur.grad(run.get_params().astype(np.float64), penalty), msg="gradient after a stopped run")
    assert _state(run)[L.PPO_ST_STOP] == k
    # a second run starts from a clear stop word
    run.ppo_run(run.ppo_cfg(clip_ratio=CLIP, pi_lr=lr, target_kl=1e9), 1)
    assert _state(run)[L.PPO_ST_STOP] == 0 and _state(run)[L.PPO_ST_ADAM_T] == k


AGENT = dict(pi_lr=3e-4, pi_iters=10)      # with target_kl 0.01 the reference stops at 3, 4, 5 with >= 20 % to the threshold


def _policy(D, A, hidden=128, **kw):
    from cmbpo_amd.cpo_policy import CPOPolicy
    return CPOPolicy(_Space(D), _Space(A), a_hidden_layer_sizes=(hidden, hidden), vf_hidden_layer_sizes=(128, 128),
                     vf_ensemble_size=3, vf_elites=2, vf_activation="swish", vf_loss="MSE", device="cuda:0",
                     max_path_length=T, **kw)


def _buf(batch):
    z = np.zeros(batch["obs"].shape[0], np.float32)
    return [batch["obs"], batch["act"], batch["adv"], batch["cadv"], z, z, batch["logp_old"], z, z, batch["cost"],
            batch["log_std_old"], batch["mu_old"]]


def test_agent_matches_the_reference_agent_and_survives_a_checkpoint(hip_lib, tmp_path):
    _need_gpu()
    from worlds import make_update_batch
    D, A, n, hidden = 29, 8, 1037, 128
    data = []
    for seed, cost_p in ((41, 0.9), (42, 0.1), (43, 0.9)):
        data.append(make_update_batch(np.random.default_rng(seed), n, D, A, hidden, cost_p, 1.0, T))
    kw = dict(pi_optimizer="first_order", cost_lim=25.0, target_kl=0.01, **AGENT)
    pol = _policy(D, A, **kw)
    agent = ref.RefAgent(data[0][0].size, max_path_length=T, **AGENT)
    infos = []
    for i, (params, batch) in enumerate(data):
        if i == 2:
            pol.save(str(tmp_path), 7)
        pol.set_params(params)                      # from outside: moments and penalty stay
        info = pol.update_policy(_buf(batch))
        infos.append(info)
        want = agent.update_pi(ref.make_graph(D, A, batch, hidden=hidden, max_path_length=T), params, 0.01, 25.0)
        lim, k = want["kl_lim"], want["StopIter"]
        assert len(want["kls"]) == k < 10, "the reference must stop inside the loop"
        assert np.all(want["kls"][:k - 1] <= 0.9 * lim) and want["kls"][k - 1] >= 1.1 * lim, want["kls"] / lim
        assert info["StopIter"] == k, (i, info["StopIter"], k)
        np.testing.assert_allclose(float(info["Penalty"]), want["Penalty"], rtol=1e-5)
        np.testing.assert_allclose(float(info["PenaltyDelta"]), want["PenaltyDelta"], rtol=1e-3, atol=1e-6)
        for key in ("KL", "SurrAdv", "SurrCost"):
            np.testing.assert_allclose(float(info["post"][key]), want["post"][key], rtol=2e-2, atol=1e-7, err_msg=key)
        assert abs(float(info["ClipFrac"]) - want["ClipFrac"]) <= 2.0 / n
        assert float(info["cur_cret_avg"]) == pytest.approx(float(batch["cost"].mean()) * T, rel=1e-6)
        np.testing.assert_array_equal(pol.actor.get_flat_params(), pol.ops.get_params())
    assert infos[1]["Penalty"] < infos[0]["Penalty"]            # cost 3.5 against a limit of 25
    # the checkpoint written before the third update carries everything the optimiser remembers
    z = np.load(os.path.join(str(tmp_path), "policy_7.npz"))
    for name in ("ppo_penalty_param", "ppo_adam_t", "ppo_adam_m", "ppo_adam_v", "W0", "log_std"):
        assert name in z.files, name
    pol2 = _policy(D, A, **kw)
    pol2.load(str(tmp_path), 7)
    pol2.set_params(data[2][0])
    info2 = pol2.update_policy(_buf(data[2][1]))
    np.testing.assert_array_equal(pol2.ops.get_params(), pol.ops.get_params())
    np.testing.assert_array_equal(pol2.ops.adam_m.cpu().numpy(), pol.ops.adam_m.cpu().numpy())
    np.testing.assert_array_equal(pol2.ops.adam_v.cpu().numpy(), pol.ops.adam_v.cpu().numpy())
    from cmbpo_amd import _lib as L
    np.testing.assert_array_equal(_state(pol2.ops)[:L.PPO_ST_POST], _state(pol.ops)[:L.PPO_ST_POST])
    assert info2["StopIter"] == infos[2]["StopIter"] and info2["Penalty"] == infos[2]["Penalty"]


def _toy_epoch(pol, env, steps, gamma=0.9):
    """`steps` real steps of the toy point-mass under the policy, as the twelve buffer columns (model-free)"""
    cols = {k: [] for k in ("obs", "act", "rew", "cost", "logp", "mu", "ls", "v", "vc", "done")}
    obs = env.reset()
    for _ in range(steps):
        out = pol.get_action_outs(obs.astype(np.float32))
        nxt, rew, done, info = env.step(out["pi"][0])
        for k, x in (("obs", obs[0]), ("act", out["pi"][0]), ("rew", rew[0]), ("cost", info.get("cost", 0.0)),
                     ("logp", out["logp_pi"][0]), ("mu", out["pi_info"]["mu"][0]), ("ls", out["pi_info"]["log_std"][0]),
                     ("v", out["v"][0]), ("vc", out["vc"][0]), ("done", bool(done[0]))):
            cols[k].append(x)
        obs = env.reset() if done[0] else nxt
    c = {k: np.asarray(v, np.float32) for k, v in cols.items() if k != "done"}
    ret, cret, run_r, run_c = np.zeros(steps, np.float32), np.zeros(steps, np.float32), 0.0, 0.0
    for t in reversed(range(steps)):
        if cols["done"][t]:
            run_r = run_c = 0.0
        run_r = c["rew"][t] + gamma * run_r
        run_c = c["cost"][t] + gamma * run_c
        ret[t], cret[t] = run_r, run_c
    adv = ret - c["v"]
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    cadv = cret - c["vc"]
    cadv = cadv - cadv.mean()
    return [c["obs"], c["act"], adv.astype(np.float32), cadv.astype(np.float32), ret, cret, c["logp"], c["v"], c["vc"],
            c["cost"], c["ls"], c["mu"]]


def test_policy_runs_first_order_epochs_on_the_toy_world(hip_lib):
    _need_gpu()
    from cmbpo_amd import synthetic
    from cmbpo_amd.cpo_update import CPOAgent, PPOLagAgent
    from cmbpo_amd.logger import EpochLogger
    from toyworld import ToyEnv
    env = ToyEnv(lengths=(12, 30, 7, 20, 9, 25))
    D, A = env.D, env.A
    pol = _policy(D, A, pi_optimizer="first_order", pi_iters=5, vf_lr=1e-3, vf_epochs=2, vf_batch_size=64, logger=EpochLogger())
    assert isinstance(pol.agent, PPOLagAgent)
    pol.set_params(np.concatenate([q.reshape(-1) for q in synthetic.policy_params(np.random.default_rng(2), D, A, 128)]))
    rs = np.random.RandomState(1)
    pol.v.init_weights(rs)
    pol.vc.init_weights(rs)
    rows, excess = [], (1.0, 1.0, -10.0)          # epoch cost above the limit twice, then far below (Adam carries momentum)
    for epoch in range(3):
        buf = _toy_epoch(pol, env, 160)
        pol.cost_lim = float(buf[9].mean()) * T - excess[epoch]
        pol.update_real_c(buf)
        pol.update_policy(buf)
        pol.update_critic(buf, rng=rs)
        pol.log()
        rows.append(pol.logger.dump_tabular())
    for row in rows:
        for k in ("Penalty", "PenaltyDelta", "StopIter", "ClipFrac", "LossPi", "SurrCost", "SurrAdv", "Entropy", "KL",
                  "LossPiDelta", "SurrCostDelta", "SurrAdvDelta", "LossVEnsemble", "LossVCEnsemble"):
            assert k in row, k
        assert all(np.isfinite(float(v)) for v in row.values()), row
        assert "Optim_A" not in row and "Margin" not in row
    pen = [float(r["Penalty"]) for r in rows]
    assert pen[0] > 1.0 and pen[1] > pen[0] and pen[2] < pen[1], pen
    assert rows[0]["PenaltyDelta"] > 0 and rows[2]["PenaltyDelta"] < 0

    # the default is today's: a CPOAgent, and the old logger row
    old = _policy(D, A, logger=EpochLogger())
    assert isinstance(old.agent, CPOAgent) and old.pi_optimizer == "trust_region"
    assert not any(k in old.ops.__dict__ for k in old.ops._FIRST_ORDER)       # no first-order buffers either
    old.log()
    row = old.logger.dump_tabular()
    assert row["Penalty"] == 0 and row["PenaltyDelta"] == 0 and "StopIter" not in row and "ClipFrac" not in row

    class _World2:
        world, rank = 2, 0

    with pytest.raises(NotImplementedError):
        _policy(D, A, pi_optimizer="first_order", comm=_World2())
    with pytest.raises(ValueError):
        _policy(D, A, pi_optimizer="second_order")
