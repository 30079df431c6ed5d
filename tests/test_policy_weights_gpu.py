"""GPU: per-sample weights in the policy-update kernels -- a sample of weight w behaves as w copies of itself.

References: the float64 weighted graph of tests/policy_weights_ref.py (pinned on the CPU against the unweighted oracle on the
replicated batch), and the device's own UNWEIGHTED kernels on the replicated / truncated batch.

Tolerances are those of tests/test_cpo_update_gpu.py and tests/test_ppo_lag_gpu.py: vectors |d| <= 1e-3 |ref| +
3e-5 max|ref|; scalar sums rtol 2e-4, atol 1e-6 (KL atol 1e-7); quantities at the end of an iterated update rtol 2e-2,
atol 1e-7.  Rows whose float64 ratio lies within 1e-3 of a clip edge are dropped as in test_ppo_lag_gpu.py (here from a
slightly larger draw, so that the batch keeps the size the case names).
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

import policy_weights_ref as wref  # noqa: E402
import ppo_lag_ref as ref  # noqa: E402

KEYS = ("obs", "act", "adv", "cadv", "logp_old", "cost", "mu_old", "log_std_old")
SHAPES = [(21, 3, 31, 128), (20, 6, 64, 128), (29, 8, 1037, 128), (47, 17, 500, 128), (29, 8, 2000, 256)]
CLIP, T, PENALTY = 0.2, 35, 1.0


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
    """n rows of the batch of seed D*100 + A (drawn a little larger, rows on a clip edge removed, the first n kept), parameters
    0.01 N(0,1) off theta_old, a few rows with adv == 0 / cadv == 0; the three weight vectors of this file and every
    float64 reference, computed once and shared."""
    key = (D, A, n, hidden)
    if key in _CASES:
        return _CASES[key]
    from worlds import make_update_batch
    rng = np.random.default_rng(D * 100 + A)
    draw = n + max(8, n // 20)
    params, batch = make_update_batch(rng, draw, D, A, hidden, 0.3, 1.0, T)
    p = (params + 0.01 * rng.standard_normal(params.shape)).astype(np.float32)
    batch["adv"][[1, n // 2, n - 2]] = 0.0
    batch["cadv"][[2, n // 3, n - 1]] = 0.0
    ratio = ref.Surrogate(ref.make_graph(D, A, batch, hidden=hidden), CLIP).ratio(p)
    keep = np.flatnonzero((np.abs(ratio - (1 - CLIP)) > 1e-3) & (np.abs(ratio - (1 + CLIP)) > 1e-3))
    assert len(keep) >= n and draw - len(keep) <= 0.02 * draw, "clip-edge filter removed %d of %d rows" % (draw - len(keep), draw)
    keep = keep[:n]
    batch = {k: np.ascontiguousarray(v[keep]) for k, v in batch.items()}
    w_frac = np.exp(rng.uniform(np.log(1 / 64), np.log(64), n)).astype(np.float32)     # log-uniform in [1/64, 64]
    w_frac[::7] = 0.0
    w_int = rng.integers(0, 4, n).astype(np.float32)
    c = dict(D=D, A=A, n=n, hidden=hidden, params=params, p=p, batch=batch, w_frac=w_frac, w_int=w_int,
             v=rng.standard_normal(params.shape).astype(np.float32), refs={})
    _CASES[key] = c
    return c


def _ref(c):
    """float64: weighted gradients, Fisher-vector product, eval triple, cost mean, PPO gradient and sums under w_frac"""
    if not c["refs"]:
        g = wref.WeightedPolicyGraph(c["D"], c["A"], c["batch"], c["w_frac"], hidden=c["hidden"], max_path_length=T)
        sur = wref.WeightedSurrogate(g, CLIP)
        s = sur.sums(c["p"])
        # a run in which nothing clips cannot pass: a share of the rows as in test_ppo_lag_gpu.py, and of the weight some
        plain = ref.Surrogate(ref.make_graph(c["D"], c["A"], c["batch"], hidden=c["hidden"]), CLIP).sums(c["p"])
        assert 0.05 <= plain[5] / c["n"] <= 0.95, plain[5] / c["n"]
        assert 0 < s[5] < s[0]
        c["refs"] = dict(grads=g.grads(c["p"]), fvp=g.fisher_vp(c["params"], c["v"], 0.0), evals=g.evals(c["p"]),
                         cret=float(g.cur_cret_avg()), ppo_g=sur.grad(c["p"], PENALTY), ppo_s=s,
                         W=float(np.sum(c["w_frac"].astype(np.float64))))
    return c["refs"]


def _ops(c, params=None, batch=None, weights=None):
    from cmbpo_amd.cpo_update import PolicyOps
    ops = PolicyOps(c["D"], c["A"], c["hidden"], device="cuda:0")
    ops.set_params(c["p"] if params is None else params)
    b = c["batch"] if batch is None else batch
    ops.bind(*[b[k] for k in KEYS], weights=weights)
    return ops


def _set_penalty(ops, penalty=PENALTY):
    from cmbpo_amd import _lib
    ops.ppo_state[_lib.PPO_ST_PENALTY:_lib.PPO_ST_CC + 1] = torch.tensor(
        [penalty, 1.0 / (1.0 + penalty), penalty / (1.0 + penalty)], dtype=torch.float64, device=ops.device)


def _everything(ops, c):
    """Every fetch of the update at parameters p (the Fisher-vector product at theta_old), as NumPy: normalised vectors and
    raw sums"""
    _set_penalty(ops)
    ops.set_params(c["p"])
    g, sg = ops.loss_grad(0)
    b, sb = ops.loss_grad(1)
    ev = ops.evals()
    pg, ps = ops.ppo_grad(ops.ppo_cfg(clip_ratio=CLIP))
    ops.set_params(c["params"])
    hv = ops.fvp(c["v"])
    ops.loss_grad(0)                      # (saves the activations: the second product reads them)
    hv_saved = ops.fvp(c["v"])
    return dict(g=g, b=b, hv=hv, hv_saved=hv_saved, pg=pg, sg=sg, sb=sb, ev=ev, ps=ps)


def _same(got, want):
    """device against device, the tolerances of the module docstring; sums as means (the normalisers are compared too)"""
    for k in ("g", "b", "hv", "hv_saved", "pg"):
        _close(got[k], want[k], msg=k)
    for k in ("sg", "sb", "ev", "ps"):
        a, b = got[k], want[k]
        np.testing.assert_allclose(a[0], b[0], rtol=1e-6, err_msg=k + "[0]")
        for j, atol in ((1, 1e-6), (2, 1e-6), (3, 1e-7), (6, 1e-6)):
            np.testing.assert_allclose(a[j] / a[0], b[j] / b[0], rtol=2e-4, atol=atol, err_msg="%s[%d]" % (k, j))
        np.testing.assert_allclose(a[4], b[4], rtol=1e-6, err_msg=k + "[4]")
        np.testing.assert_allclose(a[5], b[5], rtol=2e-4, atol=1e-6, err_msg=k + "[5]")


@pytest.mark.parametrize("D,A,n,hidden", SHAPES)
def test_fractional_weights_match_the_float64_reference(hip_lib, D, A, n, hidden):
    _need_gpu()
    c = _case(D, A, n, hidden)
    r = _ref(c)
    W = r["W"]
    got = _everything(_ops(c, weights=c["w_frac"]), c)
    g_ref, b_ref, lo_ref, sc_ref = r["grads"]
    _close(got["g"], g_ref, msg="flat_g")
    _close(got["b"], b_ref, msg="flat_b")
    _close(got["hv"], r["fvp"], msg="fvp")
    _close(got["hv_saved"], r["fvp"], msg="fvp on saved activations")
    for s in (got["sg"], got["sb"], got["ev"], got["ps"]):
        np.testing.assert_allclose(s[0], W, rtol=1e-6)
        np.testing.assert_allclose(s[4] / W * T, r["cret"], rtol=1e-6)
    for s in (got["sg"], got["sb"], got["ev"]):
        np.testing.assert_allclose(-s[1] / W, lo_ref if s is not got["ev"] else r["evals"][1], rtol=2e-4, atol=1e-6)
        np.testing.assert_allclose(s[2] / W, sc_ref if s is not got["ev"] else r["evals"][2], rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(got["ev"][3] / W, r["evals"][0], rtol=2e-4, atol=1e-7)
    _close(got["pg"], r["ppo_g"], msg="ppo gradient")
    ps, ps_ref = got["ps"], r["ppo_s"]
    for k in (1, 2, 6):
        np.testing.assert_allclose(ps[k] / W, ps_ref[k] / W, rtol=2e-4, atol=1e-6, err_msg="ppo sum %d" % k)
    np.testing.assert_allclose(ps[3] / W, ps_ref[3] / W, rtol=2e-4, atol=1e-7, err_msg="ppo kl")
    np.testing.assert_allclose(ps[5] / W, ps_ref[5] / W, rtol=2e-4, atol=1e-6, err_msg="weighted clip count")
    assert ps[7] == 0 and ps[1] != ps[6]


@pytest.mark.parametrize("D,A,n,hidden", SHAPES)
def test_integer_weights_equal_the_unweighted_kernels_on_the_replicated_batch(hip_lib, D, A, n, hidden):
    _need_gpu()
    c = _case(D, A, n, hidden)
    w = c["w_int"]
    assert (w == 0).any() and (w == 3).any()
    rep, _ = wref.replicate(c["batch"], w)
    assert rep["obs"].shape[0] == int(w.sum())
    _same(_everything(_ops(c, weights=w), c), _everything(_ops(c, batch=rep), c))


def test_zero_weights_on_the_last_rows_equal_the_shorter_batch(hip_lib):
    _need_gpu()
    c = _case(29, 8, 1037, 128)
    w = np.ones(1037, np.float32)
    w[1000:] = 0.0
    head = {k: np.ascontiguousarray(v[:1000]) for k, v in c["batch"].items()}
    got, want = _everything(_ops(c, weights=w), c), _everything(_ops(c, batch=head), c)
    assert want["sg"][0] == 1000
    _same(got, want)


@pytest.mark.parametrize("D,A,n,hidden", SHAPES)
def test_all_ones_weights_are_no_weights(hip_lib, D, A, n, hidden):
    """multiplying by 1.0f and adding 1.0 are exact: the vectors agree bit for bit; the sums' float64 atomics add in no
    fixed order"""
    _need_gpu()
    c = _case(D, A, n, hidden)
    got, want = _everything(_ops(c, weights=np.ones(n, np.float32)), c), _everything(_ops(c), c)
    for k in ("g", "b", "hv", "hv_saved", "pg"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in ("sg", "sb", "ev", "ps"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, err_msg=k)
        assert got[k][0] == n


def test_no_leak_to_the_next_bind(hip_lib):
    _need_gpu()
    c = _case(29, 8, 1037, 128)
    ops = _ops(c, weights=c["w_frac"])
    weighted = _everything(ops, c)
    ops.bind(*[c["batch"][k] for k in KEYS], weights=None)
    again, fresh = _everything(ops, c), _everything(_ops(c), c)
    for k in ("g", "b", "hv", "hv_saved", "pg"):
        np.testing.assert_array_equal(again[k], fresh[k], err_msg=k)
        assert np.max(np.abs(weighted[k] - fresh[k])) > 0, k
    assert again["sg"][0] == 1037 and ops.n_global == 1037


def _policy(D, A, hidden=128, **kw):
    from cmbpo_amd.cpo_policy import CPOPolicy
    return CPOPolicy(_Space(D), _Space(A), a_hidden_layer_sizes=(hidden, hidden), vf_hidden_layer_sizes=(128, 128),
                     vf_ensemble_size=3, vf_elites=2, vf_activation="swish", vf_loss="MSE", device="cuda:0",
                     max_path_length=T, **kw)


def _buf(batch):
    z = np.zeros(batch["obs"].shape[0], np.float32)
    return [batch["obs"], batch["act"], batch["adv"], batch["cadv"], z, z, batch["logp_old"], z, z, batch["cost"],
            batch["log_std_old"], batch["mu_old"]]


SCENARIOS = {   # of tests/test_cpo_update_gpu.py: cost_p, cadv_scale, cost_lim, constrained, real_cost, seed
    "violating": (0.9, 1.0, 10.0, True, 25.0, 12),
    "unconstrained": (0.5, 1.0, 10.0, False, 10.0, 14),
}


def _scenario(name, n=4000, D=29, A=8):
    from worlds import make_update_batch
    cost_p, cadv_scale, cost_lim, constrained, real_cost, seed = SCENARIOS[name]
    rng = np.random.default_rng(seed)
    params, batch = make_update_batch(rng, n, D, A, 128, cost_p, cadv_scale, T)
    return rng, params, batch, dict(constrain_cost=constrained, cost_lim=cost_lim, target_kl=0.01), real_cost


def _update(params, batch, kw, real_cost, weights=None):
    pol = _policy(29, 8, **kw)
    pol.set_params(params)
    pol.real_c_buffer = [real_cost] * 300
    info = pol.update_policy(_buf(batch), weights=weights)
    return pol, info, pol.actor.get_flat_params()


def test_uniform_scaling_of_the_weights_changes_nothing(hip_lib):
    _need_gpu()
    rng, params, batch, kw, real_cost = _scenario("violating")
    w = np.exp(rng.uniform(np.log(1 / 64), np.log(64), 4000)).astype(np.float32)
    _, i1, p1 = _update(params, batch, kw, real_cost, w)
    _, i2, p2 = _update(params, batch, kw, real_cost, 0.5 * w)
    assert i1["OptimCase"] == i2["OptimCase"] and i1["BacktrackIters"] == i2["BacktrackIters"]
    np.testing.assert_allclose(p2, p1, rtol=2e-2, atol=1e-7)
    assert np.max(np.abs(p1 - params)) > 0
    # and the weights did something
    _, i0, p0 = _update(params, batch, kw, real_cost)
    assert np.max(np.abs(p0 - p1)) > 0


def test_cg_solve_under_weights(hip_lib):
    """graph on == graph off; a repeated solve captures nothing new, other weights capture once more; the product on saved
    activations stays bit-identical to the recomputed one"""
    _need_gpu()
    from cmbpo_amd import _lib
    c = _case(29, 8, 1037, 128)
    ops = _ops(c, params=c["params"], weights=c["w_frac"])
    caps = lambda: _lib.lib().cmbpo_pi_cg_graph_captures()
    b = torch.from_numpy(c["v"]).cuda()
    outs = []
    for use_graph in (True, False, True):
        ops.use_graph = use_graph
        x = torch.zeros_like(b)
        ops.cg_dev(b, x, 0.1)
        outs.append(x.cpu().numpy().copy())
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[0], outs[2])
    x = torch.zeros_like(b)            # (a graph belongs to a handle and a solution vector: one vector from here on)
    ops.cg_dev(b, x, 0.1)
    n0 = caps()
    for _ in range(3):
        x.zero_()
        ops.cg_dev(b, x, 0.1)
    assert caps() == n0
    np.testing.assert_array_equal(x.cpu().numpy(), outs[0])
    # the solve is the CG of the weighted float64 operator
    g = wref.WeightedPolicyGraph(c["D"], c["A"], c["batch"], c["w_frac"], hidden=c["hidden"])
    from oracle import refupdate
    if hasattr(refupdate, "cg"):
        _close(outs[0], refupdate.cg(lambda v: g.fisher_vp(c["params"], v, 0.1), c["v"].astype(np.float64)), rtol=2e-2, arel=2e-3)
    # other weights (another array): one more capture, another solution; the same array again: none
    ops.bind(*[c["batch"][k] for k in KEYS], weights=c["w_int"])
    x.zero_()
    ops.cg_dev(b, x, 0.1)
    assert caps() == n0 + 1
    assert np.max(np.abs(x.cpu().numpy() - outs[0])) > 0
    x.zero_()
    ops.cg_dev(b, x, 0.1)
    assert caps() == n0 + 1
    # clearing them re-captures too, and gives the unweighted solve
    ops.bind(*[c["batch"][k] for k in KEYS])
    x.zero_()
    ops.cg_dev(b, x, 0.1)
    assert caps() == n0 + 2
    x3 = x.clone()
    plain = _ops(c, params=c["params"])
    x4 = torch.zeros_like(b)
    plain.cg_dev(b, x4, 0.1)
    np.testing.assert_array_equal(x3.cpu().numpy(), x4.cpu().numpy())
    # saved activations under weights: kept across set_sample_weights, bit-identical products and solves
    ops.bind(*[c["batch"][k] for k in KEYS], weights=c["w_frac"])
    uses = lambda: _lib.lib().cmbpo_pi_saved_activation_uses(ops._h)
    hv_re = ops.fvp(c["v"])
    u0 = uses()
    ops.loss_grad(0)
    hv_sv = ops.fvp(c["v"])
    assert uses() == u0 + 1
    np.testing.assert_array_equal(hv_sv, hv_re)
    x5 = torch.zeros_like(b)
    ops.cg_dev(b, x5, 0.1)
    np.testing.assert_array_equal(x5.cpu().numpy(), outs[0])


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_update_policy_with_integer_weights_is_update_policy_on_the_replicated_batch(hip_lib, name):
    _need_gpu()
    rng, params, batch, kw, real_cost = _scenario(name)       # (at half the size the unconstrained line search fails)
    w = rng.integers(0, 4, 4000).astype(np.float32)
    rep, _ = wref.replicate(batch, w)
    _, iw, pw = _update(params, batch, kw, real_cost, w)
    _, ir, pr = _update(params, rep, kw, real_cost)
    assert iw["OptimCase"] == ir["OptimCase"] and iw["BacktrackIters"] == ir["BacktrackIters"], name
    assert iw["accepted"] == ir["accepted"]
    for k in ("Optim_Lam", "Optim_Nu"):
        np.testing.assert_allclose(float(iw[k]), float(ir[k]), rtol=2e-2, atol=1e-7, err_msg=k)
    np.testing.assert_allclose(float(iw["cur_cret_avg"]), float(ir["cur_cret_avg"]), rtol=1e-5)
    step = float(np.linalg.norm(pr - params)) + 1e-12
    assert step > 1e-6
    assert float(np.linalg.norm(pw - pr)) <= 5e-3 * step, name


def test_first_order_update_with_integer_weights_is_the_update_on_the_replicated_batch(hip_lib):
    _need_gpu()
    rng, params, batch, kw, real_cost = _scenario("violating", n=2000)
    w = rng.integers(0, 4, 2000).astype(np.float32)
    rep, _ = wref.replicate(batch, w)
    kw = dict(kw, pi_optimizer="first_order", pi_iters=5, kl_margin=1e9)       # (the gate is off)
    _, iw, pw = _update(params, batch, kw, real_cost, w)
    _, ir, pr = _update(params, rep, kw, real_cost)
    assert iw["steps"] == ir["steps"] == 5 and not iw["stopped"]
    np.testing.assert_allclose(pw, pr, rtol=2e-2, atol=1e-7)
    assert np.max(np.abs(pr - params)) > 0
    for k in ("LossPi", "SurrCost", "SurrAdv", "KL", "Entropy"):
        np.testing.assert_allclose(float(iw["post"][k]), float(ir["post"][k]), rtol=2e-2, atol=1e-7, err_msg=k)
    np.testing.assert_allclose(float(iw["Penalty"]), float(ir["Penalty"]), rtol=1e-5)
    np.testing.assert_allclose(float(iw["ClipFrac"]), float(ir["ClipFrac"]), rtol=2e-2, atol=1e-3)


def test_bad_weights_are_refused(hip_lib):
    _need_gpu()
    import ctypes as C
    from cmbpo_amd import _lib
    c = _case(21, 3, 31, 128)
    ops = _ops(c)
    args = [c["batch"][k] for k in KEYS]
    good = np.ones(31, np.float32)
    for bad in (np.where(np.arange(31) == 4, -1.0, 1.0), np.where(np.arange(31) == 4, np.nan, 1.0), np.zeros(31),
                np.ones(30), np.ones((31, 1))):
        with pytest.raises(ValueError):
            ops.bind(*args, weights=bad.astype(np.float32))
    ops.bind(*args, weights=good)
    pol = _policy(21, 3)
    with pytest.raises(ValueError):
        pol.update_critic(_buf(c["batch"]), weights=good)
    # C level: the handle holds 31 weights, the launch brings 30 samples -> an error code and a message, nothing launched
    lib = _lib.lib()
    ops.batch.n = 30
    sums = torch.zeros(8, dtype=torch.float64, device="cuda")
    assert lib.cmbpo_pi_eval(ops._h, C.byref(ops.batch), sums.data_ptr(), None) == -1
    assert b"sample weights" in lib.cmbpo_last_error()
    cfg = ops.ppo_cfg()
    assert lib.cmbpo_pi_ppo_run(ops._h, C.byref(ops.batch), C.byref(cfg), ops.params.data_ptr(), ops.adam_m.data_ptr(),
                                ops.adam_v.data_ptr(), ops.ppo_state.data_ptr(), 1, None) == -1
    x = torch.zeros(ops.P, device="cuda")
    assert lib.cmbpo_pi_cg_solve(ops._h, C.byref(ops.batch), ops.work["g"].data_ptr(), 1.0 / 30, 0.1, 3, x.data_ptr(),
                                 ops.work["cg_r"].data_ptr(), ops.work["cg_p"].data_ptr(), ops.vec.data_ptr(),
                                 ops.scal.data_ptr(), 1, None) == -1
    assert b"cmbpo_pi_cg_solve" in lib.cmbpo_last_error()
    ops.batch.n = 31
    assert lib.cmbpo_pi_eval(ops._h, C.byref(ops.batch), sums.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert float(sums[0]) == 31


def _world2_weights(n):
    return np.exp(np.random.default_rng(77).uniform(np.log(1 / 8), np.log(8), n)).astype(np.float32)


def _worker_weighted_update(rank, world, port, out_dir, path):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as td
    td.init_process_group("gloo", rank=rank, world_size=world)
    import cmbpo_amd  # noqa: F401
    from cmbpo_amd import _lib
    from cmbpo_amd.dist import Comm
    from test_world2_gpu import _make_policy, _update_setup
    _lib.lib().cmbpo_set_pi_matrix_path(path)          # (the fixture's choice does not reach a spawned process)
    comm = Comm(device=torch.device("cuda:0"))
    params, buf, (D, A, T_) = _update_setup()
    n = buf[0].shape[0]
    w = _world2_weights(n)
    cut = n // 3                                       # unequal shards: the reductions must weight by the weights' sums
    sl = slice(0, cut) if rank == 0 else slice(cut, n)
    pol = _make_policy(D, A, T_, comm)
    pol.set_params(params)
    pol.real_c_buffer = [12.0] * 300
    info = pol.update_policy([x[sl] for x in buf], weights=w[sl])
    np.savez(os.path.join(out_dir, f"wupd{rank}.npz"), params=pol.actor.get_flat_params(), case=info["OptimCase"],
             bt=info["BacktrackIters"], lam=float(info["Optim_Lam"]), nu=float(info["Optim_Nu"]), kl=float(pol.logger.stored["KL"]))
    comm.barrier()
    td.destroy_process_group()


def test_sharded_weighted_update_matches_single_rank(hip_lib, tmp_path, pi_path):
    """world 2 on one GPU (gloo), unequal shards: W is all-reduced where the count was"""
    _need_gpu()
    import torch.multiprocessing as mp
    from test_world2_gpu import _free_port, _make_policy, _update_setup
    world, port = 2, _free_port()
    mp.spawn(_worker_weighted_update, args=(world, port, str(tmp_path), pi_path), nprocs=world, join=True)
    r = [np.load(os.path.join(tmp_path, f"wupd{k}.npz")) for k in range(world)]
    params, buf, (D, A, T_) = _update_setup()
    pol = _make_policy(D, A, T_)
    pol.set_params(params)
    pol.real_c_buffer = [12.0] * 300
    info = pol.update_policy(buf, weights=_world2_weights(buf[0].shape[0]))
    want = pol.actor.get_flat_params()
    step = float(np.linalg.norm(want - params)) + 1e-12
    np.testing.assert_array_equal(r[0]["params"], r[1]["params"])
    for x in r:
        assert int(x["case"]) == int(info["OptimCase"]) and int(x["bt"]) == int(info["BacktrackIters"])
        np.testing.assert_allclose(float(x["lam"]), float(info["Optim_Lam"]), rtol=5e-3)
        np.testing.assert_allclose(float(x["nu"]), float(info["Optim_Nu"]), rtol=5e-3, atol=1e-7)
        assert float(np.linalg.norm(x["params"] - want)) <= 5e-3 * step
        np.testing.assert_allclose(float(x["kl"]), float(pol.logger.stored["KL"]), rtol=2e-2, atol=1e-6)
