"""GPU: the critics' own disagreement and the pessimistic value bootstraps, through every layer -- the VDIS instances of both
critic kernels against tests/value_disagreement_ref.py, the rollout state beside cmbpo_rollout_t (penalised v_t / vc_t / v_n /
vc_n, so penalised buffers, bootstraps and advantages with unchanged finish / GAE kernels; the two totals) on the one-workgroup
bookkeeping path and just above it, ModelBuffer / CPOPolicy, and the trainer.

The members' values come without a new output: a one-member pair of handles with member e's weights and the same scalers gives
x_e through the PLAIN entry bit for bit (per-member arithmetic does not depend on E), which the first assertion of every case
guards: ((0 + x0) + x1 + ...) / E equals the E-member plain entry bit for bit.

Bit for bit throughout, except the two totals: float64 sums of fewer than 1e5 non-negative terms added in another order than
the host's, bound n * 2^-53 ~ 1e-11, compared at rtol 1e-10."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import disagreement_ref as dref  # noqa: E402
import value_disagreement_ref as ref  # noqa: E402

KAPPA = (0.75, 1.5)
NAMES = ["obs", "act", "adv", "cadv", "ret", "cret", "logp", "val", "cval", "cost", "log_std", "mu"]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _bits(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, msg=""):
    """Bit for bit where the specification is finite or infinite, NaN where it is NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=msg)
    ok = ~np.isnan(b)
    np.testing.assert_array_equal(_bits(a)[ok], _bits(b)[ok], err_msg=msg)


# ------------------------------------------------------------------------------------------------------------------
# 1. the critic kernels
# ------------------------------------------------------------------------------------------------------------------
def _pe(critic, obs_dim):
    from cmbpo_amd.pens import PE
    ws, bs, sc_in, sc_out = critic
    E = ws[0].shape[0]
    m = PE(obs_dim, 1, hidden_dims=(128, 128), num_networks=E, num_elites=E, loss="MSE", use_scaler_in=True, use_scaler_out=True,
           device="cuda:0")
    m.set_weights(ws, bs, sc_in, sc_out)
    return m


class _Pair:
    """The two E-member critics on the device and, per member, the one-member pair that gives its values."""

    def __init__(self, critics, obs_dim):
        from cmbpo_amd import _lib
        self.lib, self._lib = _lib.lib(), _lib
        self.obs_dim, self.E = obs_dim, critics[0][0][0].shape[0]
        self.full = [_pe(c, obs_dim) for c in critics]
        self.single = [[_pe(ref.one_member(c, e), obs_dim) for c in critics] for e in range(self.E)]
        assert self.lib.cmbpo_critic_pair_supported(self.full[0].mlp.handle, self.full[1].mlp.handle) == 1

    def run(self, nets, obs_t, idx_t, n, slots, kappa=None):
        """Plain entry (kappa None) or the new one; outputs over `slots` slots, NaN sentinels where nothing is written."""
        dev = obs_t.device
        k = 2 if kappa is None else 4
        out = [torch.full((slots,), float("nan"), device=dev) for _ in range(k)]
        ip = None if idx_t is None else idx_t.data_ptr()
        h = (nets[0].mlp.handle, nets[1].mlp.handle)
        if kappa is None:
            rc = self.lib.cmbpo_critic_pair_predict(h[0], h[1], obs_t.data_ptr(), self.obs_dim, ip, None, n, out[0].data_ptr(),
                                                    out[1].data_ptr(), self._lib.current_stream())
            self._lib.check(rc, "cmbpo_critic_pair_predict")
        else:
            rc = self.lib.cmbpo_critic_pair_predict_var(h[0], h[1], obs_t.data_ptr(), self.obs_dim, ip, None, n, kappa[0], kappa[1],
                                                        out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
                                                        self._lib.current_stream())
            self._lib.check(rc, "cmbpo_critic_pair_predict_var")
        return [o.cpu().numpy() for o in out]

    def members(self, obs_t, idx_t, n, slots):
        """x[2][E, slots]: every member's values through the plain entry on its one-member pair."""
        per = [self.run(self.single[e], obs_t, idx_t, n, slots) for e in range(self.E)]
        return [np.stack([per[e][c] for e in range(self.E)]) for c in range(2)]


def _check_case(pair, obs_t, idx, slots, n, vacuity="relative", kappas=((0.0, 0.0), KAPPA, (0.0, 1.0))):
    """One row set (idx None: the first n rows) through the plain entry, the members' entries and the new entry."""
    dev = obs_t.device
    idx_t = None if idx is None else torch.from_numpy(idx).to(dev)
    rows = np.arange(n) if idx is None else idx[:n]
    rest = np.setdiff1d(np.arange(slots), rows)
    plain = pair.run(pair.full, obs_t, idx_t, n, slots)
    x = [xc[:, rows] for xc in pair.members(obs_t, idx_t, n, slots)]
    for c in range(2):
        # the decomposition: the members' values add up to the E-member plain entry, bit for bit
        np.testing.assert_array_equal(_bits(ref.member_mean(x[c])), _bits(plain[c][rows]), err_msg=f"decomposition, critic {c}")
        if pair.E >= 2 and vacuity is not None:
            ref.check_non_vacuous(x[c], KAPPA[c], (-1, +1)[c], relative=(vacuity == "relative"))
    for kappa in kappas:
        got = pair.run(pair.full, obs_t, idx_t, n, slots, kappa)
        want = ref.value_disagreement(x[0], x[1], *kappa)
        for k, name in enumerate(("v", "vc", "v_var", "vc_var")):
            np.testing.assert_array_equal(_bits(got[k][rows]), _bits(want[k]), err_msg=f"{name}, kappa {kappa}, n {n}")
            assert np.isnan(got[k][rest]).all(), f"{name}: a slot outside the row list was written"
        for c in range(2):
            if kappa[c] == 0.0:
                np.testing.assert_array_equal(_bits(got[c][rows]), _bits(plain[c][rows]), err_msg=f"kappa 0 == plain, critic {c}")
        if pair.E == 1:
            assert not _bits(got[2][rows]).any() and not _bits(got[3][rows]).any()      # +0
    return x


@pytest.mark.parametrize("obs_dim", [3, 29, 47, 64])       # S0 = 2, 2, 3, 4
@pytest.mark.parametrize("E", [1, 2, 3, 4])
def test_pair_kernel_value_disagreement(hip_lib, E, obs_dim):
    """critic_pair_kernel's VDIS instances, every E and input-slab count, 1 / 31 / 32 / 33 / 1001 rows (one tile, its edges,
    32 tiles), contiguous and through a row list shorter than the slot count."""
    _need_gpu()
    dev = torch.device("cuda:0")
    pair = _Pair(ref.critic_weights(11, E, obs_dim), obs_dim)
    slots = 1001 + 9
    obs_t = torch.from_numpy(ref.observations(7, slots, obs_dim)).to(dev)
    rng = np.random.default_rng([E, obs_dim])
    for n in (1, 31, 32, 33, 1001):
        _check_case(pair, obs_t, None, slots, n, vacuity="relative" if n == 1001 else None)
        idx = rng.permutation(slots)[:n].astype(np.int32)
        _check_case(pair, obs_t, idx, slots, n, vacuity=None, kappas=(KAPPA,))


@pytest.mark.parametrize("n,obs_dim", [(24576, 29), (24609, 29), (131105, 29), (24609, 47), (24609, 64)])
def test_big_kernel_value_disagreement(hip_lib, n, obs_dim):
    """critic_big_kernel's VDIS instances from the threshold on: an exact multiple of the tile, a ragged last tile, more rows
    than 512 x the CU count (the capped chunk: 448 rows at S0 = 2), and the two other input-slab counts; through a row list.
    The pair kernel on the first 3000 listed rows gives the same bits."""
    _need_gpu()
    dev = torch.device("cuda:0")
    E = 3
    pair = _Pair(ref.critic_weights(11, E, obs_dim), obs_dim)
    slots = n + 7
    obs_t = torch.from_numpy(ref.observations(8, slots, obs_dim)).to(dev)
    idx = np.sort(np.random.default_rng(n).choice(slots, size=n, replace=False)).astype(np.int32)
    _check_case(pair, obs_t, idx, slots, n, kappas=((0.0, 0.0), KAPPA))
    idx_t = torch.from_numpy(idx).to(dev)
    big = pair.run(pair.full, obs_t, idx_t, n, slots, KAPPA)
    small = pair.run(pair.full, obs_t, idx_t, 3000, slots, KAPPA)
    for k in range(4):
        np.testing.assert_array_equal(_bits(small[k][idx[:3000]]), _bits(big[k][idx[:3000]]))


def test_two_pass_variance_at_a_large_output_offset(hip_lib):
    """Output scaler out_mu = 1000, member spread ~ 0.1 (tests/test_value_disagreement_cpu.py shows that a one-pass
    E[x^2] - E[x]^2 misses the specification on > 90 % of such rows): both kernels, bit for bit."""
    _need_gpu()
    dev = torch.device("cuda:0")
    pair = _Pair(ref.critic_weights(11, 3, 29, out_mu=1000.0), 29)
    slots = 24609
    obs_t = torch.from_numpy(ref.observations(9, slots, 29)).to(dev)
    x = _check_case(pair, obs_t, None, slots, 1001, vacuity="absolute")
    assert (np.abs(x[0]) > 990).all()
    _check_case(pair, obs_t, None, slots, 24609, vacuity="absolute", kappas=(KAPPA,))


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_members(hip_lib, bad):
    """NaN / inf in one member's output bias: kappa = 0 gives the plain entry's value (NaN-aware, bit for bit), kappa > 0
    propagates as NumPy does -- in both kernels."""
    _need_gpu()
    dev = torch.device("cuda:0")
    critics = ref.critic_weights(11, 3, 29)
    critics[0][1][2][1] = bad           # V, member 1
    critics[1][1][2][2] = -bad          # VC, member 2
    pair = _Pair(critics, 29)
    for n in (33, 24609):
        obs_t = torch.from_numpy(ref.observations(10, n, 29)).to(dev)
        plain = pair.run(pair.full, obs_t, None, n, n)
        x = pair.members(obs_t, None, n, n)
        zero = pair.run(pair.full, obs_t, None, n, n, (0.0, 0.0))
        pes = pair.run(pair.full, obs_t, None, n, n, KAPPA)
        want = ref.value_disagreement(x[0], x[1], *KAPPA)
        for c in range(2):
            _same(ref.member_mean(x[c]), plain[c], "decomposition")
            _same(zero[c], plain[c], "kappa 0")
            _same(zero[2 + c], want[2 + c], "variance")
            _same(pes[c], want[c], "penalised value")
            _same(pes[2 + c], want[2 + c], "variance")
            assert np.isnan(want[2 + c]).all() and np.isnan(want[c]).all()      # (what NumPy makes of it)


# ------------------------------------------------------------------------------------------------------------------
# 2. the rollout
# ------------------------------------------------------------------------------------------------------------------
def _roll(w, start, dkl_lim, budget, vdis, kappa, how):
    """One rollout of T steps with the sampler's own draws (seed 5) on the world of tests/test_disagreement_gpu.py.  how: 'loop'
    (sample(): cmbpo_rollout_step), 'many' (sample_many(): cmbpo_rollout_run, actor and store riding with the critics) or
    'calls' (sample() with kernel events on: a step driven from Python -- cmbpo_critic_pair_predict_var into v_n / vc_n between
    the unchanged cmbpo_rollout_store and cmbpo_rollout_finish entries)."""
    import test_disagreement_gpu as tdg
    T = tdg.T
    sampler, pool = tdg._world(w, start.shape[0], dkl_lim)
    pool.set_value_disagreement(vdis, *kappa)
    if how == "calls":
        sampler.env.kernel_events = []
    sampler._gen.manual_seed(5)
    sampler.reset(start)
    on = pool.value_disagreement
    assert on == (vdis or kappa[0] > 0 or kappa[1] > 0) and ("v_var" in pool.t) == on
    rec = dict(steps=[], on=on)
    cp = lambda x: x.cpu().numpy().copy()
    if how == "many":
        steps, _ = sampler.sample_many(max_samples=budget)
        assert steps == T
    else:
        for s in range(T):
            assert sampler.any_alive() and pool.has_room
            len0 = cp(pool.t["len"])
            st = dict(v_t=cp(pool.t["v_t"]), vc_t=cp(pool.t["vc_t"]))      # the values (and variances) at cur_obs: what is stored
            if on:
                st.update(v_var=cp(pool.t["v_var"]), vc_var=cp(pool.t["vc_var"]))
            sampler.sample(max_samples=budget)
            st.update(stored=cp(pool.t["len"]) > len0, alive=cp(pool.t["alive_idx"][:pool.n_alive]), len=cp(pool.t["len"]),
                      rew_t=cp(pool.t["rew_t"]), cost_t=cp(pool.t["cost_t"]), n_budget=sampler.n_budget_terminated)
            rec["steps"].append(st)
    rec["n_budget"] = sampler.n_budget_terminated
    rec["len"] = cp(pool.t["len"])
    rec["bufs"] = {k: cp(pool.t[k]) for k in ("rew_buf", "cost_buf", "val_buf", "cval_buf", "obs_buf")}
    rec["diag"] = sampler.finish_all_paths()
    rec["dscal"] = sampler._dsc.copy() if how == "many" else pool.t["dscal"].cpu().numpy().copy()
    rec["iscal"] = pool.t["iscal"].cpu().numpy().copy()
    rec["get"], _ = pool.get()
    return rec


@pytest.mark.parametrize("which", [0, 1], ids=["one_workgroup", "above"])
def test_rollout_with_value_disagreement(hip_lib, which):
    """A 6-step uncertainty-mode rollout with a budget binding on the last step, B on the one-workgroup bookkeeping path and
    just above it: (a) the native loop, the one-call step and the Python-driven step agree bit for bit in every buffer and
    counter, (b) attached with kappa = 0 == detached, (c) kappa moves no branch, reward, cost or observation, and val / cval
    are `penalise` of the kappa = 0 run's values and variances, (d) the two totals."""
    _need_gpu()
    import test_disagreement_gpu as tdg
    from cmbpo_amd import _lib
    T = tdg.T
    B = tdg._rollout_batches()[which]
    assert (B <= hip_lib.cmbpo_rollout_book_pre_max_rows()) == (which == 0)
    w, start, dkl_lim, budget = tdg._plan(B)
    pes = _roll(w, start, dkl_lim, budget, True, KAPPA, "loop")
    assert pes["steps"][-2]["n_budget"] == 0 and pes["n_budget"] > 0 and pes["steps"][-1]["stored"].sum() > 0
    assert (pes["len"] < T).any() and (pes["len"] == T).any()

    # (a) three ways to step
    for how in ("many", "calls"):
        other = _roll(w, start, dkl_lim, budget, True, KAPPA, how)
        for k, a, b in zip(NAMES, pes["get"], other["get"]):
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"{how} {k}")
        np.testing.assert_array_equal(pes["len"], other["len"], err_msg=how)
        L = pes["len"]
        mask = (np.arange(T)[:, None] < L[None]).astype(bool)                 # [T, B]: the entries that were written
        for k in pes["bufs"]:
            np.testing.assert_array_equal(_bits(pes["bufs"][k][mask]), _bits(other["bufs"][k][mask]), err_msg=f"{how} {k}")
        assert pes["iscal"][_lib.I_SIZE] == other["iscal"][_lib.I_SIZE], how
        for slot in range(17):
            if how == "many" or slot in (_lib.D_MAX_DKL, _lib.D_MAX_PATH_RETURN, _lib.D_TOTAL_SAMPLES):
                assert pes["dscal"][slot] == other["dscal"][slot], (how, slot)                  # the same kernels / exact
            else:       # the store's own tiles and fold: float64 sums of the same terms in another order
                np.testing.assert_allclose(other["dscal"][slot], pes["dscal"][slot], rtol=1e-10, atol=0, err_msg=f"{how} {slot}")

    # (b) attached with kappa = 0 == detached
    zero = _roll(w, start, dkl_lim, budget, True, (0.0, 0.0), "loop")
    off = _roll(w, start, dkl_lim, budget, False, (0.0, 0.0), "loop")
    assert zero["on"] and not off["on"]
    for k, a, b in zip(NAMES, zero["get"], off["get"]):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=k)
    assert off["dscal"][_lib.D_TOTAL_V_VAR] == 0.0 and off["dscal"][_lib.D_TOTAL_VC_VAR] == 0.0
    assert off["diag"]["msampler/v_var_perstep"] == 0.0 and off["diag"]["msampler/vc_var_perstep"] == 0.0
    for slot in range(15):
        assert zero["dscal"][slot] == off["dscal"][slot], slot

    # (c) nothing but the values moves; the values are the penalised ones
    for k in (0, 1, 6, 9, 10, 11):                     # obs, act, logp, cost, log_std, mu
        np.testing.assert_array_equal(_bits(pes["get"][k]), _bits(zero["get"][k]), err_msg=NAMES[k])
    np.testing.assert_array_equal(pes["len"], zero["len"])
    for s, (p, z) in enumerate(zip(pes["steps"], zero["steps"])):
        np.testing.assert_array_equal(p["alive"], z["alive"], err_msg=f"alive list after step {s}")
        np.testing.assert_array_equal(p["stored"], z["stored"], err_msg=f"stored rows of step {s}")
        m = p["stored"]
        for k in ("rew_t", "cost_t", "v_var", "vc_var"):
            np.testing.assert_array_equal(_bits(p[k][m]), _bits(z[k][m]), err_msg=f"{k} of step {s}")
        _same(p["v_t"][m], dref.penalise(z["v_t"][m], z["v_var"][m], KAPPA[0], -1), f"v_t of step {s}")
        _same(p["vc_t"][m], dref.penalise(z["vc_t"][m], z["vc_var"][m], KAPPA[1], +1), f"vc_t of step {s}")
        assert (p["v_t"][m] <= z["v_t"][m]).all() and (p["vc_t"][m] >= z["vc_t"][m]).all()
        assert (p["v_t"][m] < z["v_t"][m]).mean() > 0.9 and (p["vc_t"][m] > z["vc_t"][m]).mean() > 0.9
    for k in ("rew_buf", "cost_buf", "obs_buf"):
        mask = (np.arange(T)[:, None] < pes["len"][None]).astype(bool)
        np.testing.assert_array_equal(_bits(pes["bufs"][k][mask]), _bits(zero["bufs"][k][mask]), err_msg=k)
    Lm = np.arange(T)[None] < pes["len"][:, None]              # [B, T], get()'s branch-major order
    v0 = np.stack([st["v_t"] for st in zero["steps"]], 1)
    vc0 = np.stack([st["vc_t"] for st in zero["steps"]], 1)
    vv = np.stack([st["v_var"] for st in zero["steps"]], 1)
    vcv = np.stack([st["vc_var"] for st in zero["steps"]], 1)
    _same(pes["get"][7], dref.penalise(v0[Lm], vv[Lm], KAPPA[0], -1), "val")
    _same(pes["get"][8], dref.penalise(vc0[Lm], vcv[Lm], KAPPA[1], +1), "cval")
    np.testing.assert_array_equal(_bits(zero["get"][7]), _bits(v0[Lm]))
    assert (pes["get"][2] != zero["get"][2]).any() and (pes["get"][3] != zero["get"][3]).any()      # the GAE saw them

    # (d) the totals: float64 sums over the stored rows
    for run in (pes, zero):
        tv = np.concatenate([st["v_var"][st["stored"]].astype(np.float64) for st in run["steps"]])
        tc = np.concatenate([st["vc_var"][st["stored"]].astype(np.float64) for st in run["steps"]])
        n = len(tv)
        assert n == run["dscal"][_lib.D_TOTAL_SAMPLES] and n < 1e5 and (tv >= 0).all() and (tc >= 0).all()
        assert tv.sum() > 0 and tc.sum() > 0
        print(f"B = {B}: {n} stored samples, mean v_var {tv.mean():.3e}, mean vc_var {tc.mean():.3e}, totals' relative distance "
              f"to the host sums {abs(run['dscal'][_lib.D_TOTAL_V_VAR] / tv.sum() - 1):.1e} / "
              f"{abs(run['dscal'][_lib.D_TOTAL_VC_VAR] / tc.sum() - 1):.1e}")
        np.testing.assert_allclose(run["dscal"][_lib.D_TOTAL_V_VAR], tv.sum(), rtol=1e-10, atol=0)
        np.testing.assert_allclose(run["dscal"][_lib.D_TOTAL_VC_VAR], tc.sum(), rtol=1e-10, atol=0)
        np.testing.assert_allclose(run["diag"]["msampler/v_var_perstep"], tv.sum() / (n + 1e-8), rtol=1e-10)
        np.testing.assert_allclose(run["diag"]["msampler/vc_var_perstep"], tc.sum() / (n + 1e-8), rtol=1e-10)


def test_rollout_step_refuses_critics_the_pair_kernel_does_not_take(hip_lib):
    """Attached, cmbpo_rollout_step with 256-wide critics returns -1 before its first launch: nothing of the state moves."""
    _need_gpu()
    import ctypes as C
    import test_disagreement_gpu as tdg
    from cmbpo_amd import _lib
    from cmbpo_amd.pens import PE
    B = 64
    w, start, dkl_lim, _ = tdg._plan(tdg._rollout_batches()[0])
    sampler, pool = tdg._world(w, B, dkl_lim)
    sampler._gen.manual_seed(5)
    sampler.reset(start[:B])
    D = pool.obs_dim
    wide = []
    for _ in range(2):
        m = PE(D, 1, hidden_dims=(256, 256), num_networks=3, num_elites=2, loss="MSE", use_scaler_in=True, use_scaler_out=True,
               device="cuda:0")
        m.init_weights(np.random.RandomState(3))
        wide.append(m)
    assert hip_lib.cmbpo_critic_pair_supported(wide[0].mlp.handle, wide[1].mlp.handle) == 0
    h = sampler._prepare_call(None)
    ck, k, eps_ptr, inds_ptr, _ = sampler._next_draws()
    args = (C.byref(pool.rs), B, h[0], h[1], wide[0].mlp.handle, wide[1].mlp.handle, sampler.env._task_id,
            sampler.env._model.num_nets, eps_ptr, inds_ptr, h[4], h[5], _lib.current_stream())
    pool.set_value_disagreement(True, *KAPPA)
    torch.cuda.synchronize()
    before = {k2: pool.t[k2].clone() for k2 in ("act_t", "next_obs", "rew_t", "v_n", "scal_bytes", "rew_buf")}
    assert hip_lib.cmbpo_rollout_step(*args) == -1
    msg = hip_lib.cmbpo_last_error()
    assert b"cmbpo_rollout_step" in msg and b"cmbpo_value_disagreement_t" in msg and b"128" in msg, msg
    torch.cuda.synchronize()
    for k2, v in before.items():
        assert torch.equal(pool.t[k2].view(torch.uint8), v.view(torch.uint8)), k2
    # detached, the same call takes the general critic kernels as before
    pool.set_value_disagreement(False)
    assert hip_lib.cmbpo_rollout_step(*args) in (0, 1)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------
# 3. ModelBuffer, CPOPolicy
# ------------------------------------------------------------------------------------------------------------------
def test_buffer_and_policy_api(hip_lib):
    _need_gpu()
    from cmbpo_amd.cpo_policy import CPOPolicy
    from cmbpo_amd.modelbuffer import ModelBuffer
    import test_disagreement_gpu as tdg
    buf = ModelBuffer(10, 5, 2, 4, device="cuda:0")
    assert not buf.value_disagreement and "v_var" not in buf.t
    for bad in ((-1.0, 0.0), (0.0, float("nan")), (float("inf"), 0.0)):
        with pytest.raises(ValueError, match="pessimism"):
            buf.set_value_disagreement(True, *bad)
    buf.set_value_disagreement(False, 0.0, 0.25)                           # a coefficient > 0 implies the measurement
    assert buf.value_disagreement and tuple(buf.t["v_var"].shape) == (10,) and buf.t["vdis_part"].dtype == torch.float64
    buf.reset(20)                                                          # new arrays: attached again
    assert tuple(buf.t["vc_var"].shape) == (20,)
    buf.set_value_disagreement(False)
    assert not buf.value_disagreement and "v_var" not in buf.t

    D = 29
    critics = ref.critic_weights(11, 3, D)
    policy = CPOPolicy(tdg._Space(D), tdg._Space(8), a_hidden_layer_sizes=(128, 128), vf_hidden_layer_sizes=(128, 128),
                       vf_ensemble_size=3, vf_elites=2, vf_activation="swish", vf_loss="MSE", device="cuda:0")
    policy.v.set_weights(*critics[0])
    policy.vc.set_weights(*critics[1])
    obs = ref.observations(12, 77, D)
    pair = _Pair(critics, D)
    obs_t = torch.from_numpy(obs).cuda()
    x = pair.members(obs_t, None, 77, 77)
    want = ref.value_disagreement(x[0], x[1])
    for inp in (obs, obs_t):
        got = policy.value_disagreement(inp)
        assert isinstance(got["v"], np.ndarray) == isinstance(inp, np.ndarray)
        for k, name in enumerate(("v", "vc", "v_var", "vc_var")):
            g = got[name] if isinstance(got[name], np.ndarray) else got[name].cpu().numpy()
            np.testing.assert_array_equal(_bits(g), _bits(want[k]), err_msg=name)
    assert policy.value_disagreement_limit() is None
    wide = CPOPolicy(tdg._Space(D), tdg._Space(8), a_hidden_layer_sizes=(128, 128), vf_hidden_layer_sizes=(256, 256),
                     vf_ensemble_size=3, vf_elites=2, vf_activation="swish", vf_loss="MSE", device="cuda:0")
    with pytest.raises(ValueError, match="128"):
        wide.value_disagreement(obs)
    # the limits CMBPO(m_value_disagreement=...) names: width 128, E <= 4, inputs <= 64
    assert "128" in wide.value_disagreement_limit()
    policy.vf_ensemble = 5
    assert "E <= 4" in policy.value_disagreement_limit()
    policy.vf_ensemble, policy.obs_dim = 3, 65
    assert "64" in policy.value_disagreement_limit()


# ------------------------------------------------------------------------------------------------------------------
# 4. the trainer
# ------------------------------------------------------------------------------------------------------------------
def test_cmbpo_pessimistic_value_bootstraps(hip_lib):
    """CMBPO(m_vc_pessimism=1.0) runs two epochs on tests/toyworld.py and logs both new keys > 0; with the three switches at
    their defaults policy and model parameters after two epochs are bitwise those of a run that never passes them (the seeded
    two-epoch run of tests/test_replay_cmbpo_gpu.py); bad coefficients are refused in words."""
    _need_gpu()
    from test_replay_cmbpo_gpu import _two_epochs
    keys = ("model/msampler/v_var_perstep", "model/msampler/vc_var_perstep")
    algo, pes, pi_pes, w_pes = _two_epochs(m_vc_pessimism=1.0)
    assert algo.model_buf.value_disagreement and algo.model_buf.vc_pessimism == 1.0 and algo.model_buf.v_pessimism == 0.0
    assert len(pes) == 2
    for d in pes:
        for k in keys:
            assert np.isfinite(d[k]) and d[k] > 0.0, (k, d[k])
    never, off0, pi0, w0 = _two_epochs()
    default, off1, pi1, w1 = _two_epochs(m_value_disagreement=False, m_v_pessimism=0.0, m_vc_pessimism=0.0)
    assert not never.model_buf.value_disagreement and "v_var" not in never.model_buf.t and "v_var" not in default.model_buf.t
    for d in off0 + off1:
        for k in keys:
            assert d[k] == 0.0, (k, d[k])
    np.testing.assert_array_equal(_bits(pi0), _bits(pi1))
    assert len(w0) == len(w1) == 6
    for a, b in zip(w0, w1):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    measured, on, pi_on, _ = _two_epochs(m_value_disagreement=True)      # measuring alone (kappa = 0) steers nothing
    assert measured.model_buf.value_disagreement and all(d[k] > 0.0 for d in on for k in keys)
    np.testing.assert_array_equal(_bits(pi0), _bits(pi_on))
    for kw in (dict(m_v_pessimism=-1.0), dict(m_vc_pessimism=float("nan")), dict(m_v_pessimism=float("inf"))):
        with pytest.raises(ValueError, match="pessimism"):
            _two_epochs(**kw)


@pytest.mark.parametrize("policy_kw,limit", [(dict(vf_hidden_layer_sizes=(256, 256)), "width 128"), (dict(vf_ensemble_size=5), "E <= 4")])
def test_cmbpo_refuses_critics_the_pair_kernel_does_not_take(hip_lib, policy_kw, limit):
    """Asked for the feature (the switch or a coefficient), CMBPO names the limit the policy's critics break; not asked, it
    builds with the same policy."""
    _need_gpu()
    import toyworld
    from cmbpo_amd.cmbpo import CMBPO
    from cmbpo_amd.cpo_policy import CPOPolicy
    from cmbpo_amd.cpo_sampler import CpoSampler
    from cmbpo_amd.cpobuffer import CPOBuffer
    env = toyworld.ToyEnv()
    kw = dict(a_hidden_layer_sizes=(128, 128), vf_hidden_layer_sizes=(128, 128), vf_ensemble_size=3, vf_elites=2,
              vf_activation="swish", vf_loss="MSE", device="cuda:0", max_path_length=40)
    kw.update(policy_kw)
    policy = CPOPolicy(env.observation_space, env.action_space, **kw)

    def build(**akw):
        buf = CPOBuffer(600, 6000, env.observation_space, env.action_space)
        return CMBPO(env, policy, buf, sampler=CpoSampler(max_path_length=40), task="default", m_networks=4, m_elites=3,
                     m_hidden_dims=(128, 128), rollout_batch_size=64, maxroll=6, **akw)

    for akw in (dict(m_value_disagreement=True), dict(m_v_pessimism=0.5), dict(m_vc_pessimism=1.0)):
        with pytest.raises(ValueError, match=limit):
            build(**akw)
    assert not build().model_buf.value_disagreement
