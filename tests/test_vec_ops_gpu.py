"""GPU: the parameter-vector algebra of the CPO update (csrc/vec_ops.hip) called through the C ABI, against float64 and the
emulations of tests/vec_gae_ref.py (whose docstring derives every bound used here).

Sizes run from 1 over the wave (64) and the reducing workgroup (1024, ragged and full last strides) to the policy's 17154
parameters; lincomb and adam go on to the 64-workgroup cap (65536) and the grid stride beyond it.  Inputs are N(0,1) and
magnitudes spread over 1e-4 .. 1e3.  Ten cmbpo_cg_step on a dense SPD operator are held to float64 CG with the measured
CG_STEP_MARGIN; the fused single-rank solve and the sharded init / fvp / step route are held to the same float64 solve.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import vec_gae_ref as V  # noqa: E402

F32, F64 = np.float32, np.float64
EINVAL = -1          # CMBPO_EINVAL (include/cmbpo_hip.h)
TAIL = 8             # sentinel entries behind every output vector


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _stream():
    from cmbpo_amd import _lib
    return _lib.current_stream()


def _dev(a, tail=0):
    a = np.array(a)              # (a copy: the case arrays are read-only)
    if tail:
        a = np.concatenate([a, np.full(tail, V.SENTINEL, a.dtype)])
    return torch.from_numpy(a).cuda()


def _host(t, P):
    """the first P entries, after asserting that the sentinel behind them is intact"""
    a = t.cpu().numpy()
    assert np.all(a[P:] == V.SENTINEL), "wrote behind entry P - 1"
    return a[:P]


# ---------------------------------------------------------------------------------------------------------------------------
# cmbpo_vec_lincomb
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", V.VEC_SIZES)
def test_lincomb_against_float64(hip_lib, P):
    _need_gpu()
    from cmbpo_amd import _lib
    a, b = V.LINCOMB_A, V.LINCOMB_B
    worst = 0.0
    for fam in V.VEC_FAMILIES:
        x, y = V.vec_input(P, fam, "lin_x"), V.vec_input(P, fam, "lin_y")
        want, scale = V.lincomb64(a, x, b, y)
        for alias in (None, "x", "y"):
            dx, dy, out = _dev(x, TAIL), _dev(y, TAIL), _dev(np.zeros(P, F32), TAIL)
            out = dx if alias == "x" else dy if alias == "y" else out
            _lib.check(hip_lib.cmbpo_vec_lincomb(P, a, dx.data_ptr(), b, dy.data_ptr(), out.data_ptr(), _stream()), "lincomb")
            got = _host(out, P).astype(F64)
            f = V.record("lincomb/%s" % fam, V.frac(np.abs(got - want), V.bound_lincomb(scale)))
            worst = max(worst, f)
            assert f <= 1.0, (P, fam, alias, f)
            for name, t, src in (("x", dx, x), ("y", dy, y)):       # an input that is not the output is left alone
                if alias != name:
                    np.testing.assert_array_equal(_host(t, P), src)
        # y = NULL: b is ignored and the result is the one product, bit for bit
        dx, out = _dev(x, TAIL), _dev(np.zeros(P, F32), TAIL)
        _lib.check(hip_lib.cmbpo_vec_lincomb(P, a, dx.data_ptr(), 7.5, None, out.data_ptr(), _stream()), "lincomb")
        np.testing.assert_array_equal(_host(out, P), V.lincomb_emul(a, x))
    print("lincomb P = %d: worst error %.3f of the bound" % (P, worst))


def test_lincomb_arguments(hip_lib):
    _need_gpu()
    x = _dev(np.ones(4, F32))
    assert hip_lib.cmbpo_vec_lincomb(0, 1.0, x.data_ptr(), 0.0, None, x.data_ptr(), _stream()) == EINVAL
    assert hip_lib.cmbpo_vec_lincomb(4, 1.0, None, 0.0, None, x.data_ptr(), _stream()) == EINVAL
    assert hip_lib.cmbpo_vec_lincomb(4, 1.0, x.data_ptr(), 0.0, None, None, _stream()) == EINVAL


# ---------------------------------------------------------------------------------------------------------------------------
# cmbpo_vec_dots
# ---------------------------------------------------------------------------------------------------------------------------
def _dots(hip_lib, P, n, xs, ys, out):
    px = (C.c_void_p * max(n, 1))(*[t.data_ptr() for t in xs[:n]])
    py = (C.c_void_p * max(n, 1))(*[t.data_ptr() for t in ys[:n]])
    return hip_lib.cmbpo_vec_dots(P, n, px, py, out.data_ptr(), _stream())


@pytest.mark.parametrize("P", V.VEC_SMALL)
def test_dots_against_float64(hip_lib, P):
    _need_gpu()
    worst = 0.0
    for fam in V.VEC_FAMILIES:
        vs = V.dots_case(P, fam)
        dv = [_dev(v) for v in vs]
        ref = [V.dots64(vs[i], vs[j]) for i, j in V.DOT_PAIRS]
        for n in V.DOT_COUNTS:
            out = torch.full((16,), V.SENTINEL, dtype=torch.float64, device="cuda")
            rc = _dots(hip_lib, P, n, [dv[i] for i, _ in V.DOT_PAIRS], [dv[j] for _, j in V.DOT_PAIRS], out)
            assert rc == 0, hip_lib.cmbpo_last_error()
            got = out.cpu().numpy()
            assert np.all(got[n:] == V.SENTINEL), "a slot beyond n was written"
            for k in range(n):
                s64, sabs = ref[k]
                f = V.record("dots/%s" % fam, V.frac(abs(got[k] - s64), V.bound_dot(P, sabs)))
                worst = max(worst, f)
                assert f <= 1.0, (P, fam, n, k, got[k], s64, f)
    print("dots P = %d: worst error %.3g of the bound" % (P, worst))


def test_dots_arguments(hip_lib):
    _need_gpu()
    v = [_dev(np.ones(8, F32))] * 9
    out = torch.full((16,), V.SENTINEL, dtype=torch.float64, device="cuda")
    assert _dots(hip_lib, 8, 9, v, v, out) == EINVAL
    assert _dots(hip_lib, 0, 1, v, v, out) == EINVAL
    assert _dots(hip_lib, 8, 0, v, v, out) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == V.SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------------
# cmbpo_cg_init, cmbpo_cg_step
# ---------------------------------------------------------------------------------------------------------------------------
def _scal(rr=0.0):
    s = torch.full((16,), V.SENTINEL, dtype=torch.float64, device="cuda")
    s[0] = float(rr)
    return s


@pytest.mark.parametrize("P", V.VEC_SMALL)
def test_cg_init(hip_lib, P):
    _need_gpu()
    from cmbpo_amd import _lib
    for fam in V.VEC_FAMILIES:
        b = V.vec_input(P, fam, "cg_b")
        db = _dev(b, TAIL)
        x, r, p = (_dev(np.full(P, 3.5, F32), TAIL) for _ in range(3))
        scal = _scal(123.0)
        _lib.check(hip_lib.cmbpo_cg_init(P, db.data_ptr(), x.data_ptr(), r.data_ptr(), p.data_ptr(), scal.data_ptr(), _stream()),
                   "cmbpo_cg_init")
        assert np.all(_host(x, P) == 0)
        np.testing.assert_array_equal(_host(r, P), b)
        np.testing.assert_array_equal(_host(p, P), b)
        np.testing.assert_array_equal(_host(db, P), b)
        s = scal.cpu().numpy()
        assert s[1] == -1.0 and np.all(s[2:] == V.SENTINEL)
        assert s[0] == float(F32(s[0])), "scal[0] is not a float32 value"
        u = V.record("cg_init/rr_ulp", float(V.ulps(s[0], F32(V.dots64(b, b)[0]))))
        assert u <= 1.0, (P, fam, s[0])


@pytest.mark.parametrize("P", V.VEC_SMALL)
def test_cg_single_step_against_the_emulation(hip_lib, P):
    _need_gpu()
    from cmbpo_amd import _lib
    worst = {}
    for fam in V.VEC_FAMILIES:
        c = V.cg_step_case(P, fam)
        hp, x, r, p = (_dev(c[k], TAIL) for k in ("hp_sum", "x", "r", "p"))
        scal = _scal(c["rr"])
        _lib.check(hip_lib.cmbpo_cg_step(P, hp.data_ptr(), V.CG_INV_N, V.CG_DAMPING, x.data_ptr(), r.data_ptr(), p.data_ptr(),
                                         scal.data_ptr(), _stream()), "cmbpo_cg_step")
        s = scal.cpu().numpy()
        assert np.all(s[1:] == V.SENTINEL), "scal[1] or a slot behind it was written"
        assert s[0] == float(F32(s[0])), "scal[0] is not a float32 value"
        np.testing.assert_array_equal(_host(hp, P), c["hp_sum"])
        got = dict(x=_host(x, P), r=_host(r, P), p=_host(p, P), rr=s[0])
        if P >= 3:
            got["alpha"] = got["x"][P // 2]             # x_j = 0, p_j = 1 went in
        f = V.cg_step_fractions(got, c)
        for k, v in f.items():
            V.record("cg_step/%s/%s" % (fam, k), v)
            worst[k] = max(worst.get(k, 0.0), v)
        assert max(f.values()) <= 1.0, (P, fam, f)
    print("cg_step P = %d: worst fraction of the bound %s" % (P, {k: "%.3g" % v for k, v in worst.items()}))


def _device_cg_dense(hip_lib, op):
    """cmbpo_cg_init and CG_ITERS cmbpo_cg_step, the operator's hp_sum computed in float64 on the host from the device's p"""
    from cmbpo_amd import _lib
    P = op.P
    b = _dev(op.b)
    x, r, p = (_dev(np.full(P, 3.5, F32), TAIL) for _ in range(3))
    scal = _scal()
    _lib.check(hip_lib.cmbpo_cg_init(P, b.data_ptr(), x.data_ptr(), r.data_ptr(), p.data_ptr(), scal.data_ptr(), _stream()),
               "cmbpo_cg_init")
    for _ in range(V.CG_ITERS):
        hp = _dev(op.hp_sum(_host(p, P)))
        _lib.check(hip_lib.cmbpo_cg_step(P, hp.data_ptr(), V.CG_INV_N, V.CG_DAMPING, x.data_ptr(), r.data_ptr(), p.data_ptr(),
                                         scal.data_ptr(), _stream()), "cmbpo_cg_step")
    return _host(x, P)


def cg_dense_ratio(hip_lib, P):
    """(err, e32, err / max(e32, FLOOR)) of the device's ten steps against float64 CG (also what tools/probe_vec_gae.py records)"""
    op = V.dense_operator(P)
    fig = op.figures()
    err = V.whole_error(_device_cg_dense(hip_lib, op), fig["x64"])
    return err, fig["e32"], err / max(fig["e32"], V.FLOOR)


@pytest.mark.parametrize("P", V.CG_DENSE_SIZES)
def test_ten_cg_steps_against_float64_cg(hip_lib, P):
    _need_gpu()
    assert V.CG_STEP_MARGIN is not None
    err, e32, ratio = cg_dense_ratio(hip_lib, P)
    V.record("cg_dense/%d/ratio" % P, ratio)
    V.RECORDS["cg_dense/%d/err" % P], V.RECORDS["cg_dense/%d/e32" % P] = err, e32
    print("cg dense P = %d: err %.3g / e32 %.3g = %.3f (margin %g)" % (P, err, e32, ratio, V.CG_STEP_MARGIN))
    assert err <= V.CG_STEP_MARGIN * max(e32, V.FLOOR), (err, e32)


class _World2:
    """two ranks whose all-reduce is the identity: PolicyOps takes the sharded route on the whole batch"""
    world, rank = 2, 0

    def __init__(self):
        self.reduced = 0

    def all_reduce_sum(self, t):
        self.reduced += 1
        return t

    def all_reduce_host(self, x):
        return x


@pytest.fixture(params=[1, 0], ids=["splitf16", "fp32mfma"])
def pi_path(request, hip_lib):
    before = hip_lib.cmbpo_get_pi_matrix_path()
    hip_lib.cmbpo_set_pi_matrix_path(request.param)
    yield request.param
    hip_lib.cmbpo_set_pi_matrix_path(before)


def test_the_two_cg_routes_meet_the_same_float64_solve(hip_lib, pi_path):
    _need_gpu()
    import pi_f64_ref as R
    from cmbpo_amd.cpo_update import PolicyOps
    c = R.case(29, 8, 1037, 128)
    ref = R.reference_of(c)
    fig = ref.cg_figures()
    bound = R.CG_MARGIN * max(fig["e32"], R.FLOOR)
    comm = _World2()
    sharded = PolicyOps(c.D, c.A, c.hidden, device="cuda:0", comm=comm)
    sharded.set_params(np.array(ref.theta))
    errs = {}
    for name, ops in (("fused", R.make_ops(ref)), ("sharded", sharded)):
        R.bind(ops, ref)
        assert ops.n_global == ref.n
        before = getattr(ops, "n_fvp", 0)
        x = R.gpu_cg(ops, ref)          # (sets theta_old; both routes get the same b)
        assert getattr(ops, "n_fvp", 0) - before == R.CG_ITERS
        errs[name] = R.whole_error(x, fig["x64"])
        V.record("cg_routes/%s/path%d" % (name, pi_path), errs[name] / bound)
    assert comm.reduced == R.CG_ITERS, "the stub's all-reduce did not see one product per iteration"
    print("cg routes (path %d): fused %.3g, sharded %.3g, bound %.3g (e32 %.3g)" % (pi_path, errs["fused"], errs["sharded"], bound,
                                                                                   fig["e32"]))
    assert errs["fused"] <= bound and errs["sharded"] <= bound, (errs, bound)


# ---------------------------------------------------------------------------------------------------------------------------
# cmbpo_vec_adam_step
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", V.ADAM_SIZES)
def test_adam_step_matches_float64_tf_adam(hip_lib, P):
    """tests/test_ppo_lag_gpu.py::test_adam_step_matches_float64_tf_adam at other sizes, through the C ABI: five steps, the same
    gradient five times and five different ones, the change of the parameter per step and entry within 1e-5 lr + 2 ulp(theta)."""
    _need_gpu()
    import ppo_lag_ref as ref
    from cmbpo_amd import _lib
    rng = np.random.default_rng(5 + P)
    lr = 1e-3
    theta0 = rng.standard_normal(P).astype(F32)
    special = np.array([0.0, 1e-12, -1e-12, 1e3, -1e3], F32)
    k = min(P, 50)
    worst = 0.0
    for same in (True, False):
        theta, m_d, v_d = _dev(theta0, TAIL), _dev(np.zeros(P, F32), TAIL), _dev(np.zeros(P, F32), TAIL)
        state = torch.zeros(_lib.PPO_STATE_DOUBLES, dtype=torch.float64, device="cuda")
        th, m, v, t = theta0.astype(F64), np.zeros(P), np.zeros(P), 0
        prev = theta0.astype(F64)
        gmax = np.zeros(P)
        for step in range(5):
            if step == 0 or not same:
                g = (rng.standard_normal(P) * 10.0 ** rng.uniform(-6, 1, P)).astype(F32)
                g[:k] = np.tile(special, 10)[:k]
                if not same:
                    g[:k] = np.roll(g[:k], step)
            gmax = np.maximum(gmax, np.abs(g))
            dg = _dev(g)
            _lib.check(hip_lib.cmbpo_vec_adam_step(P, dg.data_ptr(), m_d.data_ptr(), v_d.data_ptr(), theta.data_ptr(),
                                                   state.data_ptr(), lr, 0.9, 0.999, 1e-8, _stream()), "cmbpo_vec_adam_step")
            th_new, m, v, t = ref.adam_step(th, m, v, t, g.astype(F64), lr, b1=float(F32(0.9)), b2=float(F32(0.999)))
            got = _host(theta, P).astype(F64)
            err = np.abs((got - prev) - (th_new - th))
            bound = V.adam_bound(lr, got)
            worst = max(worst, V.record("adam/%d" % P, float(np.max(err / bound))))
            assert np.all(err <= bound), "step %d: worst %g of the bound" % (step, float(np.max(err / bound)))
            prev, th = got, th_new
        st = state.cpu().numpy()
        assert st[_lib.PPO_ST_ADAM_T] == 5 and np.all(np.delete(st, _lib.PPO_ST_ADAM_T) == 0)
        assert np.all(np.abs(_host(m_d, P) - m) <= 1e-5 * np.abs(m) + 1e-6 * gmax)
        assert np.all(np.abs(_host(v_d, P) - v) <= 1e-5 * np.abs(v) + 1e-6 * gmax ** 2)
    print("adam_step P = %d: worst error %.3f of the bound" % (P, worst))
