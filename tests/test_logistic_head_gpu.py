"""GPU: training steps of the probabilistic heads with logistic columns against tests/logistic_head_ref.py (float64
torch on oracle/reftrain.py's forward).

Tolerances are those of tests/test_ens_train_gpu.py, the arithmetic being the same (fp32 / two-piece f16 products, sums over the
batch in another order than the reference):
  * gradients (read back as 10 x the first Adam moment after step 1): |d| <= 2e-3 |ref| + 5e-5 max|ref| per tensor;
  * per-member losses: rtol 2e-4;
  * k Adam steps: || w_hip - w_ref || <= 3e-2 || w_ref - w_init ||.
The shapes are those of tests/test_column_weights_gpu.py: both f16 kernels with a full and a ragged item, the fp32 chain and
forward, the f16 chain behind the fp32 forward."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import logistic_head_ref as ref  # noqa: E402


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# E, I, H, D, loss, batch, f16 paths (bit 0 the f16 backward chain, bit 1 the f16 training forward), logistic columns
SHAPES = [
    (3, 11, 128, 4, "MSPE", 100, 0, (-1,)),
    (2, 37, 512, 32, "MSPE", 97, 3, (-1,)),
    (2, 37, 512, 32, "NLL", 97, 3, (-2, -1)),     # the last two columns
    (2, 20, 512, 40, "MSPE", 70, 0, (-1,)),
    (2, 70, 512, 5, "MSPE", 40, 1, (-1,)),
    (4, 20, 256, 6, "MSPE", 33, 0, (-1,)),
    (3, 11, 128, 4, "NLL", 1, 0, (-1,)),          # a single row
]
_ID = lambda s: "%dx%d-%d-%d-%s-b%d" % s[:6]
MODES = (None, "col", "pos", "both")


def _weights(D, mode, rng):
    cw = rng.uniform(0.5, 4.0, D).astype(np.float32)
    cw[1] = 0.0
    pw = np.ones(D, np.float32)
    pw[-2:] = (7.0, 3.0)
    return (cw if mode in ("both", "col") else None), (pw if mode in ("both", "pos") else None)


_DATA = {}


def _data(E, I, D, n, seed):
    """Inputs, targets (the last two columns Bernoulli(sigma(1.5 x0 - 1.5)), drawn independently) and their scalers: computed
    once per shape and shared, never written."""
    key = (E, I, D, n, seed)
    if key not in _DATA:
        rng = np.random.RandomState(seed)
        x = (rng.standard_normal((n, I)) * (1 + rng.rand(I)) + rng.standard_normal(I)).astype(np.float32)
        wtrue = rng.standard_normal((I, D)) / np.sqrt(I)
        t = (np.tanh(x @ wtrue) + 0.1 * rng.standard_normal((n, D))).astype(np.float32)
        x0 = (x[:, 0] - x[:, 0].mean()) / x[:, 0].std()
        p = 1.0 / (1.0 + np.exp(-(1.5 * x0 - 1.5)))
        for col in (D - 2, D - 1):
            t[:, col] = (rng.rand(n) < p).astype(np.float32)
        sc_in = (x.mean(0, keepdims=True), x.var(0, keepdims=True))
        sc_out = (t.mean(0, keepdims=True), t.var(0, keepdims=True))
        for a in (x, t):
            a.setflags(write=False)
        _DATA[key] = (x, t, sc_in, sc_out)
    return _DATA[key]


def _kinds(D, cols):
    k = np.zeros(D, np.uint8)
    for c in cols:
        k[c] = 1
    return k


def _make(E, I, H, D, loss, n, seed, cols=(-1,), mode=None, lr=1e-3, decay=1e-3, b2=None):
    """PE with `cols` logistic and the float64 reference on the same weights.  b2: a hand-set bias of the last layer."""
    from cmbpo_amd.pens import PE
    x, t, sc_in, sc_out = _data(E, I, D, n, seed)
    rng = np.random.RandomState(seed + 1)
    cw, pw = _weights(D, mode, rng) if mode else (None, None)
    pe = PE(I, D, name="T", hidden_dims=(H, H), num_networks=E, num_elites=max(1, E - 2), loss=loss, use_scaler_in=True,
            use_scaler_out=True, device="cuda:0", lr=lr, decay=decay, col_weight=cw, pos_weight=pw, logistic_columns=cols)
    ws, bs = pe.init_weights(rng)
    bs = [(0.1 * rng.standard_normal(b.shape)).astype(np.float32) for b in bs]
    ws[2] = (ws[2] * 3).astype(np.float32)
    if b2 is not None:
        bs[2] = b2(bs[2])
    pe.set_weights(ws, bs, sc_in, sc_out)
    kinds = None if not cols else _kinds(D, cols)
    rt = ref.LogisticTrainer(ws, bs, loss, pe.decays, lr=lr, kinds=kinds, col_weight=cw, pos_weight=pw)
    # (the reference ignores the output scaler on logistic columns; PE pinned it there, and both see the pinned moments)
    rt.set_scalers(sc_in, (pe.scaler_out.cached_mu, pe.scaler_out.cached_var) if cols else sc_out)
    return rng, pe, rt, x, t, ws, bs


def _close(got, want, rtol, arel, msg):
    np.testing.assert_allclose(got, want, rtol=rtol, atol=arel * float(np.max(np.abs(want))) + 1e-12, err_msg=msg)


def _dev(a):
    return torch.tensor(np.asarray(a)).cuda()      # (a copy: the shared arrays are read-only)


def test_the_targets_are_bernoulli_of_the_stated_rate():
    """On the reference's side, before anything else: mean sigma(1.5 x0 - 1.5) over a standard normal x0 is 0.23; 300 draws lie
    within 4 standard errors (4 sqrt(0.23 0.77 / 300) = 0.10), and both classes occur."""
    for s in SHAPES:
        E, I, H, D = s[:4]
        _, t, _, _ = _data(E, I, D, 300, seed=E * 1000 + I + D)
        for col in (D - 2, D - 1):
            share = float(t[:, col].mean())
            assert set(np.unique(t[:, col])) == {0.0, 1.0}
            assert 0.13 <= share <= 0.33, (s, col, share)


CASES = [(s, None) for s in SHAPES] + [(s, m) for s in SHAPES[:3] for m in ("col", "pos", "both")]


@pytest.mark.parametrize("shape,mode", CASES, ids=[_ID(s) + "-" + str(m) for s, m in CASES])
def test_first_step_gradients_and_losses(hip_lib, shape, mode):
    _need_gpu()
    E, I, H, D, loss, batch, bits, cols = shape
    rng, pe, rt, x, t, ws, bs = _make(E, I, H, D, loss, max(300, 2 * batch), seed=E * 1000 + I + D, cols=cols, mode=mode)
    tr = pe._ensure_trainer(batch)
    assert tr.f16_paths == bits
    idx = rng.randint(0, x.shape[0], size=(E, batch)).astype(np.int32)
    xd, td, idx_d = _dev(x), _dev(t), _dev(idx)
    hold = rng.permutation(x.shape[0])[:157].astype(np.int32)
    got = tr.losses(xd, td, _dev(hold), 0, hold.shape[0]).cpu().numpy()
    np.testing.assert_allclose(got, rt.losses(np.tile(x[hold][None], (E, 1, 1)), np.tile(t[hold][None], (E, 1, 1))), rtol=2e-4)
    got = tr.losses(xd, td, idx_d, batch, batch).cpu().numpy()
    np.testing.assert_allclose(got, rt.losses(x[idx], t[idx]), rtol=2e-4)

    _, gs = rt.grads(x[idx], t[idx])
    tr.step(xd, td, idx_d.data_ptr(), batch, batch)
    mw, mb = tr.get_moments(0)
    for l in range(3):
        _close(10.0 * mw[l], gs[l].numpy(), 2e-3, 5e-5, f"dW{l}")
        _close(10.0 * mb[l], gs[3 + l].numpy().reshape(mb[l].shape), 2e-3, 5e-5, f"db{l}")
    if loss == "NLL":
        # the log-variance output of a logistic column has no term at all: every delta exactly 0, so is their column sum
        for c in cols:
            assert float(np.abs(mb[2][:, 0, 2 * D + c]).max()) == 0.0
    assert tr.steps_done == 1


def _steps(pe, x, t, E, batch, n_steps, seed, before=None):
    """n_steps steps on index lists drawn from `seed`; the trainer's weights and first moments afterwards."""
    tr = pe._ensure_trainer(batch)
    if before is not None:
        before(pe)
    rng = np.random.RandomState(seed)
    xd, td = _dev(x), _dev(t)
    for _ in range(n_steps):
        idx = _dev(rng.randint(0, x.shape[0], size=(E, batch)).astype(np.int32))
        tr.step(xd, td, idx.data_ptr(), batch, batch)
    w, b = tr.get_weights()
    mw, mb = tr.get_moments(0)
    return w + b + mw + mb


@pytest.mark.parametrize("shape", SHAPES[:2] + SHAPES[2:3], ids=[_ID(s) for s in SHAPES[:3]])
def test_the_columns_do_not_leak_into_each_other(hip_lib, shape):
    """The mean-head bias gradient of every Gaussian column equals, bit for bit, the one of a step on the same model whose
    logistic columns are Gaussian columns of weight 0 -- no data term there at all.  A column of weight 0 adds exact zeros to
    'MSPE''s two sums, so even the ratio, the one coupling the reference states, is the same number in both steps."""
    _need_gpu()
    E, I, H, D, loss, batch, _, cols = shape
    _, pe, _, x, t, _, _ = _make(E, I, H, D, loss, 300, seed=41, cols=cols)
    with_kinds = _steps(pe, x, t, E, batch, 1, seed=8)
    _, pe2, _, _, _, _, _ = _make(E, I, H, D, loss, 300, seed=41, cols=())
    # (the same pinned scaler, so that the Gaussian columns see the same scaled targets; the silent columns' do not matter)
    pe2.set_weights(*pe2.get_weights(), None, (pe.scaler_out.cached_mu, pe.scaler_out.cached_var))
    cw = np.ones(D, np.float32)
    for c in cols:
        cw[c] = 0.0
    silent = _steps(pe2, x, t, E, batch, 1, seed=8, before=lambda p: p.set_column_weights(cw, None))
    gauss = [d for d in range(D) if d not in [c % D for c in cols]]
    mb_a, mb_b = with_kinds[-1], silent[-1]              # first moment of b2
    np.testing.assert_array_equal(mb_a[:, 0, gauss], mb_b[:, 0, gauss])
    assert float(np.abs(mb_a[:, 0, [c % D for c in cols]]).max()) > 0.0 and float(np.abs(mb_b[:, 0, [c % D for c in cols]]).max()) == 0.0


BITWISE = SHAPES[:5]


@pytest.mark.parametrize("shape", BITWISE, ids=[_ID(s) for s in BITWISE])
def test_a_step_with_kinds_is_bitwise_reproducible(hip_lib, shape):
    """No atomics on the gradient path, the statistics over the Gaussian columns included."""
    _need_gpu()
    E, I, H, D, loss, batch, _, cols = shape
    outs = []
    for _ in range(2):
        _, pe, _, x, t, _, _ = _make(E, I, H, D, loss, 300, seed=99, cols=cols, mode="both")
        outs.append(_steps(pe, x, t, E, batch, 2, seed=5))
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("weights", [None, "both"])
@pytest.mark.parametrize("shape", BITWISE, ids=[_ID(s) for s in BITWISE])
def test_detached_and_all_zero_kinds_are_the_step_without_kinds(hip_lib, shape, weights):
    """Attach, detach, step == a trainer that never had kinds, and so are all-zero kinds (at the C-ABI; PE's ``()``), bit for
    bit, with and without column weights attached; kinds with all-ones weights == kinds alone."""
    _need_gpu()
    E, I, H, D, loss, batch, _, cols = shape

    def run(before, cols_at_start=()):
        _, pe, _, x, t, _, _ = _make(E, I, H, D, loss, 300, seed=17, cols=cols_at_start, mode=weights)
        return _steps(pe, x, t, E, batch, 2, seed=6, before=before), pe

    plain, _ = run(None)

    def attach_detach(pe):
        mu, var = pe.scaler_out.cached_mu.copy(), pe.scaler_out.cached_var.copy()
        pe.set_logistic_columns(cols)
        pe.set_logistic_columns(None)
        pe.set_weights(*pe.get_weights(), None, (mu, var))        # (the pin is PE's business: the scaler it replaced comes back)
        pe._trainer.set_column_kinds(None)

    def zero_kinds(pe):
        pe._trainer.set_column_kinds(np.zeros(D, np.uint8))

    for before in (attach_detach, zero_kinds):
        got, _ = run(before)
        for a, b in zip(plain, got):
            np.testing.assert_array_equal(a, b)
    # ... and the kinds do change the step (the comparison above is not vacuous)
    with_kinds, _ = run(None, cols)
    assert any(not np.array_equal(a, b) for a, b in zip(plain, with_kinds))
    if weights is None:
        one = np.ones(D, np.float32)
        for cw, pw in ((one, one), (one, None), (None, one)):
            got, _ = run(lambda pe: pe.set_column_weights(cw, pw), cols)
            for a, b in zip(with_kinds, got):
                np.testing.assert_array_equal(a, b)


TRACK = [SHAPES[0], SHAPES[1], SHAPES[2], SHAPES[5]]


@pytest.mark.parametrize("shape", TRACK, ids=[_ID(s) for s in TRACK])
def test_three_adam_steps_track_the_reference(hip_lib, shape):
    _need_gpu()
    E, I, H, D, loss, batch, _, cols = shape
    rng, pe, rt, x, t, ws, bs = _make(E, I, H, D, loss, 300, seed=7 + E, cols=cols, mode="pos")
    tr = pe._ensure_trainer(batch)
    xd, td = _dev(x), _dev(t)
    w_init = [w.copy() for w in ws]
    for k in range(3):
        b = batch if k != 1 else max(1, batch - 9)      # a ragged batch in the middle
        idx = rng.randint(0, x.shape[0], size=(E, b)).astype(np.int32)
        tr.step(xd, td, _dev(idx).data_ptr(), b, b)
        rt.step(x[idx], t[idx])
    gw, gb = tr.get_weights()
    for l in range(3):
        rw = rt.ws[l].numpy()
        moved = float(np.linalg.norm(rw - w_init[l]))
        assert float(np.linalg.norm(gw[l] - rw)) <= 3e-2 * moved, (l, moved)
        rb = rt.bs[l].numpy().reshape(gb[l].shape)
        assert float(np.linalg.norm(gb[l] - rb)) <= 3e-2 * float(np.linalg.norm(rb - bs[l].reshape(rb.shape))) + 1e-7


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[3]], ids=[_ID(s) for s in (SHAPES[0], SHAPES[1], SHAPES[3])])
@pytest.mark.parametrize("sign", [60.0, -60.0])
def test_a_saturated_logit_gives_finite_deltas_equal_to_the_reference(hip_lib, shape, sign):
    """The output bias of the logistic column set by hand to +-60 on one member: sigma - y is 0 or +-1 to float32 precision on
    every row, l is 60 or e^-60; gradients and `self.loss` stay finite and equal the reference's."""
    _need_gpu()
    E, I, H, D, loss, batch, _, cols = shape

    def b2(b):
        b = b.copy()
        b.reshape(E, -1)[0, D - 1] = sign
        return b

    rng, pe, rt, x, t, ws, bs = _make(E, I, H, D, loss, 300, seed=23, cols=cols, b2=b2)
    tr = pe._ensure_trainer(batch)
    idx = rng.randint(0, x.shape[0], size=(E, batch)).astype(np.int32)
    xd, td, idx_d = _dev(x), _dev(t), _dev(idx)
    got = tr.losses(xd, td, idx_d, batch, batch).cpu().numpy()
    want = rt.losses(x[idx], t[idx])
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want))
    np.testing.assert_allclose(got, want, rtol=2e-4)
    _, gs = rt.grads(x[idx], t[idx])
    tr.step(xd, td, idx_d.data_ptr(), batch, batch)
    mw, mb = tr.get_moments(0)
    for l in range(3):
        assert np.all(np.isfinite(mw[l])) and np.all(np.isfinite(mb[l]))
        _close(10.0 * mw[l], gs[l].numpy(), 2e-3, 5e-5, f"dW{l}")
        _close(10.0 * mb[l], gs[3 + l].numpy().reshape(mb[l].shape), 2e-3, 5e-5, f"db{l}")


def test_refusals_that_need_a_trainer(hip_lib):
    """A deterministic head and a wrong target_dim, by name; the *_ex entries go on refusing a probabilistic head with kinds
    attached; a new, larger trainer gets the kinds again."""
    _need_gpu()
    from cmbpo_amd import _lib
    from cmbpo_amd.pens import PE
    two = (C.c_ubyte * 2)(0, 1)
    det = PE(5, 2, hidden_dims=(128, 128), num_networks=2, num_elites=1, loss="MSE", device="cuda:0")
    det.init_weights(np.random.RandomState(0))
    h = det._ensure_trainer(32)._h
    assert hip_lib.cmbpo_trainer_set_column_kinds(h, C.cast(two, C.c_void_p), 2, None) == -1
    msg = hip_lib.cmbpo_last_error()
    assert b"cmbpo_trainer_set_column_kinds" in msg and b"deterministic" in msg
    assert hip_lib.cmbpo_trainer_set_column_kinds(h, None, 0, None) == 0        # detaching nothing is no error

    _, pe, _, x, t, _, _ = _make(3, 11, 128, 4, "MSPE", 300, seed=3)
    tr = pe._ensure_trainer(32)
    assert hip_lib.cmbpo_trainer_set_column_kinds(tr._h, C.cast(two, C.c_void_p), 2, None) == -1
    assert b"target_dim 2 != 4" in hip_lib.cmbpo_last_error()
    xd, td = _dev(x), _dev(t)
    idx = _dev(np.zeros((3, 32), np.int32))
    with pytest.raises(_lib.CmbpoHipError, match="MSPE"):
        tr.step(xd, td, idx.data_ptr(), 32, 32, weights=torch.ones(300, device="cuda"))
    with pytest.raises(_lib.CmbpoHipError, match="MSPE"):
        tr.losses(xd, td, idx, 32, 32, weights=torch.ones(300, device="cuda"))
    before = tr.losses(xd, td, idx, 32, 32).cpu().numpy()
    tr2 = pe._ensure_trainer(64)
    assert tr2 is not tr
    np.testing.assert_array_equal(tr2.losses(xd, td, idx, 32, 32).cpu().numpy(), before)
    tr2.set_column_kinds(None)
    assert not np.array_equal(tr2.losses(xd, td, idx, 32, 32).cpu().numpy(), before)


def test_predict_returns_the_logit(hip_lib):
    """With the scaler pinned the forward's mean in a logistic column is the raw output: the reference's z, to the forward's
    tolerance."""
    _need_gpu()
    _, pe, rt, x, t, _, _ = _make(3, 11, 128, 4, "MSPE", 300, seed=29)
    mean, _ = pe.predict_ensemble(x[:64])
    o, _, _, _, _ = rt._forward(rt.ws, rt.bs, np.tile(x[:64][None], (3, 1, 1)), np.tile(t[:64][None], (3, 1, 1)))
    np.testing.assert_allclose(mean[:, :, 3], o[:, :, 3].numpy(), rtol=2e-3, atol=2e-4)


# -----------------------------------------------------------------------------------------------------------------------
# Fixed point.  One target column Bernoulli(sigma(3 x0)) beside three Gaussian columns; E = 3, H = 128, 4000 training rows, 40
# epochs, 4000 fresh rows.  The held-out Bernoulli NLL of every member's sigma(z) against the Bayes value of those rows, computed
# on the host from the generating p.
# EXCESS_BOUND is twice the largest excess measured for three seeds on an MI355X (profiles/r19/logistic_head.json).
# -----------------------------------------------------------------------------------------------------------------------
# Largest excess over a seed's three members and both losses, seeds 0 / 1 / 2 (tools/probe_logistic_head.py --fixed-point).  The third
# is negative: the held-out NLL is a mean over 4000 realised labels, the Bayes value its expectation.
MEASURED_EXCESS = (0.0168, 0.0117, -0.0189)
EXCESS_BOUND = 2.0 * max(MEASURED_EXCESS)


def fixed_point(loss, seed, logistic=True):
    """(per-member held-out NLL excess over Bayes, per-member mean sigma(z), the rows' positive rate, share of predictions
    outside [0, 1])."""
    from cmbpo_amd.pens import PE
    from cmbpo_amd.utils import sigmoid
    rng = np.random.RandomState(seed)
    n = 4000

    def draw(n):
        x = rng.standard_normal((n, 6)).astype(np.float32)
        p = sigmoid(3.0 * x[:, 0].astype(np.float64))
        t = np.empty((n, 4), np.float32)
        t[:, :3] = np.tanh(x @ W) + 0.1 * rng.standard_normal((n, 3))
        t[:, 3] = rng.rand(n) < p
        return x, t, p

    W = rng.standard_normal((6, 3)) / np.sqrt(6)
    x, t, _ = draw(n)
    fx, ft, fp = draw(n)
    bayes = float(np.mean(-fp * np.log(fp) - (1 - fp) * np.log1p(-fp)))
    pe = PE(6, 4, name="T", hidden_dims=(128, 128), num_networks=3, num_elites=2, loss=loss, use_scaler_in=True,
            use_scaler_out=True, device="cuda:0", lr=1e-3, logistic_columns=[-1] if logistic else None)
    pe.init_weights(np.random.RandomState(seed + 1))
    pe.train(x, t, batch_size=256, max_epochs=40, holdout_ratio=0.0, rng=np.random.RandomState(seed + 2))
    mean, _ = pe.predict_ensemble(fx)
    z = mean[:, :, 3].astype(np.float64)
    if not logistic:
        return None, z.mean(axis=1), float(ft[:, 3].mean()), float(np.mean((z < 0.0) | (z > 1.0)))
    y = ft[:, 3].astype(np.float64)[None]
    nll = (np.maximum(z, 0.0) - y * z + np.log1p(np.exp(-np.abs(z)))).mean(axis=1)
    sg = sigmoid(z)
    return nll - bayes, sg.mean(axis=1), float(ft[:, 3].mean()), float(np.mean((sg < 0.0) | (sg > 1.0)))


@pytest.mark.parametrize("loss", ["MSPE", "NLL"])
def test_fixed_point_reaches_the_bayes_value(hip_lib, loss):
    """Fails without the feature: the Gaussian head's values are no logits (a share of them lies outside [0, 1], measured
    0.20-0.24 under 'MSPE' and 0.075-0.085 under 'NLL'), the logistic head's sigma(z) cannot."""
    _need_gpu()
    excess, level, rate, outside = fixed_point(loss, 0)
    print("loss %s: excess over Bayes per member %s (bound %.4f), mean sigma %s against the rate %.4f"
          % (loss, np.round(excess, 4), EXCESS_BOUND, np.round(level, 4), rate))
    assert np.all(excess <= EXCESS_BOUND), (excess, EXCESS_BOUND)
    assert np.all(np.abs(level - rate) <= 0.05), (level, rate)
    assert outside == 0.0
    _, _, _, gaussian_outside = fixed_point(loss, 0, logistic=False)
    assert gaussian_outside > 0.0


# -----------------------------------------------------------------------------------------------------------------------
# Float64 inputs: the new chain, statistics and loss instances under the yardstick, the data and the bound MARGIN * max(e32,
# FLOOR) of tests/ens_train_f64_ref.py (imported as it stands).  Its column-weighted reference (the last two columns Bernoulli,
# both weight arrays) with the last column logistic: the float64 and the float32 evaluation are tests/logistic_head_ref.py's.
# -----------------------------------------------------------------------------------------------------------------------
F64_CASES = [(2, 37, 512, 32, "MSPE", 65, 3), (2, 20, 512, 11, "NLL", 63, 3), (2, 70, 512, 5, "MSPE", 63, 1),
             (2, 20, 512, 40, "MSPE", 65, 0), (2, 20, 256, 6, "MSPE", 33, 0), (2, 11, 128, 4, "MSPE", 33, 0)]


@pytest.mark.parametrize("shape", F64_CASES, ids=["%dx%d-%d-%d-%s-b%d" % s[:6] for s in F64_CASES])
def test_first_step_against_float64(hip_lib, shape):
    _need_gpu()
    import ens_train_f64_ref as R
    from cmbpo_amd.pens import PE
    E, I, H, D, loss, batch, paths = shape
    r = R.reference(E, I, H, D, loss, batch=batch, weighted=True, paths=paths)
    kinds = _kinds(D, (-1,))
    r.r64 = ref.LogisticTrainer(r.ws, r.bs, loss, r.decays, lr=r.lr, kinds=kinds, col_weight=r.cw, pos_weight=r.pw)
    r.r32 = ref.LogisticTrainer32(r.ws, r.bs, loss, r.decays, lr=r.lr, kinds=kinds, col_weight=r.cw, pos_weight=r.pw)
    for t_ in (r.r64, r.r32):
        t_.set_scalers(r.sc_in, r.sc_out)
    fig = r.figures()
    pe = PE(I, D, name="T", hidden_dims=(H, H), num_networks=E, num_elites=max(1, E - 2), loss=loss, use_scaler_in=True,
            use_scaler_out=True, device="cuda:0", lr=r.lr, decay=r.decay, col_weight=r.cw, pos_weight=r.pw, logistic_columns=[-1])
    pe.set_weights(r.ws, r.bs, r.sc_in, r.sc_out)
    tr = pe._ensure_trainer(batch)
    assert tr.f16_paths == paths and not tr.fused
    hold, boot = R.gpu_losses(r, tr)
    R.gpu_step(r, tr)
    errs = dict(zip(R.TENSORS, R.tensor_errors(R.gradient_of_first_step(tr), fig["g64"])))
    e_hold, e_boot = R.loss_errors(hold, fig["hold64"]), R.loss_errors(boot, fig["boot64"])
    print({k: "%.3g / e32 %.3g" % (float(errs[k].max()), e) for k, e in zip(R.TENSORS, fig["e32"])},
          "losses %.3g (e32 %.3g), %.3g (e32 %.3g)" % (e_hold.max(), fig["e32_hold"], e_boot.max(), fig["e32_boot"]))
    for name, e32 in zip(R.TENSORS, fig["e32"]):
        assert float(errs[name].max()) <= r.bound(e32), (name, errs[name], e32)
    assert e_hold.max() <= r.bound(fig["e32_hold"]) and e_boot.max() <= r.bound(fig["e32_boot"])
