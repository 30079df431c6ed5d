"""GPU: column- and class-weighted training steps of the probabilistic heads against tests/column_weights_ref.py
(float64 torch on oracle/reftrain.py's forward).

Tolerances are those of tests/test_ens_train_gpu.py, the arithmetic being the same (fp32 / two-piece f16 products, sums over the
batch in another order than the reference):
  * gradients (read back as 10 x the first Adam moment after step 1): |d| <= 2e-3 |ref| + 5e-5 max|ref| per tensor;
  * per-member losses: rtol 2e-4;
  * k Adam steps: || w_hip - w_ref || <= 3e-2 || w_ref - w_init ||.
All-ones weights against the plain step are compared bit for bit, for 'MSPE' too: col_stats_kernel keeps the summation order of
the forward whose statistics it rewrites.

The fixed-point test's bound (0.05) is 2.5 times the worst distance of the float32 reference loop's members from the level
(0.019 weighted, 0.012 unweighted, three seeds, both losses)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import column_weights_ref as ref  # noqa: E402


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# E, I, H, D, loss, batch, f16 paths (bit 0 the f16 backward chain, bit 1 the f16 training forward: test_f16_path_selection's rule)
SHAPES = [
    (3, 11, 128, 4, "MSPE", 100, 0),
    (2, 37, 512, 32, "MSPE", 97, 3),     # AntSafe with both heads: 64 raw outputs, one full f16 item and a ragged one
    (2, 37, 512, 32, "NLL", 97, 3),
    (2, 20, 512, 40, "MSPE", 70, 0),     # 80 raw outputs: fp32 chain and forward of a 512-wide ensemble
    (2, 70, 512, 5, "MSPE", 40, 1),      # 72 padded inputs: the f16 chain behind the fp32 forward
    (4, 20, 256, 6, "MSPE", 33, 0),
    (3, 11, 128, 4, "NLL", 1, 0),        # a single row
]
_ID = lambda s: "%dx%d-%d-%d-%s-b%d" % s[:6]
MODES = ("both", "col", "pos")


def _weights(D, mode, rng):
    cw = rng.uniform(0.5, 4.0, D).astype(np.float32)
    cw[1] = 0.0                              # one observation column carries no data term at all
    pw = np.ones(D, np.float32)
    pw[-2:] = (7.0, 3.0)
    return (cw if mode in ("both", "col") else None), (pw if mode in ("both", "pos") else None)


_DATA = {}


def _data(E, I, D, n, seed):
    """Inputs, targets (the last two columns Bernoulli, rates 0.1 and 0.3, dependent on x) and their scalers: computed once per
    shape and shared, never written."""
    key = (E, I, D, n, seed)
    if key not in _DATA:
        rng = np.random.RandomState(seed)
        x = (rng.standard_normal((n, I)) * (1 + rng.rand(I)) + rng.standard_normal(I)).astype(np.float32)
        wtrue = rng.standard_normal((I, D)) / np.sqrt(I)
        t = (np.tanh(x @ wtrue) + 0.1 * rng.standard_normal((n, D))).astype(np.float32)
        for col, rate in ((D - 2, 0.1), (D - 1, 0.3)):
            z = x @ wtrue[:, col] + rng.standard_normal(n)
            t[:, col] = (z > np.quantile(z, 1.0 - rate)).astype(np.float32)
        sc_in = (x.mean(0, keepdims=True), x.var(0, keepdims=True))
        sc_out = (t.mean(0, keepdims=True), t.var(0, keepdims=True))
        for a in (x, t):
            a.setflags(write=False)
        _DATA[key] = (x, t, sc_in, sc_out)
    return _DATA[key]


def _make(E, I, H, D, loss, n, seed, mode="both", lr=1e-3, decay=1e-3):
    from cmbpo_amd.pens import PE
    x, t, sc_in, sc_out = _data(E, I, D, n, seed)
    rng = np.random.RandomState(seed + 1)
    cw, pw = _weights(D, mode, rng) if mode else (None, None)
    pe = PE(I, D, name="T", hidden_dims=(H, H), num_networks=E, num_elites=max(1, E - 2), loss=loss, use_scaler_in=True,
            use_scaler_out=True, device="cuda:0", lr=lr, decay=decay, col_weight=cw, pos_weight=pw)
    ws, bs = pe.init_weights(rng)
    bs = [(0.1 * rng.standard_normal(b.shape)).astype(np.float32) for b in bs]
    ws[2] = (ws[2] * 3).astype(np.float32)
    pe.set_weights(ws, bs, sc_in, sc_out)
    rt = ref.WeightedTrainer(ws, bs, loss, pe.decays, lr=lr, col_weight=cw, pos_weight=pw)
    rt.set_scalers(sc_in, sc_out)
    return rng, pe, rt, x, t, ws, bs


def _close(got, want, rtol, arel, msg):
    np.testing.assert_allclose(got, want, rtol=rtol, atol=arel * float(np.max(np.abs(want))) + 1e-12, err_msg=msg)


def _dev(a):
    return torch.tensor(np.asarray(a)).cuda()      # (a copy: the shared arrays are read-only)


CASES = [(s, "both") for s in SHAPES] + [(s, m) for s in SHAPES[:3] for m in ("col", "pos")]


@pytest.mark.parametrize("shape,mode", CASES, ids=[_ID(s) + "-" + m for s, m in CASES])
def test_first_step_gradients_and_losses(hip_lib, shape, mode):
    _need_gpu()
    E, I, H, D, loss, batch, bits = shape
    rng, pe, rt, x, t, ws, bs = _make(E, I, H, D, loss, max(300, 2 * batch), seed=E * 1000 + I + D, mode=mode)
    tr = pe._ensure_trainer(batch)
    assert tr.f16_paths == bits
    idx = rng.randint(0, x.shape[0], size=(E, batch)).astype(np.int32)
    xd, td, idx_d = _dev(x), _dev(t), _dev(idx)
    # `self.loss` with the weights attached: a shared holdout list (idx_stride 0), then per-member lists
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
    if mode in ("both", "col"):
        # the column of weight 0: every output delta of its mean head is exactly 0, so is their column sum
        assert float(np.abs(mb[2][:, 0, 1]).max()) == 0.0
        assert float(np.abs(gs[5].numpy().reshape(mb[2].shape)[:, 0, 1]).max()) == 0.0
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


BITWISE = [SHAPES[0], SHAPES[1], SHAPES[2], SHAPES[3], SHAPES[4]]


@pytest.mark.parametrize("shape", BITWISE, ids=[_ID(s) for s in BITWISE])
def test_a_weighted_step_is_bitwise_reproducible(hip_lib, shape):
    """No atomics on the gradient path, the weighted statistics included."""
    _need_gpu()
    E, I, H, D, loss, batch, _ = shape
    outs = []
    for _ in range(2):
        _, pe, _, x, t, _, _ = _make(E, I, H, D, loss, 300, seed=99)
        outs.append(_steps(pe, x, t, E, batch, 2, seed=5))
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("shape", BITWISE, ids=[_ID(s) for s in BITWISE])
def test_detached_and_all_ones_weights_are_the_plain_step(hip_lib, shape):
    """Attach, detach, step == a trainer that never had weights; all-ones weights (either array alone, or both) == the plain
    step, bit for bit: w == 1 changes no product, and the weighted statistics keep the forward's summation order."""
    _need_gpu()
    E, I, H, D, loss, batch, _ = shape
    one = np.ones(D, np.float32)

    def run(before):
        _, pe, _, x, t, _, _ = _make(E, I, H, D, loss, 300, seed=17, mode=None)
        return _steps(pe, x, t, E, batch, 2, seed=6, before=before)

    plain = run(None)

    def attach_detach(pe):
        pe.set_column_weights({1: 0.0, -1: 2.5}, {-1: 7.0})
        pe.set_column_weights(None, None)

    for before in (attach_detach, lambda pe: pe.set_column_weights(one, one), lambda pe: pe.set_column_weights(one, None),
                   lambda pe: pe.set_column_weights(None, one)):
        for a, b in zip(plain, run(before)):
            np.testing.assert_array_equal(a, b)
    # ... and the weights do change the step (the comparison above is not vacuous)
    changed = run(lambda pe: pe.set_column_weights(None, {-1: 7.0}))
    assert any(not np.array_equal(a, b) for a, b in zip(plain, changed))


TRACK = [SHAPES[0], SHAPES[1], SHAPES[2], SHAPES[5]]


@pytest.mark.parametrize("shape", TRACK, ids=[_ID(s) for s in TRACK])
def test_three_adam_steps_track_the_reference(hip_lib, shape):
    _need_gpu()
    E, I, H, D, loss, batch, _ = shape
    rng, pe, rt, x, t, ws, bs = _make(E, I, H, D, loss, 300, seed=7 + E)
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


def test_refusals_that_need_a_trainer(hip_lib):
    """A deterministic head (pointed to cmbpo_trainer_step_ex) and a wrong target_dim; the *_ex entries go on refusing a
    probabilistic head with column weights attached; a new, larger trainer gets the weights again."""
    _need_gpu()
    from cmbpo_amd import _lib
    from cmbpo_amd.pens import PE
    two = (C.c_float * 2)(1.0, 2.0)
    det = PE(5, 2, hidden_dims=(128, 128), num_networks=2, num_elites=1, loss="MSE", device="cuda:0")
    det.init_weights(np.random.RandomState(0))
    h = det._ensure_trainer(32)._h
    assert hip_lib.cmbpo_trainer_set_column_weights(h, C.cast(two, C.c_void_p), None, 2, None) == -1
    msg = hip_lib.cmbpo_last_error()
    assert b"cmbpo_trainer_set_column_weights" in msg and b"deterministic" in msg and b"cmbpo_trainer_step_ex" in msg
    assert hip_lib.cmbpo_trainer_set_column_weights(h, None, None, 0, None) == 0        # detaching nothing is no error

    _, pe, _, x, t, _, _ = _make(3, 11, 128, 4, "MSPE", 300, seed=3)
    tr = pe._ensure_trainer(32)
    assert hip_lib.cmbpo_trainer_set_column_weights(tr._h, C.cast(two, C.c_void_p), None, 2, None) == -1
    assert b"target_dim 2 != 4" in hip_lib.cmbpo_last_error()
    xd, td = _dev(x), _dev(t)
    idx = _dev(np.zeros((3, 32), np.int32))
    with pytest.raises(_lib.CmbpoHipError, match="MSPE"):
        tr.step(xd, td, idx.data_ptr(), 32, 32, weights=torch.ones(300, device="cuda"))
    with pytest.raises(_lib.CmbpoHipError, match="MSPE"):
        tr.losses(xd, td, idx, 32, 32, weights=torch.ones(300, device="cuda"))
    # a larger batch builds a new trainer: the weights move over with the Adam state
    before = tr.losses(xd, td, idx, 32, 32).cpu().numpy()
    tr2 = pe._ensure_trainer(64)
    assert tr2 is not tr
    np.testing.assert_array_equal(tr2.losses(xd, td, idx, 32, 32).cpu().numpy(), before)
    pe.set_column_weights(None, None)
    assert not np.array_equal(tr2.losses(xd, td, idx, 32, 32).cpu().numpy(), before)


@pytest.mark.parametrize("loss", ["MSPE", "NLL"])
def test_pos_weight_moves_the_level(hip_lib, loss):
    """A Bernoulli(0.2) column independent of x under class weight 4 settles at q = pos_weight_level(p, 4) (about 0.5), not at
    p; the same run without the weight settles at p.  Every member, within 0.05 (module docstring)."""
    _need_gpu()
    from cmbpo_amd.pens import PE
    from cmbpo_amd.utils import pos_weight_level
    rng = np.random.RandomState(11)
    n = 2048
    x = rng.standard_normal((n, 6)).astype(np.float32)
    W = rng.standard_normal((6, 2)) / np.sqrt(6)
    t = np.empty((n, 3), np.float32)
    t[:, :2] = np.tanh(x @ W) + 0.1 * rng.standard_normal((n, 2))
    t[:, 2] = rng.rand(n) < 0.2
    p_hat = float(t[:, 2].mean())
    q = pos_weight_level(p_hat, 4.0)
    assert 0.47 < q < 0.53
    fresh = rng.standard_normal((4000, 6)).astype(np.float32)
    for pos_weight, level in (({-1: 4.0}, q), (None, p_hat)):
        pe = PE(6, 3, name="T", hidden_dims=(128, 128), num_networks=3, num_elites=2, loss=loss, use_scaler_in=True,
                use_scaler_out=True, device="cuda:0", lr=1e-3, pos_weight=pos_weight)
        pe.init_weights(np.random.RandomState(12))
        pe.train(x, t, batch_size=256, max_epochs=40, holdout_ratio=0.0, rng=np.random.RandomState(13))
        mean, _ = pe.predict_ensemble(fresh)
        got = mean[:, :, 2].mean(axis=1)
        print("loss %s pos_weight %r: level %.4f, members %s" % (loss, pos_weight, level, np.round(got, 4)))
        assert np.all(np.abs(got - level) <= 0.05), (loss, pos_weight, level, got)
