"""CPU: the C-ABI of the clipped / sample-weighted value loss (cmbpo_train_extras_t, cmbpo_trainer_*_ex) is
exported and versioned, refuses what it can judge without a handle before any HIP call, the Python layer refuses the
out-of-scope models before it touches a device, and the restatement the GPU tests are judged by (tests/value_clip_ref.py)
agrees with its closed form.  (The refusals that depend on the handle's head -- a probabilistic head, the 'MSPE' loss --
need a handle, and a handle needs a device: tests/test_value_clip_gpu.py::test_refusals.)"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import value_clip_ref as vref  # noqa: E402
from oracle import reftrain  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cmbpo_amd import _lib
    return _lib.lib()


def test_symbols_and_version(lib):
    from cmbpo_amd import _lib
    assert lib.cmbpo_version() >= 3
    for name in ("cmbpo_trainer_step_ex", "cmbpo_trainer_epoch_ex", "cmbpo_trainer_losses_ex"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    ex = _lib.TrainExtrasStruct()
    assert ex.d_weights is None and ex.d_old_pred is None and ex.kl_cliprange == 0.0
    assert [f[0] for f in _lib.TrainExtrasStruct._fields_] == ["d_weights", "d_old_pred", "kl_cliprange"]
    assert C.sizeof(_lib.TrainExtrasStruct) == 24


def _calls(lib, t, ex):
    """The three new entries on handle t (NULL: every call fails a check first); ex: a TrainExtrasStruct or None."""
    e = None if ex is None else C.byref(ex)
    return {
        "cmbpo_trainer_step_ex": lambda: lib.cmbpo_trainer_step_ex(t, None, 3, None, 1, None, 0, 4, e, None),
        "cmbpo_trainer_epoch_ex": lambda: lib.cmbpo_trainer_epoch_ex(t, None, 3, None, 1, None, 8, 8, 4, e, None),
        "cmbpo_trainer_losses_ex": lambda: lib.cmbpo_trainer_losses_ex(t, None, 3, None, 1, None, 0, 4, None, e, None),
    }


def test_bad_clip_range_is_refused_without_a_gpu(lib):
    from cmbpo_amd import _lib
    host = (C.c_float * 16)()                       # never dereferenced
    p = C.cast(host, C.c_void_p).value
    for kl in (-1e-3, -1.0, float("nan"), float("inf"), -float("inf")):
        for with_w in (False, True):
            ex = _lib.TrainExtrasStruct(p if with_w else None, p, kl)
            calls = _calls(lib, None, ex)
            for name in ("cmbpo_trainer_step_ex", "cmbpo_trainer_epoch_ex"):
                assert calls[name]() == -1
                msg = lib.cmbpo_last_error()
                assert name.encode() in msg and b"kl_cliprange" in msg, msg
    # `self.loss` is never clipped: the range is not read there, the NULL handle is what fails
    ex = _lib.TrainExtrasStruct(p, p, -1.0)
    assert _calls(lib, None, ex)["cmbpo_trainer_losses_ex"]() == -1
    assert b"cmbpo_trainer_losses_ex: NULL argument" in lib.cmbpo_last_error()


def test_null_handle_and_forwarding_without_a_gpu(lib):
    from cmbpo_amd import _lib
    host = (C.c_float * 16)()
    p = C.cast(host, C.c_void_p).value
    # a block that asks for something: the entry's own checks, its own name
    for ex in (_lib.TrainExtrasStruct(p, None, 0.1), _lib.TrainExtrasStruct(None, p, 0.1), _lib.TrainExtrasStruct(p, p, 0.0)):
        for name, call in _calls(lib, None, ex).items():
            if name == "cmbpo_trainer_losses_ex" and ex.d_weights is None:
                continue                            # (forwards: old_pred alone asks nothing of `self.loss`)
            assert call() == -1
            assert (name + ": NULL argument").encode() in lib.cmbpo_last_error(), lib.cmbpo_last_error()
    # a NULL block, or one with both pointers NULL, is the existing entry: its checks, its name
    for ex in (None, _lib.TrainExtrasStruct(None, None, -5.0)):
        for name, call in _calls(lib, None, ex).items():
            assert call() == -1
            assert (name[:-3] + ": NULL argument").encode() in lib.cmbpo_last_error(), lib.cmbpo_last_error()
    ex = _lib.TrainExtrasStruct(None, p, 0.1)
    assert _calls(lib, None, ex)["cmbpo_trainer_losses_ex"]() == -1
    assert b"cmbpo_trainer_losses: NULL argument" in lib.cmbpo_last_error()


def test_python_layer_refuses_out_of_scope_models_before_any_device_call(lib):
    """clip_loss / weighted on a probabilistic loss, a bad range: raised by the constructor before it creates a handle."""
    from cmbpo_amd.pens import PE, build_PE
    for loss in ("MSPE", "NLL"):
        for kw in (dict(clip_loss=True), dict(weighted=True), dict(clip_loss=True, weighted=True)):
            with pytest.raises(NotImplementedError, match="MSE"):
                PE(5, 2, loss=loss, hidden_dims=(128, 128), device="cuda:0", **kw)
        with pytest.raises(NotImplementedError, match="MSE"):
            build_PE(5, 2, loss=loss, hidden_dims=(128, 128), clip_loss=True, device="cuda:0")
    for kl in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="kl_cliprange"):
            PE(5, 1, loss="MSE", hidden_dims=(128, 128), clip_loss=True, kl_cliprange=kl, device="cuda:0")
    with pytest.raises(NotImplementedError):        # unchanged
        build_PE(5, 1, loss="MSE", hidden_dims=(128, 128), lr_decay=0.5, device="cuda:0")


# ---- the restatement against its closed form -------------------------------------------------------------------------------
def _problem(seed, E=3, B=23, I=7, H=16, D=2, dtype=torch.float64, scalers=True):
    rng = np.random.RandomState(seed)
    ws = [rng.standard_normal(s) / np.sqrt(s[1]) for s in ((E, I, H), (E, H, H), (E, H, D))]
    bs = [0.1 * rng.standard_normal((E, 1, s)) for s in (H, H, D)]
    x = rng.standard_normal((E, B, I))
    t = rng.standard_normal((E, B, D)) * 2.0 + 1.0
    tr = vref.ValueTrainer(ws, bs, decays=(1e-3, 2e-3, 4e-3), dtype=dtype)
    if scalers:
        tr.set_scalers((x.mean((0, 1)), x.var((0, 1))), (t.mean((0, 1)), t.var((0, 1))))
    w = rng.uniform(0.25, 2.0, (E, B))
    w[0, :3] = 0.0
    old = t + rng.standard_normal((E, B, D)) * 1.5
    return rng, tr, x, t, w, old


@pytest.mark.parametrize("scalers", [True, False])
@pytest.mark.parametrize("mode", ["clip", "weights", "both"])
def test_autograd_gradient_is_the_closed_form_delta(mode, scalers):
    rng, tr, x, t, w, old = _problem(3, scalers=scalers)
    w_, old_, kl = (None if mode == "clip" else w), (None if mode == "weights" else old), 0.1
    o = tr.outputs(x).clone().requires_grad_(True)
    ts = tr.scaled(t)
    os_ = None if old_ is None else tr.scaled(old_)
    loss = vref.value_losses(o, ts, tr._t(w_), os_, kl).sum()
    got, = torch.autograd.grad(loss, o)
    want = vref.closed_form_delta(o.detach(), ts, tr._t(w_), os_, kl)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-13, atol=1e-16)
    if old_ is not None:
        c, share, margin = tr.clip_state(x, t, old_, kl)
        assert 0.1 < share < 0.9 and margin > 0, (share, margin)      # both branches carry elements
        assert float((got == 0).double().mean()) >= share             # the clipped elements, and the zero weights, pass nothing
    if w_ is not None:
        assert float(got[0, :3].abs().max()) == 0.0


def test_infinite_range_is_the_plain_mse_gradient():
    rng, tr, x, t, w, old = _problem(5)
    ref = reftrain.EnsembleTrainer([p.numpy() for p in tr.ws], [p.numpy() for p in tr.bs], loss_type="MSE",
                                   decays=tr.decays, dtype=torch.float64)
    ref.scaler_in, ref.scaler_out = tr.scaler_in, tr.scaler_out
    l0, g0 = ref.grads(x, t)
    for kl in (1e6, 1e12):
        c, share, _ = tr.clip_state(x, t, old, kl)
        assert share == 0.0
        l1, g1 = tr.grads(x, t, old=old, kl=kl)
        assert abs(l1 - l0) <= 1e-12 * abs(l0)
        for a, b in zip(g0, g1):       # m_c = old' + (m - old') rounds once more than m: float64 rounding, relative to c
            np.testing.assert_allclose(b.numpy(), a.numpy(), rtol=1e-9, atol=1e-13)
    o = tr.outputs(x)
    np.testing.assert_allclose(vref.value_losses(o, tr.scaled(t)).numpy(), reftrain.mse_losses(o, tr.scaled(t)).numpy(), rtol=0, atol=0)


def test_unit_weights_change_nothing():
    rng, tr, x, t, w, old = _problem(7)
    ones = np.ones_like(w)
    for old_ in (None, old):
        la, ga = tr.grads(x, t, old=old_, kl=0.1)
        lb, gb = tr.grads(x, t, w=ones, old=old_, kl=0.1)
        assert la == lb
        for a, b in zip(ga, gb):
            np.testing.assert_array_equal(a.numpy(), b.numpy())
    np.testing.assert_array_equal(tr.losses(x, t), tr.losses(x, t, ones))
    # the mean divides by the batch, not by the sum of the weights
    np.testing.assert_allclose(tr.losses(x, t, 3.0 * ones), 3.0 * tr.losses(x, t), rtol=1e-14)


def test_zero_old_var_gives_zero_range_and_no_nan():
    rng, tr, x, t, w, old = _problem(9)
    c, share, _ = tr.clip_state(x, t, t, 0.1)            # old_pred == targets: old_var == 0
    assert c == 0.0 and share == 1.0
    loss, gs = tr.grads(x, t, old=t, kl=0.1)
    assert np.isfinite(loss)
    decay_only = [d * p for d, p in zip(tr.decays, tr.ws)]
    for g, d in zip(gs[:3], decay_only):
        np.testing.assert_allclose(g.numpy(), d.numpy(), rtol=1e-14, atol=0)      # the rows with m != old' contribute nothing
    for g in gs[3:]:
        assert float(g.abs().max()) == 0.0
