"""CPU: column- and class-weighted losses of the probabilistic heads without a GPU -- the float64 reference against
autograd and against oracle/reftrain.py, the repeated-rows identity of an integer class weight, the rule on NaN targets and on
targets at, one ulp below and one ulp above 0.5, `utils.pos_weight_level`, the refusals of the C-ABI that need no trainer (the
two that need one, a deterministic head and a wrong target_dim, are in tests/test_column_weights_gpu.py), and every ValueError of
`PE` / `CMBPO`."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import column_weights_ref as ref  # noqa: E402
from oracle import reftrain  # noqa: E402

F64 = torch.float64
WHO = b"cmbpo_trainer_set_column_weights"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cmbpo_amd import _lib
    return _lib.lib()


def _problem(seed, E=3, B=17, I=5, H=8, D=4, binary=2):
    rng = np.random.RandomState(seed)
    ws = [rng.standard_normal(s) * 0.4 for s in ((E, I, H), (E, H, H), (E, H, 2 * D))]
    bs = [rng.standard_normal((E, 1, s)) * 0.1 for s in (H, H, 2 * D)]
    x = rng.standard_normal((E, B, I)).astype(np.float32)
    t = rng.standard_normal((E, B, D)).astype(np.float32)
    t[..., D - binary:] = (rng.rand(E, B, binary) < 0.3).astype(np.float32)
    cw = rng.uniform(0.5, 4.0, D).astype(np.float32)
    cw[0] = 0.0
    pw = np.ones(D, np.float32)
    pw[D - binary:] = (7.0, 3.0)[:binary]
    sc_in = (x.reshape(-1, I).mean(0, keepdims=True), x.reshape(-1, I).var(0, keepdims=True))
    sc_out = (t.reshape(-1, D).mean(0, keepdims=True), t.reshape(-1, D).var(0, keepdims=True))
    return ws, bs, x, t, cw, pw, sc_in, sc_out


# ------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["MSPE", "NLL"])
def test_closed_form_deltas_equal_autograd(loss):
    ws, bs, x, t, cw, pw, sc_in, sc_out = _problem(1)
    tr = ref.WeightedTrainer(ws, bs, loss, (0.0, 0.0, 0.0), col_weight=cw, pos_weight=pw)
    tr.set_scalers(sc_in, sc_out)
    o, ts, w = tr._forward(tr.ws, tr.bs, x, t)
    o = o.detach().requires_grad_(True)
    total = {"MSPE": ref.mspe_losses, "NLL": ref.nll_losses}[loss](o, ts, w).sum()
    (g,) = torch.autograd.grad(total, o)
    d = ref.output_deltas(o.detach(), ts, w, loss)
    np.testing.assert_allclose(d.numpy(), g.numpy(), rtol=1e-10, atol=1e-10 * float(g.abs().max()))
    # a column of weight 0 carries no data gradient: its mean head none at all
    assert float(d[..., 0].abs().max()) == 0.0


@pytest.mark.parametrize("loss", ["MSPE", "NLL"])
def test_all_ones_weights_are_reftrain(loss):
    ws, bs, x, t, _, _, sc_in, sc_out = _problem(2)
    D = t.shape[-1]
    decays = (1e-3, 2e-3, 4e-3)
    a = ref.WeightedTrainer(ws, bs, loss, decays, col_weight=np.ones(D), pos_weight=np.ones(D))
    b = reftrain.EnsembleTrainer(ws, bs, loss_type=loss, decays=decays, dtype=F64)
    for tr in (a, b):
        tr.set_scalers(sc_in, sc_out)
    la, ga = a.grads(x, t)
    lb, gb = b.grads(x, t)
    assert abs(la - lb) <= 1e-10 * abs(lb)
    for p, q in zip(ga, gb):
        np.testing.assert_allclose(p.numpy(), q.numpy(), rtol=1e-10, atol=1e-10 * float(q.abs().max()))
    np.testing.assert_allclose(a.losses(x, t), b.losses(x, t), rtol=1e-12)
    # NULL arrays are all ones
    c = ref.WeightedTrainer(ws, bs, loss, decays)
    c.set_scalers(sc_in, sc_out)
    assert c.grads(x, t)[0] == la


def test_integer_pos_weight_is_the_batch_with_its_positive_rows_repeated():
    """D = 1 'NLL' (no coupling between rows or members): class weight k on the positives = those rows k times in the batch,
    up to the divisor B' / B."""
    ws, bs, x, t, _, _, _, _ = _problem(3, E=2, B=23, D=1, binary=1)
    k = 3
    a = ref.WeightedTrainer(ws, bs, "NLL", (0.0, 0.0, 0.0), pos_weight=np.array([k], np.float32))
    b = reftrain.EnsembleTrainer(ws, bs, loss_type="NLL", decays=(0.0, 0.0, 0.0), dtype=F64)
    pos = t[0, :, 0] > 0.5
    t[1] = t[0]                                     # the same rows for both members, so one repeat list serves both
    x[1] = x[0]
    assert 0 < pos.sum() < pos.size
    rep = np.concatenate([np.arange(pos.size)] + [np.nonzero(pos)[0]] * (k - 1))
    _, ga = a.grads(x, t)
    _, gb = b.grads(x[:, rep], t[:, rep])
    scale = rep.size / pos.size
    for p, q in zip(ga, gb):
        np.testing.assert_allclose(p.numpy(), scale * q.numpy(), rtol=1e-10, atol=1e-12)


def test_pos_weight_level():
    from cmbpo_amd.utils import pos_weight_level
    assert pos_weight_level(0.2, 1.0) == pytest.approx(0.2, abs=1e-15)
    assert pos_weight_level(0.2, 4.0) == pytest.approx(0.8 / 1.6, abs=1e-15)
    assert pos_weight_level(0.1, 9.0) == pytest.approx(0.5, abs=1e-15)
    assert pos_weight_level(0.3, 0.0) == 0.0 and pos_weight_level(0.0, 5.0) == 0.0 and pos_weight_level(1.0, 5.0) == 1.0
    # it is the minimiser of the weighted squared error of a constant
    p, om = 0.27, 6.0
    q = np.linspace(0, 1, 100001)
    assert abs(q[np.argmin(om * p * (q - 1) ** 2 + (1 - p) * q ** 2)] - pos_weight_level(p, om)) < 2e-5
    for bad in ((-0.1, 1.0), (1.1, 1.0), (0.5, -1.0), (float("nan"), 1.0)):
        with pytest.raises(ValueError):
            pos_weight_level(*bad)


def test_the_rule_on_nan_targets_and_around_one_half():
    half = np.float32(0.5)
    up, dn = np.nextafter(half, np.float32(1)), np.nextafter(half, np.float32(0))
    t = np.array([[[np.nan, half, dn, up, 1.0, 0.0, -3.0, np.inf, -np.inf]]], np.float32)
    D = t.shape[-1]
    w = ref.element_weights(t, np.full(D, 2.0), np.full(D, 5.0)).numpy()[0, 0]
    np.testing.assert_array_equal(w, [2.0, 2.0, 2.0, 10.0, 10.0, 2.0, 2.0, 10.0, 2.0])
    # float64 input just above one half that rounds to it in float32 is NOT positive: the kernels see float32 targets
    assert float(ref.element_weights(np.array([[[0.5 + 1e-9]]]), [1.0], [5.0])) == 1.0


# ------------------------------------------------------------------------------------------------------------------
# the C-ABI: refusals by name, before any HIP call (host arrays, no trainer, no device)
# ------------------------------------------------------------------------------------------------------------------
def _arr(*v):
    return (C.c_float * len(v))(*v)


def _set(lib, t, cw, pw, d):
    return lib.cmbpo_trainer_set_column_weights(t, None if cw is None else C.cast(cw, C.c_void_p),
                                                None if pw is None else C.cast(pw, C.c_void_p), d, None)


def test_signature_and_export(lib):
    from cmbpo_amd import _lib
    assert hasattr(C.CDLL(_lib.LIB_PATH), "cmbpo_trainer_set_column_weights")
    assert _lib.SIGNATURES["cmbpo_trainer_set_column_weights"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p])


def test_refusals_by_name(lib):
    for cw, pw, d, word in (
            (_arr(1.0, 1.0), None, 2, b"handle is NULL"),
            (None, _arr(1.0, 2.0), 2, b"handle is NULL"),
            (None, None, 0, b"handle is NULL"),                      # detaching needs a trainer too
            (_arr(1.0, -0.5), None, 2, b"col_weight[1]"),
            (_arr(float("nan"), 1.0), None, 2, b"col_weight[0]"),
            (_arr(1.0, float("inf")), None, 2, b"col_weight[1]"),
            (None, _arr(-1.0, 1.0), 2, b"pos_weight[0]"),
            (_arr(1.0, 1.0), _arr(1.0, float("nan")), 2, b"pos_weight[1]"),
            (_arr(1.0, 1.0), _arr(1.0, float("-inf")), 2, b"pos_weight[1]"),
            (_arr(0.0, 0.0), None, 2, b"no positive entry"),
            (_arr(0.0, 0.0), _arr(3.0, 3.0), 2, b"no positive entry"),
            (_arr(1.0), None, 0, b"target_dim 0")):
        assert _set(lib, None, cw, pw, d) == -1
        msg = lib.cmbpo_last_error()
        assert WHO in msg and word in msg, msg


def test_the_ex_entries_still_refuse_nothing_new(lib):
    """The per-sample block of the deterministic heads is untouched: a NULL trainer is still named by the entry itself."""
    from cmbpo_amd import _lib
    host = (C.c_float * 8)()
    ex = _lib.TrainExtrasStruct(C.cast(host, C.c_void_p), None, 0.1)
    assert lib.cmbpo_trainer_step_ex(None, None, 1, None, 1, None, 0, 1, C.byref(ex), None) == -1
    assert b"cmbpo_trainer_step_ex" in lib.cmbpo_last_error()


# ------------------------------------------------------------------------------------------------------------------
# PE and CMBPO: every ValueError, before anything is created on a device
# ------------------------------------------------------------------------------------------------------------------
def test_pe_refusals():
    from cmbpo_amd.pens import PE, column_weight_array
    for kw in (dict(col_weight=[1.0, 2.0]), dict(pos_weight=np.ones(4)), dict(col_weight=[1.0, -1.0, 1.0]),
               dict(pos_weight=[1.0, np.nan, 1.0]), dict(col_weight=[1.0, np.inf, 1.0]), dict(col_weight={3: 2.0}),
               dict(pos_weight={-4: 2.0}), dict(col_weight={0.5: 2.0}), dict(pos_weight={-1: -2.0}),
               dict(col_weight=[0.0, 0.0, 0.0]), dict(col_weight={0: 0.0, 1: 0.0, 2: 0.0})):
        for loss in ("MSPE", "NLL"):
            with pytest.raises(ValueError):
                PE(6, 3, hidden_dims=(128, 128), num_networks=2, num_elites=1, loss=loss, device="cpu", **kw)
    with pytest.raises(NotImplementedError, match="probabilistic"):
        PE(6, 3, hidden_dims=(128, 128), num_networks=2, num_elites=1, loss="MSE", device="cpu", pos_weight={-1: 2.0})
    np.testing.assert_array_equal(column_weight_array({-1: 4.0, 0: 0.5}, 3, "w"), np.array([0.5, 1.0, 4.0], np.float32))
    np.testing.assert_array_equal(column_weight_array((1, 2, 3), 3, "w"), np.array([1, 2, 3], np.float32))
    assert column_weight_array(None, 3, "w") is None


def test_existing_refusals_still_hold():
    from cmbpo_amd.pens import PE
    with pytest.raises(NotImplementedError, match="MSE"):
        PE(6, 3, hidden_dims=(128, 128), num_networks=2, num_elites=1, loss="MSPE", weighted=True, device="cpu")
    with pytest.raises(NotImplementedError, match="MSE"):
        PE(6, 3, hidden_dims=(128, 128), num_networks=2, num_elites=1, loss="NLL", weighted=True, pos_weight={-1: 2.0}, device="cpu")
    # train(weights=) on a model built without weighted=True: the check of PE.train, which runs before any device work
    pe = PE.__new__(PE)
    pe.loss_type, pe.weighted, pe.clip_loss, pe.kl_cliprange = "MSPE", False, False, 0.1
    with pytest.raises(NotImplementedError, match="weighted=True"):
        pe._check_train_args({"weights": np.ones(4)})


def test_cmbpo_refusals_and_balanced():
    from cmbpo_amd.cmbpo import _column_weight_args, balanced_pos_weight
    ok = _column_weight_args(True, True, "balanced", 2.0, 3.0, 20.0)
    assert ok == {"m_term_pos_weight": "balanced", "m_term_loss_weight": 2.0, "m_cost_loss_weight": 3.0, "m_pos_weight_max": 20.0}
    assert _column_weight_args(False, False, 1.0, 1.0, 1.0, 20.0)["m_term_pos_weight"] == 1.0
    for args, word in (((False, True, 4.0, 1.0, 1.0, 20.0), "m_learn_term"),
                       ((False, True, "balanced", 1.0, 1.0, 20.0), "m_learn_term"),
                       ((False, True, 1.0, 2.0, 1.0, 20.0), "m_learn_term"),
                       ((True, False, 1.0, 1.0, 2.0, 20.0), "m_learn_cost"),
                       ((True, True, -1.0, 1.0, 1.0, 20.0), "m_term_pos_weight"),
                       ((True, True, "auto", 1.0, 1.0, 20.0), "m_term_pos_weight"),
                       ((True, True, float("nan"), 1.0, 1.0, 20.0), "m_term_pos_weight"),
                       ((True, True, 1.0, float("inf"), 1.0, 20.0), "m_term_loss_weight"),
                       ((True, True, 1.0, 1.0, -2.0, 20.0), "m_cost_loss_weight"),
                       ((True, True, 1.0, 1.0, None, 20.0), "m_cost_loss_weight"),
                       ((True, True, "balanced", 1.0, 1.0, 0.5), "m_pos_weight_max"),
                       ((True, True, "balanced", 1.0, 1.0, float("inf")), "m_pos_weight_max")):
        with pytest.raises(ValueError, match=word):
            _column_weight_args(*args)
    t = np.zeros(100)
    t[:10] = 1.0
    assert balanced_pos_weight(t, 20.0) == 9.0
    assert balanced_pos_weight(t, 5.0) == 5.0                       # clipped from above
    assert balanced_pos_weight(np.ones(10), 20.0) == 1.0            # ... and from below
    assert balanced_pos_weight(np.zeros(10), 20.0) == 10.0          # no positive: n_neg / 1
    assert balanced_pos_weight(np.zeros(1000), 20.0) == 20.0
