"""CPU: the logistic termination head without a GPU -- the float64 reference against autograd, against
oracle/reftrain.py and tests/column_weights_ref.py with all-zero kinds, the Bernoulli term and sigma - y at extreme logits, the
label rule on NaN targets and around 0.5, the repeated-rows identity of an integer class weight, the threshold conversion, the
scaler pin, the refusals of the C-ABI that need no trainer (the two that need one, a deterministic head and a wrong target_dim,
are in tests/test_logistic_head_gpu.py), every new ValueError / NotImplementedError of `PE`, `FakeEnv` and `CMBPO`, and the
round trip of the file `CMBPO.save` writes."""
import ctypes as C
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import column_weights_ref as cw_ref  # noqa: E402
import logistic_head_ref as ref  # noqa: E402
from oracle import reftrain  # noqa: E402

F64 = torch.float64
WHO = b"cmbpo_trainer_set_column_kinds"


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
    kinds = np.zeros(D, np.uint8)
    kinds[D - binary:] = 1
    sc_in = (x.reshape(-1, I).mean(0, keepdims=True), x.reshape(-1, I).var(0, keepdims=True))
    sc_out = (t.reshape(-1, D).mean(0, keepdims=True), t.reshape(-1, D).var(0, keepdims=True))
    return ws, bs, x, t, cw, pw, kinds, sc_in, sc_out


# ------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("loss", ["MSPE", "NLL"])
def test_closed_form_deltas_equal_autograd(loss, weighted):
    ws, bs, x, t, cw, pw, kinds, sc_in, sc_out = _problem(1)
    tr = ref.LogisticTrainer(ws, bs, loss, (0.0, 0.0, 0.0), kinds=kinds, col_weight=cw if weighted else None,
                             pos_weight=pw if weighted else None)
    tr.set_scalers(sc_in, sc_out)
    o, ts, w, y, km = tr._forward(tr.ws, tr.bs, x, t)
    o = o.detach().requires_grad_(True)
    total = {"MSPE": ref.mspe_losses, "NLL": ref.nll_losses}[loss](o, ts, w, y, km).sum()
    (g,) = torch.autograd.grad(total, o)
    d = ref.output_deltas(o.detach(), ts, w, y, km, loss)
    np.testing.assert_allclose(d.numpy(), g.numpy(), rtol=1e-10, atol=1e-10 * float(g.abs().max()))
    D = t.shape[-1]
    # the log-variance output of a logistic column: no data term ('NLL': nothing at all, 'MSPE': the regulariser alone)
    lv_delta = d[..., D:][..., kinds.astype(bool)]
    if loss == "NLL":
        assert float(lv_delta.abs().max()) == 0.0
    else:
        want = 0.1 * o.detach()[..., D:][..., kinds.astype(bool)] / (t.shape[1] * D)
        np.testing.assert_allclose(lv_delta.numpy(), want.numpy(), rtol=1e-14)
    # the output scaler does not touch a logistic column: other moments there, the same deltas
    mu, var = sc_out[0].copy(), sc_out[1].copy()
    mu[:, kinds.astype(bool)] += 3.0
    var[:, kinds.astype(bool)] *= 7.0
    tr.set_scalers(sc_in, (mu, var))
    _, ts2, _, _, _ = tr._forward(tr.ws, tr.bs, x, t)
    np.testing.assert_array_equal(ref.output_deltas(o.detach(), ts2, w, y, km, loss).numpy(), d.numpy())


@pytest.mark.parametrize("loss", ["MSPE", "NLL"])
def test_all_zero_kinds_are_reftrain_and_column_weights_ref(loss):
    ws, bs, x, t, cw, pw, _, sc_in, sc_out = _problem(2)
    D = t.shape[-1]
    decays = (1e-3, 2e-3, 4e-3)
    pairs = [(ref.LogisticTrainer(ws, bs, loss, decays, kinds=np.zeros(D, np.uint8)),
              reftrain.EnsembleTrainer(ws, bs, loss_type=loss, decays=decays, dtype=F64)),
             (ref.LogisticTrainer(ws, bs, loss, decays, kinds=None, col_weight=cw, pos_weight=pw),
              cw_ref.WeightedTrainer(ws, bs, loss, decays, col_weight=cw, pos_weight=pw))]
    for a, b in pairs:
        for tr in (a, b):
            tr.set_scalers(sc_in, sc_out)
        la, ga = a.grads(x, t)
        lb, gb = b.grads(x, t)
        assert la == lb
        for p, q in zip(ga, gb):
            np.testing.assert_array_equal(p.numpy(), q.numpy())
        np.testing.assert_array_equal(a.losses(x, t), b.losses(x, t))


def test_bernoulli_term_and_its_gradient_at_extreme_logits():
    zs = np.array([0.0, 1e-8, -1e-8, 20.0, -20.0, 100.0, -100.0, 1e4, -1e4])
    for y in (0.0, 1.0):
        z = torch.tensor(zs, dtype=F64)
        l = ref.bernoulli_nll(z, torch.full_like(z, y)).numpy()
        g = (ref.sigmoid(z) - y).numpy()
        assert np.all(np.isfinite(l)) and np.all(np.isfinite(g))
        # l = softplus(z) for y = 0 and softplus(-z) for y = 1 (no cancellation), in extended precision on the host
        zl = zs.astype(np.longdouble)
        a = -zl if y else zl
        with np.errstate(over="ignore"):
            want_l = np.where(a > 0, a + np.log1p(np.exp(-np.abs(a))), np.log1p(np.exp(-np.abs(a))))
        ea = np.exp(-np.abs(zl))
        # sigma(z) for y = 0, -(1 - sigma(z)) = -sigma(-z) for y = 1
        want_g = -np.where(zl > 0, ea / (1 + ea), 1 / (1 + ea)) if y else np.where(zl > 0, 1 / (1 + ea), ea / (1 + ea))
        np.testing.assert_allclose(l, want_l.astype(np.float64), rtol=1e-14, atol=1e-300)
        # sigma - y in float64 cancels where sigma is within an ulp of y: the absolute error is an ulp of 1
        np.testing.assert_allclose(g, want_g.astype(np.float64), rtol=1e-14, atol=2.3e-16)
    assert float(ref.bernoulli_nll(torch.tensor(0.0, dtype=F64), torch.tensor(0.0, dtype=F64))) == pytest.approx(np.log(2.0), abs=1e-16)
    assert float(ref.bernoulli_nll(torch.tensor(1e4, dtype=F64), torch.tensor(0.0, dtype=F64))) == 1e4
    assert float(ref.bernoulli_nll(torch.tensor(-1e4, dtype=F64), torch.tensor(1.0, dtype=F64))) == 1e4
    # the package's pair agrees
    from cmbpo_amd.utils import logit, sigmoid
    np.testing.assert_allclose(sigmoid(zs), ref.sigmoid(torch.tensor(zs, dtype=F64)).numpy(), rtol=1e-15, atol=0)
    for p in (0.1, 0.5, 0.9, 1e-9):
        assert sigmoid(logit(p)) == pytest.approx(p, rel=1e-12)


def test_the_label_rule_on_nan_targets_and_around_one_half():
    half = np.float32(0.5)
    up, dn = np.nextafter(half, np.float32(1)), np.nextafter(half, np.float32(0))
    t = np.array([[[np.nan, half, dn, up, 1.0, 0.0, -3.0, np.inf, -np.inf]]], np.float32)
    np.testing.assert_array_equal(ref.labels(t).numpy()[0, 0], [0, 0, 0, 1, 1, 0, 0, 1, 0])
    # float64 input just above one half that rounds to it in float32 is NOT positive: the kernels see float32 targets
    assert float(ref.labels(np.array([[[0.5 + 1e-9]]]))) == 0.0


def test_integer_pos_weight_is_the_batch_with_its_positive_rows_repeated():
    """D = 2 'NLL' with one logistic column (no coupling between rows, members or columns): class weight k on the positives of
    that column = those rows k times in the batch, up to the divisor B' / B, in every gradient that the column feeds.  The
    Gaussian column's own rows are repeated too, so its part is compared on the logistic column's output weights alone."""
    ws, bs, x, t, _, _, _, _, _ = _problem(3, E=2, B=23, D=2, binary=1)
    k = 3
    kinds = np.array([0, 1], np.uint8)
    cw = np.array([0.0, 1.0], np.float32)          # the Gaussian column is silent: only the logistic column's term remains
    a = ref.LogisticTrainer(ws, bs, "NLL", (0.0, 0.0, 0.0), kinds=kinds, col_weight=cw, pos_weight=np.array([1.0, k], np.float32))
    b = ref.LogisticTrainer(ws, bs, "NLL", (0.0, 0.0, 0.0), kinds=kinds, col_weight=cw)
    pos = t[0, :, 1] > 0.5
    t[1] = t[0]
    x[1] = x[0]
    assert 0 < pos.sum() < pos.size
    rep = np.concatenate([np.arange(pos.size)] + [np.nonzero(pos)[0]] * (k - 1))
    _, ga = a.grads(x, t)
    _, gb = b.grads(x[:, rep], t[:, rep])
    scale = rep.size / pos.size
    assert float(ga[-1].abs().max()) > 0
    for p, q in zip(ga, gb):
        np.testing.assert_allclose(p.numpy(), scale * q.numpy(), rtol=1e-10, atol=1e-12)


def test_threshold_conversion():
    from cmbpo_amd.utils import logit, logit_threshold
    z = logit_threshold(0.5)
    assert z == 0.0 and np.float32(z).view(np.uint32) == 0            # exactly +0.0f
    assert logit_threshold(0.1) == float(np.float32(np.log(0.1 / 0.9)))
    assert logit_threshold(0.9) == float(np.float32(np.log(0.9 / 0.1)))
    assert logit_threshold(0.1) == -logit_threshold(0.9) or abs(logit_threshold(0.1) + logit_threshold(0.9)) < 1e-6
    for bad in (0.0, 1.0, float("nan"), 1.5, -0.2):
        with pytest.raises(ValueError, match="strictly inside"):
            logit_threshold(bad)
        with pytest.raises(ValueError):
            logit(bad)


# ------------------------------------------------------------------------------------------------------------------
# the C-ABI: refusals by name, before any HIP call (host arrays, no trainer, no device)
# ------------------------------------------------------------------------------------------------------------------
def _kinds(*v):
    return (C.c_ubyte * len(v))(*v)


def test_signature_and_export(lib):
    from cmbpo_amd import _lib
    assert hasattr(C.CDLL(_lib.LIB_PATH), "cmbpo_trainer_set_column_kinds")
    assert _lib.SIGNATURES["cmbpo_trainer_set_column_kinds"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p])
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "cmbpo_hip.h")).read()
    assert "int cmbpo_trainer_set_column_kinds(cmbpo_trainer_t *t, const unsigned char *h_kind, int target_dim, void *stream);" in header


def test_refusals_by_name(lib):
    for k, d, word in ((_kinds(0, 1), 2, b"handle is NULL"),
                       (None, 0, b"handle is NULL"),                    # detaching needs a trainer too
                       (_kinds(0, 0), 2, b"handle is NULL"),
                       (_kinds(0, 2), 2, b"kind[1] = 2"),
                       (_kinds(255, 0, 0), 3, b"kind[0] = 255"),
                       (_kinds(1, 1), 2, b"every column is logistic"),
                       (_kinds(1), 1, b"every column is logistic"),
                       (_kinds(1), 0, b"target_dim 0")):
        assert lib.cmbpo_trainer_set_column_kinds(None, None if k is None else C.cast(k, C.c_void_p), d, None) == -1
        msg = lib.cmbpo_last_error()
        assert WHO in msg and word in msg, msg


# ------------------------------------------------------------------------------------------------------------------
# PE, FakeEnv and CMBPO: every new refusal, before anything is created on a device
# ------------------------------------------------------------------------------------------------------------------
def _pe(**kw):
    from cmbpo_amd.pens import PE
    return PE(6, 3, hidden_dims=(128, 128), num_networks=2, num_elites=1, device="cpu", **kw)


def test_pe_refusals_and_the_kind_array():
    from cmbpo_amd.pens import column_kind_array
    for cols in ([3], [-4], [0.5], [0, 1, 2], [-1, -2, -3], [True]):
        for loss in ("MSPE", "NLL"):
            with pytest.raises(ValueError, match="logistic_columns"):
                _pe(loss=loss, logistic_columns=cols)
    with pytest.raises(NotImplementedError, match="'MSE'"):
        _pe(loss="MSE", logistic_columns=[-1])
    np.testing.assert_array_equal(column_kind_array([-1], 3), [0, 0, 1])
    np.testing.assert_array_equal(column_kind_array([0, -2], 3), [1, 1, 0])
    np.testing.assert_array_equal(column_kind_array(-1, 3), [0, 0, 1])
    assert column_kind_array(None, 3) is None and column_kind_array((), 3) is None and column_kind_array([], 3) is None
    assert column_kind_array([-1], 3).dtype == np.uint8


def test_the_scaler_pin():
    """mu = 0, var = 1 in the logistic columns after a fit and whenever a scaler comes in; the other columns keep theirs."""
    from cmbpo_amd.pens import PE, _CachedScaler
    pe = PE.__new__(PE)
    pe.loss_type, pe._out_dim, pe._trainer, pe.finalized = "MSPE", 3, None, False
    pe.scaler_out = _CachedScaler(3)
    pe.set_logistic_columns([-1])
    assert pe.logistic_columns == (2,)
    rng = np.random.RandomState(0)
    data = rng.standard_normal((50, 3)) * 3 + 2
    data[:, 2] = rng.rand(50) < 0.2
    pe.scaler_out.fit(data)
    assert pe.scaler_out.cached_mu[0, 2] != 0.0
    assert pe._pin_logistic_scaler()
    plain = _CachedScaler(3)
    plain.fit(data)
    np.testing.assert_array_equal(pe.scaler_out.cached_mu[0, :2], plain.cached_mu[0, :2])
    np.testing.assert_array_equal(pe.scaler_out.cached_var[0, :2], plain.cached_var[0, :2])
    assert pe.scaler_out.cached_mu[0, 2] == 0.0 and pe.scaler_out.cached_var[0, 2] == 1.0
    assert pe.scaler_out.cached_mu.dtype == np.float32 and pe.scaler_out.cached_mu.shape == (1, 3)
    # detached: nothing is pinned; no output scaler: nothing to pin
    pe.set_logistic_columns(None)
    pe.scaler_out.fit(data)
    assert not pe._pin_logistic_scaler() and pe.scaler_out.cached_mu[0, 2] != 0.0
    pe.set_logistic_columns([2])
    pe.scaler_out = None
    assert not pe._pin_logistic_scaler()


def test_set_weights_pins_an_incoming_scaler(monkeypatch):
    from cmbpo_amd.pens import PE, _CachedScaler
    pe = PE.__new__(PE)
    pe.loss_type, pe._out_dim, pe._trainer, pe.finalized = "NLL", 3, None, False
    pe.use_scaler_in, pe.use_scaler_out, pe.scaler_in, pe.scaler_out = False, True, None, _CachedScaler(3)
    pe.set_logistic_columns([1])
    seen = {}

    class Mlp:
        def load(self, weights, biases, in_scaler=None, out_scaler=None):
            seen["out"] = out_scaler
    pe.mlp = Mlp()
    pe.set_weights([], [], None, (np.array([[1.0, 2.0, 3.0]]), np.array([[4.0, 5.0, 6.0]])))
    np.testing.assert_array_equal(seen["out"][0], np.array([[1.0, 0.0, 3.0]], np.float32))
    np.testing.assert_array_equal(seen["out"][1], np.array([[4.0, 1.0, 6.0]], np.float32))
    np.testing.assert_array_equal(pe.scaler_out.cached_mu, seen["out"][0])


def _fake_env(**kw):
    """A FakeEnv up to its checks: a model stub, no device."""
    from toyworld import ToyEnv
    from cmbpo_amd.fake_env import FakeEnv
    env = ToyEnv()
    obs, act = int(np.prod(env.observation_space.shape)), int(np.prod(env.action_space.shape))

    class Model:
        is_ensemble = is_probabilistic = True
        in_dim, out_dim, device = obs + act, obs + 2, "cpu"
    return FakeEnv(env, "default", Model(), True, True, False, predicts_term=True, **kw)


def test_fake_env_refusals_and_descriptor():
    fe = _fake_env(term_threshold=0.1, term_loss="logistic")
    assert fe.term_threshold == 0.1 and fe.term_loss == "logistic"
    th = fe.term_head_struct()
    assert th.threshold == float(np.float32(np.log(0.1 / 0.9)))
    assert _fake_env(term_threshold=0.5, term_loss="logistic").term_head_struct().threshold == 0.0
    g = _fake_env(term_threshold=1.5)                     # a Gaussian head takes any finite threshold, as before
    assert g.term_head_struct().threshold == 1.5 and g.term_loss == "gaussian" and g.term_kernel_threshold == 1.5
    for bad in (0.0, 1.0, 1.5, -0.1):
        with pytest.raises(ValueError, match="strictly inside"):
            _fake_env(term_threshold=bad, term_loss="logistic")
        with pytest.raises(ValueError, match="strictly inside"):
            fe.set_term_head(bad, "elite")
    with pytest.raises(ValueError, match="finite"):
        _fake_env(term_threshold=float("nan"), term_loss="logistic")
    with pytest.raises(ValueError, match="term_loss"):
        _fake_env(term_loss="probit")
    with pytest.raises(ValueError, match="term_loss"):
        fe.set_term_head(0.5, "elite", loss="probit")
    assert (fe.term_threshold, fe.term_members, fe.term_loss) == (0.1, "elite", "logistic")     # a refusal changes nothing
    fe.set_term_head(1.5, "any", loss="gaussian")
    assert fe.term_head_struct().threshold == 1.5
    fe.set_term_head(0.9, "majority", loss="logistic")
    assert fe.term_head_struct().threshold == float(np.float32(np.log(9.0)))
    # without the column there is no head to be logistic
    from toyworld import ToyEnv
    from cmbpo_amd.fake_env import FakeEnv
    env = ToyEnv()
    n = int(np.prod(env.observation_space.shape))

    class Model:
        is_ensemble = is_probabilistic = True
        in_dim, out_dim, device = n + int(np.prod(env.action_space.shape)), n + 1, "cpu"
    with pytest.raises(ValueError, match="predicts_term"):
        FakeEnv(env, "default", Model(), True, True, False, term_loss="logistic")


def test_cmbpo_refusals():
    from cmbpo_amd.cmbpo import _term_loss_args
    assert _term_loss_args(True, "logistic", 0.5) == "logistic"
    assert _term_loss_args(False, "gaussian", 7.0) == "gaussian" and _term_loss_args(True, "gaussian", 7.0) == "gaussian"
    with pytest.raises(ValueError, match="m_learn_term"):
        _term_loss_args(False, "logistic", 0.5)
    with pytest.raises(ValueError, match="m_term_loss"):
        _term_loss_args(True, "sigmoid", 0.5)
    for bad in (0.0, 1.0, 2.0, float("nan")):
        with pytest.raises(ValueError, match="m_term_threshold"):
            _term_loss_args(True, "logistic", bad)


def test_save_load_round_trip_of_the_term_loss_file(tmp_path):
    """`save` writes term_loss_<epoch>.json beside term_head_<epoch>.json, whose keys stay; `load` sets the model's kinds BEFORE
    its weights and scalers come in; a missing file means 'gaussian'."""
    from cmbpo_amd.cmbpo import CMBPO
    calls = []

    class Model:
        def save(self, d, e):
            calls.append(("save", e))

        def load(self, d, e):
            calls.append(("load", e))

        def set_logistic_columns(self, cols):
            calls.append(("kinds", cols))

        def set_column_weights(self, *a):
            pass

    class Env:
        term_threshold, term_members, term_loss = 0.3, "any", "logistic"

        def set_term_head(self, threshold, members, loss=None):
            calls.append(("head", threshold, members, loss))

    a = CMBPO.__new__(CMBPO)
    a._use_model, a._m_learn_term, a._m_learn_cost, a._epoch = True, True, False, 4
    a._model, a.fake_env, a._m_term_loss = Model(), Env(), "logistic"
    a._column_weights = {"m_term_pos_weight": 1.0, "m_term_loss_weight": 1.0, "m_cost_loss_weight": 1.0, "m_pos_weight_max": 20.0}
    a.save(str(tmp_path))
    assert json.load(open(tmp_path / "term_head_4.json")) == {"threshold": 0.3, "members": "any"}
    assert json.load(open(tmp_path / "term_loss_4.json")) == {"m_term_loss": "logistic"}
    b = CMBPO.__new__(CMBPO)
    b._use_model, b._m_learn_term, b._m_learn_cost = True, True, False
    b._model, b.fake_env, b._m_term_loss = Model(), Env(), "gaussian"
    b._column_weights = dict(a._column_weights)
    del calls[:]
    b.load(str(tmp_path), 4)
    assert b._m_term_loss == "logistic"
    assert calls == [("kinds", [-1]), ("load", 4), ("head", 0.3, "any", "logistic")]
    os.remove(tmp_path / "term_loss_4.json")
    del calls[:]
    b.load(str(tmp_path), 4)
    assert b._m_term_loss == "gaussian"
    assert calls == [("kinds", None), ("load", 4), ("head", 0.3, "any", "gaussian")]
