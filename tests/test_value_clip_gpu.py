"""GPU parity of the clipped / sample-weighted value loss against its restatement tests/value_clip_ref.py.

Tolerances are those of tests/test_ens_train_gpu.py (fp32; sums over the batch in another order than the restatement):
  * gradients (10 x the first Adam moment after step 1): |d| <= 2e-3 |ref| + 5e-5 max|ref| per tensor;
  * per-member losses: rtol 2e-4;
  * k Adam steps: || w_hip - w_ref || <= 3e-2 || w_ref - w_init ||.
A clipped element passes no gradient, so an element that sits on the edge of the clip range would make the comparison a
coin toss.  The first-step cases therefore PLACE old_pred: with a = m0' - t' (m0' the float64 restatement's output) and u a
draw with |u| in [0.1, 0.6] for half of the elements and in [1.5, 3] for the rest, old' = m0' + s u where s is the positive
root of s^2 (1 - kl mean u^2) - 2 kl mean(a u) s - kl mean a^2 = 0, which makes c == s: exactly the elements with |u| > 1
are clipped and none lies within 0.4 c of the edge.  Every (member, slot) has a data row of its own, so old_pred can be
placed per member.  The several-step cases cannot place anything after the first step; their seeds were chosen on the CPU
so that no element comes within 1e-3 c of the edge, and the tests assert that on the restatement before the GPU runs."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import value_clip_ref as vref  # noqa: E402
from oracle import refcpu, reftrain  # noqa: E402

MODES = {"clip": (False, True, 0.1), "weights": (True, False, 0.1), "both": (True, True, 0.02)}   # weights, old_pred, kl


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _weights_and_data(rng, E, I, H, D, n):
    """Initial weights and data as tests/test_ens_train_gpu.py::_make draws them."""
    ws, bs = [], []
    for k, m in ((I, H), (H, H), (H, D)):
        w = rng.standard_normal((E, k, m))
        bad = np.abs(w) > 2.0
        while bad.any():
            w[bad] = rng.standard_normal(int(bad.sum()))
            bad = np.abs(w) > 2.0
        ws.append((w / (2.0 * np.sqrt(k))).astype(np.float32))
        bs.append((0.1 * rng.standard_normal((E, 1, m))).astype(np.float32))
    ws[2] = (ws[2] * 3).astype(np.float32)
    x = (rng.standard_normal((n, I)) * (1 + rng.rand(I)) + rng.standard_normal(I)).astype(np.float32)
    wtrue = rng.standard_normal((I, D)) / np.sqrt(I)
    t = (np.tanh(x @ wtrue) + 0.1 * rng.standard_normal((n, D))).astype(np.float32)
    sc_in = (x.mean(0, keepdims=True), x.var(0, keepdims=True))
    sc_out = (t.mean(0, keepdims=True), t.var(0, keepdims=True))
    return ws, bs, x, t, sc_in, sc_out


def _sample_weights(rng, n):
    w = rng.uniform(0.25, 2.0, n).astype(np.float32)
    w[rng.permutation(n)[:min(5, n // 4)]] = 0.0          # a handful of exact zeros
    return w


def _mixture(rng, shape):
    """|u| in [0.1, 0.6] for half of the elements, in [1.5, 3] for the other half, random sign."""
    n = int(np.prod(shape))
    mag = rng.uniform(0.1, 0.6, n)
    big = rng.permutation(n)[:n // 2]
    mag[big] = rng.uniform(1.5, 3.0, big.size)
    return (mag * rng.choice([-1.0, 1.0], n)).reshape(shape)


def _root(a, u, kl):
    """s > 0 with kl mean (a + s u)^2 == s^2."""
    A, Bq, Cq = 1.0 - kl * np.mean(u * u), -2.0 * kl * np.mean(a * u), -kl * np.mean(a * a)
    assert A > 0
    return (-Bq + np.sqrt(Bq * Bq - 4.0 * A * Cq)) / (2.0 * A)


def _sigma_mu(sc_out):
    return np.maximum(np.sqrt(sc_out[1].astype(np.float64)), 1e-2).reshape(-1), sc_out[0].astype(np.float64).reshape(-1)


def _make_pe(E, I, H, D, ws, bs, sc_in, sc_out, lr=1e-3, decay=1e-3, **kw):
    from cmbpo_amd.pens import PE
    pe = PE(I, D, name="T", hidden_dims=(H, H), num_networks=E, num_elites=max(1, E - 2), loss="MSE", use_scaler_in=True,
            use_scaler_out=True, device="cuda:0", lr=lr, decay=decay, **kw)
    pe.set_weights(ws, bs, sc_in, sc_out)
    return pe


FIRST_STEP_CASES = [  # E, I, H, D, batch
    (3, 29, 128, 1, 77),      # fused
    (3, 45, 128, 2, 100),     # fused, two outputs
    (2, 5, 128, 1, 1),        # a single row
    (2, 100, 128, 2, 40),     # general fp32
    (3, 29, 256, 1, 100),     # width 256
    (2, 20, 512, 1, 64),      # f16 chain
]


@functools.lru_cache(maxsize=None)
def _first_step_case(E, I, H, D, batch):
    """Data, the placed old predictions for both clip ranges, and the restatement's gradients / losses of the three modes:
    computed once per case on the CPU, read by the three tests of the case."""
    rng = np.random.RandomState(1000 * E + I + H)
    N = E * batch
    ws, bs, x, t, sc_in, sc_out = _weights_and_data(rng, E, I, H, D, N)
    idx = rng.permutation(N).reshape(E, batch).astype(np.int32)      # a data row of its own for every (member, slot)
    w = _sample_weights(rng, N)
    decays = (1e-3 / 4.0, 1e-3 / 2.0, 1e-3)
    r64 = vref.ValueTrainer(ws, bs, decays, dtype=torch.float64)
    r64.set_scalers(sc_in, sc_out)
    ref = vref.ValueTrainer(ws, bs, decays)
    ref.set_scalers(sc_in, sc_out)
    m0 = r64.outputs(x[idx]).numpy()
    a = m0 - r64.scaled(t[idx]).numpy()
    u = _mixture(rng, a.shape)
    sig, mu = _sigma_mu(sc_out)
    case = dict(ws=ws, bs=bs, x=x, t=t, sc_in=sc_in, sc_out=sc_out, idx=idx, w=w, ref=ref, hold=rng.permutation(N)[:min(157, N)])
    _, case["g_plain"] = ref.grads(x[idx], t[idx])
    for mode, (use_w, use_old, kl) in MODES.items():
        old = None
        if use_old:
            s = _root(a, u, kl)
            old = np.zeros((N, D), np.float32)
            old[idx] = ((m0 + s * u) * sig + mu).astype(np.float32)
            case["state_" + mode] = ref.clip_state(x[idx], t[idx], old[idx], kl)
        case["old_" + mode] = old
        _, case["g_" + mode] = ref.grads(x[idx], t[idx], w[idx] if use_w else None, None if old is None else old[idx], kl)
    return case


def _close(got, ref, rtol, arel, msg):
    print("%s: max |d| = %.3g, max |ref| = %.3g" % (msg, float(np.max(np.abs(got - ref))), float(np.max(np.abs(ref)))))
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=arel * float(np.max(np.abs(ref))) + 1e-12, err_msg=msg)


def _differs(a, b, rtol, arel):
    return bool(np.any(np.abs(a - b) > rtol * np.abs(b) + arel * float(np.max(np.abs(b)))))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("E,I,H,D,batch", FIRST_STEP_CASES)
def test_first_step_gradients_and_losses(hip_lib, E, I, H, D, batch, mode):
    _need_gpu()
    c = _first_step_case(E, I, H, D, batch)
    use_w, use_old, kl = MODES[mode]
    x, t, idx, ref, old = c["x"], c["t"], c["idx"], c["ref"], c["old_" + mode]
    gs = c["g_" + mode]
    n = 3
    # conditions on the inputs, checked on the restatement before the GPU is touched
    if use_old:
        clip_c, share, margin = c["state_" + mode]
        print("c = %.4g, clipped share = %.3f, smallest margin = %.3f c" % (clip_c, share, margin))
        assert 0.25 <= share <= 0.75
        assert margin > 0.1
        for l in range(2 * n):
            assert _differs(gs[l].numpy(), c["g_plain"][l].numpy(), 2e-3, 5e-5), "tensor %d: clipping changes nothing" % l

    pe = _make_pe(E, I, H, D, c["ws"], c["bs"], c["sc_in"], c["sc_out"], clip_loss=True, weighted=True)
    tr = pe._ensure_trainer(batch)
    xd, td, idx_d = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(idx).cuda()
    wd = torch.from_numpy(c["w"]).cuda() if use_w else None
    od = torch.from_numpy(old).cuda() if use_old else None
    if use_w:
        # weighted `self.loss` before the step: a shared holdout set, then per-member rows
        hold = c["hold"].astype(np.int32)
        got_l = tr.losses(xd, td, torch.from_numpy(hold).cuda(), 0, hold.shape[0], weights=wd).cpu().numpy()
        tile = lambda a: np.tile(a[hold][None], (E,) + (1,) * a[hold].ndim)
        np.testing.assert_allclose(got_l, ref.losses(tile(x), tile(t), tile(c["w"])), rtol=2e-4)
        got_lb = tr.losses(xd, td, idx_d, batch, batch, weights=wd).cpu().numpy()
        np.testing.assert_allclose(got_lb, ref.losses(x[idx], t[idx], c["w"][idx]), rtol=2e-4)
    tr.step(xd, td, idx_d.data_ptr(), batch, batch, weights=wd, old_pred=od, kl_cliprange=kl)
    mw, mb = tr.get_moments(0)
    for l in range(n):
        _close(10.0 * mw[l], gs[l].numpy(), 2e-3, 5e-5, f"dW{l}")
        _close(10.0 * mb[l], gs[n + l].numpy().reshape(mb[l].shape), 2e-3, 5e-5, f"db{l}")
    vw, _ = tr.get_moments(1)
    _close(1000.0 * vw[1], gs[1].numpy() ** 2, 5e-3, 1e-6, "v1")
    assert tr.steps_done == 1


# ---- several steps -----------------------------------------------------------------------------------------------------------
STEP_SEEDS = {(3, 29, 128, 1, 77): 0, (3, 29, 256, 1, 100): 8}      # chosen on the CPU: see _steps_case


@functools.lru_cache(maxsize=None)
def _steps_case(E, I, H, D, batch, seed, steps=6, kl=0.1):
    """Six clipped, weighted Adam steps of the restatement (one of them ragged).  old_pred sits around the members' mean
    initial prediction, s u away from it (s as in the first-step cases, from the whole data set), so that both sides of the
    clip hold elements while the members move.  Returns the smallest boundary margin and the clipped shares seen."""
    rng = np.random.RandomState(7919 * seed + E + H)
    N = 500
    ws, bs, x, t, sc_in, sc_out = _weights_and_data(rng, E, I, H, D, N)
    decays = (1e-3 / 4.0, 1e-3 / 2.0, 1e-3)
    ref = vref.ValueTrainer(ws, bs, decays)
    ref.set_scalers(sc_in, sc_out)
    r64 = vref.ValueTrainer(ws, bs, decays, dtype=torch.float64)
    r64.set_scalers(sc_in, sc_out)
    mbar = r64.outputs(np.tile(x[None], (E, 1, 1))).numpy().mean(0)
    a = mbar - r64.scaled(t).numpy().reshape(N, D)
    u = _mixture(rng, a.shape)
    sig, mu = _sigma_mu(sc_out)
    old = ((mbar + _root(a, u, kl) * u) * sig + mu).astype(np.float32)
    w = _sample_weights(rng, N)
    idxs, margins, shares = [], [], []
    for k in range(steps):
        b = batch if k != 3 else batch - 9
        idx = rng.randint(0, N, size=(E, b)).astype(np.int32)
        _, share, margin = ref.clip_state(x[idx], t[idx], old[idx], kl)
        ref.step(x[idx], t[idx], w[idx], old[idx], kl)
        idxs.append(idx), margins.append(margin), shares.append(share)
    return dict(ws=ws, bs=bs, x=x, t=t, sc_in=sc_in, sc_out=sc_out, old=old, w=w, idxs=idxs, ref=ref, kl=kl,
                margin=min(margins), shares=shares)


@pytest.mark.parametrize("E,I,H,D,batch", list(STEP_SEEDS))
def test_several_adam_steps_track_the_restatement(hip_lib, E, I, H, D, batch):
    _need_gpu()
    c = _steps_case(E, I, H, D, batch, STEP_SEEDS[(E, I, H, D, batch)])
    print("smallest margin %.3g c, clipped shares %s" % (c["margin"], np.round(c["shares"], 3)))
    assert c["margin"] > 1e-3                                  # no element near the edge of the clip range in any step
    assert all(0.1 < s < 0.9 for s in c["shares"])
    pe = _make_pe(E, I, H, D, c["ws"], c["bs"], c["sc_in"], c["sc_out"], clip_loss=True, weighted=True)
    tr = pe._ensure_trainer(batch)
    xd, td = torch.from_numpy(c["x"]).cuda(), torch.from_numpy(c["t"]).cuda()
    wd, od = torch.from_numpy(c["w"]).cuda(), torch.from_numpy(c["old"]).cuda()
    for idx in c["idxs"]:
        idx_d = torch.from_numpy(idx).cuda()
        tr.step(xd, td, idx_d.data_ptr(), idx.shape[1], idx.shape[1], weights=wd, old_pred=od, kl_cliprange=c["kl"])
    gw, gb = tr.get_weights()
    ref = c["ref"]
    for l in range(3):
        rw = ref.ws[l].numpy()
        moved = float(np.linalg.norm(rw - c["ws"][l]))
        print("layer %d: |w - ref| = %.3g, moved %.3g" % (l, float(np.linalg.norm(gw[l] - rw)), moved))
        assert float(np.linalg.norm(gw[l] - rw)) <= 3e-2 * moved, (l, moved)
        rb = ref.bs[l].numpy().reshape(gb[l].shape)
        assert float(np.linalg.norm(gb[l] - rb)) <= 3e-2 * float(np.linalg.norm(rb - c["bs"][l].reshape(rb.shape))) + 1e-7


# ---- bitwise -----------------------------------------------------------------------------------------------------------------
def _state(tr):
    return [a for k in (tr.get_weights(), tr.get_moments(0), tr.get_moments(1)) for part in k for a in part]


@pytest.mark.parametrize("E,I,H,D,batch", [(3, 29, 128, 1, 77), (3, 29, 256, 1, 100), (2, 20, 512, 1, 64)])
def test_null_block_and_unit_weights_are_the_plain_step_bitwise(hip_lib, E, I, H, D, batch):
    _need_gpu()
    from cmbpo_amd import _lib
    c = _first_step_case(E, I, H, D, batch)
    x, t = c["x"], c["t"]
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    ones = torch.ones(x.shape[0], dtype=torch.float32, device="cuda")
    rng = np.random.RandomState(5)
    idxs = [torch.from_numpy(rng.randint(0, x.shape[0], size=(E, batch)).astype(np.int32)).cuda() for _ in range(3)]
    states = []
    for how in ("plain", "null", "empty", "ones"):
        pe = _make_pe(E, I, H, D, c["ws"], c["bs"], c["sc_in"], c["sc_out"], weighted=True)
        tr = pe._ensure_trainer(batch)
        for idx in idxs:
            if how == "plain":
                tr.step(xd, td, idx.data_ptr(), batch, batch)
            elif how == "ones":
                tr.step(xd, td, idx.data_ptr(), batch, batch, weights=ones)
            else:
                ex = None if how == "null" else C.byref(_lib.TrainExtrasStruct(None, None, 0.1))
                _lib.check(hip_lib.cmbpo_trainer_step_ex(tr._h, xd.data_ptr(), I, td.data_ptr(), D, idx.data_ptr(), batch, batch,
                                                         ex, _lib.current_stream()), "cmbpo_trainer_step_ex")
        assert tr.steps_done == 3
        states.append(_state(tr))
    for other in states[1:]:
        for a, b in zip(states[0], other):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("E,I,H,D,batch", [(3, 45, 128, 2, 100), (2, 100, 128, 2, 40), (2, 20, 512, 1, 64)])
def test_clipped_weighted_step_is_bitwise_reproducible(hip_lib, E, I, H, D, batch):
    _need_gpu()
    c = _first_step_case(E, I, H, D, batch)
    xd, td = torch.from_numpy(c["x"]).cuda(), torch.from_numpy(c["t"]).cuda()
    wd, od, idx_d = torch.from_numpy(c["w"]).cuda(), torch.from_numpy(c["old_both"]).cuda(), torch.from_numpy(c["idx"]).cuda()
    states = []
    for rep in range(2):
        pe = _make_pe(E, I, H, D, c["ws"], c["bs"], c["sc_in"], c["sc_out"], clip_loss=True, weighted=True)
        tr = pe._ensure_trainer(batch)
        for k in range(3):
            tr.step(xd, td, idx_d.data_ptr(), batch, batch, weights=wd, old_pred=od, kl_cliprange=0.02)
        states.append(_state(tr))
    for a, b in zip(*states):
        np.testing.assert_array_equal(a, b)
    assert any(float(np.abs(a).max()) > 0 for a in states[0][6:12])          # (the moments are not all zero)


# ---- host layers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True])
def test_pe_train_with_old_pred_and_weights(hip_lib, on_device):
    _need_gpu()
    E, I, H, D, N = 3, 9, 128, 1, 400
    rng = np.random.RandomState(11)
    ws, bs, x, t, sc_in, sc_out = _weights_and_data(rng, E, I, H, D, N)
    w = _sample_weights(rng, N)
    old = (t + 0.3 * rng.standard_normal(t.shape)).astype(np.float32)
    pe = _make_pe(E, I, H, D, ws, bs, sc_in, sc_out, clip_loss=True, weighted=True, kl_cliprange=0.05)
    dev = (lambda a: torch.from_numpy(a).cuda()) if on_device else (lambda a: a)
    # [N] and [N, D] are both accepted
    out = pe.train(dev(x), dev(t), batch_size=64, max_epochs=2, holdout_ratio=0.25, rng=np.random.RandomState(3),
                   old_pred=dev(old[:, 0]), weights=dev(w[:, None] if on_device else w))
    n_train = N - int(N * 0.25)
    assert pe.train_epochs == 2 and pe.train_grad_updates == 2 * int(np.ceil(n_train / 64)) == pe._trainer.steps_done
    hold = np.random.RandomState(3).permutation(N)[:int(N * 0.25)]
    gw, gb = pe.get_weights()
    ref = vref.ValueTrainer(gw, gb, pe.decays)
    ref.set_scalers((pe.scaler_in.cached_mu, pe.scaler_in.cached_var), (pe.scaler_out.cached_mu, pe.scaler_out.cached_var))
    tile = lambda a: np.tile(a[hold][None], (E,) + (1,) * a[hold].ndim)
    want = ref.losses(tile(x), tile(t), tile(w))
    np.testing.assert_allclose(out["T/val_loss"], np.sort(want)[:pe.num_elites].mean(), rtol=2e-4)
    assert not np.allclose(want, ref.losses(tile(x), tile(t)), rtol=1e-2)      # (the weights matter on this holdout set)
    assert any(float(np.abs(a - b).max()) > 0 for a, b in zip(gw, ws))


def test_refusals(hip_lib):
    """A model built without the flags keeps refusing the arrays; a clip_loss model needs old_pred; the C-ABI refuses a
    probabilistic head before any device work."""
    _need_gpu()
    from cmbpo_amd import _lib
    from cmbpo_amd.pens import PE
    E, I, H, D, N = 2, 5, 128, 1, 64
    rng = np.random.RandomState(2)
    ws, bs, x, t, sc_in, sc_out = _weights_and_data(rng, E, I, H, D, N)
    kw = dict(batch_size=32, max_epochs=1)
    plain = _make_pe(E, I, H, D, ws, bs, sc_in, sc_out)
    with pytest.raises(NotImplementedError):
        plain.train(x, t, weights=np.ones(N), **kw)
    with pytest.raises(NotImplementedError):
        plain.train(x, t, old_pred=t, **kw)
    only_w = _make_pe(E, I, H, D, ws, bs, sc_in, sc_out, weighted=True)
    with pytest.raises(NotImplementedError):
        only_w.train(x, t, weights=np.ones(N), old_pred=t, **kw)
    clip = _make_pe(E, I, H, D, ws, bs, sc_in, sc_out, clip_loss=True)
    with pytest.raises(ValueError, match="old_pred"):
        clip.train(x, t, **kw)
    with pytest.raises(NotImplementedError):
        clip.train(x, t, old_pred=t, weights=np.ones(N), **kw)
    with pytest.raises(ValueError, match="kl_cliprange"):
        clip.train(x, t, old_pred=t, kl_cliprange=-1.0, **kw)
    with pytest.raises(ValueError):
        clip.train(x, t, old_pred=t[:-1], **kw)
    assert plain._trainer is None or plain._trainer.steps_done == 0
    # C-ABI: 'MSPE' and 'NLL' handles
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(np.tile(t, (1, 2))).cuda()
    wd = torch.ones(N, device="cuda")
    for loss, words in (("MSPE", b"MSPE"), ("NLL", b"probabilistic"), ("NLL", b"deterministic")):
        pe = PE(I, 2, name="P", hidden_dims=(H, H), num_networks=E, num_elites=1, loss=loss, device="cuda:0")
        pe.init_weights(rng)
        tr = pe._ensure_trainer(32)
        ex = _lib.TrainExtrasStruct(wd.data_ptr(), None if words == b"deterministic" else yd.data_ptr(), 0.1)
        for name, call in (
                ("cmbpo_trainer_step_ex", lambda: hip_lib.cmbpo_trainer_step_ex(tr._h, xd.data_ptr(), I, yd.data_ptr(), 2, None, 0, 32,
                                                                                C.byref(ex), None)),
                ("cmbpo_trainer_epoch_ex", lambda: hip_lib.cmbpo_trainer_epoch_ex(tr._h, xd.data_ptr(), I, yd.data_ptr(), 2, None, 64, 64,
                                                                                  32, C.byref(ex), None)),
                ("cmbpo_trainer_losses_ex", lambda: hip_lib.cmbpo_trainer_losses_ex(tr._h, xd.data_ptr(), I, yd.data_ptr(), 2, None, 0, 32,
                                                                                    None, C.byref(ex), None))):
            assert call() == -1
            msg = hip_lib.cmbpo_last_error()
            if name == "cmbpo_trainer_losses_ex" and words == b"probabilistic":
                words_ = b"deterministic"           # `self.loss` never reads old_pred: the weights are what is refused
            else:
                words_ = words
            assert name.encode() in msg and words_ in msg, msg
        assert tr.steps_done == 0


class _ClipOps:
    """The numerics behind reftrain.train_loop for one critic under vf_clipping."""

    def __init__(self, ref, x, t, old, kl):
        self.ref, self.x, self.t, self.old, self.kl = ref, x, t, old, kl
        self.sc_in, self.sc_out = reftrain.RunningScaler(x.shape[1]), reftrain.RunningScaler(1)

    def fit_scalers(self, rows):
        self.sc_in.fit(self.x[rows])
        self.sc_out.fit(self.t[rows])
        f = lambda s: (s.mu.astype(np.float32), s.var.astype(np.float32))
        self.ref.set_scalers(f(self.sc_in), f(self.sc_out))

    def train_step(self, rows):
        self.ref.step(self.x[rows], self.t[rows], None, None if self.old is None else self.old[rows], self.kl)

    def holdout_losses(self, rows):
        E = self.ref.ws[0].shape[0]
        return self.ref.losses(np.tile(self.x[rows][None], (E, 1, 1)), np.tile(self.t[rows][None], (E, 1, 1)))


def test_update_critic_with_vf_clipping(hip_lib):
    """CPOPolicy(vf_clipping=True).update_critic: both critics train on the buffer's v / vc columns as old_pred, each with
    its own clip range, exactly as the restated loop does (same numpy RandomState on both sides)."""
    _need_gpu()
    from cmbpo_amd.cpo_policy import CPOPolicy

    class _Space:
        def __init__(self, d):
            self.shape = (d,)

    Dm, A, n = 12, 3, 600
    kw = dict(a_hidden_layer_sizes=(128, 128), vf_hidden_layer_sizes=(128, 128), vf_ensemble_size=3, vf_elites=2,
              vf_activation="swish", vf_loss="MSE", device="cuda:0", vf_lr=3e-4, vf_epochs=2, vf_batch_size=256, max_path_length=10)
    with pytest.raises(NotImplementedError):
        CPOPolicy(_Space(Dm), _Space(A), vf_clipping=True, **dict(kw, vf_loss="NLL"))
    pol = CPOPolicy(_Space(Dm), _Space(A), vf_clipping=True, vf_cliprange=0.1, cvf_cliprange=0.03, **kw)
    assert pol.v.clip_loss and pol.vc.clip_loss and (pol.v.kl_cliprange, pol.vc.kl_cliprange) == (0.1, 0.03)
    rng = np.random.RandomState(3)
    wv, bv = pol.v.init_weights(rng)
    wc, bc = pol.vc.init_weights(rng)
    obs = rng.standard_normal((n, Dm)).astype(np.float32)
    ret = (np.sin(obs[:, 0]) + 0.5 * obs[:, 1] + 3.0).astype(np.float32)
    cret = (np.abs(obs[:, 2]) * 2.0).astype(np.float32)
    old_v = (ret + 0.6 * rng.standard_normal(n)).astype(np.float32)
    old_vc = (cret + 0.6 * rng.standard_normal(n)).astype(np.float32)
    z = np.zeros(n, np.float32)
    buf = [obs, np.zeros((n, A), np.float32), z, z, ret, cret, z, old_v, old_vc, z, np.zeros((n, A), np.float32),
           np.zeros((n, A), np.float32)]
    out = pol.update_critic(buf, rng=np.random.RandomState(17))
    assert np.isfinite(out["post"]["LossVEnsemble"]) and np.isfinite(out["post"]["LossVCEnsemble"])
    steps = 2 * int(np.ceil((n - int(n * 0.1)) / 256))
    assert pol.v.train_grad_updates == steps == pol.vc.train_grad_updates
    # the restated loop, clipped and (to show that the comparison can tell) unclipped: v first, then vc, on one stream of
    # draws as update_critic makes them (the draws do not depend on the numerics: no early stop within two epochs)
    tk = dict(batch_size=256, max_epochs=2, min_epoch_before_break=2, holdout_ratio=0.1)
    f = lambda s: (s.mu.astype(np.float32), s.var.astype(np.float32))
    preds = {}
    for clipped in (True, False):
        loop_rng = np.random.RandomState(17)
        for name, pe, ws, bs, tgt, old, kl in (("v", pol.v, wv, bv, ret, old_v, 0.1), ("vc", pol.vc, wc, bc, cret, old_vc, 0.03)):
            ref = vref.ValueTrainer(ws, bs, pe.decays, lr=3e-4)
            ops = _ClipOps(ref, obs, tgt[:, None], old[:, None] if clipped else None, kl)
            reftrain.train_loop(ops, n, 3, 2, loop_rng, **tk)
            preds[name, clipped] = refcpu.ens_predict_mean(obs[:200], [p.numpy() for p in ref.ws], [p.numpy() for p in ref.bs],
                                                           f(ops.sc_in), f(ops.sc_out))[:, 0]
    for name, get in (("v", pol.get_v), ("vc", pol.get_vc)):
        got = get(obs[:200])
        print("%s: max |got - restated| = %.3g, max |clipped - unclipped restated| = %.3g"
              % (name, float(np.abs(got - preds[name, True]).max()), float(np.abs(preds[name, True] - preds[name, False]).max())))
        assert not np.allclose(preds[name, False], preds[name, True], rtol=2e-4, atol=2e-4)
        np.testing.assert_allclose(got, preds[name, True], rtol=2e-4, atol=2e-4)


def test_cmbpo_runs_epochs_with_vf_clipping(hip_lib):
    _need_gpu()
    import toyworld
    from cmbpo_amd import synthetic
    from cmbpo_amd.cmbpo import CMBPO
    from cmbpo_amd.cpo_policy import CPOPolicy
    from cmbpo_amd.cpo_sampler import CpoSampler
    from cmbpo_amd.cpobuffer import CPOBuffer
    np.random.seed(0)
    env = toyworld.ToyEnv()
    D, A, T = env.D, env.A, 40
    policy = CPOPolicy(env.observation_space, env.action_space, a_hidden_layer_sizes=(128, 128),
                       vf_hidden_layer_sizes=(128, 128), vf_ensemble_size=3, vf_elites=2, vf_activation="swish",
                       vf_loss="MSE", vf_lr=1e-3, vf_epochs=2, vf_batch_size=256, device="cuda:0", max_path_length=T,
                       cost_lim=5.0, target_kl=0.01, vf_clipping=True)
    policy.set_params(synthetic.policy_params(np.random.default_rng(2), D, A, 128))
    rng = np.random.RandomState(1)
    policy.v.init_weights(rng)
    policy.vc.init_weights(rng)
    v0, vc0 = [w.copy() for w in policy.v.get_weights()[0]], [w.copy() for w in policy.vc.get_weights()[0]]
    buf = CPOBuffer(600, 6000, env.observation_space, env.action_space)
    algo = CMBPO(env, policy, buf, sampler=CpoSampler(max_path_length=T), task="default", n_env_interacts=10 ** 9,
                 eval_every_n_steps=1, m_train_freq=100, m_networks=4, m_elites=3, m_hidden_dims=(128, 128),
                 rollout_batch_size=400, rollout_mode="schedule", rollout_schedule=[0, 1, 4, 4], maxroll=6,
                 initial_real_samples_per_epoch=150, min_real_samples_per_epoch=100, batch_size_policy=2500,
                 n_initial_exploration_steps=300, n_epochs=50,
                 initial_model_train_kwargs=dict(min_epochs=3, max_epochs=6, batch_size=128),
                 model_train_kwargs=dict(min_epochs=1, max_epochs=2, batch_size=128))
    seen = []
    train = policy.v.train
    policy.v.train = lambda *a, **k: seen.append(k.get("old_pred")) or train(*a, **k)
    diags = []
    for d in algo.train():
        diags.append(d)
        if len(diags) >= 2:
            break
    assert len(diags) == 2
    assert seen and all(o is not None and o.shape[1] == 1 for o in seen)      # the buffer's value column reached the critic
    for d in diags:
        for k in ("LossVEnsemble", "LossVCEnsemble"):
            assert k in d and np.isfinite(d[k]), (k, d.get(k))
    assert policy.v.train_grad_updates > 0
    assert any(float(np.abs(a - b).max()) > 0 for a, b in zip(policy.v.get_weights()[0], v0))
    assert any(float(np.abs(a - b).max()) > 0 for a, b in zip(policy.vc.get_weights()[0], vc0))
