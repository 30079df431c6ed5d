"""GPU: ModelBuffer.set_trust_weights -- one weight ref_var / (ref_var + accumulated model variance) per sample that get()
returns, in get()'s order (cmbpo_buffer_trust_weights), against the NumPy statement of tests/policy_weights_ref.py.
A float32 store of a float64 quotient of exactly known float64 sums: rtol 1e-6."""
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

GAMMAS = dict(gamma=0.99, lam=0.95, cost_gamma=0.97, cost_lam=0.5)
B, T, D, A = 70, 6, 4, 2


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _schedule(seed):
    """ragged paths of lengths 1..6 (a fifth of the branches finish at step 1), dyn_error log-uniform in [1e-6, 1e2] with
    some exact zeros, obs[..., 0] = the unique id t * B + b of the entry"""
    rng = np.random.default_rng(seed)
    L = rng.integers(1, T + 1, B)
    L[::5] = 1
    L[3] = T
    assert set(L) == set(range(1, T + 1))
    step = {k: rng.standard_normal((T, B)).astype(np.float32) for k in ("rew", "val", "cost", "cval", "logp")}
    step["dyn_error"] = (10.0 ** rng.uniform(-6, 2, (T, B))).astype(np.float32)
    step["dyn_error"][rng.random((T, B)) < 0.1] = 0.0
    step["obs"] = rng.standard_normal((T, B, D)).astype(np.float32)
    step["obs"][..., 0] = (np.arange(T)[:, None] * B + np.arange(B)[None]).astype(np.float32)
    for k in ("act", "mu", "log_std"):
        step[k] = rng.standard_normal((T, B, A)).astype(np.float32)
    return L, step


def _fill(buf, L, step):
    alive = np.ones(B, bool)
    for t in range(int(L.max())):
        idx = np.flatnonzero(alive)
        s = {k: v[t, idx] for k, v in step.items()}
        buf.store_multiple(s["obs"], s["act"], s["obs"], s["rew"], s["val"], s["cost"], s["cval"], s["dyn_error"], s["logp"],
                           {"mu": s["mu"], "log_std": s["log_std"]}, np.zeros(len(idx), bool))
        tm = L[idx] == t + 1
        if tm.any():
            buf.finish_path_multiple(tm, np.zeros(int(tm.sum()), np.float32), np.zeros(int(tm.sum()), np.float32))
            alive[idx[tm]] = False
    assert not alive.any()


def _buffer(**kw):
    from cmbpo_amd.modelbuffer import ModelBuffer
    buf = ModelBuffer(B, D, A, T, device="cuda:0", **kw)
    buf.initialize({"mu": [A], "log_std": [A]}, **GAMMAS)
    return buf


@pytest.mark.parametrize("as_tensors", [False, True])
@pytest.mark.parametrize("ref_var", [1e-2, 1e-8])
def test_weights_follow_the_formula_in_the_order_of_get(hip_lib, ref_var, as_tensors):
    _need_gpu()
    L, step = _schedule(31)
    buf = _buffer(iv_gae=True)
    assert buf.last_weights is None
    buf.set_trust_weights(ref_var)
    _fill(buf, L, step)
    res, diag = buf.get(as_tensors=as_tensors)
    w = buf.last_weights
    assert isinstance(w, torch.Tensor) == as_tensors and len(res) == 12
    if as_tensors:
        assert w.dtype == torch.float32 and w.is_cuda
        w, ids = w.cpu().numpy(), res[0][:, 0].cpu().numpy()
    else:
        assert w.dtype == np.float32
        ids = res[0][:, 0]
    n = int(L.sum())
    assert w.shape == (n,) == ids.shape and diag["poolm_batch_size"] == n
    ids = ids.astype(np.int64)
    assert len(set(ids)) == n
    tt, bb = ids // B, ids % B
    cum = np.cumsum(step["dyn_error"].astype(np.float64), axis=0)       # the float64 running sum the buffer keeps
    want = (np.float64(ref_var) / (np.float64(ref_var) + cum[tt, bb])).astype(np.float32)
    np.testing.assert_allclose(w, want, rtol=1e-6, atol=0)
    # the same thing said once more: the restated order is get()'s order
    np.testing.assert_array_equal(want, wref.trust_weights(cum, L, ref_var))
    assert w.max() <= 1.0 and w.min() > 0.0 and (w == 1.0).any() and w.min() < 1e-3
    np.testing.assert_allclose(diag["poolm_weight_mean"], want.astype(np.float64).mean(), rtol=1e-6)
    np.testing.assert_allclose(diag["poolm_weight_min"], want.min(), rtol=1e-6)
    # get() has reset the buffer; the feature stays on
    assert buf.trust_var == ref_var and buf.size == 0 and buf.ptr == 0


def test_refusals_and_off(hip_lib):
    _need_gpu()
    L, step = _schedule(32)
    plain = _buffer()
    with pytest.raises(ValueError):
        plain.set_trust_weights(1e-2)                      # no iv_gae: no accumulated variance
    plain.set_trust_weights(None)                          # off is always legal
    buf = _buffer(iv_gae=True)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            buf.set_trust_weights(bad)
    buf.set_trust_weights(1e-2)                            # legal when nothing is stored
    with pytest.raises(ValueError):
        buf.set_iv_gae(False)                              # the weights read what it keeps
    idx = np.arange(B)
    s = {k: v[0, idx] for k, v in step.items()}
    buf.store_multiple(s["obs"], s["act"], s["obs"], s["rew"], s["val"], s["cost"], s["cval"], s["dyn_error"], s["logp"],
                       {"mu": s["mu"], "log_std": s["log_std"]}, np.zeros(B, bool))
    with pytest.raises(RuntimeError):
        buf.set_trust_weights(None)                        # samples are stored
    with pytest.raises(RuntimeError):
        buf.set_trust_weights(1.0)
    buf.finish_path_multiple(np.ones(B, bool), np.zeros(B, np.float32), np.zeros(B, np.float32))
    res_on, diag_on = buf.get()
    assert buf.last_weights.shape == (B,) and "poolm_weight_mean" in diag_on
    # off: no weights, no keys, and get() returns what it returned
    buf.set_trust_weights(None)
    assert buf.last_weights is None
    on, off = _buffer(iv_gae=True), _buffer(iv_gae=True)
    on.set_trust_weights(1e-2)
    _fill(on, L, step)
    _fill(off, L, step)
    r_on, d_on = on.get()
    r_off, d_off = off.get()
    assert off.last_weights is None and sorted(d_off) == ["poolm_batch_size", "poolm_cret_mean", "poolm_ret_mean"]
    assert sorted(set(d_on) - set(d_off)) == ["poolm_weight_mean", "poolm_weight_min"]
    for a, b in zip(r_on, r_off):
        np.testing.assert_array_equal(a, b)
    # from C: an error code without the attached variance table
    import ctypes as C
    from cmbpo_amd import _lib
    out = torch.zeros(B * T, dtype=torch.float32, device="cuda")
    rc = _lib.lib().cmbpo_buffer_trust_weights(C.byref(plain.rs), plain.t["offsets"].data_ptr(), 1e-2, out.data_ptr(), None)
    assert rc == -1 and b"cmbpo_rollout_iv_attach" in _lib.lib().cmbpo_last_error()
