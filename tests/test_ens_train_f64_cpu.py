"""CPU: the yardstick of tests/test_ens_train_f64_gpu.py is sound (tests/ens_train_f64_ref.py; no GPU, no HIP library).

  * A hand-written float64 backward pass of the three-layer swish network whose five matrix products (dW2 = h2^T d3,
    d2 = d3 W2^T, dW1 = h1^T d2, d1 = d2 W1^T, dW0 = x^T d1) take their operands through a hook.  With the identity hook it is
    the float64 autograd reference to 1e-12.  With every operand cut to ONE f16 piece (lifted by a power of two per member, so
    nothing is lost to the f16 range) it errs like a two-piece kernel that lost a low piece or a cross term: the bound the GPU
    tests hold the kernels to must stay below an eighth of that on dW0 and dW1, on every 512-wide case.
    (d3, the derivative of the loss by the raw outputs, comes from autograd, so the one pass serves all three losses.)
  * Every case of the GPU tests is non-degenerate: each gradient tensor has a non-zero maximum, and the float32 reference's own
    error stays below 1e-5 (the worst measured was 2.4e-6): the yardstick is not itself ill-conditioned.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import column_weights_ref  # noqa: E402
import ens_train_f64_ref as R  # noqa: E402
from oracle import reftrain  # noqa: E402

F64 = torch.float64


def _lift(a):
    """Power of two per member that takes the slice's largest magnitude into [2^14, 2^15)."""
    m = a.abs().reshape(a.shape[0], -1).max(dim=1).values.clamp_min(1e-300)
    return torch.exp2(14.0 - torch.floor(torch.log2(m))).reshape(-1, 1, 1)


def one_piece(a):
    s = _lift(a)
    return (a * s).to(torch.float16).to(F64) / s


def two_pieces_no_lift(a):
    hi = a.to(torch.float16).to(F64)
    return hi + (a - hi).to(torch.float16).to(F64)


def emulated_grads(ref, hook):
    """[dW0, dW1, dW2, db0, db1, db2] in float64 on the case's bootstrap batch, matrix operands of the backward through `hook`."""
    r = ref.r64
    x = torch.as_tensor(ref.x[ref.idx], dtype=F64)
    t = torch.as_tensor(ref.t[ref.idx], dtype=F64)
    mu, var = r.scaler_in
    xn = (x - mu.reshape(1, 1, -1)) / reftrain.sigma_of(var).reshape(1, 1, -1)
    (W0, W1, W2), (b0, b1, b2) = r.ws, r.bs

    def swish(z):
        s = torch.sigmoid(z)
        return z * s, s * (1.0 + z * (1.0 - s))

    h1, g1 = swish(torch.matmul(xn, W0) + b0)
    h2, g2 = swish(torch.matmul(h1, W1) + b1)
    o = (torch.matmul(h2, W2) + b2).requires_grad_(True)
    ts = reftrain.scale_targets(t, r.scaler_out)
    if ref.case.weighted:
        w = column_weights_ref.element_weights(ref.t[ref.idx], ref.cw, ref.pw)
        per_member = {"MSPE": column_weights_ref.mspe_losses, "NLL": column_weights_ref.nll_losses}[ref.case.loss](o, ts, w)
    else:
        per_member = {"MSPE": reftrain.mspe_losses, "NLL": reftrain.nll_losses, "MSE": reftrain.mse_losses}[ref.case.loss](o, ts)
    d3, = torch.autograd.grad(per_member.sum(), o)
    T = lambda a: a.transpose(-1, -2)
    dW2 = torch.matmul(T(hook(h2)), hook(d3))
    d2 = torch.matmul(hook(d3), T(hook(W2))) * g2
    dW1 = torch.matmul(T(hook(h1)), hook(d2))
    d1 = torch.matmul(hook(d2), T(hook(W1))) * g1
    dW0 = torch.matmul(T(hook(xn)), hook(d1))
    gw = [g + dec * W for g, dec, W in zip((dW0, dW1, dW2), r.decays, r.ws)]
    return [g.numpy() for g in gw + [d.sum(dim=1, keepdim=True) for d in (d1, d2, d3)]]


@pytest.mark.parametrize("c", [R.CASES_A[0], R.CASES_A[11], R.CASES_A[16], R.CASES_A[23], R.CASES_A[28]], ids=R.case_id)
def test_hand_written_backward_is_the_autograd_reference(c):
    ref = R.reference_of(c)
    errs = R.tensor_errors(emulated_grads(ref, lambda a: a), ref.figures()["g64"])
    assert max(float(e.max()) for e in errs) <= 1e-12, errs


WIDE = [c for c in R.CASES_A + R.CASES_B + R.CASES_C if c.H == 512] + [R.case(2, 20, 512, 8, "MSE", 65, 1)]


@pytest.mark.parametrize("c", WIDE, ids=R.case_id)
def test_bound_is_an_eighth_of_a_lost_f16_piece(c):
    """MARGIN * max(e32, FLOOR) <= (one-piece emulation's error) / 8 on dW0 and dW1: the 512-wide 'MSE' case, an 8-output case,
    and every other 512-wide case of the GPU tests."""
    assert R.MARGIN is not None and R.MARGIN == 2.0 ** round(np.log2(R.MARGIN)) and R.MARGIN >= 2.0 * R.MEASURED_WORST_RATIO
    assert R.MARGIN < 4.0 * R.MEASURED_WORST_RATIO        # twice the measured worst ratio, rounded UP to a power of two: no more
    ref = R.reference_of(c)
    fig = ref.figures()
    one = R.tensor_errors(emulated_grads(ref, one_piece), fig["g64"])
    two = R.tensor_errors(emulated_grads(ref, two_pieces_no_lift), fig["g64"])
    for k in (0, 1):
        bound = ref.bound(fig["e32"][k])
        assert bound <= float(one[k].min()) / 8.0, \
            "%s %s: bound %.3g (e32 %.3g) against one f16 piece %s; two pieces without a lift (not asserted) %s, all tensors %s" % (
                R.case_id(c), R.TENSORS[k], bound, fig["e32"][k], one[k], two[k], [float(e.max()) for e in two])


@pytest.mark.parametrize("c", R.CASES_A + R.CASES_B + R.CASES_C, ids=R.case_id)
def test_cases_are_not_degenerate(c):
    fig = R.reference_of(c).figures()
    for name, g64, e32 in zip(R.TENSORS, fig["g64"], fig["e32"]):
        assert (np.abs(g64).reshape(g64.shape[0], -1).max(axis=1) > 0).all(), name
        assert e32 < 1e-5, (name, e32)
    for name in ("hold", "boot"):
        assert (fig[name + "64"] > 0).all() and fig["e32_" + name] < 1e-5, (name, fig["e32_" + name])


def test_tensor_errors_measure():
    ref64 = [np.array([[1.0, -4.0], [0.0, 0.5]]).reshape(2, 1, 2)]
    got = [np.array([[1.0, -3.0], [0.25, 0.5]]).reshape(2, 2)]
    np.testing.assert_allclose(R.tensor_errors(got, ref64)[0], [0.25, 0.5])
    assert R.tensor_errors([np.ones((1, 3))], [np.zeros((1, 3))])[0][0] > 1e100      # a reference of all zeros hides nothing
