"""GPU: every path of the ensemble training step (csrc/ens_train.hip) against a FLOAT64 evaluation of the training graph.

The yardstick, the cases and the bound MARGIN * max(e32, FLOOR) are those of tests/ens_train_f64_ref.py (its docstring states
where MARGIN comes from); tests/test_ens_train_f64_cpu.py shows that the bound separates a sound two-piece f16 product from one
that lost a piece.  A case asserts the kernels it is meant for (cmbpo_trainer_f16_paths, cmbpo_trainer_fused), so that it cannot
silently move to another kernel.

  A  first-step gradients (10 x the first Adam moment of a fresh trainer) and `self.loss`, every kernel path at its smallest shapes
     and edge widths: half-filled 16-wide k-slabs (in_pad 8 / 24 / 40, OPk 8 / 24 / 40 / 56), the OPk 64 / 72 switch to the fp32
     kernels, batches of 1, 31, 33, 63, 65 and 97 rows (f16 items are 64 rows, weight-gradient blocks 16 rows);
  B  ranges inside one batch, which the power-of-two lifts of the two-piece f16 operands have to cover; the error stays relative
     to the tensor's maximum, which is what a batch-wide lift can promise (with the input row of 1e3 x on the probabilistic
     head the log-variance half of W2 is a hundredth of its usual size: otherwise the float32 reference itself overflows exp
     on that row and has no gradient to compare with);
  C  a batch of 1, 17 or 33 rows on a trainer created for 2048, after a 2048-row step wrote into every partial-gradient slot: Adam
     adds up all `ks` slots, so the slots beyond the batch must be written as zeros;
  D  adam_all_kernel element by element from non-zero moments and seven steps done: m, v and w within 1e-6 (sixteen float32
     roundings; the chain is at most eight operations on values each known to one rounding) of a float64 evaluation of
     tf.train.AdamOptimizer's step on the float32 m0, v0, g, W0 and the trainer's float32 lr, beta1, beta2; the step count; and the
     prediction kernels' packed and f16 images followed the masters.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import ens_train_f64_ref as R  # noqa: E402


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _assert_gradients(ref, errs):
    fig = ref.figures()
    worst = {}
    for name, e32 in zip(R.TENSORS, fig["e32"]):
        worst[name] = (float(errs[name].max()), e32, float(errs[name].max()) / max(e32, R.FLOOR))
    print(R.case_id(ref.case), {k: "%.3g / e32 %.3g = %.2f" % v for k, v in worst.items()})
    for name, (err, e32, ratio) in worst.items():
        assert err <= ref.bound(e32), "%s %s: err %.3g per member %s > %g * max(e32 %.3g, %g); all: %s" % (
            R.case_id(ref.case), name, err, errs[name], R.MARGIN, e32, R.FLOOR, worst)


def _first_step(c):
    ref = R.reference_of(c)
    fig = ref.figures()
    errs, e_hold, e_boot = R.gpu_first_step_errors(ref)
    print(R.case_id(c), "loss errors: holdout %.3g (e32 %.3g), bootstrap rows %.3g (e32 %.3g)"
          % (e_hold.max(), fig["e32_hold"], e_boot.max(), fig["e32_boot"]))
    _assert_gradients(ref, errs)
    assert e_hold.max() <= ref.bound(fig["e32_hold"]), (e_hold, fig["e32_hold"])
    assert e_boot.max() <= ref.bound(fig["e32_boot"]), (e_boot, fig["e32_boot"])


@pytest.mark.parametrize("c", R.CASES_A, ids=R.case_id)
def test_first_step_gradients_and_losses_against_float64(hip_lib, c):
    _need_gpu()
    _first_step(c)


@pytest.mark.parametrize("c", R.CASES_B, ids=R.case_id)
def test_ranges_inside_one_batch_against_float64(hip_lib, c):
    _need_gpu()
    _first_step(c)


@pytest.mark.parametrize("c", R.CASES_C, ids=R.case_id)
def test_small_batch_on_a_large_trainer_against_float64(hip_lib, c):
    _need_gpu()
    ref = R.reference_of(c)
    _assert_gradients(ref, R.gpu_small_batch_errors(ref))


ADAM_TOL = 1e-6


@pytest.mark.parametrize("c", R.CASES_D, ids=R.case_id)
def test_adam_element_by_element(hip_lib, c):
    _need_gpu()
    ref = R.reference_of(c)
    d = R.gpu_adam(ref)
    errs = R.adam_errors(d)
    print(R.case_id(c), "adam errors (m, v, w) per tensor:", [(e["m"], e["v"], e["w"]) for e in errs])
    for name, e in zip(("W0", "W1", "W2", "b0", "b1", "b2"), errs):
        for what in ("m", "v", "w"):
            assert e[what] <= ADAM_TOL, (name, what, e)
    assert d["got"]["steps_done"] == 8
    # the images the prediction kernels read follow the masters: the floor-and-twice rule of tests/test_f16_range_gpu.py, the
    # float32 yardstick being a float32 numpy evaluation of the trainer's own weights
    pe = d["pe"]
    pe._weights_on_device = True
    e_hip, e_32 = R.forward_errors(pe, np.array(ref.x[:40]))
    print(R.case_id(c), "forward after the step: hip %s, float32 %s" % (e_hip.max(axis=1), e_32.max(axis=1)))
    worst = e_32.max(axis=1, keepdims=True)
    assert (e_hip <= 2.0 * np.maximum(np.maximum(worst, worst.mean()), R.FLOOR)).all(), (e_hip.max(axis=1), e_32.max(axis=1))
