"""GPU: the policy-update kernels (pi_kernel_h<MODE_GRAD | MODE_FVP | MODE_EVAL | MODE_PPO>, the partial-vector reductions behind
them and the CG solve) against a FLOAT64 evaluation of the policy graph, on both matrix paths.

The yardstick, the cases and the bound MARGIN * max(e32[block], mean e32, FLOOR) are those of tests/pi_f64_ref.py (its docstring
states where MARGIN comes from); tests/test_pi_f64_cpu.py shows that the bound separates a sound two-piece f16 product from one
that lost a piece.  Every case runs both gradients, the eval sums and the Fisher-vector product at theta_old and 0.03 off it, for
three directions, on the recomputing and on the saved-activation kernel (asserted through cmbpo_pi_saved_activation_uses).

  A   smallest shapes at every border (in_pad groups of 8, half-filled 16-wide k-slabs, n_it 1 / 2, ragged and full last tiles);
  A2  more tiles than resident workgroups (asserted through cmbpo_pi_last_grid): next-tile prefetch, gradients carried in registers;
  B   ranges inside one batch, which the lifts of the two-piece operands have to cover;
  C   a batch of 1, 17 or 33 rows on the handle that just ran A2: only the slots the launch wrote are added, the large batch's
      saved activations are not read;
  W / PPO  fractional sample weights; ppo_grad with `clipped_adv` on and off at penalty 0 and 7.5;
  D   cg_dev against refupdate.cg on the float64 operator (CG_MARGIN, from its own measured ratio).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import pi_f64_ref as R  # noqa: E402


@pytest.fixture(autouse=True, params=[1, 0], ids=["splitf16", "fp32mfma"])
def pi_path(request, hip_lib):
    """Every test of this file on both arithmetic paths of the 128 x 128 products (cmbpo_set_pi_matrix_path)."""
    before = hip_lib.cmbpo_get_pi_matrix_path()
    hip_lib.cmbpo_set_pi_matrix_path(request.param)
    yield request.param
    hip_lib.cmbpo_set_pi_matrix_path(before)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _assert_records(c, records, margin=None):
    margin = R.MARGIN if margin is None else margin
    assert margin is not None
    worst = {}
    for mode, name, err, yard in records:
        if mode not in worst or err / yard > worst[mode][1] / worst[mode][2]:
            worst[mode] = (name, err, yard)
    print(R.case_id(c), {m: "%s %.3g / yardstick %.3g = %.2f" % (n, e, y, e / y) for m, (n, e, y) in worst.items()})
    bad = ["%s %s: err %.3g > %g * %.3g (ratio %.2f)" % (m, n, e, margin, y, e / y) for m, n, e, y in records if not e <= margin * y]
    assert not bad, "%s: %d of %d figures over the bound:\n%s" % (R.case_id(c), len(bad), len(records), "\n".join(bad))


def _plain(c):
    ref = R.reference_of(c)
    ops = R.make_ops(ref)
    R.bind(ops, ref)
    got = R.gpu_modes(ops, ref)
    _assert_records(c, R.mode_records(ref, got))
    return ref, got


@pytest.mark.parametrize("c", R.CASES_A, ids=R.case_id)
def test_smallest_shapes_at_every_border_against_float64(hip_lib, c):
    _need_gpu()
    _plain(c)


@pytest.mark.parametrize("c", R.CASES_A2, ids=R.case_id)
def test_two_tiles_per_workgroup_against_float64(hip_lib, c):
    _need_gpu()
    ref, got = _plain(c)
    tiles = -(-ref.n // 32)
    assert 0 < got["grid"] < tiles <= 2 * got["grid"], (got["grid"], tiles)       # some workgroups walked two tiles, none three


@pytest.mark.parametrize("c", R.CASES_B, ids=R.case_id)
def test_ranges_the_lifts_have_to_cover_against_float64(hip_lib, c):
    _need_gpu()
    _plain(c)


@pytest.mark.parametrize("c", R.CASES_C, ids=R.case_id)
def test_small_batch_after_a_large_one_on_the_same_handle_against_float64(hip_lib, c):
    _need_gpu()
    big, ref = R.reference_of(R.big_case_of(c)), R.reference_of(c)
    ops = R.make_ops(big)
    R.bind(ops, big)
    first = R.gpu_modes(ops, big)              # every partial-vector slot and the saved-activation block hold its data
    assert first["grid"] < -(-big.n // 32)
    R.bind(ops, ref)
    got = R.gpu_modes(ops, ref)
    assert got["grid"] == -(-ref.n // 32) < first["grid"]
    _assert_records(c, R.mode_records(ref, got))


@pytest.mark.parametrize("c", R.CASES_W, ids=R.case_id)
def test_fractional_sample_weights_against_float64(hip_lib, c):
    _need_gpu()
    _plain(c)


@pytest.mark.parametrize("c", R.CASES_PPO, ids=R.case_id)
def test_first_order_gradient_against_float64(hip_lib, c):
    _need_gpu()
    ref = R.reference_of(c)
    ops = R.make_ops(ref)
    R.bind(ops, ref)
    got = R.gpu_ppo(ops, ref)
    for combo, (g, s) in got.items():
        if combo[0] and ref.n >= 31:
            assert s[1] != s[6], "nothing clipped"
    _assert_records(c, R.ppo_records(ref, got))


@pytest.mark.parametrize("c", R.CASES_D, ids=R.case_id)
def test_cg_solve_against_float64(hip_lib, c):
    _need_gpu()
    assert R.CG_MARGIN is not None
    ref = R.reference_of(c)
    fig = ref.cg_figures()
    ops = R.make_ops(ref)
    R.bind(ops, ref)
    err = R.whole_error(R.gpu_cg(ops, ref), fig["x64"])
    print(R.case_id(c), "cg: err %.3g / e32 %.3g = %.2f" % (err, fig["e32"], err / max(fig["e32"], R.FLOOR)))
    assert err <= R.CG_MARGIN * max(fig["e32"], R.FLOOR), (err, fig["e32"])
