"""GPU: the three-term f16 ensemble forward (ens_h3.hip, layer 1 and the output layer on v_mfma_f32_16x16x32_f16) at every
item size (32 / 64 / 128 rows) and both output-tile counts (two: AntSafe; four: HumanoidSafe's 2 x 46 outputs) against a
float64 evaluation of the same network, with the fp32-MFMA path's error as the yardstick."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F64 = np.float64
FLOOR = 6e-7


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _model(rng, task, E=7):
    from cmbpo_amd import synthetic
    from cmbpo_amd.pens import PE
    obs_dim, act_dim = synthetic.ENV_DIMS[task]
    ws, bs = synthetic.ensemble_weights(rng, E, obs_dim + act_dim, 512, 2 * (obs_dim + 1), bias_scale=0.05)
    sc_in, sc_out = synthetic.scaler(rng, obs_dim + act_dim), synthetic.scaler(rng, obs_dim + 1)
    m = PE(obs_dim + act_dim, obs_dim + 1, hidden_dims=(512, 512), num_networks=E, num_elites=5,
           loss="MSPE", use_scaler_in=True, use_scaler_out=True, device="cuda:0")
    m.set_weights(ws, bs, sc_in, sc_out)
    return m, ws, bs, sc_in, sc_out, obs_dim + act_dim


def _f64(x, ws, bs, sc_in, sc_out):
    """(mean, logvar)[E, B, out] in float64 (the scaler sigma as float32, models/pens/utils.py:156-187)."""
    sig_in = np.maximum(np.sqrt(np.asarray(sc_in[1], np.float32)), np.float32(1e-2)).astype(F64).reshape(1, -1)
    sig_out = np.maximum(np.sqrt(np.asarray(sc_out[1], np.float32)), np.float32(1e-2)).astype(F64).reshape(1, 1, -1)
    h = (x.astype(F64) - np.asarray(sc_in[0], F64).reshape(1, -1)) / sig_in
    h = np.einsum("ij,ajk->aik", h, ws[0].astype(F64)) + bs[0].astype(F64).reshape(ws[0].shape[0], 1, -1)
    h = h / (1.0 + np.exp(-h))
    h = np.matmul(h, ws[1].astype(F64)) + bs[1].astype(F64).reshape(ws[1].shape[0], 1, -1)
    h = h / (1.0 + np.exp(-h))
    o = np.matmul(h, ws[2].astype(F64)) + bs[2].astype(F64).reshape(ws[2].shape[0], 1, -1)
    half = o.shape[-1] // 2
    return sig_out * o[..., :half] + np.asarray(sc_out[0], F64).reshape(1, 1, -1), 2.0 * np.log(sig_out) + o[..., half:]


def _run(hip_lib, m, x, path, rt):
    before = hip_lib.cmbpo_get_ens_matrix_path()
    try:
        assert hip_lib.cmbpo_set_ens_matrix_path(path) == 0 and hip_lib.cmbpo_set_ens_f16_min_rows(0) == 0
        assert hip_lib.cmbpo_set_ens_f16_row_tiles(rt) == 0
        return m.predict_ensemble(x)
    finally:
        hip_lib.cmbpo_set_ens_f16_row_tiles(0)
        hip_lib.cmbpo_set_ens_f16_min_rows(0)
        hip_lib.cmbpo_set_ens_matrix_path(before)


def _errors(mean, var, rmean, rlv):
    """max over a (member, row)'s outputs of |out - ref| / that row's output scale, for the means and the log-variances"""
    e_mean = np.abs(mean.astype(F64) - rmean).max(axis=2) / np.maximum(np.abs(rmean).max(axis=2), 1e-30)
    e_lv = np.abs(np.log(var.astype(F64)) - rlv).max(axis=2) / np.maximum(np.abs(rlv).max(axis=2), 1.0)
    return e_mean, e_lv


@pytest.mark.parametrize("rt", [1, 2, 4])
@pytest.mark.parametrize("task", ["AntSafe-v2", "HumanoidSafe-v2"])      # two and four output tiles
@pytest.mark.parametrize("n", [7, 45, 150, 333])                        # neither multiples of 16 nor of 32
def test_f16_item_sizes_against_float64(hip_lib, rt, task, n):
    _cuda()
    rng = np.random.default_rng(zlib.crc32(f"mfma16/{task}/{n}/{rt}".encode()))
    m, ws, bs, sc_in, sc_out, in_dim = _model(rng, task)
    x = rng.standard_normal((n, in_dim)).astype(np.float32)
    rmean, rlv = _f64(x, ws, bs, sc_in, sc_out)
    f16 = _errors(*_run(hip_lib, m, x, 2, rt), rmean, rlv)
    f32 = _errors(*_run(hip_lib, m, x, 0, rt), rmean, rlv)
    for a, b, what in zip(f16, f32, ("mean", "logvar")):
        assert np.isfinite(a).all(), what
        # the three-term error stays within the fp32-MFMA path's (same measure as test_f16_range_gpu.py)
        bound = 2.0 * max(float(b.max()), FLOOR)
        assert float(a.max()) <= bound, (what, float(a.max()), float(b.max()))


@pytest.mark.parametrize("rt", [1, 2, 4])
@pytest.mark.parametrize("task", ["AntSafe-v2", "HumanoidSafe-v2"])
def test_f16_nonfinite_row_stays_in_its_row(hip_lib, rt, task):
    _cuda()
    rng = np.random.default_rng(zlib.crc32(f"mfma16-nan/{task}/{rt}".encode()))
    m, ws, bs, sc_in, sc_out, in_dim = _model(rng, task)
    n = 77
    x = rng.standard_normal((n, in_dim)).astype(np.float32)
    bad = (5, 38, 70)         # rows in different 16-row tiles, at different columns of their tiles
    x[bad[0], 3] = np.nan
    x[bad[1], 0] = np.inf
    x[bad[2], in_dim - 1] = -np.inf
    mean, var = _run(hip_lib, m, x, 2, rt)
    good = np.setdiff1d(np.arange(n), bad)
    for r in bad:
        assert not np.isfinite(mean[:, r]).all(), r
    clean_mean, clean_var = _run(hip_lib, m, x[good], 2, rt)
    np.testing.assert_array_equal(mean[:, good], clean_mean)
    np.testing.assert_array_equal(var[:, good], clean_var)
    rmean, rlv = _f64(x[good], ws, bs, sc_in, sc_out)
    e_mean, e_lv = _errors(mean[:, good], var[:, good], rmean, rlv)
    assert e_mean.max() < 1e-5 and e_lv.max() < 1e-5
