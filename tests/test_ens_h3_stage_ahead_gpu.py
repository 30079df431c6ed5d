"""GPU: a row's outputs of the f16 ensemble forward do not depend on whether its item was staged up front or ahead.

ens_h3_kernel stages the first item of a workgroup in front of its layers and every later item during the last fused step of
its predecessor (into the other copy of the per-item constants, behind the tail's buffers).  The other tests of this kernel
compare one multi-item forward with another, or with the oracle at 2e-4; this one compares bitwise
  * one forward of all rows, where a workgroup takes many items (all but its first staged ahead), with
  * the same rows forwarded in slices of at most floor(n_cu / E) row tiles of a forced item size, so that a launch has at most
    n_cu items and every item is the first of its workgroup (staged up front).
A row's bits do not depend on the item size it travels in (test_ens_forward_tail_round_as_shorter_items pins that), so the
slices of the automatic-plan case use a forced size too.

Every case runs with a row_idx list with holes (untouched rows must still be NaN), with and without a device row count below
the host's bound (the items at the end of the workgroups' lists are skipped), and with one row of inf and one of 1e30 whose
neighbours in the same and in the next item must stay finite and bit-equal.
"""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

E = 7


def _model(rng, task):
    from cmbpo_amd import synthetic
    from cmbpo_amd.pens import PE
    obs_dim, act_dim = synthetic.ENV_DIMS[task]
    ws, bs = synthetic.ensemble_weights(rng, E, obs_dim + act_dim, 512, 2 * (obs_dim + 1), bias_scale=0.05)
    m = PE(obs_dim + act_dim, obs_dim + 1, hidden_dims=(512, 512), num_networks=E, num_elites=5, loss="MSPE",
           use_scaler_in=True, use_scaler_out=True, device="cuda:0")
    m.set_weights(ws, bs, synthetic.scaler(rng, obs_dim + act_dim), synthetic.scaler(rng, obs_dim + 1))
    return m, obs_dim, act_dim


def _forward(lib, m, obs, act, rows, d_n, n_rows, mean, var):
    from cmbpo_amd import _lib
    with torch.cuda.device(0):
        _lib.check(lib.cmbpo_ens_forward(m.mlp.handle, _lib.ptr(obs), obs.shape[1], _lib.ptr(act), act.shape[1], _lib.ptr(rows),
                                         _lib.ptr(d_n), n_rows, mean.shape[1], _lib.ptr(mean), _lib.ptr(var),
                                         _lib.current_stream()), "cmbpo_ens_forward")


# (forced 32-row tiles per item -- 0: the automatic plan, which splits off a leftover launch with item0 > 0 --, task, rows).
# HalfCheetah / Ant / Humanoid: 2 / 3 / 4 input slabs, 2 / 2 / 4 output tiles.  Row counts are no multiples of an item; on 256
# CUs every forced case gives a workgroup three items or more (4 001 rows x 7 members = 882 items of 32 rows, 9 001 -> 987 of
# 64, 20 011 -> 1 099 of 128: both constants copies are reused), and consecutive items of a workgroup (256 apart, 126 .. 157
# tiles per member) belong to different members.
CASES = [(1, "AntSafe-v2", 4001), (1, "HalfCheetahSafe-v2", 4001), (1, "HumanoidSafe-v2", 4001),
         (2, "AntSafe-v2", 9001), (2, "HalfCheetahSafe-v2", 9001), (2, "HumanoidSafe-v2", 9001),
         (4, "AntSafe-v2", 20011), (4, "HalfCheetahSafe-v2", 20011), (4, "HumanoidSafe-v2", 20011),
         (0, "AntSafe-v2", 10000), (0, "HalfCheetahSafe-v2", 10000), (0, "HumanoidSafe-v2", 10000), (0, "AntSafe-v2", 35000)]


@pytest.mark.parametrize("rt,task,n", CASES)
@pytest.mark.parametrize("dev_count", [False, True], ids=["hostcount", "devcount"])
def test_row_bits_do_not_depend_on_where_the_item_was_staged(hip_lib, rt, task, n, dev_count):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda:0")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(zlib.crc32(f"stage-ahead/{task}/{n}/{rt}/{dev_count}".encode()))
    m, obs_dim, act_dim = _model(rng, task)
    out = obs_dim + 1
    ld = n + n // 3                                          # branch slots: a third of them never named by the row list
    rows_np = rng.permutation(ld)[:n].astype(np.int32)       # the row list: holes, no order
    obs_np = (rng.standard_normal((ld, obs_dim)) * 0.5).astype(np.float32)
    act_np = rng.uniform(-1.0, 1.0, (ld, act_dim)).astype(np.float32)
    item_rows = 32 * (rt if rt else 4)
    bad_inf, bad_big = int(rows_np[3]), int(rows_np[item_rows * (n_cu // E) + 7])     # in the first item / in a later item of a member
    obs_np[bad_inf, 0] = np.inf
    obs_np[bad_big, 1] = 1e30
    obs, act, rows = torch.from_numpy(obs_np).to(dev), torch.from_numpy(act_np).to(dev), torch.from_numpy(rows_np).to(dev)
    n_alive = n - n // 4 - 5 if dev_count else n              # the device's row count: below the host's bound, mid-item
    d_n = torch.tensor([n_alive], dtype=torch.int32, device=dev) if dev_count else None

    def blank():
        return torch.full((E, ld, out), float("nan"), dtype=torch.float32, device=dev)

    mean_all, var_all, mean_ref, var_ref = blank(), blank(), blank(), blank()
    before = hip_lib.cmbpo_get_ens_matrix_path()
    try:
        assert hip_lib.cmbpo_set_ens_matrix_path(2) == 0 and hip_lib.cmbpo_set_ens_f16_min_rows(0) == 0
        # one forward of all rows: workgroups take many items
        assert hip_lib.cmbpo_set_ens_f16_row_tiles(rt) == 0
        _forward(hip_lib, m, obs, act, rows, d_n, n, mean_all, var_all)
        # the reference: slices of at most floor(n_cu / E) row tiles of a forced item size -> at most n_cu items a launch
        rt_ref = rt if rt else 4
        assert hip_lib.cmbpo_set_ens_f16_row_tiles(rt_ref) == 0
        cap = (n_cu // E) * 32 * rt_ref
        assert cap > 0
        for s in range(0, n_alive, cap):
            cnt = min(cap, n_alive - s)
            assert (cnt + 32 * rt_ref - 1) // (32 * rt_ref) * E <= n_cu
            _forward(hip_lib, m, obs, act, rows[s:s + cnt], None, cnt, mean_ref, var_ref)
        torch.cuda.synchronize()
    finally:
        hip_lib.cmbpo_set_ens_f16_row_tiles(0)
        hip_lib.cmbpo_set_ens_f16_min_rows(0)
        hip_lib.cmbpo_set_ens_matrix_path(before)
    mean_all, var_all, mean_ref, var_ref = (t.cpu().numpy() for t in (mean_all, var_all, mean_ref, var_ref))
    touched = np.zeros(ld, dtype=bool)
    touched[rows_np[:n_alive]] = True
    # untouched branch slots (never in the list, or beyond the device's row count) are still NaN
    assert np.isnan(mean_all[:, ~touched]).all() and np.isnan(var_all[:, ~touched]).all()
    assert np.isnan(mean_ref[:, ~touched]).all() and np.isnan(var_ref[:, ~touched]).all()
    # every other row is finite but the two poisoned ones
    clean = touched.copy()
    clean[[bad_inf, bad_big]] = False
    assert np.isfinite(mean_ref[:, clean]).all() and np.isfinite(var_ref[:, clean]).all()
    assert touched[bad_inf] and not np.isfinite(mean_ref[:, bad_inf]).all()
    # bit for bit, every slot (NaNs and infinities in the same places)
    np.testing.assert_array_equal(mean_all, mean_ref)
    np.testing.assert_array_equal(var_all, var_ref)
