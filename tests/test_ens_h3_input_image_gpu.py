"""GPU: the f16 ensemble forward writes the same bits whether its main launch builds the split input image itself, once per
(member, row), or reads the image that h3_ximage_kernel built once per row.

cmbpo_set_ens_f16_image_min_rows(1) sends every main launch of 128-row items on a stage-ahead instance (input width <= 48:
AntSafe, HalfCheetahSafe) through the image; (-1) never does.  Every case runs the same forward both ways and compares mean
and var in every slot with assert_array_equal: slots the row list never names, or beyond the device's row count, must still
be NaN both ways.  HumanoidSafe (input width 64: the old-order instance) never takes the image and must not change either.
"""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

E = 7


def _model(seed, task, scaler_in=True):
    from cmbpo_amd import synthetic
    from cmbpo_amd.pens import PE
    rng = np.random.default_rng(seed)
    obs_dim, act_dim = synthetic.ENV_DIMS[task]
    ws, bs = synthetic.ensemble_weights(rng, E, obs_dim + act_dim, 512, 2 * (obs_dim + 1), bias_scale=0.05)
    m = PE(obs_dim + act_dim, obs_dim + 1, hidden_dims=(512, 512), num_networks=E, num_elites=5, loss="MSPE",
           use_scaler_in=scaler_in, use_scaler_out=True, device="cuda:0")
    m.set_weights(ws, bs, synthetic.scaler(rng, obs_dim + act_dim) if scaler_in else None, synthetic.scaler(rng, obs_dim + 1))
    return m, obs_dim, act_dim


def _forward(lib, m, obs, act, rows, d_n, n_rows, mean, var):
    from cmbpo_amd import _lib
    with torch.cuda.device(0):
        _lib.check(lib.cmbpo_ens_forward(m.mlp.handle, _lib.ptr(obs), obs.shape[1], _lib.ptr(act), act.shape[1],
                                         _lib.ptr(rows) if rows is not None else None,
                                         _lib.ptr(d_n) if d_n is not None else None, n_rows, mean.shape[1], _lib.ptr(mean),
                                         _lib.ptr(var), _lib.current_stream()), "cmbpo_ens_forward")


class _Knobs:
    """the f16 path at every size, a forced item size, the image threshold; everything back to its default on exit"""

    def __init__(self, lib, rt):
        self.lib, self.rt = lib, rt

    def __enter__(self):
        self.before = self.lib.cmbpo_get_ens_matrix_path()
        assert self.lib.cmbpo_set_ens_matrix_path(2) == 0 and self.lib.cmbpo_set_ens_f16_min_rows(0) == 0
        assert self.lib.cmbpo_set_ens_f16_row_tiles(self.rt) == 0
        return self

    def image(self, rows):
        assert self.lib.cmbpo_set_ens_f16_image_min_rows(rows) == 0

    def __exit__(self, *exc):
        self.lib.cmbpo_set_ens_f16_image_min_rows(0)
        self.lib.cmbpo_set_ens_f16_row_tiles(0)
        self.lib.cmbpo_set_ens_f16_min_rows(0)
        self.lib.cmbpo_set_ens_matrix_path(self.before)
        return False


def _inputs(rng, n, ld, obs_dim, act_dim, with_list=True):
    dev = torch.device("cuda:0")
    rows_np = rng.permutation(ld)[:n].astype(np.int32) if with_list else None
    obs_np = (rng.standard_normal((ld, obs_dim)) * 0.5).astype(np.float32)
    act_np = rng.uniform(-1.0, 1.0, (ld, act_dim)).astype(np.float32)
    return rows_np, obs_np, act_np, dev


def _both_ways(lib, rt, m, out, ld, obs, act, rows, d_n, n):
    """the same forward with the image (1) and without (-1) -> (mean, var) of each, as numpy"""
    dev = obs.device
    res = []
    with _Knobs(lib, rt) as k:
        for setting in (1, -1):
            k.image(setting)
            mean = torch.full((E, ld, out), float("nan"), dtype=torch.float32, device=dev)
            var = torch.full((E, ld, out), float("nan"), dtype=torch.float32, device=dev)
            _forward(lib, m, obs, act, rows, d_n, n, mean, var)
            torch.cuda.synchronize()
            res.append((mean.cpu().numpy(), var.cpu().numpy()))
    return res


def _check(res, touched, poisoned=()):
    (mean_i, var_i), (mean_o, var_o) = res
    for a in (mean_i, var_i, mean_o, var_o):
        assert np.isnan(a[:, ~touched]).all()
    clean = touched.copy()
    clean[list(poisoned)] = False
    assert np.isfinite(mean_o[:, clean]).all() and np.isfinite(var_o[:, clean]).all()
    assert np.isfinite(mean_i[:, clean]).all() and np.isfinite(var_i[:, clean]).all()
    np.testing.assert_array_equal(mean_i, mean_o)
    np.testing.assert_array_equal(var_i, var_o)


# Forced 128-row items, 20 011 rows: 1 099 items, on 256 CUs four or five per workgroup (all but the first staged ahead, both
# constants copies reused), consecutive items of a workgroup 256 apart = in different members (157 tiles per member).
@pytest.mark.parametrize("task", ["AntSafe-v2", "HalfCheetahSafe-v2", "HumanoidSafe-v2"])
@pytest.mark.parametrize("dev_count", [False, True], ids=["hostcount", "devcount"])
def test_forced_128_row_items(hip_lib, task, dev_count):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 20011
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    seed = zlib.crc32(f"input-image/{task}/{dev_count}".encode())
    m, obs_dim, act_dim = _model(seed, task)
    rng = np.random.default_rng(seed + 1)
    ld = n + n // 3
    rows_np, obs_np, act_np, dev = _inputs(rng, n, ld, obs_dim, act_dim)
    bad_inf, bad_big = int(rows_np[3]), int(rows_np[128 * (n_cu // E) + 7])     # in the first item / in a later item of a member
    obs_np[bad_inf, 0] = np.inf
    obs_np[bad_big, 1] = 1e30
    obs, act, rows = torch.from_numpy(obs_np).to(dev), torch.from_numpy(act_np).to(dev), torch.from_numpy(rows_np).to(dev)
    n_alive = n - n // 4 - 5 if dev_count else n              # the device's row count: below the host's bound, mid-item
    d_n = torch.tensor([n_alive], dtype=torch.int32, device=dev) if dev_count else None
    res = _both_ways(hip_lib, 4, m, obs_dim + 1, ld, obs, act, rows, d_n, n)
    touched = np.zeros(ld, dtype=bool)
    touched[rows_np[:n_alive]] = True
    assert touched[bad_inf] and not np.isfinite(res[1][0][:, bad_inf]).all()
    _check(res, touched, (bad_inf, bad_big))


# one thread's row; a tile short by one; an exact tile; a second tile with a single row
@pytest.mark.parametrize("n", [1, 127, 128, 129])
def test_small_row_counts(hip_lib, n):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    seed = zlib.crc32(f"input-image/small/{n}".encode())
    m, obs_dim, act_dim = _model(seed, "AntSafe-v2")
    rng = np.random.default_rng(seed + 1)
    ld = n + n // 3 + 5
    rows_np, obs_np, act_np, dev = _inputs(rng, n, ld, obs_dim, act_dim)
    obs, act, rows = torch.from_numpy(obs_np).to(dev), torch.from_numpy(act_np).to(dev), torch.from_numpy(rows_np).to(dev)
    res = _both_ways(hip_lib, 4, m, obs_dim + 1, ld, obs, act, rows, None, n)
    touched = np.zeros(ld, dtype=bool)
    touched[rows_np] = True
    _check(res, touched)


# the automatic plan at 10 000 rows: two rounds of 128-row items (the image) + a leftover launch of 32-row items (no image)
def test_automatic_plan_10000_rows(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 10000
    seed = zlib.crc32(b"input-image/auto/10000")
    m, obs_dim, act_dim = _model(seed, "AntSafe-v2")
    rng = np.random.default_rng(seed + 1)
    ld = n + n // 3
    rows_np, obs_np, act_np, dev = _inputs(rng, n, ld, obs_dim, act_dim)
    obs, act, rows = torch.from_numpy(obs_np).to(dev), torch.from_numpy(act_np).to(dev), torch.from_numpy(rows_np).to(dev)
    res = _both_ways(hip_lib, 0, m, obs_dim + 1, ld, obs, act, rows, None, n)
    touched = np.zeros(ld, dtype=bool)
    touched[rows_np] = True
    _check(res, touched)


def test_no_input_scaler(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n = 3001
    seed = zlib.crc32(b"input-image/noscaler")
    m, obs_dim, act_dim = _model(seed, "AntSafe-v2", scaler_in=False)
    rng = np.random.default_rng(seed + 1)
    ld = n + n // 3
    rows_np, obs_np, act_np, dev = _inputs(rng, n, ld, obs_dim, act_dim)
    obs, act, rows = torch.from_numpy(obs_np).to(dev), torch.from_numpy(act_np).to(dev), torch.from_numpy(rows_np).to(dev)
    res = _both_ways(hip_lib, 4, m, obs_dim + 1, ld, obs, act, rows, None, n)
    touched = np.zeros(ld, dtype=bool)
    touched[rows_np] = True
    _check(res, touched)


def test_buffer_life_on_one_handle(hip_lib):
    """ld = 300, then ld = 40 000 (the buffer is regrown), then the first again; then two forwards back to back with different
    inputs.  Every result equals that of a fresh handle which never takes the image.  No row list: row i is slot i."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    seed = zlib.crc32(b"input-image/buffer")
    m, obs_dim, act_dim = _model(seed, "AntSafe-v2")
    out = obs_dim + 1
    rng = np.random.default_rng(seed + 1)
    dev = torch.device("cuda:0")

    def make(ld):
        _, obs_np, act_np, _ = _inputs(rng, ld, ld, obs_dim, act_dim, with_list=False)
        return torch.from_numpy(obs_np).to(dev), torch.from_numpy(act_np).to(dev)

    def blank(ld):
        return (torch.full((E, ld, out), float("nan"), dtype=torch.float32, device=dev),
                torch.full((E, ld, out), float("nan"), dtype=torch.float32, device=dev))

    small, big, small2 = make(300), make(40000), make(300)
    calls = [small, big, small, small2]
    got, ref = [], []
    with _Knobs(hip_lib, 4) as k:
        k.image(1)
        for obs, act in calls[:3]:                      # small, regrowth, small again
            mean, var = blank(obs.shape[0])
            _forward(hip_lib, m, obs, act, None, None, obs.shape[0], mean, var)
            torch.cuda.synchronize()
            got.append((mean.cpu().numpy(), var.cpu().numpy()))
        pair = [blank(300), blank(300)]                 # back to back on one stream, different inputs, no wait between them
        _forward(hip_lib, m, small[0], small[1], None, None, 300, *pair[0])
        _forward(hip_lib, m, small2[0], small2[1], None, None, 300, *pair[1])
        torch.cuda.synchronize()
        got.append((pair[1][0].cpu().numpy(), pair[1][1].cpu().numpy()))
        np.testing.assert_array_equal(pair[0][0].cpu().numpy(), got[0][0])
        k.image(-1)
        for obs, act in calls:
            fresh, _, _ = _model(seed, "AntSafe-v2")    # the same weights in a handle of its own
            mean, var = blank(obs.shape[0])
            _forward(hip_lib, fresh, obs, act, None, None, obs.shape[0], mean, var)
            torch.cuda.synchronize()
            ref.append((mean.cpu().numpy(), var.cpu().numpy()))
    for (gm, gv), (rm, rv) in zip(got, ref):
        assert np.isfinite(rm).all() and np.isfinite(rv).all()
        np.testing.assert_array_equal(gm, rm)
        np.testing.assert_array_equal(gv, rv)
