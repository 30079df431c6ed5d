"""CPU: predictive calibration in the model replay without a device -- the NumPy specification
tests/replay_calibration_ref.py on a case small enough to verify by eye and on a synthetic calibrated one, the host's derived
table and temperature(), the C-ABI of the three cmbpo_replay_calib* entry points (exports, header against binding, the struct
image, every refusal before any HIP call) and the argument refusals of CMBPO."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import replay_calibration_ref as cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------
# 1. the specification, by eye
# ------------------------------------------------------------------------------------------------------------------
def _hand_case():
    """3 windows x 2 steps x 2 members x 2 calibrated columns (one observation column and the reward; out_dim = 2).
    Window 1 has a zero variance in member 1's reward column at h = 0 and is dead on entry to h = 1 (with usable variances)."""
    f = lambda *a: np.array(a, np.float32)
    mean = np.zeros((2, 3, 2), np.float32)
    var = np.ones((2, 3, 2), np.float32)
    # window 0: the members disagree on the observation (1 and 3), both say variance 4; the reward: 0 +- 1
    mean[:, 0, 0], var[:, 0, 0] = (1.0, 3.0), (4.0, 4.0)
    # window 1: fine but for one variance
    var0 = var.copy()
    var0[1, 1, 1] = 0.0
    # window 2: the members agree on the mean (2) and not on the variance (1 and 4); the reward: 1 +- 0.5
    mean[:, 2, 0], var[:, 2, 0] = (2.0, 2.0), (1.0, 4.0)
    var0[:, 2, 0] = (1.0, 4.0)
    mean[:, 2, 1], var[:, 2, 1], var0[:, 2, 1] = 1.0, 0.25, 0.25
    var0[:, 0, 0] = 4.0
    pred = dict(next_obs=f([5.0], [7.0], [0.0]), rew=f(1.0, 0.0, 1.0), cost=f(0.0, 0.0, 0.0))
    rec = dict(next_obs=np.stack([f([3.0], [7.0], [4.0])] * 2), rew=np.stack([f(0.5, 0.0, 1.0)] * 2))
    elite = np.array([[0, 0, 1], [0, 0, 1]], np.int32)
    return pred, mean, (var0, var), rec, elite


def test_spec_by_eye():
    pred, mean, (var_h0, var_h1), rec, elite = _hand_case()
    tab = cref.new_table(2, 1)
    alive = np.array([True, True, True])
    m0 = cref.calibrate(tab, 0, alive, pred, mean, var_h0, rec, elite[0], 1)
    np.testing.assert_array_equal(m0, [True, False, True])             # window 1: skipped for var == 0
    alive = np.array([True, False, True])                               # ... and dead on entry to h = 1
    m1 = cref.calibrate(tab, 1, alive, pred, mean, var_h1, rec, elite[1], 1)
    np.testing.assert_array_equal(m1, [True, False, True])
    np.testing.assert_array_equal(tab["n"], [2, 2])
    np.testing.assert_array_equal(tab["n_skipped"], [1, 0])            # a dead row is not a skipped one
    # observation column.  window 0 (m = 0): e = 2, mu_bar = 2, v_bar = 4, s2 = 1; v_al = 4, v_tot = 5, e_tot = 2 + (2 - 1) = 3.
    # window 2 (m = 1): e = -4, mu_bar = 2, v_bar = 2.5, s2 = 0; v_al = 4, v_tot = 2.5, e_tot = -4.
    # reward column.  window 0: e = 0.5, v = 1, s2 = 0.  window 2: e = 0, v = 0.25, s2 = 0.
    want_sums = np.array([[4 / 4 + 16 / 4, 0.25 / 1 + 0.0],
                          [9 / 5 + 16 / 2.5, 0.25 / 1 + 0.0],
                          [math.log(4) + math.log(4), math.log(1) + math.log(0.25)],
                          [math.log(5) + math.log(2.5), math.log(1) + math.log(0.25)],
                          [4 + 2.5, 1 + 0.25],
                          [1 + 0, 0 + 0]])
    want_counts = np.array([[1, 2],          # e^2 <= v_al: 4 <= 4 yes, 16 <= 4 no
                            [2, 2],          # e^2 <= 4 v_al: 16 <= 16 yes
                            [0, 2],          # e_tot^2 <= v_tot: 9 <= 5 no, 16 <= 2.5 no
                            [1, 2]])         # e_tot^2 <= 4 v_tot: 9 <= 20 yes, 16 <= 10 no
    for h in (0, 1):
        np.testing.assert_allclose(tab["sums"][h], want_sums, rtol=4e-16, atol=0)
        np.testing.assert_array_equal(tab["counts"][h], want_counts)
    d = cref.derived(tab)
    np.testing.assert_allclose(d["z2_al"][0], [2.5, 0.125], rtol=1e-15)
    np.testing.assert_allclose(d["z2_tot"][0], [4.1, 0.125], rtol=1e-15)
    np.testing.assert_array_equal(d["cover1_al"][0], [0.5, 1.0])
    np.testing.assert_array_equal(d["cover2_tot"][0], [0.5, 1.0])
    np.testing.assert_array_equal(d["al_var"][0], [3.25, 0.625])
    np.testing.assert_array_equal(d["ep_var"][0], [0.5, 0.0])
    np.testing.assert_allclose(d["nll_al"][0, 0], 0.5 * (math.log(2 * math.pi) + math.log(4) + 2.5), rtol=1e-15)
    # the host's table from the raw arrays is the same thing
    from cmbpo_amd import replay
    got = replay.calibration_table(*cref.raw_arrays(tab), obs_dim=1)
    np.testing.assert_array_equal(got["n"], tab["n"])
    np.testing.assert_array_equal(got["n_skipped"], tab["n_skipped"])
    for k, v in d.items():
        np.testing.assert_array_equal(got[k], v, err_msg=k)
    for j, k in enumerate(replay.CALIB_SUM_KEYS):
        np.testing.assert_array_equal(got[k], tab["sums"][:, j], err_msg=k)
    for j, k in enumerate(replay.CALIB_COUNT_KEYS):
        np.testing.assert_array_equal(got[k], tab["counts"][:, j], err_msg=k)


def test_spec_rejects_each_kind_of_bad_row_once():
    pred, mean, (_, var), rec, elite = _hand_case()
    clean = cref.new_table(2, 1)
    cref.calibrate(clean, 0, np.ones(3, bool), pred, mean, var, rec, elite[0], 1)
    np.testing.assert_array_equal((clean["n"][0], clean["n_skipped"][0]), (3, 0))
    for arr, member, col, bad in (("var", 0, 0, np.inf), ("var", 1, 1, np.nan), ("var", 0, 1, -1.0), ("var", 1, 0, 0.0),
                                  ("mean", 1, 0, np.nan), ("mean", 0, 1, -np.inf)):     # (window 1's elite is member 0)
        mu, v = mean.copy(), var.copy()
        (mu if arr == "mean" else v)[member, 1, col] = bad
        tab = cref.new_table(2, 1)
        cref.calibrate(tab, 0, np.ones(3, bool), pred, mu, v, rec, elite[0], 1)
        assert (tab["n"][0], tab["n_skipped"][0]) == (2, 1), (arr, member, col, bad)
        assert np.isfinite(tab["sums"]).all()
    # a non-finite prediction: the plain table's n_nonfinite, neither count of this one
    for key in ("next_obs", "rew", "cost"):
        p = {k: v.copy() for k, v in pred.items()}
        p[key][1] = np.nan
        tab = cref.new_table(2, 1)
        cref.calibrate(tab, 0, np.ones(3, bool), p, mean, var, rec, elite[0], 1)
        assert (tab["n"][0], tab["n_skipped"][0]) == (2, 0), key
    # an empty horizon: NaN means, zero counts
    d = cref.derived(cref.new_table(1, 1))
    assert all(np.isnan(v).all() for v in d.values())


# ------------------------------------------------------------------------------------------------------------------
# 2. a calibrated model reads as calibrated
# ------------------------------------------------------------------------------------------------------------------
def check_synthetic(z2_al, cover1, cover2, shrunk_z2_al):
    """The bounds of the synthetic case (n = 20 000 rows): 5 sigma of a mean of chi^2_1 values (sqrt(2 / n) = 0.01) and of a
    binomial share (sqrt(p (1 - p) / n) = 0.0033, 0.0015)."""
    assert (np.abs(z2_al - 1.0) <= 0.05).all(), z2_al
    assert (np.abs(cover1 - cref.COVER1) <= 0.017).all(), cover1
    assert (np.abs(cover2 - cref.COVER2) <= 0.008).all(), cover2
    assert (np.abs(shrunk_z2_al - 4.0) <= 0.2).all(), shrunk_z2_al


def test_synthetic_calibrated_case():
    B, D, E = 20000, 3, 3
    out = []
    for shrink in (1.0, 0.25):
        pred, mean, var, rec, elite = cref.synthetic_case(B, D, E, seed=7, shrink=shrink)
        tab = cref.new_table(1, D)
        cref.calibrate(tab, 0, np.ones(B, bool), pred, mean, var, rec, elite, D)
        assert tab["n"][0] == B and tab["n_skipped"][0] == 0
        out.append(cref.derived(tab))
    d, s = out
    check_synthetic(d["z2_al"][0], d["cover1_al"][0], d["cover2_al"][0], s["z2_al"][0])
    # identical members: no epistemic part, the mixture is the member
    np.testing.assert_array_equal(d["ep_var"], 0.0)
    np.testing.assert_array_equal(d["z2_tot"], d["z2_al"])
    np.testing.assert_array_equal(d["cover1_tot"], d["cover1_al"])
    # the under-dispersed model pays for it in likelihood
    assert (s["nll_al"] > d["nll_al"]).all()


@pytest.mark.parametrize("learned_cost", [False, True])
@pytest.mark.parametrize("E", [3, 7])
def test_replay_world_has_finite_positive_variances(E, learned_cost):
    """The random-weight models of the whole-replay GPU test, through the oracle forward: every variance a window can meet
    on its way is finite and positive, so that test may demand n_skipped == 0."""
    from oracle import refcpu
    w = cref.replay_world(E, learned_cost)
    rng = np.random.default_rng(3)
    obs0, act, rec, _ = cref.recording(rng, 257, 3, w["D"], w["A"])
    for h in range(3):                                  # the teacher-forced inputs; the open-loop ones differ by ~0.05 a column
        x = np.concatenate([obs0 if h == 0 else rec["next_obs"][h - 1], act[h]], axis=1)
        mean, var = refcpu.ens_forward(x, w["ws"], w["bs"], w["sc_in"], w["sc_out"])
        assert mean.shape == (E, 257, w["O"]) and np.isfinite(mean).all()
        assert np.isfinite(var).all() and (var > 0).all() and var.min() > 1e-30


def test_temperature_clips_and_fills():
    from cmbpo_amd import replay
    z2 = np.array([[0.1, 1.5, np.nan, 9.0, 0.7], [2.0, 2.0, 2.0, 2.0, 2.0]])       # D = 4 and the reward column
    cal = dict(z2_al=z2, z2_tot=z2 * 2.0)
    t = replay.temperature(cal)
    assert t.dtype == np.float32 and t.shape == (4,)
    np.testing.assert_array_equal(t, np.array([0.25, 1.5, 1.0, 4.0], np.float32))
    np.testing.assert_array_equal(replay.temperature(cal, "tot", 0, 0.5, 2.5), np.array([0.5, 2.5, 1.0, 2.5], np.float32))
    np.testing.assert_array_equal(replay.temperature(cal, horizon=1), np.full(4, 2.0, np.float32))
    for bad in (dict(which="ep"), dict(lo=0.0), dict(lo=2.0, hi=1.0), dict(hi=np.inf)):
        with pytest.raises(ValueError, match="temperature"):
            replay.temperature(cal, **bad)
    with pytest.raises(ValueError, match="calibration_table"):
        replay.calibration_table(np.zeros((2, 12)), np.zeros((2, 9), np.int64), 1)


# ------------------------------------------------------------------------------------------------------------------
# 3. the C-ABI
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cmbpo_amd import _lib
    return _lib.lib()


def _header():
    text = open(os.path.join(ROOT, "include", "cmbpo_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


NAMES = ("cmbpo_replay_calibrate", "cmbpo_replay_calib_finish", "cmbpo_replay_run_calibrated")


def test_library_exports_the_three_symbols_and_keeps_its_version(lib):
    from cmbpo_amd import _lib
    assert lib.cmbpo_version() == 6
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES


def _struct_fields(text, tag, name):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (tag, name), text, flags=re.S)
    assert m, name + " is not declared"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        kind = "pointer" if "*" in decl else "int32"
        assert kind == "pointer" or decl.startswith("int32_t"), decl
        names = re.sub(r"^(const\s+)?(float|double|int32_t|int64_t|uint8_t)", "", decl)
        fields += [(n.strip().lstrip("*").strip(), kind) for n in names.split(",")]
    return fields


def test_header_signatures_and_struct_images_agree():
    from cmbpo_amd import _lib
    text = _header()
    image = lambda S: [(n, "pointer" if t is C.c_void_p else "int32" if t is C.c_int32 else "?") for n, t in S._fields_]
    fields = _struct_fields(text, "cmbpo_replay_calib", "cmbpo_replay_calib_t")
    assert image(_lib.ReplayCalibStruct) == fields
    assert fields == [("ensemble", "int32"), ("out_dim", "int32"), ("reserved", "int32"), ("elite", "pointer"),
                      ("part_sum", "pointer"), ("part_cnt", "pointer"), ("sums", "pointer"), ("counts", "pointer")]
    S = _lib.ReplayCalibStruct
    assert C.sizeof(S) == 56 and S.reserved.offset == 8 and S.elite.offset == 16 and S.counts.offset == 48
    # the replay descriptor is what it was
    assert image(_lib.ReplayStruct) == _struct_fields(text, "cmbpo_replay", "cmbpo_replay_t")
    assert C.sizeof(_lib.ReplayStruct) == 184 and len(_lib.ReplayStruct._fields_) == 26
    rp, cp = C.POINTER(_lib.ReplayStruct), C.POINTER(S)
    sig = _lib.SIGNATURES
    assert sig["cmbpo_replay_calibrate"] == (C.c_int, [rp, cp, C.c_int, C.c_void_p])
    assert sig["cmbpo_replay_calib_finish"] == (C.c_int, [rp, cp, C.c_void_p])
    assert sig["cmbpo_replay_run_calibrated"] == (C.c_int, [rp, cp, C.c_void_p, C.c_int, C.c_int, C.c_void_p])
    assert sig["cmbpo_replay_run"] == (C.c_int, [rp, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p])
    assert re.search(r"int cmbpo_replay_calibrate\(const cmbpo_replay_t \*rp, const cmbpo_replay_calib_t \*rc, int h, "
                     r"void \*stream\);", text)
    assert re.search(r"int cmbpo_replay_calib_finish\(const cmbpo_replay_t \*rp, const cmbpo_replay_calib_t \*rc, "
                     r"void \*stream\);", text)
    assert re.search(r"int cmbpo_replay_run_calibrated\(const cmbpo_replay_t \*rp, const cmbpo_replay_calib_t \*rc, "
                     r"cmbpo_mlp_t \*model, int task,\s*int ensemble, void \*stream\);", text)
    assert (_lib.REPLAY_CALIB_SUMS, _lib.REPLAY_CALIB_COUNTS) == (6, 4)
    assert re.search(r"#define CMBPO_REPLAY_CALIB_SUMS 6\b", text) and re.search(r"#define CMBPO_REPLAY_CALIB_COUNTS 4\b", text)


RP_ARRAYS = ("next_obs", "rew", "cost", "term", "len", "cur_obs", "alive", "p_next_obs", "p_rew", "p_term", "p_cost",
             "p_dkl_path", "p_ep_var_mean", "part_sum", "part_cnt", "mean", "var")
CALIBRATE_ARRAYS = ("elite", "part_sum", "part_cnt")
FINISH_ARRAYS = ("part_sum", "part_cnt", "sums", "counts")


def _images(rp_kw=None, rc_kw=None):
    """Descriptors whose every array points at host memory that is never read: each call below fails a check first."""
    from cmbpo_amd import _lib
    host = (C.c_double * 8)()
    addr = C.cast(host, C.c_void_p).value
    rs, cs = _lib.ReplayStruct(), _lib.ReplayCalibStruct()
    rs._keep = cs._keep = host
    rs.B, rs.H, rs.obs_dim, rs.act_dim, rs.mode = 5, 3, 11, 3, 0
    cs.ensemble, cs.out_dim = 7, 12
    for S, s in ((_lib.ReplayStruct, rs), (_lib.ReplayCalibStruct, cs)):
        for n, t in S._fields_:
            if t is C.c_void_p:
                setattr(s, n, addr)
    for k, v in (rp_kw or {}).items():
        setattr(rs, k, v)
    for k, v in (rc_kw or {}).items():
        setattr(cs, k, v)
    return rs, cs


def test_every_entry_refuses_bad_arguments_without_a_gpu(lib):
    fake = C.cast((C.c_double * 8)(), C.c_void_p)          # stands for a model handle that is never reached

    def calls(rs, cs, h=0):
        return (("cmbpo_replay_calibrate", lambda: lib.cmbpo_replay_calibrate(C.byref(rs), C.byref(cs), h, None)),
                ("cmbpo_replay_calib_finish", lambda: lib.cmbpo_replay_calib_finish(C.byref(rs), C.byref(cs), None)),
                ("cmbpo_replay_run_calibrated", lambda: lib.cmbpo_replay_run_calibrated(C.byref(rs), C.byref(cs), fake, 0, 7, None)))

    def refused(name, call, *words):
        assert call() == -1, name
        msg = lib.cmbpo_last_error()
        assert name.encode() in msg, msg
        for w in words:
            assert w in msg, msg

    # the shape refusals of the compare call, in all three
    for bad, word in ((dict(B=0), b"B 0"), (dict(B=-4), b"B -4"), (dict(H=0), b"H 0"), (dict(H=-1), b"H -1"),
                      (dict(mode=2), b"unknown mode 2"), (dict(mode=-1), b"unknown mode"), (dict(obs_dim=0), b"bad dims"),
                      (dict(obs_dim=513), b"bad dims"), (dict(act_dim=-1), b"bad dims"), (dict(reserved=1), b"reserved")):
        for name, call in calls(*_images(rp_kw=bad)):
            refused(name, call, word)
    # the calibration descriptor's own
    for bad, word in ((dict(ensemble=0), b"ensemble 0"), (dict(ensemble=-2), b"ensemble -2"), (dict(out_dim=11), b"out_dim 11"),
                      (dict(out_dim=0), b"out_dim 0"), (dict(reserved=3), b"reserved 3")):
        for name, call in calls(*_images(rc_kw=bad)):
            refused(name, call, word)
    # NULL descriptors
    rs, cs = _images()
    for name, call in (("cmbpo_replay_calibrate", lambda: lib.cmbpo_replay_calibrate(None, C.byref(cs), 0, None)),
                       ("cmbpo_replay_calibrate", lambda: lib.cmbpo_replay_calibrate(C.byref(rs), None, 0, None)),
                       ("cmbpo_replay_calib_finish", lambda: lib.cmbpo_replay_calib_finish(None, C.byref(cs), None)),
                       ("cmbpo_replay_calib_finish", lambda: lib.cmbpo_replay_calib_finish(C.byref(rs), None, None)),
                       ("cmbpo_replay_run_calibrated", lambda: lib.cmbpo_replay_run_calibrated(None, C.byref(cs), fake, 0, 7, None)),
                       ("cmbpo_replay_run_calibrated", lambda: lib.cmbpo_replay_run_calibrated(C.byref(rs), None, fake, 0, 7, None))):
        refused(name, call, b"NULL")
    # NULL arrays
    for k in RP_ARRAYS:
        rs, cs = _images(rp_kw={k: None})
        refused("cmbpo_replay_calibrate", lambda: lib.cmbpo_replay_calibrate(C.byref(rs), C.byref(cs), 0, None), b"NULL")
        refused("cmbpo_replay_run_calibrated", lambda: lib.cmbpo_replay_run_calibrated(C.byref(rs), C.byref(cs), fake, 0, 7, None),
                b"NULL")
    for k in ("act", "sums", "counts"):
        rs, cs = _images(rp_kw={k: None})
        refused("cmbpo_replay_run_calibrated", lambda: lib.cmbpo_replay_run_calibrated(C.byref(rs), C.byref(cs), fake, 0, 7, None),
                b"NULL")
    for k in CALIBRATE_ARRAYS:
        rs, cs = _images(rc_kw={k: None})
        refused("cmbpo_replay_calibrate", lambda: lib.cmbpo_replay_calibrate(C.byref(rs), C.byref(cs), 0, None), b"NULL")
        refused("cmbpo_replay_run_calibrated", lambda: lib.cmbpo_replay_run_calibrated(C.byref(rs), C.byref(cs), fake, 0, 7, None),
                b"NULL")
    for k in FINISH_ARRAYS:
        rs, cs = _images(rc_kw={k: None})
        refused("cmbpo_replay_calib_finish", lambda: lib.cmbpo_replay_calib_finish(C.byref(rs), C.byref(cs), None), b"NULL")
        refused("cmbpo_replay_run_calibrated", lambda: lib.cmbpo_replay_run_calibrated(C.byref(rs), C.byref(cs), fake, 0, 7, None),
                b"NULL")
    # h outside [0, H)
    rs, cs = _images()
    for h in (-1, 3, 4, 1 << 20):
        refused("cmbpo_replay_calibrate", lambda: lib.cmbpo_replay_calibrate(C.byref(rs), C.byref(cs), h, None), b"outside [0, 3)")
    # cmbpo_replay_run_calibrated alone: the handle, an ensemble that is not the descriptor's
    refused("cmbpo_replay_run_calibrated", lambda: lib.cmbpo_replay_run_calibrated(C.byref(rs), C.byref(cs), None, 0, 7, None), b"model")
    refused("cmbpo_replay_run_calibrated", lambda: lib.cmbpo_replay_run_calibrated(C.byref(rs), C.byref(cs), fake, 0, 5, None),
            b"ensemble 5")


# ------------------------------------------------------------------------------------------------------------------
# 4. the trainer's arguments
# ------------------------------------------------------------------------------------------------------------------
def test_cmbpo_refuses_calibration_arguments_that_do_not_fit():
    """The checks come first in the constructor: nothing is built, nothing needs a device (or an environment)."""
    from cmbpo_amd.cmbpo import CMBPO
    make = lambda **kw: CMBPO(None, None, None, **kw)
    with pytest.raises(ValueError, match="m_validate_calibration needs m_validate_horizon"):
        make(m_validate_calibration=True)
    with pytest.raises(ValueError, match="m_validate_calibration needs m_validate_horizon"):
        make(m_validate_calibration=True, m_validate_horizon=5, use_model=False)
    with pytest.raises(ValueError, match="m_calibrated_noise needs m_stochastic=True and m_validate_calibration=True"):
        make(m_calibrated_noise=True, m_validate_horizon=5, m_validate_calibration=True)
    with pytest.raises(ValueError, match="m_calibrated_noise needs"):
        make(m_calibrated_noise=True, m_validate_horizon=5, m_stochastic=True)
    with pytest.raises(ValueError, match="m_calibrated_noise needs"):
        make(m_calibrated_noise=True, m_stochastic=True)
    for bad in ((0.0, 4.0), (2.0, 1.0), (0.25, np.inf), (1.0,), None, (-1.0, 1.0)):
        with pytest.raises(ValueError, match="m_noise_temperature_range"):
            make(m_noise_temperature_range=bad)
