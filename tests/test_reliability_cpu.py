"""CPU: reliability tables of the logistic columns in the model replay without a device -- the NumPy specification
tests/reliability_ref.py on a case small enough to verify by eye and on a synthetic calibrated one, the host's derived table
and logit_offset(), the C-ABI of the three cmbpo_replay_reliab* entry points (exports, header against binding, the struct image,
every refusal before any HIP call), the refusals of FakeEnv / ModelSampler / CMBPO and the checkpoint file."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import reliability_ref as rref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
up = lambda x: np.nextafter(F32(x), F32(np.inf))
dn = lambda x: np.nextafter(F32(x), F32(-np.inf))
sig = lambda z: 1.0 / (1.0 + math.exp(-z))
nll = lambda z, y: max(z, 0.0) - y * z + math.log1p(math.exp(-abs(z)))


# ------------------------------------------------------------------------------------------------------------------
# 1. the specification, by eye
# ------------------------------------------------------------------------------------------------------------------
EDGES = np.array([-1.0, 0.5], F32)                                   # K = 3
COLS = [(2, rref.COST, 0.25), (3, rref.TERM, 0.0)]                   # D = 1: [obs | rew | cost | term]


def _hand_case():
    """4 windows x 2 steps x 2 members, the cost column (2, shift 0.25) and the termination column (3).  Per step the members'
    logits of the two columns; the comments of test_spec_by_eye say where each row goes."""
    nan, inf = np.nan, np.inf
    cost0 = [(0.75, 1.25), (0.25, 0.25), (nan, 0.0), (0.0, 0.0)]
    term0 = [(-1.0, -3.0), (up(0.5), dn(0.5)), (2.0, 2.0), (0.0, 0.0)]
    cost1 = [(0.0, inf), (nan, nan), (-2.25, -0.75), (1.0, 3.0)]
    term1 = [(up(-1.0), 0.0), (nan, nan), (0.5, 1.5), (-4.0, -2.0)]
    means = []
    for cost, term in ((cost0, term0), (cost1, term1)):
        m = np.zeros((2, 4, 4), F32)
        m[:, :, 2], m[:, :, 3] = np.array(cost, F32).T, np.array(term, F32).T
        means.append(m)
    elite = np.array([[0, 1, 0, 2], [0, 0, 1, 0]], np.int32)         # window 3 at h = 0: no such member
    alive = (np.array([1, 1, 1, 1], bool), np.array([1, 0, 1, 1], bool))      # window 1 is dead on entry to h = 1
    rec = dict(cost=np.array([[1.0, 0.4, 0.0, 1.0], [0.0, 0.0, 0.6, 0.0]], F32), term=np.array([[0, 1, 1, 0], [0, 0, 0, 1]], np.uint8))
    pred = dict(next_obs=np.zeros((4, 1), F32), rew=np.zeros(4, F32), cost=np.zeros(4, F32))
    return pred, means, rec, elite, alive


def _run_hand_case():
    pred, means, rec, elite, alive = _hand_case()
    tab = rref.new_table(2, 2, 3)
    masks = [rref.reliab(tab, h, alive[h], pred, means[h], rec, elite[h], COLS, EDGES) for h in range(2)]
    return tab, masks


def test_spec_by_eye():
    tab, masks = _run_hand_case()
    # h = 0.  cost: window 2 has a NaN logit, window 3 an elite out of range: skipped.  z' = logit - 0.25.
    #   window 0: z' = (0.5, 1.0), elite 0: 0.5 EXACTLY on the edge 0.5 -> bin 1 (equality stays below); pooled 0.75 -> bin 2; y = 1
    #   window 1: z' = (0, 0): bin 1 in both readings; cost 0.4 is not > 0.5: y = 0
    # term: window 3 skipped.
    #   window 0: (-1, -3), elite 0: -1 exactly on the edge -1 -> bin 0; pooled -2 -> bin 0; y = 0
    #   window 1: (0.5 + ulp, 0.5 - ulp), elite 1: one ulp below the edge -> bin 1; pooled 0.5 + 2^-26 (float64) -> bin 2; y = 1
    #   window 2: (2, 2) -> bin 2; y = 1
    np.testing.assert_array_equal(masks[0], [[True, True, False, False], [True, True, True, False]])
    np.testing.assert_array_equal(tab["n_rel"], [[2, 3], [2, 3]])
    np.testing.assert_array_equal(tab["n_skipped"], [[2, 1], [1, 0]])
    np.testing.assert_array_equal(tab["n"][0, 0], [[0, 2, 0], [0, 1, 1]])
    np.testing.assert_array_equal(tab["pos"][0, 0], [[0, 1, 0], [0, 0, 1]])
    np.testing.assert_array_equal(tab["n"][0, 1], [[1, 1, 1], [1, 0, 2]])
    np.testing.assert_array_equal(tab["pos"][0, 1], [[0, 1, 1], [0, 0, 2]])
    # h = 1.  window 1 is dead: in no count, its NaNs are never looked at.  cost: window 0 has an infinite logit: skipped.
    #   window 2: z' = (-2.5, -1.0), elite 1: -1 on the edge -> bin 0; pooled -1.75 -> bin 0; cost 0.6: y = 1
    #   window 3: z' = (0.75, 2.75), elite 0 -> bin 2; pooled 1.75 -> bin 2; y = 0
    # term: window 0: (-1 + ulp, 0), elite 0: one ulp above the edge -1 -> bin 1; pooled ~ -0.5 -> bin 1; y = 0
    #   window 2: (0.5, 1.5), elite 1 -> bin 2; pooled 1.0 -> bin 2; y = 0       window 3: (-4, -2) -> bin 0 in both; y = 1
    np.testing.assert_array_equal(masks[1], [[False, False, True, True], [True, False, True, True]])
    np.testing.assert_array_equal(tab["n"][1, 0], [[1, 0, 1], [1, 0, 1]])
    np.testing.assert_array_equal(tab["pos"][1, 0], [[1, 0, 0], [1, 0, 0]])
    np.testing.assert_array_equal(tab["n"][1, 1], [[1, 1, 1], [1, 1, 1]])
    np.testing.assert_array_equal(tab["pos"][1, 1], [[1, 0, 0], [1, 0, 0]])
    # the sums of the cost column at h = 0
    np.testing.assert_allclose(tab["sum_z"][0, 0], [[0, 0.5 + 0.0, 0], [0, 0.0, 0.75]], rtol=0, atol=0)
    np.testing.assert_allclose(tab["sum_p"][0, 0], [[0, sig(0.5) + 0.5, 0], [0, 0.5, sig(0.75)]], rtol=4e-16)
    np.testing.assert_allclose(tab["sum_brier"][0, 0], [sig(-0.5) ** 2 + 0.25, 0.25 + sig(-0.75) ** 2], rtol=1e-15)
    np.testing.assert_allclose(tab["sum_logloss"][0, 0], [nll(0.5, 1) + math.log(2), math.log(2) + nll(0.75, 1)], rtol=1e-15)
    # ... and of the termination column at h = 1, elite reading
    z0 = float(up(-1.0))
    np.testing.assert_allclose(tab["sum_z"][1, 1, 0], [-4.0, z0, 1.5], rtol=0, atol=0)
    np.testing.assert_allclose(tab["sum_logloss"][1, 1, 0], nll(z0, 0) + nll(1.5, 0) + nll(-4.0, 1), rtol=1e-15)
    # the host's table from the raw arrays is the same thing
    from cmbpo_amd import replay
    got = replay.reliability_table(*rref.raw_arrays(tab), n_bins=3, names=("cost", "term"), edges=EDGES)
    assert sorted(got) == ["cost", "term"]
    for j, name in enumerate(("cost", "term")):
        np.testing.assert_array_equal(got[name]["n_rel"], tab["n_rel"][:, j])
        np.testing.assert_array_equal(got[name]["n_skipped"], tab["n_skipped"][:, j])
        np.testing.assert_array_equal(got[name]["edges"], EDGES)
        for r, reading in enumerate(replay.READINGS):
            d = got[name][reading]
            for k in ("n", "pos", "sum_p", "sum_z", "sum_brier", "sum_logloss"):
                np.testing.assert_array_equal(d[k], tab[k][:, j, r], err_msg=k)
            for k, v in rref.derived(tab, j, r).items():
                np.testing.assert_array_equal(d[k], v, err_msg=k)
    d = got["cost"]["elite"]
    assert np.isnan(d["conf"][0, 0]) and np.isnan(d["freq"][0, 2]) and d["freq"][0, 1] == 0.5          # empty bins: NaN
    assert d["ece"][0] == pytest.approx(abs((sig(0.5) + 0.5) / 2 - 0.5), rel=1e-13) and d["mce"][0] == d["ece"][0]
    assert d["base_rate"][0] == 0.5


def test_spec_rejects_a_non_finite_prediction_and_counts_per_column():
    pred, means, rec, elite, alive = _hand_case()
    for key in ("next_obs", "rew", "cost"):
        p = {k: v.copy() for k, v in pred.items()}
        p[key][0] = np.inf                                            # the plain table's n_nonfinite: in neither count here
        tab = rref.new_table(2, 2, 3)
        rref.reliab(tab, 0, alive[0], p, means[0], rec, elite[0], COLS, EDGES)
        np.testing.assert_array_equal((tab["n_rel"][0], tab["n_skipped"][0]), ([1, 2], [2, 1]), err_msg=key)
    # the descriptor's own flags take the place of the recorded terminals for TERM columns only
    tab = rref.new_table(2, 2, 3)
    rref.reliab(tab, 0, alive[0], pred, means[0], dict(rec, term_target=np.zeros((2, 4), np.uint8)), elite[0], COLS, EDGES)
    assert tab["pos"][0, 1].sum() == 0 and tab["pos"][0, 0].sum() == 2
    # an empty horizon: NaN everywhere, zero counts
    d = rref.derived(rref.new_table(1, 1, 3), 0, 0)
    assert all(np.isnan(v).all() for v in d.values())


def test_reliability_table_with_one_bin_and_bad_shapes():
    from cmbpo_amd import replay
    tab = rref.new_table(1, 1, 1)
    pred, means, rec, elite, alive = _hand_case()
    rref.reliab(tab, 0, alive[0], pred, means[0], rec, elite[0], [COLS[1]], np.zeros(0, F32))
    got = replay.reliability_table(*rref.raw_arrays(tab), n_bins=1, names=("term",))["term"]
    assert got["n_rel"][0] == 3 and got["elite"]["n"].shape == (1, 1) and got["elite"]["n"][0, 0] == 3 and got["edges"] is None
    assert got["elite"]["freq"][0, 0] == 2 / 3 == got["elite"]["base_rate"][0]
    assert got["elite"]["ece"][0] == abs(got["elite"]["conf"][0, 0] - 2 / 3) == got["elite"]["mce"][0]
    with pytest.raises(ValueError, match="reliability_table"):
        replay.reliability_table(np.zeros((1, 7)), np.zeros((1, 4), np.int64), 1, ("term",))
    np.testing.assert_array_equal(replay.default_edges(15), rref.default_edges(15))
    e = replay.default_edges(4)
    assert e.dtype == F32 and e.shape == (3,) and e[1] == 0.0 and e[0] == F32(math.log(1 / 3)) and (np.diff(e) > 0).all()
    assert replay.default_edges(1).shape == (0,)


# ------------------------------------------------------------------------------------------------------------------
# 2. the logit offset
# ------------------------------------------------------------------------------------------------------------------
def _rel(n, pos, zbar):
    n, pos, zbar = np.asarray([n], np.int64), np.asarray([pos], np.int64), np.asarray([zbar], np.float64)
    return {"c": {"elite": dict(n=n, pos=pos, zbar=zbar), "pooled": dict(n=n, pos=pos, zbar=zbar + 1.0)}}


def test_logit_offset():
    from cmbpo_amd.replay import logit_offset
    sym = _rel([100, 50, 100], [12, 25, 88], [-2.0, 0.0, 2.0])       # sigma(-2) = 0.1192: 100 (s(-2) + s(2)) + 50 / 2 = 125 = pos
    assert abs(logit_offset(sym, "c")) < 1e-12
    assert abs(logit_offset(sym, "c", reading="pooled") - 1.0) < 1e-12            # every logit one too high: subtract one
    # fewer positives than the column says: a positive offset, found to the last bit the bisection can give
    less = _rel([100, 50, 100], [5, 10, 50], [-2.0, 0.0, 2.0])
    b = logit_offset(less, "c")
    n, z = np.array([100, 50, 100.0]), np.array([-2.0, 0.0, 2.0])
    assert 0 < b < 2 and abs((n / (1 + np.exp(-(z - b)))).sum() - 65) < 1e-9
    assert logit_offset(less, "c", lo=-0.25, hi=0.25) == 0.25 and logit_offset(less, "c", lo=-3, hi=-1) == -1.0       # the clip
    assert logit_offset(sym, "c", min_n=251) is None and logit_offset(sym, "c", min_n=250) is not None              # N = 250
    assert logit_offset(_rel([0, 0, 0], [0, 0, 0], [np.nan] * 3), "c", min_n=0) is None
    assert logit_offset(_rel([100, 50, 100], [0, 0, 0], [-2.0, 0.0, 2.0]), "c") == 2.0                # no positives: the upper end
    assert logit_offset(_rel([100, 50, 100], [100, 50, 100], [-2.0, 0.0, 2.0]), "c") == -2.0          # only positives: the lower
    assert logit_offset(_rel([100, 0, 100], [50, 0, 50], [-1.0, np.nan, 1.0]), "c") == pytest.approx(0.0, abs=1e-12)  # empty bin
    for bad in (dict(reading="mean"), dict(lo=1.0, hi=0.0), dict(lo=-np.inf)):
        with pytest.raises(ValueError, match="logit_offset"):
            logit_offset(sym, "c", **bad)


# ------------------------------------------------------------------------------------------------------------------
# 3. a calibrated column reads as calibrated
# ------------------------------------------------------------------------------------------------------------------
# |logit_offset - exact per-row offset| on the synthetic case shifted by +1, measured once from the reference alone (this file's
# test prints it: logit_offset 1.029115, exact 1.003374, bias 0.025740): every row of a bin stands at the bin's mean logit, and
# sigma is not linear over a bin -- least of all over the two outermost bins, which are unbounded in logit space
BIN_MEAN_BIAS = 0.0258


def check_synthetic(rel, rel_shifted, p_true):
    """The bounds of the synthetic case (n = 20 000 rows, z ~ N(0, 2^2), y ~ Bernoulli(sigma(z))): in every bin of at least 50
    rows confidence and frequency differ by at most 5 sigma of a binomial share at its widest, sqrt(0.25 / n_k); with every logit
    one too high, logit_offset gives 1 within 5 standard errors of the maximum-likelihood offset, 1 / sqrt(sum p (1 - p)) (its
    Fisher information), plus twice the measured bias of the bin-mean approximation."""
    from cmbpo_amd.replay import logit_offset
    for reading in ("elite", "pooled"):
        d = rel[reading]
        big = d["n"][0] >= 50
        assert big.sum() >= 10
        gap = np.abs(d["conf"][0] - d["freq"][0])[big]
        assert (gap <= 5.0 * np.sqrt(0.25 / d["n"][0][big])).all(), (reading, gap)
        b = logit_offset({"c": rel_shifted}, "c", reading=reading)
        se = 1.0 / math.sqrt(float((p_true * (1.0 - p_true)).sum()))
        assert abs(b - 1.0) <= 5.0 * se + 2.0 * BIN_MEAN_BIAS, (reading, b, se)
    return b


def _synthetic_tables(reliab_fn):
    out = []
    for offset in (0.0, 1.0):
        pred, mean, rec, elite, z = rref.synthetic_case(20000, 3, seed=11, offset=offset)
        out.append(reliab_fn(pred, mean, rec, elite))
    return out[0], out[1], 1.0 / (1.0 + np.exp(-z.astype(np.float64)))


def test_synthetic_calibrated_case():
    from cmbpo_amd import replay
    edges = rref.default_edges(15)

    def by_reference(pred, mean, rec, elite):
        tab = rref.new_table(1, 1, 15)
        rref.reliab(tab, 0, np.ones(20000, bool), pred, mean, rec, elite, [(0, rref.TERM, 0.0)], edges)
        assert tab["n_rel"][0, 0] == 20000 and tab["n_skipped"][0, 0] == 0
        return replay.reliability_table(*rref.raw_arrays(tab), 15, ("c",), edges=edges)["c"]

    rel, shifted, p_true = _synthetic_tables(by_reference)
    b = check_synthetic(rel, shifted, p_true)
    # identical members: the two readings see the same logits (the mean of three equal float32 numbers is that number)
    np.testing.assert_array_equal(rel["elite"]["n"], rel["pooled"]["n"])
    assert rel["elite"]["ece"][0] < 0.02 < shifted["elite"]["ece"][0]
    assert abs(shifted["elite"]["mean_p"][0] - shifted["elite"]["base_rate"][0]) > 0.05
    # the bias of the bin-mean approximation against the exact per-row solve on the same data
    pred, mean, rec, elite, _ = rref.synthetic_case(20000, 3, seed=11, offset=1.0)
    exact = rref.exact_offset(mean[0, :, 0], rec["term"][0])
    bias = abs(b - exact)
    print("logit_offset %.6f, exact per-row offset %.6f, bias %.6f" % (b, exact, bias))
    assert bias <= BIN_MEAN_BIAS and bias >= 0.5 * BIN_MEAN_BIAS, bias      # the constant above is the measurement, not a guess


# ------------------------------------------------------------------------------------------------------------------
# 4. the C-ABI
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


NAMES = ("cmbpo_replay_reliab", "cmbpo_replay_reliab_finish", "cmbpo_replay_run_reliab")


def test_library_exports_the_three_symbols_and_keeps_its_version(lib):
    from cmbpo_amd import _lib
    assert lib.cmbpo_version() == 6
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES


def test_header_signatures_and_struct_image_agree():
    from cmbpo_amd import _lib
    text = _header()
    m = re.search(r"typedef struct cmbpo_replay_reliab \{(.*?)\} cmbpo_replay_reliab_t;", text, flags=re.S)
    assert m, "cmbpo_replay_reliab_t is not declared"
    fields = []
    for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
        base = "pointer" if "*" in decl else "float" if decl.startswith("float") else "int32"
        assert base != "int32" or decl.startswith("int32_t"), decl
        names = re.sub(r"^(const\s+)?(float|double|int32_t|int64_t|uint8_t)", "", decl)
        for n in names.split(","):
            n = n.strip().lstrip("*").strip()
            arr = re.match(r"(\w+)\[(\d+)\]$", n)
            fields.append((arr.group(1), base, int(arr.group(2))) if arr else (n, base, 0))
    kind = {C.c_void_p: ("pointer", 0), C.c_int32: ("int32", 0), C.c_int32 * 2: ("int32", 2), C.c_float * 2: ("float", 2)}
    S = _lib.ReplayReliabStruct
    assert [(n,) + kind[t] for n, t in S._fields_] == fields
    assert [f[0] for f in fields] == ["ensemble", "out_dim", "n_bins", "n_cols", "reserved", "col", "target", "shift", "elite",
                                      "edges", "term", "part_sum", "part_cnt", "sums", "counts"]
    assert C.sizeof(S) == 104 and S.reserved.offset == 16 and S.col.offset == 20 and S.shift.offset == 36
    assert S.elite.offset == 48 and S.counts.offset == 96
    # the two other descriptors are what they were
    assert C.sizeof(_lib.ReplayStruct) == 184 and C.sizeof(_lib.ReplayCalibStruct) == 56
    rp, cp, rr = C.POINTER(_lib.ReplayStruct), C.POINTER(_lib.ReplayCalibStruct), C.POINTER(S)
    tp, chp = C.POINTER(_lib.TermHeadStruct), C.POINTER(_lib.CostHeadStruct)
    sig_ = _lib.SIGNATURES
    assert sig_["cmbpo_replay_reliab"] == (C.c_int, [rp, rr, C.c_int, C.c_void_p])
    assert sig_["cmbpo_replay_reliab_finish"] == (C.c_int, [rp, rr, C.c_void_p])
    assert sig_["cmbpo_replay_run_reliab"] == (C.c_int, [rp, cp, rr, tp, chp, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p])
    assert re.search(r"int cmbpo_replay_reliab\(const cmbpo_replay_t \*rp, const cmbpo_replay_reliab_t \*rr, int h, void \*stream\);", text)
    assert re.search(r"int cmbpo_replay_reliab_finish\(const cmbpo_replay_t \*rp, const cmbpo_replay_reliab_t \*rr, void \*stream\);", text)
    assert re.search(r"int cmbpo_replay_run_reliab\(const cmbpo_replay_t \*rp, const cmbpo_replay_calib_t \*rc, const cmbpo_replay_reliab_t \*rr,"
                     r"\s*const cmbpo_term_head_t \*th, const cmbpo_cost_head_t \*ch, cmbpo_mlp_t \*model, int task,\s*int ensemble, "
                     r"const int32_t \*d_elite, void \*stream\);", text)
    for name, value in (("COST", 0), ("TERM", 1), ("MAX_BINS", 32), ("MAX_COLS", 2), ("MAX_ENSEMBLE", 8)):
        assert re.search(r"#define CMBPO_RELIAB_%s %d\b" % (name, value), text), name
        assert getattr(_lib, "RELIAB_" + name) == value


def _images(rp_kw=None, rr_kw=None, rc_kw=None):
    """Descriptors whose every array points at host memory that is never read: each call below fails a check first."""
    from cmbpo_amd import _lib
    host = (C.c_double * 8)()
    addr = C.cast(host, C.c_void_p).value
    rs, cs, rr = _lib.ReplayStruct(), _lib.ReplayCalibStruct(), _lib.ReplayReliabStruct()
    rs._keep = cs._keep = rr._keep = host
    rs.B, rs.H, rs.obs_dim, rs.act_dim, rs.mode = 5, 3, 11, 3, 0
    cs.ensemble, cs.out_dim = 7, 14
    rr.ensemble, rr.out_dim, rr.n_bins, rr.n_cols = 7, 14, 15, 2
    rr.col[0], rr.col[1], rr.target[0], rr.target[1], rr.shift[0] = 12, 13, 0, 1, 0.5
    for S, s in ((_lib.ReplayStruct, rs), (_lib.ReplayCalibStruct, cs), (_lib.ReplayReliabStruct, rr)):
        for n, t in S._fields_:
            if t is C.c_void_p:
                setattr(s, n, addr)
    for s, kw in ((rs, rp_kw), (cs, rc_kw), (rr, rr_kw)):
        for k, v in (kw or {}).items():
            if isinstance(v, tuple):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
    return rs, rr, cs


def _fake_model(out_dim):
    """Stands for a model handle of which only out_dim is read (the cost and termination heads' checks read it the same way):
    a block of ints with out_dim where csrc/ens_mlp_internal.h declares it."""
    src = open(os.path.join(ROOT, "constrained-model-based-policy-optimization_amd", "csrc", "ens_mlp_internal.h")).read()
    first = re.search(r"struct cmbpo_mlp \{\s*int ([^;]*);", src).group(1)
    ints = (C.c_int * 256)()
    ints[[n.strip() for n in first.split(",")].index("out_dim")] = out_dim
    return ints


def test_every_entry_refuses_bad_arguments_without_a_gpu(lib):
    model = _fake_model(14)
    fake = C.cast(model, C.c_void_p)

    def calls(rs, rr, cs=None, h=0, ens=7, d_elite=None):
        rc = C.byref(cs) if cs is not None else None
        return (("cmbpo_replay_reliab", lambda: lib.cmbpo_replay_reliab(C.byref(rs), C.byref(rr), h, None)),
                ("cmbpo_replay_reliab_finish", lambda: lib.cmbpo_replay_reliab_finish(C.byref(rs), C.byref(rr), None)),
                ("cmbpo_replay_run_reliab", lambda: lib.cmbpo_replay_run_reliab(C.byref(rs), rc, C.byref(rr), None, None, fake, 0, ens,
                                                                               d_elite, None)))

    def refused(name, call, *words):
        assert call() == -1, name
        msg = lib.cmbpo_last_error()
        assert name.encode() in msg, msg
        for w in words:
            assert w in msg, msg

    # the shape refusals of the compare call, in all three
    for bad, word in ((dict(B=0), b"B 0"), (dict(H=-1), b"H -1"), (dict(mode=2), b"unknown mode 2"), (dict(obs_dim=0), b"bad dims"),
                      (dict(reserved=1), b"reserved")):
        for name, call in calls(*_images(rp_kw=bad)[:2]):
            refused(name, call, word)
    # the reliability descriptor's own
    for bad, word in ((dict(n_bins=0), b"n_bins 0 outside [1, 32]"), (dict(n_bins=33), b"n_bins 33"), (dict(n_cols=0), b"n_cols 0 outside [1, 2]"),
                      (dict(n_cols=3), b"n_cols 3"), (dict(col=(0, -1)), b"col[0] -1 outside [0, out_dim = 14)"),
                      (dict(col=(1, 14)), b"col[1] 14"), (dict(target=(0, 2)), b"unknown target[0] 2"),
                      (dict(target=(1, -1)), b"unknown target[1] -1"), (dict(shift=(0, float("nan"))), b"shift[0] is not finite"),
                      (dict(shift=(1, float("inf"))), b"shift[1] is not finite"), (dict(reserved=3), b"reserved 3"),
                      (dict(ensemble=0), b"ensemble 0 outside [1, 8]"), (dict(ensemble=9), b"ensemble 9")):
        for name, call in calls(*_images(rr_kw=bad)[:2]):
            refused(name, call, word)
    # entries behind n_cols are ignored: a descriptor of one column with rubbish in the second slot passes its own checks
    rs, rr, _ = _images(rr_kw=dict(n_cols=1, col=(1, 99), target=(1, 7), shift=(1, float("nan"))))
    refused("cmbpo_replay_reliab", lambda: lib.cmbpo_replay_reliab(C.byref(rs), C.byref(rr), 3, None), b"h 3 outside [0, 3)")
    # NULL descriptors
    rs, rr, cs = _images()
    for name, call in (("cmbpo_replay_reliab", lambda: lib.cmbpo_replay_reliab(None, C.byref(rr), 0, None)),
                       ("cmbpo_replay_reliab", lambda: lib.cmbpo_replay_reliab(C.byref(rs), None, 0, None)),
                       ("cmbpo_replay_reliab_finish", lambda: lib.cmbpo_replay_reliab_finish(None, C.byref(rr), None)),
                       ("cmbpo_replay_reliab_finish", lambda: lib.cmbpo_replay_reliab_finish(C.byref(rs), None, None)),
                       ("cmbpo_replay_run_reliab", lambda: lib.cmbpo_replay_run_reliab(None, None, C.byref(rr), None, None, fake, 0, 7, None, None))):
        refused(name, call, b"NULL")
    # rr == NULL is cmbpo_replay_run_cost's call, under that entry's name rules (here: the plain run's, nothing else is given)
    assert lib.cmbpo_replay_run_reliab(C.byref(rs), None, None, None, None, None, 0, 7, None, None) == -1
    assert b"cmbpo_replay_run:" in lib.cmbpo_last_error() and b"model" in lib.cmbpo_last_error()
    # NULL arrays
    for k in ("next_obs", "rew", "cost", "term", "len", "cur_obs", "alive", "p_next_obs", "p_rew", "p_term", "p_cost", "p_dkl_path",
              "p_ep_var_mean", "part_sum", "part_cnt", "mean"):
        rs, rr, _ = _images(rp_kw={k: None})
        refused("cmbpo_replay_reliab", lambda: lib.cmbpo_replay_reliab(C.byref(rs), C.byref(rr), 0, None), b"NULL")
        refused("cmbpo_replay_run_reliab", calls(rs, rr)[2][1], b"NULL")
    for k in ("act", "var", "sums", "counts"):
        rs, rr, _ = _images(rp_kw={k: None})
        refused("cmbpo_replay_run_reliab", calls(rs, rr)[2][1], b"NULL")
    for k in ("elite", "edges", "part_sum", "part_cnt"):
        rs, rr, _ = _images(rr_kw={k: None})
        refused("cmbpo_replay_reliab", lambda: lib.cmbpo_replay_reliab(C.byref(rs), C.byref(rr), 0, None), b"NULL")
        refused("cmbpo_replay_run_reliab", calls(rs, rr)[2][1], b"NULL")
    for k in ("part_sum", "part_cnt", "sums", "counts"):
        rs, rr, _ = _images(rr_kw={k: None})
        refused("cmbpo_replay_reliab_finish", lambda: lib.cmbpo_replay_reliab_finish(C.byref(rs), C.byref(rr), None), b"NULL")
        refused("cmbpo_replay_run_reliab", calls(rs, rr)[2][1], b"NULL")
    # one bin has no edges, and the descriptor's own terminals are optional: neither NULL is refused (h is, behind them)
    rs, rr, _ = _images(rr_kw=dict(n_bins=1, edges=None, term=None))
    refused("cmbpo_replay_reliab", lambda: lib.cmbpo_replay_reliab(C.byref(rs), C.byref(rr), -1, None), b"h -1 outside [0, 3)")
    # h outside [0, H)
    rs, rr, cs = _images()
    for h in (-1, 3, 1 << 20):
        refused("cmbpo_replay_reliab", lambda: lib.cmbpo_replay_reliab(C.byref(rs), C.byref(rr), h, None), b"outside [0, 3)")
    # cmbpo_replay_run_reliab alone: the handle, the run's ensemble, the model's out_dim, the three elite arrays
    refused("cmbpo_replay_run_reliab", lambda: lib.cmbpo_replay_run_reliab(C.byref(rs), None, C.byref(rr), None, None, None, 0, 7, None, None),
            b"model")
    refused("cmbpo_replay_run_reliab", calls(rs, rr, ens=5)[2][1], b"ensemble 5, the reliability descriptor's is 7")
    rs2, rr2, _ = _images(rr_kw=dict(out_dim=15))
    refused("cmbpo_replay_run_reliab", calls(rs2, rr2)[2][1], b"out_dim 15 is not the model's 14")
    other = (C.c_int32 * 16)()
    refused("cmbpo_replay_run_reliab", calls(rs, rr, d_elite=C.cast(other, C.c_void_p))[2][1], b"d_elite differs from the reliability")
    rs3, rr3, cs3 = _images(rc_kw=dict(elite=C.cast(other, C.c_void_p).value))
    refused("cmbpo_replay_run_reliab", calls(rs3, rr3, cs3)[2][1], b"calibration descriptor's elite differs")
    refused("cmbpo_replay_run_reliab", calls(*_images(rc_kw=dict(ensemble=5))[:2], _images(rc_kw=dict(ensemble=5))[2])[2][1], b"ensemble 7")


# ------------------------------------------------------------------------------------------------------------------
# 5. FakeEnv, ModelSampler, CMBPO
# ------------------------------------------------------------------------------------------------------------------
def _fake_env(predicts_cost=True, predicts_term=True, **kw):
    """A FakeEnv up to its checks: a model stub, no device."""
    from toyworld import ToyEnv
    from cmbpo_amd.fake_env import FakeEnv
    env = ToyEnv()
    obs, act = int(np.prod(env.observation_space.shape)), int(np.prod(env.action_space.shape))

    class Model:
        is_ensemble = is_probabilistic = True
        in_dim, out_dim, device = obs + act, obs + 1 + int(predicts_cost) + int(predicts_term), "cpu"
    return FakeEnv(env, "default", Model(), True, True, predicts_cost, predicts_term=predicts_term, **kw)


def test_fake_env_columns_recalibration_and_refusals():
    both = _fake_env(cost_loss="logistic", cost_logit_shift=0.75, term_loss="logistic")
    assert both.reliability_columns() == [dict(name="cost", col=6, target="cost", shift=0.75),
                                          dict(name="term", col=7, target="term", shift=0.0)]
    assert _fake_env(cost_loss="logistic").reliability_columns() == [dict(name="cost", col=6, target="cost", shift=0.0)]
    assert _fake_env(predicts_cost=False, term_loss="logistic").reliability_columns() == [dict(name="term", col=6, target="term", shift=0.0)]
    for gaussian in (_fake_env(), _fake_env(predicts_cost=False, predicts_term=False)):
        with pytest.raises(ValueError, match="a Gaussian column is not a logit"):
            gaussian.reliability_columns()
        with pytest.raises(ValueError, match="a Gaussian column is not a logit"):      # replay() asks before it touches a device
            gaussian.replay(None, None, None, None, None, None, reliability=True)
    with pytest.raises(ValueError, match="reliability_terminals needs reliability=True"):
        both.replay(None, None, None, None, None, None, reliability_terminals=np.zeros((1, 1)))
    # the offset: the default hands over the old number itself, another one the float32 sum; the table's shift never moves
    assert both.cost_recalibration == 0.0 and both.cost_kernel_shift == 0.75 and both.cost_head_struct().logit_shift == 0.75
    both.set_cost_recalibration(0.1)
    want = float(F32(0.75 + 0.1))
    assert both.cost_kernel_shift == want and both.cost_head_struct().logit_shift == want and both.cost_logit_shift == 0.75
    assert both.reliability_columns()[0]["shift"] == 0.75
    both.set_cost_recalibration(-0.3)                                  # absolute, not accumulated
    assert both.cost_kernel_shift == float(F32(0.75 - 0.3))
    both.set_cost_recalibration(0.0)
    assert both.cost_head_struct().logit_shift == 0.75
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="set_cost_recalibration"):
            both.set_cost_recalibration(bad)
    g = _fake_env()
    g.set_cost_recalibration(0.0)
    with pytest.raises(ValueError, match="set_cost_recalibration needs cost_loss='logistic'"):
        g.set_cost_recalibration(0.5)


def test_model_sampler_offset_refusals():
    from cmbpo_amd.model_sampler import ModelSampler
    s = ModelSampler(5, batch_size=8, term_sampling=True)
    assert s.term_logit_offset is None
    s.set_term_logit_offset(0.0)
    s.set_term_logit_offset(None)
    assert s.term_logit_offset is None
    s.set_term_logit_offset(0.25)                                      # (no environment yet: checked again at initialize)
    assert s.term_logit_offset == 0.25
    with pytest.raises(ValueError, match="term_loss='logistic'"):
        s.initialize(_fake_env(), None, None)
    s.env = _fake_env(term_loss="logistic")
    s.set_term_logit_offset(-0.5)
    assert s.term_logit_offset == -0.5 and s._draws is None
    s.env = _fake_env()
    with pytest.raises(ValueError, match="a Gaussian termination column is not a logit"):
        s.set_term_logit_offset(0.5)
    assert s.term_logit_offset == -0.5                                 # a refusal changes nothing
    for bad in (float("nan"), float("-inf")):
        with pytest.raises(ValueError, match="finite"):
            s.set_term_logit_offset(bad)
    plain = ModelSampler(5, batch_size=8)
    plain.set_term_logit_offset(None)
    plain.set_term_logit_offset(0.0)
    with pytest.raises(ValueError, match="term_sampling=False"):
        plain.set_term_logit_offset(0.5)


def test_cmbpo_refuses_reliability_arguments_that_do_not_fit():
    """The checks come first in the constructor: nothing is built, nothing needs a device (or an environment)."""
    from cmbpo_amd.cmbpo import CMBPO
    make = lambda **kw: CMBPO(None, None, None, **kw)
    term = dict(m_learn_term=True, m_term_loss="logistic")
    cost = dict(m_learn_cost=True, m_cost_loss="logistic")
    with pytest.raises(ValueError, match="m_validate_reliability needs m_validate_horizon"):
        make(m_validate_reliability=True, **term)
    with pytest.raises(ValueError, match="m_validate_reliability needs m_validate_horizon"):
        make(m_validate_reliability=True, m_validate_horizon=5, use_model=False)
    with pytest.raises(ValueError, match="a Gaussian column is not a logit"):
        make(m_validate_reliability=True, m_validate_horizon=5)
    with pytest.raises(ValueError, match="a Gaussian column is not a logit"):
        make(m_validate_reliability=True, m_validate_horizon=5, m_learn_term=True, m_learn_cost=True)
    for bad in (0, 33, "many", None):
        with pytest.raises(ValueError, match="m_reliability_bins"):
            make(m_reliability_bins=bad)
    with pytest.raises(ValueError, match="m_recalibrate_cost needs m_validate_reliability=True and m_cost_loss='logistic'"):
        make(m_recalibrate_cost=True, m_validate_horizon=5, **cost)
    with pytest.raises(ValueError, match="m_recalibrate_cost needs"):
        make(m_recalibrate_cost=True, m_validate_reliability=True, m_validate_horizon=5, **term)
    with pytest.raises(ValueError, match="m_recalibrate_term needs m_validate_reliability=True, m_term_loss='logistic' and m_term_sampling=True"):
        make(m_recalibrate_term=True, m_validate_reliability=True, m_validate_horizon=5, **term)
    with pytest.raises(ValueError, match="m_recalibrate_term needs"):
        make(m_recalibrate_term=True, m_validate_horizon=5, m_term_sampling=True, **term)
    with pytest.raises(ValueError, match="m_recalibrate_term needs"):
        make(m_recalibrate_term=True, m_validate_reliability=True, m_validate_horizon=5, m_learn_term=True, m_term_sampling=True, **cost)
    for bad in ((1.0, -1.0), (-np.inf, 1.0), (0.0,), None, (0.0, np.nan)):
        with pytest.raises(ValueError, match="m_recalibration_range"):
            make(m_recalibration_range=bad)


def test_save_load_round_trip_of_the_recalibration_file(tmp_path):
    """`save` writes recalibration_<epoch>.json, a file of its own (the existing files keep exactly their keys); `load` hands
    the offsets to the environment and the sampler; a checkpoint without the file loads with offsets 0."""
    from cmbpo_amd.cmbpo import CMBPO
    from cmbpo_amd.model_sampler import ModelSampler

    class Model:
        def save(self, d, e):
            pass

        def load(self, d, e):
            pass

        def set_logistic_columns(self, cols):
            pass

        def set_column_weights(self, *a):
            pass

    def trainer(**kw):
        a = CMBPO.__new__(CMBPO)
        a._use_model, a._m_learn_term, a._m_learn_cost, a._epoch, a.obs_dim = True, True, True, 4, 5
        a._m_term_loss, a._m_cost_loss, a._m_term_sampling, a._validate_horizon = "logistic", "logistic", True, 3
        a._model, a.fake_env = Model(), _fake_env(cost_loss="logistic", cost_logit_shift=0.5, term_loss="logistic")
        a.model_sampler = ModelSampler(5, batch_size=8, term_sampling=True)
        a.model_sampler.env = a.fake_env
        a._column_weights = {"m_term_pos_weight": 1.0, "m_term_loss_weight": 1.0, "m_cost_loss_weight": 1.0, "m_pos_weight_max": 20.0}
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    a = trainer(_validate_reliability=True, _reliability_bins=10, _recalibrate_cost=True, _recalibrate_term=True,
                _recalibration_range=(-1.0, 1.5))
    a.fake_env.set_cost_recalibration(0.375)
    a.model_sampler.set_term_logit_offset(-0.625)
    a.save(str(tmp_path))
    assert json.load(open(tmp_path / "recalibration_4.json")) == {
        "m_validate_reliability": True, "m_reliability_bins": 10, "m_recalibrate_cost": True, "m_recalibrate_term": True,
        "m_recalibration_range": [-1.0, 1.5], "cost_recal_offset": 0.375, "term_recal_offset": -0.625}
    assert sorted(json.load(open(tmp_path / "recalibration_4.json"))) == sorted(CMBPO.RECALIBRATION_KEYS)
    # the files that were there keep their pinned keys
    assert sorted(json.load(open(tmp_path / "cost_loss_4.json"))) == ["cost_logit_shift", "m_cost_loss", "m_cost_pos_weight",
                                                                    "m_cost_pos_weight_undo"]
    assert json.load(open(tmp_path / "cost_loss_4.json"))["cost_logit_shift"] == 0.5       # the shift without the offset
    assert sorted(json.load(open(tmp_path / "term_head_4.json"))) == ["members", "threshold"]
    assert sorted(json.load(open(tmp_path / "term_sampling_4.json"))) == ["m_term_sampling"]
    b = trainer()
    assert (b._validate_reliability, b._recalibrate_cost, b.fake_env.cost_recalibration, b.model_sampler.term_logit_offset) == \
        (False, False, 0.0, None)
    b.load(str(tmp_path), 4)
    assert (b._validate_reliability, b._reliability_bins, b._recalibrate_cost, b._recalibrate_term) == (True, 10, True, True)
    assert b._recalibration_range == (-1.0, 1.5)
    assert b.fake_env.cost_recalibration == 0.375 and b.fake_env.cost_kernel_shift == float(F32(0.875))
    assert b.model_sampler.term_logit_offset == -0.625
    # a checkpoint from before the file: the switches stay, the offsets are 0
    os.remove(tmp_path / "recalibration_4.json")
    b.load(str(tmp_path), 4)
    assert (b._validate_reliability, b._recalibrate_cost) == (True, True)
    assert b.fake_env.cost_recalibration == 0.0 and b.fake_env.cost_head_struct().logit_shift == 0.5
    assert b.model_sampler.term_logit_offset is None
