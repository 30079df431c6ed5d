"""CPU: the inverse-variance-weighted GAE's checker (tests/iv_gae_ref.py) against calls of the reference's own
discount_cumsum(..., weights=...) recorded in tests/golden/g17_iv_cumsum.npz, the host's lambda tables, and the C-ABI
additions (header, ctypes image, argument checks) -- none of which needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import iv_gae_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "g17_iv_cumsum.npz"), allow_pickle=False)


def _cases(g):
    for L in g["Ls"]:
        for gi, (gam, lam) in enumerate(g["gl"]):
            for ei, eps in enumerate(g["eps"]):
                for tag in ("32", "64"):
                    yield int(L), gi, float(gam), float(lam), ei, float(eps), tag


def test_restatement_equals_the_reference_bit_for_bit(gold):
    n = 0
    for L, gi, gam, lam, ei, eps, tag in _cases(gold):
        x, var = gold[f"L{L}_x{tag}"], gold[f"L{L}_var"]
        assert x.dtype == (np.float32 if tag == "32" else np.float64) and var.dtype == np.float32
        assert (var == 0).any() or L < 3
        want = gold[f"L{L}_g{gi}_e{ei}_y{tag}"]
        got = ref.iv_discount_cumsum(x, gam, lam, ref.iv_weights(var, eps))
        assert got.dtype == np.float64 and want.dtype == np.float64
        np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64), err_msg=f"L={L} g{gi} e{ei} x{tag}")
        n += 1
    assert n == 5 * 2 * 2 * 2


def test_length_one_returns_the_deltas(gold):
    """L = 1: out = (x * lw) / lw, two roundings -- within one float64 ulp of x, so a float32 x comes back exactly once the
    result is stored as float32 (the buffers' type)."""
    rng = np.random.default_rng(3)
    x32 = rng.standard_normal((64, 1)).astype(np.float32)
    w = ref.iv_weights(gold["L1_var"].repeat(4, axis=0), 1e-8)
    out = ref.iv_discount_cumsum(x32, 0.99, 0.95, w)
    np.testing.assert_array_equal(out.astype(np.float32), x32)
    x64 = rng.standard_normal((64, 1))
    np.testing.assert_allclose(ref.iv_discount_cumsum(x64, 0.97, 0.5, w), x64, rtol=2.0 ** -52, atol=0)
    for gi in (0, 1):
        np.testing.assert_array_equal(gold[f"L1_g{gi}_e0_y32"].astype(np.float32), gold["L1_x32"])


def test_a_common_factor_of_the_weights_changes_nothing_and_constant_weights_are_not_plain_gae(gold):
    from oracle import refcpu
    x, var = gold["L7_x64"], gold["L7_var"]
    w = ref.iv_weights(var, 1e-8)
    base = ref.iv_discount_cumsum(x, 0.99, 0.95, w)
    for c in (2.0, 2.0 ** -30, 2.0 ** 40):            # powers of two: every intermediate scales exactly
        np.testing.assert_array_equal(ref.iv_discount_cumsum(x, 0.99, 0.95, c * w), base)
    np.testing.assert_allclose(ref.iv_discount_cumsum(x, 0.99, 0.95, 3.7 * w), base, rtol=1e-13, atol=1e-15)
    # constant weights: the same whatever the constant ...
    one = ref.iv_discount_cumsum(x, 0.99, 0.95, np.ones_like(w))
    np.testing.assert_allclose(ref.iv_discount_cumsum(x, 0.99, 0.95, np.full_like(w, 123.0)), one, rtol=1e-13, atol=1e-15)
    # ... but not GAE(lambda): the reference gives the last step lam^L where GAE's geometric tail sums to lam^(L-1)
    plain = refcpu.discount_cumsum(x, 0.99, 0.95)
    rel = np.abs(one - plain).max() / np.abs(plain).max()
    assert 1e-3 < rel < 0.2, rel
    np.testing.assert_array_equal(one[:, -1:].astype(np.float32), plain[:, -1:].astype(np.float32))   # the last step has one term


def test_the_package_builds_the_recorded_tables(gold):
    from cmbpo_amd.modelbuffer import iv_tables
    T = int(gold["table_T"])
    for gi, (_, lam) in enumerate(gold["gl"]):
        vec, pw = iv_tables(float(lam), T)
        assert vec.dtype == np.float64 and pw.dtype == np.float64 and vec.shape == (T,) and pw.shape == (T + 1,)
        np.testing.assert_array_equal(vec, gold[f"lam_vec_g{gi}"])       # lfilter's recurrence
        np.testing.assert_array_equal(pw, gold[f"lam_pow_g{gi}"])        # Python's pow
        rvec, rpw = ref.lam_tables(float(lam), T)
        np.testing.assert_array_equal(vec, rvec)
        np.testing.assert_array_equal(pw, rpw)


def _header():
    text = open(os.path.join(ROOT, "include", "cmbpo_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_signatures_and_struct_image_agree():
    from cmbpo_amd import _lib
    text = _header()
    m = re.search(r"typedef struct cmbpo_iv_gae \{(.*?)\} cmbpo_iv_gae_t;", text, flags=re.S)
    assert m, "cmbpo_iv_gae_t is not declared"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        kind = "double" if "*" not in decl else "pointer"
        names = re.sub(r"^(const\s+)?double", "", decl)
        fields += [(n.strip().lstrip("*").strip(), kind) for n in names.split(",")]
    assert fields == [("cumvar_buf", "pointer"), ("lam_vec", "pointer"), ("lam_pow", "pointer"), ("clam_vec", "pointer"),
                      ("clam_pow", "pointer"), ("eps", "double")]
    image = [(n, "pointer" if t is C.c_void_p else "double" if t is C.c_double else "?") for n, t in _lib.IvGaeStruct._fields_]
    assert image == fields
    assert C.sizeof(_lib.IvGaeStruct) == 48 and _lib.IvGaeStruct.eps.offset == 40
    assert re.search(r"int cmbpo_rollout_iv_attach\(const cmbpo_rollout_t \*r, const cmbpo_iv_gae_t \*iv\);", text)
    assert re.search(r"int cmbpo_rollout_iv_detach\(const cmbpo_rollout_t \*r\);", text)
    rp = C.POINTER(_lib.RolloutStruct)
    assert _lib.SIGNATURES["cmbpo_rollout_iv_attach"] == (C.c_int, [rp, C.POINTER(_lib.IvGaeStruct)])
    assert _lib.SIGNATURES["cmbpo_rollout_iv_detach"] == (C.c_int, [rp])


def test_rollout_struct_is_unchanged():
    from cmbpo_amd import _lib
    names = [f[0] for f in _lib.RolloutStruct._fields_]
    assert names[-2:] == ["xi", "xi_stride"] and len(names) == 60 and C.sizeof(_lib.RolloutStruct) == 440
    assert not any(n.startswith("iv") or "cumvar" in n or "lam_" in n for n in names)
    m = re.search(r"typedef struct cmbpo_rollout \{(.*?)\} cmbpo_rollout_t;", _header(), flags=re.S)
    assert m and "cumvar" not in m.group(1) and m.group(1).rstrip().endswith("int64_t xi_stride;")


def test_attach_rejects_bad_arguments_without_a_gpu():
    import __graft_entry__ as g
    g.build()
    from cmbpo_amd import _lib
    lib = _lib.lib()
    assert lib.cmbpo_version() >= 4
    host = (C.c_double * 8)()                  # never dereferenced: attach only records the pointers
    p = C.cast(host, C.c_void_p).value
    rs = _lib.RolloutStruct()
    who = b"cmbpo_rollout_iv_attach"

    def image(**kw):
        iv = _lib.IvGaeStruct()
        for n in ("cumvar_buf", "lam_vec", "lam_pow", "clam_vec", "clam_pow"):
            setattr(iv, n, p)
        iv.eps = 1e-8
        for k, v in kw.items():
            setattr(iv, k, v)
        return iv

    assert lib.cmbpo_rollout_iv_attach(C.byref(rs), C.byref(image())) == -1 and who in lib.cmbpo_last_error()   # NULL iscal
    assert lib.cmbpo_rollout_iv_detach(C.byref(rs)) == -1 and b"cmbpo_rollout_iv_detach" in lib.cmbpo_last_error()
    rs.iscal = p
    assert lib.cmbpo_rollout_iv_attach(C.byref(rs), None) == -1 and who in lib.cmbpo_last_error()
    for n in ("cumvar_buf", "lam_vec", "lam_pow", "clam_vec", "clam_pow"):
        assert lib.cmbpo_rollout_iv_attach(C.byref(rs), C.byref(image(**{n: None}))) == -1
        assert who in lib.cmbpo_last_error() and b"NULL" in lib.cmbpo_last_error()
    for eps in (0.0, -1e-8, float("inf"), float("nan")):
        assert lib.cmbpo_rollout_iv_attach(C.byref(rs), C.byref(image(eps=eps))) == -1
        assert who in lib.cmbpo_last_error() and b"eps" in lib.cmbpo_last_error()
    assert lib.cmbpo_rollout_iv_attach(C.byref(rs), C.byref(image())) == 0
    assert lib.cmbpo_rollout_iv_attach(C.byref(rs), C.byref(image(eps=1e-2))) == 0       # attaching again replaces the entry
    assert lib.cmbpo_rollout_iv_detach(C.byref(rs)) == 0
    assert lib.cmbpo_rollout_iv_detach(C.byref(rs)) == 0                                  # nothing attached: not an error
