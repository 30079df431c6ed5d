"""CPU: the C-ABI of the ensemble disagreement on reward / cost -- the library exports the three new symbols, header and
binding agree, the argument checks of cmbpo_fakeenv_post_disagreement and cmbpo_rollout_disagreement_attach precede any HIP
call (-1 with a message naming the entry point), and cmbpo_rollout_t is what it was."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = b"cmbpo_fakeenv_post_disagreement"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cmbpo_amd import _lib
    return _lib.lib()


def _header():
    text = open(os.path.join(ROOT, "include", "cmbpo_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _post(lib, task, ensemble, obs_dim, act_dim, buffers=None, n_rows=0, ld_rows=0, kr=0.0, kc=0.0, xi=None, outs="both"):
    from cmbpo_amd import _lib
    b = buffers or [None] * 10       # mean, var, obs, elite, next_obs, rew, term, cost, dkl_path, ep_var_mean
    host = (C.c_float * 64)()        # never dereferenced: every call fails its checks (or has no rows) first
    p = C.cast(host, C.c_void_p)
    rv = p if outs in ("both", "rew") else None
    cv = p if outs in ("both", "cost") else None
    return lib.cmbpo_fakeenv_post_disagreement(task, ensemble, obs_dim, act_dim, b[0], b[1], ld_rows, b[2], None, b[3], None, None,
                                               n_rows, b[4], b[5], b[6], b[7], b[8], b[9], None, xi, kr, kc, rv, cv, None)


def test_library_exports_the_new_symbols(lib):
    from cmbpo_amd import _lib
    assert lib.cmbpo_version() >= 5
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("cmbpo_fakeenv_post_disagreement", "cmbpo_rollout_disagreement_attach", "cmbpo_rollout_disagreement_detach"):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
    assert (_lib.D_TOTAL_REW_VAR, _lib.D_TOTAL_COST_VAR) == (13, 14)
    text = _header()
    assert re.search(r"#define CMBPO_D_TOTAL_REW_VAR 13\b", text) and re.search(r"#define CMBPO_D_TOTAL_COST_VAR 14\b", text)


def test_header_signatures_and_struct_image_agree():
    from cmbpo_amd import _lib
    text = _header()
    m = re.search(r"typedef struct cmbpo_disagreement \{(.*?)\} cmbpo_disagreement_t;", text, flags=re.S)
    assert m, "cmbpo_disagreement_t is not declared"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        kind = "pointer" if "*" in decl else "float"
        names = re.sub(r"^(float|double)", "", decl)
        fields += [(n.strip().lstrip("*").strip(), kind) for n in names.split(",")]
    assert fields == [("kappa_rew", "float"), ("kappa_cost", "float"), ("rew_var_t", "pointer"), ("cost_var_t", "pointer"),
                      ("path_rew_var", "pointer"), ("path_cost_var", "pointer"), ("part", "pointer")]
    image = [(n, "pointer" if t is C.c_void_p else "float" if t is C.c_float else "?") for n, t in _lib.DisagreementStruct._fields_]
    assert image == fields
    assert C.sizeof(_lib.DisagreementStruct) == 48 and _lib.DisagreementStruct.rew_var_t.offset == 8
    assert re.search(r"int cmbpo_rollout_disagreement_attach\(const cmbpo_rollout_t \*r, const cmbpo_disagreement_t \*dg\);", text)
    assert re.search(r"int cmbpo_rollout_disagreement_detach\(const cmbpo_rollout_t \*r\);", text)
    rp = C.POINTER(_lib.RolloutStruct)
    assert _lib.SIGNATURES["cmbpo_rollout_disagreement_attach"] == (C.c_int, [rp, C.POINTER(_lib.DisagreementStruct)])
    assert _lib.SIGNATURES["cmbpo_rollout_disagreement_detach"] == (C.c_int, [rp])
    # the post entry point: cmbpo_fakeenv_post_noise's arguments, then kappa_rew, kappa_cost, d_rew_var, d_cost_var, stream
    noise = _lib.SIGNATURES["cmbpo_fakeenv_post_noise"]
    dis = _lib.SIGNATURES["cmbpo_fakeenv_post_disagreement"]
    assert dis[0] is C.c_int and dis[1] == noise[1][:-1] + [C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    m = re.search(r"int cmbpo_fakeenv_post_disagreement\((.*?)\);", text, flags=re.S)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == len(dis[1])
    assert args[-5:] == ["float kappa_rew", "float kappa_cost", "float *d_rew_var", "float *d_cost_var", "void *stream"]
    assert args[-6] == "const float *d_xi"


def test_rollout_struct_is_unchanged():
    from cmbpo_amd import _lib
    names = [f[0] for f in _lib.RolloutStruct._fields_]
    assert names[-2:] == ["xi", "xi_stride"] and len(names) == 60 and C.sizeof(_lib.RolloutStruct) == 440
    assert not any("var" in n and n != "path_dyn_var" or "kappa" in n for n in names)
    m = re.search(r"typedef struct cmbpo_rollout \{(.*?)\} cmbpo_rollout_t;", _header(), flags=re.S)
    assert m and "kappa" not in m.group(1) and "rew_var" not in m.group(1) and m.group(1).rstrip().endswith("int64_t xi_stride;")


def test_post_disagreement_rejects_bad_arguments_without_a_gpu(lib):
    from cmbpo_amd import _lib
    host = (C.c_float * 64)()
    p = C.cast(host, C.c_void_p)
    F = _lib.TASK_LEARNED_COST
    for xi in (None, p):                    # d_xi may be NULL: the entry point keeps its own checks and its own name
        for task in (9, 3, -1, _lib.TASK_ANTSAFE | 0x200, _lib.TASK_USER_BASE + _lib.TASK_USER_SLOTS):
            assert _post(lib, task, 7, 29, 8, xi=xi) == -1
            msg = lib.cmbpo_last_error()
            assert WHO in msg and (b"bad task" in msg or b"not registered" in msg), msg
        for E in (1, 9):
            assert _post(lib, _lib.TASK_HCS, E, 18, 6, xi=xi) == -1
            assert WHO in lib.cmbpo_last_error() and b"ensemble" in lib.cmbpo_last_error()
        for obs_dim, act_dim in ((0, 6), (513, 6), (18, -1)):
            assert _post(lib, _lib.TASK_HCS, 7, obs_dim, act_dim, xi=xi) == -1
            assert WHO in lib.cmbpo_last_error() and b"bad dims" in lib.cmbpo_last_error()
        assert _post(lib, _lib.TASK_ANTSAFE, 7, 4, 2, xi=xi) == -1
        assert WHO in lib.cmbpo_last_error() and b"obs_dim >= 5" in lib.cmbpo_last_error()
        # NULL buffers: all of them, each of the ten required ones in turn, each of the two new outputs
        assert _post(lib, _lib.TASK_DEFAULT, 7, 11, 3, xi=xi) == -1
        assert WHO in lib.cmbpo_last_error() and b"NULL buffer" in lib.cmbpo_last_error()
        for k in range(10):
            bufs = [p] * 10
            bufs[k] = None
            assert _post(lib, _lib.TASK_DEFAULT | F, 7, 11, 3, bufs, xi=xi) == -1
            assert WHO in lib.cmbpo_last_error() and b"NULL buffer" in lib.cmbpo_last_error()
        for outs in ("rew", "cost", "none"):
            assert _post(lib, _lib.TASK_DEFAULT | F, 7, 11, 3, [p] * 10, xi=xi, outs=outs) == -1
            assert WHO in lib.cmbpo_last_error() and b"NULL buffer" in lib.cmbpo_last_error()
        # the coefficients: finite and >= 0, each of the two
        for bad in (-1e-3, -0.5, float("nan"), float("inf"), float("-inf")):
            assert _post(lib, _lib.TASK_DEFAULT | F, 7, 11, 3, [p] * 10, xi=xi, kr=bad) == -1
            assert WHO in lib.cmbpo_last_error() and b"kappa_rew" in lib.cmbpo_last_error()
            assert _post(lib, _lib.TASK_DEFAULT | F, 7, 11, 3, [p] * 10, xi=xi, kc=bad) == -1
            assert WHO in lib.cmbpo_last_error() and b"kappa_cost" in lib.cmbpo_last_error()
        # a pessimistic cost needs the learned cost head
        for task in (_lib.TASK_DEFAULT, _lib.TASK_HCS, _lib.TASK_ANTSAFE):
            assert _post(lib, task, 7, 11, 3, [p] * 10, xi=xi, kc=0.5) == -1
            msg = lib.cmbpo_last_error()
            assert WHO in msg and b"kappa_cost" in msg and b"CMBPO_TASK_LEARNED_COST" in msg, msg
        assert _post(lib, _lib.TASK_DEFAULT, 7, 11, 3, [p] * 10, n_rows=5, ld_rows=4, xi=xi) == -1
        assert WHO in lib.cmbpo_last_error() and b"ld_rows" in lib.cmbpo_last_error()
        # no rows: nothing to launch -- with and without the flag, with every legal coefficient
        assert _post(lib, _lib.TASK_DEFAULT, 7, 11, 3, [p] * 10, xi=xi, kr=0.5) == 0
        assert _post(lib, _lib.TASK_ANTSAFE | F, 7, 11, 3, [p] * 10, xi=xi, kr=0.5, kc=2.0) == 0
        assert _post(lib, _lib.TASK_HCS, 3, 11, 3, [p] * 10, xi=xi) == 0


def test_attach_rejects_bad_arguments_without_a_gpu(lib):
    from cmbpo_amd import _lib
    host = (C.c_double * 8)()                  # never dereferenced: attach only records the pointers
    p = C.cast(host, C.c_void_p).value
    rs = _lib.RolloutStruct()
    who = b"cmbpo_rollout_disagreement_attach"
    names = ("rew_var_t", "cost_var_t", "path_rew_var", "path_cost_var", "part")

    def image(**kw):
        dg = _lib.DisagreementStruct()
        for n in names:
            setattr(dg, n, p)
        dg.kappa_rew, dg.kappa_cost = 0.5, 0.0
        for k, v in kw.items():
            setattr(dg, k, v)
        return dg

    assert lib.cmbpo_rollout_disagreement_attach(C.byref(rs), C.byref(image())) == -1 and who in lib.cmbpo_last_error()   # NULL iscal
    assert lib.cmbpo_rollout_disagreement_detach(C.byref(rs)) == -1
    assert b"cmbpo_rollout_disagreement_detach" in lib.cmbpo_last_error()
    assert lib.cmbpo_rollout_disagreement_attach(None, C.byref(image())) == -1 and who in lib.cmbpo_last_error()
    rs.iscal = p
    assert lib.cmbpo_rollout_disagreement_detach(C.byref(rs)) == 0                 # never attached: not an error
    assert lib.cmbpo_rollout_disagreement_attach(C.byref(rs), None) == -1 and who in lib.cmbpo_last_error()
    for n in names:
        assert lib.cmbpo_rollout_disagreement_attach(C.byref(rs), C.byref(image(**{n: None}))) == -1
        assert who in lib.cmbpo_last_error() and b"NULL" in lib.cmbpo_last_error()
    for bad in (-1.0, float("nan"), float("inf")):
        for k in ("kappa_rew", "kappa_cost"):
            assert lib.cmbpo_rollout_disagreement_attach(C.byref(rs), C.byref(image(**{k: bad}))) == -1
            assert who in lib.cmbpo_last_error() and b"kappa" in lib.cmbpo_last_error()
    assert lib.cmbpo_rollout_disagreement_attach(C.byref(rs), C.byref(image())) == 0
    assert lib.cmbpo_rollout_disagreement_attach(C.byref(rs), C.byref(image(kappa_rew=0.0))) == 0     # replaces the entry
    assert lib.cmbpo_rollout_disagreement_detach(C.byref(rs)) == 0
    assert lib.cmbpo_rollout_disagreement_detach(C.byref(rs)) == 0
