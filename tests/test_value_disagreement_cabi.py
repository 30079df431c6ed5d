"""CPU: the C-ABI of the critics' disagreement -- the library exports the three new symbols, header and
binding agree, cmbpo_value_disagreement_t has the layout the binding gives it, and the argument checks of
cmbpo_critic_pair_predict_var and cmbpo_rollout_value_disagreement_attach that need no network handle precede any HIP call (-1
with a message naming the entry point).  The checks that need a loaded handle are in tests/test_value_disagreement_gpu.py."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHO = b"cmbpo_critic_pair_predict_var"
NEW = ("cmbpo_critic_pair_predict_var", "cmbpo_rollout_value_disagreement_attach", "cmbpo_rollout_value_disagreement_detach")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cmbpo_amd import _lib
    return _lib.lib()


def _header():
    text = open(os.path.join(ROOT, "include", "cmbpo_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_library_exports_the_new_symbols(lib):
    from cmbpo_amd import _lib
    assert lib.cmbpo_version() >= 6          # (additions only: the new entries are asked for by name below)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
    assert (_lib.D_TOTAL_V_VAR, _lib.D_TOTAL_VC_VAR) == (15, 16)
    text = _header()
    assert re.search(r"#define CMBPO_D_TOTAL_V_VAR 15\b", text) and re.search(r"#define CMBPO_D_TOTAL_VC_VAR 16\b", text)
    # the two slots were free: no other dscal slot has their numbers
    slots = re.findall(r"#define (CMBPO_D_\w+) (\d+)\b", text)
    assert sorted(int(n) for _, n in slots) == list(range(len(slots)))


def test_header_signatures_and_struct_image_agree():
    from cmbpo_amd import _lib
    text = _header()
    m = re.search(r"typedef struct cmbpo_value_disagreement \{(.*?)\} cmbpo_value_disagreement_t;", text, flags=re.S)
    assert m, "cmbpo_value_disagreement_t is not declared"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        kind = "pointer" if "*" in decl else "float"
        names = re.sub(r"^(float|double)", "", decl)
        fields += [(n.strip().lstrip("*").strip(), kind) for n in names.split(",")]
    assert fields == [("kappa_v", "float"), ("kappa_vc", "float"), ("v_var", "pointer"), ("vc_var", "pointer"), ("part", "pointer")]
    S = _lib.ValueDisagreementStruct
    image = [(n, "pointer" if t is C.c_void_p else "float" if t is C.c_float else "?") for n, t in S._fields_]
    assert image == fields
    assert C.sizeof(S) == 32 and (S.kappa_v.offset, S.kappa_vc.offset, S.v_var.offset, S.vc_var.offset, S.part.offset) == (0, 4, 8, 16, 24)
    assert re.search(r"int cmbpo_rollout_value_disagreement_attach\(const cmbpo_rollout_t \*r, const cmbpo_value_disagreement_t \*vd\);", text)
    assert re.search(r"int cmbpo_rollout_value_disagreement_detach\(const cmbpo_rollout_t \*r\);", text)
    rp = C.POINTER(_lib.RolloutStruct)
    assert _lib.SIGNATURES["cmbpo_rollout_value_disagreement_attach"] == (C.c_int, [rp, C.POINTER(S)])
    assert _lib.SIGNATURES["cmbpo_rollout_value_disagreement_detach"] == (C.c_int, [rp])
    # the new critic entry: the plain entry's arguments with kappa_v, kappa_vc in front of the outputs and the two variances behind
    plain = _lib.SIGNATURES["cmbpo_critic_pair_predict"]
    var = _lib.SIGNATURES["cmbpo_critic_pair_predict_var"]
    assert var[0] is C.c_int and var[1] == plain[1][:7] + [C.c_float, C.c_float] + plain[1][7:9] + [C.c_void_p, C.c_void_p] + plain[1][9:]
    m = re.search(r"int cmbpo_critic_pair_predict_var\((.*?)\);", text, flags=re.S)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == len(var[1]) == 14
    assert args[6:] == ["int n_rows", "float kappa_v", "float kappa_vc", "float *d_v", "float *d_vc", "float *d_v_var",
                        "float *d_vc_var", "void *stream"]
    mp = re.search(r"int cmbpo_critic_pair_predict\((.*?)\);", text, flags=re.S)
    assert [a.strip() for a in mp.group(1).split(",")][:7] == args[:7]


def test_rollout_struct_is_unchanged():
    from cmbpo_amd import _lib
    names = [f[0] for f in _lib.RolloutStruct._fields_]
    assert names[-2:] == ["xi", "xi_stride"] and len(names) == 60 and C.sizeof(_lib.RolloutStruct) == 440
    assert not any(n in ("v_var", "vc_var", "kappa_v", "kappa_vc") for n in names)


def test_predict_var_rejects_bad_arguments_without_a_gpu(lib):
    host = (C.c_float * 64)()           # stands in for every pointer: each call below is refused before anything is read
    p = C.cast(host, C.c_void_p)

    def call(v=p, vc=p, obs=p, n=5, kv=0.0, kc=0.0, dv=p, dvc=p, vv=p, vcv=p):
        return lib.cmbpo_critic_pair_predict_var(v, vc, obs, 29, None, None, n, kv, kc, dv, dvc, vv, vcv, None)

    for kw in (dict(v=None), dict(vc=None), dict(obs=None), dict(dv=None), dict(dvc=None)):
        assert call(**kw) == -1
        assert WHO in lib.cmbpo_last_error() and b"NULL argument" in lib.cmbpo_last_error()
    for kw in (dict(vv=None), dict(vcv=None), dict(vv=None, vcv=None)):
        assert call(**kw) == -1
        assert WHO in lib.cmbpo_last_error() and b"NULL variance output" in lib.cmbpo_last_error()
    for bad in (-1e-3, -0.5, float("nan"), float("inf"), float("-inf")):
        for kw in (dict(kv=bad), dict(kc=bad), dict(kv=bad, kc=1.0)):
            assert call(**kw) == -1
            assert WHO in lib.cmbpo_last_error() and b"kappa" in lib.cmbpo_last_error()
    assert call(n=-1) == -1
    assert WHO in lib.cmbpo_last_error() and b"n_rows" in lib.cmbpo_last_error()
    # the plain entry keeps its own name
    assert lib.cmbpo_critic_pair_predict(None, p, p, 29, None, None, 5, p, p, None) == -1
    assert b"cmbpo_critic_pair_predict:" in lib.cmbpo_last_error()


def test_attach_rejects_bad_arguments_without_a_gpu(lib):
    from cmbpo_amd import _lib
    host = (C.c_double * 8)()                  # never dereferenced: attach only records the pointers
    p = C.cast(host, C.c_void_p).value
    rs = _lib.RolloutStruct()
    who = b"cmbpo_rollout_value_disagreement_attach"
    names = ("v_var", "vc_var", "part")

    def image(**kw):
        vd = _lib.ValueDisagreementStruct()
        for n in names:
            setattr(vd, n, p)
        vd.kappa_v, vd.kappa_vc = 0.0, 0.5
        for k, v in kw.items():
            setattr(vd, k, v)
        return vd

    attach, detach = lib.cmbpo_rollout_value_disagreement_attach, lib.cmbpo_rollout_value_disagreement_detach
    assert attach(C.byref(rs), C.byref(image())) == -1 and who in lib.cmbpo_last_error()   # NULL iscal
    assert detach(C.byref(rs)) == -1
    assert b"cmbpo_rollout_value_disagreement_detach" in lib.cmbpo_last_error()
    assert attach(None, C.byref(image())) == -1 and who in lib.cmbpo_last_error()
    rs.iscal = p
    assert detach(C.byref(rs)) == 0                 # never attached: not an error
    assert attach(C.byref(rs), None) == -1 and who in lib.cmbpo_last_error()
    for n in names:
        assert attach(C.byref(rs), C.byref(image(**{n: None}))) == -1
        assert who in lib.cmbpo_last_error() and b"NULL" in lib.cmbpo_last_error()
    for bad in (-1.0, float("nan"), float("inf")):
        for k in ("kappa_v", "kappa_vc"):
            assert attach(C.byref(rs), C.byref(image(**{k: bad}))) == -1
            assert who in lib.cmbpo_last_error() and b"kappa" in lib.cmbpo_last_error()
    assert attach(C.byref(rs), C.byref(image())) == 0
    assert attach(C.byref(rs), C.byref(image(kappa_vc=0.0))) == 0     # replaces the entry
    # the three features share one table entry: detaching one leaves the others
    dg = _lib.DisagreementStruct()
    for n in ("rew_var_t", "cost_var_t", "path_rew_var", "path_cost_var", "part"):
        setattr(dg, n, p)
    assert lib.cmbpo_rollout_disagreement_attach(C.byref(rs), C.byref(dg)) == 0
    assert detach(C.byref(rs)) == 0
    assert detach(C.byref(rs)) == 0
    assert lib.cmbpo_rollout_disagreement_detach(C.byref(rs)) == 0
