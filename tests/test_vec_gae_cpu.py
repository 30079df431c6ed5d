"""CPU: the restatements of tests/vec_gae_ref.py against the recorded reference and the oracle, and the proof that the bounds of
the GPU tests (tests/test_gae_segments_gpu.py, tests/test_vec_ops_gpu.py) reject a wrong kernel.

* `gae_segments` + `adv_normalize64` on golden G8 (recorded from the reference's CPOBuffer): ret / cret bit for bit, the
  normalised advantages within the adv / cadv bounds (measured: adv 2.2e-7 at most, the golden being float32 arithmetic).
* ten `cg_step64` against ten iterations of oracle/refupdate.cg on a dense SPD operator, rtol 1e-12.
* each defect of `vec_gae_ref.DEFECTS`, applied to the emulations on exactly the GPU cases' inputs, leaves its bound by a factor
  of 4 or more on at least one case, and the undamaged emulation stays below half of every bound on all of them.
"""
import os

import numpy as np
import pytest

import vec_gae_ref as V

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32, F64 = np.float32, np.float64


def test_restatement_reproduces_the_recorded_cpobuffer():
    g = np.load(os.path.join(GOLD, "g8_cpobuffer.npz"), allow_pickle=False)
    offs = np.concatenate([[0], np.cumsum(g["lengths"])])
    mask = g["zero_val"].astype(np.uint8)                       # a float64-zero reward bootstrap: bit 0; the cost's is float32
    last_val = np.where(g["zero_val"], F32(0), g["last_val"]).astype(F32)
    adv, ret, cadv, cret = V.gae_segments(offs, g["rew"], g["val"], g["cost"], g["cval"], last_val, g["last_cval"], mask,
                                          0.99, 0.95, 0.97, 0.5)
    np.testing.assert_array_equal(ret, g["get_ret"])
    np.testing.assert_array_equal(cret, g["get_cret"])
    ref = V.adv_normalize64(adv, cadv)
    got = dict(adv=g["get_adv"], cadv=g["get_cadv"])
    fa = V.frac(np.abs(got["adv"].astype(F64) - ref["adv"]), V.bound_adv(ref))
    fc = V.frac(np.abs(got["cadv"].astype(F64) - ref["cadv"]), V.bound_cadv(ref))
    print("G8: adv %.3f, cadv %.3f of the bound; max |adv - adv64| %.3g" % (fa, fc, np.abs(got["adv"] - ref["adv"]).max()))
    assert fa <= 1.0 and fc <= 1.0, (fa, fc)
    # and the emulation of the kernel's order
    emu = V.adv_normalize64(adv, cadv, emulate=True)
    f = V.norm_fractions(emu, ref)
    assert max(f.values()) <= 1.0, f


def test_ten_cg_step64_are_the_oracles_cg():
    from oracle import refupdate
    for P in (63, 65):
        op = V.dense_operator(P)
        want = op.figures()["x64"]
        b = op.b.astype(F64)
        x, r, p, rr = np.zeros(P), b.copy(), b.copy(), float(np.dot(b, b))
        for _ in range(V.CG_ITERS):
            s = V.cg_step64(V.CG_N * op.gram64(p), V.CG_INV_N, V.CG_DAMPING, x, r, p, rr)
            x, r, p, rr = s["x"], s["r"], s["p"], s["rr"]
        np.testing.assert_allclose(x, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
        # (the operator is well posed: ten iterations have not converged to rounding, and the float32 run errs visibly)
        assert 1e-8 < op.figures()["e32"] < 1e-3
        assert refupdate.cg(op.A64, b, 3).dtype == F64


# ---------------------------------------------------------------------------------------------------------------------------
# The bounds on the GPU cases' inputs: {quantity: worst fraction of its bound over the cases}, clean and under each defect
# ---------------------------------------------------------------------------------------------------------------------------
def _worst(acc, f):
    for k, v in f.items():
        acc[k] = max(acc.get(k, 0.0), float(v))


_MEMO = {}


def _dots(defect):
    """the dot products of every dots launch and of every single cg step (alpha, beta, float32(r.r)) on the GPU cases' inputs"""
    if ("dots", defect) in _MEMO:
        return _MEMO[("dots", defect)]
    acc = {}
    for P in V.VEC_SMALL:
        for fam in V.VEC_FAMILIES:
            vs = V.dots_case(P, fam)
            for k, (i, j) in enumerate(V.DOT_PAIRS):
                s64, sabs = V.dots64(vs[i], vs[j])
                _worst(acc, {"dots": V.frac(abs(V.dot_emul(vs[i], vs[j], defect) - s64), V.bound_dot(P, sabs))})
            c = V.cg_step_case(P, fam)
            emu = V.cg_step64(c["hp_sum"], V.CG_INV_N, V.CG_DAMPING, c["x"], c["r"], c["p"], c["rr"], emulate=True)
            bad = V.cg_step64(c["hp_sum"], V.CG_INV_N, V.CG_DAMPING, c["x"], c["r"], c["p"], c["rr"], emulate=True,
                              dot=lambda a, b: V.dot_emul(a, b, defect))
            f = V.cg_step_fractions(dict(x=bad["x"], r=bad["r"], p=bad["p"], rr=bad["rr"], alpha=bad["alpha"]), c, emu)
            if defect is not None:      # the device's r.r is held to the r it returned: damage shows there too
                f["rr"] = float(V.ulps(bad["rr"], F32(V.dots64(bad["r"], bad["r"])[0])))
            _worst(acc, {"cg_" + k: v for k, v in f.items()})
    _MEMO[("dots", defect)] = acc
    return acc


def _gae(defect):
    """elements that differ from the undamaged restatement, per output, at most over the layouts and parameter sets"""
    if ("gae", defect) in _MEMO:
        return _MEMO[("gae", defect)]
    acc = {}
    for n_paths, variant in V.GAE_LAYOUTS:
        c = V.gae_case(n_paths, variant)
        for prm in V.GAE_PARAMS:
            args = (c["offs"], c["rew"], c["val"], c["cost"], c["cval"], c["last_val"], c["last_cval"], c["mask"]) + prm
            key = ("gae_clean", n_paths, variant, prm)
            if key not in _MEMO:
                _MEMO[key] = V.gae_segments(*args)
            out = V.gae_segments(*args, defect=defect) if defect else _MEMO[key]
            _worst(acc, {name: int(np.sum(a != b)) for name, a, b in zip(("adv", "ret", "cadv", "cret"), out, _MEMO[key])})
    _MEMO[("gae", defect)] = acc
    return acc


def _norm(defect):
    if ("norm", defect) in _MEMO:
        return _MEMO[("norm", defect)]
    acc = {}
    for n, fam in V.NORM_CASES:
        adv, cadv = V.norm_input(n, fam)
        ref = V.adv_normalize64(adv, cadv)
        emu = V.adv_normalize64(adv, cadv, emulate=True, defect=defect)
        assert np.all(np.isfinite(emu["adv"])) and np.all(np.isfinite(emu["cadv"]))
        _worst(acc, {"norm_" + k: v for k, v in V.norm_fractions(emu, ref).items()})
    _MEMO[("norm", defect)] = acc
    return acc


_OF = {"wave_dropped": _dots, "tail_dropped": _dots, "gl_float32": _gae, "delta_float32": _gae, "one_pass_var": _norm,
       "cadv_adv_mean": _norm}


@pytest.mark.parametrize("defect", V.DEFECTS)
def test_each_defect_leaves_its_bound_by_a_factor_of_four(defect):
    f = _OF[defect](defect)
    print(defect, {k: "%.3g" % v for k, v in f.items()})
    if _OF[defect] is _gae:             # bit-exact: at least four elements differ
        assert max(f.values()) >= 4, f
        return
    assert max(f.values()) >= 4.0, f
    want = {"wave_dropped": ("dots", "cg_alpha", "cg_beta"), "tail_dropped": ("dots", "cg_alpha", "cg_beta"),
            "one_pass_var": ("norm_adv", "norm_std"), "cadv_adv_mean": ("norm_cadv",)}[defect]
    for k in want:                      # every check that is meant to see the defect sees it
        assert f[k] >= 4.0, (k, f)


@pytest.mark.parametrize("what", ["dots", "gae", "norm_adv_std", "norm_cadv"])
def test_the_undamaged_emulation_stays_below_half_of_every_bound(what):
    """Measured on the GPU cases' inputs: dots 0.018, cg step x / r / p / alpha / beta 0 (the emulation is its own reference), GAE 0
    differing elements, norm adv 0.43, std 0.085, cadv 0.495 (one rounding of the float64 difference against a bound of twice
    that and the |cmean64| term; with the mean cast to float32 ahead of the subtraction it was 0.806)."""
    f = {"dots": _dots, "gae": _gae}.get(what, _norm)(None)
    if what == "norm_adv_std":
        f = {k: v for k, v in f.items() if k != "norm_cadv"}
    elif what == "norm_cadv":
        f = {"norm_cadv": f["norm_cadv"]}
    print(what, {k: "%.3g" % v for k, v in f.items()})
    if what == "gae":
        assert max(f.values()) == 0, f
    else:
        assert max(f.values()) <= 0.5, f
