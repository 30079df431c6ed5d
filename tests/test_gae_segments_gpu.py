"""GPU: cmbpo_gae_segments and cmbpo_adv_normalize (csrc/gae_segments.hip) called through the C ABI, against the restatements of
tests/vec_gae_ref.py (whose docstring derives every bound used here).

cmbpo_gae_segments is bit-exact against `gae_segments` at 1 .. 130 paths (one and three workgroups), with empty segments first,
last and in the middle, 1000-row paths, a first offset of 5, spare rows behind the last, every mask value and a NULL mask, at three
sets of discounts.  cmbpo_adv_normalize is held to float64 at sizes around the wave, the workgroup and the 512-workgroup cap, on
inputs with a far-off mean, nine decades of magnitudes, a constant and zeros.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import vec_gae_ref as V  # noqa: E402

F32, F64 = np.float32, np.float64
EINVAL = -1          # CMBPO_EINVAL (include/cmbpo_hip.h)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the case arrays are read-only)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    from cmbpo_amd import _lib
    return _lib.current_stream()


@pytest.mark.parametrize("n_paths,variant", V.GAE_LAYOUTS, ids=["%d%s" % (n, v) for n, v in V.GAE_LAYOUTS])
def test_gae_segments_is_the_restatement_bit_for_bit(hip_lib, n_paths, variant):
    _need_gpu()
    from cmbpo_amd import _lib
    c = V.gae_case(n_paths, variant)
    ins = [_dev(c[k]) for k in ("offs", "rew", "val", "cost", "cval", "last_val", "last_cval")]
    mask = None if c["mask"] is None else _dev(c["mask"])
    assert (mask is None) == (variant == "nullmask")
    for prm in V.GAE_PARAMS:
        outs = [torch.full((c["N"],), V.SENTINEL, dtype=torch.float32, device="cuda") for _ in range(4)]
        _lib.check(hip_lib.cmbpo_gae_segments(n_paths, *[t.data_ptr() for t in ins], _ptr(mask), *prm,
                                              *[t.data_ptr() for t in outs], _stream()), "cmbpo_gae_segments")
        want = V.gae_segments(c["offs"], c["rew"], c["val"], c["cost"], c["cval"], c["last_val"], c["last_cval"], c["mask"], *prm)
        lo, hi = int(c["offs"][0]), int(c["offs"][-1])
        for name, t, w in zip(("adv", "ret", "cadv", "cret"), outs, want):
            got = t.cpu().numpy()
            # (the restatement is filled with the sentinel outside [offs[0], offs[n_paths]) as well)
            assert np.all(w[:lo] == F32(V.SENTINEL)) and np.all(w[hi:] == F32(V.SENTINEL)) and lo == V.GAE_FIRST
            np.testing.assert_array_equal(got, w, err_msg="%s at %r" % (name, prm))
            V.record("gae_segments/%d%s/%s" % (n_paths, variant, name), float(np.sum(got != w)))
        if hi > lo:
            assert np.all(np.isfinite(outs[0][lo:hi].cpu().numpy()))
    print("gae_segments %d%s: %d rows in %d paths, bit-exact at %d discount sets" % (n_paths, variant, hi - lo, n_paths,
                                                                                     len(V.GAE_PARAMS)))


def test_gae_segments_arguments(hip_lib):
    _need_gpu()
    assert hip_lib.cmbpo_gae_segments(0, *([None] * 8), 0.99, 0.95, 0.97, 0.5, *([None] * 4), _stream()) == 0
    c = V.gae_case(1, "long")
    ins = [_dev(c[k]) for k in ("offs", "rew", "val", "cost", "cval", "last_val", "last_cval")]
    outs = [torch.full((c["N"],), V.SENTINEL, dtype=torch.float32, device="cuda") for _ in range(4)]
    for missing in (0, 3, 6, 12, 15):         # offsets, a row array, a bootstrap, the first and the last output
        args = [t.data_ptr() for t in ins] + [None] + [0.99, 0.95, 0.97, 0.5] + [t.data_ptr() for t in outs]
        assert len(args) == 16 and args[missing] is not None
        args[missing] = None
        rc = hip_lib.cmbpo_gae_segments(1, *args, _stream())
        assert rc == EINVAL, missing
        assert b"NULL buffer" in hip_lib.cmbpo_last_error()
    assert hip_lib.cmbpo_gae_segments(-1, *([None] * 8), 0.99, 0.95, 0.97, 0.5, *([None] * 4), _stream()) == EINVAL
    torch.cuda.synchronize()
    for t in outs:                              # nothing was launched
        assert bool((t == V.SENTINEL).all())


def _normalize(hip_lib, adv, cadv):
    from cmbpo_amd import _lib
    n = adv.size
    tail = np.full(4, V.SENTINEL, F32)
    a, c = _dev(np.concatenate([adv, tail])), _dev(np.concatenate([cadv, tail]))
    stats = torch.full((20,), V.SENTINEL, dtype=torch.float64, device="cuda")
    _lib.check(hip_lib.cmbpo_adv_normalize(n, a.data_ptr(), c.data_ptr(), stats.data_ptr(), _stream()), "cmbpo_adv_normalize")
    a, c, st = a.cpu().numpy(), c.cpu().numpy(), stats.cpu().numpy()
    assert np.all(a[n:] == F32(V.SENTINEL)) and np.all(c[n:] == F32(V.SENTINEL)) and np.all(st[16:] == V.SENTINEL)
    return dict(adv=a[:n], cadv=c[:n], n=st[0], mean=st[1], std=st[2], cmean=st[3], stats=st[:16])


def _check_normalize(hip_lib, n, fam):
    adv, cadv = V.norm_input(n, fam)
    ref = V.adv_normalize64(adv, cadv)
    got = _normalize(hip_lib, adv, cadv)
    assert got["n"] == n
    assert np.all(np.isfinite(got["adv"])) and np.all(np.isfinite(got["cadv"])) and np.all(np.isfinite(got["stats"]))
    f = V.norm_fractions(got, ref)
    f["mean"] = V.frac(abs(got["mean"] - ref["mean"]), V.bound_mean(adv))
    f["cmean"] = V.frac(abs(got["cmean"] - ref["cmean"]), V.bound_mean(cadv))
    for k, v in f.items():
        V.record("adv_normalize/%s/%s" % (fam, k), v)
    assert max(f.values()) <= 1.0, (n, fam, f)
    if fam in ("const", "zeros") or n == 1:
        assert np.all(got["adv"] == 0) and got["std"] == 0, (n, fam)
    if fam in ("const", "zeros"):
        assert np.all(got["cadv"] == 0)
    return f


@pytest.mark.parametrize("n", V.NORM_SIZES)
def test_adv_normalize_against_float64(hip_lib, n):
    _need_gpu()
    worst = {}
    for fam in [f for (m, f) in V.NORM_CASES if m == n]:
        for k, v in _check_normalize(hip_lib, n, fam).items():
            if v > worst.get(k, (-1.0, ""))[0]:
                worst[k] = (v, fam)
    print("adv_normalize n = %d: worst fraction of the bound %s" % (n, {k: "%.3g (%s)" % v for k, v in worst.items()}))


def test_adv_normalize_of_nothing_leaves_sixteen_zeros(hip_lib):
    _need_gpu()
    from cmbpo_amd import _lib
    stats = torch.full((20,), V.SENTINEL, dtype=torch.float64, device="cuda")
    _lib.check(hip_lib.cmbpo_adv_normalize(0, None, None, stats.data_ptr(), _stream()), "cmbpo_adv_normalize")
    st = stats.cpu().numpy()
    assert np.all(st[:16] == 0) and np.all(st[16:] == V.SENTINEL)
    assert hip_lib.cmbpo_adv_normalize(3, None, None, stats.data_ptr(), _stream()) == EINVAL
    assert hip_lib.cmbpo_adv_normalize(3, None, None, None, _stream()) == EINVAL


def test_adv_normalize_repeats_within_one_ulp(hip_lib):
    """The float64 atomicAdds of norm_moments add the 512 workgroups' partial sums in no fixed order; at float32 that does not
    show beyond the last place."""
    _need_gpu()
    adv, cadv = V.norm_input(300001, "n01+3")
    a, b = _normalize(hip_lib, adv, cadv), _normalize(hip_lib, adv, cadv)
    for k in ("adv", "cadv"):
        u = float(np.max(V.ulps(a[k], b[k])))
        print("adv_normalize twice at n = 300001: %s differs by %.2g ulp at most, stats by %.3g relative" %
              (k, u, np.max(np.abs(a["stats"][:4] - b["stats"][:4]) / np.abs(a["stats"][:4]))))
        V.record("adv_normalize/repeat/%s_ulp" % k, u)
        assert u <= 1.0
