"""CPU: the yardstick of tests/test_pi_f64_gpu.py is sound (tests/pi_f64_ref.py; no GPU, no HIP library).

  * The bound separates a sound two-piece product from one that lost a piece: on every hidden-128 case of A and B, for flat_g,
    flat_b and the dense Fisher-vector product at theta_old, MARGIN * max(e32[block], mean e32, FLOOR) on the W0 and on the W1
    block is at most a QUARTER of what a float64 evaluation errs by on that block once W1 -- and, separately, W0 -- is cut to one
    lifted f16 piece (lift 2^(13 - floor(log2 max |W|)), round to float16, unlift).  BLIND lists the (mutation, vector, cut, block)
    where a cut cannot show on one of the two blocks whatever the arithmetic, with the reason; there the other block has to meet
    the condition.
  * Every case of the GPU tests is non-degenerate: the float32 reference is finite and no reference vector is all zeros; the
    clip-edge filter of the first-order cases stays within 2 % of the rows, and something clips.
  * The reference itself: `fisher_vp` equals `hvp` at theta_old in float64 to 1e-10 once mu_old is the float64 mean.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import pi_f64_ref as R  # noqa: E402
from oracle import refupdate  # noqa: E402

W0, W1 = R.BLOCKS.index("W0"), R.BLOCKS.index("W1")

# (mutation, vector, cut block, blind block): reason
BLIND = {
    ("w1_1e-2", "fvp", W1, W1): "with W1 a hundredth of its size h2 barely depends on it, and the W1 block of the product (h1^T d2) "
                                "depends on W1 through h2 alone: the cut moves it by ~2e-6; the W0 block (d1 = d2 W1^T) shows it",
    ("obs_row_1e3", "fvp", W1, W0): "the W0 block of the product is the 1e3 x row's (x^T d1): on its nearly saturated units tanh' = "
                                    "1 - h^2 cancels in float32 (e32 ~1e-5) and the cut of W1 reaches it through tanh' ~ 0; the W1 "
                                    "block shows it",
}


def _damaged(ref, block):
    c = ref.case
    g, b, _, _ = ref.g64.grads(R.cut_block(ref.p, c.D, c.A, c.hidden, block))
    hv = ref.g64.fisher_vp(R.cut_block(ref.theta, c.D, c.A, c.hidden, block), ref.dirs["dense"], 0.0)
    return dict(g=g, b=b, fvp=hv)


@pytest.mark.parametrize("c", [c for c in R.CASES_A + R.CASES_B if c.hidden == 128], ids=R.case_id)
def test_bound_is_a_quarter_of_a_lost_f16_piece(c):
    assert R.MARGIN is not None and R.MARGIN == 2.0 ** round(np.log2(R.MARGIN)) and R.MARGIN >= 2.0 * R.MEASURED_WORST_RATIO
    assert R.MARGIN < 4.0 * R.MEASURED_WORST_RATIO        # twice the measured worst ratio, rounded UP to a power of two: no more
    ref = R.reference_of(c)
    fig = ref.figures()
    refs = dict(g=fig["g"], b=fig["b"], fvp=fig[("fvp", "old", "dense")])
    for cut in (W1, W0):
        dam = _damaged(ref, cut)
        for name, (x64, e32) in refs.items():
            damage, bound = ref.errors(dam[name], x64), R.MARGIN * R.yardstick(e32)
            ok = {k: bound[k] <= damage[k] / 4.0 for k in (W0, W1)}
            for k in (W0, W1):
                if (c.mutation, name, cut, k) in BLIND:
                    assert ok[W0 + W1 - k], (R.case_id(c), name, R.BLOCKS[cut], damage, bound)
                    continue
                assert ok[k], "%s %s with %s cut to one f16 piece: bound %.3g on block %s (e32 %s) against a damage of %.3g; all blocks %s" % (
                    R.case_id(c), name, R.BLOCKS[cut], bound[k], R.BLOCKS[k], e32, damage[k], damage)


ALL = R.CASES_A + R.CASES_A2 + R.CASES_B + R.CASES_C + R.CASES_PPO


@pytest.mark.parametrize("c", ALL, ids=R.case_id)
def test_cases_are_not_degenerate(c):
    ref = R.reference_of(c)
    fig = ref.figures()
    for key, val in fig.items():
        if key == "cost_sum":
            continue
        x64, e32 = val[:2]
        assert np.isfinite(x64).all() and np.isfinite(e32).all() and np.isfinite(val[-1]).all(), key
        assert np.abs(x64).max() > 0, key
        assert np.max(e32) < 1e-3, (key, e32)      # (the float32 reference itself still knows three digits)


@pytest.mark.parametrize("c", R.CASES_PPO, ids=R.case_id)
def test_clip_edge_cap_and_something_clips(c):
    ref = R.reference_of(c)                          # (the constructor asserts the cap)
    assert ref.dropped <= 0.02 * (ref.n + ref.dropped)
    for (clipped, penalty), f in ref.ppo_figures().items():
        assert np.isfinite(f["g"][0]).all() and np.isfinite(f["g"][1]).all() and np.isfinite(f["sums32"]).all()
        s = f["sums64"]
        if clipped:
            assert 0 < s[5] < s[0] and s[1] != s[6]      # a run in which nothing clips cannot pass
            plain = R.ppo_lag_ref.Surrogate(R.ppo_lag_ref.make_graph(c.D, c.A, ref.batch, hidden=c.hidden), R.CLIP).sums(ref.p)
            assert 0.05 <= plain[5] / ref.n <= 0.95, plain[5] / ref.n
            # the same mask in float32 (the filter did its work); a weighted count is a float32 sum of the weights
            np.testing.assert_allclose(f["sums32"][5], s[5], rtol=0 if ref.weights is None else 1e-6)
        else:
            assert s[5] == 0 and abs(s[1] - s[6]) <= 1e-12 * abs(s[6])      # (w obj and w ratio adv multiply in another order)


@pytest.mark.parametrize("c", R.CASES_D, ids=R.case_id)
def test_cg_reference_is_finite(c):
    fig = R.reference_of(c).cg_figures()
    assert np.isfinite(fig["x64"]).all() and np.isfinite(fig["e32"]) and fig["e32"] < 1e-2


@pytest.mark.parametrize("c", [R.CASES_A[4], R.CASES_A[21], R.CASES_B[5], R.CASES_A[24]], ids=R.case_id)
def test_fisher_vp_is_hvp_at_theta_old(c):
    ref = R.reference_of(c)
    batch = {k: np.array(v, np.float64) for k, v in ref.batch.items()}
    g = refupdate.PolicyGraph(c.D, c.A, batch, dtype=torch.float64, hidden=c.hidden)
    with torch.no_grad():
        batch["mu_old"] = g._mu(torch.as_tensor(ref.theta, dtype=torch.float64))[0].numpy()
    g = refupdate.PolicyGraph(c.D, c.A, batch, dtype=torch.float64, hidden=c.hidden)
    for d in R.DIRECTIONS:
        v = ref.dirs[d].astype(np.float64)
        assert R.whole_error(g.fisher_vp(ref.theta, v, R.DAMPING), g.hvp(ref.theta, v, R.DAMPING)) <= 1e-10, d


def test_measures():
    D, A, H = 2, 1, 128
    P = refupdate.n_params(D, A, H)
    x64 = np.zeros(P)
    x64[0], x64[D * H] = 4.0, 1.0                      # W0 block max 4, b0 block max 1, the rest zero
    x = x64.copy()
    x[1] += 1.0                                        # W0: 1 / 4
    x[D * H + 1] += 0.5                                # b0: 0.5 / 1
    x[-1] += 2.0 ** -10                                # log_std (all zero): against 2^-10 of the vector's maximum = 2^-8
    e = R.block_errors(x, x64, D, A, H)
    np.testing.assert_allclose(e, [0.25, 0.5, 0, 0, 0, 0, 0.25])
    np.testing.assert_allclose(R.yardstick([8e-6, 0, 0, 0, 0, 0, 6e-6]), [8e-6, 2e-6, 2e-6, 2e-6, 2e-6, 2e-6, 6e-6])
    assert (R.yardstick(np.zeros(7)) == R.FLOOR).all()
    w = np.random.default_rng(0).standard_normal((64, 64)) * 3e-3
    cut = R.one_piece(w)
    assert 0 < np.abs(cut - w).max() <= 2.0 ** -11 * 2.0 * np.abs(w).max()
    assert np.array_equal(cut.astype(np.float32).astype(np.float64), cut)
