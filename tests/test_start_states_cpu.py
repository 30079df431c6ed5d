"""CPU: the arithmetic device-side start-state sampling rests on (csrc/start_states.hip), pinned to the reference.

Golden G13 (tests/golden/make_golden_start_states.py) was recorded from the reference's own CPOBuffer on an archive that
wrapped around: epochs_list, boltz_dist for two alphas and, per np.random seed, the archive indices
distributed_batch_from_archive used together with the uniforms np.random.choice consumed.  The NumPy restatements below
are the specification of the device kernels: (b) the per-epoch uniform draw, (d) the Boltzmann distribution and the
inverse-CDF draw.  tests/test_start_states_gpu.py holds the kernels to them."""
import ctypes as C
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- the specification -----------------------------------------------------------------------------------------------
def spec_epochs_list(ep):
    """buffers/cpobuffer.py:148-153."""
    return np.flatnonzero(np.bincount(ep[ep >= 0]))


def spec_epoch_draw(ep, epochs, u):
    """(b): row [e, b] is member min(floor(u n_e), n_e - 1) of the epoch's archive indices in ascending order."""
    out = np.empty(u.shape, np.int64)
    for k, e in enumerate(epochs):
        members = np.flatnonzero(ep == e)
        n_e = members.size
        out[k] = members[np.minimum(np.floor(u[k] * n_e).astype(np.int64), n_e - 1)]
    return out


def spec_boltz_dist(ep, kls, alpha):
    """(d), buffers/cpobuffer.py:385-396: float64 Boltzmann weights of the epochs, spread over each epoch's samples and
    stored as float32; 0 for empty slots."""
    ep_probs = np.exp(alpha * np.negative(np.asarray(kls, np.float64)))
    ep_probs /= np.sum(ep_probs)
    sample_p = np.bincount(ep[ep >= 0]).astype(np.float32)
    sample_p[sample_p > 0] = ep_probs / sample_p[sample_p > 0]
    return np.where(ep >= 0, sample_p[ep], 0).astype(np.float32), ep_probs


def spec_cdf(dist):
    """What np.random.choice(p=dist) searches: the float64 inclusive sum over archive indices over its last element."""
    cdf = np.cumsum(dist.astype(np.float64))
    return cdf / cdf[-1]


def spec_boltz_draw(dist, u):
    """(d): searchsorted(cdf, u, side='right')."""
    return np.searchsorted(spec_cdf(dist), u, side="right")


def avoid_cdf_edges(cdf, u, rng):
    """Uniforms within N 2^-52 of an edge of the CDF are redrawn: there -- and only there -- another summation order of
    the same float64 CDF may choose the neighbouring slot.  Returns the uniforms and how many were redrawn."""
    band = cdf.size * 2.0 ** -52
    edges = np.unique(cdf)
    u = u.copy()
    redrawn = 0
    while True:
        k = np.searchsorted(edges, u)
        near = np.minimum(np.abs(edges[np.minimum(k, edges.size - 1)] - u), np.abs(u - edges[np.maximum(k - 1, 0)])) <= band
        if not near.any():
            return u, redrawn
        redrawn += int(near.sum())
        u[near] = rng.random(int(near.sum()))


# ---- G13 ---------------------------------------------------------------------------------------------------------------
def _g13():
    return np.load(os.path.join(GOLD, "g13_start_states.npz"), allow_pickle=False)


def test_g13_archive_has_the_shapes_the_kernels_must_handle():
    g = _g13()
    ep = g["arch_epochs"]
    heads = np.flatnonzero(np.diff(ep)) + 1
    runs = [int(ep[0])] + [int(ep[h]) for h in heads]
    assert runs.count(6) == 2, "an epoch split into two runs by the wrap-around"
    assert 0 < np.sum(ep == 2) < 30, "an overwritten epoch partly alive"
    assert np.sum(ep == -1) == 10 and len(set(np.bincount(ep[ep >= 0])) - {0}) >= 4, "empty tail, unequal epochs"
    np.testing.assert_array_equal(spec_epochs_list(ep), g["epochs_list"])


def test_boltz_dist_restatement_is_the_reference():
    g = _g13()
    ep = g["arch_epochs"]
    for a, alpha in enumerate(g["alphas"]):
        dist, ep_probs = spec_boltz_dist(ep, g["kls"], float(alpha))
        assert dist.dtype == g[f"boltz{a}"].dtype == np.float32
        np.testing.assert_array_equal(dist, g[f"boltz{a}"])
        assert np.all(dist[ep < 0] == 0) and abs(ep_probs.sum() - 1) < 1e-12


def test_choice_is_the_inverse_cdf_draw_with_its_own_uniforms():
    """np.random.choice(arange(N), size, p=dist) == searchsorted(cumsum(p) / last, u, 'right') for every recorded draw."""
    g = _g13()
    ep = g["arch_epochs"]
    n = 0
    for a in range(len(g["alphas"])):
        dist = g[f"boltz{a}"]
        for s, size in zip(g["seeds"], g["sizes"]):
            idx, u = g[f"draw{a}_{s}_idx"], g[f"draw{a}_{s}_u"]
            assert idx.shape == u.shape == (int(size),)
            np.testing.assert_array_equal(spec_boltz_draw(dist, u), idx)
            np.testing.assert_array_equal(g["arch_observations"][idx], g[f"draw{a}_{s}_obs"])
            assert np.all(ep[idx] >= 0)
            n += idx.size
    assert n == 2 * (23 + 64 + 257)


def test_inverse_cdf_draw_never_returns_an_empty_or_zero_probability_slot():
    g = _g13()
    ep = g["arch_epochs"]
    dist, _ = spec_boltz_dist(ep, np.array([0.31, 0.02, 2000.0, 0.1]), 1.0)       # epoch 5 underflows to probability 0
    assert np.all(dist[ep == 5] == 0)
    u = np.array([0.0, np.nextafter(1.0, 0.0), 0.5])
    idx = spec_boltz_draw(dist, u)
    assert np.all(dist[idx] > 0) and np.all(ep[idx] >= 0)


def test_epoch_draw_restatement():
    g = _g13()
    ep = g["arch_epochs"]
    epochs = g["epochs_list"]
    u = np.random.default_rng(3).random((len(epochs), 50))
    u[:, 0], u[:, 1] = 0.0, np.nextafter(1.0, 0.0)
    idx = spec_epoch_draw(ep, epochs, u)
    for k, e in enumerate(epochs):
        members = np.flatnonzero(ep == e)
        assert np.all(ep[idx[k]] == e) and idx[k, 0] == members[0] and idx[k, 1] == members[-1]
    assert idx[3, 0] == 0 and idx[3, 1] == 89, "epoch 6 starts in the wrapped run and ends in the old one"


def test_edge_avoidance_leaves_no_uniform_near_an_edge():
    g = _g13()
    cdf = spec_cdf(g["boltz0"])
    rng = np.random.default_rng(0)
    u = rng.random(1000)
    u[:5] = cdf[[0, 20, 40, 60, 89]]
    v, redrawn = avoid_cdf_edges(cdf, u, rng)
    assert redrawn >= 5 and np.array_equal(v[5:], u[5:])
    assert np.min(np.abs(v[:, None] - cdf[None, :])) > cdf.size * 2.0 ** -52


# ---- the C-ABI validates its arguments before any HIP call ------------------------------------------------------------------
def test_start_state_entries_reject_bad_arguments_without_a_gpu():
    import __graft_entry__ as g
    g.build()
    from cmbpo_amd import _lib
    lib = _lib.lib()
    host = (C.c_int32 * 4)()
    p = C.cast(host, C.c_void_p)
    assert lib.cmbpo_start_table_build(p, 0, p, None) == -1                       # empty archive column
    assert b"archive size" in lib.cmbpo_last_error()
    assert lib.cmbpo_start_table_build(None, 10, p, None) == -1
    assert lib.cmbpo_start_epoch_draw(p, None, _lib.START_MAX_RUNS + 1, 8, p, p, p, p, 10, 5, 2, p, p, p, p, None) == -1
    assert b"n_epochs" in lib.cmbpo_last_error()
    assert lib.cmbpo_start_kl_parts(1000) == 1 and lib.cmbpo_start_kl_parts(100000) == 98
    assert lib.cmbpo_start_kl_partials(p, p, p, p, 4, 1000, 2, p, 3, None) == -1   # n_part is not cmbpo_start_kl_parts(batch)
    assert b"n_part" in lib.cmbpo_last_error()
    assert lib.cmbpo_start_cdf(p, None, 0, 0, p, float("nan"), p, None) == -1
    assert lib.cmbpo_start_boltz_draw(p, p, p, 0, p, 10, 5, p, p, None) == -1      # batch 0
    assert b"batch" in lib.cmbpo_last_error()
