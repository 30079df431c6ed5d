"""GPU: device-side start-state sampling (csrc/start_states.hip behind CPOBuffer.sample_start_states) against the NumPy
specification of tests/test_start_states_cpu.py, golden G13 (the reference's recorded draws) and the existing host path.
Injected uniforms make every comparison of indices and rows exact."""
import os
import warnings

import numpy as np
import pytest

from test_start_states_cpu import (avoid_cdf_edges, spec_boltz_dist, spec_boltz_draw, spec_cdf, spec_epoch_draw,
                                   spec_epochs_list)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KL_TOL = dict(rtol=2e-4, atol=1e-7)      # what test_compute_dkl_run_diagnostics_update_real_c grants compute_DKL


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class _Space:
    def __init__(self, d):
        self.shape = (d,)


def _new_buffer(size, archive_size, D, A):
    from cmbpo_amd.cpobuffer import CPOBuffer
    buf = CPOBuffer(size, archive_size, _Space(D), _Space(A), device="cuda:0")
    buf.initialize({"mu": [A], "log_std": [A]}, gamma=0.99, lam=0.95, cost_gamma=0.97, cost_lam=0.5)
    return buf


def _replay_g13(buf, g):
    i = p = 0
    lengths = iter(g["path_lengths"])
    for epoch, n_paths in zip(g["plan_epochs"], g["plan_lengths"]):
        for _ in range(int(n_paths)):
            for _ in range(int(next(lengths))):
                buf.store(g["obs"][i], g["act"][i], g["obs"][i] + 1, g["rew"][i], g["val"][i], g["cost"][i], g["cval"][i],
                          g["logp"][i], {"mu": g["mu"][i], "log_std": g["log_std"][i]}, False, int(epoch))
                i += 1
            buf.finish_path(g["last"][p, 0:1], g["last"][p, 1:2])
            p += 1
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # 'Archive is full, deleting old samples.' at the wrap-around
            buf.get()


def _g13_buffer():
    g = np.load(os.path.join(GOLD, "g13_start_states.npz"), allow_pickle=False)
    buf = _new_buffer(40, int(g["N"]), int(g["D"]), int(g["A"]))
    buf.enable_device_archive()
    _replay_g13(buf, g)
    return buf, g


def _synthetic_buffer(N, n_epochs=60, D=29, A=8, seed=0):
    """An archive of N slots in the state the trainer leaves after one wrap-around, laid out directly (N store() calls
    are not the subject) and then mirrored: n_epochs epochs in contiguous slabs of unequal size; the newest three were
    written from slot 0 again, the first of them (tag n_epochs + 2) also has an older slab at the end -- two runs of one
    epoch --, the oldest epoch alive (tag 5) is partly overwritten, the tail is empty."""
    rng = np.random.default_rng(seed)
    buf = _new_buffer(8, N, D, A)
    tags = [n_epochs + 2, n_epochs + 3, n_epochs + 4] + list(range(5, n_epochs + 2)) + [n_epochs + 2]
    sizes = rng.integers(int(0.6 * N / len(tags)), N // len(tags), len(tags))
    ep, pos = buf.arch_dict["epochs"], 0
    for k, (tag, sz) in enumerate(zip(tags, sizes)):
        ep[pos:pos + sz] = tag
        pos += int(sz)
        if k == 2:
            buf.archive_ptr = pos
    buf.max_pointer, buf.archive_full = pos, True
    assert pos < N and len(spec_epochs_list(ep)) == n_epochs
    buf.arch_dict["observations"][:] = rng.standard_normal((N, D)).astype(np.float32)
    buf.pi_info_archive["mu"][:] = rng.standard_normal((N, A)).astype(np.float32)
    buf.pi_info_archive["log_std"][:] = (-0.5 + 0.1 * rng.standard_normal((N, A))).astype(np.float32)
    buf.enable_device_archive()
    return buf


def _policy(D, A, seed=2):
    from cmbpo_amd import synthetic
    from cmbpo_amd.cpo_policy import CPOPolicy
    policy = CPOPolicy(_Space(D), _Space(A), a_hidden_layer_sizes=(128, 128), vf_hidden_layer_sizes=(128, 128),
                       vf_ensemble_size=3, vf_elites=2, vf_activation="swish", vf_loss="MSE", device="cuda:0")
    policy.set_params(synthetic.policy_params(np.random.default_rng(seed), D, A, 128))
    return policy


def _host(t):
    return t.cpu().numpy()


# ---- mirror ----------------------------------------------------------------------------------------------------------------
def test_mirror_follows_the_archive_through_a_wrap_around(hip_lib):
    _need_gpu()
    buf, g = _g13_buffer()
    assert buf.archive_full and buf.archive_ptr == 12
    np.testing.assert_array_equal(buf.epoch_archive, g["arch_epochs"])
    dev = buf.device_archive()
    assert dev["epochs"].dtype == torch.int32 and dev["observations"].dtype == torch.float32
    np.testing.assert_array_equal(_host(dev["epochs"]), buf.epoch_archive)
    np.testing.assert_array_equal(_host(dev["observations"]), buf.arch_dict["observations"])
    np.testing.assert_array_equal(_host(dev["observations"]), g["arch_observations"])
    np.testing.assert_array_equal(_host(dev["mu"]), buf.pi_info_archive["mu"])
    np.testing.assert_array_equal(_host(dev["log_std"]), buf.pi_info_archive["log_std"])
    info = buf._start_table()
    np.testing.assert_array_equal(info["epochs"], g["epochs_list"])
    np.testing.assert_array_equal(info["counts"], np.bincount(g["arch_epochs"][g["arch_epochs"] >= 0])[g["epochs_list"]])
    assert list(info["run_start"]) == [0, 12, 30, 50, 75, 90] and info["filled"] == 90
    # enabled late: filled from the host archive; never enabled: nothing allocated
    late = _new_buffer(40, int(g["N"]), int(g["D"]), int(g["A"]))
    _replay_g13(late, g)
    assert late._dev is None
    np.testing.assert_array_equal(_host(late.device_archive()["epochs"]), g["arch_epochs"])
    buf.reset_arch()
    assert np.all(_host(buf.device_archive()["epochs"]) == -1)
    from cmbpo_amd._lib import CmbpoHipError
    with pytest.raises(CmbpoHipError, match="empty"):
        buf.sample_start_states(None, 8)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["g13", "synthetic"])
def test_epoch_draw_is_the_specified_member_for_every_draw(hip_lib, which):
    _need_gpu()
    if which == "g13":
        buf, _ = _g13_buffer()
        B = 257
    else:
        buf = _synthetic_buffer(300000)
        B = 5000
    ep = buf.epoch_archive
    epochs = spec_epochs_list(ep)
    u = np.random.default_rng(4).random((len(epochs), B))
    u[:, 0], u[:, 1] = 0.0, np.nextafter(1.0, 0.0)
    out = buf.device_epoch_batch(B, u=u)
    idx = _host(out["idx"]).astype(np.int64)
    np.testing.assert_array_equal(idx, spec_epoch_draw(ep, epochs, u))
    assert np.all(ep[idx] == epochs[:, None])
    np.testing.assert_array_equal(_host(out["observations"]), buf.arch_dict["observations"][idx])
    np.testing.assert_array_equal(_host(out["mu"]), buf.pi_info_archive["mu"][idx])
    np.testing.assert_array_equal(_host(out["log_std"]), buf.pi_info_archive["log_std"][idx])
    # a subset of the epochs, and the reference's answer to an epoch outside [min_ep, max_ep]
    sub = buf.device_epoch_batch(B, epochs=epochs[[2, 0]], u=u[:2])
    np.testing.assert_array_equal(_host(sub["idx"]), spec_epoch_draw(ep, epochs[[2, 0]], u[:2]))
    assert buf.device_epoch_batch(B, epochs=[int(epochs[-1]) + 1]) is None


# ---- (d) ---------------------------------------------------------------------------------------------------------------------
def test_boltz_draw_returns_the_reference_indices_on_g13(hip_lib):
    _need_gpu()
    buf, g = _g13_buffer()
    for a, alpha in enumerate(g["alphas"]):
        for s, size in zip(g["seeds"], g["sizes"]):
            rows, idx = buf.device_boltz_draw(int(size), u=g[f"draw{a}_{s}_u"], kls=g["kls"], alpha=float(alpha))
            np.testing.assert_array_equal(_host(idx), g[f"draw{a}_{s}_idx"])
            np.testing.assert_array_equal(_host(rows), g[f"draw{a}_{s}_obs"])
        _, ep_probs = spec_boltz_dist(g["arch_epochs"], g["kls"], float(alpha))
        np.testing.assert_allclose(_host(buf._cdf[8 + 3 * 1024:][:4]), ep_probs, rtol=1e-15)
    # an epoch whose weight underflows to 0, and the ends of [0, 1)
    kls = np.array([0.31, 0.02, 2000.0, 0.1])
    u = np.array([0.0, np.nextafter(1.0, 0.0), 0.5, 0.25])
    _, idx = buf.device_boltz_draw(4, u=u, kls=kls, alpha=1.0)
    dist, _ = spec_boltz_dist(g["arch_epochs"], kls, 1.0)
    np.testing.assert_array_equal(_host(idx), spec_boltz_draw(dist, u))
    assert np.all(dist[_host(idx)] > 0) and np.all(g["arch_epochs"][_host(idx)] >= 0)


@pytest.mark.parametrize("N", [300000, 1000000])
def test_boltz_draw_equals_the_specification_at_scale(hip_lib, N):
    _need_gpu()
    buf = _synthetic_buffer(N, seed=N % 97)
    ep = buf.epoch_archive
    rng = np.random.default_rng(8)
    kls = rng.random(len(spec_epochs_list(ep))) * 0.05
    B = 100000
    dist, _ = spec_boltz_dist(ep, kls, 1.0)
    cdf = spec_cdf(dist)
    u, redrawn = avoid_cdf_edges(cdf, rng.random(B), rng)
    u[0], u[1] = 0.0, np.nextafter(1.0, 0.0)
    print("N", N, "smallest CDF gap", np.diff(np.unique(cdf)).min(), "uniforms redrawn", redrawn)
    rows, idx = buf.device_boltz_draw(B, u=u, kls=kls, alpha=1.0)
    idx = _host(idx).astype(np.int64)
    np.testing.assert_array_equal(idx, spec_boltz_draw(dist, u))          # every draw, no exclusions
    assert np.all(ep[idx] >= 0) and np.all(dist[idx] > 0)
    np.testing.assert_array_equal(_host(rows), buf.arch_dict["observations"][idx])


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
def test_epoch_kl_matches_compute_dkl_and_is_reproducible(hip_lib):
    _need_gpu()
    buf = _synthetic_buffer(300000)
    policy = _policy(29, 8)
    E = len(spec_epochs_list(buf.epoch_archive))
    u = np.random.default_rng(5).random((E, 3000))
    ep_b = buf.device_epoch_batch(3000, u=u)
    kl = _host(buf.device_epoch_kl(policy, ep_b)).copy()
    ref = np.clip(policy.compute_DKL(_host(ep_b["observations"]), _host(ep_b["mu"]), _host(ep_b["log_std"])), 0, None)
    print("device KL", kl[:4], "host KL", ref[:4], "max rel", np.max(np.abs(kl - ref) / np.abs(ref)))
    assert kl.shape == (E,) and np.all(kl > 1e-3), "the policy is away from the stored mu / log_std"
    np.testing.assert_allclose(kl, ref, **KL_TOL)
    again = _host(buf.device_epoch_kl(policy, buf.device_epoch_batch(3000, u=u)))
    assert np.array_equal(kl.view(np.int64), again.view(np.int64)), "two calls, the same bits"


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1000, 100000])
def test_sample_start_states_writes_the_host_chains_rows_into_cur_obs(hip_lib, B):
    _need_gpu()
    from cmbpo_amd.modelbuffer import ModelBuffer
    D, A = 29, 8
    buf = _synthetic_buffer(300000)
    policy = _policy(D, A)
    pool = ModelBuffer(batch_size=B, obs_dim=D, act_dim=A, max_path_length=2, device="cuda:0")
    ep = buf.epoch_archive
    epochs = spec_epochs_list(ep)
    rng = np.random.default_rng(6)
    u_epoch = rng.random((len(epochs), B))
    # the CDF of this round (the KLs are reproducible bit for bit), to keep the injected uniforms off its edges
    kl_dev = _host(buf.device_epoch_kl(policy, buf.device_epoch_batch(B, u=u_epoch))).copy()
    dist_dev, _ = spec_boltz_dist(ep, kl_dev, 1.5)
    u_draw, _ = avoid_cdf_edges(spec_cdf(dist_dev), rng.random(B), rng)

    cur = pool.t["cur_obs"]
    ret = buf.sample_start_states(policy, B, alpha=1.5, out=cur, u_epoch=u_epoch, u_draw=u_draw)
    assert ret.data_ptr() == cur.data_ptr() == pool.rs.cur_obs
    assert np.array_equal(_host(buf.last_start["kl"]).view(np.int64), kl_dev.view(np.int64))
    # the host chain: epoch_batch restated with the same uniforms, compute_DKL, boltz_dist, searchsorted
    idx_e = spec_epoch_draw(ep, epochs, u_epoch)
    np.testing.assert_array_equal(_host(buf.last_start["idx_epoch"]), idx_e)
    kl_host = np.clip(policy.compute_DKL(buf.arch_dict["observations"][idx_e], buf.pi_info_archive["mu"][idx_e],
                                         buf.pi_info_archive["log_std"][idx_e]), 0, None)
    np.testing.assert_allclose(kl_dev, kl_host, **KL_TOL)
    np.testing.assert_array_equal(buf.boltz_dist(kl_host, alpha=1.5), spec_boltz_dist(ep, kl_host, 1.5)[0])
    want = spec_boltz_draw(buf.boltz_dist(kl_host, alpha=1.5), u_draw)
    got = _host(buf.last_start["idx"]).astype(np.int64)
    moved = int(np.sum(want != got))
    print("B", B, "draws that differ from the host-KL chain", moved)
    if moved:      # KLs equal within KL_TOL moved an edge across a uniform: the draw itself is judged on the device KLs
        want = spec_boltz_draw(dist_dev, u_draw)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(_host(cur), buf.arch_dict["observations"][want])
    # another batch size reallocates the scratch
    small = buf.sample_start_states(policy, 64)
    assert tuple(small.shape) == (64, D) and tuple(buf.last_start["idx_epoch"].shape) == (len(epochs), 64)


def test_drawn_epoch_frequencies_follow_the_boltzmann_distribution(hip_lib):
    """No injected uniforms: 200 000 draws from the buffer's own generator; every epoch's frequency lies within five
    binomial standard deviations of its Boltzmann probability."""
    _need_gpu()
    buf, g = _g13_buffer()
    policy = _policy(int(g["D"]), int(g["A"]))
    n = 200000
    buf.start_generator.manual_seed(1234)
    rows = buf.sample_start_states(policy, n, alpha=0.5)
    idx = _host(buf.last_start["idx"])
    ep = g["arch_epochs"]
    assert np.all(ep[idx] >= 0)
    np.testing.assert_array_equal(_host(rows), g["arch_observations"][idx])
    kl = _host(buf.last_start["kl"])
    _, ep_probs = spec_boltz_dist(ep, kl, 0.5)
    np.testing.assert_allclose(_host(buf.last_start["ep_probs"]), ep_probs, rtol=1e-12)
    freq = np.array([np.sum(ep[idx] == e) for e in g["epochs_list"]])
    sd = np.sqrt(n * ep_probs * (1 - ep_probs))
    print("epoch frequencies", freq, "expected", n * ep_probs, "sd", sd)
    assert np.all(np.abs(freq - n * ep_probs) <= 5 * sd)


def test_a_void_boltzmann_distribution_is_reported_at_the_next_archive_change(hip_lib):
    """A NaN KL leaves no distribution to draw from (np.random.choice raises on the host path).  The device path does not
    read anything back per round; the kernel's flag is looked at where the host synchronises anyway, at the table rebuild."""
    _need_gpu()
    from cmbpo_amd._lib import CmbpoHipError
    buf, g = _g13_buffer()
    _, idx = buf.device_boltz_draw(4, u=np.array([0.1, 0.2, 0.6, 0.9]), kls=np.array([np.nan, 0.1, 0.1, 0.1]), alpha=1.0)
    assert np.all((_host(idx) >= 0) & (_host(idx) < 100)), "indices stay inside the archive"
    buf.store(g["obs"][0], g["act"][0], g["obs"][0], 0.0, 0.0, 0.0, 0.0, 0.0, {"mu": g["mu"][0], "log_std": g["log_std"][0]},
              False, 7)
    buf.finish_path()
    buf.get()
    with pytest.raises(CmbpoHipError, match="void"):
        buf.device_epoch_batch(8)
    assert list(buf.device_epoch_batch(8)["idx"].shape) == [5, 8]          # reported once; epoch 7 is the fifth
