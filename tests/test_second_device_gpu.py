"""A second device in the same process: every kernel family that asks for more than 64 KB of dynamic LDS is run on
device 0 and then, with handles and streams made there, on device 1.  The dynamic-LDS grants and the CU counts of
the launchers are per device, so device 1's launches must succeed and compute what device 0's did: bitwise, except
the advantage normalisation of ModelBuffer.get(), whose sums are float atomics (test_api_and_fullsize_gpu's tolerance).
"""
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

ROWS = 10000


def _ens_forward(dev, paths):
    """The 512-wide probabilistic ensemble forward on the given matrix paths (f16, bf16 split, fp32 MFMAs)."""
    from cmbpo_amd import _lib, synthetic
    from cmbpo_amd.pens import PE
    lib = _lib.lib()
    rng = np.random.default_rng(5)
    D, A = synthetic.ENV_DIMS["AntSafe-v2"]
    ws, bs = synthetic.ensemble_weights(rng, 7, D + A, 512, 2 * (D + 1), bias_scale=0.05)
    m = PE(D + A, D + 1, hidden_dims=(512, 512), num_networks=7, num_elites=5, loss="MSPE", use_scaler_in=True,
           use_scaler_out=True, device=dev)
    m.set_weights(ws, bs, synthetic.scaler(rng, D + A), synthetic.scaler(rng, D + 1))
    x = rng.standard_normal((ROWS, D + A)).astype(np.float32)
    out = {}
    before = lib.cmbpo_get_ens_matrix_path()
    try:
        for p in paths:
            _lib.check(lib.cmbpo_set_ens_matrix_path(p), "cmbpo_set_ens_matrix_path")
            out[f"ens{p}_mean"], out[f"ens{p}_var"] = m.predict_ensemble(x)
    finally:
        lib.cmbpo_set_ens_matrix_path(before)
    return out


def _critic_big(dev):
    """Both critics in one launch at 24 576 rows and more: members in turn with their weights in LDS."""
    from cmbpo_amd import _lib, synthetic
    from cmbpo_amd.pens import PE
    lib = _lib.lib()
    rng = np.random.default_rng(zlib.crc32(b"second-device/critic"))
    n, obs_dim = 24576 + 45, 29
    nets = []
    for k in range(2):
        ws, bs = synthetic.ensemble_weights(rng, 3, obs_dim, 128, 1, bias_scale=0.1)
        m = PE(obs_dim, 1, hidden_dims=(128, 128), num_networks=3, num_elites=2, loss="MSE", use_scaler_in=True,
               use_scaler_out=False, device=dev)
        m.set_weights(ws, bs, synthetic.scaler(rng, obs_dim), None)
        nets.append(m)
    assert lib.cmbpo_critic_pair_supported(nets[0].mlp.handle, nets[1].mlp.handle) == 1
    o = torch.from_numpy(rng.standard_normal((n, obs_dim)).astype(np.float32)).to(dev)
    ix = torch.arange(n, dtype=torch.int32, device=dev)
    out = [torch.empty(n, device=dev) for _ in range(2)]
    _lib.check(lib.cmbpo_critic_pair_predict(nets[0].mlp.handle, nets[1].mlp.handle, o.data_ptr(), obs_dim, ix.data_ptr(), None, n,
                                             out[0].data_ptr(), out[1].data_ptr(), _lib.current_stream()), "pair")
    return {"critic_v": out[0].cpu().numpy(), "critic_vc": out[1].cpu().numpy()}


def _train(dev):
    """cmbpo_trainer_step on the f16 path: the dynamics ensemble and a critic (the fused step) at the shipped batch."""
    from cmbpo_amd.pens import PE
    out = {}
    for name, (E, I, H, D, loss, batch) in {"dyn": (7, 37, 512, 30, "MSPE", 256), "critic": (2, 29, 128, 1, "MSE", 2048)}.items():
        rng = np.random.RandomState(zlib.crc32(name.encode()))
        pe = PE(I, D, name="T", hidden_dims=(H, H), num_networks=E, num_elites=max(1, E - 2), loss=loss, use_scaler_in=True,
                use_scaler_out=True, device=dev)
        ws, bs = pe.init_weights(rng)
        n = 3 * batch
        x = rng.standard_normal((n, I)).astype(np.float32)
        t = np.tanh(x @ rng.standard_normal((I, D)) / np.sqrt(I)).astype(np.float32)
        pe.set_weights(ws, bs, (x.mean(0, keepdims=True), x.var(0, keepdims=True)), (t.mean(0, keepdims=True), t.var(0, keepdims=True)))
        tr = pe._ensure_trainer(batch)
        xd, td = torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev)
        for _ in range(2):
            idx = torch.from_numpy(rng.randint(0, n, size=(E, batch)).astype(np.int32)).to(dev)
            tr.step(xd, td, idx.data_ptr(), batch, batch)
        w, b = tr.get_weights()
        for k, a in enumerate(list(w) + list(b)):
            out[f"train_{name}_{k}"] = np.asarray(a)
    return out


def _buffer_get(dev):
    """ModelBuffer.get() after a full-length rollout at a batch where the flatten's scalar tiles exceed 64 KB."""
    import bench
    from cmbpo_amd import synthetic
    task, B = "HalfCheetahSafe-v2", 33000
    w = bench.build_world(0, task)
    sampler, pool, env, policy = bench.build_hip(w, task, B, torch.device(dev))
    start = torch.from_numpy(synthetic.start_states(np.random.default_rng(11), B, task)).to(dev)
    _, res = bench.rollout_phase(sampler, pool, start)
    names = ("obs", "act", "adv", "cadv", "ret", "cret", "logp", "val", "cval", "cost", "ls", "mu")
    return {f"get_{k}": r.cpu().numpy() for k, r in zip(names, res)}


def _fvp(dev):
    """A Fisher-vector product of the policy update at 50 k samples."""
    from worlds import make_update_batch
    from cmbpo_amd.cpo_update import PolicyOps
    rng = np.random.default_rng(9)
    D, A = 29, 8
    params, batch = make_update_batch(rng, 50000, D, A, 128, 0.3, 1.0, 35)
    ops = PolicyOps(D, A, 128, device=dev)
    ops.set_params(params)
    ops.bind(batch["obs"], batch["act"], batch["adv"], batch["cadv"], batch["logp_old"], batch["cost"], batch["mu_old"],
             batch["log_std_old"])
    return {"fvp": ops.fvp(rng.standard_normal(params.shape).astype(np.float32))}


def run_on(index):
    """Every family on cuda:<index>, made current for the whole run; name -> numpy result."""
    dev = f"cuda:{index}"
    out = {}
    with torch.cuda.device(index):
        out.update(_ens_forward(dev, paths=(2, 1, 0)))
        out.update(_critic_big(dev))
        out.update(_train(dev))
        out.update(_buffer_get(dev))
        out.update(_fvp(dev))
        torch.cuda.synchronize()
    return out


def assert_same(first, second):
    assert first.keys() == second.keys()
    for k in first:
        if k in ("get_adv", "get_cadv"):
            np.testing.assert_allclose(second[k], first[k], rtol=1e-4, atol=1e-5, err_msg=k)
        else:
            np.testing.assert_array_equal(second[k], first[k], err_msg=k)


def test_every_large_lds_kernel_runs_on_a_second_device(hip_lib):
    if not torch.cuda.is_available() or torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    assert_same(run_on(0), run_on(1))
