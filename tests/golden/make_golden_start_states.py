"""Generate golden G13: the start-state sampling chain of the trainer loop (algorithms/cmbpo.py:239-251) on an archive
that has wrapped around, recorded from the REFERENCE's own CPOBuffer (buffers/cpobuffer.py).

Usage (build container only, like make_golden.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_start_states.py

Writes tests/golden/g13_start_states.npz (data only).  The archive holds 100 slots and takes five dumps: epochs 2, 3, 5
(30 + 20 + 25 samples), then epoch 6 twice (15, then 12 that no longer fit: the pointer wraps to 0).  Afterwards epoch 6
is two runs ([0, 12) and [75, 90)), the overwritten epoch 2 is partly alive ([12, 30)) and slots [90, 100) are empty.
Per case: epochs_list, boltz_dist(kls, alpha) for two alphas and, under np.random.seed(s), the rows
distributed_batch_from_archive returned, the indices behind them (np.random.choice called as the reference calls it,
from the same seed; checked against the rows) and the uniforms that call consumed (np.random.random_sample from the same
seed).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (the stubs behind which the reference imports; puts the reference on sys.path)


def gen_start_states(out):
    from buffers.cpobuffer import CPOBuffer
    rng = np.random.default_rng(1313)
    D, A, N = 5, 2, 100
    buf = CPOBuffer(size=40, archive_size=N, observation_space=mg._Space(D), action_space=mg._Space(A))
    buf.initialize({"mu": [A], "log_std": [A]}, gamma=0.99, lam=0.95, cost_gamma=0.97, cost_lam=0.5)
    plan = [(2, [12, 18]), (3, [20]), (5, [10, 15]), (6, [15]), (6, [5, 7])]          # (epoch tag, path lengths) per dump
    n = sum(sum(ls) for _, ls in plan)
    data = dict(D=D, A=A, N=N, obs=rng.standard_normal((n, D)).astype(np.float32),
                act=rng.standard_normal((n, A)).astype(np.float32), rew=rng.standard_normal(n).astype(np.float32),
                val=rng.standard_normal(n).astype(np.float32), cost=(rng.random(n) < 0.3).astype(np.float32),
                cval=rng.standard_normal(n).astype(np.float32), logp=rng.standard_normal(n).astype(np.float32),
                mu=rng.standard_normal((n, A)).astype(np.float32),
                log_std=(-0.5 + 0.1 * rng.standard_normal((n, A))).astype(np.float32),
                last=rng.standard_normal((8, 2)).astype(np.float32),
                plan_epochs=np.array([e for e, _ in plan]), plan_lengths=np.array([len(ls) for _, ls in plan]),
                path_lengths=np.array([l for _, ls in plan for l in ls]))
    i = p = 0
    for epoch, ls in plan:
        for L in ls:
            for _ in range(L):
                buf.store(data["obs"][i], data["act"][i], data["obs"][i] + 1, data["rew"][i], data["val"][i], data["cost"][i],
                          data["cval"][i], data["logp"][i], {"mu": data["mu"][i], "log_std": data["log_std"][i]}, False, epoch)
                i += 1
            buf.finish_path(data["last"][p, 0:1], data["last"][p, 1:2])
            p += 1
        buf.get()
    assert buf.archive_full and buf.archive_ptr == 12 and buf.arch_size == 90
    ea = np.asarray(buf.epoch_archive)
    assert list(np.flatnonzero(np.diff(ea)) + 1) == [12, 30, 50, 75, 90], "the runs the docstring promises"
    data["arch_size"], data["epochs_list"] = buf.arch_size, np.array(buf.epochs_list)
    data["max_ep"], data["min_ep"] = buf.max_ep, buf.min_ep
    data["arch_epochs"] = ea.astype(np.int64)
    data["arch_observations"] = buf.obs_archive
    data["arch_mu"], data["arch_log_std"] = buf.pi_info_archive["mu"], buf.pi_info_archive["log_std"]
    kls = np.array([0.31, 0.02, 0.5, 0.1])
    data["kls"] = kls
    alphas = np.array([1.0, 2.5])
    seeds, sizes = np.array([5, 11, 23]), np.array([23, 64, 257])
    data["alphas"], data["seeds"], data["sizes"] = alphas, seeds, sizes
    for a, alpha in enumerate(alphas):
        dist = buf.boltz_dist(kls, alpha=alpha)
        data[f"boltz{a}"] = dist
        for s, size in zip(seeds, sizes):
            np.random.seed(s)
            b = buf.distributed_batch_from_archive(int(size), dist, fields=["observations", "pi_infos"])
            np.random.seed(s)
            idx = np.random.choice(np.arange(buf.archive_size), size=int(size), p=dist)      # cpobuffer.py:454
            np.random.seed(s)
            u = np.random.random_sample(int(size))
            assert np.array_equal(buf.obs_archive[idx], b["observations"]) and np.array_equal(
                buf.pi_info_archive["mu"][idx], b["mu"])
            assert np.all(ea[idx] >= 0)
            data[f"draw{a}_{s}_obs"], data[f"draw{a}_{s}_idx"], data[f"draw{a}_{s}_u"] = b["observations"], idx, u
    np.savez_compressed(os.path.join(out, "g13_start_states.npz"), **data)
    print("start states: archive", buf.arch_size, "of", N, "epochs", list(buf.epochs_list), "runs at", [0, 12, 30, 50, 75, 90])


if __name__ == "__main__":
    mg.install_stubs()
    gen_start_states(HERE)
