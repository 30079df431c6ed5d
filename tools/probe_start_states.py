"""Start states of an imagined-rollout round: the host chain (algorithms/cmbpo.py:239-251 as cmbpo.py runs it with
start_state_sampling='host': epoch_batch, compute_DKL, boltz_dist, distributed_batch_from_archive, upload into cur_obs)
against CPOBuffer.sample_start_states on the device mirror, next to a rollout phase of the same batch size.
Archive: 3e5 samples in 60 epochs (one wrap-around), AntSafe dimensions.  Medians over 20 rounds after 3 warm-ups.
    python tools/probe_start_states.py [out.json] [B ...]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from cmbpo_amd import synthetic
from cmbpo_amd.cpobuffer import CPOBuffer

TASK, N, EPOCHS, ROUNDS, WARM = "AntSafe-v2", 300000, 60, 20, 3
out_path = sys.argv[1] if len(sys.argv) > 1 else None
sizes = [int(a) for a in sys.argv[2:]] or [1000, 100000]
dev = torch.device("cuda:0")
w = bench.build_world(0, TASK)
D, A = w["obs_dim"], w["act_dim"]


def archive():
    """The archive after one wrap-around: the newest three epochs at the start, one of them also at the end, an empty tail."""
    rng = np.random.default_rng(3)
    buf = CPOBuffer(8, N, bench._Space(D), bench._Space(A), device=dev)
    buf.initialize({"mu": [A], "log_std": [A]})
    tags = [EPOCHS + 2, EPOCHS + 3, EPOCHS + 4] + list(range(5, EPOCHS + 2)) + [EPOCHS + 2]
    szs = rng.integers(int(0.6 * N / len(tags)), N // len(tags), len(tags))
    pos = 0
    for tag, sz in zip(tags, szs):
        buf.arch_dict["epochs"][pos:pos + sz] = tag
        pos += int(sz)
    buf.max_pointer = pos
    buf.arch_dict["observations"][:] = synthetic.start_states(rng, N, TASK)
    buf.pi_info_archive["mu"][:] = (0.3 * rng.standard_normal((N, A))).astype(np.float32)
    buf.pi_info_archive["log_std"][:] = -0.5
    return buf


def median_ms(fn, events=False):
    ts = []
    for k in range(WARM + ROUNDS):
        torch.cuda.synchronize()
        if events:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            t = s.elapsed_time(e)
        else:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t = (time.perf_counter() - t0) * 1e3
        if k >= WARM:
            ts.append(t)
    return statistics.median(ts)


buf = archive()
res = dict(task=TASK, archive=N, epochs=len(buf.epochs_list), rounds=ROUNDS, warmups=WARM, sizes={})
for B in sizes:
    sampler, pool, env, policy = bench.build_hip(w, TASK, B, dev, None, bench.MAXROLL, "schedule")
    pool.reset(B)
    cur = pool.t["cur_obs"]

    def host():
        ep_b = buf.epoch_batch(batch_size=B, epochs=buf.epochs_list, fields=['observations', 'pi_infos'])
        kls = np.clip(policy.compute_DKL(ep_b['observations'], ep_b['mu'], ep_b['log_std']), a_min=0, a_max=None)
        dist = buf.boltz_dist(kls, alpha=1)
        b = buf.distributed_batch_from_archive(B, dist, fields=['observations', 'pi_infos'])
        cur.copy_(torch.from_numpy(np.ascontiguousarray(b['observations'], dtype=np.float32)).to(dev))

    def device():
        buf.sample_start_states(policy, B, alpha=1, out=cur)

    start = torch.from_numpy(synthetic.start_states(np.random.default_rng(1), B, TASK)).to(dev)
    t_host = median_ms(host)
    buf.enable_device_archive()
    t_dev_events = median_ms(device, events=True)
    t_dev_wall = median_ms(device)
    t_roll = median_ms(lambda: bench.rollout_phase(sampler, pool, start))
    res["sizes"][str(B)] = dict(host_chain_ms=t_host, device_call_ms=t_dev_events, device_call_wall_ms=t_dev_wall,
                                rollout_phase_ms=t_roll)
    print(f"B={B}: host chain {t_host:.3f} ms, device call {t_dev_events:.3f} ms (HIP events; {t_dev_wall:.3f} ms wall), "
          f"rollout phase {t_roll:.3f} ms", flush=True)
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
