"""Cost of the sample weights in the policy-update kernels, on the GPU: at N = 50 000 and 3 400 000 samples a
Fisher-vector product (on saved activations, as the update runs it), a gradient pass and 80 iterations of the first-order
loop, each without and with weights on the same handle, alternating, `--rounds` times; and cmbpo_buffer_trust_weights on a
full model buffer of 100 000 branches x 34 steps.  Times are HIP events on the launch stream, milliseconds.

    python tools/probe_policy_weights.py --out profiles/r10/policy_weights.json [--bench-dir DIR]

--bench-dir: a directory of `parent_<k>.json` / `tree_<k>.json` files, each the JSON line of `bench.py --full` run on the
parent commit / on this tree (alternating, one GPU visit); their `cpo_update` blocks are folded into the output.
"""
import argparse
import ctypes as C
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cmbpo_amd  # noqa: E402,F401
from cmbpo_amd import _lib, synthetic  # noqa: E402
from cmbpo_amd.cpo_policy import GaussianActor  # noqa: E402
from cmbpo_amd.cpo_update import PolicyOps  # noqa: E402
from cmbpo_amd.modelbuffer import ModelBuffer  # noqa: E402

D, A, H = 29, 8, 128


def events(fn, reps):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def make_batch(n, params, gen):
    """a consistent batch from the policy itself: actions drawn from it, logp_old / mu_old / log_std_old its own"""
    dev = "cuda:0"
    actor = GaussianActor(D, A, (H, H), device=dev)
    actor.set_params(params)
    obs = torch.randn(n, D, device=dev, generator=gen)
    eps = torch.randn(n, A, device=dev, generator=gen)
    out = {"pi": torch.empty(n, A, device=dev), "logp_pi": torch.empty(n, device=dev), "mu": torch.empty(n, A, device=dev),
           "log_std": torch.empty(n, A, device=dev)}
    actor.forward_device(obs, eps, out)
    adv = torch.randn(n, device=dev, generator=gen)
    cadv = torch.randn(n, device=dev, generator=gen)
    cost = (torch.rand(n, device=dev, generator=gen) < 0.05).float()
    w = torch.exp(torch.empty(n, device=dev).uniform_(float(np.log(1 / 64)), float(np.log(64)), generator=gen))
    return [obs, out["pi"], adv, cadv, out["logp_pi"], cost, out["mu"], out["log_std"]], w


def probe_n(n, rounds):
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(n)
    params = np.concatenate([p.reshape(-1) for p in synthetic.policy_params(np.random.default_rng(2), D, A, H)]).astype(np.float32)
    batch, w = make_batch(n, params, gen)
    ops = PolicyOps(D, A, H, device="cuda:0")
    cfg = ops.ppo_cfg(pi_lr=1e-6, target_kl=1e9)          # the gate never stops the loop
    res = {k: {"unweighted": [], "weighted": []} for k in ("fvp_ms", "grad_ms", "ppo_run_80_ms")}

    def run_ppo():
        ops.params.copy_(torch.from_numpy(params))
        ops.set_params(ops.params)
        ops.ppo_run(cfg, 80)

    for _ in range(rounds):
        for tag, wt in (("unweighted", None), ("weighted", w)):
            ops.set_params(params)
            ops.bind(*batch, weights=wt)
            ops.set_penalty_param(0.5)
            ops.grad_dev(0, ops.work["g"], ops.sums)          # saves the activations
            ops.dirv.normal_()
            res["fvp_ms"][tag].append(events(lambda: ops.fvp_raw(ops.dirv), 10 if n <= 100000 else 5))
            res["grad_ms"][tag].append(events(lambda: ops.grad_dev(0, ops.work["g"], ops.sums), 10 if n <= 100000 else 5))
            res["ppo_run_80_ms"][tag].append(events(run_ppo, 2 if n <= 100000 else 1))
            st = ops.ppo_state.cpu().numpy()
            assert st[_lib.PPO_ST_STOP] == 0 and st[_lib.PPO_ST_ITERS] == 80, st[:4]
    for k, v in res.items():
        v["median_unweighted"] = float(np.median(v["unweighted"]))
        v["median_weighted"] = float(np.median(v["weighted"]))
        v["weighted_over_unweighted"] = v["median_weighted"] / v["median_unweighted"]
    res["n"] = n
    return res


def probe_trust(B=100000, T=34, reps=20):
    buf = ModelBuffer(B, D, A, T, device="cuda:0", iv_gae=True)
    buf.initialize({"mu": [A], "log_std": [A]})
    buf.set_trust_weights(1e-2)
    dev = buf.device
    z, zD, zA = torch.zeros(B, device=dev), torch.zeros(B, D, device=dev), torch.zeros(B, A, device=dev)
    var = torch.rand(B, device=dev) * 1e-2
    for _ in range(T):
        buf.store_multiple(zD, zA, zD, z, z, z, z, var, z, {"mu": zA, "log_std": zA}, np.zeros(B, bool))
    buf.finish_path_multiple(np.ones(B, bool), np.zeros(B, np.float32), np.zeros(B, np.float32))
    n = B * T
    assert buf.size == n
    out = torch.empty(n, device=dev)
    buf._call("cmbpo_buffer_prepare", buf.t["offsets"].data_ptr(), buf.t["stats"].data_ptr())
    ms = events(lambda: buf._call("cmbpo_buffer_trust_weights", buf.t["offsets"].data_ptr(), C.c_double(1e-2), out.data_ptr()), reps)
    torch.cuda.synchronize()
    assert float(out.min()) > 0 and float(out.max()) <= 1
    # bytes the kernel must move: the float64 variance table and the lengths in, the float32 weights out
    return {"samples": n, "ms": ms, "min_bytes": n * 12 + B * 8, "gb_per_s": (n * 12 + B * 8) / ms / 1e6}


def fold_bench(d):
    out = {"parent": [], "tree": []}
    for side in out:
        for f in sorted(glob.glob(os.path.join(d, side + "_*.json"))):
            try:
                line = [ln for ln in open(f).read().splitlines() if ln.startswith("{")][-1]
                upd = json.loads(line)["cpo_update"]
            except (IndexError, KeyError, ValueError):
                continue
            out[side].append({"file": os.path.basename(f),
                              **{t + "_" + k: upd[t][k] for t in ("constrained", "unconstrained") for k in ("ms_50k", "ms_full", "fvp_ms_full")}})
    keys = sorted(out["parent"][0]) if out["parent"] else []
    summary = {}
    for k in keys:
        if k == "file":
            continue
        p, t = [r[k] for r in out["parent"]], [r[k] for r in out["tree"]]
        if p and t:
            summary[k] = {"parent_median": float(np.median(p)), "parent_spread": float(max(p) - min(p)),
                          "tree_median": float(np.median(t)), "tree_spread": float(max(t) - min(t)),
                          "tree_minus_parent": float(np.median(t) - np.median(p))}
    out["summary"] = summary
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "policy_weights.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[50000, 3400000])
    ap.add_argument("--bench-dir", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_policy_weights.py needs a GPU")
    res = {"what": "sample weights in the policy-update kernels: weighted against unweighted on one handle, HIP events, ms",
           "device": torch.cuda.get_device_name(0), "matrix_path": int(_lib.lib().cmbpo_get_pi_matrix_path()),
           "policy": "%d -> %d -> %d -> %d" % (D, H, H, A), "rounds": a.rounds,
           "sizes": [probe_n(n, a.rounds) for n in a.sizes], "trust_weights": probe_trust()}
    if a.bench_dir:
        res["bench_full_cpo_update_unweighted"] = fold_bench(a.bench_dir)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
