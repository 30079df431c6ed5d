"""What the critics' own disagreement costs in the critic launch of a rollout step: cmbpo_critic_pair_predict alone,
HIP events around REPS back-to-back launches, AntSafe observations (29), E = 3 members, a row list, after warm-up; alternating
rounds in one process, the first two timed rounds of a part dropped.
  (a) with --other-lib PATH (another build of libcmbpo_hip.so, e.g. the parent commit's): the plain entry there against the
      plain entry here at 1000 and 100 000 rows -- a launch without the feature must not pay for it.  The yardstick is the
      spread the other library shows against itself over its own repeats, (max - min) / median; the median ratio has to lie
      within 1 + twice that.
  (b) here: cmbpo_critic_pair_predict against cmbpo_critic_pair_predict_var with kappa = (0, 0) and with kappa = (0.75, 1.5) at
      1000, 24 575 (the last size of the one-wave-per-member kernel), 24 576 (the first of the member-after-member kernel, whose
      VDIS instance takes 448-row chunks at these dims) and 100 000 rows.  Reported, not gated.
The exit status is non-zero if (a) is outside; the record is written either way.
    python tools/probe_value_disagreement.py [out.json] [--other-lib PATH] [--pairs K] [--reps R]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import cmbpo_amd  # noqa: F401
from cmbpo_amd import _lib, synthetic
from cmbpo_amd.pens import PE

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--other-lib")
ap.add_argument("--pairs", type=int, default=8)
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()

D, E, WARM, DROP = 29, 3, 200, 2
GATED, SIZES = (1000, 100000), (1000, 24575, 24576, 100000)
NMAX = max(SIZES)
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
obs = torch.from_numpy(rng.standard_normal((NMAX, D)).astype(np.float32)).to(dev)
idx = torch.arange(NMAX, dtype=torch.int32, device=dev)
nets = []
for _ in range(2):
    ws, bs = synthetic.ensemble_weights(rng, E, D, 128, 1, bias_scale=0.1)
    m = PE(D, 1, hidden_dims=(128, 128), num_networks=E, num_elites=2, loss="MSE", use_scaler_in=True, use_scaler_out=True,
           device="cuda:0")
    m.set_weights(ws, bs, synthetic.scaler(rng, D), synthetic.scaler(rng, 1))
    nets.append(m)
f = dict(dtype=torch.float32, device=dev)
out = [torch.empty(NMAX, **f) for _ in range(4)]

here = _lib.lib()
other = None
if args.other_lib:
    # (the handles are plain records of device addresses: another build of the same struct reads them as well)
    other = C.CDLL(os.path.abspath(args.other_lib))
    other.cmbpo_critic_pair_predict.restype, other.cmbpo_critic_pair_predict.argtypes = _lib.SIGNATURES["cmbpo_critic_pair_predict"]
    other.cmbpo_last_error.restype = C.c_char_p


def launch(lib, n, kappa):
    """kappa None: cmbpo_critic_pair_predict; else cmbpo_critic_pair_predict_var with those coefficients."""
    a = (nets[0].mlp.handle, nets[1].mlp.handle, obs.data_ptr(), D, idx.data_ptr(), None, n)
    if kappa is None:
        rc = lib.cmbpo_critic_pair_predict(*a, out[0].data_ptr(), out[1].data_ptr(), _lib.current_stream())
    else:
        rc = lib.cmbpo_critic_pair_predict_var(*a, kappa[0], kappa[1], out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                               out[3].data_ptr(), _lib.current_stream())
    if rc != 0:
        raise RuntimeError(lib.cmbpo_last_error())


def measure(cfg):
    """Microseconds per launch over args.reps back-to-back launches."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        launch(*cfg)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.reps


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def rounds(configs):
    us = {n: [] for n in configs}
    for n, cfg in configs.items():
        for _ in range(WARM):
            launch(*cfg)
    torch.cuda.synchronize()
    for rnd in range(DROP + args.pairs):
        for n, cfg in configs.items():
            t_us = measure(cfg)
            if rnd >= DROP:
                us[n].append(t_us)
    return us


def values(cfg):
    for o in out:
        o.fill_(float("nan"))
    launch(*cfg)
    torch.cuda.synchronize()
    return [o[:cfg[1]].clone().view(torch.int32) for o in out[:2]]


res = dict(command="python tools/probe_value_disagreement.py " + " ".join(sys.argv[1:]), obs_dim=D, ensemble=E, reps=args.reps,
           pairs=args.pairs, warmups=WARM, dropped_rounds=DROP, device=torch.cuda.get_device_name(0), a={}, b={})
ok = True
for n in SIZES:
    plain, zero = values((here, n, None)), values((here, n, (0.0, 0.0)))
    assert all(torch.equal(p, z) for p, z in zip(plain, zero)), n
    if other is not None:
        assert all(torch.equal(p, z) for p, z in zip(plain, values((other, n, None)))), n
res["kappa0_values_bit_identical_to_plain_entry"] = True
if other is not None:
    res["plain_values_bit_identical_to_other_lib"] = True
    for n in GATED:
        us = rounds({"other_plain": (other, n, None), "here_plain": (here, n, None)})
        sp = spread(us["other_plain"])
        ratio = statistics.median(us["here_plain"]) / statistics.median(us["other_plain"])
        res["a"][str(n)] = dict(us_per_launch=us, median_us={k: statistics.median(v) for k, v in us.items()}, other_spread=sp,
                                here_spread=spread(us["here_plain"]), median_ratio_here_over_other=ratio, gate=2.0 * sp,
                                within_gate=bool(ratio - 1.0 <= 2.0 * sp))
        ok = ok and res["a"][str(n)]["within_gate"]
        print("(a) %6d rows, plain entry here / other: %.4f (gate: 1 + %.4f) -> %s" % (
            n, ratio, 2.0 * sp, "within" if res["a"][str(n)]["within_gate"] else "OUTSIDE"))
for n in SIZES:
    us = rounds({"plain": (here, n, None), "kappa0": (here, n, (0.0, 0.0)), "pessimistic": (here, n, (0.75, 1.5))})
    med = {k: statistics.median(v) for k, v in us.items()}
    res["b"][str(n)] = dict(us_per_launch=us, median_us=med, spread={k: spread(v) for k, v in us.items()},
                            median_ratio_kappa0_over_plain=med["kappa0"] / med["plain"],
                            median_ratio_pessimistic_over_plain=med["pessimistic"] / med["plain"])
    print("(b) %6d rows, VDIS / plain: kappa 0 %.4f, kappa > 0 %.4f (%.2f / %.2f / %.2f us)" % (
        n, res["b"][str(n)]["median_ratio_kappa0_over_plain"], res["b"][str(n)]["median_ratio_pessimistic_over_plain"],
        med["plain"], med["kappa0"], med["pessimistic"]))
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
if not ok:
    sys.exit("outside: a")
