"""The training step's gradients against float64, every case of tests/test_ens_train_f64_gpu.py once (A first step, B ranges inside
one batch, C a small batch on a 2048-row trainer, D Adam element by element): one JSON record per (case, tensor) with err_hip
(the HIP gradient's max |g - g64| / max |g64|, the worst member), e32 (the float32 torch reference's same error), their ratio
err_hip / max(e32, FLOOR) and f16_paths.  The worst ratio over the plain cases (A and C) is what MARGIN of
tests/ens_train_f64_ref.py is set from (twice that, rounded up to a power of two); nothing here asserts a bound.
    python tools/probe_ens_train_f64.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import cmbpo_amd  # noqa: F401
import ens_train_f64_ref as R

records, adam, worst = [], [], {}


def add(part, c, name, err_hip, e32):
    ratio = err_hip / max(e32, R.FLOOR)
    records.append(dict(part=part, case=R.case_id(c), tensor=name, err_hip=err_hip, e32=e32, ratio=ratio, f16_paths=c.paths,
                        fused=bool(c.fused)))
    key = "%s/%s" % (part, "fused" if c.fused else "f16_paths=%d,H=%d" % (c.paths, c.H))
    worst[key] = max(worst.get(key, 0.0), ratio)
    worst[part] = max(worst.get(part, 0.0), ratio)


for part, cases in (("A", R.CASES_A), ("B", R.CASES_B)):
    for c in cases:
        ref = R.reference_of(c)
        fig = ref.figures()
        errs, e_hold, e_boot = R.gpu_first_step_errors(ref)
        for name, e32 in zip(R.TENSORS, fig["e32"]):
            add(part, c, name, float(errs[name].max()), e32)
        add(part, c, "loss_holdout", float(e_hold.max()), fig["e32_hold"])
        add(part, c, "loss_bootstrap", float(e_boot.max()), fig["e32_boot"])
        print(part, R.case_id(c), "worst ratio %.2f" % max(r["ratio"] for r in records[-8:]), flush=True)
for c in R.CASES_C:
    ref = R.reference_of(c)
    errs = R.gpu_small_batch_errors(ref)
    for name, e32 in zip(R.TENSORS, ref.figures()["e32"]):
        add("C", c, name, float(errs[name].max()), e32)
    print("C", R.case_id(c), "worst ratio %.2f" % max(r["ratio"] for r in records[-6:]), flush=True)
for c in R.CASES_D:
    ref = R.reference_of(c)
    d = R.gpu_adam(ref)
    d["pe"]._weights_on_device = True
    e_hip, e_32 = R.forward_errors(d["pe"], np.array(ref.x[:40]))
    adam.append(dict(part="D", case=R.case_id(c), f16_paths=c.paths, fused=bool(c.fused), steps_done=d["got"]["steps_done"],
                     errors=dict(zip(("W0", "W1", "W2", "b0", "b1", "b2"), R.adam_errors(d))),
                     forward_err_hip=e_hip.max(axis=1).tolist(), forward_err_float32=e_32.max(axis=1).tolist()))
    print("D", adam[-1], flush=True)

plain = max(worst["A"], worst["C"])
res = dict(command="python tools/probe_ens_train_f64.py " + " ".join(sys.argv[1:]), device=torch.cuda.get_device_name(0),
           floor=R.FLOOR, worst_ratio=worst, worst_ratio_plain_cases_A_and_C=plain,
           margin_by_the_rule=float(2.0 ** np.ceil(np.log2(2.0 * plain))), margin_in_the_helper=R.MARGIN, records=records, adam=adam)
print(json.dumps({k: v for k, v in res.items() if k not in ("records", "adam")}))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
