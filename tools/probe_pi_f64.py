"""The policy-update kernels against float64, every case of tests/test_pi_f64_gpu.py once on both matrix paths (A smallest shapes,
A2 two tiles per workgroup, B ranges, C a small batch after a large one, W sample weights, PPO the first-order gradient, D the CG
solve): one JSON record per (part, case, path, mode, block) -- the worst of the mode's vectors on that block, 'sums' for its loss
sums -- with err_hip, the yardstick max(e32, mean e32, FLOOR) of the float32 reference and their ratio.  The worst ratio over the
plain cases (A, A2, C) of the f16 path is what MARGIN of tests/pi_f64_ref.py is set from (twice that, rounded up to a power of
two), CG_MARGIN likewise from part D; nothing here asserts a bound (what the helpers hold exact -- counts, cost sums, the use of
saved activations -- is listed under `failures` when it does not hold).  Last, the sanity check of the yardstick: the three
single-tile A cases with W1 replaced by its one-piece rounding IN THE PARAMETERS handed to PolicyOps (the kernels are sound, the
parameters damaged) against the float64 reference of the undamaged parameters -- their worst ratio must lie far above MARGIN.
    python tools/probe_pi_f64.py [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import cmbpo_amd  # noqa: F401
from cmbpo_amd import _lib
import pi_f64_ref as R

records, worst, sanity, failures = [], {}, [], []
PATHS = ((1, "splitf16"), (0, "fp32mfma"))


def add(part, c, path, recs):
    """one record per (case, path, mode, block): the worst of the mode's vectors on that block ('sums': of its loss sums)"""
    top, agg = 0.0, {}
    for mode, name, err, yard in recs:
        ratio = err / yard
        block = name.split("/")[-1] if name.split("/")[-1] in R.BLOCKS else "sums"
        if (mode, block) not in agg or ratio > agg[(mode, block)][0]:
            agg[(mode, block)] = (ratio, name, err, yard)
        for key in ("%s/%s/%s/h%d" % (part, mode, path, c.hidden), "%s/%s" % (part, path)):
            worst[key] = max(worst.get(key, 0.0), ratio)
        top = max(top, ratio)
    for (mode, block), (ratio, name, err, yard) in agg.items():
        records.append([part, R.case_id(c), path, mode, block, float("%.4g" % ratio), name, float("%.4g" % err), float("%.4g" % yard)])
    print(part, R.case_id(c), path, "worst ratio %.2f" % top, flush=True)


def modes(c, ops=None):
    ref = R.reference_of(c)
    ops = R.make_ops(ref) if ops is None else ops
    R.bind(ops, ref)
    return ref, R.gpu_modes(ops, ref)


def plain_case(part, c, path):
    ref, got = modes(c)
    add(part, c, path, R.mode_records(ref, got))


def small_after_big(part, c, path):
    big = R.reference_of(R.big_case_of(c))
    ops = R.make_ops(big)
    R.bind(ops, big)
    R.gpu_modes(ops, big)
    ref, got = modes(c, ops)
    add(part, c, path, R.mode_records(ref, got))


def ppo_case(part, c, path):
    ref = R.reference_of(c)
    ops = R.make_ops(ref)
    R.bind(ops, ref)
    add(part, c, path, R.ppo_records(ref, R.gpu_ppo(ops, ref)))


def cg_case(part, c, path):
    ref = R.reference_of(c)
    fig = ref.cg_figures()
    ops = R.make_ops(ref)
    R.bind(ops, ref)
    add(part, c, path, [("cg", "x", R.whole_error(R.gpu_cg(ops, ref), fig["x64"]), max(fig["e32"], R.FLOOR))])


def one_piece_case(part, c, path):
    """the yardstick's sanity check: sound kernels, W1 of the parameters cut to one f16 piece"""
    ref = R.reference_of(c)
    ops = R.make_ops(ref)
    R.bind(ops, ref)
    cut = [R.cut_block(x, c.D, c.A, c.hidden, 2).astype(np.float32) for x in (ref.theta, ref.p)]
    recs = [r for r in R.mode_records(ref, R.gpu_modes(ops, ref, theta=cut[0], p=cut[1]))
            if r[1].split("/")[0] in ("g", "b") or r[1].startswith("fvp@old/dense")]
    top = max(e / y for _, _, e, y in recs)
    sanity.append(dict(case=R.case_id(c), path=path, worst_ratio_with_one_piece_W1=top))
    print("sanity", R.case_id(c), path, "one-piece W1 in the parameters: worst ratio %.1f" % top, flush=True)


lib = _lib.lib()
before = lib.cmbpo_get_pi_matrix_path()
for flag, path in PATHS:
    lib.cmbpo_set_pi_matrix_path(flag)
    for part, cases, fn in (("A", R.CASES_A, plain_case), ("A2", R.CASES_A2, plain_case), ("B", R.CASES_B, plain_case),
                            ("W", R.CASES_W, plain_case), ("C", R.CASES_C, small_after_big), ("PPO", R.CASES_PPO, ppo_case),
                            ("D", R.CASES_D, cg_case), ("sanity", R.SINGLE_TILE_A, one_piece_case)):
        for c in cases:
            try:
                fn(part, c, path)
            except AssertionError as e:      # (an exactness check of the helpers; a HIP error ends the run)
                failures.append(dict(part=part, case=R.case_id(c), path=path, error=str(e)[:400]))
                print("FAILED", part, R.case_id(c), path, str(e)[:400], flush=True)
lib.cmbpo_set_pi_matrix_path(before)

rule = lambda x: float(2.0 ** np.ceil(np.log2(2.0 * x)))
plain = max(worst["%s/splitf16" % p] for p in ("A", "A2", "C"))
res = dict(command="python tools/probe_pi_f64.py " + " ".join(os.path.basename(a) for a in sys.argv[1:]), device=torch.cuda.get_device_name(0),
           compute_units=R.cu_count(), floor=R.FLOOR, worst_ratio=dict(sorted(worst.items())),
           worst_ratio_plain_cases_A_A2_C_f16_path=plain, margin_by_the_rule=rule(plain), margin_in_the_helper=R.MARGIN,
           cg_worst_ratio_f16_path=worst["D/splitf16"], cg_margin_by_the_rule=rule(worst["D/splitf16"]),
           cg_margin_in_the_helper=R.CG_MARGIN, one_piece_sanity=sanity, failures=failures,
           record_fields=["part", "case", "path", "mode", "block", "ratio", "worst_vector", "err_hip", "yardstick"])
print(json.dumps(res))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as fh:
        fh.write(json.dumps(res, indent=1)[:-2] + ',\n "records": [\n' + ",\n".join("  " + json.dumps(r) for r in records) + "\n ]\n}\n")
