"""The vector-algebra and GAE kernels (csrc/vec_ops.hip, csrc/gae_segments.hip) against their float64 restatements: what
profiles/r22/vec_gae.json holds.

First the measurement CG_STEP_MARGIN of tests/vec_gae_ref.py is set from: cmbpo_cg_init and ten cmbpo_cg_step on the dense SPD
operator of every size in CG_DENSE_SIZES against float64 CG, err = max |x - x64| / max |x64|, beside e32, the same for
oracle/refupdate.cg run in float32 on the same operator; the constant is twice the worst err / max(e32, 6e-7), rounded up to a
power of two.  Nothing is asserted there.  Then tests/test_gae_segments_gpu.py and tests/test_vec_ops_gpu.py run in this process
and every worst error they recorded, as a fraction of its derived bound, is written out (`fractions`; for gae_segments the number
of elements that differ from the restatement).
    python tools/probe_vec_gae.py [out.json]"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pytest

import cmbpo_amd  # noqa: F401
from cmbpo_amd import _lib
import vec_gae_ref as V
import test_vec_ops_gpu as T

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r22", "vec_gae.json")
cg = []
for P in V.CG_DENSE_SIZES:
    err, e32, ratio = T.cg_dense_ratio(_lib.lib(), P)
    cg.append(dict(P=P, err=float("%.4g" % err), e32=float("%.4g" % e32), ratio=float("%.4g" % ratio)))
    print("cg dense P = %d: err %.3g / max(e32 %.3g, %g) = %.3f" % (P, err, e32, V.FLOOR, ratio), flush=True)
worst = max(r["ratio"] for r in cg)
margin = 2.0 ** math.ceil(math.log2(2.0 * worst))
print("worst ratio %.4g -> CG_STEP_MARGIN %g (tests/vec_gae_ref.py holds %r)" % (worst, margin, V.CG_STEP_MARGIN), flush=True)

V.RECORDS.clear()
tests = [os.path.join(ROOT, "tests", f) for f in ("test_gae_segments_gpu.py", "test_vec_ops_gpu.py")]
rc = int(pytest.main(["-m", "gpu", "-q", "-s", "-p", "no:cacheprovider"] + tests))
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    json.dump(dict(cg_dense=cg, cg_step_worst_ratio=worst, cg_step_margin_rule=margin, cg_step_margin=V.CG_STEP_MARGIN,
                   floor=V.FLOOR, pytest_exit=rc,
                   fractions={k: float("%.4g" % v) for k, v in sorted(V.RECORDS.items())}), f, indent=1)
    f.write("\n")
print("wrote", out, "pytest exit", rc)
sys.exit(rc)
