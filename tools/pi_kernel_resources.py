#!/usr/bin/env python
"""Registers, scratch and LDS of every pi_kernel* instantiation (or, with --file / --kernels, of the kernels of another
source file whose demangled name matches a regular expression), as the compiler reports them
(-Rpass-analysis=kernel-resource-usage, the build's flags, no GPU needed), for several trees side by side.

    python tools/pi_kernel_resources.py --tree parent=/path/to/parent/checkout --tree tree=. \
        --out profiles/r25/kernel_resources_pi.tsv

A tree is `label=checkout[:extra flag]`.  One row per (instantiation, tree); the last template argument says whether the
instantiation takes sample weights (a tree from before the weights has only `false` rows).  Every row of the first tree must
be found unchanged in the others: the tool lists the ones that are not and exits 1.

    python tools/pi_kernel_resources.py --file ens_train.hip --kernels . --tree parent=... --tree tree=. --out ...
"""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402

CSRC = os.path.join("constrained-model-based-policy-optimization_amd", "csrc")
FIELDS = (("TotalSGPRs", "sgprs"), ("VGPRs", "vgprs"), ("AGPRs", "agprs"), ("ScratchSize [bytes/lane]", "scratch_bytes_per_lane"),
          ("Occupancy [waves/SIMD]", "waves_per_simd"), ("SGPRs Spill", "sgpr_spills"), ("VGPRs Spill", "vgpr_spills"),
          ("LDS Size [bytes/block]", "static_lds_bytes"))


def remarks(checkout, extra, src):
    cmd = [G.HIPCC] + G.HIP_FLAGS + G.FILE_FLAGS.get(src, []) + extra + ["-Rpass-analysis=kernel-resource-usage",
                                                                       "--cuda-device-only", "-c", src, "-o", os.devnull]
    return subprocess.run(cmd, cwd=os.path.join(checkout, CSRC), check=True, capture_output=True, text=True).stderr


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), check=True, capture_output=True, text=True).stdout.split("\n")
    clean = []
    for d in out[:len(names)]:
        d = d.replace("(anonymous namespace)::", "").replace("void ", "")
        clean.append(re.sub(r"\((?!\w+\)\d).*$", "", d))      # the parameter list goes, an enum template argument `(LossMode)2` stays
    return clean


def parse(text, kernels):
    rows, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        for key, col in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(key) + r": (\d+)", line)
            if m and cur is not None:
                cur[col] = int(m.group(1))
    names = list(rows)
    out = {}
    for n, d in zip(names, demangle(names)):
        if kernels.search(d):
            if d.startswith("pi_kernel") and d.count(",") == 2:      # a tree from before the weights: its instantiations are the unweighted ones
                d = d[:-1] + ", false>"
            out[d] = rows[n]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", action="append", required=True, help="label=checkout[:extra compiler flag]")
    ap.add_argument("--out", required=True)
    ap.add_argument("--file", default="policy_update.hip", help="source file under csrc/")
    ap.add_argument("--kernels", default="^pi_kernel", help="regular expression searched in the demangled kernel names")
    a = ap.parse_args()
    tables = []
    for spec in a.tree:
        label, rest = spec.split("=", 1)
        checkout, _, flag = rest.partition(":")
        tables.append((label, parse(remarks(os.path.abspath(checkout), [flag] if flag else [], a.file), re.compile(a.kernels))))
    cols = [c for _, c in FIELDS]
    with open(a.out, "w") as f:
        f.write("\t".join(["kernel", "tree"] + cols) + "\n")
        for k in sorted(set().union(*[set(t) for _, t in tables])):
            for label, t in tables:
                if k in t:
                    f.write("\t".join([k, label] + [str(t[k].get(c, "")) for c in cols]) + "\n")
    base = tables[0][1]
    bad = []
    for label, t in tables[1:]:
        for k, v in base.items():
            if t.get(k) != v:
                bad.append((label, k, v, t.get(k)))
    for b in bad:
        print("DIFFERS: %s %s %r -> %r" % b)
    print("%d instantiations in %s, %d rows differ in the other trees" % (len(base), tables[0][0], len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
