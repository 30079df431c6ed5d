"""Are the policy-update kernels of another build of the library (the parent commit's libcmbpo_hip.so) the kernels of this
tree, bit for bit -- and as fast?
  parity (default): CASES_A, CASES_A2, CASES_C and CASES_W of tests/pi_f64_ref.py through loss_grad(0), loss_grad(1), the
      Fisher-vector product (one before any loss_grad, three directions after it, at theta_old and at p) and evals, CASES_PPO
      through ppo_grad at its four (clipped, penalty) settings; every case on both matrix paths with keep_activations off and
      on (on: the products after loss_grad run the saved-activation instance, and their count is asserted).  Same seeded
      parameters and batch under both libraries.  Vectors and the MODE_PPO sums (ordered reductions) are compared bit for
      bit; the MODE_EVAL / MODE_GRAD sums (float64 atomics across workgroups) bit for bit where one workgroup ran (n <= 32),
      else to one ulp of float32, the type the update's host side hands them on in (cpo_update: F32(sums / n)).  The raw
      float64 sums of several workgroups are not repeatable below that: the atomics arrive in any order.  By how much is
      printed twice per line, in float64 ulps: this library against the other, and this library against a second run of
      itself.  One line per (case, path, keep); exit status 1 on any mismatch.
  --time: D = 29, A = 8 at N = 50 000 and N = 3 400 000, hidden 128 on both matrix paths and hidden 256: loss_grad, the product
      with and without saved activations, evals, and the first-order gradient with and without weights, each as HIP events
      around REPS calls (the reduction / scaling kernels that follow a pass included), the two libraries in alternating rounds
      (probe_column_weights.alternate).  Per kernel: median here / median other, and each side's (max - min) / median.
      A second set of handles of the OTHER library is timed with them (other_again): what it differs by from the first is what
      two sets of buffers differ by, whatever the code.
    python tools/probe_pi_parity.py [out.json] --other-lib PATH [--time] [--rounds 10]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np
import torch

import cmbpo_amd  # noqa: F401
from cmbpo_amd import _lib
from cmbpo_amd.cpo_update import PolicyOps
from probe_column_weights import alternate, library, other_library, spread

import pi_f64_ref as R


def plain_modes(ops, ref, keep):
    """{name: array} of every plain fetch on the bound batch (gpu_modes of the tests, for either setting of keep_activations)."""
    out = {}
    for at, params in (("old", ref.theta), ("off", ref.p)):
        ops.set_params(np.array(params))
        before = R._uses(ops)
        out["fvp@%s/dense/before" % at] = ops.fvp(np.array(ref.dirs["dense"]))
        out["g@" + at], out["sums_g@" + at] = ops.loss_grad(0)
        out["b@" + at], out["sums_b@" + at] = ops.loss_grad(1)
        for d in R.DIRECTIONS:
            out["fvp@%s/%s/after" % (at, d)] = ops.fvp(np.array(ref.dirs[d]))
        assert R._uses(ops) - before == (len(R.DIRECTIONS) if keep else 0), "saved-activation products: %d" % (R._uses(ops) - before)
    out["sums_ev"] = ops.evals()
    return out


def run_case(c, path, keep):
    """({name: array}, rows of the case) under the current library."""
    _lib.lib().cmbpo_set_pi_matrix_path(path)
    ref = R.reference_of(c)
    first = R.reference_of(R.big_case_of(c)) if c.after_big else ref
    ops = R.make_ops(first)
    ops.keep_activations = keep
    out = {}
    try:
        if c.after_big:
            R.bind(ops, first)
            out.update({"big/" + k: v for k, v in plain_modes(ops, first, keep).items()})
        R.bind(ops, ref)
        if c.ppo:
            for combo, (g, s) in R.gpu_ppo(ops, ref).items():
                out["ppo_g/clip%d_pen%g" % combo], out["ppo_sums/clip%d_pen%g" % combo] = g, s
        if not c.ppo or c.weighted:
            out.update(plain_modes(ops, ref, keep))
    finally:
        ops.__del__()
        _lib.lib().cmbpo_set_pi_matrix_path(1)
    return out, ref.n


def ulps(a, b, ftype, itype):
    a, b = np.ascontiguousarray(a, ftype), np.ascontiguousarray(b, ftype)
    return int(np.abs(a.view(itype).astype(np.int64) - b.view(itype).astype(np.int64)).max())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def parity(libs):
    cases = R.CASES_A + R.CASES_A2 + R.CASES_C + R.CASES_PPO      # (CASES_W: the weighted half of CASES_PPO, both ways)
    rows, bad = [], 0
    for c in cases:
        for path in (1, 0):
            for keep in (False, True):
                got = {}
                for which, handle in (("here", libs["here"]), ("other", libs["other"]), ("again", libs["here"])):
                    with library(handle):
                        got[which], n = run_case(c, path, keep)
                here, other, again = got["here"], got["other"], got["again"]
                diff, worst, noise = [], 0, 0
                for k in here:
                    atomic = k.startswith("sums_") or k.startswith("big/sums_")
                    rows_k = R.reference_of(R.big_case_of(c)).n if k.startswith("big/") else n
                    if atomic and rows_k > 32:
                        worst = max(worst, ulps(here[k], other[k], np.float64, np.int64))
                        noise = max(noise, ulps(here[k], again[k], np.float64, np.int64))
                        if ulps(here[k], other[k], np.float32, np.int32) > 1:
                            diff.append(k)
                    elif not (same_bits(here[k], other[k]) and same_bits(here[k], again[k])):
                        diff.append(k)
                finite = all(np.isfinite(v).all() for v in here.values())
                moved = any(float(np.abs(v).max()) > 0 for k, v in here.items() if k.startswith(("g@", "ppo_g/")))
                ok = not diff and finite and moved and set(here) == set(other)
                bad += not ok
                rows.append(dict(case=R.case_id(c), path="splitf16" if path else "fp32mfma", keep_activations=keep, results=len(here),
                                 differing=diff, atomic_sums_f64_ulps_here_other=worst,
                                 atomic_sums_f64_ulps_here_again=noise, ok=bool(ok)))
                print("%-34s %-9s keep %d: %3d results, %s; multi-workgroup atomic sums: %d float64 ulp to the other, %d to a second run%s"
                      % (R.case_id(c), rows[-1]["path"], keep, len(here), "identical" if not diff else "DIFFERENT " + ",".join(diff),
                         worst, noise, "" if ok else "   <-- MISMATCH"), flush=True)
    return dict(rows=rows, mismatches=bad)


def timed(libs, name, fn, reps):
    def run():
        with library(libs[name]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    return run


def timing(libs, rounds):
    from worlds import make_update_batch
    libs = dict(libs, other_again=libs["other"])
    D, A = 29, 8
    out = []
    for N in (50_000, 3_400_000):
        reps = 100 if N < 1_000_000 else 4
        for hidden in (128, 256):
            rng = np.random.default_rng(0)
            params, batch = make_update_batch(rng, N, D, A, hidden, 0.3, 1.0, 35)
            v = rng.standard_normal(params.shape).astype(np.float32)
            w = np.exp(rng.uniform(np.log(1 / 64), np.log(64), N)).astype(np.float32)
            for path in ((1, 0) if hidden == 128 else (0,)):
                fns, keepalive = {}, []
                for name, handle in libs.items():
                    with library(handle):
                        handle.cmbpo_set_pi_matrix_path(path)
                        made = {}
                        for tag, keep, weights in (("keep", True, None), ("nokeep", False, None), ("weighted", True, w)):
                            ops = made[tag] = PolicyOps(D, A, hidden, device="cuda:0")
                            ops.keep_activations = keep
                            ops.set_params(params)
                            ops.bind(*[batch[k] for k in R.KEYS], weights=weights)
                            ops.dv = torch.from_numpy(v).cuda()
                            ops.out = torch.zeros_like(ops.dv)
                            ops.cfg = ops.ppo_cfg(clip_ratio=R.CLIP, clipped_adv=True, objective_penalized=True)
                            R.set_penalty(ops, 1.0)
                            ops.loss_grad(0)       # (keep: the activations are saved from here on)
                        keepalive.append((name, made))
                        k, nk, wt = made["keep"], made["nokeep"], made["weighted"]
                        for kern, fn in (("loss_grad", lambda k=k: k.grad_dev(0, k.out, k.sums)),
                                         ("fvp_saved", lambda k=k: k.fvp_raw(k.dv)),
                                         ("fvp_recomputed", lambda nk=nk: nk.fvp_raw(nk.dv)),
                                         ("evals", lambda k=k: k.eval_dev(k.sums)),
                                         ("ppo_grad", lambda k=k: k.ppo_grad_dev(k.cfg, k.out, k.ppo_sums)),
                                         ("ppo_grad_weighted", lambda wt=wt: wt.ppo_grad_dev(wt.cfg, wt.out, wt.ppo_sums))):
                            fns.setdefault(kern, {})[name] = timed(libs, name, fn, reps)
                        k.fvp_raw(k.dv)
                        nk.fvp_raw(nk.dv)
                        assert (R._uses(k), R._uses(nk)) == (1, 0), "which product read saved activations"
                for kern, pair in fns.items():
                    us = alternate(pair, rounds)
                    med = {n: statistics.median(x) for n, x in us.items()}
                    row = dict(N=N, hidden=hidden, path="splitf16" if path else "fp32mfma", kernel=kern, reps=reps, us_per_call=us,
                               median_us=med, ratio_here_over_other=med["here"] / med["other"], spread_here=spread(us["here"]),
                               spread_other=spread(us["other"]), second_set_over_first_same_code=med["other_again"] / med["other"])
                    row["within_other_spread"] = bool(row["ratio_here_over_other"] - 1.0 <= row["spread_other"])
                    out.append(row)
                    print("N=%-8d h%d %-9s %-18s here/other %.4f  (other %.1f us, spread other %.4f, here %.4f; other again/other %.4f) -> %s"
                          % (N, hidden, row["path"], kern, row["ratio_here_over_other"], med["other"], row["spread_other"], row["spread_here"],
                             row["second_set_over_first_same_code"], "within" if row["within_other_spread"] else "OUTSIDE"), flush=True)
                for name, made in keepalive:
                    with library(libs[name]):
                        for ops in made.values():
                            ops.__del__()
                        libs[name].cmbpo_set_pi_matrix_path(1)
    return dict(rounds=rounds, rows=out, outside=sum(not r["within_other_spread"] for r in out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--other-lib", required=True)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--rounds", type=int, default=10)
    args = ap.parse_args()
    libs = {"here": _lib.lib(), "other": other_library(args.other_lib)}
    res = dict(command="python tools/probe_pi_parity.py <out.json> --other-lib <the parent commit's libcmbpo_hip.so>" +
               (" --time --rounds %d" % args.rounds if args.time else ""), device=torch.cuda.get_device_name(0))
    res.update(timing(libs, args.rounds) if args.time else parity(libs))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    return 1 if res.get("mismatches") else 0


if __name__ == "__main__":
    sys.exit(main())
